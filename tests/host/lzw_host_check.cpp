// The LZW decoder of csrc/tiff_lzw_dev.h as a plain host program (tests/test_tiff_lzw_host.py builds it with the address and
// undefined-behaviour sanitizers).  Usage: lzw_host_check LIST -- LIST holds one case per line, "strip_file expected_size
// output_file"; per case one line "status bytes_written_to_output_file name" goes to stdout.  The strip, the output and the two
// halves of the table live in heap blocks of exactly their sizes (the table: table_entries(expected_size) entries, what a launch
// sizes it to), so a read past the strip, a write past the rows or an entry past the table is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "tiff_lzw_dev.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s LIST\n", argv[0]);
        return 2;
    }
    std::ifstream list(argv[1]);
    if (!list) {
        std::fprintf(stderr, "%s: cannot be read\n", argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(list, line)) {
        std::istringstream ls(line);
        std::string in_path, out_path;
        unsigned long long want = 0;
        if (!(ls >> in_path >> want >> out_path)) continue;
        std::ifstream f(in_path, std::ios::binary);
        if (!f) {
            std::fprintf(stderr, "%s: cannot be read\n", in_path.c_str());
            return 2;
        }
        const std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const uint32_t entries = mi_lzw::table_entries((uint32_t)want);
        unsigned char* in = static_cast<unsigned char*>(std::malloc(bytes.size() ? bytes.size() : 1));
        unsigned char* out = static_cast<unsigned char*>(std::calloc(want ? want : 1, 1));
        uint32_t* off = static_cast<uint32_t*>(std::malloc(entries ? entries * sizeof(uint32_t) : 1));
        uint16_t* len = static_cast<uint16_t*>(std::malloc(entries ? entries * sizeof(uint16_t) : 1));
        if (!in || !out || !off || !len) return 2;
        for (size_t i = 0; i < bytes.size(); ++i) in[i] = (unsigned char)bytes[i];
        const int st = mi_lzw::lzw_host(in, (uint32_t)bytes.size(), out, (uint32_t)want, off, len);
        size_t wrote = 0;
        if (st == mi_lzw::kLzwOk) {
            std::ofstream o(out_path, std::ios::binary);
            o.write(reinterpret_cast<const char*>(out), (std::streamsize)want);
            wrote = (size_t)want;
        }
        std::printf("%d %zu %s\n", st, wrote, mi_lzw::status_name(st));
        std::free(in);
        std::free(out);
        std::free(off);
        std::free(len);
    }
    return 0;
}
