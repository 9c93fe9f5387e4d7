// The inflater of csrc/tiff_inflate_dev.h as a plain host program (tests/test_tiff_inflate_host.py builds it with the address and
// undefined-behaviour sanitizers).  Usage: inflate_host_check LIST -- LIST holds one case per line, "stream_file expected_size
// output_file"; per case one line "status bytes_written_to_output_file" goes to stdout.  The stream and the output live in heap
// blocks of exactly their sizes, so a read past the stream or a write past the expected size is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "tiff_inflate_dev.h"

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
        unsigned char* in = static_cast<unsigned char*>(std::malloc(bytes.size() ? bytes.size() : 1));
        unsigned char* out = static_cast<unsigned char*>(std::calloc(want ? want : 1, 1));
        if (!in || !out) return 2;
        for (size_t i = 0; i < bytes.size(); ++i) in[i] = (unsigned char)bytes[i];
        const int st = mi_inflate::inflate_host(in, (uint32_t)bytes.size(), out, (uint32_t)want);
        size_t wrote = 0;
        if (st == mi_inflate::kInfOk) {
            std::ofstream o(out_path, std::ios::binary);
            o.write(reinterpret_cast<const char*>(out), (std::streamsize)want);
            wrote = (size_t)want;
        }
        std::printf("%d %zu %s\n", st, wrote, mi_inflate::status_name(st));
        std::free(in);
        std::free(out);
    }
    return 0;
}
