// The LZW encoder of csrc/tiff_lzw_enc_dev.h as a plain host program (tests/test_tiff_lzw_enc_host.py builds it with the address and
// undefined-behaviour sanitizers).  Usage: lzw_enc_host_check LIST -- LIST holds one case per line, "raw_file slot_bytes
// output_file"; per case one line "status stream_length bytes_written_to_output_file" goes to stdout.  The strip, the table
// (table_slots(strip bytes) words, what a launch sizes it to) and the slot live in heap blocks of exactly their sizes, so a read
// past the strip, a probe past the table or a store past the slot is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "tiff_lzw_enc_dev.h"

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
        unsigned long long cap = 0;
        if (!(ls >> in_path >> cap >> out_path)) continue;
        std::ifstream f(in_path, std::ios::binary);
        if (!f) {
            std::fprintf(stderr, "%s: cannot be read\n", in_path.c_str());
            return 2;
        }
        const std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const uint32_t n = (uint32_t)bytes.size();
        const uint32_t slots = mi_lzw_enc::table_slots(n);
        unsigned char* in = static_cast<unsigned char*>(std::malloc(n ? n : 1));
        uint32_t* table = static_cast<uint32_t*>(std::malloc(slots * sizeof(uint32_t)));
        unsigned char* slot = static_cast<unsigned char*>(std::malloc(cap ? cap : 1));
        if (!in || !table || !slot) return 2;
        for (size_t i = 0; i < bytes.size(); ++i) in[i] = (unsigned char)bytes[i];
        uint64_t len = 0;
        const int st = mi_lzw_enc::lzw_encode_host(in, n, table, slot, cap, &len);
        const uint64_t stored = len < cap ? len : cap;
        std::ofstream o(out_path, std::ios::binary);
        o.write(reinterpret_cast<const char*>(slot), (std::streamsize)stored);
        std::printf("%d %llu %llu\n", st, (unsigned long long)len, (unsigned long long)stored);
        std::free(in);
        std::free(table);
        std::free(slot);
    }
    return 0;
}
