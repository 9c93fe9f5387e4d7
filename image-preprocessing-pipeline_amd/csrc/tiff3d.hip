// Multi-page TIFF block files of the TeraFly tree (include/mi_pyramid.h): host code, no GPU.
//
// What Tiff3DMngr.cpp's initTiff3DFile / appendSlice2Tiff3DFile write through libtiff (one page per slice, LZW or none,
// RowsPerStrip rows per strip, PageNumber = (slice, block depth)), written here without libtiff: every strip is encoded on its own,
// so a thread pool encodes the strips of all pages of all blocks at once, then each file gets its pages appended in one write and
// the previous page's next-IFD pointer patched.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "mi_internal.h"
#include "mi_pyramid.h"
#include "tiffio_internal.h"

namespace {

using mi::pread_all;
using mi::put16;
using mi::put32;
using mi::put64;

// ------------------------------------------------------------------------------------------------------------------ LZW (TIFF)
// The encoder of libtiff's tif_lzw.c restated: 9..12-bit codes, MSB first, Clear (256) first, EOI (257) last, code width grown when
// the next free code passes the current maximum, table reset (Clear) when it reaches 4094.  Decoders apply TIFF's "early change",
// which this schedule matches.
constexpr int kClear = 256, kEoi = 257, kFirst = 258, kMaxCode = 4095, kHashBits = 13, kHashSize = 1 << kHashBits;

struct LzwTable {
    uint32_t key[kHashSize];     // (prefix << 8 | byte) + 1; valid when stamp matches
    uint16_t code[kHashSize];
    uint32_t stamp[kHashSize];
    uint32_t gen = 0;
    LzwTable() { std::memset(stamp, 0, sizeof stamp); }
    void reset() {
        if (++gen == 0) {            // wrapped: clear for real
            std::memset(stamp, 0, sizeof stamp);
            gen = 1;
        }
    }
};

struct BitWriter {
    uint8_t* out;
    int64_t cap, n = 0;
    uint64_t acc = 0;
    int bits = 0;
    bool overflow = false;
    void put(uint32_t code, int width) {
        acc = (acc << width) | code;
        bits += width;
        while (bits >= 8) {
            bits -= 8;
            if (n < cap) out[n] = (uint8_t)(acc >> bits); else overflow = true;
            ++n;
        }
    }
    void flush() {
        if (bits > 0) {
            if (n < cap) out[n] = (uint8_t)(acc << (8 - bits)); else overflow = true;
            ++n;
            bits = 0;
        }
    }
};

int64_t lzw_encode(LzwTable& T, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap) {
    BitWriter bw{dst, cap};
    T.reset();
    int nbits = 9, maxcode = 511, free_ent = kFirst;
    bw.put(kClear, nbits);
    if (n == 0) {
        bw.put(kEoi, nbits);
        bw.flush();
        return bw.overflow ? -1 : bw.n;
    }
    int ent = src[0];
    for (int64_t i = 1; i < n; ++i) {
        const int c = src[i];
        const uint32_t k = ((uint32_t)ent << 8 | (uint32_t)c) + 1u;
        uint32_t h = (k * 2654435761u) >> (32 - kHashBits);
        bool found = false;
        while (T.stamp[h] == T.gen) {
            if (T.key[h] == k) { ent = T.code[h]; found = true; break; }
            h = (h + 1) & (kHashSize - 1);
        }
        if (found) continue;
        bw.put((uint32_t)ent, nbits);
        ent = c;
        T.stamp[h] = T.gen;
        T.key[h] = k;
        T.code[h] = (uint16_t)free_ent++;
        if (free_ent == kMaxCode - 1) {
            T.reset();
            free_ent = kFirst;
            bw.put(kClear, nbits);
            nbits = 9;
            maxcode = 511;
        } else if (free_ent > maxcode) {
            ++nbits;
            maxcode = (1 << nbits) - 1;
        }
    }
    bw.put((uint32_t)ent, nbits);
    ++free_ent;                        // the decoder adds an entry after the last code and may widen before reading EOI
    if (free_ent == kMaxCode - 1) {
        bw.put(kClear, nbits);
        nbits = 9;
    } else if (free_ent > maxcode) {
        ++nbits;
    }
    bw.put(kEoi, nbits);
    bw.flush();
    return bw.overflow ? -1 : bw.n;
}

template <class F>
void parallel_for(int64_t n, int threads, F f) {
    const int nt = (int)std::min<int64_t>(threads, n);
    if (nt <= 1) {
        for (int64_t i = 0; i < n; ++i) f(i, 0);
        return;
    }
    std::atomic<int64_t> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            for (int64_t i; (i = next.fetch_add(1)) < n;) f(i, t);
        });
    for (auto& th : pool) th.join();
}

// ------------------------------------------------------------------------------------------------------------------ TIFF pages
using Block = mi::Tiff3dBlock;
using mi::StripRef;

// offset of the next-IFD field of the last IFD of a file this writer made (walks the chain)
int last_ifd_link(int fd, bool big, const std::string& path, int expect_pages, uint64_t* link) {
    uint64_t off = 0;
    uint64_t pos = big ? 8 : 4;   // the header's first-IFD field
    int pages = 0;
    for (;;) {
        if (big) {
            if (!pread_all(fd, &off, 8, pos)) return mi::fail(MI_ERR_INVALID, "%s: truncated TIFF", path.c_str());
        } else {
            uint32_t o32;
            if (!pread_all(fd, &o32, 4, pos)) return mi::fail(MI_ERR_INVALID, "%s: truncated TIFF", path.c_str());
            off = o32;
        }
        if (off == 0) break;
        ++pages;
        if (big) {
            uint64_t cnt;
            if (!pread_all(fd, &cnt, 8, off)) return mi::fail(MI_ERR_INVALID, "%s: truncated IFD", path.c_str());
            pos = off + 8 + cnt * 20;
        } else {
            uint16_t cnt;
            if (!pread_all(fd, &cnt, 2, off)) return mi::fail(MI_ERR_INVALID, "%s: truncated IFD", path.c_str());
            pos = off + 2 + (uint64_t)cnt * 12;
        }
    }
    if (pages != expect_pages)
        return mi::fail(MI_ERR_INVALID, "%s: holds %d pages, the append expects %d", path.c_str(), pages, expect_pages);
    *link = pos;
    return MI_OK;
}

// Appends the IFD of one page to `buf` (which will start at file offset `base`); returns the buffer index of its next-IFD field.
size_t add_ifd(std::vector<uint8_t>& buf, uint64_t base, bool big, int w, int h, int bytes, int comp, int rps,
               const std::vector<uint64_t>& offs, const std::vector<uint64_t>& counts, int page, int total) {
    const int nstrips = (int)offs.size();
    // out-of-line arrays first (word aligned)
    if (buf.size() % 2) buf.push_back(0);
    uint64_t offs_at = 0, counts_at = 0;
    const int inline_cap = 1;   // a single LONG / LONG8 fits in the entry
    if (nstrips > inline_cap) {
        offs_at = base + buf.size();
        for (uint64_t o : offs) big ? put64(buf, o) : put32(buf, (uint32_t)o);
        counts_at = base + buf.size();
        for (uint64_t c : counts) big ? put64(buf, c) : put32(buf, (uint32_t)c);
    }
    struct E { uint16_t tag, type; uint64_t count, value; };
    const uint16_t SHORT = 3, LONG = 4, LONG8 = 16;
    const uint16_t OFFT = big ? LONG8 : LONG;
    std::vector<E> es = {
        {254, LONG, 1, 2},                                  // NewSubfileType: FILETYPE_PAGE
        {256, LONG, 1, (uint64_t)w},
        {257, LONG, 1, (uint64_t)h},
        {258, SHORT, 1, (uint64_t)(8 * bytes)},
        {259, SHORT, 1, (uint64_t)(comp ? 5 : 1)},
        {262, SHORT, 1, 1},                                 // MinIsBlack
        {273, OFFT, (uint64_t)nstrips, nstrips > inline_cap ? offs_at : offs[0]},
        {274, SHORT, 1, 1},                                 // Orientation: top-left
        {277, SHORT, 1, 1},
        {278, LONG, 1, (uint64_t)rps},
        {279, OFFT, (uint64_t)nstrips, nstrips > inline_cap ? counts_at : counts[0]},
        {284, SHORT, 1, 1},                                 // PlanarConfig: contiguous
        {297, SHORT, 2, (uint64_t)(page & 0xffff) | ((uint64_t)(total & 0xffff) << 16)},
    };
    if (big) put64(buf, es.size()); else put16(buf, (uint16_t)es.size());
    for (const E& e : es) {
        put16(buf, e.tag);
        put16(buf, e.type);
        if (big) {
            put64(buf, e.count);
            put64(buf, e.value);     // SHORT / LONG values sit left-justified: little-endian puts them first
        } else {
            put32(buf, (uint32_t)e.count);
            put32(buf, (uint32_t)e.value);
        }
    }
    const size_t link = buf.size();
    if (big) put64(buf, 0); else put32(buf, 0);
    return link;
}

int write_block(const Block& B, const StripRef* strips, int bytes, int comp, int rps, int force_big) {
    const int nstrip_page = (B.h + rps - 1) / rps;
    int fd;
    bool big;
    uint64_t end, link;
    if (B.page0 == 0) {
        fd = open(B.path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) return mi::fail(MI_ERR_INVALID, "%s: cannot create (%s)", B.path.c_str(), strerror(errno));
        const uint64_t expected = (uint64_t)B.w * B.h * (uint64_t)std::max(B.total, B.pages) * bytes;
        big = force_big || expected > (4ull << 30);
        std::vector<uint8_t> hdr = {'I', 'I'};
        if (big) { put16(hdr, 43); put16(hdr, 8); put16(hdr, 0); put64(hdr, 0); }
        else { put16(hdr, 42); put32(hdr, 0); }
        if (pwrite(fd, hdr.data(), hdr.size(), 0) != (ssize_t)hdr.size()) {
            close(fd);
            return mi::fail(MI_ERR_INVALID, "%s: write failed (%s)", B.path.c_str(), strerror(errno));
        }
        end = hdr.size();
        link = big ? 8 : 4;
    } else {
        fd = open(B.path.c_str(), O_RDWR);
        if (fd < 0) return mi::fail(MI_ERR_INVALID, "%s: cannot open for appending (%s)", B.path.c_str(), strerror(errno));
        uint8_t hdr[4];
        if (!pread_all(fd, hdr, 4, 0) || hdr[0] != 'I' || hdr[1] != 'I' || (hdr[2] != 42 && hdr[2] != 43)) {
            close(fd);
            return mi::fail(MI_ERR_INVALID, "%s: not a little-endian TIFF this writer made", B.path.c_str());
        }
        big = hdr[2] == 43;
        const int rc = last_ifd_link(fd, big, B.path, B.page0, &link);
        if (rc != MI_OK) { close(fd); return rc; }
        struct stat st;
        fstat(fd, &st);
        end = (uint64_t)st.st_size;
    }
    std::vector<uint8_t> buf;
    std::vector<uint64_t> offs(nstrip_page), counts(nstrip_page);
    uint64_t prev_link_abs = link;
    std::vector<std::pair<uint64_t, uint64_t>> patches;   // (absolute field offset, value) outside `buf`
    std::vector<std::pair<size_t, uint64_t>> inner;       // (buffer field index, value)
    bool prev_in_buf = false;
    size_t prev_link_idx = 0;
    for (int p = 0; p < B.pages; ++p) {
        for (int s = 0; s < nstrip_page; ++s) {
            const StripRef& S = strips[B.strip0 + (int64_t)p * nstrip_page + s];
            if (buf.size() % 2) buf.push_back(0);
            offs[s] = end + buf.size();
            counts[s] = S.n;
            buf.insert(buf.end(), S.p, S.p + S.n);
        }
        if (buf.size() % 2) buf.push_back(0);
        const size_t at = buf.size();
        const size_t l = add_ifd(buf, end, big, B.w, B.h, bytes, comp, rps, offs, counts, B.page0 + p, B.total);
        // the IFD itself starts after its out-of-line arrays: find it from the entry count position
        const int ns = nstrip_page;
        const size_t arrays = ns > 1 ? (size_t)ns * (big ? 16 : 8) : 0;
        const uint64_t ifd_abs = end + at + arrays;
        if (prev_in_buf) inner.push_back({prev_link_idx, ifd_abs});
        else patches.push_back({prev_link_abs, ifd_abs});
        prev_in_buf = true;
        prev_link_idx = l;
    }
    if (!big && end + buf.size() > 0xffffffffull) {
        close(fd);
        return mi::fail(MI_ERR_INVALID, "%s: a classic TIFF cannot pass 4 GiB (%llu bytes); use BigTIFF (--libtiff_bigtiff)",
                        B.path.c_str(), (unsigned long long)(end + buf.size()));
    }
    for (auto& [idx, v] : inner) {
        if (big) std::memcpy(&buf[idx], &v, 8);
        else { const uint32_t v32 = (uint32_t)v; std::memcpy(&buf[idx], &v32, 4); }
    }
    bool ok = true;
    size_t done = 0;
    while (ok && done < buf.size()) {
        const ssize_t k = pwrite(fd, buf.data() + done, buf.size() - done, (off_t)(end + done));
        if (k <= 0) ok = false; else done += (size_t)k;
    }
    for (auto& [pos, v] : patches) {
        if (!ok) break;
        if (big) ok = pwrite(fd, &v, 8, (off_t)pos) == 8;
        else { const uint32_t v32 = (uint32_t)v; ok = pwrite(fd, &v32, 4, (off_t)pos) == 4; }
    }
    close(fd);
    if (!ok) return mi::fail(MI_ERR_INVALID, "%s: write failed (%s)", B.path.c_str(), strerror(errno));
    return MI_OK;
}

}  // namespace

namespace mi {

int tiff3d_parse_blocks(const char* who, int n, const char* const* paths, const void* const* first, const int64_t* strides, const int* dims,
                        const int* page0, const int* page_total, int bytes, int rows_per_strip, std::vector<Tiff3dBlock>& blocks, int64_t* n_strips) {
    blocks.assign((size_t)n, Block());
    int64_t nstrips = 0;
    for (int b = 0; b < n; ++b) {
        Block& B = blocks[b];
        MI_REQUIRE(paths[b] && (!first || first[b]), "%s: block %d has no path or samples", who, b);
        B.path = paths[b];
        B.first = first ? static_cast<const uint8_t*>(first[b]) : nullptr;
        B.sp = strides[2 * b];
        B.sr = strides[2 * b + 1];
        B.w = dims[3 * b];
        B.h = dims[3 * b + 1];
        B.pages = dims[3 * b + 2];
        B.page0 = page0[b];
        B.total = page_total[b];
        MI_REQUIRE(B.w > 0 && B.h > 0 && B.pages >= 0 && B.page0 >= 0, "%s: block %d of %d x %d x %d from page %d", who, b,
                   B.w, B.h, B.pages, B.page0);
        MI_REQUIRE((int64_t)rows_per_strip * B.w * bytes <= 0xffffffffll, "%s: a strip of block %d passes 4 GiB", who, b);
        B.strip0 = nstrips;
        nstrips += (int64_t)B.pages * ((B.h + rows_per_strip - 1) / rows_per_strip);
    }
    *n_strips = nstrips;
    return MI_OK;
}

int tiff3d_write_files(const std::vector<Tiff3dBlock>& blocks, const StripRef* strips, int bytes, int compression, int rows_per_strip, int bigtiff,
                       int threads) {
    const int n = (int)blocks.size();
    std::vector<int> rc(n, MI_OK);
    std::vector<std::string> msg(n);
    parallel_for(n, threads, [&](int64_t b, int) {
        rc[b] = write_block(blocks[b], strips, bytes, compression, rows_per_strip, bigtiff);
        if (rc[b] != MI_OK) msg[b] = mi::last_error_ref();
    });
    for (int b = 0; b < n; ++b)
        if (rc[b] != MI_OK) return mi::fail(rc[b], "%s", msg[b].c_str());
    return MI_OK;
}

}  // namespace mi

extern "C" int mi_tiff_lzw_encode(const void* src, int64_t n, void* dst, int64_t cap, int64_t* written) {
    MI_REQUIRE((src || n == 0) && dst && written && n >= 0, "mi_tiff_lzw_encode: bad arguments");
    std::unique_ptr<LzwTable> T(new LzwTable());
    const int64_t k = lzw_encode(*T, static_cast<const uint8_t*>(src), n, static_cast<uint8_t*>(dst), cap);
    if (k < 0) return mi::fail(MI_ERR_NOMEM, "mi_tiff_lzw_encode: %lld bytes of output space are too few", (long long)cap);
    *written = k;
    return MI_OK;
}

extern "C" int mi_tiff3d_write_blocks(int n, const char* const* paths, const void* const* first, const int64_t* strides, const int* dims,
                                      const int* page0, const int* page_total, int bytes, int compression, int rows_per_strip,
                                      int bigtiff, int n_threads) {
    MI_REQUIRE(n >= 0 && (n == 0 || (paths && first && strides && dims && page0 && page_total)), "mi_tiff3d_write_blocks: null pointer");
    MI_REQUIRE(bytes == 1 || bytes == 2, "mi_tiff3d_write_blocks: %d bytes per sample (1 or 2)", bytes);
    MI_REQUIRE(compression == 0 || compression == 1, "mi_tiff3d_write_blocks: compression %d (0 none, 1 LZW)", compression);
    MI_REQUIRE(rows_per_strip >= 1, "mi_tiff3d_write_blocks: %d rows per strip", rows_per_strip);
    std::vector<Block> blocks;
    int64_t nstrips = 0;
    MI_TRY(mi::tiff3d_parse_blocks("mi_tiff3d_write_blocks", n, paths, first, strides, dims, page0, page_total, bytes, rows_per_strip, blocks, &nstrips));
    const int threads = mi::tree_pool_threads(n_threads);
    // 1) every strip of every page of every block, encoded in parallel
    struct Strip {
        std::vector<uint8_t> data;
    };
    std::vector<Strip> strips(nstrips);
    std::vector<std::unique_ptr<LzwTable>> tables(threads);
    std::vector<std::vector<uint8_t>> rowbuf(threads);
    std::atomic<int> fail_nomem{0};
    std::vector<int> owner(nstrips);
    for (int b = 0; b < n; ++b)
        for (int64_t s = blocks[b].strip0; s < (b + 1 < n ? blocks[b + 1].strip0 : nstrips); ++s) owner[s] = b;
    parallel_for(nstrips, threads, [&](int64_t s, int t) {
        const Block& B = blocks[owner[s]];
        const int per_page = (B.h + rows_per_strip - 1) / rows_per_strip;
        const int64_t k = s - B.strip0;
        const int p = (int)(k / per_page), r0 = (int)(k % per_page) * rows_per_strip;
        const int nr = std::min(rows_per_strip, B.h - r0);
        const int64_t row_bytes = (int64_t)B.w * bytes;
        std::vector<uint8_t>& raw = rowbuf[t];
        raw.resize((size_t)(row_bytes * nr));
        for (int r = 0; r < nr; ++r)
            std::memcpy(raw.data() + r * row_bytes, B.first + ((int64_t)p * B.sp + (int64_t)(r0 + r) * B.sr) * bytes, (size_t)row_bytes);
        Strip& S = strips[s];
        if (!compression) {
            S.data = raw;
            return;
        }
        if (!tables[t]) tables[t].reset(new LzwTable());
        S.data.resize((size_t)(raw.size() * 3 / 2 + 16));
        const int64_t m = lzw_encode(*tables[t], raw.data(), (int64_t)raw.size(), S.data.data(), (int64_t)S.data.size());
        if (m < 0) { fail_nomem = 1; return; }
        S.data.resize((size_t)m);
    });
    if (fail_nomem) return mi::fail(MI_ERR_NOMEM, "mi_tiff3d_write_blocks: LZW output larger than its bound");
    // 2) each file gets its pages appended
    std::vector<StripRef> refs(nstrips);
    for (int64_t k = 0; k < nstrips; ++k) refs[k] = {strips[k].data.data(), strips[k].data.size()};
    return mi::tiff3d_write_files(blocks, refs.data(), bytes, compression, rows_per_strip, bigtiff, threads);
}

extern "C" int mi_tiff3d_write_blocks_encoded(int n, const char* const* paths, const int* dims, const int* page0, const int* page_total, int bytes,
                                              int rows_per_strip, int bigtiff, const void* const* strips, const int64_t* lengths, int n_threads) {
    MI_REQUIRE(n >= 0 && (n == 0 || (paths && dims && page0 && page_total && strips && lengths)), "mi_tiff3d_write_blocks_encoded: null pointer");
    MI_REQUIRE(bytes == 1 || bytes == 2, "mi_tiff3d_write_blocks_encoded: %d bytes per sample (1 or 2)", bytes);
    MI_REQUIRE(rows_per_strip >= 1, "mi_tiff3d_write_blocks_encoded: %d rows per strip", rows_per_strip);
    std::vector<int64_t> strides(2 * (size_t)n, 0);
    std::vector<Block> blocks;
    int64_t nstrips = 0;
    MI_TRY(mi::tiff3d_parse_blocks("mi_tiff3d_write_blocks_encoded", n, paths, nullptr, strides.data(), dims, page0, page_total, bytes, rows_per_strip,
                                   blocks, &nstrips));
    std::vector<StripRef> refs(nstrips);
    for (int64_t k = 0; k < nstrips; ++k) {
        MI_REQUIRE(strips[k] && lengths[k] > 0, "mi_tiff3d_write_blocks_encoded: strip %lld has no bytes", (long long)k);
        refs[k] = {static_cast<const uint8_t*>(strips[k]), (size_t)lengths[k]};
    }
    return mi::tiff3d_write_files(blocks, refs.data(), bytes, 1, rows_per_strip, bigtiff, mi::tree_pool_threads(n_threads));
}
