// The readers of the TeraFly tree's block files (include/mi_tiff3d.h): the mirror of the writer in tiff3d.hip.  What Tiff3DMngr.cpp's
// readTiff3DFile2Buffer does through libtiff page by page, done without libtiff for all blocks of a box at once: the directories are
// parsed here, only the strips a piece's rows touch are read, and every strip is decoded on its own -- on a host thread pool
// (mi_tiff3d_read_box) or a strip per wave on the device (mi_tiff3d_read_box_device):
//   k_strip_lzw    one LZW strip per wave (a work-group is one wave).  The decoder is the text of tiff_lzw_dev.h: every lane runs
//                  the serial code walk with the same values (the code comes through readfirstlane, so the bit buffer, the positions
//                  and the table index live in scalar registers), and the lanes part in the copy of a string, a byte per lane.
//                  The table of (offset, length) is in LDS, sized per launch to the longest strip of the launch.  Strips of at
//                  most kLdsRows bytes keep their rows in LDS and write them out once, as words; longer strips copy in global memory.
//   k_tree_place   copies rows [y0, y1) and columns [x0, x1) of each decoded (or uncompressed) page to its place in the box, a wave
//                  per row, 64-bit offsets.
//
// What orders the accesses of k_strip_lzw (the three patterns of tiff_inflate.hip):
//   - a lane reads bytes another lane wrote (staged input words; the source of a copy, in LDS or -- long strips -- in global
//     memory): a __syncthreads() stands between every such write and read.  A work-group is one wave, so the barrier costs no
//     waiting; it is the fence that counts (LDS, and a work-group release / acquire of global memory).  copy() begins with it; the
//     bytes it reads all lie before `pos`, so the lanes of one copy never read what that copy writes.
//   - the table: set_entry / get_entry are run by all 64 lanes with the same index and value; every lane reads what it wrote
//     itself, in program order.  This rests on the work-group being ONE wave (__launch_bounds__(64), launched with 64 threads).
//   - a literal is one byte written by lane 0; nothing reads it before the next copy's barrier or the barrier before the rows go out.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "mi_internal.h"
#include "mi_tiff3d.h"
#include "tiff_lzw_dev.h"
#include "tiffio_internal.h"

namespace {

using mi::fail;
using namespace mi_lzw;

// ------------------------------------------------------------------------------------------------------------------ kernels
constexpr uint32_t kStageWords = 64;     // compressed bytes in LDS: 256 at a time (+ one word: a strip begins at any byte)
constexpr uint32_t kLdsRows = 16384;     // strips of at most this many raw bytes keep their rows in LDS

struct LzwJob {
    unsigned long long in_off, out_off;   // into the uploaded bytes (any byte) / the decoded rows
    uint32_t in_n, out_n;
};

// the context of tiff_lzw_dev.h for a wave.  kLds: the rows wait in LDS (rows) and go out at the end; else they are written to
// global memory (out) as they come.  kWide: offsets of 32 bits (strips of more than 64 KB), else offset and length share a word.
template <bool kLds, bool kWide>
struct WaveCtx {
    uint32_t* stage;                        // LDS: aligned words [stage_base, stage_base + kStageWords] of the upload, masked to the strip
    uint32_t* tab;                          // LDS: entries
    uint16_t* tlen;                         // LDS: lengths (kWide)
    unsigned char* rows;                    // LDS (kLds) or global: the strip's output
    const uint32_t* __restrict__ in_words;  // the upload from the aligned word that holds the strip's first byte
    uint32_t shift, in_n, lane, stage_base;

    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

    // aligned words [first, first + kStageWords]; no word without a byte of the strip is read, bytes outside the strip become 0
    __device__ __forceinline__ void fill_stage(uint32_t first) {
        __syncthreads();
        stage_base = first;
        for (uint32_t k = lane; k <= kStageWords; k += 64) {
            const unsigned long long b0 = ((unsigned long long)first + k) * 4u;   // of the word's first byte, from the aligned start
            const unsigned long long lo = shift, hi = (unsigned long long)shift + in_n;   // the strip's bytes there
            uint32_t v = 0;
            if (b0 + 4 > lo && b0 < hi) {
                v = in_words[(unsigned long long)first + k];
                if (b0 < lo) v &= 0xffffffffu << (8 * (uint32_t)(lo - b0));
                if (b0 + 4 > hi) v &= 0xffffffffu >> (8 * (uint32_t)(b0 + 4 - hi));
            }
            stage[k] = v;
        }
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t word(uint32_t i) {
        if (i - stage_base >= kStageWords) fill_stage(i);
        const uint32_t k = i - stage_base;
        const unsigned long long two = (unsigned long long)stage[k + 1] << 32 | stage[k];
        return uni(__builtin_bswap32((uint32_t)(two >> (8 * shift))));
    }
    __device__ __forceinline__ void set_entry(uint32_t i, uint32_t off, uint32_t len) {
        if (kWide) {
            tab[i] = off;
            tlen[i] = (uint16_t)len;
        } else {
            tab[i] = off | len << 16;
        }
    }
    __device__ __forceinline__ void get_entry(uint32_t i, uint32_t& off, uint32_t& len) const {
        if (kWide) {
            off = uni(tab[i]);
            len = uni((uint32_t)tlen[i]);
        } else {
            const uint32_t e = uni(tab[i]);
            off = e & 0xffffu;
            len = e >> 16;
        }
    }
    __device__ __forceinline__ void literal(uint32_t pos, uint32_t b) {
        if (lane == 0) rows[pos] = (unsigned char)b;
    }
    // len <= pos - off + 1: byte k comes from off + k, the last byte of a KwKwK string from off
    __device__ __forceinline__ void copy(uint32_t pos, uint32_t off, uint32_t len) {
        const uint32_t dist = pos - off;
        __syncthreads();
        for (uint32_t k = lane; k < len; k += 64) rows[pos + k] = rows[off + (k >= dist ? k - dist : k)];
    }
};

template <bool kLds, bool kWide>
__global__ __launch_bounds__(64) void k_strip_lzw(const unsigned char* __restrict__ in, unsigned char* out, const LzwJob* __restrict__ jobs,
                                                  int32_t* __restrict__ status, uint32_t entries) {
    extern __shared__ uint32_t lds[];   // [stage: kStageWords + 1][entries][kWide: entries / 2 rounded up][kLds: rows]
    const LzwJob j = jobs[blockIdx.x];
    const uint32_t in_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)j.in_n), out_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)j.out_n);
    uint32_t* stage = lds;
    uint32_t* tab = stage + (kStageWords + 1);
    uint16_t* tlen = reinterpret_cast<uint16_t*>(tab + entries);
    unsigned char* lrows = reinterpret_cast<unsigned char*>(tab + entries + (kWide ? (entries + 1) / 2 : 0));
    unsigned char* grows = out + j.out_off;
    WaveCtx<kLds, kWide> ctx{stage, tab, tlen, kLds ? lrows : grows, reinterpret_cast<const uint32_t*>(in + (j.in_off & ~3ull)),
                             (uint32_t)(j.in_off & 3ull), in_n, threadIdx.x, 0};
    ctx.fill_stage(0);
    const int st = lzw_decode(ctx, in_n, out_n);
    if (kLds) {
        // the rows go out as whole words where the global address allows it
        __syncthreads();
        const uint32_t head = (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(grows) & 3u)) & 3u);
        const uint32_t h = head < out_n ? head : out_n, nw = (out_n - h) / 4;
        if (threadIdx.x < h) grows[threadIdx.x] = lrows[threadIdx.x];
        for (uint32_t w = threadIdx.x; w < nw; w += 64) {
            const unsigned char* p = lrows + h + 4 * w;
            *reinterpret_cast<uint32_t*>(grows + h + 4 * w) = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
        }
        const uint32_t tail = h + 4 * nw;
        if (tail + threadIdx.x < out_n && threadIdx.x < 4) grows[tail + threadIdx.x] = lrows[tail + threadIdx.x];
    }
    if (threadIdx.x == 0) status[blockIdx.x] = st;
}

struct PlaceJob {
    unsigned long long src_off, dst_off;   // the first row's first sample of the file's page, in bytes; its place in the box, in samples
    uint32_t src_pitch, x0, ncols, nrows;  // bytes between rows of the source; the first column, the columns and the rows to copy
};

template <class T>
__global__ __launch_bounds__(256) void k_tree_place(const unsigned char* __restrict__ src, const PlaceJob* __restrict__ jobs, T* __restrict__ out,
                                                    unsigned long long box_x) {
    const PlaceJob j = jobs[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t r = blockIdx.x * 4 + wave; r < j.nrows; r += gridDim.x * 4) {
        const T* row = reinterpret_cast<const T*>(src + j.src_off + (unsigned long long)r * j.src_pitch) + j.x0;
        T* dst = out + j.dst_off + (unsigned long long)r * box_x;
        for (uint32_t x = lane; x < j.ncols; x += 64) dst[x] = row[x];
    }
}

// ------------------------------------------------------------------------------------------------------------------ directories
struct Page {
    std::vector<uint64_t> off, cnt;
};

struct File3D {
    std::string path;
    int fd = -1;
    bool big = false;
    uint64_t size = 0;
    uint32_t w = 0, h = 0, bytes = 0, comp = 1, rps = 0, nstrips = 0;
    std::vector<Page> pages;
    File3D() = default;
    File3D(const File3D&) = delete;
    File3D& operator=(const File3D&) = delete;
    ~File3D() {
        if (fd >= 0) close(fd);
    }
    uint32_t strip_rows(uint32_t s) const { return std::min(rps, h - s * rps); }
};

std::string sfmt(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
std::string sfmt(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

const char* tag_name(uint32_t tag) {
    switch (tag) {
        case 256: return "ImageWidth";
        case 257: return "ImageLength";
        case 258: return "BitsPerSample";
        case 259: return "Compression";
        case 273: return "StripOffsets";
        case 277: return "SamplesPerPixel";
        case 278: return "RowsPerStrip";
        case 279: return "StripByteCounts";
        case 317: return "Predictor";
        case 322: return "TileWidth";
        case 339: return "SampleFormat";
        default: return "tag";
    }
}

uint64_t le(const unsigned char* p, int n) {
    uint64_t v = 0;
    for (int k = 0; k < n; ++k) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

// Opens and parses the whole directory chain; "" or the message.  The file stays open (fd) for the strips.
std::string parse_file(const char* path, File3D& f) {
    f.path = path;
    f.fd = open(path, O_RDONLY | O_CLOEXEC);
    if (f.fd < 0) return sfmt("%s: %s", path, std::strerror(errno));
    struct stat st;
    if (fstat(f.fd, &st) != 0) return sfmt("%s: %s", path, std::strerror(errno));
    f.size = (uint64_t)st.st_size;
    unsigned char hdr[16];
    if (f.size < 8 || !mi::pread_all(f.fd, hdr, 8, 0)) return sfmt("%s: not a TIFF (shorter than a header)", path);
    if (hdr[0] != 'I' || hdr[1] != 'I') return sfmt("%s: not a little-endian TIFF", path);
    const uint64_t magic = le(hdr + 2, 2);
    if (magic != 42 && magic != 43) return sfmt("%s: not a TIFF (magic %llu)", path, (unsigned long long)magic);
    f.big = magic == 43;
    uint64_t ifd;
    if (f.big) {
        if (f.size < 16 || !mi::pread_all(f.fd, hdr, 16, 0) || le(hdr + 4, 2) != 8) return sfmt("%s: not a BigTIFF with 8-byte offsets", path);
        ifd = le(hdr + 8, 8);
    } else {
        ifd = le(hdr + 4, 4);
    }
    const int esize = f.big ? 20 : 12, csize = f.big ? 8 : 2, osize = f.big ? 8 : 4;
    const uint64_t max_pages = f.size / (uint64_t)(csize + esize + osize) + 1;   // a chain with more directories than fit loops
    std::vector<unsigned char> buf, arr;
    while (ifd != 0) {
        const int page = (int)f.pages.size();
        if ((uint64_t)page >= max_pages) return sfmt("%s: page %d: the directory chain loops", path, page);
        unsigned char cb[8];
        if (ifd + (uint64_t)csize > f.size || ifd + (uint64_t)csize < ifd || !mi::pread_all(f.fd, cb, (size_t)csize, ifd))
            return sfmt("%s: page %d: directory at %llu outside the file", path, page, (unsigned long long)ifd);
        const uint64_t n = le(cb, csize);
        if (n == 0 || n > 4096) return sfmt("%s: page %d: directory of %llu entries", path, page, (unsigned long long)n);
        buf.resize((size_t)(n * esize + osize));
        if (ifd + csize + buf.size() > f.size || !mi::pread_all(f.fd, buf.data(), buf.size(), ifd + csize))
            return sfmt("%s: page %d: directory at %llu outside the file", path, page, (unsigned long long)ifd);
        uint64_t w = 0, h = 0, bits = 1, comp = 1, spp = 1, rps = ~0ull, pred = 1, fmt = 1;
        uint64_t so_count = 0, so_val = 0, so_type = 0, sc_count = 0, sc_val = 0, sc_type = 0;
        bool have_so = false, have_sc = false;
        for (uint64_t e = 0; e < n; ++e) {
            const unsigned char* p = buf.data() + e * esize;
            const uint32_t tag = (uint32_t)le(p, 2), type = (uint32_t)le(p + 2, 2);
            const uint64_t count = le(p + 4, osize);
            const unsigned char* vp = p + 4 + osize;
            const int tsize = type == 3 ? 2 : type == 4 ? 4 : type == 16 ? 8 : type == 1 ? 1 : 0;
            auto scalar = [&](uint64_t& dst) -> std::string {
                if (tsize == 0 || count < 1 || (uint64_t)tsize * count > (uint64_t)osize)
                    return sfmt("%s: page %d: tag %u (%s) of type %u and count %llu", path, page, tag, tag_name(tag), type, (unsigned long long)count);
                dst = le(vp, tsize);
                for (uint64_t k = 1; k < count; ++k)
                    if (le(vp + k * tsize, tsize) != dst)
                        return sfmt("%s: page %d: tag %u (%s) differs between samples", path, page, tag, tag_name(tag));
                return std::string();
            };
            std::string err;
            switch (tag) {
                case 256: err = scalar(w); break;
                case 257: err = scalar(h); break;
                case 258: err = scalar(bits); break;
                case 259: err = scalar(comp); break;
                case 277: err = scalar(spp); break;
                case 278: err = scalar(rps); break;
                case 317: err = scalar(pred); break;
                case 339: err = scalar(fmt); break;
                case 273: have_so = true; so_count = count; so_val = le(vp, osize); so_type = type; break;
                case 279: have_sc = true; sc_count = count; sc_val = le(vp, osize); sc_type = type; break;
                case 322: case 323: case 324: case 325:
                    return sfmt("%s: page %d: tag %u (%s): tiled pages are not read (strips only)", path, page, tag, tag_name(322));
                default: break;
            }
            if (!err.empty()) return err;
        }
        if (spp != 1) return sfmt("%s: page %d: tag 277 (SamplesPerPixel) is %llu: one sample per pixel is read", path, page, (unsigned long long)spp);
        if (bits != 8 && bits != 16) return sfmt("%s: page %d: tag 258 (BitsPerSample) is %llu: 8 or 16 bits are read", path, page, (unsigned long long)bits);
        if (fmt != 1) return sfmt("%s: page %d: tag 339 (SampleFormat) is %llu: unsigned samples are read", path, page, (unsigned long long)fmt);
        if (comp != 1 && comp != 5)
            return sfmt("%s: page %d: tag 259 (Compression) is %llu: uncompressed (1) and LZW (5) are read", path, page, (unsigned long long)comp);
        if (pred == 2) return sfmt("%s: page %d: tag 317 (Predictor) is 2: horizontal differencing is not read", path, page);
        if (pred != 1) return sfmt("%s: page %d: tag 317 (Predictor) is %llu", path, page, (unsigned long long)pred);
        if (w == 0 || h == 0 || w > 0x7fffffffull || h > 0x7fffffffull)
            return sfmt("%s: page %d: tags 256 / 257 (ImageWidth / ImageLength): %llu x %llu", path, page, (unsigned long long)w, (unsigned long long)h);
        if (rps == 0) return sfmt("%s: page %d: tag 278 (RowsPerStrip) is 0", path, page);
        if (rps > h) rps = h;
        const uint64_t rowb = w * (bits / 8), nstrips = (h + rps - 1) / rps;
        if (rps * rowb >= 0x7fffffffull) return sfmt("%s: page %d: tag 278 (RowsPerStrip): a strip of %llu rows is larger than 2 GB", path, page, (unsigned long long)rps);
        if (page == 0) {
            f.w = (uint32_t)w;
            f.h = (uint32_t)h;
            f.bytes = (uint32_t)(bits / 8);
            f.comp = (uint32_t)comp;
            f.rps = (uint32_t)rps;
            f.nstrips = (uint32_t)nstrips;
        } else if (w != f.w || h != f.h || bits / 8 != f.bytes || comp != f.comp || rps != f.rps) {
            return sfmt("%s: page %d: tags 256 / 257 / 258 / 259 / 278: %llu x %llu of %llu bits, compression %llu, %llu rows per strip differ from page 0 "
                        "(%u x %u of %u bits, compression %u, %u rows per strip)",
                        path, page, (unsigned long long)w, (unsigned long long)h, (unsigned long long)bits, (unsigned long long)comp,
                        (unsigned long long)rps, f.w, f.h, 8 * f.bytes, f.comp, f.rps);
        }
        if (!have_so || so_count != nstrips)
            return sfmt("%s: page %d: tag 273 (StripOffsets) has %llu values, the page has %llu strips", path, page,
                        (unsigned long long)(have_so ? so_count : 0), (unsigned long long)nstrips);
        if (!have_sc || sc_count != nstrips)
            return sfmt("%s: page %d: tag 279 (StripByteCounts) has %llu values, the page has %llu strips", path, page,
                        (unsigned long long)(have_sc ? sc_count : 0), (unsigned long long)nstrips);
        Page pg;
        auto load = [&](uint32_t tag, uint64_t type, uint64_t val, const unsigned char* inl, std::vector<uint64_t>& dst) -> std::string {
            const int tsize = type == 3 ? 2 : type == 4 ? 4 : type == 16 ? 8 : 0;
            if (tsize == 0) return sfmt("%s: page %d: tag %u (%s) of type %llu", path, page, tag, tag_name(tag), (unsigned long long)type);
            const uint64_t nb = nstrips * (uint64_t)tsize;
            const unsigned char* p = inl;
            if (nb > (uint64_t)osize) {
                if (val > f.size || nb > f.size - val) return sfmt("%s: page %d: tag %u (%s): its values lie outside the file", path, page, tag, tag_name(tag));
                arr.resize((size_t)nb);
                if (!mi::pread_all(f.fd, arr.data(), arr.size(), val)) return sfmt("%s: page %d: tag %u (%s) cannot be read", path, page, tag, tag_name(tag));
                p = arr.data();
            }
            dst.resize((size_t)nstrips);
            for (uint64_t s = 0; s < nstrips; ++s) dst[(size_t)s] = le(p + s * tsize, tsize);
            return std::string();
        };
        // (the inline value was read as osize bytes little-endian: hand its bytes back)
        unsigned char so_inl[8], sc_inl[8];
        for (int k = 0; k < 8; ++k) {
            so_inl[k] = (unsigned char)(so_val >> (8 * k));
            sc_inl[k] = (unsigned char)(sc_val >> (8 * k));
        }
        std::string err = load(273, so_type, so_val, so_inl, pg.off);
        if (err.empty()) err = load(279, sc_type, sc_val, sc_inl, pg.cnt);
        if (!err.empty()) return err;
        // the bounds of checked_strips (tiffio.hip): strips inside the file, raw strips as long as their rows
        for (uint64_t s = 0; s < nstrips; ++s) {
            const uint64_t o = pg.off[(size_t)s], c = pg.cnt[(size_t)s];
            if (o > f.size || c > f.size - o)
                return sfmt("%s: page %d: strip %llu: tags 273 / 279 (StripOffsets / StripByteCounts) put it outside the file", path, page, (unsigned long long)s);
            const uint64_t want = std::min<uint64_t>(rps, h - s * rps) * rowb;
            if (comp == 1 && c < want)
                return sfmt("%s: page %d: strip %llu: tag 279 (StripByteCounts) is %llu, its rows have %llu bytes", path, page, (unsigned long long)s,
                            (unsigned long long)c, (unsigned long long)want);
            if (c >= 0x7fffffffull) return sfmt("%s: page %d: strip %llu: tag 279 (StripByteCounts): larger than 2 GB", path, page, (unsigned long long)s);
        }
        f.pages.push_back(std::move(pg));
        ifd = le(buf.data() + n * esize, osize);
    }
    if (f.pages.empty()) return sfmt("%s: page 0: no directory", path);
    return std::string();
}

// ------------------------------------------------------------------------------------------------------------------ the plan of a call
// a run: strips [s0, s1) of a page that are read with one pread (they follow each other in the file)
struct Run {
    uint32_t s0, s1;
    uint64_t off, len;
};

// a piece: one page of one job
struct Piece {
    int job, file;
    uint32_t page, s0, s1;   // the strips its rows touch
};

struct Plan {
    std::vector<std::unique_ptr<File3D>> files;
    std::vector<int> job_file;
    std::vector<Piece> pieces;
};

// the runs of strips [s0, s1): LZW strips may have gaps (the bytes between are read and ignored), raw strips must touch, so that
// their rows are contiguous where they land
void runs_of(const File3D& f, const Page& pg, uint32_t s0, uint32_t s1, std::vector<Run>& out) {
    constexpr uint64_t kMaxGap = 4096, kMaxRun = 16u << 20;
    out.clear();
    for (uint32_t s = s0; s < s1; ++s) {
        const uint64_t o = pg.off[s], c = f.comp == 1 ? (uint64_t)f.strip_rows(s) * f.w * f.bytes : pg.cnt[s];
        if (!out.empty()) {
            Run& r = out.back();
            const uint64_t end = r.off + r.len;
            const bool follows = f.comp == 1 ? o == end : (o >= end && o - end <= kMaxGap);
            if (follows && o + c - r.off <= kMaxRun) {
                r.s1 = s + 1;
                r.len = o + c - r.off;
                continue;
            }
        }
        out.push_back({s, s + 1, o, c});
    }
}

int make_plan(const char* who, const mi_tiff3d_job* jobs, int n_jobs, int box_z, int box_y, int box_x, int bytes, const void* out, int n_threads,
              Plan& P) {
    MI_REQUIRE(n_jobs >= 0 && (n_jobs == 0 || jobs) && out, "%s: null pointer", who);
    MI_REQUIRE(box_z > 0 && box_y > 0 && box_x > 0 && (bytes == 1 || bytes == 2), "%s: a box of %d x %d x %d samples of %d bytes", who, box_z, box_y,
               box_x, bytes);
    std::map<std::string, int> index;
    std::vector<const char*> paths;
    P.job_file.resize((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        MI_REQUIRE(jobs[j].path, "%s: job %d has no path", who, j);
        auto it = index.find(jobs[j].path);
        if (it == index.end()) {
            it = index.emplace(jobs[j].path, (int)paths.size()).first;
            paths.push_back(jobs[j].path);
        }
        P.job_file[(size_t)j] = it->second;
    }
    const int nf = (int)paths.size();
    P.files.resize((size_t)nf);
    for (auto& f : P.files) f.reset(new File3D());
    MI_TRY(mi::run_jobs(nf, std::max(1, std::min(mi::tree_pool_threads(n_threads), nf)), [&](int k, int) { return parse_file(paths[(size_t)k], *P.files[(size_t)k]); }));
    for (int j = 0; j < n_jobs; ++j) {
        const mi_tiff3d_job& J = jobs[j];
        const File3D& f = *P.files[(size_t)P.job_file[(size_t)j]];
        MI_REQUIRE((int)f.bytes == bytes, "%s: samples of %u bytes, the box has samples of %d bytes", J.path, f.bytes, bytes);
        MI_REQUIRE(0 <= J.p0 && J.p0 < J.p1 && (size_t)J.p1 <= f.pages.size() && 0 <= J.y0 && J.y0 < J.y1 && (uint32_t)J.y1 <= f.h && 0 <= J.x0 &&
                       J.x0 < J.x1 && (uint32_t)J.x1 <= f.w,
                   "%s: pages [%d, %d) x rows [%d, %d) x columns [%d, %d) outside the file's %zu pages of %u x %u", J.path, J.p0, J.p1, J.y0, J.y1, J.x0,
                   J.x1, f.pages.size(), f.h, f.w);
        MI_REQUIRE(J.oz >= 0 && J.oy >= 0 && J.ox >= 0 && (long long)J.oz + (J.p1 - J.p0) <= box_z && (long long)J.oy + (J.y1 - J.y0) <= box_y &&
                       (long long)J.ox + (J.x1 - J.x0) <= box_x,
                   "%s: job %d: a piece of %d x %d x %d at (%d, %d, %d) passes the box of %d x %d x %d", who, j, J.p1 - J.p0, J.y1 - J.y0, J.x1 - J.x0,
                   J.oz, J.oy, J.ox, box_z, box_y, box_x);
        for (int p = J.p0; p < J.p1; ++p)
            P.pieces.push_back({j, P.job_file[(size_t)j], (uint32_t)p, (uint32_t)J.y0 / f.rps, ((uint32_t)J.y1 - 1) / f.rps + 1});
    }
    return MI_OK;
}

std::string strip_error(const File3D& f, uint32_t page, uint32_t strip, int status) {
    return sfmt("%s: page %u: strip %u does not decode to its rows (status %d: %s)", f.path.c_str(), page, strip, status, status_name(status));
}

// ------------------------------------------------------------------------------------------------------------------ device scratch
using mi::slot;

mi::ScratchPool g_scratch;   // this reader's own

size_t lzw_lds_bytes(bool lds_rows, bool wide, uint32_t entries, uint32_t max_rows) {
    return 4 * ((size_t)kStageWords + 1 + entries + (wide ? (entries + 1) / 2 : 0)) + (lds_rows ? (size_t)((max_rows + 3) & ~3u) : 0);
}

template <class T>
void launch_place(hipStream_t s, uint32_t max_rows, uint32_t njobs, const unsigned char* src, const PlaceJob* jobs, void* out, int box_x) {
    const uint32_t gx = std::min<uint32_t>(1024u, (max_rows + 3) / 4);
    for (uint32_t j0 = 0; j0 < njobs; j0 += 65535u)   // (grid y)
        hipLaunchKernelGGL(k_tree_place<T>, dim3(gx, std::min<uint32_t>(65535u, njobs - j0)), dim3(256), 0, s, src, jobs + j0, static_cast<T*>(out),
                           (unsigned long long)box_x);
}

}  // namespace

namespace mi {
void tiff3d_read_drop_scratch(int dev) { g_scratch.drop(dev); }
}  // namespace mi

extern "C" int mi_tiff3d_info(const char* path, int* nx, int* ny, int* pages, int* dtype, int* compression, int* rows_per_strip, int* bigtiff) {
    MI_REQUIRE(path && nx && ny && pages && dtype && compression && rows_per_strip && bigtiff, "mi_tiff3d_info: null pointer");
    File3D f;
    const std::string err = parse_file(path, f);
    if (!err.empty()) return fail(MI_ERR_INVALID, "%s", err.c_str());
    MI_REQUIRE(f.pages.size() <= 0x7fffffffull, "%s: more than 2^31 pages", path);
    *nx = (int)f.w;
    *ny = (int)f.h;
    *pages = (int)f.pages.size();
    *dtype = (int)f.bytes;
    *compression = (int)f.comp;
    *rows_per_strip = (int)f.rps;
    *bigtiff = f.big ? 1 : 0;
    return MI_OK;
}

extern "C" int mi_tiff_lzw_decode(const void* src, int64_t n, void* dst, int64_t want, int* status) {
    MI_REQUIRE((src || n == 0) && (dst || want == 0) && status && n >= 0 && want >= 0, "mi_tiff_lzw_decode: bad arguments");
    MI_REQUIRE(n < 0x7fffffffll && want < 0x7fffffffll, "mi_tiff_lzw_decode: a strip of %lld bytes for %lld is larger than 2 GB", (long long)n,
               (long long)want);
    const uint32_t entries = table_entries((uint32_t)want);
    std::vector<uint32_t> off(entries ? entries : 1);
    std::vector<uint16_t> len(entries ? entries : 1);
    *status = lzw_host(static_cast<const unsigned char*>(src), (uint32_t)n, static_cast<unsigned char*>(dst), (uint32_t)want, off.data(), len.data());
    if (*status != kLzwOk)
        return fail(MI_ERR_INVALID, "mi_tiff_lzw_decode: the strip does not decode to %lld bytes (status %d: %s)", (long long)want, *status,
                    status_name(*status));
    return MI_OK;
}

extern "C" int mi_tiff3d_read_box(const mi_tiff3d_job* jobs, int n_jobs, int box_z, int box_y, int box_x, int bytes, void* out, int n_threads) {
    Plan P;
    MI_TRY(make_plan("mi_tiff3d_read_box", jobs, n_jobs, box_z, box_y, box_x, bytes, out, n_threads, P));
    MI_REQUIRE(P.pieces.size() < 0x7fffffffull, "mi_tiff3d_read_box: more than 2^31 pages in the box");
    const int np = (int)P.pieces.size();
    if (np == 0) return MI_OK;
    const int nt = std::max(1, std::min(mi::tree_pool_threads(n_threads), np));
    struct Work {
        std::vector<unsigned char> file, rows;
        std::vector<uint32_t> off;
        std::vector<uint16_t> len;
        std::vector<Run> runs;
    };
    std::vector<Work> work((size_t)nt);
    unsigned char* dst = static_cast<unsigned char*>(out);
    return mi::run_jobs(np, nt, [&](int i, int t) -> std::string {
        const Piece& pc = P.pieces[(size_t)i];
        const mi_tiff3d_job& J = jobs[pc.job];
        const File3D& f = *P.files[(size_t)pc.file];
        const Page& pg = f.pages[pc.page];
        Work& W = work[(size_t)t];
        const size_t rowb = (size_t)f.w * f.bytes, colb = (size_t)(J.x1 - J.x0) * f.bytes;
        runs_of(f, pg, pc.s0, pc.s1, W.runs);
        for (const Run& r : W.runs) {
            W.file.resize((size_t)r.len);
            if (!mi::pread_all(f.fd, W.file.data(), (size_t)r.len, r.off)) return f.path + ": " + mi::kTruncatedStrip;
            for (uint32_t s = r.s0; s < r.s1; ++s) {
                const uint32_t r0 = s * f.rps, nr = f.strip_rows(s);
                const size_t want = (size_t)nr * rowb;
                const unsigned char* raw = W.file.data() + (pg.off[s] - r.off);
                if (f.comp == 5) {
                    W.rows.resize(want);
                    const uint32_t entries = table_entries((uint32_t)want);
                    if (W.off.size() < entries) {
                        W.off.resize(entries);
                        W.len.resize(entries);
                    }
                    const int st = lzw_host(raw, (uint32_t)pg.cnt[s], W.rows.data(), (uint32_t)want, W.off.data(), W.len.data());
                    if (st != kLzwOk) return strip_error(f, pc.page, s, st);
                    raw = W.rows.data();
                }
                const uint32_t a = std::max<uint32_t>(r0, (uint32_t)J.y0), b = std::min<uint32_t>(r0 + nr, (uint32_t)J.y1);
                for (uint32_t y = a; y < b; ++y) {
                    const size_t at = (((size_t)(J.oz + (int)pc.page - J.p0) * (size_t)box_y + (size_t)(J.oy + (int)y - J.y0)) * (size_t)box_x + (size_t)J.ox) *
                                      (size_t)bytes;
                    std::memcpy(dst + at, raw + (size_t)(y - r0) * rowb + (size_t)J.x0 * f.bytes, colb);
                }
            }
        }
        return std::string();
    });
}

extern "C" int mi_tiff3d_read_box_device(int dev, void* stream, const mi_tiff3d_job* jobs, int n_jobs, int box_z, int box_y, int box_x, int bytes,
                                         void* out, int n_threads) {
    MI_TRY(mi::use_device(dev));
    Plan P;
    MI_TRY(make_plan("mi_tiff3d_read_box_device", jobs, n_jobs, box_z, box_y, box_x, bytes, out, n_threads, P));
    if (P.pieces.empty()) return MI_OK;
    hipStream_t s = mi::as_stream(stream);

    const std::shared_ptr<mi::DeviceScratch> sc = g_scratch.get(dev);
    std::lock_guard<std::mutex> hold(sc->mu);

    // Batches of whole pieces (a page of a job), bounded as the slice reader bounds its batches: at most 1 GB of file bytes and 1 GB
    // of decoded rows at a time.  The strip bound is another one: there a strip is a megabyte and 16 384 of them are the gigabyte;
    // here a strip is a row -- one block of the tree's own files has 16 384 of 512 bytes, 8 MB -- and a wave lasts microseconds, so
    // the device wants tens of thousands at once.  2^20 strips bound the job lists (24 + 4 bytes per strip, 32 bytes per place job:
    // about 60 MB pinned and on the device) and are half a gigabyte of such rows, so for the tree's own files the byte bounds and
    // the strip bound meet.
    constexpr size_t kMaxRead = (size_t)1 << 30, kMaxRows = (size_t)1 << 30, kMaxStrips = (size_t)1 << 20;
    struct RunAt {
        Run r;
        size_t piece, at;   // the piece (of the batch) and where its bytes go in the upload
    };
    std::vector<Run> runs;
    std::vector<RunAt> reads;
    struct LzwRef {
        uint32_t piece, strip;
    };
    for (size_t b0 = 0; b0 < P.pieces.size();) {
        // 1) the batch and its layout: [upload: the runs, each from a multiple of 16][decoded rows: the pieces, each from a multiple of 16]
        reads.clear();
        std::vector<size_t> dec_at;   // per piece: its decoded rows (LZW), relative to the decoded part
        size_t b1 = b0, read_bytes = 0, row_bytes = 0, n_strips = 0;
        while (b1 < P.pieces.size()) {
            const Piece& pc = P.pieces[b1];
            const File3D& f = *P.files[(size_t)pc.file];
            runs_of(f, f.pages[pc.page], pc.s0, pc.s1, runs);
            size_t rb = read_bytes, wb = row_bytes;
            for (const Run& r : runs) rb += slot((size_t)r.len);
            if (f.comp == 5) wb += slot((size_t)(std::min(pc.s1 * f.rps, f.h) - pc.s0 * f.rps) * f.w * f.bytes);
            if (b1 > b0 && (rb > kMaxRead || wb > kMaxRows || n_strips + (pc.s1 - pc.s0) > kMaxStrips)) break;
            size_t at = read_bytes;
            for (const Run& r : runs) {
                reads.push_back({r, b1 - b0, at});
                at += slot((size_t)r.len);
            }
            dec_at.push_back(row_bytes);
            read_bytes = rb;
            row_bytes = wb;
            n_strips += pc.s1 - pc.s0;
            ++b1;
        }
        MI_REQUIRE(reads.size() < 0x7fffffffull, "mi_tiff3d_read_box_device: more than 2^31 reads in a batch");
        // 2) the jobs: LZW strips in three classes (rows in LDS / rows in global memory / offsets of 32 bits), place jobs
        std::vector<LzwJob> lj[3];
        std::vector<LzwRef> lref[3];
        uint32_t lmax[3] = {0, 0, 0};
        std::vector<PlaceJob> pj;
        uint32_t max_rows = 0;
        for (const RunAt& ra : reads) {
            const Piece& pc = P.pieces[b0 + ra.piece];
            const mi_tiff3d_job& J = jobs[pc.job];
            const File3D& f = *P.files[(size_t)pc.file];
            const Page& pg = f.pages[pc.page];
            const size_t rowb = (size_t)f.w * f.bytes;
            if (f.comp == 5) {
                for (uint32_t q = ra.r.s0; q < ra.r.s1; ++q) {
                    const uint32_t want = (uint32_t)(f.strip_rows(q) * rowb);
                    const int cls = want <= kLdsRows ? 0 : want <= 65536u ? 1 : 2;
                    lj[cls].push_back({(unsigned long long)(ra.at + (pg.off[q] - ra.r.off)),
                                       (unsigned long long)(dec_at[ra.piece] + (size_t)(q - pc.s0) * f.rps * rowb), (uint32_t)pg.cnt[q], want});
                    lref[cls].push_back({(uint32_t)ra.piece, q});
                    lmax[cls] = std::max(lmax[cls], want);
                }
                if (ra.r.s0 != pc.s0) continue;   // one place job per LZW piece: its decoded strips are contiguous
            }
            // rows [a, b) of the page: those of the run (raw) or of the piece (LZW) that lie in the job
            const uint32_t first = f.comp == 5 ? pc.s0 : ra.r.s0, last = f.comp == 5 ? pc.s1 : ra.r.s1;
            const uint32_t a = std::max<uint32_t>(first * f.rps, (uint32_t)J.y0), b = std::min<uint32_t>(std::min(last * f.rps, f.h), (uint32_t)J.y1);
            PlaceJob q;
            q.src_off = (f.comp == 5 ? read_bytes + dec_at[ra.piece] : ra.at) + (size_t)(a - first * f.rps) * rowb;
            q.dst_off = ((unsigned long long)(J.oz + (int)pc.page - J.p0) * (unsigned long long)box_y + (unsigned long long)(J.oy + (int)a - J.y0)) *
                            (unsigned long long)box_x +
                        (unsigned long long)J.ox;
            q.src_pitch = (uint32_t)rowb;
            q.x0 = (uint32_t)J.x0;
            q.ncols = (uint32_t)(J.x1 - J.x0);
            q.nrows = b - a;
            max_rows = std::max(max_rows, q.nrows);
            pj.push_back(q);
        }
        const size_t n_lzw = lj[0].size() + lj[1].size() + lj[2].size();
        // [LzwJob x n_lzw | PlaceJob x | status x n_lzw], the same layout on both sides
        const auto [place_at, status_at, jobs_bytes] = mi::job_layout(n_lzw, sizeof(LzwJob), pj.size(), sizeof(PlaceJob), n_lzw, sizeof(int32_t));
        MI_TRY(sc->h_bytes.reserve(read_bytes));
        MI_TRY(sc->h_jobs.reserve(jobs_bytes));
        MI_TRY(sc->grow(sc->d_bytes, read_bytes + row_bytes));
        MI_TRY(sc->grow(sc->d_jobs, jobs_bytes));
        unsigned char* hb = sc->h_bytes.as<unsigned char>();
        unsigned char* hj = sc->h_jobs.as<unsigned char>();
        int32_t* status = reinterpret_cast<int32_t*>(hj + status_at);
        {
            size_t k = 0;
            for (int c = 0; c < 3; ++c) {
                if (!lj[c].empty()) std::memcpy(hj + k * sizeof(LzwJob), lj[c].data(), lj[c].size() * sizeof(LzwJob));
                k += lj[c].size();
            }
            if (!pj.empty()) std::memcpy(hj + place_at, pj.data(), pj.size() * sizeof(PlaceJob));
            for (size_t q = 0; q < n_lzw; ++q) status[q] = -1;
        }
        // 3) the strips' bytes into pinned memory (the bytes between a run's end and the next multiple of 16 stay as they are: the
        //    kernel masks what is not the strip's)
        MI_TRY(mi::run_jobs((int)reads.size(), std::max(1, std::min<int>(mi::tree_pool_threads(n_threads), (int)reads.size())), [&](int i, int) -> std::string {
            const RunAt& ra = reads[(size_t)i];
            const File3D& f = *P.files[(size_t)P.pieces[b0 + ra.piece].file];
            return mi::pread_all(f.fd, hb + ra.at, (size_t)ra.r.len, ra.r.off) ? std::string() : f.path + ": " + mi::kTruncatedStrip;
        }));
        unsigned char* d_all = sc->d_bytes.as<unsigned char>();
        unsigned char* dj = sc->d_jobs.as<unsigned char>();
        MI_HIP(hipMemcpyAsync(d_all, hb, read_bytes, hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(dj, hj, jobs_bytes, hipMemcpyHostToDevice, s));
        // 4) decode: a launch per class, its table sized to the class' longest strip
        size_t k0 = 0;
        for (int c = 0; c < 3; ++c) {
            const size_t n = lj[c].size();
            if (n == 0) continue;
            const uint32_t entries = table_entries(lmax[c]);
            const size_t lds = lzw_lds_bytes(c == 0, c == 2, entries, lmax[c]);
            const LzwJob* d_lj = reinterpret_cast<const LzwJob*>(dj) + k0;
            int32_t* d_st = reinterpret_cast<int32_t*>(dj + status_at) + k0;
            if (c == 0) hipLaunchKernelGGL((k_strip_lzw<true, false>), dim3((uint32_t)n), dim3(64), lds, s, d_all, d_all + read_bytes, d_lj, d_st, entries);
            else if (c == 1) hipLaunchKernelGGL((k_strip_lzw<false, false>), dim3((uint32_t)n), dim3(64), lds, s, d_all, d_all + read_bytes, d_lj, d_st, entries);
            else hipLaunchKernelGGL((k_strip_lzw<false, true>), dim3((uint32_t)n), dim3(64), lds, s, d_all, d_all + read_bytes, d_lj, d_st, entries);
            MI_TRY(mi::launch_check("k_strip_lzw"));
            k0 += n;
        }
        if (n_lzw) MI_HIP(hipMemcpyAsync(status, dj + status_at, n_lzw * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        // 5) place
        const PlaceJob* d_pj = reinterpret_cast<const PlaceJob*>(dj + place_at);
        if (bytes == 1) launch_place<uint8_t>(s, max_rows, (uint32_t)pj.size(), d_all, d_pj, out, box_x);
        else launch_place<uint16_t>(s, max_rows, (uint32_t)pj.size(), d_all, d_pj, out, box_x);
        MI_TRY(mi::launch_check("k_tree_place"));
        MI_HIP(hipStreamSynchronize(s));
        size_t q = 0;
        for (int c = 0; c < 3; ++c)
            for (size_t i = 0; i < lj[c].size(); ++i, ++q) {
                if (status[q] == kLzwOk) continue;
                const Piece& pc = P.pieces[b0 + lref[c][i].piece];
                return fail(MI_ERR_INVALID, "%s", strip_error(*P.files[(size_t)pc.file], pc.page, lref[c][i].strip, (int)status[q]).c_str());
            }
        b0 = b1;
    }
    return MI_OK;
}
