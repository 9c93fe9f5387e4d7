// The device TIFF writer (include/mi_tiffio.h, mi_tiff_write_series_device): the mirror of the device reader in tiff_inflate.hip.
//
// The writer of tiffio.hip spends the host's cores on deflate: 2.7 GB/s on the 16 CPUs of a one-GPU container, while the slab it writes was
// computed on the device in a fraction of that time.  mi_tiff_write_series_device compresses where the samples are: every strip
// becomes ONE dynamic-Huffman deflate block.  Microscope samples are noise on a smooth field: what deflate saves on them at level 1 is
// the entropy coding, matches are rare -- except in the background of a stitched, cleaned or clipped volume, which is runs of equal
// bytes.  So a strip takes one of two forms, the shorter: every byte a literal, or its runs as matches at distance 1 (zlib's Z_RLE;
// the token rule stands at length_code below).  Three steps:
//   k_strip_count   per strip: histogram of its bytes and the two sums of its Adler-32 (strip_hist), and what the run form changes in
//                   them (strip_runs: the bytes inside matches, the matches per length symbol, their extra bits);
//   host            per strip: length-limited Huffman code (15 bits) of the literals + end-of-block (+ the length symbols in use),
//                   the block header (RFC 1951 3.2.7: every code length sent plainly through the code-length code, no run symbols),
//                   the exact size of both forms and the choice; the streams' places in one compact buffer;
//   k_strip_encode  per strip: a work-group walks over tiles of 8 KB; a lane takes 32 bytes, the lanes' bit counts are scanned, every
//                   lane ORs its codes into the tile's bit image in LDS, the image goes out as whole words.
// The host then only frames the streams (zlib header, header bits, Adler-32) and writes the files.  Any inflater reads the result;
// a strip whose bytes are all equally likely costs 130 bytes more than stored.  MI_TIFF_DEVICE_RUNS=0: the literal form only.
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mi_internal.h"
#include "mi_tiffio.h"
#include "tiffio_internal.h"

namespace {

using mi::fail;
using mi::run_jobs;

struct HuffCode {
    uint8_t len[288];
    uint16_t code[288];  // bit-reversed: emitted least significant bit first
};

// code lengths of at most `maxlen` bits for the symbols with f[i] > 0 (n <= 288, at least two of them used)
void huff_lengths(const uint32_t* f, int n, int maxlen, uint8_t* len) {
    struct Node { uint64_t w; int l, r; };
    std::vector<Node> nodes;
    std::vector<int> used;
    for (int i = 0; i < n; ++i) {
        len[i] = 0;
        if (f[i]) used.push_back(i);
    }
    if (used.size() == 1) { len[used[0]] = 1; return; }
    std::sort(used.begin(), used.end(), [&](int a, int b) { return f[a] != f[b] ? f[a] < f[b] : a < b; });
    const int m = (int)used.size();
    nodes.reserve(2 * (size_t)m);
    for (int i = 0; i < m; ++i) nodes.push_back({f[used[(size_t)i]], -1, -1});
    // two queues: leaves in ascending order, internal nodes in creation order (ascending too)
    int a = 0, b = m;
    auto take = [&]() {
        int pick;
        if (a < m && (b >= (int)nodes.size() || nodes[(size_t)a].w <= nodes[(size_t)b].w)) pick = a++;
        else pick = b++;
        return pick;
    };
    for (int k = 0; k < m - 1; ++k) {
        const int x = take(), y = take();
        nodes.push_back({nodes[(size_t)x].w + nodes[(size_t)y].w, x, y});
    }
    std::vector<int> depth(nodes.size(), 0);
    for (int i = (int)nodes.size() - 1; i >= m; --i) {
        depth[(size_t)nodes[(size_t)i].l] = depth[(size_t)i] + 1;
        depth[(size_t)nodes[(size_t)i].r] = depth[(size_t)i] + 1;
    }
    // the number of codes of every length, limited to maxlen (the usual Kraft repair: a code moves down from the deepest occupied
    // level above, its two children take the place), then handed out by frequency: the rarest symbols get the longest codes
    int cnt[64] = {0};
    for (int i = 0; i < m; ++i) cnt[std::min(depth[(size_t)i], 63)]++;
    for (int i = maxlen + 1; i < 64; ++i) { cnt[maxlen] += cnt[i]; cnt[i] = 0; }
    uint64_t total = 0;
    for (int i = maxlen; i > 0; --i) total += (uint64_t)cnt[i] << (maxlen - i);
    while (total != (1ull << maxlen)) {
        cnt[maxlen]--;
        for (int i = maxlen - 1; i > 0; --i)
            if (cnt[i]) { cnt[i]--; cnt[i + 1] += 2; break; }
        total--;
    }
    int at = 0;
    for (int l = maxlen; l > 0; --l)
        for (int c = 0; c < cnt[l]; ++c) len[used[(size_t)at++]] = (uint8_t)l;
}

// canonical codes of RFC 1951 3.2.2, each reversed over its own length
void huff_codes(const uint8_t* len, int n, uint16_t* code) {
    int bl[16] = {0}, next[16] = {0};
    for (int i = 0; i < n; ++i) bl[len[i]]++;
    bl[0] = 0;
    int c = 0;
    for (int b = 1; b <= 15; ++b) { c = (c + bl[b - 1]) << 1; next[b] = c; }
    for (int i = 0; i < n; ++i) {
        code[i] = 0;
        if (!len[i]) continue;
        const int v = next[len[i]]++;
        int r = 0;
        for (int k = 0; k < len[i]; ++k) r |= ((v >> k) & 1) << (len[i] - 1 - k);
        code[i] = (uint16_t)r;
    }
}

struct BitWriter {
    std::vector<unsigned char> b;
    uint64_t n = 0;
    void put(uint32_t v, int bits) {
        for (int k = 0; k < bits; ++k, ++n) {
            if ((n & 7) == 0) b.push_back(0);
            b.back() |= (unsigned char)(((v >> k) & 1u) << (n & 7));
        }
    }
};

// The token rule of the run form (DESIGN, "TIFF on the device"): a run is a maximal stretch of equal bytes inside a strip; its first
// byte is a literal; of the R bytes that follow, while R >= 3 one match of min(R, 258) bytes at distance 1 is taken off; the last
// 0 - 2 bytes are literals.  Length symbol, number of extra bits and their value of a match of `len` bytes (RFC 1951 3.2.5; 258 is
// symbol 285, never 284 with extra 31):
__host__ __device__ inline void length_code(uint32_t len, uint32_t& sym, uint32_t& nbits, uint32_t& val) {
    sym = 285; nbits = 0; val = 0;
    if (len == 258) return;
    const uint32_t l = len - 3;
    if (l < 8) { sym = 257 + l; return; }
    nbits = (uint32_t)(31 - __builtin_clz(l)) - 2;
    sym = 261 + 4 * nbits + ((l >> nbits) & 3);
    val = l & ((1u << nbits) - 1);
}

constexpr int kSyms = 286;       // literals, end of block, length symbols 257 .. 285
constexpr int kRunWords = 288;   // what strip_runs counts per strip and variant: [v] the bytes of value v that lie inside matches,
                                 // [256 + k] the matches of length symbol 257 + k, [285] the matches, [286] the sum of their extra bits

// the block header (bits before the first symbol) of the code of f[0 .. nsym) (257 <= nsym <= 286: HLIT as needed) and the table the
// encode kernel takes: [s] = len << 16 | code; payload_bits: the symbols' bits + other_bits (extra and distance bits of the matches)
void block_code(const uint32_t* f, int nsym, uint64_t other_bits, BitWriter& hdr, uint32_t* table /* kSyms */, uint64_t* payload_bits) {
    HuffCode lit;
    huff_lengths(f, nsym, 15, lit.len);
    huff_codes(lit.len, nsym, lit.code);
    // the literal / length code lengths + two distance codes of one bit each (the literal form uses none, the run form the first:
    // distance 1; two, because some inflaters want a complete distance code) sent one by one through the code-length code
    uint8_t all[kSyms + 2];
    for (int i = 0; i < nsym; ++i) all[i] = lit.len[i];
    all[nsym] = all[nsym + 1] = 1;
    uint32_t cf[19] = {0};
    for (int i = 0; i < nsym + 2; ++i) cf[all[i]]++;
    uint8_t cl[19];
    uint16_t cc[19];
    huff_lengths(cf, 19, 7, cl);
    huff_codes(cl, 19, cc);
    hdr.put(1, 1);                        // BFINAL
    hdr.put(2, 2);                        // BTYPE: dynamic Huffman
    hdr.put((uint32_t)(nsym - 257), 5);   // HLIT: 257 codes in the literal form
    hdr.put(1, 5);                        // HDIST: 2 codes
    hdr.put(15, 4);                       // HCLEN: all 19 code-length code lengths
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) hdr.put(cl[order[i]], 3);
    for (int i = 0; i < nsym + 2; ++i) hdr.put(cc[all[i]], cl[all[i]]);
    uint64_t bits = other_bits;
    for (int i = 0; i < nsym; ++i) bits += (uint64_t)f[i] * lit.len[i];
    *payload_bits = bits;
    for (int i = 0; i < kSyms; ++i) table[i] = i < nsym ? (uint32_t)lit.len[i] << 16 | lit.code[i] : 0u;
}

// One strip's code from its byte histogram and -- runs != nullptr -- its run counts (kRunWords): the literal form (every byte a
// literal: 257 codes, what the writer has always produced) or, when that makes header + payload shorter, the run form.
void strip_code(const uint32_t* hist, const uint32_t* runs, BitWriter& hdr, uint32_t* table /* kSyms */, uint64_t* payload_bits, bool* used_runs) {
    uint32_t f[kSyms];
    for (int i = 0; i < 256; ++i) f[i] = hist[i];
    f[256] = 1;  // end of block
    block_code(f, 257, 0, hdr, table, payload_bits);
    *used_runs = false;
    if (!runs || runs[285] == 0) return;
    int nsym = 257;
    for (int i = 0; i < 256; ++i) f[i] = hist[i] - runs[i];
    for (int i = 257; i < kSyms; ++i) {
        f[i] = runs[i - 1];
        if (f[i]) nsym = i + 1;
    }
    BitWriter hdr2;
    uint32_t table2[kSyms];
    uint64_t bits2 = 0;
    block_code(f, nsym, (uint64_t)runs[286] + runs[285], hdr2, table2, &bits2);   // (+ one distance bit per match)
    if (hdr2.n + bits2 >= hdr.n + *payload_bits) return;
    hdr = std::move(hdr2);
    std::memcpy(table, table2, sizeof table2);
    *payload_bits = bits2;
    *used_runs = true;
}

// the run counts of strip_runs and the tokens themselves on the host, run by run: tok(literal) / tok(256 + length) in stream order
template <class F>
void host_tokens(const unsigned char* b, size_t n, uint32_t* runs /* kRunWords, zeroed */, F&& tok) {
    for (size_t i = 0; i < n;) {
        size_t e = i + 1;
        while (e < n && b[e] == b[i]) ++e;
        tok((uint32_t)b[i]);
        size_t r = e - i - 1;
        while (r >= 3) {
            const uint32_t len = (uint32_t)std::min<size_t>(r, 258);
            uint32_t sym, nbits, val;
            length_code(len, sym, nbits, val);
            runs[b[i]] += len;
            runs[sym - 1]++;
            runs[285]++;
            runs[286] += nbits;
            tok(256 + len);
            r -= len;
        }
        for (; r > 0; --r) tok((uint32_t)b[i]);
        i = e;
    }
}

constexpr int kEncThreads = 256, kEncBytes = 32, kTileBytes = kEncThreads * kEncBytes;   // 8 KB of samples per tile
constexpr int kTileWords = kTileBytes * 15 / 8 / 4 + 6;   // its bit image at 15 bits per byte (+ the end of block, + in the run form the
                                                          // two literals that close a run which began in the tile before)

struct StripGeom {
    size_t slice_bytes, rowb;
    uint32_t rps, ns, ny, bps;
    __host__ __device__ size_t start(uint32_t strip) const { return (size_t)(strip / ns) * slice_bytes + (size_t)(strip % ns) * rps * rowb; }
    __host__ __device__ uint32_t bytes(uint32_t strip) const {
        const uint32_t r0 = (strip % ns) * rps, r1 = r0 + rps < ny ? r0 + rps : ny;
        return (uint32_t)((r1 - r0) * rowb);
    }
};

// NB bytes of a strip from byte j0 on (cnt of them exist), as stored: plain, or -- pred -- every 8 / 16-bit sample minus its left
// neighbour in the row (TIFF 6.0 section 14, horizontal differencing; the first sample of a row stays).  j0 is a multiple of NB.
template <int NB>
__device__ __forceinline__ void strip_bytes(const unsigned char* __restrict__ p, uint32_t j0, uint32_t cnt, bool aligned, uint32_t bps, uint32_t rowb,
                                            bool pred, unsigned char (&b)[NB]) {
    if (aligned && cnt == (uint32_t)NB) {
#pragma unroll
        for (int q = 0; q < NB / 16; ++q) *reinterpret_cast<uint4*>(b + 16 * q) = *reinterpret_cast<const uint4*>(p + j0 + 16 * q);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)NB; ++k) b[k] = k < cnt ? p[j0 + k] : 0;
    }
    if (!pred || cnt == 0) return;
    uint32_t col = j0 % rowb;   // byte column of the chunk's first byte
    if (bps == 2) {
        uint32_t prev = col ? (uint32_t)p[j0 - 2] | (uint32_t)p[j0 - 1] << 8 : 0;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)NB / 2; ++k) {
            const uint32_t v = (uint32_t)b[2 * k] | (uint32_t)b[2 * k + 1] << 8;
            const uint32_t d = (v - (col ? prev : 0u)) & 0xffffu;
            b[2 * k] = (unsigned char)(d & 255);
            b[2 * k + 1] = (unsigned char)(d >> 8);
            prev = v;
            col += 2;
            if (col >= rowb) col -= rowb;
        }
    } else {
        uint32_t prev = col ? (uint32_t)p[j0 - 1] : 0;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)NB; ++k) {
            const uint32_t v = b[k];
            b[k] = (unsigned char)((v - (col ? prev : 0u)) & 255);
            prev = v;
            col += 1;
            if (col >= rowb) col -= rowb;
        }
    }
}

// byte j of a strip as stored (strip_bytes for one byte)
__device__ __forceinline__ uint32_t stored_byte(const unsigned char* __restrict__ p, uint32_t j, uint32_t bps, uint32_t rowb, bool pred) {
    if (!pred) return p[j];
    const uint32_t col = j % rowb;
    if (bps == 2) {
        const uint32_t j2 = j - (col & 1), v = (uint32_t)p[j2] | (uint32_t)p[j2 + 1] << 8;
        const uint32_t prev = col >= 2 ? (uint32_t)p[j2 - 2] | (uint32_t)p[j2 - 1] << 8 : 0u;
        const uint32_t d = (v - prev) & 0xffffu;
        return col & 1 ? d >> 8 : d & 255;
    }
    return ((uint32_t)p[j] - (col ? (uint32_t)p[j - 1] : 0u)) & 255;
}

// The run form, a lane at a time.  The tokens of a run are handed out where their bytes END, so that a lane looks one byte ahead
// and no further: the head of a run is a literal; every other byte adds one to r, the bytes of the open chunk (the run's bytes after
// its head, in chunks of 258), and the byte that closes the chunk -- the 258th, or the last of the run -- emits it: one match of r
// bytes when r >= 3, else r literals.  That is the token rule, and the tokens leave in stream order.
//   head0: b[0] begins a run; end_after: the byte after the lane's last differs from it (or the strip ends there);
//   r: the open chunk's bytes before b[0] (0 .. 257; 0 when head0)
//   emit(t, v, twice): at most once per byte -- t < 256: the literal v = t, `twice` when two of them close a run; else a match of
//   t - 256 bytes of value v
template <class Emit>
__device__ __forceinline__ void lane_tokens(const unsigned char (&b)[kEncBytes], uint32_t cnt, bool head0, bool end_after, uint32_t r, Emit&& emit) {
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kEncBytes; ++k) {
        if (k < cnt) {
            const uint32_t v = b[k];
            const bool head = k == 0 ? head0 : b[k] != b[k ? k - 1 : 0];
            const bool closes = (k + 1 < (uint32_t)kEncBytes && k + 1 < cnt) ? b[(k + 1) % kEncBytes] != v : end_after;
            r = head ? 0u : r + 1;
            const bool flush = !head && (r == 258 || closes);
            if (head || flush) emit(flush && r >= 3 ? 256 + r : v, v, flush && r == 2);
            if (flush) r = 0;
        }
    }
}

// What lane_tokens needs from the lane's neighbours, over a work-group of kEncThreads lanes that hold kEncBytes consecutive bytes
// each from byte t0 of the strip on: the bytes next to the lane's own (through LDS; the tile's two ends are read from memory) and the
// open chunk at its first byte (a max-scan of the positions of the run heads; `carry`: the last head of the tiles before, + 1).
// Three steps with a barrier between them: publish | neighbours | finish.  Tile after tile needs no further barrier: a lane writes
// the next tile's bytes after the second barrier, when every neighbour has read this tile's, and the next wave maxima after the next
// tile's first barrier, when every lane has finished this tile.
struct RunLds {
    unsigned char first[kEncThreads], last[kEncThreads];
    uint32_t wmax[kEncThreads / 64];
};
struct LaneRuns {
    bool head0, end_after;   // of lane_tokens
    uint32_t r;              // of lane_tokens, after finish
    uint32_t before;         // the last run head (+ 1) of the lanes before this one in its wave
    __device__ __forceinline__ static void publish(RunLds& lds, const unsigned char (&b)[kEncBytes]) {
        lds.first[threadIdx.x] = b[0];
        lds.last[threadIdx.x] = b[kEncBytes - 1];
    }
    __device__ __forceinline__ void neighbours(RunLds& lds, const unsigned char* __restrict__ p, uint32_t n, uint32_t j0, uint32_t cnt, uint32_t bps,
                                               uint32_t rowb, bool pred, const unsigned char (&b)[kEncBytes]) {
        const uint32_t tid = threadIdx.x;
        head0 = false;
        end_after = false;
        uint32_t lh = 0;   // the lane's last run head, + 1 (0: none)
        if (cnt > 0) {
            head0 = j0 == 0 || (tid > 0 ? (uint32_t)lds.last[tid - 1] : stored_byte(p, j0 - 1, bps, rowb, pred)) != b[0];
            // (a lane of fewer than kEncBytes bytes is the strip's last)
            end_after = j0 + cnt >= n ||
                        (tid + 1 < (uint32_t)kEncThreads ? (uint32_t)lds.first[tid + 1] : stored_byte(p, j0 + cnt, bps, rowb, pred)) != b[kEncBytes - 1];
            if (head0) lh = j0 + 1;
#pragma unroll
            for (uint32_t k = 1; k < (uint32_t)kEncBytes; ++k)
                if (k < cnt && b[k] != b[k - 1]) lh = j0 + k + 1;
        }
        uint32_t incl = lh;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o, 64);
            if ((int)(tid & 63) >= o) incl = incl > v ? incl : v;
        }
        if ((tid & 63) == 63) lds.wmax[tid >> 6] = incl;
        const uint32_t left = __shfl_up(incl, 1, 64);
        before = (tid & 63) ? left : 0u;
    }
    __device__ __forceinline__ void finish(const RunLds& lds, uint32_t j0, uint32_t cnt, uint32_t& carry) {
        const uint32_t tid = threadIdx.x;
        before = before > carry ? before : carry;
        for (int w = 0; w < kEncThreads / 64; ++w) {
            const uint32_t m = lds.wmax[w];
            if (w < (int)(tid >> 6)) before = before > m ? before : m;
            carry = carry > m ? carry : m;
        }
        // byte j0 lies j0 - (before - 1) bytes behind its run's head: that many minus one precede it in the run's chunks
        r = (head0 || cnt == 0) ? 0u : (j0 - before) % 258u;
    }
};

// per strip: the run counts (kRunWords) of the bytes as they are and -- `both` -- horizontally differenced: runs[strip][v][kRunWords].
// Both variants of a tile share its two barriers.
__device__ __forceinline__ void strip_runs(uint32_t strip, const unsigned char* __restrict__ base, const StripGeom& g, int both, uint32_t* __restrict__ runs) {
    __shared__ uint32_t cnts[2][kRunWords];
    __shared__ RunLds lds[2];
    const uint32_t n = g.bytes(strip), tid = threadIdx.x;
    const unsigned char* p = base + g.start(strip);
    for (int i = tid; i < 2 * kRunWords; i += kEncThreads) (&cnts[0][0])[i] = 0;
    __syncthreads();
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    const uint32_t rowb = (uint32_t)g.rowb;
    uint32_t carry[2] = {0, 0}, matches[2] = {0, 0}, extra[2] = {0, 0};
    for (uint32_t t0 = 0; t0 < n; t0 += kTileBytes) {
        const uint32_t j0 = t0 + tid * kEncBytes;
        const uint32_t cnt = j0 < n ? (n - j0 < (uint32_t)kEncBytes ? n - j0 : (uint32_t)kEncBytes) : 0;
        unsigned char b0[kEncBytes], b1[kEncBytes];
        strip_bytes<kEncBytes>(p, j0 < n ? j0 : 0, cnt, aligned, g.bps, rowb, false, b0);
        LaneRuns::publish(lds[0], b0);
        if (both) {
            strip_bytes<kEncBytes>(p, j0 < n ? j0 : 0, cnt, aligned, g.bps, rowb, true, b1);
            LaneRuns::publish(lds[1], b1);
        }
        __syncthreads();
        LaneRuns l0, l1;
        l0.neighbours(lds[0], p, n, j0, cnt, g.bps, rowb, false, b0);
        if (both) l1.neighbours(lds[1], p, n, j0, cnt, g.bps, rowb, true, b1);
        __syncthreads();
        auto count = [&](int v, const unsigned char (&b)[kEncBytes], LaneRuns& l) {
            l.finish(lds[v], j0, cnt, carry[v]);
            uint32_t* c = cnts[v];
            lane_tokens(b, cnt, l.head0, l.end_after, l.r, [&](uint32_t t, uint32_t val, bool) {
                if (t < 256) return;
                uint32_t sym, nbits, x;
                length_code(t - 256, sym, nbits, x);
                atomicAdd(&c[val], t - 256);
                atomicAdd(&c[sym - 1], 1u);
                matches[v] += 1;
                extra[v] += nbits;
            });
        };
        count(0, b0, l0);
        if (both) count(1, b1, l1);
    }
    for (int v = 0; v < 2; ++v)
        if (matches[v]) {
            atomicAdd(&cnts[v][285], matches[v]);
            atomicAdd(&cnts[v][286], extra[v]);
        }
    __syncthreads();
    for (int i = tid; i < 2 * kRunWords; i += kEncThreads) runs[(size_t)strip * 2 * kRunWords + i] = (&cnts[0][0])[i];
}

// per strip: hist[strip][v][256] and sums[strip][v][2] for v = 0 (the bytes as they are) and -- `both` -- v = 1 (horizontally differenced)
__device__ __forceinline__ void strip_hist(uint32_t strip, const unsigned char* __restrict__ base, const StripGeom& g, int both, uint32_t* __restrict__ hist,
                                           unsigned long long* __restrict__ sums) {
    __shared__ uint32_t h[2][2][256];
    __shared__ unsigned long long ssum[4];
    const uint32_t n = g.bytes(strip), tid = threadIdx.x;
    const unsigned char* p = base + g.start(strip);
    for (int i = tid; i < 1024; i += 256) (&h[0][0][0])[i] = 0;
    if (tid < 4) ssum[tid] = 0;
    __syncthreads();
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    for (int v = 0; v < (both ? 2 : 1); ++v) {
        unsigned long long s1 = 0, s2 = 0;
        uint32_t* mine = h[v][tid & 1];
        for (uint32_t i = tid * 16; i < n; i += 256 * 16) {
            unsigned char b[16];
            const uint32_t m = n - i < 16 ? n - i : 16;
            strip_bytes<16>(p, i, m, aligned, g.bps, (uint32_t)g.rowb, v == 1, b);
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                if (k < m) {
                    atomicAdd(&mine[b[k]], 1u);
                    s1 += b[k];
                    s2 += (unsigned long long)(n - (i + k)) * b[k];
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_down(s1, o, 64);
            s2 += __shfl_down(s2, o, 64);
        }
        if ((tid & 63) == 0) {
            atomicAdd(&ssum[2 * v], s1);
            atomicAdd(&ssum[2 * v + 1], s2);
        }
    }
    __syncthreads();
    hist[(size_t)strip * 512 + tid] = h[0][0][tid] + h[0][1][tid];
    hist[(size_t)strip * 512 + 256 + tid] = h[1][0][tid] + h[1][1][tid];
    if (tid < 4) sums[(size_t)strip * 4 + tid] = ssum[tid];
}

// the counting pass, one launch: work-groups [0, nstrip) take the histograms, [nstrip, 2 nstrip) -- when launched -- the run counts
// of the same strips; both are bound by latency at a strip per work-group, side by side they hide each other's
__global__ __launch_bounds__(kEncThreads) void k_strip_count(const unsigned char* __restrict__ base, StripGeom g, int both, uint32_t nstrip,
                                                             uint32_t* __restrict__ hist, unsigned long long* __restrict__ sums, uint32_t* __restrict__ runs) {
    if (blockIdx.x < nstrip) strip_hist(blockIdx.x, base, g, both, hist, sums);
    else strip_runs(blockIdx.x - nstrip, base, g, both, runs);
}

// The symbols of a strip as bits, from bit hbits[strip] & 0x3fffffff of its stream on (the host puts the block header in front); the
// stream lies at byte offs[strip] of out.  Bit 31 of hbits: the strip is stored horizontally differenced; bit 30: it is coded in the
// run form.  RUNS = false: every byte is a literal.  RUNS = true: a lane emits, for each of its bytes, a literal, two, a match
// (length code, extra bits, the distance bit) or nothing (lane_tokens).
struct EncodeLds {
    uint32_t tab[kSyms];       // the strip's code: [s] = len << 16 | code
    uint32_t tok[256 + 259];   // run form: bits << 24 | the bits of [v] the literal v, [256 + l] a match of l bytes (length code, extra
                               // bits, distance code 0)
    RunLds lds;
    uint32_t img[kTileWords];
    uint32_t wsum[kEncThreads / 64];
};
template <bool RUNS>
__device__ __forceinline__ void encode_strip(EncodeLds& sh, const unsigned char* __restrict__ base, const StripGeom& g, const uint32_t* __restrict__ tables,
                                             const uint32_t* __restrict__ hbits, const unsigned long long* __restrict__ offs,
                                             unsigned char* __restrict__ out) {
    uint32_t(&tab)[kSyms] = sh.tab;
    uint32_t(&tok)[256 + 259] = sh.tok;
    RunLds& lds = sh.lds;
    uint32_t(&img)[kTileWords] = sh.img;
    uint32_t(&wsum)[kEncThreads / 64] = sh.wsum;
    const uint32_t strip = blockIdx.x, n = g.bytes(strip), tid = threadIdx.x;
    const unsigned char* p = base + g.start(strip);
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + offs[strip]);
    for (int i = tid; i < (RUNS ? kSyms : 257); i += kEncThreads) tab[i] = tables[(size_t)strip * kSyms + i];
    for (int i = tid; i < kTileWords; i += kEncThreads) img[i] = 0;
    __syncthreads();
    if (RUNS) {
        tok[tid] = (tab[tid] >> 16) << 24 | (tab[tid] & 0xffffu);
        for (uint32_t l = 3 + tid; l <= 258; l += kEncThreads) {
            uint32_t sym, nbits, val;
            length_code(l, sym, nbits, val);
            const uint32_t c = tab[sym], cl = c >> 16;
            tok[256 + l] = (cl + nbits + 1) << 24 | val << cl | (c & 0xffffu);
        }
        __syncthreads();
    }
    const bool pred = (hbits[strip] >> 31) != 0;
    unsigned long long bitpos = hbits[strip] & 0x3fffffffu;          // where the next tile's first bit goes in the strip's stream
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += kTileBytes) {
        const uint32_t j0 = t0 + tid * kEncBytes;
        const uint32_t cnt = j0 < n ? (n - j0 < (uint32_t)kEncBytes ? n - j0 : (uint32_t)kEncBytes) : 0;
        unsigned char b[kEncBytes];
        strip_bytes<kEncBytes>(p, j0 < n ? j0 : 0, cnt, aligned, g.bps, (uint32_t)g.rowb, pred, b);
        const bool last = cnt > 0 && j0 + cnt == n;   // this lane appends the end-of-block symbol
        LaneRuns lr;
        if (RUNS) {
            LaneRuns::publish(lds, b);
            __syncthreads();
            lr.neighbours(lds, p, n, j0, cnt, g.bps, (uint32_t)g.rowb, pred, b);
            __syncthreads();
            lr.finish(lds, j0, cnt, carry);
        }
        uint32_t mybits = 0;
        if (RUNS) {
            lane_tokens(b, cnt, lr.head0, lr.end_after, lr.r, [&](uint32_t t, uint32_t, bool twice) { mybits += (tok[t] >> 24) << (twice ? 1 : 0); });
        } else {
#pragma unroll
            for (uint32_t k = 0; k < (uint32_t)kEncBytes; ++k) mybits += k < cnt ? tab[b[k]] >> 16 : 0;
        }
        if (last) mybits += tab[256] >> 16;
        // exclusive scan of the lanes' bit counts over the work-group
        uint32_t incl = mybits;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o, 64);
            if ((int)(tid & 63) >= o) incl += v;
        }
        if ((tid & 63) == 63) wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t before = 0, tile_bits = 0;
        for (int w = 0; w < kEncThreads / 64; ++w) {
            if (w < (int)(tid >> 6)) before += wsum[w];
            tile_bits += wsum[w];
        }
        const uint32_t rel = (uint32_t)(bitpos & 31);   // the image's word 0 is the stream's word bitpos / 32
        uint32_t pos = rel + before + incl - mybits;
        uint32_t w = pos >> 5;
        unsigned long long acc = 0;
        uint32_t nb = pos & 31;
        auto put = [&](uint32_t code, uint32_t bits) {
            acc |= (unsigned long long)code << nb;
            nb += bits;
            if (nb >= 32) {
                atomicOr(&img[w++], (uint32_t)acc);
                acc >>= 32;
                nb -= 32;
            }
        };
        if (RUNS) {
            lane_tokens(b, cnt, lr.head0, lr.end_after, lr.r, [&](uint32_t t, uint32_t, bool twice) {
                const uint32_t c = tok[t], bits = c >> 24, code = c & 0xffffffu;
                put(twice ? code | code << bits : code, twice ? 2 * bits : bits);   // (two literals: 30 bits at most)
            });
        } else {
#pragma unroll
            for (uint32_t k = 0; k < (uint32_t)kEncBytes; ++k) {
                if (k < cnt) {
                    const uint32_t c = tab[b[k]];
                    put(c & 0xffffu, c >> 16);
                }
            }
        }
        if (last) {
            const uint32_t c = tab[256];
            put(c & 0xffffu, c >> 16);
        }
        if (nb > 0) atomicOr(&img[w], (uint32_t)acc);
        __syncthreads();
        // whole words out; the last, partial one stays behind as word 0 of the next tile's image
        const uint32_t end = rel + tile_bits, full = end >> 5;
        uint32_t* d = dst + (bitpos >> 5);
        for (uint32_t i = tid; i < full; i += kEncThreads) d[i] = img[i];
        const uint32_t carry_word = img[full];
        __syncthreads();
        for (uint32_t i = tid; i <= full; i += kEncThreads) img[i] = 0;
        __syncthreads();
        if (tid == 0) img[0] = carry_word;
        bitpos += tile_bits;
        __syncthreads();
    }
    if (tid == 0) dst[bitpos >> 5] = img[0];
}

// one launch for both forms: the strips of the run form take longer, and run beside the others
__global__ __launch_bounds__(kEncThreads) void k_strip_encode(const unsigned char* __restrict__ base, StripGeom g, const uint32_t* __restrict__ tables,
                                                              const uint32_t* __restrict__ hbits, const unsigned long long* __restrict__ offs,
                                                              unsigned char* __restrict__ out) {
    __shared__ EncodeLds sh;
    if (hbits[blockIdx.x] >> 30 & 1u) encode_strip<true>(sh, base, g, tables, hbits, offs, out);
    else encode_strip<false>(sh, base, g, tables, hbits, offs, out);
}

// frames the device's streams into files: per strip zlib header | block header bits OR literals | Adler-32
struct PackedStrip {
    std::vector<unsigned char> hdr;  // the block header, its last byte partly filled
    uint64_t hbits = 0, payload_bits = 0;
    uint32_t adler = 1;
    bool runs = false;               // coded in the run form
};

struct DevMem {
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    int alloc(size_t n) {
        if (hipMalloc(&p, n) != hipSuccess) { p = nullptr; (void)hipGetLastError(); return fail(MI_ERR_NOMEM, "mi_tiff_write_series_device: hipMalloc(%zu bytes) failed", n); }
        return MI_OK;
    }
};
struct PinMem {
    void* p = nullptr;
    ~PinMem() { if (p) (void)hipHostFree(p); }
    int alloc(size_t n) {
        if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { p = nullptr; (void)hipGetLastError(); return fail(MI_ERR_NOMEM, "mi_tiff_write_series_device: %zu bytes of pinned memory", n); }
        return MI_OK;
    }
};

}  // namespace

extern "C" int mi_tiff_deflate_strip_host(const unsigned char* bytes, size_t n, int bps, size_t rowb, int pred, int runs, unsigned char* out,
                                          size_t cap, size_t* nbytes, int* used_runs) {
    MI_REQUIRE(bytes && out && nbytes, "mi_tiff_deflate_strip_host: null pointer");
    MI_REQUIRE(n > 0 && n < 0xfff00000ull && (bps == 1 || bps == 2 || bps == 4) && rowb > 0 && rowb % (size_t)bps == 0 && n % rowb == 0,
               "mi_tiff_deflate_strip_host: a strip is whole rows of whole samples");
    MI_REQUIRE((pred == 0 || pred == 1) && (runs == 0 || runs == 1) && !(pred && bps == 4), "mi_tiff_deflate_strip_host: pred 0 / 1 (integer samples), runs 0 / 1");
    std::vector<unsigned char> st(bytes, bytes + n);
    if (pred) {
        for (size_t r0 = 0; r0 < n; r0 += rowb) {
            unsigned char* p = st.data() + r0;
            if (bps == 1) for (size_t x = rowb - 1; x > 0; --x) p[x] = (unsigned char)(p[x] - p[x - 1]);
            else for (size_t x = rowb - 2; x > 0; x -= 2) {
                const uint32_t d = ((uint32_t)(p[x] | p[x + 1] << 8) - (uint32_t)(p[x - 2] | p[x - 1] << 8)) & 0xffffu;
                p[x] = (unsigned char)(d & 255);
                p[x + 1] = (unsigned char)(d >> 8);
            }
        }
    }
    uint32_t hist[256] = {0}, rc[kRunWords] = {0};
    uint64_t s1 = 1, s2 = 0;
    for (size_t i = 0; i < n; ++i) {
        hist[st[i]]++;
        s1 += st[i];
        s2 += s1;
        if ((i & 4095) == 4095) { s1 %= 65521; s2 %= 65521; }
    }
    const uint32_t adler = (uint32_t)((s2 % 65521) << 16 | (s1 % 65521));
    if (runs) host_tokens(st.data(), n, rc, [](uint32_t) {});
    BitWriter bw;
    uint32_t table[kSyms];
    uint64_t payload = 0;
    bool with_runs = false;
    strip_code(hist, runs ? rc : nullptr, bw, table, &payload, &with_runs);
    const uint64_t hbits = bw.n;
    bw.b.reserve((size_t)((hbits + payload + 7) / 8) + 1);
    auto sym = [&](uint32_t t) { bw.put(table[t] & 0xffffu, (int)(table[t] >> 16)); };
    if (with_runs) {
        uint32_t scratch[kRunWords] = {0};
        host_tokens(st.data(), n, scratch, [&](uint32_t t) {
            if (t < 256) { sym(t); return; }
            uint32_t ls, nb, val;
            length_code(t - 256, ls, nb, val);
            sym(ls);
            bw.put(val, (int)nb);
            bw.put(0, 1);   // distance 1
        });
    } else {
        for (size_t i = 0; i < n; ++i) sym(st[i]);
    }
    sym(256);
    if (bw.n != hbits + payload) return fail(MI_ERR_INVALID, "mi_tiff_deflate_strip_host: %llu bits written where %llu were counted", (unsigned long long)bw.n,
                                             (unsigned long long)(hbits + payload));
    *nbytes = 2 + bw.b.size() + 4;
    if (used_runs) *used_runs = with_runs ? 1 : 0;
    if (*nbytes > cap) return fail(MI_ERR_NOMEM, "mi_tiff_deflate_strip_host: the stream takes %zu bytes, out holds %zu", *nbytes, cap);
    out[0] = 0x78;
    out[1] = 0x01;
    std::memcpy(out + 2, bw.b.data(), bw.b.size());
    unsigned char* a = out + 2 + bw.b.size();
    a[0] = (unsigned char)(adler >> 24); a[1] = (unsigned char)(adler >> 16); a[2] = (unsigned char)(adler >> 8); a[3] = (unsigned char)adler;
    return MI_OK;
}

extern "C" int mi_tiff_write_series_device(int dev, void* stream, const char* const* paths, int nz, const void* vol, int dtype, int nx, int ny,
                                           int n_threads, int* written) {
    MI_TRY(mi::use_device(dev));
    MI_REQUIRE(paths && vol, "mi_tiff_write_series_device: null pointer");
    MI_REQUIRE(nz >= 0 && nx > 0 && ny > 0 && (dtype == 1 || dtype == 2 || dtype == 4), "mi_tiff_write_series_device: invalid extents or sample type");
    if (written) *written = 0;
    if (nz == 0) return MI_OK;
    hipStream_t s = mi::as_stream(stream);
    StripGeom g;
    const size_t bps = (size_t)(dtype == 4 ? 4 : dtype);
    g.rowb = (size_t)nx * bps;
    g.slice_bytes = g.rowb * (size_t)ny;
    g.ny = (uint32_t)ny;
    g.bps = (uint32_t)bps;
    g.rps = mi::strip_rows_per_strip((size_t)ny, g.rowb);
    g.ns = ((uint32_t)ny + g.rps - 1) / g.rps;
    MI_REQUIRE(g.slice_bytes < 0xfff00000ull, "mi_tiff_write_series_device: a slice of more than 4 GB needs BigTIFF");
    const size_t strip_max = (size_t)g.rps * g.rowb;
    const size_t cap = ((strip_max + strip_max / 32 + 4096) + 15) & ~(size_t)15;   // a strip's stream: at most ~8.01 bits per byte + header
    // slices per batch: ~512 MB of samples at a time
    const int per_batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)nz, ((size_t)512 << 20) / std::max<size_t>(1, g.slice_bytes)));
    const size_t bs = (size_t)per_batch * g.ns;   // strips per batch
    // MI_TIFF_DEVICE_RUNS=0 (read per call): every strip in the literal form
    const char* env_runs = std::getenv("MI_TIFF_DEVICE_RUNS");
    const bool with_runs = !(env_runs && env_runs[0] == '0' && env_runs[1] == 0);
    DevMem d_hist, d_sums, d_runs, d_tab, d_hbits, d_offs, d_out;
    PinMem h_hist, h_sums, h_runs, h_tab, h_hbits, h_offs, h_out;
    MI_TRY(d_hist.alloc(bs * 512 * 4));
    MI_TRY(d_sums.alloc(bs * 32));
    MI_TRY(d_tab.alloc(bs * kSyms * 4));
    MI_TRY(d_hbits.alloc(bs * 4));
    MI_TRY(d_offs.alloc(bs * 8));
    MI_TRY(d_out.alloc(bs * cap));
    MI_TRY(h_hist.alloc(bs * 512 * 4));
    MI_TRY(h_sums.alloc(bs * 32));
    MI_TRY(h_tab.alloc(bs * kSyms * 4));
    MI_TRY(h_hbits.alloc(bs * 4));
    MI_TRY(h_offs.alloc(bs * 8));
    MI_TRY(h_out.alloc(bs * cap));
    if (with_runs) {
        MI_TRY(d_runs.alloc(bs * 2 * kRunWords * 4));
        MI_TRY(h_runs.alloc(bs * 2 * kRunWords * 4));
    }
    const int nt = mi::series_threads(n_threads, std::max(1, (int)bs));
    std::atomic<int> made{0};
    std::vector<PackedStrip> ps(bs);
    std::vector<int> pred_of;
    std::vector<std::vector<unsigned char>> filebuf((size_t)nt);
    for (int z0 = 0; z0 < nz; z0 += per_batch) {
        const int nb = std::min(per_batch, nz - z0);
        const uint32_t nstrip = (uint32_t)nb * g.ns;
        const unsigned char* base = static_cast<const unsigned char*>(vol) + (size_t)z0 * g.slice_bytes;
        // integer samples: the strips are also counted horizontally differenced (TIFF predictor 2); a slice is stored that way when
        // that makes it smaller -- smooth content: entropy coding without string matching then beats deflate level 1, noise: never
        const int both = dtype != 4 ? 1 : 0;
        hipLaunchKernelGGL(k_strip_count, dim3(with_runs ? 2 * nstrip : nstrip), dim3(kEncThreads), 0, s, base, g, both, nstrip,
                           static_cast<uint32_t*>(d_hist.p), static_cast<unsigned long long*>(d_sums.p), static_cast<uint32_t*>(d_runs.p));
        MI_TRY(mi::launch_check("k_strip_count"));
        if (with_runs) MI_HIP(hipMemcpyAsync(h_runs.p, d_runs.p, (size_t)nstrip * 2 * kRunWords * 4, hipMemcpyDeviceToHost, s));
        MI_HIP(hipMemcpyAsync(h_hist.p, d_hist.p, (size_t)nstrip * 512 * 4, hipMemcpyDeviceToHost, s));
        MI_HIP(hipMemcpyAsync(h_sums.p, d_sums.p, (size_t)nstrip * 32, hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        // codes and block headers, a slice per task (its strips share the choice of the predictor; each takes the shorter of its two
        // forms, and the predictor is chosen on those minima)
        pred_of.assign((size_t)nb, 0);
        MI_TRY(run_jobs(nb, std::min(nt, nb), [&](int k, int) -> std::string {
            std::vector<uint32_t> tab2((size_t)g.ns * kSyms);
            std::vector<PackedStrip> alt(g.ns);
            uint64_t bits[2] = {0, 0};
            for (int v = 0; v < (both ? 2 : 1); ++v) {
                for (uint32_t si = 0; si < g.ns; ++si) {
                    const size_t strip = (size_t)k * g.ns + si;
                    PackedStrip& q = v ? alt[si] : ps[strip];
                    BitWriter bw;
                    strip_code(static_cast<const uint32_t*>(h_hist.p) + strip * 512 + (size_t)v * 256,
                               with_runs ? static_cast<const uint32_t*>(h_runs.p) + (strip * 2 + (size_t)v) * kRunWords : nullptr, bw,
                               v ? tab2.data() + (size_t)si * kSyms : static_cast<uint32_t*>(h_tab.p) + strip * kSyms, &q.payload_bits, &q.runs);
                    q.hbits = bw.n;
                    q.hdr.swap(bw.b);
                    const unsigned long long* sm = static_cast<const unsigned long long*>(h_sums.p) + strip * 4 + (size_t)v * 2;
                    const uint64_t n = g.bytes((uint32_t)strip);
                    q.adler = (uint32_t)(((n + sm[1]) % 65521ull) << 16 | ((1ull + sm[0]) % 65521ull));
                    bits[v] += q.hbits + q.payload_bits;
                }
            }
            const bool use_pred = both && bits[1] < bits[0];
            pred_of[(size_t)k] = use_pred ? 1 : 0;
            for (uint32_t si = 0; si < g.ns; ++si) {
                const size_t strip = (size_t)k * g.ns + si;
                if (use_pred) {
                    ps[strip] = std::move(alt[si]);
                    std::memcpy(static_cast<uint32_t*>(h_tab.p) + strip * kSyms, tab2.data() + (size_t)si * kSyms, kSyms * 4);
                }
                const PackedStrip& q = ps[strip];
                static_cast<uint32_t*>(h_hbits.p)[strip] = (uint32_t)q.hbits | (use_pred ? 0x80000000u : 0u) | (q.runs ? 0x40000000u : 0u);
                if ((q.hbits + q.payload_bits + 7) / 8 + 8 > cap) return "a strip's deflate stream does not fit its slot";
            }
            return "";
        }));
        // every stream's length is known: the streams lie one behind the other (16-byte aligned; a kernel writes whole words, up to
        // one past a stream's last byte) and only the bytes in use come back
        unsigned long long* offs = static_cast<unsigned long long*>(h_offs.p);
        size_t used = 0;
        for (uint32_t i = 0; i < nstrip; ++i) {
            offs[i] = used;
            used += ((size_t)((ps[i].hbits + ps[i].payload_bits + 7) / 8) + 4 + 15) & ~(size_t)15;
        }
        MI_HIP(hipMemcpyAsync(d_tab.p, h_tab.p, (size_t)nstrip * kSyms * 4, hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(d_hbits.p, h_hbits.p, (size_t)nstrip * 4, hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(d_offs.p, h_offs.p, (size_t)nstrip * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_strip_encode, dim3(nstrip), dim3(kEncThreads), 0, s, base, g, static_cast<const uint32_t*>(d_tab.p),
                           static_cast<const uint32_t*>(d_hbits.p), static_cast<const unsigned long long*>(d_offs.p),
                           static_cast<unsigned char*>(d_out.p));
        MI_TRY(mi::launch_check("k_strip_encode"));
        MI_HIP(hipMemcpyAsync(h_out.p, d_out.p, used, hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        // files, a slice per task
        MI_TRY(run_jobs(nb, std::min(nt, nb), [&](int k, int t) -> std::string {
            const char* path = paths[z0 + k];
            struct stat st;
            if (stat(path, &st) == 0) return "";   // LsDeconv.m:1120-1132: slices that exist are kept
            std::vector<unsigned char>& file = filebuf[(size_t)t];
            file.clear();
            file.resize(8);
            std::vector<uint32_t> off(g.ns), cnt(g.ns);
            for (uint32_t si = 0; si < g.ns; ++si) {
                const size_t strip = (size_t)k * g.ns + si;
                const PackedStrip& q = ps[strip];
                const size_t nbytes = (size_t)((q.hbits + q.payload_bits + 7) / 8), at = file.size();
                file.resize(at + 2 + nbytes + 4);
                unsigned char* w = file.data() + at;
                w[0] = 0x78;
                w[1] = 0x01;
                std::memcpy(w + 2, static_cast<const unsigned char*>(h_out.p) + offs[strip], nbytes);
                // (the kernel wrote from the word of its first bit on, zeros below that bit; the header's whole bytes are assigned, its
                //  last, partly filled byte is OR-ed onto the first literals)
                for (size_t i = 0; i < q.hdr.size(); ++i) {
                    if (i < q.hbits / 8) w[2 + i] = q.hdr[i];
                    else w[2 + i] |= q.hdr[i];
                }
                w[2 + nbytes + 0] = (unsigned char)(q.adler >> 24);
                w[2 + nbytes + 1] = (unsigned char)(q.adler >> 16);
                w[2 + nbytes + 2] = (unsigned char)(q.adler >> 8);
                w[2 + nbytes + 3] = (unsigned char)q.adler;
                off[si] = (uint32_t)at;
                cnt[si] = (uint32_t)(2 + nbytes + 4);
                if (file.size() & 1) file.push_back(0);
            }
            std::string e = mi::finish_file(path, file, off, cnt, mi::gray_entries(nx, ny, dtype, 1, g.rps, pred_of[(size_t)k] ? 2 : 1));
            if (e.empty()) made.fetch_add(1);
            return e;
        }));
    }
    if (written) *written = made.load();
    return MI_OK;
}
