// The device route of the tree writer (include/mi_pyramid.h): the LZW strips of a z-group's block files encoded where the pyramid
// kernel left the levels, so that only the streams cross to the host.  tiff3d.hip stays host code; the page and directory assembly
// is its write_block (tiffio_internal.h), which both routes hand their strips.
//   k_strip_lzw_encode   one strip per wave (a work-group is one wave).  The encoder is the text of tiff_lzw_enc_dev.h: every lane
//                        runs the serial walk with the same values (byte, prefix and free code come through readfirstlane, so the
//                        state lives in scalar registers).  The lanes part in three places: the rows are gathered from the strided
//                        level through LDS as aligned words (a source begins at any byte); the dictionary, an open-addressing
//                        table of key << 12 | code words in dynamic LDS, is probed 64 consecutive slots at a time with one LDS
//                        read and a ballot; and the codes wait in LDS (kCodeBuf of them) until the lanes place their bits -- a
//                        wave scan of the widths gives every lane the bit offset of its four codes, which it ORs into a bit
//                        image in LDS that leaves as whole words.
//   k_lzw_pack           moves the streams from their slots to the prefix-summed offsets of one buffer, a wave per strip.
//
// What orders the accesses of k_strip_lzw_encode (the three patterns of tiff3d_read.hip, for this kernel's own accesses):
//   - a lane reads what another lane wrote (the staged words of a row; a table slot that the lane owning it filled; the codes lane 0
//     stored; the bit image all lanes ORed into): a __syncthreads() stands between every such write and read.  A work-group is one
//     wave, so the barrier costs no waiting; it is the fence that counts.  fill() begins and ends with it, reset() too,
//     find_or_add() ends with it after a store, place() has one before it reads the codes, one before it reads the image and one
//     before it clears the image.
//   - the walk's state (window, code count, bit carry, words out) is the same value in every lane, kept by every lane in program
//     order.  This rests on the work-group being ONE wave (__launch_bounds__(64), launched with 64 threads).
//   - global memory: a wave reads only its strip's rows (no word without a byte of the row) and stores only into its strip's slot,
//     bytes [0, cap); no wave reads what another stored.  No work-group waits for another, and every loop is bounded by the strip's
//     byte count, the table's slot count or a constant.
// No inline assembly; every store is a vector store from plain C++.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "mi_internal.h"
#include "mi_pyramid.h"
#include "tiff_lzw_enc_dev.h"
#include "tiffio_internal.h"

namespace {

using mi::fail;
using mi::slot;
using namespace mi_lzw_enc;

// ------------------------------------------------------------------------------------------------------------------ kernels
constexpr uint32_t kStageWords = 64;                       // raw bytes in LDS: up to 256 of a row at a time (+ one word: a row begins at any byte)
constexpr uint32_t kCodeBuf = 256;                         // codes between two placings: four per lane
constexpr uint32_t kImageWords = kCodeBuf * 12 / 32 + 2;   // their bits at most, the carried word and the word a code may run into
constexpr uint32_t kFixedWords = (kStageWords + 1 + 3) / 4 * 4 + kCodeBuf + (kImageWords + 3) / 4 * 4;   // LDS words before the table

struct EncJob {
    unsigned long long src;        // device address of the strip's first byte (any byte)
    long long stride;              // bytes from a row to the next
    unsigned long long slot_off;   // of its slot in the slots' buffer, a multiple of 4
    uint32_t rows, rowb;           // rows of rowb bytes
    uint32_t cap, pad;             // bytes of the slot
};

struct WaveEncCtx {
    uint32_t* stage;    // LDS: aligned words of the source that hold the window's bytes
    uint32_t* codes;    // LDS: code | width << 16
    uint32_t* image;    // LDS: the bits of the buffered codes, the stream's first bit in the top bit of word 0
    uint32_t* table;    // LDS: slots
    unsigned char* out; // the strip's slot
    const unsigned char* src;
    long long stride;
    uint32_t rowb, cap, slots, lane;
    uint32_t win_base, win_len, win_shift;   // the window: strip bytes [win_base, win_base + win_len) begin at byte win_shift of stage
    uint32_t ncodes, carry, wout;            // buffered codes; bits of image[0] already taken; words stored so far
    uint64_t length;                         // of the stream in bytes, once place(true) has run

    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

    // the window moves to strip byte i: the rest of its row, 256 bytes at most
    __device__ __forceinline__ void fill(uint32_t i) {
        __syncthreads();
        const uint32_t r = i / rowb, c = i - r * rowb;
        const unsigned long long a = (unsigned long long)(uintptr_t)src + (unsigned long long)((long long)r * stride) + c;
        const uint32_t shift = (uint32_t)(a & 3ull), len = min(rowb - c, 4u * kStageWords);
        const uint32_t* words = reinterpret_cast<const uint32_t*>((uintptr_t)(a - shift));
        const uint32_t nw = (shift + len + 3u) / 4u;   // <= kStageWords + 1; each holds a byte of the row
        for (uint32_t k = lane; k < nw; k += 64) stage[k] = words[k];
        __syncthreads();
        win_base = i;
        win_len = len;
        win_shift = shift;
    }
    __device__ __forceinline__ uint32_t byte(uint32_t i) {
        if (i - win_base >= win_len) fill(i);
        const uint32_t k = win_shift + (i - win_base);
        return uni((stage[k >> 2] >> (8u * (k & 3u))) & 255u);
    }
    __device__ __forceinline__ void reset() {
        __syncthreads();
        for (uint32_t k = lane; k < slots; k += 64) table[k] = kEncEmpty;
        __syncthreads();
    }
    // linear probing, 64 slots a step: the first of (a slot with the key, an empty slot) from the hash on decides
    __device__ __forceinline__ uint32_t find_or_add(uint32_t key, uint32_t code) {
        const uint32_t h = table_hash(key, slots);
        for (uint32_t step = 0; step < slots; step += 64) {
            const uint32_t at = (h + step + lane) & (slots - 1u);
            const uint32_t e = table[at];
            const unsigned long long hit = __ballot(e >> 12 == key), emp = __ballot(e == kEncEmpty);
            const uint32_t fh = hit ? (uint32_t)__builtin_ctzll(hit) : 64u, fe = emp ? (uint32_t)__builtin_ctzll(emp) : 64u;
            if (fh < fe) return (uint32_t)__builtin_amdgcn_readlane((int)e, (int)fh) & 0xfffu;
            if (fe < 64u) {
                if (lane == fe) table[at] = key << 12 | code;
                __syncthreads();
                return kEncNone;
            }
        }
        return kEncNone;   // (not reached: the table is at most half full)
    }
    __device__ __forceinline__ void put(uint32_t code, uint32_t width) {
        if (lane == 0) codes[ncodes] = code | width << 16;
        ncodes += 1;
        if (ncodes == kCodeBuf) place(false);
    }
    // word w of the stream (the first byte in its top byte) into the slot: whole where it fits, else the bytes that do
    __device__ __forceinline__ void store_word(uint32_t w, uint32_t v) {
        const unsigned long long b = 4ull * w;
        if (b + 4u <= cap) {
            reinterpret_cast<uint32_t*>(out)[w] = __builtin_bswap32(v);
        } else {
            for (uint32_t k = 0; k < 4; ++k)
                if (b + k < cap) out[b + k] = (unsigned char)(v >> (24u - 8u * k));
        }
    }
    // the buffered codes become bits: lane l places codes 4l .. 4l + 3; the whole words leave, the rest is carried
    __device__ __forceinline__ void place(bool last) {
        __syncthreads();
        uint32_t c[4], w[4], sum = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t k = 4u * lane + q;
            const uint32_t v = k < ncodes ? codes[k] : 0u;
            c[q] = v & 0xffffu;
            w[q] = v >> 16;
            sum += w[q];
        }
        uint32_t inc = sum;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
            if (lane >= d) inc += t;
        }
        const uint32_t bits = carry + (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);   // <= 31 + 12 kCodeBuf
        uint32_t off = carry + inc - sum;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (w[q]) {
                const unsigned long long v = (unsigned long long)c[q] << (64u - w[q] - (off & 31u));
                atomicOr(&image[off >> 5], (uint32_t)(v >> 32));
                if ((uint32_t)v) atomicOr(&image[(off >> 5) + 1u], (uint32_t)v);
                off += w[q];
            }
        }
        __syncthreads();
        const uint32_t nw = last ? (bits + 31u) / 32u : bits / 32u;   // < kImageWords
        for (uint32_t k = lane; k < nw; k += 64) store_word(wout + k, image[k]);
        const uint32_t rem = last ? 0u : image[bits >> 5];
        __syncthreads();
        for (uint32_t k = lane; k < kImageWords; k += 64) image[k] = k == 0 ? rem : 0u;
        if (last) length = 4ull * wout + (bits + 7u) / 8u;
        wout += bits / 32u;
        carry = bits & 31u;
        ncodes = 0;
    }
};

__global__ __launch_bounds__(64) void k_strip_lzw_encode(const EncJob* __restrict__ jobs, const uint32_t* __restrict__ index, unsigned char* slots_base,
                                                         uint32_t* __restrict__ lengths, int32_t* __restrict__ status, uint32_t tslots) {
    extern __shared__ uint32_t lds[];   // [stage][codes][image][table: tslots]
    const uint32_t i = index[blockIdx.x];
    const EncJob j = jobs[i];
    uint32_t* stage = lds;
    uint32_t* codes = stage + (kStageWords + 1 + 3) / 4 * 4;
    uint32_t* image = codes + kCodeBuf;
    uint32_t* table = lds + kFixedWords;
    for (uint32_t k = threadIdx.x; k < kImageWords; k += 64) image[k] = 0;
    WaveEncCtx ctx;
    ctx.stage = stage;
    ctx.codes = codes;
    ctx.image = image;
    ctx.table = table;
    ctx.out = slots_base + j.slot_off;
    ctx.src = reinterpret_cast<const unsigned char*>((uintptr_t)j.src);
    ctx.stride = j.stride;
    ctx.rowb = ctx.uni(j.rowb);
    ctx.cap = ctx.uni(j.cap);
    ctx.slots = tslots;
    ctx.lane = threadIdx.x;
    ctx.win_base = 0;
    ctx.win_len = 0;
    ctx.win_shift = 0;
    ctx.ncodes = 0;
    ctx.carry = 0;
    ctx.wout = 0;
    ctx.length = 0;
    const uint32_t n = ctx.uni(j.rows) * ctx.rowb;
    lzw_encode_strip(ctx, n);
    ctx.place(true);
    if (threadIdx.x == 0) {
        lengths[i] = (uint32_t)ctx.length;
        status[i] = ctx.length > ctx.cap ? kEncOverflow : kEncOk;
    }
}

// the streams to their places in the packed buffer: whole words, the bytes of the last word behind the stream zero
__global__ __launch_bounds__(256) void k_lzw_pack(const EncJob* __restrict__ jobs, const unsigned char* __restrict__ slots_base,
                                                  const uint32_t* __restrict__ lengths, const unsigned long long* __restrict__ pack_off,
                                                  unsigned char* __restrict__ packed, uint32_t n) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= n) return;
    const EncJob j = jobs[i];
    const uint32_t len = min(lengths[i], j.cap), nw = (len + 3u) / 4u;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(slots_base + j.slot_off);
    uint32_t* dst = reinterpret_cast<uint32_t*>(packed + pack_off[i]);
    for (uint32_t w = lane; w < nw; w += 64) {
        uint32_t v = 0;
        if (4u * w + 4u <= len) {
            v = src[w];
        } else {   // the slot may end inside this word
            const unsigned char* p = reinterpret_cast<const unsigned char*>(src + w);
            for (uint32_t k = 0; 4u * w + k < len; ++k) v |= (uint32_t)p[k] << (8u * k);
        }
        dst[w] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ a batch
constexpr uint32_t kPackAlign = 4;
constexpr uint32_t kClassBytes[2] = {512, 2048};   // strips of at most 512 / 2048 bytes / longer: tables of 1024 / 4096 / 8192 slots

mi::ScratchPool g_scratch;   // this writer's own
std::atomic<long long> g_batches{0};

inline size_t pack_slot(size_t n) { return (n + kPackAlign - 1) & ~(size_t)(kPackAlign - 1); }

size_t enc_lds_bytes(uint32_t tslots) { return 4 * ((size_t)kFixedWords + tslots); }

// Strips [0, n) of `jobs` (slot offsets and caps set) are encoded into d_slots and packed: pinned memory h_bytes of the scratch
// receives the streams, stream k at pack_off[k] (a multiple of kPackAlign, in job order); lengths / status per strip.  One batch:
// the caller bounds it.
int encode_batch(mi::DeviceScratch& sc, hipStream_t s, const std::vector<EncJob>& jobs, unsigned char* d_slots_user, size_t slots_bytes,
                 std::vector<unsigned long long>& pack_off, uint32_t* lengths, int32_t* status, size_t* packed_bytes) {
    const size_t n = jobs.size();
    *packed_bytes = 0;
    pack_off.assign(n, 0);
    if (n == 0) return MI_OK;
    // [EncJob x n | index x n | lengths x n | status x n | pack_off x n], the same layout on both sides
    const size_t index_at = slot(n * sizeof(EncJob)), len_at = index_at + slot(n * 4), status_at = len_at + slot(n * 4),
                 off_at = status_at + slot(n * 4), jobs_bytes = off_at + slot(n * 8);
    MI_TRY(sc.h_jobs.reserve(jobs_bytes));
    MI_TRY(sc.grow(sc.d_jobs, jobs_bytes));
    // [slots | packed]: the streams are no longer than their slots
    const size_t own_slots = d_slots_user ? 0 : slot(slots_bytes), packed_cap = slot(slots_bytes) + kPackAlign * n;
    MI_TRY(sc.grow(sc.d_bytes, own_slots + packed_cap));
    unsigned char* hj = sc.h_jobs.as<unsigned char>();
    unsigned char* dj = sc.d_jobs.as<unsigned char>();
    unsigned char* d_slots = d_slots_user ? d_slots_user : sc.d_bytes.as<unsigned char>();
    unsigned char* d_packed = sc.d_bytes.as<unsigned char>() + own_slots;
    std::memcpy(hj, jobs.data(), n * sizeof(EncJob));
    uint32_t* index = reinterpret_cast<uint32_t*>(hj + index_at);
    size_t count[3] = {0, 0, 0}, first[3];
    uint32_t longest = 0;
    auto cls = [](const EncJob& j) {
        const uint64_t b = (uint64_t)j.rows * j.rowb;
        return b <= kClassBytes[0] ? 0 : b <= kClassBytes[1] ? 1 : 2;
    };
    for (const EncJob& j : jobs) {
        count[cls(j)] += 1;
        longest = std::max(longest, j.rows * j.rowb);
    }
    first[0] = 0;
    first[1] = count[0];
    first[2] = count[0] + count[1];
    {
        size_t at[3] = {first[0], first[1], first[2]};
        for (size_t k = 0; k < n; ++k) index[at[cls(jobs[k])]++] = (uint32_t)k;
    }
    MI_HIP(hipMemcpyAsync(dj, hj, len_at, hipMemcpyHostToDevice, s));
    uint32_t* d_len = reinterpret_cast<uint32_t*>(dj + len_at);
    int32_t* d_status = reinterpret_cast<int32_t*>(dj + status_at);
    for (int c = 0; c < 3; ++c) {
        if (count[c] == 0) continue;
        const uint32_t tslots = table_slots(c < 2 ? kClassBytes[c] : longest);
        hipLaunchKernelGGL(k_strip_lzw_encode, dim3((uint32_t)count[c]), dim3(64), enc_lds_bytes(tslots), s, reinterpret_cast<const EncJob*>(dj),
                           reinterpret_cast<const uint32_t*>(dj + index_at) + first[c], d_slots, d_len, d_status, tslots);
        MI_TRY(mi::launch_check("k_strip_lzw_encode"));
    }
    MI_HIP(hipMemcpyAsync(hj + len_at, dj + len_at, off_at - len_at, hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    const uint32_t* h_len = reinterpret_cast<const uint32_t*>(hj + len_at);
    const int32_t* h_status = reinterpret_cast<const int32_t*>(hj + status_at);
    unsigned long long* h_off = reinterpret_cast<unsigned long long*>(hj + off_at);
    size_t total = 0;
    for (size_t k = 0; k < n; ++k) {
        lengths[k] = h_len[k];
        status[k] = h_status[k];
        h_off[k] = pack_off[k] = total;
        total += pack_slot(std::min<uint32_t>(h_len[k], jobs[k].cap));
    }
    MI_HIP(hipMemcpyAsync(dj + off_at, hj + off_at, n * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_lzw_pack, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const EncJob*>(dj), d_slots, d_len,
                       reinterpret_cast<const unsigned long long*>(dj + off_at), d_packed, (uint32_t)n);
    MI_TRY(mi::launch_check("k_lzw_pack"));
    MI_TRY(sc.h_bytes.reserve(total));
    if (total) MI_HIP(hipMemcpyAsync(sc.h_bytes.as<unsigned char>(), d_packed, total, hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    *packed_bytes = total;
    g_batches += 1;
    return MI_OK;
}

// a batch is bounded as the tree reader bounds its own: at most 1 GB of raw rows and 2^20 strips
constexpr size_t kMaxRaw = (size_t)1 << 30, kMaxStrips = (size_t)1 << 20;
constexpr uint64_t kMaxStrip = (uint64_t)1 << 30;   // a strip's slot bound fits 32 bits

}  // namespace

namespace mi {
void tiff3d_lzw_enc_drop_scratch(int dev) { g_scratch.drop(dev); }
}  // namespace mi

extern "C" int64_t mi_tiff_lzw_encode_device_batches(void) { return (int64_t)g_batches.load(); }

extern "C" int mi_tiff_lzw_encode_strips_device(int dev, void* stream, int64_t n, const void* const* src, const int32_t* rows, const int32_t* row_bytes,
                                                const int64_t* row_stride, const int64_t* slot_off, const int64_t* slot_cap, void* d_slots,
                                                int64_t d_slots_bytes, void* out, int64_t out_cap, int64_t* out_off, int64_t* lengths, int32_t* status,
                                                int64_t* out_bytes) {
    MI_TRY(mi::use_device(dev));
    MI_REQUIRE(n >= 0 && (n == 0 || (src && rows && row_bytes && row_stride && out_off && lengths && status)) && out_bytes && (out || out_cap == 0) &&
                   out_cap >= 0,
               "mi_tiff_lzw_encode_strips_device: null pointer");
    MI_REQUIRE((slot_off != nullptr) == (d_slots != nullptr) && (!slot_off || slot_cap),
               "mi_tiff_lzw_encode_strips_device: slot offsets, slot sizes and the slots' buffer come together");
    *out_bytes = 0;
    hipStream_t s = mi::as_stream(stream);
    const std::shared_ptr<mi::DeviceScratch> sc = g_scratch.get(dev);
    std::lock_guard<std::mutex> hold(sc->mu);
    std::vector<EncJob> jobs;
    std::vector<unsigned long long> pack_off;
    std::vector<uint32_t> len32;
    bool overflow = false;
    int64_t first_over = -1;
    size_t total = 0;
    for (int64_t b0 = 0; b0 < n;) {
        jobs.clear();
        size_t raw = 0, slots_bytes = 0;
        int64_t b1 = b0;
        for (; b1 < n; ++b1) {
            MI_REQUIRE(src[b1] && rows[b1] > 0 && row_bytes[b1] > 0 && (uint64_t)rows[b1] * (uint64_t)row_bytes[b1] <= kMaxStrip,
                       "mi_tiff_lzw_encode_strips_device: strip %lld of %d rows of %d bytes", (long long)b1, rows[b1], row_bytes[b1]);
            const uint64_t bytes = (uint64_t)rows[b1] * (uint64_t)row_bytes[b1];
            if (b1 > b0 && (raw + bytes > kMaxRaw || (size_t)(b1 - b0) >= kMaxStrips)) break;
            EncJob j;
            j.src = (unsigned long long)(uintptr_t)src[b1];
            j.stride = row_stride[b1];
            j.rows = (uint32_t)rows[b1];
            j.rowb = (uint32_t)row_bytes[b1];
            j.pad = 0;
            if (slot_off) {
                MI_REQUIRE(slot_off[b1] >= 0 && slot_off[b1] % 4 == 0 && slot_cap[b1] >= 0 && slot_cap[b1] <= 0xffffffffll &&
                               slot_off[b1] + slot_cap[b1] <= d_slots_bytes,
                           "mi_tiff_lzw_encode_strips_device: strip %lld: a slot of %lld bytes at %lld (a multiple of 4, inside the %lld bytes of slots)",
                           (long long)b1, (long long)slot_cap[b1], (long long)slot_off[b1], (long long)d_slots_bytes);
                j.slot_off = (unsigned long long)slot_off[b1];
                j.cap = (uint32_t)slot_cap[b1];
                slots_bytes += (size_t)slot_cap[b1];
            } else {
                j.slot_off = slots_bytes;
                j.cap = (uint32_t)slot_bound(bytes);
                slots_bytes += slot(j.cap);
            }
            raw += bytes;
            jobs.push_back(j);
        }
        len32.resize(jobs.size());
        size_t packed = 0;
        MI_TRY(encode_batch(*sc, s, jobs, static_cast<unsigned char*>(d_slots), slots_bytes, pack_off, len32.data(), status + b0, &packed));
        MI_REQUIRE(total + packed <= (size_t)out_cap, "mi_tiff_lzw_encode_strips_device: the streams need more than the %lld bytes of `out`",
                   (long long)out_cap);
        if (packed) {   // pinned -> the caller's pages, on the tree's pool: one thread copies (and first touches) a gigabyte in a tenth of a second
            constexpr size_t kChunk = (size_t)4 << 20;
            const int chunks = (int)((packed + kChunk - 1) / kChunk);
            unsigned char* to = static_cast<unsigned char*>(out) + total;
            const unsigned char* from = sc->h_bytes.as<unsigned char>();
            MI_TRY(mi::run_jobs(chunks, std::max(1, std::min(mi::tree_pool_threads(0), chunks)), [&](int k, int) -> std::string {
                const size_t at = (size_t)k * kChunk;
                std::memcpy(to + at, from + at, std::min(kChunk, packed - at));
                return std::string();
            }));
        }
        for (size_t k = 0; k < jobs.size(); ++k) {
            out_off[b0 + (int64_t)k] = (int64_t)(total + pack_off[k]);
            lengths[b0 + (int64_t)k] = (int64_t)len32[k];
            if (status[b0 + (int64_t)k] != kEncOk && !overflow) {
                overflow = true;
                first_over = b0 + (int64_t)k;
            }
        }
        total += packed;
        b0 = b1;
    }
    *out_bytes = (int64_t)total;
    if (overflow)
        return fail(MI_ERR_NOMEM, "mi_tiff_lzw_encode_strips_device: LZW output larger than its bound (strip %lld)", (long long)first_over);
    return MI_OK;
}

extern "C" int mi_tiff3d_write_blocks_device(int dev, void* stream, int n, const char* const* paths, const void* const* first, const int64_t* strides,
                                             const int* dims, const int* page0, const int* page_total, int bytes, int compression, int rows_per_strip,
                                             int bigtiff, int n_threads) {
    MI_TRY(mi::use_device(dev));
    MI_REQUIRE(n >= 0 && (n == 0 || (paths && first && strides && dims && page0 && page_total)), "mi_tiff3d_write_blocks_device: null pointer");
    MI_REQUIRE(bytes == 1 || bytes == 2, "mi_tiff3d_write_blocks_device: %d bytes per sample (1 or 2)", bytes);
    MI_REQUIRE(compression == 1, "mi_tiff3d_write_blocks_device: compression %d (the device route writes LZW, 1)", compression);
    MI_REQUIRE(rows_per_strip >= 1, "mi_tiff3d_write_blocks_device: %d rows per strip", rows_per_strip);
    std::vector<mi::Tiff3dBlock> blocks;
    int64_t nstrips = 0;
    MI_TRY(mi::tiff3d_parse_blocks("mi_tiff3d_write_blocks_device", n, paths, first, strides, dims, page0, page_total, bytes, rows_per_strip, blocks,
                                   &nstrips));
    for (int b = 0; b < n; ++b)
        MI_REQUIRE((uint64_t)std::min(rows_per_strip, blocks[b].h) * (uint64_t)blocks[b].w * (uint64_t)bytes <= kMaxStrip,
                   "mi_tiff3d_write_blocks_device: a strip of block %d passes 1 GiB", b);
    hipStream_t s = mi::as_stream(stream);
    const std::shared_ptr<mi::DeviceScratch> sc = g_scratch.get(dev);
    std::lock_guard<std::mutex> hold(sc->mu);
    // 1) every strip of every page of every block, in the host route's order, encoded in batches; the streams gather in `all`
    std::vector<unsigned char> all;
    std::vector<uint64_t> at((size_t)nstrips), len((size_t)nstrips);
    std::vector<EncJob> jobs;
    std::vector<unsigned long long> pack_off;
    std::vector<uint32_t> len32;
    std::vector<int32_t> status;
    size_t raw = 0, slots_bytes = 0;
    int64_t batch0 = 0, done = 0;
    bool overflow = false;
    auto flush = [&]() -> int {
        if (jobs.empty()) return MI_OK;
        len32.resize(jobs.size());
        status.resize(jobs.size());
        size_t packed = 0;
        MI_TRY(encode_batch(*sc, s, jobs, nullptr, slots_bytes, pack_off, len32.data(), status.data(), &packed));
        const size_t base = all.size();
        all.insert(all.end(), sc->h_bytes.as<unsigned char>(), sc->h_bytes.as<unsigned char>() + packed);
        for (size_t k = 0; k < jobs.size(); ++k) {
            at[(size_t)batch0 + k] = base + pack_off[k];
            len[(size_t)batch0 + k] = len32[k];
            if (status[k] != kEncOk) overflow = true;
        }
        batch0 = done;
        jobs.clear();
        raw = slots_bytes = 0;
        return MI_OK;
    };
    for (int b = 0; b < n; ++b) {
        const mi::Tiff3dBlock& B = blocks[b];
        const uint64_t rowb = (uint64_t)B.w * (uint64_t)bytes;
        for (int p = 0; p < B.pages; ++p)
            for (int r0 = 0; r0 < B.h; r0 += rows_per_strip) {
                const int nr = std::min(rows_per_strip, B.h - r0);
                const uint64_t sb = rowb * (uint64_t)nr;
                if (!jobs.empty() && (raw + sb > kMaxRaw || jobs.size() >= kMaxStrips)) MI_TRY(flush());
                EncJob j;
                j.src = (unsigned long long)(uintptr_t)(B.first + ((int64_t)p * B.sp + (int64_t)r0 * B.sr) * bytes);
                j.stride = B.sr * bytes;
                j.rows = (uint32_t)nr;
                j.rowb = (uint32_t)rowb;
                j.slot_off = slots_bytes;
                j.cap = (uint32_t)slot_bound(sb);
                j.pad = 0;
                slots_bytes += slot(j.cap);
                raw += sb;
                jobs.push_back(j);
                ++done;
            }
    }
    MI_TRY(flush());
    if (overflow) return fail(MI_ERR_NOMEM, "mi_tiff3d_write_blocks: LZW output larger than its bound");
    // 2) each file gets its pages appended: the host route's assembly
    std::vector<mi::StripRef> refs((size_t)nstrips);
    for (int64_t k = 0; k < nstrips; ++k) refs[(size_t)k] = {all.data() + at[(size_t)k], (size_t)len[(size_t)k]};
    return mi::tiff3d_write_files(blocks, refs.data(), bytes, 1, rows_per_strip, bigtiff, mi::tree_pool_threads(n_threads));
}
