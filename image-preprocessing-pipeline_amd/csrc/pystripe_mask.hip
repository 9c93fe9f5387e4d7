// The foreground mask of filter_streaks (get_img_mask, pystripe/core.py:475-489) on batches of equally shaped 2-D tiles, as
// include/mi_tile_mask.h states it: threshold, close, open with k x k boxes, removal of the background regions that hold a corner.
// Everything runs on the caller's stream; per group of at most max_batch tiles:
//
//   threshold  one thread per sample -> bytes 0 / 1 in the caller's mask buffer.
//   morphology four operators (dilate, erode | erode, dilate), each an x pass and a y pass; an operator with k = 1 is left out.  On a
//              binary image a dilation is "ones in the window > 0" and an erosion "ones in the window == samples of the window inside
//              the tile", so both are one count and no pass looks at k samples:
//     x pass   one work-group per row, in place.  The exclusive prefix count of the row goes to global scratch, 256 samples per
//              step: the count inside a wave is a ballot and a popcount, the four wave totals meet in LDS, the carry stays in a
//              register.  After a barrier every sample reads the two ends of its window from the prefix.  Nothing is sized by nx.
//     y pass   one thread per column walks the rows with a running count: + the row that enters the window, - the row that left.
//              Lanes are adjacent columns, so every load and store is one run of 64 bytes.  The walk starts r rows above the tile
//              (r = k - 1 - k / 2, limited to ny) to collect the first window, so a column costs ny + min(r, ny) steps, never k
//              per sample.  The loads of kAhead steps are issued together; their addresses do not depend on the count.
//   fill       on bit-packed maps, 64 samples to a word, rows padded to whole words with zeros: inv = !m and reached, seeded with
//              the corners that are 1 in inv.  A round is a row sweep (one thread per row, left to right and back: inside a word
//              the carry of an addition runs through a run of ones, between words one bit is handed on), a column sweep (one
//              thread per word column, down and up: reached |= inv & reached of the row before) and, for connectivity 8, one step
//              to the eight neighbours.  Words are updated in place; a word read while a neighbour writes it is either the old or
//              the new one, and both hold only samples that are connected to a corner, so the fixed point is the same.  Every kernel
//              of a round sets that round's flag when it changes a word.  Rounds are separate launches, kRoundsPerBatch of them
//              (kFirstRounds at first) between two reads of the flags by the host; the first round that changed nothing ends the
//              fill.  No kernel waits for another work-group.
//   finish     mask = !reached (reached is a subset of inv = !m), masked_out = mask ? in : 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "mi_internal.h"
#include "mi_pystripe.h"
#include "mi_tile_mask.h"

namespace mi {
namespace {

using i64 = long long;
using u64 = unsigned long long;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRoundsPerBatch = 4;   // fill rounds between two reads of the flags; the first batch has kFirstRounds
constexpr int kFirstRounds = 2;
constexpr int kAhead = 16;           // steps of a serial walk whose loads are issued together
constexpr int kMaxChunk = 32768;   // tiles of one launch (grid y)
constexpr int kMaxExtent = 1 << 30;

size_t dtype_bytes(int dt) { return dt == MI_PS_U8 ? 1 : dt == MI_PS_U16 ? 2 : 4; }
bool dtype_ok(int dt) { return dt == MI_PS_U8 || dt == MI_PS_U16 || dt == MI_PS_F32; }

// ---- threshold ------------------------------------------------------------------------------------------------------------------

template <class T> __device__ inline bool above(T v, double thr, float, int) { return (double)v > thr; }
template <> __device__ inline bool above<float>(float v, double, float thr, int log_domain) {
    return (log_domain ? log1pf(v) : v) > thr;   // NaN compares false
}

template <class T>
__global__ void __launch_bounds__(kThreads) threshold_kernel(const T* __restrict__ in, uint8_t* __restrict__ m, i64 total, double thr,
                                                             float thr32, int log_domain) {
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < total; i += (i64)gridDim.x * kThreads)
        m[i] = above<T>(in[i], thr, thr32, log_domain) ? 1 : 0;
}

// ---- morphology -----------------------------------------------------------------------------------------------------------------

// window of sample i: [i - a, i + r], cut to [0, n - 1]; a and r are limited to n by the host, so i + r cannot overflow
template <bool kDilate>
__global__ void __launch_bounds__(kThreads) morph_x_kernel(uint8_t* __restrict__ img, int* __restrict__ prefix, int ny, int nx, int a, int r) {
    const i64 row = (i64)blockIdx.y * ny + blockIdx.x;
    uint8_t* line = img + row * nx;
    int* P = prefix + row * ((i64)nx + 1);   // P[i] = ones in [0, i)
    __shared__ int wave_sum[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nx; base += kThreads) {   // nx <= 2^30: base + kThreads does not overflow
        const int x = base + threadIdx.x;
        const bool v = x < nx && line[x] != 0;
        const u64 b = __ballot(v);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wave_sum[wave] = __popcll(b);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            off += w < wave ? wave_sum[w] : 0;
            tot += wave_sum[w];
        }
        if (x < nx) P[x] = carry + off + before;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) P[nx] = carry;
    __syncthreads();   // the prefix of this row is written and read by this work-group alone
    for (int base = 0; base < nx; base += kThreads) {
        const int x = base + threadIdx.x;
        if (x < nx) {
            const int lo = x - a > 0 ? x - a : 0, hi = x + r < nx - 1 ? x + r : nx - 1;
            const int cnt = P[hi + 1] - P[lo];
            line[x] = (kDilate ? cnt > 0 : cnt == hi - lo + 1) ? 1 : 0;
        }
    }
}

template <bool kDilate>
__global__ void __launch_bounds__(64) morph_y_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int ny, int nx, int a, int r) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= nx) return;   // no barrier below
    const uint8_t* src = in + (i64)blockIdx.y * ny * nx + x;
    uint8_t* dst = out + (i64)blockIdx.y * ny * nx + x;
    int cnt = 0;
    for (int y0 = -r; y0 < ny; y0 += kAhead) {   // r <= ny <= 2^30
        int lead[kAhead], trail[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int y = y0 + j, li = y + r, ti = y - a - 1;   // li >= 0; ti < y
            lead[j] = (y < ny && li < ny) ? src[(i64)li * nx] : 0;
            trail[j] = (y < ny && ti >= 0) ? src[(i64)ti * nx] : 0;
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int y = y0 + j;
            if (y < ny) {
                cnt += lead[j] - trail[j];
                if (y >= 0) {
                    const int lo = y - a > 0 ? y - a : 0, hi = y + r < ny - 1 ? y + r : ny - 1;
                    dst[(i64)y * nx] = (kDilate ? cnt > 0 : cnt == hi - lo + 1) ? 1 : 0;
                }
            }
        }
    }
}

// ---- fill -----------------------------------------------------------------------------------------------------------------------

// inv = !m packed 64 samples to a word (bit j of word w of a row: sample 64 w + j; bits beyond nx are 0), reached = corners & inv.
// One wave per word; words: ny * W per tile.
__global__ void __launch_bounds__(kThreads) pack_kernel(const uint8_t* __restrict__ m, u64* __restrict__ inv, u64* __restrict__ reached, int ny,
                                                        int nx, int W) {
    const i64 words = (i64)ny * W;
    const i64 gw = (i64)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (gw >= words) return;   // whole waves leave together; no barrier below
    const int lane = threadIdx.x & 63;
    const int y = (int)(gw / W), w = (int)(gw % W);
    const i64 x = (i64)w * 64 + lane;
    const bool bit = x < nx && m[(i64)blockIdx.y * ny * nx + (i64)y * nx + x] == 0;
    const u64 b = __ballot(bit);
    if (lane == 0) {
        u64 corner = 0;
        if (y == 0 || y == ny - 1) {
            if (w == 0) corner |= 1ull;
            if (w == (nx - 1) / 64) corner |= 1ull << ((nx - 1) % 64);
        }
        inv[(i64)blockIdx.y * words + gw] = b;
        reached[(i64)blockIdx.y * words + gw] = b & corner;
    }
}

// seeds S (a subset of M) spread towards higher bits through the runs of ones of M; carry: the bit handed over from the word before / to the next
__device__ inline u64 flood_up(u64 M, u64 S, unsigned& carry) {
    S |= (u64)carry & M & 1ull;
    const u64 R = (M & ~(M + S)) | S;   // the addition's carry runs from the lowest seed of a run to the run's end
    carry = (unsigned)(R >> 63);
    return R;
}

__global__ void __launch_bounds__(64) sweep_rows_kernel(const u64* __restrict__ inv, u64* __restrict__ reached, i64 rows, int W, int* __restrict__ flag) {
    const i64 row = (i64)blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const u64* M = inv + row * W;
    u64* R = reached + row * W;
    bool changed = false;
    unsigned carry = 0;
    for (int w = 0; w < W; ++w) {
        const u64 s = R[w], f = flood_up(M[w], s, carry);
        if (f != s) {
            R[w] = f;
            changed = true;
        }
    }
    carry = 0;
    for (int w = W - 1; w >= 0; --w) {
        const u64 s = R[w], f = __brevll(flood_up(__brevll(M[w]), __brevll(s), carry));
        if (f != s) {
            R[w] = f;
            changed = true;
        }
    }
    if (changed) *flag = 1;
}

__global__ void __launch_bounds__(64) sweep_cols_kernel(const u64* __restrict__ inv, u64* __restrict__ reached, int ny, int W, int* __restrict__ flag) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= W) return;
    const u64* M = inv + (i64)blockIdx.y * ny * W + w;
    u64* R = reached + (i64)blockIdx.y * ny * W + w;
    bool changed = false;
    u64 prev = 0;
    for (int y0 = 0; y0 < ny; y0 += kAhead) {
        u64 mv[kAhead], sv[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const bool ok = y0 + j < ny;
            mv[j] = ok ? M[(i64)(y0 + j) * W] : 0;
            sv[j] = ok ? R[(i64)(y0 + j) * W] : 0;
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            if (y0 + j < ny) {
                prev = sv[j] | (mv[j] & prev);
                if (prev != sv[j]) {
                    R[(i64)(y0 + j) * W] = prev;
                    changed = true;
                }
            }
        }
    }
    prev = 0;
    for (int y0 = ny - 1; y0 >= 0; y0 -= kAhead) {
        u64 mv[kAhead], sv[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const bool ok = y0 - j >= 0;
            mv[j] = ok ? M[(i64)(y0 - j) * W] : 0;
            sv[j] = ok ? R[(i64)(y0 - j) * W] : 0;
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            if (y0 - j >= 0) {
                prev = sv[j] | (mv[j] & prev);
                if (prev != sv[j]) {
                    R[(i64)(y0 - j) * W] = prev;
                    changed = true;
                }
            }
        }
    }
    if (changed) *flag = 1;
}

// connectivity 8: one step to the eight neighbours, restricted to inv.  One thread per word.
// reached carries no __restrict__ here: a thread reads its neighbours' words while their owners may store to them
__global__ void __launch_bounds__(kThreads) spread8_kernel(const u64* __restrict__ inv, u64* reached, int ny, int W, int* flag) {
    const i64 words = (i64)ny * W;
    const i64 gw = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (gw >= words) return;
    const int y = (int)(gw / W), w = (int)(gw % W);
    const u64* R = reached + (i64)blockIdx.y * words;
    u64 t[3] = {0, 0, 0};   // rows y - 1 .. y + 1 or-ed, for the words w - 1, w, w + 1
    for (int dy = -1; dy <= 1; ++dy) {
        if (y + dy < 0 || y + dy >= ny) continue;
        const u64* line = R + (i64)(y + dy) * W;
        if (w > 0) t[0] |= line[w - 1];
        t[1] |= line[w];
        if (w + 1 < W) t[2] |= line[w + 1];
    }
    const u64 near = t[1] | (t[1] << 1) | (t[1] >> 1) | (t[0] >> 63) | (t[2] << 63);
    const u64 s = R[gw], f = s | (inv[(i64)blockIdx.y * words + gw] & near);
    if (f != s) {
        reached[(i64)blockIdx.y * words + gw] = f;
        *flag = 1;
    }
}

template <class T>
__global__ void __launch_bounds__(kThreads) finish_kernel(const u64* __restrict__ reached, uint8_t* __restrict__ mask, const T* in, T* masked, int ny,
                                                          int nx, int W, i64 total) {
    const i64 tile_px = (i64)ny * nx;
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < total; i += (i64)gridDim.x * kThreads) {
        const i64 tile = i / tile_px, rem = i - tile * tile_px;
        const int y = (int)(rem / nx), x = (int)(rem - (i64)y * nx);
        const u64 word = reached[(tile * ny + y) * W + (x >> 6)];
        const bool keep = !((word >> (x & 63)) & 1ull);
        mask[i] = keep ? 1 : 0;
        if (masked) masked[i] = keep ? in[i] : (T)0;   // masked may be in: the same sample, read before it is written
    }
}

struct Plan {
    int dev = 0, dt = 0, ny = 0, nx = 0, W = 0, close_k = 1, open_k = 1, conn = 4, max_batch = 0, fill_rounds = 0;
    size_t scratch_bytes = 0;
    DevBuf other, prefix, inv, reached, flags;   // second byte image; row prefixes; packed maps; kRoundsPerBatch flags
    PinnedBuf host_flags;
};

unsigned flat_blocks(i64 total) { return (unsigned)std::min<i64>((total + kThreads - 1) / kThreads, 1 << 20); }

template <bool kDilate>
int morph_op(const Plan& P, hipStream_t st, uint8_t*& cur, uint8_t*& other, int k, int cnt) {
    if (k == 1) return MI_OK;
    const int a = k / 2, r = k - 1 - a;
    hipLaunchKernelGGL(morph_x_kernel<kDilate>, dim3(P.ny, cnt), dim3(kThreads), 0, st, cur, P.prefix.as<int>(), P.ny, P.nx, std::min(a, P.nx),
                       std::min(r, P.nx));
    MI_TRY(launch_check("tile_mask morph_x_kernel"));
    hipLaunchKernelGGL(morph_y_kernel<kDilate>, dim3(cdiv((size_t)P.nx, 64), cnt), dim3(64), 0, st, cur, other, P.ny, P.nx, std::min(a, P.ny),
                       std::min(r, P.ny));
    MI_TRY(launch_check("tile_mask morph_y_kernel"));
    std::swap(cur, other);
    return MI_OK;
}

template <class T>
int run_chunk_t(Plan& P, hipStream_t st, const void* in, double thr, int log_domain, uint8_t* mask, void* masked, int cnt) {
    const i64 tile_px = (i64)P.ny * P.nx, total = tile_px * cnt, words = (i64)P.ny * P.W;
    hipLaunchKernelGGL(threshold_kernel<T>, dim3(flat_blocks(total)), dim3(kThreads), 0, st, static_cast<const T*>(in), mask, total, thr, (float)thr,
                       log_domain);
    MI_TRY(launch_check("tile_mask threshold_kernel"));
    uint8_t *cur = mask, *other = P.other.as<uint8_t>();
    MI_TRY(morph_op<true>(P, st, cur, other, P.close_k, cnt));
    MI_TRY(morph_op<false>(P, st, cur, other, P.close_k, cnt));
    MI_TRY(morph_op<false>(P, st, cur, other, P.open_k, cnt));
    MI_TRY(morph_op<true>(P, st, cur, other, P.open_k, cnt));
    // close and open swap the two images twice each or not at all: cur is the caller's buffer again
    u64 *inv = P.inv.as<u64>(), *reached = P.reached.as<u64>();
    hipLaunchKernelGGL(pack_kernel, dim3(cdiv((size_t)words, kWaves), cnt), dim3(kThreads), 0, st, cur, inv, reached, P.ny, P.nx, P.W);
    MI_TRY(launch_check("tile_mask pack_kernel"));
    int* flags = P.flags.as<int>();
    int* host = P.host_flags.as<int>();
    const i64 cap = tile_px;
    i64 rounds = 0;
    for (bool settled = false; !settled;) {
        if (rounds >= cap) return fail(MI_ERR_INTERNAL, "mi_tile_mask_run: the fill has not settled after %lld rounds", (long long)rounds);
        const int nr = rounds == 0 ? kFirstRounds : kRoundsPerBatch;   // most masks settle at once
        MI_HIP(hipMemsetAsync(flags, 0, kRoundsPerBatch * sizeof(int), st));
        for (int j = 0; j < nr; ++j) {
            hipLaunchKernelGGL(sweep_rows_kernel, dim3(cdiv((size_t)P.ny * cnt, 64)), dim3(64), 0, st, inv, reached, (i64)P.ny * cnt, P.W, flags + j);
            MI_TRY(launch_check("tile_mask sweep_rows_kernel"));
            hipLaunchKernelGGL(sweep_cols_kernel, dim3(cdiv((size_t)P.W, 64), cnt), dim3(64), 0, st, inv, reached, P.ny, P.W, flags + j);
            MI_TRY(launch_check("tile_mask sweep_cols_kernel"));
            if (P.conn == 8) {
                hipLaunchKernelGGL(spread8_kernel, dim3(cdiv((size_t)words, kThreads), cnt), dim3(kThreads), 0, st, inv, reached, P.ny, P.W, flags + j);
                MI_TRY(launch_check("tile_mask spread8_kernel"));
            }
        }
        MI_HIP(hipMemcpyAsync(host, flags, kRoundsPerBatch * sizeof(int), hipMemcpyDeviceToHost, st));
        MI_HIP(hipStreamSynchronize(st));
        for (int j = 0; j < nr && !settled; ++j) {
            ++rounds;
            settled = host[j] == 0;
        }
    }
    P.fill_rounds = (int)std::max<i64>(P.fill_rounds, rounds);
    hipLaunchKernelGGL(finish_kernel<T>, dim3(flat_blocks(total)), dim3(kThreads), 0, st, reached, mask, static_cast<const T*>(in),
                       static_cast<T*>(masked), P.ny, P.nx, P.W, total);
    return launch_check("tile_mask finish_kernel");
}

}  // namespace
}  // namespace mi

using mi::Plan;

extern "C" int mi_tile_mask_plan_create(int dev, int ny, int nx, int dtype, int close_steps, int open_steps, int connectivity, int max_batch,
                                        void** plan) {
    MI_REQUIRE(plan, "mi_tile_mask_plan_create: null pointer");
    *plan = nullptr;
    MI_REQUIRE(ny >= 1 && ny <= mi::kMaxExtent, "mi_tile_mask_plan_create: ny=%d: an extent of 1 .. 2^30 is expected", ny);
    MI_REQUIRE(nx >= 1 && nx <= mi::kMaxExtent, "mi_tile_mask_plan_create: nx=%d: an extent of 1 .. 2^30 is expected", nx);
    MI_REQUIRE((long long)ny * nx <= INT32_MAX, "mi_tile_mask_plan_create: a tile of (ny, nx) = (%d, %d): at most 2^31 - 1 samples per tile", ny, nx);
    MI_REQUIRE(mi::dtype_ok(dtype), "mi_tile_mask_plan_create: dtype=%d: MI_PS_U8, MI_PS_U16 or MI_PS_F32 is expected", dtype);
    MI_REQUIRE(close_steps >= 1, "mi_tile_mask_plan_create: close_steps=%d: a box of 1 or more is expected", close_steps);
    MI_REQUIRE(open_steps >= 1, "mi_tile_mask_plan_create: open_steps=%d: a box of 1 or more is expected", open_steps);
    MI_REQUIRE(connectivity == 4 || connectivity == 8, "mi_tile_mask_plan_create: connectivity=%d: 4 or 8 is expected", connectivity);
    MI_TRY(mi::use_device(dev));
    Plan* P = new Plan;
    P->dev = dev;
    P->dt = dtype;
    P->ny = ny;
    P->nx = nx;
    P->W = (nx + 63) / 64;
    P->close_k = close_steps;
    P->open_k = open_steps;
    P->conn = connectivity;
    P->max_batch = std::min(max_batch > 0 ? max_batch : 16, mi::kMaxChunk);
    const size_t n = (size_t)P->max_batch, px = (size_t)ny * nx, words = (size_t)ny * P->W;
    const bool morph = close_steps > 1 || open_steps > 1;
    const size_t b_other = morph ? n * px : 0, b_prefix = morph ? n * (size_t)ny * ((size_t)nx + 1) * sizeof(int) : 0;
    const size_t b_words = n * words * sizeof(mi::u64), b_flags = mi::kRoundsPerBatch * sizeof(int);
    int rc = P->other.alloc(b_other);
    if (rc == MI_OK) rc = P->prefix.alloc(b_prefix);
    if (rc == MI_OK) rc = P->inv.alloc(b_words);
    if (rc == MI_OK) rc = P->reached.alloc(b_words);
    if (rc == MI_OK) rc = P->flags.alloc(b_flags);
    if (rc == MI_OK) rc = P->host_flags.reserve(b_flags);
    if (rc != MI_OK) {
        delete P;
        return rc;
    }
    P->scratch_bytes = b_other + b_prefix + 2 * b_words + b_flags;
    *plan = P;
    return MI_OK;
}

extern "C" int mi_tile_mask_plan_info(void* plan, mi_tile_mask_info* info) {
    MI_REQUIRE(plan && info, "mi_tile_mask_plan_info: null pointer");
    const Plan& P = *static_cast<Plan*>(plan);
    info->scratch_bytes = P.scratch_bytes;
    info->max_batch = P.max_batch;
    info->fill_rounds = P.fill_rounds;
    return MI_OK;
}

extern "C" int mi_tile_mask_plan_destroy(void* plan) {
    if (!plan) return MI_OK;
    Plan* P = static_cast<Plan*>(plan);
    const int rc = mi::use_device(P->dev);
    delete P;
    return rc;
}

extern "C" int mi_tile_mask_run(void* plan, void* stream, const void* in, double threshold, int log_domain, void* mask, void* masked_out,
                                int64_t count) {
    MI_REQUIRE(plan, "mi_tile_mask_run: plan: null pointer");
    MI_REQUIRE(in, "mi_tile_mask_run: in: null pointer");
    MI_REQUIRE(mask, "mi_tile_mask_run: mask: null pointer");
    MI_REQUIRE(count >= 0, "mi_tile_mask_run: count=%lld: 0 or more tiles are expected", (long long)count);
    Plan& P = *static_cast<Plan*>(plan);
    MI_REQUIRE(!(threshold != threshold), "mi_tile_mask_run: threshold is not a number");
    MI_REQUIRE(!log_domain || P.dt == MI_PS_F32, "mi_tile_mask_run: log_domain=%d: the log-domain compare is built for float32 tiles", log_domain);
    const size_t sb = mi::dtype_bytes(P.dt);
    MI_REQUIRE(reinterpret_cast<uintptr_t>(in) % sb == 0, "mi_tile_mask_run: in is not aligned to a sample");
    MI_REQUIRE(!masked_out || reinterpret_cast<uintptr_t>(masked_out) % sb == 0, "mi_tile_mask_run: masked_out is not aligned to a sample");
    MI_REQUIRE(mask != in && mask != masked_out, "mi_tile_mask_run: mask must be a buffer of its own");
    P.fill_rounds = 0;
    if (count == 0) return MI_OK;
    MI_TRY(mi::use_device(P.dev));
    hipStream_t st = mi::as_stream(stream);
    const size_t px = (size_t)P.ny * P.nx;
    for (int64_t t0 = 0; t0 < count; t0 += P.max_batch) {
        const int cnt = (int)std::min<int64_t>(P.max_batch, count - t0);
        const void* src = static_cast<const char*>(in) + (size_t)t0 * px * sb;
        uint8_t* m = static_cast<uint8_t*>(mask) + (size_t)t0 * px;
        void* out = masked_out ? static_cast<char*>(masked_out) + (size_t)t0 * px * sb : nullptr;
        if (P.dt == MI_PS_U8) MI_TRY(mi::run_chunk_t<uint8_t>(P, st, src, threshold, log_domain, m, out, cnt));
        else if (P.dt == MI_PS_U16) MI_TRY(mi::run_chunk_t<uint16_t>(P, st, src, threshold, log_domain, m, out, cnt));
        else MI_TRY(mi::run_chunk_t<float>(P, st, src, threshold, log_domain, m, out, cnt));
    }
    return MI_OK;
}
