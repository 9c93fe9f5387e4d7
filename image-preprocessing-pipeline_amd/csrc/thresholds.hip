// mi_thresholds.h: the slice estimates of process_images.py:594-655 on the device.
//   mi_hist256_f32       numpy.histogram(image, 256) of float32 images: range, edges and counts, equal to numpy's
//   mi_code_hist         exact counts per code of u8 / u16 images
//   mi_multiotsu_search  threshold_multiotsu's search over a 256-bin histogram (float32 arithmetic in a fixed
//                        order, so the indices are equal to the restatement's)
// All three stream the images once or twice (HBM-bound) and count into LDS; the search is 2.7 M triples of two divisions each.
// The restatement fixes the rounding of every float operation (separate multiply and add): contraction is off for the whole file,
// and written with plain operators: hipcc contracts by default, also across __fmul_rn / __fadd_rn, and an FMA moves an edge or a
// sum by an ulp.  Plain / is the correctly rounded division.
#include <cmath>
#include <cstdint>

#include "mi_internal.h"
#include "mi_thresholds.h"
#include "thresholds_dev.h"

#pragma clang fp contract(off)

namespace mi {
namespace {

using i64 = long long;
using u64 = unsigned long long;

constexpr int kThreads = 256;        // streaming kernels with 256-bin histograms: 4 waves, one histogram each
constexpr int kWaves = kThreads / 64;
constexpr int kU16Threads = 1024;    // u16 codes: one work-group per CU, half of the codes in its LDS per pass
constexpr int kU16Span = 32768;      // counters of one pass: 128 KiB of the CU's 160
constexpr i64 kMaxSamples = 1ll << 38;   // per image: keeps the 32-bit LDS counters of one work-group from overflowing

using namespace histdev;   // float_key, key_float, wave_count, hist_bin (thresholds_dev.h)

template <class T> struct Unpack;
template <> struct Unpack<float> {
    template <class F> static __device__ __forceinline__ void all(const uint4& q, F& f) {
        f(__uint_as_float(q.x)); f(__uint_as_float(q.y)); f(__uint_as_float(q.z)); f(__uint_as_float(q.w));
    }
};
template <> struct Unpack<uint16_t> {
    template <class F> static __device__ __forceinline__ void all(const uint4& q, F& f) {
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { f((uint16_t)(w[k] & 0xffffu)); f((uint16_t)(w[k] >> 16)); }
    }
};
template <> struct Unpack<uint8_t> {
    template <class F> static __device__ __forceinline__ void all(const uint4& q, F& f) {
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { f((uint8_t)(w[k] & 0xffu)); f((uint8_t)((w[k] >> 8) & 0xffu)); f((uint8_t)((w[k] >> 16) & 0xffu)); f((uint8_t)(w[k] >> 24)); }
    }
};

// Every sample of image `img` (n samples at base + img * n) goes to f once, over the work-groups of grid.x: 16-byte loads between
// the first and the last 16-byte boundary, the fewer than 16 / sizeof(T) samples before and behind by elements (work-group 0).
// f may be called by a part of a wave.
template <class T, class F> __device__ __forceinline__ void for_each_sample(const T* base, i64 img, i64 n, F f) {
    constexpr int V = 16 / sizeof(T);
    const T* p = base + img * n;
    i64 head = (i64)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(T));
    if (head > n) head = n;
    const i64 nvec = (n - head) / V;
    const i64 tail_at = head + nvec * V;
    const uint4* body = reinterpret_cast<const uint4*>(p + head);
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        const uint4 q = body[i];
        Unpack<T>::all(q, f);
    }
    if (blockIdx.x == 0) {
        const i64 e = threadIdx.x;
        if (e < head) f(p[e]);
        if (tail_at + e < n) f(p[tail_at + e]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// mi_hist256_f32

__global__ void __launch_bounds__(kThreads) hist_init_kernel(unsigned* keys, int* nonfinite, u64* counts) {
    const i64 img = blockIdx.x;
    counts[img * MI_HIST_BINS + threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        keys[2 * img] = 0xffffffffu;
        keys[2 * img + 1] = 0u;
        nonfinite[img] = 0;
    }
}

__global__ void __launch_bounds__(kThreads) minmax_kernel(const float* base, i64 n, unsigned* keys, int* nonfinite) {
    const i64 img = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for_each_sample<float>(base, img, n, [&](float v) {
        if (fabsf(v) < INFINITY) {
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        } else {
            bad = 1;
        }
    });
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d));
        hi = fmaxf(hi, __shfl_xor(hi, d));
        bad |= __shfl_xor(bad, d);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (lo <= hi) {
            atomicMin(&keys[2 * img], float_key(lo));
            atomicMax(&keys[2 * img + 1], float_key(hi));
        }
        if (bad) atomicOr(&nonfinite[img], 1);
    }
}

// keys -> range in place, and the 257 edges as numpy.linspace(first, last, 257, dtype=float32) makes them
__global__ void __launch_bounds__(kThreads) edges_kernel(unsigned* keys, float* edges) {
    const i64 img = blockIdx.x;
    const int t = threadIdx.x;
    const float first = key_float(keys[2 * img]), last = key_float(keys[2 * img + 1]);
    __syncthreads();
    float e0 = first, e1 = last;
    if (first == last) {
        e0 = (first - 0.5f);
        e1 = (last + 0.5f);
    }
    const float step = (e1 - e0) / 256.0f;
    edges[img * (MI_HIST_BINS + 1) + t] = (float)t * step + e0;
    if (t == 0) {
        edges[img * (MI_HIST_BINS + 1) + MI_HIST_BINS] = e1;
        float* range = reinterpret_cast<float*>(keys);
        range[2 * img] = first;
        range[2 * img + 1] = last;
    }
}

__global__ void __launch_bounds__(kThreads) hist256_kernel(const float* base, i64 n, const float* edges, const int* nonfinite, u64* counts) {
    __shared__ float e[MI_HIST_BINS + 1];
    __shared__ unsigned h[kWaves][MI_HIST_BINS];
    const i64 img = blockIdx.y;
    const int t = threadIdx.x;
    if (nonfinite[img]) return;   // the whole work-group
    e[t] = edges[img * (MI_HIST_BINS + 1) + t];
    if (t == 0) e[MI_HIST_BINS] = edges[img * (MI_HIST_BINS + 1) + MI_HIST_BINS];
    for (int w = 0; w < kWaves; ++w) h[w][t] = 0;
    __syncthreads();
    const float e0 = e[0];
    const float scale = 256.0f / (e[MI_HIST_BINS] - e0);
    unsigned* mine = h[t >> 6];
    for_each_sample<float>(base, img, n, [&](float v) {
        wave_count(mine, hist_bin(e, e0, scale, v));
    });
    __syncthreads();
    unsigned sum = 0;
    for (int w = 0; w < kWaves; ++w) sum += h[w][t];
    if (sum) atomicAdd(&counts[img * MI_HIST_BINS + t], (u64)sum);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// mi_code_hist

__global__ void __launch_bounds__(kThreads) zero_kernel(u64* p, i64 n) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0;
}

__global__ void __launch_bounds__(kThreads) code_hist_u8_kernel(const uint8_t* base, i64 n, u64* counts) {
    __shared__ unsigned h[kWaves][256];
    const i64 img = blockIdx.y;
    const int t = threadIdx.x;
    for (int w = 0; w < kWaves; ++w) h[w][t] = 0;
    __syncthreads();
    unsigned* mine = h[t >> 6];
    for_each_sample<uint8_t>(base, img, n, [&](uint8_t c) { wave_count(mine, (int)c); });
    __syncthreads();
    unsigned sum = 0;
    for (int w = 0; w < kWaves; ++w) sum += h[w][t];
    if (sum) atomicAdd(&counts[img * 256 + t], (u64)sum);
}

// 65 536 counters of 32 bits are 256 KiB, more than the CU's LDS: two passes over the work-group's share of the image, each
// counting the codes of one half of the range (DESIGN section 17 has the reason for passes rather than global atomics)
__global__ void __launch_bounds__(kU16Threads) code_hist_u16_kernel(const uint16_t* base, i64 n, u64* counts) {
    __shared__ unsigned h[kU16Span];
    const i64 img = blockIdx.y;
    const int t = threadIdx.x;
    for (int pass = 0; pass < 65536 / kU16Span; ++pass) {
        for (int i = t; i < kU16Span; i += kU16Threads) h[i] = 0;
        __syncthreads();
        const int first = pass * kU16Span;
        for_each_sample<uint16_t>(base, img, n, [&](uint16_t c) {
            const unsigned r = (unsigned)((int)c - first);
            if (r < (unsigned)kU16Span) wave_count(h, (int)r);
        });
        __syncthreads();
        for (int i = t; i < kU16Span; i += kU16Threads) {
            const unsigned v = h[i];
            if (v) atomicAdd(&counts[img * 65536 + first + i], (u64)v);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// mi_multiotsu_search

constexpr int kSearchBlocks = 64;

// H(i, j) = s^2 / p over the bins i .. j; P1[k] and S1[k] are the sums over the bins below k (P1[0] = 0, and x - 0 is x)
__device__ __forceinline__ float class_term(const float* P1, const float* S1, int i, int j) {
    const float p = P1[j + 1] - P1[i];
    const float s = S1[j + 1] - S1[i];
    return p > 0.0f ? (s * s) / p : 0.0f;
}

__global__ void __launch_bounds__(kThreads) otsu_search_kernel(const u64* counts, int classes, int* indices, int* nvalues, int* status,
                                                               u64* work) {
    __shared__ float P1[MI_HIST_BINS + 1], S1[MI_HIST_BINS + 1], prob[MI_HIST_BINS];
    __shared__ u64 total_s, best_s[kWaves];
    __shared__ int nv_s;
    const i64 img = blockIdx.y;
    const int t = threadIdx.x;
    const u64* c = counts + img * MI_HIST_BINS;
    if (t == 0) {
        u64 total = 0;
        for (int i = 0; i < MI_HIST_BINS; ++i) total += c[i];
        total_s = total;
    }
    __syncthreads();
    prob[t] = total_s ? (float)((double)c[t] / (double)total_s) : 0.0f;   // float64 division, then rounded
    __syncthreads();
    if (t == 0) {   // the sums are sequential by definition
        int nv = 0;
        float p = 0.0f, s = 0.0f;
        P1[0] = 0.0f;
        S1[0] = 0.0f;
        for (int i = 0; i < MI_HIST_BINS; ++i) {
            const float q = prob[i];
            nv += q != 0.0f;
            if (i == 0) {
                p = q;
                s = 0.0f;
            } else {
                p = p + q;
                s = s + (float)i * q;
            }
            P1[i + 1] = p;
            S1[i + 1] = s;
        }
        nv_s = nv;
    }
    __syncthreads();
    const int nv = nv_s;
    const int m = classes - 1;
    if (blockIdx.x == 0 && t == 0) {
        nvalues[img] = nv;
        status[img] = nv < classes ? MI_OTSU_TOO_FEW_VALUES : nv == classes ? MI_OTSU_VALUES_ARE_CLASSES : MI_OTSU_OK;
        int* out = indices + img * (MI_OTSU_MAX_CLASSES - 1);
        for (int k = 0; k < MI_OTSU_MAX_CLASSES - 1; ++k) out[k] = -1;
        if (nv == classes) {
            int k = 0;
            for (int i = 0; i < MI_HIST_BINS && k < m; ++i)
                if (prob[i] != 0.0f) out[k++] = i;
        }
    }
    if (nv <= classes) return;

    // work items: the thresholds but the last (a = item / 256, b = item % 256); the last one is the inner loop
    u64 best = 0;
    for (int item = blockIdx.x * kThreads + t; item < 65536; item += kSearchBlocks * kThreads) {
        const int a = item >> 8, b = item & 255;
        int t0 = 0, t1 = 0, lo = 0;
        float h0 = 0.0f, hm = 0.0f;
        bool ok;
        if (m == 3) {
            ok = a < 253 && b > a && b < 254;
            t0 = a; t1 = b; lo = b + 1;
        } else if (m == 2) {
            ok = a == 0 && b < 254;
            t0 = b; lo = b + 1;
        } else {
            ok = item == 0;
        }
        if (!ok) continue;
        if (m >= 2) h0 = class_term(P1, S1, 0, t0);
        if (m == 3) hm = class_term(P1, S1, t0 + 1, t1);
        for (int last = lo; last < MI_HIST_BINS - 1; ++last) {
            float sigma;
            unsigned rank;
            const float top = class_term(P1, S1, last + 1, MI_HIST_BINS - 1);
            if (m == 3) {
                sigma = ((h0 + top) + hm) + class_term(P1, S1, t1 + 1, last);
                rank = ((unsigned)t0 << 16) | ((unsigned)t1 << 8) | (unsigned)last;
            } else if (m == 2) {
                sigma = (h0 + top) + class_term(P1, S1, t0 + 1, last);
                rank = ((unsigned)t0 << 16) | ((unsigned)last << 8);
            } else {
                sigma = class_term(P1, S1, 0, last) + top;
                rank = (unsigned)last << 16;
            }
            // the largest sigma and, among equals, the lexicographically first thresholds (sigma >= 0: its bits keep the order)
            const u64 key = ((u64)__float_as_uint(sigma) << 32) | (u64)(~rank);
            best = key > best ? key : best;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 other = __shfl_xor(best, d);
        best = other > best ? other : best;
    }
    if ((t & 63) == 0) best_s[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kWaves; ++w) best = best_s[w] > best ? best_s[w] : best;
        if (best) atomicMax(&work[img], best);
    }
}

__global__ void otsu_finish_kernel(int count, int classes, const u64* work, const int* status, int* indices) {
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= count || status[img] != MI_OTSU_OK) return;
    const u64 key = work[img];
    const unsigned rank = (key >> 32) ? ~(unsigned)(key & 0xffffffffu) : 0u;   // no sigma above 0: the thresholds stay at 0
    int* out = indices + (i64)img * (MI_OTSU_MAX_CLASSES - 1);
    for (int k = 0; k < classes - 1; ++k) out[k] = (int)((rank >> (16 - 8 * k)) & 255u);
}

unsigned stream_blocks(i64 items_per_thread_unit, int threads, unsigned cap) {
    const i64 b = (items_per_thread_unit + threads - 1) / threads;
    return (unsigned)(b < 1 ? 1 : (b > (i64)cap ? (i64)cap : b));
}

}  // namespace

int hist_init_launch(hipStream_t s, unsigned* keys, int* nonfinite, unsigned long long* counts, int count) {
    hipLaunchKernelGGL(hist_init_kernel, dim3(count), dim3(kThreads), 0, s, keys, nonfinite, counts);
    return launch_check("hist_init_kernel");
}

int hist_edges_launch(hipStream_t s, unsigned* keys, float* edges, int count) {
    hipLaunchKernelGGL(edges_kernel, dim3(count), dim3(kThreads), 0, s, keys, edges);
    return launch_check("edges_kernel");
}

int multiotsu_launch(hipStream_t s, const unsigned long long* counts, int count, int classes, int* indices, int* nvalues, int* status,
                     unsigned long long* work) {
    MI_HIP(hipMemsetAsync(work, 0, sizeof(unsigned long long) * (size_t)count, s));
    hipLaunchKernelGGL(otsu_search_kernel, dim3(kSearchBlocks, count), dim3(kThreads), 0, s, counts, classes, indices, nvalues, status, work);
    MI_TRY(launch_check("otsu_search_kernel"));
    hipLaunchKernelGGL(otsu_finish_kernel, dim3(cdiv((size_t)count, 64)), dim3(64), 0, s, count, classes, work, status, indices);
    return launch_check("otsu_finish_kernel");
}

}  // namespace mi

using namespace mi;

extern "C" int mi_hist256_f32(int device, void* stream, const float* images, int count, int64_t n, float* range, int* nonfinite,
                              float* edges, unsigned long long* counts) {
    MI_TRY(use_device(device));
    MI_REQUIRE(images && range && nonfinite && edges && counts, "mi_hist256_f32: null pointer");
    MI_REQUIRE(count >= 1 && count <= 65535, "mi_hist256_f32: count=%d, 1 .. 65535 images per call", count);
    MI_REQUIRE(n >= 1 && n <= kMaxSamples, "mi_hist256_f32: n=%lld samples per image, 1 .. 2^38", (long long)n);
    MI_REQUIRE(((uintptr_t)images % 4) == 0 && ((uintptr_t)range % 4) == 0 && ((uintptr_t)edges % 4) == 0 && ((uintptr_t)nonfinite % 4) == 0,
               "mi_hist256_f32: float and int buffers must be 4-byte aligned");
    MI_REQUIRE(((uintptr_t)counts % 8) == 0, "mi_hist256_f32: counts must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    unsigned* keys = reinterpret_cast<unsigned*>(range);
    MI_TRY(hist_init_launch(s, keys, nonfinite, counts, count));
    const dim3 grid(stream_blocks(n / 4 + 1, kThreads * 4, 2048), count);
    hipLaunchKernelGGL(minmax_kernel, grid, dim3(kThreads), 0, s, images, (i64)n, keys, nonfinite);
    MI_TRY(launch_check("minmax_kernel"));
    MI_TRY(hist_edges_launch(s, keys, edges, count));
    hipLaunchKernelGGL(hist256_kernel, grid, dim3(kThreads), 0, s, images, (i64)n, edges, nonfinite, counts);
    return launch_check("hist256_kernel");
}

extern "C" int mi_code_hist(int device, void* stream, const void* images, int dtype, int count, int64_t n, unsigned long long* counts) {
    MI_TRY(use_device(device));
    MI_REQUIRE(images && counts, "mi_code_hist: null pointer");
    MI_REQUIRE(dtype == MI_CODES_U8 || dtype == MI_CODES_U16, "mi_code_hist: dtype=%d, MI_CODES_U8 or MI_CODES_U16", dtype);
    MI_REQUIRE(count >= 1 && count <= 65535, "mi_code_hist: count=%d, 1 .. 65535 images per call", count);
    MI_REQUIRE(n >= 1 && n <= kMaxSamples, "mi_code_hist: n=%lld samples per image, 1 .. 2^38", (long long)n);
    MI_REQUIRE(dtype == MI_CODES_U8 || ((uintptr_t)images % 2) == 0, "mi_code_hist: u16 images must be 2-byte aligned");
    MI_REQUIRE(((uintptr_t)counts % 8) == 0, "mi_code_hist: counts must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const i64 codes = dtype == MI_CODES_U8 ? 256 : 65536;
    hipLaunchKernelGGL(zero_kernel, dim3(stream_blocks(codes * count, kThreads, 1024)), dim3(kThreads), 0, s, counts, codes * count);
    MI_TRY(launch_check("zero_kernel"));
    if (dtype == MI_CODES_U8) {
        const dim3 grid(stream_blocks(n / 16 + 1, kThreads * 4, 2048), count);
        hipLaunchKernelGGL(code_hist_u8_kernel, grid, dim3(kThreads), 0, s, static_cast<const uint8_t*>(images), (i64)n, counts);
        return launch_check("code_hist_u8_kernel");
    }
    // one work-group holds a CU's LDS: at most one per CU, and enough samples each to pay for flushing 65 536 counters
    const dim3 grid(stream_blocks(n / 8 + 1, kU16Threads * 16, 256), count);
    hipLaunchKernelGGL(code_hist_u16_kernel, grid, dim3(kU16Threads), 0, s, static_cast<const uint16_t*>(images), (i64)n, counts);
    return launch_check("code_hist_u16_kernel");
}

extern "C" int mi_multiotsu_search(int device, void* stream, const unsigned long long* counts, int count, int classes, int* indices,
                                   int* nvalues, int* status, unsigned long long* work) {
    MI_TRY(use_device(device));
    MI_REQUIRE(counts && indices && nvalues && status && work, "mi_multiotsu_search: null pointer");
    MI_REQUIRE(count >= 1 && count <= 65535, "mi_multiotsu_search: count=%d, 1 .. 65535 histograms per call", count);
    MI_REQUIRE(classes >= 2 && classes <= MI_OTSU_MAX_CLASSES, "mi_multiotsu_search: classes=%d, 2 .. %d are built", classes, MI_OTSU_MAX_CLASSES);
    MI_REQUIRE(((uintptr_t)counts % 8) == 0 && ((uintptr_t)work % 8) == 0, "mi_multiotsu_search: counts and work must be 8-byte aligned");
    MI_REQUIRE(((uintptr_t)indices % 4) == 0 && ((uintptr_t)nvalues % 4) == 0 && ((uintptr_t)status % 4) == 0,
               "mi_multiotsu_search: int buffers must be 4-byte aligned");
    return multiotsu_launch(as_stream(stream), counts, count, classes, indices, nvalues, status, work);
}
