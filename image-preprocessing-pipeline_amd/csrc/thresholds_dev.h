// What thresholds.hip shares with the per-tile clip estimate of pystripe_clips.hip: the device pieces of the 256-bin histogram (keys,
// the bin of a sample, the wave-aggregated LDS count) and launchers of the kernels that stay compiled once, in thresholds.hip
// (range / counter initialisation, the edges of numpy.histogram, the multi-Otsu search).  Launchers enqueue on `s` and check
// nothing but the launch: the callers have checked their arguments.
#ifndef MI_THRESHOLDS_DEV_H
#define MI_THRESHOLDS_DEV_H

#include <hip/hip_runtime.h>

#include "mi_thresholds.h"

namespace mi {

// keys[2 * i] = largest key, keys[2 * i + 1] = 0, nonfinite[i] = 0, counts[i][256] = 0 for i < count
int hist_init_launch(hipStream_t s, unsigned* keys, int* nonfinite, unsigned long long* counts, int count);
// keys (atomicMin / atomicMax of float_key over the finite samples) -> the range in place as floats, and edges[count][257]
int hist_edges_launch(hipStream_t s, unsigned* keys, float* edges, int count);
// mi_multiotsu_search without its argument checks
int multiotsu_launch(hipStream_t s, const unsigned long long* counts, int count, int classes, int* indices, int* nvalues, int* status,
                     unsigned long long* work);

namespace histdev {

// float -> unsigned whose order is the floats' order for either sign
__device__ __forceinline__ unsigned float_key(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// One count into an LDS histogram.  The lanes that hold the same bin as the wave's first active lane add once, together: microscopy
// slices put most samples into a few bins, and 64 atomics on one address run one after the other.
__device__ __forceinline__ void wave_count(unsigned* h, int b) {
    const int lead = __builtin_amdgcn_readfirstlane(b);
    if (b == lead) {
        const unsigned long long m = __ballot(1);
        if ((int)(threadIdx.x & 63u) == __ffsll((long long)m) - 1) atomicAdd(&h[lead], (unsigned)__popcll(m));
    } else {
        atomicAdd(&h[b], 1u);
    }
}

// numpy.histogram's bin of v among the 257 edges e (LDS): edges[b] <= v < edges[b + 1], v == last in bin 255.  scale = 256 / (e[256]
// - e[0]) only seeds the search: the edges decide, so its rounding does not matter.
__device__ __forceinline__ int hist_bin(const float* e, float e0, float scale, float v) {
    int b = (int)((v - e0) * scale);
    b = min(max(b, 0), MI_HIST_BINS - 1);
    while (b > 0 && v < e[b]) --b;
    while (b < MI_HIST_BINS - 1 && v >= e[b + 1]) ++b;
    return b;
}

}  // namespace histdev
}  // namespace mi

#endif
