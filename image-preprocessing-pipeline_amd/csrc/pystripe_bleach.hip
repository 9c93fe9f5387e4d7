// pystripe's bleach correction (pystripe_internal.h: bleach): the row low-pass, the maxima and the apply pass.
#include <algorithm>

#include "pystripe_internal.h"

namespace mi {
namespace ps {
namespace {

__device__ __forceinline__ double bleach_sample(const Src& s, const Bleach& q, i64 tile, int line, int j) {
    float v = src_load(s, tile, line, j);
    if (v == 0.f) v = q.med;
    return (double)fminf(fmaxf(v, q.lo), q.hi);
}

// sample p of the line extended by 6 per side (scipy's odd_ext): 2 x[0] - x[6 .. 1], x, 2 x[n-1] - x[n-2 .. n-7]
__device__ __forceinline__ double bleach_extended(const Src& s, const Bleach& q, i64 tile, int line, int n, int p) {
    const int j = p - kBleachExt;
    if (j < 0) return 2.0 * bleach_sample(s, q, tile, line, 0) - bleach_sample(s, q, tile, line, -j);
    if (j >= n) return 2.0 * bleach_sample(s, q, tile, line, n - 1) - bleach_sample(s, q, tile, line, 2 * (n - 1) - j);
    return bleach_sample(s, q, tile, line, j);
}

// One direction of the recurrence over u[0 .. m) in LDS, in place, from the state z0; returns the state behind the last sample.
// REV walks from u[m - 1] down.  A chunk of `chunk` samples (odd: the threads' 8-byte accesses then fall on different banks)
// per thread: run from state 0 for the chunk's affine map z -> A z + P, scan the maps over the group (shuffles inside a wave, the
// wave totals through `tot`), run again from the carried state.  Every thread of the group calls it.
template <bool REV>
__device__ double bleach_pass(double* u, int m, int chunk, double z0, const Bleach& q, double2* tot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int i0 = min(m, tid * chunk), i1 = min(m, i0 + chunk);
    double A = 1.0, P = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double x = u[REV ? m - 1 - i : i];
        const double y = q.b * x + P;
        P = q.b * x + q.a * y;
        A *= q.a;
    }
    // inclusive scan inside the wave: (Ao, Po) of the lanes before, then (A, P)
    for (int d = 1; d < 64; d <<= 1) {
        const double Ao = __shfl_up(A, d), Po = __shfl_up(P, d);
        if (lane >= d) {
            P = A * Po + P;
            A = A * Ao;
        }
    }
    if (lane == 63) tot[wave] = make_double2(A, P);
    double Ae = __shfl_up(A, 1), Pe = __shfl_up(P, 1);   // the lanes before this one
    if (lane == 0) { Ae = 1.0; Pe = 0.0; }
    __syncthreads();
    double z = z0, zend = z0;
    for (int w = 0; w < nwaves; ++w) {
        const double2 t = tot[w];
        zend = t.x * zend + t.y;
        if (w + 1 == wave) z = zend;
    }
    z = Ae * z + Pe;
    for (int i = i0; i < i1; ++i) {
        const int at = REV ? m - 1 - i : i;
        const double x = u[at];
        const double y = q.b * x + z;
        z = q.b * x + q.a * y;
        u[at] = y;
    }
    __syncthreads();
    return zend;
}

// sosfiltfilt of line blockIdx.x of tile blockIdx.y: n samples through `s`, F as float32 (row stride f_row) and the line's maximum
// of F (lmax may be null).  len = n + 12 <= seg: the whole extended line stays in LDS.  Otherwise segments of seg samples go through
// LDS left to right with the carried state, the forward result goes to fwd (len doubles per line), and the backward pass takes it
// from there in segments right to left.
__global__ void __launch_bounds__(kBleachMaxThreads) bleach_filter_kernel(Src s, int n, int seg, int chunk, Bleach q, float* F, i64 f_tile_stride,
                                                                          int f_row, float* lmax, i64 lmax_tile_stride, double* fwd,
                                                                          i64 fwd_tile_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* u = reinterpret_cast<double*>(smem);
    const int len = n + 2 * kBleachExt, cap = min(len, seg);
    double2* tot = reinterpret_cast<double2*>(u + cap + (cap & 1));
    const int line = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const i64 tile = blockIdx.y;
    if (q.clips) {
        const float* c = q.clips + 3 * tile;
        q.lo = c[0]; q.med = c[1]; q.hi = c[2];
    }
    float* f = F + tile * f_tile_stride + (i64)line * f_row;
    float mx = -INFINITY;
    if (len <= seg) {
        for (int p = tid; p < len; p += T) u[p] = bleach_extended(s, q, tile, line, n, p);
        __syncthreads();
        bleach_pass<false>(u, len, chunk, (1.0 - q.b) * u[0], q, tot);
        bleach_pass<true>(u, len, chunk, (1.0 - q.b) * u[len - 1], q, tot);
        for (int j = tid; j < n; j += T) {
            const float v = (float)u[j + kBleachExt];
            f[j] = v;
            mx = fmaxf(mx, v);
        }
    } else {
        double* y = fwd + tile * fwd_tile_stride + (i64)line * len;
        double z = (1.0 - q.b) * bleach_extended(s, q, tile, line, n, 0);
        for (int s0 = 0; s0 < len; s0 += seg) {
            const int m = min(seg, len - s0);
            for (int p = tid; p < m; p += T) u[p] = bleach_extended(s, q, tile, line, n, s0 + p);
            __syncthreads();
            z = bleach_pass<false>(u, m, chunk, z, q, tot);
            for (int p = tid; p < m; p += T) y[s0 + p] = u[p];
            __syncthreads();
        }
        // the forward result written above is read back by other threads of this group
        __threadfence_block();
        __syncthreads();
        z = (1.0 - q.b) * y[len - 1];
        for (int s1 = len; s1 > 0; s1 -= seg) {
            const int s0 = max(0, s1 - seg), m = s1 - s0;
            for (int p = tid; p < m; p += T) u[p] = y[s0 + p];
            __syncthreads();
            z = bleach_pass<true>(u, m, chunk, z, q, tot);
            for (int p = tid; p < m; p += T) {
                const int j = s0 + p - kBleachExt;
                if (j >= 0 && j < n) {
                    const float v = (float)u[p];
                    f[j] = v;
                    mx = fmaxf(mx, v);
                }
            }
            __syncthreads();
        }
    }
    if (!lmax) return;
    for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    float* red = reinterpret_cast<float*>(tot);   // the last pass has left it
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < (T >> 6); ++w) mx = fmaxf(mx, red[w]);
        lmax[tile * lmax_tile_stride + line] = mx;
    }
}

// max method: the row and column maxima of L in one pass, as keys (zeroed before the launch).  A block covers 64 columns x 64 rows,
// one wave per row at a time.
__global__ void __launch_bounds__(256) bleach_maxima_kernel(Src s, int ny, int nx, unsigned* row_key, unsigned* col_key, i64 key_tile_stride) {
    __shared__ float colmax[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane, y0 = blockIdx.y * 64;
    const i64 tile = blockIdx.z;
    float cm = -INFINITY;
    for (int y = y0 + wave; y < min(ny, y0 + 64); y += 4) {
        const float v = x < nx ? src_load(s, tile, y, x) : -INFINITY;
        cm = fmaxf(cm, v);
        float rm = v;
        for (int d = 32; d >= 1; d >>= 1) rm = fmaxf(rm, __shfl_xor(rm, d));
        if (lane == 0) atomicMax(&row_key[tile * key_tile_stride + y], float_key(rm));
    }
    colmax[wave][lane] = cm;
    __syncthreads();
    if (wave == 0 && x < nx) {
        cm = fmaxf(fmaxf(colmax[0][lane], colmax[1][lane]), fmaxf(colmax[2][lane], colmax[3][lane]));
        atomicMax(&col_key[tile * key_tile_stride + x], float_key(cm));
    }
}

// M[tile] = max F.  max_method: F = ry (x) cx is never stored; a product of two factors is largest at a corner of their ranges and
// float32 rounding keeps the order, so M is the largest of the four float32 products of the vectors' extremes -- for any signs.
__global__ void __launch_bounds__(256) bleach_tilemax_kernel(const float* a, int na, const float* c, int nc, i64 tile_stride, int max_method,
                                                             float* M) {
    __shared__ float red[4][4];
    const i64 tile = blockIdx.x;
    const float* pa = a + tile * tile_stride;
    float v[4] = {-INFINITY, INFINITY, -INFINITY, INFINITY};   // max a, min a, max c, min c
    for (int i = threadIdx.x; i < na; i += 256) { v[0] = fmaxf(v[0], pa[i]); v[1] = fminf(v[1], pa[i]); }
    if (max_method) {
        const float* pc = c + tile * tile_stride;
        for (int i = threadIdx.x; i < nc; i += 256) { v[2] = fmaxf(v[2], pc[i]); v[3] = fminf(v[3], pc[i]); }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        v[0] = fmaxf(v[0], __shfl_xor(v[0], d)); v[1] = fminf(v[1], __shfl_xor(v[1], d));
        v[2] = fmaxf(v[2], __shfl_xor(v[2], d)); v[3] = fminf(v[3], __shfl_xor(v[3], d));
    }
    if ((threadIdx.x & 63) == 0)
        for (int e = 0; e < 4; ++e) red[threadIdx.x >> 6][e] = v[e];
    __syncthreads();
    if (threadIdx.x) return;
    for (int w = 1; w < 4; ++w) {
        v[0] = fmaxf(v[0], red[w][0]); v[1] = fminf(v[1], red[w][1]);
        v[2] = fmaxf(v[2], red[w][2]); v[3] = fminf(v[3], red[w][3]);
    }
    M[tile] = max_method ? fmaxf(fmaxf(v[0] * v[2], v[0] * v[3]), fmaxf(v[1] * v[2], v[1] * v[3])) : v[0];
}

// (L / F) * M in float32, in that order, then the tail every filtered sample takes
__global__ void __launch_bounds__(256) bleach_apply_kernel(Src s, const float* F, i64 f_tile_stride, const float* ry, const float* cx,
                                                           i64 vec_tile_stride, const float* M, Sink k) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const i64 tile = blockIdx.z;
    if (x >= k.nx || y >= k.ny) return;
    const float f = ry ? ry[tile * vec_tile_stride + y] * cx[tile * vec_tile_stride + x] : F[tile * f_tile_stride + (i64)y * k.nx + x];
    const float v = src_load(s, tile, y, x) / f;
    sink_store(k, tile, y, x, v * M[tile]);
}

// sosfiltfilt of `lines` lines of n samples per tile.  The group: a chunk of about nine samples per thread, an odd number of them.
int launch_bleach_filter(const Plan& P, hipStream_t st, const Src& s, int n, int lines, float* F, i64 f_tile_stride, int f_row, float* lmax,
                         i64 lmax_tile_stride, double* fwd, i64 fwd_tile_stride, int cnt) {
    const int len = n + 2 * kBleachExt, cap = std::min(len, kBleachSeg);
    const int threads = std::min(kBleachMaxThreads, std::max(64, (cap / 9 + 63) / 64 * 64));
    const int chunk = ((cap + threads - 1) / threads) | 1;
    const size_t lds = (size_t)(cap + (cap & 1)) * sizeof(double) + kBleachTotals;
    MI_TRY(raise_lds(reinterpret_cast<const void*>(&bleach_filter_kernel), lds));
    hipLaunchKernelGGL(bleach_filter_kernel, dim3(lines, cnt), dim3(threads), lds, st, s, n, kBleachSeg, chunk, P.bq, F, f_tile_stride, f_row, lmax,
                       lmax_tile_stride, len > kBleachSeg ? fwd : nullptr, fwd_tile_stride);
    return launch_check("bleach_filter_kernel");
}

}  // namespace

int run_bleach(const Plan& P, hipStream_t st, const Src& L, const Sink& k, int cnt) {
    const mi_pystripe_info& I = P.info;
    float* M = P.buf(P.off_M);
    double* fwd = P.sz_fwd ? reinterpret_cast<double*>(P.buf(P.off_fwd)) : nullptr;
    const dim3 grid(cdiv(I.nx, 64), cdiv(I.ny, 4), cnt);
    if (P.prm.bleach_max_method) {
        unsigned* key = reinterpret_cast<unsigned*>(P.buf(P.off_key));
        float* vec = P.buf(P.off_vec);
        const i64 vs = (i64)P.sz_vec;
        MI_HIP(hipMemsetAsync(key, 0, sizeof(unsigned) * (size_t)vs * (size_t)cnt, st));
        hipLaunchKernelGGL(bleach_maxima_kernel, dim3(cdiv(I.nx, 64), cdiv(I.ny, 64), cnt), dim3(256), 0, st, L, I.ny, I.nx, key, key + I.ny, vs);
        MI_TRY(launch_check("bleach_maxima_kernel"));
        const Src rows{key, vs, SRC_KEY, 1, I.ny, I.ny, 0, MAP_IDENTITY, 0}, cols{key + I.ny, vs, SRC_KEY, 1, I.nx, I.nx, 0, MAP_IDENTITY, 0};
        MI_TRY(launch_bleach_filter(P, st, rows, I.ny, 1, vec, vs, I.ny, nullptr, 0, fwd, (i64)P.sz_fwd / 2, cnt));
        MI_TRY(launch_bleach_filter(P, st, cols, I.nx, 1, vec + I.ny, vs, I.nx, nullptr, 0, fwd, (i64)P.sz_fwd / 2, cnt));
        hipLaunchKernelGGL(bleach_tilemax_kernel, dim3(cnt), dim3(256), 0, st, vec, I.ny, vec + I.ny, I.nx, vs, 1, M);
        MI_TRY(launch_check("bleach_tilemax_kernel"));
        hipLaunchKernelGGL(bleach_apply_kernel, grid, dim3(256), 0, st, L, (const float*)nullptr, (i64)0, vec, vec + I.ny, vs, M, k);
    } else {
        float* F = P.buf(P.off_F);
        float* lmax = P.buf(P.off_lmax);
        MI_TRY(launch_bleach_filter(P, st, L, I.nx, I.ny, F, (i64)P.sz_F, I.nx, lmax, (i64)P.sz_lmax, fwd, (i64)P.sz_fwd / 2, cnt));
        hipLaunchKernelGGL(bleach_tilemax_kernel, dim3(cnt), dim3(256), 0, st, lmax, I.ny, (const float*)nullptr, 0, (i64)P.sz_lmax, 0, M);
        MI_TRY(launch_check("bleach_tilemax_kernel"));
        hipLaunchKernelGGL(bleach_apply_kernel, grid, dim3(256), 0, st, L, F, (i64)P.sz_F, (const float*)nullptr, (const float*)nullptr, (i64)0, M, k);
    }
    return launch_check("bleach_apply_kernel");
}

}  // namespace ps
}  // namespace mi
