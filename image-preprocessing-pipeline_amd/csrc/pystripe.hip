// pystripe tile preprocessing (pystripe/core.py process_img :1190, filter_streaks :982, filter_subband :927-940,
// np_filter_coefficient :749) on batches of equally shaped 2-D tiles.  Every launch covers the whole batch (grid z / y = tile):
// one 2048^2 tile leaves most of the device idle at the deep wavelet levels.
//
//   load      the first analysis level reads the tile itself: integer load, log1p and the numpy.pad index map (reflect / wrap /
//             symmetric / edge) are folded into its addressing, so the padded image is never written.  The row pass runs over
//             the SOURCE rows only; the column pass looks rows up through the same map.
//   analysis  out[i] = sum_t F[t] in[sym(2 i + 1 - t)], floor((n + 17) / 2) coefficients ('symmetric', db9); rows then columns:
//             L, H along axis -1, then A, cH (from L) and cV, cD (from H) along axis -2 -- cH is the high-pass along axis -2 of
//             the low-pass along axis -1, PyWavelets' 'da'.
//   notch     np_filter_coefficient multiplies scipy.fftpack.rfft's packed spectrum [r0, r1, i1, r2, i2, ...] by
//             g[j] = 1 - exp(-j^2 / (2 s^2)) BY PACKED POSITION (real part of bin k: g[2k-1], imaginary part: g[2k]), so it is
//             not a convolution.  1 - g[j] is exactly 0 in float32 beyond j ~ 5.9 s: evaluated as c - irfft((1 - g) * rfft(c))
//             over those low positions only, as direct sums in float64 folded over the j <-> n - j symmetry of the twiddles (up to
//             four lines, the twiddle table and their kept spectrum stay in LDS).
//   synthesis out[j] = sum_k a[k] Lo_R[j + 16 - 2 k] + d[k] Hi_R[j + 16 - 2 k]; a thread makes the pair (2p, 2p + 1), which shares
//             its nine k.  waverec2's trim of the approximation is a smaller extent read with the wider stride.
//   store     the last synthesis level computes only the un-padded window and finishes every sample in registers: expm1, rint + clip
//             (integer tiles), dark, 8 / 16-bit conversion, flip and rotation in the store address.
//   bleach    correct_bleaching (:501): with it on, the last synthesis level stores the log image L instead (at sigma == (0, 0)
//             L is log1p on load and never stored); a work-group per row runs sosfiltfilt's forward-backward first-order
//             recurrence in float64 as a scan of affine maps over the clipped, odd-extended row in LDS and writes F and its row
//             maximum; a block per tile reduces the maxima; the apply pass hands (L / F) * max F to the same store.
//   clips     a clip given as NaN: threshold_multiotsu(log1p(tile), 4) per tile before anything else of the run (the "automatic clips" section
//             below): range and 256-bin histogram of the source read through src_load, the search and edges of thresholds.hip,
//             a triple and a status per tile in device memory; the row filter takes its clips from there.
//   wavelets  the kernels named above are db9's (mi_pystripe_plan_create); mi_pystripe_plan_create_wavelet runs their counterparts
//             for any even tap count up to MI_PS_MAX_TAPS (the *_gen_kernel section): same load, notch, store and bleach route.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mi_internal.h"
#include "mi_pystripe.h"
#include "thresholds_dev.h"

namespace mi {
namespace {

constexpr int LF = 18;           // db9
constexpr int kRowBlock = 256;   // outputs of one block of the analysis row pass
constexpr int kMinLength = 34;   // filter_streaks :1092
using i64 = long long;

// Lo_R of db9 (the table of destripe.hip; tests recompute it by spectral factorisation)
const double kLoR[LF] = {3.80779473638783381e-02,  2.43834674612590230e-01,  6.04823123690111153e-01,  6.57288078051299962e-01,
                         1.33197385825007591e-01,  -2.93273783279174305e-01, -9.68407832229760124e-02, 1.48540749338105876e-01,
                         3.07256814793338794e-02,  -6.76328290613307237e-02, 2.50947114831909018e-04,  2.23616621236789742e-02,
                         -4.72320475775138936e-03, -4.28150368246343286e-03, 1.84764688305622871e-03,  2.30385763523196190e-04,
                         -2.51963188942710503e-04, 3.93473203162716365e-05};

struct Filters {
    float lo_d[LF], hi_d[LF], lo_r[LF], hi_r[LF];
};

Filters make_filters() {
    Filters f;
    for (int t = 0; t < LF; ++t) {
        f.lo_r[t] = (float)kLoR[t];
        f.hi_r[t] = (float)(kLoR[LF - 1 - t] * ((t & 1) ? -1.0 : 1.0));   // qmf
    }
    for (int t = 0; t < LF; ++t) {
        f.lo_d[t] = f.lo_r[LF - 1 - t];
        f.hi_d[t] = f.hi_r[LF - 1 - t];
    }
    return f;
}

enum { MAP_IDENTITY = 4 };
enum { SRC_KEY = 3 };   // Src::dtype beside mi_pystripe_dtype: order-preserving keys of floats (float_key)
enum { OUT_FLOAT = 0, OUT_TO8 = 1, OUT_CLIPCAST = 2 };

__device__ __forceinline__ int sym_index(int j, int n) {   // half-point symmetric extension, any distance
    const int p = 2 * n;
    j %= p;
    if (j < 0) j += p;
    return j < n ? j : p - 1 - j;
}

// numpy.pad's index map: padded coordinate i (pad samples in front) -> source index in [0, n)
__device__ __forceinline__ int pad_index(int i, int pad, int n, int mode) {
    int q = i - pad;
    if (mode == MAP_IDENTITY || (q >= 0 && q < n)) return q;
    if (mode == MI_PS_EDGE) return q < 0 ? 0 : n - 1;
    if (mode == MI_PS_WRAP) {
        q %= n;
        return q < 0 ? q + n : q;
    }
    if (mode == MI_PS_SYMMETRIC) return sym_index(q, n);
    if (n == 1) return 0;   // reflect
    const int p = 2 * n - 2;
    q %= p;
    if (q < 0) q += p;
    return q < n ? q : p - q;
}

// where a level's input comes from: the tile itself (any dtype, through the padding map, log1p) or a float image of the pyramid
struct Src {
    const void* p;
    i64 tile_stride;   // samples
    int dtype, ny, nx, row_stride;
    int pad, mode, logp;
};

// float -> unsigned whose order is the floats' order for either sign (0 lies below every float's key)
__device__ __forceinline__ unsigned float_key(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float src_load(const Src& s, i64 tile, int y, int x) {
    const i64 o = tile * s.tile_stride + (i64)y * s.row_stride + x;
    float v;
    if (s.dtype == MI_PS_U16) v = (float)static_cast<const uint16_t*>(s.p)[o];
    else if (s.dtype == MI_PS_U8) v = (float)static_cast<const uint8_t*>(s.p)[o];
    else if (s.dtype == SRC_KEY) v = key_float(static_cast<const unsigned*>(s.p)[o]);
    else v = static_cast<const float*>(s.p)[o];
    return s.logp ? log1pf(v) : v;
}

// what happens to a sample after the filter (process_img :1322-1379 and the tail of filter_streaks :1150-1158)
struct Sink {
    void* out;
    i64 tile_stride;        // samples
    int ny, nx;             // the un-padded tile
    int pad;                // rows / columns in front of it in the padded image
    int filtered;           // the value is in the log domain: expm1 (and rint + clip for integer tiles)
    int log_out;
    int integer_kind;
    float in_max;
    float dark;
    int mode, shift, out_dtype;
    float cast_max;
    int flip, rot;
    const int* varies;      // per tile: 0 = uniform tile -> zeros
    const int* clip_status; // automatic clips: per tile, > 0 = no usable clips -> zeros, also in the log output; else null
};

__device__ __forceinline__ void sink_store(const Sink& k, i64 tile, int y, int x, float v) {
    if (k.log_out) {
        if (k.clip_status && k.clip_status[tile] > 0) v = 0.f;
        static_cast<float*>(k.out)[tile * k.tile_stride + (i64)y * k.nx + x] = v;
        return;
    }
    if (k.filtered) {
        v = expm1f(v);
        if (k.integer_kind) v = fminf(fmaxf(rintf(v), 0.f), k.in_max);
    }
    if (k.dark > 0.f) {
        v = v > k.dark ? v - k.dark : 0.f;
        if (k.integer_kind) v = truncf(v);
    }
    if (!k.varies[tile]) v = 0.f;
    if (k.flip) y = k.ny - 1 - y;
    int oy = y, ox = x, onx = k.nx;
    if (k.rot == 1) { oy = k.nx - 1 - x; ox = y; onx = k.ny; }
    else if (k.rot == 2) { oy = k.ny - 1 - y; ox = k.nx - 1 - x; }
    else if (k.rot == 3) { oy = x; ox = k.ny - 1 - y; onx = k.ny; }
    const i64 o = tile * k.tile_stride + (i64)oy * onx + ox;
    if (k.mode == OUT_FLOAT) {
        static_cast<float*>(k.out)[o] = v;
        return;
    }
    int u;
    if (k.mode == OUT_TO8) {
        u = (int)fminf(fmaxf(v, 0.f), 65535.f);
        u = (u > 0 && u < (1 << k.shift)) ? 1 : (u >> k.shift);
        u = min(u, 255);
    } else {
        u = (int)fminf(fmaxf(v, 0.f), k.cast_max);
    }
    if (k.out_dtype == MI_PS_U16) static_cast<uint16_t*>(k.out)[o] = (uint16_t)u;
    else static_cast<uint8_t*>(k.out)[o] = (uint8_t)u;
}

// is_uniform_2d (:107): varies[tile] |= any sample differs from the first.  VEC: 16-byte loads (the tile's bytes are a multiple of 16 and
// the batch is 16-byte aligned).
template <class T, bool VEC>
__global__ void __launch_bounds__(256) uniform_kernel(const T* in, i64 npix, int* varies) {
    const i64 tile = blockIdx.y;
    const T* p = in + tile * npix;
    const T first = p[0];
    bool d = false;
    const i64 t0 = (i64)blockIdx.x * blockDim.x + threadIdx.x, step = (i64)gridDim.x * blockDim.x;
    if (VEC) {
        constexpr int E = 16 / sizeof(T);
        const uint4* p4 = reinterpret_cast<const uint4*>(p);
        for (i64 i = t0; i < npix / E; i += step) {
            union { uint4 v; T e[E]; } u;
            u.v = p4[i];
#pragma unroll
            for (int q = 0; q < E; ++q) d |= (u.e[q] != first);
        }
    } else {
        for (i64 i = t0; i < npix; i += step) d |= (p[i] != first);
    }
    // one atomic per wave that saw a difference, and none once the flag is up (a stale read only costs a redundant atomic)
    if (__any(d) && (threadIdx.x & 63) == 0 && __atomic_load_n(&varies[tile], __ATOMIC_RELAXED) == 0) atomicOr(&varies[tile], 1);
}

template <class T>
int launch_uniform(hipStream_t st, const void* in, i64 npix, int cnt, int* varies) {
    const bool vec = (npix * sizeof(T)) % 16 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;
    const i64 items = vec ? npix * (i64)sizeof(T) / 16 : npix;
    const dim3 grid((unsigned)std::max<i64>(1, std::min<i64>((items + 256 * 4 - 1) / (256 * 4), 2048)), cnt);
    if (vec) hipLaunchKernelGGL((uniform_kernel<T, true>), grid, dim3(256), 0, st, static_cast<const T*>(in), npix, varies);
    else hipLaunchKernelGGL((uniform_kernel<T, false>), grid, dim3(256), 0, st, static_cast<const T*>(in), npix, varies);
    return launch_check("uniform_kernel");
}

// flat field and skimage's block_reduce (zero padding up to a multiple of the block) -> a float32 tile
__global__ void __launch_bounds__(256) pre_kernel(Src s, const float* flat, int by, int bx, int method, float* stage, int ny, int nx) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const i64 tile = blockIdx.z;
    if (x >= nx || y >= ny) return;
    double sum = 0.0;
    float mx = -INFINITY, mn = INFINITY;
    for (int dy = 0; dy < by; ++dy)
        for (int dx = 0; dx < bx; ++dx) {
            const int yy = y * by + dy, xx = x * bx + dx;
            float v = 0.f;
            if (yy < s.ny && xx < s.nx) {
                v = src_load(s, tile, yy, xx);
                if (flat) v = v / flat[(i64)yy * s.nx + xx];
            }
            sum += (double)v;
            mx = fmaxf(mx, v);
            mn = fminf(mn, v);
        }
    const float r = method == MI_PS_DOWN_MAX ? mx : method == MI_PS_DOWN_MIN ? mn : (float)(sum / (double)(by * bx));
    stage[tile * ((i64)ny * nx) + (i64)y * nx + x] = r;
}

// block_reduce with numpy.median: the by * bx <= N samples of a block (zeros beyond the tile, +inf up to N) are sorted in registers
// by a bitonic network, every index static; an even count gives the mean of the two middle values, taken in float64.
template <int N>
__global__ void __launch_bounds__(256) pre_median_kernel(Src s, const float* flat, int by, int bx, float* stage, int ny, int nx) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const i64 tile = blockIdx.z;
    if (x >= nx || y >= ny) return;
    const int cnt = by * bx;
    float v[N];
    int dy = 0, dx = 0;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        float t = INFINITY;
        if (e < cnt) {
            const int yy = y * by + dy, xx = x * bx + dx;
            t = 0.f;
            if (yy < s.ny && xx < s.nx) {
                t = src_load(s, tile, yy, xx);
                if (flat) t = t / flat[(i64)yy * s.nx + xx];
            }
            if (++dx == bx) { dx = 0; ++dy; }
        }
        v[e] = t;
    }
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
                    v[i] = up ? lo : hi;
                    v[l] = up ? hi : lo;
                }
            }
        }
    }
    const int k0 = (cnt - 1) / 2, k1 = cnt / 2;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i == k0) a = v[i];
        if (i == k1) b = v[i];
    }
    stage[tile * ((i64)ny * nx) + (i64)y * nx + x] = (float)(((double)a + (double)b) * 0.5);
}

template <int N>
int launch_pre_median(hipStream_t st, dim3 grid, const Src& s, const float* flat, int by, int bx, float* stage, int ny, int nx) {
    hipLaunchKernelGGL(pre_median_kernel<N>, grid, dim3(256), 0, st, s, flat, by, bx, stage, ny, nx);
    return launch_check("pre_median_kernel");
}

// no stripe filter: every sample straight to the sink
__global__ void __launch_bounds__(256) point_kernel(Src s, Sink k) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= k.nx || y >= k.ny) return;
    sink_store(k, blockIdx.z, y, x, src_load(s, blockIdx.z, y, x));
}

// analysis along axis -1.  n: extent of the (padded) row, m = (n + 17) / 2 outputs.  A block stages the 2 * 256 + 16 inputs of its
// 256 outputs in LDS (the index maps and log1p are applied once per staged sample), then every thread runs its 18 taps on them.
__global__ void __launch_bounds__(kRowBlock) ana_rows_kernel(Src s, int n, int m, float* L, float* H, i64 out_tile_stride, Filters f) {
    __shared__ float sh[2 * kRowBlock + 16];
    const int i0 = blockIdx.x * kRowBlock, row = blockIdx.y;
    const i64 tile = blockIdx.z;
    const int base = 2 * i0 - 16;
    for (int q = threadIdx.x; q < 2 * kRowBlock + 16; q += kRowBlock) {
        const int j = sym_index(base + q, n);
        sh[q] = src_load(s, tile, row, pad_index(j, s.pad, s.nx, s.mode));
    }
    __syncthreads();
    const int i = i0 + threadIdx.x;
    if (i >= m) return;
    float lo = 0.f, hi = 0.f;
#pragma unroll
    for (int t = 0; t < LF; ++t) {
        const float v = sh[2 * threadIdx.x + 17 - t];
        lo = fmaf(f.lo_d[t], v, lo);
        hi = fmaf(f.hi_d[t], v, hi);
    }
    const i64 o = tile * out_tile_stride + (i64)row * m + i;
    L[o] = lo;
    H[o] = hi;
}

// analysis along axis -2 of L and H ([rows][w], rows looked up through the padding map at the first level): A, cH from L and cV, cD
// from H, each [m][w].  Threads run along x, so every load is a contiguous row segment.
__global__ void __launch_bounds__(256) ana_cols_kernel(const float* L, const float* H, i64 in_tile_stride, int n, int m, int w, int pad,
                                                       int src_rows, int mode, float* A, i64 a_tile_stride, float* cH, float* cV,
                                                       float* cD, i64 d_tile_stride, Filters f) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    const i64 tile = blockIdx.z;
    if (x >= w || i >= m) return;
    const float* l = L + tile * in_tile_stride + x;
    const float* h = H + tile * in_tile_stride + x;
    float a = 0.f, ch = 0.f, cv = 0.f, cd = 0.f;
#pragma unroll
    for (int t = 0; t < LF; ++t) {
        const int r = pad_index(sym_index(2 * i + 1 - t, n), pad, src_rows, mode);
        const float lv = l[(i64)r * w], hv = h[(i64)r * w];
        a = fmaf(f.lo_d[t], lv, a);
        ch = fmaf(f.hi_d[t], lv, ch);
        cv = fmaf(f.lo_d[t], hv, cv);
        cd = fmaf(f.hi_d[t], hv, cd);
    }
    const i64 o = (i64)i * w + x;
    A[tile * a_tile_stride + o] = a;
    cH[tile * d_tile_stride + o] = ch;
    cV[tile * d_tile_stride + o] = cv;
    cD[tile * d_tile_stride + o] = cd;
}

// The packed-position notch on lines of n samples (element stride es, line stride ls, in place).  LDS: the twiddle table
// (cos, sin)(2 pi j / n), R lines, their kept spectrum.  Phase 1: thread = bin k, the R lines share every twiddle read.  Phase 2:
// thread = sample pair (j, n - j) -- the sums are folded over that symmetry.  kp packed positions have a non-zero weight 1 - g; bins 0 .. kb-1 cover them.
template <int R>
__global__ void __launch_bounds__(512) notch_kernel(float* c, i64 tile_stride, int n, int nlines, i64 es, i64 ls, const double2* tw_g,
                                                    const float* wt, int kp, int kb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* tw = reinterpret_cast<double2*>(smem);
    double2* S = tw + n;
    float* xs = reinterpret_cast<float*>(S + (size_t)R * kb);
    const int line0 = blockIdx.x * R;
    float* base = c + (i64)blockIdx.y * tile_stride;
    for (int j = threadIdx.x; j < n; j += blockDim.x) tw[j] = tw_g[j];
    for (int e = threadIdx.x; e < R * n; e += blockDim.x) {
        int r, j;
        if (es == 1) { r = e / n; j = e - r * n; }
        else { j = e / R; r = e - j * R; }
        xs[r * n + j] = (line0 + r < nlines) ? base[(i64)(line0 + r) * ls + (i64)j * es] : 0.f;
    }
    __syncthreads();
    // fold: cos is even and sin odd under j -> n - j, so the samples j and n - j share a twiddle: e_j = x_j + x_{n-j} meets the cosine
    // only, o_j = x_j - x_{n-j} the sine only (kept in place of x_j and x_{n-j}); j = 0 and, for an even n, j = n / 2 stand alone.
    // Half the float64 sums of the plain form, in both phases.
    const int hp = (n - 1) / 2;   // pairs j = 1 .. hp
    for (int e = threadIdx.x; e < R * hp; e += blockDim.x) {
        const int r = e / hp, j = 1 + e - r * hp;
        const float a = xs[r * n + j], b = xs[r * n + n - j];
        xs[r * n + j] = a + b;
        xs[r * n + n - j] = a - b;
    }
    __syncthreads();
    const double inv_n = 1.0 / (double)n;
    const bool even = (n & 1) == 0;
    for (int k = threadIdx.x; k < kb; k += blockDim.x) {
        double re[R], im[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            re[r] = (double)xs[r * n];
            if (even) re[r] += (k & 1) ? -(double)xs[r * n + n / 2] : (double)xs[r * n + n / 2];
            im[r] = 0.0;
        }
        int idx = k;
        for (int j = 1; j <= hp; ++j) {
            const double2 t = tw[idx];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                re[r] = fma((double)xs[r * n + j], t.x, re[r]);
                im[r] = fma(-(double)xs[r * n + n - j], t.y, im[r]);
            }
            idx += k;
            if (idx >= n) idx -= n;
        }
        // gains by packed position: real part of bin k at 2k - 1, imaginary part at 2k; DC at 0; the Nyquist bin of an even n has no
        // imaginary part and counts once
        const int pr = k == 0 ? 0 : 2 * k - 1, pi = 2 * k;
        const double wr = pr < kp ? (double)wt[pr] : 0.0;
        const double wi = (k == 0 || pi >= kp || pi >= n) ? 0.0 : (double)wt[pi];
        const double sc = (k == 0 || 2 * k == n) ? inv_n : 2.0 * inv_n;
#pragma unroll
        for (int r = 0; r < R; ++r) S[r * kb + k] = make_double2(re[r] * wr * sc, im[r] * wi * sc);
    }
    __syncthreads();
    // thread = the pair (j, n - j): smooth_j = S_0 + A - B, smooth_{n-j} = S_0 + A + B with A the cosine and B the sine sum
    for (int j = threadIdx.x; j <= n / 2; j += blockDim.x) {
        double A[R], B[R];
#pragma unroll
        for (int r = 0; r < R; ++r) A[r] = B[r] = 0.0;
        int idx = j;
        for (int k = 1; k < kb; ++k) {
            const double2 t = tw[idx];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double2 sv = S[r * kb + k];
                A[r] = fma(sv.x, t.x, A[r]);
                B[r] = fma(sv.y, t.y, B[r]);
            }
            idx += j;
            if (idx >= n) idx -= n;
        }
        const bool twin = j != 0 && 2 * j != n;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (line0 + r >= nlines) continue;
            float* line = base + (i64)(line0 + r) * ls;
            const double s0 = S[r * kb].x;
            line[(i64)j * es] = line[(i64)j * es] - (float)(s0 + A[r] - B[r]);
            if (twin) line[(i64)(n - j) * es] = line[(i64)(n - j) * es] - (float)(s0 + A[r] + B[r]);
        }
    }
}

// synthesis along axis -2: rows 2p, 2p + 1 of lo1 (from a, cH) and hi1 (from cV, cD); blockIdx.z = 2 * tile + which.  a has its
// own row stride (the approximation of a deeper level is one row / column larger than the details: waverec2 trims it).
__global__ void __launch_bounds__(256) syn_cols_kernel(const float* a, i64 a_tile_stride, int a_stride, const float* cH, const float* cV,
                                                       const float* cD, i64 d_tile_stride, int w, int p0, int p1, int s0, float* lo1,
                                                       float* hi1, i64 out_tile_stride, Filters f) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), p = p0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    const i64 tile = blockIdx.z >> 1;
    const int which = blockIdx.z & 1;
    if (x >= w || p >= p1) return;
    const float* lo = which ? cV + tile * d_tile_stride : a + tile * a_tile_stride;
    const float* hi = (which ? cD : cH) + tile * d_tile_stride;
    const int lo_stride = which ? w : a_stride;
    float e = 0.f, o = 0.f;
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        const float av = lo[(i64)(p + d) * lo_stride + x], dv = hi[(i64)(p + d) * w + x];
        e = fmaf(av, f.lo_r[16 - 2 * d], e);
        e = fmaf(dv, f.hi_r[16 - 2 * d], e);
        o = fmaf(av, f.lo_r[17 - 2 * d], o);
        o = fmaf(dv, f.hi_r[17 - 2 * d], o);
    }
    float* dst = (which ? hi1 : lo1) + tile * out_tile_stride;
    dst[(i64)(2 * p) * w + x] = e;
    if (2 * p + 1 < s0) dst[(i64)(2 * p + 1) * w + x] = o;
}

// synthesis along axis -1: columns 2p, 2p + 1 of rows y0 + blockIdx.y.  FINAL: only the un-padded window, through the sink.
template <bool FINAL>
__global__ void __launch_bounds__(256) syn_rows_kernel(const float* lo1, const float* hi1, i64 in_tile_stride, int w, int y0, int p0, int p1,
                                                       int s1, float* out, i64 out_tile_stride, Sink k, Filters f) {
    const int p = p0 + blockIdx.x * 256 + threadIdx.x, y = y0 + blockIdx.y;
    const i64 tile = blockIdx.z;
    if (p >= p1) return;
    const float* lo = lo1 + tile * in_tile_stride + (i64)y * w + p;
    const float* hi = hi1 + tile * in_tile_stride + (i64)y * w + p;
    float e = 0.f, o = 0.f;
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        const float av = lo[d], dv = hi[d];
        e = fmaf(av, f.lo_r[16 - 2 * d], e);
        e = fmaf(dv, f.hi_r[16 - 2 * d], e);
        o = fmaf(av, f.lo_r[17 - 2 * d], o);
        o = fmaf(dv, f.hi_r[17 - 2 * d], o);
    }
    if (FINAL) {
        const int yy = y - k.pad, x0 = 2 * p - k.pad;
        if (x0 >= 0 && x0 < k.nx) sink_store(k, tile, yy, x0, e);
        if (x0 + 1 >= 0 && x0 + 1 < k.nx) sink_store(k, tile, yy, x0 + 1, o);
    } else {
        float* dst = out + tile * out_tile_stride + (i64)y * s1;
        dst[2 * p] = e;
        if (2 * p + 1 < s1) dst[2 * p + 1] = o;
    }
}

// ---- any orthogonal wavelet of L taps (L even, 2 .. MI_PS_MAX_TAPS) ---------------------------------------------------------------
// The transform above with the tap count as a run-time value: m = (n + L - 1) / 2 coefficients, 2 m - L + 2 samples back.  4 x 90
// coefficients do not fit a wave's scalar registers, so the four filters lie in device memory, each with kTabPad zeros on either
// side, and are read at wave-uniform addresses inside loops that are not unrolled by L; the zeros let a thread that makes four
// neighbouring outputs run one loop over all the inputs they share.  The column passes stage their input rows in LDS, so a row is
// read once per block instead of L / 2 times.

constexpr int kTabPad = 8;      // zeros on either side of a filter in the table
constexpr int kColRows = 16;    // output rows of a block of the column analysis
constexpr int kColPairs = 16;   // output row pairs of a block of the column synthesis

__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// analysis along axis -1: 2 * 256 + L - 2 inputs of a block in LDS (the symmetric extension may reflect more than once: L - 2 can
// exceed the row); a thread takes its taps two at a time as one 8-byte LDS read.
__global__ void __launch_bounds__(kRowBlock) ana_rows_gen_kernel(Src s, int n, int m, float* __restrict__ Lo, float* __restrict__ Hi,
                                                                 i64 out_tile_stride, const float* __restrict__ tab, int L) {
    __shared__ __attribute__((aligned(16))) float sh[2 * kRowBlock + MI_PS_MAX_TAPS - 2];
    const int i0 = blockIdx.x * kRowBlock, row = blockIdx.y;
    const i64 tile = blockIdx.z;
    const int base = 2 * i0 - (L - 2);
    const int cnt = 2 * min(kRowBlock, m - i0) + L - 2;
    for (int q = threadIdx.x; q < cnt; q += kRowBlock) sh[q] = src_load(s, tile, row, pad_index(sym_index(base + q, n), s.pad, s.nx, s.mode));
    __syncthreads();
    const int i = i0 + threadIdx.x;
    if (i >= m) return;
    const float* lo_d = tab + kTabPad;
    const float* hi_d = tab + (L + 2 * kTabPad) + kTabPad;
    const float2* v2 = reinterpret_cast<const float2*>(sh) + threadIdx.x;   // sh[2 tid + 2 c]: tap L - 1 - 2 c, then tap L - 2 - 2 c
    float lo = 0.f, hi = 0.f;
    for (int c = 0; c < L / 2; ++c) {
        const float2 v = v2[c];
        const int t = L - 2 - 2 * c;
        lo = fmaf(lo_d[t + 1], v.x, lo);
        hi = fmaf(hi_d[t + 1], v.x, hi);
        lo = fmaf(lo_d[t], v.y, lo);
        hi = fmaf(hi_d[t], v.y, hi);
    }
    const i64 o = tile * out_tile_stride + (i64)row * m + i;
    Lo[o] = lo;
    Hi[o] = hi;
}

// analysis along axis -2: a block makes kColRows output rows of 64 columns from the (2 kColRows + L - 2) x 64 segments of L and H in
// LDS (rows through the padding map at the first level; all of them are staged, also behind the last output row: a zero filter
// entry must not meet an unwritten word).  A wave makes four neighbouring output rows: staged row 2 il0 + q meets tap L - 1 - q + 2 j
// of output il0 + j.
__global__ void __launch_bounds__(256) ana_cols_gen_kernel(const float* __restrict__ Lo, const float* __restrict__ Hi, i64 in_tile_stride, int n,
                                                           int m, int w, int pad, int src_rows, int mode, float* __restrict__ A,
                                                           i64 a_tile_stride, float* __restrict__ cH, float* __restrict__ cV,
                                                           float* __restrict__ cD, i64 d_tile_stride, const float* __restrict__ tab, int L) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nrows = 2 * kColRows + L - 2;
    float* shL = reinterpret_cast<float*>(smem);
    float* shH = shL + nrows * 64;
    const int lane = threadIdx.x & 63, wave = wave_index();
    const int x = blockIdx.x * 64 + lane, i0 = blockIdx.y * kColRows;
    const i64 tile = blockIdx.z;
    const int base = 2 * i0 - (L - 2);
    const float* l = Lo + tile * in_tile_stride + x;
    const float* h = Hi + tile * in_tile_stride + x;
    for (int q = wave; q < nrows; q += 4) {
        const int r = pad_index(sym_index(base + q, n), pad, src_rows, mode);
        float lv = 0.f, hv = 0.f;
        if (x < w) {
            lv = l[(i64)r * w];
            hv = h[(i64)r * w];
        }
        shL[q * 64 + lane] = lv;
        shH[q * 64 + lane] = hv;
    }
    __syncthreads();
    const int il0 = 4 * wave;
    if (i0 + il0 >= m) return;
    const float* lo_d = tab + kTabPad;
    const float* hi_d = tab + (L + 2 * kTabPad) + kTabPad;
    const float* pl = shL + 2 * il0 * 64 + lane;
    const float* ph = shH + 2 * il0 * 64 + lane;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, ch[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f}, cd[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < L + 6; q += 2) {
        const float l0 = pl[q * 64], h0 = ph[q * 64], l1 = pl[(q + 1) * 64], h1 = ph[(q + 1) * 64];
        const int t0 = L - 1 - q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float fl0 = lo_d[t0 + 2 * j], fh0 = hi_d[t0 + 2 * j], fl1 = lo_d[t0 - 1 + 2 * j], fh1 = hi_d[t0 - 1 + 2 * j];
            a[j] = fmaf(fl0, l0, a[j]);
            ch[j] = fmaf(fh0, l0, ch[j]);
            cv[j] = fmaf(fl0, h0, cv[j]);
            cd[j] = fmaf(fh0, h0, cd[j]);
            a[j] = fmaf(fl1, l1, a[j]);
            ch[j] = fmaf(fh1, l1, ch[j]);
            cv[j] = fmaf(fl1, h1, cv[j]);
            cd[j] = fmaf(fh1, h1, cd[j]);
        }
    }
    if (x >= w) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = i0 + il0 + j;
        if (i >= m) break;
        const i64 o = (i64)i * w + x;
        A[tile * a_tile_stride + o] = a[j];
        cH[tile * d_tile_stride + o] = ch[j];
        cV[tile * d_tile_stride + o] = cv[j];
        cD[tile * d_tile_stride + o] = cd[j];
    }
}

// synthesis along axis -2: a block makes kColPairs row pairs (2 p, 2 p + 1) of 64 columns from rows p .. p + L / 2 - 1 of its two
// inputs, staged in LDS (zeros behind the last coefficient row m - 1).  blockIdx.z = 2 * tile + which, as in syn_cols_kernel.  A wave
// makes four neighbouring pairs: staged row pl0 + q meets taps L - 2 - 2 (q - j) (even output) and L - 1 - 2 (q - j) (odd) of pair pl0 + j.
__global__ void __launch_bounds__(256) syn_cols_gen_kernel(const float* __restrict__ a, i64 a_tile_stride, int a_stride, const float* __restrict__ cH,
                                                           const float* __restrict__ cV, const float* __restrict__ cD, i64 d_tile_stride, int w,
                                                           int m, int p0, int p1, int s0, float* __restrict__ lo1, float* __restrict__ hi1,
                                                           i64 out_tile_stride, const float* __restrict__ tab, int L) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int half = L / 2, nrows = kColPairs + half - 1;
    float* shA = reinterpret_cast<float*>(smem);
    float* shD = shA + nrows * 64;
    const int lane = threadIdx.x & 63, wave = wave_index();
    const int x = blockIdx.x * 64 + lane, pb = p0 + blockIdx.y * kColPairs;
    const i64 tile = blockIdx.z >> 1;
    const int which = blockIdx.z & 1;
    const float* lo = (which ? cV + tile * d_tile_stride : a + tile * a_tile_stride) + x;
    const float* hi = (which ? cD : cH) + tile * d_tile_stride + x;
    const int lo_stride = which ? w : a_stride;
    for (int q = wave; q < nrows; q += 4) {
        const int r = pb + q;
        float av = 0.f, dv = 0.f;
        if (x < w && r < m) {
            av = lo[(i64)r * lo_stride];
            dv = hi[(i64)r * w];
        }
        shA[q * 64 + lane] = av;
        shD[q * 64 + lane] = dv;
    }
    __syncthreads();
    const int pl0 = 4 * wave;
    if (pb + pl0 >= p1) return;
    const int TS = L + 2 * kTabPad;
    const float* lo_r = tab + 2 * TS + kTabPad;
    const float* hi_r = tab + 3 * TS + kTabPad;
    const float* pa = shA + pl0 * 64 + lane;
    const float* pd = shD + pl0 * 64 + lane;
    float e[4] = {0.f, 0.f, 0.f, 0.f}, o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < half + 3; ++q) {
        const float av = pa[q * 64], dv = pd[q * 64];
        const int t0 = L - 2 - 2 * q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = fmaf(av, lo_r[t0 + 2 * j], e[j]);
            e[j] = fmaf(dv, hi_r[t0 + 2 * j], e[j]);
            o[j] = fmaf(av, lo_r[t0 + 2 * j + 1], o[j]);
            o[j] = fmaf(dv, hi_r[t0 + 2 * j + 1], o[j]);
        }
    }
    if (x >= w) return;
    float* dst = (which ? hi1 : lo1) + tile * out_tile_stride + x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = pb + pl0 + j;
        if (p >= p1) break;
        dst[(i64)(2 * p) * w] = e[j];
        if (2 * p + 1 < s0) dst[(i64)(2 * p + 1) * w] = o[j];
    }
}

// synthesis along axis -1: the 256 + L / 2 - 1 inputs of a block's 256 pairs in LDS.  FINAL as in syn_rows_kernel.
template <bool FINAL>
__global__ void __launch_bounds__(256) syn_rows_gen_kernel(const float* __restrict__ lo1, const float* __restrict__ hi1, i64 in_tile_stride, int w,
                                                           int y0, int p0, int p1, int s1, float* __restrict__ out, i64 out_tile_stride, Sink k,
                                                           const float* __restrict__ tab, int L) {
    __shared__ float shA[256 + MI_PS_MAX_TAPS / 2 - 1], shD[256 + MI_PS_MAX_TAPS / 2 - 1];
    const int pb = p0 + blockIdx.x * 256, y = y0 + blockIdx.y;
    const i64 tile = blockIdx.z;
    const int half = L / 2, cnt = min(256, p1 - pb) + half - 1;
    const float* lo = lo1 + tile * in_tile_stride + (i64)y * w + pb;
    const float* hi = hi1 + tile * in_tile_stride + (i64)y * w + pb;
    for (int q = threadIdx.x; q < cnt; q += 256) {
        shA[q] = lo[q];
        shD[q] = hi[q];
    }
    __syncthreads();
    const int p = pb + threadIdx.x;
    if (p >= p1) return;
    const int TS = L + 2 * kTabPad;
    const float* lo_r = tab + 2 * TS + kTabPad;
    const float* hi_r = tab + 3 * TS + kTabPad;
    float e = 0.f, o = 0.f;
    for (int d = 0; d < half; ++d) {
        const float av = shA[threadIdx.x + d], dv = shD[threadIdx.x + d];
        const int t = L - 2 - 2 * d;
        e = fmaf(av, lo_r[t], e);
        e = fmaf(dv, hi_r[t], e);
        o = fmaf(av, lo_r[t + 1], o);
        o = fmaf(dv, hi_r[t + 1], o);
    }
    if (FINAL) {
        const int yy = y - k.pad, x0 = 2 * p - k.pad;
        if (x0 >= 0 && x0 < k.nx) sink_store(k, tile, yy, x0, e);
        if (x0 + 1 >= 0 && x0 + 1 < k.nx) sink_store(k, tile, yy, x0 + 1, o);
    } else {
        float* dst = out + tile * out_tile_stride + (i64)y * s1;
        dst[2 * p] = e;
        if (2 * p + 1 < s1) dst[2 * p + 1] = o;
    }
}

// ---- bleach correction (correct_bleaching :501, butter_lowpass_filter :492) -----------------------------------------------------

constexpr int kBleachExt = 6;                         // sosfiltfilt's padlen for one section
constexpr int kBleachMaxThreads = 1024;
constexpr size_t kBleachLds = 160 * 1024;              // all of a CU's LDS
constexpr size_t kBleachTotals = (kBleachMaxThreads / 64) * sizeof(double2);   // the scan's wave totals, behind the row
constexpr int kBleachSeg = (int)((kBleachLds - kBleachTotals) / sizeof(double));   // doubles of a row (or of a segment of it) in LDS
static_assert(kBleachSeg - 2 * kBleachExt == MI_PS_BLEACH_LDS_ROW, "MI_PS_BLEACH_LDS_ROW is derived from the LDS request");

struct Bleach {
    double b, a;              // y = b u + z;  z' = b u + a y
    float lo, med, hi;        // G = clip(L == 0 ? med : L, lo, hi)
    const float* clips;       // automatic clips: [tile][3] = lo, med, hi in device memory, instead of the three above; else null
};

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

// ---- automatic clips (filter_streaks :1066-1077: threshold_multiotsu(log1p(tile), classes=4)) --------------------------------------
// The value of a sample of the log image: for an integer-kind tile table[code] (numpy's float32 log1p of the code, so that the
// counts are numpy.histogram's exactly; the staged float of a max / min down-sample is a whole code), else log1pf on load (s.logp).

__device__ __forceinline__ float auto_value(const Src& s, const float* table, int ncodes, i64 tile, int y, int x) {
    const float v = src_load(s, tile, y, x);
    return table ? table[min(max((int)v, 0), ncodes - 1)] : v;
}

// finite range per tile as keys (thresholds.hip's minmax_kernel on this source); rows over the work-groups of grid.x
__global__ void __launch_bounds__(256) auto_range_kernel(Src s, const float* table, int ncodes, unsigned* keys, int* nonfinite) {
    const i64 tile = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int y = blockIdx.x; y < s.ny; y += gridDim.x)
        for (int x = threadIdx.x; x < s.nx; x += 256) {
            const float v = auto_value(s, table, ncodes, tile, y, x);
            if (fabsf(v) < INFINITY) {
                lo = fminf(lo, v);
                hi = fmaxf(hi, v);
            } else {
                bad = 1;
            }
        }
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d));
        hi = fmaxf(hi, __shfl_xor(hi, d));
        bad |= __shfl_xor(bad, d);
    }
    // one pair of atomics per work-group: every group of a tile lands on the same two addresses, and they run one after the other
    __shared__ float wlo[4], whi[4];
    __shared__ int wbad[4];
    if ((threadIdx.x & 63u) == 0) {
        wlo[threadIdx.x >> 6] = lo;
        whi[threadIdx.x >> 6] = hi;
        wbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lo = fminf(lo, wlo[w]);
            hi = fmaxf(hi, whi[w]);
            bad |= wbad[w];
        }
        if (lo <= hi) {
            atomicMin(&keys[2 * tile], histdev::float_key(lo));
            atomicMax(&keys[2 * tile + 1], histdev::float_key(hi));
        }
        if (bad) atomicOr(&nonfinite[tile], 1);
    }
}

// numpy.histogram(., 256) per tile (thresholds.hip's hist256_kernel on this source)
__global__ void __launch_bounds__(256) auto_hist_kernel(Src s, const float* table, int ncodes, const float* edges, const int* nonfinite,
                                                        unsigned long long* counts) {
    __shared__ float e[MI_HIST_BINS + 1];
    __shared__ unsigned h[4][MI_HIST_BINS];
    const i64 tile = blockIdx.y;
    const int t = threadIdx.x;
    if (nonfinite[tile]) return;   // the whole work-group
    e[t] = edges[tile * (MI_HIST_BINS + 1) + t];
    if (t == 0) e[MI_HIST_BINS] = edges[tile * (MI_HIST_BINS + 1) + MI_HIST_BINS];
    for (int w = 0; w < 4; ++w) h[w][t] = 0;
    __syncthreads();
    const float e0 = e[0];
    const float scale = 256.0f / (e[MI_HIST_BINS] - e0);
    unsigned* mine = h[t >> 6];
    for (int y = blockIdx.x; y < s.ny; y += gridDim.x)
        for (int x = t; x < s.nx; x += 256) histdev::wave_count(mine, histdev::hist_bin(e, e0, scale, auto_value(s, table, ncodes, tile, y, x)));
    __syncthreads();
    unsigned sum = 0;
    for (int w = 0; w < 4; ++w) sum += h[w][t];
    if (sum) atomicAdd(&counts[tile * MI_HIST_BINS + t], (unsigned long long)sum);
}

// The triple and the status of every tile: given clips keep their slot, an estimated one is the float32 centre of the bin the search
// named; min is raised to log1p(1); the asserts of correct_bleaching :524-528 on the result.  A tile without usable clips is zeroed
// through `varies`; its estimated slots hold NaN unless the order check failed (the triple is then what the caller reports).
__global__ void __launch_bounds__(64) auto_clips_kernel(int cnt, int bits, float gmin, float gmed, float gmax, double floor_lo, const float* edges,
                                                        const int* indices, const int* otsu_status, const int* nonfinite, int uniform_rule,
                                                        int* varies, float* clips, int* status) {
    const int tile = blockIdx.x * 64 + threadIdx.x;
    if (tile >= cnt) return;
    float c[3] = {gmin, gmed, gmax};
    int st = MI_PS_CLIPS_OK;
    if (uniform_rule && !varies[tile]) st = MI_PS_CLIPS_UNIFORM;
    else if (nonfinite[tile]) st = MI_PS_CLIPS_NONFINITE;
    else if (otsu_status[tile] == MI_OTSU_TOO_FEW_VALUES) st = MI_PS_CLIPS_TOO_FEW;
    const float* e = edges + (i64)tile * (MI_HIST_BINS + 1);
    for (int k = 0; k < 3; ++k)
        if ((bits >> k) & 1) {
            const int i = min(max(indices[tile * (MI_OTSU_MAX_CLASSES - 1) + k], 0), MI_HIST_BINS - 1);
            c[k] = st == MI_PS_CLIPS_OK ? (e[i] + e[i + 1]) / 2.0f : NAN;
        }
    if (st == MI_PS_CLIPS_OK && !(c[0] >= 0.f && c[1] > c[0] && c[2] > c[0] && c[2] > c[1])) st = MI_PS_CLIPS_ORDER;
    if (st == MI_PS_CLIPS_OK) c[0] = (float)fmax((double)c[0], floor_lo);
    if (st > 0) varies[tile] = 0;
    clips[3 * tile] = c[0]; clips[3 * tile + 1] = c[1]; clips[3 * tile + 2] = c[2];
    status[tile] = st;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

int notch_rise_point(double sigma, double rise) {   // :670
    return (int)(std::sqrt(-2.0 * sigma * sigma * std::log(1.0 - rise)) + 0.5) / 2 * 2;
}

int pad_size(int ny, int nx, double sigma) {   // calculate_pad_size :681
    if (sigma == 0) return 0;
    const double x = nx + 1.0, y = ny + 1.0, c = 5e14;
    const double s = std::sqrt(x * x - 2 * x * y + y * y + 4 * c);
    const double r = std::nearbyint((1.0 - std::exp((x + y - s) / (4 * sigma * sigma))) * 100.0) / 100.0 - 0.01;
    return notch_rise_point(sigma, std::min(r, 0.5));
}

int max_level(int n, int L) { return n >= L - 1 ? std::max((int)std::floor(std::log2((double)n / (L - 1))), 0) : 0; }   // pywt.dwt_max_level

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

struct NotchTab {          // one (pass, level, axis)
    int n, kp, kb, R, threads;
    size_t lds;
    size_t tw_off, w_off;  // into the plan's table buffers (elements)
};

struct Plan {
    int dev = 0, in_ny = 0, in_nx = 0, in_dtype = 0;
    mi_pystripe_params prm{};
    mi_pystripe_info info{};
    bool filter = false, pre = false, bleach = false;
    int passes = 0;
    Bleach bq{};
    Filters f{};
    int L = LF;               // taps; generic: the run-time-length kernels with their filter table (mi_pystripe_plan_create_wavelet)
    bool generic = false;
    DevBuf tab_buf;
    int h[MI_PS_MAX_LEVELS + 1] = {0}, w[MI_PS_MAX_LEVELS + 1] = {0};   // extents per level, [0] = padded image
    // per-tile scratch, offsets in floats
    size_t off_stage = 0, off_P = 0, off_rowL = 0, off_rowH = 0, off_A[MI_PS_MAX_LEVELS + 1] = {0}, off_cH[MI_PS_MAX_LEVELS + 1] = {0},
           off_cV[MI_PS_MAX_LEVELS + 1] = {0}, off_cD[MI_PS_MAX_LEVELS + 1] = {0};
    size_t sz_stage = 0, sz_P = 0, sz_row = 0, sz_A[MI_PS_MAX_LEVELS + 1] = {0}, sz_d[MI_PS_MAX_LEVELS + 1] = {0};
    // bleach correction: the log image (with a stripe filter), F and its row maxima, or (max method) the maxima keys and the filtered
    // vectors, rows first; the tile maximum; the forward result of lines too long for LDS (doubles, two floats each)
    size_t off_L = 0, off_F = 0, off_lmax = 0, off_key = 0, off_vec = 0, off_M = 0, off_fwd = 0;
    size_t sz_L = 0, sz_F = 0, sz_lmax = 0, sz_vec = 0, sz_fwd = 0;
    std::vector<NotchTab> tabs;   // [pass][level 1..L][axis 0: cH along -1, 1: cV along -2]
    DevBuf tw_buf, w_buf, scratch, varies;
    i64 cap = 0;
    // automatic clips: the work space of the estimate for `cap` tiles; the triples and the status of every tile of the last run
    // (clips_cap tiles); the log1p table of integer tiles
    DevBuf auto_buf, clips_buf, status_buf, table_buf;
    i64 clips_cap = 0, last_count = 0;
    int ncodes = 0;
    int au = 0;               // MI_PS_AUTO_* of the clips that are NaN
};

constexpr size_t kAutoBytesPerTile = MI_HIST_BINS * 8 + 8 + (MI_HIST_BINS + 1) * 4 + 2 * 4 + (MI_OTSU_MAX_CLASSES - 1) * 4 + 3 * 4;

// sizes, modes and the scratch layout: everything that needs no device
int derive(int ny_in, int nx_in, int in_dtype, const mi_pystripe_params& q, Plan& P) {
    MI_REQUIRE(ny_in > 0 && nx_in > 0, "mi_pystripe: tile of %d x %d", ny_in, nx_in);
    MI_REQUIRE(in_dtype >= MI_PS_U8 && in_dtype <= MI_PS_F32, "mi_pystripe: in_dtype %d (0 uint8, 1 uint16, 2 float32)", in_dtype);
    MI_REQUIRE(q.out_dtype >= MI_PS_U8 && q.out_dtype <= MI_PS_F32, "mi_pystripe: out_dtype %d (0 uint8, 1 uint16, 2 float32)", q.out_dtype);
    MI_REQUIRE(q.sigma1 >= 0 && q.sigma2 >= 0, "mi_pystripe: sigma (%g, %g) is negative", q.sigma1, q.sigma2);
    P.filter = q.sigma1 > 0 || q.sigma2 > 0;
    MI_REQUIRE(!P.filter || (q.sigma1 > 0 && q.sigma2 > 0), "np_notch: sigma must be positive (sigma = (%g, %g))", q.sigma1, q.sigma2);
    MI_REQUIRE(q.padding_mode >= MI_PS_REFLECT && q.padding_mode <= MI_PS_EDGE, "mi_pystripe: padding_mode %d", q.padding_mode);
    MI_REQUIRE(q.down_method >= MI_PS_DOWN_MAX && q.down_method <= MI_PS_DOWN_MEDIAN, "mi_pystripe: down_method %d", q.down_method);
    MI_REQUIRE(q.down_y >= 0 && q.down_x >= 0 && (q.down_y > 0) == (q.down_x > 0), "mi_pystripe: down_sample (%d, %d)", q.down_y, q.down_x);
    MI_REQUIRE(q.rotate == 0 || q.rotate == 90 || q.rotate == 180 || q.rotate == 270, "mi_pystripe: rotate %d (0, 90, 180, 270)", q.rotate);
    MI_REQUIRE(q.level >= 0 && q.level <= MI_PS_MAX_LEVELS, "mi_pystripe: level %d", q.level);
    MI_REQUIRE(!(q.convert_to_16bit && q.convert_to_8bit), "mi_pystripe: convert_to_16bit and convert_to_8bit are both set");
    MI_REQUIRE(!q.convert_to_8bit || (q.bit_shift >= 0 && q.bit_shift <= 8), "right shift should be between 0 and 8 (bit_shift_to_right = %d)",
               q.bit_shift);
    P.in_ny = ny_in; P.in_nx = nx_in; P.in_dtype = in_dtype; P.prm = q;
    mi_pystripe_info& I = P.info;
    std::memset(&I, 0, sizeof I);
    const bool down = q.down_y > 0;
    if (down && q.down_method == MI_PS_DOWN_MEDIAN && (i64)q.down_y * q.down_x > MI_PS_MEDIAN_MAX_BLOCK)
        return fail(MI_ERR_UNSUPPORTED, "mi_pystripe: median down_sample over blocks of %d x %d samples (at most %d samples per block)", q.down_y,
                    q.down_x, MI_PS_MEDIAN_MAX_BLOCK);
    P.pre = down || q.use_flat;
    I.ny = down ? (ny_in + q.down_y - 1) / q.down_y : ny_in;
    I.nx = down ? (nx_in + q.down_x - 1) / q.down_x : nx_in;
    I.integer_kind = in_dtype != MI_PS_F32 && !q.use_flat && !(down && (q.down_method == MI_PS_DOWN_MEAN || q.down_method == MI_PS_DOWN_MEDIAN));
    I.max_batch = q.max_batch > 0 ? q.max_batch : 16;
    // grid limits: rows go to gridDim.y, tiles (twice, in the column synthesis) to gridDim.z
    MI_REQUIRE(I.max_batch <= 16384, "mi_pystripe: max_batch %d (at most 16384 tiles per launch)", I.max_batch);
    P.bleach = q.bleach_frequency != 0;
    // a clip given as NaN is estimated per tile (without a bleach_frequency the three values are not looked at)
    const int au = !P.bleach ? 0 : (std::isnan(q.bleach_clip_min) ? MI_PS_AUTO_MIN : 0) | (std::isnan(q.bleach_clip_med) ? MI_PS_AUTO_MED : 0) |
                                       (std::isnan(q.bleach_clip_max) ? MI_PS_AUTO_MAX : 0);
    P.au = au;
    if (P.bleach) {
        MI_REQUIRE(q.bleach_frequency > 0 && q.bleach_frequency < 1, "mi_pystripe: bleach_frequency %g is not in (0, 1)", q.bleach_frequency);
        // the checks between given clips; an estimated one is checked on the device, tile by tile
        MI_REQUIRE((au & MI_PS_AUTO_MIN) || q.bleach_clip_min >= 0, "mi_pystripe: bleach_clip_min %g is negative", q.bleach_clip_min);
        MI_REQUIRE((au & (MI_PS_AUTO_MIN | MI_PS_AUTO_MED)) || q.bleach_clip_med > q.bleach_clip_min,
                   "mi_pystripe: bleach_clip_med %g is not above bleach_clip_min %g", q.bleach_clip_med, q.bleach_clip_min);
        MI_REQUIRE((au & (MI_PS_AUTO_MED | MI_PS_AUTO_MAX)) || q.bleach_clip_max > q.bleach_clip_med,
                   "mi_pystripe: bleach_clip_max %g is not above bleach_clip_med %g", q.bleach_clip_max, q.bleach_clip_med);
        MI_REQUIRE((au & (MI_PS_AUTO_MIN | MI_PS_AUTO_MAX)) || q.bleach_clip_max > q.bleach_clip_min,
                   "mi_pystripe: bleach_clip_max %g is not above bleach_clip_min %g", q.bleach_clip_max, q.bleach_clip_min);
        // sosfiltfilt's padlen: a filtered line has more than 6 samples
        MI_REQUIRE(I.nx > kBleachExt, "mi_pystripe: bleach correction filters rows of nx = %d samples (after down_sample); at least 7", I.nx);
        MI_REQUIRE(!q.bleach_max_method || I.ny > kBleachExt,
                   "mi_pystripe: bleach_max_method filters the column of ny = %d row maxima (after down_sample); at least 7", I.ny);
        const double k = std::tan(M_PI * q.bleach_frequency / 2.0);
        P.bq.b = k / (1.0 + k);
        P.bq.a = (1.0 - k) / (1.0 + k);
        P.bq.lo = (float)std::max(q.bleach_clip_min, std::log1p(1.0));
        P.bq.med = (float)q.bleach_clip_med;
        P.bq.hi = (float)q.bleach_clip_max;
        P.bq.clips = nullptr;
        P.ncodes = au && I.integer_kind ? (in_dtype == MI_PS_U8 ? 256 : 65536) : 0;
    }
    if (q.log_output) {
        MI_REQUIRE(P.filter || P.bleach, "mi_pystripe: log_output needs a stripe filter (sigma > 0) or the bleach correction");
        I.out_ny = I.ny; I.out_nx = I.nx; I.out_dtype = MI_PS_F32;
    } else {
        const bool swap = q.rotate == 90 || q.rotate == 270;
        I.out_ny = swap ? I.nx : I.ny;
        I.out_nx = swap ? I.ny : I.nx;
        I.out_dtype = q.out_dtype;
    }
    P.passes = !P.filter ? 0 : (q.sigma1 == q.sigma2 ? 1 : 2);
    size_t off = 0;
    auto take = [&off](size_t n) { const size_t o = off; off += (n + 3) / 4 * 4; return o; };
    if (P.pre) { P.sz_stage = (size_t)I.ny * I.nx; P.off_stage = take(P.sz_stage); }
    if (P.filter) {
        I.base_pad = pad_size(I.ny, I.nx, std::max(q.sigma1, q.sigma2));
        I.pad_y = I.ny % 2; I.pad_x = I.nx % 2;
        if (I.ny + 2 * I.base_pad + I.pad_y < kMinLength) I.pad_y = kMinLength - (I.ny + 2 * I.base_pad);
        if (I.nx + 2 * I.base_pad + I.pad_x < kMinLength) I.pad_x = kMinLength - (I.nx + 2 * I.base_pad);
        I.padded_ny = I.ny + 2 * I.base_pad + I.pad_y;
        I.padded_nx = I.nx + 2 * I.base_pad + I.pad_x;
        MI_REQUIRE((i64)I.padded_ny * I.padded_nx < (1ll << 31), "mi_pystripe: padded tile of %d x %d samples", I.padded_ny, I.padded_nx);
        MI_REQUIRE(I.padded_ny <= 65535, "mi_pystripe: padded tile of %d rows (at most 65535)", I.padded_ny);
        // the automatic level is 0 where a padded extent is below L - 1 (never for db9: 34 samples at least): wavedec2 then returns the
        // approximation alone and the filter leaves the log image as it is
        const int L = P.L;
        I.levels = q.level > 0 ? q.level : std::min(max_level(I.padded_ny, L), max_level(I.padded_nx, L));
        P.h[0] = I.padded_ny; P.w[0] = I.padded_nx;
        for (int l = 1; l <= I.levels; ++l) {
            P.h[l] = (P.h[l - 1] + L - 1) / 2;
            P.w[l] = (P.w[l - 1] + L - 1) / 2;
            I.coef_ny[l - 1] = P.h[l]; I.coef_nx[l - 1] = P.w[l];
            // a synthesis pair reads rows p .. p + L / 2 - 1 of a level: s = 2 m - L + 2 outputs need m >= L / 2, true for every
            // m = (n + L - 1) / 2 with n >= 1
            MI_REQUIRE(P.h[l] >= L / 2 && P.w[l] >= L / 2, "mi_pystripe: level %d has %d x %d coefficients", l, P.h[l], P.w[l]);
        }
        if (P.passes == 2 && I.levels) { P.sz_P = (size_t)P.h[0] * P.w[0]; P.off_P = take(P.sz_P); }
        // L / H of a level's analysis (h[l - 1] rows of w[l]); lo1 / hi1 of its synthesis (2 h[l] - L + 2 <= h[l - 1] + 1 rows).  The
        // first level is the largest while the extents are L - 1 or more; an explicit level on a shorter extent n GROWS it towards
        // L - 1 ((n + L - 1) / 2 > n), so the largest level is looked for.
        for (int l = 1; l <= I.levels; ++l) P.sz_row = std::max(P.sz_row, (size_t)(P.h[l - 1] + 1) * P.w[l]);
        if (I.levels) {
            P.off_rowL = take(P.sz_row);
            P.off_rowH = take(P.sz_row);
        }
        for (int l = 1; l <= I.levels; ++l) {
            // also holds the reconstruction of level l + 1: with m' = (m + L - 1) / 2, 2 m' - L + 2 <= m + 1 for every L
            P.sz_A[l] = (size_t)(P.h[l] + 1) * (P.w[l] + 1);
            P.sz_d[l] = (size_t)P.h[l] * P.w[l];
            P.off_A[l] = take(P.sz_A[l]);
            P.off_cH[l] = take(P.sz_d[l]);
            P.off_cV[l] = take(P.sz_d[l]);
            P.off_cD[l] = take(P.sz_d[l]);
        }
    }
    if (P.bleach) {
        const size_t npix = (size_t)I.ny * I.nx;
        const int longest = q.bleach_max_method ? std::max(I.ny, I.nx) : I.nx;
        I.bleach_long_rows = longest > MI_PS_BLEACH_LDS_ROW;
        if (P.filter) { P.sz_L = npix; P.off_L = take(P.sz_L); }
        if (q.bleach_max_method) {
            P.sz_vec = (size_t)I.ny + I.nx;
            P.off_key = take(P.sz_vec);
            P.off_vec = take(P.sz_vec);
            if (I.bleach_long_rows) P.sz_fwd = 2 * ((size_t)longest + 2 * kBleachExt);
        } else {
            P.sz_F = npix; P.off_F = take(P.sz_F);
            P.sz_lmax = (size_t)I.ny; P.off_lmax = take(P.sz_lmax);
            if (I.bleach_long_rows) P.sz_fwd = 2 * (size_t)I.ny * ((size_t)I.nx + 2 * kBleachExt);
        }
        P.off_M = take(1);
        if (P.sz_fwd) P.off_fwd = take(P.sz_fwd);
    }
    I.scratch_bytes_per_tile = off * sizeof(float);
    // the output conversion (:1361-1369)
    const int cur = I.integer_kind ? in_dtype : MI_PS_F32;
    if (!q.log_output) {
        if (q.convert_to_16bit && cur != MI_PS_U16)
            MI_REQUIRE(q.out_dtype == MI_PS_U16, "mi_pystripe: convert_to_16bit with out_dtype %d", q.out_dtype);
        else if (q.convert_to_8bit && cur != MI_PS_U8)
            MI_REQUIRE(q.out_dtype == MI_PS_U8, "mi_pystripe: convert_to_8bit with out_dtype %d", q.out_dtype);
    }
    return MI_OK;
}

int build_tables(Plan& P) {
    const mi_pystripe_info& I = P.info;
    std::vector<double2> tw;
    std::vector<float> wt;
    P.tabs.clear();
    for (int pass = 0; pass < P.passes; ++pass) {
        const double sigma = pass == 0 ? P.prm.sigma1 : P.prm.sigma2;
        for (int l = 1; l <= I.levels; ++l)
            for (int axis = 0; axis < 2; ++axis) {
                NotchTab t{};
                t.n = axis == 0 ? P.w[l] : P.h[l];
                // np_filter_coefficient :750: sigma' = coef.shape[axis + 1] * sigma / padded extent of the OTHER axis' count
                const double sp = axis == 0 ? P.h[l] * (sigma / I.padded_ny) : P.w[l] * (sigma / I.padded_nx);
                const float den = 2.0f * (float)(sp * sp);   // float32(2) * sigma ** 2 lands in float32 (np_notch :660)
                t.tw_off = tw.size();
                t.w_off = wt.size();
                for (int j = 0; j < t.n; ++j) {
                    const double a = 2.0 * M_PI * (double)j / (double)t.n;
                    tw.push_back(make_double2(std::cos(a), std::sin(a)));
                }
                t.kp = 0;
                for (int j = 0; j < t.n; ++j) {
                    const float jf = (float)j;
                    const float g = 1.0f - std::exp(-(jf * jf) / den);
                    const float wv = 1.0f - g;
                    wt.push_back(wv);
                    if (wv != 0.f) t.kp = j + 1;
                }
                t.kb = t.kp / 2 + 1;
                t.R = 0;
                for (int R : {4, 2, 1}) {
                    const size_t lds = round16((size_t)t.n * 16 + (size_t)R * t.kb * 16 + (size_t)R * t.n * 4);
                    // two blocks of four lines per CU (160 KB of LDS), three of two lines; one line when nothing else fits
                    if (lds <= (R == 4 ? 80u : R == 2 ? 53u : 160u) * 1024u) { t.R = R; t.lds = lds; break; }
                }
                if (!t.R)
                    return fail(MI_ERR_UNSUPPORTED, "mi_pystripe: a coefficient line of %d samples (sigma' = %g) does not fit the notch kernel's LDS",
                                t.n, sp);
                t.threads = std::min(512, std::max(64, (t.kb + 63) / 64 * 64));
                P.tabs.push_back(t);
            }
    }
    if (tw.empty()) return MI_OK;
    MI_TRY(P.tw_buf.alloc(tw.size() * sizeof(double2)));
    MI_TRY(P.w_buf.alloc(wt.size() * sizeof(float)));
    MI_HIP(hipMemcpy(P.tw_buf.p, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));
    MI_HIP(hipMemcpy(P.w_buf.p, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
    return MI_OK;
}

// The dynamic-LDS limit is an attribute of the kernel, not of a plan: it is set right before every launch that needs more than the
// default, to that launch's own need (several plans of different shapes live side by side in batch_filter).
template <int R>
int launch_notch(const Plan& P, hipStream_t st, const NotchTab& t, float* c, i64 tile_stride, int nlines, i64 es, i64 ls, int cnt) {
    const double2* tw = P.tw_buf.as<double2>() + t.tw_off;
    const float* wt = P.w_buf.as<float>() + t.w_off;
    if (t.lds > 48 * 1024)
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&notch_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds));
    hipLaunchKernelGGL(notch_kernel<R>, dim3(cdiv(nlines, R), cnt), dim3(t.threads), t.lds, st, c, tile_stride, t.n, nlines, es, ls, tw, wt, t.kp,
                       t.kb);
    return launch_check("notch_kernel");
}

int run_notch(const Plan& P, hipStream_t st, const NotchTab& t, float* c, i64 tile_stride, int nlines, i64 es, i64 ls, int cnt) {
    if (t.R == 4) return launch_notch<4>(P, st, t, c, tile_stride, nlines, es, ls, cnt);
    if (t.R == 2) return launch_notch<2>(P, st, t, c, tile_stride, nlines, es, ls, cnt);
    return launch_notch<1>(P, st, t, c, tile_stride, nlines, es, ls, cnt);
}

// sosfiltfilt of `lines` lines of n samples per tile.  The group: a chunk of about nine samples per thread, an odd number of them.
int launch_bleach_filter(const Plan& P, hipStream_t st, const Src& s, int n, int lines, float* F, i64 f_tile_stride, int f_row, float* lmax,
                         i64 lmax_tile_stride, double* fwd, i64 fwd_tile_stride, int cnt) {
    const int len = n + 2 * kBleachExt, cap = std::min(len, kBleachSeg);
    const int threads = std::min(kBleachMaxThreads, std::max(64, (cap / 9 + 63) / 64 * 64));
    const int chunk = ((cap + threads - 1) / threads) | 1;
    const size_t lds = (size_t)(cap + (cap & 1)) * sizeof(double) + kBleachTotals;
    if (lds > 48 * 1024)
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&bleach_filter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(bleach_filter_kernel, dim3(lines, cnt), dim3(threads), lds, st, s, n, kBleachSeg, chunk, P.bq, F, f_tile_stride, f_row, lmax,
                       lmax_tile_stride, len > kBleachSeg ? fwd : nullptr, fwd_tile_stride);
    return launch_check("bleach_filter_kernel");
}

// correct_bleaching on the log image behind `L` (the tile through log1p, or the stripe filter's stored result), into the sink
int run_bleach(Plan& P, hipStream_t st, const Src& L, const Sink& k, int cnt) {
    const mi_pystripe_info& I = P.info;
    float* sc = P.scratch.as<float>();
    const i64 cap = P.cap;
    auto buf = [&](size_t off) { return sc + (i64)off * cap; };
    float* M = buf(P.off_M);
    double* fwd = P.sz_fwd ? reinterpret_cast<double*>(buf(P.off_fwd)) : nullptr;
    const dim3 grid(cdiv(I.nx, 64), cdiv(I.ny, 4), cnt);
    if (P.prm.bleach_max_method) {
        unsigned* key = reinterpret_cast<unsigned*>(buf(P.off_key));
        float* vec = buf(P.off_vec);
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
        float* F = buf(P.off_F);
        float* lmax = buf(P.off_lmax);
        MI_TRY(launch_bleach_filter(P, st, L, I.nx, I.ny, F, (i64)P.sz_F, I.nx, lmax, (i64)P.sz_lmax, fwd, (i64)P.sz_fwd / 2, cnt));
        hipLaunchKernelGGL(bleach_tilemax_kernel, dim3(cnt), dim3(256), 0, st, lmax, I.ny, (const float*)nullptr, 0, (i64)P.sz_lmax, 0, M);
        MI_TRY(launch_check("bleach_tilemax_kernel"));
        hipLaunchKernelGGL(bleach_apply_kernel, grid, dim3(256), 0, st, L, F, (i64)P.sz_F, (const float*)nullptr, (const float*)nullptr, (i64)0, M, k);
    }
    return launch_check("bleach_apply_kernel");
}

// the dynamic-LDS limit of a kernel, raised to one launch's need (see launch_notch)
int raise_lds(const void* kernel, size_t lds) {
    if (lds > 48 * 1024) MI_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MI_OK;
}

// The four filters of the orthogonal wavelet with the reconstruction low-pass rec_lo[L] as float32, by the rule of make_filters(),
// each between kTabPad zeros: [lo_d | hi_d | lo_r | hi_r], L + 2 kTabPad floats each.
int upload_filter_table(Plan& P, const double* rec_lo) {
    const int L = P.L, TS = L + 2 * kTabPad;
    std::vector<float> t(4 * (size_t)TS, 0.f);
    for (int i = 0; i < L; ++i) {
        const float lo_r = (float)rec_lo[i], hi_r = (float)(rec_lo[L - 1 - i] * ((i & 1) ? -1.0 : 1.0));   // qmf
        t[2 * TS + kTabPad + i] = lo_r;
        t[3 * TS + kTabPad + i] = hi_r;
        t[0 * TS + kTabPad + (L - 1 - i)] = lo_r;
        t[1 * TS + kTabPad + (L - 1 - i)] = hi_r;
    }
    MI_TRY(P.tab_buf.alloc(t.size() * sizeof(float)));
    MI_HIP(hipMemcpy(P.tab_buf.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    return MI_OK;
}

// the log1p table of an integer tile's automatic clips: the caller's, or libm's log1pf of every code
int upload_log_table(Plan& P, const float* table) {
    if (!P.ncodes) return MI_OK;
    std::vector<float> own;
    if (!table) {
        own.resize((size_t)P.ncodes);
        for (int c = 0; c < P.ncodes; ++c) own[(size_t)c] = log1pf((float)c);
        table = own.data();
    }
    if (!P.table_buf.p) MI_TRY(P.table_buf.alloc(sizeof(float) * (size_t)P.ncodes));
    MI_HIP(hipMemcpy(P.table_buf.p, table, sizeof(float) * (size_t)P.ncodes, hipMemcpyHostToDevice));
    return MI_OK;
}

int check_taps(const char* who, int taps) {
    MI_REQUIRE(taps >= 2 && taps <= MI_PS_MAX_TAPS && taps % 2 == 0, "%s: wavelet of %d taps (an even number, 2 .. %d)", who, taps, MI_PS_MAX_TAPS);
    return MI_OK;
}

// The clips of the cnt tiles behind `src` (the tile after flat and down_sample, not yet in the log domain) into clips[cnt][3] and
// status[cnt]: range, edges, histogram, search, triple.  Everything stays on the stream.
int run_auto_clips(Plan& P, hipStream_t st, Src src, int cnt, int* varies, float* clips, int* status) {
    const mi_pystripe_info& I = P.info;
    const mi_pystripe_params& q = P.prm;
    char* base = P.auto_buf.as<char>();
    const size_t cap = (size_t)P.cap;
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(base);
    unsigned long long* work = counts + MI_HIST_BINS * cap;
    float* edges = reinterpret_cast<float*>(work + cap);
    unsigned* keys = reinterpret_cast<unsigned*>(edges + (MI_HIST_BINS + 1) * cap);
    int* indices = reinterpret_cast<int*>(keys + 2 * cap);
    int* nonfinite = indices + (MI_OTSU_MAX_CLASSES - 1) * cap;
    int* nvalues = nonfinite + cap;
    int* otsu_status = nvalues + cap;
    const float* table = nullptr;
    if (I.integer_kind) table = P.table_buf.as<float>();
    else src.logp = 1;
    MI_TRY(hist_init_launch(st, keys, nonfinite, counts, cnt));
    const dim3 grid((unsigned)std::min(I.ny, 256), cnt);   // rows over the groups of a tile: few groups, few same-address atomics at the end
    hipLaunchKernelGGL(auto_range_kernel, grid, dim3(256), 0, st, src, table, P.ncodes, keys, nonfinite);
    MI_TRY(launch_check("auto_range_kernel"));
    MI_TRY(hist_edges_launch(st, keys, edges, cnt));
    hipLaunchKernelGGL(auto_hist_kernel, grid, dim3(256), 0, st, src, table, P.ncodes, edges, nonfinite, counts);
    MI_TRY(launch_check("auto_hist_kernel"));
    MI_TRY(multiotsu_launch(st, counts, cnt, MI_OTSU_MAX_CLASSES, indices, nvalues, otsu_status, work));
    hipLaunchKernelGGL(auto_clips_kernel, dim3(cdiv((size_t)cnt, 64)), dim3(64), 0, st, cnt, P.au, (float)q.bleach_clip_min,
                       (float)q.bleach_clip_med, (float)q.bleach_clip_max, std::log1p(1.0), edges, indices, otsu_status, nonfinite,
                       !q.keep_uniform && !q.log_output, varies, clips, status);
    return launch_check("auto_clips_kernel");
}

int run_chunk(Plan& P, hipStream_t st, const void* in, const float* flat, void* out, int cnt, i64 t0) {
    const mi_pystripe_info& I = P.info;
    const mi_pystripe_params& q = P.prm;
    float* sc = P.scratch.as<float>();
    const i64 cap = P.cap;
    auto buf = [&](size_t off) { return sc + (i64)off * cap; };   // buffer b of all tiles: [tile][size_b]
    int* varies = P.varies.as<int>();
    const i64 npix = (i64)P.in_ny * P.in_nx;
    MI_HIP(hipMemsetAsync(varies, q.keep_uniform ? 1 : 0, sizeof(int) * (size_t)cnt, st));
    if (!q.keep_uniform && !q.log_output) {
        if (P.in_dtype == MI_PS_U16) MI_TRY(launch_uniform<uint16_t>(st, in, npix, cnt, varies));
        else if (P.in_dtype == MI_PS_U8) MI_TRY(launch_uniform<uint8_t>(st, in, npix, cnt, varies));
        else MI_TRY(launch_uniform<float>(st, in, npix, cnt, varies));
    }
    Src src{in, npix, P.in_dtype, P.in_ny, P.in_nx, P.in_nx, 0, MAP_IDENTITY, 0};
    if (P.pre) {
        const int by = q.down_y > 0 ? q.down_y : 1, bx = q.down_x > 0 ? q.down_x : 1;
        const dim3 grid(cdiv(I.nx, 64), cdiv(I.ny, 4), cnt);
        const float* fl = q.use_flat ? flat : nullptr;
        if (q.down_y > 0 && q.down_method == MI_PS_DOWN_MEDIAN) {
            const int n = by * bx;
            if (n <= 4) MI_TRY(launch_pre_median<4>(st, grid, src, fl, by, bx, buf(P.off_stage), I.ny, I.nx));
            else if (n <= 8) MI_TRY(launch_pre_median<8>(st, grid, src, fl, by, bx, buf(P.off_stage), I.ny, I.nx));
            else if (n <= 16) MI_TRY(launch_pre_median<16>(st, grid, src, fl, by, bx, buf(P.off_stage), I.ny, I.nx));
            else if (n <= 32) MI_TRY(launch_pre_median<32>(st, grid, src, fl, by, bx, buf(P.off_stage), I.ny, I.nx));
            else MI_TRY(launch_pre_median<64>(st, grid, src, fl, by, bx, buf(P.off_stage), I.ny, I.nx));
        } else {
            hipLaunchKernelGGL(pre_kernel, grid, dim3(256), 0, st, src, fl, by, bx, q.down_method, buf(P.off_stage), I.ny, I.nx);
            MI_TRY(launch_check("pre_kernel"));
        }
        src = Src{buf(P.off_stage), (i64)P.sz_stage, MI_PS_F32, I.ny, I.nx, I.nx, 0, MAP_IDENTITY, 0};
    }
    Sink k{};
    if (P.au) {
        float* clips = P.clips_buf.as<float>() + 3 * t0;
        int* status = P.status_buf.as<int>() + t0;
        MI_TRY(run_auto_clips(P, st, src, cnt, varies, clips, status));
        P.bq.clips = clips;
        k.clip_status = status;
    }
    k.out = out;
    k.tile_stride = (i64)I.out_ny * I.out_nx;
    k.ny = I.ny; k.nx = I.nx; k.pad = I.base_pad;
    k.filtered = P.filter || P.bleach; k.log_out = q.log_output; k.integer_kind = I.integer_kind;
    k.in_max = P.in_dtype == MI_PS_U8 ? 255.f : 65535.f;
    k.dark = q.dark;
    const int cur = I.integer_kind ? P.in_dtype : MI_PS_F32;
    k.out_dtype = I.out_dtype;
    if (q.convert_to_16bit && cur != MI_PS_U16) { k.mode = OUT_CLIPCAST; k.cast_max = 65535.f; }
    else if (q.convert_to_8bit && cur != MI_PS_U8) { k.mode = OUT_TO8; k.shift = q.bit_shift; }
    else if (I.out_dtype != MI_PS_F32) { k.mode = OUT_CLIPCAST; k.cast_max = I.out_dtype == MI_PS_U8 ? 255.f : 65535.f; }
    else k.mode = OUT_FLOAT;
    k.flip = q.flip_upside_down; k.rot = q.rotate / 90;
    k.varies = varies;
    if (!P.filter || I.levels == 0) {
        if (P.filter) src.logp = 1;   // no wavelet level: the filter's result is log1p of the tile
        if (P.bleach) {
            src.logp = 1;   // L is log1p on load: no log image is written
            return run_bleach(P, st, src, k, cnt);
        }
        const dim3 grid(cdiv(I.nx, 64), cdiv(I.ny, 4), cnt);
        hipLaunchKernelGGL(point_kernel, grid, dim3(256), 0, st, src, k);
        return launch_check("point_kernel");
    }
    // with the bleach correction behind it, the last synthesis level stores the log image; the correction feeds the real sink
    Sink kL = k;
    if (P.bleach) {
        kL.out = buf(P.off_L);
        kL.tile_stride = (i64)P.sz_L;
        kL.log_out = 1;
        kL.clip_status = nullptr;
    }
    const int Lv = I.levels, LT = P.L;
    const float* tab = P.tab_buf.as<float>();
    for (int pass = 0; pass < P.passes; ++pass) {
        // analysis
        for (int l = 1; l <= Lv; ++l) {
            Src s;
            int rows, map_mode = MAP_IDENTITY, map_pad = 0, map_rows = P.h[l - 1];
            if (l == 1 && pass == 0) {
                s = src;
                s.pad = I.base_pad; s.mode = q.padding_mode; s.logp = 1;
                rows = I.ny;
                map_mode = q.padding_mode; map_pad = I.base_pad; map_rows = I.ny;
            } else if (l == 1) {
                s = Src{buf(P.off_P), (i64)P.sz_P, MI_PS_F32, P.h[0], P.w[0], P.w[0], 0, MAP_IDENTITY, 0};
                rows = P.h[0];
            } else {
                s = Src{buf(P.off_A[l - 1]), (i64)P.sz_A[l - 1], MI_PS_F32, P.h[l - 1], P.w[l - 1], P.w[l - 1], 0, MAP_IDENTITY, 0};
                rows = P.h[l - 1];
            }
            const int n = P.w[l - 1], m = P.w[l];
            if (P.generic) {
                hipLaunchKernelGGL(ana_rows_gen_kernel, dim3(cdiv(m, kRowBlock), rows, cnt), dim3(kRowBlock), 0, st, s, n, m, buf(P.off_rowL),
                                   buf(P.off_rowH), (i64)P.sz_row, tab, LT);
                MI_TRY(launch_check("ana_rows_gen_kernel"));
                const size_t lds = (size_t)(2 * kColRows + LT - 2) * 64 * 2 * sizeof(float);
                MI_TRY(raise_lds(reinterpret_cast<const void*>(&ana_cols_gen_kernel), lds));
                hipLaunchKernelGGL(ana_cols_gen_kernel, dim3(cdiv(m, 64), cdiv(P.h[l], kColRows), cnt), dim3(256), lds, st, buf(P.off_rowL),
                                   buf(P.off_rowH), (i64)P.sz_row, P.h[l - 1], P.h[l], m, map_pad, map_rows, map_mode, buf(P.off_A[l]),
                                   (i64)P.sz_A[l], buf(P.off_cH[l]), buf(P.off_cV[l]), buf(P.off_cD[l]), (i64)P.sz_d[l], tab, LT);
                MI_TRY(launch_check("ana_cols_gen_kernel"));
                continue;
            }
            hipLaunchKernelGGL(ana_rows_kernel, dim3(cdiv(m, kRowBlock), rows, cnt), dim3(kRowBlock), 0, st, s, n, m, buf(P.off_rowL),
                               buf(P.off_rowH), (i64)P.sz_row, P.f);
            MI_TRY(launch_check("ana_rows_kernel"));
            hipLaunchKernelGGL(ana_cols_kernel, dim3(cdiv(m, 64), cdiv(P.h[l], 4), cnt), dim3(256), 0, st, buf(P.off_rowL), buf(P.off_rowH),
                               (i64)P.sz_row, P.h[l - 1], P.h[l], m, map_pad, map_rows, map_mode, buf(P.off_A[l]), (i64)P.sz_A[l],
                               buf(P.off_cH[l]), buf(P.off_cV[l]), buf(P.off_cD[l]), (i64)P.sz_d[l], P.f);
            MI_TRY(launch_check("ana_cols_kernel"));
        }
        // notch
        for (int l = 1; l <= Lv; ++l) {
            const NotchTab* t = &P.tabs[((size_t)pass * Lv + (l - 1)) * 2];
            MI_TRY(run_notch(P, st, t[0], buf(P.off_cH[l]), (i64)P.sz_d[l], P.h[l], 1, P.w[l], cnt));
            if (q.bidirectional) MI_TRY(run_notch(P, st, t[1], buf(P.off_cV[l]), (i64)P.sz_d[l], P.w[l], P.w[l], 1, cnt));
        }
        // synthesis, deepest level first; the reconstruction of level l lands in A[l - 1]'s buffer
        const bool last_pass = pass == P.passes - 1;
        for (int l = Lv; l >= 1; --l) {
            const int m0 = P.h[l], m1 = P.w[l], s0 = 2 * m0 - LT + 2, s1 = 2 * m1 - LT + 2;
            const float* a = buf(P.off_A[l]);
            const int a_stride = l == Lv ? m1 : 2 * P.w[l + 1] - LT + 2;
            const bool fin = l == 1 && last_pass;
            int y0 = 0, y1 = s0, xp0 = 0, xp1 = s1 / 2;
            if (fin) {
                y0 = I.base_pad; y1 = I.base_pad + I.ny;
                xp0 = I.base_pad / 2; xp1 = (I.base_pad + I.nx + 1) / 2;
            }
            const int p0 = y0 / 2, p1 = (y1 + 1) / 2;
            if (P.generic) {
                const size_t lds = (size_t)(kColPairs + LT / 2 - 1) * 64 * 2 * sizeof(float);
                MI_TRY(raise_lds(reinterpret_cast<const void*>(&syn_cols_gen_kernel), lds));
                hipLaunchKernelGGL(syn_cols_gen_kernel, dim3(cdiv(m1, 64), cdiv(p1 - p0, kColPairs), 2 * cnt), dim3(256), lds, st, a, (i64)P.sz_A[l],
                                   a_stride, buf(P.off_cH[l]), buf(P.off_cV[l]), buf(P.off_cD[l]), (i64)P.sz_d[l], m1, m0, p0, p1, s0,
                                   buf(P.off_rowL), buf(P.off_rowH), (i64)P.sz_row, tab, LT);
                MI_TRY(launch_check("syn_cols_gen_kernel"));
                const dim3 grid(cdiv(xp1 - xp0, 256), y1 - y0, cnt);
                if (fin) {
                    hipLaunchKernelGGL(syn_rows_gen_kernel<true>, grid, dim3(256), 0, st, buf(P.off_rowL), buf(P.off_rowH), (i64)P.sz_row, m1, y0,
                                       xp0, xp1, s1, (float*)nullptr, (i64)0, kL, tab, LT);
                } else {
                    float* dst = l == 1 ? buf(P.off_P) : buf(P.off_A[l - 1]);
                    const i64 dst_stride = l == 1 ? (i64)P.sz_P : (i64)P.sz_A[l - 1];
                    hipLaunchKernelGGL(syn_rows_gen_kernel<false>, grid, dim3(256), 0, st, buf(P.off_rowL), buf(P.off_rowH), (i64)P.sz_row, m1, y0,
                                       xp0, xp1, s1, dst, dst_stride, kL, tab, LT);
                }
                MI_TRY(launch_check("syn_rows_gen_kernel"));
                continue;
            }
            hipLaunchKernelGGL(syn_cols_kernel, dim3(cdiv(m1, 64), cdiv(p1 - p0, 4), 2 * cnt), dim3(256), 0, st, a, (i64)P.sz_A[l], a_stride,
                               buf(P.off_cH[l]), buf(P.off_cV[l]), buf(P.off_cD[l]), (i64)P.sz_d[l], m1, p0, p1, s0, buf(P.off_rowL),
                               buf(P.off_rowH), (i64)P.sz_row, P.f);
            MI_TRY(launch_check("syn_cols_kernel"));
            const dim3 grid(cdiv(xp1 - xp0, 256), y1 - y0, cnt);
            if (fin) {
                hipLaunchKernelGGL(syn_rows_kernel<true>, grid, dim3(256), 0, st, buf(P.off_rowL), buf(P.off_rowH), (i64)P.sz_row, m1, y0, xp0, xp1,
                                   s1, (float*)nullptr, (i64)0, kL, P.f);
            } else {
                float* dst = l == 1 ? buf(P.off_P) : buf(P.off_A[l - 1]);
                const i64 dst_stride = l == 1 ? (i64)P.sz_P : (i64)P.sz_A[l - 1];
                hipLaunchKernelGGL(syn_rows_kernel<false>, grid, dim3(256), 0, st, buf(P.off_rowL), buf(P.off_rowH), (i64)P.sz_row, m1, y0, xp0, xp1,
                                   s1, dst, dst_stride, kL, P.f);
            }
            MI_TRY(launch_check("syn_rows_kernel"));
        }
    }
    if (P.bleach)
        return run_bleach(P, st, Src{buf(P.off_L), (i64)P.sz_L, MI_PS_F32, I.ny, I.nx, I.nx, 0, MAP_IDENTITY, 0}, k, cnt);
    return MI_OK;
}

}  // namespace
}  // namespace mi

using mi::Plan;

extern "C" int mi_pystripe_pad_size(int ny, int nx, double sigma) {
    if (ny <= 0 || nx <= 0 || sigma < 0) return mi::fail(MI_ERR_INVALID, "mi_pystripe_pad_size: shape (%d, %d), sigma %g", ny, nx, sigma);
    return mi::pad_size(ny, nx, sigma);
}

extern "C" int mi_pystripe_derive(int ny, int nx, int in_dtype, const mi_pystripe_params* params, mi_pystripe_info* info) {
    MI_REQUIRE(params && info, "mi_pystripe_derive: null pointer");
    Plan P;
    MI_TRY(mi::derive(ny, nx, in_dtype, *params, P));
    *info = P.info;
    return MI_OK;
}

extern "C" int mi_pystripe_plan_create(int dev, int ny, int nx, int in_dtype, const mi_pystripe_params* params, void** plan) {
    MI_REQUIRE(params && plan, "mi_pystripe_plan_create: null pointer");
    *plan = nullptr;
    MI_TRY(mi::use_device(dev));
    Plan* P = new Plan;
    P->dev = dev;
    P->f = mi::make_filters();
    int rc = mi::derive(ny, nx, in_dtype, *params, *P);
    if (rc == MI_OK) rc = mi::build_tables(*P);
    if (rc == MI_OK) rc = mi::upload_log_table(*P, nullptr);
    if (rc != MI_OK) {
        delete P;
        return rc;
    }
    *plan = P;
    return MI_OK;
}

extern "C" int mi_pystripe_derive_wavelet(int ny, int nx, int in_dtype, const mi_pystripe_params* params, int taps, mi_pystripe_info* info) {
    MI_REQUIRE(params && info, "mi_pystripe_derive_wavelet: null pointer");
    MI_TRY(mi::check_taps("mi_pystripe_derive_wavelet", taps));
    Plan P;
    P.L = taps;
    P.generic = true;
    MI_TRY(mi::derive(ny, nx, in_dtype, *params, P));
    *info = P.info;
    return MI_OK;
}

extern "C" int mi_pystripe_plan_create_wavelet(int dev, int ny, int nx, int in_dtype, const mi_pystripe_params* params, const double* rec_lo,
                                               int taps, void** plan) {
    MI_REQUIRE(params && plan && rec_lo, "mi_pystripe_plan_create_wavelet: null pointer");
    *plan = nullptr;
    MI_TRY(mi::check_taps("mi_pystripe_plan_create_wavelet", taps));
    // orthonormal under double shifts: what the quadrature-mirror construction of the other three filters needs
    for (int i = 0; i < taps; ++i) MI_REQUIRE(std::isfinite(rec_lo[i]), "mi_pystripe_plan_create_wavelet: rec_lo[%d] is not finite", i);
    double worst = 0.0;
    for (int k = 0; 2 * k < taps; ++k) {
        double sum = 0.0;
        for (int i = 0; i + 2 * k < taps; ++i) sum += rec_lo[i] * rec_lo[i + 2 * k];
        worst = std::max(worst, std::fabs(sum - (k == 0 ? 1.0 : 0.0)));
    }
    MI_REQUIRE(worst <= 1e-6, "mi_pystripe_plan_create_wavelet: rec_lo is not the low-pass of an orthogonal wavelet (residual %g, allowed 1e-6)",
               worst);
    MI_TRY(mi::use_device(dev));
    Plan* P = new Plan;
    P->dev = dev;
    P->L = taps;
    P->generic = true;
    int rc = mi::derive(ny, nx, in_dtype, *params, *P);
    if (rc == MI_OK) rc = mi::build_tables(*P);
    if (rc == MI_OK) rc = mi::upload_filter_table(*P, rec_lo);
    if (rc == MI_OK) rc = mi::upload_log_table(*P, nullptr);
    if (rc != MI_OK) {
        delete P;
        return rc;
    }
    *plan = P;
    return MI_OK;
}

extern "C" int mi_pystripe_plan_destroy(void* plan) {
    if (!plan) return MI_OK;
    Plan* P = static_cast<Plan*>(plan);
    const int rc = mi::use_device(P->dev);
    delete P;
    return rc;
}

extern "C" int mi_pystripe_plan_info(void* plan, mi_pystripe_info* info) {
    MI_REQUIRE(plan && info, "mi_pystripe_plan_info: null pointer");
    *info = static_cast<Plan*>(plan)->info;
    return MI_OK;
}

extern "C" int mi_pystripe_plan_set_log_table(void* plan, const float* table, int ncodes) {
    MI_REQUIRE(plan && table, "mi_pystripe_plan_set_log_table: null pointer");
    Plan& P = *static_cast<Plan*>(plan);
    MI_REQUIRE(P.ncodes > 0, "mi_pystripe_plan_set_log_table: the plan estimates no clips of an integer tile");
    MI_REQUIRE(ncodes == P.ncodes, "mi_pystripe_plan_set_log_table: %d codes, the plan's tiles have %d", ncodes, P.ncodes);
    MI_TRY(mi::use_device(P.dev));
    MI_HIP(hipDeviceSynchronize());   // a run that reads the table may still be under way
    return mi::upload_log_table(P, table);
}

extern "C" int mi_pystripe_plan_clips(void* plan, float* clips_host, int* status_host, int n) {
    MI_REQUIRE(plan, "mi_pystripe_plan_clips: null pointer");
    Plan& P = *static_cast<Plan*>(plan);
    MI_REQUIRE(P.bleach, "mi_pystripe_plan_clips: the plan has no bleach correction");
    MI_REQUIRE(n >= 0 && n <= P.last_count, "mi_pystripe_plan_clips: %d tiles, the last run had %lld", n, (long long)P.last_count);
    if (n == 0) return MI_OK;
    if (!P.au) {
        for (int t = 0; t < n; ++t) {
            if (clips_host) { clips_host[3 * t] = P.bq.lo; clips_host[3 * t + 1] = P.bq.med; clips_host[3 * t + 2] = P.bq.hi; }
            if (status_host) status_host[t] = MI_PS_CLIPS_OK;
        }
        return MI_OK;
    }
    MI_TRY(mi::use_device(P.dev));
    if (clips_host) MI_HIP(hipMemcpy(clips_host, P.clips_buf.p, 3 * sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    if (status_host) MI_HIP(hipMemcpy(status_host, P.status_buf.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_pystripe_run(void* plan, void* stream, const void* in, const void* flat, void* out, int64_t count) {
    MI_REQUIRE(plan && in && out, "mi_pystripe_run: null pointer");
    MI_REQUIRE(count >= 0, "mi_pystripe_run: count %lld", (long long)count);
    Plan& P = *static_cast<Plan*>(plan);
    MI_REQUIRE(!P.prm.use_flat || flat, "mi_pystripe_run: the plan divides by a flat field and none is given");
    if (count == 0) return MI_OK;
    MI_TRY(mi::use_device(P.dev));
    hipStream_t st = mi::as_stream(stream);
    const int64_t want = std::min<int64_t>(count, P.info.max_batch);
    if (want > P.cap) {
        // work of an earlier call may still use the smaller scratch
        MI_HIP(hipStreamSynchronize(st));
        P.cap = 0;
        MI_TRY(P.scratch.alloc(std::max<size_t>(P.info.scratch_bytes_per_tile * (size_t)want, 16)));
        MI_TRY(P.varies.alloc(sizeof(int) * (size_t)want));
        if (P.au) MI_TRY(P.auto_buf.alloc(mi::kAutoBytesPerTile * (size_t)want));
        P.cap = want;
    }
    if (P.au && count > P.clips_cap) {
        MI_HIP(hipStreamSynchronize(st));
        P.clips_cap = 0;
        MI_TRY(P.clips_buf.alloc(3 * sizeof(float) * (size_t)count));
        MI_TRY(P.status_buf.alloc(sizeof(int) * (size_t)count));
        P.clips_cap = count;
    }
    P.last_count = count;
    const size_t in_bytes = (size_t)P.in_ny * P.in_nx * (P.in_dtype == MI_PS_U8 ? 1 : P.in_dtype == MI_PS_U16 ? 2 : 4);
    const size_t out_bytes = (size_t)P.info.out_ny * P.info.out_nx * (P.info.out_dtype == MI_PS_U8 ? 1 : P.info.out_dtype == MI_PS_U16 ? 2 : 4);
    for (int64_t t0 = 0; t0 < count; t0 += P.cap) {
        const int cnt = (int)std::min<int64_t>(P.cap, count - t0);
        MI_TRY(mi::run_chunk(P, st, static_cast<const char*>(in) + (size_t)t0 * in_bytes, static_cast<const float*>(flat),
                             static_cast<char*>(out) + (size_t)t0 * out_bytes, cnt, t0));
    }
    return MI_OK;
}
