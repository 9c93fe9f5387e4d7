// pystripe's value padding modes (pystripe_internal.h: pad): numpy.pad's constant, linear_ramp, maximum, minimum, mean and median
// on the log image.  A padded sample of these modes is no copy of a source sample, so the padded image is written once (into the
// buffer a two-pass plan keeps anyway) and the first analysis level reads it like the image a first pass left.
#include <algorithm>
#include <cmath>

#include "pystripe_internal.h"

namespace mi {
namespace ps {
namespace {

constexpr int kStatWaves = 16;                 // waves of a statistics work-group: wave w takes rows w, w + 16, ... of 64 columns
constexpr int kSelHist = 256, kSelCtl = 16;    // the selection's LDS in front of the keys: digit counts, then the chosen bin
static_assert((size_t)(kSelHist + kSelCtl + MI_PS_PAD_LDS_LINE) * sizeof(unsigned) == 160 * 1024 / 4,
              "MI_PS_PAD_LDS_LINE is derived from a quarter of a CU's LDS");

// max / min / sum, all carried in double (a float converts exactly): one code path for the three statistics
__device__ __forceinline__ double stat_neutral(int mode) { return mode == MI_PS_MAXIMUM ? -INFINITY : mode == MI_PS_MINIMUM ? INFINITY : 0.0; }
__device__ __forceinline__ double stat_join(int mode, double a, double b) {
    return mode == MI_PS_MAXIMUM ? fmax(a, b) : mode == MI_PS_MINIMUM ? fmin(a, b) : a + b;
}
__device__ __forceinline__ float stat_finish(int mode, double a, int n) { return mode == MI_PS_MEAN ? (float)(a / (double)n) : (float)a; }

// One pass over the tile: a work-group takes 64 columns over all rows.  A thread carries its column; a wave reduces its 64 samples
// of a row to one partial per (row, column block).  Every order is fixed, so a tile's statistics do not depend on the batch.
__global__ void __launch_bounds__(64 * kStatWaves) pad_stats_kernel(Src s, int mode, double* part, i64 part_ts, int ncb, float* vec, i64 vec_ts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* sh = reinterpret_cast<double*>(smem);   // [kStatWaves][64]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cb = blockIdx.x, x = cb * 64 + lane;
    const i64 tile = blockIdx.y;
    const bool in = x < s.nx;
    const double none = stat_neutral(mode);
    double col = none;
    for (int y = w; y < s.ny; y += kStatWaves) {   // uniform over the wave
        const double v = in ? (double)src_load(s, tile, y, x) : none;
        col = stat_join(mode, col, v);
        double r = v;
        for (int d = 32; d >= 1; d >>= 1) r = stat_join(mode, r, __shfl_xor(r, d));
        if (lane == 0) part[tile * part_ts + (i64)y * ncb + cb] = r;
    }
    sh[w * 64 + lane] = col;
    __syncthreads();
    if (w == 0 && in) {
        double c = sh[lane];
        for (int k = 1; k < kStatWaves; ++k) c = stat_join(mode, c, sh[k * 64 + lane]);
        vec[tile * vec_ts + s.ny + x] = stat_finish(mode, c, s.ny);
    }
}

// the row statistics from their partials, column block by column block
__global__ void __launch_bounds__(256) pad_rows_kernel(const double* part, i64 part_ts, int ncb, int mode, int ny, int nx, float* vec, i64 vec_ts) {
    const int y = blockIdx.x * 256 + threadIdx.x;
    const i64 tile = blockIdx.y;
    if (y >= ny) return;
    const double* p = part + tile * part_ts + (i64)y * ncb;
    double r = p[0];
    for (int cb = 1; cb < ncb; ++cb) r = stat_join(mode, r, p[cb]);
    vec[tile * vec_ts + y] = stat_finish(mode, r, nx);
}

// the corner: the statistic of the column statistics (axis 1 pads the rows axis 0 has made).  One work-group per tile.
__global__ void __launch_bounds__(256) pad_corner_kernel(int mode, int ny, int nx, float* vec, i64 vec_ts) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    float* v = vec + (i64)blockIdx.x * vec_ts;
    const float* c = v + ny;
    double a = stat_neutral(mode);
    for (int i = t; i < nx; i += 256) a = stat_join(mode, a, (double)c[i]);
    sh[t] = a;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) sh[t] = stat_join(mode, sh[t], sh[t + d]);
        __syncthreads();
    }
    if (t == 0) v[ny + nx] = stat_finish(mode, sh[0], nx);
}

// numpy.median of one line per work-group: the sample of rank n / 2 by a radix selection, most significant byte first, over the
// order-preserving keys; an even count adds the largest key below it (or the same key again, when it ties) and takes the float32
// mean of the two.  STAGED: the keys of the line stay in LDS; else every pass reads the line again through src_load.
// along_x: line = row `line` of s; else column `line`.
template <bool STAGED>
__global__ void __launch_bounds__(256) pad_median_kernel(Src s, int along_x, int n, float* out, i64 out_ts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* hist = reinterpret_cast<unsigned*>(smem);
    unsigned* ctl = hist + kSelHist;
    unsigned* keys = ctl + kSelCtl;
    const int line = blockIdx.x, t = threadIdx.x;
    const i64 tile = blockIdx.y;
    auto fresh = [&](int i) { return float_key(along_x ? src_load(s, tile, line, i) : src_load(s, tile, i, line)); };
    auto key_at = [&](int i) { return STAGED ? keys[i] : fresh(i); };
    if (STAGED)
        for (int i = t; i < n; i += 256) keys[i] = fresh(i);
    unsigned prefix = 0, mask = 0;
    int rank = n / 2, below = 0;   // rank among the keys that share the prefix; keys below all of those
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        for (int i = t; i < n; i += 256) {
            const unsigned k = key_at(i);
            if ((k & mask) == prefix) histdev::wave_count(hist, (int)((k >> shift) & 255u));
        }
        __syncthreads();
        if (t < 64) {
            // the bin that holds the rank, by the first wave: four bins per lane, a scan over the lanes, then the lane that owns it.
            // rank is below the count of the keys that share the prefix, so exactly one lane does
            const unsigned r = (unsigned)rank, h0 = hist[4 * t], h1 = hist[4 * t + 1], h2 = hist[4 * t + 2], h3 = hist[4 * t + 3];
            const unsigned own = h0 + h1 + h2 + h3;
            unsigned upto = own;
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = (unsigned)__shfl_up((int)upto, d);
                if (t >= d) upto += v;
            }
            unsigned c = upto - own;
            if (c <= r && r < upto) {
                int b = 4 * t;
                if (c + h0 <= r) {
                    c += h0; ++b;
                    if (c + h1 <= r) {
                        c += h1; ++b;
                        if (c + h2 <= r) { c += h2; ++b; }
                    }
                }
                ctl[0] = (unsigned)b;
                ctl[1] = c;
            }
        }
        __syncthreads();
        prefix |= ctl[0] << shift;
        mask |= 255u << shift;
        rank -= (int)ctl[1];
        below += (int)ctl[1];
    }
    const float hi = key_float(prefix);
    float lo = hi;
    if (n % 2 == 0 && below == n / 2) {   // uniform over the work-group: the lower middle sample is the largest key below
        unsigned m = 0;
        for (int i = t; i < n; i += 256) {
            const unsigned k = key_at(i);
            if (k < prefix) m = max(m, k);
        }
        for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d));
        __syncthreads();   // everyone has read ctl
        if ((t & 63) == 0) ctl[t >> 6] = m;
        __syncthreads();
        lo = key_float(max(max(ctl[0], ctl[1]), max(ctl[2], ctl[3])));
    }
    if (t == 0) out[tile * out_ts + line] = (n & 1) ? hi : (lo + hi) * 0.5f;
}

// numpy.linspace(0, edge, p, endpoint=False)[k]
__device__ __forceinline__ float ramp(float edge, int k, int p) { return (float)((double)edge * (double)k / (double)p); }

// the padded log image: bp samples in front of the tile, bp + py (bp + px) behind it.  Axis 0 is padded first, then axis 1 over
// all rows, the new ones included: a corner ramps the ramped edge, and holds the statistic of the column statistics.
__global__ void __launch_bounds__(256) pad_image_kernel(Src s, int mode, int bp, int py, int px, float cval, const float* cper, const float* vec,
                                                        i64 vec_ts, float* out, i64 out_ts, int H, int W) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const i64 tile = blockIdx.z;
    if (X >= W || Y >= H) return;
    const int y = Y - bp, x = X - bp;
    const bool iny = y >= 0 && y < s.ny, inx = x >= 0 && x < s.nx;
    float v;
    if (iny && inx) {
        v = src_load(s, tile, y, x);
    } else if (mode == MI_PS_CONSTANT) {
        v = cper ? cper[tile * vec_ts] : cval;
    } else if (mode == MI_PS_LINEAR_RAMP) {
        v = src_load(s, tile, min(max(y, 0), s.ny - 1), min(max(x, 0), s.nx - 1));
        if (!iny) v = y < 0 ? ramp(v, Y, bp) : ramp(v, H - 1 - Y, bp + py);
        if (!inx) v = x < 0 ? ramp(v, X, bp) : ramp(v, W - 1 - X, bp + px);
    } else {
        const float* q = vec + tile * vec_ts;
        v = iny ? q[y] : inx ? q[s.ny + x] : q[s.ny + s.nx];
    }
    out[tile * out_ts + (i64)Y * W + X] = v;
}

int launch_median(hipStream_t st, const Src& s, int along_x, int n, int nlines, int cnt, float* out, i64 out_ts) {
    const dim3 grid(nlines, cnt);
    if (n <= MI_PS_PAD_LDS_LINE) {
        const size_t lds = (size_t)(kSelHist + kSelCtl + n) * sizeof(unsigned);
        MI_TRY(raise_lds(reinterpret_cast<const void*>(&pad_median_kernel<true>), lds));
        hipLaunchKernelGGL(pad_median_kernel<true>, grid, dim3(256), lds, st, s, along_x, n, out, out_ts);
    } else {
        hipLaunchKernelGGL(pad_median_kernel<false>, grid, dim3(256), (kSelHist + kSelCtl) * sizeof(unsigned), st, s, along_x, n, out, out_ts);
    }
    return launch_check("pad_median_kernel");
}

}  // namespace

int run_value_pad(const Plan& P, hipStream_t st, Src src, int cnt) {
    const mi_pystripe_info& I = P.info;
    const int mode = P.prm.padding_mode;
    src.logp = 1;
    float* vec = P.sz_pvec ? P.buf(P.off_pvec) : nullptr;   // [rows ny | columns nx | corner], or the tile's constant alone
    const i64 vec_ts = (i64)P.sz_pvec;
    if (mode == MI_PS_MEDIAN) {
        MI_TRY(launch_median(st, src, 1, I.nx, I.ny, cnt, vec, vec_ts));
        MI_TRY(launch_median(st, src, 0, I.ny, I.nx, cnt, vec + I.ny, vec_ts));
        const Src cols{vec + I.ny, vec_ts, MI_PS_F32, 1, I.nx, I.nx, 0, MAP_IDENTITY, 0};
        MI_TRY(launch_median(st, cols, 1, I.nx, 1, cnt, vec + I.ny + I.nx, vec_ts));
    } else if (mode == MI_PS_MAXIMUM || mode == MI_PS_MINIMUM || mode == MI_PS_MEAN) {
        const int ncb = cdiv(I.nx, 64);
        double* part = reinterpret_cast<double*>(P.buf(P.off_ppart));
        const i64 part_ts = (i64)P.sz_ppart / 2;
        hipLaunchKernelGGL(pad_stats_kernel, dim3(ncb, cnt), dim3(64 * kStatWaves), kStatWaves * 64 * sizeof(double), st, src, mode, part, part_ts,
                           ncb, vec, vec_ts);
        MI_TRY(launch_check("pad_stats_kernel"));
        hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv(I.ny, 256), cnt), dim3(256), 0, st, part, part_ts, ncb, mode, I.ny, I.nx, vec, vec_ts);
        MI_TRY(launch_check("pad_rows_kernel"));
        hipLaunchKernelGGL(pad_corner_kernel, dim3(cnt), dim3(256), 0, st, mode, I.ny, I.nx, vec, vec_ts);
        MI_TRY(launch_check("pad_corner_kernel"));
    }
    const float* cper = mode == MI_PS_CONSTANT ? vec : nullptr;   // the tile's own constant (an estimated clip_min), else the plan's
    const float cval = cper || mode != MI_PS_CONSTANT ? 0.f : (float)std::log1p(P.prm.bleach_clip_min);
    hipLaunchKernelGGL(pad_image_kernel, dim3(cdiv(P.w[0], 64), cdiv(P.h[0], 4), cnt), dim3(256), 0, st, src, mode, I.base_pad, I.pad_y, I.pad_x,
                       cval, cper, vec, vec_ts, P.buf(P.off_P), (i64)P.sz_P, P.h[0], P.w[0]);
    return launch_check("pad_image_kernel");
}

}  // namespace ps
}  // namespace mi
