// pystripe's 2-D wavelet transform (pystripe_internal.h: load, analysis, synthesis, store): db9's kernels, their counterparts for
// any orthogonal wavelet, and the two launchers that run a level's analysis or synthesis with either family.
#include "pystripe_internal.h"

namespace mi {
namespace ps {
namespace {

constexpr int kRowBlock = 256;   // outputs of one block of the analysis row pass

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

}  // namespace

int launch_analysis(const Plan& P, hipStream_t st, int l, const Src& s, int cnt) {
    const int n0 = P.h[l - 1], n1 = P.w[l - 1], m0 = P.h[l], m1 = P.w[l], LT = P.L;
    float *rowL = P.buf(P.off_rowL), *rowH = P.buf(P.off_rowH), *A = P.buf(P.off_A[l]);
    float *cH = P.buf(P.off_cH[l]), *cV = P.buf(P.off_cV[l]), *cD = P.buf(P.off_cD[l]);
    const i64 row_ts = (i64)P.sz_row, a_ts = (i64)P.sz_A[l], d_ts = (i64)P.sz_d[l];
    const float* tab = P.tab_buf.as<float>();
    // the rows of s (the source rows only, at the first level); the column pass looks them up through the map s is read through
    const dim3 rgrid(cdiv(m1, kRowBlock), s.ny, cnt);
    if (P.generic) hipLaunchKernelGGL(ana_rows_gen_kernel, rgrid, dim3(kRowBlock), 0, st, s, n1, m1, rowL, rowH, row_ts, tab, LT);
    else hipLaunchKernelGGL(ana_rows_kernel, rgrid, dim3(kRowBlock), 0, st, s, n1, m1, rowL, rowH, row_ts, P.f);
    MI_TRY(launch_check(P.generic ? "ana_rows_gen_kernel" : "ana_rows_kernel"));
    if (P.generic) {
        const size_t lds = (size_t)(2 * kColRows + LT - 2) * 64 * 2 * sizeof(float);
        MI_TRY(raise_lds(reinterpret_cast<const void*>(&ana_cols_gen_kernel), lds));
        hipLaunchKernelGGL(ana_cols_gen_kernel, dim3(cdiv(m1, 64), cdiv(m0, kColRows), cnt), dim3(256), lds, st, rowL, rowH, row_ts, n0, m0, m1,
                           s.pad, s.ny, s.mode, A, a_ts, cH, cV, cD, d_ts, tab, LT);
    } else {
        hipLaunchKernelGGL(ana_cols_kernel, dim3(cdiv(m1, 64), cdiv(m0, 4), cnt), dim3(256), 0, st, rowL, rowH, row_ts, n0, m0, m1, s.pad, s.ny,
                           s.mode, A, a_ts, cH, cV, cD, d_ts, P.f);
    }
    return launch_check(P.generic ? "ana_cols_gen_kernel" : "ana_cols_kernel");
}

// the reconstruction of level l lands in A[l - 1]'s buffer (level 1: in the padded image P of a two-pass plan, or in the sink)
int launch_synthesis(const Plan& P, hipStream_t st, int l, bool fin, const Sink& k, int cnt) {
    const mi_pystripe_info& I = P.info;
    const int LT = P.L, m0 = P.h[l], m1 = P.w[l], s0 = 2 * m0 - LT + 2, s1 = 2 * m1 - LT + 2;
    const int a_stride = l == I.levels ? m1 : 2 * P.w[l + 1] - LT + 2;
    int y0 = 0, y1 = s0, xp0 = 0, xp1 = s1 / 2;
    if (fin) {
        y0 = I.base_pad; y1 = I.base_pad + I.ny;
        xp0 = I.base_pad / 2; xp1 = (I.base_pad + I.nx + 1) / 2;
    }
    const int p0 = y0 / 2, p1 = (y1 + 1) / 2;
    const float *a = P.buf(P.off_A[l]), *cH = P.buf(P.off_cH[l]), *cV = P.buf(P.off_cV[l]), *cD = P.buf(P.off_cD[l]);
    float *lo1 = P.buf(P.off_rowL), *hi1 = P.buf(P.off_rowH);
    const i64 row_ts = (i64)P.sz_row, a_ts = (i64)P.sz_A[l], d_ts = (i64)P.sz_d[l];
    const float* tab = P.tab_buf.as<float>();
    if (P.generic) {
        const size_t lds = (size_t)(kColPairs + LT / 2 - 1) * 64 * 2 * sizeof(float);
        MI_TRY(raise_lds(reinterpret_cast<const void*>(&syn_cols_gen_kernel), lds));
        hipLaunchKernelGGL(syn_cols_gen_kernel, dim3(cdiv(m1, 64), cdiv(p1 - p0, kColPairs), 2 * cnt), dim3(256), lds, st, a, a_ts, a_stride, cH, cV,
                           cD, d_ts, m1, m0, p0, p1, s0, lo1, hi1, row_ts, tab, LT);
    } else {
        hipLaunchKernelGGL(syn_cols_kernel, dim3(cdiv(m1, 64), cdiv(p1 - p0, 4), 2 * cnt), dim3(256), 0, st, a, a_ts, a_stride, cH, cV, cD, d_ts, m1,
                           p0, p1, s0, lo1, hi1, row_ts, P.f);
    }
    MI_TRY(launch_check(P.generic ? "syn_cols_gen_kernel" : "syn_cols_kernel"));
    float* dst = fin ? nullptr : l == 1 ? P.buf(P.off_P) : P.buf(P.off_A[l - 1]);
    const i64 dst_ts = fin ? 0 : l == 1 ? (i64)P.sz_P : (i64)P.sz_A[l - 1];
    const dim3 grid(cdiv(xp1 - xp0, 256), y1 - y0, cnt);
    if (P.generic) {
        const auto kernel = fin ? syn_rows_gen_kernel<true> : syn_rows_gen_kernel<false>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, lo1, hi1, row_ts, m1, y0, xp0, xp1, s1, dst, dst_ts, k, tab, LT);
    } else {
        const auto kernel = fin ? syn_rows_kernel<true> : syn_rows_kernel<false>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, lo1, hi1, row_ts, m1, y0, xp0, xp1, s1, dst, dst_ts, k, P.f);
    }
    return launch_check(P.generic ? "syn_rows_gen_kernel" : "syn_rows_kernel");
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

}  // namespace ps
}  // namespace mi
