// pystripe's notch on the detail coefficients (pystripe_internal.h: notch): the kernel, its tables and route (lines per block,
// threads, LDS) per (pass, level, axis), and its launcher.
#include <algorithm>
#include <cmath>

#include "pystripe_internal.h"

namespace mi {
namespace ps {
namespace {

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

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

template <int R>
int launch_notch(const Plan& P, hipStream_t st, const NotchTab& t, float* c, i64 tile_stride, int nlines, i64 es, i64 ls, int cnt) {
    const double2* tw = P.tw_buf.as<double2>() + t.tw_off;
    const float* wt = P.w_buf.as<float>() + t.w_off;
    MI_TRY(raise_lds(reinterpret_cast<const void*>(&notch_kernel<R>), t.lds));
    hipLaunchKernelGGL(notch_kernel<R>, dim3(cdiv(nlines, R), cnt), dim3(t.threads), t.lds, st, c, tile_stride, t.n, nlines, es, ls, tw, wt, t.kp,
                       t.kb);
    return launch_check("notch_kernel");
}

}  // namespace

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

int run_notch(const Plan& P, hipStream_t st, const NotchTab& t, float* c, i64 tile_stride, int nlines, i64 es, i64 ls, int cnt) {
    if (t.R == 4) return launch_notch<4>(P, st, t, c, tile_stride, nlines, es, ls, cnt);
    if (t.R == 2) return launch_notch<2>(P, st, t, c, tile_stride, nlines, es, ls, cnt);
    return launch_notch<1>(P, st, t, c, tile_stride, nlines, es, ls, cnt);
}

}  // namespace ps
}  // namespace mi
