// The decon.m drivers around the RL context (rl.hip): deconSpatial and deconFFT (decon.m:24-204, one driver: decon_fixed_psf),
// deconFFT_Wiener (decon.m:206-321), the dispatch of decon (decon.m:1-22) and the deconvolution plan that keeps a context
// between the blocks of a volume.  The regularisation schedule, the Gaussian pre-smooth (5 taps on the GPU path), the Tikhonov
// blend and the ||bl||_2 stop test follow decon.m:41-59,67-79,108-118.
#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "rl_internal.h"

using namespace mi;

namespace {

bool regularization_time(int i, int niter, int interval) {  // decon.m:54-55, i is 1-based
    const bool apply = interval > 0 && interval < niter;
    return apply && i > 1 && i < niter && (i % interval) == 0;
}

int host_norm(hipStream_t s, const float* x, size_t n, double* d_scratch, double* out) {
    MI_TRY(sumsq_async(s, x, n, d_scratch));
    double h = 0.0;
    MI_HIP(hipMemcpyAsync(&h, d_scratch, sizeof(double), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    *out = std::sqrt(h);
    return MI_OK;
}

// the loop shared by deconSpatial and deconFFT once bl has its working shape
int rl_iterate(mi_rl_ctx* ctx, hipStream_t s, float* bl, float* ratio, float* reg, double* d_scratch, int nx, int ny, int nz,
               const mi_rl_options& o, double delta_prev, int* iters_done) {
    const size_t N = (size_t)nx * ny * nz;
    const float sig[3] = {0.5f, 0.5f, 0.5f};
    const int k3[3] = {3, 3, 3};
    int done = 0;
    // the estimate ping-pongs between the caller's array and the scratch volume: the single-pass Gaussian of the regularisation
    // step writes into the other buffer (8 B/voxel, no copy back), which then IS the estimate; the buffer it leaves is the
    // scratch of the following steps.  One copy at the end when the estimate sits in the scratch volume.
    float* const home = bl;
    for (int i = 1; i <= o.niter;) {
        const bool reg_time = regularization_time(i, o.niter, o.regularize_interval);
        int span = 1;
        if (reg_time) {
            MI_REQUIRE(ratio, "decon: the regularisation step needs the scratch volume");
            bool fused = false;
            MI_TRY(gauss3d_to(s, bl, ratio, nx, ny, nz, sig, o.gauss_taps == 3 ? k3 : nullptr, &fused));  // decon.m:57-59
            if (fused) std::swap(bl, ratio);
            if (o.lambda > 0.0f) {
                MI_TRY(mi_rl_forward_ratio(ctx, s, bl, ratio));
                MI_TRY(mi_rl_reg_term(ctx->dev, s, bl, reg, nx, ny, nz));
                MI_TRY(mi_rl_adjoint_update(ctx, s, ratio, bl, o.lambda, reg));
            } else {
                // without the Tikhonov term the smoothed estimate simply goes through a plain iteration (fused on the native pipeline)
                MI_TRY(mi_rl_iterate(ctx, s, bl, ratio, 1));
            }
        } else {
            // run of plain iterations up to the next regularisation step: one call, so an engine that can fuse
            // consecutive iterations (native FFT pipeline) does; the stop test needs the norm after every iteration
            if (o.stop_criterion <= 0.0f)
                while (i + span <= o.niter && !regularization_time(i + span, o.niter, o.regularize_interval)) ++span;
            MI_TRY(mi_rl_iterate(ctx, s, bl, ratio, span));
        }
        i += span;
        done = i - 1;
        if (o.stop_criterion > 0.0f) {  // decon.m:108-118
            double cur = 0.0;
            MI_TRY(host_norm(s, bl, N, d_scratch, &cur));
            const double rel = std::fabs(delta_prev - cur) / delta_prev * 100.0;
            delta_prev = cur;
            if (done > 1 && rel <= (double)o.stop_criterion) break;
        }
    }
    if (bl != home) MI_HIP(hipMemcpyAsync(home, bl, sizeof(float) * N, hipMemcpyDeviceToDevice, s));
    if (iters_done) *iters_done = done;
    return MI_OK;
}

int check_options(const mi_rl_options* o) {
    MI_REQUIRE(o, "decon: null options");
    MI_REQUIRE(o->niter >= 0, "decon: niter must be >= 0");
    MI_REQUIRE(o->lambda >= 0.0f && o->lambda < 1.0f, "decon: lambda must be in [0,1)");
    MI_REQUIRE(o->gauss_taps == 0 || o->gauss_taps == 3 || o->gauss_taps == 5, "decon: gauss_taps must be 0, 3 or 5");
    MI_REQUIRE(o->psf_grid[0] >= 0 && o->psf_grid[1] >= 0 && o->psf_grid[2] >= 0, "decon: psf_grid extents must be >= 0");
    return MI_OK;
}

// pad_block_to_fft_shape (decon.m:144 / 213): the block's working volume on the grid F -- bl itself, or its centred zero-padded copy
// in `own`, which mi_crop_center brings back after the loop
int pad_block(int dev, void* stream, float* bl, const int n[3], const int F[3], DevBuf& own, float** work) {
    *work = bl;
    if (F[0] == n[0] && F[1] == n[1] && F[2] == n[2]) return MI_OK;
    MI_TRY(own.alloc(sizeof(float) * (size_t)F[0] * F[1] * F[2]));
    *work = own.as<float>();
    return mi_pad_center(dev, stream, bl, n[0], n[1], n[2], *work, F[0], F[1], F[2]);
}

// deconFFT's context: circular axes of extent F and psf alone (decon.m:18), its samples placed as ifftshift(zero-pad-centre(psf))
// does on the grid opt->psf_grid names (default: the FFT shape; see mi_rl_options)
int create_circular(int dev, void* stream, const int F[3], const float* psf, const int k[3], const mi_rl_options* opt, mi_rl_ctx** ctx) {
    const int circ[3] = {MI_BOUNDARY_CIRCULAR, MI_BOUNDARY_CIRCULAR, MI_BOUNDARY_CIRCULAR};
    const int engine = opt->engine == MI_ENGINE_DIRECT ? MI_ENGINE_DIRECT : MI_ENGINE_FFT;
    int shift[3];
    for (int d = 0; d < 3; ++d) {
        const int g = opt->psf_grid[d] > 0 ? opt->psf_grid[d] : F[d];
        MI_REQUIRE(g >= k[d], "deconFFT: psf_grid extent %d smaller than the PSF extent %d on axis %d", g, k[d], d);
        shift[d] = g / 2 - (g - k[d]) / 2;
    }
    return mi_rl_create_ex(dev, stream, F[0], F[1], F[2], psf, nullptr, k[0], k[1], k[2], circ, shift, engine, ctx);
}

// deconSpatial and deconFFT.  fft_shape == null is deconSpatial: the block's own grid under the zero rule with the caller's psf_inv,
// the first stop norm taken before the taper.  Otherwise deconFFT: the circular grid fft_shape (x, y, z) the block is padded to
// and cropped from, psf alone, the first stop norm taken on the padded volume.  Everything else is common.
// keep_ctx / keep_taper (a deconvolution plan): the RL context and the taper's FFT engine are created into / reused from them.
// (The host-time spans of a probe build carry deconFFT's labels for either flavour: profiles/ is keyed by them.)
int decon_fixed_psf(int dev, void* stream, float* bl, const float* psf, const float* psf_inv, const int n[3], const int k[3],
                    const int* fft_shape, const mi_rl_options* opt, int* iters_done, mi_rl_ctx** keep_ctx, TaperKeep** keep_taper) {
    const bool fft = fft_shape != nullptr;
    const char* who = fft ? "deconFFT" : "deconSpatial";
    const int* F = fft ? fft_shape : n;  // the working grid
    MI_TRY(use_device(dev));
    MI_TRY(check_options(opt));
    MI_TRY(check_decon_shapes(who, bl, psf, n, k, fft_shape));
    hipStream_t s = as_stream(stream);
    const size_t NF = (size_t)F[0] * F[1] * F[2];
    const bool padded = F[0] != n[0] || F[1] != n[1] || F[2] != n[2];
    // the scratch volume serves the edge taper's blur, the regularisation step's Gaussian and the ratio of engines that do not
    // fuse an iteration: a fused loop without regularisation never touches it and does not allocate it (8.6 GB on config C3)
    const bool reg_sched = opt->regularize_interval > 0 && opt->regularize_interval < opt->niter;
    DevBuf ratio, reg, scratch, blF;
    MI_SPAN_BEGIN(sp0, "deconFFT: allocations");
    if (opt->lambda > 0.0f && reg_sched) MI_TRY(reg.alloc(sizeof(float) * NF));
    MI_TRY(scratch.alloc(sizeof(double)));
    if (!opt->skip_edgetaper) MI_TRY(ratio.alloc(sizeof(float) * NF));
    MI_SPAN_END(sp0);
    double delta_prev = 0.0;
    if (opt->stop_criterion > 0.0f && !fft) MI_TRY(host_norm(s, bl, NF, scratch.as<double>(), &delta_prev));  // deconSpatial: before the taper (decon.m:46-50)
    if (!opt->skip_edgetaper) {  // decon.m:50 / 143
        MI_SPAN_BEGIN(sp1, "deconFFT: edgetaper (ends with a wait)");
        MI_TRY(edgetaper_async(s, bl, ratio.as<float>(), psf, n[0], n[1], n[2], k[0], k[1], k[2], keep_taper));
        MI_SPAN_END(sp1);
    }
    float* work_bl = bl;
    if (padded) {  // decon.m:144
        MI_SPAN_BEGIN(sp2, "deconFFT: padded copy (alloc + enqueue)");
        MI_TRY(pad_block(dev, stream, bl, n, F, blF, &work_bl));
        MI_SPAN_END(sp2);
    }
    if (opt->stop_criterion > 0.0f && fft) MI_TRY(host_norm(s, work_bl, NF, scratch.as<double>(), &delta_prev));  // deconFFT: after the pad (decon.m:145-147)
    mi_rl_ctx* ctx = keep_ctx ? *keep_ctx : nullptr;
    if (!ctx) {
        MI_SPAN_BEGIN(sp3, "deconFFT: mi_rl_create (a new shape)");
        NoPlacementTrial as_they_come;   // (a handful of iterations per context: see fft_native.h)
        MI_TRY(fft ? create_circular(dev, stream, F, psf, k, opt, &ctx)
                   : mi_rl_create(dev, stream, n[0], n[1], n[2], psf, psf_inv, k[0], k[1], k[2], MI_BOUNDARY_ZERO, opt->engine, &ctx));
        MI_SPAN_END(sp3);
    }
    if (keep_ctx) *keep_ctx = ctx;
    CtxGuard own{keep_ctx ? nullptr : ctx, s};  // declared after the volumes: on a failure below it waits before they are released
    MI_SPAN_BEGIN(sp4, "deconFFT: wait + release of the taper's work");
    if (reg_sched || !mi_rl_fuses(ctx)) {
        if (!ratio.p) MI_TRY(ratio.alloc(sizeof(float) * NF));
    } else {
        MI_HIP(hipStreamSynchronize(s));  // the taper may still be reading it
        ratio.release();
    }
    MI_SPAN_END(sp4);
    MI_SPAN_BEGIN(sp5, "deconFFT: rl_iterate (enqueue)");
    int rc = rl_iterate(ctx, s, work_bl, ratio.as<float>(), reg.as<float>(), scratch.as<double>(), F[0], F[1], F[2], *opt, delta_prev, iters_done);
    if (rc == MI_OK && padded) rc = mi_crop_center(dev, stream, work_bl, F[0], F[1], F[2], bl, n[0], n[1], n[2]);  // decon.m:203
    MI_SPAN_END(sp5);
    MI_SPAN_BEGIN(sp6, "deconFFT: final wait for the stream");
    hipError_t e = hipStreamSynchronize(s);
    MI_SPAN_END(sp6);
    mi_rl_destroy(own.c);  // the stream has just been waited for: the guard has nothing left to do
    own.c = nullptr;
    if (rc == MI_OK && e != hipSuccess) rc = fail(MI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return rc;
}

}  // namespace

extern "C" int mi_rl_spatial(int dev, void* stream, float* bl, const float* psf, const float* psf_inv, int nx, int ny, int nz, int kx,
                             int ky, int kz, const mi_rl_options* opt, int* iters_done) {
    const int n[3] = {nx, ny, nz}, k[3] = {kx, ky, kz};
    return decon_fixed_psf(dev, stream, bl, psf, psf_inv, n, k, nullptr, opt, iters_done, nullptr, nullptr);
}

extern "C" int mi_rl_fft(int dev, void* stream, float* bl, const float* psf, int nx, int ny, int nz, int kx, int ky, int kz, int fx,
                         int fy, int fz, const mi_rl_options* opt, int* iters_done) {
    const int n[3] = {nx, ny, nz}, k[3] = {kx, ky, kz}, F[3] = {fx, fy, fz};
    return decon_fixed_psf(dev, stream, bl, psf, nullptr, n, k, F, opt, iters_done, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------ deconFFT_Wiener
namespace {

constexpr int kThreads = 256;
inline unsigned stream_grid(size_t n_items) {
    const size_t b = (n_items + kThreads - 1) / kThreads, cap = 256 * 16;  // grid-stride beyond 16 work-groups per CU
    return static_cast<unsigned>(b < 1 ? 1 : (b > cap ? cap : b));
}

// otf_new = F{Y} conj(F{X}) / max(|F{X}|^2, eps) (decon.m:282-288), element-wise on the untangled half spectra; `scale` folds in
// the 2 / (Fx Fy Fz) of the pipeline's unnormalised inverse
__global__ __launch_bounds__(kThreads) void k_wiener_otf(const float2* __restrict__ fy, const float2* __restrict__ fx, float2* __restrict__ otf,
                                                       size_t n, float scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float2 y = fy[i], x = fx[i];
        const float den = fmaxf(x.x * x.x + x.y * x.y, kEpsSingle);
        const float re = y.x * x.x + y.y * x.y, im = y.y * x.x - y.x * x.y;  // y * conj(x)
        otf[i] = make_float2(re / den * scale, im / den * scale);
    }
}

__global__ __launch_bounds__(kThreads) void k_delta(float* __restrict__ v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) v[i] = i == 0 ? 1.0f : 0.0f;
}

// psf = max(full(centre box), 0); psf /= sum(psf) when the sum is positive (decon.m:293-301).  One work-group: a PSF is small.
__global__ __launch_bounds__(256) void k_wiener_psf(const float* __restrict__ full, float* __restrict__ psf, int fx, int fy, int kx, int ky,
                                                     int kz, int cx, int cy, int cz) {
    __shared__ float part[256];
    const int n = kx * ky * kz;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int x = i % kx, r = i / kx, y = r % ky, z = r / ky;
        const float v = fmaxf(full[((size_t)(cz + z) * fy + (cy + y)) * fx + (cx + x)], 0.0f);
        psf[i] = v;
        acc += v;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    const float sum = part[0];
    if (sum > 0.0f)
        for (int i = threadIdx.x; i < n; i += 256) psf[i] = psf[i] / sum;
}

}  // namespace

extern "C" int mi_rl_fft_wiener(int dev, void* stream, float* bl, float* psf, int nx, int ny, int nz, int kx, int ky, int kz, int fx,
                                int fy, int fz, const mi_rl_options* opt, int* iters_done) {
    const int n[3] = {nx, ny, nz}, k[3] = {kx, ky, kz}, F[3] = {fx, fy, fz};
    MI_TRY(use_device(dev));
    MI_TRY(check_options(opt));
    MI_TRY(check_decon_shapes("deconFFT_Wiener", bl, psf, n, k, F));
    // the spectra F{Y}, F{X} live in the hand-written pipeline's own layout; rocFFT-only shapes are not served
    if (!(mi_fft_good_size(fx, 0) == fx && mi_fft_good_size(fy, 1) == fy && mi_fft_good_size(fz, 2) == fz))
        return fail(MI_ERR_UNSUPPORTED, "deconFFT_Wiener: fft_shape [%d %d %d] must be made of extents mi_fft_good_size accepts (2^a, 3 * 2^a or 9 * 2^a; x even)", fx, fy, fz);
    hipStream_t s = as_stream(stream);
    const size_t NF = (size_t)fx * fy * fz;
    const int nk = kx * ky * kz;
    DevBuf ratio, reg, scratch, blF, psf_cur, FY, FX;
    MI_TRY(ratio.alloc(sizeof(float) * NF));
    // no `interval < niter` here, unlike decon_fixed_psf: this variant regularises on every multiple of the interval (intended, decon.m:272)
    if (opt->lambda > 0.0f && opt->regularize_interval > 0) MI_TRY(reg.alloc(sizeof(float) * NF));
    MI_TRY(scratch.alloc(sizeof(double)));
    MI_TRY(psf_cur.alloc(sizeof(float) * nk));
    MI_HIP(hipMemcpyAsync(psf_cur.p, psf, sizeof(float) * nk, hipMemcpyDeviceToDevice, s));
    if (!opt->skip_edgetaper) MI_TRY(edgetaper_async(s, bl, ratio.as<float>(), psf, nx, ny, nz, kx, ky, kz));  // decon.m:212
    float* work_bl = nullptr;
    MI_TRY(pad_block(dev, stream, bl, n, F, blF, &work_bl));  // decon.m:213
    double delta_prev = 0.0;
    if (opt->stop_criterion > 0.0f) MI_TRY(host_norm(s, work_bl, NF, scratch.as<double>(), &delta_prev));  // decon.m:215
    mi_rl_ctx* ctx = nullptr;
    const int b[3] = {MI_BOUNDARY_CIRCULAR, MI_BOUNDARY_CIRCULAR, MI_BOUNDARY_CIRCULAR};
    {
        NoPlacementTrial as_they_come;
        MI_TRY(rl_create(dev, stream, fx, fy, fz, psf, nullptr, kx, ky, kz, b, nullptr, MI_ENGINE_FFT, /*fixed_psf=*/false, &ctx));
    }
    CtxGuard guard{ctx, s};
    FftEngine* fe = ctx->fft;
    MI_REQUIRE(fe->native, "deconFFT_Wiener: the hand-written FFT pipeline refused fft_shape [%d %d %d]", fx, fy, fz);
    NativeFft* nf = fe->native;
    const size_t items = nf->otf_items();
    MI_TRY(FY.alloc(sizeof(float4) * items));
    MI_TRY(FX.alloc(sizeof(float4) * items));
    float4 *fy_p = FY.as<float4>(), *fx_p = FX.as<float4>();
    const float nscale = 2.0f / (float)((double)fx * fy * fz);
    const float sig[3] = {0.5f, 0.5f, 0.5f};
    const int k3[3] = {3, 3, 3};
    const int cx = (fx - kx) / 2, cy = (fy - ky) / 2, cz = (fz - kz) / 2;  // floor((fft_shape - psf_sz) / 2) + 1, 0-based (decon.m:236)
    ConvEpilogue none;
    int done = 0;
    for (int i = 1; i <= opt->niter; ++i) {
        if (i > 1) MI_TRY(fe->set_psf(s, psf_cur.as<float>()));  // decon.m:243-245 (iteration 1: the OTF mi_rl_create built)
        const bool reg_i = opt->regularize_interval > 0 && (i % opt->regularize_interval) == 0;
        // F{Y} (decon.m:248-256) only feeds the Wiener quotient here: the RL step transforms bl itself
        if (i > 1 && reg_i) MI_TRY(gauss3d_async(s, work_bl, ratio.as<float>(), fx, fy, fz, sig, opt->gauss_taps == 3 ? k3 : nullptr));
        if (i < opt->niter && (i == 1 || reg_i)) MI_TRY(nf->spectrum(s, work_bl, fy_p, 1.0f));
        if (reg_i && opt->lambda > 0.0f && i < opt->niter) {  // decon.m:273-275
            MI_TRY(mi_rl_forward_ratio(ctx, s, work_bl, ratio.as<float>()));
            MI_TRY(mi_rl_reg_term(dev, s, work_bl, reg.as<float>(), fx, fy, fz));
            MI_TRY(mi_rl_adjoint_update(ctx, s, ratio.as<float>(), work_bl, opt->lambda, reg.as<float>()));
        } else {
            MI_TRY(mi_rl_iterate(ctx, s, work_bl, ratio.as<float>(), 1));
        }
        if (i < opt->niter) {  // decon.m:281-307
            MI_TRY(nf->spectrum(s, work_bl, fx_p, 1.0f));
            hipLaunchKernelGGL(k_wiener_otf, dim3(stream_grid(2 * items)), dim3(kThreads), 0, s, reinterpret_cast<const float2*>(fy_p),
                               reinterpret_cast<const float2*>(fx_p), reinterpret_cast<float2*>(nf->otf()), 2 * items, nscale);
            MI_TRY(launch_check("k_wiener_otf"));
            std::swap(fy_p, fx_p);  // F{X} is the next iteration's F{Y}
            // real(ifftn(otf_new)): the response of the new OTF to a unit impulse at the origin
            hipLaunchKernelGGL(k_delta, dim3(stream_grid(NF)), dim3(kThreads), 0, s, ratio.as<float>(), NF);
            MI_TRY(launch_check("k_delta"));
            MI_TRY(fe->conv(s, ratio.as<float>(), false, ratio.as<float>(), EPI_NONE, none));
            hipLaunchKernelGGL(k_wiener_psf, dim3(1), dim3(256), 0, s, ratio.as<float>(), psf_cur.as<float>(), fx, fy, kx, ky, kz, cx, cy, cz);
            MI_TRY(launch_check("k_wiener_psf"));
        }
        done = i;
        // no `done > 1` guard and delta_prev moves only past the test, unlike rl_iterate (intended, decon.m:310-317)
        if (opt->stop_criterion > 0.0f) {
            double cur = 0.0;
            MI_TRY(host_norm(s, work_bl, NF, scratch.as<double>(), &cur));
            if (std::fabs(delta_prev - cur) / delta_prev * 100.0 <= (double)opt->stop_criterion) break;
            delta_prev = cur;
        }
    }
    if (iters_done) *iters_done = done;
    if (work_bl != bl) MI_TRY(mi_crop_center(dev, stream, work_bl, fx, fy, fz, bl, nx, ny, nz));  // decon.m:320
    MI_HIP(hipMemcpyAsync(psf, psf_cur.p, sizeof(float) * nk, hipMemcpyDeviceToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
    return MI_OK;
}

extern "C" int mi_decon(int dev, void* stream, float* bl, const float* psf, const float* psf_inv, int nx, int ny, int nz, int kx, int ky,
                        int kz, const mi_rl_options* opt, int use_fft, const int* fft_shape_xyz, int adaptive_psf, int* iters_done) {
    if (use_fft) {
        int f[3] = {nx, ny, nz};
        if (fft_shape_xyz) { f[0] = fft_shape_xyz[0]; f[1] = fft_shape_xyz[1]; f[2] = fft_shape_xyz[2]; }
        if (adaptive_psf) {  // decon.m:15-16; the caller's PSF stays as it was (the refined one is deconFFT_Wiener's local)
            MI_REQUIRE(psf && kx > 0 && ky > 0 && kz > 0, "deconFFT_Wiener: null pointer");
            MI_TRY(use_device(dev));
            DevBuf p;
            MI_TRY(p.alloc(sizeof(float) * (size_t)kx * ky * kz));
            MI_HIP(hipMemcpyAsync(p.p, psf, sizeof(float) * (size_t)kx * ky * kz, hipMemcpyDeviceToDevice, as_stream(stream)));
            return mi_rl_fft_wiener(dev, stream, bl, p.as<float>(), nx, ny, nz, kx, ky, kz, f[0], f[1], f[2], opt, iters_done);
        }
        return mi_rl_fft(dev, stream, bl, psf, nx, ny, nz, kx, ky, kz, f[0], f[1], f[2], opt, iters_done);
    }
    return mi_rl_spatial(dev, stream, bl, psf, psf_inv, nx, ny, nz, kx, ky, kz, opt, iters_done);  // adaptive_psf: FFT path only (decon.m:14-22)
}

// ------------------------------------------------------------------------------------------------ deconvolution plans
// The blocks of a volume share shape and PSF (LsDeconv.m:620-668): a plan keeps what `decon` would rebuild for every block --
// the RL context (OTF, twiddles, scratch) and the FFT engine of edgetaper_3d's blur -- and rebuilds it only when shape, PSF or
// engine change.  One plan per worker thread (it is not re-entrant).
struct mi_decon_plan {
    int dev = 0;
    int key[15] = {0};          // nx ny nz kx ky kz use_fft fx fy fz engine has_inv psf_grid[3]
    std::vector<float> psf, psf_inv;
    mi_rl_ctx* ctx = nullptr;
    TaperKeep* taper = nullptr;
    void drop() {
        if (ctx) mi_rl_destroy(ctx);
        taper_keep_free(taper);
        ctx = nullptr;
        taper = nullptr;
    }
};

extern "C" int mi_decon_plan_create(int dev, mi_decon_plan** out) {
    MI_TRY(use_device(dev));
    MI_REQUIRE(out, "mi_decon_plan_create: null pointer");
    *out = new (std::nothrow) mi_decon_plan;
    if (!*out) return fail(MI_ERR_NOMEM, "mi_decon_plan_create: out of host memory");
    (*out)->dev = dev;
    return MI_OK;
}

extern "C" int mi_decon_plan_destroy(mi_decon_plan* plan) {
    if (!plan) return MI_OK;
    (void)hipSetDevice(plan->dev);
    (void)hipDeviceSynchronize();
    plan->drop();
    delete plan;
    return MI_OK;
}

extern "C" int mi_decon_plan_run(mi_decon_plan* plan, void* stream, float* bl, const float* psf, const float* psf_inv, int nx, int ny, int nz,
                                 int kx, int ky, int kz, const mi_rl_options* opt, int use_fft, const int* fft_shape_xyz, int adaptive_psf,
                                 int* iters_done) {
    MI_REQUIRE(plan && opt && psf, "mi_decon_plan_run: null pointer");
    const int dev = plan->dev;
    if (adaptive_psf && use_fft)  // the Wiener variant rebuilds its OTF every iteration: nothing to keep
        return mi_decon(dev, stream, bl, psf, psf_inv, nx, ny, nz, kx, ky, kz, opt, use_fft, fft_shape_xyz, adaptive_psf, iters_done);
    MI_TRY(use_device(dev));
    MI_REQUIRE(kx > 0 && ky > 0 && kz > 0, "decon: psf must be 3D and non-empty");
    int f[3] = {nx, ny, nz};
    if (use_fft && fft_shape_xyz) { f[0] = fft_shape_xyz[0]; f[1] = fft_shape_xyz[1]; f[2] = fft_shape_xyz[2]; }
    const int key[15] = {nx, ny, nz, kx, ky, kz, use_fft ? 1 : 0, f[0], f[1], f[2], opt->engine, (!use_fft && psf_inv) ? 1 : 0,
                         use_fft ? opt->psf_grid[0] : 0, use_fft ? opt->psf_grid[1] : 0, use_fft ? opt->psf_grid[2] : 0};
    // the PSFs are small: compare their values with the ones the kept objects were built from
    hipStream_t s = as_stream(stream);
    const size_t nk = (size_t)kx * ky * kz;
    std::vector<float> h(nk), hi;
    MI_SPAN_BEGIN(sp0, "plan_run: psf fetch + wait for the stream");
    MI_HIP(hipMemcpyAsync(h.data(), psf, sizeof(float) * nk, hipMemcpyDeviceToHost, s));
    if (key[11]) {
        hi.resize(nk);
        MI_HIP(hipMemcpyAsync(hi.data(), psf_inv, sizeof(float) * nk, hipMemcpyDeviceToHost, s));
    }
    MI_HIP(hipStreamSynchronize(s));
    MI_SPAN_END(sp0);
    if (std::memcmp(key, plan->key, sizeof(key)) != 0 || h != plan->psf || hi != plan->psf_inv) {
        MI_SPAN_BEGIN(sp1, "plan_run: drop of the kept objects");
        MI_HIP(hipStreamSynchronize(s));
        plan->drop();
        std::memcpy(plan->key, key, sizeof(key));
        plan->psf.swap(h);
        plan->psf_inv.swap(hi);
        MI_SPAN_END(sp1);
    }
    const int n[3] = {nx, ny, nz}, k[3] = {kx, ky, kz};
    int rc = decon_fixed_psf(dev, stream, bl, psf, psf_inv, n, k, use_fft ? f : nullptr, opt, iters_done, &plan->ctx, &plan->taper);
    if (rc != MI_OK) {  // whatever was half built is not trusted
        (void)hipStreamSynchronize(s);
        plan->drop();
        plan->key[0] = 0;
    }
    return rc;
}
