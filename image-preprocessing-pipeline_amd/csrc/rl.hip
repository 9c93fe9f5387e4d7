// Richardson-Lucy context: the iteration of decon.m:1-204 (deconSpatial / deconFFT) on either engine.
//
// One iteration = two fused passes regardless of engine:
//   forward_ratio : ratio = bl ./ max(conv(bl, psf), eps)       (decon.m:61-63 / 162-167)
//   adjoint_update: bl    = abs(bl .* conv(ratio, psf_inv))     (decon.m:64,76,79 / 169-186)
// The numerator is the running estimate (no stored observation) and abs() follows the product,
// exactly as the reference does.
// The context (mi_rl_ctx, rl_internal.h) holds what either engine prepares once per shape and PSF; the loops around the two
// passes -- regularisation schedule, stop test, taper, padding -- are rl_decon.hip's.
#include <cmath>
#include <new>
#include <vector>

#include "rl_internal.h"

using namespace mi;

namespace {
// Rank-1 test on the host: with the largest sample p0 at (z0, y0, x0), psf is separable iff psf[z][y][x] = a[z] b[y] c[x] / p0^2
// for the lines a, b, c through that sample, to fp32 rounding.  factors[0..2] = taps along x, y, z (product = the PSF).
bool factor_rank1(const std::vector<float>& p, int kx, int ky, int kz, std::vector<float> (&factors)[3]) {
    size_t best = 0;
    for (size_t i = 1; i < p.size(); ++i)
        if (std::fabs(p[i]) > std::fabs(p[best])) best = i;
    const double p0 = p[best];
    if (!(std::fabs(p0) > 0.0) || kx * ky * kz == 1) return false;
    const int z0 = (int)(best / ((size_t)ky * kx)), y0 = (int)((best / kx) % ky), x0 = (int)(best % kx);
    auto at = [&](int z, int y, int x) { return (double)p[((size_t)z * ky + y) * kx + x]; };
    // every sample within a few fp32 roundings of the product of its three line samples RELATIVE TO THE SAMPLE (four roundings:
    // its own and those of the three line samples), with an absolute floor of 1e-9 of the peak for samples that underflow; the
    // flux the rank-1 form takes from or adds to the PSF is then below 4e-7 of its own (an absolute bound of 4e-7 of the peak
    // per sample allowed up to K * 4e-7 * peak)
    for (int z = 0; z < kz; ++z)
        for (int y = 0; y < ky; ++y)
            for (int x = 0; x < kx; ++x) {
                const double v = at(z, y, x), r = std::fabs(v - at(z, y0, x0) * at(z0, y, x0) * at(z0, y0, x) / (p0 * p0));
                if (r > 4e-7 * std::fabs(v) + 1e-9 * std::fabs(p0)) return false;
            }
    factors[0].resize(kx);
    factors[1].resize(ky);
    factors[2].resize(kz);
    for (int x = 0; x < kx; ++x) factors[0][x] = (float)at(z0, y0, x);
    for (int y = 0; y < ky; ++y) factors[1][y] = (float)(at(z0, y, x0) / p0);
    for (int z = 0; z < kz; ++z) factors[2][z] = (float)(at(z, y0, x0) / p0);
    return true;
}

// the three 1-D tap tables of a rank-1 kernel for the direct engine
int prepare_separable(hipStream_t s, const std::vector<float> (&f)[3], bool flip, DevBuf (&tabs)[3], int (&kxp)[3]) {
    for (int d = 0; d < 3; ++d) {
        DevBuf line;
        const int n = (int)f[d].size();
        MI_TRY(line.alloc(sizeof(float) * (size_t)n));
        MI_HIP(hipMemcpyAsync(line.p, f[d].data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
        MI_TRY(direct_prepare_psf(s, line.as<float>(), d == 0 ? n : 1, d == 1 ? n : 1, d == 2 ? n : 1, false, flip, tabs[d], &kxp[d]));
        MI_HIP(hipStreamSynchronize(s));  // `line` and the host vector die at scope exit
    }
    return MI_OK;
}
}  // namespace

extern "C" int mi_engine_select(int nx, int ny, int nz, int kx, int ky, int kz, int boundary) {
    // direct: 2*K flop per voxel at ~60 TFLOP/s sustained fp32.  FFT, per grid point and convolution (measured):
    // ~9.5 ps through the hand-written pipeline on a padded grid (8.2 ps on a circular one), ~29 ps through rocFFT.
    const double K = (double)kx * ky * kz;
    const double N = (double)nx * ny * nz;
    const int n[3] = {nx, ny, nz}, k[3] = {kx, ky, kz}, bnd[3] = {boundary, boundary, boundary};
    int need[3], F[3];
    for (int d = 0; d < 3; ++d) {
        need[d] = n[d];
        if (boundary == MI_BOUNDARY_ZERO) need[d] = n[d] + k[d] / 2;
        if (boundary == MI_BOUNDARY_REPLICATE) need[d] = n[d] + k[d] - 1;
    }
    const bool native = choose_fft_lengths(need, bnd, F);
    const double Nf = (double)F[0] * F[1] * F[2];
    const double t_direct = N * 2.0 * K / 60e12;
    const double t_fft = Nf * (native ? (boundary == MI_BOUNDARY_CIRCULAR ? 8.2e-12 : 9.5e-12) : 29e-12) + 60e-6;
    // without an explicit adjoint kernel the flipped PSF is conj(OTF), which needs centred odd extents off the circular rule
    const bool odd = (kx & 1) && (ky & 1) && (kz & 1);
    return ((odd || boundary == MI_BOUNDARY_CIRCULAR) && t_fft < t_direct) ? MI_ENGINE_FFT : MI_ENGINE_DIRECT;
}

// default PSF placement shift of one axis: sample j of the PSF sits at index (j - shift) of the circular kernel
static int default_shift(int n, int k, int boundary) {
    if (boundary == MI_BOUNDARY_CIRCULAR) return n / 2 - (n - k) / 2;  // ifftshift(zero-pad-centre(psf)), decon.m:131-133
    return k - 1 - conv_kernel_offset(k, boundary);
}

// psf(end:-1:1,end:-1:1,end:-1:1) of a contiguous array = its samples in reverse linear order (LsDeconv.m:163)
__global__ void k_reverse(const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[n - 1 - i];
}

int mi::rl_create(int dev, void* stream, int nx, int ny, int nz, const float* psf, const float* psf_inv, int kx, int ky, int kz,
                  const int* boundary_xyz, const int* shift_xyz, int engine, bool fixed_psf, mi_rl_ctx** out) {
    MI_TRY(use_device(dev));
    MI_REQUIRE(out, "mi_rl_create: null ctx pointer");
    *out = nullptr;
    MI_REQUIRE(psf && boundary_xyz, "mi_rl_create: null psf / boundary");
    MI_REQUIRE(nx > 0 && ny > 0 && nz > 0 && kx > 0 && ky > 0 && kz > 0, "mi_rl_create: bl and psf must be 3D and non-empty");
    const int n[3] = {nx, ny, nz}, k[3] = {kx, ky, kz};
    int shift[3];
    bool uniform = true;
    for (int d = 0; d < 3; ++d) {
        MI_REQUIRE(boundary_xyz[d] >= MI_BOUNDARY_ZERO && boundary_xyz[d] <= MI_BOUNDARY_CIRCULAR, "mi_rl_create: unknown boundary rule %d",
                   boundary_xyz[d]);
        if (boundary_xyz[d] == MI_BOUNDARY_CIRCULAR)
            MI_REQUIRE(k[d] <= n[d], "pad_block_to_fft_shape: psf larger than FFT shape on axis %d", d);
        shift[d] = (shift_xyz && shift_xyz[d] >= 0) ? shift_xyz[d] : default_shift(n[d], k[d], boundary_xyz[d]);
        MI_REQUIRE(shift[d] >= 0 && shift[d] < k[d], "mi_rl_create: PSF shift %d outside [0,%d) on axis %d", shift[d], k[d], d);
        uniform = uniform && boundary_xyz[d] == boundary_xyz[0];
    }
    if (engine == MI_ENGINE_AUTO) engine = mi_engine_select(nx, ny, nz, kx, ky, kz, uniform ? boundary_xyz[0] : MI_BOUNDARY_ZERO);
    MI_REQUIRE(engine == MI_ENGINE_DIRECT || engine == MI_ENGINE_FFT, "mi_rl_create: engine %d not available", engine);
    hipStream_t s = as_stream(stream);
    // psf_inv == NULL stands for the flipped PSF of LsDeconv.m:163, which decon.m:64 convolves with convn(., 'same'): the same
    // centre as the forward convolution.  On a circular axis (deconFFT: conj(otf), decon.m:168) and on every axis whose placement
    // is mirror-symmetric (k - 1 - shift == shift: odd extents, centred) that is the transpose of the forward operator, which both
    // engines get for free; on a non-circular axis of EVEN extent it is one sample off the transpose, so the flipped kernel is
    // materialised and takes the explicit-psf_inv path.
    DevBuf flipped;
    if (!psf_inv) {
        bool off_transpose = false, circular_skew = false;
        for (int d = 0; d < 3; ++d) {
            const bool skew = (k[d] - 1 - shift[d]) != shift[d];
            off_transpose = off_transpose || (skew && boundary_xyz[d] != MI_BOUNDARY_CIRCULAR);
            circular_skew = circular_skew || (skew && boundary_xyz[d] == MI_BOUNDARY_CIRCULAR);
        }
        if (off_transpose) {
            MI_REQUIRE(!circular_skew, "mi_rl_create: psf_inv == NULL is ambiguous for even PSF extents on a mix of circular and "
                                       "non-circular axes; pass the adjoint kernel explicitly");
            const int nk = kx * ky * kz;
            MI_TRY(flipped.alloc(sizeof(float) * (size_t)nk));
            k_reverse<<<cdiv(nk, 256), 256, 0, s>>>(psf, flipped.as<float>(), nk);
            MI_TRY(launch_check("k_reverse"));
            psf_inv = flipped.as<float>();
        }
    }
    mi_rl_ctx* c = new (std::nothrow) mi_rl_ctx;
    if (!c) return fail(MI_ERR_NOMEM, "mi_rl_create: out of host memory");
    c->dev = dev;
    c->engine = engine;
    for (int d = 0; d < 3; ++d) {
        c->n[d] = n[d];
        c->k[d] = k[d];
        c->bnd[d] = boundary_xyz[d];
        // forward: out[x] = sum_j in[x - j + shift] psf[j]  -> window starts k-1-shift before x (flipped taps)
        // adjoint (conj OTF): out[x] = sum_j in[x + j - shift] psf[j] -> window starts shift before x (plain taps);
        // with an explicit psf_inv it is an ordinary convolution with that kernel
        c->off_fwd[d] = k[d] - 1 - shift[d];
        c->off_adj[d] = psf_inv ? k[d] - 1 - shift[d] : shift[d];
    }
    int rc = MI_OK;
    if (engine == MI_ENGINE_DIRECT && !std::getenv("MI_NO_SEPARABLE")) {
        // rank-1 PSF (and adjoint kernel): three 1-D passes instead of the dense taps
        const size_t nk = (size_t)kx * ky * kz;
        std::vector<float> hp(nk), hi(psf_inv ? nk : 0);
        std::vector<float> ff[3], fi[3];
        hipError_t e = hipMemcpyAsync(hp.data(), psf, sizeof(float) * nk, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && psf_inv) e = hipMemcpyAsync(hi.data(), psf_inv, sizeof(float) * nk, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = fail(MI_ERR_HIP, "mi_rl_create: %s", hipGetErrorString(e));
        if (rc == MI_OK && factor_rank1(hp, kx, ky, kz, ff) && (!psf_inv || factor_rank1(hi, kx, ky, kz, fi))) {
            rc = prepare_separable(s, ff, /*flip=*/true, c->sep_fwd, c->sep_kxp);
            // adjoint taps: flip(psf_inv); without psf_inv the transpose of the forward operator = the plain taps of psf
            if (rc == MI_OK) rc = psf_inv ? prepare_separable(s, fi, true, c->sep_adj, c->sep_kxp) : prepare_separable(s, ff, false, c->sep_adj, c->sep_kxp);
            c->separable = rc == MI_OK;
            if (c->separable) {  // window-order taps: forward = the flipped lines; adjoint = flip(psf_inv), or the plain lines of psf
                bool fits = true;
                for (int d = 0; d < 3; ++d) {
                    const std::vector<float>& fl = ff[d];
                    const std::vector<float>& al = psf_inv ? fi[d] : ff[d];
                    const int nt = (int)fl.size();
                    fits = fits && nt <= kSepMaxTaps;
                    if (!fits) break;
                    c->sep_tf[d].n = c->sep_ta[d].n = nt;
                    for (int t = 0; t < nt; ++t) {
                        c->sep_tf[d].w[t] = fl[nt - 1 - t];
                        c->sep_ta[d].w[t] = psf_inv ? al[nt - 1 - t] : al[t];
                    }
                }
                c->sep_single = fits && !std::getenv("MI_NO_SEP_SINGLE") && sep3d_fits(nx, c->k, c->off_fwd) && sep3d_fits(nx, c->k, c->off_adj);
            }
        }
    }
    if (rc == MI_OK && engine == MI_ENGINE_DIRECT) {
        rc = direct_prepare_psf(s, psf, kx, ky, kz, false, /*flip=*/true, c->kf_fwd, &c->kxp);
        // adjoint taps: flip(psf_inv); with psf_inv = flip(psf) (LsDeconv.m:163) that is psf itself
        if (rc == MI_OK)
            rc = psf_inv ? direct_prepare_psf(s, psf_inv, kx, ky, kz, false, true, c->kf_adj, &c->kxp)
                         : direct_prepare_psf(s, psf, kx, ky, kz, false, false, c->kf_adj, &c->kxp);
    } else {
        c->fft = new (std::nothrow) FftEngine;
        if (!c->fft) rc = fail(MI_ERR_NOMEM, "mi_rl_create: out of host memory");
        if (rc == MI_OK) rc = c->fft->init(s, n, k, c->bnd, shift, psf, psf_inv, true, fixed_psf);
    }
    if (rc == MI_OK) {
        MI_SPAN_BEGIN(spw, "rl_create: final wait for the stream");
        hipError_t e = hipStreamSynchronize(s);
        MI_SPAN_END(spw);
        if (e != hipSuccess) rc = fail(MI_ERR_HIP, "mi_rl_create: %s", hipGetErrorString(e));
    }
    if (rc != MI_OK) {
        delete c;
        return rc;
    }
    *out = c;
    return MI_OK;
}

extern "C" int mi_rl_create_ex(int dev, void* stream, int nx, int ny, int nz, const float* psf, const float* psf_inv, int kx, int ky,
                               int kz, const int* boundary_xyz, const int* shift_xyz, int engine, mi_rl_ctx** out) {
    return rl_create(dev, stream, nx, ny, nz, psf, psf_inv, kx, ky, kz, boundary_xyz, shift_xyz, engine, true, out);
}

extern "C" int mi_rl_create(int dev, void* stream, int nx, int ny, int nz, const float* psf, const float* psf_inv, int kx, int ky,
                            int kz, int boundary, int engine, mi_rl_ctx** out) {
    const int b[3] = {boundary, boundary, boundary};
    // deconFFT takes only psf.psf (decon.m:18): the circular flavour ignores psf_inv
    return mi_rl_create_ex(dev, stream, nx, ny, nz, psf, boundary == MI_BOUNDARY_CIRCULAR ? nullptr : psf_inv, kx, ky, kz, b, nullptr,
                           engine, out);
}

extern "C" int mi_rl_destroy(mi_rl_ctx* ctx) {
    if (!ctx) return MI_OK;
    (void)hipSetDevice(ctx->dev);
    delete ctx;
    return MI_OK;
}

extern "C" int mi_rl_engine(const mi_rl_ctx* ctx) { return ctx ? ctx->engine : MI_ERR_INVALID; }

extern "C" size_t mi_rl_device_bytes(const mi_rl_ctx* ctx) {
    if (!ctx) return 0;
    return ctx->kf_fwd.bytes + ctx->kf_adj.bytes + ctx->sep_t0.bytes + ctx->sep_t1.bytes + (ctx->fft ? ctx->fft->device_bytes() : 0);
}

extern "C" int mi_rl_separable(const mi_rl_ctx* ctx) { return ctx && ctx->separable ? (ctx->sep_single ? 2 : 1) : 0; }
extern "C" int mi_rl_sep_route(const mi_rl_ctx* ctx, int adjoint, int* out) {
    MI_REQUIRE(ctx && out, "mi_rl_sep_route: null pointer");
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (!(ctx->engine == MI_ENGINE_DIRECT && ctx->separable && ctx->sep_single)) return MI_OK;
    const SepRoute r = sep3d_route(ctx->n[0], ctx->n[1], ctx->n[2], ctx->k, adjoint ? ctx->off_adj : ctx->off_fwd);
    out[0] = r.acc ? 1 : 2;
    out[1] = r.kzb;
    out[2] = r.npre;
    out[3] = r.zchunk;
    out[4] = r.chunks;
    out[5] = (int)r.lds;
    return MI_OK;
}
extern "C" int mi_rl_pair_layout(const mi_rl_ctx* ctx) {
    return native_of(ctx) && native_of(ctx)->dims.paired ? 1 : 0;
}

static int ctx_conv(mi_rl_ctx* c, hipStream_t s, const float* in, bool adjoint, float* out, int epi_kind, const ConvEpilogue& epi) {
    if (c->engine == MI_ENGINE_DIRECT && c->separable && c->sep_single && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
        ((uintptr_t)epi.a % 16) == 0 && ((uintptr_t)epi.b % 16) == 0 && epi_kind != EPI_TAPER_SHELL)
        return sep3d_launch(s, in, out, c->n[0], c->n[1], c->n[2], adjoint ? c->sep_ta : c->sep_tf, adjoint ? c->off_adj : c->off_fwd, c->bnd,
                            epi_kind, epi);
    if (c->engine == MI_ENGINE_DIRECT && c->separable) {
        const size_t bytes = sizeof(float) * (size_t)c->n[0] * c->n[1] * c->n[2];
        if (!c->sep_t0.p) MI_TRY(c->sep_t0.alloc(bytes));
        if (!c->sep_t1.p) MI_TRY(c->sep_t1.alloc(bytes));
        const int* off = adjoint ? c->off_adj : c->off_fwd;
        DevBuf* tab = adjoint ? c->sep_adj : c->sep_fwd;
        const float* src = in;
        float* dsts[3] = {c->sep_t0.as<float>(), c->sep_t1.as<float>(), out};
        for (int d = 0; d < 3; ++d) {  // x, then y, then z; window offsets of the other axes are 0 for a 1-tap kernel
            const int o[3] = {d == 0 ? off[0] : 0, d == 1 ? off[1] : 0, d == 2 ? off[2] : 0};
            MI_TRY(direct_conv_launch(s, src, tab[d].as<float>(), dsts[d], c->n[0], c->n[1], c->n[2], d == 0 ? c->k[0] : 1, d == 1 ? c->k[1] : 1,
                                      d == 2 ? c->k[2] : 1, c->sep_kxp[d], c->bnd[0], d == 2 ? epi_kind : EPI_NONE, d == 2 ? epi : ConvEpilogue(), o,
                                      c->bnd));
            src = dsts[d];
        }
        return MI_OK;
    }
    if (c->engine == MI_ENGINE_DIRECT)
        return direct_conv_launch(s, in, adjoint ? c->kf_adj.as<float>() : c->kf_fwd.as<float>(), out, c->n[0], c->n[1], c->n[2], c->k[0],
                                  c->k[1], c->k[2], c->kxp, c->bnd[0], epi_kind, epi, adjoint ? c->off_adj : c->off_fwd, c->bnd);
    return c->fft->conv(s, in, adjoint, out, epi_kind, epi);
}

extern "C" int mi_rl_forward_ratio(mi_rl_ctx* ctx, void* stream, const float* bl, float* ratio) {
    MI_REQUIRE(ctx && bl && ratio && bl != ratio, "mi_rl_forward_ratio: null or aliased pointers");
    MI_TRY(use_device(ctx->dev));
    ConvEpilogue e;
    e.a = bl;
    return ctx_conv(ctx, as_stream(stream), bl, false, ratio, EPI_RATIO, e);
}

extern "C" int mi_rl_adjoint_update(mi_rl_ctx* ctx, void* stream, const float* ratio, float* bl, float lambda, const float* reg) {
    MI_REQUIRE(ctx && bl && ratio && bl != ratio, "mi_rl_adjoint_update: null or aliased pointers");
    MI_TRY(use_device(ctx->dev));
    ConvEpilogue e;
    e.a = bl;
    e.b = reg;
    e.lambda = lambda;
    const bool with_reg = lambda > 0.0f && reg != nullptr;
    return ctx_conv(ctx, as_stream(stream), ratio, true, bl, with_reg ? EPI_UPDATE_REG : EPI_UPDATE, e);
}

extern "C" int mi_rl_iterate(mi_rl_ctx* ctx, void* stream, float* bl, float* ratio, int n_iters) {
    MI_REQUIRE(ctx && bl, "mi_rl_iterate: null pointer");
    MI_REQUIRE(n_iters >= 0, "mi_rl_iterate: negative iteration count");
    MI_TRY(use_device(ctx->dev));
    if (NativeFft* nf = fusing_native(ctx)) return nf->iterate(as_stream(stream), bl, n_iters);
    MI_REQUIRE(ratio && ratio != bl, "mi_rl_iterate: this engine needs a ratio scratch volume");
    for (int i = 0; i < n_iters; ++i) {
        MI_TRY(mi_rl_forward_ratio(ctx, stream, bl, ratio));
        MI_TRY(mi_rl_adjoint_update(ctx, stream, ratio, bl, 0.0f, nullptr));
    }
    return MI_OK;
}

extern "C" int mi_fft_good_size(int n, int axis) {
    // extents the hand-written FFT pipeline takes without falling back to rocFFT: 2^a * {1, 3, 9} per axis (x: even, the
    // transform runs on x/2 complex points); 0 when no such extent exists (z beyond the LDS tile)
    if (axis < 0 || axis > 2 || n < 1) return 0;
    return NativeFft::good_size(n, axis);
}

extern "C" int mi_rl_fuses(mi_rl_ctx* ctx) {
    const NativeFft* nf = fusing_native(ctx);
    return !nf ? 0 : nf->splits() ? 2 : 1;
}

extern "C" int mi_rl_otf_is_real(mi_rl_ctx* ctx) {
    return native_of(ctx) && native_of(ctx)->real_otf ? 1 : 0;
}

extern "C" int mi_rl_otf_form(mi_rl_ctx* ctx, int* rank, int* rank_adj) {
    const NativeFft* f = native_of(ctx);
    if (rank) *rank = f ? f->otf_rank : 0;
    if (rank_adj) *rank_adj = f ? f->otf_rank_adj : 0;
    return !f || !f->real_otf ? 0 : f->otf_factored() ? 2 : 1;
}

extern "C" int mi_rl_fft_route(mi_rl_ctx* ctx, mi_fft_route* out) {
    MI_REQUIRE(ctx && out, "mi_rl_fft_route: null pointer");
    *out = mi_fft_route{};
    if (!native_of(ctx)) return MI_OK;
    const NativeFft& f = *native_of(ctx);
    const ZRoute z = z_route(f.dims, f.sw, f.real_otf);
    XCall fused;
    fused.fuse_forward = true;
    fused.ek = EPI_RATIO;
    out->native = 1;
    out->paired = f.dims.paired;
    out->z_kernel = z == ZRoute::conv ? 0 : (z == ZRoute::conv_pipe || z == ZRoute::conv_pipe_real) ? 1 : 2;
    out->real_otf = f.real_otf ? 1 : 0;
    out->x_pipelined = x_route(f.dims, f.sw, f.pw, fused) == XRoute::pipe_fused ? 1 : 0;
    out->x_splits = f.splits() ? 1 : 0;
    out->x_dynamic = x_tiles_dynamic(f.sw) ? 1 : 0;
    out->z_dynamic = z_tiles_dynamic(f.sw) ? 1 : 0;
    out->pruned = f.pw.on && !f.sw.no_prune ? 1 : 0;
    out->ty = f.dims.ty;
    out->tc = f.dims.tc;
    out->tl = f.dims.tl;
    out->z_full_grid = z_full_grid(f.dims, f.sw) ? 1 : 0;
    return MI_OK;
}

extern "C" size_t mi_rl_spectrum_row_floats(mi_rl_ctx* ctx) {
    return fusing_native(ctx) ? fusing_native(ctx)->spectrum_row_floats() : 0;
}

extern "C" size_t mi_rl_fft_spectrum_bytes(mi_rl_ctx* ctx) {
    return native_of(ctx) ? native_of(ctx)->spectrum_bytes() : 0;
}

