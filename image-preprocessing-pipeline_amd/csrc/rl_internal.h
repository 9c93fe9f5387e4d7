// Internal interface of the Richardson-Lucy units: the context every one of them works on and the few helpers they share.
//   rl.hip          the context: creation, queries, the two fused passes of an iteration, mi_rl_iterate
//   rl_sharded.hip  the slab driver's iteration, cut where the halos of a convolution's input are refreshed
//   rl_probe.hip    measurement entries no product path calls
//   rl_decon.hip    the decon.m drivers (deconSpatial / deconFFT / deconFFT_Wiener) and the deconvolution plan
#pragma once
#include "fftconv.h"

struct mi_rl_ctx {
    int dev = 0;
    int n[3] = {0, 0, 0};
    int k[3] = {0, 0, 0};
    int bnd[3] = {MI_BOUNDARY_ZERO, MI_BOUNDARY_ZERO, MI_BOUNDARY_ZERO};
    int engine = MI_ENGINE_DIRECT;
    // direct engine: tap tables + window offsets for the forward and adjoint kernels
    mi::DevBuf kf_fwd, kf_adj;
    int kxp = 0;
    int off_fwd[3] = {0, 0, 0}, off_adj[3] = {0, 0, 0};
    // separable fast path of the direct engine: a PSF that is an outer product a (x) b (x) c (a Gaussian: BASELINE config 1) is
    // applied as three 1-D convolutions -- kx + ky + kz instead of kx * ky * kz taps per voxel; the RL epilogue rides on the last
    bool separable = false;
    mi::DevBuf sep_fwd[3], sep_adj[3];  // 1-D tap tables per axis
    int sep_kxp[3] = {0, 0, 0};
    mi::DevBuf sep_t0, sep_t1;          // intermediate volumes of the three-launch route (allocated with its first convolution)
    mi::SepTaps sep_tf[3], sep_ta[3];   // the same taps in window order for the single-pass kernel (sep3d.hip)
    bool sep_single = false;            // ... which takes this PSF (tap counts, LDS ring of kz planes, whole float4 rows)
    mi::FftEngine* fft = nullptr;
    ~mi_rl_ctx() { delete fft; }
};

namespace mi {

// rl.hip: mi_rl_create_ex with the choice deconFFT_Wiener needs (fixed_psf = false: the OTF keeps its general complex form)
int rl_create(int dev, void* stream, int nx, int ny, int nz, const float* psf, const float* psf_inv, int kx, int ky, int kz,
              const int* boundary_xyz, const int* shift_xyz, int engine, bool fixed_psf, mi_rl_ctx** out);
// rl_sharded.hip: the fusing native pipeline of `ctx` with its spare array released, or an error
int sharded_native(mi_rl_ctx* ctx, NativeFft** out);

// the hand-written FFT pipeline of a context, or null (another engine, a rocFFT-only shape, no context)
inline NativeFft* native_of(const mi_rl_ctx* ctx) { return ctx && ctx->engine == MI_ENGINE_FFT && ctx->fft ? ctx->fft->native : nullptr; }
// ... when consecutive convolutions may share their x passes
inline NativeFft* fusing_native(const mi_rl_ctx* ctx) { return native_of(ctx) && native_of(ctx)->can_fuse() ? native_of(ctx) : nullptr; }

// edge row ranges [e0,e1) and [e2,e3) of a split x pass
inline int check_edge_rows(const char* who, const int* edges, int ny) {
    MI_REQUIRE(edges && edges[0] >= 0 && edges[0] < edges[1] && edges[1] <= edges[2] && edges[2] < edges[3] && edges[3] <= ny,
               "%s: edge row ranges must be ordered and inside the volume", who);
    return MI_OK;
}

// what every decon.m driver asks of its block and PSF; F (null: deconSpatial) adds pad_block_to_fft_shape's two requirements
inline int check_decon_shapes(const char* who, const void* bl, const void* psf, const int n[3], const int k[3], const int* F) {
    MI_REQUIRE(bl && psf, "%s: null pointer", who);
    MI_REQUIRE(n[0] > 0 && n[1] > 0 && n[2] > 0 && k[0] > 0 && k[1] > 0 && k[2] > 0, "%s: bl and psf must be 3D and non-empty", who);
    if (!F) return MI_OK;
    MI_REQUIRE(F[0] >= n[0] && F[1] >= n[1] && F[2] >= n[2], "pad_block_to_fft_shape: bl [%d %d %d] is larger than FFT shape [%d %d %d], cannot pad",
               n[0], n[1], n[2], F[0], F[1], F[2]);
    MI_REQUIRE(F[0] >= k[0] && F[1] >= k[1] && F[2] >= k[2], "pad_block_to_fft_shape: psf [%d %d %d] is larger than FFT shape [%d %d %d], cannot pad",
               k[0], k[1], k[2], F[0], F[1], F[2]);
    return MI_OK;
}

// A context a driver created and nobody keeps: destroyed on every exit, once the stream no longer uses it (c == null: nothing held)
struct CtxGuard {
    mi_rl_ctx* c;
    hipStream_t s;
    ~CtxGuard() { if (c) { (void)hipStreamSynchronize(s); mi_rl_destroy(c); } }
};

}  // namespace mi
