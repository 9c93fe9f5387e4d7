// Internal interface of the hand-written FFT convolution pipeline: the plan (fft_native.hip), its passes (fft_native_x.hip,
// fft_native_yz.hip; device building blocks in fft_native_dev.h) and where its arrays lie
// (fft_native_place.hip).  The grid's geometry, the plan's switches and the kernel route of every pass are pure host functions in
// fft_native_route.h.
#pragma once
#include <vector>
#include <algorithm>
#include "conv3d_direct.h"
#include "fft_native_route.h"

namespace mi {

// Subset of the y tiles of the fused x pass: mode 0 all, 1 only the tiles [lo0, lo0+n0) and [lo1, lo1+n1), 2 all the others
struct TileSelect {
    int mode = 0, lo0 = 0, n0 = 0, lo1 = 0, n1 = 0;
    int z0 = 0, nz = 0;  // only the planes [z0, z0 + nz) (nz = 0: all): the z-chunked halo exchange runs the edge tiles chunk by chunk
};

// While one of these exists on a thread, the contexts that thread creates take their spectrum arrays as they come instead of placing
// them by trial (NativeFft::init): the whole-loop entry points (mi_decon, mi_decon_plan_run, mi_rl_fft) run a handful of iterations per
// context, the trial costs 0.5 s, holds six candidates of the arrays, is serialised per device and trims the pool -- with five
// decwrap workers on blocks of 1024^3 it made 27 blocks take 14.5 s (profiles/r05_decwrap_scale.txt).  Contexts made with
// mi_rl_create (a bench, a slab rank: thousands of iterations on one placement) are placed by trial as before.
struct NoPlacementTrial {
    NoPlacementTrial();
    ~NoPlacementTrial();
    NoPlacementTrial(const NoPlacementTrial&) = delete;
    NoPlacementTrial& operator=(const NoPlacementTrial&) = delete;
    static bool active();  // one exists on the calling thread
};

struct NativeFft {
    // ---- the plan (fft_native.hip)
    NativeDims dims{};
    NativeSwitches sw;  // the environment at the moment of init, for the plan's whole life
    DevBuf S, G, G_adj, tw;  // S: both spectrum arrays, S first
    float2* t_spec = nullptr;  // the second spectrum array T (inside S's allocation, or place.T2 when the arrays were placed by trial)
    DevBuf Gr, Gr_adj, ph;  // real form of the OTF(s) + phase tables (symmetric PSFs), see try_real_otf
    bool real_otf = false;
    // the real OTF(s) as rank-R factors (otf_factor.h): per slot the four A_r by z position, then the four Bh_r of every line (xk, py,
    // side); Gr / Gr_adj are released when these are adopted (try_factored_otf)
    DevBuf Gf, Gf_adj;
    int otf_rank = 0, otf_rank_adj = 0;  // 0: not factored
    bool otf_factored() const { return otf_rank > 0; }
    bool have_adj = false;  // adjoint = second OTF (G_adj) instead of conj(G)
    const float2* tw_x = nullptr;
    const float2* tw_y = nullptr;
    const float2* tw_z = nullptr;
    const float2* tw_plane = nullptr;  // exp(-2 pi i xk / (2 Hx)), xk <= Hx/2, behind the axis tables in `tw` (fill_plane_twiddles: the paired z pass)
    size_t n_cplx = 0;
    size_t spec_bytes = 0;
    int n_cu = 256;  // persistent kernels launch one work-group per CU
    ~NativeFft();

    static bool supported(const int F[3]) { return native_supported(F); }
    // smallest supported extent >= n of axis 0 (x), 1 (y), 2 (z); 0 when there is none
    static int good_size(int n, int axis) { return native_good_size(n, axis); }
    // buffers, tile sizes, twiddles; the OTF(s) are then built with build_otf
    int init(hipStream_t s, const int F[3], bool explicit_adjoint);
    // placed: the kernel on the circular grid (real, shape F; may alias scratch()); G (or G_adj) <- scale * FFT(placed)
    int build_otf(hipStream_t s, const float* placed, bool adjoint_slot, float scale);
    // the same transform into a caller buffer of otf_items() float4: spectrum of any real F volume, scaled (deconFFT_Wiener)
    int spectrum(hipStream_t s, const float* vol, float4* dst, float scale);
    size_t otf_items() const { return G.bytes / sizeof(float4); }
    float4* otf() { return G.as<float4>(); }
    // after build_otf: switch to the real OTF form when the PSF allows it (delta: centre offset from the grid origin)
    int try_real_otf(hipStream_t s, const int delta[3]);
    // after try_real_otf adopted the real form: factor the PSF(s) (device pointers, extents k = (x, y, z), centre offset delta as for try_real_otf) and, when the tables rebuild
    // Gr to the criterion of the real form itself, keep the tables instead of the arrays.  `scale`: the scale build_otf was given.
    int try_factored_otf(hipStream_t s, const float* psf, const float* psf_adj, const int k[3], const int delta[3], float scale);
    float* scratch() { return reinterpret_cast<float*>(t_spec); }  // F floats, free between convolutions
    // after the OTFs are built: volumes handed to conv / iterate have extents n (x, y, z) and are padded on the fly
    void set_window(const int n[3], const int o[3], const int rep[3], const int k[3]);
    bool can_fuse() const { return pad_can_fuse(pw); }  // consecutive convolutions may share their x passes (every padded axis follows the zero rule)
    int conv(hipStream_t s, const float* in, bool conj_otf, float* out, int epi_kind, const ConvEpilogue& epi);
    // `conj_otf` selects the adjoint: conj(OTF), or the explicit adjoint OTF when one was given
    // n fused RL iterations on bl in place (lambda = 0, no regularisation step in between)
    int iterate(hipStream_t s, float* bl, int n_iters);
    size_t spectrum_bytes() const { return spec_bytes; }   // one of the two spectrum arrays
    size_t spectrum_row_floats() const { return (size_t)2 * dims.nz * dims.hx; }
    size_t device_bytes() const {
        return S.bytes + place.T2.bytes + place.S_alt.bytes + G.bytes + G_adj.bytes + Gr.bytes + Gr_adj.bytes + Gf.bytes + Gf_adj.bytes + ph.bytes + tw.bytes;
    }

    // ---- the passes (fft_native_x.hip, fft_native_yz.hip)
    int fill_plane_twiddles(hipStream_t s, float2* dst);
    int x_forward(hipStream_t s, const float* in);
    int middle(hipStream_t s, bool conj_otf);
    int y_pass(hipStream_t s, bool inverse, YRoute route, const float2* src = nullptr, float2* dst = nullptr, int xk0 = 0, int xkn = -1);
    int z_conv(hipStream_t s, bool conj_otf, const float2* src = nullptr, float2* dst = nullptr, int xk0 = 0, int xkn = -1);
    int x_inverse(hipStream_t s, float* out, int epi_kind, const ConvEpilogue& epi, bool fuse_forward, const TileSelect* part = nullptr);
    bool z_pipelined() const { return z_pipe_ok(dims, sw); }
    // rows [y0, y0 + rows) of S (the x-transformed input of the next convolution): dir 0 pack into buf, 1 unpack from buf, 2 zero
    // (z0, nzc: only the planes [z0, z0 + nzc), which keep their place in the packed buffer; nzc = 0: all)
    int spectrum_rows(hipStream_t s, int y0, int rows, float2* buf, int dir, int z0 = 0, int nzc = 0);
    // forward y pass of the planes [z0, z0 + nzc) only (both layouts); z0 and nzc multiples of y_z_granule()
    int y_forward_planes(hipStream_t s, int z0, int nzc);
    int y_z_granule() const { return dims.paired ? std::max(1, dims.tc / 2) : 1; }

    // ---- pad window and tiles of the x passes
    PadWindow pw{};
    bool pipe_ok() const { return x_pipe_ok(dims, sw); }  // the fused x pass can run as the persistent pipelined kernel
    bool splits() const { return !pw.on && pipe_ok(); }   // ... and a subset of its tiles (unpadded grids)
    TileSelect edge_tiles(int mode, int a0, int a1, int b0, int b1) const;
    // padded grids take the persistent x kernels too: zero rule, data at the origin, whole float4 rows and what the call site asks
    // of its pointers (`aligned`)
    bool pad_pipe(bool aligned) const { return x_pad_pipe(dims, sw, pw, aligned); }
    // tiles of a pipelined x launch: those of the pad window (`padded`), else the caller's subset `part`, else all
    int pipe_tiles(bool padded, const TileSelect* part, TileSelect* sel, int* ntiles) const;
    // k_x_fused_pipe<.., mode> on those tiles (mode 0 fused, 1 forward only, 2 inverse only)
    int x_pipelined(hipStream_t s, int mode, const float2* T, float* out, const ConvEpilogue& epi, int ek, const TileSelect& sel, int ntiles);
    // x launches that run beside a halo exchange (part 2 of a sharded step): compute units left free for the collective's
    // kernels, tiles handed out by a device counter instead of a fixed stride (mi_rl_set_overlap)
    int overlap_free_cus = 0;
    bool overlap_dynamic = true;
    DevBuf ctr;   // (every other persistent x launch and the paired z pass take their tiles from a counter too: x_tiles_dynamic, z_tiles_dynamic)
    int ctr_slot = 0;
    int persistent_grid(hipStream_t s, int ntiles, bool overlapped, unsigned* grid, int** ctr_out);

    // ---- where the spectrum arrays lie (fft_native_place.hip)
    struct Placement {
        DevBuf T2, S_alt;  // S_alt: a second buffer for S, kept until the caller's volume is known (settle_decide)
        int alt_phase = 0;  // 0 / 1: the next timed update launch writes the first / second S buffer; 2: decide; 3: settled
        hipEvent_t alt_ev[4] = {nullptr, nullptr, nullptr, nullptr};
        std::vector<float> placement_ms;  // cost of each candidate placement of the spectrum arrays (place_by_trial)
        int placement_kept = -1;
    } place;
    // the two arrays on the best ordered pair of several buffers allocated side by side (init: large plans only; gap: bytes between
    // S and T in init's single allocation, which stands when the candidates do not fit)
    int place_by_trial(hipStream_t s, size_t gap);
    void settle_before_update();
    int settle_decide(hipStream_t s);
    // the spare buffer for S goes back to the driver (every consumer of S other than iterate() calls this first: the sharded steps of
    // the slab driver, single convolutions -- a C4-shaped rank carried 9.7 GB of it for the whole run)
    int release_spare();

    // ---- timing (bench.py's roofline leg; fft_native_place.hip)
    int time_pass(hipStream_t s, int which, const float* bl, int reps, float* avg_ms);
    int time_between(hipStream_t s, int which, const float2* src, float2* dst, float* bl, int reps, float* avg_ms);
};

}  // namespace mi
