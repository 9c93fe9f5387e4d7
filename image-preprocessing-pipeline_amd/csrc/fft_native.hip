// Hand-written FFT convolution pipeline for gfx950 (engine MI_ENGINE_FFT whenever every transform length is 2^a * {1,3,9};
// rocFFT remains the fallback for other shapes).
//
// Why: the rocFFT R2C/C2R route costs 12 transform kernels + multiply + epilogue per convolution
// (profiles/r01_bench_c3_rocfft_kernel_stats.csv: 62 ms per convolution on C3, its strided z pass alone
// 13.8 ms).  The RL iteration is HBM-bound, so the design goal is the minimum number of full-volume passes
// with every global access in >= 64-B contiguous segments:
//
//   real volume (Z,Y,X) is read as complex rows of Hx = X/2 samples z[n] = x[2n] + i x[2n+1]; a COMPLEX 3-D FFT
//   of size (Z, Y, Hx) is taken; the real-spectrum untangling, the OTF product and the re-tangling are done
//   point-wise on mirror pairs (k, -k) in the middle pass, so no (X/2+1)-wide array ever exists.
//
//   P1  x forward   rows -> LDS -> DIF FFT(Hx) -> S[z][px][y]            (transposed write: y fastest, px stride 16 KB)
//   P2  y forward   whole contiguous columns: S[z][px][.] -> T[px][z][.]   (the re-layout is free: 16-KB chunks)
//   P3  z forward + untangle * OTF (or conj / explicit adjoint OTF) + retangle + z inverse, on mirror line pairs,
//                   T -> S, both [px][z][py] (z stride 16 KB instead of 16 MB in the [z][px][py] layout)
//   P4  y inverse   S[px][z][.] -> T[z][px][.]
//   P5  x inverse   T[z][px][y] -> LDS -> DIT IFFT(Hx) -> real row -> fused RL epilogue -> out
//   P5+P1 fused     ... -> epilogue result stays in LDS -> DIF FFT(Hx) -> S of the NEXT convolution (8 passes / RL iteration)
//
// Forward transforms are decimation-in-frequency (natural in, permuted out), inverse ones decimation-in-time
// (permuted in, natural out), so no reordering pass exists: frequency-domain arrays simply live in permuted
// positions (px, py, pz) and the OTF is built by the pipeline itself in that order (k_z_conv<BUILD>).  (x of 2048 and 4096 samples:
// the positions are rotated once more, so that the bottom super-stage of the fused x pass needs no LDS -- x_rotated().)
// Each transform runs inside LDS as super-stages of 3 fused radix-2 stages held in registers (8 points per lane);
// see "LDS image" and "super-stage chains" (fft_native_dev.h) and the pipelined kernels (fft_native_x.hip, fft_native_yz.hip) for
// how the LDS, VALU and HBM phases are kept conflict-free, short and overlapped.
//
// This file is the plan: sizes, buffers, twiddles and the order of the passes.  The kernels live with their launchers in
// fft_native_x.hip (x passes) and fft_native_yz.hip (y and z passes) on top of fft_native_dev.h; where the spectrum arrays lie and
// the timing entry points are fft_native_place.hip.
#include "fft_native_dev.h"

namespace mi {

// The switches of a plan, from the environment of this moment: the only place of the pipeline that reads it (names, defaults and
// clamping of every switch are the public ones of DESIGN section 5; MI_PROBE_ENV: the probe build's experiments, absent from the product)
static NativeSwitches read_switches() {
    NativeSwitches w;
    const auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    const auto mb = [](const char* name, size_t dflt) {
        const char* e = std::getenv(name);
        return e ? (size_t)std::max(0LL, atoll(e)) << 20 : dflt;
    };
    w.no_pair = set("MI_FFT_NO_PAIR");
    w.no_pipe = set("MI_FFT_NO_PIPE");
    w.no_xpipe = set("MI_FFT_NO_XPIPE");
    w.no_prune = set("MI_FFT_NO_PRUNE");
    w.complex_otf = set("MI_FFT_COMPLEX_OTF");
    w.stored_otf = set("MI_FFT_STORED_OTF");
    w.z_general = set("MI_FFT_Z_GENERAL");
    if (const char* e = std::getenv("MI_X_DYN")) w.x_dyn = atoi(e) != 0;
    if (const char* e = std::getenv("MI_Z_DYN")) w.z_dyn = atoi(e) != 0;
    w.place_min = mb("MI_FFT_PLACE_MIN_MB", w.place_min);
    w.alt_min = mb("MI_FFT_PLACE_ALT_MIN_MB", w.alt_min);
    if (const char* e = std::getenv("MI_FFT_PLACE_CANDIDATES")) w.place_candidates = std::max(1, std::min(8, atoi(e)));
    w.place_log = set("MI_FFT_PLACE_LOG");
    if (const char* e = MI_PROBE_ENV("MI_FFT_ZDBG")) w.dbg = atoi(e);  // phase knock-out for timing experiments
    if (const char* e = MI_PROBE_ENV("MI_FFT_TY")) w.ty = std::max(2, atoi(e));  // tuning overrides
    if (const char* e = MI_PROBE_ENV("MI_FFT_TC")) w.tc = std::max(1, atoi(e));
    if (const char* e = MI_PROBE_ENV("MI_FFT_TL")) w.tl = std::max(2, atoi(e));
    if (const char* e = MI_PROBE_ENV("MI_FFT_ZPAD")) w.zpad = std::max(0, atoi(e));
    if (const char* e = MI_PROBE_ENV("MI_FFT_XPAD")) w.xpad = std::max(0, atoi(e));
    if (const char* e = MI_PROBE_ENV("MI_X_FREE_CUS")) w.x_free_cus = std::max(0, atoi(e));
    if (const char* e = MI_PROBE_ENV("MI_FFT_STGAP")) w.stgap = (size_t)atoll(e) & ~(size_t)127;
    return w;
}

// resolve the switches, the geometry (plan_geometry), allocate, fill the tables, place the arrays
int NativeFft::init(hipStream_t s, const int F[3], bool explicit_adjoint) {
    sw = read_switches();
    MI_REQUIRE(supported(F), "native FFT: unsupported shape %d x %d x %d", F[0], F[1], F[2]);
    NativeSizes sz{};
    const int miss = plan_geometry(F, sw, &dims, &sz);
    MI_REQUIRE(miss != 1, "native FFT: x tile of %d rows does not divide y = %d", dims.ty, F[1]);
    MI_REQUIRE(miss != 2, "native FFT: z tile of %d lines does not fit y = %d", dims.tl, F[1]);
    MI_REQUIRE(miss == 0, "native FFT: transform too long for LDS");
    const int Hx = dims.hx;
    const size_t n_buf = sz.n_buf, gap = sw.stgap;
    n_cplx = sz.n_cplx;
    // one allocation for both arrays, NativeSwitches::stgap apart
    // (measuring the passes for six distances at plan time did not pay: in a process where the y passes run in their slow mode
    // they do so for every distance tried)
    MI_TRY(S.alloc(sizeof(float2) * 2 * n_buf + gap));
    t_spec = S.as<float2>() + n_buf + gap / sizeof(float2);
    spec_bytes = sizeof(float2) * n_buf;
    MI_TRY(G.alloc(sizeof(float4) * (size_t)(Hx / 2 + 1) * F[1] * F[2]));
    // twiddle tables exp(-2 pi i e / N) in double on the host, per axis (NativeSizes)
    const int lens[3] = {Hx, F[1], F[2]};
    const int subs[3] = {1 << dims.lhx2, 1 << dims.ly2, 1 << dims.lz2};
    const size_t off = sz.tw_total, *offs = sz.tw_at;
    std::vector<float2> h(off);
    const double two_pi = 6.283185307179586476925286766559;
    for (int a = 0; a < 3; ++a) {
        for (int e = 0; e < subs[a] / 2; ++e)
            h[offs[a] + e] = make_float2((float)std::cos(two_pi * e / subs[a]), (float)-std::sin(two_pi * e / subs[a]));
        if (lens[a] != subs[a])
            for (int e = 0; e < lens[a]; ++e)
                h[offs[a] + subs[a] / 2 + e] = make_float2((float)std::cos(two_pi * e / lens[a]), (float)-std::sin(two_pi * e / lens[a]));
    }
    MI_TRY(tw.alloc(sizeof(float2) * (off + (size_t)(Hx / 2 + 1))));  // (behind the axis tables: the plane twiddles of the paired z pass)
    MI_HIP(hipMemcpyAsync(tw.p, h.data(), sizeof(float2) * off, hipMemcpyHostToDevice, s));
    MI_TRY(fill_plane_twiddles(s, tw.as<float2>() + off));
    tw_x = tw.as<float2>() + offs[0];
    tw_y = tw.as<float2>() + offs[1];
    tw_z = tw.as<float2>() + offs[2];
    {
        int devid = 0, cus = 0;
        MI_HIP(hipGetDevice(&devid));
        MI_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devid));
        n_cu = cus > 0 ? cus : 256;
    }
    have_adj = explicit_adjoint;
    if (have_adj) MI_TRY(G_adj.alloc(G.bytes));  // explicit adjoint kernel (psf_inv of the 'same'-convolution flavour) instead of conj(OTF)
    MI_HIP(hipStreamSynchronize(s));  // host twiddle vector dies at scope exit
    // large arrays are placed by trial (fft_native_place.hip): MI_FFT_PLACE_MIN_MB (6144, both together) and more -- smaller plans are
    // not tried: decwrap creates its block plans, 3-4 GB each, on several workers per device while others compute, and every released
    // candidate is a device-wide synchronisation (slab.SlabRL lowers the limit for its rank, which has its device to itself)
    if (S.bytes >= sw.place_min && !NoPlacementTrial::active()) MI_TRY(place_by_trial(s, gap));
    return MI_OK;
}

void NativeFft::set_window(const int n[3], const int o[3], const int rep[3], const int k[3]) {
    pw.on = 1;
    if (place.S_alt.p && place.alt_phase < 3) {   // (padded grids do not settle S on their update launches: the second buffer is not needed;
        // nothing to undo: S.p is whichever buffer the last launch wrote)
        (void)hipFree(place.S_alt.p);
        place.S_alt.p = nullptr;
        place.S_alt.bytes = 0;
        place.alt_phase = 3;
    }
    for (int a = 0; a < 3; ++a) {
        pw.n[a] = n[a];
        pw.o[a] = o[a];
        pw.rep[a] = rep[a];
        pw.w[a] = n[a] + k[a] - 1;
    }
    // what the padding leaves to prune (MI_FFT_NO_PRUNE=1 keeps the full passes, for A/B measurements)
    if (sw.no_prune) return;
    const int in_hi = rep[2] ? pw.w[2] : o[2] + n[2];
    dims.z_in_hi = std::min(in_hi, dims.nz);
    dims.z_out_lo = o[2];
    dims.z_out_hi = std::min(o[2] + n[2], dims.nz);
    const int yh = ((o[1] + n[1] + dims.ty - 1) / dims.ty) * dims.ty;  // the x pass reads whole tiles of rows
    dims.y_out_hi = std::min(yh, dims.ny);
}

// P2, P3, P4: S[z][px][py] -> T[z][px][py] (x still transformed), multiplied by the OTF or its conjugate
int NativeFft::middle(hipStream_t s, bool conj_otf) {
    MI_TRY(y_pass(s, false, y_route(dims)));
    MI_TRY(z_conv(s, conj_otf));
    return y_pass(s, true, y_route(dims));
}

NativeFft::~NativeFft() {
    for (auto& e : place.alt_ev)
        if (e) (void)hipEventDestroy(e);
}

static int check_aligned(const void* p, const char* what) {
    MI_REQUIRE(p == nullptr || ((uintptr_t)p % 16) == 0, "native FFT: %s must be 16-byte aligned", what);
    return MI_OK;
}

int NativeFft::conv(hipStream_t s, const float* in, bool conj_otf, float* out, int epi_kind, const ConvEpilogue& epi) {
    if (!pw.on) {  // 16-byte accesses on the caller's volumes; the padded mode reads and writes them element-wise
        MI_TRY(check_aligned(in, "input"));
        MI_TRY(check_aligned(out, "output"));
        MI_TRY(check_aligned(epi.a, "epilogue operand"));
        MI_TRY(check_aligned(epi.b, "epilogue operand"));
    }
    MI_TRY(release_spare());
    MI_TRY(x_forward(s, in));
    MI_TRY(middle(s, conj_otf));
    return x_inverse(s, out, epi_kind, epi, false);
}

// n whole RL iterations (decon.m:162-186 with lambda = 0) in 8 passes each: the x passes of consecutive
// convolutions are fused, so per iteration bl is read twice and written once and the ratio never exists in HBM.
// (Which of the two buffers kept for S goes with the caller's volume is settled on the first update launches of this loop:
// settle_before_update, fft_native_place.hip.)
int NativeFft::iterate(hipStream_t s, float* bl, int n_iters) {
    if (!pw.on) MI_TRY(check_aligned(bl, "bl"));
    MI_REQUIRE(can_fuse(), "native FFT: a replicate-padded axis cannot fuse consecutive convolutions");
    if (n_iters <= 0) return MI_OK;
    ConvEpilogue e;
    e.a = bl;
    if (place.S_alt.p && place.alt_phase == 2) MI_TRY(settle_decide(s));   // (see settle_before_update)
    MI_TRY(x_forward(s, bl));
    for (int it = 0; it < n_iters; ++it) {
        MI_TRY(middle(s, false));
        if (place.S_alt.p && place.alt_phase == 2) MI_TRY(settle_decide(s));
        MI_TRY(x_inverse(s, nullptr, EPI_RATIO, e, true));   // ratio = bl ./ max(c, eps) -> S, not stored
        MI_TRY(middle(s, true));
        const bool fuse = it + 1 < n_iters, timed = place.S_alt.p != nullptr && place.alt_phase < 2 && fuse && !pw.on;
        if (timed) {
            settle_before_update();
            if (!place.alt_ev[0]) for (auto& ev : place.alt_ev) MI_HIP(hipEventCreate(&ev));
            (void)hipEventRecord(place.alt_ev[2 * place.alt_phase], s);
        }
        MI_TRY(x_inverse(s, bl, EPI_UPDATE, e, fuse));  // bl = |bl .* a| (-> S for the next iteration)
        if (timed) {
            (void)hipEventRecord(place.alt_ev[2 * place.alt_phase + 1], s);
            ++place.alt_phase;
        }
    }
    return MI_OK;
}

}  // namespace mi
