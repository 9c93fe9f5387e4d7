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

// An axis length n = r3 * 2^l2 with r3 in {1, 3, 9}: powers of two from 8 to 4096, or 3 * / 9 * (32 .. 512).  (A radix-3/9
// factor matters most on y, the axis the slab driver shards, where slab + halos is rarely a power of two; on x and z it
// keeps zero-padded deconFFT shapes close to the 7-smooth ones.)
static bool split_axis(int n, int* r3, int* l2, bool five = false) {
    for (int r : {1, 3, 5, 9}) {
        if (n % r || (r == 5 && !five)) continue;
        const int m = n / r;
        if (!is_pow2(m)) continue;
        const int l = ilog2(m);
        if (r == 1 ? (l >= 3 && l <= 12) : (l >= 5 && l <= (r == 5 ? 8 : 9))) { *r3 = r; *l2 = l; return true; }
    }
    return false;
}

static const int kMaxZ = 2304;  // 2 * TL >= 4 rows of the z pass must fit the LDS tile
static const int kMaxLen = 9 << 9;  // the longest length of split_axis

bool NativeFft::supported(const int F[3]) {
    // x: real length 2 * Hx, the transform runs on Hx complex points
    int r3, l2;
    return F[0] % 2 == 0 && split_axis(F[0] / 2, &r3, &l2) && split_axis(F[1], &r3, &l2, true) && split_axis(F[2], &r3, &l2) && F[2] <= kMaxZ;
}

int NativeFft::good_size(int n, int axis) {
    // (the searches end at the longest length split_axis takes, 9 * 2^9: beyond it there is no extent, and the answer is 0)
    int r3, l2;
    if (axis == 0) {
        for (int h = n < 16 ? 8 : (n + 1) / 2; h <= kMaxLen; ++h)
            if (split_axis(h, &r3, &l2)) return 2 * h;
        return 0;
    }
    for (int m = n < 8 ? 8 : n; m <= (axis == 2 ? kMaxZ : kMaxLen); ++m)
        if (split_axis(m, &r3, &l2, axis == 1)) return m;
    return 0;
}

int NativeFft::init(hipStream_t s, const int F[3], bool explicit_adjoint) {
    MI_REQUIRE(supported(F), "native FFT: unsupported shape %d x %d x %d", F[0], F[1], F[2]);
    const int Hx = F[0] / 2;
    split_axis(Hx, &dims.r3x, &dims.lhx2);
    split_axis(F[1], &dims.r3, &dims.ly2, true);  // (the y axis also takes 5 * 2^a: 320 rows of a slab rank instead of 384)
    split_axis(F[2], &dims.r3z, &dims.lz2);
    dims.hx = Hx;
    dims.xrot = x_rotated(dims.lhx2, dims.r3x) ? 1 : 0;
    dims.ny = F[1];
    dims.nz = F[2];
    dims.ty = std::min(x_tile_rows(Hx), F[1]);
    dims.tc = y_tile_cols(F[1]);
    dims.tl = std::min(z_tile_lines(F[2]), F[1]);
    dims.z_in_hi = F[2];
    dims.z_out_lo = 0;
    dims.z_out_hi = F[2];
    dims.y_out_hi = F[1];
    dims.xk0 = 0;
    dims.xkn = Hx / 2 + 1;
    dims.yz0 = 0;
    dims.dbg = 0;
    if (const char* e = MI_PROBE_ENV("MI_FFT_ZDBG")) dims.dbg = atoi(e);  // phase knock-out for timing experiments
    // tuning overrides (experiments only): MI_FFT_TY / MI_FFT_TC / MI_FFT_TL
    if (const char* e = MI_PROBE_ENV("MI_FFT_TY")) dims.ty = std::max(2, std::min(atoi(e), F[1]));
    if (const char* e = MI_PROBE_ENV("MI_FFT_TC")) dims.tc = std::max(1, atoi(e));
    if (const char* e = MI_PROBE_ENV("MI_FFT_TL")) dims.tl = std::max(2, std::min(atoi(e), F[1]));
    while ((size_t)F[2] * Hx % dims.tc) dims.tc >>= 1;
    // tiles are whole float4 groups of rows / lines and must divide y; z tiles of TL positions must map onto aligned
    // mirror blocks, which holds for TL <= 2^ly2 (positions inside one power-of-two sub-block mirror inside one)
    MI_REQUIRE(dims.ty >= 2 && dims.ty % 2 == 0 && F[1] % dims.ty == 0, "native FFT: x tile of %d rows does not divide y = %d", dims.ty, F[1]);
    MI_REQUIRE(dims.tl >= 2 && is_pow2(dims.tl) && dims.tl <= (1 << dims.ly2), "native FFT: z tile of %d lines does not fit y = %d", dims.tl, F[1]);
    MI_REQUIRE(lds_bytes(dims.ty, Hx) <= 160 * 1024 && lds_bytes(dims.tc, F[1]) <= 160 * 1024 &&
                   lds_bytes(2 * dims.tl, F[2]) <= 160 * 1024,
               "native FFT: transform too long for LDS");
    // pair-interleaved z-side layout (k_y_pair / k_z_pair_pipe): z a power of two the paired z pass takes, whole blocks of
    // kPairLines lines, an even number of columns per y tile; MI_FFT_NO_PAIR=1 keeps the plain layout (A/B measurements)
    const bool z_pairs = dims.r3z == 1 ? (dims.lz2 >= 6 && dims.lz2 <= 10)
                         : dims.r3z == 3 ? (dims.lz2 >= 6 && dims.lz2 <= 8) : (dims.r3z == 9 && dims.lz2 >= 6 && dims.lz2 <= 7);
    dims.paired = z_pairs && F[1] % (2 * kPairLines) == 0 && dims.tc >= 2 && dims.tc % 2 == 0 &&
                  F[2] % (dims.tc / 2) == 0 && dims.dbg == 0 && std::getenv("MI_FFT_NO_PAIR") == nullptr &&
                  std::getenv("MI_FFT_NO_PIPE") == nullptr && MI_PROBE_ENV("MI_FFT_TL") == nullptr;
    n_cplx = (size_t)Hx * F[1] * F[2];
    // (the two planes that are their own mirror partners are stored twice in the paired layout)
    // Rows an exact power of two apart camp on few HBM channels: behind every row of the x side ([z][px][.]) and of the paired z
    // side ([xk][z][.]) that is at least 8 KB long lie 4 KB + 128 B of padding.  C3 (profiles/zpad_probe.py): z pass 4.75 -> 4.2 ms
    // with any odd multiple of 128 B behind the z rows (64-byte offsets break the 128-byte lines: 6.2 ms); with 4 KB + 128 B
    // on both sides the y passes drop from 3.2-3.35 to 2.85-3.35 ms and the x pass from 5.1 / 6.0-7.2 to 4.75 / 5.7-6.8 ms.
    const int pad_x = (size_t)F[1] * sizeof(float2) >= kPadRowBytes ? kRowPadBytes : 0;
    const int pad_z = (size_t)F[1] * 2 * sizeof(float2) >= kPadRowBytes ? kRowPadBytes : 0;
    dims.zpad = dims.paired ? pad_z / 16 : 0;
    dims.xrow = F[1] + pad_x / 8;
    if (const char* e = MI_PROBE_ENV("MI_FFT_ZPAD")) dims.zpad = dims.paired ? std::max(0, atoi(e)) : 0;   // float4 per row
    if (const char* e = MI_PROBE_ENV("MI_FFT_XPAD")) dims.xrow = F[1] + 2 * std::max(0, atoi(e));          // float4 per row
    const size_t n_x = (size_t)Hx * F[2] * dims.xrow;
    const size_t n_buf = std::max(n_x, dims.paired ? (size_t)(Hx / 2 + 1) * F[2] * 2 * (size_t)(F[1] + dims.zpad) : n_cplx);
    // one allocation for both arrays: their distance -- which decides how the strided streams of a pass that reads one and
    // writes the other fall onto the HBM channels -- is then the same in every context instead of whatever the driver returns
    // (measuring the passes for six distances at plan time did not pay: in a process where the y passes run in their slow mode
    // they do so for every distance tried)
    size_t gap = kSpecGapBytes;
    if (const char* e = MI_PROBE_ENV("MI_FFT_STGAP")) gap = (size_t)atoll(e) & ~(size_t)127;
    MI_TRY(S.alloc(sizeof(float2) * 2 * n_buf + gap));
    t_spec = S.as<float2>() + n_buf + gap / sizeof(float2);
    spec_bytes = sizeof(float2) * n_buf;
    MI_TRY(G.alloc(sizeof(float4) * (size_t)(Hx / 2 + 1) * F[1] * F[2]));
    // twiddle tables exp(-2 pi i e / N) in double on the host, per axis: e < sub/2 for the power-of-two sub-transform
    // (sub = 2^l2), followed by the full circle e < n of the radix-3/9 stage when the axis has one
    const int lens[3] = {Hx, F[1], F[2]};
    const int subs[3] = {1 << dims.lhx2, 1 << dims.ly2, 1 << dims.lz2};
    size_t off = 0, offs[3];
    for (int a = 0; a < 3; ++a) { offs[a] = off; off += (size_t)std::max(1, subs[a] / 2) + (lens[a] != subs[a] ? (size_t)lens[a] : 0); }
    std::vector<float2> h(off);
    const double two_pi = 6.283185307179586476925286766559;
    for (int a = 0; a < 3; ++a) {
        for (int e = 0; e < subs[a] / 2; ++e)
            h[offs[a] + e] = make_float2((float)std::cos(two_pi * e / subs[a]), (float)-std::sin(two_pi * e / subs[a]));
        if (lens[a] != subs[a])
            for (int e = 0; e < lens[a]; ++e)
                h[offs[a] + subs[a] / 2 + e] = make_float2((float)std::cos(two_pi * e / lens[a]), (float)-std::sin(two_pi * e / lens[a]));
    }
    MI_TRY(tw.alloc(sizeof(float2) * off));
    MI_HIP(hipMemcpyAsync(tw.p, h.data(), sizeof(float2) * off, hipMemcpyHostToDevice, s));
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
    size_t place_min = (size_t)6 << 30;
    if (const char* e = std::getenv("MI_FFT_PLACE_MIN_MB")) place_min = (size_t)std::max(0LL, atoll(e)) << 20;
    if (S.bytes >= place_min && !NoPlacementTrial::active()) MI_TRY(place_by_trial(s, gap));
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
    if (std::getenv("MI_FFT_NO_PRUNE") != nullptr) return;
    const int in_hi = rep[2] ? pw.w[2] : o[2] + n[2];
    dims.z_in_hi = std::min(in_hi, dims.nz);
    dims.z_out_lo = o[2];
    dims.z_out_hi = std::min(o[2] + n[2], dims.nz);
    const int yh = ((o[1] + n[1] + dims.ty - 1) / dims.ty) * dims.ty;  // the x pass reads whole tiles of rows
    dims.y_out_hi = std::min(yh, dims.ny);
}

bool NativeFft::can_fuse() const { return !pw.on || !(pw.rep[0] || pw.rep[1] || pw.rep[2]); }

// P2, P3, P4: S[z][px][py] -> T[z][px][py] (x still transformed), multiplied by the OTF or its conjugate
int NativeFft::middle(hipStream_t s, bool conj_otf) {
    MI_TRY(y_pass(s, false, dims.paired != 0));
    MI_TRY(z_conv(s, conj_otf));
    return y_pass(s, true, dims.paired != 0);
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
