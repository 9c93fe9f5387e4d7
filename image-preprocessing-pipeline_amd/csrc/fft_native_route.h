// Geometry and routes of the hand-written FFT pipeline as pure functions of the grid, the plan's switches and the facts of a call:
// the table of transform lengths, what NativeFft::init computes before its first allocation (plan_geometry) and which kernel family
// a pass launches (x_route, y_route, z_route).  Plain C++17 without HIP types: tests/test_fft_native_route_host.py compiles this
// header with g++ and checks all of it without a device; the launchers (fft_native_x.hip, fft_native_yz.hip) switch on the routes.
#pragma once
#include <algorithm>
#include <cstddef>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_RT_HD __host__ __device__
#else
#define MI_RT_HD
#endif

namespace mi {

struct NativeDims {
    // every axis length is r3 * 2^l2 with r3 in {1, 3, 9}: x (Hx = X/2 complex points), y, z
    int lhx2, r3x;
    int ly2, r3;
    int lz2, r3z;
    int hx, ny, nz;
    int ty, tc, tl;  // rows per x tile, columns per y tile, lines per z tile (A and B tiles each)
    // padded grids: planes z >= z_in_hi of a convolution's input are all zero (never stored, never loaded); of its result only
    // planes [z_out_lo, z_out_hi) and rows < y_out_hi are ever read.  Whole grid when nothing is padded.
    int z_in_hi, z_out_lo, z_out_hi, y_out_hi;
    int dbg;          // timing experiments only: knocks out phases of the z pass (results are then wrong)
    int paired;       // spectra around the z pass in the pair-interleaved layout (k_y_pair, k_z_pair_pipe)
    int zpad;         // paired layout: float4 of padding behind every row (xk, z)
    int xrow;         // x side: complex samples from one row (z, px) to the next (ny + padding)
    int xk0, xkn;     // paired layout: planes xk0 .. xk0 + xkn - 1 of a y / z launch (all of them, or one chunk of the blocked chain)
    int yz0;          // forward y pass: first z plane of the launch (a z chunk of the sharded step; multiple of the planes per work-group)
    // order of the x positions of the spectrum arrays: 0 = position p holds working index p of the x transform; 1 = the low radix-8
    // digit rotated to the top, p = (w & 7) * (hx / 8) + (w >> 3), so that a lane of the fused x pass holds the eight points of a
    // bottom butterfly in the registers of its global access (k_x_fused_pipe; x_rotated() picks the shapes)
    int xrot;
};

// Padded mode: the caller's volume (extents n) sits at offset o inside the transform grid; the x passes apply the boundary
// rule while loading (zero rule: zeros outside the data; replicate rule: clamped samples inside the window [0, w), zeros beyond)
// and crop while storing, so no padded copy of the volume exists.
struct PadWindow {
    int on = 0;
    int n[3] = {0, 0, 0};
    int o[3] = {0, 0, 0};
    int rep[3] = {0, 0, 0};
    int w[3] = {0, 0, 0};
};

// The environment switches of a plan, read once when it is created (read_switches, fft_native.hip): the plan obeys them for its
// whole life, whatever the environment says later.
struct NativeSwitches {
    bool no_pair = false;      // MI_FFT_NO_PAIR: the plain layout around the z pass (A/B measurements)
    bool no_pipe = false;      // MI_FFT_NO_PIPE: no persistent kernels (and so no paired layout)
    bool no_xpipe = false;     // MI_FFT_NO_XPIPE: whole x passes through the unpipelined kernels (every stage in LDS)
    bool no_prune = false;     // MI_FFT_NO_PRUNE: padded grids keep the full passes
    bool complex_otf = false;  // MI_FFT_COMPLEX_OTF: never the real form of the OTF
    bool stored_otf = false;   // MI_FFT_STORED_OTF: the real form stays a stored array, never its rank-4 factors (A/B measurements)
    bool z_general = false;    // MI_FFT_Z_GENERAL: the paired z pass keeps the plane bounds of a pruned grid on a full one (parity test, A/B measurements)
    int x_dyn = -1, z_dyn = -1;  // MI_X_DYN / MI_Z_DYN: tiles of the persistent x / paired z launches from a device counter (1) or at a fixed stride (0); -1 unset
    size_t place_min = (size_t)6 << 30;  // MI_FFT_PLACE_MIN_MB: the smallest arrays (both together) placed by trial
    size_t alt_min = (size_t)8 << 30;    // MI_FFT_PLACE_ALT_MIN_MB: the smallest array that keeps a second buffer for S
    int place_candidates = 6;            // MI_FFT_PLACE_CANDIDATES, 1 .. 8
    bool place_log = false;              // MI_FFT_PLACE_LOG: diagnostics on stderr
    // probe builds only (MI_PROBE_ENV): MI_FFT_ZDBG; MI_FFT_TY / TC / TL (0 unset); MI_FFT_ZPAD / XPAD in float4 per row, MI_X_FREE_CUS
    // (-1 unset); MI_FFT_STGAP in bytes
    int dbg = 0, ty = 0, tc = 0, tl = 0, zpad = -1, xpad = -1, x_free_cus = -1;
    // bytes between the end of S and the start of T in the plan's single allocation: their distance -- which decides how the strided
    // streams of a pass that reads one and writes the other fall onto the HBM channels -- is then the same in every context
    size_t stgap = 4224;
};

// what plan_geometry sizes besides the dims
struct NativeSizes {
    size_t n_cplx;               // complex points of the grid
    size_t n_buf;                // complex entries of each of the two spectrum arrays
    size_t tw_at[3], tw_total;   // twiddle tables per axis in one array: e < sub/2 of the power-of-two sub-transform (sub = 2^l2), then
                                 // the full circle e < n of the radix-3/9 stage when the axis has one
};

// the kernel family of the z pass and its OTF form; real_needs_pipe: the real OTF form exists only in the persistent kernels
enum class ZRoute { conv, conv_pipe, conv_pipe_real, pair_pipe, pair_pipe_real, real_needs_pipe };
// the y passes around it: k_y_pass on the plain layout [px][z][py], k_y_pair on the pair-interleaved one
enum class YRoute { pass, pair };

// One x launch.  forward: P1 of a volume (only `aligned` counts: its 16-byte alignment).  Else P5: fuse_forward (+ P1 of the next
// convolution), whole (no subset of the tiles), aligned (the epilogue operand and the output), ek (ConvEpi: 0 none, 1 ratio,
// 2 update, 3 regularised update), taper_shell (the caller asked for EPI_TAPER_SHELL), has_out (an output volume is stored).
struct XCall {
    bool forward = false, fuse_forward = false, whole = true, aligned = true;
    int ek = 0;
    bool taper_shell = false, has_out = true;
};
// pipe_*: the modes of k_x_fused_pipe; plain_*: k_x_forward, k_x_inverse<plain / fused>; no_subset: a subset of the tiles exists only
// in the fused persistent kernel.  (no_xpipe sends every WHOLE pass through the plain kernels.)
enum class XRoute { pipe_forward, pipe_fused, pipe_inverse, plain_forward, plain_inverse, plain_fused, no_subset };

namespace {

constexpr int kThreadsXZ = 1024;  // strided passes: one ~140-KB work-group of 16 waves per CU
constexpr int kWavesXZ = 4;       // waves per SIMD the register budget is sized for (128 VGPRs)
constexpr int kThreadsY = 512;    // contiguous pass: two work-groups per CU

// rows start on a multiple of 32 slots, so that only the masks decide the banks
MI_RT_HD constexpr int row_pitch(int n) { return (n + 31) & ~31; }
// the x lengths whose spectra take the rotated order (NativeDims::xrot): power-of-two rows whose tile is eight float4 per lane, Hx / 8 apart
MI_RT_HD constexpr bool x_rotated(int lhx2, int r3) { return r3 == 1 && (lhx2 == 10 || lhx2 == 11); }

// ------------------------------------------------------------------------------------------------ super-stage chains
// The log2(N) radix-2 stages of a transform are cut, bottom-up, into super-stages of 3 stages (8 points per lane in
// registers; a remainder of 4 becomes 2 + 2 -- one stage of 16 points for 1024-point transforms --, a remainder of 1 or 2 sits at the top): seg_r(logn, s) is the length of the
// super-stage that starts at stage s.  The same cut serves both directions (forward walks it top-down, inverse bottom-up),
// and all its (S_LO, LR) pairs below stage 5 are among the conflict-free patterns of the swizzle.
MI_RT_HD constexpr int seg_r(int logn, int s, int cut = 0) {
    const int rem = logn - s;
    if (logn == 4) return s == 0 ? 3 : 1;
    // 1024 points as 8 x 8 x 16 -- three LDS round trips instead of the four of 8 x 8 x 4 x 4 (round 4; C3: ratio launch of the x
    // pass 5.07 -> 4.76 ms, the z pass of 1024-point lines 6.15 -> 5.71 ms, the y passes of C2 0.426 -> 0.416 ms).  The sixteen-point
    // butterfly reads its fifteen twiddles where it uses them (butterflies): held together they spilled.
    if (logn == 10 && rem == 4) return 4;
    // cut 1 (the y kernels: 512 threads, 256 registers to spend): 2048 points as 16 x 16 x 8 and 4096 as 16 x 16 x 16 -- three round
    // trips instead of four (round 5; C3: y passes 3.06 / 3.10 -> 2.99 / 2.93 ms).  The x kernels keep 8 x 8 x 8 x 4 for 2048 points:
    // at their 128 registers the sixteen-point butterflies cost more than the round trip (C4-shaped rank: x pass 7.0 / 7.9 ms
    // against 7.7 / 8.6 with 16 x 16 x 8 and 9.5 / 10.6 with 8 x 16 x 16, profiles/r05_fft_cut_2048.txt).
    if (cut == 1 && logn == 11) return s < 8 ? 4 : 3;
    if (cut == 1 && logn == 12) return 4;
    return rem >= 5 ? 3 : rem == 4 ? 2 : rem;  // rem in {1, 2, 3}: all of it
}
// start of the super-stage that ends at stage `top` (exclusive)
MI_RT_HD constexpr int seg_below(int logn, int top, int cut = 0) {
    int s = 0;
    while (s + seg_r(logn, s, cut) < top) s += seg_r(logn, s, cut);
    return s;
}
// LDS twiddle tables: every super-stage with S_LO > 0 owns a packed table of 2^S_LO entries, exp(-2 pi i m / 2^(S_LO+LR))
// (stride-1 look-ups: no bank conflicts, and no vector-memory loads inside the FFT phases -- those would drain the prefetch
// queue, vmcnt being in order); the tables lie one after the other, bottom-up.  tw_off: offset of the table of stage s.
// Powers kept per lane-twiddle index: all R - 1 of them while the table stays small (stage <= 6), else only the first (the
// others are derived by multiplications).
MI_RT_HD constexpr int tw_powers(int s, int r) { return s <= 6 ? (1 << r) - 1 : 1; }
MI_RT_HD constexpr int tw_off(int logn, int s, int cut = 0) {
    int off = 0, t = 0;
    while (t < s) {
        if (t > 0) off += tw_powers(t, seg_r(logn, t, cut)) << t;
        t += seg_r(logn, t, cut);
    }
    return off;
}
MI_RT_HD constexpr int chain_entries(int logn, int cut = 0) { return tw_off(logn, logn, cut); }
// twiddle entries in LDS for an axis of length n = r3 * 2^l2
MI_RT_HD constexpr int axis_tw_entries(int n) {
    int r3 = 1, l2 = 0;
    while (n % 3 == 0) { n /= 3; r3 *= 3; }
    while (n % 5 == 0) { n /= 5; r3 *= 5; }
    while ((1 << l2) < n) ++l2;
    return chain_entries(l2) + (r3 > 1 ? (1 << l2) : 0);
}
#ifndef MI_Y_TILE_CAP
#define MI_Y_TILE_CAP 16
#endif
constexpr int kLdsOneWg = 156 * 1024;  // one work-group per CU (160 KB LDS)
constexpr int kLdsTwoWg = 78 * 1024;   // two work-groups per CU
constexpr int kRowPadBytes = 4224;     // padding behind the rows of the spectrum arrays ...
constexpr size_t kPadRowBytes = 8192;  // ... that are at least this long (plan_geometry)
constexpr int kPairLines = 8;          // lines per block of the pair-interleaved z-side layout (8 A + 8 B lines = 128 bytes)
// rows of an x tile / line pairs of a z tile: 16 (full 128-B lines in the transposed layouts) while tile + tables fit one
// work-group per CU; columns of a y tile: two work-groups per CU
MI_RT_HD constexpr int x_tile_rows(int hx) {
    int rows = 16;
    while (rows > 2 && 8 * (rows * row_pitch(hx) + axis_tw_entries(hx)) > kLdsOneWg) rows >>= 1;
    return rows;
}
MI_RT_HD constexpr int z_tile_lines(int nz) {
    int tl = 16;
    while (tl > 2 && 8 * (2 * tl * row_pitch(nz) + axis_tw_entries(nz)) > kLdsOneWg) tl >>= 1;
    return tl;
}
MI_RT_HD constexpr int y_tile_cols(int ny) {
    int tc = MI_Y_TILE_CAP;
    while (tc > 1 && 8 * (tc * row_pitch(ny) + axis_tw_entries(ny)) > kLdsTwoWg) tc >>= 1;
    return tc;
}
// the real form of the OTF in k_z_conv_pipe needs line-uniform phases per item: either the lines divide the work-group evenly, or
// every wave owns one pair of lines (the WP layout of k_z_conv_pipe)
constexpr bool z_pipe_even(int L) {
    return (L % 64 == 0) && ((z_tile_lines(L) * L) % kThreadsXZ == 0) && ((kThreadsXZ % L == 0) || z_tile_lines(L) == kThreadsXZ / 64);
}

constexpr bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
constexpr int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
// LDS of an axis kernel: the tile, then the twiddle tables (both chains and the radix-3/9 table: what the fused kernels of
// the axis use, an upper bound for the others; see TwLds) -- 8 bytes per complex entry
constexpr size_t lds_bytes(int rows, int n) { return 8 * ((size_t)rows * row_pitch(n) + axis_tw_entries(n)); }

// ------------------------------------------------------------------------------------------------ the length table
// An axis length n = r3 * 2^l2, one M(l2, r3) per length the kernels are built for: powers of two from 8 to 4096, or 3 * / 9 * (32 ..
// 512).  (A radix-3/9 factor matters most on y, the axis the slab driver shards, where slab + halos is rarely a power of two; on x
// and z it keeps zero-padded deconFFT shapes close to the 7-smooth ones.)  The launch dispatch (x_case, y_case, z_case, z_pair_case)
// and every predicate below expand these lists, so a length is stated here and nowhere else.
#define MI_AXIS_CASES(M) M(3, 1) M(4, 1) M(5, 1) M(6, 1) M(7, 1) M(8, 1) M(9, 1) M(10, 1) M(11, 1) M(12, 1) \
    M(5, 3) M(6, 3) M(7, 3) M(8, 3) M(9, 3) M(5, 9) M(6, 9) M(7, 9) M(8, 9) M(9, 9)
// y: also 5 * 2^a (320 rows of a slab rank instead of 384; only the y kernels are built for it)
#define MI_Y_ONLY_CASES(M) M(5, 5) M(6, 5) M(7, 5) M(8, 5)
#define MI_Y_CASES(M) MI_AXIS_CASES(M) MI_Y_ONLY_CASES(M)
// z: the lengths of MI_AXIS_CASES up to kMaxZ -- 2 * TL >= 4 rows of the z pass must fit the LDS tile
constexpr int kMaxZ = 2304;
// The paired z pass: its lengths, each with the threads per work-group and whether the z ramp has its LDS table (PHL).
// Lines of up to 576 points: 8 waves on a 64-KB tile, two work-groups per CU (576 points: the LDS phase table would cost the
// second work-group); 768 and 1152 points: 16 waves, one line per wave; 1024 points: 8 waves again, a line pair per wave -- with
// the 16-point top stage a lane's 16 float4 are exactly that stage's points of two lines, so it runs on the registers of the
// global access like the 512-point pass (246 registers, one work-group per CU): 5.60 -> 5.11 ms on 1024 x 576 x 4096 against the
// 16-wave form, A / B in one process.
#define MI_ZQ_CASES(M) M(6, 1, 512, true) M(7, 1, 512, true) M(8, 1, 512, true) M(9, 1, 512, true) M(10, 1, 512, true) \
    M(6, 3, 512, true) M(7, 3, 512, true) M(8, 3, 1024, true) M(6, 9, 512, false) M(7, 9, 1024, true)

// axis 0 (x, on its Hx complex points), 1 (y) or 2 (z) takes the length r3 * 2^l2
constexpr bool axis_takes(int axis, int l2, int r3) {
#define MI_TAKES(LG, R) if (l2 == LG && r3 == R) return axis != 2 || (R << LG) <= kMaxZ;
    MI_AXIS_CASES(MI_TAKES)
#undef MI_TAKES
#define MI_TAKES(LG, R) if (l2 == LG && r3 == R) return axis == 1;
    MI_Y_ONLY_CASES(MI_TAKES)
#undef MI_TAKES
    return false;
}
// the paired z pass takes it (nth, ph: its threads per work-group and whether it keeps the LDS phase table)
constexpr bool z_pair_takes(int l2, int r3, int* nth = nullptr, bool* ph = nullptr) {
#define MI_TAKES(LG, R, NTH, PH) if (l2 == LG && r3 == R) { if (nth) *nth = NTH; if (ph) *ph = PH; return true; }
    MI_ZQ_CASES(MI_TAKES)
#undef MI_TAKES
    return false;
}
// LDS of a work-group of the paired z pass, without its 4-byte tile counter: the tile of 2 * kPairLines rows and the twiddle tables, then
// the table of the OTF form -- the four A_r (16 B per z position) of the factored form, or the z ramp (8 B) of the stored real form where
// the length keeps one (PHL).  The kernel declares exactly this as a static array; the launch derives the work-groups per CU from it.
constexpr size_t z_pair_lds(int l2, int r3, bool real_otf, bool factored) {
    bool ph = false;
    z_pair_takes(l2, r3, nullptr, &ph);
    const int L = r3 << l2;
    return lds_bytes(2 * kPairLines, L) + (factored ? 16 * (size_t)L : real_otf && ph ? 8 * (size_t)L : 0);
}
// The paired z pass of this length can rebuild the real OTF from its rank-4 factors (k_z_pair_pipe<.., FACT>): the table of the four
// A_r, 16 bytes per z position, must fit LDS where the z ramp's 8-byte table lay without costing a work-group per CU.  576-point
// lines have no room for either table beside their 72-KB tile (two work-groups per CU), and the 16 rows of 1152 points leave 10 KB
// of the 156: both lengths keep the stored real form.
constexpr bool z_pair_factored(int l2, int r3) {
    bool ph = false;
    if (!z_pair_takes(l2, r3, nullptr, &ph) || !ph) return false;
    const int L = r3 << l2;
    const size_t stored = lds_bytes(2 * kPairLines, L) + 8 * (size_t)L, fact = lds_bytes(2 * kPairLines, L) + 16 * (size_t)L;
    return fact <= (size_t)kLdsOneWg && std::min<size_t>(2, kLdsOneWg / fact) == std::min<size_t>(2, kLdsOneWg / stored);  // (the launch's per_cu)
}
// n = r3 * 2^l2 as the axis takes it
constexpr bool split_axis(int n, int axis, int* r3, int* l2) {
    for (int r = 1; r <= 9; r += 2)
        if (n % r == 0 && is_pow2(n / r) && axis_takes(axis, ilog2(n / r), r)) { *r3 = r; *l2 = ilog2(n / r); return true; }
    return false;
}
constexpr int axis_longest(int axis) {
    int m = 0;
#define MI_TAKES(LG, R) if (axis_takes(axis, LG, R)) m = std::max(m, R << LG);
    MI_Y_CASES(MI_TAKES)
#undef MI_TAKES
    return m;
}
// F = (x, y, z); x: real length 2 * Hx, the transform runs on Hx complex points
constexpr bool native_supported(const int F[3]) {
    int r3 = 0, l2 = 0;
    return F[0] % 2 == 0 && split_axis(F[0] / 2, 0, &r3, &l2) && split_axis(F[1], 1, &r3, &l2) && split_axis(F[2], 2, &r3, &l2);
}
// smallest supported extent >= n of an axis; 0 when there is none (beyond the longest length of the table)
constexpr int native_good_size(int n, int axis) {
    int r3 = 0, l2 = 0;
    for (int m = axis == 0 ? (n + 1) / 2 : n; m <= axis_longest(axis); ++m)
        if (split_axis(m, axis, &r3, &l2)) return axis == 0 ? 2 * m : m;
    return 0;
}

// ------------------------------------------------------------------------------------------------ the plan's geometry
// Everything NativeFft::init decides before its first allocation.  0, or the requirement the tiles miss: 1 the x tile does not
// divide y, 2 the z tile does not fit y, 3 a transform is too long for LDS; -1 for a shape outside the length table.
inline int plan_geometry(const int F[3], const NativeSwitches& sw, NativeDims* dims, NativeSizes* sz) {
    if (!native_supported(F)) return -1;
    NativeDims& d = *dims;
    const int Hx = F[0] / 2;
    split_axis(Hx, 0, &d.r3x, &d.lhx2);
    split_axis(F[1], 1, &d.r3, &d.ly2);
    split_axis(F[2], 2, &d.r3z, &d.lz2);
    d.hx = Hx;
    d.xrot = x_rotated(d.lhx2, d.r3x) ? 1 : 0;
    d.ny = F[1];
    d.nz = F[2];
    d.ty = std::min(sw.ty ? sw.ty : x_tile_rows(Hx), F[1]);
    d.tc = sw.tc ? sw.tc : y_tile_cols(F[1]);
    d.tl = std::min(sw.tl ? sw.tl : z_tile_lines(F[2]), F[1]);
    d.z_in_hi = F[2];
    d.z_out_lo = 0;
    d.z_out_hi = F[2];
    d.y_out_hi = F[1];
    d.xk0 = 0;
    d.xkn = Hx / 2 + 1;
    d.yz0 = 0;
    d.dbg = sw.dbg;
    while ((size_t)F[2] * Hx % d.tc) d.tc >>= 1;
    // tiles are whole float4 groups of rows / lines and must divide y; z tiles of TL positions must map onto aligned
    // mirror blocks, which holds for TL <= 2^ly2 (positions inside one power-of-two sub-block mirror inside one)
    if (!(d.ty >= 2 && d.ty % 2 == 0 && F[1] % d.ty == 0)) return 1;
    if (!(d.tl >= 2 && is_pow2(d.tl) && d.tl <= (1 << d.ly2))) return 2;
    if (lds_bytes(d.ty, Hx) > 160 * 1024 || lds_bytes(d.tc, F[1]) > 160 * 1024 || lds_bytes(2 * d.tl, F[2]) > 160 * 1024) return 3;
    // pair-interleaved z-side layout (k_y_pair / k_z_pair_pipe): a z length the paired z pass takes, whole blocks of kPairLines
    // lines, an even number of columns per y tile
    d.paired = z_pair_takes(d.lz2, d.r3z) && F[1] % (2 * kPairLines) == 0 && d.tc >= 2 && d.tc % 2 == 0 && F[2] % (d.tc / 2) == 0 &&
               d.dbg == 0 && !sw.no_pair && !sw.no_pipe && sw.tl == 0;
    sz->n_cplx = (size_t)Hx * F[1] * F[2];
    // (the two planes that are their own mirror partners are stored twice in the paired layout)
    // Rows an exact power of two apart camp on few HBM channels: behind every row of the x side ([z][px][.]) and of the paired z
    // side ([xk][z][.]) that is at least 8 KB long lie 4 KB + 128 B of padding.  C3 (profiles/zpad_probe.py): z pass 4.75 -> 4.2 ms
    // with any odd multiple of 128 B behind the z rows (64-byte offsets break the 128-byte lines: 6.2 ms); with 4 KB + 128 B
    // on both sides the y passes drop from 3.2-3.35 to 2.85-3.35 ms and the x pass from 5.1 / 6.0-7.2 to 4.75 / 5.7-6.8 ms.
    const int pad_x = (size_t)F[1] * 8 >= kPadRowBytes ? kRowPadBytes : 0;
    const int pad_z = (size_t)F[1] * 16 >= kPadRowBytes ? kRowPadBytes : 0;
    d.zpad = d.paired ? (sw.zpad >= 0 ? sw.zpad : pad_z / 16) : 0;
    d.xrow = F[1] + (sw.xpad >= 0 ? 2 * sw.xpad : pad_x / 8);
    const size_t n_x = (size_t)Hx * F[2] * d.xrow;
    sz->n_buf = std::max(n_x, d.paired ? (size_t)(Hx / 2 + 1) * F[2] * 2 * (size_t)(F[1] + d.zpad) : sz->n_cplx);
    const int lens[3] = {Hx, F[1], F[2]}, subs[3] = {1 << d.lhx2, 1 << d.ly2, 1 << d.lz2};
    sz->tw_total = 0;
    for (int a = 0; a < 3; ++a) {
        sz->tw_at[a] = sz->tw_total;
        sz->tw_total += (size_t)std::max(1, subs[a] / 2) + (lens[a] != subs[a] ? (size_t)lens[a] : 0);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ routes
// the x pass can run as the persistent pipelined kernel / the z pass as one of the persistent kernels
inline bool x_pipe_ok(const NativeDims& d, const NativeSwitches& sw) { return d.dbg == 0 && !sw.no_pipe && d.ty == x_tile_rows(d.hx); }
inline bool z_pipe_ok(const NativeDims& d, const NativeSwitches& sw) {
    return d.paired || (d.dbg == 0 && !sw.no_pipe && d.tl == z_tile_lines(d.nz));
}
// the z pass of this plan can take the real form of the OTF (NativeFft::try_real_otf then looks at the PSF)
inline bool real_otf_possible(const NativeDims& d, const NativeSwitches& sw) {
    return !sw.complex_otf && z_pipe_ok(d, sw) && (d.paired || z_pipe_even(d.nz));
}
// tiles of the persistent x launches (`overlapped`: beside a halo exchange, which follows mi_rl_set_overlap) and of the paired z pass
// come from a device counter
inline bool x_tiles_dynamic(const NativeSwitches& sw, bool by_default = true) { return sw.x_dyn >= 0 ? sw.x_dyn != 0 : by_default; }
inline bool z_tiles_dynamic(const NativeSwitches& sw) { return sw.z_dyn != 0; }

inline ZRoute z_route(const NativeDims& d, const NativeSwitches& sw, bool real_otf) {
    if (d.paired) return real_otf ? ZRoute::pair_pipe_real : ZRoute::pair_pipe;
    if (z_pipe_ok(d, sw)) return real_otf && z_pipe_even(d.nz) ? ZRoute::conv_pipe_real : ZRoute::conv_pipe;
    return real_otf ? ZRoute::real_needs_pipe : ZRoute::conv;
}
inline YRoute y_route(const NativeDims& d) { return d.paired ? YRoute::pair : YRoute::pass; }
// The paired z pass runs in its full-grid form, without plane bounds on its loads and stores: every z plane is read and written (a
// circular grid, or a padded one whose window prunes nothing along z).  Any bound short of the grid, or MI_FFT_Z_GENERAL, keeps the
// predicated form.
inline bool z_full_grid(const NativeDims& d, const NativeSwitches& sw) {
    return d.paired && !sw.z_general && d.z_in_hi == d.nz && d.z_out_lo == 0 && d.z_out_hi == d.nz;
}

inline bool pad_can_fuse(const PadWindow& pw) { return !pw.on || !(pw.rep[0] || pw.rep[1] || pw.rep[2]); }
// padded grids take the persistent x kernels too: zero rule, data at the origin, whole float4 rows and what the call site asks
// of its pointers (`aligned`)
inline bool x_pad_pipe(const NativeDims& d, const NativeSwitches& sw, const PadWindow& pw, bool aligned) {
    return pw.on && pad_can_fuse(pw) && x_pipe_ok(d, sw) && pw.o[0] == 0 && pw.o[1] == 0 && pw.o[2] == 0 && pw.n[0] % 4 == 0 && aligned;
}
inline XRoute x_route(const NativeDims& d, const NativeSwitches& sw, const PadWindow& pw, const XCall& c) {
    const bool pipe = pw.on ? x_pad_pipe(d, sw, pw, c.forward || (c.aligned && c.whole)) : x_pipe_ok(d, sw);
    if (c.forward) return pipe && c.aligned && !sw.no_xpipe ? XRoute::pipe_forward : XRoute::plain_forward;
    if (c.fuse_forward && pipe && !(c.whole && sw.no_xpipe)) return XRoute::pipe_fused;
    if (!c.whole) return XRoute::no_subset;
    if (!c.fuse_forward && pipe && c.ek <= 2 && !c.taper_shell && c.has_out && c.aligned && !sw.no_xpipe) return XRoute::pipe_inverse;
    return c.fuse_forward ? XRoute::plain_fused : XRoute::plain_inverse;
}

}  // namespace
}  // namespace mi
