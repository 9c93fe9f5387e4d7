// The middle passes of the native FFT pipeline and their launchers: the y passes (P2 / P4) in the plain and the pair-interleaved
// layout, the z pass (P3: z transforms around the OTF product), the OTF itself and its real form.
// One unit for both axes, y first: the y kernels and the paired z kernels share their 512-thread super-stages, and the compiler
// inlines the always-inline building blocks in the order the unit first emits them, so what it makes of a z kernel depends on the
// y kernels named before it (profiles/NOTES.md, "FFT source split").
#include "fft_native_dev.h"
#include "otf_factor.h"

namespace mi {
namespace {

// ---------------------------------------------------------------------------------------------- P2 / P4: y passes
// whole contiguous columns.  Forward: column (z, px) of src[z][px][.] -> dst[px][z][.]; inverse: the way back.
template <int LY2, int R3, bool INVERSE>
__global__ __launch_bounds__(kThreadsY, 4) void k_y_pass(const float2* __restrict__ src, float2* __restrict__ dst, NativeDims d,
                                                      const float2* __restrict__ tw) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];
    constexpr int M = R3 << LY2, NW = kThreadsY / 64;
    constexpr int pitch = row_pitch(M), quads = M / 2;
    constexpr int TCC = y_tile_cols(M);  // the tile height the host normally picks: compile-time item decomposition
    const int TC = d.tc, Hx = d.hx, L = d.nz;
    const size_t c0 = (size_t)blockIdx.x * TC + (INVERSE ? (size_t)0 : (size_t)d.yz0 * Hx);  // (forward: columns (z, px), z slowest)
    // padded grids: forward, the columns of all-zero input planes are neither read nor produced (the z pass knows they are
    // zero); inverse, only the planes that survive the crop are transformed
    if (!INVERSE) {
        if ((int)(c0 / Hx) >= d.z_in_hi) return;
    } else if (L % TC == 0) {
        const int z_first = (int)(c0 % L);
        if (z_first >= d.z_out_hi || z_first + TC <= d.z_out_lo) return;
    }
    // row pitches: the x side ([z][px][py]) may carry padding behind every row (NativeDims::xrow)
    const size_t src_pitch = INVERSE ? (size_t)M : (size_t)d.xrow, dst_pitch = INVERSE ? (size_t)d.xrow : (size_t)M;
    const float4* base = reinterpret_cast<const float4*>(src + c0 * src_pitch);
    // columns dealt to the waves when there are enough of them: then the fill, the transform and the drain of a column all
    // belong to one wave and the kernel has no work-group barrier besides the one behind the table fill
    const bool priv = (TC % NW) == 0;
    using TW = TwLds<LY2, R3, kYCut>;
    float2* twl = tile + TC * pitch;
    TW::template fill<kThreadsY>(twl, tw);
    // destination of source column sc: forward [z][px] -> [px][z], inverse [px][z] -> [z][px]
    auto dest_col = [&](size_t sc) {
        if (INVERSE) { const size_t px = sc / L, z = sc - px * L; return z * Hx + px; }
        const size_t z = sc / Hx, px = sc - z * Hx;
        return px * L + z;
    };
    // fast path: float4 item k of a lane is quad tid + (k NT mod quads) of column (k NT) / quads -- the column is a
    // compile-time number (its addresses are scalar), the slot is the lane's constant XOR a compile-time constant
    constexpr bool FAST_OK = (quads % kThreadsY == 0) && ((TCC * quads) % kThreadsY == 0);
    constexpr int NIT = FAST_OK ? TCC * quads / kThreadsY : 1;
    const bool fast = FAST_OK && TC == TCC && !priv;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_items = priv ? (TC / NW) * quads : TC * quads, first = priv ? lane : threadIdx.x, step = priv ? 64 : kThreadsY;
    if (fast) {
        const int s_lane = phys(2 * (int)threadIdx.x);
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int c = (k * kThreadsY) / quads, qk = (k * kThreadsY) % quads;
            const float4 v = base[(size_t)c * (src_pitch / 2) + qk + threadIdx.x];
            const int s0 = c * pitch + (s_lane ^ swz_c(2 * qk));
            tile[s0] = make_float2(v.x, v.y);
            tile[s0 ^ 1] = make_float2(v.z, v.w);
        }
    } else {
#pragma unroll MI_FFT_UNROLL
        for (int i = first; i < n_items; i += step) {
            const int cl = i / quads, q = i - cl * quads;
            const int c = priv ? cl * NW + wave : cl;
            const float4 v = base[(size_t)c * (src_pitch / 2) + q];
            const int s0 = c * pitch + phys(2 * q);
            tile[s0] = make_float2(v.x, v.y);
            tile[s0 ^ 1] = make_float2(v.z, v.w);
        }
    }
    lds_barrier();
    if constexpr (!INVERSE && R3 > 1) {
        radix3_stage<R3, false, kThreadsY>(tile, TC, pitch, 1, priv, 1 << LY2, twl + TW::r3);
        stage_sync(priv);
    }
    lds_fft<LY2, INVERSE, kThreadsY, R3, 0, LY2, kYCut>(tile, TC * R3, pitch, 1, priv, twl);
    if constexpr (INVERSE && R3 > 1) {
        radix3_stage<R3, true, kThreadsY>(tile, TC, pitch, 1, priv, 1 << LY2, twl + TW::r3);
        stage_sync(priv);
    }
    if (fast) {
        const int s_lane = phys(2 * (int)threadIdx.x);
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int c = (k * kThreadsY) / quads, qk = (k * kThreadsY) % quads;
            const int s0 = c * pitch + (s_lane ^ swz_c(2 * qk));
            const float2 a = tile[s0], b = tile[s0 ^ 1];
            float4* dcol = reinterpret_cast<float4*>(dst + dest_col(c0 + c) * dst_pitch);  // scalar
            if (!INVERSE || 2 * (qk + (int)threadIdx.x) < d.y_out_hi) dcol[qk + threadIdx.x] = make_float4(a.x, a.y, b.x, b.y);
        }
    } else {
#pragma unroll MI_FFT_UNROLL
        for (int i = first; i < n_items; i += step) {
            const int cl = i / quads, q = i - cl * quads;
            const int c = priv ? cl * NW + wave : cl;
            const int s0 = c * pitch + phys(2 * q);
            const float2 a = tile[s0], b = tile[s0 ^ 1];
            if (!INVERSE || 2 * q < d.y_out_hi) reinterpret_cast<float4*>(dst + dest_col(c0 + c) * dst_pitch)[q] = make_float4(a.x, a.y, b.x, b.y);
        }
    }
}

// ---------------------------------------------------------------------------------------------- P2 / P4, pair-interleaved
// The y passes on the pair-interleaved layout of the z side (NativeDims::paired): row (xk, z), xk <= Hx/2, holds 2 M samples,
// for every block of 8 y positions the 8 lines of plane xk ("A") followed by their 8 mirror partners from plane Hx - xk ("B", in
// partner order: B slot j is the line the z pass pairs with A slot j).  A work-group takes TC/2 z planes x {A, B} of one xk, so
// that it reads and writes whole rows although each plane only owns every other 64 bytes.  Planes 0 and Hx/2 are their own
// partners: their lines are stored twice (as A of their block and as B of the mirror block).
template <int LY2, int R3, bool INVERSE>
__global__ __launch_bounds__(kThreadsY, 4) void k_y_pair(const float2* __restrict__ src, float2* __restrict__ dst, NativeDims d,
                                                      const float2* __restrict__ tw) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];
    constexpr int M = R3 << LY2, NW = kThreadsY / 64;
    constexpr int pitch = row_pitch(M), quads = M / 2;
    const int TC = d.tc, Hx = d.hx, L = d.nz;
    const int zper = TC / 2, zblocks = L / zper, nxk = d.xkn;  // (a launch covers the planes xk0 .. xk0 + xkn - 1: all, or a chunk)
    // work-groups in flight read neighbouring memory (reads wait, writes do not): forward, the planes of one z pair on the x
    // side; inverse, consecutive rows of one xk on the z side
    const int xkl = INVERSE ? blockIdx.x / zblocks : blockIdx.x % nxk;
    const int xk = d.xk0 + xkl;
    const int z0 = (INVERSE ? blockIdx.x - xkl * zblocks : blockIdx.x / nxk) * zper + (INVERSE ? 0 : d.yz0);
    if (!INVERSE) {
        if (z0 >= d.z_in_hi) return;  // all-zero input planes of a padded grid: neither read nor produced
    } else if (z0 >= d.z_out_hi || z0 + zper <= d.z_out_lo) {
        return;                       // planes the crop drops
    }
    const int pxA = x_freq2pos(xk, d), pxB = x_freq2pos(xk == 0 ? 0 : Hx - xk, d);
    const bool self = pxA == pxB;
    // LDS row c of the tile: side c & 1, plane z0 + (c >> 1)
    // x side ([z][px][py], whole columns): float4 q of column c = positions 2 q, 2 q + 1
    auto x_item = [&](int i, int& c, int& q, size_t& g) {
        c = i / quads;
        q = i - c * quads;
        g = (((size_t)(z0 + (c >> 1)) * Hx + ((c & 1) ? pxB : pxA)) * d.xrow) / 2 + q;
    };
    // z side, by float4 f of row (xk, z0 + zi): block f >> 3; f & 7 < 4: lines 2 (f & 3), + 1 of the block from the A column,
    // else the partners of those two lines from the B column -- the mirrors of neighbouring positions are neighbours (they
    // differ by M/2 in frequency), so both sides read or write one LDS slot pair
    auto z_item = [&](int i, int& c, int& s0, size_t& g) {
        const int zi = i / M, f = i - zi * M;
        const int py = ((f >> 3) << 3) + 2 * (f & 3), side = (f >> 2) & 1;
        c = 2 * zi + side;
        // (inverse: B columns are transformed as they lie and leave row-reversed, see x_slots; forward: the mirror map)
        s0 = c * pitch + phys(!INVERSE && side ? mirror_pos(py, M, LY2, R3) : py);
        g = ((size_t)xk * L + z0 + zi) * (size_t)(M + d.zpad) + f;
    };
    // General path, B columns.  Forward: the transform of the column is stored through the mirror map of the frequency positions
    // (B slot of position p <- position mirror(p)).  Inverse: the B slots are loaded in position order -- the array at position
    // p is X_B[-k(p)], whose inverse transform is the column ROW-REVERSED -- and row n is stored from LDS position -n mod M:
    // no mirror arithmetic and, for every radix, contiguous LDS traffic where the mirror map scatters (y = 9 * 64: inverse
    // pass 1.16 -> 0.97 ms; the forward pass is faster with the mirror map, 0.97 against 1.14 ms).  (The fast path below uses
    // the mirror map in both directions: for power-of-two columns it is XOR-linear.)
    auto x_slots = [&](int c, int q, int& s_lo, int& s_hi) {  // LDS slots of rows 2 q and 2 q + 1 of column c
        if (INVERSE && (c & 1)) {
            s_lo = c * pitch + phys(q == 0 ? 0 : M - 2 * q);
            s_hi = c * pitch + phys(M - 2 * q - 1);
        } else {
            s_lo = c * pitch + phys(2 * q);
            s_hi = s_lo ^ 1;
        }
    };
    const bool priv = (TC % NW) == 0;  // (the transform only: fill and drain cross the columns)
    using TW = TwLds<LY2, R3, kYCut>;
    float2* twl = tile + TC * pitch;
    TW::template fill<kThreadsY>(twl, tw);
    const int n_items = TC * quads;
    // fast path (power-of-two columns of at least 2 NT samples): item k of a lane is float4 tid + k NT of the tile on either
    // side, so columns, rows and the high position bits are compile-time numbers and -- the swizzle being XOR-linear -- a slot
    // is a lane constant XOR a compile-time constant.  x side: position 2 tid + (2 k NT mod M).  z side: the lane's block
    // position py_l = 8 (tid >> 3) + 2 (tid & 3) plus f0 = k NT mod M; the mirror of f0 + py_l is (py_l ^ (NT - 1)) + [mirror
    // of the high bits] unless f0 = 0, when it is the mirror of py_l inside the first NT positions.
    constexpr int TCC = y_tile_cols(M);
    constexpr bool FAST_OK = R3 == 1 && quads % kThreadsY == 0;
    constexpr int NIT = FAST_OK ? TCC * quads / kThreadsY : 1;
    const bool fast = FAST_OK && TC == TCC;
    constexpr int WHI = FAST_OK ? LY2 - 9 : 0;  // position bits above the lane's 9 (kThreadsY = 512)
    static_assert(kThreadsY == 512, "the fast path of k_y_pair counts on 512 lanes");
    struct ZLane { int a, b0, b1, side; };
    auto z_lane = [&]() {
        const int tid = launder(threadIdx.x);
        const int py_l = ((tid >> 3) << 3) + 2 * (tid & 3), side = (tid >> 2) & 1;
        return ZLane{phys(py_l), phys(mirror_pos(py_l, M, LY2, R3)), phys(py_l ^ 511), side};
    };
    auto z_slot_fast = [&](const ZLane& zl, int k) {  // k: compile-time after unrolling
        const int zi = (k * kThreadsY) / M, f0 = (k * kThreadsY) % M;
        const int flo = (int)brev_n((unsigned)f0, LY2);                          // the low WHI frequency bits
        const int mhi = flo ? (int)brev_n((unsigned)((1 << WHI) - flo), LY2) : 0;  // position bits of their negative
        const int sa = zl.a ^ swz_c(f0), sb = flo ? (zl.b1 ^ swz_c(mhi)) : zl.b0;
        return (2 * zi) * pitch + (zl.side ? pitch + sb : sa);
    };
    if (fast) {
        if (INVERSE) {
            const ZLane zl = z_lane();
            const float4* rowp = reinterpret_cast<const float4*>(src) + ((size_t)xk * L + z0) * (size_t)(M + d.zpad) + threadIdx.x;
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                const float4 v = rowp[(size_t)((k * kThreadsY) / M) * (M + d.zpad) + (k * kThreadsY) % M];
                const int s0 = z_slot_fast(zl, k);
                tile[s0] = make_float2(v.x, v.y);
                tile[s0 ^ 1] = make_float2(v.z, v.w);
            }
        } else {
            const int s_lane = phys(2 * (int)threadIdx.x);
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                const int c = (k * kThreadsY) / quads, qk = (k * kThreadsY) % quads;
                const size_t col = (((size_t)(z0 + (c >> 1)) * Hx + ((c & 1) ? pxB : pxA)) * d.xrow) / 2;  // scalar
                const float4 v = reinterpret_cast<const float4*>(src)[col + qk + threadIdx.x];
                const int s0 = c * pitch + (s_lane ^ swz_c(2 * qk));
                tile[s0] = make_float2(v.x, v.y);
                tile[s0 ^ 1] = make_float2(v.z, v.w);
            }
        }
    } else {
#pragma unroll MI_FFT_UNROLL
    for (int i = threadIdx.x; i < n_items; i += kThreadsY) {
        int c, s0, s1;
        size_t g;
        if (INVERSE) {
            z_item(i, c, s0, g);
            s1 = s0 ^ 1;
        } else {
            int q;
            x_item(i, c, q, g);
            x_slots(c, q, s0, s1);
        }
        const float4 v = reinterpret_cast<const float4*>(src)[g];
        tile[s0] = make_float2(v.x, v.y);
        tile[s1] = make_float2(v.z, v.w);
    }
    }
    lds_barrier();
    if constexpr (!INVERSE && R3 > 1) {
        radix3_stage<R3, false, kThreadsY>(tile, TC, pitch, 1, priv, 1 << LY2, twl + TW::r3);
        stage_sync(priv);
    }
    lds_fft<LY2, INVERSE, kThreadsY, R3, 0, LY2, kYCut>(tile, TC * R3, pitch, 1, priv, twl);
    if constexpr (INVERSE && R3 > 1) {
        radix3_stage<R3, true, kThreadsY>(tile, TC, pitch, 1, priv, 1 << LY2, twl + TW::r3);
        stage_sync(priv);
    }
    if (priv) lds_barrier();
    if (fast) {
        if (INVERSE) {
            const int s_lane = phys(2 * (int)threadIdx.x);
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                const int c = (k * kThreadsY) / quads, qk = (k * kThreadsY) % quads;
                const int z = z0 + (c >> 1);
                // (a plane that is its own partner is written once, from its A copy)
                if ((self && (c & 1)) || 2 * (qk + (int)threadIdx.x) >= d.y_out_hi || z < d.z_out_lo || z >= d.z_out_hi) continue;
                const size_t col = (((size_t)z * Hx + ((c & 1) ? pxB : pxA)) * d.xrow) / 2;  // scalar
                const int s0 = c * pitch + (s_lane ^ swz_c(2 * qk));
                const float2 a = tile[s0], b = tile[s0 ^ 1];
                reinterpret_cast<float4*>(dst)[col + qk + threadIdx.x] = make_float4(a.x, a.y, b.x, b.y);
            }
        } else {
            const ZLane zl = z_lane();
            float4* rowp = reinterpret_cast<float4*>(dst) + ((size_t)xk * L + z0) * (size_t)(M + d.zpad) + threadIdx.x;
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                const int s0 = z_slot_fast(zl, k);
                const float2 a = tile[s0], b = tile[s0 ^ 1];
                rowp[(size_t)((k * kThreadsY) / M) * (M + d.zpad) + (k * kThreadsY) % M] = make_float4(a.x, a.y, b.x, b.y);
            }
        }
        return;
    }
#pragma unroll MI_FFT_UNROLL
    for (int i = threadIdx.x; i < n_items; i += kThreadsY) {
        int c, s0, s1;
        size_t g;
        if (INVERSE) {
            int q;
            x_item(i, c, q, g);
            const int z = z0 + (c >> 1);
            // (a plane that is its own partner is written once, from its A copy)
            if ((self && (c & 1)) || 2 * q >= d.y_out_hi || z < d.z_out_lo || z >= d.z_out_hi) continue;
            x_slots(c, q, s0, s1);
        } else {
            z_item(i, c, s0, g);
            s1 = s0 ^ 1;
        }
        const float2 a = tile[s0], b = tile[s1];
        reinterpret_cast<float4*>(dst)[g] = make_float4(a.x, a.y, b.x, b.y);
    }
}

// one launch of the y kernel of the layout and direction: `ycols` work-groups on the planes and columns that `d` names
int y_launch(const NativeFft& f, hipStream_t s, bool inverse, YRoute route, unsigned ycols, const NativeDims& d, const float2* src, float2* dst) {
    const size_t yl = lds_bytes(d.tc, d.ny);
    return y_case(d, [&](auto lg, auto r) {
        constexpr int LG = lg(), R = r();
        if (route == YRoute::pair)
            return inverse ? launch_lds(k_y_pair<LG, R, true>, ycols, kThreadsY, yl, s, "k_y_pair<inv>", src, dst, d, f.tw_y)
                           : launch_lds(k_y_pair<LG, R, false>, ycols, kThreadsY, yl, s, "k_y_pair<fwd>", src, dst, d, f.tw_y);
        return inverse ? launch_lds(k_y_pass<LG, R, true>, ycols, kThreadsY, yl, s, "k_y_pass<inv>", src, dst, d, f.tw_y)
                       : launch_lds(k_y_pass<LG, R, false>, ycols, kThreadsY, yl, s, "k_y_pass<fwd>", src, dst, d, f.tw_y);
    });
}


// ---------------------------------------------------------------------------------------------- P3: z pass + OTF
// One tile = the TL lines (py0 .. py0 + TL) of plane xk ("A", rows 0 .. TL-1 of the LDS tile) and their mirror lines in plane
// Hx - xk ("B", rows TL .. 2 TL - 1): xk runs over 0 .. Hx/2, one representative of every mirror pair of planes.  For
// xk in {0, Hx/2} the mirror line lies in the same plane: every tile is processed in the A role (its mirror tile is only read)
// and only A is written, so each line is still written exactly once; otherwise both lines of a pair are written by the one
// tile that owns the pair.  grid: (Hx/2 + 1) * (Y / TL) tiles.
// OTF layout: G[xk][py][pz] as float4 {Ga.re, Ga.im, Gb.re, Gb.im}, already scaled by 2/(X*Y*Z).
// BUILD: instead of multiplying, the untangled spectrum of the (real) input -- a placed PSF -- is stored as the OTF in that
// same layout, scaled: the pipeline builds its own OTF with the transform it will later apply.
template <int LZ2, int R3, bool BUILD>
__global__ __launch_bounds__(kThreadsXZ, kWavesXZ) void k_z_conv(const float2* __restrict__ S, float2* __restrict__ T, const float4* __restrict__ G,
                                                      NativeDims d, const float2* __restrict__ tw, int conj_otf, float4* __restrict__ Gout,
                                                      float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];
    constexpr int L = R3 << LZ2, NW = kThreadsXZ / 64;
    const int Hx = d.hx, M = d.ny, TL = d.tl, hp = TL / 2, pitch = row_pitch(L);
    const int ytiles = M / TL;
    const int plane = blockIdx.x / ytiles;
    const int py0 = (blockIdx.x % ytiles) * TL;
    const int xk = plane;
    const int px = x_freq2pos(xk, d);
    const int pxB = x_freq2pos(xk == 0 ? 0 : Hx - xk, d);
    // mirror block of py positions: an aligned block of TL positions maps onto an aligned block (within one power-of-two
    // sub-block: low bits of the frequency fixed -> low bits of its negative fixed)
    const int pyB_any = y_mirror_pos(py0, d);
    const int pyB0 = pyB_any & ~(TL - 1);
    const bool self_plane = (px == pxB);  // xk == 0 or xk == Hx/2
    // layout [px][z][py]: element (px, z, py) at ((px * L + z) * M + py); one float4 = lines (2 jp, 2 jp + 1)
    const float4* sA = reinterpret_cast<const float4*>(S + (size_t)px * L * M + py0);
    const float4* sB = reinterpret_cast<const float4*>(S + (size_t)pxB * L * M + pyB0);
    const int rowq = M / 2;
#pragma unroll MI_FFT_UNROLL
    for (int i = threadIdx.x; i < hp * L; i += kThreadsXZ) {
        const int z = i / hp, jp = i - z * hp;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        if (z < d.z_in_hi) { a = sA[(size_t)z * rowq + jp]; b = sB[(size_t)z * rowq + jp]; }  // planes beyond: all zero, not stored
        const int cA = cell(2 * jp, pitch, hp, z), cB = cA + TL * pitch;  // rows TL + 2 jp carry the same mask
        tile[cA] = make_float2(a.x, a.y);
        tile[cA + pitch] = make_float2(a.z, a.w);
        tile[cB] = make_float2(b.x, b.y);
        tile[cB + pitch] = make_float2(b.z, b.w);
    }
    const float4* Gp = G + ((size_t)plane * M + py0) * L;
    using TW = TwLds<LZ2, R3>;
    float2* twl = tile + 2 * TL * pitch;
    TW::template fill<kThreadsXZ>(twl, tw);
    lds_barrier();
    const bool priv = ((2 * TL) % NW) == 0;
    if (!(d.dbg & 1)) {
        if constexpr (R3 > 1) {
            radix3_stage<R3, false, kThreadsXZ>(tile, 2 * TL, pitch, hp, priv, 1 << LZ2, twl + TW::r3);
            stage_sync(priv);
        }
        lds_fft<LZ2, false, kThreadsXZ, R3>(tile, 2 * TL * R3, pitch, hp, priv, twl);
    }
    if (priv) lds_barrier();  // the point-wise step pairs rows of different owners
    // point-wise: element (line j, position pz) of A pairs with (line jB, position pzB) of B
    float sw, cw;
    sincospif(-2.0f * (float)xk / (float)(2 * Hx), &sw, &cw);  // w = exp(-2 pi i xk / Nx), Nx = 2 Hx
    const float2 w = make_float2(cw, sw);
    const int n_it = (TL * L + kThreadsXZ - 1) / kThreadsXZ;
#pragma unroll 1
    for (int q = 0; q < n_it; ++q) {
        const int i = threadIdx.x + q * kThreadsXZ;
        if (i >= TL * L || (d.dbg & 2)) break;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (!BUILD) g = Gp[i];  // Gp[(size_t)j * L + pz] with i = j * L + pz
        int j = i / L;
        if (L % 64 == 0) j = __builtin_amdgcn_readfirstlane(j);  // a wave's 64 items share the line: scalar mirror math
        const int pz = i - j * L;
        const int jB = y_mirror_pos(py0 + j, d) - pyB0;
        const int pzB = mirror_pos(pz, L, LZ2, R3);
        const int cA = cell(j, pitch, hp, pz), cB = cell(TL + jB, pitch, hp, pzB);
        const float2 a = tile[cA];
        const float2 bm = tile[cB];
        const float2 bc = cconj(bm);
        const float2 E = make_float2(0.5f * (a.x + bc.x), 0.5f * (a.y + bc.y));
        const float2 dlt = csub(a, bc);                          // a - conj(b)
        const float2 O = make_float2(0.5f * dlt.y, -0.5f * dlt.x);  // -i/2 * (a - conj(b))
        const float2 wO = cmul(w, O);
        const float2 Xa = cadd(E, wO), Xb = csub(E, wO);
        if constexpr (BUILD) {
            Gout[((size_t)plane * M + py0) * L + i] = make_float4(Xa.x * scale, Xa.y * scale, Xb.x * scale, Xb.y * scale);
            continue;
        }
        float2 Ga = make_float2(g.x, g.y), Gb = make_float2(g.z, g.w);
        if (conj_otf) { Ga.y = -Ga.y; Gb.y = -Gb.y; }
        const float2 Ya = cmul(Xa, Ga), Yb = cmul(Xb, Gb);
        const float2 E2 = make_float2(0.5f * (Ya.x + Yb.x), 0.5f * (Ya.y + Yb.y));
        const float2 dY = csub(Ya, Yb);
        const float2 O2 = cmulc(make_float2(0.5f * dY.x, 0.5f * dY.y), w);  // (Ya - Yb) conj(w) / 2
        // Z'[k] = E' + i O' ; Z'[-k] = conj(E') + i conj(O')
        tile[cA] = make_float2(E2.x - O2.y, E2.y + O2.x);
        tile[cB] = make_float2(E2.x + O2.y, O2.x - E2.y);
    }
    if constexpr (BUILD) return;
    lds_barrier();
    if (!(d.dbg & 4)) {
        lds_fft<LZ2, true, kThreadsXZ, R3>(tile, 2 * TL * R3, pitch, hp, priv, twl);
        if constexpr (R3 > 1) {
            radix3_stage<R3, true, kThreadsXZ>(tile, 2 * TL, pitch, hp, priv, 1 << LZ2, twl + TW::r3);
            stage_sync(priv);
        }
    }
    if (priv) lds_barrier();
    float4* dA = reinterpret_cast<float4*>(T + (size_t)px * L * M + py0);
    float4* dB = reinterpret_cast<float4*>(T + (size_t)pxB * L * M + pyB0);
#pragma unroll MI_FFT_UNROLL
    for (int i = threadIdx.x; i < hp * L; i += kThreadsXZ) {
        const int z = i / hp, jp = i - z * hp;
        if (z < d.z_out_lo || z >= d.z_out_hi) continue;  // planes the crop drops
        const int cA = cell(2 * jp, pitch, hp, z), cB = cA + TL * pitch;
        const float2 a0 = tile[cA], a1 = tile[cA + pitch];
        dA[(size_t)z * rowq + jp] = make_float4(a0.x, a0.y, a1.x, a1.y);
        if (!self_plane) {
            const float2 b0 = tile[cB], b1 = tile[cB + pitch];
            dB[(size_t)z * rowq + jp] = make_float4(b0.x, b0.y, b1.x, b1.y);
        }
    }
}

// ---------------------------------------------------------------------------------------------- P3, pipelined
// The z pass as a persistent kernel (one work-group per CU): the OTF of the current tile is requested before the forward
// transform and the next tile's lines before the inverse transform, both into registers, so HBM stays busy during the FFT
// phases; stores drain behind.
// REALG: the OTF of a PSF that is mirror-symmetric about its centre sample is a real function times the phase ramp of the
// centre's offset from the grid origin: G holds the two real factors of a pair (float2 instead of float4: 4 instead of 8 B per
// voxel of OTF traffic, a sixth of this pass) and the ramp exp(-2 pi i (kx dx/Fx + ky dy/Fy + kz dz/Fz)) is put back from three
// small per-axis tables (x and y: scalar loads, z: one look-up per lane and tile).
struct RealOtf {
    const float2* g;     // [xk][py][pz] {Ra, Rb}
    const float2* ph_x;  // by xk
    const float2* ph_y;  // by ky
    const float2* ph_z;  // by kz
    // the factored form (otf_factor.h; k_z_pair_pipe<.., FACT>): {Ra, Rb} = (sum_r A_r[pz] Bh_r[side A], sum_r A_r[pz] Bh_r[side B])
    const float4* fa;    // [pz] the four A_r of a z position
    const float4* fb;    // [xk][py][side] the four Bh_r of a line: the 8 floats of a line pair are contiguous
};

template <int LZ2, int R3, bool REALG>
__global__ __launch_bounds__(kThreadsXZ, kWavesXZ) void k_z_conv_pipe(const float2* __restrict__ S, float2* __restrict__ T, const float4* __restrict__ G,
                                                           NativeDims d, const float2* __restrict__ tw, int conj_otf, int ntiles, RealOtf ro) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];
    constexpr int L = R3 << LZ2, NW = kThreadsXZ / 64;
    constexpr int TL = z_tile_lines(L), hp = TL / 2, pitch = row_pitch(L);
    constexpr int NA = hp * L;                                   // float4 of the A lines (and of the B lines) of a tile
    constexpr int NPA = (NA + kThreadsXZ - 1) / kThreadsXZ;
    constexpr int NG = TL * L;                                   // OTF float4 of a tile = point-wise items
    constexpr int NPG = (NG + kThreadsXZ - 1) / kThreadsXZ;
    constexpr int P = kThreadsXZ / hp;                           // transposed view: item k of a lane is position z0 + k * P
    constexpr bool PRIV = ((2 * TL) % NW) == 0;
    // WP: with one A line and one B line per wave, the B lines are stored so that LDS row TL + j holds the MIRROR PARTNER of A
    // line j -- both rows of a pair then belong to wave j and the point-wise step needs no work-group barrier either: forward
    // transforms, point-wise product and inverse transforms of a pair run back to back inside its wave (3 barriers per tile
    // instead of 5, all of them around the transposed fill and drain)
    constexpr bool WP = PRIV && TL == NW && (L % 64 == 0) && (NG % kThreadsXZ == 0);
    // point-wise view: item k of a lane is element pz0 of line j0 + k * JS when the lines divide the work-group evenly
    constexpr bool EVEN = (kThreadsXZ % L == 0) && (L % 64 == 0) && (NG % kThreadsXZ == 0) && ((kThreadsXZ / L) % 2 == 0 || kThreadsXZ == L);
    constexpr int JS = kThreadsXZ / (L > 0 ? L : 1);
    const int Hx = d.hx, M = d.ny;
    const int ytiles = M / TL, rowq = M / 2;
    // lane constants (tile-invariant; recomputed per phase from a laundered thread index so that they do not occupy registers
    // across the FFT phases): the swizzle is XOR-linear, so item k's slot is item 0's slot XOR a constant
    struct FView { int row, slot, z0, jp, pz; size_t off; };  // transposed view: item k = position z0 + k * P, line pair jp
    auto f_view = [&]() {
        const int tid = launder(threadIdx.x);
        const int z0 = tid / hp, jp = tid - z0 * hp;
        const int pz = phys(z0);
        return FView{(2 * jp) * pitch, pz ^ rmask(2 * jp, hp), z0, jp, pz, (size_t)z0 * rowq + jp};
    };
    // WP: A line index (0..TL-1) whose mirror partner is B line jb, 4 bits each (wave-uniform, recomputed per tile)
    auto partner_table = [&](const auto& w) {
        unsigned long long tab = 0;
        for (int jb = 0; jb < TL; ++jb) tab |= (unsigned long long)((y_mirror_pos(w.pyB0 + jb, d) - w.py0) & 15) << (4 * jb);
        return tab;
    };
    // WP: LDS cells of the B lines (2 jp, 2 jp + 1) at position slot `pzs` (unmasked)
    auto b_cells = [&](unsigned long long tab, int jp, int pzs, int& c0, int& c1) {
        const int r0 = TL + (int)((tab >> (8 * jp)) & 15), r1 = TL + (int)((tab >> (8 * jp + 4)) & 15);
        c0 = r0 * pitch + (pzs ^ rmask(r0, hp));
        c1 = r1 * pitch + (pzs ^ rmask(r1, hp));
    };
    float4 preA[NPA], preB[NPA];
    struct Where { int plane, py0, px, pxB, pyB0; };
    auto where = [&](int t) {
        Where w;
        w.plane = t / ytiles;
        w.py0 = (t - w.plane * ytiles) * TL;
        w.px = __builtin_amdgcn_readfirstlane(x_freq2pos(w.plane, d));
        w.pxB = __builtin_amdgcn_readfirstlane(x_freq2pos(w.plane == 0 ? 0 : Hx - w.plane, d));
        w.pyB0 = y_mirror_pos(w.py0, d) & ~(TL - 1);
        return w;
    };
    auto load_S = [&](int t) {
        const Where w = where(t);
        const FView fv = f_view();
        const float4* sA = reinterpret_cast<const float4*>(S + (size_t)w.px * L * M + w.py0) + fv.off;
        const float4* sB = reinterpret_cast<const float4*>(S + (size_t)w.pxB * L * M + w.pyB0) + fv.off;
#pragma unroll
        for (int k = 0; k < NPA; ++k) {
            if (NA % kThreadsXZ == 0 || (int)threadIdx.x + k * kThreadsXZ < NA) {
                float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vb = va;
                if (fv.z0 + k * P < d.z_in_hi) {  // planes beyond: all-zero input of a padded grid, never stored
                    va = sA[(size_t)(k * P) * rowq];
                    vb = sB[(size_t)(k * P) * rowq];
                }
                preA[k] = va;
                preB[k] = vb;
            }
        }
    };
    using TW = TwLds<LZ2, R3>;
    float2* twl = tile + 2 * TL * pitch;
    TW::template fill<kThreadsXZ>(twl, tw);
    int t = blockIdx.x;
    if (t < ntiles) load_S(t);
    for (; t < ntiles; t += gridDim.x) {
        const Where w = where(t);
        unsigned long long ptab = 0;
        if constexpr (WP) ptab = partner_table(w);
        {
        const FView fv = f_view();
#pragma unroll
        for (int k = 0; k < NPA; ++k) {
            if (NA % kThreadsXZ == 0 || (int)threadIdx.x + k * kThreadsXZ < NA) {
                const int cA = fv.row + (fv.slot ^ swz_c(k * P));
                int cB0 = cA + TL * pitch, cB1 = cB0 + pitch;  // rows TL + 2 jp (+1) carry the same mask
                if constexpr (WP) b_cells(ptab, fv.jp, fv.pz ^ swz_c(k * P), cB0, cB1);
                tile[cA] = make_float2(preA[k].x, preA[k].y);
                tile[cA + pitch] = make_float2(preA[k].z, preA[k].w);
                tile[cB0] = make_float2(preB[k].x, preB[k].y);
                tile[cB1] = make_float2(preB[k].z, preB[k].w);
            }
        }
        }
        const size_t g0 = ((size_t)w.plane * M + w.py0) * L;
        float4 gv[REALG ? 1 : NPG];
        float2 gr[REALG ? NPG : 1];
        float2 ph_xz = make_float2(1.0f, 0.0f), ph_yk[REALG ? NPG : 1];
        auto load_G = [&]() {
            // REALG: phase of (this tile's xk) x (this lane's kz), and of the ky of the line of every item (wave-uniform); requested
            // here, together with the OTF, so that they have arrived long before the point-wise step
            // (WP: item k of a lane is position lane + 64 k of its wave's line: one ky per wave, one kz per item)
            if constexpr (REALG) {
                const int tid = launder(threadIdx.x);
                if constexpr (WP) {
                    ph_xz = cmul(ro.ph_x[w.plane], ro.ph_y[y_pos2freq(w.py0 + __builtin_amdgcn_readfirstlane(tid >> 6), d)]);
    #pragma unroll
                    for (int k = 0; k < NPG; ++k) ph_yk[k] = ro.ph_z[pos2freq((tid & 63) + 64 * k, LZ2, R3)];
                } else {
                    ph_xz = cmul(ro.ph_x[w.plane], ro.ph_z[pos2freq(tid % L, LZ2, R3)]);
                    const int j0e = __builtin_amdgcn_readfirstlane(tid / L);
    #pragma unroll
                    for (int k = 0; k < NPG; ++k) ph_yk[k] = ro.ph_y[y_pos2freq(w.py0 + j0e + k * JS, d)];
                }
            }
            {
                const int tid = launder(threadIdx.x);
                // WP: the OTF entries of line `wave`, positions lane + 64 k
                const size_t gl = WP ? g0 + (size_t)(tid >> 6) * L + (tid & 63) : g0 + tid;
    #pragma unroll
                for (int k = 0; k < NPG; ++k) {
                    if (NG % kThreadsXZ == 0 || tid + k * kThreadsXZ < NG) {
                        if constexpr (REALG) gr[k] = ro.g[gl + (WP ? 64 : kThreadsXZ) * k];
                        else gv[k] = G[gl + (WP ? 64 : kThreadsXZ) * k];
                    }
                }
            }
        };
        // (a sixteen-point top stage -- the FIRST of the forward transform -- and the OTF registers do not fit 128 registers together:
        // the OTF is then requested behind that stage)
        constexpr bool LATE_G = R3 == 1 && LZ2 - seg_below(LZ2, LZ2) == 4;
        if (R3 != 9 && !LATE_G) load_G();  // (radix-9 lines: requested behind the 9-point stage, which needs the registers)
        lds_barrier();
        if constexpr (R3 > 1) {
            radix3_stage<R3, false, kThreadsXZ>(tile, 2 * TL, pitch, hp, PRIV, 1 << LZ2, twl + TW::r3);
            stage_sync(PRIV);
        }
        if (R3 == 9) load_G();
        if constexpr (LATE_G) {
            lds_fft<LZ2, false, kThreadsXZ, R3, 0, 4>(tile, 2 * TL * R3, pitch, hp, PRIV, twl);
            load_G();
            lds_fft<LZ2, false, kThreadsXZ, R3, 4, LZ2>(tile, 2 * TL * R3, pitch, hp, PRIV, twl);
        } else {
            lds_fft<LZ2, false, kThreadsXZ, R3>(tile, 2 * TL * R3, pitch, hp, PRIV, twl);
        }
        if (PRIV && !WP) lds_barrier();  // the point-wise step pairs rows of different owners
        float sw, cw;
        sincospif(-2.0f * (float)w.plane / (float)(2 * Hx), &sw, &cw);  // exp(-2 pi i xk / Nx), Nx = 2 Hx
        const float2 wx = make_float2(cw, sw);
        const int tid = launder(threadIdx.x);
        const int pz0 = tid % L, j0 = __builtin_amdgcn_readfirstlane(tid / L);
        const int pA = phys(WP ? (tid & 63) : pz0), pB = phys(mirror_pos(pz0, L, LZ2, R3));
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
        for (int k = 0; k < NPG; ++k) {
            const int i = tid + k * kThreadsXZ;
            if (NG % kThreadsXZ == 0 || i < NG) {
                int cA, cB;
                if constexpr (WP) {  // lines A[wave] and its partner in row TL + wave, position lane + 64 k
                    cA = wv * pitch + (pA ^ swz_c(64 * k) ^ rmask(wv, hp));
                    cB = (TL + wv) * pitch + (phys(mirror_pos((tid & 63) + 64 * k, L, LZ2, R3)) ^ rmask(TL + wv, hp));
                } else if (EVEN) {
                    const int j = j0 + k * JS;                                // scalar: the line is shared by the wave
                    const int jB = y_mirror_pos(w.py0 + j, d) - w.pyB0;       // scalar mirror math
                    cA = j * pitch + (pA ^ rmask(j, hp));
                    cB = (TL + jB) * pitch + (pB ^ rmask(TL + jB, hp));
                } else {
                    int j = i / L;
                    if (L % 64 == 0) j = __builtin_amdgcn_readfirstlane(j);
                    const int pz = i - j * L;
                    const int jB = y_mirror_pos(w.py0 + j, d) - w.pyB0;
                    cA = cell(j, pitch, hp, pz);
                    cB = cell(TL + jB, pitch, hp, mirror_pos(pz, L, LZ2, R3));
                }
                const float2 a = tile[cA];
                const float2 bc = cconj(tile[cB]);
                const float2 E = make_float2(0.5f * (a.x + bc.x), 0.5f * (a.y + bc.y));
                const float2 dlt = csub(a, bc);
                const float2 O = make_float2(0.5f * dlt.y, -0.5f * dlt.x);  // -i/2 * (a - conj(b))
                const float2 wO = cmul(wx, O);
                const float2 Xa = cadd(E, wO), Xb = csub(E, wO);
                float2 Ya, Yb;
                if constexpr (REALG) {
                    float2 P = cmul(ph_xz, ph_yk[k]);                         // (REALG requires the EVEN item layout)
                    if (conj_otf) P.y = -P.y;
                    const float2 XaP = cmul(Xa, P), XbP = cmul(Xb, P);
                    Ya = make_float2(XaP.x * gr[k].x, XaP.y * gr[k].x);
                    Yb = make_float2(XbP.x * gr[k].y, XbP.y * gr[k].y);
                } else {
                    float2 Ga = make_float2(gv[k].x, gv[k].y), Gb = make_float2(gv[k].z, gv[k].w);
                    if (conj_otf) { Ga.y = -Ga.y; Gb.y = -Gb.y; }
                    Ya = cmul(Xa, Ga);
                    Yb = cmul(Xb, Gb);
                }
                const float2 E2 = make_float2(0.5f * (Ya.x + Yb.x), 0.5f * (Ya.y + Yb.y));
                const float2 dY = csub(Ya, Yb);
                const float2 O2 = cmulc(make_float2(0.5f * dY.x, 0.5f * dY.y), wx);
                tile[cA] = make_float2(E2.x - O2.y, E2.y + O2.x);
                tile[cB] = make_float2(E2.x + O2.y, O2.x - E2.y);
            }
        }
        const int tn = t + gridDim.x;
        if (R3 != 9 && tn < ntiles) load_S(tn);
        if (WP) wave_lds_fence();
        else lds_barrier();
        lds_fft<LZ2, true, kThreadsXZ, R3>(tile, 2 * TL * R3, pitch, hp, PRIV, twl);
        if constexpr (R3 > 1) {
            radix3_stage<R3, true, kThreadsXZ>(tile, 2 * TL, pitch, hp, PRIV, 1 << LZ2, twl + TW::r3);
            stage_sync(PRIV);
        }
        if (R3 == 9 && tn < ntiles) load_S(tn);
        if (PRIV) lds_barrier();
        const bool self_plane = (w.px == w.pxB);
        const FView fv = f_view();
        float4* dA = reinterpret_cast<float4*>(T + (size_t)w.px * L * M + w.py0) + fv.off;
        float4* dB = reinterpret_cast<float4*>(T + (size_t)w.pxB * L * M + w.pyB0) + fv.off;
#pragma unroll
        for (int k = 0; k < NPA; ++k) {
            const int zk = fv.z0 + k * P;
            if ((NA % kThreadsXZ == 0 || (int)threadIdx.x + k * kThreadsXZ < NA) && zk >= d.z_out_lo && zk < d.z_out_hi) {
                const int cA = fv.row + (fv.slot ^ swz_c(k * P));
                int cB0 = cA + TL * pitch, cB1 = cB0 + pitch;
                if constexpr (WP) b_cells(ptab, fv.jp, fv.pz ^ swz_c(k * P), cB0, cB1);
                const float2 a0 = tile[cA], a1 = tile[cA + pitch];
                dA[(size_t)(k * P) * rowq] = make_float4(a0.x, a0.y, a1.x, a1.y);
                if (!self_plane) {
                    const float2 b0 = tile[cB0], b1 = tile[cB1];
                    dB[(size_t)(k * P) * rowq] = make_float4(b0.x, b0.y, b1.x, b1.y);
                }
            }
        }
        lds_barrier();  // the tile is free for the next fill
    }
}

// ---------------------------------------------------------------------------------------------- P3, pair-interleaved layout
// The spectra around the z pass as [xk][z][ty][side][TL]: the TL A lines of a tile and, right behind them, their TL mirror
// partners (in partner order), so that a tile of only TL = 8 line pairs still moves whole 128-byte segments and two 8-wave
// work-groups with a 64-KB tile each share a CU: one transforms while the other waits for HBM.  Replaces the same chain as
// k_z_conv_pipe (decon.m:162-172: the z part of fftn, .* otf, the z part of ifftn); same OTF array, same point-wise step.
//   NT = 512 (lines of up to 576 points): a wave owns one A line and its partner -- forward transform, point-wise step and
//     inverse transform of the pair run inside the wave, the only work-group barriers surround the transposed fill and drain;
//     for 2^a lines of 256 / 512 points the fill and the drain ARE the top super-stage (on the registers of the global access).
//   NT = 1024 (768, 1152 points): a wave owns one line; the point-wise step sits between two barriers.  (1024-point lines run on
//     NT = 512 with 246 registers: see the launch.)
//   Lines of 3 * 2^a / 9 * 2^a points carry the radix-3 / 9 stage in front (behind, inverse) of the power-of-two chain.
// FACT (with REALG): the real OTF is rebuilt from its rank-4 factors instead of being read -- 8 B instead of 10 B per voxel.  The
// A_r table (16 B per z position) takes the place of the z ramp's table in LDS, which leaves the two work-groups per CU of the 64-KB
// tiles; the ramp of the lane's positions comes from the L1-hot global table into the registers the stored entries arrived in, and
// the eight Bh_r of the wave's line pair are a uniform load.  Four FMAs per entry more in the point-wise step.
// FULLZ: every z plane is read and written (a circular grid, or a padded one that prunes nothing): the fill and the drain carry no
// plane bounds (z_full_grid, fft_native_route.h).  wxt: exp(-2 pi i xk / Nx) by plane (NativeFft::fill_plane_twiddles).
template <int LZ2, int R3, bool REALG, int NT, int TL, bool PHL = true, bool TOPON = true, bool FACT = false, bool FULLZ = false>
__global__ __launch_bounds__(NT, (NT == 512 && (R3 << LZ2) > 576) ? 2 : kWavesXZ) void k_z_pair_pipe(const float2* __restrict__ S, float2* __restrict__ T, const float4* __restrict__ G,
                                                              NativeDims d, const float2* __restrict__ tw, int conj_otf, int ntiles, RealOtf ro,
                                                              int* __restrict__ tile_ctr, const float2* __restrict__ wxt) {
    constexpr int L = R3 << LZ2, NW = NT / 64, hp = TL, pitch = row_pitch(L);
    // All of the work-group's LDS as ONE static array -- tile, twiddle tables, the table of the OTF form, the tile counter -- so that the
    // compiler knows every address as a number (behind a dynamic array's base each swizzled access costs a second instruction).  Its size
    // is what the launch computes the work-groups per CU from (z_pair_lds); the launch passes no dynamic bytes.
    constexpr size_t kLds = z_pair_lds(LZ2, R3, REALG, FACT);
    static_assert(kLds == lds_bytes(2 * TL, L) + (FACT ? 16 : REALG && PHL ? 8 : 0) * (size_t)L && kLds % 16 == 0, "the static array is the launch's LDS figure");
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[kLds + sizeof(int)];
    float2* const tile = reinterpret_cast<float2*>(lds_all);
    int& s_next_tile = *reinterpret_cast<int*>(lds_all + kLds);  // tiles from a device counter when tile_ctr != nullptr (see k_x_fused_pipe)
    // LIT: power-of-two lines (pitch = L): a row's base and a slot occupy disjoint bits, so every swizzled access is addressed by
    // BYTE offset as (lane constant) XOR (literal), one instruction; lines of 3 * 2^a and 9 * 2^a points keep slot arithmetic
    constexpr bool LIT = R3 == 1;
    static_assert(!LIT || (pitch == L && (L & (L - 1)) == 0), "power-of-two lines are their own pitch");
    const auto at = [&](unsigned byte_off) -> float2& { return *reinterpret_cast<float2*>(lds_all + byte_off); };
    // WP: every wave owns one A line and its partner (rows wave, TL + wave), so the point-wise step is wave-private too;
    // else (1024-point lines: 16 waves on 16 rows) a wave owns ONE row, the point-wise step of line `wave % TL` is shared by the
    // owners of its two rows -- half of the positions each -- and sits between two work-group barriers
    constexpr bool WP = TL == NW;
    static_assert((WP || (NW == 2 * TL && L % 128 == 0)) && L % 64 == 0 && (TL * L) % NT == 0, "one or two waves per line pair");
    constexpr int NPA = TL * L / NT;  // float4 (two neighbouring lines at one z) per lane and tile
    constexpr int P = NT / TL;        // item k of a lane: position z0 + k * P
    constexpr int NPG = TL * L / NT;  // point-wise items (mirror pairs) per lane
    // the top super-stage of the chain (stages TOPS .. LZ2-1) works on elements z0 + k * 2^TOPS: exactly the items of a lane
    constexpr int TOPS = seg_below(LZ2, LZ2), TOPR = LZ2 - TOPS;
    constexpr bool TOPREG = TOPON && R3 == 1 && (1 << TOPS) == P && (1 << TOPR) == NPA;
    const int M = d.ny, ytiles = M / TL;
    const size_t ZR = (size_t)(M + d.zpad);  // float4 per row (xk, z) of the paired layout
    struct FView { int row, slot, z0; size_t off; };
    auto f_view = [&]() {
        const int tid = launder(threadIdx.x);
        const int z0 = tid / TL, jq = tid - z0 * TL;  // float4 jq of the segment: lines 2 jq, 2 jq + 1 (rows TL.. = B side)
        return FView{(2 * jq) * pitch, phys(z0) ^ rmask(2 * jq, hp), z0, (size_t)z0 * ZR + jq};
    };
    // the cells of item k of the transposed view (lines 2 jq and 2 jq + 1 at position z0 + k P)
    const auto f_cells = [&](const FView& fv, int k, float2*& c0, float2*& c1) {
        if constexpr (LIT) {
            const unsigned b = (((unsigned)fv.row | (unsigned)fv.slot) << 3) ^ ((unsigned)swz_c(k * P) << 3);
            c0 = &at(b);
            c1 = &at(b + pitch * 8);
        } else {
            const int c = fv.row + (fv.slot ^ swz_c(k * P));
            c0 = tile + c;
            c1 = tile + c + pitch;
        }
    };
    float4 pre[NPA];
    auto load_S = [&](int t) {
        const int pl = t / ytiles, ty = t - pl * ytiles, plane = d.xk0 + pl;  // (tiles of the planes xk0 ..: all, or a chunk)
        const FView fv = f_view();
        const float4* sp = reinterpret_cast<const float4*>(S) + (size_t)plane * L * ZR + (size_t)ty * TL + fv.off;
#pragma unroll
        for (int k = 0; k < NPA; ++k) pre[k] = (FULLZ || fv.z0 + k * P < d.z_in_hi) ? sp[(size_t)(k * P) * ZR] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
    using TW = TwLds<LZ2, R3>;
    float2* twl = tile + 2 * TL * pitch;
    TW::template fill<NT>(twl, tw);
    // REALG: the z ramp by POSITION, behind the twiddle tables (stride-1 look-ups in the point-wise step; PHL = false when that
    // table would cost the second work-group of the CU: the ramp then comes from global memory, by frequency)
    float2* phl = twl + TW::total;
    float4* atab = reinterpret_cast<float4*>(twl + TW::total);
    static_assert(!FACT || (REALG && PHL && TW::total % 2 == 0 && (2 * TL * row_pitch(R3 << LZ2)) % 2 == 0), "the A table is float4-aligned, in place of phl");
    if constexpr (FACT) {
        for (int p = threadIdx.x; p < L; p += NT) atab[p] = ro.fa[p];
    } else if constexpr (REALG && PHL) {
        for (int p = threadIdx.x; p < L; p += NT) phl[p] = ro.ph_z[pos2freq(p, LZ2, R3)];
    }
    const bool dyn = tile_ctr != nullptr;
    int t = blockIdx.x, tn = t + (int)gridDim.x;
    if (dyn) {
        if (threadIdx.x == 0) s_next_tile = atomicAdd(tile_ctr, 2);
        lds_barrier();
        t = __builtin_amdgcn_readfirstlane(s_next_tile);
        tn = t + 1;
    }
    if (t < ntiles) load_S(t);
    lds_barrier();  // the tables: the first tile's top super-stage reads them before any other barrier
    for (; t < ntiles;) {
        int fetched = 0;
        if (dyn && threadIdx.x == 0) fetched = atomicAdd(tile_ctr, 1);  // the tile after the next one
        const int pl_ = t / ytiles, py0 = (t - pl_ * ytiles) * TL, plane = d.xk0 + pl_;
        {
            const FView fv = f_view();
            if constexpr (TOPREG) {  // the top super-stage on the registers the loads arrived in
                float2 v[NPA], u[NPA];
#pragma unroll
                for (int k = 0; k < NPA; ++k) { v[k] = make_float2(pre[k].x, pre[k].y); u[k] = make_float2(pre[k].z, pre[k].w); }
                butterflies<TOPR, TOPS, false>(v, twl + tw_off(LZ2, TOPS), fv.z0);
                butterflies<TOPR, TOPS, false>(u, twl + tw_off(LZ2, TOPS), fv.z0);
#pragma unroll
                for (int k = 0; k < NPA; ++k) {
                    float2 *c0, *c1;
                    f_cells(fv, k, c0, c1);
                    *c0 = v[k];
                    *c1 = u[k];
                }
            } else {
#pragma unroll
            for (int k = 0; k < NPA; ++k) {
                float2 *c0, *c1;
                f_cells(fv, k, c0, c1);
                *c0 = make_float2(pre[k].x, pre[k].y);
                *c1 = make_float2(pre[k].z, pre[k].w);
            }
            }
        }
        const size_t g0 = ((size_t)plane * M + py0) * L;
        // exp(-2 pi i xk / Nx), Nx = 2 Hx, of the point-wise step: a uniform load, requested a transform ahead (k_plane_twiddles evaluates
        // the expression this step used to, per tile and wave)
        const float2 wx = wxt[plane];
        float4 gv[REALG ? 1 : NPG];
        float2 gr[REALG ? NPG : 1];
        float2 ph_xy = make_float2(1.0f, 0.0f);
        float4 b_a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b_b = b_a;
        auto load_G = [&]() {
            const int tid = launder(threadIdx.x);
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int line = WP ? wv : wv % TL, p0 = WP ? 0 : (wv / TL) * (L / 2);
            if constexpr (REALG) {
                ph_xy = cmul(ro.ph_x[plane], ro.ph_y[y_pos2freq(py0 + line, d)]);
            }
            if constexpr (FACT) {  // gr[k]: the z ramp of position lane + 64 k (+ p0); b_a, b_b: the line's factors (wave-uniform)
                const float4* bp = ro.fb + ((size_t)plane * M + py0 + line) * 2;
                b_a = bp[0];
                b_b = bp[1];
                if constexpr (R3 == 1 && WP && NPG >= 2) {
                    // frequency of position lane + 64 k: (brev6(lane) << (LZ2 - 6)) | brev(k) -- the NPG entries of a lane are neighbours
                    // behind one lane base (16-byte aligned: real_otf_args), taken as float4 and handed out in bit-reversed order
                    constexpr int KB = LZ2 - 6;
                    const float4* rp = reinterpret_cast<const float4*>(ro.ph_z + ((int)brev_n((unsigned)(tid & 63), 6) << KB));
                    float4 blk[NPG / 2];
#pragma unroll
                    for (int q = 0; q < NPG / 2; ++q) blk[q] = rp[q];
#pragma unroll
                    for (int k = 0; k < NPG; ++k) {
                        const int f = bit_rev(k, KB);
                        gr[k] = (f & 1) ? make_float2(blk[f / 2].z, blk[f / 2].w) : make_float2(blk[f / 2].x, blk[f / 2].y);
                    }
                    return;
                }
#pragma unroll
                for (int k = 0; k < NPG; ++k) gr[k] = ro.ph_z[pos2freq(p0 + (tid & 63) + 64 * k, LZ2, R3)];
                return;
            }
            const size_t gl = g0 + (size_t)line * L + p0 + (tid & 63);
#pragma unroll
            for (int k = 0; k < NPG; ++k) {
                if constexpr (REALG) gr[k] = ro.g[gl + 64 * k];
                else gv[k] = G[gl + 64 * k];
            }
        };
        // (complex OTF and a sixteen-point top stage, the first of the forward transform: see k_z_conv_pipe)
        constexpr bool LATE_G = !REALG && R3 == 1 && !TOPREG && LZ2 - seg_below(LZ2, LZ2) == 4;
        if (R3 != 9 && !LATE_G) load_G();  // (radix-9 lines: requested behind the 9-point stage, which needs the registers)
        lds_barrier();
        if constexpr (R3 > 1) {
            radix3_stage<R3, false, NT>(tile, 2 * TL, pitch, hp, true, 1 << LZ2, twl + TW::r3);
            wave_lds_fence();
        }
        if (R3 == 9) load_G();
        if constexpr (LATE_G) {
            lds_fft<LZ2, false, NT, R3, 0, 4, 0, LIT>(tile, 2 * TL * R3, pitch, hp, true, twl);
            load_G();
            lds_fft<LZ2, false, NT, R3, 4, LZ2, 0, LIT>(tile, 2 * TL * R3, pitch, hp, true, twl);
        } else {
            lds_fft<LZ2, false, NT, R3, TOPREG ? TOPR : 0, LZ2, 0, LIT>(tile, 2 * TL * R3, pitch, hp, true, twl);
        }
        if constexpr (!WP) lds_barrier();
        {
            const int tid = launder(threadIdx.x);
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            // item k: position lane + 64 k of the wave's A line and its mirror in the partner line.  The mirror of a position
            // whose high bits 64 k are not zero is (lane ^ 63) + [mirror of the high bits alone], else the mirror of `lane` among
            // the first 64 positions: lane constants XOR compile-time numbers, like every slot here
            const int lane = tid & 63;
            const int line = WP ? wv : wv % TL, p0 = WP ? 0 : (wv / TL) * (L / 2);  // (scalar)
            const int pA = phys(lane) ^ rmask(line, hp), pB1 = phys(lane ^ 63) ^ rmask(TL + line, hp);
            const int pB0 = phys(mirror_pos(lane, L, LZ2, R3)) ^ rmask(TL + line, hp);
#pragma unroll
            for (int k = 0; k < NPG; ++k) {
                const int hb = 64 * k + p0;  // the position bits above the lane's six
                float2 *qA, *qB;
                if constexpr (LIT) {  // (byte offsets: the rows' bases OR-ed into the lane constants, one XOR of a literal per cell)
                    const int flo = (int)brev_n((unsigned)hb, LZ2);
                    const int mhi = flo ? (int)brev_n((unsigned)((1 << (LZ2 - 6)) - flo), LZ2) : 0;
                    const unsigned rA = (unsigned)(line * pitch), rB = (unsigned)((TL + line) * pitch);
                    qA = &at(((rA | (unsigned)pA) << 3) ^ ((unsigned)swz_c(hb) << 3));
                    qB = &at(flo ? ((rB | (unsigned)pB1) << 3) ^ ((unsigned)swz_c(mhi) << 3) : (rB | (unsigned)pB0) << 3);
                } else {  // (3 * 2^a, 9 * 2^a: the mirror map is not XOR-linear)
                    qA = tile + line * pitch + (pA ^ swz_c(hb));
                    qB = tile + (TL + line) * pitch + (phys(mirror_pos(lane + hb, L, LZ2, R3)) ^ rmask(TL + line, hp));
                }
                const float2 a = *qA;
                const float2 bc = cconj(*qB);
                const float2 E = make_float2(0.5f * (a.x + bc.x), 0.5f * (a.y + bc.y));
                const float2 dlt = csub(a, bc);
                const float2 O = make_float2(0.5f * dlt.y, -0.5f * dlt.x);
                const float2 wO = cmul(wx, O);
                const float2 Xa = cadd(E, wO), Xb = csub(E, wO);
                float2 Ya, Yb;
                if constexpr (FACT) {
                    float2 Pq = cmul(ph_xy, gr[k]);
                    if (conj_otf) Pq.y = -Pq.y;
                    const float4 A4 = atab[lane + hb];
                    const float ga = fmaf(A4.w, b_a.w, fmaf(A4.z, b_a.z, fmaf(A4.y, b_a.y, A4.x * b_a.x)));
                    const float gb = fmaf(A4.w, b_b.w, fmaf(A4.z, b_b.z, fmaf(A4.y, b_b.y, A4.x * b_b.x)));
                    const float2 XaP = cmul(Xa, Pq), XbP = cmul(Xb, Pq);
                    Ya = make_float2(XaP.x * ga, XaP.y * ga);
                    Yb = make_float2(XbP.x * gb, XbP.y * gb);
                } else if constexpr (REALG) {
                    float2 Pq = cmul(ph_xy, PHL ? phl[lane + hb] : ro.ph_z[pos2freq(lane + hb, LZ2, R3)]);
                    if (conj_otf) Pq.y = -Pq.y;
                    const float2 XaP = cmul(Xa, Pq), XbP = cmul(Xb, Pq);
                    Ya = make_float2(XaP.x * gr[k].x, XaP.y * gr[k].x);
                    Yb = make_float2(XbP.x * gr[k].y, XbP.y * gr[k].y);
                } else {
                    float2 Ga = make_float2(gv[k].x, gv[k].y), Gb = make_float2(gv[k].z, gv[k].w);
                    if (conj_otf) { Ga.y = -Ga.y; Gb.y = -Gb.y; }
                    Ya = cmul(Xa, Ga);
                    Yb = cmul(Xb, Gb);
                }
                const float2 E2 = make_float2(0.5f * (Ya.x + Yb.x), 0.5f * (Ya.y + Yb.y));
                const float2 dY = csub(Ya, Yb);
                const float2 O2 = cmulc(make_float2(0.5f * dY.x, 0.5f * dY.y), wx);
                *qA = make_float2(E2.x - O2.y, E2.y + O2.x);
                *qB = make_float2(E2.x + O2.y, O2.x - E2.y);
            }
        }
        // (requesting them right after the fill, a whole tile ahead, gains nothing with two work-groups per CU: 4.72 vs 4.68 ms; with
        // the one 1024-thread work-group of 1024-point lines it LOSES -- 6.28 against 5.90 ms on 1024 x 576 x 4096, A / B in one
        // process, the loads unconditional and behind the OTF loads so that every wait stays counted; a 512-thread variant with a
        // line pair per wave measured 6.00 with the 4 x 4 top stages -- with the 16-point top stage on the registers of the global
        // access it became the kept form, see the launch: round 4, profiles/zpass_ab.py)
        if (R3 != 9 && tn < ntiles) load_S(tn);
        if constexpr (WP) wave_lds_fence();
        else lds_barrier();
        lds_fft<LZ2, true, NT, R3, 0, TOPREG ? TOPS : LZ2, 0, LIT>(tile, 2 * TL * R3, pitch, hp, true, twl);
        if constexpr (R3 > 1) {
            radix3_stage<R3, true, NT>(tile, 2 * TL, pitch, hp, true, 1 << LZ2, twl + TW::r3);
            wave_lds_fence();
        }
        if (R3 == 9 && tn < ntiles) load_S(tn);
        lds_barrier();
        {
            const FView fv = f_view();
            float4* dp = reinterpret_cast<float4*>(T) + (size_t)plane * L * ZR + (size_t)(py0 / TL) * TL + fv.off;
#pragma unroll
            for (int k = 0; k < NPA; ++k) {
                const int zk = fv.z0 + k * P;
                if constexpr (!TOPREG) {
                if (FULLZ || (zk >= d.z_out_lo && zk < d.z_out_hi)) {
                    float2 *c0, *c1;
                    f_cells(fv, k, c0, c1);
                    const float2 a0 = *c0, a1 = *c1;
                    dp[(size_t)(k * P) * ZR] = make_float4(a0.x, a0.y, a1.x, a1.y);
                }
                }
            }
            if constexpr (TOPREG) {
                float2 v[NPA], u[NPA];
#pragma unroll
                for (int k = 0; k < NPA; ++k) {
                    float2 *c0, *c1;
                    f_cells(fv, k, c0, c1);
                    v[k] = *c0;
                    u[k] = *c1;
                }
                butterflies<TOPR, TOPS, true>(v, twl + tw_off(LZ2, TOPS), fv.z0);
                butterflies<TOPR, TOPS, true>(u, twl + tw_off(LZ2, TOPS), fv.z0);
#pragma unroll
                for (int k = 0; k < NPA; ++k) {
                    const int zk = fv.z0 + k * P;
                    if (FULLZ || (zk >= d.z_out_lo && zk < d.z_out_hi)) dp[(size_t)(k * P) * ZR] = make_float4(v[k].x, v[k].y, u[k].x, u[k].y);
                }
            }
        }
        if (dyn && threadIdx.x == 0) s_next_tile = fetched;
        lds_barrier();
        t = tn;
        tn = dyn ? __builtin_amdgcn_readfirstlane(s_next_tile) : tn + (int)gridDim.x;
    }
}

// exp(-2 pi i xk / Nx), Nx = 2 Hx, for xk <= Hx/2: the plane twiddle of the point-wise step of k_z_pair_pipe, evaluated on the device
// by the expression the other z kernels evaluate per tile, so that the paired pass reads the bits it used to compute
__global__ __launch_bounds__(256) void k_plane_twiddles(float2* __restrict__ wxt, int Hx) {
    const int plane = blockIdx.x * blockDim.x + threadIdx.x;
    if (plane > Hx / 2) return;
    float sw, cw;
    sincospif(-2.0f * (float)plane / (float)(2 * Hx), &sw, &cw);
    wxt[plane] = make_float2(cw, sw);
}

// Complex pair OTF -> real pair OTF: Gr = Re(G * conj(P)) with P the phase ramp of the PSF centre's offset; the largest
// imaginary part that is dropped and the largest magnitude are returned (float bits, atomic max) for the host's decision.
__global__ __launch_bounds__(256) void k_g_to_real(const float4* __restrict__ G, float2* __restrict__ Gr, NativeDims d, RealOtf ro,
                                                    size_t total, unsigned* __restrict__ stats) {
    const int M = d.ny, L = d.nz;
    float max_im = 0.0f, max_re = 0.0f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pz = (int)(i % L);
        const size_t r = i / L;
        const int py = (int)(r % M), xk = (int)(r / M);
        const float2 P = cmul(cmul(ro.ph_x[xk], ro.ph_y[y_pos2freq(py, d)]), ro.ph_z[pos2freq(pz, d.lz2, d.r3z)]);
        const float4 g = G[i];
        const float2 a = cmulc(make_float2(g.x, g.y), P), b = cmulc(make_float2(g.z, g.w), P);
        Gr[i] = make_float2(a.x, b.x);
        max_im = fmaxf(max_im, fmaxf(fabsf(a.y), fabsf(b.y)));
        max_re = fmaxf(max_re, fmaxf(fabsf(a.x), fabsf(b.x)));
    }
    atomicMax(&stats[0], __float_as_uint(max_im));  // non-negative floats order like their bit patterns
    atomicMax(&stats[1], __float_as_uint(max_re));
}

// the real OTF of a slot and its phase tables ([xk <= Hx/2, rounded up to an even count][ky][kz] behind each other in `ph`)
constexpr int ph_x_entries(int hx) { return (hx / 2 + 2) & ~1; }
RealOtf real_otf_args(const NativeFft& f, bool adj_slot) {
    RealOtf ro{};
    ro.g = adj_slot ? f.Gr_adj.as<float2>() : f.Gr.as<float2>();
    ro.ph_x = f.ph.as<float2>();
    ro.ph_y = ro.ph_x + ph_x_entries(f.dims.hx);  // (an even count, and y is even: the z table starts on 16 bytes, k_z_pair_pipe reads it as float4)
    ro.ph_z = ro.ph_y + f.dims.ny;
    if (f.otf_factored()) {
        ro.fa = adj_slot ? f.Gf_adj.as<float4>() : f.Gf.as<float4>();
        ro.fb = ro.fa + f.dims.nz;
    }
    return ro;
}

// ---------------------------------------------------------------------------------------------- the factored real OTF: tables
// (otf_factor.h has the model and the host half.)  All sums in double.
// A_r by z POSITION from A_r by frequency: the z pass looks its entries up by position
__global__ __launch_bounds__(256) void k_fact_a_table(const double* __restrict__ a_freq, float4* __restrict__ fa, NativeDims d) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= d.nz) return;
    const double* a = a_freq + 4 * (size_t)pos2freq(p, d.lz2, d.r3z);
    fa[p] = make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
}
// Bh_r of the line (xk, py, side): kx = xk (side A) or xk + Hx (side B) -- the two spectrum entries Xa, Xb the point-wise step untangles
// -- and ky = the frequency at position py; side B carries the sign the stored form carries (try_factored_otf).  cs: [kx < 2 nx][r][y]{C, S}, the x half of the cosine sum (otf_factor_B_x) times the scale.
__global__ __launch_bounds__(256) void k_fact_b_table(const double2* __restrict__ cs, float4* __restrict__ fb, NativeDims d, int ky_psf, size_t total) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int side = (int)(i & 1);
    const size_t ln = i >> 1;
    const int py = (int)(ln % d.ny), xk = (int)(ln / d.ny), nx = d.hx / 2 + 1;
    const int ky = y_pos2freq(py, d);
    const double2* c = cs + (size_t)(xk + side * nx) * 4 * ky_psf;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int y = 0; y < ky_psf; ++y) {
        const long long t = (((long long)ky * (y - ky_psf / 2)) % d.ny + d.ny) % d.ny;
        double sn, cn;
        sincospi(2.0 * (double)t / (double)d.ny, &sn, &cn);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += cn * c[r * ky_psf + y].x - sn * c[r * ky_psf + y].y;
    }
    fb[i] = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
}
// largest |Gr - sum_r A_r Bh_r| and largest |Gr| over the whole array (float bits, atomic max)
__global__ __launch_bounds__(256) void k_fact_compare(const float2* __restrict__ Gr, const float4* __restrict__ fa, const float4* __restrict__ fb,
                                                       NativeDims d, size_t total, unsigned* __restrict__ stats) {
    const int L = d.nz;
    float max_d = 0.0f, max_g = 0.0f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pz = (int)(i % L);
        const size_t ln = i / L;
        const float4 a = fa[pz], ba = fb[2 * ln], bb = fb[2 * ln + 1];
        const float2 g = Gr[i];
        const float ga = fmaf(a.w, ba.w, fmaf(a.z, ba.z, fmaf(a.y, ba.y, a.x * ba.x)));
        const float gb = fmaf(a.w, bb.w, fmaf(a.z, bb.z, fmaf(a.y, bb.y, a.x * bb.x)));
        max_d = fmaxf(max_d, fmaxf(fabsf(g.x - ga), fabsf(g.y - gb)));
        max_g = fmaxf(max_g, fmaxf(fabsf(g.x), fabsf(g.y)));
    }
    atomicMax(&stats[0], __float_as_uint(max_d));
    atomicMax(&stats[1], __float_as_uint(max_g));
}

// the paired z pass: one case per length of MI_ZQ_CASES (fft_native_route.h), with its threads per work-group and its PHL flag
#define MI_ZQ_CALL(LG, R, NTH, PH) case LG * 16 + R: return f(Int<LG>{}, Int<R>{}, Int<NTH>{}, std::bool_constant<PH>{});
template <class F>
int z_pair_case(const NativeDims& d, F&& f) {
    switch (d.lz2 * 16 + d.r3z) { MI_ZQ_CASES(MI_ZQ_CALL) default: return fail(MI_ERR_UNSUPPORTED, "native FFT: paired z length %d", d.nz); }
}
#undef MI_ZQ_CALL

}  // namespace

// the table of plane twiddles behind the axis twiddles (init)
int NativeFft::fill_plane_twiddles(hipStream_t s, float2* dst) {
    tw_plane = dst;
    hipLaunchKernelGGL(k_plane_twiddles, dim3((unsigned)((dims.hx / 2 + 1 + 255) / 256)), dim3(256), 0, s, dst, dims.hx);
    return launch_check("k_plane_twiddles");
}

int NativeFft::y_pass(hipStream_t s, bool inverse, YRoute route, const float2* src_o, float2* dst_o, int xk0, int xkn) {
    const int Hx = dims.hx, L = dims.nz;
    if (xkn < 0) xkn = Hx / 2 + 1;
    const bool paired = route == YRoute::pair;
    MI_REQUIRE(paired || (xk0 == 0 && xkn == Hx / 2 + 1), "native FFT: only the paired y pass runs on a chunk of planes");
    const unsigned ycols = paired ? (unsigned)((size_t)xkn * (L / (dims.tc / 2))) : (unsigned)((size_t)L * Hx / dims.tc);
    NativeDims d = dims;
    d.xk0 = xk0;
    d.xkn = xkn;
    return y_launch(*this, s, inverse, route, ycols, d, src_o ? src_o : S.as<float2>(), dst_o ? dst_o : t_spec);
}

// forward y pass of a range of z planes (the z-chunked halo exchange: a chunk's columns are transformed as soon as its halo rows
// have landed, while the later chunks still travel)
int NativeFft::y_forward_planes(hipStream_t s, int z0, int nzc) {
    const int Hx = dims.hx, L = dims.nz, gran = y_z_granule();
    MI_REQUIRE(z0 >= 0 && nzc > 0 && z0 + nzc <= L && z0 % gran == 0 && (nzc % gran == 0 || z0 + nzc == L),
               "native FFT: plane range [%d, %d) must be cut at multiples of %d", z0, z0 + nzc, gran);
    const bool paired = dims.paired != 0;
    if (!paired) MI_REQUIRE(((size_t)nzc * Hx) % dims.tc == 0 && ((size_t)z0 * Hx) % dims.tc == 0, "native FFT: plane range does not hold whole y tiles");
    const unsigned ycols = paired ? (unsigned)((size_t)(Hx / 2 + 1) * ((nzc + gran - 1) / gran)) : (unsigned)((size_t)nzc * Hx / dims.tc);
    NativeDims d = dims;
    d.yz0 = z0;
    d.z_in_hi = std::min(dims.z_in_hi, z0 + nzc);   // (work-groups of the last, partial granule stop here)
    return y_launch(*this, s, false, y_route(dims), ycols, d, S.as<float2>(), t_spec);
}


int NativeFft::z_conv(hipStream_t s, bool conj_otf, const float2* src_o, float2* dst_o, int xk0, int xkn) {
    const int Hx = dims.hx, M = dims.ny, L = dims.nz;
    if (xkn < 0) xkn = Hx / 2 + 1;
    MI_REQUIRE(dims.paired || (xk0 == 0 && xkn == Hx / 2 + 1), "native FFT: only the paired z pass runs on a chunk of planes");
    const unsigned ztiles = (unsigned)((size_t)(Hx / 2 + 1) * (M / dims.tl));
    const size_t zl = lds_bytes(2 * dims.tl, L);
    NativeDims d = dims;
    d.xk0 = xk0;
    d.xkn = xkn;
    const float2* Tp = src_o ? src_o : t_spec;
    float2* Sp = dst_o ? dst_o : S.as<float2>();
    const bool adj_slot = conj_otf && have_adj;
    const float4* Gp = adj_slot ? G_adj.as<float4>() : G.as<float4>();
    const float2* twz = tw_z;
    const int cj = (conj_otf && !have_adj) ? 1 : 0;
    const RealOtf ro = real_otf ? real_otf_args(*this, adj_slot) : RealOtf{};
    switch (z_route(dims, sw, real_otf)) {
        case ZRoute::pair_pipe:
        case ZRoute::pair_pipe_real: {
            const int ntiles = xkn * (M / kPairLines);
            const bool fact = real_otf && otf_factored();  // (the A_r table in place of the z ramp's: z_pair_factored)
            const bool full = z_full_grid(d, sw);
            // (576-point lines have no LDS phase table: MI_ZQ_CASES.)  The kernel holds these bytes as a static array: no dynamic LDS
            const size_t lds = z_pair_lds(dims.lz2, dims.r3z, real_otf, fact);
            const int per_cu = std::max(1, std::min(2, (int)(kLdsOneWg / lds)));  // 8 waves of 128 registers each: two fit a CU
            const unsigned grid = (unsigned)std::min(ntiles, per_cu * n_cu);
            int* ctr_p = nullptr;
            if (z_tiles_dynamic(sw)) {
                if (!ctr.p) MI_TRY(ctr.alloc(256));
                ctr_p = ctr.as<int>() + 16 + 4 * (ctr_slot & 7);
                MI_HIP(hipMemsetAsync(ctr_p, 0, sizeof(int), s));
            }
            return z_pair_case(dims, [&](auto lg, auto r, auto nth, auto ph_lds) {
                constexpr int LG = lg(), R = r(), NTH = nth();
                constexpr bool PH = ph_lds();
                const auto go = [&](auto kernel, const char* name) {
                    return launch_lds(kernel, grid, NTH, 0, s, name, Tp, Sp, Gp, d, twz, cj, ntiles, ro, ctr_p, tw_plane);
                };
                // every form of the OTF with and without the plane bounds of a pruned grid (z_full_grid)
                if constexpr (z_pair_factored(LG, R)) {
                    if (fact)
                        return full ? go(k_z_pair_pipe<LG, R, true, NTH, kPairLines, PH, true, true, true>, "k_z_pair_pipe<factored OTF, full grid>")
                                    : go(k_z_pair_pipe<LG, R, true, NTH, kPairLines, PH, true, true, false>, "k_z_pair_pipe<factored OTF>");
                }
                if (real_otf)
                    return full ? go(k_z_pair_pipe<LG, R, true, NTH, kPairLines, PH, true, false, true>, "k_z_pair_pipe<real OTF, full grid>")
                                : go(k_z_pair_pipe<LG, R, true, NTH, kPairLines, PH, true, false, false>, "k_z_pair_pipe<real OTF>");
                return full ? go(k_z_pair_pipe<LG, R, false, NTH, kPairLines, PH, true, false, true>, "k_z_pair_pipe<full grid>")
                            : go(k_z_pair_pipe<LG, R, false, NTH, kPairLines, PH, true, false, false>, "k_z_pair_pipe");
            });
        }
        case ZRoute::conv_pipe:
        case ZRoute::conv_pipe_real: {
            const int ntiles = (int)ztiles;
            const unsigned grid = (unsigned)std::min(ntiles, n_cu);
            return z_case(dims, [&](auto lg, auto r) {
                constexpr int LG = lg(), R = r();
                if constexpr (z_pipe_even(R << LG)) {
                    if (real_otf)
                        return launch_lds(k_z_conv_pipe<LG, R, true>, grid, kThreadsXZ, zl, s, "k_z_conv_pipe<real OTF>", Tp, Sp, Gp, d, twz, cj, ntiles, ro);
                }
                return launch_lds(k_z_conv_pipe<LG, R, false>, grid, kThreadsXZ, zl, s, "k_z_conv_pipe", Tp, Sp, Gp, d, twz, cj, ntiles, ro);
            });
        }
        case ZRoute::conv:
            return z_case(dims, [&](auto lg, auto r) {
                return launch_lds(k_z_conv<lg(), r(), false>, ztiles, kThreadsXZ, zl, s, "k_z_conv", Tp, Sp, Gp, d, twz, cj, (float4*)nullptr, 0.0f);
            });
        case ZRoute::real_needs_pipe: break;
    }
    return fail(MI_ERR_INVALID, "native FFT: the real OTF form needs the pipelined z pass");
}

// Tries the real form of the OTF(s): `delta` = offset (x, y, z) of the PSF's centre sample from the grid origin.  Keeps the
// complex form when the PSF is not mirror-symmetric about that sample (the imaginary parts left after removing the phase ramp
// exceed the rounding noise of the transform) or when the z pass of this shape cannot take it.
int NativeFft::try_real_otf(hipStream_t s, const int delta[3]) {
    const int Hx = dims.hx, M = dims.ny, L = dims.nz;
    if (!real_otf_possible(dims, sw)) return MI_OK;
    // phase tables exp(-2 pi i (k delta mod F) / F) in double on the host: x by xk <= Hx/2 (F = 2 Hx), y by ky, z by kz
    const int nx = Hx / 2 + 1;
    const int nxp = ph_x_entries(Hx);
    MI_REQUIRE(M % 2 == 0, "native FFT: odd y length %d", M);  // (the z table must start on 16 bytes)
    std::vector<float2> h((size_t)nxp + M + L, make_float2(1.0f, 0.0f));
    const double two_pi = 6.283185307179586476925286766559;
    auto fill = [&](float2* dst, int n, long long F, int dl) {
        for (int k = 0; k < n; ++k) {
            const long long t = (((long long)k * dl) % F + F) % F;
            dst[k] = make_float2((float)std::cos(two_pi * (double)t / (double)F), (float)-std::sin(two_pi * (double)t / (double)F));
        }
    };
    fill(h.data(), nx, 2LL * Hx, delta[0]);
    fill(h.data() + nxp, M, M, delta[1]);
    fill(h.data() + nxp + M, L, L, delta[2]);
    MI_TRY(ph.alloc(sizeof(float2) * h.size()));
    MI_HIP(hipMemcpyAsync(ph.p, h.data(), sizeof(float2) * h.size(), hipMemcpyHostToDevice, s));
    const RealOtf ro = real_otf_args(*this, false);  // (k_g_to_real reads the phase tables only)
    const size_t total = (size_t)nx * M * L;
    DevBuf st;
    MI_TRY(st.alloc(4 * sizeof(unsigned)));
    MI_HIP(hipMemsetAsync(st.p, 0, 4 * sizeof(unsigned), s));
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    for (int slot = 0; slot < (have_adj ? 2 : 1); ++slot) {
        DevBuf& dst = slot ? Gr_adj : Gr;
        MI_TRY(dst.alloc(sizeof(float2) * total));
        hipLaunchKernelGGL(k_g_to_real, dim3((unsigned)blocks), dim3(256), 0, s, (slot ? G_adj : G).as<float4>(), dst.as<float2>(), dims, ro,
                           total, st.as<unsigned>() + 2 * slot);
        MI_TRY(launch_check("k_g_to_real"));
    }
    float hs[4] = {0, 0, 0, 0};
    MI_HIP(hipMemcpyAsync(hs, st.p, sizeof(hs), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    bool ok = hs[0] <= 4e-6f * hs[1] && (!have_adj || hs[2] <= 4e-6f * hs[3]);
    if (ok) {
        real_otf = true;
        G.release();
        G_adj.release();
    } else {
        Gr.release();
        Gr_adj.release();
        ph.release();
    }
    return MI_OK;
}

// Tries the factored form of the real OTF(s) (otf_factor.h) where the z route is the paired pipelined kernel of a length that takes it
// (z_pair_factored; the plain-layout kernels keep the stored form).  Per slot: factor the PSF on the host, build the tables, and compare
// sum_r A_r Bh_r with the Gr that try_real_otf stored, entry by entry -- adopted when they differ by at most 4e-6 of the largest entry, the
// criterion of the real form itself (the difference is the float32 rounding of the transform that built Gr).  Adopted: Gr is released;
// otherwise the tables are, and the plan goes on with the stored form.
int NativeFft::try_factored_otf(hipStream_t s, const float* psf, const float* psf_adj, const int k[3], const int delta[3], float scale) {
    if (!real_otf || sw.stored_otf || z_route(dims, sw, true) != ZRoute::pair_pipe_real || !z_pair_factored(dims.lz2, dims.r3z)) return MI_OK;
    MI_REQUIRE(have_adj == (psf_adj != nullptr), "native FFT: the factored OTF needs the PSF of every slot");
    const int Hx = dims.hx, M = dims.ny, L = dims.nz, nx = Hx / 2 + 1, slots = have_adj ? 2 : 1;
    const size_t nk = (size_t)k[0] * k[1] * k[2], lines = (size_t)nx * M, total = lines * L;
    std::vector<float> hpsf(nk);
    int ranks[2] = {0, 0};
    DevBuf st, da, dcs;
    MI_TRY(st.alloc(4 * sizeof(unsigned)));
    MI_HIP(hipMemsetAsync(st.p, 0, 4 * sizeof(unsigned), s));
    MI_TRY(da.alloc(sizeof(double) * 4 * (size_t)L));
    MI_TRY(dcs.alloc(sizeof(double) * 2 * (size_t)(2 * nx) * 4 * k[1]));
    std::vector<double> ha(4 * (size_t)L), hcs(2 * (size_t)(2 * nx) * 4 * k[1]), C(k[1]), S(k[1]);
    bool ok = true;
    for (int slot = 0; slot < slots && ok; ++slot) {
        MI_HIP(hipMemcpyAsync(hpsf.data(), slot ? psf_adj : psf, sizeof(float) * nk, hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        const OtfFactors f = otf_factor(hpsf.data(), k[0], k[1], k[2]);
        ranks[slot] = f.rank;
        if (f.rank == 0) { ok = false; break; }
        for (int kz = 0; kz < L; ++kz)
            for (int r = 0; r < kOtfMaxRank; ++r) ha[4 * (size_t)kz + r] = r < f.rank ? otf_factor_A(f, r, kz, L) : 0.0;
        for (int side = 0; side < 2; ++side)
            for (int xk = 0; xk < nx; ++xk)
                for (int r = 0; r < kOtfMaxRank; ++r) {
                    otf_factor_B_x(f, r, xk + side * Hx, 2 * Hx, C.data(), S.data());
                    double* dst = &hcs[2 * (((size_t)(xk + side * nx) * 4 + r) * k[1])];
                    // (side B: the stored form removes the ramp of xk, not of xk + Hx -- the two differ by exp(-pi i delta_x), a sign)
                    const double sc = (double)scale * (side && (delta[0] & 1) ? -1.0 : 1.0);
                    for (int y = 0; y < k[1]; ++y) { dst[2 * y] = C[y] * sc; dst[2 * y + 1] = S[y] * sc; }
                }
        DevBuf& tab = slot ? Gf_adj : Gf;
        MI_TRY(tab.alloc(sizeof(float4) * ((size_t)L + 2 * lines)));
        MI_HIP(hipMemcpyAsync(da.p, ha.data(), sizeof(double) * ha.size(), hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(dcs.p, hcs.data(), sizeof(double) * hcs.size(), hipMemcpyHostToDevice, s));
        float4* fa = tab.as<float4>();
        float4* fb = fa + L;
        hipLaunchKernelGGL(k_fact_a_table, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, s, da.as<double>(), fa, dims);
        MI_TRY(launch_check("k_fact_a_table"));
        hipLaunchKernelGGL(k_fact_b_table, dim3((unsigned)((2 * lines + 255) / 256)), dim3(256), 0, s, dcs.as<double2>(), fb, dims, k[1], 2 * lines);
        MI_TRY(launch_check("k_fact_b_table"));
        const size_t blocks = std::min<size_t>((total + 255) / 256, 256 * 16);
        hipLaunchKernelGGL(k_fact_compare, dim3((unsigned)blocks), dim3(256), 0, s, (slot ? Gr_adj : Gr).as<float2>(), (const float4*)fa, (const float4*)fb,
                           dims, total, st.as<unsigned>() + 2 * slot);
        MI_TRY(launch_check("k_fact_compare"));
        MI_HIP(hipStreamSynchronize(s));  // (the host tables are reused by the next slot)
    }
    float hs[4] = {0, 0, 0, 0};
    MI_HIP(hipMemcpyAsync(hs, st.p, sizeof(hs), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    ok = ok && hs[0] <= 4e-6f * hs[1] && (!have_adj || hs[2] <= 4e-6f * hs[3]);
    if (sw.place_log)
        fprintf(stderr, "native FFT: factored OTF ranks %d / %d, max|Gr - sum A B| %.3e of %.3e (adjoint %.3e of %.3e): %s\n", ranks[0], ranks[1],
                (double)hs[0], (double)hs[1], (double)hs[2], (double)hs[3], ok ? "adopted" : "stored form kept");
    if (ok) {
        otf_rank = ranks[0];
        otf_rank_adj = ranks[1];
        Gr.release();
        Gr_adj.release();
    } else {
        Gf.release();
        Gf_adj.release();
    }
    return MI_OK;
}

// OTF of the placed kernel volume `placed` (shape F, real; may be the T buffer itself): forward x, y and z transforms, then
// the untangled spectrum is stored in the z pass' pair layout, times `scale`.
int NativeFft::build_otf(hipStream_t s, const float* placed, bool adjoint_slot, float scale) {
    MI_REQUIRE(!adjoint_slot || have_adj, "native FFT: no adjoint OTF slot");
    return spectrum(s, placed, adjoint_slot ? G_adj.as<float4>() : G.as<float4>(), scale);
}

// untangled half spectrum of a real F volume in the OTF layout (pairs (X[k], X[mirror k]) per point-wise item of the z pass)
int NativeFft::spectrum(hipStream_t s, const float* vol, float4* Gp, float scale) {
    MI_REQUIRE(!pw.on, "native FFT: spectra are taken on the unpadded grid (before the pad window is set)");
    MI_TRY(x_forward(s, vol));
    MI_TRY(y_pass(s, false, YRoute::pass));  // (k_z_conv<build> reads the plain [px][z][py] layout)
    const unsigned ztiles = (unsigned)((size_t)(dims.hx / 2 + 1) * (dims.ny / dims.tl));
    return z_case(dims, [&](auto lg, auto r) {
        return launch_lds(k_z_conv<lg(), r(), true>, ztiles, kThreadsXZ, lds_bytes(2 * dims.tl, dims.nz), s, "k_z_conv<build>", (const float2*)t_spec,
                          S.as<float2>(), (const float4*)nullptr, dims, tw_z, 0, Gp, scale);
    });
}

}  // namespace mi
