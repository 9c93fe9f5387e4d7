// The x passes of the native FFT pipeline: the unpipelined kernels (P1, P5, P5 + P1 with every stage in LDS), the persistent pipelined
// kernel (k_x_fused_pipe: fused, forward only, inverse only), the halo rows of S, and the x launchers.
// One unit for all of them, and the kernels are named in the order x_pipelined (forward only, fused, inverse only), x_forward,
// x_inverse: the compiler inlines the always-inline building blocks in the order the unit first emits them, so what it makes of a
// kernel depends on the kernels named before it (profiles/NOTES.md, "FFT source split").
#include "fft_native_dev.h"

namespace mi {
namespace {

// ---------------------------------------------------------------------------------------------- P1: x forward
// grid: (Y / TY) * Z tiles; tile = TY consecutive rows of one z-plane
template <int LHX2, int R3>
__global__ __launch_bounds__(kThreadsXZ, kWavesXZ) void k_x_forward(const float* __restrict__ in, float2* __restrict__ S, NativeDims d,
                                                         const float2* __restrict__ tw, PadWindow pw) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];
    constexpr int Hx = R3 << LHX2, NW = kThreadsXZ / 64;
    const int TY = d.ty, hp = TY / 2, pitch = row_pitch(Hx);
    const int ytiles = d.ny / TY;
    const int z = blockIdx.x / ytiles, y0 = (blockIdx.x % ytiles) * TY;
    const int rowq = d.xrow / 2;
    float4* dst = reinterpret_cast<float4*>(S + ((size_t)z * Hx) * d.xrow + y0);
    if (pw.on) {
        // staged load with the boundary rule; a tile that lies entirely in the zero padding transforms to zeros
        const int sz = pad_src(pw, 2, z);
        bool live = false;
        for (int r = 0; r < TY; ++r) live = live || pad_src(pw, 1, y0 + r) >= 0;
        if (sz < 0 || !live) {
            if (z >= d.z_in_hi) return;  // the y pass does not read these planes
            for (int i = threadIdx.x; i < hp * Hx; i += kThreadsXZ) {
                const int px = i / hp, rp = i - px * hp;
                dst[(size_t)px * rowq + rp] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            return;
        }
        for (int i = threadIdx.x; i < TY * Hx; i += kThreadsXZ) {
            const int r = i / Hx, q = i - r * Hx;
            const int sy = pad_src(pw, 1, y0 + r);
            float2 v = make_float2(0.0f, 0.0f);
            if (sy >= 0) {
                const float* row = in + ((size_t)sz * pw.n[1] + sy) * (size_t)pw.n[0];
                const int s0 = pad_src(pw, 0, 2 * q), s1 = pad_src(pw, 0, 2 * q + 1);
                if (s0 >= 0) v.x = row[s0];
                if (s1 >= 0) v.y = row[s1];
            }
            tile[cell(r, pitch, hp, q)] = v;
        }
    } else {
        const float4* src = reinterpret_cast<const float4*>(in + ((size_t)z * d.ny + y0) * (size_t)(2 * Hx));
        const int quads = Hx / 2;  // float4 = 2 complex
        for (int i = threadIdx.x; i < TY * quads; i += kThreadsXZ) {
            const int r = i / quads, q = i - r * quads;
            const float4 v = src[(size_t)r * quads + q];
            const int c0 = cell(r, pitch, hp, 2 * q);  // elements 2q, 2q + 1 are slot neighbours (same bits 4..7)
            tile[c0] = make_float2(v.x, v.y);
            tile[c0 ^ 1] = make_float2(v.z, v.w);
        }
    }
    using TW = TwLds<LHX2, R3>;
    float2* twl = tile + TY * pitch;
    TW::template fill<kThreadsXZ>(twl, tw);
    lds_barrier();
    const bool priv = (TY % NW) == 0;
    if constexpr (R3 > 1) {
        radix3_stage<R3, false, kThreadsXZ>(tile, TY, pitch, hp, priv, 1 << LHX2, twl + TW::r3);
        stage_sync(priv);
    }
    lds_fft<LHX2, false, kThreadsXZ, R3>(tile, TY * R3, pitch, hp, priv, twl);
    if (priv) lds_barrier();
    // transposed store: S[z][px][y0 + r], r fastest; one float4 = rows (2 rp, 2 rp + 1) of one px
#pragma unroll MI_FFT_UNROLL
    for (int i = threadIdx.x; i < hp * Hx; i += kThreadsXZ) {
        const int px = i / hp, rp = i - px * hp;
        const int c0 = cell(2 * rp, pitch, hp, x_pos2work(px, d));
        const float2 a = tile[c0], b = tile[c0 + pitch];
        dst[(size_t)px * rowq + rp] = make_float4(a.x, a.y, b.x, b.y);
    }
}

// ---------------------------------------------------------------------------------------------- P5: x inverse + epilogue
// FUSE: the epilogue result stays in LDS and is transformed forward again into S_next (the P1 of the NEXT
// convolution): the ratio never touches HBM, and bl is read once and written once per iteration.
template <int LHX2, int R3, bool FUSE>
__global__ __launch_bounds__(kThreadsXZ, kWavesXZ) void k_x_inverse(const float2* __restrict__ T, float* __restrict__ out, ConvEpilogue e, NativeDims d,
                                                         const float2* __restrict__ tw, float2* __restrict__ S_next, int EPI, PadWindow pw) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];
    constexpr int Hx = R3 << LHX2, NW = kThreadsXZ / 64;
    const int TY = d.ty, hp = TY / 2, pitch = row_pitch(Hx);
    const int ytiles = d.ny / TY;
    const int z = blockIdx.x / ytiles, y0 = (blockIdx.x % ytiles) * TY;
    const float4* src = reinterpret_cast<const float4*>(T + ((size_t)z * Hx) * d.xrow + y0);
    const int rowq = d.xrow / 2;
    int oz = z;
    if (pw.on) {
        // rows outside the cropped result are never stored: a tile without any is skipped (fused: its part of the next
        // convolution's input is the zero padding)
        oz = pad_dst(pw, 2, z);
        bool live = false;
        for (int r = 0; r < TY; ++r) live = live || pad_dst(pw, 1, y0 + r) >= 0;
        if (oz < 0 || !live) {
            if (FUSE && z < d.z_in_hi) {  // planes beyond are never read by the next y pass
                float4* sdst = reinterpret_cast<float4*>(S_next + ((size_t)z * Hx) * d.xrow + y0);
                for (int i = threadIdx.x; i < hp * Hx; i += kThreadsXZ) {
                    const int px = i / hp, rp = i - px * hp;
                    sdst[(size_t)px * rowq + rp] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
            return;
        }
    }
#pragma unroll MI_FFT_UNROLL
    for (int i = threadIdx.x; i < hp * Hx; i += kThreadsXZ) {
        const int px = i / hp, rp = i - px * hp;
        const float4 v = src[(size_t)px * rowq + rp];
        const int c0 = cell(2 * rp, pitch, hp, x_pos2work(px, d));
        tile[c0] = make_float2(v.x, v.y);
        tile[c0 + pitch] = make_float2(v.z, v.w);
    }
    using TW = TwLds<LHX2, R3>;
    float2* twl = tile + TY * pitch;
    TW::template fill<kThreadsXZ>(twl, tw);
    lds_barrier();
    // rows dealt to the waves: the inverse transform, the epilogue and the forward transform of a row all belong to its owner
    const bool priv = (TY % NW) == 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (!(d.dbg & 8)) {
        lds_fft<LHX2, true, kThreadsXZ, R3>(tile, TY * R3, pitch, hp, priv, twl);
        if constexpr (R3 > 1) {
            radix3_stage<R3, true, kThreadsXZ>(tile, TY, pitch, hp, priv, 1 << LHX2, twl + TW::r3);
            stage_sync(priv);
        }
    }
    if (pw.on) {
        // crop + epilogue on the caller's (unpadded) volume; fused: the zero padding of the next input is re-created
        const float l = e.lambda, m = 1.0f - e.lambda;
        const int n_items = priv ? (TY / NW) * Hx : TY * Hx;
        for (int i = priv ? lane : threadIdx.x; i < n_items; i += priv ? 64 : kThreadsXZ) {
            const int rl = i / Hx, q = i - rl * Hx;
            const int r = priv ? rl * NW + wave : rl;
            const int oy = pad_dst(pw, 1, y0 + r);
            float2* cl = tile + cell(r, pitch, hp, q);
            const float2 c = *cl;
            float2 o = make_float2(0.0f, 0.0f);
            if (oy >= 0) {
                const size_t rbase = ((size_t)oz * pw.n[1] + oy) * (size_t)pw.n[0];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int ox = pad_dst(pw, 0, 2 * q + h);
                    if (ox < 0) continue;
                    const float cv = h ? c.y : c.x;
                    const size_t gi = rbase + ox;
                    float v;
                    if (EPI == EPI_NONE) v = cv;
                    else if (EPI == EPI_RATIO) v = e.a[gi] * rcp_eps(cv);
                    else if (EPI == EPI_UPDATE) v = fabsf(e.a[gi] * cv);
                    else v = fabsf(e.a[gi] * cv * m + e.b[gi] * l);
                    if (!FUSE || out != nullptr) out[gi] = v;
                    if (h) o.y = v; else o.x = v;
                }
            }
            if (FUSE) *cl = o;
        }
    } else {
        const size_t row0 = ((size_t)z * d.ny + y0) * (size_t)(2 * Hx);
        const int quads = Hx / 2;
        float4* dst = reinterpret_cast<float4*>(out + row0);
        const float4* a4 = reinterpret_cast<const float4*>(e.a + row0);
        const float4* b4 = reinterpret_cast<const float4*>(e.b + row0);
        const int n_items = priv ? (TY / NW) * quads : TY * quads;
        for (int i = priv ? lane : threadIdx.x; i < n_items; i += priv ? 64 : kThreadsXZ) {
            const int rl = i / quads, q = i - rl * quads;
            const int r = priv ? rl * NW + wave : rl;
            const int c0i = cell(r, pitch, hp, 2 * q);
            const float2 c0 = tile[c0i], c1 = tile[c0i ^ 1];
            float4 c = make_float4(c0.x, c0.y, c1.x, c1.y), o;
            const size_t gi = (size_t)r * quads + q;
            if (EPI == EPI_NONE) {
                o = c;
            } else {
                const float4 av = a4[gi];
                if (EPI == EPI_RATIO) {
                    o = make_float4(av.x * rcp_eps(c.x), av.y * rcp_eps(c.y), av.z * rcp_eps(c.z), av.w * rcp_eps(c.w));
                } else if (EPI == EPI_UPDATE) {
                    o = make_float4(fabsf(av.x * c.x), fabsf(av.y * c.y), fabsf(av.z * c.z), fabsf(av.w * c.w));
                } else {
                    const float4 bv = b4[gi];
                    const float l = e.lambda, m = 1.0f - e.lambda;
                    o = make_float4(fabsf(av.x * c.x * m + bv.x * l), fabsf(av.y * c.y * m + bv.y * l), fabsf(av.z * c.z * m + bv.z * l),
                                    fabsf(av.w * c.w * m + bv.w * l));
                }
            }
            if (!FUSE || out != nullptr) dst[gi] = o;
            if (FUSE) {
                tile[c0i] = make_float2(o.x, o.y);
                tile[c0i ^ 1] = make_float2(o.z, o.w);
            }
        }
    }
    if (FUSE) {
        stage_sync(priv);
        if (!(d.dbg & 16)) {
            if constexpr (R3 > 1) {
                radix3_stage<R3, false, kThreadsXZ>(tile, TY, pitch, hp, priv, 1 << LHX2, twl + TW::r3);
                stage_sync(priv);
            }
            lds_fft<LHX2, false, kThreadsXZ, R3>(tile, TY * R3, pitch, hp, priv, twl);
        }
        if (priv) lds_barrier();
        float4* sdst = reinterpret_cast<float4*>(S_next + ((size_t)z * Hx) * d.xrow + y0);
#pragma unroll MI_FFT_UNROLL
        for (int i = threadIdx.x; i < hp * Hx; i += kThreadsXZ) {
            const int px = i / hp, rp = i - px * hp;
            const int c0 = cell(2 * rp, pitch, hp, x_pos2work(px, d));
            const float2 a = tile[c0], b = tile[c0 + pitch];
            sdst[(size_t)px * rowq + rp] = make_float4(a.x, a.y, b.x, b.y);
        }
    }
}


// ---------------------------------------------------------------------------------------------- P5 + P1, pipelined
// The fused x pass as a persistent kernel: one work-group per CU walks over tiles and keeps HBM busy during the FFT phases --
// the epilogue operand of the current tile is requested before the inverse transform and the next tile's spectrum before the
// forward transform, both into registers (8 float4 each for a 16 x 1024 tile); stores drain behind.
// Unpadded volumes only (the padded mode keeps k_x_inverse).
// MODE 0: the fused pass.  MODE 1: forward only -- the rows of the real volume `e.a` are transformed into S_next (k_x_forward as a
// persistent kernel: the next tile's rows travel during the transform and the store of the current one).  MODE 2: inverse only --
// T -> epilogue (none / ratio / update) -> out, nothing is transformed forward (k_x_inverse without the regularised epilogues).
template <int LHX2, int R3, int MODE = 0>
__global__ __launch_bounds__(kThreadsXZ, kWavesXZ) void k_x_fused_pipe(const float2* __restrict__ T, float* __restrict__ out, ConvEpilogue e, NativeDims d,
                                                            const float2* __restrict__ tw, float2* __restrict__ S_next, int EPI, int ntiles,
                                                            TileSelect sel, PadWindow pw, int* __restrict__ tile_ctr) {
    extern __shared__ __attribute__((aligned(16))) float2 tile[];
    // Tile hand-out.  tile_ctr == nullptr: work-group b takes tiles b, b + grid, b + 2 grid, ...  Otherwise every tile comes from a
    // device counter (zeroed by the host; a work-group takes two numbers when it starts, then one atomicAdd per tile): a work-group
    // whose CU was busy with something else when the launch began -- a collective's kernels during a halo exchange -- then simply
    // takes fewer tiles, or none, instead of leaving a fixed share as the tail of the pass.  A number is fetched a whole tile
    // ahead (requested at the top of a tile, published through LDS behind the tile's last barrier), so its latency never sits on
    // the tile's chain; only the first fetch of a work-group is waited for.
    __shared__ int s_next_tile;
    constexpr int Hx = R3 << LHX2, NW = kThreadsXZ / 64;
    constexpr int TY = x_tile_rows(Hx), hp = TY / 2, quads = Hx / 2;
    constexpr int NQ = hp * Hx;  // float4 per tile, in the transposed (T / S) and in the row (bl) view alike
    constexpr int NPF = (NQ + kThreadsXZ - 1) / kThreadsXZ;
    constexpr int pitch = row_pitch(Hx);
    constexpr int P = kThreadsXZ / hp;  // item j of a lane in the transposed view: column px0 + j * P, row pair rp
    // REG (the rotated x order, NativeDims::xrot): column px0 + j * P holds working index 8 px0 + j, so the eight items of a lane are
    // the points of one bottom radix-8 butterfly (stages 0-2: compile-time twiddles, no table) of each of its two rows.  That
    // super-stage -- the first of the inverse transform, the last of the forward one -- runs on the registers the loads arrive in
    // and the stores leave from: the fill writes its results to the slots 8 px0 .. 8 px0 + 7 and the inverse chain starts at stage
    // 3, the forward chain stops there and the drain finishes the transform (one LDS round trip fewer per direction; the z pass
    // does the same with its top super-stage, k_z_pair_pipe).  The arithmetic is that of super_stage<.., 3, 0, ..>.
    constexpr bool REG = x_rotated(LHX2, R3);
    static_assert(!REG || (NPF == 8 && P * 8 == Hx && NQ % kThreadsXZ == 0), "rotated x order: eight items per lane, Hx / 8 apart");
    constexpr int hpm = REG ? (hp | kRowsRot) : hp;  // row masks for the eight-neighbour accesses of the fill and the drain (rmask)
    constexpr int REG_R = REG ? 3 : 0;
    // rows dealt to the waves: the inverse transform, the epilogue and the forward transform of a row all belong to its owner
    // and run without work-group barriers; only the transposed fill and drain are tile-wide
    constexpr bool PRIV = (TY % NW == 0) && (NQ % kThreadsXZ == 0) && (quads % 64 == 0);
    const int ytiles = d.ny / TY, rowq = d.xrow / 2;
    // Lane constants of the two views (tile-invariant, a handful of registers).  The swizzle is XOR-linear, so the slot of
    // item j is the slot of item 0 XOR a compile-time constant: px0 < P and j * P (2 * lane < 128 and the multiples of 128 of
    // the row view) occupy disjoint bits.
    // (They are recomputed at the start of every phase from a laundered thread index: kept live across the FFT phases they
    // push the kernel over its 128 VGPRs, and every spilled dword costs ~0.5 GB of scratch traffic per launch.)
    struct TView { int row, slot; size_t off; };   // transposed view: item j = column px0 + j * P, row pair rp
    auto t_view = [&]() {
        const int tid = launder(threadIdx.x);
        const int px0 = tid / hp, rp = tid - px0 * hp;
        return TView{(2 * rp) * pitch, phys(REG ? 8 * px0 : px0) ^ rmask(2 * rp, hpm), (size_t)px0 * rowq + rp};
    };
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // row view, item j: PRIV: float4 u = lane + 64 j of the wave's rows -> row rl * NW + wave, quad q; else float4 tid + j * NT
    struct RView { int tid, lane, slot; };
    auto r_view = [&]() {
        const int tid = launder(threadIdx.x);
        return RView{tid, tid & 63, phys(2 * (tid & 63))};
    };
    auto r_item = [&](const RView& rv, int j, int& i, int& c, int& r, int& q) {
        if (PRIV) {
            const int rl = (64 * j) / quads, q0 = (64 * j) % quads;  // compile-time after unrolling
            r = rl * NW + wave;                                        // scalar
            q = q0 + rv.lane;
            i = r * quads + q;
            c = r * pitch + (rv.slot ^ swz_c(2 * q0) ^ rmask(r, hpm));
        } else {
            i = rv.tid + j * kThreadsXZ;
            r = i / quads;
            q = i - r * quads;
            c = cell(r, pitch, hpm, 2 * q);
        }
    };
    // Padded grids (zero rule, data at the origin, nx a multiple of 4): row r of a tile is row y0 + r of the caller's volume when
    // that is < ny, its quads q < nx / 4 hold data; everything else is padding (epilogue result 0).  Only the live tiles are
    // enumerated (mode 3); the tiles of live planes that lie entirely in the y padding are zero-filled first.
    const int data_quads = pw.on ? pw.n[0] / 4 : quads;
    if (pw.on && MODE != 2) {  // (the inverse-only mode writes no spectrum)
        const int nty = sel.n0, nzl = pw.n[2];
        for (int u = blockIdx.x; u < d.z_in_hi * ytiles; u += gridDim.x) {  // every tile the next y pass reads ...
            const int z = u / ytiles, ty = u - z * ytiles;
            if (z < nzl && ty < nty) continue;                               // ... that the loop below does not produce
            float4* sdst = reinterpret_cast<float4*>(S_next + ((size_t)z * Hx) * d.xrow + ty * TY);
            for (int i = threadIdx.x; i < hp * Hx; i += kThreadsXZ) {
                const int px = i / hp, rp = i - px * hp;
                sdst[(size_t)px * rowq + rp] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    }
    float4 pre[NPF];
    // tile number -> (z, first row): all y tiles of a plane, or only / all but the tiles of two row ranges (the slab driver
    // sends the edge rows off while the rest of the pass runs)
    auto tile_zy = [&](int t, int& z, int& y0) {
        const int per = sel.mode == 0 ? ytiles : (sel.mode == 1 ? sel.n0 + sel.n1 : sel.mode == 3 ? sel.n0 : ytiles - sel.n0 - sel.n1);
        const int zl = t / per;
        z = sel.z0 + zl;
        int ty = t - zl * per;
        if (sel.mode == 1) {
            ty = ty < sel.n0 ? sel.lo0 + ty : sel.lo1 + (ty - sel.n0);
        } else if (sel.mode == 2) {
            if (ty >= sel.lo0) ty += sel.n0;
            if (ty >= sel.lo1) ty += sel.n1;
        }
        y0 = ty * TY;
    };
    auto tile_base = [&](int t) { int z, y0; tile_zy(t, z, y0); return ((size_t)z * Hx) * d.xrow + y0; };
    auto load_T = [&](int t) {
        const TView tv = t_view();
        const float4* src = reinterpret_cast<const float4*>(T + tile_base(t)) + tv.off;
#pragma unroll
        for (int j = 0; j < NPF; ++j)
            if (NQ % kThreadsXZ == 0 || (int)threadIdx.x + j * kThreadsXZ < NQ) pre[j] = src[(size_t)(j * P) * rowq];
    };
    using TW = TwLds<LHX2, R3>;
    float2* twl = tile + TY * pitch;
    TW::template fill<kThreadsXZ>(twl, tw);
    // MODE 1: the rows of a tile in the row view (float4 j of a lane as in r_item), requested one tile ahead into `pre`
    auto load_rows = [&](int t) {
        int z, y0;
        tile_zy(t, z, y0);
        // (padded grids: rows and quads beyond the caller's volume are zero, as in the epilogue below)
        const size_t row0 = pw.on ? ((size_t)z * pw.n[1] + y0) * (size_t)data_quads : ((size_t)z * d.ny + y0) * (size_t)quads;
        const int rows_live = pw.on ? pw.n[1] - y0 : TY;
        const float4* src4 = reinterpret_cast<const float4*>(e.a);
        const RView rv = r_view();
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            int i, c, r, q;
            r_item(rv, j, i, c, r, q);
            if (NQ % kThreadsXZ == 0 || i < NQ) {
                const bool live = r < rows_live && q < data_quads;
                pre[j] = live ? src4[pw.on ? row0 + (size_t)r * data_quads + q : row0 + i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    };
    const bool dyn = tile_ctr != nullptr;
    int t = blockIdx.x, tn = t + (int)gridDim.x;
    if (dyn) {
        if (threadIdx.x == 0) s_next_tile = atomicAdd(tile_ctr, 2);
        lds_barrier();
        t = __builtin_amdgcn_readfirstlane(s_next_tile);
        tn = t + 1;
        lds_barrier();  // (everybody has read the slot before the first tile's owner of lane 0 overwrites it)
    }
    if (t < ntiles) {
        if constexpr (MODE == 1) load_rows(t);
        else load_T(t);
    }
    if constexpr (MODE == 1) lds_barrier();  // the tables (the other modes meet a barrier before their first transform)
    for (; t < ntiles;) {
        int fetched = 0;
        if (dyn && threadIdx.x == 0) fetched = atomicAdd(tile_ctr, 1);  // the tile after the next one
        // behind the last barrier of a tile: t <- tn, tn <- the fetched number (or the static successor)
        auto advance = [&]() {
            t = tn;
            tn = dyn ? __builtin_amdgcn_readfirstlane(s_next_tile) : tn + (int)gridDim.x;
        };
        if constexpr (MODE != 1) {
            const TView tv = t_view();
            if constexpr (REG) {
                float2 v[8], u[8];  // rows 2 rp and 2 rp + 1
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v[j] = make_float2(pre[j].x, pre[j].y);
                    u[j] = make_float2(pre[j].z, pre[j].w);
                }
                butterflies<3, 0, true>(v, nullptr, 0);
                butterflies<3, 0, true>(u, nullptr, 0);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c0 = tv.row + (tv.slot ^ j);
                    tile[c0] = v[j];
                    tile[c0 + pitch] = u[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < NPF; ++j) {
                    if (NQ % kThreadsXZ == 0 || (int)threadIdx.x + j * kThreadsXZ < NQ) {
                        const int c0 = tv.row + (tv.slot ^ swz_c(j * P));
                        tile[c0] = make_float2(pre[j].x, pre[j].y);
                        tile[c0 + pitch] = make_float2(pre[j].z, pre[j].w);
                    }
                }
            }
        }
        // rows of this tile in the real volume: contiguous TY * 2 Hx floats
        int z, y0;
        tile_zy(t, z, y0);
        // float4 index of (row r, quad q) of this tile in the caller's volume: rows are 2 Hx floats apart, or nx on a padded grid
        const size_t row0 = pw.on ? ((size_t)z * pw.n[1] + y0) * (size_t)data_quads : ((size_t)z * d.ny + y0) * (size_t)quads;
        const int rows_live = pw.on ? pw.n[1] - y0 : TY;  // rows of the tile that exist in the caller's volume
        auto g_index = [&](int i, int r, int q) { return pw.on ? row0 + (size_t)r * data_quads + q : row0 + i; };
        const float4* a4 = reinterpret_cast<const float4*>(e.a);
        float4 av[NPF];
        auto load_a = [&]() {
            {
                const RView rv = r_view();
    #pragma unroll
                for (int j = 0; j < NPF; ++j) {
                    int i, c, r, q;
                    r_item(rv, j, i, c, r, q);
                    if (NQ % kThreadsXZ == 0 || i < NQ) {
                        const bool live = r < rows_live && q < data_quads && !(MODE == 2 && EPI == EPI_NONE);  // (no operand then)
                        av[j] = live ? a4[g_index(i, r, q)] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    }
                }
            }
        };
        if constexpr (MODE == 1) {
#pragma unroll
            for (int j = 0; j < NPF; ++j) av[j] = pre[j];
            if (tn < ntiles) load_rows(tn);
        } else {
        // (the inverse-only launch with a sixteen-point top stage: the operand is requested in front of that stage -- held across
        // the whole transform it does not fit the 128 registers beside the stage's sixteen points)
        constexpr int TOP_LO = seg_below(LHX2, LHX2);
        constexpr bool LATE_A = MODE == 2 && R3 == 1 && LHX2 - TOP_LO == 4;
        if (R3 != 9 && !LATE_A) load_a();  // (radix-9 rows: requested behind the 9-point stage, which needs the registers)
        lds_barrier();
        if constexpr (LATE_A) {
            lds_fft<LHX2, true, kThreadsXZ, R3, REG_R, TOP_LO>(tile, TY * R3, pitch, hpm, PRIV, twl);
            load_a();
            lds_fft<LHX2, true, kThreadsXZ, R3, TOP_LO, LHX2>(tile, TY * R3, pitch, hpm, PRIV, twl);
        } else {
            lds_fft<LHX2, true, kThreadsXZ, R3, REG_R>(tile, TY * R3, pitch, hpm, PRIV, twl);
        }
        if constexpr (R3 > 1) {
            radix3_stage<R3, true, kThreadsXZ>(tile, TY, pitch, hp, PRIV, 1 << LHX2, twl + TW::r3);
            stage_sync(PRIV);
        }
        if (R3 == 9) load_a();
        }
        float4* dst = reinterpret_cast<float4*>(out);
        const RView rv = r_view();
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            int i, s0, r, q;
            r_item(rv, j, i, s0, r, q);  // elements 2q and 2q + 1 are slot neighbours
            if (NQ % kThreadsXZ == 0 || i < NQ) {
                const float4 a = av[j];
                if constexpr (MODE == 1) {  // the volume's rows, as they are
                    tile[s0] = make_float2(a.x, a.y);
                    tile[s0 ^ 1] = make_float2(a.z, a.w);
                    continue;
                }
                const float2 c0 = tile[s0], c1 = tile[s0 ^ 1];
                const bool live = r < rows_live && q < data_quads;
                float4 o;
                if (MODE == 2 && EPI == EPI_NONE)
                    o = make_float4(c0.x, c0.y, c1.x, c1.y);
                else if (EPI == EPI_RATIO)
                    o = make_float4(a.x * rcp_eps(c0.x), a.y * rcp_eps(c0.y), a.z * rcp_eps(c1.x), a.w * rcp_eps(c1.y));
                else
                    o = make_float4(fabsf(a.x * c0.x), fabsf(a.y * c0.y), fabsf(a.z * c1.x), fabsf(a.w * c1.y));
                if (!live) o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // the zero padding of the next convolution's input
                if (out != nullptr && live) dst[g_index(i, r, q)] = o;
                if constexpr (MODE != 2) {
                    tile[s0] = make_float2(o.x, o.y);
                    tile[s0 ^ 1] = make_float2(o.z, o.w);
                }
            }
        }
        // (radix-9 rows: the 9-point stage needs the registers, so the next tile is requested behind it)
        if constexpr (MODE == 2) {  // nothing goes forward: the tile is free once everybody has read its rows
            if (tn < ntiles) load_T(tn);
            if (dyn && threadIdx.x == 0) s_next_tile = fetched;
            lds_barrier();
            advance();
            continue;
        }
        if (MODE == 0 && R3 != 9 && tn < ntiles) load_T(tn);
        stage_sync(PRIV);
        if constexpr (R3 > 1) {
            radix3_stage<R3, false, kThreadsXZ>(tile, TY, pitch, hp, PRIV, 1 << LHX2, twl + TW::r3);
            stage_sync(PRIV);
        }
        if (MODE == 0 && R3 == 9 && tn < ntiles) load_T(tn);
        lds_fft<LHX2, false, kThreadsXZ, R3, 0, LHX2 - REG_R>(tile, TY * R3, pitch, hpm, PRIV, twl);
        if (PRIV) lds_barrier();  // rows complete for everybody before the transposed drain
        const TView tv = t_view();
        float4* sdst = reinterpret_cast<float4*>(S_next + tile_base(t)) + tv.off;
        if constexpr (REG) {
            float2 v[8], u[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c0 = tv.row + (tv.slot ^ j);
                v[j] = tile[c0];
                u[j] = tile[c0 + pitch];
            }
            butterflies<3, 0, false>(v, nullptr, 0);
            butterflies<3, 0, false>(u, nullptr, 0);
#pragma unroll
            for (int j = 0; j < 8; ++j) sdst[(size_t)(j * P) * rowq] = make_float4(v[j].x, v[j].y, u[j].x, u[j].y);
        } else {
#pragma unroll
            for (int j = 0; j < NPF; ++j) {
                if (NQ % kThreadsXZ == 0 || (int)threadIdx.x + j * kThreadsXZ < NQ) {
                    const int c0 = tv.row + (tv.slot ^ swz_c(j * P));
                    const float2 a = tile[c0], b = tile[c0 + pitch];
                    sdst[(size_t)(j * P) * rowq] = make_float4(a.x, a.y, b.x, b.y);
                }
            }
        }
        if (dyn && threadIdx.x == 0) s_next_tile = fetched;
        lds_barrier();  // the tile is free for the next fill
        advance();
    }
}

// rows [y0, y0 + rows) of the x-transformed buffer S[z][px][py] <-> a contiguous buffer [z * Hx + px][rows] (halo exchange of
// the sharded iteration); dir 0: pack, 1: unpack, 2: zero-fill
__global__ __launch_bounds__(256) void k_spectrum_rows(float2* __restrict__ S, float2* __restrict__ buf, size_t lines, int M, int y0, int rows,
                                                       int dir) {
    const size_t total = lines * (size_t)rows;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t line = i / rows;
        const int j = (int)(i - line * rows);
        float2* cell = S + line * M + (y0 + j);
        if (dir == 0) buf[i] = *cell;
        else if (dir == 1) *cell = buf[i];
        else *cell = make_float2(0.0f, 0.0f);
    }
}

}  // namespace

// Grid of a persistent x launch and, when its tiles are handed out dynamically, the armed counter (see k_x_fused_pipe).
// Tiles come from the counter by default: compute units do not all run at the same speed, and the static stride left the
// slowest one as the tail (C3: paired z pass 4.36 -> 3.94 ms, fused x pass 5.13 / 5.71 -> 5.06 / 5.61 ms; part 2 of a slab rank's
// x pass at N = 8: 0.77 -> 0.66 ms; profiles/r03_overlap_probe.txt).  `overlapped`: the launch runs beside a halo exchange
// (part 2 of a sharded step) and follows mi_rl_set_overlap: `free_cus` compute units are left to the collective's kernels.
// MI_X_DYN=0|1 / MI_X_FREE_CUS=<k> (NativeSwitches) override for every launch (A/B measurements).
int NativeFft::persistent_grid(hipStream_t s, int ntiles, bool overlapped, unsigned* grid, int** ctr_out) {
    const bool dyn = x_tiles_dynamic(sw, overlapped ? overlap_dynamic : true);
    const int free_cus = sw.x_free_cus >= 0 ? sw.x_free_cus : (overlapped ? overlap_free_cus : 0);
    const int cus = std::max(1, n_cu - std::max(0, free_cus));
    *grid = (unsigned)std::min(ntiles, cus);
    *ctr_out = nullptr;
    if (dyn) {
        if (!ctr.p) MI_TRY(ctr.alloc(256));
        // one counter per launch in flight would be needed if two dynamic launches of one context could overlap; they cannot:
        // every launch of a context goes to the caller's stream
        MI_HIP(hipMemsetAsync(ctr.p, 0, sizeof(int), s));
        *ctr_out = ctr.as<int>();
    }
    return MI_OK;
}

// One launch of the persistent kernel on `ntiles` tiles picked by `sel`: mode 0 fused (T -> epilogue -> out, S), 1 forward only
// (epi.a -> S), 2 inverse only (T -> epilogue -> out)
int NativeFft::x_pipelined(hipStream_t s, int mode, const float2* T, float* out, const ConvEpilogue& epi, int ek, const TileSelect& sel, int ntiles) {
    if (ntiles <= 0) return MI_OK;
    unsigned grid = 0;
    int* ctr_p = nullptr;
    MI_TRY(persistent_grid(s, ntiles, sel.mode == 2, &grid, &ctr_p));  // (the tiles beside the edge ones run during the halo exchange)
    const size_t xl = lds_bytes(dims.ty, dims.hx);
    // (one dispatch per mode, forward first: the order in which the kernels are instantiated, see the top of the file)
    if (mode == 1)
        return x_case(dims, [&](auto lg, auto r) {
            return launch_lds(k_x_fused_pipe<lg(), r(), 1>, grid, kThreadsXZ, xl, s, "k_x_fused_pipe<forward>", T, out, epi, dims, tw_x, S.as<float2>(), ek, ntiles, sel, pw, ctr_p);
        });
    if (mode == 0)
        return x_case(dims, [&](auto lg, auto r) {
            return launch_lds(k_x_fused_pipe<lg(), r()>, grid, kThreadsXZ, xl, s, "k_x_fused_pipe", T, out, epi, dims, tw_x, S.as<float2>(), ek, ntiles, sel, pw, ctr_p);
        });
    return x_case(dims, [&](auto lg, auto r) {
        return launch_lds(k_x_fused_pipe<lg(), r(), 2>, grid, kThreadsXZ, xl, s, "k_x_fused_pipe<inverse>", T, out, epi, dims, tw_x, (float2*)nullptr, ek, ntiles, sel, pw, ctr_p);
    });
}

// tiles of the fused x pass that hold rows of [a0, a1) or [b0, b1) (a before b): mode 1 = only those, 2 = all the others
TileSelect NativeFft::edge_tiles(int mode, int a0, int a1, int b0, int b1) const {
    TileSelect t{};
    const int ty = dims.ty;
    t.mode = mode;
    t.lo0 = a0 / ty;
    t.n0 = (a1 + ty - 1) / ty - t.lo0;
    t.lo1 = std::max(b0 / ty, t.lo0 + t.n0);   // overlapping ranges: the second one starts behind the first
    t.n1 = std::max((b1 + ty - 1) / ty - t.lo1, 0);
    return t;
}

int NativeFft::pipe_tiles(bool padded, const TileSelect* part, TileSelect* sel, int* ntiles) const {
    *sel = TileSelect{};
    int per = dims.ny / dims.ty, planes = dims.nz;
    if (padded) {  // only the tiles that hold rows of the caller's volume; the others are zero-filled
        sel->mode = 3;
        sel->n0 = (pw.n[1] + dims.ty - 1) / dims.ty;
        per = sel->n0;
        planes = pw.n[2];
    } else if (part && part->mode != 0) {
        *sel = *part;
        per = sel->mode == 1 ? sel->n0 + sel->n1 : per - sel->n0 - sel->n1;
        if (sel->nz > 0) {
            MI_REQUIRE(sel->z0 >= 0 && sel->z0 + sel->nz <= dims.nz, "native FFT: plane range [%d, %d) outside [0, %d)", sel->z0,
                       sel->z0 + sel->nz, dims.nz);
            planes = sel->nz;
        }
    }
    *ntiles = planes * per;
    return MI_OK;
}

int NativeFft::x_forward(hipStream_t s, const float* in) {
    // persistent kernel with prefetch: unpadded grids, and padded ones under the conditions of the fused pass (x_route)
    XCall c;
    c.forward = true;
    c.aligned = ((uintptr_t)in % 16) == 0;
    if (x_route(dims, sw, pw, c) == XRoute::pipe_forward) {
        ConvEpilogue e;
        e.a = in;
        TileSelect sel;
        int ntiles = 0;
        MI_TRY(pipe_tiles(pw.on != 0, nullptr, &sel, &ntiles));
        return x_pipelined(s, 1, nullptr, nullptr, e, EPI_NONE, sel, ntiles);
    }
    const unsigned xtiles = (unsigned)((size_t)dims.nz * (dims.ny / dims.ty));
    return x_case(dims, [&](auto lg, auto r) {
        return launch_lds(k_x_forward<lg(), r()>, xtiles, kThreadsXZ, lds_bytes(dims.ty, dims.hx), s, "k_x_forward", in, S.as<float2>(), dims, tw_x, pw);
    });
}

// P5 (+ P1 of the next convolution when fuse_forward): T -> out (may be null when fused) [-> S]
int NativeFft::x_inverse(hipStream_t s, float* out, int epi_kind, const ConvEpilogue& epi, bool fuse_forward, const TileSelect* part) {
    const int ek = epi_kind == EPI_TAPER_SHELL ? EPI_NONE : epi_kind;
    MI_REQUIRE(ek == EPI_NONE || ek == EPI_RATIO || ek == EPI_UPDATE || ek == EPI_UPDATE_REG, "native FFT: unknown epilogue %d", epi_kind);
    MI_REQUIRE(!fuse_forward || ek == EPI_RATIO || ek == EPI_UPDATE, "native FFT: only the plain RL epilogues fuse");
    MI_REQUIRE(!fuse_forward || can_fuse(), "native FFT: a replicate-padded axis cannot fuse consecutive convolutions");
    // (MI_FFT_NO_XPIPE=1 sends a whole fused pass through k_x_inverse too -- every stage in LDS, same arithmetic: the reference route
    // of tests/test_gpu_x_register_stage.py; a subset of the tiles exists only in the persistent kernel)
    XCall c;
    c.fuse_forward = fuse_forward;
    c.whole = !(part && part->mode != 0);
    c.aligned = ((uintptr_t)epi.a % 16) == 0 && ((uintptr_t)out % 16) == 0;
    c.ek = ek;
    c.taper_shell = epi_kind == EPI_TAPER_SHELL;
    c.has_out = out != nullptr;
    const XRoute route = x_route(dims, sw, pw, c);
    MI_REQUIRE(route != XRoute::no_subset, "native FFT: this kernel cannot run a subset of its tiles");
    if (route == XRoute::pipe_fused || route == XRoute::pipe_inverse) {
        TileSelect sel;
        int ntiles = 0;
        MI_TRY(pipe_tiles(pw.on != 0, route == XRoute::pipe_fused ? part : nullptr, &sel, &ntiles));
        return x_pipelined(s, route == XRoute::pipe_fused ? 0 : 2, t_spec, out, epi, ek, sel, ntiles);
    }
    const unsigned xtiles = (unsigned)((size_t)dims.nz * (dims.ny / dims.ty));
    const size_t xl = lds_bytes(dims.ty, dims.hx);
    return x_case(dims, [&](auto lg, auto r) {
        return fuse_forward ? launch_lds(k_x_inverse<lg(), r(), true>, xtiles, kThreadsXZ, xl, s, "k_x_inverse<fused>", t_spec, out, epi, dims, tw_x, S.as<float2>(), ek, pw)
                            : launch_lds(k_x_inverse<lg(), r(), false>, xtiles, kThreadsXZ, xl, s, "k_x_inverse", t_spec, out, epi, dims, tw_x, S.as<float2>(), ek, pw);
    });
}

int NativeFft::spectrum_rows(hipStream_t s, int y0, int rows, float2* buf, int dir, int z0, int nzc) {
    MI_REQUIRE(y0 >= 0 && rows > 0 && y0 + rows <= dims.ny, "spectrum rows [%d, %d) outside [0, %d)", y0, y0 + rows, dims.ny);
    MI_REQUIRE(dir == 2 || buf, "spectrum rows: null buffer");
    if (nzc <= 0) { z0 = 0; nzc = dims.nz; }
    MI_REQUIRE(z0 >= 0 && z0 + nzc <= dims.nz, "spectrum rows: planes [%d, %d) outside [0, %d)", z0, z0 + nzc, dims.nz);
    // lines (z, px) of the chunk: they keep their place in S and in the packed buffer [z * Hx + px][rows]
    const size_t line0 = (size_t)z0 * dims.hx, lines = (size_t)nzc * dims.hx, total = lines * (size_t)rows;
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(k_spectrum_rows, dim3((unsigned)blocks), dim3(256), 0, s, S.as<float2>() + line0 * dims.xrow,
                       buf ? buf + line0 * (size_t)rows : buf, lines, dims.xrow, y0, rows, dir);
    return launch_check("k_spectrum_rows");
}

}  // namespace mi
