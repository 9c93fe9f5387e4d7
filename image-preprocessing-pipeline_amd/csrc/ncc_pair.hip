// The per-pair path of MIP-NCC (libcrossmips.cpp:319-481 for one pair; also the careful path of pairs the batched pipeline hands
// back): float tile sums in the reference's order, fp64 summed-area tables, cross terms shift by shift (k_ncc_blk), entries in the
// two-pass form where a decision is close (k_ncc_exact), the refinement driven from the host, the working sets kept between calls.
#include "ncc_dev.h"

using namespace mi;

namespace {

// one wave per tile (blockIdx.y = MIP of the plane): the tile is staged in LDS with coalesced loads, then lane 0 adds its 1024
// pixels in the reference's row-major order with a FLOAT running sum (bit-identical by construction)
__global__ __launch_bounds__(64) void k_tile_sums(const float* __restrict__ img1, const float* __restrict__ img2, size_t pstride, int height,
                                                  int width, float* __restrict__ ps1, float* __restrict__ ps2) {
    __shared__ float tile[TILE * TILE];
    const float* img = (blockIdx.y ? img2 : img1) + (size_t)blockIdx.z * pstride;
    float* ps = (blockIdx.y ? ps2 : ps1) + (size_t)blockIdx.z * pstride;
    const int pw = width / TILE, t = blockIdx.x;
    const int ti = t / pw, tj = t - ti * pw;
    const float* p = img + (size_t)ti * TILE * width + tj * TILE;
    const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
#pragma unroll
    for (int l = 0; l < TILE; l += 2) tile[(l + half) * TILE + col] = p[(size_t)(l + half) * width + col];
    __syncthreads();
    if (lane == 0) {
        float s = 0.0f;
#pragma unroll 32
        for (int i = 0; i < TILE * TILE; ++i) s += tile[i];
        ps[t] = s;
    }
}

template <int NT>
__device__ __forceinline__ double block_sum(double v, double* sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < NT / 64; ++w) r += sh[w];
    return r;
}

// pixel sums of both MIPs of a plane in MEAN_PARTS slices each (blockIdx.y = MIP), for the global means
__global__ __launch_bounds__(256) void k_mip_partial(const float* __restrict__ m1, const float* __restrict__ m2, size_t pstride, size_t sstride,
                                                     size_t n, double* __restrict__ part) {
    __shared__ double sh[4];
    const float* m = (blockIdx.y ? m2 : m1) + (size_t)blockIdx.z * pstride;
    part += (size_t)blockIdx.z * sstride;
    const size_t per = (n + MEAN_PARTS - 1) / MEAN_PARTS, lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    double acc = 0.0;
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) acc += (double)m[i];
    acc = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.y * MEAN_PARTS + blockIdx.x] = acc;
}

// global mean c0 of each of the two MIPs of a plane (blockIdx.x = 0 / 1) from the slices' sums (fixed order) and the table of
// its float tile sums
constexpr int kMeanLdsEntries = 4096;  // 32 KB of doubles: tile-sum tables of planes up to e.g. 2048 x 2016 pixels
__global__ __launch_bounds__(1024) void k_mip_mean(const double* __restrict__ part, size_t pstride, size_t sstride, int dimu, int dimv,
                                                   const float* __restrict__ ps1, const float* __restrict__ ps2, double* __restrict__ c0a,
                                                   double* __restrict__ c0b, double* __restrict__ ts1, double* __restrict__ ts2) {
    const size_t po = (size_t)blockIdx.z * pstride, so = (size_t)blockIdx.z * sstride;
    part += so; c0a += so; c0b += so;
    const float* ps = blockIdx.x ? ps2 : ps1;
    if (ps) ps += po;
    double* ts = (blockIdx.x ? ts2 : ts1) + so;
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int k = 0; k < MEAN_PARTS; ++k) acc += part[blockIdx.x * MEAN_PARTS + k];
        *(blockIdx.x ? c0b : c0a) = acc / ((double)dimu * (double)dimv);
    }
    const int ph = dimu / TILE, pw = dimv / TILE;
    if (ps && ph * pw > 0) {
        // (ph+1) x (pw+1) inclusive table; a few hundred entries: one lane per row, then one per column.  The two running sums
        // are chains of dependent read-modify-writes: through global memory they cost ~1.5 us per step (64 steps: 0.1 ms for a
        // kernel that does nothing else), so the table is built in LDS when it fits and written out once
        const int w1 = pw + 1, n = (ph + 1) * w1;
        __shared__ double tl[kMeanLdsEntries];
        double* t = n <= kMeanLdsEntries ? tl : ts;
        for (int i = threadIdx.x; i < n; i += 1024) t[i] = 0.0;
        __syncthreads();
        for (int r = threadIdx.x; r < ph; r += 1024) {
            double run = 0.0;
            for (int c = 0; c < pw; ++c) { run += (double)ps[r * pw + c]; t[(r + 1) * w1 + c + 1] = run; }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < pw; c += 1024) {
            double run = 0.0;
            for (int r = 0; r < ph; ++r) { run += t[(r + 1) * w1 + c + 1]; t[(r + 1) * w1 + c + 1] = run; }
        }
        if (t != ts) {
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += 1024) ts[i] = tl[i];
        }
    }
}

__device__ __forceinline__ double wave_inclusive_scan(double v) {
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// row pass: one wave per (row, MIP): P/Q[(i+1)][j+1] = prefix along j of (f - c0), (f - c0)^2; row 0 and column 0 are zero
__global__ __launch_bounds__(64) void k_sat_rows(const float* __restrict__ m1, const float* __restrict__ m2, size_t pstride, size_t sstride,
                                                 int dimu, int dimv, const double* __restrict__ c0a, const double* __restrict__ c0b,
                                                 double* __restrict__ P1, double* __restrict__ Q1, double* __restrict__ P2,
                                                 double* __restrict__ Q2) {
    const size_t so = (size_t)blockIdx.z * sstride;
    const float* m = (blockIdx.y ? m2 : m1) + (size_t)blockIdx.z * pstride;
    double* P = (blockIdx.y ? P2 : P1) + so;
    double* Q = (blockIdx.y ? Q2 : Q1) + so;
    const double cm = (blockIdx.y ? c0b : c0a)[so];
    const int w1 = dimv + 1, lane = threadIdx.x;
    const int i = blockIdx.x;  // 0 .. dimu (row i of the table; table row 0 is all zero)
    if (i == 0) {
        for (int j = lane; j < w1; j += 64) { P[j] = 0.0; Q[j] = 0.0; }
        return;
    }
    const float* row = m + (size_t)(i - 1) * dimv;
    double cp = 0.0, cq = 0.0;
    if (lane == 0) { P[(size_t)i * w1] = 0.0; Q[(size_t)i * w1] = 0.0; }
    for (int j0 = 0; j0 < dimv; j0 += 64) {
        const int j = j0 + lane;
        const double g = j < dimv ? (double)row[j] - cm : 0.0;
        const double sp = wave_inclusive_scan(g) + cp, sq = wave_inclusive_scan(g * g) + cq;
        if (j < dimv) { P[(size_t)i * w1 + j + 1] = sp; Q[(size_t)i * w1 + j + 1] = sq; }
        cp = __shfl(sp, 63, 64);
        cq = __shfl(sq, 63, 64);
    }
}

// column pass, in place: a wave owns 64 neighbouring columns of one table (blockIdx.y) and walks down the rows with a running
// sum per lane -- every access is a 512-byte row segment; the loads of UNR rows are in flight together (they do not depend on
// the running sums).  The first version gave each wave ONE column (lanes = rows, stride of a whole table row between lanes):
// 88 us per C5 pair, more than the six MIPs.
__global__ __launch_bounds__(64) void k_sat_cols(size_t sstride, int dimu, int dimv, double* __restrict__ P1, double* __restrict__ Q1,
                                                 double* __restrict__ P2, double* __restrict__ Q2) {
    double* S = (blockIdx.y == 0 ? P1 : (blockIdx.y == 1 ? Q1 : (blockIdx.y == 2 ? P2 : Q2))) + (size_t)blockIdx.z * sstride;
    const int w1 = dimv + 1, j = blockIdx.x * 64 + threadIdx.x + 1;
    if (j > dimv) return;
    constexpr int UNR = 8;
    double run = 0.0;
    double* p = S + (size_t)w1 + j;  // table row 1
    int i = 1;
    for (; i + UNR - 1 <= dimu; i += UNR, p += (size_t)UNR * w1) {
        double v[UNR];
#pragma unroll
        for (int q = 0; q < UNR; ++q) v[q] = p[(size_t)q * w1];
#pragma unroll
        for (int q = 0; q < UNR; ++q) { run += v[q]; p[(size_t)q * w1] = run; }
    }
    for (; i <= dimu; ++i, p += w1) { run += *p; *p = run; }
}

// NCC cross terms, register-blocked.  A block is (4 u) x (8 v) shifts; a work-group takes a GROUP of up to 8 blocks that share
// u0 (a "row" of the shift map), a chunk of m2 rows and a segment of <= 512 m2 columns: wave w owns block w.  The m2 rows and
// the window of m1 rows all the group's blocks need (columns from the smallest v0 on, zero outside the MIP) are staged in LDS
// ONCE for the eight blocks with unit-stride loads -- staging, not the fp64 pipe, was the bound when every block staged its
// own window.  A lane then owns 4 neighbouring m2 columns of a row and, per u, the 11 m1 values its 8 shifts pair them with:
// thirteen 16-byte LDS reads feed 128 fp64 FMAs (exact fp32 products accumulated in fp64).  Zeros outside the MIP restrict
// every shift's sum to its own window.  Each wave reduces its own 32 sums (no work-group reduction).  Groups come from the
// regular grid (full maps: group = u-block, wave = v-block) or from a list (the "missing entries" of the neighbourhood
// refinement, gpu_NCC_miss).  The chunks' partial sums are added up in a fixed order by k_ncc_finish, which also applies the
// window statistics from the summed-area tables: deterministic, whatever the launch geometry.  Replaces gpu_NCC_map /
// gpu_NCC_miss (compute_funcs.cu:730-935).
constexpr int BU = 4, BV = 8, BC = 4, GW = 8, BLK_THREADS = 64 * GW;
// groups (list mode): 2 + GW ints each: {u0, number of blocks nb <= GW, v0[0] <= v0[1] <= ... (multiples of BV apart)}
__global__ __launch_bounds__(BLK_THREADS) void k_ncc_blk(const float* __restrict__ m1, const float* __restrict__ m2, int dimu, int dimv, int du,
                                                         int dv, int nvb, const int* __restrict__ groups, int n_groups, int rows_per_chunk,
                                                         int R, int seg_w, int nseg, int pitch1, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int u0, nb, vmin, voff;  // voff: this wave's v0 - vmin
    if (groups) {
        const int* g = groups + (size_t)blockIdx.x * (2 + GW);
        u0 = g[0];
        nb = g[1];
        vmin = g[2];
        voff = g[2 + min(wave, nb - 1)] - vmin;
    } else {  // group = (u-block, run of GW v-blocks)
        const int nvg = (nvb + GW - 1) / GW, ub = (int)blockIdx.x / nvg, vg = (int)blockIdx.x - ub * nvg;
        u0 = ub * BU - du;
        nb = min(GW, nvb - vg * GW);
        vmin = vg * GW * BV - dv;
        voff = min(wave, nb - 1) * BV;
    }
    // chunk = (row chunk, column segment of seg_w m2 columns): wide MIPs are cut so that many rows fit one LDS stage
    const int rc = (int)blockIdx.y / nseg, sg = (int)blockIdx.y - rc * nseg;
    const int r_begin = rc * rows_per_chunk, r_end = min(dimu, r_begin + rows_per_chunk);
    const int cbeg = sg * seg_w, cw = min(seg_w, dimv - cbeg);  // m2 columns [cbeg, cbeg + cw)
    const int quads = (cw + BC - 1) / BC, pitch2 = seg_w;        // seg_w and pitch1 are multiples of BC
    float* l1 = lds;                            // R + BU - 1 rows of m1: l1[j][x] = m1[rb + u0 + j][cbeg + vmin + x]
    float* l2 = lds + (R + BU - 1) * pitch1;    // R rows of m2
    double acc[BU][BV];
#pragma unroll
    for (int a = 0; a < BU; ++a)
#pragma unroll
        for (int b = 0; b < BV; ++b) acc[a][b] = 0.0;
    for (int rb = r_begin; rb < r_end; rb += R) {
        const int nrow = min(R, r_end - rb);
        __syncthreads();
        {   // staging: a wave per row (no index division), four independent 64-column loads per lane in flight
            constexpr int UNR = 4;
            for (int j = wave; j < nrow + BU - 1; j += GW) {
                const int r1 = rb + u0 + j;
                const bool row_ok = r1 >= 0 && r1 < dimu;
                const float* src = m1 + (size_t)(row_ok ? r1 : 0) * dimv + cbeg + vmin;
                float* dst = l1 + j * pitch1;
                for (int x0 = lane; x0 < pitch1; x0 += 64 * UNR) {
                    float v[UNR];
#pragma unroll
                    for (int q = 0; q < UNR; ++q) {
                        const int x = x0 + 64 * q, c1 = cbeg + vmin + x;
                        v[q] = (row_ok && x < pitch1 && c1 >= 0 && c1 < dimv) ? src[x] : 0.0f;
                    }
#pragma unroll
                    for (int q = 0; q < UNR; ++q)
                        if (x0 + 64 * q < pitch1) dst[x0 + 64 * q] = v[q];
                }
            }
            for (int j = wave; j < nrow; j += GW) {
                const float* src = m2 + (size_t)(rb + j) * dimv + cbeg;
                float* dst = l2 + j * pitch2;
                for (int x0 = lane; x0 < pitch2; x0 += 64 * UNR) {
                    float v[UNR];
#pragma unroll
                    for (int q = 0; q < UNR; ++q) v[q] = x0 + 64 * q < cw ? src[x0 + 64 * q] : 0.0f;
#pragma unroll
                    for (int q = 0; q < UNR; ++q)
                        if (x0 + 64 * q < pitch2) dst[x0 + 64 * q] = v[q];
                }
            }
        }
        __syncthreads();
        if (wave < nb) {
            for (int it = lane; it < nrow * quads; it += 64) {
                const int rr = it / quads, c = (it - rr * quads) * BC;
                const float4 tq = *reinterpret_cast<const float4*>(l2 + rr * pitch2 + c);
                const double t[BC] = {(double)tq.x, (double)tq.y, (double)tq.z, (double)tq.w};
#pragma unroll
                for (int a = 0; a < BU; ++a) {
                    const float4* row = reinterpret_cast<const float4*>(l1 + (rr + a) * pitch1 + voff + c);
                    const float4 f0 = row[0], f1 = row[1], f2 = row[2];
                    const double f[12] = {(double)f0.x, (double)f0.y, (double)f0.z, (double)f0.w, (double)f1.x, (double)f1.y,
                                          (double)f1.z, (double)f1.w, (double)f2.x, (double)f2.y, (double)f2.z, (double)f2.w};
#pragma unroll
                    for (int b = 0; b < BV; ++b)
#pragma unroll
                        for (int x = 0; x < BC; ++x) acc[a][b] = fma(f[x + b], t[x], acc[a][b]);
                }
            }
        }
    }
    if (wave >= nb) return;
    // the wave's own 32 sums: shuffle tree, lane 0 stores
    double* dst = partial + (((size_t)blockIdx.y * n_groups + blockIdx.x) * GW + wave) * (BU * BV);
#pragma unroll
    for (int a = 0; a < BU; ++a)
#pragma unroll
        for (int b = 0; b < BV; ++b) {
            double v = acc[a][b];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) dst[a * BV + b] = v;
        }
}

// one lane per requested entry: cross term = sum of the chunks' partials (fixed order), then the NCC value of
// compute_NCC (compute_funcs.cu:1163-1292).  entries == nullptr: the full (2du+1) x (2dv+1) map in row-major order;
// else entry e = {u, v, slot in the partials of a chunk ((group * GW + wave) * 32 + a * 8 + b), output slot}
__global__ __launch_bounds__(256) void k_ncc_finish(const double* __restrict__ partial, int n_chunks, int n_groups,
                                                    const int* __restrict__ entries, int n_entries, int dimu, int dimv, int du, int dv,
                                                    SatView s1, SatView s2, float* __restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    int u, v, pidx, slot;
    if (entries) {
        u = entries[4 * e];
        v = entries[4 * e + 1];
        pidx = entries[4 * e + 2];
        slot = entries[4 * e + 3];
    } else {
        const int W = 2 * dv + 1, iu = e / W, iv = e - iu * W;
        u = iu - du;
        v = iv - dv;
        const int nvb = (W + BV - 1) / BV, slots = (nvb + GW - 1) / GW * GW;  // block slots per u-block: its groups x GW
        pidx = (((iu / BU) * slots + iv / BV) * BU + iu % BU) * BV + iv % BV;
        slot = e;
    }
    const int nr = dimu - abs(u), nc = dimv - abs(v);
    if (nr <= 0 || nc <= 0) { out[slot] = __int_as_float(0x7fc00000); return; }  // reference: empty loops, 0/0
    double cr = 0.0;
#pragma unroll 8
    for (int ch = 0; ch < n_chunks; ++ch) cr += partial[(size_t)ch * n_groups * (GW * BU * BV) + pidx];  // fixed order
    double fm, sf, F1, tm, st, F2;
    window_stats(s1, dimu, dimv, max(u, 0), max(v, 0), nr, nc, &fm, &sf, &F1);
    window_stats(s2, dimu, dimv, max(-u, 0), max(-v, 0), nr, nc, &tm, &st, &F2);
    (void)fm; (void)st;
    const double num = cr - tm * sf;
    // a window without variance: the reference's two-pass sums are exactly 0 there and it returns 0/0 = NaN
    // (compute_funcs.cu:1277-1290); the table differences are exact for such data too, but the cross term is not
    out[slot] = (F1 > 0.0 && F2 > 0.0) ? (float)(num / sqrt(F1 * F2)) : __int_as_float(0x7fc00000);
}

// builds tile sums (float, reference order), global means and the summed-area tables of both MIPs of a plane
// (of `np` pairs at once: pair q's MIPs / tile sums sit q * pstride floats, its tables q * sstride doubles behind pair 0's)
int prepare_plane(hipStream_t s, const float* m1, const float* m2, int dimu, int dimv, float* ps1, float* ps2, double* sat, SatView* v1,
                  SatView* v2, int np = 1, size_t pstride = 0, size_t sstride = 0) {
    const SatLayout L(dimu, dimv);
    const bool tiled = (dimu / TILE) * (dimv / TILE) > 0;
    double *c0a = sat, *c0b = sat + 1, *P1 = sat + 2, *Q1 = P1 + L.tab, *P2 = Q1 + L.tab, *Q2 = P2 + L.tab, *T1 = Q2 + L.tab, *T2 = T1 + L.ts;
    if (tiled) {
        const int nt = (dimu / TILE) * (dimv / TILE);
        hipLaunchKernelGGL(k_tile_sums, dim3(nt, 2, np), dim3(64), 0, s, m1, m2, pstride, dimu, dimv, ps1, ps2);
        MI_TRY(launch_check("k_tile_sums"));
    }
    double* part = T2 + L.ts;
    hipLaunchKernelGGL(k_mip_partial, dim3(MEAN_PARTS, 2, np), dim3(256), 0, s, m1, m2, pstride, sstride, (size_t)dimu * dimv, part);
    MI_TRY(launch_check("k_mip_partial"));
    hipLaunchKernelGGL(k_mip_mean, dim3(2, 1, np), dim3(1024), 0, s, part, pstride, sstride, dimu, dimv, tiled ? ps1 : nullptr,
                       tiled ? ps2 : nullptr, c0a, c0b, T1, T2);
    MI_TRY(launch_check("k_mip_mean"));
    hipLaunchKernelGGL(k_sat_rows, dim3(dimu + 1, 2, np), dim3(64), 0, s, m1, m2, pstride, sstride, dimu, dimv, c0a, c0b, P1, Q1, P2, Q2);
    MI_TRY(launch_check("k_sat_rows"));
    hipLaunchKernelGGL(k_sat_cols, dim3((dimv + 63) / 64, 4, np), dim3(64), 0, s, sstride, dimu, dimv, P1, Q1, P2, Q2);
    MI_TRY(launch_check("k_sat_cols"));
    *v1 = SatView{P1, Q1, tiled ? T1 : nullptr, c0a, dimv + 1};
    *v2 = SatView{P2, Q2, tiled ? T2 : nullptr, c0b, dimv + 1};
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ exact entries (two-pass form)
// A decision whose operands are closer than ncc_margin() is re-taken on entries recomputed by k_ncc_exact.
// One work-group per listed entry {u, v, slot}: compute_NCC's own two-pass form (compute_funcs.cu:1163-1292) -- the window means
// first (the reference's flavour: float tile sums + border pixels, here from the tables, identical to 1e-16), then
//   num = sum f (t - tmean),  F1 = sum (f - fmean)^2,  F2 = sum (t - tmean)^2
// by direct fp64 summation over the window (no algebraic rearrangement, no cancellation), lanes and waves added in a fixed order.
__global__ __launch_bounds__(256) void k_ncc_exact(const float* __restrict__ m1, const float* __restrict__ m2, int dimu, int dimv, SatView s1, SatView s2,
                                                   const int* __restrict__ entries, float* __restrict__ out) {
    __shared__ double sh[4];
    const int u = entries[3 * blockIdx.x], v = entries[3 * blockIdx.x + 1], slot = entries[3 * blockIdx.x + 2];
    const int nr = dimu - abs(u), nc = dimv - abs(v);
    if (nr <= 0 || nc <= 0) { if (threadIdx.x == 0) out[slot] = __int_as_float(0x7fc00000); return; }
    const int r1 = max(u, 0), c1 = max(v, 0), r2 = max(-u, 0), c2 = max(-v, 0);
    double fm, sf, F1s, tm, st, F2s;
    window_stats(s1, dimu, dimv, r1, c1, nr, nc, &fm, &sf, &F1s);
    window_stats(s2, dimu, dimv, r2, c2, nr, nc, &tm, &st, &F2s);
    (void)sf; (void)st; (void)F1s; (void)F2s;
    double num = 0.0, F1 = 0.0, F2 = 0.0;
    const size_t n = (size_t)nr * nc;
    for (size_t e = threadIdx.x; e < n; e += 256) {
        const int i = (int)(e / nc), j = (int)(e - (size_t)i * nc);
        const double f = (double)m1[(size_t)(r1 + i) * dimv + c1 + j], t = (double)m2[(size_t)(r2 + i) * dimv + c2 + j];
        const double df = f - fm, dt = t - tm;
        num += f * dt;
        F1 += df * df;
        F2 += dt * dt;
    }
    num = block_sum<256>(num, sh);
    F1 = block_sum<256>(F1, sh);
    F2 = block_sum<256>(F2, sh);
    if (threadIdx.x == 0) out[slot] = (float)(num / sqrt(F1 * F2));  // flat window: 0 / 0 = NaN like the reference
}

struct Workspace {
    DevBuf buf;       // floats: MIPs | tile sums | maps | miss results
    DevBuf sat;       // doubles: per plane c0, P, Q, TS tables of both MIPs
    DevBuf mip_tmp;   // floats: per tile and row band, the column maxima the yz MIPs are reduced from
    SatView v1[3], v2[3];
    DevBuf list;      // ints: {u, v0, count, slot} groups of missing entries
    DevBuf partial[3]; // doubles: per plane, the row chunks' partial cross terms of a full map
    size_t floats = 0;
    int list_cap = 0;
    std::vector<int> host_groups, host_entries, host_slots;
    std::vector<long long> host_keys;
    PinnedBuf pin_groups, pin_res, pin_maps;
    DevBuf exact_list, exact_out;   // k_ncc_exact: {u, v, slot} entries and their values
    PinnedBuf pin_exact_in, pin_exact_out;
    int n_exact = 0;                // entries recomputed exactly for the current pair (statistics / tests)
};

// values[q] = the exact NCC of shift uv[2q], uv[2q+1] of a plane.  Synchronises `s`.
int exact_entries(hipStream_t s, const PlaneGeom& g, int plane, const float* d_base, Workspace& ws, const std::vector<int>& uv,
                  std::vector<float>& values) {
    const int n = (int)uv.size() / 2;
    values.assign(n, 0.0f);
    if (n == 0) return MI_OK;
    MI_TRY(ws.pin_exact_in.reserve(sizeof(int) * 3 * (size_t)n));
    MI_TRY(ws.pin_exact_out.reserve(sizeof(float) * (size_t)n));
    if (ws.exact_list.bytes < sizeof(int) * 3 * (size_t)n || ws.exact_out.bytes < sizeof(float) * (size_t)n) {
        MI_HIP(hipStreamSynchronize(s));
        MI_TRY(ws.exact_list.alloc(sizeof(int) * 3 * (size_t)n * 2));
        MI_TRY(ws.exact_out.alloc(sizeof(float) * (size_t)n * 2));
    }
    int* h = ws.pin_exact_in.as<int>();
    for (int q = 0; q < n; ++q) { h[3 * q] = uv[2 * q]; h[3 * q + 1] = uv[2 * q + 1]; h[3 * q + 2] = q; }
    MI_HIP(hipMemcpyAsync(ws.exact_list.p, h, sizeof(int) * 3 * (size_t)n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ncc_exact, dim3(n), dim3(256), 0, s, d_base + g.mip1, d_base + g.mip2, g.dimu, g.dimv, ws.v1[plane], ws.v2[plane],
                       ws.exact_list.as<int>(), ws.exact_out.as<float>());
    MI_TRY(launch_check("k_ncc_exact"));
    MI_HIP(hipMemcpyAsync(ws.pin_exact_out.p, ws.exact_out.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    std::memcpy(values.data(), ws.pin_exact_out.p, sizeof(float) * (size_t)n);
    ws.n_exact += n;
    ncc_count(2, n);
    return MI_OK;
}

// compute_MAX_ind (compute_funcs.cu:1294-1305) decided on exact values: every entry within the decision margin of the largest
// value is recomputed by k_ncc_exact (once: `exact` remembers) before the first strict maximum is taken.  `to_uv(i, &u, &v)` maps
// an index of `v` to its shift.
template <class ToUV>
int argmax_exact(hipStream_t s, const PlaneGeom& g, int plane, const float* d_base, Workspace& ws, float* v, int len, std::vector<unsigned char>& exact,
                 ToUV to_uv, int* ind) {
    const float margin = ncc_margin();
    for (int round = 0; round < 2; ++round) {
        const int best = argmax_first(v, len);
        if (!(v[best] == v[best])) { *ind = best; return MI_OK; }  // leading NaN: the reference keeps it whatever follows
        std::vector<int> uv, idx;
        int close = 0;
        for (int i = 0; i < len; ++i)
            if (v[i] == v[i] && v[best] - v[i] < margin) {
                ++close;
                if (!exact[i]) { int a, b; to_uv(i, &a, &b); uv.push_back(a); uv.push_back(b); idx.push_back(i); }
            }
        if (close < 2 || idx.empty()) { *ind = best; return MI_OK; }
        std::vector<float> val;
        MI_TRY(exact_entries(s, g, plane, d_base, ws, uv, val));
        for (size_t q = 0; q < idx.size(); ++q) { v[idx[q]] = val[q]; exact[idx[q]] = 1; }
    }
    *ind = argmax_first(v, len);
    return MI_OK;
}


// NCC values of one plane: the blocked cross terms + the finishing pass.  d_groups / d_entries == nullptr: the full map into
// d_out; else the listed groups {u0, nb, v0[GW]} and entries {u, v, partial index, output slot}.  `partial` grows as needed.
int ncc_launch(hipStream_t s, const float* m1, const float* m2, int dimu, int dimv, int delayu, int delayv, const SatView& v1, const SatView& v2,
               const int* d_groups, int n_groups, const int* d_entries, int n_entries, DevBuf& partial, float* d_out) {
    const int nvb = (2 * delayv + 1 + BV - 1) / BV;
    if (!d_groups) {
        n_groups = ((2 * delayu + 1 + BU - 1) / BU) * ((nvb + GW - 1) / GW);
        n_entries = (2 * delayu + 1) * (2 * delayv + 1);
    }
    if (n_groups <= 0 || n_entries <= 0) return MI_OK;
    // column segments of at most 512 m2 columns, row chunks so that about 768 work-groups of 8 waves exist
    const int nseg = (dimv + 511) / 512;
    const int seg_w = ((dimv + nseg - 1) / nseg + BC - 1) / BC * BC;
    int rchunks = (768 + n_groups * nseg - 1) / (n_groups * nseg);
    rchunks = imax(1, imin(rchunks, (dimu + 7) / 8));
    const int rows_per_chunk = (dimu + rchunks - 1) / rchunks;
    rchunks = (dimu + rows_per_chunk - 1) / rows_per_chunk;
    const int chunks = rchunks * nseg;
    // the m1 window of a group: its blocks start at most (GW - 1) * BV columns apart
    const int quads = seg_w / BC, pitch1 = seg_w + GW * BV, pitch2 = seg_w;
    // rows staged together: a few items per lane and stage, within 60 KB of LDS (two work-groups per CU)
    const int fit = ((60 * 1024) / (int)sizeof(float) - (BU - 1) * pitch1) / (pitch1 + pitch2);
    const int R = imax(1, imin(imin(rows_per_chunk, 1536 / quads), fit));
    const size_t lds = sizeof(float) * ((size_t)(R + BU - 1) * pitch1 + (size_t)R * pitch2);
    const size_t need = sizeof(double) * (size_t)chunks * n_groups * GW * BU * BV;
    if (partial.bytes < need) {
        MI_HIP(hipStreamSynchronize(s));  // an earlier launch of this stream may still read the old buffer
        MI_TRY(partial.alloc(need));
    }
    hipLaunchKernelGGL(k_ncc_blk, dim3(n_groups, chunks), dim3(BLK_THREADS), lds, s, m1, m2, dimu, dimv, delayu, delayv, nvb, d_groups, n_groups,
                       rows_per_chunk, R, seg_w, nseg, pitch1, partial.as<double>());
    MI_TRY(launch_check("k_ncc_blk"));
    hipLaunchKernelGGL(k_ncc_finish, dim3((n_entries + 255) / 256), dim3(256), 0, s, partial.as<double>(), chunks, n_groups, d_entries, n_entries,
                       dimu, dimv, delayu, delayv, v1, v2, d_out);
    return launch_check("k_ncc_finish");
}

// compute_Neighborhood (compute_funcs.cu:1324-1592): win = (2wu+1)x(2wv+1) window around the peak,
// re-centred up to maxIter times; entries exposed by a move are computed on the device.
int refine_neighbourhood(hipStream_t s, const mi_ncc_params& P, const float* map, const PlaneGeom& g, int plane, const float* d_base,
                         Workspace& ws,
                         std::vector<float>& win, int* du, int* dv, bool* failed, std::vector<unsigned char>* exact_out = nullptr) {
    const int H = 2 * g.wu + 1, W = 2 * g.wv + 1, Wm = 2 * g.delayv + 1, Hm = 2 * g.delayu + 1;
    std::vector<float> mapv(map, map + (size_t)Hm * Wm);
    std::vector<unsigned char> map_exact((size_t)Hm * Wm, 0);
    int ind_max = 0;
    MI_TRY(argmax_exact(s, g, plane, d_base, ws, mapv.data(), Hm * Wm, map_exact,
                        [&](int i, int* a, int* b) { *a = i / Wm - g.delayu; *b = i % Wm - g.delayv; }, &ind_max));
    map = mapv.data();
    const int initu = imin(imax(0, ind_max / Wm - g.wu), 2 * (g.delayu - g.wu));
    const int initv = imin(imax(0, ind_max % Wm - g.wv), 2 * (g.delayv - g.wv));
    MI_REQUIRE(initu >= 0 && initv >= 0, "CrossMIPs: negative index detected (initi)");
    win.assign((size_t)H * W, 0.0f);
    std::vector<unsigned char> win_exact((size_t)H * W, 0), old_exact;
    for (int r = 0; r < H; ++r) {
        std::memcpy(&win[(size_t)r * W], &map[(size_t)(initu + r) * Wm + initv], sizeof(float) * W);
        std::memcpy(&win_exact[(size_t)r * W], &map_exact[(size_t)(initu + r) * Wm + initv], W);
    }
    *du = initu - g.delayu + g.wu;
    *dv = initv - g.delayv + g.wv;
    ind_max = W * (ind_max / Wm - initu) + (ind_max % Wm - initv);
    const int ind_ref = W * g.wu + g.wv;
    std::vector<float> old;
    std::vector<int> miss;
    for (int it = 0; it < P.maxIter && ind_max != ind_ref; ++it) {
        const int deltau = ind_max / W - g.wu, deltav = ind_max % W - g.wv;
        old = win;
        old_exact = win_exact;
        *du += deltau;
        *dv += deltav;
        miss.clear();
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const int sr = r + deltau, sc = c + deltav;
                if (sr >= 0 && sr < H && sc >= 0 && sc < W) {
                    win[(size_t)r * W + c] = old[(size_t)sr * W + sc];
                    win_exact[(size_t)r * W + c] = old_exact[(size_t)sr * W + sc];
                } else {
                    miss.push_back(r - g.wu + *du); miss.push_back(c - g.wv + *dv); miss.push_back(r * W + c);
                    win_exact[(size_t)r * W + c] = 0;
                }
            }
        const int n_miss = (int)miss.size() / 3;
        MI_REQUIRE(n_miss == H * W - (H - std::abs(deltau)) * (W - std::abs(deltav)), "CrossMIPs: incomplete NCC map in compute_Neighborhood");
        if (n_miss > 0) {
            // the missing entries are covered by 4 x 8 blocks of shifts anchored at the smallest missing (u, v); blocks of one
            // u-row form groups of up to GW blocks (one wave each) that share their staged rows
            int ub = miss[0], vb = miss[1];
            for (int q = 1; q < n_miss; ++q) { ub = imin(ub, miss[3 * q]); vb = imin(vb, miss[3 * q + 1]); }
            std::vector<long long>& keys = ws.host_keys;   // distinct blocks (bu << 20 | bv), sorted
            keys.clear();
            for (int q = 0; q < n_miss; ++q) keys.push_back((long long)((miss[3 * q] - ub) / BU) * (1 << 20) + (miss[3 * q + 1] - vb) / BV);
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            std::vector<int>& lst = ws.host_groups;        // groups {u0, nb, v0[GW]}
            lst.clear();
            std::vector<int>& slot_of = ws.host_slots;     // per block (in `keys` order): group * GW + wave
            slot_of.assign(keys.size(), 0);
            int n_groups = 0;
            for (size_t k = 0; k < keys.size();) {
                const int bu = (int)(keys[k] >> 20), bv0 = (int)(keys[k] & ((1 << 20) - 1));
                const size_t base = lst.size();
                lst.resize(base + 2 + GW, 0);
                int nb = 0;
                while (k < keys.size() && nb < GW && (int)(keys[k] >> 20) == bu && (int)(keys[k] & ((1 << 20) - 1)) - bv0 < GW) {
                    lst[base + 2 + nb] = vb + (int)(keys[k] & ((1 << 20) - 1)) * BV;
                    slot_of[k] = n_groups * GW + nb;
                    ++nb;
                    ++k;
                }
                lst[base] = ub + bu * BU;
                lst[base + 1] = nb;
                for (int w = nb; w < GW; ++w) lst[base + 2 + w] = lst[base + 2 + nb - 1];
                ++n_groups;
            }
            std::vector<int>& ent = ws.host_entries;       // entries {u, v, partial index, output slot}
            ent.clear();
            for (int q = 0; q < n_miss; ++q) {
                const int u = miss[3 * q], v = miss[3 * q + 1];
                const long long key = (long long)((u - ub) / BU) * (1 << 20) + (v - vb) / BV;
                const size_t k = std::lower_bound(keys.begin(), keys.end(), key) - keys.begin();
                ent.push_back(u); ent.push_back(v);
                ent.push_back((slot_of[k] * BU + (u - ub) % BU) * BV + (v - vb) % BV);
                ent.push_back(miss[3 * q + 2]);
            }
            const size_t ints = lst.size() + ent.size();
            if ((size_t)ws.list_cap < ints) {
                MI_HIP(hipStreamSynchronize(s));
                MI_TRY(ws.list.alloc(sizeof(int) * ints));
                ws.list_cap = (int)ints;
            }
            float* d_res = ws.buf.as<float>() + ws.floats;  // H*W result slots reserved behind the maps
            MI_TRY(ws.pin_groups.reserve(sizeof(int) * ints));
            MI_TRY(ws.pin_res.reserve(sizeof(float) * (size_t)H * W));
            std::memcpy(ws.pin_groups.p, lst.data(), sizeof(int) * lst.size());
            std::memcpy(ws.pin_groups.as<int>() + lst.size(), ent.data(), sizeof(int) * ent.size());
            MI_HIP(hipMemcpyAsync(ws.list.p, ws.pin_groups.p, sizeof(int) * ints, hipMemcpyHostToDevice, s));
            MI_TRY(ncc_launch(s, d_base + g.mip1, d_base + g.mip2, g.dimu, g.dimv, g.delayu, g.delayv, ws.v1[plane], ws.v2[plane],
                              ws.list.as<int>(), n_groups, ws.list.as<int>() + lst.size(), n_miss, ws.partial[plane], d_res));
            const float* res = ws.pin_res.as<float>();
            MI_HIP(hipMemcpyAsync(ws.pin_res.p, d_res, sizeof(float) * H * W, hipMemcpyDeviceToHost, s));
            MI_HIP(hipStreamSynchronize(s));
            for (int q = 0; q < n_miss; ++q) win[miss[3 * q + 2]] = res[miss[3 * q + 2]];
        }
        const int cu = *du, cv = *dv;
        MI_TRY(argmax_exact(s, g, plane, d_base, ws, win.data(), H * W, win_exact,
                            [&](int i, int* a, int* b) { *a = i / W - g.wu + cu; *b = i % W - g.wv + cv; }, &ind_max));
    }
    if (exact_out) *exact_out = win_exact;
    if (ind_ref != ind_max) {
        *du += ind_max / W - g.wu;
        *dv += ind_max % W - g.wv;
        *failed = true;
    }
    return MI_OK;
}

// stage 1 of a pair: everything up to the D2H copy of the three NCC maps is enqueued on `s`, nothing is waited for
int pair_enqueue(hipStream_t s, const float* A, const float* B, int dimi, int dimj, const PairPlan& pl, Workspace& ws, TileFmt fmt = TileFmt()) {
    const size_t need = pl.total_floats + pl.res_floats;
    if (ws.buf.bytes < sizeof(float) * need) MI_TRY(ws.buf.alloc(sizeof(float) * need));
    ws.floats = pl.total_floats;
    float* base = ws.buf.as<float>();
    {
        const size_t tmp = sizeof(float) * mips_tmp_floats(pl.dimk, pl.dimi_v, pl.dimj_v);
        if (ws.mip_tmp.bytes < tmp) {
            MI_HIP(hipStreamSynchronize(s));
            MI_TRY(ws.mip_tmp.alloc(tmp));
        }
    }
    MI_TRY(launch_mips(s, A, B, nullptr, 1, 0, pl.dimk, pl.dimi_v, pl.dimj_v, (size_t)dimi * dimj, dimj, pl.ai0, pl.aj0, base + pl.g[0].mip1,
                       base + pl.g[1].mip1, base + pl.g[2].mip1, base + pl.g[0].mip2, base + pl.g[1].mip2, base + pl.g[2].mip2,
                       ws.mip_tmp.as<float>(), nullptr, fmt));
    if (ws.sat.bytes < sizeof(double) * pl.sat_doubles) MI_TRY(ws.sat.alloc(sizeof(double) * pl.sat_doubles));
    for (int m = 0; m < 3; ++m) {
        const PlaneGeom& g = pl.g[m];
        MI_TRY(prepare_plane(s, base + g.mip1, base + g.mip2, g.dimu, g.dimv, base + g.ps1, base + g.ps2, ws.sat.as<double>() + g.sat,
                             &ws.v1[m], &ws.v2[m]));
        MI_TRY(ncc_launch(s, base + g.mip1, base + g.mip2, g.dimu, g.dimv, g.delayu, g.delayv, ws.v1[m], ws.v2[m], nullptr, 0, nullptr, 0,
                          ws.partial[m], base + g.map));
    }
    MI_TRY(ws.pin_maps.reserve(sizeof(float) * pl.map_floats));
    MI_HIP(hipMemcpyAsync(ws.pin_maps.p, base + pl.map_begin, sizeof(float) * pl.map_floats, hipMemcpyDeviceToHost, s));
    return MI_OK;
}

// stage 2: wait for the maps, then the host-side logic (argmax, neighbourhood refinement with its small device
// launches on the same stream, widths, alignment)
int pair_finish(hipStream_t s, int ni, int nj, int side, mi_ncc_params* p, const PairPlan& pl, Workspace& ws, mi_ncc_descr* out) {
    MI_HIP(hipStreamSynchronize(s));
    float* base = ws.buf.as<float>();
    const float* host_maps = ws.pin_maps.as<float>();

    std::vector<float> win[3];
    std::vector<unsigned char> wex[3];
    int du[3], dv[3];
    bool failed[3] = {false, false, false};
    ws.n_exact = 0;
    for (int m = 0; m < 3; ++m)
        MI_TRY(refine_neighbourhood(s, *p, host_maps + (pl.g[m].map - pl.map_begin), pl.g[m], m, base, ws, win[m], &du[m], &dv[m],
                                    &failed[m], &wex[m]));
    // compute_Alignment (compute_funcs.cu:1597-1609).  Every comparison of the width / alignment rules reads entries of the row
    // and the column through the window centre only: when one of them is decided by less than the resolution of the map values
    // those entries are recomputed in the two-pass form and the rules run again on them.
    for (int pass = 0; pass < 2; ++pass) {
        int w1[3], w2[3];
        float peak[3];
        float tight = 3.0e38f;
        for (int m = 0; m < 3; ++m) {
            const PlaneGeom& g = pl.g[m];
            const int rowlen = 2 * g.wv + 1, c = g.wu * rowlen + g.wv;
            peak[m] = win[m][c];
            if (failed[m]) { w1[m] = w2[m] = p->INF_W; continue; }
            w2[m] = peak_half_width(*p, win[m].data(), c, 1, g.wv, g.wv, &tight);
            w1[m] = peak_half_width(*p, win[m].data(), c, rowlen, g.wu, g.wv, &tight);
        }
        combine_axis(*p, out, 0, du[0], peak[0], w1[0], du[1], peak[1], w1[1], &tight);  // V: xy rows, xz rows
        combine_axis(*p, out, 1, dv[0], peak[0], w2[0], du[2], peak[2], w1[2], &tight);  // H: xy cols, yz rows
        combine_axis(*p, out, 2, dv[1], peak[1], w2[1], dv[2], peak[2], w2[2], &tight);  // D: xz cols, yz cols
        if (pass == 1 || !(tight < ncc_margin())) break;
        for (int m = 0; m < 3; ++m) {
            const PlaneGeom& g = pl.g[m];
            const int H = 2 * g.wu + 1, W = 2 * g.wv + 1;
            std::vector<int> uv, idx;
            for (int r = 0; r < H; ++r)
                for (int c = 0; c < W; ++c)
                    if ((r == g.wu || c == g.wv) && !wex[m][(size_t)r * W + c]) {
                        uv.push_back(r - g.wu + du[m]); uv.push_back(c - g.wv + dv[m]); idx.push_back(r * W + c);
                    }
            std::vector<float> val;
            MI_TRY(exact_entries(s, g, m, base, ws, uv, val));
            for (size_t q = 0; q < idx.size(); ++q) { win[m][idx[q]] = val[q]; wex[m][idx[q]] = 1; }
        }
    }
    if (side == MI_NORTH_SOUTH) out->coord[0] += ni; else out->coord[1] += nj;  // libcrossmips.cpp:483-486
    return MI_OK;
}

}  // namespace

namespace mi {

int pair_direct(hipStream_t s, const float* A, const float* B, int dimk, int dimi, int dimj, int ni, int nj, int delayk, int delayi, int delayj,
                int side, mi_ncc_params* p, mi_ncc_descr* out) {
    PairPlan pl;
    MI_TRY(plan_pair(dimk, dimi, dimj, 0, ni, nj, delayk, delayi, delayj, side, p, pl));
    Workspace ws;
    MI_TRY(pair_enqueue(s, A, B, dimi, dimj, pl, ws));
    ncc_count(1, 1);
    return pair_finish(s, ni, nj, side, p, pl, ws, out);
}

int pair_map(hipStream_t s, const float* mip1, const float* mip2, int dimu, int dimv, int delayu, int delayv, float* map) {
    const int nt = (dimu / TILE) * (dimv / TILE);
    DevBuf ps, sat;
    MI_TRY(ps.alloc(sizeof(float) * 2 * (size_t)(nt > 0 ? nt : 1)));
    MI_TRY(sat.alloc(sizeof(double) * SatLayout(dimu, dimv).total));
    SatView v1, v2;
    MI_TRY(prepare_plane(s, mip1, mip2, dimu, dimv, ps.as<float>(), ps.as<float>() + (nt > 0 ? nt : 0), sat.as<double>(), &v1, &v2));
    DevBuf partial;
    MI_TRY(ncc_launch(s, mip1, mip2, dimu, dimv, delayu, delayv, v1, v2, nullptr, 0, nullptr, 0, partial, map));
    MI_HIP(hipStreamSynchronize(s));  // ps / sat / partial die at scope exit
    return MI_OK;
}

struct PairSlot {
    int dev = 0;
    Workspace ws;
    hipStream_t s = nullptr;
    ~PairSlot() {
        if (s) {
            (void)hipSetDevice(dev);
            (void)hipStreamDestroy(s);
        }
    }
};
// never destroyed: at process exit the HIP runtime may already be gone
static std::mutex& g_slot_mu = *new std::mutex;
static std::vector<PairSlotPtr>& g_slots = *new std::vector<PairSlotPtr>;
void PairSlotDelete::operator()(PairSlot* slot) const { delete slot; }

PairSlotPtr take_pair_slot(int dev) {
    {
        std::lock_guard<std::mutex> g(g_slot_mu);
        for (size_t i = 0; i < g_slots.size(); ++i)
            if (g_slots[i]->dev == dev) {
                PairSlotPtr r = std::move(g_slots[i]);
                g_slots.erase(g_slots.begin() + i);
                return r;
            }
    }
    PairSlotPtr r(new (std::nothrow) PairSlot);
    if (!r) return r;
    r->dev = dev;
    if (hipStreamCreateWithFlags(&r->s, hipStreamNonBlocking) != hipSuccess) {
        r->s = nullptr;
        r.reset();
    }
    return r;
}

void give_pair_slot(PairSlotPtr r) {
    if (!r) return;
    std::lock_guard<std::mutex> g(g_slot_mu);
    if (g_slots.size() < 16) g_slots.push_back(std::move(r));  // beyond that the slot is simply destroyed
}

hipStream_t pair_slot_stream(const PairSlot& slot) { return slot.s; }

int pair_enqueue(PairSlot& slot, const float* A, const float* B, int dimi, int dimj, const PairPlan& pl, TileFmt fmt) {
    return pair_enqueue(slot.s, A, B, dimi, dimj, pl, slot.ws, fmt);
}
int pair_finish(PairSlot& slot, int ni, int nj, int side, mi_ncc_params* p, const PairPlan& pl, mi_ncc_descr* out) {
    return pair_finish(slot.s, ni, nj, side, p, pl, slot.ws, out);
}

// the cached pair slots of a device (-1: all) are destroyed; their buffers return to the pool (mi_release_cached_memory)
void ncc_drop_cached_slots(int dev) {
    std::vector<PairSlotPtr> drop;
    {
        std::lock_guard<std::mutex> g(g_slot_mu);
        for (size_t i = 0; i < g_slots.size();)
            if (dev < 0 || g_slots[i]->dev == dev) { drop.push_back(std::move(g_slots[i])); g_slots.erase(g_slots.begin() + i); }
            else ++i;
    }
    ncc_lag_drop_cached(dev);
}

}  // namespace mi
