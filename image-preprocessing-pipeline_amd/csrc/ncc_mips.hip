// The six MIPs of the overlap views of tile pairs (compute_3_MIPs, libcrossmips.cpp:502-521) in one streaming pass: the kernels
// of the three sample formats, their launch geometry, the one launcher every caller goes through and the timed launch.
#include <cstdlib>

#include "ncc_internal.h"

using namespace mi;

namespace {

__device__ __forceinline__ void atomic_max_nonneg(float* addr, float v) {
    atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
}

// Maxima of 16 per-lane values over the 64 lanes of a wave, all 16 rows at once (transpose reduction): in each of four steps a lane
// hands one half of its rows to the partner lane^m and keeps the other half, taking the maximum with what it receives -- 8 + 4 +
// 2 + 1 exchanges instead of 16 x 4 -- then two more exchanges merge the four 16-lane groups.  Returns, in EVERY lane, the maximum
// of row rows_of_lane(lane) = bit-reversal of (lane & 15).  Values >= 0.
__device__ __forceinline__ int row_of_lane(int lane) { return ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3); }
__device__ __forceinline__ float rows_max16(const float (&v)[MIP_ROWS], int lane) {
    float w[8];
    {   // partner lane ^ 1 (DPP quad_perm [1,0,3,2])
        const bool up = lane & 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float mine = up ? v[i + 8] : v[i], send = up ? v[i] : v[i + 8];
            const float recv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(send), 0xB1, 0xf, 0xf, false));
            w[i] = fmaxf(mine, recv);
        }
    }
    {   // partner lane ^ 2 (DPP quad_perm [2,3,0,1])
        const bool up = lane & 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float mine = up ? w[i + 4] : w[i], send = up ? w[i] : w[i + 4];
            const float recv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(send), 0x4E, 0xf, 0xf, false));
            w[i] = fmaxf(mine, recv);
        }
    }
    {
        const bool up = lane & 4;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float mine = up ? w[i + 2] : w[i], send = up ? w[i] : w[i + 2];
            w[i] = fmaxf(mine, __shfl_xor(send, 4, 64));
        }
    }
    {
        const bool up = lane & 8;
        const float mine = up ? w[1] : w[0], send = up ? w[0] : w[1];
        w[0] = fmaxf(mine, __shfl_xor(send, 8, 64));
    }
    w[0] = fmaxf(w[0], __shfl_xor(w[0], 16, 64));
    w[0] = fmaxf(w[0], __shfl_xor(w[0], 32, 64));
    return w[0];
}

// view(k,i,j) = vol[k*slice + (i+i0)*pitch + (j+j0)]; blockIdx.z = 2 * pair + (0: A, 1: B).  A batch hands the tile pointers
// over as a device table (tab[2 * pair + which]); every output array of pair q sits q * pstride floats behind pair 0's.
// Since round 5 this is the pass for stacks DEEPER than 4 * MIP_KPW slices only (k_mips5 below takes the others): partial row / column
// maxima per band and column block in `yz_tmp` / `xz_tmp`, reduced by k_mips_yz / k_mips_xz.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_mips(const float* __restrict__ A, const float* __restrict__ B, const float* const* __restrict__ tab,
                                               size_t pstride, int dimk, int dimi_v, int dimj_v,
                                               size_t slice, int pitch, int ai0, int aj0, float* __restrict__ xy1, float* __restrict__ xz1,
                                               float* __restrict__ yz1, float* __restrict__ xy2, float* __restrict__ xz2,
                                               float* __restrict__ yz2, float* __restrict__ yz_tmp, float* __restrict__ xz_tmp, int knock,
                                               float* __restrict__ xyT, size_t tstride) {
    // xyT (batched pipeline, views whose rows are the long axis): a second, TRANSPOSED copy of the xy MIP -- [j][i], MIP `second` of
    // pair q at xyT + (2 q + second) * tstride -- so that the lag transform along i reads contiguous lines (as a strided gather
    // it took 0.46 instead of 0.24 ms per 56 pairs: every lane of a load another 128-byte line)
    // (knock: measurement aid, MI_NCC_MIPS_KNOCK -- 1: no xz maxima, 2: no yz maxima, 4: no xy store)
    // a work-group owns a 16-row x 64-column patch of the view; its four waves share the slices (wave w: k = w, w + 4, ...),
    // so a patch keeps four times as many loads in flight as one wave walking all slices
    extern __shared__ float xzp[];  // [band][MIP_ROWS][dimk] row maxima of the work-group's patches (xz_tmp != nullptr)
    const bool second = blockIdx.z & 1;
    const size_t poff = (size_t)(blockIdx.z >> 1) * pstride;
    const float* vol = tab ? tab[blockIdx.z] : (second ? B : A);
    if (!second) vol += (size_t)ai0 * pitch + aj0;
    float* xy = (second ? xy2 : xy1) + poff;
    float* xz = (second ? xz2 : xz1) + poff;
    (void)yz1; (void)yz2;  // written by k_mips_yz
    // (the wave index as a scalar: row addresses are then scalar bases + one per-lane offset instead of 16 address pairs)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // column blocks start on 256-byte boundaries of the TILE rows, not of the view (the first tile's view of a west-east pair
    // starts at column 1741 of 2048: blocks laid out from there shared their first and last 128-byte lines with their neighbours,
    // three lines fetched for two used); the first block is then the partial one
    const int jshift = second ? 0 : (aj0 & 63);
    const int j = (int)blockIdx.x * 64 + lane - jshift;
    const bool live = j >= 0 && j < dimj_v;
    // A work-group walks MIP_NB consecutive row bands (stacks of up to 4 * MIP_KPW slices): the column maxima of the slices a wave
    // owns stay with it across the bands (in LDS, one column per lane and slice of the wave) and go to yz_tmp ONCE per band group
    // -- a quarter of the partial maxima that k_mips_yz has to read back.  Deeper stacks write them per band (nb = 1 below).
    // NOTHING is stored to memory before the last slice has been requested: loads and stores of a wave return in order, so a
    // store in the middle of the stream -- the xy rows of a band, its xz maxima -- held up the loads requested behind it until
    // its acknowledgement came back, and the other three waves at the next barrier (switching the xy store off saved 11 % of
    // the pass although it is 3 % of its bytes: profiles/r03_mips_knock.txt).  The xy maxima of a band are merged across the
    // waves with LDS atomics, the xz maxima of all bands wait in LDS: the band loop has no barrier left.
    const bool keep = dimk <= 4 * MIP_KPW;
    const int nb = keep ? MIP_NB : 1;
    __shared__ float xyb[MIP_NB][MIP_ROWS][64];
    __shared__ float cacc[4][MIP_KPW][64];
    float* colacc = &cacc[wave][0][lane];
    if (keep) {
#pragma unroll
        for (int q = 0; q < MIP_KPW; ++q) colacc[q * 64] = 0.0f;
    }
    for (int e = threadIdx.x; e < MIP_NB * MIP_ROWS * 64; e += 256) (&xyb[0][0][0])[e] = 0.0f;
    const int ib0 = __builtin_amdgcn_readfirstlane((int)blockIdx.y * nb * MIP_ROWS);
    const int nbv = min(nb, (dimi_v - ib0 + MIP_ROWS - 1) / MIP_ROWS);  // bands of this work-group inside the view (>= 1)
    // the wave's slices of all its bands form one sequence: the next slice -- of this band or the first of the next -- is requested
    // before the current one is reduced
    float v[MIP_ROWS], vn[MIP_ROWS];
    // Every load is unconditional: lanes outside the view read its nearest column, rows past the last band its last row -- a
    // maximum does not change when a sample is taken twice (the partial results of such lanes are never stored).  Predicated
    // loads cost a branch around each of the 16 rows of a slice (`s_cbranch_execz`), in the inner loop of a memory-bound pass.
    const int jc = min(max(j, 0), dimj_v - 1);
    auto load_slice = [&](int bb, int k, float (&dst)[MIP_ROWS]) {
        const int i0 = ib0 + bb * MIP_ROWS, last = min(MIP_ROWS, dimi_v - i0) - 1;
        // (a GLOBAL pointer, said explicitly: the tile pointer comes out of a table in memory, and what the compiler cannot prove
        // global it reads with FLAT loads -- which count against the LDS counter as well and are waited for with vmcnt(0).
        // Measured on one box, same run: 1.87 / 1.81 ms with global loads and counted waits, 1.90 / 1.82 ms with FLAT loads -- the
        // pass is not bound by what a wave keeps in flight (three or four waves per SIMD are the optimum, five or two are slower))
        typedef const float __attribute__((address_space(1))) gfloat;
        gfloat* p = (gfloat*)(vol + (size_t)k * slice + (size_t)i0 * pitch);  // wave-uniform
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) dst[r] = (p + (size_t)min(r, last) * pitch)[jc];
    };
    if (wave < dimk) load_slice(0, wave, v);
    __syncthreads();  // (xyb is zero)
#pragma unroll 1
    for (int b = 0; b < nbv; ++b) {
        const int i0 = ib0 + b * MIP_ROWS;  // (scalar: so are the row addresses)
        const int rows = min(MIP_ROWS, dimi_v - i0);
        float best[MIP_ROWS];
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) best[r] = 0.0f;
        // one slice of the wave, held in `cur`; the wave's next one is requested into `nxt` first.  Returns the column maximum.
        // (The two buffers swap roles from slice to slice -- the loops below take two slices per trip.  With one loop body and a
        // copy nxt -> cur at its end the compiler had to wait for the slice it had just requested: `s_waitcnt vmcnt(0)` in every
        // step, no load in flight while a slice was reduced.)
        auto slice_step = [&](int k, float (&cur)[MIP_ROWS], float (&nxt)[MIP_ROWS]) {
            const bool wrap = k + 4 >= dimk;  // (wave-uniform)
            const int kn = __builtin_amdgcn_readfirstlane(wrap ? wave : k + 4), bn = __builtin_amdgcn_readfirstlane(wrap ? b + 1 : b);
            // (behind the work-group's last slice there is nothing to fetch: the first slice of its last band is read once more --
            // one slice in 128 -- so that the number of loads in flight is the same in every step)
            if (bn < nbv) load_slice(bn, kn, nxt);
            float colmax = 0.0f;
#pragma unroll
            for (int r = 0; r < MIP_ROWS; ++r) {
                best[r] = fmaxf(best[r], cur[r]);
                colmax = fmaxf(colmax, cur[r]);
            }
            // xz: the 16 row maxima over the 64 columns of the patch, per patch through LDS into xz_tmp[tile][column block][i][k]
            // (k_mips_xz takes the maximum over the column blocks); as atomics on the MIP they were 655 thousand single-lane
            // atomics per C5 pair, as 16 separate wave reductions 96 DPP steps per slice
            if (!(knock & 1)) {
                const float rowmax = rows_max16(cur, lane);
                const int r = row_of_lane(lane);
                if (lane < 16) {
                    if (xz_tmp) xzp[(b * MIP_ROWS + r) * dimk + k] = rowmax;
                    else if (r < rows) atomic_max_nonneg(&xz[(size_t)(i0 + r) * dimk + k], rowmax);
                }
            }
            return (knock & 2) ? 0.0f : colmax;
        };
        // yz: the column maxima of this band (group) go to yz_tmp[tile][group][k][j] (unit-stride stores); k_mips_yz takes the
        // maximum over the groups -- 2.6 million atomics per pair on the yz MIPs cost more than the whole streaming pass
        auto yz_out = [&](int k, int q, float colmax) {
            if (keep) colacc[q * 64] = fmaxf(colacc[q * 64], colmax);
            else if (live) yz_tmp[(((size_t)blockIdx.z * gridDim.y + blockIdx.y) * dimk + k) * dimj_v + j] = colmax;
        };
        int k = wave, q = 0;
#pragma unroll 1
        for (; k + 4 < dimk; k += 8, q += 2) {
            yz_out(k, q, slice_step(k, v, vn));
            yz_out(k + 4, q + 1, slice_step(k + 4, vn, v));
        }
        if (k < dimk) {  // an odd number of slices: the next band's first slice has arrived in the other buffer
            yz_out(k, q, slice_step(k, v, vn));
#pragma unroll
            for (int r = 0; r < MIP_ROWS; ++r) v[r] = vn[r];
        }
        // xy: maximum over the four waves' slices
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) atomic_max_nonneg(&xyb[b][r][lane], best[r]);
    }
    __syncthreads();
    if (wave < nbv && live && !(knock & 4)) {  // wave b stores band b
        const int i0 = ib0 + wave * MIP_ROWS, rows = min(MIP_ROWS, dimi_v - i0);
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r)
            if (r < rows) xy[(size_t)(i0 + r) * dimj_v + j] = xyb[wave][r][lane];
    }
    if (xyT) {  // column c of the patch = 16 nbv consecutive floats of line j of the transposed copy: the lanes run along i
        float* t = xyT + (size_t)blockIdx.z * tstride;
        const int i = ib0 + lane;
        if (lane < nbv * MIP_ROWS && i < dimi_v)
            for (int c = wave; c < 64; c += 4) {
                const int jc_ = (int)blockIdx.x * 64 + c - jshift;
                if (jc_ >= 0 && jc_ < dimj_v) t[(size_t)jc_ * dimi_v + i] = xyb[lane >> 4][lane & 15][c];
            }
    }
    if (xz_tmp) {  // the rows of all bands * dimk: contiguous floats
        float* dst = xz_tmp + (((size_t)blockIdx.z * gridDim.x + blockIdx.x) * dimi_v + ib0) * dimk;
        const int total = min(nbv * MIP_ROWS, dimi_v - ib0) * dimk;
        for (int e = threadIdx.x; e < total; e += 256) dst[e] = xzp[e];
    }
    if (keep && live) {
#pragma unroll
        for (int q = 0; q < MIP_KPW; ++q) {
            const int k = wave + 4 * q;
            if (k < dimk) yz_tmp[(((size_t)blockIdx.z * gridDim.y + blockIdx.y) * dimk + k) * dimj_v + j] = colacc[q * 64];
        }
    }
}

// ---- k_mips5: the float pass for stacks of up to 4 * MIP_KPW slices (every C5-like stack), round-5 form of k_mips<true>.  Same
// patches, same slice pipeline (a work-group owns 16 rows x 64 columns x MIP_NB bands, its four waves share the slices, the next
// slice is requested before the current one is reduced, nothing is stored before the last load).  What changed:
//  * addressing: BUFFER loads -- the slice's first row is the descriptor base (wave-uniform, five scalar instructions per slice), the 16
//    row offsets of the wave's band wait in SGPRs (recomputed when the band changes, once per 8 slices) and go into the instruction's
//    scalar offset, the lane's column into its vector offset.  k_mips<true> rebuilt 16 64-bit row addresses per slice: 92 scalar
//    instructions per slice against 155 vector ones (profiles/r04_ncc_sq_counters.txt).
//  * no partial maxima in memory: the column maxima (yz) and row maxima (xz) a work-group has gathered in LDS are merged into the
//    MIPs themselves with integer atomic maxima (non-negative floats order like their bit patterns), 256 contiguous bytes per wave
//    instruction, ONCE per work-group -- 0.29 GB per 56-pair launch were written as yz_tmp / xz_tmp and read back by k_mips_yz /
//    k_mips_xz.  The MIPs must be zero when the pass starts (k_mips_zero).
//  * LDS images without bank conflicts: the row maxima at a stride of 33 words (16 lanes stored at a stride of dimk = 32 words: one
//    bank), the xy rows and column maxima at 65 (the transposed copy read them at a stride of 64 words: one bank for 64 lanes).
constexpr int MIP5_XS = 4 * MIP_KPW + 1;  // words per row of the xz image
__global__ __launch_bounds__(256) void k_mips_zero(size_t pstride, size_t n_xz, size_t n_yz, float* __restrict__ xz1, float* __restrict__ yz1,
                                                   float* __restrict__ xz2, float* __restrict__ yz2) {
    const size_t poff = (size_t)(blockIdx.y >> 1) * pstride;
    float* xz = ((blockIdx.y & 1) ? xz2 : xz1) + poff;
    float* yz = ((blockIdx.y & 1) ? yz2 : yz1) + poff;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n_xz + n_yz; e += (size_t)gridDim.x * 256) {
        if (e < n_xz) xz[e] = 0.0f;
        else yz[e - n_xz] = 0.0f;
    }
}

template <int WPE>  // waves per SIMD = work-groups per compute unit
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_mips5(
    const float* __restrict__ A, const float* __restrict__ B, const float* const* __restrict__ tab, size_t pstride, int dimk, int dimi_v, int dimj_v,
    size_t slice, int pitch, int ai0, int aj0, float* __restrict__ xy1, float* __restrict__ xz1, float* __restrict__ yz1, float* __restrict__ xy2,
    float* __restrict__ xz2, float* __restrict__ yz2, int knock, float* __restrict__ xyT, size_t tstride, int cblocks, int groups, int nviews, int remap) {
    // Patch of this work-group: column block bx, band group by, view bz, from a one-dimensional grid.  remap: work-groups b, b + 8,
    // b + 16, ... -- they run on one XCD and start together -- take the `cblocks` column blocks of ONE group of rows: their xy rows
    // are pieces of the same lines and of the same DRAM pages, and what one L2 collects it writes back as whole runs.
    int bx, by, bz;
    {
        const int id = (int)blockIdx.x;
        int rg;
        if (remap) {
            const int s_ = id >> 3;
            bx = s_ % cblocks;
            rg = (s_ / cblocks) * 8 + (id & 7);
        } else {
            bx = id % cblocks;
            rg = id / cblocks;
        }
        by = rg % groups;
        bz = rg / groups;
        if (bz >= nviews) return;   // (the grid is padded to whole groups of 8 row groups)
    }
    __shared__ float xyb[MIP_NB][MIP_ROWS][65];        // xy maxima of the bands (merged across the waves with LDS atomics)
    __shared__ float cacc[4][MIP_KPW][65];             // column maxima of the wave's slices over all bands: slice k = wave + 4 q
    __shared__ float xzp[MIP_NB * MIP_ROWS][MIP5_XS];  // row maxima over the patch's 64 columns
    const bool second = bz & 1;
    const size_t poff = (size_t)(bz >> 1) * pstride;
    const float* vol = tab ? tab[bz] : (second ? B : A);
    if (!second) vol += (size_t)ai0 * pitch + aj0;
    float* xy = (second ? xy2 : xy1) + poff;
    float* xz = (second ? xz2 : xz1) + poff;
    float* yz = (second ? yz2 : yz1) + poff;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int jshift = second ? 0 : (aj0 & 63);  // column blocks start on 256-byte boundaries of the TILE rows (see k_mips)
    const int j = bx * 64 + lane - jshift;
    const bool live = j >= 0 && j < dimj_v;
    float* colacc = &cacc[wave][0][lane];
#pragma unroll
    for (int q = 0; q < MIP_KPW; ++q) colacc[q * 65] = 0.0f;
    for (int e = threadIdx.x; e < MIP_NB * MIP_ROWS * 65; e += 256) (&xyb[0][0][0])[e] = 0.0f;
    const int ib0 = __builtin_amdgcn_readfirstlane(by * MIP_NB * MIP_ROWS);
    const int nbv = min(MIP_NB, (dimi_v - ib0 + MIP_ROWS - 1) / MIP_ROWS);  // bands of this work-group inside the view (>= 1)
    float v[MIP_ROWS], vn[MIP_ROWS];
    // every load is unconditional (see k_mips): lanes outside the view read its nearest column, rows past the last band its last row
    const int voff = 4 * min(max(j, 0), dimj_v - 1);
    const int pitch4 = 4 * pitch;
    int ro[MIP_ROWS];  // byte offsets of the 16 rows of the band being REQUESTED from the first row of its slice (scalars)
    auto set_band = [&](int bb) {
        const int last = min(MIP_ROWS, dimi_v - (ib0 + bb * MIP_ROWS)) - 1;
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) ro[r] = __builtin_amdgcn_readfirstlane(min(r, last) * pitch4);
    };
    auto load_slice = [&](int bb, int k, float (&dst)[MIP_ROWS]) {
        const float* p = vol + (size_t)k * slice + (size_t)(ib0 + bb * MIP_ROWS) * pitch;  // wave-uniform
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) dst[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, ro[r], 0));
    };
    set_band(0);
    if (wave < dimk) load_slice(0, wave, v);
    __syncthreads();  // (the LDS images are zero)
#pragma unroll 1
    for (int b = 0; b < nbv; ++b) {
        float best[MIP_ROWS];
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) best[r] = 0.0f;
        auto slice_step = [&](int k, int q, float (&cur)[MIP_ROWS], float (&nxt)[MIP_ROWS]) {
            const bool wrap = k + 4 >= dimk;  // (wave-uniform)
            const int kn = __builtin_amdgcn_readfirstlane(wrap ? wave : k + 4);
            // (behind the work-group's last slice there is nothing to fetch: the first slice of its last band is read once more --
            // one slice in 128 -- so that the number of loads in flight is the same in every step)
            const int bn = __builtin_amdgcn_readfirstlane(wrap ? min(b + 1, nbv - 1) : b);
            if (wrap) set_band(bn);
            load_slice(bn, kn, nxt);
            float colmax = 0.0f;
#pragma unroll
            for (int r = 0; r < MIP_ROWS; ++r) {
                best[r] = fmaxf(best[r], cur[r]);
                colmax = fmaxf(colmax, cur[r]);
            }
            if (!(knock & 1)) {
                const float rowmax = rows_max16(cur, lane);
                if (lane < 16) xzp[b * MIP_ROWS + row_of_lane(lane)][k] = rowmax;
            }
            if (!(knock & 2)) colacc[q * 65] = fmaxf(colacc[q * 65], colmax);
        };
        int k = wave, q = 0;
#pragma unroll 1
        for (; k + 4 < dimk; k += 8, q += 2) {
            slice_step(k, q, v, vn);
            slice_step(k + 4, q + 1, vn, v);
        }
        if (k < dimk) {  // an odd number of slices: the next band's first slice has arrived in the other buffer
            slice_step(k, q, v, vn);
#pragma unroll
            for (int r = 0; r < MIP_ROWS; ++r) v[r] = vn[r];
        }
        // xy: maximum over the four waves' slices
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) atomic_max_nonneg(&xyb[b][r][lane], best[r]);
    }
    __syncthreads();
    if (wave < nbv && live && !(knock & 4)) {  // wave b stores band b
        const int i0 = ib0 + wave * MIP_ROWS, rows = min(MIP_ROWS, dimi_v - i0);
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r)
            if (r < rows) xy[(size_t)(i0 + r) * dimj_v + j] = xyb[wave][r][lane];
    }
    if (xyT) {  // column c of the patch = 16 nbv consecutive floats of line j of the transposed copy: the lanes run along i
        float* t = xyT + (size_t)bz * tstride;
        const int i = ib0 + lane;
        if (lane < nbv * MIP_ROWS && i < dimi_v)
            for (int c = wave; c < 64; c += 4) {
                const int jc_ = bx * 64 + c - jshift;
                if (jc_ >= 0 && jc_ < dimj_v) t[(size_t)jc_ * dimi_v + i] = xyb[lane >> 4][lane & 15][c];
            }
    }
    // xz[i][k] and yz[j][k]: a half-wave takes the dimk slices of one row / column -- 128 contiguous bytes of the MIP when dimk = 32
    {
        const int k = threadIdx.x & 31;
        const int rows = min(nbv * MIP_ROWS, dimi_v - ib0);
        if (k < dimk && !(knock & 8)) {
#pragma unroll
            for (int it = 0; it < MIP_NB * MIP_ROWS / 8; ++it) {
                const int r = (threadIdx.x >> 5) + 8 * it;
                if (r < rows) atomic_max_nonneg(&xz[(size_t)(ib0 + r) * dimk + k], xzp[r][k]);
            }
            const float* ck = &cacc[k & 3][k >> 2][0];
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int c = (threadIdx.x >> 5) + 8 * it, jc_ = bx * 64 + c - jshift;
                if (jc_ >= 0 && jc_ < dimj_v) atomic_max_nonneg(&yz[(size_t)jc_ * dimk + k], ck[c]);
            }
        }
    }
}

// ---- 16-bit tiles.  TeraStitcher turns the 8 / 16-bit samples of its TIFF tiles into floats in [0, 1] when it loads them (value /
// 255 or / 65535, tiff2D.cpp:606-610) and compute_3_MIPs reads those; the division is monotonic, so the MIPs of the floats are the
// divided MIPs of the integers, bit for bit.  k_mips_int reads the tiles as they are stored -- half or a quarter of the bytes of the pass that
// dominates a batch -- and a lane takes TWO neighbouring columns as one packed 32-bit value: running maxima, column maxima and the
// transpose reduction of the row maxima work on both halves at once (v_pk_max_u16), i.e. the same instructions as for one float
// column move twice the voxels.  Only the results are divided (IEEE division: what numpy's float32 division gives the host mirror).
typedef unsigned short mi_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(mi_u16x2, a), __builtin_bit_cast(mi_u16x2, b)));
}
// rows_max16 for packed pairs: returns, in every lane, the packed maxima of row row_of_lane(lane) over the 64 lanes
__device__ __forceinline__ unsigned rows_max16_pk(const unsigned (&v)[MIP_ROWS], int lane) {
    unsigned w[8];
    {
        const bool up = lane & 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned mine = up ? v[i + 8] : v[i], send = up ? v[i] : v[i + 8];
            w[i] = pk_max_u16(mine, (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0xB1, 0xf, 0xf, false));
        }
    }
    {
        const bool up = lane & 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned mine = up ? w[i + 4] : w[i], send = up ? w[i] : w[i + 4];
            w[i] = pk_max_u16(mine, (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0x4E, 0xf, 0xf, false));
        }
    }
    {
        const bool up = lane & 4;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned mine = up ? w[i + 2] : w[i], send = up ? w[i] : w[i + 2];
            w[i] = pk_max_u16(mine, (unsigned)__shfl_xor((int)send, 4, 64));
        }
    }
    {
        const bool up = lane & 8;
        const unsigned mine = up ? w[1] : w[0], send = up ? w[0] : w[1];
        w[0] = pk_max_u16(mine, (unsigned)__shfl_xor((int)send, 8, 64));
    }
    w[0] = pk_max_u16(w[0], (unsigned)__shfl_xor((int)w[0], 16, 64));
    w[0] = pk_max_u16(w[0], (unsigned)__shfl_xor((int)w[0], 32, 64));
    return w[0];
}

// The views as in k_mips (grid z = 2 * pair + tile, tab / A / B, ai0 / aj0 of the first tile).  BYTES = 2: a lane's word holds two
// columns, a work-group owns 16 rows x 128 columns per band and walks MIP_NB bands.  BYTES = 1: four columns per word, taken apart
// into two packed pairs (even / odd bytes) that go through the same packed instructions -- 16 rows x 256 columns per band, half
// as many bands per work-group (the xy maxima of its bands wait in LDS, one word per column).  Words are aligned to the TILE rows
// (dimj and the slice size a multiple of 4 / BYTES samples: 32-bit loads).  Stacks of up to 4 * MIP_KPW slices.
// `scale`: 65535 for 16-bit, 255 for 8-bit samples (tiff2D.cpp:606-610).
template <int BYTES>
struct IntTiles {
    static constexpr int P = BYTES == 2 ? 1 : 2;  // packed pairs per word
    static constexpr int C = 2 * P;               // columns per lane
    static constexpr int NB = MIP_NB / P;         // row bands per work-group
    static constexpr int W = 64 * C;              // columns per work-group
};
template <int BYTES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_mips_int(
    const unsigned char* __restrict__ A, const unsigned char* __restrict__ B, const unsigned char* const* __restrict__ tab, size_t pstride, int dimk,
    int dimi_v, int dimj_v, size_t slice, int pitch, int ai0, int aj0, float scale, float* __restrict__ xy1, float* __restrict__ xz1,
    float* __restrict__ yz1, float* __restrict__ xy2, float* __restrict__ xz2, float* __restrict__ yz2, float* __restrict__ xyT, size_t tstride,
    int cblocks, int groups, int nviews) {
    int bx, by, bz;   // column block, band group, view: the column blocks of one group of rows on ONE XCD (see k_mips5)
    {
        const int id = (int)blockIdx.x, s_ = id >> 3;
        bx = s_ % cblocks;
        const int rg = (s_ / cblocks) * 8 + (id & 7);
        by = rg % groups;
        bz = rg / groups;
        if (bz >= nviews) return;   // (the grid is padded to whole groups of 8 row groups)
    }
    // (round 5, as k_mips5: buffer loads with the band's row offsets in SGPRs; row and column maxima merged into the zeroed MIPs with
    // atomic maxima of the DIVIDED values -- the division is monotonic --, LDS images at odd strides)
    using G = IntTiles<BYTES>;
    constexpr int P = G::P, C = G::C, NB = G::NB;
    constexpr int XW = 64 * C + 1;                     // words per row of the xy image
    constexpr int CS = P * 64 + 1;                     // words per (wave, q) row of the column maxima
    __shared__ float xzp[NB * MIP_ROWS][MIP5_XS];      // row maxima, already divided
    __shared__ unsigned xyb[NB][MIP_ROWS][XW];         // xy maxima of the bands, one word per column (merged with LDS atomics)
    __shared__ unsigned cacc[4 * MIP_KPW][CS];         // packed column maxima of the wave's slices: row wave * MIP_KPW + q, word p * 64 + lane
    const bool second = bz & 1;
    const size_t poff = (size_t)(bz >> 1) * pstride;
    const unsigned char* vol = tab ? tab[bz] : (second ? B : A);
    if (!second) vol += (size_t)ai0 * pitch * BYTES;
    float* xy = (second ? xy2 : xy1) + poff;
    float* xz = (second ? xz2 : xz1) + poff;
    float* yz = (second ? yz2 : yz1) + poff;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int a0 = second ? 0 : aj0, alast = a0 + dimj_v - 1;          // first / last tile column of the view
    const int cj = (a0 & ~(G::W - 1)) + bx * G::W + C * lane;  // tile column of the lane's word
    const int jv0 = cj - a0;                                             // view column of its first sample
    // every load is unconditional (see k_mips): a word outside the view reads the nearest word inside, a word that straddles the
    // view's edge takes its nearest inside sample in place of the outside ones (byte permute with a lane-constant selector)
    const int cc = min(max(cj, a0 & ~(C - 1)), alast & ~(C - 1));
    unsigned sel;
    if (BYTES == 2) {
        sel = cc < a0 ? 0x03020302u : (cc + 1 > alast ? 0x01000100u : 0x03020100u);
    } else {
        const int f = max(0, a0 - cc), l = min(3, alast - cc);
        sel = 0;
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) sel |= (unsigned)min(max(bb, f), l) << (8 * bb);
    }
    // column c of the lane's word sits in half h of packed pair p
    auto col_of = [](int p, int h) { return BYTES == 2 ? h : 2 * h + p; };
    unsigned* colacc = &cacc[wave * MIP_KPW][lane];  // [q][p]: q * CS + p * 64
#pragma unroll
    for (int q = 0; q < MIP_KPW; ++q)
#pragma unroll
        for (int p = 0; p < P; ++p) colacc[q * CS + p * 64] = 0u;
    for (int e = threadIdx.x; e < NB * MIP_ROWS * XW; e += 256) (&xyb[0][0][0])[e] = 0u;
    const int ib0 = __builtin_amdgcn_readfirstlane(by * NB * MIP_ROWS);
    const int nbv = min(NB, (dimi_v - ib0 + MIP_ROWS - 1) / MIP_ROWS);
    unsigned v[MIP_ROWS], vn[MIP_ROWS];
    const int voff = cc * BYTES, pitchb = pitch * BYTES;
    int ro[MIP_ROWS];  // byte offsets of the 16 rows of the band being requested from the first row of its slice (scalars)
    auto set_band = [&](int bb) {
        const int last = min(MIP_ROWS, dimi_v - (ib0 + bb * MIP_ROWS)) - 1;
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) ro[r] = __builtin_amdgcn_readfirstlane(min(r, last) * pitchb);
    };
    auto load_slice = [&](int bb, int k, unsigned (&dst)[MIP_ROWS]) {
        const unsigned char* p = vol + ((size_t)k * slice + (size_t)(ib0 + bb * MIP_ROWS) * pitch) * BYTES;  // wave-uniform
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r) dst[r] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, ro[r], 0);
    };
    set_band(0);
    if (wave < dimk) load_slice(0, wave, v);
    __syncthreads();  // (the LDS images are zero)
#pragma unroll 1
    for (int b = 0; b < nbv; ++b) {
        unsigned best[P][MIP_ROWS];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int r = 0; r < MIP_ROWS; ++r) best[p][r] = 0u;
        // one slice: the packed column maxima of its pairs go to colacc[q]
        auto slice_step = [&](int k, int q, unsigned (&cur)[MIP_ROWS], unsigned (&nxt)[MIP_ROWS]) {
            const bool wrap = k + 4 >= dimk;  // (wave-uniform)
            const int kn = __builtin_amdgcn_readfirstlane(wrap ? wave : k + 4);
            const int bn = __builtin_amdgcn_readfirstlane(wrap ? min(b + 1, nbv - 1) : b);
            if (wrap) set_band(bn);
            load_slice(bn, kn, nxt);
            unsigned colmax[P];
#pragma unroll
            for (int p = 0; p < P; ++p) colmax[p] = 0u;
#pragma unroll
            for (int r = 0; r < MIP_ROWS; ++r) {
                const unsigned w = __builtin_amdgcn_perm(cur[r], cur[r], sel);
                if (BYTES == 2) {
                    best[0][r] = pk_max_u16(best[0][r], w);
                    colmax[0] = pk_max_u16(colmax[0], w);
                    cur[r] = w;
                } else {
                    const unsigned e = w & 0x00ff00ffu, o = (w >> 8) & 0x00ff00ffu;
                    best[0][r] = pk_max_u16(best[0][r], e);
                    best[P - 1][r] = pk_max_u16(best[P - 1][r], o);
                    colmax[0] = pk_max_u16(colmax[0], e);
                    colmax[P - 1] = pk_max_u16(colmax[P - 1], o);
                    cur[r] = pk_max_u16(e, o);  // (the row maximum does not care which column)
                }
            }
            const unsigned rm = rows_max16_pk(cur, lane);
            if (lane < 16) xzp[b * MIP_ROWS + row_of_lane(lane)][k] = (float)max(rm & 0xffffu, rm >> 16) / scale;
#pragma unroll
            for (int p = 0; p < P; ++p) colacc[q * CS + p * 64] = pk_max_u16(colacc[q * CS + p * 64], colmax[p]);
        };
        int k = wave, q = 0;
#pragma unroll 1
        for (; k + 4 < dimk; k += 8, q += 2) {
            slice_step(k, q, v, vn);
            slice_step(k + 4, q + 1, vn, v);
        }
        if (k < dimk) {
            slice_step(k, q, v, vn);
#pragma unroll
            for (int r = 0; r < MIP_ROWS; ++r) v[r] = vn[r];
        }
#pragma unroll
        for (int r = 0; r < MIP_ROWS; ++r)
#pragma unroll
            for (int p = 0; p < P; ++p) {
                atomicMax(&xyb[b][r][C * lane + col_of(p, 0)], best[p][r] & 0xffffu);
                atomicMax(&xyb[b][r][C * lane + col_of(p, 1)], best[p][r] >> 16);
            }
    }
    __syncthreads();
    {   // 4 / NB waves share a band's rows
        constexpr int WPB = 4 / NB, RPW = MIP_ROWS / WPB;
        const int bnd = wave % NB, r0 = (wave / NB) * RPW;
        if (bnd < nbv) {
            const int i0 = ib0 + bnd * MIP_ROWS, rows = min(MIP_ROWS, dimi_v - i0);
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int r = r0 + rr;
                if (r < rows) {
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (jv0 + c >= 0 && jv0 + c < dimj_v) xy[(size_t)(i0 + r) * dimj_v + jv0 + c] = (float)xyb[bnd][r][C * lane + c] / scale;
                }
            }
        }
    }
    const int jv_first = (a0 & ~(G::W - 1)) + bx * G::W - a0;  // view column of the work-group's word 0, sample 0
    if (xyT) {  // the transposed copy (see k_mips): lanes along i, a wave per column
        float* t = xyT + (size_t)bz * tstride;
        const int i = ib0 + lane;
        if (lane < nbv * MIP_ROWS && i < dimi_v)
            for (int c = wave; c < G::W; c += 4) {
                const int jv = jv_first + c;
                if (jv >= 0 && jv < dimj_v) t[(size_t)jv * dimi_v + i] = (float)xyb[lane >> 4][lane & 15][c] / scale;
            }
    }
    {   // xz[i][k] and yz[j][k]: a half-wave takes the dimk slices of one row / column (see k_mips5)
        const int k = threadIdx.x & 31;
        const int rows = min(nbv * MIP_ROWS, dimi_v - ib0);
        if (k < dimk) {
#pragma unroll
            for (int it = 0; it < NB * MIP_ROWS / 8; ++it) {
                const int r = (threadIdx.x >> 5) + 8 * it;
                if (r < rows) atomic_max_nonneg(&xz[(size_t)(ib0 + r) * dimk + k], xzp[r][k]);
            }
            const unsigned* ck = &cacc[(k & 3) * MIP_KPW + (k >> 2)][0];
#pragma unroll 4
            for (int it = 0; it < G::W / 8; ++it) {
                const int c = (threadIdx.x >> 5) + 8 * it;   // column of the work-group: word c / C, sample c % C of it
                const int l = c / C, cs = c % C;
                const int p = BYTES == 2 ? 0 : (cs & 1), h = BYTES == 2 ? cs : (cs >> 1);
                const unsigned wv = ck[p * 64 + l];
                const int jv = jv_first + c;
                if (jv >= 0 && jv < dimj_v) atomic_max_nonneg(&yz[(size_t)jv * dimk + k], (float)(h ? (wv >> 16) : (wv & 0xffffu)) / scale);
            }
        }
    }
}

// yz[j][k] = max over the row bands of yz_tmp[tile][band][k][j]; one lane per (k, j), tile = blockIdx.y = 2 * pair + which
__global__ __launch_bounds__(256) void k_mips_yz(const float* __restrict__ yz_tmp, size_t pstride, int bands, int dimk, int dimj_v,
                                                  float* __restrict__ yz1, float* __restrict__ yz2) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= dimk * dimj_v) return;
    const int k = e / dimj_v, j = e - k * dimj_v;
    const float* p = yz_tmp + (size_t)blockIdx.y * bands * dimk * dimj_v + e;
    float m = 0.0f;
    for (int b = 0; b < bands; ++b) m = fmaxf(m, p[(size_t)b * dimk * dimj_v]);
    ((blockIdx.y & 1) ? yz2 : yz1)[(size_t)(blockIdx.y >> 1) * pstride + (size_t)j * dimk + k] = m;
}

// xz[i][k] = max over the column blocks of xz_tmp[tile][block][i][k]; one lane per (i, k), tile = blockIdx.y = 2 * pair + which
__global__ __launch_bounds__(256) void k_mips_xz(const float* __restrict__ xz_tmp, size_t pstride, int blocks, int dimk, int dimi_v,
                                                  float* __restrict__ xz1, float* __restrict__ xz2) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= dimk * dimi_v) return;
    const float* p = xz_tmp + (size_t)blockIdx.y * blocks * dimk * dimi_v + e;
    float m = 0.0f;
    for (int b = 0; b < blocks; ++b) m = fmaxf(m, p[(size_t)b * dimk * dimi_v]);
    ((blockIdx.y & 1) ? xz2 : xz1)[(size_t)(blockIdx.y >> 1) * pstride + e] = m;
}

// row bands per work-group of k_mips (see there) and the number of band groups of a view
inline int mips_band_group(int dimk) { return dimk <= 4 * MIP_KPW ? MIP_NB : 1; }
inline int mips_groups(int dimk, int dimi_v) {
    const int per = MIP_ROWS * mips_band_group(dimk);
    return (dimi_v + per - 1) / per;
}
// k_mips5: stacks whose xz maxima fit its LDS image, row offsets that fit the buffer instructions' 32-bit offsets
inline bool mips5_ok(int dimk, int pitch) { return dimk <= 4 * MIP_KPW && pitch < (1 << 24); }
// launch geometry of the MIP kernel of a sample format: row bands per work-group, columns per work-group
inline int mips_fmt_bands(int bytes, int dimk) { return bytes == 4 ? mips_band_group(dimk) : (bytes == 2 ? IntTiles<2>::NB : IntTiles<1>::NB); }
inline int mips_fmt_width(int bytes) { return bytes == 4 ? 64 : (bytes == 2 ? IntTiles<2>::W : IntTiles<1>::W); }

}  // namespace

namespace mi {

size_t mips_tmp_floats(int dimk, int dimi_v, int dimj_v) {
    // (only the pass for stacks deeper than 4 * MIP_KPW slices still writes partial maxima: k_mips5 and k_mips_int merge theirs into the
    // MIPs.  A few floats all the same, so that a buffer exists.  Rows too long for k_mips5's 32-bit offsets -- 2^24 samples -- do not occur
    // with stacks this shallow in any caller's tiles; launch_mips refuses them.)
    if (dimk <= 4 * MIP_KPW) return 16;
    const size_t bands = std::max<size_t>(mips_groups(dimk, dimi_v), (dimi_v + 2 * MIP_ROWS - 1) / (2 * MIP_ROWS)), cblocks = (dimj_v + 63) / 64 + 1;
    return 2 * (bands * dimk * dimj_v + cblocks * (size_t)dimi_v * dimk);
}
bool mips_int_ok(int bytes, int dimk, int pitch, size_t slice) {
    const int per = 4 / bytes;  // samples per 32-bit word
    return (bytes == 1 || bytes == 2) && dimk <= 4 * MIP_KPW && pitch % per == 0 && slice % per == 0;
}

// `beside_chain`: a lag chain of an earlier group runs while this pass does -- the pass then keeps TWO work-groups per compute
// unit instead of four (half of the LDS and of the registers stay free for the chain's work-groups, which otherwise wait for whole
// work-groups of the pass to retire and see none of the memory system: beside a pass at four the xy forward transform of 56 pairs
// took 2.3 ms instead of 0.24 -- profiles/r05_ncc_timeline_default.txt, r05_ncc_wpe.txt, r05_ncc_sched.txt: 5.8-5.9 ms per 112
// pairs at two, 6.1-6.3 at three, 6.3 at one)
int launch_mips(hipStream_t s, const float* A, const float* B, const float* const* tab, int np, size_t pstride, int dimk, int dimi_v, int dimj_v,
                size_t slice, int pitch, int ai0, int aj0, float* xy1, float* xz1, float* yz1, float* xy2, float* xz2, float* yz2, float* tmp,
                hipEvent_t xy_done, TileFmt fmt, float* xyT, size_t tstride, bool beside_chain, bool timed) {
    const int nb = mips_fmt_bands(fmt.bytes, dimk), wcol = mips_fmt_width(fmt.bytes);
    const int bands = (dimi_v + MIP_ROWS * nb - 1) / (MIP_ROWS * nb);
    const int cblocks = (dimj_v + (aj0 & (wcol - 1)) + wcol - 1) / wcol;  // (band groups, column blocks aligned to the tile rows)
    const dim3 grid(cblocks, bands, 2 * np);   // (the deep-stack pass; k_mips5 and k_mips_int enumerate the same patches from a one-dimensional grid)
    const size_t n_xz = (size_t)dimi_v * dimk, n_yz = (size_t)dimj_v * dimk;
    auto zero_mips = [&]() {  // the passes that merge their row / column maxima into the MIPs with atomic maxima start from zero
        hipLaunchKernelGGL(k_mips_zero, dim3((unsigned)std::min<size_t>((n_xz + n_yz + 255) / 256, 64), 2 * np), dim3(256), 0, s, pstride, n_xz, n_yz, xz1,
                           yz1, xz2, yz2);
        return launch_check("k_mips_zero");
    };
    if (fmt.bytes != 4) {
        MI_REQUIRE(mips_int_ok(fmt.bytes, dimk, pitch, slice), "integer tiles: stacks of up to %d slices, rows of whole 32-bit words", 4 * MIP_KPW);
        const unsigned char* a8 = reinterpret_cast<const unsigned char*>(A);
        const unsigned char* b8 = reinterpret_cast<const unsigned char*>(B);
        const unsigned char* const* t8 = reinterpret_cast<const unsigned char* const*>(tab);
        if (!timed) MI_TRY(zero_mips());  // (timed: the maxima merge into whatever the MIPs hold)
        const dim3 grid_i((unsigned)((bands * 2 * np + 7) / 8 * 8 * cblocks));
        if (fmt.bytes == 2)
            hipLaunchKernelGGL(k_mips_int<2>, grid_i, dim3(256), 0, s, a8, b8, t8, pstride, dimk, dimi_v, dimj_v, slice, pitch, ai0, aj0, fmt.scale, xy1,
                               xz1, yz1, xy2, xz2, yz2, xyT, tstride, cblocks, bands, 2 * np);
        else
            hipLaunchKernelGGL(k_mips_int<1>, grid_i, dim3(256), 0, s, a8, b8, t8, pstride, dimk, dimi_v, dimj_v, slice, pitch, ai0, aj0, fmt.scale, xy1,
                               xz1, yz1, xy2, xz2, yz2, xyT, tstride, cblocks, bands, 2 * np);
        MI_TRY(launch_check("k_mips_int"));
        if (xy_done) MI_HIP(hipEventRecord(xy_done, s));
        return MI_OK;
    }
    // (the experiment switches are read on every call: profiles/r5_mips_knock.py changes them between timed launches of one process)
    auto probe_int = [](const char* e) { return e ? std::atoi(e) : 0; };
    const int knock = probe_int(MI_PROBE_ENV("MI_NCC_MIPS_KNOCK"));
    if (mips5_ok(dimk, pitch)) {
        const int wpe_env = probe_int(MI_PROBE_ENV("MI_NCC_MIPS_WPE")), wpe_beside = probe_int(MI_PROBE_ENV("MI_NCC_MIPS_WPE_BESIDE"));
        const int wpe = beside_chain ? (wpe_beside ? wpe_beside : (wpe_env ? wpe_env : 2)) : (wpe_env ? wpe_env : 4);
        if (!timed) MI_TRY(zero_mips());
        const int remap = probe_int(MI_PROBE_ENV("MI_NCC_MIPS_NOREMAP")) != 0 ? 0 : 1;
        const int row_groups = bands * 2 * np;
        const dim3 grid1((unsigned)((row_groups + 7) / 8 * 8 * cblocks));
#define MI_LAUNCH_MIPS5(W)                                                                                                                        \
    hipLaunchKernelGGL(k_mips5<W>, grid1, dim3(256), 0, s, A, B, tab, pstride, dimk, dimi_v, dimj_v, slice, pitch, ai0, aj0, xy1, xz1, yz1, xy2, xz2, yz2, \
                       knock, xyT, tstride, cblocks, bands, 2 * np, remap)
        if (wpe == 1) MI_LAUNCH_MIPS5(1);
        else if (wpe == 2) MI_LAUNCH_MIPS5(2);
        else if (wpe == 3) MI_LAUNCH_MIPS5(3);
        else MI_LAUNCH_MIPS5(4);
#undef MI_LAUNCH_MIPS5
        MI_TRY(launch_check("k_mips5"));
        if (xy_done) MI_HIP(hipEventRecord(xy_done, s));
        return MI_OK;
    }
    MI_REQUIRE(dimk > 4 * MIP_KPW, "compute_3_MIPs: rows of %d samples are too long for the MIP pass", pitch);
    // deeper stacks: the round-3 pass with its partial maxima and their reductions
    float* yz_tmp = tmp;
    float* xz_tmp = tmp + 2 * (size_t)np * bands * dimk * dimj_v;
    const size_t lds = sizeof(float) * MIP_ROWS * (size_t)dimk * mips_band_group(dimk);  // (k_mips: xzp)
    const bool via_lds = lds <= 32 * 1024;
    MI_REQUIRE(via_lds || !timed, "mi_ncc_time_mips: stack too deep for the timed variant");
    if (!via_lds) {  // very deep stacks: the xz MIPs are merged with atomicMax and must start at 0 (libcrossmips.cpp:319-337)
        MI_HIP(hipMemset2DAsync(xz1, sizeof(float) * (pstride ? pstride : 1), 0, sizeof(float) * (size_t)dimi_v * dimk, np, s));
        MI_HIP(hipMemset2DAsync(xz2, sizeof(float) * (pstride ? pstride : 1), 0, sizeof(float) * (size_t)dimi_v * dimk, np, s));
    }
    hipLaunchKernelGGL(k_mips, grid, dim3(256), via_lds ? lds : 0, s, A, B, tab, pstride, dimk, dimi_v, dimj_v, slice, pitch, ai0, aj0, xy1, xz1, yz1,
                       xy2, xz2, yz2, yz_tmp, via_lds ? xz_tmp : (float*)nullptr, knock, xyT, tstride);
    MI_TRY(launch_check("k_mips"));
    if (xy_done) MI_HIP(hipEventRecord(xy_done, s));
    if (timed) return MI_OK;
    hipLaunchKernelGGL(k_mips_yz, dim3((dimk * dimj_v + 255) / 256, 2 * np), dim3(256), 0, s, yz_tmp, pstride, bands, dimk, dimj_v, yz1, yz2);
    MI_TRY(launch_check("k_mips_yz"));
    if (via_lds) {
        hipLaunchKernelGGL(k_mips_xz, dim3((dimk * dimi_v + 255) / 256, 2 * np), dim3(256), 0, s, xz_tmp, pstride, cblocks, dimk, dimi_v, xz1, xz2);
        MI_TRY(launch_check("k_mips_xz"));
    }
    return MI_OK;
}

int ncc_time_mips(hipStream_t s, int n, const float* const* a_ptrs, const float* const* b_ptrs, int dimk, int dimi, int dimj, int ni, int nj, int side,
                  int reps, float* ms, TileFmt fmt) {
    MI_REQUIRE(n > 0 && reps > 0 && ms && a_ptrs && b_ptrs, "mi_ncc_time_mips: invalid arguments");
    MI_REQUIRE(side == MI_NORTH_SOUTH || side == MI_WEST_EAST, "CrossMIPs: unexpected alignment configuration");
    MI_REQUIRE(fmt.bytes == 4 || mips_int_ok(fmt.bytes, dimk, dimj, (size_t)dimi * dimj),
               "mi_ncc_time_mips: integer tiles need rows of whole 32-bit words and at most %d slices", 4 * MIP_KPW);
    const int dimi_v = side == MI_NORTH_SOUTH ? dimi - ni : dimi, dimj_v = side == MI_WEST_EAST ? dimj - nj : dimj;
    MI_REQUIRE(dimi_v > 0 && dimj_v > 0 && dimk > 0, "mi_ncc_time_mips: empty view");
    MI_REQUIRE(fmt.bytes != 4 || dimk > 4 * MIP_KPW || mips5_ok(dimk, dimj), "mi_ncc_time_mips: rows of %d samples are too long for the MIP pass", dimj);
    const size_t xy = (size_t)dimi_v * dimj_v, xz = (size_t)dimi_v * dimk, yz = (size_t)dimj_v * dimk;
    const size_t pstride = (2 * (xy + xz + yz) + 3) / 4 * 4, tmpf = mips_tmp_floats(dimk, dimi_v, dimj_v);
    DevBuf out, tmp, tab;
    MI_TRY(out.alloc(4 * pstride * n));
    MI_TRY(tmp.alloc(4 * tmpf * n));
    MI_TRY(tab.alloc(sizeof(void*) * 2 * n));
    std::vector<const float*> h(2 * (size_t)n);
    for (int q = 0; q < n; ++q) { h[2 * q] = a_ptrs[q]; h[2 * q + 1] = b_ptrs[q]; }
    MI_HIP(hipMemcpyAsync(tab.p, h.data(), sizeof(void*) * 2 * n, hipMemcpyHostToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
    float *o = out.as<float>(), *o2 = o + xy + xz + yz;  // the MIPs of a pair's first / second tile: xy | xz | yz
    struct Events {  // (destroyed on every path out of this function)
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } evs;
    MI_HIP(hipEventCreate(&evs.a));
    MI_HIP(hipEventCreate(&evs.b));
    for (int r = -1; r < reps; ++r) {  // r = -1: warm-up
        if (r == 0) MI_HIP(hipEventRecord(evs.a, s));
        MI_TRY(launch_mips(s, nullptr, nullptr, tab.as<const float*>(), n, pstride, dimk, dimi_v, dimj_v, (size_t)dimi * dimj, dimj,
                           side == MI_NORTH_SOUTH ? ni : 0, side == MI_WEST_EAST ? nj : 0, o, o + xy, o + xy + xz, o2, o2 + xy, o2 + xy + xz, tmp.as<float>(),
                           nullptr, fmt, nullptr, 0, false, true));
    }
    MI_HIP(hipEventRecord(evs.b, s));
    MI_HIP(hipEventSynchronize(evs.b));
    float total = 0.0f;
    MI_HIP(hipEventElapsedTime(&total, evs.a, evs.b));
    *ms = total / (float)reps;
    return launch_check("k_mips");
}

}  // namespace mi
