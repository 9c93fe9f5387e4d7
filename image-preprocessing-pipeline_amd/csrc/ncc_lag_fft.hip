// The lag transform of the batched MIP-NCC pipeline (ncc_lag.hip): the cross terms  sum f[i+u][j+v] t[i][j]  of a plane for every
// shift at once, in fp64 --
//   k_lag_fwd   column j of both MIPs -> one zero-padded complex FFT of length N >= n_long + E (f in the real, t in the
//               imaginary part), untangled into F_j[k], T_j[k], k = 0 .. N/2;
//   k_lag_mac / k_lag_corr   per frequency k a correlation along the SHORT axis:  C_s[k] = sum_j F_{j+s}[k] conj(T_j[k])
//               for every short-axis lag s in [-Es, Es], lag by lag or through a second transform;
//   k_lag_inv   per short-axis lag the inverse transform over k (two lags per complex FFT) -> cross[u][v] for EVERY long-axis
//               lag, of which [-El, El] are kept
// -- with the plan of a plane (lengths, tiles, LDS), the per-device twiddle and slot tables and the launcher.
#include <map>

#include "fft64_lds.h"
#include "ncc_internal.h"

using namespace mi;

namespace {

typedef double2 cplx;
using fft64::Plan;

__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }

// The transforms are those of fft64_lds.h: length N = 2^a * {1, 3, 9} (2048-row MIPs with 75 lags need N >= 2123: 2304 = 9 * 16 * 16),
// a thread owns a whole radix-16 / 9 / 8 butterfly, three LDS round trips for 2304 points under a conflict-free XOR image.
// First stage of a forward transform whose inputs come from load(i), i = logical index, instead of LDS (no fill pass).
template <int R, class Load>
__device__ __forceinline__ void first_stage_from(cplx* x, const Plan& pl, const cplx* __restrict__ tw, int first, int step, Load load) {
    const int nb = pl.N / R, q = pl.lr[0] == 0 ? (1 << pl.a) : (1 << pl.lq[0]);
    const cplx* stw = tw + pl.twoff[0];
    for (int t = first; t < nb; t += step) {
        cplx v[R];
#pragma unroll
        for (int m = 0; m < R; ++m) v[m] = load(t + m * q);
        fft64::butterfly<R, false>(v, stw, q, t);
        const int base = fft64::phys(pl, t);
#pragma unroll
        for (int m = 0; m < R; ++m) x[base ^ pl.pm[0][m]] = v[m];
    }
}
template <class Load>
__device__ __forceinline__ void first_stage_any(cplx* x, const Plan& pl, const cplx* __restrict__ tw, int first, int step, Load load) {
    switch (pl.radix[0]) {
        case 16: first_stage_from<16>(x, pl, tw, first, step, load); break;
        case 12: first_stage_from<12>(x, pl, tw, first, step, load); break;
        case 9: first_stage_from<9>(x, pl, tw, first, step, load); break;
        case 8: first_stage_from<8>(x, pl, tw, first, step, load); break;
        case 6: first_stage_from<6>(x, pl, tw, first, step, load); break;
        case 4: first_stage_from<4>(x, pl, tw, first, step, load); break;
        case 3: first_stage_from<3>(x, pl, tw, first, step, load); break;
        default: first_stage_from<2>(x, pl, tw, first, step, load); break;
    }
}

// Spectra of a plane: SP[((pair * ntile + tile) * n_short + j) * 2 KT + {0: F, 1: T} * KT + l] -- the KT frequency slots of a tile,
// for line j, F then T: one 128-byte line when KT = 4.  The forward transform of line j stores whole lines; the correlation
// kernels read a tile (all j of KT slots) as ONE contiguous block.

// forward lag transform of short-axis line j (blockIdx.x) of pair blockIdx.y: element i of the line = m[i * ls + j * ss]
template <int TH>
__global__ __launch_bounds__(TH) void k_lag_fwd(const float* __restrict__ m1, const float* __restrict__ m2, size_t pstride, int n_long, int n_short,
                                                 int ls, int ss, int KT, int ntile, const Plan* __restrict__ plp, const cplx* __restrict__ tw,
                                                 const int* __restrict__ slot_pos, const int* __restrict__ slot_neg, cplx* __restrict__ SP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lag_lds[];
    cplx* x = reinterpret_cast<cplx*>(lag_lds);
    const Plan& pl = *plp;  // (in device memory, not a by-value argument: the stage loops index its tables with the stage number, and a
                            // by-value struct indexed that way is copied to scratch memory first)
    // gridDim.x = 8 * ceil(n_short / 8): work-groups b, b + 8, ... run on one XCD and take NEIGHBOURING lines j -- with the long
    // axis strided in memory (west-east pairs) 32 neighbouring lines share every 128-byte line they read, and spread over the
    // eight L2s each of them fetched it again (0.81 GB fetched for 0.28 GB of MIPs)
    const int N = pl.N, NK = N / 2 + 1, j = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    if (j >= n_short) return;
    const float* a = m1 + (size_t)blockIdx.y * pstride + (size_t)j * ss;
    const float* b = m2 + (size_t)blockIdx.y * pstride + (size_t)j * ss;
    // f in the real, t in the imaginary part; the zero padding never exists in memory
    // (unconditional loads through a clamped index: a load inside a predicated block is waited for on the spot, and the nine
    // inputs of a butterfly then arrive one memory latency after the other)
    cplx* twl = x + N;  // the later stages' twiddles (fft64::lds_twiddles)
    for (int e = threadIdx.x; e < fft64::lds_twiddles(pl); e += TH) twl[e] = tw[pl.twoff[1] + e];
    const cplx* tws = twl - (pl.nst > 1 ? pl.twoff[1] : 0);
    first_stage_any(x, pl, tw, threadIdx.x, TH, [&](int i) {
        const size_t o = (size_t)min(i, n_long - 1) * ls;
        const float fa = a[o], fb = b[o];
        return make_double2(i < n_long ? (double)fa : 0.0, i < n_long ? (double)fb : 0.0);
    });
    __syncthreads();
    for (int st = 1; st < pl.nst; ++st) {
        fft64::stage_any<false>(x, 0, 1, pl, st, tws, threadIdx.x, TH);
        __syncthreads();
    }
    // The N/2 + 1 frequencies 0 .. N/2 of a real signal's spectrum are kept in POSITION order ("slots": slot_pos = LDS slot of the
    // frequency, ascending in logical position; slot_neg = slot of the mirror frequency N - k): the untangling pass reads LDS
    // nearly contiguously, and the per-frequency correlation does not care about the order of its frequencies.
    cplx* row = SP + ((size_t)blockIdx.y * ntile * n_short + j) * 2 * KT;
    const size_t tstride = (size_t)n_short * 2 * KT;
    for (int sl = threadIdx.x; sl < NK; sl += TH) {
        const cplx zk = x[slot_pos[sl]], zn = x[slot_neg[sl]];
        const int tile = sl / KT, l = sl - tile * KT;
        cplx* o = row + (size_t)tile * tstride + l;
        o[0] = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y));    // (Z[k] + conj Z[N-k]) / 2
        o[KT] = make_double2(0.5 * (zk.y + zn.y), -0.5 * (zk.x - zn.x));  // (Z[k] - conj Z[N-k]) / (2 i)
    }
}

// Correlation along the short axis through a second transform (planes whose short axis is long enough to pay for it): per
// frequency slot k,  C_s[k] = sum_j F_{j+s}[k] conj(T_j[k])  is the inverse transform of  F^[m] conj(T^[m])  on a zero-padded circle
// of M >= n_short + Es points.  A work-group takes the KT slots of a tile: 2 KT transforms of M points side by side in LDS (images
// M + 1 elements apart, so the 2 KT elements a wave writes for one t land in different banks), first stage straight from the
// tile in global memory, point-wise product in digit-reversed order, backward pass on KT images, last stage straight to CH.
// 3 x 5 M log2 M flops per slot instead of 8 n_short (2 Es + 1): config 5's xy plane 5 x fewer, and LDS-bound instead of fp64-bound.
template <int R, int KT2>
__device__ __forceinline__ void corr_first(cplx* arr, int AS, const cplx* __restrict__ src, int n_short, int nk, const Plan& pl,
                                           const cplx* __restrict__ tw, int first, int step) {
    const int nb = pl.N / R, q = pl.lr[0] == 0 ? (1 << pl.a) : (1 << pl.lq[0]);
    const cplx* stw = tw + pl.twoff[0];
    for (int e = first; e < nb * KT2; e += step) {
        const int t = e / KT2, f = e % KT2;  // f fastest: a wave reads whole 128-byte lines of the tile
        cplx v[R];
#pragma unroll
        for (int m = 0; m < R; ++m) {
            const int i = t + m * q;  // (clamped index + select: see k_lag_fwd; a tile is a few thousand elements: 32-bit offsets)
            const cplx g = src[min(i, n_short - 1) * KT2 + f];
            const bool on = i < n_short && (f % (KT2 / 2)) < nk;   // (slots past the spectrum's end in the last tile were never written)
            v[m] = make_double2(on ? g.x : 0.0, on ? g.y : 0.0);
        }
        fft64::butterfly<R, false>(v, stw, q, t);
        cplx* x = arr + (size_t)f * AS;
        const int base = fft64::phys(pl, t);
#pragma unroll
        for (int m = 0; m < R; ++m) x[base ^ pl.pm[0][m]] = v[m];
    }
}
template <int R>
__device__ __forceinline__ void corr_last(const cplx* arr, int AS, int nk, const Plan& pl, const cplx* __restrict__ tw, int Es, int nlp,
                                          cplx* __restrict__ dst, int first, int step) {
    const int nb = pl.N / R, q = pl.lr[0] == 0 ? (1 << pl.a) : (1 << pl.lq[0]), ls = pl.lslot[0], M = pl.N;
    const cplx* stw = tw + pl.twoff[0];
    const double inv = 1.0 / (double)M;
    for (int e = first; e < (nk << ls); e += step) {
        const int l = e >> ls, t = e & ((1 << ls) - 1);
        if (t >= nb) continue;
        bool need = false;
#pragma unroll
        for (int m = 0; m < R; ++m) need = need || t + m * q <= Es || t + m * q >= M - Es;
        if (!need) continue;
        const cplx* x = arr + (size_t)l * AS;
        const int base = fft64::phys(pl, t);
        cplx v[R];
#pragma unroll
        for (int m = 0; m < R; ++m) v[m] = x[base ^ pl.pm[0][m]];
        fft64::butterfly<R, true>(v, stw, q, t);
        cplx* o = dst + (size_t)l * nlp;
#pragma unroll
        for (int m = 0; m < R; ++m) {
            const int pos = t + m * q;  // lag s >= 0 at s, s < 0 at M + s
            if (pos <= Es) o[pos + Es] = make_double2(v[m].x * inv, -v[m].y * inv);
            else if (pos >= M - Es) o[pos - M + Es] = make_double2(v[m].x * inv, -v[m].y * inv);
        }
    }
}
template <int TH, int KT>
__global__ __launch_bounds__(TH) void k_lag_corr(const cplx* __restrict__ SP, int n_short, int NK, int Es, int nlp, int tiles_per_pair, const Plan* __restrict__ plp,
                                                  const cplx* __restrict__ tw, cplx* __restrict__ CH) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lag_lds[];
    cplx* arr = reinterpret_cast<cplx*>(lag_lds);
    const Plan& pl = *plp;
    constexpr int KT2 = 2 * KT;
    const int tile = blockIdx.x, pair = blockIdx.y, M = pl.N, AS = M + 1;
    const int k0 = tile * KT, nk = min(KT, NK - k0);
    if (nk <= 0) return;
    const cplx* src = SP + ((size_t)pair * tiles_per_pair + tile) * n_short * KT2;
    cplx* twl = arr + (size_t)KT2 * AS;
    for (int e = threadIdx.x; e < fft64::lds_twiddles(pl); e += TH) twl[e] = tw[pl.twoff[1] + e];
    const cplx* tws = twl - (pl.nst > 1 ? pl.twoff[1] : 0);
    switch (pl.radix[0]) {
        case 16: corr_first<16, KT2>(arr, AS, src, n_short, nk, pl, tw, threadIdx.x, TH); break;
        case 12: corr_first<12, KT2>(arr, AS, src, n_short, nk, pl, tw, threadIdx.x, TH); break;
        case 9: corr_first<9, KT2>(arr, AS, src, n_short, nk, pl, tw, threadIdx.x, TH); break;
        case 8: corr_first<8, KT2>(arr, AS, src, n_short, nk, pl, tw, threadIdx.x, TH); break;
        case 6: corr_first<6, KT2>(arr, AS, src, n_short, nk, pl, tw, threadIdx.x, TH); break;
        case 4: corr_first<4, KT2>(arr, AS, src, n_short, nk, pl, tw, threadIdx.x, TH); break;
        case 3: corr_first<3, KT2>(arr, AS, src, n_short, nk, pl, tw, threadIdx.x, TH); break;
        default: corr_first<2, KT2>(arr, AS, src, n_short, nk, pl, tw, threadIdx.x, TH); break;
    }
    __syncthreads();
    for (int st = 1; st < pl.nst; ++st) {
        fft64::stage_any<false>(arr, AS, KT2, pl, st, tws, threadIdx.x, TH);
        __syncthreads();
    }
    // conj(F^ conj(T^)) = conj(F^) T^, position by position (both spectra sit in the same digit-reversed, swizzled order), into F's image
    for (int l = 0; l < nk; ++l) {
        cplx* F = arr + (size_t)l * AS;
        const cplx* T = arr + (size_t)(KT + l) * AS;
        for (int p = threadIdx.x; p < M; p += TH) {
            const cplx f = F[p], t = T[p];
            F[p] = make_double2(f.x * t.x + f.y * t.y, f.x * t.y - f.y * t.x);
        }
    }
    __syncthreads();
    for (int st = pl.nst - 1; st >= 1; --st) {
        fft64::stage_any<true>(arr, AS, nk, pl, st, tws, threadIdx.x, TH);
        __syncthreads();
    }
    cplx* dst = CH + ((size_t)pair * NK + k0) * nlp;
    switch (pl.radix[0]) {
        case 16: corr_last<16>(arr, AS, nk, pl, tw, Es, nlp, dst, threadIdx.x, TH); break;
        case 12: corr_last<12>(arr, AS, nk, pl, tw, Es, nlp, dst, threadIdx.x, TH); break;
        case 9: corr_last<9>(arr, AS, nk, pl, tw, Es, nlp, dst, threadIdx.x, TH); break;
        case 8: corr_last<8>(arr, AS, nk, pl, tw, Es, nlp, dst, threadIdx.x, TH); break;
        case 6: corr_last<6>(arr, AS, nk, pl, tw, Es, nlp, dst, threadIdx.x, TH); break;
        case 4: corr_last<4>(arr, AS, nk, pl, tw, Es, nlp, dst, threadIdx.x, TH); break;
        case 3: corr_last<3>(arr, AS, nk, pl, tw, Es, nlp, dst, threadIdx.x, TH); break;
        default: corr_last<2>(arr, AS, nk, pl, tw, Es, nlp, dst, threadIdx.x, TH); break;
    }
}

// per frequency: C_s[k] = sum_j F_{j+s}[k] conj(T_j[k]),  s = -Es .. Es.  A TILE is KT frequencies of one pair; a thread takes one
// frequency, LB neighbouring lags and one of JP parts of the j range.  The LB samples of F a step needs sit in a ring of registers
// (two 16-byte LDS reads feed 4 LB FMAs; LB steps bring every sample back to its slot).
// The work-groups are persistent (tile blockIdx.x, + gridDim.x, ...) and carry the NEXT tile's spectra in registers (PF elements
// of F and of T per thread, requested right after the current tile reached LDS): work-groups of one CU start together and stay in
// step, so without this every fill phase -- 39 KB per tile on the xy plane of config 5 -- was a phase in which the CU computed
// nothing (600 -> 4xx us for that plane: profiles/r03_lag_shapes.txt).
template <int LB, int PF>
__global__ __launch_bounds__(256) void k_lag_mac(const cplx* __restrict__ SP, int n_short, int NK, int Es, int KT, int JP, int FW, int TW, int nlp,
                                                 int tiles_per_pair, int ntiles, cplx* __restrict__ CH) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lag_lds[];
    cplx* Fs = reinterpret_cast<cplx*>(lag_lds);  // KT rows of FW: PAD zeros | n_short samples | zeros
    cplx* Ts = Fs + (size_t)KT * FW;              // KT rows of TW
    cplx* red = Ts + (size_t)KT * TW;             // [jp - 1][vb][kl][LB]: the partial sums of the parts jp > 0
    const int PAD = Es + LB - 1;
    for (int e = threadIdx.x; e < KT * FW; e += blockDim.x) Fs[e] = make_double2(0.0, 0.0);
    const int nvb = nlp / LB;
    const int jlen = (n_short + JP - 1) / JP;
    const int item = threadIdx.x;  // (jp, vb, kl), kl fastest
    const int kl = item % KT, vb = (item / KT) % nvb, jp = item / (KT * nvb);
    const int v0 = -Es + LB * vb, jb = jp * jlen, je = min(n_short, jb + jlen);
    const cplx* fr = Fs + (size_t)kl * FW + PAD + v0;
    const cplx* tr = Ts + (size_t)kl * TW;
    const int nelem = n_short * KT;  // elements of a tile, kl fastest: 16 * KT contiguous bytes per line j
    const size_t tsz = (size_t)n_short * 2 * KT;  // a tile of SP: [j][F | T][KT]

    // Slot b of the persistent sequence (blockIdx.x, + gridDim.x, ...; both multiples of 16) -> tile (neighbouring tiles on one
    // XCD).  Tiles past the end and the padding tile of a pair are empty (nk <= 0).
    auto decode = [&](int b, int& tile, int& k0, int& nk) {
        tile = (b & ~15) | ((b & 7) << 1) | ((b >> 3) & 1);
        const int pair = tile / tiles_per_pair;
        k0 = (tile - pair * tiles_per_pair) * KT;
        nk = tile < ntiles ? min(KT, NK - k0) : 0;
    };
    const int nslots = (ntiles + 15) & ~15;
    int slot = blockIdx.x;
    __syncthreads();
    if (slot < nslots) {  // the first tile goes to LDS directly
        int tile, k0, nk;
        decode(slot, tile, k0, nk);
        const cplx* src = SP + (size_t)tile * tsz;
        for (int e = threadIdx.x; e < nelem; e += 256) {
            const int x = e / KT, l = e - x * KT;
            if (l < nk) {
                Fs[(size_t)l * FW + PAD + x] = src[(size_t)x * 2 * KT + l];
                Ts[(size_t)l * TW + x] = src[(size_t)x * 2 * KT + KT + l];
            }
        }
    }
    while (slot < nslots) {
        int tile, k0, nk;
        decode(slot, tile, k0, nk);
        const int pair = tile / tiles_per_pair;
        __syncthreads();  // the tile is in LDS
        const int next = slot + gridDim.x;
        const bool has_next = next < nslots;
        int ntile_ = 0, nk0 = 0, nnk = 0;
        if (has_next) decode(next, ntile_, nk0, nnk);
        const cplx* nsrc = SP + (size_t)ntile_ * tsz;
        cplx pf[PF > 0 ? PF : 1], pt[PF > 0 ? PF : 1];  // (PF = 0: rows too long for the registers -- the next tile is fetched behind this one)
        if (PF > 0 && has_next) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int e = threadIdx.x + i * 256;
                const int x = e / KT, l = e - x * KT;
                const bool ok = e < nelem && l < nnk;
                pf[i] = ok ? nsrc[(size_t)x * 2 * KT + l] : make_double2(0.0, 0.0);
                pt[i] = ok ? nsrc[(size_t)x * 2 * KT + KT + l] : make_double2(0.0, 0.0);
            }
        }

        const bool live = jp < JP && kl < nk;
        cplx acc[LB];
#pragma unroll
        for (int q = 0; q < LB; ++q) acc[q] = make_double2(0.0, 0.0);
        if (live) {
            const cplx* fp = fr + jb;
            const cplx* tp = tr + jb;
            cplx f[LB];
#pragma unroll
            for (int q = 0; q < LB - 1; ++q) f[q] = fp[q];
            auto steps = [&](int rem) {  // LB steps; rem < LB: only the first rem count (the others see t = 0)
#pragma unroll
                for (int jj = 0; jj < LB; ++jj) {
                    f[(jj + LB - 1) % LB] = fp[jj + LB - 1];  // (zeros past the row: FW leaves room for a whole trip)
                    cplx t = tp[jj];
                    if (jj >= rem) t = make_double2(0.0, 0.0);  // (the next part's samples, or what lies past the row)
#pragma unroll
                    for (int q = 0; q < LB; ++q) {
                        const cplx fv = f[(jj + q) % LB];
                        acc[q].x = fma(fv.x, t.x, fma(fv.y, t.y, acc[q].x));
                        acc[q].y = fma(fv.y, t.x, fma(-fv.x, t.y, acc[q].y));
                    }
                }
            };
            const int trips = (je - jb) / LB;
            for (int it = 0; it < trips; ++it) {
                steps(LB);
                fp += LB;
                tp += LB;
            }
            if (je - jb > trips * LB) steps(je - jb - trips * LB);
        }
        // the JP parts of a (kl, vb) are added in a fixed order
        if (live && jp > 0) {
#pragma unroll
            for (int q = 0; q < LB; ++q) red[(((size_t)(jp - 1) * nvb + vb) * KT + kl) * LB + q] = acc[q];
        }
        __syncthreads();  // (also: every read of this tile's spectra is done)
        if (live && jp == 0) {
            for (int p = 1; p < JP; ++p)
#pragma unroll
                for (int q = 0; q < LB; ++q) acc[q] = cadd(acc[q], red[(((size_t)(p - 1) * nvb + vb) * KT + kl) * LB + q]);
            cplx* dst = CH + ((size_t)pair * NK + k0 + kl) * nlp + LB * vb;
#pragma unroll
            for (int q = 0; q < LB; ++q) dst[q] = acc[q];
        }
        if (PF == 0 && has_next) {
            for (int e = threadIdx.x; e < nelem; e += 256) {
                const int x = e / KT, l = e - x * KT;
                if (l < nnk) {
                    Fs[(size_t)l * FW + PAD + x] = nsrc[(size_t)x * 2 * KT + l];
                    Ts[(size_t)l * TW + x] = nsrc[(size_t)x * 2 * KT + KT + l];
                }
            }
        }
        if (PF > 0 && has_next) {  // (every read of this tile's spectra lies before the barrier above; `red` is its own region)
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int e = threadIdx.x + i * 256;
                const int x = e / KT, l = e - x * KT;
                if (e < nelem && l < nnk) {
                    Fs[(size_t)l * FW + PAD + x] = pf[i];
                    Ts[(size_t)l * TW + x] = pt[i];
                }
            }
        }
        slot = next;
    }
}

// inverse lag transform of two short-axis lags (sa, sa + 1) of a pair: c_a[n] + i c_b[n] = FFT(conj C_a + i conj C_b) / N (both c
// real); the long-axis lags [-El, El] go to cross[(u + Eu) * (2 Ev + 1) + (v + Ev)].  The first stage gathers its inputs from CH
// (slot of frequency k: freq_slot[k]).  Work-groups b, b + 8, ... share an XCD and take the lag pairs of ONE pair after another: its
// block of CH (2 MB on config 5, read as 32-byte pieces of 1.6-KB rows) is then fetched once into that L2.
template <int TH>
__global__ __launch_bounds__(TH) void k_lag_inv(const cplx* __restrict__ CH, int NK, int nlp, const Plan* __restrict__ plp, int Es, int El, int long_is_u, int Eu, int Ev,
                                                 const cplx* __restrict__ tw, const int* __restrict__ freq_slot, int np, int lagpairs,
                                                 double* __restrict__ cross) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lag_lds[];
    cplx* x = reinterpret_cast<cplx*>(lag_lds);
    const Plan& pl = *plp;
    const int N = pl.N, nlag = 2 * Es + 1;
    const int slot = (int)(blockIdx.x >> 3), pair = 8 * (slot / lagpairs) + (int)(blockIdx.x & 7);
    if (pair >= np) return;
    const int sa = 2 * (slot % lagpairs), sb = sa + 1;
    const bool has_b = sb < nlag;
    const cplx* src = CH + (size_t)pair * NK * nlp;
    cplx* twl = x + N;
    for (int e = threadIdx.x; e < fft64::lds_twiddles(pl); e += TH) twl[e] = tw[pl.twoff[1] + e];
    const cplx* tws = twl - (pl.nst > 1 ? pl.twoff[1] : 0);
    first_stage_any(x, pl, tw, threadIdx.x, TH, [&](int kk) {
        const bool low = 2 * kk <= N;
        const int sl = freq_slot[low ? kk : N - kk];
        const cplx xa = src[(size_t)sl * nlp + sa];
        cplx xb = src[(size_t)sl * nlp + (has_b ? sb : sa)];
        if (!has_b) xb = make_double2(0.0, 0.0);
        return low ? make_double2(xa.x + xb.y, -xa.y + xb.x)   // conj(Xa) + i conj(Xb)
                   : make_double2(xa.x - xb.y, xa.y + xb.x);   // Xa + i Xb  (= conj X[N-k] terms)
    });
    __syncthreads();
    for (int st = 1; st < pl.nst; ++st) {
        fft64::stage_any<false>(x, 0, 1, pl, st, tws, threadIdx.x, TH);
        __syncthreads();
    }
    const double inv = 1.0 / (double)N;
    const int W = 2 * Ev + 1;
    double* out = cross + (size_t)pair * (2 * Eu + 1) * W;
    for (int e = threadIdx.x; e < 2 * El + 1; e += TH) {
        const int l = e - El;
        const cplx v = x[fft64::phys(pl, fft64::pos_of_freq(pl, (l + N) % N))];
        if (long_is_u) {
            out[(size_t)(l + Eu) * W + (sa - Es + Ev)] = v.x * inv;
            if (has_b) out[(size_t)(l + Eu) * W + (sb - Es + Ev)] = v.y * inv;
        } else {
            out[(size_t)(sa - Es + Eu) * W + (l + Ev)] = v.x * inv;
            if (has_b) out[(size_t)(sb - Es + Eu) * W + (l + Ev)] = v.y * inv;
        }
    }
}

// make_plan searches the LDS image of a length: once per length and process
const Plan& plan_for(int need) {
    static std::mutex& mu = *new std::mutex;
    static std::map<int, Plan>& plans = *new std::map<int, Plan>;  // keyed by the request; several requests may share a length
    std::lock_guard<std::mutex> lock(mu);
    auto it = plans.find(need);
    if (it == plans.end()) it = plans.emplace(need, fft64::make_plan(need)).first;
    return it->second;  // (a node of a map that is never destroyed: the address stays valid)
}

}  // namespace

LagPlane mi::plan_lag_plane(const PlaneGeom& g, int maxIter) {
    LagPlane p{};
    p.long_is_u = g.dimu >= g.dimv;
    p.n_long = p.long_is_u ? g.dimu : g.dimv;
    p.n_short = p.long_is_u ? g.dimv : g.dimu;
    p.ls = p.long_is_u ? g.dimv : 1;
    p.ss = p.long_is_u ? 1 : g.dimv;
    const int dl = p.long_is_u ? g.delayu : g.delayv, ds = p.long_is_u ? g.delayv : g.delayu;
    const int wl = p.long_is_u ? g.wu : g.wv, wsh = p.long_is_u ? g.wv : g.wu;
    // every long-axis lag comes out of the inverse transform: keep all that the re-centring moves can reach; along the short axis a
    // lag costs a correlation: keep one move's worth (a second move beyond it is rare and sends the pair to the careful path)
    p.El = dl + maxIter * wl;
    p.Es = ds + (maxIter > 0 ? wsh : 0);
    p.Eu = p.long_is_u ? p.El : p.Es;
    p.Ev = p.long_is_u ? p.Es : p.El;
    p.ok = p.n_long + p.El <= 8192;
    if (!p.ok) return p;
    p.fft = &plan_for(p.n_long + p.El);
    p.N = p.fft->N;
    p.lds_fft = sizeof(double) * 2 * ((size_t)p.N + fft64::lds_twiddles(*p.fft));
    const int nlag = 2 * p.Es + 1;
    p.LB = 4;  // lags per thread of the direct correlation kernel (8 was measured: twice the registers, bank conflicts, no faster)
    p.nlp = (nlag + p.LB - 1) / p.LB * p.LB;
    // Short axes of 64 lines and more are correlated through a second transform (k_lag_corr), the others lag by lag (k_lag_mac):
    // 32-line planes (the xz / yz MIPs of thin stacks) have too few samples per frequency to fill a transform's work-group.
    p.use_corr = p.n_short >= 64;
    if (p.use_corr) {
        p.cfft = &plan_for(p.n_short + p.Es);
        const size_t img = sizeof(double) * 2 * ((size_t)p.cfft->N + 1);
        p.KT = 2 * img * 4 <= 52 * 1024 ? 4 : (2 * img * 2 <= 80 * 1024 ? 2 : 1);  // (three work-groups per CU where the images allow)
        p.lds_corr = 2 * (size_t)p.KT * img + sizeof(double) * 2 * (size_t)fft64::lds_twiddles(*p.cfft);
        p.JP = 1; p.FW = p.TW = 0;
        p.lds_mac = 0;
        p.ok = p.lds_corr <= 150 * 1024;
    } else {
        const int PAD = p.Es + p.LB - 1;
        // odd row lengths (in 16-byte slots): the KT rows a wave touches at once start in different banks, and a lag block is four slots
        p.FW = (p.n_short + 2 * PAD + p.LB) | 1;
        p.TW = (p.n_short + p.LB) | 1;
        const size_t row = sizeof(double) * 2 * (size_t)(p.FW + p.TW);
        // four frequencies per work-group: with rows one 16-byte slot apart and lanes ordered (frequency fastest, then lag block) the
        // 16-byte LDS reads of a wave are conflict-free; the j range is cut into JP parts so that all 256 threads have an item
        p.KT = (int)std::min<size_t>(4, (48 * 1024) / row);
        if (p.KT < 1) p.KT = 1;
        const int nvb = p.nlp / p.LB;
        while (p.KT > 1 && p.KT * nvb > 256) --p.KT;
        p.JP = std::max(1, std::min(8, 256 / (p.KT * nvb)));
        p.lds_mac = row * p.KT + sizeof(double) * 2 * p.LB * (size_t)(p.JP - 1) * nvb * p.KT;
        p.ok = p.lds_mac <= 150 * 1024 && nvb <= 256;
    }
    p.fft_threads = p.N >= 1024 ? 256 : 128;
    const int Hm = 2 * g.delayu + 1, Wm = 2 * g.delayv + 1, H = 2 * g.wu + 1, W = 2 * g.wv + 1;
    p.lds_refine = sizeof(float) * ((size_t)Hm * Wm + 2 * (size_t)H * W);
    p.ok = p.ok && p.N <= 8192 && p.lds_refine <= 120 * 1024;
    return p;
}

namespace {

// Per (device, N), kept for the life of the process: the stages' twiddle tables in fp64 and the slot tables of the half spectrum
// (LDS slot of the s-th frequency in ascending logical position, LDS slot of its mirror frequency, slot of a frequency).
struct FftTables {
    const cplx* tw;
    const int *slot_pos, *slot_neg, *freq_slot;
    const Plan* plan;  // the plan itself, for the kernels
};
struct TwiddleKey { int dev, n; bool operator<(const TwiddleKey& o) const { return dev != o.dev ? dev < o.dev : n < o.n; } };
std::mutex& g_tw_mu = *new std::mutex;
std::map<TwiddleKey, FftTables>& g_tw = *new std::map<TwiddleKey, FftTables>;

int fft_tables(int dev, const Plan& pl, hipStream_t s, FftTables* out) {
    std::lock_guard<std::mutex> lock(g_tw_mu);
    auto it = g_tw.find(TwiddleKey{dev, pl.N});
    if (it != g_tw.end()) { *out = it->second; return MI_OK; }
    const size_t N = (size_t)pl.N, NK = N / 2 + 1;
    const std::vector<double> hs = fft64::make_twiddles(pl);
    // Which frequency sits in which slot is free (the correlation kernels do not care, the inverse transform looks slots up), so the
    // order is chosen for the untangling pass of k_lag_fwd: lane l of a wave reads Z[k] and Z[N - k] of slot 64 w + l with 16-byte
    // LDS reads, which are served in four groups of 16 lanes over 16 bank quads -- every group gets 16 frequencies whose Z[k] fall
    // into 16 different quads AND whose Z[N - k] do.  Frequencies are bucketed by the two quads; a group is a perfect matching
    // between the quads of the first read and those of the second (Kuhn's augmenting paths on a 16 x 16 graph), fullest buckets
    // first; what cannot be matched at the end fills the last slots.  (In position order the first read was 2-way, the second up
    // to 4-way conflicted: SQ_LDS_BANK_CONFLICT 14 % of the LDS cycles of the transform.)
    std::vector<int> p1(NK), p2(NK);
    std::vector<std::vector<int>> bucket(256);
    for (size_t k = 0; k < NK; ++k) {
        p1[k] = fft64::phys(pl, fft64::pos_of_freq(pl, (int)k));
        p2[k] = fft64::phys(pl, fft64::pos_of_freq(pl, (int)((N - k) % N)));
        bucket[(size_t)(p1[k] & 15) * 16 + (size_t)(p2[k] & 15)].push_back((int)k);
    }
    static const int lanes_of_group[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                               {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                               {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                               {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    std::vector<int> slot_freq(NK, -1);
    size_t placed = 0;
    for (size_t w = 0; w * 64 < NK && placed < NK; ++w)
        for (int g = 0; g < 4 && placed < NK; ++g) {
            int match_of_b2[16];
            for (int& m : match_of_b2) m = -1;
            // Kuhn: first-read quads in turn, their edges tried in the order of bucket size
            for (int a = 0; a < 16; ++a) {
                bool seen[16] = {false};
                struct Rec {
                    static bool go(int a_, const std::vector<std::vector<int>>& bk, int* mb, bool* sn) {
                        int ord[16];
                        for (int i = 0; i < 16; ++i) ord[i] = i;
                        std::sort(ord, ord + 16, [&](int x, int y) { return bk[(size_t)a_ * 16 + x].size() > bk[(size_t)a_ * 16 + y].size(); });
                        for (int oi = 0; oi < 16; ++oi) {
                            const int b = ord[oi];
                            if (bk[(size_t)a_ * 16 + b].empty() || sn[b]) continue;
                            sn[b] = true;
                            if (mb[b] < 0 || go(mb[b], bk, mb, sn)) { mb[b] = a_; return true; }
                        }
                        return false;
                    }
                };
                (void)Rec::go(a, bucket, match_of_b2, seen);
            }
            int li = 0;
            for (int b = 0; b < 16; ++b) {
                if (match_of_b2[b] < 0) continue;
                std::vector<int>& bk = bucket[(size_t)match_of_b2[b] * 16 + b];
                const size_t sl = w * 64 + (size_t)lanes_of_group[g][li];
                if (sl >= NK) continue;  // (the last, partial wave)
                slot_freq[sl] = bk.back();
                bk.pop_back();
                ++li;
                ++placed;
            }
            // lanes the matching left empty are filled at the end
        }
    {
        std::vector<int> rest;
        for (auto& bk : bucket) rest.insert(rest.end(), bk.begin(), bk.end());
        size_t ri = 0;
        for (size_t sl = 0; sl < NK; ++sl)
            if (slot_freq[sl] < 0) slot_freq[sl] = rest[ri++];
    }
    std::vector<int> tabs(3 * NK);
    for (size_t sl = 0; sl < NK; ++sl) {
        const size_t k = (size_t)slot_freq[sl];
        tabs[sl] = p1[k];
        tabs[NK + sl] = p2[k];
        tabs[2 * NK + k] = (int)sl;
    }
    void *d = nullptr, *di = nullptr, *dp = nullptr;
    MI_HIP(hipMalloc(&d, sizeof(double) * hs.size()));
    MI_HIP(hipMalloc(&di, sizeof(int) * 3 * NK));
    MI_HIP(hipMalloc(&dp, sizeof(Plan)));
    MI_HIP(hipMemcpyAsync(d, hs.data(), sizeof(double) * hs.size(), hipMemcpyHostToDevice, s));
    MI_HIP(hipMemcpyAsync(di, tabs.data(), sizeof(int) * 3 * NK, hipMemcpyHostToDevice, s));
    MI_HIP(hipMemcpyAsync(dp, &pl, sizeof(Plan), hipMemcpyHostToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
    const int* ti = static_cast<const int*>(di);
    FftTables t{static_cast<const cplx*>(d), ti, ti + NK, ti + 2 * NK, static_cast<const Plan*>(dp)};
    g_tw[TwiddleKey{dev, pl.N}] = t;
    *out = t;
    return MI_OK;
}

}  // namespace

int mi::lag_cross(int dev, hipStream_t s, const LagPlane& lp, const float* m1, const float* m2, size_t pstride, int np, DevBuf& SP, DevBuf& CH,
                  DevBuf& cross, hipEvent_t after_fwd) {
    const int N = lp.N, NK = N / 2 + 1, nlag = 2 * lp.Es + 1, nlp = lp.nlp;
    const int tiles_per_pair = ((NK + lp.KT - 1) / lp.KT + 1) & ~1, ntiles = tiles_per_pair * np;  // (even: see k_lag_mac)
    FftTables ft;
    MI_TRY(fft_tables(dev, *lp.fft, s, &ft));
    MI_TRY(grow(SP, sizeof(double) * 2 * (size_t)ntiles * lp.n_short * 2 * lp.KT));
    MI_TRY(grow(CH, sizeof(double) * 2 * (size_t)np * NK * nlp));
    MI_TRY(grow(cross, sizeof(double) * (size_t)np * (2 * lp.Eu + 1) * (2 * lp.Ev + 1)));
    const bool big = lp.fft_threads == 256;
    {
        auto fwd = big ? k_lag_fwd<256> : k_lag_fwd<128>;
        if (lp.lds_fft > 64 * 1024)
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lp.lds_fft));
        hipLaunchKernelGGL(fwd, dim3(8 * ((lp.n_short + 7) / 8), np), dim3(lp.fft_threads), lp.lds_fft, s, m1, m2, pstride, lp.n_long, lp.n_short, lp.ls,
                           lp.ss, lp.KT, tiles_per_pair, ft.plan, ft.tw, ft.slot_pos, ft.slot_neg, SP.as<cplx>());
        MI_TRY(launch_check("k_lag_fwd"));
    }
    if (after_fwd) MI_HIP(hipEventRecord(after_fwd, s));
    if (lp.use_corr) {
        FftTables ct;
        MI_TRY(fft_tables(dev, *lp.cfft, s, &ct));
        auto corr = lp.KT == 4 ? k_lag_corr<256, 4> : (lp.KT == 2 ? k_lag_corr<256, 2> : k_lag_corr<256, 1>);
        if (lp.lds_corr > 64 * 1024)
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(corr), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lp.lds_corr));
        hipLaunchKernelGGL(corr, dim3(tiles_per_pair, np), dim3(256), lp.lds_corr, s, SP.as<cplx>(), lp.n_short, NK, lp.Es, nlp, tiles_per_pair,
                           ct.plan, ct.tw, CH.as<cplx>());
        MI_TRY(launch_check("k_lag_corr"));
    } else {
        using MacFn = void (*)(const cplx*, int, int, int, int, int, int, int, int, int, int, cplx*);
        static const MacFn macs[] = {k_lag_mac<4, 0>, k_lag_mac<4, 1>, k_lag_mac<4, 2>, k_lag_mac<4, 3>, k_lag_mac<4, 4>, k_lag_mac<4, 5>, k_lag_mac<4, 6>};
        const int pfn = (lp.n_short * lp.KT + 255) / 256;  // float4 pairs per thread of a tile; beyond the table: no register prefetch
        MacFn mac = macs[pfn <= 6 ? pfn : 0];
        int cus = 256, per_cu = 1;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (lp.lds_mac > 64 * 1024)
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mac), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lp.lds_mac));
        per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lp.lds_mac, 1)));
        const int grid = std::max(16, std::min((ntiles + 15) & ~15, (cus * per_cu) & ~15));
        hipLaunchKernelGGL(mac, dim3(grid), dim3(256), lp.lds_mac, s, SP.as<cplx>(), lp.n_short, NK, lp.Es, lp.KT, lp.JP, lp.FW, lp.TW, nlp,
                           tiles_per_pair, ntiles, CH.as<cplx>());
        MI_TRY(launch_check("k_lag_mac"));
    }
    {
        auto inv = big ? k_lag_inv<256> : k_lag_inv<128>;
        if (lp.lds_fft > 64 * 1024)
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(inv), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lp.lds_fft));
        const int lagpairs = (nlag + 1) / 2;
        hipLaunchKernelGGL(inv, dim3(8 * ((np + 7) / 8) * lagpairs), dim3(lp.fft_threads), lp.lds_fft, s, CH.as<cplx>(), NK, nlp, ft.plan, lp.Es,
                           lp.El, lp.long_is_u ? 1 : 0, lp.Eu, lp.Ev, ft.tw, ft.freq_slot, np, lagpairs, cross.as<double>());
    }
    return launch_check("k_lag_inv");
}
