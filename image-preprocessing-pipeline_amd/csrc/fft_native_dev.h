// Device building blocks of the hand-written FFT pipeline (see fft_native.hip for the design): the LDS image, the super-stage
// chains and the tile extents every axis kernel is made of, and the launch helpers of the units that hold the kernels
// (fft_native_x.hip, fft_native_yz.hip).
#pragma once
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "fft_native.h"

namespace mi {
namespace {

#ifndef MI_FFT_UNROLL
#define MI_FFT_UNROLL 4
#endif
#ifndef MI_YCUT
#define MI_YCUT 1
#endif
constexpr int kYCut = MI_YCUT;    // super-stage cut of the y kernels (seg_r); -DMI_YCUT=0: the round-4 cut, for A/B builds

// ------------------------------------------------------------------------------------------------ LDS image
// Element i (8 B) of a row sits at slot i ^ G(bits 4..7 of i) ^ rmask(row).  DS traffic is banked per instruction
// (MI355X_MICROARCH.md "LDS"): ds_read_b64 serves 32 lanes per LDS cycle from 64 dword banks, i.e. it is conflict-free when
// the 32 slots differ mod 32; ds_write_b64 serves 16 lanes from 32 dword banks (slots must differ mod 16).  G is GF(2)-linear
// with columns (15, 13, 25, 16) for bits 4..7: with it every butterfly pattern of the super-stage chains below ((0,3), (3,3),
// (3,2), (3,1) and all S_LO >= 5), the stride-2 row accesses and -- together with rmask -- the transposed tile accesses are
// conflict-free under both rules.  (An additive pad of one slot per 32 leaves 2- and 4-way conflicts on the stages with
// 0 < S_LO < 5: 43 % of the LDS cycles of the x pass were conflict cycles, profiles/r01_sq_counters_padded_layout.txt.)
__host__ __device__ constexpr int swz_g(int t) { return ((t & 1) ? 15 : 0) ^ ((t & 2) ? 13 : 0) ^ ((t & 4) ? 25 : 0) ^ ((t & 8) ? 16 : 0); }
__host__ __device__ constexpr int swz_c(int i) { return i ^ swz_g((i >> 4) & 15); }
__host__ __device__ constexpr unsigned long long swz_table_hi() {  // G restricted to bits 5..7, 8 entries of 5 bits
    unsigned long long v = 0;
    for (int t = 0; t < 8; ++t) v |= (unsigned long long)swz_g(2 * t) << (5 * t);
    return v;
}
__device__ __forceinline__ int phys(int i) {
    constexpr unsigned long long T = swz_table_hi();
    const int hi = (int)((T >> (5 * ((i >> 5) & 7))) & 31ull);
    return i ^ hi ^ (__builtin_amdgcn_sbfe(i, 4, 1) & 15);
}
// Rows: the transposed accesses of the x and z passes put `hp` row pairs x (32 / hp) consecutive elements into one lane group
// (16 / hp for a store); row 2 rp (+1) is XOR-ed with a mask that spreads the rp bits over the banks the elements leave free.
// hp | kRowsRot (the fused x pass on the rotated x order, hp = 8 or 4): a lane of the transposed accesses touches the eight
// NEIGHBOURING elements 8 a .. 8 a + 7, one per instruction, and a lane group holds 32 / hp (16 / hp) consecutive a: the elements of
// an instruction differ in bits 3.. and the rp bits go to the low bits, which they leave free (bit 3 maps to slot bit 3, bit 4 to
// 0b11111, bit 5 to 0b01101: with 0b00001 .. 0b00100 for rp they are linearly independent, so the slots differ mod 32).
constexpr int kRowsRot = 256;
__device__ __forceinline__ int rmask(int row, int hp) {
    if (hp & kRowsRot) return (row >> 1) & ((hp & (kRowsRot - 1)) - 1);
    const int rp = (row >> 1) & (hp - 1);
    const int s = hp == 8 ? 1 : hp == 4 ? 2 : hp == 2 ? 3 : 0;
    return (rp << s) ^ ((rp & 1) << 4);
}

__device__ __forceinline__ int launder(int x) {
    asm volatile("" : "+v"(x));
    return x;
}
// Work-group barrier that orders LDS traffic only.  Nothing in these kernels communicates through global memory inside a
// launch, so the barrier must not drain the vector-memory queue: global loads issued before an FFT phase (the next tile,
// the epilogue operand) stay in flight across the phase's barriers and are waited for at their first use.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// Wave-level ordering of LDS traffic: DS operations of one wave execute in order, so data a wave wrote is visible to its own
// later reads (any lane) without a barrier; the fence only keeps the compiler from reordering them.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// between two phases on a tile: rows private to their owner waves need no work-group barrier
__device__ __forceinline__ void stage_sync(bool priv) {
    if (priv) wave_lds_fence();
    else lds_barrier();
}

// 1 / max(c, eps) of the RL ratio step (decon.m:164) with the hardware reciprocal (1 ulp): the IEEE division sequence costs
// 11 VALU instructions per value, a sixth of the fused x pass, for a difference far inside the fp32 noise of the transforms
__device__ __forceinline__ float rcp_eps(float c) { return __builtin_amdgcn_rcpf(fmaxf(c, kEpsSingle)); }

// Complex arithmetic on packed pairs: written on 2-vectors with explicit lane shuffles so that every complex product becomes
// v_pk_mul_f32 + v_pk_fma_f32 (lane selects and the swapped / negated twiddle are operand modifiers or hoisted set-up);
// from the scalar formulas the compiler emits one v_pk_mul + two half-used v_pk_fma + a move per product.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f V2(float2 a) { return v2f{a.x, a.y}; }
__device__ __forceinline__ float2 F2(v2f a) { return make_float2(a.x, a.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    const v2f A = V2(a), B = V2(b);
    const v2f axx = __builtin_shufflevector(A, A, 0, 0), ayy = __builtin_shufflevector(A, A, 1, 1);
    const v2f bs = {-B.y, B.x};
    return F2(__builtin_elementwise_fma(ayy, bs, axx * B));
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {  // a * conj(b)
    const v2f A = V2(a), B = V2(b);
    const v2f axx = __builtin_shufflevector(A, A, 0, 0), ayy = __builtin_shufflevector(A, A, 1, 1);
    const v2f bc = {B.x, -B.y}, bsw = {B.y, B.x};
    return F2(__builtin_elementwise_fma(ayy, bsw, axx * bc));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return F2(V2(a) + V2(b)); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return F2(V2(a) - V2(b)); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ unsigned brev_n(unsigned v, int bits) { return bits == 0 ? 0u : (__brev(v) >> (32 - bits)); }

// An axis of length N = r3 * 2^l2 (r3 in {1, 3, 9}) is transformed by one radix-r3 DIF stage followed by r3 power-of-two
// sub-transforms; position p = k1 * 2^l2 + p' then holds frequency k1 + r3 * brev(p').
__device__ __forceinline__ int pos2freq(int p, int l2, int r3) {
    const int k1 = p >> l2, pp = p & ((1 << l2) - 1);
    return k1 + r3 * (int)brev_n((unsigned)pp, l2);
}
__device__ __forceinline__ int freq2pos(int k, int l2, int r3) {
    const int k2 = k / r3, k1 = k - k2 * r3;
    return (k1 << l2) + (int)brev_n((unsigned)k2, l2);
}
__device__ __forceinline__ int mirror_pos(int p, int n, int l2, int r3) {
    const int k = pos2freq(p, l2, r3);
    return freq2pos(k == 0 ? 0 : n - k, l2, r3);
}
// x positions (NativeDims::xrot): the index w the x transform works with ("working index": w = freq2pos(xk) of the rule above) sits
// at position w, or -- rotated order -- at (w & 7) * (Hx / 8) + (w >> 3).  The eight points 8a .. 8a + 7 of a bottom radix-8
// butterfly then lie Hx / 8 positions apart, which is the stride of the eight items a lane of k_x_fused_pipe loads and stores.
// (branch-free: digit width r = 3 and shift s = lhx2 - 3 when rotated, both 0 otherwise -- then both maps are the identity)
__device__ __forceinline__ int x_work2pos(int w, const NativeDims& d) {
    const int r = 3 * d.xrot, s = d.xrot * (d.lhx2 - 3);
    return ((w & ((1 << r) - 1)) << s) | (w >> r);
}
__device__ __forceinline__ int x_pos2work(int p, const NativeDims& d) {
    const int r = 3 * d.xrot, s = d.xrot * (d.lhx2 - 3);
    return ((p & ((1 << s) - 1)) << r) | (p >> s);
}
__device__ __forceinline__ int x_freq2pos(int k, const NativeDims& d) { return x_work2pos(freq2pos(k, d.lhx2, d.r3x), d); }
__device__ __forceinline__ int y_pos2freq(int p, const NativeDims& d) { return pos2freq(p, d.ly2, d.r3); }
__device__ __forceinline__ int y_mirror_pos(int p, const NativeDims& d) { return mirror_pos(p, d.ny, d.ly2, d.r3); }

// Padded mode (PadWindow::on): the transform grid is larger than the caller's volume.  Source sample of grid coordinate g
// on axis a (-1: zero): zero rule = the data sits at [o, o + n); replicate rule = clamped samples inside the window [0, w).
__device__ __forceinline__ int pad_src(const PadWindow& p, int a, int g) {
    if (p.rep[a]) return g < p.w[a] ? min(max(g - p.o[a], 0), p.n[a] - 1) : -1;
    const int s = g - p.o[a];
    return (s >= 0 && s < p.n[a]) ? s : -1;
}
// Output sample of grid coordinate g (-1: the grid point is not part of the cropped result)
__device__ __forceinline__ int pad_dst(const PadWindow& p, int a, int g) {
    const int s = g - p.o[a];
    return (s >= 0 && s < p.n[a]) ? s : -1;
}

// exp(-2 pi i m / 2^(bpos+1)), m < 2^bpos, bpos <= 3: the part of a butterfly twiddle that depends only on the
// register index, as compile-time constants (cos/sin of multiples of 2 pi / 16)
__device__ __forceinline__ constexpr float c16(int k) {
    constexpr float c[8] = {1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f,
                            0.0f, -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f};
    return c[k];
}
__device__ __forceinline__ constexpr float s16(int k) {
    constexpr float sn[8] = {0.0f, 0.38268343236508977f, 0.70710678118654752f, 0.92387953251128674f,
                             1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f};
    return sn[k];
}

// ------------------------------------------------------------------------------------------------ super-stage chains
// gather the tables from the global table tw[e] = exp(-2 pi i e / 2^LOGN), e < 2^(LOGN-1): entry [p - 1][m] of the super-stage
// at S is exp(-2 pi i m p / 2^(S+r)), the p-th power of the lane twiddle of group element m
template <int LOGN, int NT, int S = 0, int CUT = 0>
__device__ __forceinline__ void fill_chain_tw(float2* twl, const float2* __restrict__ tw) {
    if constexpr (S < LOGN) {
        constexpr int r = seg_r(LOGN, S, CUT);
        if constexpr (S > 0) {
            constexpr int np = tw_powers(S, r);
            for (int i = threadIdx.x; i < (np << S); i += NT) {
                const int p = (i >> S) + 1, m = i & ((1 << S) - 1);
                const int e = (m * p) << (LOGN - S - r);  // < 2^LOGN
                const float2 t = tw[e & ((1 << (LOGN - 1)) - 1)];
                twl[tw_off(LOGN, S, CUT) + i] = (e >> (LOGN - 1)) ? make_float2(-t.x, -t.y) : t;  // exp(-i(x + pi)) = -exp(-ix)
            }
        }
        fill_chain_tw<LOGN, NT, S + r, CUT>(twl, tw);
    }
}
// LDS layout behind the tile of an axis kernel: [chain tables][radix-3/9 table: exp(-2 pi i n2 / N), n2 < 2^L2]
template <int L2, int R3, int CUT = 0>
struct TwLds {
    static constexpr int r3 = chain_entries(L2, CUT);
    static constexpr int total = r3 + (R3 > 1 ? (1 << L2) : 0);
    // tw: global table of the axis ([sub/2 power-of-two part][full circle of N when R3 > 1])
    template <int NT>
    static __device__ __forceinline__ void fill(float2* twl, const float2* __restrict__ tw) {
        fill_chain_tw<L2, NT, 0, CUT>(twl, tw);
        if constexpr (R3 > 1) {
            const float2* twM = tw + (1 << L2) / 2;
            for (int n2 = threadIdx.x; n2 < (1 << L2); n2 += NT) twl[r3 + n2] = twM[n2];
        }
    }
};

// Sequences of a tile: `batch` = rows * R3 power-of-two sub-transforms of length 2^LOGN; sequence b = row b / R3, sub-block
// b % R3 (elements [sub << LOGN, (sub + 1) << LOGN) of the row).  PRIV: the rows are dealt to the waves (row r belongs to
// wave r mod NW) and every phase between two tile-wide barriers touches a row only through its owner, so the super-stages of
// a chain follow each other without work-group barriers and the waves drift apart (LDS and VALU phases of different waves
// overlap).  Otherwise the sequences are split over all lanes and a barrier follows every super-stage.
template <int LOGN, int LR, int NT, int R3>
struct SeqMap {
    static constexpr int GL = LOGN - LR, NW = NT / 64;
    int total, first, step;
    int wave;
    bool PRIV;
    __device__ __forceinline__ SeqMap(int batch, bool priv) : PRIV(priv) {
        if (PRIV) {
            wave = threadIdx.x >> 6;
            total = ((batch / R3) / NW * R3) << GL;  // rows % NW == 0 (checked by the caller)
            first = threadIdx.x & 63;
            step = 64;
        } else {
            wave = 0;
            total = batch << GL;
            first = threadIdx.x;
            step = NT;
        }
    }
    // work item u -> (row, sub-block, group g)
    __device__ __forceinline__ void at(int u, int& row, int& sub, int& g) const {
        int bl = u >> GL;
        if (GL >= 6) bl = __builtin_amdgcn_readfirstlane(bl);  // 64 consecutive items of a wave share the sequence: SALU row math
        g = u & ((1 << GL) - 1);
        if (R3 == 1) {
            sub = 0;
            row = PRIV ? bl * NW + wave : bl;
        } else {
            const int rl = bl / R3;
            sub = bl - rl * R3;
            row = PRIV ? rl * NW + wave : rl;
        }
    }
};

// multiplication by exp(-2 pi i k16 / 16) (forward) or its conjugate (inverse): compile-time constants; -i / +i are swaps
template <bool CONJ>
__device__ __forceinline__ float2 mul_c16(float2 a, int k16) {
    if (k16 == 0) return a;
    if (k16 == 4) return CONJ ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x);
    const float2 c = make_float2(c16(k16), CONJ ? s16(k16) : -s16(k16));
    return cmul(a, c);
}
__host__ __device__ constexpr int bit_rev(int j, int bits) {
    int r = 0;
    for (int b = 0; b < bits; ++b) r |= ((j >> b) & 1) << (bits - 1 - b);
    return r;
}

// The LR radix-2 stages of a super-stage on the R = 2^LR points of one lane, as one radix-R butterfly: the stages only carry
// their compile-time constants exp(-2 pi i jl / 2^(bpos+1)); the lane-dependent part of all twiddles on the path of register j
// collapses to ONE factor w^rev(j), w = exp(-2 pi i m / 2^(S_LO+LR)), applied after the stages (forward, DIF) or, conjugated,
// before them (inverse, DIT) -- R - 1 complex products instead of LR * R / 2.  twl: the super-stage's table, [p - 1][m] = w^p
// for the tw_powers() powers it keeps (unused when S_LO == 0).
template <int LR, int S_LO, bool INVERSE>
__device__ __forceinline__ void butterflies(float2 (&v)[1 << LR], const float2* twl, int m) {
    constexpr int R = 1 << LR, NP = tw_powers(S_LO, LR);
    float2 w[NP == R - 1 ? 1 : R];
    // (all powers in the table: each is read where it is used -- sixteen points per lane and their fifteen twiddles at once do not
    // fit the 128 registers of the strided passes)
    auto tw_of = [&](int j) { return twl[((bit_rev(j, LR) - 1) << S_LO) + m]; };
    if constexpr (S_LO > 0) {
        if constexpr (NP != R - 1) {
            w[1] = twl[m];
#pragma unroll
            for (int p = 2; p < R; ++p) w[p] = (p & 1) ? cmul(w[p - 1], w[1]) : cmul(w[p / 2], w[p / 2]);
        }
        if constexpr (INVERSE) {
#pragma unroll
            for (int j = 1; j < R; ++j) v[j] = cmulc(v[j], NP == R - 1 ? tw_of(j) : w[NP == R - 1 ? 0 : bit_rev(j, LR)]);
        }
    }
#pragma unroll
    for (int step = 0; step < LR; ++step) {
        const int bpos = INVERSE ? step : LR - 1 - step;  // local bit handled by this radix-2 stage
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (j & (1 << bpos)) continue;
            const int jl = j & ((1 << bpos) - 1);
            const int k16 = jl * (8 >> bpos);  // jl / 2^(bpos+1) turns = k16 / 16
            const float2 a = v[j], c = v[j | (1 << bpos)];
            if (INVERSE) {
                const float2 t = mul_c16<true>(c, k16);
                v[j] = cadd(a, t);
                v[j | (1 << bpos)] = csub(a, t);
            } else {
                v[j] = cadd(a, c);
                v[j | (1 << bpos)] = mul_c16<false>(csub(a, c), k16);
            }
        }
    }
    if constexpr (S_LO > 0 && !INVERSE) {
#pragma unroll
        for (int j = 1; j < R; ++j) v[j] = cmul(v[j], NP == R - 1 ? tw_of(j) : w[NP == R - 1 ? 0 : bit_rev(j, LR)]);
    }
}

// element of register 0 of group g: the LR-bit register field is inserted at bit S_LO (register j: | (j << S_LO)).  The map is
// a bit permutation, hence OR/XOR-linear: p0(g1 | g2) = p0(g1) | p0(g2) for disjoint g1, g2.
template <int LR, int S_LO>
__host__ __device__ constexpr int group_elem(int g) { return ((g >> S_LO) << (S_LO + LR)) | (g & ((1 << S_LO) - 1)); }

// One super-stage, everything about the transform compile-time: R = 2^LR points per lane, radix-2 stages
// S_LO+LR-1..S_LO (forward, DIF) or S_LO..S_LO+LR-1 (inverse, DIT) on the sequences of the tile.
// twl: the super-stage's LDS table of lane twiddles and their powers (see butterflies).
// LIT (the paired z pass on power-of-two lines, whose tile is a static array): rows are a power of two long (pitch = row length), so
// a row's base and a slot occupy disjoint bits and the BYTE address of register j is the lane's XOR one literal -- one instruction per
// access where slot-then-scale takes two.
template <int LOGN, int LR, int S_LO, bool INVERSE, int NT, int R3, bool LIT = false>
__device__ __forceinline__ void super_stage(float2* tile, int batch, int pitch, int hp, bool priv, const float2* twl) {
    constexpr int R = 1 << LR, H_LO = 1 << S_LO, GL = LOGN - LR, NW = NT / 64;
    if constexpr (GL >= 6) {
        // The group index of a lane is (lane part) | (step part): `coop` lanes work on one sequence (the wave's 64 when rows are
        // private, else min(NT, groups)), so everything that depends on the sequence and on the step is wave-uniform (SALU)
        // and, the swizzle being XOR-linear, a lane's slots are its own constants XOR one scalar per step.
        constexpr int G = 1 << GL;
        const int coop = priv ? 64 : (NT < G ? NT : G);           // power of two >= 64
        const int lid = priv ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
        const int gl = lid & (coop - 1);
        const int a_lane = phys(group_elem<LR, S_LO>(gl));
        const int m_lane = gl & (H_LO - 1);
        // sequences: private rows -> those of the wave's rows; else sequence (lid / coop) + kb * (NT / coop)
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int b0 = priv ? 0 : __builtin_amdgcn_readfirstlane(lid / coop);
        const int bstep = priv ? 1 : NT / coop;
        const int nseq = priv ? (batch / R3) / NW * R3 : batch;
        for (int bl = b0; bl < nseq; bl += bstep) {
            const int rl = bl / R3, sub = bl - rl * R3, rowi = priv ? rl * NW + wave : rl;
            float2* row = tile + rowi * pitch;
            const int s_seq = swz_c(sub << LOGN) ^ rmask(rowi, hp);
#pragma unroll 1
            for (int gk = 0; gk < G; gk += coop) {
                const int a0 = a_lane ^ (s_seq ^ swz_c(group_elem<LR, S_LO>(gk)));
                float2 v[R];
                if constexpr (LIT) {
                    const unsigned ab = ((unsigned)(rowi * pitch) | (unsigned)a0) << 3;
                    const auto reg = [&](int j) -> float2& {
                        return *reinterpret_cast<float2*>(reinterpret_cast<char*>(tile) + (H_LO >= 256 ? ab + (unsigned)(j * H_LO) * 8u : ab ^ ((unsigned)swz_c(j << S_LO) << 3)));
                    };
#pragma unroll
                    for (int j = 0; j < R; ++j) v[j] = reg(j);
                    butterflies<LR, S_LO, INVERSE>(v, twl, m_lane | (gk & (H_LO - 1)));
#pragma unroll
                    for (int j = 0; j < R; ++j) reg(j) = v[j];
                    continue;
                }
#pragma unroll
                for (int j = 0; j < R; ++j) v[j] = H_LO >= 256 ? row[a0 + j * H_LO] : row[a0 ^ swz_c(j << S_LO)];
                butterflies<LR, S_LO, INVERSE>(v, twl, m_lane | (gk & (H_LO - 1)));
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    if (H_LO >= 256) row[a0 + j * H_LO] = v[j];
                    else row[a0 ^ swz_c(j << S_LO)] = v[j];
                }
            }
        }
        return;
    }
    const SeqMap<LOGN, LR, NT, R3> map(batch, priv);
#pragma unroll 1
    for (int u = map.first; u < map.total; u += map.step) {
        int rowi, sub, g;
        map.at(u, rowi, sub, g);
        const int m = g & (H_LO - 1);
        const int p0 = (sub << LOGN) | group_elem<LR, S_LO>(g);  // element of register 0; register j: p0 | (j << S_LO)
        float2* row = tile + rowi * pitch;
        // slot(p0 | J) = slot(p0) ^ swz_c(J) (the swizzle is linear and the j field of p0 is zero); for H_LO >= 256 the j
        // field lies above the swizzled bits and the R slots are slot(p0) + j * H_LO: immediate offsets
        const int a0 = phys(p0) ^ rmask(rowi, hp);
        float2 v[R];
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = H_LO >= 256 ? row[a0 + j * H_LO] : row[a0 ^ swz_c(j << S_LO)];
        butterflies<LR, S_LO, INVERSE>(v, twl, m);
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (H_LO >= 256) row[a0 + j * H_LO] = v[j];
            else row[a0 ^ swz_c(j << S_LO)] = v[j];
        }
    }
}

// full transform of the tile's sequences as the chain of super-stages; twl: the axis' LDS tables.  The caller synchronises
// before (tile and tables filled): with a work-group barrier, or -- PRIV, and the rows were filled by their owners -- not at
// all.  On return the tile is consistent for the work-group (!PRIV) or for each row's owner (PRIV).
template <int LOGN, bool INVERSE, int NT, int R3 = 1, int DONE = 0, int STOP = LOGN, int CUT = 0, bool LIT = false>
__device__ __forceinline__ void lds_fft(float2* tile, int batch, int pitch, int hp, bool priv, const float2* twl) {
    if constexpr (DONE < STOP) {
        constexpr int s_lo = INVERSE ? DONE : seg_below(LOGN, LOGN - DONE, CUT);  // forward: top stages first; inverse: bottom first
        constexpr int r = INVERSE ? seg_r(LOGN, DONE, CUT) : LOGN - DONE - s_lo;
        super_stage<LOGN, r, s_lo, INVERSE, NT, R3, LIT>(tile, batch, pitch, hp, priv, twl + tw_off(LOGN, s_lo, CUT));
        stage_sync(priv);
        lds_fft<LOGN, INVERSE, NT, R3, DONE + r, STOP, CUT, LIT>(tile, batch, pitch, hp, priv, twl);
    }
}

// 3-point DFT in place (forward: exp(-2 pi i /3); inverse: conjugate)
template <bool INVERSE>
__device__ __forceinline__ void dft3(float2& a, float2& b, float2& c) {
    const float hs = 0.86602540378443865f;  // sqrt(3)/2
    const float2 t1 = cadd(b, c);
    const float2 t2 = make_float2(a.x - 0.5f * t1.x, a.y - 0.5f * t1.y);
    const float2 dd = csub(b, c);
    // forward: -i * hs * (b - c) ; inverse: +i * hs * (b - c)
    const float2 t3 = INVERSE ? make_float2(-hs * dd.y, hs * dd.x) : make_float2(hs * dd.y, -hs * dd.x);
    a = cadd(a, t1);
    b = cadd(t2, t3);
    c = csub(t2, t3);
}

// 5-point DFT in place (forward: exp(-2 pi i / 5); inverse: conjugate), in the usual sum / difference form
template <bool INVERSE>
__device__ __forceinline__ void dft5(float2 (&v)[5]) {
    const float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;  // cos(2 pi / 5), cos(4 pi / 5)
    const float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;   // sin(2 pi / 5), sin(4 pi / 5)
    const float2 a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]), b1 = csub(v[1], v[4]), b2 = csub(v[2], v[3]);
    const float2 x0 = v[0];
    const float2 p1 = make_float2(x0.x + c1 * a1.x + c2 * a2.x, x0.y + c1 * a1.y + c2 * a2.y);
    const float2 p2 = make_float2(x0.x + c2 * a1.x + c1 * a2.x, x0.y + c2 * a1.y + c1 * a2.y);
    const float2 q1 = make_float2(s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y);
    const float2 q2 = make_float2(s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y);
    // forward: X[k] = p -+ i q ... with -i q = (q.y, -q.x); inverse: +i q = (-q.y, q.x)
    const float2 iq1 = INVERSE ? make_float2(-q1.y, q1.x) : make_float2(q1.y, -q1.x);
    const float2 iq2 = INVERSE ? make_float2(-q2.y, q2.x) : make_float2(q2.y, -q2.x);
    v[0] = cadd(x0, cadd(a1, a2));
    v[1] = cadd(p1, iq1);
    v[4] = csub(p1, iq1);
    v[2] = cadd(p2, iq2);
    v[3] = csub(p2, iq2);
}

// radix-R3 stage of the y transform on `cols` LDS rows of length M = R3 * Msub: forward = DIF first stage
// (DFT over n1 of x[n1 * Msub + n2], times W_M^(n2 k1), stored at k1 * Msub + n2); inverse = its exact reverse.
// tw3[n2] = exp(-2 pi i n2 / M), n2 < Msub (LDS); the twiddles W_M^(n2 q), q < R3, are its powers.
template <int R3, bool INVERSE, int NT>
__device__ __forceinline__ void radix3_stage(float2* tile, int cols, int pitch, int hp, bool PRIV, int msub, const float2* tw3) {
    constexpr int NW = NT / 64;
    const int wave = threadIdx.x >> 6;
    const int total = PRIV ? (cols / NW) * msub : cols * msub;
    for (int idx = PRIV ? (threadIdx.x & 63) : threadIdx.x; idx < total; idx += PRIV ? 64 : NT) {
        int cl = idx / msub;
        if (msub >= 64) cl = __builtin_amdgcn_readfirstlane(cl);  // msub is a power of two: a wave's 64 items share the row
        const int n2 = idx - cl * msub;
        const int c = PRIV ? cl * NW + wave : cl;
        float2* row = tile + c * pitch;
        float2 v[R3];
        // slot of element q * msub + n2: n2 < msub and the multiples of msub occupy disjoint bits and the swizzle is XOR-linear,
        // so it is the slot of n2 XOR a constant (no per-q address registers)
        const int s0 = phys(n2) ^ rmask(c, hp);
#pragma unroll
        for (int q = 0; q < R3; ++q) v[q] = row[s0 ^ swz_c(q * msub)];
        float2 wq[R3];  // wq[q] = w1^q, by squaring / one multiplication from lower powers (depth <= 3)
        wq[1] = tw3[n2];
#pragma unroll
        for (int q = 2; q < R3; ++q) wq[q] = (q & 1) ? cmul(wq[q - 1], wq[1]) : cmul(wq[q / 2], wq[q / 2]);
        if (INVERSE) {
#pragma unroll
            for (int q = 1; q < R3; ++q) v[q] = cmulc(v[q], wq[q]);
        }
        if constexpr (R3 == 3) {
            dft3<INVERSE>(v[0], v[1], v[2]);
        } else if constexpr (R3 == 5) {
            dft5<INVERSE>(v);
        } else {  // 9 = 3 x 3: index n = 3 n1 + n2' , k = k1' + 3 k2'
            // DIF order for the forward transform, reversed for the inverse (which takes k-ordered input)
            if constexpr (!INVERSE) {
#pragma unroll
                for (int r = 0; r < 3; ++r) dft3<false>(v[r], v[r + 3], v[r + 6]);       // over n1 (stride 3): -> A[n2'][k1'] at r + 3 k1'
                const float c9[3] = {1.0f, 0.76604444311897801f, 0.17364817766693033f};   // cos(2 pi {0,1,2}/9)
                const float s9[3] = {0.0f, 0.64278760968653933f, 0.98480775301220802f};   // sin(2 pi {0,1,2}/9)
                const float c94 = -0.93969262078590843f, s94 = 0.34202014332566871f;      // 4/9 turn
                v[4] = cmul(v[4], make_float2(c9[1], -s9[1]));   // n2'=1,k1'=1: W9^1
                v[7] = cmul(v[7], make_float2(c9[2], -s9[2]));   // n2'=1,k1'=2: W9^2
                v[5] = cmul(v[5], make_float2(c9[2], -s9[2]));   // n2'=2,k1'=1: W9^2
                v[8] = cmul(v[8], make_float2(c94, -s94));       // n2'=2,k1'=2: W9^4
                // over n2' for each k1': inputs v[0 + 3k1'], v[1 + 3k1'], v[2 + 3k1'] -> X[k1' + 3 k2'] for k2' = 0,1,2
#pragma unroll
                for (int k1 = 0; k1 < 3; ++k1) dft3<false>(v[3 * k1], v[3 * k1 + 1], v[3 * k1 + 2]);
                // now v[3 k1' + k2'] = X[k1' + 3 k2'] : reorder to k order
                float2 t[9];
#pragma unroll
                for (int k1 = 0; k1 < 3; ++k1)
#pragma unroll
                    for (int k2 = 0; k2 < 3; ++k2) t[k1 + 3 * k2] = v[3 * k1 + k2];
#pragma unroll
                for (int q = 0; q < 9; ++q) v[q] = t[q];
            } else {
                float2 t[9];
#pragma unroll
                for (int k1 = 0; k1 < 3; ++k1)
#pragma unroll
                    for (int k2 = 0; k2 < 3; ++k2) t[3 * k1 + k2] = v[k1 + 3 * k2];
#pragma unroll
                for (int q = 0; q < 9; ++q) v[q] = t[q];
#pragma unroll
                for (int k1 = 0; k1 < 3; ++k1) dft3<true>(v[3 * k1], v[3 * k1 + 1], v[3 * k1 + 2]);
                const float c9[3] = {1.0f, 0.76604444311897801f, 0.17364817766693033f};
                const float s9[3] = {0.0f, 0.64278760968653933f, 0.98480775301220802f};
                const float c94 = -0.93969262078590843f, s94 = 0.34202014332566871f;
                v[4] = cmul(v[4], make_float2(c9[1], s9[1]));
                v[7] = cmul(v[7], make_float2(c9[2], s9[2]));
                v[5] = cmul(v[5], make_float2(c9[2], s9[2]));
                v[8] = cmul(v[8], make_float2(c94, s94));
#pragma unroll
                for (int r = 0; r < 3; ++r) dft3<true>(v[r], v[r + 3], v[r + 6]);
            }
        }
        if (!INVERSE) {
#pragma unroll
            for (int q = 1; q < R3; ++q) v[q] = cmul(v[q], wq[q]);
        }
#pragma unroll
        for (int q = 0; q < R3; ++q) row[s0 ^ swz_c(q * msub)] = v[q];
    }
}

// slot of element e in row `row` of a tile (in float2 units from the tile start)
__device__ __forceinline__ int cell(int row, int pitch, int hp, int e) { return row * pitch + (phys(e) ^ rmask(row, hp)); }

// ------------------------------------------------------------------------------------------------ host side of the units
template <class K, class... Args>
int launch_lds(K kernel, unsigned grid, int threads, size_t lds, hipStream_t s, const char* name, Args... args) {
    if (lds > 64 * 1024)
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, args...);
    return launch_check(name);
}

// ---- launch dispatch: the kernels are templated on (log2 of the power-of-two part, radix-3/9 factor) of their axis;
// key = l2 * 16 + r3
// One switch per case list of the length table (fft_native_route.h): f -- a generic lambda that names the kernel -- is called with
// the (LG, R) of the axis as std::integral_constant arguments and its result returned; a length outside the list is the
// "unsupported" failure.
template <int V>
using Int = std::integral_constant<int, V>;
#define MI_CASE_CALL(LG, R) case LG * 16 + R: return f(Int<LG>{}, Int<R>{});
template <class F>
int x_case(const NativeDims& d, F&& f) {
    switch (d.lhx2 * 16 + d.r3x) { MI_AXIS_CASES(MI_CASE_CALL) default: return fail(MI_ERR_UNSUPPORTED, "native FFT: x length %d", 2 * d.hx); }
}
template <class F>
int y_case(const NativeDims& d, F&& f) {
    switch (d.ly2 * 16 + d.r3) { MI_Y_CASES(MI_CASE_CALL) default: return fail(MI_ERR_UNSUPPORTED, "native FFT: y length %d", d.ny); }
}
#undef MI_CASE_CALL
// (z: no kernel is built for the lengths beyond kMaxZ)
#define MI_CASE_CALL(LG, R) case LG * 16 + R: if constexpr (axis_takes(2, LG, R)) return f(Int<LG>{}, Int<R>{}); else break;
template <class F>
int z_case(const NativeDims& d, F&& f) {
    switch (d.lz2 * 16 + d.r3z) { MI_AXIS_CASES(MI_CASE_CALL) default: break; }
    return fail(MI_ERR_UNSUPPORTED, "native FFT: z length %d", d.nz);
}
#undef MI_CASE_CALL

}  // namespace
}  // namespace mi
