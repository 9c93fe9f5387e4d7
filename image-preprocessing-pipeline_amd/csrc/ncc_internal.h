// MIP-NCC (TeraStitcher's crossmips) inside the library: the types and functions its translation units share -- ncc_mips.hip (the six
// MIPs of a pair), ncc_pair.hip (the per-pair path), ncc_rules.hip (host rules, geometry of a pair), ncc_lag_fft.hip (cross terms of every
// shift through a lag transform), ncc_lag.hip (the batched pipeline around it), ncc.hip (C ABI, batch orchestration).  Device code: ncc_dev.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "mi_crossmips.h"
#include "mi_internal.h"

namespace fft64 { struct Plan; }

namespace mi {

constexpr int TILE = 32;  // TILE_SIDE, compute_funcs.h:66
constexpr int MIP_KPW = 8;    // slices per wave whose column maxima stay in registers (stacks of up to 32 slices)
constexpr int MIP_NB = 4;     // row bands per work-group in that case
constexpr int MIP_ROWS = 16;
constexpr int MEAN_PARTS = 64;  // slices the pixel sums of a MIP are taken in (k_mip_partial)

inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }
inline int grow(DevBuf& b, size_t bytes) { return b.bytes >= bytes ? MI_OK : b.alloc(bytes); }

// Sample format of the tiles: float (iom::real_t, the reference's) or the 8 / 16-bit integers they were loaded from (k_mips_int), with
// the divisor that turns those into the reference's floats.  Tile pointers travel as `const float*` either way.
struct TileFmt {
    int bytes = 4;  // 4: float; 2 / 1: the integer samples the tiles were loaded from
    float scale = 65535.0f;
};

struct PlaneGeom {  // one of the three MIP planes
    int dimu, dimv;     // MIP extents
    int delayu, delayv; // search half ranges
    int wu, wv;         // window half extents (wRangeThr)
    size_t mip1, mip2, ps1, ps2, map;  // float offsets inside the workspace
    size_t sat;                        // double offset of this plane's summed-area tables inside the per-pair workspace
    bool tiled;
};

struct PairPlan {
    int dimk, dimi_v, dimj_v;
    int delayi, delayj, delayk;
    int ai0, aj0;
    PlaneGeom g[3];
    size_t total_floats, map_floats, map_begin, res_floats, sat_doubles;
};

// layout of one plane's tables (doubles): c0a, c0b | P1 | Q1 | P2 | Q2 | TS1 | TS2
struct SatLayout {
    size_t tab, ts, total;
    SatLayout(int dimu, int dimv) {
        tab = (size_t)(dimu + 1) * (dimv + 1);
        ts = (size_t)(dimu / TILE + 1) * (dimv / TILE + 1);
        total = 2 + 4 * tab + 2 * ts + 2 * MEAN_PARTS;  // c0a, c0b | P1 Q1 P2 Q2 | TS1 TS2 | partial pixel sums
    }
};

// ------------------------------------------------------------------------------------------------ ncc.hip
// cumulative counters behind mi_ncc_stats: pairs finished by the batched pipeline, pairs finished by the per-pair (careful)
// path, entries recomputed in the two-pass form
void ncc_count(int which, long long n);

// ------------------------------------------------------------------------------------------------ ncc_rules.hip
// resolution below which a decision is not taken on lag-transform / summed-area-table values (MI_NCC_MARGIN, default 4e-6)
float ncc_margin();
int argmax_first(const float* v, int len);
// `tight` (optional) receives the smallest margin, in NCC units, by which any comparison or rounding step was decided
int peak_half_width(const mi_ncc_params& P, const float* M, int ind, int step, int range, int second_bound, float* tight = nullptr);
void combine_axis(const mi_ncc_params& P, mi_ncc_descr* R, int ax, int d1, float p1, int w1, int d2, float p2, int w2, float* tight = nullptr);
int plan_pair(int dimk, int dimi, int dimj, int nk, int ni, int nj, int delayk, int delayi, int delayj, int side, mi_ncc_params* p, PairPlan& pl);

// ------------------------------------------------------------------------------------------------ ncc_mips.hip
// floats per pair that launch_mips needs as `tmp`
size_t mips_tmp_floats(int dimk, int dimi_v, int dimj_v);
bool mips_int_ok(int bytes, int dimk, int pitch, size_t slice);
// The six MIPs of `np` pairs (np == 1 and tab == nullptr: the pair A, B).  xy_done: recorded when the MIPs of k_mips5 / k_mips_int
// are final (deep stacks: the xy MIPs).  xyT, beside_chain: see k_mips and the definition.  timed: the pass alone, as
// mi_ncc_time_mips measures it -- no zeroing launch, no reductions of a deep stack's partial maxima.
int launch_mips(hipStream_t s, const float* A, const float* B, const float* const* tab, int np, size_t pstride, int dimk, int dimi_v, int dimj_v,
                size_t slice, int pitch, int ai0, int aj0, float* xy1, float* xz1, float* yz1, float* xy2, float* xz2, float* yz2, float* tmp,
                hipEvent_t xy_done = nullptr, TileFmt fmt = TileFmt(), float* xyT = nullptr, size_t tstride = 0, bool beside_chain = false,
                bool timed = false);
// average duration of ONE such pass over n pairs (HIP events on `s` around `reps` launches; the bench's roofline hook)
int ncc_time_mips(hipStream_t s, int n, const float* const* a_ptrs, const float* const* b_ptrs, int dimk, int dimi, int dimj, int ni, int nj, int side,
                  int reps, float* ms, TileFmt fmt = TileFmt());

// ------------------------------------------------------------------------------------------------ ncc_pair.hip
// the per-pair path of one pair on `s` (also the careful path of pairs the batched pipeline hands back)
int pair_direct(hipStream_t s, const float* A, const float* B, int dimk, int dimi, int dimj, int ni, int nj, int delayk, int delayi, int delayj,
                int side, mi_ncc_params* p, mi_ncc_descr* out);
// the full NCC map of one pair of MIPs, shift by shift; synchronises `s`
int pair_map(hipStream_t s, const float* mip1, const float* mip2, int dimu, int dimv, int delayu, int delayv, float* map);
// A pair's working set between batch calls: workspace + stream, per device.  take: from the cache or new, null when there is no
// memory or no stream; give: back into the cache.  A slot that is not given back is destroyed with its stream.
struct PairSlot;
struct PairSlotDelete { void operator()(PairSlot* slot) const; };
typedef std::unique_ptr<PairSlot, PairSlotDelete> PairSlotPtr;
PairSlotPtr take_pair_slot(int dev);
void give_pair_slot(PairSlotPtr slot);
hipStream_t pair_slot_stream(const PairSlot& slot);
// the two stages of a pair on its slot's stream: enqueue everything up to the D2H copy of the NCC maps; wait and run the host logic
int pair_enqueue(PairSlot& slot, const float* A, const float* B, int dimi, int dimj, const PairPlan& pl, TileFmt fmt = TileFmt());
int pair_finish(PairSlot& slot, int ni, int nj, int side, mi_ncc_params* p, const PairPlan& pl, mi_ncc_descr* out);

// ------------------------------------------------------------------------------------------------ ncc_lag_fft.hip
struct LagPlane {
    bool long_is_u;
    int n_long, n_short, ls, ss, El, Es, Eu, Ev;
    const fft64::Plan *fft, *cfft;  // along the long axis (N points); along the short axis (use_corr).  They live as long as the process.
    bool use_corr;
    int N, KT, JP, FW, TW, LB, nlp, fft_threads;
    size_t lds_fft, lds_mac, lds_corr, lds_refine;
    bool ok;
};
LagPlane plan_lag_plane(const PlaneGeom& g, int maxIter);
// cross terms of `np` pairs of one plane through the lag transform (MIPs at m1 / m2 + q * pstride) into `cross`; SP and CH: scratch
int lag_cross(int dev, hipStream_t s, const LagPlane& lp, const float* m1, const float* m2, size_t pstride, int np, DevBuf& SP, DevBuf& CH,
              DevBuf& cross, hipEvent_t after_fwd = nullptr);

// ------------------------------------------------------------------------------------------------ ncc_lag.hip
// whether every plane of this geometry fits the lag transform (FFT length <= 8192, LDS)
bool ncc_lag_supported(int dimk, int dimi, int dimj, int ni, int nj, int delayk, int delayi, int delayj, int side, const mi_ncc_params* p);
// n pairs of one geometry in two steps, so that several groups can be in flight: enqueue the device stage (on streams of the job's
// own, behind what `s` holds so far), then wait for it and run the host rules.  careful[q] != 0: pair q must be redone by the
// per-pair path, out[q] untouched.  A job that is not finished must be abandoned.
struct LagJob;
// groups_in_flight: how many groups the caller keeps enqueued at once -- they share the device-memory budget of a chunk
// (MI_NCC_CHUNK_MB); concurrent callers on one device share its three streams and serialise on them.
// defer_chains: only the MIP pass is enqueued; the caller enqueues the chains of all its jobs afterwards (ncc_lag_enqueue_chains)
// behind an event it records on the MIP stream after the last job's MIP pass
// chain_beside: an earlier group's chain is still running when this group's MIP pass starts (launch_mips)
int ncc_lag_enqueue(int dev, hipStream_t s, int n, const float* const* a_ptrs, const float* const* b_ptrs, int dimk, int dimi, int dimj, int ni,
                    int nj, int delayk, int delayi, int delayj, int side, mi_ncc_params* params, LagJob** job, bool defer_chains = false,
                    TileFmt fmt = TileFmt(), int groups_in_flight = 1, bool chain_beside = false);
int ncc_lag_enqueue_chains(LagJob* job, hipEvent_t gate);
hipStream_t ncc_lag_mip_stream(LagJob* job);
int ncc_lag_finish(LagJob* job, mi_ncc_params* params, mi_ncc_descr* out, unsigned char* careful);
void ncc_lag_abandon(LagJob* job);
// both steps at once
int ncc_lag_group(int dev, hipStream_t s, int n, const float* const* a_ptrs, const float* const* b_ptrs, int dimk, int dimi, int dimj, int ni,
                  int nj, int delayk, int delayi, int delayj, int side, mi_ncc_params* params, mi_ncc_descr* out, unsigned char* careful,
                  TileFmt fmt = TileFmt());
int ncc_lag_map(int dev, hipStream_t s, const float* mip1, const float* mip2, int dimu, int dimv, int delayu, int delayv, float* map);
void ncc_lag_drop_cached(int dev);

}  // namespace mi
