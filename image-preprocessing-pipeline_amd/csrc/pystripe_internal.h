// pystripe tile preprocessing (pystripe/core.py process_img :1190, filter_streaks :982, filter_subband :927-940,
// np_filter_coefficient :749) on batches of equally shaped 2-D tiles: the plan and the launchers its translation units share.  Every
// launch covers the whole batch (grid z / y = tile): one 2048^2 tile leaves most of the device idle at the deep wavelet levels.
// Each kernel is compiled in one unit; the units talk through the host launchers declared below.  Device code: pystripe_dev.h.
//
//   load      (pystripe_wavelet.hip) the first analysis level reads the tile itself: integer load, log1p and the numpy.pad index map
//             (reflect / wrap / symmetric / edge) are folded into its addressing, so the padded image is never written.  The row pass
//             runs over the SOURCE rows only; the column pass looks rows up through the same map.
//   pad       (pystripe_pad.hip) the value modes of numpy.pad (constant, linear_ramp, maximum, minimum, mean, median) are no index
//             maps: the row and column statistics of the log image (one pass for max / min / mean, a radix selection per line for the
//             median), their corner value, then the padded log image itself, which the first level reads as it lies.
//   analysis  (pystripe_wavelet.hip) out[i] = sum_t F[t] in[sym(2 i + 1 - t)], floor((n + 17) / 2) coefficients ('symmetric', db9);
//             rows then columns: L, H along axis -1, then A, cH (from L) and cV, cD (from H) along axis -2 -- cH is the high-pass along
//             axis -2 of the low-pass along axis -1, PyWavelets' 'da'.
//   notch     (pystripe_notch.hip) np_filter_coefficient multiplies scipy.fftpack.rfft's packed spectrum [r0, r1, i1, r2, i2, ...] by
//             g[j] = 1 - exp(-j^2 / (2 s^2)) BY PACKED POSITION (real part of bin k: g[2k-1], imaginary part: g[2k]), so it is not a
//             convolution.  1 - g[j] is exactly 0 in float32 beyond j ~ 5.9 s: evaluated as c - irfft((1 - g) * rfft(c)) over those low
//             positions only, as direct sums in float64 folded over the j <-> n - j symmetry of the twiddles (up to four lines, the
//             twiddle table and their kept spectrum stay in LDS).
//   synthesis (pystripe_wavelet.hip) out[j] = sum_k a[k] Lo_R[j + 16 - 2 k] + d[k] Hi_R[j + 16 - 2 k]; a thread makes the pair
//             (2p, 2p + 1), which shares its nine k.  waverec2's trim of the approximation is a smaller extent read with the wider stride.
//   store     (sink_store, pystripe_dev.h) the last synthesis level computes only the un-padded window and finishes every sample in
//             registers: expm1, rint + clip (integer tiles), dark, 8 / 16-bit conversion, flip and rotation in the store address.
//   bleach    (pystripe_bleach.hip) correct_bleaching (:501): with it on, the last synthesis level stores the log image L instead (at
//             sigma == (0, 0) L is log1p on load and never stored); a work-group per row runs sosfiltfilt's forward-backward
//             first-order recurrence in float64 as a scan of affine maps over the clipped, odd-extended row in LDS and writes F and its
//             row maximum; a block per tile reduces the maxima; the apply pass hands (L / F) * max F to the same store.
//   clips     (pystripe_clips.hip) a clip given as NaN: threshold_multiotsu(log1p(tile), 4) per tile before anything else of the run:
//             range and 256-bin histogram of the source read through src_load, the search and edges of thresholds.hip, a triple and a
//             status per tile in device memory; the row filter takes its clips from there.
//   wavelets  the kernels named above are db9's (mi_pystripe_plan_create); mi_pystripe_plan_create_wavelet runs their counterparts for
//             any even tap count up to MI_PS_MAX_TAPS (the *_gen_kernel family of pystripe_wavelet.hip): same load, notch, store and
//             bleach route.
//   pystripe.hip: uniform tiles, flat field / down-sample, the filter-less path, the plan (derive), run_chunk and the C ABI.
#pragma once
#include <vector>

#include "mi_internal.h"
#include "pystripe_dev.h"

namespace mi {
namespace ps {

constexpr int kMinLength = 34;   // filter_streaks :1092
constexpr int kTabPad = 8;       // zeros on either side of a filter in the generic kernels' table

constexpr int kBleachExt = 6;                         // sosfiltfilt's padlen for one section
constexpr int kBleachMaxThreads = 1024;
constexpr size_t kBleachLds = 160 * 1024;              // all of a CU's LDS
constexpr size_t kBleachTotals = (kBleachMaxThreads / 64) * sizeof(double2);   // the scan's wave totals, behind the row
constexpr int kBleachSeg = (int)((kBleachLds - kBleachTotals) / sizeof(double));   // doubles of a row (or of a segment of it) in LDS
static_assert(kBleachSeg - 2 * kBleachExt == MI_PS_BLEACH_LDS_ROW, "MI_PS_BLEACH_LDS_ROW is derived from the LDS request");

// the work space of run_auto_clips per tile
constexpr size_t kAutoBytesPerTile = MI_HIST_BINS * 8 + 8 + (MI_HIST_BINS + 1) * 4 + 2 * 4 + (MI_OTSU_MAX_CLASSES - 1) * 4 + 3 * 4;

struct Bleach {
    double b, a;              // y = b u + z;  z' = b u + a y
    float lo, med, hi;        // G = clip(L == 0 ? med : L, lo, hi)
    const float* clips;       // automatic clips: [tile][3] = lo, med, hi in device memory, instead of the three above; else null
};

struct NotchTab {          // one (pass, level, axis)
    int n, kp, kb, R, threads;
    size_t lds;
    size_t tw_off, w_off;  // into the plan's table buffers (elements)
};

struct Plan {
    int dev = 0, in_ny = 0, in_nx = 0, in_dtype = 0;
    mi_pystripe_params prm{};
    mi_pystripe_info info{};
    bool filter = false, pre = false, bleach = false;
    int passes = 0;
    Bleach bq{};
    Filters f{};
    int L = LF;               // taps; generic: the run-time-length kernels with their filter table (mi_pystripe_plan_create_wavelet)
    bool generic = false;
    DevBuf tab_buf;
    int h[MI_PS_MAX_LEVELS + 1] = {0}, w[MI_PS_MAX_LEVELS + 1] = {0};   // extents per level, [0] = padded image
    // per-tile scratch, offsets in floats
    size_t off_stage = 0, off_P = 0, off_rowL = 0, off_rowH = 0, off_A[MI_PS_MAX_LEVELS + 1] = {0}, off_cH[MI_PS_MAX_LEVELS + 1] = {0},
           off_cV[MI_PS_MAX_LEVELS + 1] = {0}, off_cD[MI_PS_MAX_LEVELS + 1] = {0};
    size_t sz_stage = 0, sz_P = 0, sz_row = 0, sz_A[MI_PS_MAX_LEVELS + 1] = {0}, sz_d[MI_PS_MAX_LEVELS + 1] = {0};
    // bleach correction: the log image (with a stripe filter), F and its row maxima, or (max method) the maxima keys and the filtered
    // vectors, rows first; the tile maximum; the forward result of lines too long for LDS (doubles, two floats each)
    size_t off_L = 0, off_F = 0, off_lmax = 0, off_key = 0, off_vec = 0, off_M = 0, off_fwd = 0;
    size_t sz_L = 0, sz_F = 0, sz_lmax = 0, sz_vec = 0, sz_fwd = 0;
    // value padding (the padded image itself is P): [row statistics ny | column statistics nx | corner], or the tile's constant
    // alone (log1p of its estimated clip_min); the row partials of the statistics pass (doubles, two floats each)
    bool valpad = false;
    size_t off_pvec = 0, off_ppart = 0, sz_pvec = 0, sz_ppart = 0;
    std::vector<NotchTab> tabs;   // [pass][level 1..L][axis 0: cH along -1, 1: cV along -2]
    DevBuf tw_buf, w_buf, scratch, varies;
    i64 cap = 0;
    // automatic clips: the work space of the estimate for `cap` tiles; the triples and the status of every tile of the last run
    // (clips_cap tiles); the log1p table of integer tiles
    DevBuf auto_buf, clips_buf, status_buf, table_buf;
    i64 clips_cap = 0, last_count = 0;
    int ncodes = 0;
    int au = 0;               // MI_PS_AUTO_* of the clips that are NaN

    float* buf(size_t off) const { return scratch.as<float>() + (i64)off * cap; }   // buffer b of all tiles: [tile][size_b]
};

// The dynamic-LDS limit is an attribute of the kernel, not of a plan: it is set right before every launch that needs more than the
// default, to that launch's own need (several plans of different shapes live side by side in batch_filter).
inline int raise_lds(const void* kernel, size_t lds) {
    if (lds > 48 * 1024) MI_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MI_OK;
}

// pystripe_wavelet.hip.  Level l of the plan's pyramid, db9's kernels or the generic ones by P.generic.
// analysis: rows then columns of `s` (the tile through its padding map, or a float image) -> A, cH, cV, cD of level l
int launch_analysis(const Plan& P, hipStream_t st, int l, const Src& s, int cnt);
// synthesis: columns then rows of level l into the level above; fin: only the un-padded window, through the sink
int launch_synthesis(const Plan& P, hipStream_t st, int l, bool fin, const Sink& k, int cnt);
// the four filters of the orthogonal wavelet with the reconstruction low-pass rec_lo[P.L], for the generic kernels
int upload_filter_table(Plan& P, const double* rec_lo);

// pystripe_pad.hip: a value padding mode (P.valpad): the padded log image of the cnt tiles behind `src` into the plan's P
int run_value_pad(const Plan& P, hipStream_t st, Src src, int cnt);

// pystripe_notch.hip: the tables of every (pass, level, axis), and the notch on nlines lines (element stride es, line stride ls)
int build_tables(Plan& P);
int run_notch(const Plan& P, hipStream_t st, const NotchTab& t, float* c, i64 tile_stride, int nlines, i64 es, i64 ls, int cnt);

// pystripe_bleach.hip: correct_bleaching on the log image behind `L` (the tile through log1p, or the stripe filter's stored result),
// into the sink
int run_bleach(const Plan& P, hipStream_t st, const Src& L, const Sink& k, int cnt);

// pystripe_clips.hip.  The clips of the cnt tiles behind `src` (the tile after flat and down_sample, not yet in the log domain)
// into clips[cnt][3] and status[cnt]; the log1p table of an integer tile's clips: the caller's, or libm's log1pf of every code
int run_auto_clips(const Plan& P, hipStream_t st, Src src, int cnt, int* varies, float* clips, int* status);
int upload_log_table(Plan& P, const float* table);

}  // namespace ps
}  // namespace mi
