/* mi_pystripe.h -- pystripe tile preprocessing: the wavelet-FFT stripe filter and the per-tile conversions around it, on
 * batches of equally shaped 2-D tiles in device memory.
 *
 * Replaces, for the options process_images.py uses, pystripe/core.py:
 *   process_img            :1190-1381  (uniform tile, flat, down_sample, filter_streaks, dark, 8/16-bit conversion, flip, rotate)
 *   filter_streaks         :982-1159   (log1p, padding, filter_streak_dual_band, crop, bleach correction, expm1, rint + clip for
 *                                       integer tiles)
 *   correct_bleaching      :501-559, butter_lowpass_filter :492-498  (with explicit clips; see "Bleach correction" below)
 *   filter_streak_dual_band:943-979    (sigma1 == sigma2: one filter_subband; else one after the other)
 *   filter_subband         :927-940    (numpy branch: wavedec2 'symmetric', np_filter_coefficient on cH and cV, waverec2; db9 by
 *                                       mi_pystripe_plan_create, any orthogonal wavelet of up to MI_PS_MAX_TAPS taps by
 *                                       mi_pystripe_plan_create_wavelet; see "Wavelets" below)
 *   np_filter_coefficient  :749-754, np_notch :637-667  (gains applied by PACKED position of scipy.fftpack.rfft's real spectrum)
 *   calculate_pad_size     :681-698, notch_rise_point :670-678, convert_to_8bit_fun :402-425, convert_to_16bit_fun :397-399,
 *   is_uniform_2d          :107-121,  calculate_down_sampled_size :1162-1170
 * skimage.measure.block_reduce (zero padding to a multiple of the block) is restated for max / min / mean.
 *
 * skimage.measure.block_reduce with numpy.median: blocks of up to MI_PS_MEDIAN_MAX_BLOCK samples, an even count gives the mean of the
 * two middle values; a NaN sorts by fminf / fmaxf, not as numpy sorts it.
 *
 * The foreground mask of filter_streaks (enable_masking, get_img_mask :475-489) is mi_tile_mask.h; the Python layer runs it in front
 * of a plan of this header, behind extended=True, and hands that plan the clips explicitly.  Its box window follows OpenCV's
 * documented formula (an even box moves content by one sample); agreement with cv2 itself is not verified.
 * Not built (refused by the Python layer by name): dark-edge
 * exclusion, biorthogonal wavelets and wavelets named without a table (the library holds the Daubechies family only; the
 * Python layer takes any other orthogonal wavelet as its coefficients), the padding mode 'empty'.
 * The lightsheet correction of process_img :1333-1348 is mi_lightsheet.h; the Python layer runs it between two
 * plans of this header, and so it does with the resize to new_size (:1356-1359), which is mi_tile_resize.h.
 *
 * Automatic clips (a clip given as NaN; filter_streaks :1066-1077): threshold_multiotsu(log1p(tile), classes=4) per tile, inside the run,
 * of the tile after flat and down_sample and before padding and the stripe filter; the log image is not stored for it.  Two passes
 * read the source: the finite range, then numpy.histogram(., 256) with the edges of mi_thresholds.h; the four-class search of
 * mi_thresholds.h follows, and the thresholds are the float32 centres (edges[i] + edges[i + 1]) / 2 of the bins it names.  For an
 * integer-kind tile the value of a sample is table[code] (mi_pystripe_plan_set_log_table), so the counts are those of
 * numpy.histogram(log1p(codes)) exactly; for a float tile it is log1pf on load, as the filter reads it.  Given clips keep their
 * slot, min is raised to log1p(1), and the asserts of correct_bleaching run on the result.  A tile whose status is 1, 2 or 3 is
 * written as zeros; the run returns MI_OK, reads nothing back and does not wait.
 *
 * Bleach correction (bleach_frequency > 0), on the float32 log-domain image L (the stripe filter's cropped result, or log1p(tile)
 * when sigma == (0, 0)), just before expm1:
 *   G  = L with exact zeros replaced by clip_med, limited to [max(clip_min, log1p(1)), clip_max] (the bounds as float32);
 *   F  = every row of G through scipy's sosfiltfilt(butter(1, frequency, 'sos'), .) in float64, stored as float32: the row is
 *        extended by 6 samples per side (odd extension), then y[i] = b u[i] + z, z = b u[i] + a y[i] runs forward from
 *        z = (1 - b) u[0] and once more backward over the result, with k = tan(pi frequency / 2), b = k / (1 + k),
 *        a = (1 - k) / (1 + k);
 *        max_method: the row maxima and column maxima of L go through the same clip and filter over their own length, and
 *        F[y][x] = ry[y] * cx[x] (a float32 product, never stored);
 *   L' = (L / F) * max(F) in float32, the maximum over the tile; then the tail as before.
 *
 * Wavelets.  A wavelet is its reconstruction low-pass rec_lo[L], L even; hi_r[t] = (-1)^t rec_lo[L - 1 - t] and the decomposition
 * pair is the reversed reconstruction pair.  PyWavelets' wavedec2 / waverec2, mode 'symmetric': an extent n gives (n + L - 1) / 2
 * coefficients, m coefficients reconstruct 2 m - L + 2 samples, and the automatic level (params.level == 0) is the minimum over both
 * padded extents of floor(log2(n / (L - 1))), 0 when n < L - 1.  At level 0 the filter leaves the log image as it is (info.levels
 * == 0; log1p, expm1 and everything behind them still run).  An explicit level beyond the automatic one is allowed: the symmetric
 * extension then reflects more than once and a coefficient line may be as short as L / 2 samples.  The 34-sample minimum and
 * calculate_pad_size do not depend on the wavelet.  Which kernels run is decided by the entry alone: mi_pystripe_plan_create runs
 * the db9 kernels (18 taps unrolled, filters in scalar registers); mi_pystripe_plan_create_wavelet runs the kernels with a
 * run-time tap count (filter table in device memory, column passes staged in LDS), also when rec_lo holds the 18 db9 values.
 *
 * Value padding (MI_PS_CONSTANT .. MI_PS_MINIMUM; filter_streaks :1088-1110, numpy.pad's semantics on the float32 log image L with
 * the pad widths ((base_pad, base_pad + pad_y), (base_pad, base_pad + pad_x))): the padded image is written once per run and the first
 * level reads it; reflect / wrap / symmetric / edge stay index maps and write none.  Axis 0 is padded first, then axis 1 over all rows:
 *   maximum / minimum / mean / median  the pad rows hold the statistic of every column of L, the pad columns of a row that row's
 *             statistic over its nx un-padded samples, so a corner holds the statistic of the column statistics.  The mean is
 *             accumulated in float64; the median of an even count is the float32 mean of the two middle samples.  A line of up to
 *             MI_PS_PAD_LDS_LINE samples is selected in LDS, a longer one by radix passes over global memory;
 *   linear_ramp  from 0 at the outer edge: sample k of a front pad of width p is edge * k / p, sample k of a back pad of width p'
 *             (counted from the tile) edge * (p' - 1 - k) / p'; axis 1 ramps the ramped pad rows;
 *   constant  log1p(bleach_clip_min), also when bleach_frequency is 0 (the one case in which a clip is looked at without a
 *             frequency; a zeroed field pads with 0): the clip is in log units and the reference takes the logarithm once more.  When
 *             bleach_clip_min is estimated per tile (bleach_frequency > 0 and a NaN), log1p of that tile's estimate BEFORE it is
 *             raised to log1p(1) -- mi_pystripe_plan_clips reports the raised one.  The struct has no field of its own for it.
 *
 * A row (or maxima vector) of n samples stays in LDS as n + 12 doubles while n <= MI_PS_BLEACH_LDS_ROW; a longer one goes through
 * LDS in segments with the carried filter state and a float64 scratch row for the forward result.
 */
#ifndef MI_PYSTRIPE_H
#define MI_PYSTRIPE_H

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MI_PS_U8 = 0, MI_PS_U16 = 1, MI_PS_F32 = 2 } mi_pystripe_dtype;
/* numpy.pad modes.  The first four are index maps (a padded sample is a copy of a source sample); the others are value modes: see
 * "Value padding" above */
typedef enum {
    MI_PS_REFLECT = 0, MI_PS_WRAP = 1, MI_PS_SYMMETRIC = 2, MI_PS_EDGE = 3,
    MI_PS_CONSTANT = 4, MI_PS_LINEAR_RAMP = 5, MI_PS_MAXIMUM = 6, MI_PS_MEAN = 7, MI_PS_MEDIAN = 8, MI_PS_MINIMUM = 9
} mi_pystripe_padding;
typedef enum { MI_PS_DOWN_MAX = 0, MI_PS_DOWN_MIN = 1, MI_PS_DOWN_MEAN = 2, MI_PS_DOWN_MEDIAN = 3 } mi_pystripe_down;
#define MI_PS_MEDIAN_MAX_BLOCK 64   /* samples of a median block (down_y * down_x): they are sorted in registers */
/* the clips estimated per tile (those given as NaN), as bits: what the Python layer reports as bleach_auto */
#define MI_PS_AUTO_MIN 1
#define MI_PS_AUTO_MED 2
#define MI_PS_AUTO_MAX 4
/* status of a tile's clips (mi_pystripe_plan_clips) */
typedef enum {
    MI_PS_CLIPS_UNIFORM = -1,     /* uniform tile: zeros, nothing estimated */
    MI_PS_CLIPS_OK = 0,
    MI_PS_CLIPS_TOO_FEW = 1,      /* fewer than four occupied bins (threshold_multiotsu's ValueError) */
    MI_PS_CLIPS_ORDER = 2,        /* not 0 <= min < med < max (the asserts of correct_bleaching) */
    MI_PS_CLIPS_NONFINITE = 3     /* the log image holds a NaN or an infinity (numpy.histogram's ValueError) */
} mi_pystripe_clip_status;
#define MI_PS_MAX_LEVELS 24
#define MI_PS_MAX_TAPS 128
/* bleach correction: the longest row whose n + 12 doubles fit the LDS of one work-group beside the 16 wave totals of the scan:
 * (160 KiB - 16 * 16 B) / 8 B - 12 */
#define MI_PS_BLEACH_LDS_ROW 20436
/* median padding: the longest line whose keys stay in LDS beside the 256 digit counts and 16 control words of the selection.  A
 * work-group takes a quarter of a CU's 160 KiB, so that four of them share a CU: 40 KiB / 4 B - 256 - 16.  (The notch kernel bounds a
 * coefficient line to 8191 samples and with it a padded extent to 16365: a limit of all 160 KiB would never be passed.) */
#define MI_PS_PAD_LDS_LINE 9968

typedef struct {
    double sigma1, sigma2;     /* (0, 0): no stripe filter; both > 0 otherwise ("sigma must be positive", np_notch :654) */
    int level;                 /* 0: min over both padded extents of floor(log2(n / (taps - 1))), taps = 18 for db9 */
    int padding_mode;          /* mi_pystripe_padding */
    int bidirectional;         /* also filter cV along axis -2 */
    int down_y, down_x;        /* block of down_sample (1: that axis is kept); both 0: no down_sample at all */
    int down_method;           /* mi_pystripe_down */
    int use_flat;              /* divide by the flat field given to mi_pystripe_run (float32; the tile turns into a float tile) */
    float dark;                /* > 0: where(img > dark, img - dark, 0) in the tile's own kind (truncated for integer tiles) */
    int convert_to_16bit;      /* clip 0..65535, truncate */
    int convert_to_8bit;       /* convert_to_8bit_fun with bit_shift (0..8) */
    int bit_shift;
    int out_dtype;             /* mi_pystripe_dtype of the result (d_type; uint16 / uint8 when a conversion flag is set) */
    int flip_upside_down;
    int rotate;                /* 0, 90, 180, 270: numpy.rot90(img, rotate / 90) after the flip */
    int log_output;            /* 1: float32 output of the log-domain image BEFORE expm1 (cropped, nothing after it applied): the stripe
                                  filter's result, after the bleach correction when that is on; needs one of the two */
    int max_batch;             /* tiles that go through one launch (scratch is held for this many); <= 0: 16 */
    int keep_uniform;          /* 1: no uniform-tile rule (filter_streaks called on its own filters a uniform tile like any other) */
    double bleach_frequency;   /* 0: no bleach correction; else butter's Wn, in (0, 1) (1: the Nyquist frequency) */
    double bleach_clip_min, bleach_clip_med, bleach_clip_max;   /* log1p units: 0 <= min < med < max; min is raised to log1p(1); a clip
                                  that is NaN is estimated per tile ("Automatic clips" above).  MI_PS_CONSTANT pads with log1p(bleach_clip_min),
                                  with or without a frequency */
    int bleach_max_method;     /* 1: F is the outer product of the filtered row and column maxima of L */
} mi_pystripe_params;

typedef struct {
    int ny, nx;                /* tile after down_sample */
    int base_pad, pad_y, pad_x;/* calculate_pad_size and the extra rows / columns at the end (odd extent, 34-pixel rule) */
    int padded_ny, padded_nx;
    int levels;
    int coef_ny[MI_PS_MAX_LEVELS], coef_nx[MI_PS_MAX_LEVELS];   /* detail shapes, finest level first */
    int out_ny, out_nx, out_dtype;
    int integer_kind;          /* 1: the tile is an integer tile inside process_img (rint + clip after expm1, truncating dark) */
    int max_batch;
    size_t scratch_bytes_per_tile;
    int bleach_long_rows;      /* 1: a filtered line of the bleach correction is longer than MI_PS_BLEACH_LDS_ROW (segmented route) */
} mi_pystripe_info;

/* A plan for tiles of ny x nx samples of in_dtype on device dev.  Synchronises (uploads its tables).  A plan owns its scratch:
 * one thread and one stream use it at a time. */
int mi_pystripe_plan_create(int dev, int ny, int nx, int in_dtype, const mi_pystripe_params* params, void** plan);
/* as mi_pystripe_plan_create / _derive, for the orthogonal wavelet whose reconstruction low-pass is rec_lo[taps] (host memory,
 * float64; the kernels use it as float32): taps even, 2 .. MI_PS_MAX_TAPS, every value finite, and
 * max_k |sum_n rec_lo[n] rec_lo[n + 2 k] - delta_k| <= 1e-6, else MI_ERR_INVALID. */
int mi_pystripe_plan_create_wavelet(int dev, int ny, int nx, int in_dtype, const mi_pystripe_params* params, const double* rec_lo, int taps,
                                    void** plan);
int mi_pystripe_derive_wavelet(int ny, int nx, int in_dtype, const mi_pystripe_params* params, int taps, mi_pystripe_info* info);
int mi_pystripe_plan_destroy(void* plan);
int mi_pystripe_plan_info(void* plan, mi_pystripe_info* info);
/* The notch kernel's route per (pass, level, axis), for tests and profiles: MI_PS_NOTCH_ROUTE_INTS ints per record into out[cap]
 * (host memory) -- pass, level (1 = finest), axis (0: cH along axis -1, 1: cV along axis -2), line length n, packed positions with a
 * non-zero weight kp, bins kb, lines per work-group R, threads, dynamic LDS in bytes -- in the order the plan holds them: pass,
 * then level, then axis (axis 1 is listed whether or not the plan is bidirectional).  Returns the number of records (0 for a plan
 * without a stripe filter); MI_ERR_INVALID naming cap when cap ints do not hold them.  Reads the plan only. */
#define MI_PS_NOTCH_ROUTE_INTS 9
int mi_pystripe_plan_notch_routes(void* plan, int* out, int cap);
/* The bookkeeping alone, without a device: what a plan for this shape would derive (scratch_bytes_per_tile included). */
int mi_pystripe_derive(int ny, int nx, int in_dtype, const mi_pystripe_params* params, mi_pystripe_info* info);
/* count tiles, dense one after the other in `in` (ny x nx of in_dtype) -> `out` (out_ny x out_nx of out_dtype); flat: ny x nx
 * float32 on the device when params.use_flat, else NULL.  Tiles are independent: a tile's result does not depend on count or
 * on its place in the batch.  Enqueues on `stream`; the first call (and a call after a larger count) allocates the scratch. */
int mi_pystripe_run(void* plan, void* stream, const void* in, const void* flat, void* out, int64_t count);
/* Automatic clips of integer tiles: table[code] = log1p(code) as float32 for code < ncodes (256 for uint8 tiles, 65536 for uint16),
 * from host memory.  The table, never the device's log1pf, decides a sample's bin.  A plan starts with libm's log1pf; the Python
 * layer hands in numpy's.  Synchronises.  MI_ERR_INVALID for a plan without automatic clips on an integer tile. */
int mi_pystripe_plan_set_log_table(void* plan, const float* table, int ncodes);
/* The clips (clips_host[n][3]: min as used, i.e. raised to log1p(1), med, max) and the mi_pystripe_clip_status (status_host[n]) of
 * the n tiles of the plan's last run, whatever max_batch did to it; a plan without automatic clips reports its constants and 0.
 * The caller has synchronised the run's stream.  Either pointer may be NULL. */
int mi_pystripe_plan_clips(void* plan, float* clips_host, int* status_host, int n);
/* calculate_pad_size(shape=(ny, nx), sigma) (:681) */
int mi_pystripe_pad_size(int ny, int nx, double sigma);

#ifdef __cplusplus
}
#endif
#endif /* MI_PYSTRIPE_H */
