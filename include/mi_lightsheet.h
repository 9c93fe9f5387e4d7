/* mi_lightsheet.h -- pystripe's lightsheet correction (ClearMap's algorithm): local percentiles on two sub-grids, their order-1
 * resampling to the image and the subtraction, on batches of equally shaped 2-D tiles in device memory.
 *
 * Replaces pystripe/lightsheet_correct.py as pystripe/core.py:1333-1348 calls it:
 *   correct_lightsheet    :31-106    (lightsheet estimate, background estimate, img -= min(img, min(ls, bg * factor)))
 *   local_percentile      :245-312   (one percentile, numpy.percentile's 'linear' method)
 *   apply_local_function  :113-237   (centres :168-175, clipped and stepped windows :193-198, scipy.ndimage.zoom(order=1) :218-229)
 * Not built (refused by the Python layer by name): masks, array-shaped windows, lists of percentiles, interpolation orders other
 * than 1 / None.
 *
 * float32 samples must be FINITE.  Samples are ranked by their bit patterns (sign bit flipped, negative values wholly inverted):
 * -0.0 sorts just below +0.0 (one value to numpy, so the percentile is the same) and denormals keep their place, but a NaN is
 * ranked like a number -- above +inf, or below -inf when its sign bit is set -- and does not poison its window as it does in numpy
 * (windows that do not hold it are the same in both).  At percentile 1 numpy forms inf - inf in its lerp and returns NaN for a
 * window whose maximum is infinite; this library returns the maximum.
 *
 * Semantics kept: per axis `n = extent / spacing` centres at `left + i * spacing`, `left = (extent - (n - 1) *
 * spacing) / 2`; window [max(0, c - selem / 2), min(c + selem - selem / 2, extent)) walked with `step` from its clipped start; the
 * percentile in float64 (integer images) or float32 (float32 images), truncated into an integer grid; scipy's order-1 zoom in
 * float64 with its fixed order of operations, half-up rounding into an integer map and its zero line when the last coordinate
 * rounds past the last node; `bg * int(factor)` wrapping in the grid's integer type when image and grids are all integers.
 */
#ifndef MI_LIGHTSHEET_H
#define MI_LIGHTSHEET_H

#include "mi_common.h"
#include "mi_pystripe.h" /* mi_pystripe_dtype */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_LS_MAX_WINDOW 16384  /* samples of one window after stepping */
#define MI_LS_MAX_LENGTH 4096   /* artifact_length */

typedef struct {
    int artifact_length;             /* L: the lightsheet estimate uses windows and spacing (1, L) (core.py:1338) */
    int artifact_along_y;            /* 1: windows and spacing (L, 1) instead, correct_lightsheet's own default (:35) */
    int background_window_size;      /* W: the background estimate uses windows (W, W) (core.py:1342) */
    int background_spacing;          /* 25 in process_img (core.py:1343); <= 0: 25 */
    int background_step;             /* 2 in process_img (core.py:1346); <= 0: 2 */
    double percentile;               /* in [0, 1] */
    double lightsheet_vs_background; /* the factor on the background (lightsheet_correct.py:89-95) */
    int factor_is_integer;           /* the caller's factor was an integer object: never the float expression, no truncation needed */
    int map_dtype;                   /* mi_pystripe_dtype of both grids and maps (process_img's d_type) */
    int max_batch;                   /* tiles that go through one launch (scratch is held for this many); <= 0: 16 */
} mi_lightsheet_params;

typedef struct {
    int ny, nx;
    int ls_ny, ls_nx, ls_left_y, ls_left_x;      /* centres of the lightsheet estimate: every row, every L-th column from ls_left_x */
    int bg_ny, bg_nx, bg_left_y, bg_left_x;      /* centres of the background estimate */
    int bg_first_y0, bg_first_y1, bg_last_y0, bg_last_y1;   /* clipped window [y0, y1) of the first and the last centre row */
    int bg_first_x0, bg_first_x1, bg_last_x0, bg_last_x1;   /* the same for the centre columns */
    int max_window_samples;                      /* samples of the largest window after stepping (at least L) */
    int ls_zero_last_row, ls_zero_last_col;      /* scipy's zoom writes 0 into the last row / column of the lightsheet map */
    int bg_zero_last_row, bg_zero_last_col;      /* ... into the last row / column of the background map */
    int integer_mode;                            /* image and grids are integers: truncated factor, wrapping product */
    int max_batch;
    size_t scratch_bytes_per_tile;               /* the two grids */
} mi_lightsheet_info;

/* The bookkeeping alone, without a device (apply_local_function :168-198, the zoom of :218-229). */
int mi_lightsheet_derive(int ny, int nx, int img_dtype, const mi_lightsheet_params* params, mi_lightsheet_info* info);
/* A plan for tiles of ny x nx samples of img_dtype on device dev.  A plan owns its scratch: one thread and one stream at a time. */
int mi_lightsheet_plan_create(int dev, int ny, int nx, int img_dtype, const mi_lightsheet_params* params, void** plan);
int mi_lightsheet_plan_destroy(void* plan);
int mi_lightsheet_plan_info(void* plan, mi_lightsheet_info* info);
/* correct_lightsheet (:31-106) on count tiles, dense one after the other in `in` -> `out` (same shape and type; out == in is
 * allowed).  ls_map / bg_map: NULL, or count full-size maps of map_dtype (return_lightsheet / return_background).  Tiles are
 * independent.  Enqueues on `stream`; the first call (and a call after a larger count) allocates the scratch. */
int mi_lightsheet_run(void* plan, void* stream, const void* in, void* out, void* ls_map, void* bg_map, int64_t count);
/* local_percentile (:245-312) of count tiles for one rectangular window: selem, spacing, step per axis (y, x), percentile in
 * [0, 1].  interpolate 0: `out` receives the sub-grids [count][ny / spacing_y][nx / spacing_x] of out_dtype (interpolate=None);
 * 1: the grids resampled to [count][ny][nx] (order 1).  Synchronises before it returns (it owns its scratch). */
int mi_lightsheet_local_percentile(int dev, void* stream, const void* in, int img_dtype, int ny, int nx, int64_t count, int selem_y,
                                   int selem_x, int spacing_y, int spacing_x, int step_y, int step_x, double percentile, int interpolate,
                                   void* out, int out_dtype);

#ifdef __cplusplus
}
#endif
#endif /* MI_LIGHTSHEET_H */
