/* mi_tile_resize.h -- process_img's resize of a tile to new_size, on batches of equally shaped 2-D tiles in device memory.
 *
 * Replaces pystripe/core.py:1356-1359 (`resize(img, new_size, preserve_range=True, anti_aliasing=...)`) for the case without a Gaussian
 * pre-filter, as DESIGN.md section 14 restates skimage.transform.resize and section 12c states the arithmetic:
 *   scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True), then a clip to the [min, max] of the tile that was handed in.
 * Both shapes process_images.py asks for (:1163-1183) are this case: growing both axes (sigma 0) and anti_aliasing=False.  A mixed
 * new_size (the tile shape lexicographically below new_size with a shrinking axis) needs the pre-filter; the Python layer refuses it.
 *
 * Per axis n -> m, in float64 (mi_tile_resize_tables): z = n / m; c = (k + 0.5) z - 0.5, mirrored into [0, n - 1] (c < 0: -c;
 * c > n - 1: 2 (n - 1) - c; n == 1: 0); i0 = floor(c), t = c - i0, i1 = i0 + 1 mirrored the same way.  A sample is
 *   (a[y0][x0] (1 - ty)) (1 - tx) + (a[y0][x1] (1 - ty)) tx + (a[y1][x0] ty) (1 - tx) + (a[y1][x1] ty) tx
 * summed left to right in float64 without fused operations.  A float32 tile stores that sum rounded to float32 and clipped; a uint8 /
 * uint16 tile stores the float64 clipped and truncated -- what the reference's clip and astype (:1361-1369) make of the float64 image
 * `preserve_range=True` yields for an integer tile.
 */
#ifndef MI_TILE_RESIZE_H
#define MI_TILE_RESIZE_H

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tables of one axis of core.py:1356-1359 (DESIGN.md sections 14 and 12c): n input samples -> m output samples, i0[m], i1[m], t[m]
 * in host memory.  Host only, no device is needed.  MI_ERR_INVALID for an extent below 1. */
int mi_tile_resize_tables(int n, int m, int* i0, int* i1, double* t);
/* A plan for core.py:1356-1359 (DESIGN.md sections 14 and 12c) on tiles of ny x nx samples of dtype (mi_pystripe_dtype,
 * mi_pystripe.h) -> my x mx samples of the same type, on device dev.  The plan owns the tables and the (min, max) slots of
 * max_batch tiles (<= 0: 16): one thread and one stream use it at a time.  Synchronises (uploads the tables).  MI_ERR_INVALID naming
 * the argument for an extent below 1 or an unknown dtype.  Equal shapes are allowed: mi_tile_resize_run is then a copy. */
int mi_tile_resize_plan_create(int dev, int ny, int nx, int my, int mx, int dtype, int max_batch, void** plan);
/* core.py:1356-1359 (DESIGN.md sections 14 and 12c) on count tiles, dense one after the other in `in` -> `out` (device memory, not
 * overlapping).  Only enqueues on `stream`; more than max_batch tiles go through in several rounds.  Tiles are independent: a tile's
 * result does not depend on count or on its place in the batch. */
int mi_tile_resize_run(void* plan, void* stream, const void* in, void* out, int64_t count);
/* Releases a plan of mi_tile_resize_plan_create (core.py:1356-1359, DESIGN.md sections 14 and 12c); NULL is allowed. */
int mi_tile_resize_plan_destroy(void* plan);

#ifdef __cplusplus
}
#endif
#endif /* MI_TILE_RESIZE_H */
