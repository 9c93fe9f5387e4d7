/* mi_tile_mask.h -- the foreground mask of pystripe's filter_streaks (enable_masking), on batches of equally shaped 2-D tiles in
 * device memory.
 *
 * Replaces get_img_mask (pystripe/core.py:475-489, called at :1079-1080).  One tile of ny x nx samples gives ny x nx bytes, 0 or 1:
 *   1. threshold  m = sample > threshold.  Integer tiles compare the code; float32 tiles compare v > (float)threshold (NaN gives 0),
 *                 or, with log_domain, log1pf(v) > (float)threshold.
 *   2. close      dilation, then erosion, with a close_steps x close_steps box of ones.
 *   3. open       erosion, then dilation, with an open_steps x open_steps box.
 *                 Both operators use ONE window: along each axis the positions [i - a, i - a + k - 1] with the anchor a = k / 2
 *                 (OpenCV's documented formula and default anchor).  Samples outside the tile are ignored: a dilation sees them as
 *                 0, an erosion as 1.  For an even k the window is not centred, so close and open each move content by one sample
 *                 towards higher indices; that shift is kept.  k = 1 is the identity; k above an extent covers the whole line.
 *   4. fill       inv = !m.  Every connected region of ones of inv (connectivity 4 or 8) that holds one of the four corner samples
 *                 is removed; a corner that is 0 in inv removes nothing; a region that touches the border but no corner stays.
 *                 mask = m | what is left of inv.
 * OpenCV is not among this project's tools: the window above is the restatement the tests check (tests/mask_util.py), agreement
 * with cv2 for even k is not verified.
 *
 * The cost of the morphology per sample does not grow with k (counts of ones from row prefix sums along x, a running count per
 * column along y).  The fill is exact for any shape: rounds of sweeps along the rows and the columns of a bit-packed map (and, for
 * connectivity 8, one step to the eight neighbours), each round its own launches, until a round changes nothing.
 */
#ifndef MI_TILE_MASK_H
#define MI_TILE_MASK_H

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    size_t scratch_bytes; /* device memory the plan owns */
    int max_batch;        /* tiles of one round of mi_tile_mask_run */
    int fill_rounds;      /* rounds of the fill in the last mi_tile_mask_run, the one that changed nothing included (the largest
                             over that run's groups of max_batch tiles); 0 before the first run */
} mi_tile_mask_info;

/* A plan for get_img_mask (core.py:475-489) on tiles of ny x nx samples of dtype (mi_pystripe_dtype, mi_pystripe.h) on device dev.
 * connectivity is 4 or 8 (cv2.floodFill's flags & 0xff).  The plan owns the scratch of max_batch tiles (<= 0: 16): one thread and
 * one stream use it at a time.  MI_ERR_INVALID naming the argument for an extent below 1 or above 2^30, an unknown dtype,
 * close_steps or open_steps below 1, a connectivity that is neither 4 nor 8. */
int mi_tile_mask_plan_create(int dev, int ny, int nx, int dtype, int close_steps, int open_steps, int connectivity, int max_batch,
                             void** plan);
/* get_img_mask (core.py:475-489) on count tiles, dense one after the other in `in` -> `mask` (count x ny x nx bytes, 0 or 1).
 * log_domain (float32 tiles only) compares log1pf of the sample.  masked_out is NULL, or tiles of the input type: `in` where the
 * mask is set, else 0; it may be `in` itself.  Tiles are independent: a tile's result does not depend on count or on its place in
 * the batch; more than max_batch tiles go through in several rounds.  Synchronises: the host reads one flag per batch of fill
 * rounds from `stream`.  MI_ERR_INTERNAL if the fill has not settled after ny * nx rounds (it settles in fewer for any input). */
int mi_tile_mask_run(void* plan, void* stream, const void* in, double threshold, int log_domain, void* mask, void* masked_out,
                     int64_t count);
/* The bookkeeping of a plan of mi_tile_mask_plan_create (core.py:475-489): scratch bytes, batch, fill rounds of the last run. */
int mi_tile_mask_plan_info(void* plan, mi_tile_mask_info* info);
/* Releases a plan of mi_tile_mask_plan_create (core.py:475-489); NULL is allowed. */
int mi_tile_mask_plan_destroy(void* plan);

#ifdef __cplusplus
}
#endif
#endif /* MI_TILE_MASK_H */
