/* mi_stitch.h -- stitching step 6 (tile merge) on the device: the stitched volume of a grid of placed stacks.
 *
 * Semantics of the reference's `terastitcher -6` at resolution 0 (UnstitchedVolume::internal_loadSubvolume_to_real32,
 * StackStitcher::getStripe2, StackStitcher::sinusoidal_blending / no_blending, VolumeConverter's real32 -> integer step):
 * samples are scaled to [0,1] float (/ 255 or / 65535); each row of stacks is a stripe whose adjacent stacks are blended
 * across their H overlap; the stripes are blended across their V overlap column by column between the corners of the two
 * stripes; the blend angle runs 0..PI over an overlap in steps of PI/(overlap-1) accumulated in double; the sinusoidal blend
 * is ((cos+1)*0.5)*p1 + (1-(cos+1)*0.5)*p2 in double, stored as float, and a zero sample on either side gives the larger of
 * the two; the float result becomes uint16(v * 65535.0F) (uint8(v * 255.0f)).  The volume is the union of the stacks in V
 * and H (first row / first column to last row / last column, as computeVolumeDims) and the range all stacks share in D.
 */
#ifndef MI_STITCH_H
#define MI_STITCH_H

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MI_SINBLEND = 0, MI_NOBLEND = 1 } mi_blending;

/* Stitched volume extent [v0,v1) x [h0,h1) x [d0,d1) of the grid in the stacks' absolute frame ([host] arrays of
 * n_rows * n_cols ABS_V / ABS_H / ABS_D, row-major; dims[6] receives v0, v1, h0, h1, d0, d1).  Host only. */
int mi_merge_volume_dims(int n_rows, int n_cols, const int* abs_v, const int* abs_h, const int* abs_d, int height, int width,
                         int n_slices, int* dims);

/* One output box of the stitched volume.  Box coordinates are 0-based in the stitched volume (what the output tree names):
 * slices [D0,D1), rows [V0,V1), columns [H0,H1).  stacks[r * n_cols + c] [host array of device pointers] holds stack (r, c)'s
 * samples for output slices D0..D1-1, i.e. its own slices z + dims.d0 - ABS_D for z in [D0,D1), each height x width,
 * C-order, uint8 (bytes = 1) or uint16 (bytes = 2).  out (device, same sample type) receives (D1-D0) x (V1-V0) x (H1-H0)
 * C-order.  The small blend tables are built on the host in double and travel with the call on `stream`; only enqueues
 * (stream-ordered allocation of the tables, no device-wide synchronisation). */
int mi_merge_slab(int dev, void* stream, int n_rows, int n_cols, const int* abs_v, const int* abs_h, const int* abs_d, int height,
                  int width, int n_slices, const void* const* stacks, int bytes, int blending, int D0, int D1, int V0, int V1,
                  int H0, int H1, void* out);

#ifdef __cplusplus
}
#endif
#endif
