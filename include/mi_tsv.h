/* mi_tsv.h -- the live tile merge of the pipeline on the device: a box of a TSVVolume (tsv/volume.py).
 *
 * The reference places every stack by chaining the FIRST displacement of its NORTH (rows > 0) or WEST (row 0) list
 * (make_stacks, tsv/volume.py:730-797), takes the union of the stacks in x, y and z with zero fill (:671-682) and blends
 * the stacks that cover a voxel either by `maximum` (:633-645) or by the cosine blend carried in float16 (:592-631,
 * compute_cosine :430-465, get_distance_from_edge :490-555).  Both are restated here; tsv.py holds the XML and the files.
 */
#ifndef MI_TSV_H
#define MI_TSV_H

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Placement (make_stacks) and volume extent.  Host only.  north / west [host, n_rows * n_cols * 3, row-major]: the H, V, D
 * `displ` of the first NORTH_displacements / WEST_displacements entry of every stack (north is read for rows > 0, west for
 * row 0 and columns > 0; the others are ignored and may be 0).  nz [host, n_rows * n_cols]: slices per stack.  Stack (0,0)
 * is at the origin, every other stack at its north (rows > 0) or west neighbour's offset minus the displacement; the D part
 * is dropped with ignore_z; all offsets are rebased so that their minima are 0.  x0 / y0 / z0 [host, n_rows * n_cols]
 * receive the offsets, extent[6] the union x0, x1, y0, y1, z0, z1 of the stacks. */
int mi_tsv_place(int n_rows, int n_cols, const int* north, const int* west, int ignore_z, const int* nz, int height, int width,
                 int* x0, int* y0, int* z0, int* extent);

/* One box [bx0,bx1) x [by0,by1) x [bz0,bz1) of the volume (any box: voxels no stack covers are 0).  Stack s occupies
 * [x0[s], x0[s] + width) x [y0[s], y0[s] + height) x [z0[s], z0[s] + nz[s]); the order of the stacks is the order of the
 * blend (row-major in the reference).  slices[s] [host array of device pointers]: the slices of stack s that fall into the
 * box's z range, i.e. its own slices max(z0[s], bz0) - z0[s] .. min(z0[s] + nz[s], bz1) - z0[s] - 1, each height x width,
 * C-order, uint8 (bytes = 1) or uint16 (bytes = 2), at any address; it is not read (and may be null) for a stack that does
 * not meet the box.  out (device, same sample type) receives (bz1-bz0) x (by1-by0) x (bx1-bx0), C-order.
 *
 * cosine = 0: the maximum over the covering stacks, exact.  cosine = 1: the reference's float16 blend -- per stack in order
 * part = f16(sample), mpart = 1, both times f16(w) for every OTHER covering stack in order, w = d^2 / (d^2 + od^2) in double
 * (= sin(arctan2(d, od))^2, which the reference takes in float64) of the two edge distances, rounded once; result += part,
 * multiplier += mpart; result / multiplier (or / eps16 where the multiplier is not above it); every float16 operation is the float operation rounded to nearest-even float16.
 * A result that is inf or nan in float16 saturates (65535 / 255).  Two stacks with the same x0 and y0 are refused under
 * cosine (the reference's weights then depend on the requested box).
 *
 * Stream-ordered: the small tables travel with the call on `stream` (stream-ordered allocation), only enqueues, no
 * device-wide synchronisation. */
int mi_tsv_merge(int dev, void* stream, int n_stacks, const int* x0, const int* y0, const int* z0, const int* nz, int height,
                 int width, const void* const* slices, int bytes, int cosine, int bx0, int bx1, int by0, int by1, int bz0, int bz1,
                 void* out);

#ifdef __cplusplus
}
#endif
#endif
