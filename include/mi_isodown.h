/* mi_isodown.h -- the isotropic down-sampled volume of the per-slice pass (parallel_image_processor.py): alternating max / mean
 * halvings of every processed slice in y and x, an anti-aliased resize to the target pixel grid, an alternating max / mean
 * reduction of every group of slices along z, and the anti-aliased 3-D resize of the stacked planes.
 *
 * Replaces, of parallel_image_processor.py:
 *   calculate_down_sampling_target :156-187   (target shape, halving rounds; mi_isodown_derive)
 *   MultiProcess.run               :371-384   (uniform slice -> zeros, block_reduce rounds, resize)
 *                                  :411-435   (uniform stack -> zeros, block_reduce along z, dtype of the plane)
 *   parallel_image_processor       :722       (resize of the stacked planes; mi_resize_antialias)
 * scikit-image's functions are built to the restatement of DESIGN section 14:
 *   block_reduce   zeros behind an odd extent, then max(a, b) or (a + b) / 2 in float32 of every pair
 *   resize         sigma = max(0, (in / out - 1) / 2) per axis; scipy.ndimage.gaussian_filter(mode='mirror', truncate 4, float32
 *                  between the axes) when any axis shrinks; scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True); clip to
 *                  the input's [min, max]
 */
#ifndef MI_ISODOWN_H
#define MI_ISODOWN_H

#include "mi_common.h"
#include "mi_pyramid.h"  /* mi_halve_method */
#include "mi_pystripe.h" /* mi_pystripe_dtype */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ISO_MAX_STEPS 32   /* halvings of one slice, y and x together */
#define MI_ISO_MAX_RADIUS 512 /* Gaussian radius of the resize (int(4 sigma + 0.5)); a larger one is MI_ERR_UNSUPPORTED */

typedef struct {
    double voxel_y, voxel_x; /* of the processed slice (after `fun` and rotation), in the unit of target_voxel */
    double target_voxel;
    int alternating;         /* 0: every round is mean / mean */
    int z_rounds;            /* rounds of the z reduction: ceil(sqrt(target_voxel / voxel_z)) */
    int out_dtype;           /* mi_pystripe_dtype of the group's plane: F32, or U16 (values limited to 0 .. 65535 and truncated),
                                or U8 (a plain cast when the slices are U8, else 16-bit, shifted right by 8, limited to 255, a
                                value that is not zero never below 1) */
    int max_group;           /* slices of one run (scratch is held for this many); <= 0: 16 */
} mi_isodown_params;

typedef struct {
    int ny, nx;                         /* the processed slice */
    int target_ny, target_nx;           /* numpy.round(shape / (target / voxel)), half to even */
    int rounds_y, rounds_x;             /* floor(sqrt(target / voxel)) */
    int nsteps;                         /* halvings that run (a round's halving is dropped when ceil(extent / 2) < target) */
    int step_axis[MI_ISO_MAX_STEPS];    /* 0: y, 1: x, in the order they are applied */
    int step_method[MI_ISO_MAX_STEPS];  /* mi_halve_method */
    int step_extent[MI_ISO_MAX_STEPS];  /* extent of that axis before the step */
    int ky, kx;                         /* halvings per axis */
    int halved_ny, halved_nx;
    double sigma_y, sigma_x;            /* of the resize halved -> target; 0: the axis is not filtered */
    int radius_y, radius_x, taps_y, taps_x;   /* taps = 2 radius + 1, 0 when the axis is not filtered */
    int tile_ny, tile_nx;               /* samples of the halved plane one work-group owns (source block: tile << k), for 16-bit
                                           samples; (0, 0) when the block behind one halved sample does not fit the kernel
                                           (2^(ky + kx) samples, past 8192 floats on chip): plan_create is MI_ERR_UNSUPPORTED */
    int lds_steps;                      /* steps applied in LDS (the first ones run on the registers of the load) */
    size_t scratch_bytes_per_slice;
} mi_isodown_info;

/* The plan of one slice shape without a device.  MI_ERR_INVALID when a target extent rounds to 0. */
int mi_isodown_derive(int ny, int nx, double voxel_y, double voxel_x, double target_voxel, int alternating, mi_isodown_info* info);

/* A plan for slices of ny x nx samples of src_dtype (mi_pystripe_dtype) on device dev.  A plan owns its scratch: one thread and one
 * stream at a time. */
int mi_isodown_plan_create(int dev, int ny, int nx, int src_dtype, const mi_isodown_params* params, void** plan);
int mi_isodown_plan_destroy(void* plan);
int mi_isodown_plan_info(void* plan, mi_isodown_info* info);

/* The halving chain alone: count dense slices `in` [count][ny][nx] -> halved [count][halved_ny][halved_nx] float32 and
 * differs [count] int32 (1 when a sample of the slice differs from its sample (0, 0), else 0).  One kernel; every source sample is
 * read once.  Stream-ordered. */
int mi_isodown_halve(void* plan, void* stream, const void* in, int64_t count, float* halved, int* differs);
/* Halving and resize: the float32 planes [count][target_ny][target_nx] of count slices (the reference's z_stack); a uniform slice
 * gives zeros.  Stream-ordered; the first call (and a call with a larger count) allocates the scratch. */
int mi_isodown_planes(void* plan, void* stream, const void* in, int64_t count, float* planes);
/* The whole group: mi_isodown_planes of the count slices, then mi_isodown_reduce_z -> one plane of out_dtype.  uniform (may be NULL)
 * receives 1 when the stack of planes was uniform (the reference then writes float32 zeros whatever the dtype), else 0. */
int mi_isodown_run(void* plan, void* stream, const void* in, int64_t count, void* plane, int* uniform);

/* The z reduction of a stack [n][ny][nx] float32 (device memory, overwritten): zeros when every sample of the stack is equal, else
 * `rounds` rounds (even: max, odd: mean) of block_reduce (2, 1, 1) while more than one plane is left.  MI_ERR_INVALID when more than
 * one plane would be left.  src_is_u8 selects the U8 conversion (see mi_isodown_params).  Synchronises before it returns. */
int mi_isodown_reduce_z(int dev, void* stream, float* stack, int n, int ny, int nx, int rounds, int src_is_u8, int out_dtype, void* plane,
                        int* uniform);

/* resize(in, out_shape, preserve_range=True, anti_aliasing=True) of a float32 array of ndim 2 or 3 in device memory (shapes in C
 * order, host arrays).  Synchronises before it returns (it owns its scratch). */
int mi_resize_antialias(int dev, void* stream, const float* in, int ndim, const int* in_shape, const int* out_shape, float* out);

#ifdef __cplusplus
}
#endif
#endif /* MI_ISODOWN_H */
