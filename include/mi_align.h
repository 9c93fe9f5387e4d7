/* mi_align.h -- channel alignment and the RGB composite of align_images.py on the device: scikit-image's 2-D sobel, the
 * translation-only ECC registration of OpenCV's findTransformECC, and the per-slice arithmetic of the RGB series.
 *
 * Serves, of the reference:
 *   process_images.py:310-317   get_gradient (float32, skimage.filters.sobel)
 *   process_images.py:788-818   get_transformation_matrix (findTransformECC, MOTION_TRANSLATION, gaussFiltSize=5, no mask)
 *   align_images.py:271-338     process_single_big_image (pad_to_shape, roll_pad twice, trim_to_shape, stack, astype)
 * OpenCV and scikit-image are built to the restatement of DESIGN section 18: every per-pixel value is float32 arithmetic in a fixed
 * order (bit-equal to the restatement), every sum is a float64 sum of exact products in a fixed order (two runs are bit-equal).
 *
 * Every entry enqueues on `stream` and writes to device buffers of the caller.  Only mi_ecc_translation_run waits: it reads the
 * 48-byte state back once per batch of iterations.  Planes are [ny][nx] float32, rows one behind the other.
 */
#ifndef MI_ALIGN_H
#define MI_ALIGN_H

#include <stdint.h>

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ECC_NSUMS 16        /* doubles per row of sums (15 used, see mi_ecc_sum) */
#define MI_ECC_MAX_GROUPS 1024 /* work-groups of the sum kernel at most: the scratch holds one row of sums for each */
#define MI_ECC_SCRATCH_BYTES (MI_ECC_MAX_GROUPS * MI_ECC_NSUMS * 8)
#define MI_ECC_DEFAULT_BATCH 32 /* iterations enqueued between two reads of the state */

/* Index of every sum in a row.  m is the mask, w / gxw / gyw the warped subject and its gradients, t the blurred template. */
typedef enum {
    MI_ECC_N = 0,    /* sum m */
    MI_ECC_SW = 1,   /* sum m w */
    MI_ECC_SWW = 2,  /* sum m w w */
    MI_ECC_ST = 3,   /* sum m t */
    MI_ECC_STT = 4,  /* sum m t t */
    MI_ECC_SWT = 5,  /* sum m w t */
    MI_ECC_HXX = 6,  /* sum gxw gxw   (all pixels) */
    MI_ECC_HXY = 7,  /* sum gxw gyw */
    MI_ECC_HYY = 8,  /* sum gyw gyw */
    MI_ECC_GXW = 9,  /* sum gxw w     (all pixels: w keeps its value outside the mask) */
    MI_ECC_GYW = 10, /* sum gyw w */
    MI_ECC_MGX = 11, /* sum m gxw */
    MI_ECC_MGY = 12, /* sum m gyw */
    MI_ECC_GXT = 13, /* sum m gxw t */
    MI_ECC_GYT = 14  /* sum m gyw t */
} mi_ecc_sum;

typedef enum {
    MI_ECC_OK = 0,
    MI_ECC_NAN = 1,       /* rho is NaN: findTransformECC raises "NaN encountered." */
    MI_ECC_MINIMIZED = 2  /* lambda's denominator <= 0: "The algorithm stopped before its convergence. ..." */
} mi_ecc_status;

/* The iterate.  It lives in device memory while mi_ecc_translation_run works and is copied to the caller at the end. */
typedef struct {
    double tx, ty;        /* translation of the map: the subject is sampled at (x + tx, y + ty) */
    double rho, rho_last; /* correlation coefficient of the last and the last but one iteration */
    int iteration;        /* iterations done */
    int status;           /* mi_ecc_status */
    int done;             /* 1 once the loop has ended: count reached, |rho - rho_last| < eps, or a status */
    int reserved;
} mi_ecc_state;

/* out = skimage.filters.sobel(in) of a float32 plane: the two 3 x 3 kernels ([1, 0, -1] across, [1, 2, 1] along, over 8) as
 * convolutions with scipy's `reflect` border, accumulated in float64 and rounded to float32 as scipy.ndimage does, then
 * sqrt((h * h + v * v) / 2) in float32.  `in` and `out` must not overlap.   [process_images.py:310-317] */
int mi_sobel2d_f32(int device, void* stream, const float* in, int ny, int nx, float* out);

/* What findTransformECC computes before its loop: t = blur(tmpl), s = blur(subj) with the separable taps [1, 4, 6, 4, 1] / 16
 * (rows first, then columns) and BORDER_REFLECT_101, gx[y][x] = 0.5 * s[y][x + 1] - 0.5 * s[y][x - 1] and gy likewise along y with the
 * same border.  ny, nx >= 3.  No plane may overlap another.   [process_images.py:804-812] */
int mi_ecc_prepare(int device, void* stream, const float* tmpl, const float* subj, int ny, int nx, float* t, float* s, float* gx,
                   float* gy);

/* The sums of one ECC iteration at the translation (tx, ty): sums[MI_ECC_NSUMS] doubles in device memory, indexed by mi_ecc_sum
 * (the last is 0).  scratch: MI_ECC_SCRATCH_BYTES of device memory, 8-byte aligned.  Two calls give equal bits. */
int mi_ecc_sums(int device, void* stream, const float* t, const float* s, const float* gx, const float* gy, int ny, int nx, double tx,
                double ty, double* scratch, double* sums);

/* findTransformECC's loop for MOTION_TRANSLATION from the translation (tx0, ty0): at most `iterations` iterations, until
 * |rho - rho_last| < eps.  state and scratch are device memory (sizeof(mi_ecc_state), MI_ECC_SCRATCH_BYTES); *result receives the
 * final state on the host.  batch: iterations enqueued between two reads of the state, <= 0 for MI_ECC_DEFAULT_BATCH.  A failure
 * of the algorithm is result->status, not an error of the call.   [process_images.py:804-812] */
int mi_ecc_translation_run(int device, void* stream, const float* t, const float* s, const float* gx, const float* gy, int ny, int nx,
                           double tx0, double ty0, int iterations, double eps, int batch, mi_ecc_state* state, double* scratch,
                           mi_ecc_state* result);

/* One channel of the composite.  src holds `count` source slices [count][ny][nx] of the channel, the first of them slice `first` of
 * its series; src == NULL is an absent channel (zeros).  Output slice k of the group takes source slice k + dz (zeros outside
 * first .. first + count - 1), output pixel (y, x) takes source pixel (y + dy, x + dx) (zeros outside the slice). */
typedef struct {
    const void* src;
    int count, first, ny, nx;
    int dz, dy, dx, reserved;
} mi_composite_channel;

typedef enum { MI_RGB_U8 = 1, MI_RGB_U16 = 2, MI_RGB_U32 = 3, MI_RGB_F32 = 4 } mi_rgb_dtype;

/* out[k][y][x][c] for output slices z0 .. z0 + n - 1 of extents ny x nx: pad_to_shape, roll_pad by the y and the x offset,
 * trim_to_shape, stack and astype of process_single_big_image as one index map (the caller folds the pads, the rolls and the trim
 * into dz, dy, dx; k + dz above is (z0 + k) + dz).  src_dtype: MI_RGB_U8 or MI_RGB_U16; out_dtype: any mi_rgb_dtype, converted as
 * numpy's astype does (u16 -> u8 keeps the low byte).   [align_images.py:271-338] */
int mi_channel_composite(int device, void* stream, const mi_composite_channel* channels, int src_dtype, int z0, int n, int ny, int nx,
                         void* out, int out_dtype);

#ifdef __cplusplus
}
#endif
#endif
