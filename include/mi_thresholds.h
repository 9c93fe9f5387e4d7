/* mi_thresholds.h -- the slice estimates of process_images.py on the device: the 256-bin histogram of a float32 image as
 * numpy.histogram takes it, the exact counts per code of a u8 / u16 image, and the multi-Otsu search over a 256-bin histogram.
 *
 * Serves, of process_images.py:
 *   estimate_img_related_params :594-655   (log1p, threshold_multiotsu(img, classes=4), estimate_bit_shift, dark)
 *   estimate_bit_shift          :320-331   (percentile of the samples above a threshold)
 * scikit-image's threshold_multiotsu is built to the restatement of DESIGN section 17 (float32 arithmetic in a fixed order), so the
 * threshold INDICES are equal to the restatement's, not close.
 *
 * Every entry takes `count` images of `n` samples each, one behind the other in device memory, enqueues on `stream` and writes to
 * device buffers of the caller; nothing is read back and nothing waits.  Bases need only the alignment of their sample type: a
 * base that is not 16-byte aligned is read by elements up to the first 16-byte boundary and behind the last one.
 */
#ifndef MI_THRESHOLDS_H
#define MI_THRESHOLDS_H

#include <stdint.h>

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_HIST_BINS 256
#define MI_OTSU_MAX_CLASSES 4

typedef enum { MI_CODES_U8 = 0, MI_CODES_U16 = 1 } mi_code_dtype; /* the values of mi_pystripe_dtype */

typedef enum {
    MI_OTSU_OK = 0,
    MI_OTSU_TOO_FEW_VALUES = 1, /* fewer occupied bins than classes: threshold_multiotsu raises ValueError */
    MI_OTSU_VALUES_ARE_CLASSES = 2 /* exactly `classes` occupied bins: the indices are the occupied bins but the last */
} mi_otsu_status;

/* numpy.histogram(image, 256) of every float32 image.
 *   range     [count][2]    smallest and largest finite sample (it holds order-preserving keys while the call runs)
 *   nonfinite [count]       1 when the image holds a NaN or an infinity (numpy raises ValueError); its edges and counts mean nothing
 *   edges     [count][257]  fl32(fl32(i) * step + first), step = fl32((last - first) / 256), edges[256] = last; a constant image
 *                           gets first - 0.5 and last + 0.5
 *   counts    [count][256]  samples with edges[b] <= v < edges[b + 1]; v == last counts in bin 255
 */
int mi_hist256_f32(int device, void* stream, const float* images, int count, int64_t n, float* range, int* nonfinite, float* edges,
                   unsigned long long* counts);

/* Occurrences of every code: counts[count][256] for MI_CODES_U8, counts[count][65536] for MI_CODES_U16. */
int mi_code_hist(int device, void* stream, const void* images, int dtype, int count, int64_t n, unsigned long long* counts);

/* Multi-Otsu over counts[count][256] for `classes` in 2 .. 4.
 *   indices [count][3]   the classes - 1 threshold bins in rising order, -1 behind them
 *   nvalues [count]      occupied bins
 *   status  [count]      mi_otsu_status
 *   work    [count]      8 bytes per image for the reduction
 */
int mi_multiotsu_search(int device, void* stream, const unsigned long long* counts, int count, int classes, int* indices, int* nvalues,
                        int* status, unsigned long long* work);

#ifdef __cplusplus
}
#endif
#endif
