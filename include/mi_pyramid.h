/* mi_pyramid.h -- the TeraFly conversion (teraconverter --dfmt="TIFF (tiled, 3D)"): the halving pyramid of a slab of integer
 * slices on the device, and the multi-page TIFF block files of the tree on the host.
 *
 * Halving is the reference's integer path (VirtualVolume::halveSample_UINT8 / halveSample2D_UINT8, VirtualVolume.cpp:829-1130):
 * a level halves V and H of the previous one and, when it is a 3-D level, D as well.  Mean: the 8 (3-D) or 4 (2-D) samples summed
 * in float in the order (z,i,j), (z,i,j+1), (z,i+1,j), (z,i+1,j+1) [then z+1], divided by 8 (4) and rounded half away from zero
 * (iim::round) -- exact for 8- and 16-bit samples, so the result is ((sum + 4) >> 3) ((sum + 2) >> 2).  Max: the largest sample.
 * An odd extent loses its last row, column or slice.  The slab is one z-group of VolumeConverter::generateTilesVaa3DRaw
 * (z_max_res slices, or the leftover group): groups are halved independently.
 */
#ifndef MI_PYRAMID_H
#define MI_PYRAMID_H

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MI_HALVE_MEAN = 0, MI_HALVE_MAX = 1 } mi_halve_method;

/* Levels 1..n_levels of the slab `in` (device, nz x ny x nx C-order samples of `bytes` = 1 (uint8) or 2 (uint16)).
 * halve_d[k] [host] says whether level k+1 also halves D (1: 3-D halving) or only V and H (0: 2-D halving).  Level L has
 * nx >> L columns, ny >> L rows and nz_L slices with nz_L = nz_{L-1} / 2 (3-D) or nz_{L-1} (2-D), nz_0 = nz.
 * out[k] [host array of device pointers] receives level k+1 as dense C-order planes.  Level 0 is read once; the kernel keeps the
 * first level's values on chip and writes the next level from them, so one launch makes two levels (levels 3-4, 5-6, ... chain from
 * the level two above).  out[k] may be NULL when level k+1 is not wanted, unless it feeds the next launch (k = 1, 3, 5, ... with a
 * deeper level).  Stream-ordered: only enqueues on `stream`.  64-bit indices throughout. */
int mi_pyramid_slab(int dev, void* stream, const void* in, int bytes, int nx, int ny, int nz, int method, int n_levels,
                    const int* halve_d, void* const* out);

/* Writes / extends n multi-page TIFF files (host code, no GPU), files in parallel and, with LZW, strips in parallel.
 * Block b: pages dims[3b+2] of dims[3b] columns x dims[3b+1] rows, sample (p, y, x) at
 *   ((const char*)first[b])[(p * strides[2b] + y * strides[2b+1] + x) * bytes]     [host memory, strides in samples].
 * page0[b] = 0 creates paths[b] (replacing any file); page0[b] > 0 appends to a file this writer made, whose pages so far must
 * number page0[b].  Every page carries PageNumber (page index, page_total[b]) -- the reference's block depth, which TeraFly
 * reads from the first page.  compression: 0 none, 1 LZW (TIFF's, with the early change); rows_per_strip >= 1.  bigtiff != 0
 * makes BigTIFF files; so does a block of more than 4 GiB (width * height * page_total * bytes), as initTiff3DFile
 * (Tiff3DMngr.cpp) does.  A classic file that would pass 4 GiB fails with MI_ERR_INVALID.  n_threads <= 0: OMP_NUM_THREADS,
 * else 16.  Decoded pages equal the input; bytes need not equal libtiff's. */
int mi_tiff3d_write_blocks(int n, const char* const* paths, const void* const* first, const int64_t* strides, const int* dims,
                           const int* page0, const int* page_total, int bytes, int compression, int rows_per_strip, int bigtiff,
                           int n_threads);

/* LZW (TIFF) encoding of n bytes of src into dst (capacity cap bytes): *written receives the stream's length, a Clear code
 * first and EOI last.  MI_ERR_NOMEM when cap is too small (n * 3 / 2 + 16 always suffices).  Host only. */
int mi_tiff_lzw_encode(const void* src, int64_t n, void* dst, int64_t cap, int64_t* written);

/* ---- the device route of the tree writer: the LZW strips encoded on the GPU (csrc/tiff3d_lzw_enc.hip), one strip per wave.  The
 * stream of a strip is the one mi_tiff_lzw_encode writes, byte for byte. */

/* Encodes n strips that lie in device memory.  Strip k: rows[k] rows of row_bytes[k] bytes, row r at (const char*)src[k] +
 * r * row_stride[k] (any byte address; at most 1 GiB a strip).  The streams return packed in `out` [host, out_cap bytes]: strip
 * k at out_off[k] with lengths[k] bytes, in strip order, each stream beginning at a multiple of 4 bytes -- the up to 3 bytes
 * between a stream's end and the next stream's start are 0 and nothing else lies between them; *out_bytes is the end of the last.
 * status[k] is 0, or 1 when the stream is longer than the strip's slot; lengths[k] then still is the whole stream's length, `out`
 * holds what fitted, and the call returns MI_ERR_NOMEM after all strips are done.  The slots: with slot_off == NULL (and
 * slot_cap == NULL, d_slots == NULL) the library's own scratch, each slot rows * row_bytes * 3 / 2 + 16 bytes, which always
 * suffice.  Otherwise strip k is encoded into bytes [slot_off[k], slot_off[k] + slot_cap[k]) of d_slots [device, d_slots_bytes
 * bytes, 4-byte aligned; slot_off[k] a multiple of 4]; no other byte of d_slots is written.  Batches of at most 1 GB of rows and
 * 2^20 strips; synchronises `stream`. */
int mi_tiff_lzw_encode_strips_device(int dev, void* stream, int64_t n, const void* const* src, const int32_t* rows, const int32_t* row_bytes,
                                     const int64_t* row_stride, const int64_t* slot_off, const int64_t* slot_cap, void* d_slots,
                                     int64_t d_slots_bytes, void* out, int64_t out_cap, int64_t* out_off, int64_t* lengths, int32_t* status,
                                     int64_t* out_bytes);

/* mi_tiff3d_write_blocks with first[b] pointing into device memory: the same block / page / strip walk, the strips encoded on
 * the device, the same page and directory assembly -- the files equal the host route's byte for byte.  compression must be 1.
 * A stream longer than its bound is MI_ERR_NOMEM with the host route's message.  Synchronises `stream`. */
int mi_tiff3d_write_blocks_device(int dev, void* stream, int n, const char* const* paths, const void* const* first, const int64_t* strides,
                                  const int* dims, const int* page0, const int* page_total, int bytes, int compression, int rows_per_strip,
                                  int bigtiff, int n_threads);

/* The page and directory assembly alone, for strips that are already LZW streams [host]: the blocks as in mi_tiff3d_write_blocks
 * (no samples, no strides); strips[] / lengths[] hold every strip in (block, page, strip of the page) order.  What a caller uses
 * that encoded a block's strips in several mi_tiff_lzw_encode_strips_device calls (row bands).  Host only. */
int mi_tiff3d_write_blocks_encoded(int n, const char* const* paths, const int* dims, const int* page0, const int* page_total, int bytes,
                                   int rows_per_strip, int bigtiff, const void* const* strips, const int64_t* lengths, int n_threads);

/* Batches the device encoder has run in this process: the route report of the conversion's tests. */
int64_t mi_tiff_lzw_encode_device_batches(void);

#ifdef __cplusplus
}
#endif
#endif
