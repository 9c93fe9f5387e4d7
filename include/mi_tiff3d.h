/* mi_tiff3d.h -- reading the block files of a TeraFly tree ("TIFF (tiled, 3D)"): multi-page TIFF, one page per slice, strips of
 * any RowsPerStrip, uncompressed or LZW.  The host reader and the device reader take the same files and refuse the others in the
 * same words.  The device reader decodes the LZW strips on the device (a strip per wave) and never holds a decoded page on the host.
 *
 * A file is taken when it is a little-endian classic TIFF or BigTIFF whose pages all have the same extents and type, one sample per
 * pixel, 8 or 16 bits unsigned, strips, compression 1 (none) or 5 (LZW), no predictor (tag 317 absent or 1).  Anything else is
 * MI_ERR_INVALID with the file, the page and the tag in the message.  Strips must lie inside the file, uncompressed strips must be
 * as long as their rows.
 */
#ifndef MI_TIFF3D_H
#define MI_TIFF3D_H

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A piece of one block file and where it goes in the box: pages [p0, p1), rows [y0, y1) and columns [x0, x1) of the file land at
 * out[oz + p - p0][oy + y - y0][ox + x - x0]. */
typedef struct {
    const char* path;
    int p0, p1, y0, y1, x0, x1;
    int oz, oy, ox;
} mi_tiff3d_job;

/* status of an LZW strip (csrc/tiff_lzw_dev.h) */
typedef enum {
    MI_LZW_OK = 0,
    MI_LZW_CODE = 1,      /* a code above the next free entry */
    MI_LZW_FIRST = 2,     /* the first code of the strip, or after Clear, is not a literal */
    MI_LZW_INPUT = 3,     /* the input ended before the rows were full */
    MI_LZW_OUTPUT = 4,    /* a string would pass the end of the rows */
    MI_LZW_OLD_STYLE = 5, /* the LSB-first stream of writers before TIFF 5.0 */
    MI_LZW_TABLE = 6      /* the table is full and no Clear came */
} mi_lzw_status;

/* What a block file holds: columns, rows, pages, bytes per sample (1 or 2), the compression tag (1 or 5), RowsPerStrip and whether
 * it is a BigTIFF.  Runs every check of the readers.  Replaces the open / TIFFGetField part of Tiff3DMngr.cpp: readTiff3DFile2Buffer
 * and loadTiff3D2Metadata. */
int mi_tiff3d_info(const char* path, int* nx, int* ny, int* pages, int* dtype, int* compression, int* rows_per_strip, int* bigtiff);

/* LZW (TIFF) decoding of the n bytes of src into exactly `want` bytes of dst: the inverse of the encoder of mi_pyramid.h, and what
 * libtiff's LZWDecode does for one strip.  *status receives an mi_lzw_status; a status other than 0 returns MI_ERR_INVALID (dst is then
 * unspecified).  Host only: the yardstick of the device decoder, which runs the same text. */
int mi_tiff_lzw_decode(const void* src, int64_t n, void* dst, int64_t want, int* status);

/* Fills the box out[box_z][box_y][box_x] (host memory, samples of `bytes` = 1 or 2 bytes, C order) from n_jobs pieces of block files.
 * Only the strips that the rows of a piece touch are read and decoded.  Voxels of the box that no piece covers are left as they
 * are.  n_threads <= 0: OMP_NUM_THREADS, else 16.  A strip that does not decode to its rows is MI_ERR_INVALID naming the file, the
 * page, the strip and the status; the box is then unspecified.  Replaces Tiff3DMngr.cpp: readTiff3DFile2Buffer under
 * TiledVolume::loadSubvolume_to_UINT8 (one call per block there, all blocks of the box here). */
int mi_tiff3d_read_box(const mi_tiff3d_job* jobs, int n_jobs, int box_z, int box_y, int box_x, int bytes, void* out, int n_threads);

/* The same box in device memory (`out` on device `dev`): the host parses and reads the touched strips into pinned memory, the
 * device decodes the LZW strips and places the rows.  Same files, same refusals, same words.  Returns when the box is complete on
 * `stream`.  Keeps pinned and device scratch per device, sized by the largest batch seen; mi_release_cached_memory gives it back.
 * Replaces TiledVolume::loadSubvolume_to_UINT8 followed by an upload. */
int mi_tiff3d_read_box_device(int dev, void* stream, const mi_tiff3d_job* jobs, int n_jobs, int box_z, int box_y, int box_x, int bytes,
                              void* out, int n_threads);

#ifdef __cplusplus
}
#endif
#endif
