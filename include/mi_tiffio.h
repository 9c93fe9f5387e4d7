/* TIFF series I/O of the block pipeline: the slices decwrap.py reads its boxes from and writes its result to.  Host code, but for the
 * two *_device functions: the writer that deflates on the device and the reader that inflates there.
 *
 * Replaces, for the files the pipeline itself meets, LsDeconvolveMultiGPU/load_bl_tif.cpp (a box of a folder of 2-D TIFF slices,
 * one libtiff handle per thread) and save_bl_tif.cpp (one slice per task on all cores, Adobe deflate at ZIPQUALITY 1, predictor 1:
 * save_bl_tif.cpp:336-346, called with 'deflate' by LsDeconv.m:1140-1145).  Python's Pillow writes 29 MB/s of deflate TIFF and holds
 * the interpreter lock while it does: 17 GB of result would take ten minutes where the deconvolution takes five seconds.
 *
 * Scope of the reader ("fast" files): classic little-endian TIFF, one sample per pixel, 8 / 16 / 32 bits (unsigned integer or IEEE
 * float), strips (any RowsPerStrip), compression none / Adobe deflate (8) / deflate (32946), predictor none or horizontal
 * differencing (2).  Everything else -- tiles, LZW, BigTIFF, big-endian, palettes -- is reported as not fast and left to the caller's
 * general reader (brickio.py falls back to Pillow).  The writer produces exactly such files.
 *
 * All functions return MI_OK or an mi_status (mi_common.h); the message is available through mi_last_error(). */
#ifndef MI_TIFFIO_H
#define MI_TIFFIO_H

#include "mi_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Width, height and sample type (1 = uint8, 2 = uint16, 4 = float32; 0 = none of these) of the first image of a file, and
 * whether mi_tiff_read_box can decode it (*fast = 1).  MI_ERR_INVALID when the file cannot be opened or is not a TIFF. */
int mi_tiff_info(const char* path, int* nx, int* ny, int* dtype, int* fast);

/* out[k][y - y0][x - x0] = slice paths[k] at (y, x) for y in [y0, y1), x in [x0, x1): a box of n slices, decoded on n_threads
 * threads (<= 0: all cores), only the strips the rows touch.  Every file must be fast (mi_tiff_info), of extents nx x ny and
 * sample type dtype; out holds n * (y1 - y0) * (x1 - x0) samples.   [load_bl_tif.cpp: load_bl_tif(files, y, x, height, width)] */
int mi_tiff_read_box(const char* const* paths, int n, int nx, int ny, int dtype, int y0, int y1, int x0, int x1, void* out,
                     int n_threads);

/* One file per z slice of vol [nz][ny][nx]: paths[k] <- slice k, written under a temporary name and renamed when complete; a path
 * that already exists is left alone (LsDeconv.m:1120-1132) -- *written (may be NULL) counts the files produced.
 * compression: 0 none, 1 Adobe deflate at `level` (1 .. 9; save_bl_tif.cpp uses 1).  n_threads <= 0: all cores.
 * [save_bl_tif.cpp: save_bl_tif(volume, fileList, isXYZ, compression, nThreads, useTiles = false)] */
int mi_tiff_write_series(const char* const* paths, int nz, const void* vol, int dtype, int nx, int ny, int compression, int level,
                         int n_threads, int* written);

/* The same files from a volume that lies in DEVICE memory (vol [nz][ny][nx] on device `dev`), deflated there: every strip is one
 * dynamic-Huffman block (csrc/tiff_deflate.hip: counting kernels, codes built on the host, encode kernel), the host only frames the streams
 * and writes the files.  The only string matching is that of runs: a strip is coded either with every byte a literal, or -- when that
 * is shorter, as on the zero background of a stitched or clipped volume -- with its runs of equal bytes as matches at distance 1
 * (zlib's Z_RLE; the token rule is in DESIGN.md, "TIFF on the device").  MI_TIFF_DEVICE_RUNS=0 in the environment (read per call)
 * keeps every strip in the literal form.  Adobe deflate always; readable by any inflater.  Enqueues on `stream` and synchronises
 * it.  No counterpart in the reference (save_bl_tif.cpp compresses on the host's cores). */
int mi_tiff_write_series_device(int dev, void* stream, const char* const* paths, int nz, const void* vol, int dtype, int nx, int ny,
                                int n_threads, int* written);

/* mi_tiff_read_box with `out` in DEVICE memory (n * (y1 - y0) * (x1 - x0) samples on device `dev`): the same files, the same
 * refusals in the same words -- the host parses the directories exactly as mi_tiff_read_box does -- but the strips the rows touch
 * cross to the device as they are in the files (pread into pinned memory on n_threads threads, copied in batches of at most 1 GB
 * of file bytes, 1 GB of inflated rows and 16384 strips) and are decoded there: k_strip_inflate inflates one zlib stream per wave (csrc/tiff_inflate_dev.h: a complete RFC 1950 / 1951
 * inflater -- stored, fixed and dynamic blocks, any number of them, distances up to 32768, Adler-32 verified; bytes after the
 * trailer are ignored), k_strip_unpredict_crop undoes predictor 2 and copies the box's rows and columns (strips that are not
 * compressed take it alone).  A strip that does not inflate to its rows gives MI_ERR_INVALID; the message names the file, the strip
 * and the decoder's status (header, block type, stored length, over-subscribed / incomplete code, no end-of-block code, invalid
 * symbol, distance before the start, input exhausted, output size, checksum); what `out` holds is then unspecified.  No input makes
 * the decoder read past a strip's bytes, write past its rows or run on.  Enqueues on `stream` and synchronises it.  The pinned and
 * device scratch is kept per device between calls, sized by the largest batch seen; mi_release_cached_memory gives it back.
 * No counterpart in the reference (load_bl_tif.cpp inflates on the host's cores). */
int mi_tiff_read_box_device(int dev, void* stream, const char* const* paths, int n, int nx, int ny, int dtype, int y0, int y1, int x0,
                            int x1, void* out /* device */, int n_threads);

/* one strip (n bytes, rows of rowb bytes, samples of bps bytes) as the device writer codes it, computed on the host by the same rule:
 * pred 0 / 1 (horizontal differencing), runs 0 (literal-only) / 1 (the shorter of the two forms); the whole zlib stream goes to out.
 * *nbytes receives its length (MI_ERR_NOMEM when cap is smaller; n + n / 32 + 4096 always suffices), *used_runs (may be NULL)
 * whether the run form was taken.  The yardstick of the device path in tests; needs no GPU. */
int mi_tiff_deflate_strip_host(const unsigned char* bytes, size_t n, int bps, size_t rowb, int pred, int runs, unsigned char* out, size_t cap,
                               size_t* nbytes, int* used_runs);

/* One RGB file per z slice of vol [nz][ny][nx][3] (host memory), the `RGB` series of align_images.py: classic little-endian TIFF,
 * SamplesPerPixel 3, PhotometricInterpretation 2 (RGB), PlanarConfiguration 1 (chunky), strips, SampleFormat per type.
 * dtype: 1 = uint8, 2 = uint16, 3 = uint32, 4 = float32.  compression: 0 none (what the reference's imwrite writes), 1 Adobe deflate
 * at `level` (1 .. 9).  As with mi_tiff_write_series, a file is written under a temporary name and renamed, and a path that exists
 * is left alone; *written (may be NULL) counts the files produced.  mi_tiff_info reports such files as not fast.
 * [align_images.py:51-63 and :322-328: imwrite(path, composite.astype(dtype))] */
int mi_tiff_write_rgb_series(const char* const* paths, int nz, const void* vol, int dtype, int nx, int ny, int compression, int level,
                             int n_threads, int* written);

/* Name of the deflate implementation in use: "libdeflate" when libdeflate.so.0 could be loaded, else "zlib". */
const char* mi_tiff_codec(void);

#ifdef __cplusplus
}
#endif
#endif
