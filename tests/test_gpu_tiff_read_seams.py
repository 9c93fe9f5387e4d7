"""GPU: the code of the two device TIFF readers that exists only on the device, at its seams -- the wave contexts of k_strip_inflate
(csrc/tiff_inflate.hip: input staged a kilobyte at a time, the pending window in LDS and its offset ``flushed & 3``, matches taken
from LDS or global memory, the Adler sums) and of k_strip_lzw (csrc/tiff3d_read.hip: strips that begin at any byte, the three strip
classes), the predictor scan and the row loops of k_strip_unpredict_crop and k_tree_place, and the host code that cuts a call into
batches.  All inputs are valid files; the yardsticks are the bytes the files were made from and the host readers; everything is exact.

The streams come from tests/inflate_util.py, tests/lzw_util.py and tests/terafly_read_util.py; that each one reaches the seam it is
named after (``flushed % 4``, the bytes pending before a match, clears, offsets above 65535 ...) is asserted by
tests/test_tiff_seam_streams_host.py, which also passes every stream through the decoder cores under the host sanitizers."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

from ipp_amd import brickio, capi
from tests import inflate_util as iu
from tests import lzw_util as lu
from tests import terafly_read_util as ru

pytestmark = pytest.mark.gpu


def _both(files, shape, dtype, box, dev):
    """the box through the device reader, required to equal the host reader's; returns it as numpy"""
    y0, y1, x0, x1 = box
    want = brickio.read_tiff_box(files, shape, dtype, y0, y1, x0, x1)
    got = brickio.read_tiff_box_device(files, shape, dtype, y0, y1, x0, x1, device=dev)
    assert got.device == dev and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (shape, str(np.dtype(dtype)), box)
    return got


def _read_both(items, box, dev):
    """items: [(path, pages, (y0, y1), cols, oz)]: rows [y0, y1) of every page of uint8 files into a box of uint8, through both tree
    readers; (host bytes, device bytes), no error allowed"""
    jobs = (capi.Tiff3dJob * len(items))(*[capi.Tiff3dJob(os.fsencode(p), 0, n, y0, y1, 0, w, oz, 0, 0) for p, n, (y0, y1), w, oz in items])
    lib = capi.lib()
    host = np.full(box, 0xee, np.uint8)
    capi.check(lib.mi_tiff3d_read_box(jobs, len(items), box[0], box[1], box[2], 1, host.ctypes.data, 2))
    out = torch.full(box, 0xee, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.mi_tiff3d_read_box_device(dev.index, capi.current_stream_ptr(dev), jobs, len(items), box[0], box[1], box[2], 1, out.data_ptr(), 2))
    return host, out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ inflate: the wave context
def test_every_inflate_seam_stream_as_the_strip_of_a_file(dev, tmp_path):
    """pend_offset_0..3 (``flushed & 3``, the last byte of the pending window, sources in LDS, in global memory and across both),
    overlap_across_flush, stage_edge_* (the last staged word), adler_tail_* and adler_big (the sums)"""
    c = iu.seam_corpus()
    assert len(c) == 4 + 1 + 12 + 1 + 5 + 1
    for name, (stream, data) in sorted(c.items()):
        f = iu.stream_tiff(tmp_path / f"{name}.tif", stream, len(data))
        got = _both([f], (1, len(data)), np.uint8, (0, 1, 0, len(data)), dev)
        assert got.tobytes() == data, name


# ------------------------------------------------------------------------------------------------ LZW: alignment and classes
def test_every_lzw_seam_strip_as_the_strip_of_a_one_page_file(dev, tmp_path):
    for name, (stream, data) in sorted(lu.seam_corpus().items()):
        f = ru.strip_tiff(tmp_path / f"{name}.tif", stream, len(data))
        host, got = _read_both([(f, 1, (0, 1), len(data), 0)], (1, 1, len(data)), dev)
        assert got.tobytes() == host.tobytes() == data, name


def test_the_three_lzw_classes_launch_together(dev, tmp_path):
    """noise that fills and resets the table with its rows in global memory (16-bit and 32-bit offsets), strings defined and used
    above offset 65535, and a strip of one byte (rows in LDS), in one call"""
    c = dict(lu.seam_corpus())
    c["one_byte"] = lu.corpus()["one_byte"]
    names = ["noise_40000", "noise_65536", "noise_70001", "far_strings", "one_byte"]
    sizes = [len(c[k][1]) for k in names]
    assert sum(n <= 16384 for n in sizes) == 1 and sum(16384 < n <= 65536 for n in sizes) == 2 and sum(n > 65536 for n in sizes) == 2
    items = [(ru.strip_tiff(tmp_path / f"{k}.tif", c[k][0], len(c[k][1])), 1, (0, 1), len(c[k][1]), z) for z, k in enumerate(names)]
    host, got = _read_both(items, (len(names), 1, max(sizes)), dev)
    assert got.tobytes() == host.tobytes()
    for z, k in enumerate(names):
        assert got[z, 0, :sizes[z]].tobytes() == c[k][1] and (got[z, 0, sizes[z]:] == 0xee).all(), k


ALIGNED_SIZES = (129, 255, 256, 257, 511, 512, 513, 300, 384, 385, 640, 700, 258, 514, 256, 512)
ALIGNED_SHIFTS = (0, 1, 2, 3, 3, 1, 2, 0, 1, 2, 3, 0, 1, 2, 0, 0)


def test_lzw_strips_at_every_byte_residue(dev, tmp_path):
    """16 one-row strips of one page, 0 to 3 bytes between them: the strips of a page are read as one run and uploaded from a multiple
    of 16, so a strip's first byte lies at byte (its offset - the run's first offset) % 4 of an aligned word.  Strips of 255 to 257
    and 511 to 513 bytes (the staged 256 bytes) at every residue but 0, of 256 and 512 also at 0."""
    width = 640
    strips = [lu.sized_strip(width, n, 20) for n in ALIGNED_SIZES]
    gaps, end = [], 0
    for (s, _, _), shift in zip(strips, ALIGNED_SHIFTS):
        gaps.append((shift - end) % 4)
        end += gaps[-1] + len(s)
    assert set(gaps) == {0, 1, 2, 3}
    f = ru.multi_strip_tiff(tmp_path / "residues.tif", [s for s, _, _ in strips], width, 1, 5, gaps)
    (tags,), _ = lu.tiff_pages(f)
    offs, cnts = tags[273], tags[279]
    assert cnts == ALIGNED_SIZES and [b - (a + n) for a, n, b in zip(offs, cnts, offs[1:])] == gaps[1:]
    assert tuple((o - offs[0]) % 4 for o in offs) == ALIGNED_SHIFTS and {o % 4 for o in offs} == {0, 1, 2, 3}
    at = {}
    for n, shift in zip(cnts, ALIGNED_SHIFTS):
        at.setdefault(n, set()).add(shift)
    assert at[255] | at[256] | at[257] == at[511] | at[512] | at[513] == {0, 1, 2, 3} and at[256] == {0, 2} and at[512] == {0, 1}
    host, got = _read_both([(f, 1, (0, 16), width, 0)], (1, 16, width), dev)
    assert got.tobytes() == host.tobytes() == b"".join(d for _, d, _ in strips)
    host, got = _read_both([(f, 1, (4, 7), width, 0)], (1, 3, width), dev)        # the run begins at strip 4: other residues
    assert got.tobytes() == host.tobytes() == b"".join(d for _, d, _ in strips[4:7])
    assert [(o - offs[4]) % 4 for o in offs[4:7]] == [0, 2, 3]


# ------------------------------------------------------------------------------------------------ the predictor scan
def _wrapping(dtype, ny, nx, seed):
    """full-range noise (the differences wrap), a row of the largest value and a ramp"""
    top = np.iinfo(dtype).max
    a = np.random.default_rng(seed).integers(0, top + 1, (ny, nx)).astype(dtype)
    a[1, :] = top
    a[2, :] = (np.arange(nx) * max(1, top // nx)).astype(dtype)     # (uint8: steps of 1, wrapping every 256 samples)
    return a


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("compression", [8, 1])
def test_predictor_2_on_rows_longer_than_a_block_of_the_scan(dev, tmp_path, dtype, compression):
    """the scan carries a sum across blocks of 256 samples: rows of 257, 513 and 1030, boxes that begin in every block and end
    anywhere"""
    for nx in (257, 513, 1030):
        for rps in (1, 5):
            imgs = [_wrapping(dtype, 7, nx, 10 * nx + rps + k) for k in range(2)]
            files = [iu.image_tiff(tmp_path / f"p{nx}_{rps}_{k}.tif", im, rps, compression, 2) for k, im in enumerate(imgs)]
            for x0 in (0, 255, 256, 257, 600):
                for x1 in sorted({x0 + 1, nx - 1, nx}):
                    if not x0 < x1 <= nx:
                        continue
                    for y0, y1 in ((0, 7), (2, 6)) if x1 == nx - 1 else ((0, 7),):
                        got = _both(files, (7, nx), dtype, (y0, y1, x0, x1), dev)
                        assert got.tobytes() == np.stack(imgs)[:, y0:y1, x0:x1].tobytes(), (nx, rps, y0, y1, x0, x1)


# ------------------------------------------------------------------------------------------------ the row loops
def test_strips_of_more_rows_than_the_row_grid(dev, tmp_path):
    """4100 rows in one strip: the crop kernel's grid has 1024 blocks of 4 rows and goes round again for the last four"""
    rng = np.random.default_rng(31)
    cases = [(np.uint8, 2, rng.integers(0, 256, (4100, 8)).astype(np.uint8)), (np.uint16, 1, rng.integers(0, 65536, (4100, 8)).astype(np.uint16)),
             (np.float32, 1, rng.standard_normal((4100, 8)).astype(np.float32))]
    for dtype, predictor, img in cases:
        for compression in (8,) if dtype == np.float32 else (8, 1):
            f = iu.image_tiff(tmp_path / f"rows_{np.dtype(dtype).name}_{compression}.tif", img, 4100, compression, predictor)
            for y0, y1 in ((0, 4100), (4090, 4100)):
                got = _both([f], (4100, 8), dtype, (y0, y1, 0, 8), dev)
                assert got.tobytes() == img[y0:y1].tobytes(), (str(np.dtype(dtype)), compression, y0)


def test_pages_of_more_rows_than_the_place_grid(dev, tmp_path):
    """the same shape as a one-page file of one strip, uncompressed and LZW (32 800 bytes: its rows lie in global memory)"""
    img = np.random.default_rng(32).integers(0, 256, (4100, 8), dtype=np.uint8)
    img[1000:3000] //= 64
    raw = img.tobytes()
    files = [ru.strip_tiff(tmp_path / "rows_raw.tif", raw, 8, 4100, 1), ru.strip_tiff(tmp_path / "rows_lzw.tif", lu.encode(raw), 8, 4100, 5)]
    for y0, y1 in ((0, 4100), (4090, 4100)):
        host, got = _read_both([(f, 1, (y0, y1), 8, z) for z, f in enumerate(files)], (2, y1 - y0, 8), dev)
        assert got.tobytes() == host.tobytes() == img[y0:y1].tobytes() * 2, (y0, y1)


# ------------------------------------------------------------------------------------------------ the batches
def test_slice_reader_in_two_batches(dev, tmp_path):
    """3 x 5500 strips of one row: a batch holds 16 384 strips, the second begins at row 5384 of the third file"""
    imgs = [np.random.default_rng(40 + k).integers(0, 256, (5500, 16), dtype=np.uint8) for k in range(3)]
    files = [iu.image_tiff(tmp_path / f"b{k}.tif", im, 1) for k, im in enumerate(imgs)]
    assert 3 * 5500 > 16384 > 2 * 5500
    for y0, y1 in ((0, 5500), (5400, 5500)):
        got = _both(files, (5500, 16), np.uint8, (y0, y1, 0, 16), dev)
        assert got.tobytes() == np.stack(imgs)[:, y0:y1].tobytes(), (y0, y1)


def test_tree_reader_in_two_batches(dev, tmp_path):
    """One LZW block file of 33 pages of 32768 x 4 with a row per strip: a batch holds 2^20 strips, which 32 pages are exactly, so page
    32 is a batch of its own (and a page's 32768 rows pass the place kernel's row grid eight times).
    Measured on an MI355X: the file (17 MB) is written in 0.20 s and read on the device in 0.04 s, the whole test takes 0.3 s."""
    vol = np.random.default_rng(50).integers(0, 256, (33, 32768, 4), dtype=np.uint8)
    path = str(tmp_path / "block.tif")
    lib = capi.lib()
    t0 = time.perf_counter()
    capi.check(lib.mi_tiff3d_write_blocks(1, (C.c_char_p * 1)(os.fsencode(path)), (C.c_void_p * 1)(vol.ctypes.data), (C.c_int64 * 2)(32768 * 4, 4),
                                          (C.c_int * 3)(4, 32768, 33), (C.c_int * 1)(0), (C.c_int * 1)(33), 1, 1, 1, 0, 4))
    t1 = time.perf_counter()
    pages, _ = lu.tiff_pages(path)
    assert len(pages) == 33 and all(len(t[273]) == 32768 and t[259] == 5 and t[278] == 1 for t in pages) and 32 * 32768 == 1 << 20
    jobs = (capi.Tiff3dJob * 1)(capi.Tiff3dJob(os.fsencode(path), 0, 33, 0, 32768, 0, 4, 0, 0, 0))
    out = torch.full((33, 32768, 4), 0xee, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.mi_tiff3d_read_box_device(dev.index, capi.current_stream_ptr(dev), jobs, 1, 33, 32768, 4, 1, out.data_ptr(), 2))
    t2 = time.perf_counter()
    print(f"2^20-strip block file: written in {t1 - t0:.2f} s, read on the device in {t2 - t1:.2f} s")
    assert out.cpu().numpy().tobytes() == vol.tobytes()
