"""GPU: the run form of the device TIFF writer (mi_tiff_write_series_device: a strip's runs of equal bytes as deflate matches at
distance 1 when that is shorter than every byte a literal).  Every strip in a file must be, bit for bit, what the host yardstick
``mi_tiff_deflate_strip_host`` makes of the same rows (tests/test_tiff_runs_host.py holds that one to the token rule), runs that
straddle the lanes' 32 bytes, the waves' 2048, the tiles' 8192 and the strips included; the files read back exactly; zero and
sparse slices reach the sizes of zlib's Z_RLE; MI_TIFF_DEVICE_RUNS=0 gives the literal form of every strip.

Sparse fixture (tests/deflate_util.sparse_disc, 1024 x 1024), device bytes over Z_RLE level 1 on the same stored bytes, per strip,
measured on an MI355X: at most 1.0027 (uint16) and 1.0009 (uint8) -- see profiles/NOTES.md; asserted: that excess rounded up to the
next whole percent, plus one."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from ipp_amd import brickio
from tests import deflate_util as du

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_and_compare(dev, folder, vol, want_runs=None):
    """vol through the device writer: every strip of every file equals the host yardstick's stream of its rows, Pillow and the
    library's reader give the volume back; returns the list of (stream, used_runs) of all strips"""
    from PIL import Image
    vol = np.ascontiguousarray(vol)
    assert brickio.save_tiff_series_device(folder, torch.from_numpy(vol).to(dev)) == vol.shape[0]
    files = brickio.list_tiff_series(folder)
    assert len(files) == vol.shape[0]
    bps, rowb = vol.dtype.itemsize, vol.shape[2] * vol.dtype.itemsize
    out = []
    for z, f in enumerate(files):
        streams, pred, rps = du.file_strips(f)
        assert len(streams) == -(-vol.shape[1] // rps)
        for si, s in enumerate(streams):
            rows = vol[z, si * rps:(si + 1) * rps]
            host, used = du.host_strip(rows.tobytes(), bps, rowb, pred, 1)
            assert s == host, (vol.shape, str(vol.dtype), z, si, pred, used, len(s), len(host))
            out.append((s, used))
    back = np.stack([np.asarray(Image.open(f)).reshape(vol.shape[1:]) for f in files])
    assert back.dtype == vol.dtype and back.tobytes() == vol.tobytes()           # (bytes: folded patterns hold NaNs as float32)
    assert brickio.load_tiff_series(folder).tobytes() == vol.tobytes()
    if want_runs is not None:
        assert all(u == want_runs for _, u in out), [u for _, u in out]
    return out


def _fold(data, shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    reps = -(-n // data.size)
    return np.tile(data, reps)[:n].view(dtype).reshape(shape)


def test_equal_strips_and_run_patterns_as_single_rows(dev, tmp_path):
    k = 0
    for n in du.EQUAL_LENGTHS:
        for value in (0, 173):
            _write_and_compare(dev, tmp_path / f"e{k}", np.full((1, 1, n), value, np.uint8))
            k += 1
    for seed in (1, 2, 3):
        _write_and_compare(dev, tmp_path / f"p{seed}", du.run_pattern(seed).reshape(1, 1, -1), want_runs=1)


@pytest.mark.parametrize("shape,dtype", [((2, 37, 211), np.uint8), ((2, 64, 70), np.uint16), ((1, 50, 77), np.float32)],
                         ids=["u8_2x37x211", "u16_2x64x70", "f32_1x50x77"])
def test_run_patterns_folded_into_volumes(dev, tmp_path, shape, dtype):
    for seed in (1, 2, 3):
        vol = _fold(du.run_pattern(seed), shape, dtype)
        res = _write_and_compare(dev, tmp_path / f"s{seed}", vol)
        assert any(u for _, u in res)
    _write_and_compare(dev, tmp_path / "z", np.zeros(shape, dtype), want_runs=1)
    # a constant: runs as it is (uint8), once differenced (uint16), and none at all in the four bytes of a float32
    _write_and_compare(dev, tmp_path / "c", np.full(shape, 1234 if dtype != np.uint8 else 200, dtype), want_runs=0 if dtype == np.float32 else 1)


@pytest.mark.parametrize("edge,sizes", [(32, (31, 32, 33)), (2048, (2047, 2048, 2049, 2050)), (8192, (8191, 8192, 8193, 8194, 3 * 8192 + 5))],
                         ids=["lane_32", "wave_2048", "tile_8192"])
def test_zero_runs_that_straddle_the_boundaries(dev, tmp_path, edge, sizes):
    k = 0
    for n in sizes:
        edges = list(range(edge, n + 2, edge)) if edge == 8192 else [edge]      # every tile boundary of the strip (spans are clipped)
        cases = [np.zeros(n, np.uint8)]
        for a, b in ((1, 1), (1, 3), (2, 2), (3, 1), (2, 1), (3, 3), (260, 2), (2, 260), (300, 300)):
            cases.append(du.straddle_pattern(n, [(e - a, e + b) for e in edges]))
        cases.append(du.straddle_pattern(n, [(e - 40, n) for e in edges[:1]]))                 # a run to the end of the strip
        cases.append(du.straddle_pattern(n, [(0, edges[0] + 1)]))                               # and one from its start
        # runs over every 32-byte lane boundary of the strip, of lengths and offsets that change from one to the next
        cases.append(du.straddle_pattern(n, [(32 * i - i % 4, 32 * i - i % 4 + 1 + i % 9) for i in range(1, n // 32 + 1)]))
        for d in cases:
            res = _write_and_compare(dev, tmp_path / f"b{k}", d.reshape(1, 1, -1))
            k += 1
            if n >= 2047 and (not d.any() or (d[-300:] == 0).all()):
                assert res[0][1] == 1, (n, "a long zero run must take the run form")


def test_a_run_ends_with_its_strip(dev, tmp_path):
    vol = np.zeros((1, 1100, 1001), np.uint8)
    res = _write_and_compare(dev, tmp_path / "z", vol, want_runs=1)
    assert len(res) == 2                                    # 1047 rows and 53
    for stream, _ in res:
        tokens, _info = du.read_block(stream)
        assert tokens[0] == 0 and tokens[1] == (258, 1, 285)         # every strip opens with a literal


def test_zero_slice_size(dev, tmp_path):
    vol = np.zeros((1, 2048, 2048), np.uint16)
    assert brickio.save_tiff_series_device(tmp_path / "z", torch.from_numpy(vol).to(dev)) == 1
    f = brickio.list_tiff_series(tmp_path / "z")[0]
    streams, _pred, rps = du.file_strips(f)
    n = rps * 2048 * 2
    assert len(streams) == 8 and n == 1 << 20
    for s in streams:
        assert zlib.decompress(s) == bytes(n)
        assert len(s) <= n / 512 + 512, (len(s), n)
    assert np.array_equal(brickio.load_tiff_series(tmp_path / "z"), vol)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8], ids=["u16", "u8"])
def test_sparse_slice_against_zlib_rle(dev, tmp_path, dtype):
    vol = du.sparse_disc(dtype)[None]
    res = _write_and_compare(dev, tmp_path / "s", vol, want_runs=1)
    _streams, pred, rps = du.file_strips(brickio.list_tiff_series(tmp_path / "s")[0])
    for si, (s, _) in enumerate(res):
        rle = du.rle_size(du.stored(vol[0, si * rps:(si + 1) * rps], pred))
        print(f"sparse {np.dtype(dtype).name} strip {si}: device {len(s)} bytes, Z_RLE level 1 {rle}, ratio {len(s) / rle:.4f}, predictor {pred}")
        assert len(s) <= 1.02 * rle + 400, (si, len(s), rle)


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from ipp_amd import brickio
from tests import test_gpu_tiff_runs as t
dev = torch.device("cuda", 0)
for name, vol in t._switch_volumes():
    brickio.save_tiff_series_device(sys.argv[2] + "/" + name, torch.from_numpy(vol).to(dev))
"""


def _switch_volumes():
    rng = np.random.default_rng(12)       # the smooth field and the noise of tests/test_gpu_tiff_device.py's size test
    smooth = (np.cumsum(rng.standard_normal((4, 1024, 1024)), axis=2) * 6 + 3000 + rng.random((4, 1024, 1024)) * 40).clip(0, 65535).astype(np.uint16)
    noise = (rng.random((2, 512, 640)) * 65535).astype(np.uint16)
    return [("zero", np.zeros((1, 2048, 2048), np.uint16)), ("smooth", smooth), ("noise", noise)]


def test_switch_off_gives_the_literal_form(dev, tmp_path):
    """MI_TIFF_DEVICE_RUNS=0 in a fresh process: the zero slice is what the writer made before it knew runs (every strip the host
    yardstick's literal form, an eighth of the samples); dense content is the same file with the switch at 0 and at 1"""
    off = tmp_path / "off"
    off.mkdir()
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(off)], check=True, env=dict(os.environ, MI_TIFF_DEVICE_RUNS="0"), timeout=300)
    for name, vol in _switch_volumes():
        a = brickio.list_tiff_series(off / name)
        assert len(a) == vol.shape[0]
        if name == "zero":
            streams, pred, rps = du.file_strips(a[0])
            for si, s in enumerate(streams):
                rows = vol[0, si * rps:(si + 1) * rps]
                lit, _ = du.host_strip(rows.tobytes(), 2, 4096, pred, 0)
                assert s == lit and len(s) > rows.nbytes // 8
            continue
        brickio.save_tiff_series_device(tmp_path / name, torch.from_numpy(vol).to(dev))
        b = brickio.list_tiff_series(tmp_path / name)
        for fa, fb in zip(a, b):
            assert fa.read_bytes() == fb.read_bytes(), (name, fa.name)
