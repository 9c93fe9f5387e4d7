"""CPU: every byte of the slice files of mi_tiff_write_series and mi_tiff_write_rgb_series (tiffio.hip: append_strips, finish_file).
The uncompressed files are compared, by SHA-256, with what the writers made before the two slice writers became one
(tests/golden/tiff_layout_sums.json, recorded by tests/golden/make_tiff_layout_golden.py): strips, even-byte padding, out-of-line
strip tables, the RGB triples in front of the directory, the directory and the header.  Deflated files are not pinned by a sum (that
would pin the host's zlib or libdeflate): they are read back."""
import importlib.util
import json
import os

import numpy as np
import pytest

from ipp_amd import brickio

_spec = importlib.util.spec_from_file_location(
    "make_tiff_layout_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_tiff_layout_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def sums():
    with open(gen.GOLDEN) as f:
        return json.load(f)["host"]


def test_the_golden_holds_every_case(sums):
    assert sorted(sums) == sorted(gen.HOST_CASES)


@pytest.mark.parametrize("name", list(gen.HOST_CASES))
def test_uncompressed_files_are_byte_identical(tmp_path, sums, name):
    kind, dtype, shape, strips = gen.HOST_CASES[name]
    paths = gen.write_host(name, tmp_path / "s")
    assert not list((tmp_path / "s").glob("*.tmp"))
    d = gen.directory(paths[0])
    assert d[273][1] == d[279][1] == strips and d[259][2] == 1 and 317 not in d      # the case is what its name says
    assert d[277][2] == (3 if kind == "rgb" else 1) and d[258][1] == d[339][1] == d[277][2]
    assert [gen.sha(p) for p in paths] == sums[name]


def test_the_padding_byte_and_the_strip_tables_are_where_they_were(tmp_path):
    """what the sums pin, spelled out for the two cases chosen for it"""
    p, = gen.write_host("gray_u8_1x3x5", tmp_path / "a")
    raw = open(p, "rb").read()
    d = gen.directory(p)
    assert d[273] == (4, 1, 8) and d[279] == (4, 1, 15) and raw[23] == 0 and raw[4:8] == (24).to_bytes(4, "little")
    p, = gen.write_host("gray_u16_1x600x1000", tmp_path / "b")
    raw = open(p, "rb").read()
    d = gen.directory(p)
    assert d[278][2] == 524 and d[273][2] == 8 + 1200000 and d[279][2] == d[273][2] + 8
    assert np.frombuffer(raw, "<u4", 4, d[273][2]).tolist() == [8, 8 + 524 * 2000, 524 * 2000, 76 * 2000]
    assert raw[4:8] == (d[279][2] + 8).to_bytes(4, "little")


@pytest.mark.parametrize("name", ["gray_u16_1x600x1000", "gray_f32_2x5x7", "gray_u8_1x3x5", "rgb_u8_1x5x7", "rgb_f32_1x300x400"])
def test_deflated_files_read_back(tmp_path, name):
    from PIL import Image
    kind, dtype, shape, strips = gen.HOST_CASES[name]
    paths = gen.write_host(name, tmp_path / "s", compression="tiff_adobe_deflate")
    d = gen.directory(paths[0])
    assert d[259][2] == 8 and d[273][1] == strips
    if kind == "gray":
        vol = gen.volume(dtype, shape)
        assert np.array_equal(np.stack([np.asarray(Image.open(p)) for p in paths]), vol)      # libtiff
        back = brickio.load_tiff_series(tmp_path / "s")                                        # the library's own reader
        assert back.dtype == vol.dtype and np.array_equal(back, vol)
    elif dtype == "uint8":
        assert np.array_equal(np.stack([np.asarray(Image.open(p)) for p in paths]), gen.volume(dtype, shape + (3,)))
    else:
        # (Pillow opens no float RGB, and the library's reader takes one sample per pixel: the strips through zlib)
        import zlib
        raw = open(paths[0], "rb").read()
        offs, cnts = (np.frombuffer(raw, "<u4", strips, d[t][2]) for t in (273, 279))
        assert b"".join(zlib.decompress(raw[o:o + c]) for o, c in zip(offs, cnts)) == gen.volume(dtype, shape + (3,)).tobytes()
