"""CPU: the TeraFly conversion's rules against the reference binary's goldens (tests/golden/terafly), the host TIFF block writer,
and the converter's refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image, ImageSequence

from tests import terafly_util as tu
from tests.conftest import ROOT

RUNS = tu.golden_runs()
CLI = os.path.join(ROOT, "image-preprocessing-pipeline_amd", "teraconverter.py")


def _plan_of(g):
    from ipp_amd import terafly
    o = tu.parse_flags([str(f) for f in g["flags"]])
    return terafly.plan(tuple(int(v) for v in g["recipe_shape"]), o["resolutions"], (o["height"], o["width"], o["depth"]),
                        o["isotropic"], o["fixed_tiling"], (o["V0"], o["V1"], o["H0"], o["H1"], o["D0"], o["D1"]),
                        np.dtype(str(g["recipe_dtype"])).itemsize)


def test_golden_runs_present():
    assert len(RUNS) >= 9, RUNS


@pytest.mark.parametrize("name", RUNS)
def test_restatement_reproduces_golden(name):
    g = tu.load_golden(name)
    vol = tu.golden_input(g)
    files, mdata = tu.convert(vol, [str(f) for f in g["flags"]])
    assert sorted(list(files) + [f"{r}/mdata.bin" for r in mdata]) == [str(f) for f in g["files"]]
    for f, pages in files.items():
        n, h, w, _ = (int(v) for v in g[f"pages/{f}"])
        assert pages.shape == (n, h, w), f
        if f"sample/{f}" in g.files:
            np.testing.assert_array_equal(pages[g[f"sample_idx/{f}"]], g[f"sample/{f}"], err_msg=f)
        assert tu.pages_sha(pages) == str(g[f"sha/{f}"]), f
    for r, b in mdata.items():
        assert b == g[f"mdata/{r}/mdata.bin"].tobytes(), r


@pytest.mark.parametrize("name", RUNS)
def test_plan_names_and_mdata_match_golden(name, tmp_path):
    from ipp_amd import terafly
    g = tu.load_golden(name)
    p = _plan_of(g)
    assert terafly.output_files(p) == [str(f) for f in g["files"]]
    for i in range(p.n_res):
        if p.selected[i]:
            (tmp_path / p.res_dir(i)).mkdir()
    terafly.write_mdata(p, tmp_path)
    for f in g["files"]:
        f = str(f)
        if f.endswith("mdata.bin"):
            assert (tmp_path / f).read_bytes() == g[f"mdata/{f}"].tobytes(), f


def test_too_many_resolutions_refused_as_the_reference():
    from ipp_amd import terafly
    g = np.load(os.path.join(tu.GOLDEN, "refused.npz"))
    o = tu.parse_flags([str(f) for f in g["flags"]])
    with pytest.raises(ValueError, match="too much resolutions"):
        terafly.plan(tuple(int(v) for v in g["recipe_shape"]), o["resolutions"])
    assert "too much resolutions(6): too much slices (32)" in str(g["message"])
    with pytest.raises(ValueError, match=r"too much resolutions\(6\): too much slices \(32\)"):
        terafly.plan(tuple(int(v) for v in g["recipe_shape"]), o["resolutions"])


def test_small_blocks_refused():
    from ipp_amd import terafly
    with pytest.raises(ValueError, match="250"):
        terafly.plan((40, 300, 300), "01", block=(100, 300, -1))


def test_halving_2d_rule():
    a = np.array([[[1, 2], [3, 5]]], np.uint16)
    assert tu.halve2d(a, "mean")[0, 0, 0] == 3          # 11 / 4 = 2.75 -> 3
    a = np.array([[[1, 1], [1, 3]]], np.uint16)
    assert tu.halve2d(a, "mean")[0, 0, 0] == 2          # 6 / 4 = 1.5 -> 2 (half away from zero)
    b = np.zeros((2, 2, 2), np.uint16)
    b[0, 0, 0] = 4
    assert tu.halve3d(b, "mean")[0, 0, 0] == 1          # 4 / 8 = 0.5 -> 1
    assert tu.halve3d(b, "max")[0, 0, 0] == 4


# ------------------------------------------------------------------------------------------------------------------ TIFF writer
def _write(path, vol, comp=1, rps=1, page0=0, total=None, big=0, threads=4):
    from ipp_amd import capi
    lib = capi.lib()
    capi.check(lib.mi_tiff3d_write_blocks(1, (C.c_char_p * 1)(os.fsencode(str(path))), (C.c_void_p * 1)(vol.ctypes.data),
                                          (C.c_int64 * 2)(vol.strides[0] // vol.itemsize, vol.strides[1] // vol.itemsize),
                                          (C.c_int * 3)(vol.shape[2], vol.shape[1], vol.shape[0]), (C.c_int * 1)(page0),
                                          (C.c_int * 1)(total or vol.shape[0]), vol.itemsize, comp, rps, big, threads))


def _read(path):
    im = Image.open(path)
    return np.stack([np.asarray(p) for p in ImageSequence.Iterator(im)]), im


def _edge_rows(dtype, w):
    info = np.iinfo(dtype)
    rng = np.random.default_rng(5)
    return np.stack([
        np.full((3, w), 7, dtype),                                            # a constant row: a handful of codes
        np.tile(np.array([0, info.max], dtype), (3, (w + 1) // 2))[:, :w],    # alternating values
        rng.integers(0, info.max + 1, (3, w), dtype=dtype),                   # random: widths up to 12 bits, table resets
    ])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("comp,big,rps", [(1, 0, 1), (1, 0, 2), (0, 0, 1), (1, 1, 1), (0, 1, 3)])
def test_tiff3d_writer_reads_back(tmp_path, dtype, comp, big, rps):
    vol = _edge_rows(dtype, 9001)
    path = tmp_path / "b.tif"
    _write(path, vol[:2], comp, rps, 0, 5, big)
    _write(path, vol[2:], comp, rps, 2, 5, big)
    pages, im = _read(path)
    np.testing.assert_array_equal(pages, vol)
    assert int(im.tag_v2.get(259)) == (5 if comp else 1)
    assert int(im.tag_v2.get(278)) == rps
    im.seek(0)
    assert tuple(im.tag_v2.get(297)) == (0, 5)


def test_tiff3d_writer_views_and_many_blocks(tmp_path):
    """Blocks cut out of one level array (row / page strides) written together, as terafly.convert does."""
    from ipp_amd import capi
    lib = capi.lib()
    rng = np.random.default_rng(1)
    lv = rng.integers(0, 65536, (6, 50, 70), dtype=np.uint16)
    cuts = [(0, 3, 0, 25, 0, 33), (0, 3, 0, 25, 33, 70), (3, 6, 25, 50, 0, 70)]
    paths = [os.fsencode(str(tmp_path / f"{k}.tif")) for k in range(len(cuts))]
    first, strides, dims = [], [], []
    for z0, z1, y0, y1, x0, x1 in cuts:
        first.append(lv[z0:, y0:, x0:].ctypes.data)
        strides += [50 * 70, 70]
        dims += [x1 - x0, y1 - y0, z1 - z0]
    n = len(cuts)
    capi.check(lib.mi_tiff3d_write_blocks(n, (C.c_char_p * n)(*paths), (C.c_void_p * n)(*first), (C.c_int64 * (2 * n))(*strides),
                                          (C.c_int * (3 * n))(*dims), (C.c_int * n)(0, 0, 0), (C.c_int * n)(3, 3, 3), 2, 1, 1, 0, 0))
    for k, (z0, z1, y0, y1, x0, x1) in enumerate(cuts):
        np.testing.assert_array_equal(_read(paths[k].decode())[0], lv[z0:z1, y0:y1, x0:x1])


def test_tiff3d_append_checks_page_count(tmp_path):
    from ipp_amd import capi
    vol = np.zeros((2, 4, 4), np.uint8)
    _write(tmp_path / "a.tif", vol)
    with pytest.raises(capi.MiError, match="holds 2 pages"):
        _write(tmp_path / "a.tif", vol, page0=3)


def _lzw_decode(data):
    """A plain TIFF LZW decoder (early change), independent of the encoder."""
    bits = "".join(f"{b:08b}" for b in data)
    pos, width, table, out, prev = 0, 9, None, bytearray(), None
    while pos + width <= len(bits):
        code = int(bits[pos:pos + width], 2)
        pos += width
        if code == 256:
            table = [bytes([i]) for i in range(256)] + [b"", b""]
            width, prev = 9, None
            continue
        if code == 257:
            break
        if prev is None:
            entry = table[code]
        else:
            entry = table[code] if code < len(table) else prev + prev[:1]
            table.append(prev + entry[:1])
        out += entry
        prev = entry
        if len(table) + 1 >= (1 << width) and width < 12:
            width += 1
    return bytes(out)


@pytest.mark.parametrize("kind", ["empty", "one", "constant", "alternating", "reset"])
def test_lzw_encoder_edge_streams(kind):
    from ipp_amd import capi
    rng = np.random.default_rng(3)
    src = {"empty": b"", "one": b"\x05", "constant": b"\x07" * 5000, "alternating": b"\x00\xff" * 3000,
           "reset": rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()}[kind]
    cap = len(src) * 3 // 2 + 16
    dst = (C.c_uint8 * cap)()
    n = C.c_int64()
    capi.check(capi.lib().mi_tiff_lzw_encode(src, len(src), dst, cap, C.byref(n)))
    enc = bytes(dst[:n.value])
    assert _lzw_decode(enc) == src
    if kind == "constant":
        assert n.value < 200


# ------------------------------------------------------------------------------------------------------------------ CLI
def _cli(*args):
    return subprocess.run([sys.executable, CLI] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          cwd=ROOT)


def test_cli_refuses_other_formats_and_channels(tmp_path):
    ok = ['--sfmt=TIFF (series, 2D)', '--dfmt=TIFF (tiled, 3D)', f"-s={tmp_path}", f"-d={tmp_path}"]
    r = _cli('--sfmt=TIFF (tiled, 3D)', '--dfmt=TIFF (tiled, 3D)', f"-s={tmp_path}", f"-d={tmp_path}")
    assert r.returncode == 2 and "--sfmt" in r.stdout and "TIFF (series, 2D)" in r.stdout
    r = _cli('--sfmt=TIFF (series, 2D)', '--dfmt=HDF5 (Imaris IMS)', f"-s={tmp_path}", f"-d={tmp_path}")
    assert r.returncode == 2 and "--dfmt" in r.stdout
    r = _cli(*ok, "--clist=1")
    assert r.returncode == 2 and "--clist" in r.stdout
    r = _cli(*ok, "--halve=median")
    assert r.returncode == 2 and "--halve" in r.stdout
    src = tmp_path / "rgb"
    src.mkdir()
    for k in range(3):
        Image.fromarray(np.zeros((260, 260, 3), np.uint8)).save(src / f"s_{k}.tif")
    dst = tmp_path / "out"
    dst.mkdir()
    r = _cli('--sfmt=TIFF (series, 2D)', '--dfmt=TIFF (tiled, 3D)', f"-s={src}", f"-d={dst}", "--clist=0")
    assert r.returncode == 2 and "multi-channel" in r.stdout, r.stdout
    r = _cli(*ok[:2], f"-s={tmp_path}", f"-d={tmp_path / 'missing'}")
    assert r.returncode == 2 and "existing folder" in r.stdout
