"""CPU: the bookkeeping of the pystripe stage against the goldens of the reference's own code (tests/golden/pystripe, made by
tests/golden/make_pystripe_golden.py), the restatement of tests/pystripe_util.py against the same goldens, and the refusals."""
import glob
import json
import os

import numpy as np
import pytest

from tests import pystripe_util as U
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", U.GOLDEN_SUBDIR)
CASES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLD, "*.npz")) if not p.endswith("host.npz"))


def load_case(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    kwargs = json.loads(str(z["kwargs"]))
    for k in ("sigma", "down_sample"):
        if kwargs.get(k) is not None:
            kwargs[k] = tuple(kwargs[k])
    return z, kwargs


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


@pytest.fixture(scope="module")
def host():
    return np.load(os.path.join(GOLD, "host.npz"))


def test_goldens_are_present():
    assert len(CASES) >= 30


def test_calculate_pad_size_python_and_c(ps, host):
    from ipp_amd import capi
    lib = capi.lib()
    for s, row in zip(host["pad_shapes"], host["pad_sizes"]):
        for sigma, want in zip(host["pad_sigmas"], row):
            assert ps.calculate_pad_size(tuple(int(v) for v in s), int(sigma)) == want
            assert U.calculate_pad_size(tuple(int(v) for v in s), int(sigma)) == want
            assert lib.mi_pystripe_pad_size(int(s[0]), int(s[1]), float(sigma)) == want, (s, sigma)


def test_convert_to_8bit_and_flat(ps, host):
    for sh in range(9):
        assert np.array_equal(ps.convert_to_8bit_fun(host["ramp"].copy(), sh), host[f"to8_shift{sh}"])
        assert np.array_equal(U.convert_to_8bit_fun(host["ramp"].copy(), sh), host[f"to8_shift{sh}"])
    assert np.array_equal(ps.convert_to_8bit_fun(host["framp"].copy(), 4), host["framp_to8_shift4"])
    with pytest.raises(RuntimeError, match="right shift"):
        ps.convert_to_8bit_fun(host["ramp"].copy(), 9)
    got = ps.normalize_flat(host["flat_raw"])
    assert got.dtype == np.float32 and np.array_equal(got, host["flat_norm"])


@pytest.mark.parametrize("name", CASES)
def test_plan_bookkeeping_equals_the_reference(ps, name):
    z, kw = load_case(name)
    img = z["img"]
    prm = ps.make_params(img.dtype, flat="flat" in z, **kw)
    info = ps.derive(img.shape, img.dtype, prm)
    out = z["out"]
    assert (info.out_ny, info.out_nx) == out.shape
    assert {0: np.uint8, 1: np.uint16, 2: np.float32}[info.out_dtype] == out.dtype
    if "log64" in z:
        assert (info.ny, info.nx) == z["log64"].shape
        assert info.base_pad == int(z["base_pad"])
        assert (info.padded_ny, info.padded_nx) == tuple(z["padded"])
        assert info.levels == int(z["levels"])
        shapes = [(info.coef_ny[i], info.coef_nx[i]) for i in range(info.levels)]
        assert shapes == [tuple(s) for s in z["coef_shapes"]]
        bp, py, px, padded, lev, cs = U.geometry(z["log64"].shape, kw["sigma"], kw.get("level", 0))
        assert (bp, padded, lev, cs) == (info.base_pad, (info.padded_ny, info.padded_nx), info.levels, shapes)
        assert (py, px) == (info.pad_y, info.pad_x)
        assert info.scratch_bytes_per_tile > 0


def test_pipeline_shape_bookkeeping(ps):
    prm = ps.make_params(np.uint16, sigma=(250, 250), wavelet="db9", padding_mode="reflect", bidirectional=True)
    info = ps.derive((2048, 2048), np.uint16, prm)
    assert (info.base_pad, info.padded_ny, info.padded_nx, info.levels) == (294, 2636, 2636, 7)
    assert U.geometry((2048, 2048), (250, 250))[:5] == (294, 0, 0, (2636, 2636), 7)
    assert [info.coef_ny[i] for i in range(7)] == [1326, 671, 344, 180, 98, 57, 37]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden(name):
    z, kw = load_case(name)
    flat = z["flat"] if "flat" in z else None
    got, log = U.process_img(z["img"].copy(), flat=flat, dt=np.float32, **kw)
    want = z["out"]
    assert got.shape == want.shape and got.dtype == want.dtype
    e_ref = float(z["e_ref"]) if "e_ref" in z else 0.0
    if log is not None:
        assert np.abs(log.astype(np.float64) - z["log64"]).max() <= 4 * e_ref
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if want.dtype.kind in "ui":
        assert (d <= U.integer_allowance(want, e_ref)).all()
        assert (d != 0).mean() <= 0.01
    else:
        assert (d <= 5 * e_ref * (np.abs(want.astype(np.float64)) + 1) + 1e-6 * np.abs(want)).all()


def test_uniform_tile_is_zeros_of_the_final_shape():
    z, kw = load_case("u16_uniform")
    assert not z["out"].any() and z["out"].shape == (20, 15) and z["out"].dtype == np.uint8


def test_refusals_name_the_option(ps, host):
    ref = json.loads(str(host["refusals"]))
    assert ref["sigma_0_8"] == ["ValueError", "np_notch: sigma must be positive"] and ref["sigma_8_0"][0] == "ValueError"
    mk = ps.make_params
    for sigma in ((0, 8), (8, 0)):
        with pytest.raises(ValueError, match="sigma must be positive"):
            mk(np.uint16, sigma=sigma)
    # the reference itself refuses a flat field on an integer tile: the recorded fact behind the stated departure (float32 divide)
    assert ref["flat_on_u16"][0] == "UFuncTypeError" and "divide" in ref["flat_on_u16"][1]
    assert ref["shift_9"][0] == "RuntimeError"
    with pytest.raises(RuntimeError, match="bit_shift_to_right"):
        mk(np.uint16, convert_to_8bit=True, bit_shift_to_right=9)
    assert ref["padding_bogus"][0] == "RuntimeError"
    with pytest.raises(RuntimeError, match="padding_mode"):
        mk(np.uint16, sigma=(8, 8), padding_mode="bogus")
    assert ref["down_bogus"][0] == "RuntimeError"
    with pytest.raises(RuntimeError, match="down_sample_method"):
        mk(np.uint16, down_sample=(2, 2), down_sample_method="bogus")
    with pytest.raises(TypeError, match="convert_to_16bit and convert_to_8bit"):
        mk(np.uint16, convert_to_16bit=True, convert_to_8bit=True)
    for kw, word in ((dict(sigma=(8, 8), wavelet="coif15"), "wavelet"), (dict(sigma=(8, 8), padding_mode="constant"), "padding_mode"),
                     (dict(down_sample=(2, 2), down_sample_method="median"), "down_sample_method")):
        with pytest.raises(NotImplementedError, match=word):
            mk(np.uint16, **kw)
    with pytest.raises(TypeError, match="d_type"):
        mk(np.uint16, d_type="float64")
    tile = np.zeros((8, 8), np.uint16)
    for kw, word in ((dict(bleach_correction_frequency=0.01), "bleach_correction_frequency"), (dict(lightsheet=True), "lightsheet"),
                     (dict(exclude_dark_edges_set_them_to_zero=True), "exclude_dark_edges_set_them_to_zero"),
                     (dict(new_size=(4, 4)), "new_size"), (dict(threshold=3.0), "threshold")):
        with pytest.raises(NotImplementedError, match=word):
            ps.process_img(tile, **kw)
    with pytest.raises(NotImplementedError, match="enable_masking"):
        ps.filter_streaks(tile, sigma=(8, 8), enable_masking=True)
    with pytest.raises(NotImplementedError, match="dcimg"):
        ps.batch_filter("stack.dcimg", "out", sigma=(8, 8))
    with pytest.raises(TypeError):
        ps.batch_filter("in", "out", convert_to_16bit=True, convert_to_8bit=True)
    with pytest.raises(TypeError, match="img.dtype"):
        ps.process_img(np.zeros((8, 8), np.float64), sigma=(8, 8), wavelet="db9")


def test_c_abi_refuses_what_it_cannot_do(ps):
    from ipp_amd import capi
    import ctypes as C
    lib = capi.lib()
    info = capi.PystripeInfo()
    p = capi.PystripeParams(sigma1=0, sigma2=8, out_dtype=1)
    assert lib.mi_pystripe_derive(64, 64, 1, C.byref(p), C.byref(info)) == capi.MI_ERR_INVALID
    assert "sigma must be positive" in capi.last_error()
    p = capi.PystripeParams(convert_to_8bit=1, bit_shift=9, out_dtype=0)
    assert lib.mi_pystripe_derive(64, 64, 1, C.byref(p), C.byref(info)) == capi.MI_ERR_INVALID
    assert "right shift should be between 0 and 8" in capi.last_error()
    p = capi.PystripeParams(rotate=45, out_dtype=1)
    assert lib.mi_pystripe_derive(64, 64, 1, C.byref(p), C.byref(info)) == capi.MI_ERR_INVALID and "rotate" in capi.last_error()


def test_file_walk_rank_split_and_cli(ps, tmp_path):
    for rel in ("a/x_01.tif", "a/b/x_02.TIFF", "a/b/y.raw", "c/z.png", "c/notes.txt", "c/t.tif.bak"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    found = sorted(str(p.relative_to(tmp_path)) for p in ps.find_tiles(tmp_path))
    assert found == ["a/b/x_02.TIFF", "a/b/y.raw", "a/x_01.tif", "c/z.png"]
    files = list(range(11))
    parts = [ps.split_for_rank(files, r, 3) for r in range(3)]
    assert sorted(sum(parts, [])) == files and all(parts)
    a = ps._parse_args(["--input", "in", "--output", "out", "--sigma1", "128", "--sigma2", "256", "--level", "0", "--wavelet", "db9",
                        "--padding_mode", "reflect", "--bidirectional", "--dark", "100", "--rotate", "90", "--flip_upside_down",
                        "--down_sample", "2", "2", "--convert_to_8bit", "--bit_shift_to_right", "4", "--compression_level", "1"])
    assert (a.sigma1, a.sigma2, a.bidirectional, a.down_sample, a.convert_to_8bit, a.rotate) == (128, 256, True, [2, 2], True, 90)
    # .raw: 8-byte header (width, height), uint16 samples
    img = np.arange(12, dtype=np.uint16).reshape(3, 4)
    raw = tmp_path / "t.raw"
    raw.write_bytes(np.array([4, 3], "<u4").tobytes() + img.astype("<u2").tobytes())
    assert np.array_equal(ps.raw_imread(raw), img)
