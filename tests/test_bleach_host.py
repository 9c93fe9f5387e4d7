"""CPU: the bleach correction of the pystripe stage -- the restatement of tests/bleach_util.py against the goldens of the reference's
own code (tests/golden/bleach, made by tests/golden/make_bleach_golden.py), the explicit recurrence against scipy, the refusals of
the Python layer and of mi_pystripe_derive, and the command line."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from tests import bleach_util as B
from tests import pystripe_util as U
from tests.conftest import ROOT

CASES = B.golden_cases(ROOT)
CLIPS = dict(bleach_correction_clip_min=6.0, bleach_correction_clip_med=7.0, bleach_correction_clip_max=8.0)


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


@pytest.fixture(scope="module")
def refusals():
    return json.loads(str(np.load(os.path.join(B.golden_dir(ROOT), "refusals.npz"))["refusals"]))


def test_goldens_are_present():
    assert len(CASES) >= 14
    shapes = {name: B.load_case(ROOT, name)[0]["img"].shape for name in CASES}
    assert shapes["u16_min_row"] == (9, 7) and shapes["u16_min_column_max"] == (7, 11)
    for name in CASES:
        z, kw = B.load_case(ROOT, name)
        assert float(z["frac_ref"]) < 0.005
        assert float(z["e_ref"]) >= B.e_ref_floor(z["log64"]) and float(z["e_ref"]) >= float(z["e_ref_raw"])
    z, kw = B.load_case(ROOT, "u16_zero_block")
    assert (z["img"][10:25, 20:45] == 0).all() and not z["img"][30].any()
    assert B.load_case(ROOT, "u16_clip_min_zero")[1]["bleach_correction_clip_min"] == 0.0


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden(name):
    z, kw = B.load_case(ROOT, name)
    got, log = B.process_img(z["img"].copy(), dt=np.float32, **kw)
    want, e_ref = z["out"], float(z["e_ref"])
    assert got.shape == want.shape and got.dtype == want.dtype and log.dtype == np.float32
    if tuple(kw["sigma"]) == (0, 0):
        assert np.array_equal(log, z["log32"]) and np.array_equal(got, want)     # bit for bit
        return
    assert np.abs(log.astype(np.float64) - z["log64"]).max() <= 4 * e_ref
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (d <= U.integer_allowance(want, e_ref)).all() and (d != 0).mean() <= 0.01


@pytest.mark.parametrize("name", CASES)
def test_restatement_with_the_explicit_recurrence(name):
    """The whole step with the plain recurrence (closed-form coefficients) in place of sosfiltfilt: within the standard of the log
    domain, against the float64 restatement built on scipy."""
    z, kw = B.load_case(ROOT, name)
    _, log = B.process_img(z["img"].copy(), dt=np.float64, row_filter=B.lowpass_explicit, **kw)
    assert np.abs(log - z["log64"]).max() <= 1e-9


@pytest.mark.parametrize("frequency", [0.5, 1 / 4, 1 / 32, 1 / 64, 1 / 2000, 0.93])
def test_explicit_recurrence_equals_sosfiltfilt(frequency):
    rng = np.random.default_rng(3)
    for shape in ((5, 40), (3, 7), (2, 301)):
        x = 6 + 2 * rng.random(shape)
        want = B.lowpass(x, frequency)
        # float64 roundings (2.2e-16) carried through a memory of about 2 / (pi f) <= 1300 samples, twice: well below 1e-12; with scipy's
        # own coefficients only the initial state (scipy solves for it) and the order of the sums can differ
        for from_scipy in (True, False):
            d = np.abs(B.lowpass_explicit(x, frequency, from_scipy) - want).max() / np.abs(want).max()
            print(f"f = {frequency:.4g}, {shape}, scipy's coefficients {from_scipy}: relative difference {d:.3g}")
            assert d <= 1e-12
    b, a = B.coefficients(frequency)
    bs, as_ = B.coefficients(frequency, from_scipy=True)
    assert abs(b - bs) <= 4e-16 and abs(a - as_) <= 4e-16
    with pytest.raises(ValueError, match="padlen"):
        B.lowpass_explicit(np.ones((2, 6)), frequency)


def test_recurrence_keeps_a_constant():
    """A constant row comes back unchanged at any cutoff: the initial states are the steady state of the first sample."""
    x = np.full(33, 7.25)
    for frequency in (0.5, 1 / 32, 1 / 2000):
        assert np.abs(B.lowpass_explicit(x, frequency) - x).max() <= 1e-12


def test_refusals_as_in_the_reference(ps, refusals):
    tile = U.synthetic_tile((37, 53), 51, np.uint16)
    run = lambda im=tile, **k: ps.process_img(im, **dict(dict(bleach_correction_frequency=1 / 32, **CLIPS), **k))  # noqa: E731
    assert [refusals[k][0] for k in ("int_clip", "int_frequency", "med_not_above_min", "max_not_above_med", "negative_min")] == ["AssertionError"] * 5
    for kw in (dict(bleach_correction_clip_max=9), dict(bleach_correction_frequency=1), dict(bleach_correction_clip_med=6.0),
               dict(bleach_correction_clip_max=7.0), dict(bleach_correction_clip_min=-0.5), dict(bleach_correction_frequency=0.0),
               dict(bleach_correction_clip_min=6), dict(bleach_correction_clip_med=7)):
        with pytest.raises(AssertionError, match="bleach_correction"):
            run(**kw)
        with pytest.raises(AssertionError, match="bleach_correction"):
            ps.filter_streaks(tile, sigma=(0, 0), **dict(dict(bleach_correction_frequency=1 / 32, **CLIPS), **kw))
    assert refusals["frequency_one"] == ["ValueError", "Digital filter critical frequencies must be 0 < Wn < 1"]
    assert refusals["frequency_above_one"][0] == "ValueError"
    for f in (1.0, 1.5):
        with pytest.raises(ValueError, match="0 < Wn < 1"):
            run(bleach_correction_frequency=f)
        with pytest.raises(ValueError, match="0 < Wn < 1"):
            ps.batch_filter("in", "out", bleach_correction_frequency=f, **CLIPS)
    assert refusals["nx_6"][0] == "ValueError" and "padlen, which is 6" in refusals["nx_6"][1]
    assert refusals["ny_6_max_method"][0] == "ValueError" and refusals["nx_7"] == ["", ""] and refusals["ny_6_rows"] == ["", ""]
    with pytest.raises(ValueError, match="padlen, which is 6"):
        run(np.ones((9, 6), np.uint16))
    with pytest.raises(ValueError, match="padlen, which is 6"):
        run(np.ones((6, 9), np.uint16), bleach_correction_max_method=True)
    with pytest.raises(ValueError, match="padlen, which is 6"):
        run(np.ones((9, 12), np.uint16), down_sample=(1, 2))           # 6 samples after down_sample
    with pytest.raises(ValueError, match="padlen, which is 6"):
        ps.filter_streaks(np.ones((9, 6), np.uint16), sigma=(0, 0), bleach_correction_frequency=1 / 32, **CLIPS)
    # the asserts come first, as in the reference
    with pytest.raises(AssertionError):
        run(np.ones((9, 6), np.uint16), bleach_correction_clip_max=9)


def test_what_stays_refused(ps):
    """A frequency without all three clips (the automatic ones need threshold_multiotsu) and a threshold stay NotImplementedError by
    name, before anything else."""
    tile = np.zeros((8, 8), np.uint16)
    for missing in B.BLEACH_KEYS[2:]:
        clips = {k: v for k, v in CLIPS.items() if k != missing}
        for call in (lambda **k: ps.process_img(tile, **k), lambda **k: ps.filter_streaks(tile, sigma=(0, 0), **k),
                     lambda **k: ps.batch_filter("in", "out", **k), lambda **k: ps.make_params(np.uint16, **k)):
            with pytest.raises(NotImplementedError, match="bleach_correction_frequency.*threshold_multiotsu"):
                call(bleach_correction_frequency=0.01, **clips)
    with pytest.raises(NotImplementedError, match="bleach_correction_frequency"):
        ps.process_img(tile, bleach_correction_frequency=0.01)
    with pytest.raises(NotImplementedError, match="bleach_correction_frequency"):
        ps.process_img(tile, bleach_correction_frequency=1, bleach_correction_clip_min=5)     # before the asserts
    with pytest.raises(NotImplementedError, match="threshold"):
        ps.process_img(tile, threshold=3.0, bleach_correction_frequency=0.01, **CLIPS)
    with pytest.raises(NotImplementedError, match="threshold"):
        ps.process_img(tile, threshold=3.0)
    # no frequency: sigma (0, 0) still returns the input itself
    assert ps.filter_streaks(tile, sigma=(0, 0)) is tile
    assert ps.filter_streaks(tile, sigma=(0, 0), **CLIPS) is tile


def test_defaults_of_the_entry_points(ps):
    import inspect
    for fun, max_method in ((ps.filter_streaks, False), (ps.process_img, False), (ps.batch_filter, True)):
        sig = inspect.signature(fun).parameters
        assert sig["bleach_correction_max_method"].default is max_method
        assert all(sig[k].default is None for k in B.BLEACH_KEYS if k != "bleach_correction_max_method")


def test_make_params_and_derive(ps):
    from ipp_amd import capi
    off = ps.make_params(np.uint16)
    assert off.bleach_frequency == 0 and off.bleach_max_method == 0
    base = ps.derive((97, 128), np.uint16, off)
    p = ps.make_params(np.uint16, bleach_correction_frequency=np.float32(1 / 32), bleach_correction_max_method=True, **CLIPS)
    assert (p.bleach_frequency, p.bleach_clip_min, p.bleach_clip_med, p.bleach_clip_max, p.bleach_max_method) == (1 / 32, 6.0, 7.0, 8.0, 1)
    # the new fields are the last ones: a block zero-initialised by an older caller keeps its meaning
    names = [f[0] for f in capi.PystripeParams._fields_]
    assert names[-5:] == ["bleach_frequency", "bleach_clip_min", "bleach_clip_med", "bleach_clip_max", "bleach_max_method"]
    assert names[names.index("keep_uniform") + 1] == "bleach_frequency"
    # scratch: F and the row maxima (rows), the keys and vectors (max method), the log image with a stripe filter
    rows = ps.derive((97, 128), np.uint16, ps.make_params(np.uint16, bleach_correction_frequency=1 / 32, **CLIPS))
    mm = ps.derive((97, 128), np.uint16, p)
    assert base.scratch_bytes_per_tile == 0
    assert rows.scratch_bytes_per_tile >= 4 * (97 * 128 + 97 + 1) and rows.scratch_bytes_per_tile < 4 * (97 * 128 + 97 + 16)
    assert 4 * (2 * (97 + 128) + 1) <= mm.scratch_bytes_per_tile < 4 * (2 * (97 + 128) + 16)
    kw = dict(sigma=(16, 16), wavelet="db9", padding_mode="reflect", bidirectional=True)
    f0 = ps.derive((97, 128), np.uint16, ps.make_params(np.uint16, **kw))
    f1 = ps.derive((97, 128), np.uint16, ps.make_params(np.uint16, bleach_correction_frequency=1 / 32, **CLIPS, **kw))
    assert f1.scratch_bytes_per_tile - f0.scratch_bytes_per_tile >= 4 * (2 * 97 * 128 + 97 + 1)
    assert (f1.padded_ny, f1.padded_nx, f1.levels) == (f0.padded_ny, f0.padded_nx, f0.levels)
    # the long-row route: the float64 row scratch
    assert capi.PS_BLEACH_LDS_ROW == B.LDS_ROW == 20436
    short = ps.derive((3, B.LDS_ROW), np.float32, ps.make_params(np.float32, bleach_correction_frequency=1 / 32, **CLIPS))
    long_ = ps.derive((3, B.LDS_ROW + 1), np.float32, ps.make_params(np.float32, bleach_correction_frequency=1 / 32, **CLIPS))
    assert (short.bleach_long_rows, long_.bleach_long_rows, rows.bleach_long_rows, base.bleach_long_rows) == (0, 1, 0, 0)
    assert long_.scratch_bytes_per_tile - short.scratch_bytes_per_tile >= 8 * 3 * (B.LDS_ROW + 13)
    # log_output: allowed with the bleach correction alone, refused when nothing is on
    lo = ps.derive((37, 53), np.uint16, ps.make_params(np.uint16, log_output=True, bleach_correction_frequency=1 / 32, **CLIPS))
    assert (lo.out_ny, lo.out_nx, lo.out_dtype) == (37, 53, capi.PS_F32)
    info = capi.PystripeInfo()
    assert capi.lib().mi_pystripe_derive(37, 53, 1, C.byref(ps.make_params(np.uint16, log_output=True)), C.byref(info)) == capi.MI_ERR_INVALID
    assert "log_output" in capi.last_error()


@pytest.mark.parametrize("fields,shape,word", [
    (dict(bleach_frequency=1.0), (37, 53), "bleach_frequency"),
    (dict(bleach_frequency=-0.1), (37, 53), "bleach_frequency"),
    (dict(bleach_frequency=float("nan")), (37, 53), "bleach_frequency"),
    (dict(bleach_clip_min=-1.0), (37, 53), "bleach_clip_min"),
    (dict(bleach_clip_med=6.0), (37, 53), "bleach_clip_med"),
    (dict(bleach_clip_max=7.0), (37, 53), "bleach_clip_max"),
    (dict(), (9, 6), "nx = 6"),
    (dict(bleach_max_method=1), (6, 9), "ny = 6"),
    (dict(down_y=1, down_x=2), (9, 12), "nx = 6"),
])
def test_derive_refuses_invalid_fields(ps, fields, shape, word):
    from ipp_amd import capi
    good = dict(out_dtype=1, bleach_frequency=1 / 32, bleach_clip_min=6.0, bleach_clip_med=7.0, bleach_clip_max=8.0)
    info = capi.PystripeInfo()
    assert capi.lib().mi_pystripe_derive(37, 53, 1, C.byref(capi.PystripeParams(**good)), C.byref(info)) == capi.MI_OK
    assert capi.lib().mi_pystripe_derive(9, 7, 1, C.byref(capi.PystripeParams(**good)), C.byref(info)) == capi.MI_OK
    assert capi.lib().mi_pystripe_derive(7, 9, 1, C.byref(capi.PystripeParams(**dict(good, bleach_max_method=1))), C.byref(info)) == capi.MI_OK
    p = capi.PystripeParams(**dict(good, **fields))
    assert capi.lib().mi_pystripe_derive(shape[0], shape[1], 1, C.byref(p), C.byref(info)) == capi.MI_ERR_INVALID
    assert word in capi.last_error(), capi.last_error()


def test_command_line(ps):
    a = ps._parse_args(["--input", "in"])
    assert a.bleach_correction_frequency is None and a.bleach_correction_max_method is True
    assert (a.bleach_correction_clip_min, a.bleach_correction_clip_med, a.bleach_correction_clip_max) == (None, None, None)
    a = ps._parse_args(["--input", "in", "--bleach_correction_frequency", "0.0005", "--bleach_correction_clip_min", "5.5",
                        "--bleach_correction_clip_med", "6.5", "--bleach_correction_clip_max", "8", "--no-bleach_correction_max_method"])
    assert (a.bleach_correction_frequency, a.bleach_correction_clip_min, a.bleach_correction_clip_med, a.bleach_correction_clip_max,
            a.bleach_correction_max_method) == (0.0005, 5.5, 6.5, 8.0, False)
    assert isinstance(a.bleach_correction_clip_max, float)       # "8" arrives as a float: the asserts take it
    assert ps._parse_args(["--input", "in", "--bleach_correction_max_method"]).bleach_correction_max_method is True
    import io
    from contextlib import redirect_stdout
    text = io.StringIO()
    with pytest.raises(SystemExit), redirect_stdout(text):
        ps._parse_args(["--help"])
    assert " ".join(text.getvalue().split()).count("log1p units") == 3
    assert math.isclose(math.log1p(1), 0.6931471805599453)
