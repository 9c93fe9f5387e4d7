"""CPU: the per-tile automatic bleach clips and the median down-sampling of the pystripe stage -- the restatement of
tests/autoclips_util.py (multi-Otsu of tests/thresholds_util.py composed with tests/bleach_util.py) against the goldens of the
reference's own code (tests/golden/autoclips, made by tests/golden/make_autoclips_golden.py), the stability of the float inputs the
GPU tests use, and the Python layer and mi_pystripe_derive with clips left None."""
import ctypes as C

import numpy as np
import pytest

from tests import autoclips_util as A
from tests import pystripe_util as U
from tests import thresholds_util as T
from tests.conftest import ROOT

CASES = A.golden_cases(ROOT)
AUTO = dict(bleach_correction_clip_min=None, bleach_correction_clip_med=None, bleach_correction_clip_max=None)


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


def test_goldens_are_present():
    assert len(CASES) >= 12
    kinds = set()
    for name in CASES:
        z, kw = A.load_case(ROOT, name)
        assert z["img"].shape[0] <= 96 and z["img"].shape[1] <= 128 and any(kw[k] is None for k in A.CLIP_KEYS)
        assert z["triple"].dtype == np.float32 and 0 <= z["triple"][0] < z["triple"][1] < z["triple"][2]
        kinds.add((z["img"].dtype.name, tuple(kw["sigma"]) > (0, 0), bool(kw["bleach_correction_max_method"]), sum(kw[k] is None for k in A.CLIP_KEYS)))
    assert {k[0] for k in kinds} == {"uint8", "uint16", "float32"} and {k[1] for k in kinds} == {False, True}
    assert {k[2] for k in kinds} == {False, True} and {k[3] for k in kinds} == {1, 3}
    z, kw = A.load_case(ROOT, "u16_filter_rows")
    assert z["img"].shape == (40, 72) and kw["sigma"] == (8, 8) and kw["padding_mode"] == "reflect"


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden(name):
    z, kw = A.load_case(ROOT, name)
    assert np.array_equal(A.triple(z["img"], **kw), z["triple"])       # the thresholds, bit for bit
    got, log = A.process_img(z["img"].copy(), dt=np.float32, **kw)
    want, e_ref = z["out"], float(z["e_ref"])
    assert got.shape == want.shape and got.dtype == want.dtype and log.dtype == np.float32
    if tuple(kw["sigma"]) == (0, 0):
        assert np.array_equal(log, z["log32"]) and np.array_equal(got, want)     # bit for bit
        return
    assert np.abs(log.astype(np.float64) - z["log64"]).max() <= 4 * e_ref
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if want.dtype.kind in "ui":
        assert (d <= U.integer_allowance(want, e_ref)).all() and (d != 0).mean() <= 0.01
    else:
        assert (d <= 5 * e_ref * (np.abs(want.astype(np.float64)) + 1)).all()


def test_padded_samples_would_change_the_histogram():
    """40 x 72 at sigma (8, 8) with reflect padding: the histogram of the padded log image is another one, so an estimate taken
    behind the padding would show."""
    z, kw = A.load_case(ROOT, "u16_filter_rows")
    log = A.log_image(z["img"])
    pad = U.calculate_pad_size(log.shape, 8)
    assert pad > 0
    padded = np.pad(log, pad, mode="reflect")
    assert not np.array_equal(np.histogram(padded.reshape(-1), 256)[0], np.histogram(log.reshape(-1), 256)[0])


def test_float_inputs_are_stable_under_one_ulp():
    """Every float log image the GPU tests estimate from keeps its threshold indices when each sample moves by one float32 ulp."""
    for name in CASES:
        z, kw = A.load_case(ROOT, name)
        if z["img"].dtype == np.float32:
            assert A.indices_are_stable(A.log_image(z["img"])), name
    shape = (41, 75)
    assert A.indices_are_stable(A.log_image(A.float_tile(shape, 22)))
    assert A.indices_are_stable(A.log_image(T.four_mode_image(shape, 22), flat=A.flat_field(shape)))
    for method in ("mean", "median"):
        assert A.indices_are_stable(A.log_image(T.four_mode_image(shape, 22), down_sample=(2, 2), down_sample_method=method))
    assert A.indices_are_stable(A.log_image(A.float_tile((33, 47), 41)))


def test_median_restatement_is_block_reduce_with_numpy_median():
    """``reduced`` against the definition written out block by block: zero padding up to a block multiple, numpy.median of each."""
    for shape in ((37, 50), (64, 64)):
        for dtype in (np.uint8, np.uint16, np.float32):
            img = A.float_tile(shape, 50) if dtype == np.float32 else T.four_mode_image(shape, 50, dtype)
            for flat in (None, A.flat_field(shape)):
                src = img if flat is None else img.astype(np.float32) / flat
                for by, bx in ((2, 2), (3, 2), (1, 5), (8, 8)):
                    my, mx = -(-shape[0] // by), -(-shape[1] // bx)
                    padded = np.zeros((my * by, mx * bx), src.dtype)
                    padded[:shape[0], :shape[1]] = src
                    want = np.array([[np.median(padded[y * by:(y + 1) * by, x * bx:(x + 1) * bx]) for x in range(mx)] for y in range(my)])
                    got = A.reduced(img, flat, (by, bx), "median")
                    assert got.shape == (my, mx) and np.array_equal(got, want)
                    # the mean of the two middle values taken in float64 and rounded once is what numpy returns for float32 data
                    flat_blocks = np.sort(padded.reshape(my, by, mx, bx).transpose(0, 2, 1, 3).reshape(my, mx, by * bx).astype(np.float64), axis=-1)
                    n = by * bx
                    mid = (flat_blocks[..., (n - 1) // 2] + flat_blocks[..., n // 2]) * 0.5
                    assert np.array_equal(mid.astype(np.float32), got.astype(np.float32))


def test_make_params_with_clips_left_none(ps):
    """With ``extended=True`` a clip that is None is NaN in the struct (the plan estimates it) and ``bleach_auto`` reports the bits;
    without it every entry point refuses as it did, and the struct has no new field."""
    import math
    from ipp_amd import capi
    mk = lambda **k: ps.make_params(np.uint16, extended=True, **k)  # noqa: E731
    p = mk(bleach_correction_frequency=0.01, **AUTO)
    assert p.bleach_auto == 7 and all(math.isnan(v) for v in (p.bleach_clip_min, p.bleach_clip_med, p.bleach_clip_max))
    p = mk(bleach_correction_frequency=0.01, bleach_correction_clip_min=3.0, bleach_correction_clip_max=9.0)
    assert p.bleach_auto == capi.PS_AUTO_MED and (p.bleach_clip_min, p.bleach_clip_max) == (3.0, 9.0) and math.isnan(p.bleach_clip_med)
    p = mk(bleach_correction_frequency=0.01, bleach_correction_clip_med=7.0)
    assert p.bleach_auto == capi.PS_AUTO_MIN | capi.PS_AUTO_MAX and p.bleach_clip_med == 7.0
    assert mk(bleach_correction_frequency=0.01, bleach_correction_clip_min=6.0, bleach_correction_clip_med=7.0,
              bleach_correction_clip_max=8.0).bleach_auto == 0
    assert mk().bleach_auto == 0 and ps.make_params(np.uint16).bleach_auto == 0
    assert [f[0] for f in capi.PystripeParams._fields_][-1] == "bleach_max_method"      # the ABI of the struct is as it was
    assert mk(down_sample=(2, 2), down_sample_method="MEDIAN").down_method == capi.PS_DOWN["median"] == 3
    with pytest.raises(NotImplementedError, match="down_sample"):
        mk(down_sample=(9, 8), down_sample_method="median")
    # the defaults refuse what they refused, naming the option and the way in
    tile = np.zeros((8, 8), np.uint16)
    with pytest.raises(NotImplementedError, match="down_sample_method.*extended=True"):
        ps.make_params(np.uint16, down_sample=(2, 2), down_sample_method="median")
    for call in (lambda **k: ps.process_img(tile, **k), lambda **k: ps.filter_streaks(tile, sigma=(0, 0), **k),
                 lambda **k: ps.batch_filter("in", "out", **k), lambda **k: ps.make_params(np.uint16, **k)):
        with pytest.raises(NotImplementedError, match="bleach_correction_frequency.*extended=True"):
            call(bleach_correction_frequency=0.01)
    # the checks between given values still run before the device is touched
    for kw in (dict(bleach_correction_clip_min=9.0, bleach_correction_clip_max=3.0), dict(bleach_correction_clip_min=-1.0),
               dict(bleach_correction_clip_med=7.0, bleach_correction_clip_max=7.0), dict(bleach_correction_clip_max=9)):
        with pytest.raises(AssertionError, match="bleach_correction"):
            ps.process_img(tile, bleach_correction_frequency=0.01, extended=True, **kw)
        with pytest.raises(AssertionError, match="bleach_correction"):
            ps.batch_filter("in", "out", bleach_correction_frequency=0.01, extended=True, **kw)
    with pytest.raises(ValueError, match="padlen, which is 6"):
        ps.process_img(np.ones((9, 6), np.uint16), bleach_correction_frequency=0.01, extended=True)
    with pytest.raises(ValueError, match="0 < Wn < 1"):
        ps.filter_streaks(tile, sigma=(0, 0), bleach_correction_frequency=1.5, extended=True)


def test_derive_with_automatic_clips(ps):
    from ipp_amd import capi
    nan = float("nan")
    info = capi.PystripeInfo()
    derive = lambda p, shape=(37, 53): capi.lib().mi_pystripe_derive(shape[0], shape[1], 1, C.byref(p), C.byref(info))  # noqa: E731
    base = dict(out_dtype=1, bleach_frequency=1 / 32)
    auto = capi.PystripeParams(bleach_clip_min=nan, bleach_clip_med=nan, bleach_clip_max=nan, **base)
    assert auto.bleach_auto == 7 and derive(auto) == capi.MI_OK
    assert derive(capi.PystripeParams(bleach_clip_min=3.0, bleach_clip_med=nan, bleach_clip_max=9.0, **base)) == capi.MI_OK
    for fields, word in ((dict(bleach_clip_min=9.0, bleach_clip_med=nan, bleach_clip_max=3.0), "bleach_clip_max"),
                         (dict(bleach_clip_min=-1.0, bleach_clip_med=nan, bleach_clip_max=nan), "bleach_clip_min"),
                         (dict(bleach_clip_min=nan, bleach_clip_med=7.0, bleach_clip_max=7.0), "bleach_clip_max")):
        assert derive(capi.PystripeParams(**dict(base, **fields))) == capi.MI_ERR_INVALID
        assert word in capi.last_error()
    # without a frequency the three values are not looked at
    off = capi.PystripeParams(out_dtype=1, bleach_clip_min=nan, bleach_clip_med=nan, bleach_clip_max=nan)
    assert off.bleach_auto == 0 and derive(off) == capi.MI_OK
    # the median: a float tile; blocks of more than 64 samples are unsupported
    assert derive(capi.PystripeParams(out_dtype=1, down_y=8, down_x=8, down_method=3)) == capi.MI_OK and info.integer_kind == 0
    assert (info.ny, info.nx) == (5, 7)
    assert derive(capi.PystripeParams(out_dtype=1, down_y=9, down_x=8, down_method=3)) == capi.MI_ERR_UNSUPPORTED and "median" in capi.last_error()
    assert derive(capi.PystripeParams(out_dtype=1, down_y=2, down_x=2, down_method=4)) == capi.MI_ERR_INVALID


def test_threshold_and_new_size_from_the_values(ps):
    assert ps._single_band((8, 16), None) == (8, 16) and ps._single_band((8, 16), 5.0) == (8, 16)
    assert ps._single_band((8, 16), -1.0) == (8, 8) and ps._single_band((8, 16), 0) == (8, 8) and ps._single_band((8, 8), -1.0) == (8, 8)
    tile = np.zeros((37, 41), np.uint16)
    with pytest.raises(NotImplementedError, match="threshold"):
        ps.process_img(tile, sigma=(0, 16), threshold=-1.0, wavelet="db9", extended=True)
    with pytest.raises(NotImplementedError, match="new_size"):
        ps.process_img(tile, new_size=(53, 30), extended=True)
    with pytest.raises(ValueError, match="new_size"):
        ps.process_img(tile, new_size=(53, 0), extended=True)
    for kw, word in ((dict(new_size=(20, 20)), "new_size.*extended=True"), (dict(threshold=5.0), "threshold.*extended=True")):
        with pytest.raises(NotImplementedError, match=word):
            ps.process_img(tile, **kw)
