"""GPU: the stripe filter with any orthogonal wavelet of up to 128 taps (ipp_amd.pystripe ``wavelet=``, mi_pystripe_plan_create_wavelet)
against the restatement of tests/wavelet_util.py.

Standards, the ones of tests/test_gpu_pystripe.py:
  * log domain: max |device - float64 restatement| <= 4 E_ref, E_ref = the float32 restatement's own distance from the float64 one for
    the same wavelet and shape;
  * integer results: every pixel within 1 + ceil(5 E_ref (v + 1)) counts of the float32 restatement, at most 1 % of the pixels differ;
  * float results: |device - restatement| <= 5 E_ref (|v| + 1).
Every measured figure is printed before it is asserted; PYSTRIPE_REPORT=<file> appends them to a file.

The 90- and 128-tap wavelets are ``wavelet_util.lattice_filter``: orthonormal to rounding, of coif15's length (no coiflet table exists on
these machines).  Every call here but the one that names "db9" raises NotImplementedError on a build without the feature.
"""
import functools
import os

import numpy as np
import pytest

from oracle import destripe_oracle as O
from tests import bleach_util as B
from tests import pystripe_util as U
from tests import wavelet_util as W

pytestmark = pytest.mark.gpu


def report(line):
    print(line)
    path = os.environ.get("PYSTRIPE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


@functools.lru_cache(maxsize=None)
def lattice(taps, seed=1):
    h = W.lattice_filter(taps, seed)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def tile(shape, dtype, seed=7, stripes="rows"):
    img = U.synthetic_tile(shape, seed, np.dtype(dtype), stripes)
    img.setflags(write=False)
    return img


def check_against(name, got, want, e_ref):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if want.dtype.kind in "ui":
        share = float((d != 0).mean())
        report(f"{name}: integer result, {100 * share:.3f} % of pixels differ from the restatement, max {d.max():g} counts (E_ref {e_ref:.3g})")
        assert (d <= U.integer_allowance(want, e_ref)).all()
        assert share <= 0.01
    else:
        tol = 5 * e_ref * (np.abs(want.astype(np.float64)) + 1)
        report(f"{name}: float result, max |d| {d.max():.3g}, max d / allowance {(d / np.maximum(tol, 1e-30)).max():.3g}")
        assert (d <= tol).all()


def check_case(ps, dev, name, img, wavelet, rec_lo, bleach_kw=None, tail=None, **kw):
    """log domain and final result of one tile against the restatement with ``rec_lo``; returns the device's result.  ``kw``: the
    filter's options, ``bleach_kw``: the bleach keywords of process_img, ``tail``: what process_img does behind the filter."""
    tail = dict(tail or {})
    bleach = None
    if bleach_kw:
        bleach = dict(frequency=bleach_kw["bleach_correction_frequency"], clip_min=bleach_kw["bleach_correction_clip_min"],
                      clip_med=bleach_kw["bleach_correction_clip_med"], clip_max=bleach_kw["bleach_correction_clip_max"], max_method=False)
    r32, l64, e_ref = W.reference(img, rec_lo, bleach=bleach, **kw, **tail)
    extra = dict(bleach_kw or {})
    log = ps.filter_streaks(img.copy(), wavelet=wavelet, device=dev, log_output=True, **kw, **extra)
    assert log.dtype == np.float32 and log.shape == l64.shape
    err = float(np.abs(log.astype(np.float64) - l64).max())
    report(f"{name}: log domain, device vs float64 restatement {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f} (allowed 4)")
    assert err <= 4 * e_ref
    got = ps.process_img(img.copy(), wavelet=wavelet, device=dev, **kw, **extra, **tail)
    check_against(name, got, r32, e_ref)
    return got


def plan_info(ps, dev, img, wavelet, **kw):
    plan = ps.Plan(dev, img.shape, img.dtype, ps.make_params(img.dtype, wavelet=wavelet, **kw))
    try:
        return plan.info
    finally:
        plan.close()


HAAR = dict(sigma=(3, 3), padding_mode="reflect", bidirectional=True)


@pytest.mark.parametrize("past", [0, 1, 2])
def test_haar_down_to_lines_of_one_sample(ps, dev, past):
    img = tile((33, 70), "uint16")
    auto = W.geometry(img.shape, HAAR["sigma"], 2)[4]
    level = 0 if past == 0 else auto + past
    info = plan_info(ps, dev, img, "haar", level=level, **HAAR)
    assert info.levels == auto + past
    shortest = min(min(info.coef_ny[i], info.coef_nx[i]) for i in range(info.levels))
    report(f"haar, level {info.levels} (automatic {auto}): the shortest coefficient line has {shortest} samples")
    assert shortest == (2, 1, 1)[past] and (past < 2 or info.coef_nx[info.levels - 1] <= 2)
    check_case(ps, dev, f"haar level {info.levels}", img, "haar", O.db_filters(1)[2], level=level, **HAAR)


def test_db4_two_passes(ps, dev):
    img = tile((97, 130), "uint8")
    check_case(ps, dev, "db4 (97, 130) uint8", img, "db4", O.db_filters(4)[2], sigma=(6, 14), padding_mode="wrap", bidirectional=True)


def test_db19_one_direction_float(ps, dev):
    img = tile((129, 200), "float32")
    check_case(ps, dev, "db19 (129, 200) float32", img, "db19", O.db_filters(19)[2], sigma=(10, 10), padding_mode="symmetric", bidirectional=False)


BIG = dict(sigma=(16, 16), padding_mode="reflect", bidirectional=True)


def test_ninety_taps(ps, dev):
    img = tile((330, 421), "uint16")
    assert plan_info(ps, dev, img, lattice(90), **BIG).levels >= 2
    check_case(ps, dev, "90 taps (330, 421) uint16", img, lattice(90), lattice(90), **BIG)


def test_ninety_taps_with_bleach_correction(ps, dev):
    """the last synthesis level stores the log image, the bleach correction feeds the tail"""
    img = tile((330, 421), "uint16")
    bleach = dict(bleach_correction_frequency=1 / 64, **B.clips_for(img))
    check_case(ps, dev, "90 taps + bleach (330, 421) uint16", img, lattice(90), lattice(90), bleach_kw=bleach, **BIG)


def test_ninety_taps_on_a_tile_too_small_for_a_level(ps, dev):
    img = tile((40, 50), "uint16")
    assert plan_info(ps, dev, img, lattice(90), **BIG).levels == 0
    got = ps.process_img(img.copy(), wavelet=lattice(90), device=dev, **BIG)
    assert got.dtype == img.dtype and np.array_equal(got, img)
    # the log image is log1p of the tile: log1pf is within 2 ulp, the float64 figure rounds by half of one more
    log = ps.filter_streaks(img.copy(), wavelet=lattice(90), device=dev, log_output=True, **BIG)
    err = float(np.abs(log.astype(np.float64) - np.log1p(img.astype(np.float64))).max())
    report(f"90 taps (40, 50), no level: log image vs log1p {err:.3g} (one float32 spacing at log1p(65535): {np.spacing(np.float32(11.09)):.3g})")
    assert err <= 2.5 * np.spacing(np.float32(np.log1p(65535.0)))


@pytest.mark.parametrize("level", [1, 2])
def test_ninety_taps_explicit_level_reflects_more_than_once(ps, dev, level):
    img = tile((40, 50), "uint16")
    info = plan_info(ps, dev, img, lattice(90), level=level, **BIG)
    assert info.levels == level and info.padded_ny < 89 and info.coef_ny[0] > info.padded_ny      # (n + 89) / 2 > n: the level grows
    check_case(ps, dev, f"90 taps (40, 50) level {level}", img, lattice(90), lattice(90), level=level, **BIG)


def test_128_taps(ps, dev):
    img = tile((150, 150), "float32")
    check_case(ps, dev, "128 taps (150, 150) float32 level 1", img, lattice(128), lattice(128), sigma=(8, 8), level=1, padding_mode="reflect",
               bidirectional=True)


def test_db9_by_value_and_by_name(ps, dev):
    """the 18 db9 coefficients as an array run the kernels for any length, the name runs the db9 kernels: each within the standard"""
    img = tile((260, 131), "uint8")
    kw = dict(sigma=(12, 30), padding_mode="wrap", bidirectional=True)
    db9 = O.db_filters(9)[2]
    by_value = check_case(ps, dev, "db9 as 18 coefficients (260, 131) uint8", img, db9, db9, **kw)
    by_name = check_case(ps, dev, "db9 by name (260, 131) uint8", img, "db9", db9, **kw)
    report(f"db9 by value vs by name: {100 * float((by_value != by_name).mean()):.3f} % of pixels differ")
    # and the restatement for any length agrees with the db9 restatement of tests/pystripe_util.py
    l_any = W.filter_streaks_log(img, db9, dt=np.float64, **kw)
    l_db9 = U.filter_streaks_log(img, dt=np.float64, **kw)
    assert np.abs(l_any - l_db9).max() <= 1e-12


@pytest.mark.parametrize("wavelet,kw", [("db4", dict(sigma=(6, 14))), ("lattice90", dict(sigma=(8, 8), level=1))])
def test_batch_equals_tiles_one_by_one(ps, dev, wavelet, kw):
    import torch
    w = lattice(90) if wavelet == "lattice90" else wavelet
    tiles = np.stack([U.synthetic_tile((97, 130), 400 + i, np.uint16, "rows" if i % 2 else "cols") for i in range(5)])
    outs = {}
    for mb in (1, 5):
        for log in (False, True):
            plan = ps.Plan(dev, tiles.shape[1:], np.uint16, ps.make_params(np.uint16, wavelet=w, padding_mode="reflect", bidirectional=True, dark=20,
                                                                             rotate=90, log_output=log, max_batch=mb, **kw))
            outs[mb, log] = plan.run(torch.from_numpy(tiles).to(dev)).cpu().numpy()
            plan.close()
    for log in (False, True):
        assert outs[1, log].tobytes() == outs[5, log].tobytes()
    assert outs[1, False].any() and not np.array_equal(outs[1, False][0], outs[1, False][1])


def test_live_plans_of_2_and_90_taps(ps, dev):
    """the column passes ask for 16 KB of LDS at 2 taps and 61 KB at 90 (above the 48 KB at which a kernel's limit has to be raised): two plans
    alive together, run in turn, keep the results they gave alone"""
    import torch
    x = torch.from_numpy(tile((330, 421), "uint16")[None].copy()).to(dev)
    first = {}
    for name, w in (("haar", "haar"), ("90", lattice(90))):
        plan = ps.Plan(dev, (330, 421), np.uint16, ps.make_params(np.uint16, wavelet=w, max_batch=1, **BIG))
        first[name] = plan.run(x).clone()
        torch.cuda.synchronize(dev)
        plan.close()
    assert not torch.equal(first["haar"], first["90"])
    plans = {name: ps.Plan(dev, (330, 421), np.uint16, ps.make_params(np.uint16, wavelet=w, max_batch=1, **BIG))
             for name, w in (("haar", "haar"), ("90", lattice(90)))}
    for name in ("haar", "90", "haar", "90", "90", "haar"):
        got = plans[name].run(x)
        torch.cuda.synchronize(dev)
        assert torch.equal(got, first[name]), name
    for plan in plans.values():
        plan.close()


def test_process_img_tail_options(ps, dev):
    img = tile((97, 130), "uint16")
    check_case(ps, dev, "db4 process_img tail", img, "db4", O.db_filters(4)[2], sigma=(6, 14), padding_mode="reflect", bidirectional=True,
               tail=dict(flip_upside_down=True, rotate=90, convert_to_8bit=True, bit_shift_to_right=3, dark=20))


def test_batch_filter_with_coefficients(ps, dev, tmp_path):
    from PIL import Image
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rec_lo = np.array(lattice(12, 9))
    tiles = {f"t_{i}.tif": U.synthetic_tile((64, 80), 500 + i, np.uint16, "rows" if i else "cols") for i in range(3)}
    for name, img in tiles.items():
        Image.fromarray(img).save(src / name, format="TIFF")
    kw = dict(sigma=(8, 8), padding_mode="reflect", bidirectional=True)
    stats = {}
    assert ps.batch_filter(src, dst, wavelet=rec_lo, device=dev, stats=stats, **kw) == 0
    assert stats["written"] == 3
    for name, img in tiles.items():
        with Image.open(dst / name) as im:
            got = np.array(im)
        r32, _, e_ref = W.reference(img, rec_lo, **kw)
        check_against("batch_filter " + name, got, r32, e_ref)


def row_gain_spread(img):
    """spread of the per-row gain estimate: std of log(mean along the row) after removing its smooth part"""
    prof = np.log(img.astype(np.float64).mean(axis=1) + 1)
    k = 15
    smooth = np.convolve(np.pad(prof, k, mode="edge"), np.ones(2 * k + 1) / (2 * k + 1), mode="valid")
    return float((prof - smooth).std())


@pytest.mark.parametrize("name", ["haar", "lattice90"])
def test_structure_row_stripes(ps, dev, name):
    img = tile((330, 421), "uint16")
    got = ps.process_img(img.copy(), wavelet="haar" if name == "haar" else lattice(90), device=dev, **BIG)
    before, after = row_gain_spread(img), row_gain_spread(got)
    report(f"row stripes, {name}: gain spread before {before:.4f}, after {after:.4f}")
    assert after <= before
