"""CPU: the yardstick of the slice estimates (tests/thresholds_util.py) checked against a plain loop and against float64, the host
arithmetic of ipp_amd.thresholds on code counts checked against numpy itself, and the refusals, errors and parser wiring that need
no device."""
import argparse

import numpy as np
import pytest

from tests import thresholds_util as tu

SHAPES = [(7, 9), (48, 80), (67, 131)]


def _loop_search(hist, classes):
    """the search as three plain loops over numpy float32 scalars, the sums in the stated order"""
    prob, P1, S1, nvalues = tu.moments(hist)
    assert nvalues > classes
    n, m = prob.size, classes - 1
    f = np.float32

    def H(i, j):
        p, s = f(P1[j + 1] - P1[i]), f(S1[j + 1] - S1[i])
        return f(f(s * s) / p) if p > 0 else f(0)

    best, arg = f(0), [0] * m

    def visit(t):
        nonlocal best, arg
        sigma = f(H(0, t[0]) + H(t[-1] + 1, n - 1))
        for k in range(m - 1):
            sigma = f(sigma + H(t[k] + 1, t[k + 1]))
        if sigma > best:
            best, arg = sigma, list(t)

    def walk(prefix, k):
        if k == m:
            visit(prefix)
            return
        for idx in range(prefix[-1] + 1 if prefix else 0, n - m + k):
            walk(prefix + [idx], k + 1)

    walk([], 0)
    return arg, best


@pytest.mark.parametrize("classes", [2, 3, 4])
@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_equals_plain_loops_on_24_bins(classes, seed):
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, 50, 24) * (rng.random(24) < 0.8)   # some empty bins, so H meets p == 0
    idx, sigma = tu.multiotsu_indices(hist, classes)
    want, want_sigma = _loop_search(hist, classes)
    assert idx.tolist() == want and sigma == want_sigma


def test_restatement_keeps_the_first_of_equal_optima():
    base = np.array([0, 9, 1, 0, 7, 0, 0, 3, 0, 0, 0, 5], np.int64)
    hist = np.concatenate([base, base[::-1]])     # mirror-symmetric: every split has a mirror image of equal variance in exact terms
    for classes in (2, 3, 4):
        idx, _ = tu.multiotsu_indices(hist, classes)
        want, _ = _loop_search(hist, classes)
        assert idx.tolist() == want


@pytest.mark.parametrize("shape", SHAPES)
def test_chosen_split_is_the_float64_optimum_within_rounding(shape):
    """the chosen sigma is within 1e-5 relative of the largest of the same sums taken in float64 (float32 rounding of four terms)"""
    hist, _ = np.histogram(np.log1p(tu.four_mode_image(shape), dtype=np.float32).reshape(-1), 256)
    _, P1, S1, _ = tu.moments(hist)
    idx, sigma = tu.multiotsu_indices(hist, 4)
    best64 = tu.sigmas(P1, S1, tu.threshold_tuples(256, 3), np.float64).max()
    print(shape, idx, float(sigma), best64)
    assert abs(float(sigma) - best64) <= 1e-5 * best64


def test_shortcut_and_too_few_values():
    hist = np.zeros(256, np.int64)
    hist[[3, 40, 41, 200]] = [5, 1, 7, 2]
    assert tu.multiotsu_indices(hist, 4)[0].tolist() == [3, 40, 41]
    with pytest.raises(ValueError):
        tu.multiotsu_indices(hist, 5)


@pytest.mark.parametrize("shape", SHAPES + [(200, 300)])
def test_host_derivation_reproduces_numpy(shape):
    from ipp_amd import thresholds as th
    img = tu.four_mode_image(shape, seed=11)
    log_img = np.log1p(img, dtype=np.float32)
    code_counts = np.bincount(img.reshape(-1), minlength=65536)
    hist, edges = th.log_histogram_of_codes(code_counts)
    want_hist, want_edges = np.histogram(log_img.reshape(-1), 256)
    assert edges.dtype == np.float32 and np.array_equal(edges, want_edges)
    assert np.array_equal(hist, want_hist)
    for threshold in (np.float32(0.0), np.float32(5.0), tu.threshold_multiotsu(log_img, 4)[2], np.float32(12.0)):
        for percentile in (99.99, 99.9, 50, 0, 100):
            above = log_img[log_img > threshold]
            want = np.percentile(above, percentile) if above.size else log_img.max()
            got = th.masked_percentile_of_codes(code_counts, threshold, percentile)
            assert int(np.round(np.expm1(got))) == int(np.round(np.expm1(want))), (threshold, percentile, got, want)
            assert th.bit_shift_of_upper_bound(got) == tu.estimate_bit_shift(log_img, threshold, percentile)[0]


def test_host_derivation_u8_and_constant():
    from ipp_amd import thresholds as th
    img = tu.four_mode_image((48, 80), dtype=np.uint8)
    hist, edges = th.log_histogram_of_codes(np.bincount(img.reshape(-1), minlength=256))
    want_hist, want_edges = np.histogram(np.log1p(img, dtype=np.float32).reshape(-1), 256)
    assert np.array_equal(edges, want_edges) and np.array_equal(hist, want_hist)
    one = np.zeros(256, np.int64)
    one[17] = 99
    hist, edges = th.log_histogram_of_codes(one)
    want_hist, want_edges = np.histogram(np.full(99, np.log1p(np.float32(17)), np.float32), 256)
    assert np.array_equal(edges, want_edges) and np.array_equal(hist, want_hist)


def test_percentile_of_sorted_is_numpys():
    from ipp_amd import thresholds as th
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 1000, 100003):
        a = np.sort(rng.random(n).astype(np.float32) * 11)
        for percentile in (0, 0.01, 25, 50, 99.9, 99.99, 100):
            assert th.percentile_of_sorted(lambda k: a[k], n, percentile) == np.percentile(a, percentile), (n, percentile)


def test_bit_shift_of_upper_bound():
    from ipp_amd import thresholds as th
    f = lambda counts: th.bit_shift_of_upper_bound(np.log1p(np.float32(counts)))
    assert [f(c) for c in (10, 256, 300, 512, 600, 40000, 65535)] == [0, 0, 1, 1, 2, 8, 8]


def test_refusals_and_errors_without_a_device():
    from ipp_amd import thresholds as th
    img = np.ones((4, 5), np.float32)
    with pytest.raises(NotImplementedError, match="hist"):
        th.threshold_multiotsu(img, hist=np.ones(256))
    with pytest.raises(NotImplementedError, match="nbins"):
        th.threshold_multiotsu(img, nbins=128)
    with pytest.raises(NotImplementedError, match="classes"):
        th.threshold_multiotsu(img, classes=5)
    with pytest.raises(NotImplementedError, match="uint16"):
        th.threshold_multiotsu(img.astype(np.uint16))
    with pytest.raises(NotImplementedError, match="float64"):
        th.threshold_multiotsu(img.astype(np.float64))
    with pytest.raises(NotImplementedError, match="float64"):
        th.threshold_multiotsu_batch(img.astype(np.float64)[None], 4)
    with pytest.raises(ValueError):
        th.threshold_multiotsu()
    with pytest.raises(ValueError):
        th.threshold_multiotsu(img, classes=1)
    with pytest.raises(ValueError):
        th.threshold_multiotsu(np.ones((0, 3), np.float32))
    with pytest.raises(NotImplementedError, match="float64"):
        th.estimate_bit_shift(img.astype(np.float64), 1.0)
    with pytest.raises(ValueError):
        th.estimate_slice_params(np.ones((4, 5), np.uint16))
    with pytest.raises(NotImplementedError, match="float32"):
        th.estimate_slice_params(np.ones((4, 4, 5), np.float32))
    with pytest.raises(ValueError):
        th.percentile_of_sorted(lambda k: 0.0, 3, 101)
    import inspect
    sig = inspect.signature(th.threshold_multiotsu).parameters
    assert [sig[k].default for k in ("image", "classes", "nbins", "hist")] == [None, 3, 256, None]
    assert sig["hist"].kind is inspect.Parameter.KEYWORD_ONLY


def test_nothing_wanted_needs_no_device():
    from ipp_amd import thresholds as th
    params = th.estimate_slice_params(np.ones((4, 4, 5), np.uint16), need_bleach_correction=False, need_16bit_to_8bit_conversion=False)
    assert dict(params) == dict(bleach_correction_clip_min=None, bleach_correction_clip_med=None, bleach_correction_clip_max=None,
                                bit_shift_to_right=8, dark=0)
    assert list(params.slices) == []


def test_estimate_clips_parser_wiring(capsys):
    from ipp_amd import pystripe, thresholds as th
    base = ["--input", "slices", "--bleach_correction_frequency", "0.015625"]
    assert pystripe._parse_args(base).estimate_clips is False
    a = pystripe._parse_args(base + ["--estimate_clips", "--bleach_correction_clip_med", "6.5"])
    assert a.estimate_clips is True
    with pytest.raises(SystemExit):
        pystripe._parse_args(["--input", "slices", "--estimate_clips"])
    calls = []

    def fake(source, **kw):
        calls.append((source, kw))
        return th.SliceParams(bleach_correction_clip_min=5.25, bleach_correction_clip_med=7.0, bleach_correction_clip_max=8.5,
                              bit_shift_to_right=3, dark=190)

    clips = pystripe._estimated_clips(a, estimate=fake)
    assert clips == dict(bleach_correction_clip_min=5.25, bleach_correction_clip_med=6.5, bleach_correction_clip_max=8.5)
    assert calls == [("slices", dict(need_bleach_correction=True, need_16bit_to_8bit_conversion=False))]
    assert "--bleach_correction_clip_min=5.25" in capsys.readouterr().out
    pystripe.check_bleach((64, 64), a.bleach_correction_frequency, *clips.values())
    # every clip given, or no --estimate_clips: nothing is estimated
    given = base + ["--bleach_correction_clip_min", "5", "--bleach_correction_clip_med", "6", "--bleach_correction_clip_max", "7"]
    for argv in (given + ["--estimate_clips"], given, base):
        before = len(calls)
        got = pystripe._estimated_clips(pystripe._parse_args(argv), estimate=fake)
        assert len(calls) == before and set(got) == set(pystripe.BLEACH_CLIPS)
    assert isinstance(th._parse_args(["--input", "slices"]), argparse.Namespace)
    assert th.SliceParams(dark=1).as_json() == dict(dark=1, slices=[])
