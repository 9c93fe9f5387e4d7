"""GPU: the per-tile automatic bleach clips of the pystripe stage (a clip given as NaN, include/mi_pystripe.h; ipp_amd.pystripe with
extended=True and a clip left None) against the goldens of the reference's own code (tests/golden/autoclips) and the restatement of tests/autoclips_util.py.

Standards, those of tests/test_gpu_bleach.py: log domain within 4 E_ref of the float64 restatement; integer results within
``integer_allowance`` of the golden with at most 1 % of the pixels differing; float results within 5 E_ref (|v| + 1).  The triple of
an integer-kind tile equals the restatement's float32 thresholds bit for bit (numpy's log1p table decides the bins); on a float tile
the device's log1pf may move a sample by an ulp, so each threshold lies within one bin width and the output is compared with the
restatement fed the device's own triple.  Every measured figure is printed before it is asserted.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from tests import autoclips_util as A
from tests import bleach_util as B
from tests import pystripe_util as U
from tests import thresholds_util as T
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = A.golden_cases(ROOT)
AUTO = dict(bleach_correction_clip_min=None, bleach_correction_clip_med=None, bleach_correction_clip_max=None)
OK, UNIFORM, TOO_FEW, ORDER, NONFINITE = 0, -1, 1, 2, 3


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


def check_against(name, got, want, e_ref):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if want.dtype.kind in "ui":
        share = float((d != 0).mean())
        print(f"{name}: integer result, {100 * share:.3f} % of pixels differ from the reference, max {d.max():g} counts (E_ref {e_ref:.3g})")
        assert (d <= U.integer_allowance(want, e_ref)).all()
        assert share <= 0.01
    else:
        tol = 5 * e_ref * (np.abs(want.astype(np.float64)) + 1)
        print(f"{name}: float result, max |d| {d.max():.3g}, max d / allowance {(d / np.maximum(tol, 1e-30)).max():.3g}")
        assert (d <= tol).all()


def check_log(name, got, log64, e_ref):
    err = float(np.abs(got.astype(np.float64) - log64).max())
    print(f"{name}: log domain, device vs float64 restatement {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f} (allowed 4)")
    assert got.dtype == np.float32 and got.shape == log64.shape
    assert err <= 4 * e_ref


def run_plan(ps, dev, stack, flat=None, max_batch=0, **kw):
    """one Plan over a [n, ny, nx] stack (numpy or device tensor): (result, clips [n, 3], status [n])"""
    import torch
    tiles = stack if isinstance(stack, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(stack)).to(dev)
    dt = np.dtype(str(tiles.dtype).replace("torch.", ""))
    plan = ps.Plan(dev, tuple(tiles.shape[1:]), dt, ps.make_params(dt, flat=flat is not None, max_batch=max_batch or int(tiles.shape[0]), extended=True, **kw))
    try:
        out = plan.run(tiles, None if flat is None else torch.from_numpy(flat).to(dev))
        torch.cuda.synchronize(dev)
        clips, status = plan.clips()
        return out.cpu().numpy(), clips, status
    finally:
        plan.close()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def bin_width(img, **kw):
    log = A.log_image(img, **kw)
    return float(log.max() - log.min()) / 256


@pytest.mark.parametrize("name", CASES)
def test_golden_through_process_img(ps, dev, name):
    z, kw = A.load_case(ROOT, name)
    got = ps.process_img(z["img"].copy(), device=dev, extended=True, **kw)
    check_against(name, got, z["out"], float(z["e_ref"]))


@pytest.mark.parametrize("name", CASES)
def test_golden_log_domain_and_triple(ps, dev, name):
    z, kw = A.load_case(ROOT, name)
    img, e_ref = z["img"], float(z["e_ref"])
    stack = np.stack([img, img[::-1].copy()])
    got, clips, status = run_plan(ps, dev, stack, log_output=True, **kw)
    assert status.tolist() == [OK, OK]
    want = A.used_triple(z["triple"])
    print(f"{name}: triple {clips[0].tolist()}, the reference's {want.tolist()}")
    if img.dtype.kind in "ui":
        assert same_bits(clips[0], want) and same_bits(clips[1], want)     # a flipped tile has the same histogram
    else:
        assert (np.abs(clips[0].astype(np.float64) - want) <= bin_width(img, **kw)).all()
    check_log(name, got[0], z["log64"], e_ref)


@pytest.mark.parametrize("dtype,shape,extra", [
    (np.uint8, (37, 53), {}), (np.uint16, (37, 53), {}),
    (np.uint16, (41, 75), dict(down_sample=(2, 2), down_sample_method="max")),
    (np.uint16, (41, 75), dict(down_sample=(2, 2), down_sample_method="min")),
    (np.uint8, (41, 75), dict(down_sample=(3, 2), down_sample_method="max")),
])
def test_integer_kind_triples_equal_the_restatement(ps, dev, dtype, shape, extra):
    img = T.four_mode_image(shape, 21, dtype)
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 32, **AUTO, **extra)
    assert ps.derive(shape, dtype, ps.make_params(dtype, extended=True, **kw)).integer_kind == 1
    out, clips, status = run_plan(ps, dev, img[None], **kw)
    want = A.used_triple(A.triple(img, **kw))
    print(f"{np.dtype(dtype).name} {shape} {extra}: triple {clips[0].tolist()}, restatement {want.tolist()}")
    assert status[0] == OK and same_bits(clips[0], want)
    r32, _, e_ref = A.live_reference(img, **kw)
    check_against(f"{np.dtype(dtype).name} {shape} {extra}", out[0], r32, e_ref)


@pytest.mark.parametrize("case", ["f32", "flat", "mean", "median"])
def test_float_tiles_within_one_bin(ps, dev, case):
    shape = (41, 75)
    img = A.float_tile(shape, 22) if case == "f32" else T.four_mode_image(shape, 22)
    flat = A.flat_field(shape) if case == "flat" else None
    extra = dict(down_sample=(2, 2), down_sample_method=case) if case in ("mean", "median") else {}
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 32, **AUTO, **extra)
    assert A.indices_are_stable(A.log_image(img, flat=flat, **kw))
    out, clips, status = run_plan(ps, dev, img[None], flat=flat, **kw)
    want = A.used_triple(A.triple(img, flat=flat, **kw))
    width = bin_width(img, flat=flat, **kw)
    d = np.abs(clips[0].astype(np.float64) - want)
    print(f"{case}: triple {clips[0].tolist()}, restatement {want.tolist()}, max difference {d.max():.3g} of a bin width {width:.3g}")
    assert status[0] == OK and (d <= width).all()
    r32, _, e_ref = A.live_reference(img, clips=clips[0], flat=flat, **kw)
    check_against(case, out[0], r32, e_ref)


def test_tiles_of_a_batch_do_not_see_each_other(ps, dev):
    """Five tiles of different brightness and mixture, one of them uniform, in chunks of two: every tile's result and triple equal,
    bit for bit, what it gets alone; the uniform tile is zeros with status -1; Plan.clips() covers all five."""
    shape = (45, 70)
    tiles = np.stack([T.four_mode_image(shape, 30), (T.four_mode_image(shape, 31) // 3).astype(np.uint16), np.full(shape, 777, np.uint16),
                      np.clip(T.four_mode_image(shape, 32) * 2.5, 0, 65535).astype(np.uint16), T.four_mode_image(shape, 33)[::-1].copy()])
    for extra in (dict(sigma=(0, 0)), dict(sigma=(8, 8), wavelet="db9", padding_mode="reflect", bidirectional=True),
                  dict(sigma=(0, 0), bleach_correction_max_method=True)):
        kw = dict(bleach_correction_frequency=1 / 32, **AUTO, **extra)
        alone = [run_plan(ps, dev, tiles[i:i + 1], **kw) for i in range(5)]
        out, clips, status = run_plan(ps, dev, tiles, max_batch=2, **kw)
        assert status.tolist() == [OK, OK, UNIFORM, OK, OK] and clips.shape == (5, 3)
        assert not out[2].any() and out[0].any()
        for i in range(5):
            assert np.array_equal(out[i], alone[i][0][0]), (extra, i)
            assert alone[i][2][0] == status[i]
            if i != 2:
                assert same_bits(clips[i], alone[i][1][0]) and same_bits(clips[i], A.used_triple(A.triple(tiles[i], **kw))), (extra, i)
        assert not same_bits(clips[0], clips[1])


def test_four_and_three_distinct_codes(ps, dev):
    rng = np.random.default_rng(40)
    four = rng.choice(np.array([100, 400, 2500, 20000], np.uint16), size=(33, 47))
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 16, **AUTO)
    out, clips, status = run_plan(ps, dev, four[None], **kw)
    want = A.used_triple(A.triple(four, **kw))          # the occupied bins but the last
    assert status[0] == OK and same_bits(clips[0], want)
    r32, _, e_ref = A.live_reference(four, **kw)
    check_against("four codes", out[0], r32, e_ref)
    three = rng.choice(np.array([100, 400, 2500], np.uint16), size=(33, 47))
    with pytest.raises(ValueError, match="cannot be thresholded in 4 classes"):
        A.triple(three, **kw)
    out, clips, status = run_plan(ps, dev, np.stack([three, four]), **kw)
    assert status.tolist() == [TOO_FEW, OK] and not out[0].any() and same_bits(clips[1], want)
    with pytest.raises(ValueError, match=r"tile 0: bleach_correction_clip_min, _med, _max = \(nan, nan, nan\)"):
        ps.process_img(three, device=dev, extended=True, **kw)
    with pytest.raises(ValueError, match="tile 1"):
        ps.process_img(np.stack([four, three]), device=dev, extended=True, **kw)


def test_clips_out_of_order(ps, dev):
    """The reference's defaults of convert.py, 20 and 255 in log1p units: the estimated clip_med of an ordinary tile lies below
    clip_min and the assert of correct_bleaching fires.  A tile whose log image reaches beyond 20 shares the batch and is correct."""
    rng = np.random.default_rng(41)
    shape = (33, 47)
    ordinary = A.float_tile(shape, 41)
    high = np.exp(rng.choice([10.0, 26.0, 40.0, 70.0], p=[.4, .3, .2, .1], size=shape) * (1 + 0.01 * rng.standard_normal(shape))).astype(np.float32)
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 16, bleach_correction_clip_min=20.0, bleach_correction_clip_med=None,
              bleach_correction_clip_max=255.0)
    with pytest.raises(AssertionError, match=r"tile 0: bleach_correction_clip_min, _med, _max = \(20\.0, 6\.\d+, 255\.0\)"):
        ps.process_img(ordinary, device=dev, extended=True, **kw)
    with pytest.raises(AssertionError, match="tile 1"):
        ps.process_img(np.stack([high, ordinary]), device=dev, extended=True, **kw)
    out, clips, status = run_plan(ps, dev, np.stack([ordinary, high]), log_output=True, **kw)
    alone, clips1, status1 = run_plan(ps, dev, high[None], log_output=True, **kw)
    assert status.tolist() == [ORDER, OK] and status1[0] == OK and not out[0].any()
    assert np.array_equal(out[1], alone[0]) and same_bits(clips[1], clips1[0]) and 20 < clips[1][1] < 255
    _, l64, e_ref = A.live_reference(high, clips=clips[1], **kw)
    check_log("high tile beside a refused one", out[1], l64, e_ref)


def test_nan_raises(ps, dev):
    img = A.float_tile((33, 47), 42)
    img[5, 7] = np.nan
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 16, **AUTO)
    out, clips, status = run_plan(ps, dev, img[None], **kw)
    assert status[0] == NONFINITE and not out.any()
    with pytest.raises(ValueError, match="tile 0.*not finite"):
        ps.process_img(img, device=dev, extended=True, **kw)
    with pytest.raises(ValueError, match="not finite"):
        ps.filter_streaks(img, sigma=(0, 0), device=dev, extended=True, **{k: v for k, v in kw.items() if k != "sigma"})


def test_odd_shape_from_an_unaligned_view(ps, dev):
    """301 x 517 uint16 whose first sample lies 2 bytes behind a 16-byte boundary."""
    import torch
    img = T.four_mode_image((301, 517), 43)
    backing = torch.zeros(img.size + 8, dtype=torch.uint16, device=dev)
    view = backing[1:1 + img.size].view(1, 301, 517)
    view.copy_(torch.from_numpy(img[None]).to(dev))
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    for extra in (dict(sigma=(0, 0)), dict(sigma=(8, 8), wavelet="db9", padding_mode="reflect", bidirectional=True)):
        kw = dict(bleach_correction_frequency=1 / 256, **AUTO, **extra)
        out, clips, status = run_plan(ps, dev, view, **kw)
        assert status[0] == OK and same_bits(clips[0], A.used_triple(A.triple(img, **kw)))
        r32, _, e_ref = A.live_reference(img, **kw)
        check_against(f"unaligned 301 x 517 {extra['sigma']}", out[0], r32, e_ref)
        got = ps.process_img(view[0], device=dev, extended=True, **kw)
        assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy(), out[0])


def test_segmented_row_route_with_automatic_clips(ps, dev):
    img = T.four_mode_image((3, 20500), 44)
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 4096, **AUTO)
    assert ps.derive(img.shape, img.dtype, ps.make_params(img.dtype, extended=True, **kw)).bleach_long_rows == 1
    out, clips, status = run_plan(ps, dev, img[None], **kw)
    assert status[0] == OK and same_bits(clips[0], A.used_triple(A.triple(img, **kw)))
    r32, l64, e_ref = A.live_reference(img, **kw)
    check_against("3 x 20500", out[0], r32, e_ref)
    log, _, _ = run_plan(ps, dev, img[None], log_output=True, **kw)
    check_log("3 x 20500", log[0], l64, e_ref)


def test_given_clips_equal_the_automatic_ones_when_they_are_the_same_numbers(ps, dev):
    """The constant path (bleach_auto == 0) and the per-tile path read the same numbers: equal bytes."""
    img = T.four_mode_image((45, 70), 45)
    for extra in (dict(sigma=(0, 0)), dict(sigma=(0, 0), bleach_correction_max_method=True)):
        kw = dict(bleach_correction_frequency=1 / 32, **extra)
        auto, clips, _ = run_plan(ps, dev, img[None], **AUTO, **kw)
        given = dict(zip(A.CLIP_KEYS, (float(v) for v in A.triple(img, **AUTO))))
        const, clips0, status0 = run_plan(ps, dev, img[None], **given, **kw)
        assert np.array_equal(auto, const) and same_bits(clips, clips0) and status0[0] == OK


def test_plans_without_automatic_clips_give_the_bytes_they_gave_before(ps, dev):
    """bleach_auto == 0: the result of every committed bleach golden (tests/golden/bleach) through the C ABI has the SHA-256 recorded
    from the library as it was before bleach_auto existed (tests/golden/autoclips/bleach_before.json; results and log images)."""
    import torch
    from ipp_amd import capi
    with open(os.path.join(A.golden_dir(ROOT), "bleach_before.json")) as f:
        before = json.load(f)
    names = B.golden_cases(ROOT)
    assert sorted(before) == names and len(names) >= 14
    lib = capi.lib()
    for name in names:
        z, kw = B.load_case(ROOT, name)
        img = z["img"]
        stack = torch.from_numpy(np.stack([img, img[::-1].copy()])).to(dev)
        for log in (False, True):
            params = ps.make_params(img.dtype, log_output=log, max_batch=2, **kw)
            assert params.bleach_auto == 0
            h = C.c_void_p()
            capi.check(lib.mi_pystripe_plan_create(dev.index or 0, img.shape[0], img.shape[1], {1: 0, 2: 1, 4: 2}[img.dtype.itemsize],
                                                   C.byref(params), C.byref(h)))
            try:
                info = capi.PystripeInfo()
                capi.check(lib.mi_pystripe_plan_info(h, C.byref(info)))
                out = torch.zeros((2, info.out_ny, info.out_nx), dtype={0: torch.uint8, 1: torch.uint16, 2: torch.float32}[info.out_dtype], device=dev)
                capi.check(lib.mi_pystripe_run(h, capi.current_stream_ptr(dev), stack.data_ptr(), None, out.data_ptr(), 2))
                torch.cuda.synchronize(dev)
            finally:
                lib.mi_pystripe_plan_destroy(h)
            digest = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
            assert digest == before[name]["log" if log else "out"], (name, log)
