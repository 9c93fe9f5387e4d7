"""GPU: the bleach correction of the pystripe stage (ipp_amd.pystripe, include/mi_pystripe.h) against the goldens of the reference's
own code (tests/golden/bleach) and the restatement of tests/bleach_util.py.  Reads tests/golden/ and the two utility modules only.

Standards, those of tests/test_gpu_pystripe.py:
  * log domain: max |device - float64 restatement| <= 4 E_ref, E_ref = the float32 reference's own distance from the same float64
    result, floored at one float32 spacing of the largest |log64| (at sigma == (0, 0) E_ref is three float32 roundings, and no
    float32 image lies closer to a float64 one than its own rounding);
  * integer results: every pixel within 1 + ceil(5 E_ref (v + 1)) counts of the golden's value v, at most 1 % of the pixels differ;
  * float results: |device - golden| <= 5 E_ref (|v| + 1).
Every measured figure is printed before it is asserted; BLEACH_REPORT=<file> appends them to a file.

The row filter keeps a row of up to B.LDS_ROW = (160 KiB - 16 * 16 B) / 8 B - 12 = 20436 samples in LDS (the row, its 12 extension
samples and the 16 wave totals of the scan, all float64, in the 160 KiB one work-group may request); a longer row goes through LDS in
segments.  Both sides of that length, and a row of three segments, are live cases below.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bleach_util as B
from tests import pystripe_util as U
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = B.golden_cases(ROOT)
CLIPS = dict(bleach_correction_clip_min=6.0, bleach_correction_clip_med=7.0, bleach_correction_clip_max=8.0)


def report(line):
    print(line)
    path = os.environ.get("BLEACH_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


def check_against(name, got, want, e_ref):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if want.dtype.kind in "ui":
        share = float((d != 0).mean())
        report(f"{name}: integer result, {100 * share:.3f} % of pixels differ from the reference, max {d.max():g} counts (E_ref {e_ref:.3g})")
        assert (d <= U.integer_allowance(want, e_ref)).all()
        assert share <= 0.01
    else:
        tol = 5 * e_ref * (np.abs(want.astype(np.float64)) + 1)
        report(f"{name}: float result, max |d| {d.max():.3g}, max d / allowance {(d / np.maximum(tol, 1e-30)).max():.3g}")
        assert (d <= tol).all()


def check_log(name, got, log64, e_ref):
    err = float(np.abs(got.astype(np.float64) - log64).max())
    report(f"{name}: log domain, device vs float64 restatement {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f} (allowed 4)")
    assert got.dtype == np.float32 and got.shape == log64.shape
    assert err <= 4 * e_ref


def run_abi(dev, img_stack, params):
    """through the C ABI alone: plan_create / plan_info / run / destroy"""
    import torch
    from ipp_amd import capi
    lib = capi.lib()
    n, ny, nx = img_stack.shape
    code = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}[img_stack.dtype]
    h = C.c_void_p()
    capi.check(lib.mi_pystripe_plan_create(dev.index or 0, ny, nx, code, C.byref(params), C.byref(h)))
    try:
        info = capi.PystripeInfo()
        capi.check(lib.mi_pystripe_plan_info(h, C.byref(info)))
        tin = torch.from_numpy(img_stack).to(dev)
        tdt = {0: torch.uint8, 1: torch.uint16, 2: torch.float32}[info.out_dtype]
        out = torch.full((n, info.out_ny, info.out_nx), 77, dtype=torch.float32, device=dev).to(tdt)
        capi.check(lib.mi_pystripe_run(h, capi.current_stream_ptr(dev), tin.data_ptr(), None, out.data_ptr(), n))
        torch.cuda.synchronize(dev)
        return out.cpu().numpy(), info
    finally:
        lib.mi_pystripe_plan_destroy(h)


def live_reference(img, **kw):
    """(float32 result, float64 log image, E_ref) of the restatement for a case without a golden"""
    r32, l32 = B.process_img(img.copy(), dt=np.float32, **kw)
    _, l64 = B.process_img(img.copy(), dt=np.float64, **kw)
    return r32, l64, max(float(np.abs(l32.astype(np.float64) - l64).max()), B.e_ref_floor(l64))


@pytest.mark.parametrize("name", CASES)
def test_golden_through_process_img(ps, dev, name):
    z, kw = B.load_case(ROOT, name)
    got = ps.process_img(z["img"].copy(), device=dev, **kw)
    check_against(name, got, z["out"], float(z["e_ref"]))


@pytest.mark.parametrize("name", CASES)
def test_golden_log_domain_through_the_c_abi(ps, dev, name):
    z, kw = B.load_case(ROOT, name)
    img, e_ref = z["img"], float(z["e_ref"])
    stack = np.stack([img, img[::-1].copy()])
    got, info = run_abi(dev, stack, ps.make_params(img.dtype, log_output=True, max_batch=2, **kw))
    assert info.bleach_long_rows == 0
    check_log(name, got[0], z["log64"], e_ref)
    out, _ = run_abi(dev, stack, ps.make_params(img.dtype, max_batch=2, **kw))
    check_against(name + " (ABI)", out[0], z["out"], e_ref)


@pytest.mark.parametrize("max_method", [False, True])
def test_many_chunks_per_row(ps, dev, max_method):
    """(5, 4099) uint16 at sigma (0, 0): 4111 samples in LDS, 512 threads with nine samples each, an odd length.  The max method
    needs 7 rows for its column of row maxima: (9, 4099)."""
    img = U.synthetic_tile((9 if max_method else 5, 4099), 71, np.uint16, "cols")
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 512, bleach_correction_max_method=max_method, **B.clips_for(img))
    r32, l64, e_ref = live_reference(img, **kw)
    check_log(f"{img.shape} max_method {max_method}", ps.filter_streaks(img.copy(), device=dev, log_output=True, **kw), l64, e_ref)
    check_against(f"{img.shape} max_method {max_method}", ps.process_img(img.copy(), device=dev, **kw), r32, e_ref)


@pytest.mark.parametrize("width,long_rows", [(B.LDS_ROW, 0), (B.LDS_ROW + 1, 1), (41000, 1)])
def test_both_sides_of_the_lds_row_length(ps, dev, width, long_rows):
    """float32 tiles of 3 rows: 20436 samples, the longest row that stays in LDS; 20437, whose 20449 float64 samples go through LDS as
    segments of 20448 and 1 (forwards) and of 1 and 20448 (backwards); 41000, three segments.  The cutoff 1 / 4096 gives the filter a
    memory of thousands of samples, so the state carried from segment to segment decides the result."""
    assert B.LDS_ROW == 20436
    img = U.synthetic_tile((3, width), 72, np.float32, "cols")
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 4096, **B.clips_for(img))
    assert ps.derive(img.shape, img.dtype, ps.make_params(img.dtype, **kw)).bleach_long_rows == long_rows
    r32, l64, e_ref = live_reference(img, **kw)
    check_log(f"(3, {width})", ps.filter_streaks(img.copy(), device=dev, log_output=True, **kw), l64, e_ref)
    check_against(f"(3, {width})", ps.process_img(img.copy(), device=dev, **kw), r32, e_ref)
    # the max method filters the 3 row maxima... it needs 7 rows: a (7, width) tile, its vector of column maxima takes the same route
    img = U.synthetic_tile((7, width), 73, np.float32, "cols")
    kw = dict(kw, bleach_correction_max_method=True, **B.clips_for(img))
    assert ps.derive(img.shape, img.dtype, ps.make_params(img.dtype, **kw)).bleach_long_rows == long_rows
    r32, l64, e_ref = live_reference(img, **kw)
    check_log(f"(7, {width}) max method", ps.filter_streaks(img.copy(), device=dev, log_output=True, **kw), l64, e_ref)


def test_all_zero_row_inside_a_varying_tile(ps, dev):
    img = U.synthetic_tile((40, 300), 74, np.uint16)
    img[17] = 0
    img[30, 100:200] = 0
    for max_method in (False, True):
        kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 64, bleach_correction_max_method=max_method, **B.clips_for(img))
        r32, l64, e_ref = live_reference(img, **kw)
        assert not l64[17].any()      # log1p(0) / F = 0
        check_log(f"zero row, max_method {max_method}", ps.filter_streaks(img.copy(), device=dev, log_output=True, **kw), l64, e_ref)
        got = ps.process_img(img.copy(), device=dev, **kw)
        check_against(f"zero row, max_method {max_method}", got, r32, e_ref)
        assert not got[17].any() and got[16].any()


def test_negative_log_values(ps, dev):
    """A float32 tile with samples in (-1, 0): L has both signs, so the row and column maxima and max F must not assume positive
    floats (the maxima of the two last rows are negative before the clip lifts them)."""
    rng = np.random.default_rng(75)
    img = U.synthetic_tile((33, 70), 75, np.float32)
    img[-2:] = -0.2 - 0.5 * rng.random((2, 70), dtype=np.float32)
    img[:, 5] = -0.5
    for max_method in (False, True):
        kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 16, bleach_correction_max_method=max_method, **B.clips_for(img))
        r32, l64, e_ref = live_reference(img, **kw)
        assert l64.min() < 0 and np.log1p(img.astype(np.float64)).max(axis=1)[-1] < 0
        check_log(f"negative L, max_method {max_method}", ps.filter_streaks(img.copy(), device=dev, log_output=True, **kw), l64, e_ref)


@pytest.mark.parametrize("max_method", [False, True])
def test_tiles_of_a_batch_do_not_see_each_other(ps, dev, max_method):
    """Three tiles of very different brightness: each tile's result in the stack equals, bit for bit, the result of running it alone,
    at every position of the stack -- a maximum that leaks from tile to tile would scale the dim tiles by the bright one's."""
    import torch
    base = U.synthetic_tile((61, 150), 76, np.float32)
    tiles = np.stack([np.clip(base * np.float32(g), 0, 65535) for g in (0.02, 1.0, 12.0)]).astype(np.uint16)
    assert tiles[0].max() < 200 and tiles[2].max() > 30000
    kw = dict(bleach_correction_frequency=1 / 32, bleach_correction_max_method=max_method, bleach_correction_clip_min=float(np.log1p(5.0)),
              bleach_correction_clip_med=float(np.log1p(400.0)), bleach_correction_clip_max=float(np.log1p(20000.0)))
    for extra in (dict(sigma=(0, 0)), dict(sigma=(8, 8), wavelet="db9", padding_mode="reflect", bidirectional=True)):
        for log in (False, True):
            alone = [ps.Plan(dev, tiles.shape[1:], np.uint16, ps.make_params(np.uint16, log_output=log, max_batch=1, **kw, **extra))
                     for _ in range(3)]
            single = [p.run(torch.from_numpy(tiles[i:i + 1].copy()).to(dev))[0].cpu().numpy() for i, p in enumerate(alone)]
            for p in alone:
                p.close()
            assert not np.array_equal(single[0], single[1])
            plan = ps.Plan(dev, tiles.shape[1:], np.uint16, ps.make_params(np.uint16, log_output=log, max_batch=3, **kw, **extra))
            for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
                got = plan.run(torch.from_numpy(np.ascontiguousarray(tiles[list(order)])).to(dev)).cpu().numpy()
                for place, i in enumerate(order):
                    assert np.array_equal(got[place], single[i]), (extra, log, order, place)
            plan.close()


def test_filter_streaks_log_output_without_a_stripe_filter(ps, dev):
    z, kw = B.load_case(ROOT, "u16_nofilter_rows")
    kw.pop("sigma")
    log = ps.filter_streaks(z["img"].copy(), sigma=(0, 0), device=dev, log_output=True, **kw)
    check_log("filter_streaks, sigma (0, 0)", log, z["log64"], float(z["e_ref"]))
    check_against("filter_streaks, sigma (0, 0)", ps.filter_streaks(z["img"].copy(), sigma=(0, 0), device=dev, **kw), z["out"], float(z["e_ref"]))
    # and behind the stripe filter, a stack of two through every launch together
    z, kw = B.load_case(ROOT, "u16_filter_max")
    stack = np.stack([z["img"], z["img"][::-1].copy()])
    sigma = kw.pop("sigma")
    log = ps.filter_streaks(stack, sigma=sigma, device=dev, log_output=True, **kw)
    check_log("filter_streaks, sigma (16, 16), max method", log[0], z["log64"], float(z["e_ref"]))


def test_lightsheet_runs_behind_the_step(ps, dev):
    """With lightsheet=True the bleach correction belongs to the head plan: the result equals lightsheet correction of the tile the
    bleach-corrected head hands over (dark included), then the tail."""
    img = U.synthetic_tile((64, 180), 77, np.uint16)
    kw = dict(sigma=(0, 0), bleach_correction_frequency=1 / 32, **B.clips_for(img))
    head = ps.process_img(img.copy(), dark=40, device=dev, **kw)
    want = np.rot90(ps.correct_lightsheet(head, lightsheet=dict(selem=(1, 150, 1)), device=dev), 1)
    got = ps.process_img(img.copy(), dark=40, lightsheet=True, rotate=90, device=dev, **kw)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert not np.array_equal(head, ps.process_img(img.copy(), dark=40, device=dev))       # the step did something


def test_batch_filter_folder_to_folder(ps, dev, tmp_path):
    from PIL import Image
    src, dst = tmp_path / "in", tmp_path / "out"
    tiles = {f"ch0/t_{i:03d}.tif": U.synthetic_tile((75, 101), 320 + i, np.uint16) for i in range(2)}
    for rel, img in tiles.items():
        (src / rel).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(img).save(src / rel, format="TIFF", compression="tiff_adobe_deflate")
    clips = B.clips_for(tiles["ch0/t_000.tif"])
    stats = {}
    assert ps.batch_filter(src, dst, bleach_correction_frequency=1 / 64, device=dev, stats=stats, **clips) == 0      # max method: the default
    assert stats["written"] == 2
    for rel, img in tiles.items():
        with Image.open(dst / rel) as im:
            got = np.array(im)
        r32, l64, e_ref = live_reference(img, sigma=(0, 0), bleach_correction_frequency=1 / 64, bleach_correction_max_method=True, **clips)
        check_against("batch_filter " + rel, got, r32, e_ref)
        rows, _ = B.process_img(img.copy(), sigma=(0, 0), bleach_correction_frequency=1 / 64, bleach_correction_max_method=False, **clips)
        assert not np.array_equal(rows, r32)
