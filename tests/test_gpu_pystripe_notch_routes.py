"""GPU: the notch kernel's two- and one-line builds and its LDS edge (csrc/pystripe_notch.hip).

``notch_kernel<R>`` is built for R = 4, 2 and 1 coefficient lines per work-group; ``build_tables`` picks R per (pass, level, axis) from
the LDS request 16 n + 16 R kb + 4 R n, rounded up to 16 bytes: R = 4 up to 80 KB, R = 2 up to 53 KB, R = 1 up to 160 KB, a refusal
beyond.  Every tile of the other pystripe suites takes R = 4.  The cases here reach R = 2 (lines of about 1281 .. 1350 coefficients
with almost every bin kept: a sigma that is large against the tile) and R = 1 (any line longer than 2560 samples, whatever the
sigma: a tile or merged plane wider or taller than about 5100 pixels), along rows (element stride 1) and along columns (element
stride = the coefficient width), up to the last line length that fits, and the refusal behind it.  Only one axis has to be long, so
the tiles are a few rows high.  ``Plan.notch_routes()`` (mi_pystripe_plan_notch_routes) proves which build ran.

Standards: those of tests/test_gpu_pystripe.py, against the float64 restatement of tests/pystripe_util.py, with E_ref the float32
restatement's distance from it -- log domain within 4 E_ref, integer results within ``integer_allowance`` and at most 1 % of the
pixels differing, float results within 5 E_ref (|v| + 1).  In every case the filter moves the log image by 0.4 .. 1.0 and E_ref is
about 3e-6, so a wrong or skipped line misses the first standard by five orders of magnitude.  Every figure is printed before it is
asserted; PYSTRIPE_REPORT=<file> appends them (profiles/pystripe_notch_routes.txt was collected that way).
"""
import functools
import os

import numpy as np
import pytest

from tests import pystripe_util as U

pytestmark = pytest.mark.gpu


def report(line):
    print(line)
    path = os.environ.get("PYSTRIPE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


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

KB = 1024
LDS_LIMIT = 160 * KB

# name: tile shape, dtype, stripes, options, and what notch_routes() must report: {(pass, axis): fields}.  `lines` is the launch's line
# count.  kp is asserted where every position keeps a weight (kp == n) and printed otherwise: it sits on the last bit of expf, and the
# R of these cases holds for kp +- 2.
WIDE = dict(sigma=(600, 600), level=1, padding_mode="reflect", bidirectional=True)
THIN = dict(sigma=(4, 4), padding_mode="reflect", bidirectional=True)
CASES = {
    # 719 lines at R = 2: the last work-group has one live line
    "two_rows": ((9, 1140), np.uint16, "rows", WIDE,
                 {(0, 0): dict(n=1284, lines=719, R=2, kp=1284, lds=51392), (0, 1): dict(n=719, lines=1284, R=4)}),
    "two_cols": ((1140, 9), np.uint16, "cols", WIDE,
                 {(0, 1): dict(n=1284, lines=719, R=2, kp=1284, lds=51392), (0, 0): dict(n=719, lines=1284, R=4)}),
    # the same line length at R = 2 in the first pass and R = 4 in the second: the table index (pass * levels + level - 1) * 2
    "two_then_four": ((9, 1141), np.float32, "rows", dict(sigma=(600, 300), level=1, padding_mode="symmetric", bidirectional=True),
                      {(0, 0): dict(n=1285, lines=719, R=2, kp=1285), (1, 0): dict(n=1285, lines=719, R=4)}),
    "one_rows": ((16, 5200), np.uint16, "rows", THIN,
                 {(0, 0): dict(n=2612, lines=25, R=1, threads=64), (0, 1): dict(n=25, lines=2612, R=4)}),
    "one_cols": ((5200, 16), np.uint8, "cols", dict(sigma=(4, 4), padding_mode="wrap", bidirectional=True),
                 {(0, 1): dict(n=2612, lines=25, R=1, threads=64), (0, 0): dict(n=25, lines=2612, R=4)}),
    "one_two_pass": ((27, 5201), np.uint16, "rows", dict(sigma=(4, 9), padding_mode="reflect", bidirectional=True),
                     {(0, 0): dict(n=2619, lines=32, R=1), (1, 0): dict(n=2619, lines=32, R=1)}),
    # about 1041 bins on 512 threads: phase 1 loops more than once over the bins
    "one_wide_sigma": ((9, 2600), np.uint16, "rows", dict(sigma=(700, 700), level=1, padding_mode="reflect", bidirectional=True),
                       {(0, 0): dict(n=2132, lines=837, R=1, threads=512), (0, 1): dict(n=837, lines=2132, R=4, kp=837)}),
    # 163 408 of 163 840 bytes
    "lds_edge_rows": ((16, 16300), np.uint16, "rows", THIN, {(0, 0): dict(n=8162, lines=25, R=1, lds=163408)}),
    "lds_edge_cols": ((16300, 16), np.uint16, "cols", THIN, {(0, 1): dict(n=8162, lines=25, R=1, lds=163408)}),
}


def lds_request(n, kb, R):
    return (16 * n + 16 * R * kb + 4 * R * n + 15) // 16 * 16


def lines_per_group(n, kb):
    """build_tables' rule, restated"""
    for R, limit in ((4, 80 * KB), (2, 53 * KB), (1, LDS_LIMIT)):
        if lds_request(n, kb, R) <= limit:
            return R
    return 0


@functools.lru_cache(maxsize=None)
def reference(name):
    """(tile, float32 result, float64 log image, E_ref) of a case, computed once and shared; nobody writes to them"""
    shape, dtype, stripes, kw, _ = CASES[name]
    img = U.synthetic_tile(shape, 7, dtype, stripes)
    r32, l32 = U.process_img(img.copy(), dt=np.float32, **kw)
    _, l64 = U.process_img(img.copy(), dt=np.float64, **kw)
    for a in (img, r32, l64):
        a.setflags(write=False)
    return img, r32, l64, float(np.abs(l32.astype(np.float64) - l64).max())


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


def make_plan(ps, dev, name, **more):
    shape, dtype, _, kw, _ = CASES[name]
    return ps.Plan(dev, shape, dtype, ps.make_params(dtype, wavelet="db9", **dict(kw, **more)))


@pytest.mark.parametrize("name", list(CASES))
def test_routes_and_results(ps, dev, name):
    import torch
    shape, dtype, _, kw, expected = CASES[name]
    img, r32, l64, e_ref = reference(name)
    plan = make_plan(ps, dev, name, log_output=True, max_batch=1)
    try:
        routes = plan.notch_routes()
        log = plan.run(torch.from_numpy(img.copy()[None]).to(dev))[0].cpu().numpy()
    finally:
        plan.close()
    passes = 1 if kw["sigma"][0] == kw["sigma"][1] else 2
    assert [(r["pass"], r["level"], r["axis"]) for r in routes] == [(p, 1, a) for p in range(passes) for a in (0, 1)]
    for r in routes:
        report(f"{name} {shape} {np.dtype(dtype).name}: pass {r['pass']} level {r['level']} axis {r['axis']}: n {r['n']}, {r['lines']} lines, "
               f"kp {r['kp']}, kb {r['kb']}, R {r['R']}, {r['threads']} threads, lds {r['lds']}")
        # the record is consistent with the rule, whatever the case expects
        assert r["kb"] == r["kp"] // 2 + 1 and r["lds"] == lds_request(r["n"], r["kb"], r["R"]) <= LDS_LIMIT
        assert r["R"] == lines_per_group(r["n"], r["kb"])
        assert r["threads"] == min(512, max(64, (r["kb"] + 63) // 64 * 64))
    by_key = {(r["pass"], r["axis"]): r for r in routes}
    for key, want in expected.items():
        assert {k: by_key[key][k] for k in want} == want, (key, by_key[key])
    err = float(np.abs(log.astype(np.float64) - l64).max())
    moved = float(np.abs(l64 - np.log1p(img.astype(np.float64))).max())
    report(f"{name}: log domain, device vs float64 restatement {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f} (allowed 4); "
           f"the filter moves the log image by up to {moved:.2f}")
    assert log.dtype == np.float32 and log.shape == l64.shape
    assert err <= 4 * e_ref
    check_against(name, ps.process_img(img.copy(), device=dev, wavelet="db9", **kw), r32, e_ref)


@pytest.mark.parametrize("name", ["two_rows", "one_rows"])
def test_batch_and_chunk(ps, dev, name):
    """Three different tiles through a plan of max_batch 2: the notch runs with gridDim.y = 2, then 1.  Bit for bit what a one-tile
    plan gives for each."""
    import torch
    shape, dtype, stripes, _, _ = CASES[name]
    tiles = torch.from_numpy(np.stack([U.synthetic_tile(shape, 20 + i, dtype, stripes) for i in range(3)])).to(dev)
    for log in (False, True):
        single = make_plan(ps, dev, name, log_output=log, max_batch=1)
        batched = make_plan(ps, dev, name, log_output=log, max_batch=2)
        try:
            assert batched.info.max_batch == 2
            one = [single.run(tiles[i:i + 1])[0].clone() for i in range(3)]
            got = batched.run(tiles)
            torch.cuda.synchronize(dev)
            for i in range(3):
                assert torch.equal(got[i], one[i]), (name, log, i)
            assert not torch.equal(one[0], one[1]) and not torch.equal(one[1], one[2])
        finally:
            single.close()
            batched.close()


def test_live_plans_of_every_build(ps, dev):
    """The pattern of test_live_plans_with_different_lds_needs for the other two builds: plans whose notch takes R = 1 at 163 408
    bytes, R = 2 at 51 392 bytes and R = 4 (a 300 x 300 tile at sigma 250) are alive together and run in the order 1, 2, 4, 2, 1;
    every result equals what the plan gave before the others existed."""
    import torch
    r4 = dict(sigma=(250, 250), padding_mode="reflect", bidirectional=True)
    specs = {"R1": CASES["lds_edge_rows"][:2] + (THIN,), "R2": CASES["two_rows"][:2] + (WIDE,), "R4": ((300, 300), np.uint16, r4)}
    finest = {"R1": 1, "R2": 2, "R4": 4}
    tiles = {k: torch.from_numpy(U.synthetic_tile(shape, 50, dtype)[None]).to(dev) for k, (shape, dtype, _) in specs.items()}

    def plan_of(k):
        shape, dtype, kw = specs[k]
        return ps.Plan(dev, shape, dtype, ps.make_params(dtype, wavelet="db9", max_batch=1, **kw))

    first = {}
    for k in specs:
        plan = plan_of(k)
        assert min(r["R"] for r in plan.notch_routes()) == finest[k]
        first[k] = plan.run(tiles[k]).clone()
        torch.cuda.synchronize(dev)
        plan.close()
    plans = {k: plan_of(k) for k in specs}
    try:
        for k in ("R1", "R2", "R4", "R2", "R1"):
            got = plans[k].run(tiles[k])
            torch.cuda.synchronize(dev)
            assert torch.equal(got, first[k]), k
    finally:
        for plan in plans.values():
            plan.close()


@pytest.mark.parametrize("shape", [(16, 16400), (16400, 16)])
def test_refusal_behind_the_lds_edge(ps, dev, shape):
    """n = 8212 needs 164 400 bytes at R = 1: the plan is refused when it is made, by every entry, before anything is launched."""
    from ipp_amd import capi
    assert lds_request(8212, 10, 1) == 164400 > LDS_LIMIT
    img = U.synthetic_tile(shape, 7, np.uint16, "rows" if shape[0] < shape[1] else "cols")
    for call in (lambda: ps.Plan(dev, shape, np.uint16, ps.make_params(np.uint16, wavelet="db9", **THIN)),
                 lambda: ps.process_img(img, device=dev, wavelet="db9", **THIN),
                 lambda: ps.filter_streaks(img, device=dev, wavelet="db9", **THIN)):
        with pytest.raises(capi.MiError, match="does not fit the notch kernel") as e:
            call()
        assert e.value.code == capi.MI_ERR_UNSUPPORTED
        assert "8212 samples" in capi.last_error() and "8212 samples" in str(e.value)


@pytest.mark.parametrize("shape,levels,n,lds", [((2048, 2048), 7, 1326, 66176), ((1400, 1400), 6, 1002, 55872), ((300, 300), 5, 452, 28992)])
def test_the_other_suites_plans_take_four_lines(ps, dev, shape, levels, n, lds):
    """The plans of test_live_plans_with_different_lds_needs (tests/test_gpu_pystripe.py; the first is also test_pipeline_size_2048's):
    R = 4 at every level, and the finest level's LDS request that test's docstring quotes.  Plans only, nothing runs."""
    plan = ps.Plan(dev, shape, np.uint16, ps.make_params(np.uint16, sigma=(250, 250), wavelet="db9", padding_mode="reflect", bidirectional=True))
    try:
        routes = plan.notch_routes()
    finally:
        plan.close()
    report(f"{shape} sigma 250: {len(routes) // 2} levels, finest n {routes[0]['n']}, kp {routes[0]['kp']}, lds {routes[0]['lds']}; "
           f"R {sorted({r['R'] for r in routes})}")
    assert len(routes) == 2 * levels and {r["R"] for r in routes} == {4}
    # kp of these lines is not saturated (it sits on the last bit of expf), and one bin more or less moves the request by 64 bytes
    assert routes[0]["n"] == routes[1]["n"] == n and routes[0]["lds"] == routes[1]["lds"] == max(r["lds"] for r in routes)
    assert abs(routes[0]["lds"] - lds) <= 64


def test_routes_capacity(ps, dev):
    """mi_pystripe_plan_notch_routes: the record count, an error naming the capacity when it is too small, nothing for a plan
    without a filter."""
    import ctypes as C
    from ipp_amd import capi
    plan = make_plan(ps, dev, "one_two_pass")
    try:
        buf = (C.c_int * 36)()
        assert capi.lib().mi_pystripe_plan_notch_routes(plan._h, buf, 36) == 4
        assert list(buf[:4]) == [0, 1, 0, 2619] and list(buf[27:31]) == [1, 1, 1, 32]
        assert capi.lib().mi_pystripe_plan_notch_routes(plan._h, buf, 35) == capi.MI_ERR_INVALID
        assert "cap = 35" in capi.last_error() and "36" in capi.last_error()
    finally:
        plan.close()
    plain = ps.Plan(dev, (40, 50), np.uint16, ps.make_params(np.uint16, dark=3))
    try:
        assert plain.notch_routes() == []
    finally:
        plain.close()
