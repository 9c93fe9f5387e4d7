"""Host: the restatement of tests/gauss_util.py against the oracle (odd sizes) and against a literal triple loop (even sizes), the
measured float32-form deviation that the GPU tolerance of tests/test_gpu_gauss3d.py rests on, and the kernel route of
csrc/gauss3d.hip that every case of that module is meant to reach (mi_gauss3d_route is host arithmetic: no device needed)."""
import numpy as np
import pytest

from oracle import rl_oracle as R
from tests import gauss_util as U


@pytest.fixture(scope="module")
def decon():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import decon
    return decon


@pytest.mark.parametrize("shape,sigma,ksize", [((6, 7, 9), [0.8, 1.3, 0.6], [5, 7, 3]), ((20, 33, 47), [1.5, 1.5, 2.5], [9, 11, 15]),
                                               ((4, 5, 70), 8, 51), ((9, 8, 7), 0.5, None), ((3, 1, 4), [0.5, 0.5, 2.5], [13, 13, 25])])
def test_restatement_is_the_oracle_for_odd_sizes(shape, sigma, ksize):
    x = np.random.default_rng(3).random(shape, dtype=np.float32)
    got, want = U.gauss3d(x, sigma, ksize), R.gauss3d(x, sigma, ksize)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    s3 = [sigma] * 3 if np.isscalar(sigma) else sigma
    k3 = R.default_ksize(s3) if ksize is None else ([ksize] * 3 if np.isscalar(ksize) else ksize)
    assert U.default_ksize(s3) == R.default_ksize(s3)
    for s, k in zip(s3, k3):
        assert np.array_equal(U.taps(s, k), R.gaussian_taps(s, k))


def test_even_taps_follow_make_gaussian_kernel():
    # 4 taps: the loop writes exp(-i^2 / (2 s^2)) for i = -2 .. 2 and sums all five; the first four are kept
    s2 = float(np.float32(np.float32(1.3) * np.float32(1.3)))
    e = [np.float32(np.exp(-0.5 * i * i / s2)) for i in (-2, -1, 0, 1, 2)]
    total = sum(float(v) for v in e)
    w = U.taps(1.3, 4)
    assert w.dtype == np.float32 and len(w) == 4
    assert np.array_equal(w, np.array([np.float32(float(v) / total) for v in e[:4]], np.float32))
    assert w[2] == w.max() and w[1] == w[3] and w.sum() < 1.0 - float(e[4]) / total + 1e-6   # centre at s = k / 2; not normalised to 1
    assert np.array_equal(U.taps(0.7, 5), R.gaussian_taps(0.7, 5))


@pytest.mark.parametrize("ksize", [[4, 2, 6], [2, 2, 2], [6, 5, 4]])
def test_even_restatement_is_the_literal_triple_loop(ksize):
    x = np.random.default_rng(5).random((3, 4, 5), dtype=np.float32)
    sigma = U.case_sigma(ksize)
    assert np.array_equal(U.gauss3d(x, sigma, ksize), U.gauss3d_triple_loop(x, sigma, ksize))


def _shift_shows(case):
    """An even size along y or z on an axis longer than one sample (on an axis of one sample every window reads that sample)."""
    (nz, ny, _), (_, ky, kz) = U.CASES[case]["shape"], U.CASES[case]["ksize"]
    return (ky % 2 == 0 and ny > 1) or (kz % 2 == 0 and nz > 1)


def test_which_even_cases_can_see_the_shift():
    assert [c for c in U.EVEN_CASES if not _shift_shows(c)] == ["one_line_even"] and len(U.EVEN_CASES) == 9


@pytest.mark.parametrize("case", [c for c in U.EVEN_CASES if _shift_shows(c)])
def test_even_cases_can_see_a_window_shifted_by_one_sample(case):
    """The ring kernels once took the window yo - r + 1 .. yo + r for an even size (the y and z filters; x was right): on the GPU
    test's own inputs that result is thousands of tolerances away from the reference's window."""
    c = U.CASES[case]
    x, k = U.case_input(case), U.case_ksize(c)
    shift = [0, int(k[1] % 2 == 0), int(k[2] % 2 == 0)]
    assert any(shift), case
    want, shifted = U.gauss3d(x, c["sigma"], k), U.gauss3d(x, c["sigma"], k, shift=shift)
    d, tol = float(np.abs(want.astype(np.float64) - shifted).max()), U.gpu_tolerance(k, float(x.max()))
    U.report(f"{case}: window shifted by one sample differs by {d:.3g} = {d / tol:.0f} x the GPU tolerance {tol:.3g}")
    assert d > 1000 * tol


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_fp32_form_stays_within_the_measured_deviation(case):
    c = U.CASES[case]
    x, k = U.case_input(case), U.case_ksize(c)
    assert x.dtype == np.float32 and x.shape == c["shape"] and 0.0 <= x.min() and x.max() < 1.0
    want = U.gauss3d(x, c["sigma"], c["ksize"])
    form = U.gauss3d(x, c["sigma"], c["ksize"], acc_dtype=np.float32)
    d = float(np.abs(want.astype(np.float64) - form).max())
    U.report(f"{case}: k = {k}, float32 form vs float64-per-pass restatement max|d| {d:.4g} (FP32_FORM_DEV {U.FP32_FORM_DEV:.4g}, "
             f"GPU tolerance {U.gpu_tolerance(k, float(x.max())):.4g}, hard cap {U.hard_cap(k, float(x.max())):.4g})")
    assert d <= U.FP32_FORM_DEV
    assert U.gpu_tolerance(k, float(x.max())) <= U.hard_cap(k, float(x.max()))
    assert U.gpu_tolerance(k, float(x.max())) <= U.GPU_FACTOR * U.FP32_FORM_DEV < 5e-5 / 50


def test_measured_deviation_is_reached():
    """FP32_FORM_DEV is the measured maximum, not a rounded-up guess: some case attains it."""
    worst = 0.0
    for case in ("ring_51", "ring_13_13_27", "patch_budget_outside"):
        c = U.CASES[case]
        x = U.case_input(case)
        d = np.abs(U.gauss3d(x, c["sigma"], c["ksize"]).astype(np.float64) - U.gauss3d(x, c["sigma"], c["ksize"], acc_dtype=np.float32))
        worst = max(worst, float(d.max()))
    assert worst == U.FP32_FORM_DEV


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_case_reaches_its_route(decon, case):
    c = U.CASES[case]
    assert decon.gauss3d_route(c["shape"], c["sigma"], c["ksize"]) == c["route"], U.ROUTE_NAMES[c["route"]]


def test_every_route_and_every_built_kernel_has_a_case(decon):
    assert {c["route"] for c in U.CASES.values()} == set(U.ROUTE_NAMES) == set(range(1, 8))
    by_route = {}
    for c in U.CASES.values():
        by_route.setdefault(c["route"], []).append(U.case_ksize(c))
    for r in (U.WAVE1, U.WAVE2):
        assert {k[2] for k in by_route[r]} == {3, 5, 7}                                    # k_gauss3d_wave<KZ, WX>
    built = set(range(3, 26, 2))
    assert {k[0] for k in by_route[U.WIN_WIN] + by_route[U.WIN_RING]} == built            # k_gauss_xy_win<N>
    assert {k[2] for k in by_route[U.WIN_WIN] + by_route[U.RING_WIN]} >= built            # k_gauss_z_win<N>
    # the route flips at the two budgets of the single pass, and rows that are no whole float4 never fuse
    assert decon.gauss3d_route((21, 19, 68), 1.0, [11, 13, 11]) == U.FUSED and decon.gauss3d_route((21, 19, 68), 1.0, [11, 11, 13]) == U.WIN_WIN
    assert decon.gauss3d_route((131, 17, 68), 1.0, [25, 19, 3]) == U.FUSED and decon.gauss3d_route((131, 17, 68), 1.0, [25, 21, 3]) == U.RING_WIN
    assert decon.gauss3d_route((9, 9, 68), 1.0, [5, 5, 5]) == U.WAVE1 and decon.gauss3d_route((9, 9, 70), 1.0, [5, 5, 5]) == U.WIN_WIN
    assert decon.gauss3d_route((9, 9, 512), 0.5) == U.WAVE2 and decon.gauss3d_route((9, 9, 508), 0.5) == U.WAVE1
    # the production filters: the regularisation step and the pre-filter
    assert decon.gauss3d_route((64, 64, 64), 0.5) == U.WAVE1 and decon.gauss3d_route((64, 64, 64), [0.5, 0.5, 2.5], [13, 13, 25]) == U.WIN_WIN
    assert decon.gauss3d_route((8, 8, 8), 1.5) == U.FUSED


def test_route_refuses_what_the_filter_refuses(decon):
    from ipp_amd import capi
    with pytest.raises(capi.MiError, match="MAX_KERNEL_SIZE"):
        decon.gauss3d_route((8, 8, 8), 1.0, 53)
    with pytest.raises(capi.MiError, match="sigma"):
        decon.gauss3d_route((8, 8, 8), 0.0)
    with pytest.raises(ValueError):
        decon.gauss3d_route((8, 8), 1.0)
