"""Host: the float64 reference of tests/destripe_util.py against the float32 oracle, and the paths of csrc/destripe.hip that the
shapes of tests/test_gpu_destripe.py are meant to reach, derived from the kernel's constants restated in destripe_util.

The GPU tests allow the device TOL = 2e-5 of the volume's maximum; the reference side may use a tenth of that, so the float32
oracle and the float64 reference must agree to 2e-6 of the maximum at every case (measured 3.7e-7 to 1.13e-6)."""
import numpy as np
import pytest

from oracle import destripe_oracle as D
from tests import destripe_util as U

REF_SHARE = 2e-6   # TOL / 10


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_float32_oracle_agrees_with_float64_reference(case):
    c = U.CASES[case]
    vol, ref32, ref64 = U.reference(case)
    assert vol.dtype == np.float32 and ref32.dtype == np.float32 and ref64.dtype == np.float64
    assert vol.shape == c["shape"] == ref32.shape == ref64.shape
    d = float(np.abs(ref32.astype(np.float64) - ref64).max())
    scale = float(np.abs(ref64).max())
    U.report(f"{case}: float32 oracle vs float64 reference max|d| {d:.3g} = {d / scale:.3g} of max|ref| (allowed {REF_SHARE:g}), "
             f"log domain {U.log_distance(ref32, ref64):.3g}, ref min {ref64.min():.3g}")
    assert np.isfinite(ref64).all()
    assert d <= REF_SHARE * scale


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_level_count(case):
    c = U.CASES[case]
    z, _, x = c["shape"]
    padded = (x + x % 2, z + z % 2)
    assert (c["levels"] or D.wmaxlev(padded)) == c["nlev"]
    if case in ("over_levels", "multi_reflect", "growing", "growing_notch"):
        assert c["levels"] > D.wmaxlev(padded)
    else:
        assert c["levels"] == 0


def test_builders():
    v = U.striped((5, 2, 15), 3)
    assert v.dtype == np.float32 and 0.5 <= v.min() and v.max() < 0.7 * 1.5 + 1e-6
    assert (v[..., ::7] >= 0.75 - 1e-6).all() and (v[..., 1:7] < 0.7).all()
    w = U.striped_with_zeros((40, 5, 70), 3)
    share = float((w == 0).mean())
    assert w.dtype == np.float32 and 0.25 < share < 0.35 and w.min() == 0.0 and 1.0 < w.max() < 1.5
    assert np.array_equal(w, U.striped_with_zeros((40, 5, 70), 3))


def test_wide_cases_reach_the_multi_tile_paths():
    for case in U.WIDE:
        nx = U.CASES[case]["shape"][2]
        tiles, interior = U.x_analysis_tiles(nx)
        assert tiles >= 3 and interior >= 1, (case, tiles, interior)
        assert U.x_synthesis_tiles(nx) >= 2, case
    assert U.x_analysis_tiles(2100) == (3, 1) and U.x_synthesis_tiles(2100) == 5
    # exactly two analysis tiles and no interior segment: the last tile reflects and pads
    assert U.x_analysis_tiles(1030) == (2, 0) and U.x_synthesis_tiles(1030) >= 2
    # every older shape of the module stays on one tile of both passes
    for nx in (64, 136, 79, 68, 300):
        assert U.x_analysis_tiles(nx) == (1, 0) and U.x_synthesis_tiles(nx) == 1
    # V = 4 needs cols % 4 == 0
    assert (1 * 2100) % 4 == 0 and (2 * 2101) % 4 != 0


def test_coefficient_counts_the_cases_claim():
    assert U.coefficient_counts(140, 3) == [78, 47, 32]                       # deep3, along z
    assert U.coefficient_counts(74, 2) == [45, 31]                            # odd_wide_notch: odd, odd
    assert U.coefficient_counts(70, 2) == [43, 30]                            # odd_wide_notch_b: odd, even
    assert U.coefficient_counts(72, 2) == [44, 30]                            # the module's older sigma = 60 case: even, even
    assert U.coefficient_counts(40, 3) == [28, 22, 19]                        # over_levels
    assert min(U.CASES["multi_reflect"]["shape"][0::2]) < U.LF - 1            # shorter than the extension: reflects twice
    assert U.coefficient_counts(12, 3) == [14, 15, 16]                        # growing: every level larger than the one before
    n = U.coefficient_counts(12, 2)                                           # growing_notch: several bins at both levels
    assert all(int((D.gaussian_notch_filter_1d(m, 8.0 / m) != 1.0).sum()) >= 3 for m in n)


def test_notch_spans_several_bins_on_the_odd_counts():
    for case in ("odd_wide_notch", "odd_wide_notch_b"):
        c = U.CASES[case]
        for n in U.coefficient_counts(c["shape"][0], 2):
            g = D.gaussian_notch_filter_1d(n, max(c["sigma"] / n, float(D.EPS_SINGLE)))
            assert int((g != 1.0).sum()) >= 10, (case, n)
    # sigma = 2 on the same counts: one bin
    for n in (45, 31):
        assert int((D.gaussian_notch_filter_1d(n, 2.0 / n) != 1.0).sum()) == 1


def test_tall_case_z_chunks():
    z, y, x = U.CASES["tall"]["shape"]
    m = (z + U.LF - 1) // 2
    assert U.z_chunk_grid(y * x, m) == (17, 19) and m - 18 * 17 == 2          # analysis: 19 chunks of 17, the last of 2
    assert U.z_chunk_grid(y * x, (z + 1) // 2) == (17, 18)                    # synthesis
    assert U.z_chunk_grid(2 * 136, (72 + 17) // 2)[1] == 2                    # the tallest older column: 2 chunks
