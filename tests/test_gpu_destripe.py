"""GPU: mi_destripe_z (csrc/destripe.hip; filter_subband_3d_z.m) against the oracle restatement (parity
unpinned: MATLAB's Wavelet Toolbox is closed; see oracle/destripe_oracle.py) and against its float64 composition,
``filter_subband_3d_z_f64`` of tests/destripe_util.py.

Two bounds, neither taken from the code under test:
  * output domain: max |device - reference| <= TOL * max |reference|, TOL = 2e-5 (float32 filter sums of 18 taps over up to 4
    levels), 5 TOL where the notch spans many bins (sigma = 60).  The older tests hold it against the float32 oracle, the cases of
    destripe_util.CASES against the float64 reference, whose own share is a tenth of it (tests/test_destripe_util_host.py);
  * log domain: err = max |log1p(device) - log1p(float64 reference)| <= 4 e_ref, e_ref the float32 oracle's distance from the same
    float64 result, computed live.  The margin is that of tests/test_gpu_pystripe.py (the same kind of kernel against the same kind
    of reference).  Not applied where the output comes near or below zero (the volumes with exact zeros): the filter's error is
    absolute in the log domain, and the output-domain bound already weighs it by the volume's maximum there.
Every measured err, e_ref and ratio is printed before it is asserted (DESTRIPE_REPORT=<file> appends them to a file); the
recorded figures are in the docstring of test_destripe_cases_against_float64.  Every new case runs on a guarded view
(destripe_util.guarded) whose surroundings are checked after the call.

Left untested: the grid-stride loops of k_notch_bin / k_subtract (taken above 256 * 32 work-groups) and the single-chunk branch
of z_chunks() both need more than 2 M columns per plane -- over 600 MB of input and minutes of CPU reference."""
import numpy as np
import pytest
import torch

from oracle import destripe_oracle as D
from tests import destripe_util as U

pytestmark = pytest.mark.gpu
TOL = 2e-5
LOG_MARGIN = 4      # err <= LOG_MARGIN * e_ref (tests/test_gpu_pystripe.py)

_volume = U.striped


@pytest.mark.parametrize("shape", [(40, 3, 64), (72, 2, 136), (71, 2, 79), (70, 3, 68), (36, 1, 300)])
@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_destripe_matches_oracle(dev, shape, sigma):
    from ipp_amd import capi, decon
    vol = _volume(shape, 21)
    want = D.filter_subband_3d_z(vol, sigma)
    t = torch.from_numpy(vol).to(dev)
    got = decon.filter_subband_3d_z(t, sigma, 0, "db9")
    assert got is t
    got = got.cpu().numpy()
    assert np.abs(got - want).max() <= TOL * np.abs(want).max()
    px, pz = shape[2] + shape[2] % 2, shape[0] + shape[0] % 2
    assert capi.lib().mi_destripe_max_levels(shape[2], shape[0]) == D.wmaxlev((px, pz))


def test_destripe_explicit_levels_wide_notch_and_identity(dev):
    from ipp_amd import decon
    vol = _volume((72, 2, 136), 22)
    for levels in (1, 2):
        want = D.filter_subband_3d_z(vol, 2.0, levels)
        got = decon.filter_subband_3d_z(vol, 2.0, levels)          # numpy in -> numpy out
        assert isinstance(got, np.ndarray) and np.abs(got - want).max() <= TOL * np.abs(want).max()
    # sigma comparable to the coefficient count: the notch spans many bins (the general path of the filter)
    want = D.filter_subband_3d_z(vol, 60.0)
    got = decon.filter_subband_3d_z(vol, 60.0)
    assert np.abs(got - want).max() <= 5 * TOL * np.abs(want).max()
    # the stripes are what goes away
    prof = lambda v: np.std(v.mean(axis=(0, 1)))
    assert prof(decon.filter_subband_3d_z(vol, 2.0)) < 0.5 * prof(vol)
    # too small for one level (wmaxlev = 0): unchanged
    small = _volume((20, 2, 30), 23)
    assert np.array_equal(decon.filter_subband_3d_z(small, 2.0), small)
    with pytest.raises(ValueError):
        decon.filter_subband_3d_z(vol, 1.0, 0, "db4")


def test_process_block_with_destripe(dev):
    """process_block (LsDeconv.m:906-948) with destripe_sigma > 0: deconvolution, then the destripe filter, then the stats."""
    from ipp_amd import lsdeconv as L
    from oracle import rl_oracle as R
    psf = R.gaussian_psf((5, 5, 5), (1.0, 1.0, 1.0))
    vol = _volume((40, 8, 64), 24)
    filt = L.Filter((0.0, 0.0, 0.0), (0, 0, 0), 0.0, 2.0, 0, False, False)
    blk = L.Block(64, 8, 40, 1, 1, 1)
    out, lb, ub = L.process_block(vol, blk, psf, 2, 0.0, 0.0, filt, 99.99, 1)
    want = D.filter_subband_3d_z(R.decon_spatial(vol, psf, 2, 0.0, 0.0, 0), 2.0)
    assert np.abs(out.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()


# ---------------------------------------------------------------------------------- destripe_util.CASES against float64
_RESULTS = {}   # case id -> the device's result on the 16-byte aligned view (float64 copy), for the unaligned comparison


def _run_case(dev, case, offset=0):
    """One case on a guarded view ``offset`` elements past a 16-byte boundary; returns (device result as float64, e_ref)."""
    from ipp_amd import capi, decon
    c = U.CASES[case]
    vol, ref32, ref64 = U.reference(case)
    buf, view = U.guarded(vol, dev, offset=offset)
    out = decon.filter_subband_3d_z(view, c["sigma"], c["levels"], "db9")
    assert out is view                                                          # 1. in place
    torch.cuda.synchronize(dev)
    U.assert_guards_intact(buf, view)                                           # 2. nothing next to the block is written
    got = out.cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref64).max())
    d = float(np.abs(got - ref64).max())
    tol = c["tol_factor"] * TOL
    U.report(f"{case}+{offset}: output domain max|d| {d:.3g} = {d / scale:.3g} of max|ref| (allowed {tol:g})")
    assert np.isfinite(got).all()
    assert d <= tol * scale                                                     # 3. output domain
    e_ref = None
    # log1p is ill-conditioned near -1 and the volumes with exact zeros put outputs near and below zero: those cases stand on
    # the output-domain bound alone, and so would over_levels if the reference's minimum fell below -0.5 (it is 0.476)
    if c["log_domain"] and ref64.min() > -0.5:
        err, e_ref = U.log_distance(got, ref64), U.log_distance(ref32, ref64)
        U.report(f"{case}+{offset}: log domain, device vs float64 reference {err:.3g}, e_ref (float32 oracle) {e_ref:.3g}, "
                 f"ratio {err / e_ref:.2f} (allowed {LOG_MARGIN})")
        assert err <= LOG_MARGIN * e_ref                                        # 4. log domain
    if not c["levels"]:                                                         # 5. the level count of the C ABI
        z, _, x = c["shape"]
        assert capi.lib().mi_destripe_max_levels(x, z) == D.wmaxlev((x + x % 2, z + z % 2)) == c["nlev"]
    return got, e_ref


def _aligned_result(dev, case):
    if case not in _RESULTS:
        _RESULTS[case] = _run_case(dev, case)[0]
    return _RESULTS[case]


@pytest.mark.parametrize("case", list(U.CASES))
def test_destripe_cases_against_float64(dev, case):
    """Multi-tile x passes (wide_*, two_tiles), 3 and 4 levels, the multi-bin notch on odd coefficient counts, 19 z chunks,
    exact zeros, explicit levels above wmaxlev; what each shape reaches is asserted in tests/test_destripe_util_host.py.

    ``growing`` / ``growing_notch`` are the cases that found a defect: with extents below lf - 1 and explicit levels the
    coefficient counts grow from level to level, and the scratch shared by the levels (sized for level 1) was overrun by
    k_dwt_z at level 2 and by the notch's sum at level 1; mi_destripe_z now sizes it for the largest level.

    Recorded figures, log domain (err / e_ref = ratio, allowed 4).  These come from destripe.hip compiled for the HOST (kernels
    run serially, fused multiply-adds on, under AddressSanitizer), not from an MI355X, where they are NOT YET MEASURED; the
    device's log1pf / expm1f may move them:
      wide_even 4.22e-07 / 2.54e-07 = 1.66   wide_odd 4.50e-07 / 2.76e-07 = 1.63   two_tiles 3.81e-07 / 2.59e-07 = 1.47
      deep3 6.45e-07 / 4.17e-07 = 1.55       deep4 7.77e-07 / 5.17e-07 = 1.50      tall 3.50e-07 / 2.70e-07 = 1.30
      odd_wide_notch 5.39e-07 / 3.19e-07 = 1.69   odd_wide_notch_b 4.46e-07 / 3.51e-07 = 1.27
      over_levels 5.49e-07 / 3.71e-07 = 1.48   multi_reflect 3.16e-07 / 2.13e-07 = 1.48   growing 4.59e-07 / 3.23e-07 = 1.42
      growing_notch 3.58e-07 / 2.51e-07 = 1.43   base_1level 3.43e-07 / 2.39e-07 = 1.44   base_2level 4.96e-07 / 3.38e-07 = 1.47
    Output domain, same run: 5.7e-07 to 1.7e-06 of the maximum (allowed 2e-05)."""
    _RESULTS[case] = _run_case(dev, case)[0]


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("case", ["base_1level", "base_2level"])
def test_destripe_unaligned_base(dev, case, offset):
    """cols % 4 == 0 with a base 4, 8 or 12 bytes past a 16-byte boundary: k_dwt_z<., 1> where the aligned view takes <., 4>.  Same
    bounds; the two instantiations need not agree bit for bit (the compiler may contract their sums differently), but only the
    rounding of the level-1 z sums can differ, which is a part of what e_ref measures on the oracle's side: within 2 e_ref of
    each other in the log domain."""
    aligned = _aligned_result(dev, case)
    got, e_ref = _run_case(dev, case, offset)
    between = U.log_distance(got, aligned)
    U.report(f"{case}+{offset}: log domain, offset vs aligned view {between:.3g} = {between / e_ref:.2f} e_ref (allowed 2)")
    assert between <= 2 * e_ref


def test_destripe_identity_on_a_guarded_view(dev):
    """Too small for one level (wmaxlev = 0): the block comes back bit for bit, nothing around it is touched."""
    from ipp_amd import decon
    small = U.striped((20, 2, 30), 23)
    for offset in (0, 1):
        buf, view = U.guarded(small, dev, offset=offset)
        assert decon.filter_subband_3d_z(view, 2.0) is view
        torch.cuda.synchronize(dev)
        U.assert_guards_intact(buf, view)
        assert np.array_equal(view.cpu().numpy().view(np.uint32), small.view(np.uint32))


def test_destripe_refusals_leave_the_library_usable(dev):
    from ipp_amd import capi, decon
    vol = U.reference("base_1level")[0]

    def still_right():
        _run_case(dev, "base_1level")

    buf, view = U.guarded(vol, dev)
    with pytest.raises(capi.MiError, match="levels must be >= 0") as e:
        decon.filter_subband_3d_z(view, 2.0, -1)
    assert e.value.code == capi.MI_ERR_INVALID
    torch.cuda.synchronize(dev)
    U.assert_guards_intact(buf, view)
    assert np.array_equal(view.cpu().numpy(), vol)                              # a refused call leaves the block alone
    still_right()
    wide = torch.from_numpy(vol).to(dev)
    with pytest.raises(ValueError, match="contiguous"):
        decon.filter_subband_3d_z(wide[:, :, ::2], 2.0)
    with pytest.raises(ValueError, match="contiguous"):
        decon.filter_subband_3d_z(wide.permute(2, 1, 0), 2.0)
    still_right()
    with pytest.raises(TypeError, match="float32"):
        decon.filter_subband_3d_z(wide.double(), 2.0)
    still_right()
    with pytest.raises(ValueError, match="3D"):
        decon.filter_subband_3d_z(wide[:, 0, :].contiguous(), 2.0)
    still_right()
    assert np.array_equal(wide.cpu().numpy(), vol)
