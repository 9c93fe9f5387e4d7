"""GPU: every kernel route of csrc/gauss3d.hip against the plain restatement of tests/gauss_util.py.

Each case asserts the route it means to cover (mi_gauss3d_route, the function the launch itself is decided by), filters random data in
[0, 1) with an anisotropic sigma in place and compares with the float64-per-pass restatement to gauss_util.gpu_tolerance: 4 x the
measured deviation of a float32 restatement (9.5e-7), never more than (kx + ky + kz) 2^-23 max|x|."""
import numpy as np
import pytest
import torch

from tests import gauss_util as U

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_gauss3d_route_matches_restatement(dev, case):
    from ipp_amd import decon
    c = U.CASES[case]
    x, k = U.case_input(case), U.case_ksize(c)
    assert decon.gauss3d_route(c["shape"], c["sigma"], c["ksize"]) == c["route"], U.ROUTE_NAMES[c["route"]]
    want = U.gauss3d(x, c["sigma"], c["ksize"])
    t = torch.from_numpy(x).to(dev)
    ptr = t.data_ptr()
    out = decon.gauss3d_gpu(t, c["sigma"], c["ksize"])
    # destructive in place on the single-pass routes (one copy back) and on the two-pass ones (gauss3d_gpu.cu:289-293)
    assert out is t and t.data_ptr() == ptr
    got = t.cpu().numpy()
    d, tol = float(np.abs(got.astype(np.float64) - want).max()), U.gpu_tolerance(k, float(x.max()))
    U.report(f"{case}: {U.ROUTE_NAMES[c['route']]}, k = {k}: max|d| {d:.4g} (allowed {tol:.4g})")
    assert np.isfinite(got).all()
    assert d <= tol
