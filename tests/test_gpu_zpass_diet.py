"""GPU: the paired z pass (k_z_pair_pipe) after its integer diet -- the full-grid form without plane bounds, the z ramp as contiguous
loads, the plane twiddle from a table -- computes what it computed before, bit for bit.

No floating-point expression changed, so there is no tolerance here: every case of tests/zpass_diet_util.py must reproduce what
tests/golden/zpass_parent/record.py recorded on the GPU at the parent commit (arrays for 64-point lines, SHA-256 digests for the rest).
A difference is a finding to explain."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import rl_oracle as R
from tests import zpass_diet_util as Z

pytestmark = pytest.mark.gpu

CASES = Z.cases()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(Z.GOLDEN, "digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,case", CASES, ids=[cid for cid, _ in CASES])
def test_bit_for_bit_against_the_parent(dev, cid, case, recorded):
    ins = Z.inputs(case)
    assert Z.digest(*ins) == recorded[cid]["inputs"], "the inputs differ from the recorded ones: the random streams changed, not the kernel"
    ctx = Z.make_ctx(case, dev)
    # circular grids take the full-grid form; the padded ones prune z planes (50 of 64 hold data) and keep the predicated form
    assert ctx.z_full_grid == (case["kind"] == "circular"), (ctx.z_full_grid, ctx.fft_route)
    assert ctx.fft_route["pruned"] == int(case["kind"] != "circular")
    if case["kind"] == "adjoint":
        assert ctx.otf_form["rank_adj"] >= 1
    res = Z.run(ctx, ins, dev)
    ctx.close()
    if case["kind"] == "circular" and case["shape"][0] == 64:
        want = np.load(os.path.join(Z.GOLDEN, f"{cid}.npy"))
        for name, got, w in zip(Z.NAMES, res, want):
            assert np.array_equal(got, w), f"{cid} {name}: {int((got != w).sum())} of {w.size} values differ, max |d| {np.abs(got - w).max():.3e}"
    for name, got in zip(Z.NAMES, res):
        assert Z.digest(got) == recorded[cid][name], f"{cid} {name}"


@pytest.mark.parametrize("nz", [64, 512])
def test_general_form_switch_is_bit_identical(dev, nz):
    """MI_FFT_Z_GENERAL=1 keeps the predicated form on a full grid: same results, and the route says which form ran."""
    case = dict(shape=(nz, 16, 32), form="factored", kind="circular")
    ins = Z.inputs(case)
    full = Z.make_ctx(case, dev)
    general = Z.make_ctx(case, dev, {"MI_FFT_Z_GENERAL": "1"})
    assert full.z_full_grid is True and general.z_full_grid is False
    assert full.fft_route == general.fft_route   # (nothing else moves)
    for name, a, b in zip(Z.NAMES, Z.run(full, ins, dev), Z.run(general, ins, dev)):
        assert np.array_equal(a, b), name
    full.close()
    general.close()


# (64, 16, 32): planes 0 and X/4 are their own partners.  (128, 32, 16): 5 planes x 4 tiles.  (64, 512, 128): 33 x 64 = 2112 tiles, more
# than the two work-groups per CU of any device: a work-group takes several tiles and the counter runs past the launch's first round
@pytest.mark.parametrize("shape", [(64, 16, 32), (128, 32, 16), (64, 512, 128)])
def test_mirror_planes_and_last_tile_under_both_hand_outs(dev, shape):
    from ipp_amd import capi, decon
    psf = R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0))
    vol = torch.from_numpy(R.bead_volume(shape, seed=23, psf=psf)).to(dev)
    got = []
    for dyn in ("0", "1"):
        with Z.switches({"MI_Z_DYN": dyn}):
            ctx = decon.RLContext(shape, psf, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
        assert ctx.fft_route["z_kernel"] == 2 and ctx.fft_route["z_dynamic"] == int(dyn) and ctx.z_full_grid
        bl = vol.clone()
        ctx.iterate(bl, None, 3)
        ctx.close()
        got.append(bl)
    assert torch.equal(got[0], got[1])
    assert bool(torch.isfinite(got[0]).all())
