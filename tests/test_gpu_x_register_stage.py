"""GPU: the rotated x position order of the spectrum arrays and the bottom radix-8 super-stage of the fused x pass on the registers
of its global access (fft_native.hip: NativeDims::xrot, k_x_fused_pipe REG; reference chain decon.m:162-186).

The persistent kernel and the unpipelined kernels (MI_FFT_NO_XPIPE=1: k_x_forward / k_x_inverse, every stage in LDS) read and write
the same position order and run the same butterflies on the same operands in the same order, so their results are compared for
EQUALITY, bit for bit, not within a tolerance."""
import numpy as np
import pytest
import torch

from oracle import rl_oracle as R
from tests.rl_util import assert_close, asymmetric_psf
from tests.slab_util import lockstep_iterate

pytestmark = pytest.mark.gpu

KSHAPE = (5, 7, 9)


def _psfs(symmetric):
    if symmetric:
        return R.gaussian_psf(KSHAPE, (1.0, 1.5, 2.0)), None
    psf = asymmetric_psf(KSHAPE, seed=17)
    return psf, np.ascontiguousarray(psf[::-1, ::-1, ::-1])


def _both_routes(shape, psf, psf_inv, boundary, vol, iters, monkeypatch):
    """`iters` fused iterations on `vol`: (persistent kernel, unpipelined kernels), one context each."""
    from ipp_amd import capi, decon
    dev = torch.device("cuda", 0)
    out = []
    for unpipelined in (False, True):
        if unpipelined:
            monkeypatch.setenv("MI_FFT_NO_XPIPE", "1")
        ctx = decon.RLContext(shape, psf, psf_inv, boundary=boundary, engine=capi.ENGINE_FFT, device=dev)
        assert ctx.fuses
        bl = torch.from_numpy(vol).to(dev)
        ctx.iterate(bl, None, iters)
        torch.cuda.synchronize()
        out.append(bl.cpu())
        if unpipelined:
            monkeypatch.delenv("MI_FFT_NO_XPIPE")
    return out


# (z, y, x): Hx = x / 2 = 1024 (tiles of 16 rows, rows private to their waves) and 2048 (tiles of 8 rows): the rotated order;
# x = 1536 (Hx = 3 * 256) keeps positions = working indices
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("shape", [(64, 32, 2048), (64, 32, 4096), (64, 32, 1536)])
def test_register_stage_equals_lds_stages_bit_for_bit(dev, shape, symmetric, monkeypatch):
    from ipp_amd import capi
    psf, inv = _psfs(symmetric)
    vol = R.bead_volume(shape, seed=sum(shape), psf=R.gaussian_psf(KSHAPE, (1.0, 1.5, 2.0)))
    pipe, lds = _both_routes(shape, psf, inv, capi.BOUNDARY_CIRCULAR, vol, 3, monkeypatch)
    assert torch.isfinite(pipe).all() and float(pipe.abs().max()) > 0
    assert torch.equal(pipe, lds), f"largest difference {float((pipe - lds).abs().max()):.3e}"


def test_register_stage_matches_the_oracle(dev, monkeypatch):
    """(equality of two routes of one library says nothing about a mistake they share: the rotated order against float64, with
    an asymmetric PSF -- complex OTF, adjoint = its conjugate)"""
    from ipp_amd import capi
    shape = (16, 32, 2048)
    psf = asymmetric_psf(KSHAPE, seed=17)
    vol = R.bead_volume(shape, seed=5, psf=R.gaussian_psf(KSHAPE, (1.0, 1.5, 2.0)))
    pipe, lds = _both_routes(shape, psf, None, capi.BOUNDARY_CIRCULAR, vol, 3, monkeypatch)
    want = R.decon_fft(vol, psf, shape, 3, skip_edgetaper=True)
    assert_close(pipe.numpy(), want)
    assert_close(lds.numpy(), want)


@pytest.mark.parametrize("symmetric", [True, False])
def test_register_stage_on_a_padded_grid(dev, symmetric, monkeypatch):
    """Zero rule: a volume of 50 x 24 x 2000 on the grid 64 x 32 x 2048 (Hx = 1024); the persistent kernel enumerates the live
    tiles only, the unpipelined kernels crop row by row."""
    from ipp_amd import capi
    monkeypatch.setenv("MI_FFT_NATIVE_INFLATE", "100")
    vshape = (50, 24, 2000)
    psf, inv = _psfs(symmetric)
    vol = R.bead_volume(vshape, seed=9, psf=R.gaussian_psf(KSHAPE, (1.0, 1.5, 2.0)))
    pipe, lds = _both_routes(vshape, psf, inv, capi.BOUNDARY_ZERO, vol, 3, monkeypatch)
    assert torch.isfinite(pipe).all() and float(pipe.abs().max()) > 0
    assert torch.equal(pipe, lds), f"largest difference {float((pipe - lds).abs().max()):.3e}"


def test_register_stage_two_rank_slabs_against_the_unsharded_context(dev, monkeypatch):
    """Two slabs along y exchange x-transformed halo rows line by line (positions, whatever their order): both ranks build the
    rotated order, and the sharded run reproduces the unsharded context and the oracle."""
    from ipp_amd import capi, decon, slab
    monkeypatch.setenv("MI_FFT_NATIVE_INFLATE", "100")
    shape = (16, 64, 2048)
    psf = R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0))
    vol = R.bead_volume(shape, seed=41, psf=psf)
    slabs = [slab.SlabRL(vol.shape, psf, rank=r, world_size=2, device=dev, flavour="fft", engine=2, volume=vol) for r in range(2)]
    assert all(s.sharded for s in slabs)
    got = lockstep_iterate(slabs, 3).cpu().numpy()
    ctx = decon.RLContext(shape, psf, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
    bl = torch.from_numpy(vol).to(dev)
    ctx.iterate(bl, None, 3)
    assert_close(got, bl.cpu().numpy().astype(np.float64), rel=2e-5)  # (test_gpu_slab.py: sharded against unsharded)
    assert_close(got, R.decon_fft(vol, psf, vol.shape, 3, skip_edgetaper=True))
