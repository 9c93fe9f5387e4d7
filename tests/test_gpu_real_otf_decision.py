"""GPU: the decision of NativeFft::try_real_otf (fft_native_yz.hip) on PSFs around its threshold.

A PSF that is symmetric up to eps * (an antisymmetric pattern) gets the real form of the OTF, imaginary part dropped, when the
imaginary part left after removing the centre sample's phase ramp is at most 4e-6 of the real part.  Whatever the context decides,
its two convolutions and its fused iterations must match the float64 chain with the full OTF of that float32 PSF under the bounds
of the exact cases (tests/test_gpu_pair_layout.py); tests/test_real_otf_threshold_host.py shows the float64 cost of the dropped
part is at most a fifth of them.  The form itself is asserted only where the margin is wide."""
import numpy as np
import pytest
import torch

from oracle import rl_oracle as R
from tests import real_otf_util as U
from tests import spectral_util as S
from tests.rl_util import assert_close
from tests.test_gpu_pair_layout import _conv_pair

pytestmark = pytest.mark.gpu

assert U.PLAIN_SHAPE in S.CTX_SHAPES
# (shape, MI_FFT_NO_PAIR, pair_layout the context must report)
LAYOUTS = [(U.PAIRED_SHAPE, False, True), (U.PLAIN_SHAPE, False, False), (U.PAIRED_SHAPE, True, False)]
IDS = ["paired", "plain", "paired_shape_no_pair"]


@pytest.fixture(scope="module")
def beads():
    """Per shape: the bead volume of the iteration case (its blur is the symmetric member of the family)."""
    return {shape: R.bead_volume(shape, seed=5, psf=R.gaussian_psf(U.KSHAPE, U.SIGMA)) for shape in {U.PAIRED_SHAPE, U.PLAIN_SHAPE}}


@pytest.mark.parametrize("eps", U.EPS)
@pytest.mark.parametrize("shape,no_pair,paired", LAYOUTS, ids=IDS)
def test_convolutions_and_iterations_match_float64_on_either_side_of_the_threshold(dev, shape, no_pair, paired, eps, beads, monkeypatch):
    from ipp_amd import capi, decon
    psf = U.psf_family(eps)
    if no_pair:
        monkeypatch.setenv("MI_FFT_NO_PAIR", "1")
    ctx = decon.RLContext(shape, psf, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
    monkeypatch.delenv("MI_FFT_NO_PAIR", raising=False)
    assert ctx.engine == capi.ENGINE_FFT and ctx.pair_layout == paired
    ratio, _ = U.imag_ratio(psf, shape)
    print(f"{shape} no_pair={no_pair} eps {eps:g}: max|Im|/max|Re| {ratio:.3e} ({ratio / U.THRESHOLD:.2f} x threshold), otf_is_real {ctx.otf_is_real}")
    if eps == 0 and paired:
        assert ctx.otf_is_real          # (as test_paired_layout_equals_plain_layout_and_float64 requires)
    if eps >= 1e-4:
        assert ratio > 10 * U.THRESHOLD and not ctx.otf_is_real
    an, bn = U.operands(shape)
    a, b = torch.from_numpy(an).to(dev), torch.from_numpy(bn).to(dev)
    fwd, adj = _conv_pair(ctx, a, b)
    want_f, want_a = U.circular_pair(an, bn, R.otf_from_psf(psf, shape))
    for name, got, want in (("forward", fwd, want_f), ("adjoint", adj, want_a)):
        print(f"  {name}: max %.2e  l2 %.2e  point-wise %.2f x" % U.errors(got.astype(np.float64), want))
        assert_close(got, want, what=name, **U.BOUNDS)
    vol = beads[shape]
    want = R.decon_fft(vol, psf, shape, 5, skip_edgetaper=True)
    bl = torch.from_numpy(vol).to(dev)
    ctx.iterate(bl, None, 5)
    assert_close(bl.cpu().numpy(), want, what="5 iterations")
    ctx.close()


# what mi_rl_fft_route must report for a circular context with the symmetric 5 x 7 x 5 Gaussian PSF: (64, 64, 128) is in the paired
# range of z, (32, 64, 128) below it (and its 32-point lines cannot take the real OTF in k_z_conv_pipe); tiles 16 / 16 / 16 on both
ROUTE_SHAPES = [(64, 64, 128), (32, 64, 128)]
ROUTE_SWITCHES = [None, "MI_FFT_NO_PAIR", "MI_FFT_NO_PIPE", "MI_FFT_NO_XPIPE", "MI_FFT_COMPLEX_OTF"]


def _expected_route(shape, switch):
    in_pair_range = shape[0] == 64
    paired = int(in_pair_range and switch not in ("MI_FFT_NO_PAIR", "MI_FFT_NO_PIPE"))
    piped = int(switch != "MI_FFT_NO_PIPE")
    return dict(native=1, paired=paired, z_kernel=2 if paired else piped, real_otf=int(in_pair_range and piped and switch != "MI_FFT_COMPLEX_OTF"),
                x_pipelined=int(piped and switch != "MI_FFT_NO_XPIPE"), x_splits=piped, x_dynamic=1, z_dynamic=1, pruned=0, ty=16, tc=16, tl=16)


@pytest.fixture(scope="module")
def default_route_results():
    """Per shape: (volume, three fused iterations of a context created without any switch), computed once."""
    from ipp_amd import capi, decon
    dev = torch.device("cuda", 0)
    psf = R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0))
    out = {}
    for shape in ROUTE_SHAPES:
        vol = torch.from_numpy(R.bead_volume(shape, seed=23, psf=psf)).to(dev)
        ctx = decon.RLContext(shape, psf, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
        bl = vol.clone()
        ctx.iterate(bl, None, 3)
        ctx.close()
        out[shape] = (vol, bl)
    return out


@pytest.mark.parametrize("switch", ROUTE_SWITCHES, ids=[s or "default" for s in ROUTE_SWITCHES])
@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_fft_route_reports_what_each_switch_does(dev, shape, switch, default_route_results, monkeypatch):
    """mi_rl_fft_route under each route switch, and three fused iterations against the default route's: within the bounds between
    layouts of tests/test_gpu_pair_layout.py, bit for bit for MI_FFT_NO_XPIPE (same arithmetic, every stage in LDS:
    tests/test_gpu_x_register_stage.py).  The switch is set only while the context is created: the plan keeps it."""
    from ipp_amd import capi, decon
    psf = R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0))
    if switch:
        monkeypatch.setenv(switch, "1")
    ctx = decon.RLContext(shape, psf, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
    if switch:
        monkeypatch.delenv(switch)
    route = ctx.fft_route
    print(shape, switch, route)
    assert route == _expected_route(shape, switch)
    assert (ctx.pair_layout, ctx.otf_is_real, ctx.fuses) == (bool(route["paired"]), bool(route["real_otf"]), 2 if route["x_splits"] else 1)
    vol, want = default_route_results[shape]
    bl = vol.clone()
    ctx.iterate(bl, None, 3)
    ctx.close()
    if switch in (None, "MI_FFT_NO_XPIPE"):
        assert torch.equal(bl, want)
    else:
        assert_close(bl.cpu().numpy(), want.cpu().numpy().astype(np.float64), rel=2e-5, rel_l2=5e-6, pt_rel=5e-5)
