"""GPU: the factored form of the real OTF (csrc/otf_factor.h, NativeFft::try_factored_otf, k_z_pair_pipe<.., FACT>).

A PSF that is a sum of at most four terms even(z) (x) point-symmetric(y, x) -- every light-sheet PSF of the model -- lets the paired z
pass rebuild each real OTF entry from small tables instead of reading it.  The plan falls back to the stored array whenever the
factors do not reproduce it, which would hide a failure, so the form itself is asserted wherever it is expected.  Results are held
to the float64 chain under the bounds of the exact cases (real_otf_util.BOUNDS) and to a context created under MI_FFT_STORED_OTF=1
under the bounds test_gpu_real_otf_decision.py uses between routes.

576-point z lines (two work-groups per CU beside a 72-KB tile: no room for a table) and 1152-point lines keep the stored form:
fft_native_route.h, z_pair_factored."""
import numpy as np
import pytest
import torch

from oracle import rl_oracle as R
from tests import real_otf_util as U
from tests.rl_util import assert_close
from tests.test_gpu_pair_layout import _conv_pair
from tests.test_otf_factor_host import symmetrised_random, three_term_psf

pytestmark = pytest.mark.gpu

BETWEEN = dict(rel=2e-5, rel_l2=5e-6, pt_rel=5e-5)
ADOPT_SHAPE = (64, 64, 128)


def _ctx(shape, psf, dev, monkeypatch, stored=False, psf_inv=None, boundary=None):
    from ipp_amd import capi, decon
    if stored:
        monkeypatch.setenv("MI_FFT_STORED_OTF", "1")
    ctx = decon.RLContext(shape, psf, psf_inv, boundary=capi.BOUNDARY_CIRCULAR if boundary is None else boundary, engine=capi.ENGINE_FFT, device=dev)
    monkeypatch.delenv("MI_FFT_STORED_OTF", raising=False)
    assert ctx.engine == capi.ENGINE_FFT and ctx.pair_layout and ctx.otf_is_real
    return ctx


def _lightsheet_psf():
    from ipp_amd import psf as P
    return P.resample_psf(P.generate_psf(flavour="matlab")[0], (15, 9, 9))


ADOPT_PSFS = {"gaussian": lambda: R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0)), "lightsheet": _lightsheet_psf, "three_terms": three_term_psf}


@pytest.fixture(scope="module")
def adopt_inputs():
    an, bn = U.operands(ADOPT_SHAPE)
    vol = R.bead_volume(ADOPT_SHAPE, seed=5, psf=R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0)))
    return an, bn, vol


def _three(ctx, an, bn, vol, dev):
    fwd, adj = _conv_pair(ctx, torch.from_numpy(an).to(dev), torch.from_numpy(bn).to(dev))
    bl = torch.from_numpy(vol).to(dev)
    ctx.iterate(bl, None, 5)
    return fwd, adj, bl.cpu().numpy()


@pytest.mark.parametrize("which", sorted(ADOPT_PSFS))
def test_adopted_form_matches_float64_and_the_stored_form(dev, which, adopt_inputs, monkeypatch):
    psf = ADOPT_PSFS[which]()
    assert np.array_equal(psf, psf[::-1, ::-1, ::-1])
    an, bn, vol = adopt_inputs
    fact = _ctx(ADOPT_SHAPE, psf, dev, monkeypatch)
    stored = _ctx(ADOPT_SHAPE, psf, dev, monkeypatch, stored=True)
    print(which, fact.otf_form, stored.otf_form, fact.fft_route)
    assert fact.otf_form["form"] == "factored" and 1 <= fact.otf_form["rank"] <= 4
    assert stored.otf_form == dict(form="stored", rank=0, rank_adj=0)
    assert fact.fft_route == stored.fft_route and fact.fft_route["real_otf"] == 1 and fact.fft_route["z_kernel"] == 2
    got = _three(fact, an, bn, vol, dev)
    ref = _three(stored, an, bn, vol, dev)
    want_f, want_a = U.circular_pair(an, bn, R.otf_from_psf(psf, ADOPT_SHAPE))
    want = (want_f, want_a, R.decon_fft(vol, psf, ADOPT_SHAPE, 5, skip_edgetaper=True))
    for name, g, r, w in zip(("forward", "adjoint", "5 iterations"), got, ref, want):
        print(f"  {name}: factored max %.2e  l2 %.2e  point-wise %.2f x" % U.errors(g.astype(np.float64), w),
              "| stored max %.2e  l2 %.2e  point-wise %.2f x" % U.errors(r.astype(np.float64), w))
    for name, g, r, w in zip(("forward", "adjoint", "5 iterations"), got, ref, want):
        assert_close(g, w, what=name + " against float64", **U.BOUNDS)
        assert_close(g, r.astype(np.float64), what=name + " against the stored form", **BETWEEN)
    fact.close()
    stored.close()


def test_psf_of_higher_rank_keeps_the_stored_form_bit_for_bit(dev, adopt_inputs, monkeypatch):
    psf = symmetrised_random((11, 7, 7))   # six different z planes: rank 6 (tests/test_otf_factor_host.py)
    an, bn, vol = adopt_inputs
    free = _ctx(ADOPT_SHAPE, psf, dev, monkeypatch)
    forced = _ctx(ADOPT_SHAPE, psf, dev, monkeypatch, stored=True)
    assert free.otf_form == forced.otf_form == dict(form="stored", rank=0, rank_adj=0)
    assert free.device_bytes == forced.device_bytes
    for g, r in zip(_three(free, an, bn, vol, dev), _three(forced, an, bn, vol, dev)):
        assert np.array_equal(g, r)
    free.close()
    forced.close()


# z = 64; 192: radix-3 front; 576: no LDS phase table (stays stored); 768: 16 waves, a row per wave; 1024: the 246-register form
@pytest.mark.parametrize("nz,factored", [(64, True), (192, True), (576, False), (768, True), (1024, True)])
def test_kernel_variants_against_float64(dev, nz, factored, monkeypatch):
    shape = (nz, 16, 32)
    psf = R.gaussian_psf(U.KSHAPE, U.SIGMA)
    ctx = _ctx(shape, psf, dev, monkeypatch)
    print(shape, ctx.otf_form)
    assert ctx.otf_form["form"] == ("factored" if factored else "stored")
    an, bn = U.operands(shape)
    fwd, adj = _conv_pair(ctx, torch.from_numpy(an).to(dev), torch.from_numpy(bn).to(dev))
    want_f, want_a = U.circular_pair(an, bn, R.otf_from_psf(psf, shape))
    for name, got, want in (("forward", fwd, want_f), ("adjoint", adj, want_a)):
        print(f"  {name}: max %.2e  l2 %.2e  point-wise %.2f x" % U.errors(got.astype(np.float64), want))
        assert_close(got, want, what=name, **U.BOUNDS)
    ctx.close()


def test_padded_grid_with_an_explicit_adjoint_factors_both_slots(dev, monkeypatch):
    from ipp_amd import capi
    vshape, kshape = (50, 40, 60), (15, 9, 5)   # grid 64 x 48 x 64
    psf, inv = R.gaussian_psf(kshape, (2.5, 1.5, 0.8)), R.gaussian_psf(kshape, (1.5, 1.0, 1.2))
    monkeypatch.setenv("MI_FFT_NATIVE_INFLATE", "100")   # (as test_paired_layout_on_padded_grids)
    ctx = _ctx(vshape, psf, dev, monkeypatch, psf_inv=inv, boundary=capi.BOUNDARY_ZERO)
    print(ctx.otf_form)
    assert ctx.otf_form["form"] == "factored" and ctx.otf_form["rank"] >= 1 and ctx.otf_form["rank_adj"] >= 1
    g = torch.Generator().manual_seed(7)
    a = (torch.rand(vshape, generator=g) + 0.5).to(dev)
    b = (torch.rand(vshape, generator=g) + 0.5).to(dev)
    fwd, adj = _conv_pair(ctx, a, b)
    assert_close(fwd, R.convn_same(a.cpu().numpy(), psf).astype(np.float64), what="forward", **U.BOUNDS)
    assert_close(adj, R.convn_same(b.cpu().numpy(), inv).astype(np.float64), what="explicit adjoint", **U.BOUNDS)
    ctx.close()


def test_factored_context_gives_the_stored_array_back(dev, monkeypatch):
    psf = R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0))
    fact = _ctx(ADOPT_SHAPE, psf, dev, monkeypatch)
    stored = _ctx(ADOPT_SHAPE, psf, dev, monkeypatch, stored=True)
    assert fact.otf_form["form"] == "factored"
    nz, ny, nx = ADOPT_SHAPE
    lines = (nx // 4 + 1) * ny                       # planes xk <= Hx / 2 of the half-length x transform, times the y lines
    gr, tables = 8 * lines * nz, 16 * (nz + 2 * lines)
    print(stored.device_bytes, fact.device_bytes, gr, tables)
    assert stored.device_bytes - fact.device_bytes == gr - tables and tables < gr // 10
    fact.close()
    stored.close()
