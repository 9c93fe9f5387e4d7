"""GPU: the transfer function of the FFT convolution pipeline, bin by bin, at every length the hand-written plan takes
(fft_native.hip, split_axis) and on the routes beside it (complex OTF form, plain layout, rocFFT).  A circular convolution of a probe
with a flat spectrum, divided by the probe's spectrum, must return the OTF on every bin: fftn(got) / fftn(x) = H within a bound that
is 8 x the error of a complex64 FFT of the same case (tests/spectral_util.py, tests/test_spectral_probe_host.py, DESIGN.md
section 15).  Circular rule only -- the transfer function is diagonal only there."""
import numpy as np
import pytest
import torch

from tests import spectral_util as S

pytestmark = pytest.mark.gpu

AXIS_CASES = ([pytest.param((16, 16, n), id=f"x{n}") for n in S.NATIVE_LENGTHS["x"]]
              + [pytest.param((16, n, 16), id=f"y{n}") for n in S.NATIVE_LENGTHS["y"]]
              + [pytest.param((n, 16, 16), id=f"z{n}") for n in S.NATIVE_LENGTHS["z"]])


def _id(shape):
    return "x".join(str(n) for n in shape)


def _check_forward(dev, shape, routes=((None, ""),), monkeypatch=None):
    """mi_conv3d (EPI_NONE, so signed input is fine) on the flat probe, asymmetric and symmetric PSF, on every route of ``routes``
    (environment variable or None, label)."""
    from ipp_amd import decon
    for symmetric in (False, True):
        x, ker, H = S.forward_case(shape, symmetric)
        X = S.sfft.fftn(x.astype(np.float64), workers=S.WORKERS)
        for env, what in routes:
            if env:
                monkeypatch.setenv(env, "1")
            try:
                got = decon.convn_same(torch.from_numpy(x).to(dev), torch.from_numpy(ker).to(dev), boundary=2, engine=2).cpu().numpy()
            finally:
                if env:
                    monkeypatch.delenv(env)
            err = S.transfer_error(got, x, H, X)
            print(f"spectral fwd{what} {shape} symmetric={symmetric} max {err.max():.3e}")
            assert err.max() <= S.FWD_BOUND, f"{shape} symmetric={symmetric}{what}: " + S.describe_worst(err, shape)


@pytest.mark.parametrize("shape", AXIS_CASES)
def test_forward_transfer_function_every_length(dev, shape):
    _check_forward(dev, shape)


@pytest.mark.parametrize("shape", S.MIXED_SHAPES, ids=_id)
def test_forward_transfer_function_mixed_shapes_on_every_route(dev, shape, monkeypatch):
    """No axis trivial; the plan's own choice of OTF form, the complex form forced, and the rocFFT route of the same engine."""
    _check_forward(dev, shape, ((None, ""), ("MI_FFT_COMPLEX_OTF", " complex OTF"), ("MI_FFT_ROCFFT", " rocFFT")), monkeypatch)


@pytest.mark.parametrize("shape", S.ROCFFT_ONLY_SHAPES, ids=_id)
def test_forward_transfer_function_rocfft_only_shapes(dev, shape, monkeypatch):
    """Shapes the native plan refuses: rocFFT with the multiply kernels of fftconv.hip."""
    _check_forward(dev, shape, (("MI_FFT_ROCFFT", " rocFFT"),), monkeypatch)


def _conv_pair(ctx, a, b):
    """(conv(a), conv_adj(b)) through the two half-steps of the context, as tests/test_gpu_pair_layout.py recovers them."""
    ra = torch.empty_like(a)
    ctx.forward_ratio(a, ra)      # a ./ max(conv(a), eps): conv(a) > 0, so conv(a) = a ./ ra
    adj = torch.ones_like(b)
    ctx.adjoint_update(b, adj)    # |1 .* conv_adj(b)|
    return (a / ra).cpu().numpy(), adj.cpu().numpy()


def _check_ctx(ctx, dev, shape, x, H, X, what):
    t = torch.from_numpy(x).to(dev)
    fwd, adj = _conv_pair(ctx, t, t)
    lines = S.dc_lines(shape)
    for name, got, otf in (("forward", fwd, H), ("conjugate", adj, np.conj(H))):
        assert np.isfinite(got).all()
        err = S.transfer_error(got, x, otf, X)
        fine, on_lines = np.where(lines, 0.0, err), np.where(lines, err, 0.0)
        print(f"spectral ctx {what} {name} {shape} fine {fine.max():.3e} lines {on_lines.max():.3e}")
        assert fine.max() <= S.CTX_BOUND_FINE, f"{shape} {what} {name}: " + S.describe_worst(fine, shape)
        assert on_lines.max() <= S.CTX_BOUND_LINES, f"{shape} {what} {name}, lines through DC: " + S.describe_worst(on_lines, shape)


@pytest.mark.parametrize("shape", S.CTX_SHAPES, ids=_id)
def test_context_transfer_function_forward_and_conjugate(dev, shape, monkeypatch):
    """The RL context (deconFFT placement): both half-steps clamp or take abs, so the probe carries a DC term, which costs any
    float32 FFT accuracy on the three lines of bins through DC -- these have a bound of their own."""
    from ipp_amd import capi, decon
    for symmetric in (False, True):
        x, psf, H = S.ctx_case(shape, symmetric)
        X = S.sfft.fftn(x.astype(np.float64), workers=S.WORKERS)
        for otf in (H, np.conj(H)):                          # nothing for the clamp and the abs to do
            assert S.sfft.ifftn(X * otf, workers=S.WORKERS).real.min() > 0.25
        ctx = decon.RLContext(shape, psf, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
        print(f"spectral ctx route {shape} symmetric={symmetric} otf_is_real={ctx.otf_is_real} pair_layout={ctx.pair_layout}")
        assert ctx.fuses                                     # the hand-written plan took the shape
        # (a symmetric PSF takes the real OTF form where the z pass of the shape can hold it, NativeFft::try_real_otf: every paired
        # shape, and the pipelined plain ones whose lines divide the work-group evenly)
        assert ctx.otf_is_real == symmetric if ctx.pair_layout else not (ctx.otf_is_real and not symmetric)
        _check_ctx(ctx, dev, shape, x, H, X, f"symmetric={symmetric}")
        paired = ctx.pair_layout
        ctx.close()
        if paired:
            monkeypatch.setenv("MI_FFT_NO_PAIR", "1")
            plain = decon.RLContext(shape, psf, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
            monkeypatch.delenv("MI_FFT_NO_PAIR")
            assert not plain.pair_layout
            _check_ctx(plain, dev, shape, x, H, X, f"symmetric={symmetric} plain layout")
            plain.close()
