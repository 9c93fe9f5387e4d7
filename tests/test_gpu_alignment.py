"""GPU: the library's alignment contract ("Alignment of the caller's buffers") on buffers whose base address is only
element-aligned.

Every device allocation is 256-byte aligned, so the refusals and the element-wise fallback kernels that the entry points choose
from the caller's pointers never run unless a test offsets a pointer on purpose: tests/align_util.py cuts contiguous views at
element offsets 1 and 2 (float32: 4 and 8 bytes), 1 and 4 (uint16), 1 and 8 (uint8) out of guarded buffers.  A refusing call must
raise MI_ERR_INVALID naming alignment, leave its output alone and leave the library usable; a fallback must meet the same
comparison with the float64 oracle as the aligned test of the operation (the tolerance is that test's, cited at each case), and
where only loads and stores differ, equal the aligned run bit for bit.  Every output is a guarded view whose guard regions are
checked after the call."""
import numpy as np
import pytest
import torch

from oracle import destripe_oracle as D
from oracle import rl_oracle as R
from tests import align_util as A
from tests import isodown_util as IU
from tests import pystripe_util as PU
from tests import stitch_util as SU
from tests import terafly_util as TU
from tests.rl_util import assert_close, asymmetric_psf
from tests.test_gpu_destripe import TOL as DESTRIPE_TOL, _volume as destripe_volume
from tests.test_gpu_isodown import TOL as ISODOWN_TOL
from tests.test_gpu_rl import _rel

pytestmark = pytest.mark.gpu

F32_OFFS = (1, 2)
INT_OFFS = {np.uint16: A.OFFSETS["uint16"], np.uint8: A.OFFSETS["uint8"]}
INT_CASES = [(dt, off) for dt, offs in INT_OFFS.items() for off in offs]
INT_IDS = [f"{np.dtype(dt).name}+{off}" for dt, off in INT_CASES]
TORCH_DT = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.float32): torch.float32}
PAIR_BOUNDS = dict(rel=2e-5, rel_l2=2e-6, pt_rel=2e-5)   # tests/test_gpu_pair_layout.py


class Guards:
    """Guarded device views of one test; ``check()`` runs every guard checker."""

    def __init__(self, dev):
        self.dev, self.checks = dev, []

    def __call__(self, shape, dtype, off=0, fill=None):
        if isinstance(fill, np.ndarray) and fill.dtype == np.uint16:
            fill = fill.view(np.int16)
        v, c = A.offset_tensor(shape, dtype, off, self.dev, fill)
        self.checks.append(c)
        return v

    def like(self, a, off=0):
        """guarded device copy of a numpy array"""
        return self(a.shape, TORCH_DT[a.dtype], off, a)

    def check(self):
        torch.cuda.synchronize(self.dev)
        for c in self.checks:
            c()


@pytest.fixture
def g(dev):
    return Guards(dev)


def refused(call):
    from ipp_amd import capi
    with pytest.raises(capi.MiError) as e:
        call()
    assert e.value.code == capi.MI_ERR_INVALID, e.value
    assert "aligned" in str(e.value), e.value


def host(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _stream(dev):
    from ipp_amd import capi
    return capi.current_stream_ptr(dev)


# ================================================================================================================== refusals
@pytest.mark.parametrize("off", F32_OFFS)
def test_prctile_refuses_an_offset_volume(dev, g, off):
    """stats.hip, mi_prctile: MI_REQUIRE on the pointer; k_radix_hist reads float4."""
    from ipp_amd import decon
    data = np.random.default_rng(5).random(1003, dtype=np.float32)
    x = g.like(data, off)
    refused(lambda: decon.prctile(x, [25.0, 75.0]))
    got = decon.prctile(torch.from_numpy(data).to(dev), [25.0, 75.0])
    for a, w in zip(got, R.prctile(data, (25.0, 75.0))):
        assert a == pytest.approx(float(w), rel=2e-7, abs=0.0)   # test_prctile_matches_oracle
    assert np.array_equal(host(x), data)
    g.check()


@pytest.mark.parametrize("scal,dtype", [(255.0, np.uint8), (65535.0, np.uint16)])
@pytest.mark.parametrize("off", F32_OFFS)
def test_rescale_block_refuses_an_offset_source(dev, g, off, scal, dtype):
    """stats.hip, mi_rescale_block: the source is read as float4."""
    from ipp_amd import decon
    data = (np.random.default_rng(6).random(1003, dtype=np.float32) * np.float32(1.2))
    x = g.like(data, off)
    out = g((1003,), TORCH_DT[np.dtype(dtype)])
    refused(lambda: decon.rescale_block(x, scal, 1.0, 0.0123, 0.9871, out=out))
    assert A.payload_is_sentinel(out)
    got = decon.rescale_block(torch.from_numpy(data).to(dev), scal, 1.0, 0.0123, 0.9871, out=out)
    assert np.array_equal(host(got), R.rescale_block(data, scal, 1.0, 0.0123, 0.9871, dtype))   # test_rescale_block_bit_exact
    g.check()


@pytest.mark.parametrize("dtype,off", INT_CASES, ids=INT_IDS)
@pytest.mark.parametrize("dmin,ampl", [(0.0, 1.0), (0.02, 2.5)])
def test_rescale_block_into_an_offset_destination_is_bit_exact(dev, g, dtype, off, dmin, ampl):
    """The destination of k_rescale is written sample by sample (the four of a float4 and the scalar tail alike): any base will do."""
    from ipp_amd import decon
    scal = 255.0 if dtype == np.uint8 else 65535.0
    data = (np.random.default_rng(7).random(1003, dtype=np.float32) * np.float32(1.2))
    data[:5] = [0.0, dmin, 0.9871, 2.0, -1.0]
    out = g((1003,), TORCH_DT[np.dtype(dtype)], off)
    decon.rescale_block(torch.from_numpy(data).to(dev), scal, ampl, dmin, 0.9871, out=out)
    assert np.array_equal(host(out), R.rescale_block(data, scal, ampl, dmin, 0.9871, dtype))
    g.check()


@pytest.mark.parametrize("off", F32_OFFS)
def test_gauss3d_refuses_an_offset_volume(dev, g, off):
    """gauss3d.hip, gauss3d_to: both buffers are read and written as float4."""
    from ipp_amd import decon
    data = np.random.default_rng(8).random((8, 8, 8), dtype=np.float32)
    x = g.like(data, off)
    refused(lambda: decon.gauss3d_gpu(x, 1.0))
    assert np.array_equal(host(x), data)                       # (in place: the volume is the output)
    ok = g.like(data)
    decon.gauss3d_gpu(ok, 1.0)
    assert np.abs(host(ok) - R.gauss3d(data, 1.0)).max() < 5e-5   # test_gauss3d_gpu_matches_oracle
    g.check()


@pytest.mark.parametrize("which,off", [("source", o) for o in INT_OFFS[np.uint16]] + [("destination", o) for o in F32_OFFS])
def test_im2single_refuses_offset_buffers(dev, g, which, off):
    """common.hip, mi_u16_to_f32: uint4 loads, float4 stores."""
    from ipp_amd import capi, decon
    u = np.random.default_rng(9).integers(0, 65536, size=1003, dtype=np.uint16)
    src = g.like(u, off if which == "source" else 0)
    dst = g((1003,), torch.float32, off if which == "destination" else 0)
    refused(lambda: capi.check(capi.lib().mi_u16_to_f32(dev.index, _stream(dev), src.data_ptr(), dst.data_ptr(), 1003, 1.0 / 65535.0)))
    assert A.payload_is_sentinel(dst)
    got = decon.im2single(u, dev).cpu().numpy()
    assert np.array_equal(got, R.u16_to_f32(u)) or np.abs(got - R.u16_to_f32(u)).max() < 1e-7   # test_u16_ingest_pad_crop_norm
    g.check()


@pytest.mark.parametrize("off", F32_OFFS)
def test_norm2_refuses_an_offset_volume(dev, g, off):
    """common.hip, mi_norm2: k_sumsq reads float4 from an aligned base."""
    from ipp_amd import decon
    data = np.random.default_rng(10).random(1003, dtype=np.float32)
    x = g.like(data, off)
    refused(lambda: decon.norm2(x))
    want = float(np.linalg.norm(data.astype(np.float64)))
    assert decon.norm2(torch.from_numpy(data).to(dev)) == pytest.approx(want, rel=1e-12)   # test_u16_ingest_pad_crop_norm
    g.check()


def test_stop_criterion_norm_on_an_offset_volume(dev, g):
    """The stop test of the deconvolution loops takes the norm of the caller's volume as it is (rl_decon.hip, host_norm): k_sumsq goes
    element by element over a base that is not 16-byte aligned.  Same run as test_decon_stop_criterion_and_numpy_roundtrip."""
    from ipp_amd import decon
    psf = R.gaussian_psf((5, 5, 5), (1, 1, 1))
    vol = R.bead_volume((12, 16, 16), seed=4, psf=psf)
    want, it_want = R.decon_spatial(vol, psf, 50, stop_criterion=5.0, return_iters=True)
    bl = g.like(vol, 1)
    got, it = decon.decon(bl, psf, 50, 0.0, 5.0, 0, 1, False, None, False, return_iters=True)
    assert got is bl and it == it_want
    assert_close(host(got), want)
    g.check()


# ---- native FFT on an unpadded grid: fft_native.hip, NativeFft::conv / iterate (check_aligned)
RL_SHAPE = (64, 16, 32)


@pytest.fixture(scope="module")
def circular():
    """PSF, the two operands and the float64 references of the circular context on RL_SHAPE (decon.m:162-172)."""
    psf = R.gaussian_psf((7, 5, 9), (1.5, 1.0, 2.0))
    rng = np.random.default_rng(sum(RL_SHAPE))
    a = (rng.random(RL_SHAPE) + 0.5).astype(np.float32)
    b = (rng.random(RL_SHAPE) + 0.5).astype(np.float32)
    otf = R.otf_from_psf(psf, RL_SHAPE)
    fwd = np.real(np.fft.ifftn(np.fft.fftn(a.astype(np.float64)) * otf))
    adj = np.real(np.fft.ifftn(np.fft.fftn(b.astype(np.float64)) * np.conj(otf)))
    vol = R.bead_volume(RL_SHAPE, seed=5, psf=psf)
    return dict(psf=psf, a=a, b=b, ones=np.ones(RL_SHAPE, np.float32), fwd=fwd, adj=adj, vol=vol, iterated=R.decon_fft(vol, psf, RL_SHAPE, 3, skip_edgetaper=True))


@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("operand", ["volume", "second"])
@pytest.mark.parametrize("call", ["forward_ratio", "adjoint_update", "iterate"])
def test_native_fft_on_an_unpadded_grid_refuses_offset_volumes(dev, g, circular, call, operand, off):
    from ipp_amd import capi, decon
    c = circular
    ctx = decon.RLContext(RL_SHAPE, c["psf"], None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
    assert ctx.engine == capi.ENGINE_FFT and ctx.fuses and ctx.pair_layout
    o1, o2 = (off, 0) if operand == "volume" else (0, off)
    if call == "forward_ratio":      # bl is the input and the epilogue operand, ratio the output
        bl, ratio = g.like(c["a"], o1), g(RL_SHAPE, torch.float32, o2)
        refused(lambda: ctx.forward_ratio(bl, ratio))
        assert A.payload_is_sentinel(ratio) and np.array_equal(host(bl), c["a"])
        ok = g(RL_SHAPE, torch.float32)
        ctx.forward_ratio(g.like(c["a"]), ok)
        assert_close(c["a"] / host(ok), c["fwd"], **PAIR_BOUNDS)      # conv(a) = a ./ ratio, as _conv_pair of test_gpu_pair_layout.py
    elif call == "adjoint_update":   # bl is the epilogue operand and the output, ratio the input
        bl, ratio = g.like(c["ones"], o1), g.like(c["b"], o2)
        refused(lambda: ctx.adjoint_update(ratio, bl))
        assert np.array_equal(host(bl), c["ones"]) and np.array_equal(host(ratio), c["b"])
        ok = g.like(c["ones"])
        ctx.adjoint_update(g.like(c["b"]), ok)
        assert_close(host(ok), c["adj"], **PAIR_BOUNDS)               # |1 .* conv_adj(b)|
    else:
        bl, ratio = g.like(c["vol"], o1), g(RL_SHAPE, torch.float32, o2)
        if operand == "volume":
            refused(lambda: ctx.iterate(bl, ratio, 3))
            assert np.array_equal(host(bl), c["vol"])
            bl = g.like(c["vol"])
        # a fusing context never touches the ratio scratch: an offset one is not looked at
        ctx.iterate(bl, ratio, 3)
        assert A.payload_is_sentinel(ratio)
        assert_close(host(bl), c["iterated"])   # test_paired_layout_fused_iterations_match_the_oracle
    ctx.close()
    g.check()


# ================================================================================================================== fallbacks
# ---- direct 3-D convolution: conv3d_direct.hip reads and writes the caller's volumes element by element
CONV_SHAPE, CONV_K = (6, 10, 16), (3, 5, 7)


def _conv_want(img, ker, boundary):
    if boundary == 0:
        return R.convn_same(img, ker)
    if boundary == 1:
        return R.conv3d_replicate(img, ker)
    from scipy import ndimage
    return ndimage.convolve(img.astype(np.float64), ker.astype(np.float64), mode="wrap").astype(np.float32)


def _conv3d(dev, g, img, ker, boundary, engine, operand, off):
    from ipp_amd import capi
    o = {"image": (off, 0, 0), "kernel": (0, off, 0), "output": (0, 0, off), "none": (0, 0, 0)}[operand]
    a, k, out = g.like(img, o[0]), g.like(ker, o[1]), g(img.shape, torch.float32, o[2])
    capi.check(capi.lib().mi_conv3d(dev.index, _stream(dev), a.data_ptr(), k.data_ptr(), out.data_ptr(), img.shape[2], img.shape[1], img.shape[0],
                                    ker.shape[2], ker.shape[1], ker.shape[0], boundary, engine))
    g.check()
    return host(out)


@pytest.fixture(scope="module")
def conv_case():
    rng = np.random.default_rng(7)
    img, ker = rng.random(CONV_SHAPE, dtype=np.float32), rng.random(CONV_K, dtype=np.float32)
    return img, ker, {b: _conv_want(img, ker, b) for b in (0, 1, 2)}


@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("operand", ["image", "kernel", "output"])
@pytest.mark.parametrize("boundary", [0, 1, 2])
def test_direct_convolution_on_offset_buffers(dev, g, conv_case, boundary, operand, off):
    img, ker, want = conv_case
    got = _conv3d(dev, g, img, ker, boundary, 1, operand, off)
    assert _rel(got, want[boundary]) < 2e-6                          # test_convn_same_boundaries_and_engines, engine 1
    assert np.array_equal(got, _conv3d(dev, g, img, ker, boundary, 1, "none", 0))   # one kernel, the same arithmetic


# ---- separable context: rl.hip ctx_conv leaves the single-pass kernel (sep3d.hip) for three direct passes
SEP_SHAPE = (12, 16, 32)


@pytest.fixture(scope="module")
def separable():
    psf = R.gaussian_psf((5, 5, 5), (1.0, 1.0, 1.0))
    vol = R.bead_volume(SEP_SHAPE, seed=5, psf=psf) + np.float32(0.01)
    rng = np.random.default_rng(12)
    ratio = (rng.random(SEP_SHAPE) + 0.5).astype(np.float32)
    reg = rng.random(SEP_SHAPE).astype(np.float32)
    conv = R.convn_same(vol, psf).astype(np.float64)
    adj = R.convn_same(ratio, R.flip3(psf)).astype(np.float64)
    lam = np.float32(0.05)
    return dict(psf=psf, vol=vol, ratio=ratio, reg=reg, fwd=vol / np.maximum(conv, R.EPS_SINGLE), upd=np.abs(vol * adj),
                upd_reg=np.abs(vol * adj * (1.0 - float(lam)) + reg * float(lam)), iterated=R.decon_spatial(vol, psf, 3, skip_edgetaper=True))


@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("case", ["ratio_in", "ratio_out", "update_in", "update_bl", "update_reg", "iterate_bl", "iterate_scratch"])
def test_separable_context_on_offset_buffers(dev, g, separable, case, off):
    """Against the oracle as test_separable_psf_takes_three_1d_passes / ..._edges_and_regularised_update do (assert_close at its
    defaults), and against the aligned call of the same context (two kernels with different summation orders: fp32 rounding, the
    5e-6 of those tests)."""
    from ipp_amd import capi, decon
    s = separable
    ctx = decon.RLContext(SEP_SHAPE, s["psf"], None, boundary=capi.BOUNDARY_ZERO, engine=capi.ENGINE_DIRECT, device=dev)
    assert ctx.engine == capi.ENGINE_DIRECT and int(capi.lib().mi_rl_separable(ctx._h)) == 2   # aligned: the single-pass kernel

    def run(o):
        if case.startswith("ratio"):
            bl, out = g.like(s["vol"], o if case == "ratio_in" else 0), g(SEP_SHAPE, torch.float32, o if case == "ratio_out" else 0)
            ctx.forward_ratio(bl, out)
            return host(out), s["fwd"]
        if case.startswith("update"):
            ratio = g.like(s["ratio"], o if case == "update_in" else 0)
            bl = g.like(s["vol"], o if case == "update_bl" else 0)
            if case == "update_reg":
                ctx.adjoint_update(ratio, bl, 0.05, g.like(s["reg"], o))
                return host(bl), s["upd_reg"]
            ctx.adjoint_update(ratio, bl)
            return host(bl), s["upd"]
        bl = g.like(s["vol"], o if case == "iterate_bl" else 0)
        ctx.iterate(bl, g(SEP_SHAPE, torch.float32, o if case == "iterate_scratch" else 0), 3)
        return host(bl), s["iterated"]

    got, want = run(off)
    assert_close(got, want)
    aligned, _ = run(0)
    assert _rel(got, aligned) < 5e-6
    ctx.close()
    g.check()


# ---- native FFT on padded grids: fft_native_x.hip, the persistent x kernel (pad_pipe) against k_x_forward / k_x_inverse
PAD_SHAPE, PAD_K = (50, 40, 60), (15, 9, 5)


@pytest.fixture(scope="module")
def padded(dev):
    """Set-up of test_paired_layout_on_padded_grids; the direct-engine results per boundary, computed once on aligned buffers."""
    from ipp_amd import capi, decon
    psf = asymmetric_psf(PAD_K, seed=3)
    inv = np.ascontiguousarray(psf[::-1, ::-1, ::-1])
    gen = torch.Generator().manual_seed(7)
    a = (torch.rand(PAD_SHAPE, generator=gen) + 0.5).numpy()
    b = (torch.rand(PAD_SHAPE, generator=gen) + 0.5).numpy()
    out = dict(psf=psf, inv=inv, a=a, b=b, conv0=R.convn_same(a, psf).astype(np.float64))
    for boundary in (0, 1):
        direct = decon.RLContext(PAD_SHAPE, psf, inv, boundary=boundary, engine=capi.ENGINE_DIRECT, device=dev)
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        ra, adj = torch.empty_like(ta), torch.ones_like(tb)
        direct.forward_ratio(ta, ra)
        direct.adjoint_update(tb, adj)
        out[boundary] = ((ta / ra).cpu().numpy().astype(np.float64), adj.cpu().numpy().astype(np.float64))
        direct.close()
    vol = R.bead_volume(PAD_SHAPE, seed=5, psf=R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0)))
    out["vol"], out["iterated"] = vol, R.decon_spatial(vol, psf, 3, skip_edgetaper=True)
    return out


def _padded_ctx(dev, p, boundary, monkeypatch):
    from ipp_amd import capi, decon
    monkeypatch.setenv("MI_FFT_NATIVE_INFLATE", "100")
    ctx = decon.RLContext(PAD_SHAPE, p["psf"], p["inv"], boundary=boundary, engine=capi.ENGINE_FFT, device=dev)
    assert ctx.engine == capi.ENGINE_FFT and ctx.pair_layout and ctx.fuses == (1 if boundary == 0 else 0)
    return ctx


@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("operand", ["volume", "second"])
@pytest.mark.parametrize("boundary", [0, 1])
def test_native_fft_on_padded_grids_with_offset_volumes(dev, g, padded, boundary, operand, off, monkeypatch):
    p = padded
    ctx = _padded_ctx(dev, p, boundary, monkeypatch)
    o1, o2 = (off, 0) if operand == "volume" else (0, off)
    a, ra = g.like(p["a"], o1), g(PAD_SHAPE, torch.float32, o2)
    ctx.forward_ratio(a, ra)                       # a ./ max(conv(a), eps): conv(a) = a ./ ra
    ones = g.like(np.ones(PAD_SHAPE, np.float32), o1)
    ctx.adjoint_update(g.like(p["b"], o2), ones)   # |1 .* conv_adj(b)|
    fwd, adj = p["a"] / host(ra), host(ones)
    assert_close(fwd, p[boundary][0], **PAIR_BOUNDS)
    assert_close(adj, p[boundary][1], **PAIR_BOUNDS)
    if boundary == 0:
        assert_close(fwd, p["conv0"], **PAIR_BOUNDS)
    ctx.close()
    g.check()


@pytest.mark.parametrize("off", F32_OFFS)
def test_native_fft_fused_iterations_on_a_zero_padded_grid_with_an_offset_volume(dev, g, padded, off, monkeypatch):
    """k_x_inverse<fused> with the element-wise crop and epilogue (the aligned route: the persistent kernel)."""
    ctx = _padded_ctx(dev, padded, 0, monkeypatch)
    bl = g.like(padded["vol"], off)
    ctx.iterate(bl, None, 3)
    assert_close(host(bl), padded["iterated"])
    ctx.close()
    g.check()


# ---- rocFFT route: fftconv.hip, FftEngine::conv (input staged when its base is offset; k_fft_epilogue_flat or k_fft_epilogue)
ROC_SHAPE, ROC_K = (12, 20, 32), (3, 5, 5)


@pytest.fixture(scope="module")
def roc_case():
    rng = np.random.default_rng(17)
    img, ker = rng.random(ROC_SHAPE, dtype=np.float32) + np.float32(0.5), rng.random(ROC_K, dtype=np.float32)
    ker /= ker.sum()
    from scipy import ndimage
    conv = ndimage.convolve(img.astype(np.float64), ker.astype(np.float64), mode="wrap")
    return img, ker, conv


@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("operand", ["image", "kernel", "output"])
def test_rocfft_convolution_on_offset_buffers(dev, g, roc_case, operand, off, monkeypatch):
    monkeypatch.setenv("MI_FFT_ROCFFT", "1")
    img, ker, conv = roc_case
    got = _conv3d(dev, g, img, ker, 2, 2, operand, off)
    assert _rel(got, conv) < 2e-5                                    # test_convn_same_boundaries_and_engines, engine 2


@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("case", ["ratio_in", "ratio_out", "update_in", "update_bl", "update_reg"])
def test_rocfft_epilogues_on_offset_operands(dev, g, roc_case, case, off, monkeypatch):
    """The ratio / update / regularised-update epilogues of the rocFFT route with each operand offset in turn; the convolution is
    recovered from the result and held to the bound of the rocFFT branch of test_convn_same_boundaries_and_engines."""
    from ipp_amd import capi, decon
    monkeypatch.setenv("MI_FFT_ROCFFT", "1")
    img, ker, conv = roc_case
    # the context places the PSF as deconFFT does (ifftshift of the centred pad): its circular convolution in float64
    otf = R.otf_from_psf(ker, ROC_SHAPE)
    fwd = np.real(np.fft.ifftn(np.fft.fftn(img.astype(np.float64)) * otf))
    adj = np.real(np.fft.ifftn(np.fft.fftn(img.astype(np.float64)) * np.conj(otf)))
    ctx = decon.RLContext(ROC_SHAPE, ker, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
    assert ctx.engine == capi.ENGINE_FFT and not ctx.fuses and not ctx.pair_layout      # not the hand-written pipeline
    if case.startswith("ratio"):
        bl, out = g.like(img, off if case == "ratio_in" else 0), g(ROC_SHAPE, torch.float32, off if case == "ratio_out" else 0)
        ctx.forward_ratio(bl, out)
        assert _rel(img / host(out), fwd) < 2e-5
    else:
        ones = np.ones(ROC_SHAPE, np.float32)
        ratio = g.like(img, off if case == "update_in" else 0)
        bl = g.like(ones, off if case == "update_bl" else 0)
        if case == "update_reg":
            reg = np.full(ROC_SHAPE, 0.25, np.float32)
            ctx.adjoint_update(ratio, bl, 0.05, g.like(reg, off))
            assert _rel(host(bl), np.abs(adj * (1.0 - float(np.float32(0.05))) + 0.25 * float(np.float32(0.05)))) < 2e-5
        else:
            ctx.adjoint_update(ratio, bl)
            assert _rel(host(bl), np.abs(adj)) < 2e-5
    ctx.close()
    g.check()


# ---- edgetaper_3d: edgetaper.hip (the blur's engines read the block element by element; k_taper_blend likewise)
@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("shape,kshape", [((5, 6, 7), (3, 3, 3)), ((16, 20, 24), (7, 5, 5))])
@pytest.mark.parametrize("engine", ["fft", "direct", "slabs"])
def test_edgetaper_on_an_offset_volume(dev, g, engine, shape, kshape, off, monkeypatch):
    from ipp_amd import decon
    monkeypatch.setenv("MI_EDGETAPER_ENGINE", engine)
    bl = np.random.default_rng(42).random(shape, dtype=np.float32)
    psf = R.gaussian_psf(kshape, [k / 5.0 for k in kshape]) * 3.0
    t = g.like(bl, off)
    assert decon.edgetaper_3d(t, torch.from_numpy(psf).to(dev)) is t
    assert np.abs(host(t) - R.edgetaper_3d(bl, psf)).max() < 1e-5     # test_edgetaper_fft_route_equals_direct_route
    g.check()


# ---- filter_subband_3d_z: destripe.hip, k_dwt_z<., 4> or <., 1>
@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_destripe_on_an_offset_volume(dev, g, sigma, off):
    from ipp_amd import decon
    shape = (40, 4, 64)       # ny * nx % 4 == 0: the aligned run takes four columns per lane
    vol = destripe_volume(shape, 21)
    want = D.filter_subband_3d_z(vol, sigma)
    t = g.like(vol, off)
    assert decon.filter_subband_3d_z(t, sigma, 0, "db9") is t
    assert np.abs(host(t) - want).max() <= DESTRIPE_TOL * np.abs(want).max()   # test_destripe_matches_oracle
    g.check()


# ================================================================================================= bit-exact copies and integers
@pytest.mark.parametrize("off", F32_OFFS)
def test_pad_and_crop_center_into_offset_destinations(dev, g, off):
    """common.hip, k_pad_center / k_crop_center: float4 stores when the destination's rows allow, else per sample."""
    from ipp_amd import capi
    a = np.random.default_rng(3).random((6, 7, 8), dtype=np.float32)
    want, pre, post = R.pad_block_to_fft_shape(a, (9, 10, 12))
    src, dst = g.like(a), g((9, 10, 12), torch.float32, off)
    capi.check(capi.lib().mi_pad_center(dev.index, _stream(dev), src.data_ptr(), 8, 7, 6, dst.data_ptr(), 12, 10, 9))
    assert np.array_equal(host(dst), want)
    back = g((6, 7, 8), torch.float32, off)
    capi.check(capi.lib().mi_crop_center(dev.index, _stream(dev), dst.data_ptr(), 12, 10, 9, back.data_ptr(), 8, 7, 6))
    assert np.array_equal(host(back), R.unpad_block(want, pre, post)) and np.array_equal(host(back), a)
    g.check()


@pytest.mark.parametrize("off", F32_OFFS)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_load_block_into_an_offset_destination(dev, g, dtype, off):
    """common.hip, k_load_block, as test_load_block_on_the_device_is_bit_identical: a block whose pads reach past every face."""
    from ipp_amd import capi, lsdeconv as L
    vol = (np.random.default_rng(17).random((20, 26, 30)) * (250 if dtype == np.uint8 else 60000)).astype(dtype)
    p1, p2, pad = (1, 1, 1), (30, 26, 20), (5, 4, 3)
    want = L.load_block(vol, p1, p2, pad)
    assert want.shape[2] % 4 == 0
    raw = g.like(vol)                    # the whole volume is the box read: before = pad on every axis
    dst = g(want.shape, torch.float32, off)
    capi.check(capi.lib().mi_load_block(dev.index, _stream(dev), raw.data_ptr(), vol.dtype.itemsize, 30, 26, 20, dst.data_ptr(), want.shape[2],
                                        want.shape[1], want.shape[0], pad[0], pad[1], pad[2]))
    assert np.array_equal(host(dst), want)
    g.check()


@pytest.mark.parametrize("dtype,off", INT_CASES, ids=INT_IDS)
@pytest.mark.parametrize("method", ["mean", "max"])
def test_pyramid_slab_from_an_offset_slab(dev, g, dtype, off, method):
    """pyramid.hip, halve2_kernel<T, MAX, VEC>: four samples per load from a base aligned to four samples, else one by one."""
    from ipp_amd import terafly
    hd = [1, 1]
    slab = np.random.default_rng(100).integers(0, np.iinfo(dtype).max + 1, (4, 16, 32), dtype=dtype)
    outs = [g(s, TORCH_DT[np.dtype(dtype)]) for s in terafly.level_shapes(slab.shape, 2, hd)]
    terafly.pyramid_slab(g.like(slab, off), 2, hd, method, outs)
    a = slab
    for k, h in enumerate(hd):
        a = TU.halve3d(a, method) if h else TU.halve2d(a, method)
        np.testing.assert_array_equal(host(outs[k]), a, err_msg=f"level {k + 1}")   # test_pyramid_slab_equals_restatement
    g.check()


@pytest.mark.parametrize("dtype,off", INT_CASES + [(np.float32, 1), (np.float32, 2)], ids=INT_IDS + ["float32+1", "float32+2"])
def test_isodown_halving_of_an_offset_stack(dev, g, dtype, off):
    """isodown.hip, halve_kernel<T, VEC>: case V of tests/isodown_util.py, rows of 48 samples (a multiple of 16 / sizeof(T))."""
    from ipp_amd import parallel_image_processor as pip
    shape, voxel, target = IU.CASES["V"]
    assert shape[1] % 16 == 0
    stack = np.stack([IU.pattern(shape, dtype, seed) for seed in (1, 2)])
    want_plan = IU.plan(shape, voxel, target)
    plan = pip.Plan(dev, shape, dtype, voxel, target)
    try:
        halved, differs = plan.halve(g.like(stack, off))
        halved_a, differs_a = plan.halve(g.like(stack))
        planes, planes_a = plan.planes(g.like(stack, off)), plan.planes(g.like(stack))
    finally:
        plan.close()
    halved, planes = halved.cpu().numpy(), planes.cpu().numpy()
    assert np.array_equal(halved, halved_a.cpu().numpy()) and np.array_equal(planes, planes_a.cpu().numpy())
    assert differs.cpu().tolist() == differs_a.cpu().tolist() == [1, 1]
    for k in range(2):
        want = IU.halve_chain(stack[k], want_plan)
        assert np.array_equal(halved[k], want)                                     # test_halving_chain_is_bit_identical
        err = float(np.abs(planes[k].astype(np.float64) - IU.slice_plane(stack[k], want_plan)).max()) / float(np.abs(want).max())
        assert err <= ISODOWN_TOL, err                                               # test_slice_plane
    g.check()


@pytest.mark.parametrize("dtype,off", INT_CASES, ids=INT_IDS)
def test_pystripe_run_on_an_offset_batch(dev, g, dtype, off):
    """pystripe.hip (launch_uniform), uniform_kernel<T, VEC>: tiles of 33 x 64 samples (a multiple of 16 bytes each), one of them uniform."""
    from ipp_amd import pystripe as ps
    tiles = np.stack([PU.synthetic_tile((33, 64), 100 + i, dtype, "rows" if i % 2 else "cols") for i in range(3)])
    tiles[1] = 123
    assert tiles[0].nbytes % 16 == 0
    prm = ps.make_params(dtype, sigma=(8, 8), wavelet="db9", padding_mode="reflect", bidirectional=True, max_batch=3)
    plan = ps.Plan(dev, tiles.shape[1:], dtype, prm)
    try:
        out = g((3,) + plan.out_shape, TORCH_DT[np.dtype(plan.out_dtype)])
        plan.run(g.like(tiles, off), out=out)
        aligned = host(plan.run(g.like(tiles)))
    finally:
        plan.close()
    got = host(out)
    assert np.array_equal(got, aligned)
    assert not got[1].any() and got[0].any() and got[2].any()      # the uniform tile was recognised, its neighbours were not
    g.check()


def _merge(dev, g, stacks, av, ah, ad, blending, box, off):
    from ipp_amd import merge
    R_, C_ = av.shape
    N, Hs, Ws = stacks[0][0].shape
    geo = merge.Geometry(R_, C_, av.astype(np.int32), ah.astype(np.int32), ad.astype(np.int32), Hs, Ws, N, SU.volume_dims(av, ah, ad, Hs, Ws, N))
    D0, D1, V0, V1, H0, H1 = box
    d0v = geo.dims[4]
    dst = [[g.like(np.ascontiguousarray(stacks[r][c][D0 + d0v - ad[r, c]:D1 + d0v - ad[r, c]])) for c in range(C_)] for r in range(R_)]
    out = g((D1 - D0, V1 - V0, H1 - H0), TORCH_DT[stacks[0][0].dtype], off)
    merge.merge_slab(geo, dst, stacks[0][0].dtype, blending, D0, D1, V0, V1, H0, H1, out)
    g.check()
    return host(out)


@pytest.mark.parametrize("dtype,off", INT_CASES, ids=INT_IDS)
@pytest.mark.parametrize("blending", [SU.SINBLEND, SU.NOBLEND], ids=["sin", "noblend"])
def test_merge_slab_into_an_offset_box(dev, g, dtype, off, blending):
    """stitch.hip, merge_kernel: eight samples per store (uint4 / uint2) where the address allows, else one by one.  The two-by-two
    grid of test_merge_slab_refuses_bad_boxes with data; uint16 + 4 (8 bytes) leaves no uint4 store legal, uint8 + 8 keeps the uint2 stores."""
    from tests.test_gpu_stitch_merge import _rand_grid
    stacks, av, ah, ad = _rand_grid(np.random.default_rng(3), 2, 2, 16, 16, 4, 4, 4, dtype)
    ad[:] = 0
    V0, V1, H0, H1, D0, D1 = SU.volume_dims(av, ah, ad, 16, 16, 4)
    box = (0, D1 - D0, 0, V1 - V0, 0, 24)
    assert H1 - H0 >= 24 and (box[5] - box[4]) % 8 == 0
    got = _merge(dev, g, stacks, av, ah, ad, blending, box, off)
    assert np.array_equal(got, _merge(dev, g, stacks, av, ah, ad, blending, box, 0))
    assert np.array_equal(got, SU.merge_volume(stacks, av, ah, ad, blending)[:, :, :24])   # test_merge_slab_matches_the_restatement


@pytest.mark.parametrize("off", INT_OFFS[np.uint16])
def test_device_tiff_writer_reads_an_offset_volume(dev, g, tmp_path, off):
    """tiff_deflate.hip, strip_bytes: 16-byte loads when the strip starts on a 16-byte boundary, else byte by byte."""
    from ipp_amd import brickio
    vol = (np.cumsum(np.random.default_rng(11).standard_normal((3, 17, 32)), axis=2) * 30 + 20000).clip(0, 65535).astype(np.uint16)
    assert brickio.save_tiff_series_device(tmp_path / "d", g.like(vol, off)) == 3
    assert np.array_equal(brickio.load_tiff_series(tmp_path / "d"), vol)    # test_slices_deflated_on_the_device_read_back_exactly
    g.check()
