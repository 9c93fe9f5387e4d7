"""The PSF family and float64 references of the real-OTF decision tests (fft_native_yz.hip, NativeFft::try_real_otf).

psf(eps) = float32(normalise(G + eps * A)): G a symmetric Gaussian, A a seeded antisymmetric pattern of the same peak value, so
that eps sweeps the imaginary part of the centred OTF from rounding noise through the library's threshold to plainly complex.
Plain numpy in float64, no device code."""
import numpy as np

from oracle import rl_oracle as R

KSHAPE = (7, 5, 9)
SIGMA = (1.5, 1.0, 2.0)
EPS = [0.0, 1e-7, 1e-6, 3e-6, 1e-5, 3e-5, 1e-4, 1e-2]
# NativeFft::try_real_otf keeps the real part only when max|Im| <= 4e-6 * max|Re| after removing the phase ramp of the centre
# sample (image-preprocessing-pipeline_amd/csrc/fft_native_yz.hip:1092)
THRESHOLD = 4e-6
# bounds of tests/test_gpu_pair_layout.py::test_paired_layout_equals_plain_layout_and_float64, which the GPU test reuses
BOUNDS = dict(rel=2e-5, rel_l2=2e-6, pt_rel=2e-5)
PAIRED_SHAPE = (64, 16, 32)
PLAIN_SHAPE = (2304, 16, 16)   # of spectral_util.CTX_SHAPES: z = 9 * 2^8 is past the paired z pass, and a multiple of 64


def psf_family(eps):
    g = R.gaussian_psf(KSHAPE, SIGMA).astype(np.float64)
    a = np.random.default_rng(4242).random(KSHAPE)
    a = a - a[::-1, ::-1, ::-1]
    a *= g.max() / np.abs(a).max()
    p = g + eps * a
    return np.ascontiguousarray((p / p.sum()).astype(np.float32))


def imag_ratio(psf, shape):
    """max|Im| / max|Re| of the OTF of ``psf`` on the grid ``shape`` with the centre sample (index k // 2) at the origin."""
    p = np.zeros(shape, np.float64)
    idx = [(np.arange(k) - k // 2) % f for k, f in zip(psf.shape, shape)]
    p[np.ix_(*idx)] = psf.astype(np.float64)
    otf = np.fft.fftn(p)
    return float(np.abs(otf.imag).max() / np.abs(otf.real).max()), otf


def operands(shape):
    """The GPU test's two operands: rand + 0.5, seeded by the shape."""
    rng = np.random.default_rng(sum(shape))
    return (rng.random(shape) + 0.5).astype(np.float32), (rng.random(shape) + 0.5).astype(np.float32)


def circular_pair(a, b, otf):
    """(conv(a), conv_adj(b)) in float64: decon.m:162-172, real(ifftn(fftn(x) .* otf)) and its conjugate."""
    fwd = np.real(np.fft.ifftn(np.fft.fftn(a.astype(np.float64)) * otf))
    adj = np.real(np.fft.ifftn(np.fft.fftn(b.astype(np.float64)) * np.conj(otf)))
    return fwd, adj


def errors(got, want):
    """The three figures ``rl_util.assert_close`` bounds: (max error / max, relative L2, worst point-wise error / allowance) with
    the point-wise allowance at ``BOUNDS['pt_rel']`` and assert_close's default floor."""
    d = np.abs(got - want)
    wmax = float(np.abs(want).max())
    allow = BOUNDS["pt_rel"] * np.abs(want) + 1e-7 * max(1.0, wmax)
    return float(d.max() / wmax), float(np.sqrt((d * d).sum() / (want * want).sum())), float((d / allow).max())
