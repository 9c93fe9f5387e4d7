"""Per-bin transfer-function checks of the FFT convolution pipeline: the probe, the PSFs, the metric and the float32 yardstick.

Plain numpy / scipy in float64, no device code.  A circular convolution is diagonal in frequency: fftn(conv(x)) = fftn(x) * H.  With a
probe x whose spectrum has the same magnitude on every bin, and a PSF whose OTF H is nowhere small, fftn(got) / fftn(x) recovers H on
every single bin, and one wrong bin shows as an error of its own size -- not divided by the largest output value of the volume, which
is how a spatial-domain bound sees it."""
import numpy as np
import scipy.fft as sfft
from scipy import ndimage

from oracle import rl_oracle as R

WORKERS = 8  # threads of the reference transforms

# Every length the hand-written pipeline takes (fft_native.hip, split_axis), written out: 2^a (a = 3..12), 3 * 2^a and 9 * 2^a
# (a = 5..9), on y also 5 * 2^a (a = 5..8); x is stated as the real extent 2 * Hx; z ends at 2304.
NATIVE_LENGTHS = {
    "x": [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 192, 384, 768, 1536, 3072, 576, 1152, 2304, 4608, 9216],
    "y": [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 96, 192, 384, 768, 1536, 160, 320, 640, 1280, 288, 576, 1152, 2304, 4608],
    "z": [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 96, 192, 384, 768, 1536, 288, 576, 1152, 2304],
}

# The case lists of tests/test_gpu_fft_spectral.py (shapes are (z, y, x)); tests/test_spectral_probe_host.py measures the float32
# yardstick on the same lists.
AXIS_SHAPES = ([(16, 16, n) for n in NATIVE_LENGTHS["x"]] + [(16, n, 16) for n in NATIVE_LENGTHS["y"]]
               + [(n, 16, 16) for n in NATIVE_LENGTHS["z"]])
MIXED_SHAPES = [(96, 160, 576), (288, 320, 192), (192, 96, 1152),  # no axis trivial, the radices differ
                (64, 1024, 32),                                    # the fast path of k_y_pair
                (64, 32, 2048), (64, 32, 4096),                    # rotated x positions
                (1152, 32, 64), (128, 128, 256)]
# the RL context: the mixed shapes plus one short, one middle and the longest length of every axis
CTX_SHAPES = MIXED_SHAPES + [(16, 16, 16), (16, 16, 768), (16, 16, 9216), (16, 8, 16), (16, 320, 16), (16, 4608, 16),
                             (8, 16, 16), (384, 16, 16), (2304, 16, 16)]
ROCFFT_ONLY_SHAPES = [(15, 21, 50), (30, 44, 70), (17, 64, 96)]  # shapes the native plan refuses
KSHAPE = (5, 7, 9)

# The bounds: 8 x the largest float32 yardstick (scipy.fft in complex64) over the case list, rounded up to one significant digit.
# The measured maxima are in DESIGN.md section 15; tests/test_spectral_probe_host.py asserts yardstick <= bound / 8 for every case.
FWD_BOUND = 8e-6        # no DC term, every bin                                     (largest yardstick 9.4e-7)
CTX_BOUND_FINE = 2e-3   # DC-carrying probe, the bins outside dc_lines              (largest yardstick 1.9e-4)
CTX_BOUND_LINES = 9e-3  # DC-carrying probe, the three lines of bins through DC     (largest yardstick 1.1e-3)


def _fftn64(a):
    return sfft.fftn(np.asarray(a, dtype=np.float64), workers=WORKERS)


def flat_probe(shape, seed):
    """Real float32 volume whose DFT has magnitude sqrt(N) on every bin, with random phases (the DC bin included: its mean is
    +-1 / sqrt(N)).  The float32 rounding is part of the input: references start from fftn(float64(x32))."""
    rng = np.random.default_rng(seed)
    f = _fftn64(rng.standard_normal(shape))
    f /= np.abs(f)
    x = sfft.ifftn(f, workers=WORKERS).real * np.sqrt(float(np.prod(shape)))
    return np.ascontiguousarray(x.astype(np.float32))


def probe_psf(kshape, seed, symmetric, shape=None):
    """Float32 PSF of sum 1 that is not low-pass: random positive samples of sum 0.4 plus 0.6 on one tap, so |H| >= 0.2 on every bin
    of any grid.  ``symmetric``: the samples are made point-symmetric and the tap is the centre sample (odd extents), so the PSF is
    exactly mirror-symmetric about it; otherwise the tap lies off the centre.  Asserts min |H| >= 0.3 * max |H| on the grid ``shape``
    (callers that build the OTF of the grid anyway pass no shape and hand that OTF to ``assert_not_lowpass``)."""
    assert all(k % 2 == 1 for k in kshape)
    rng = np.random.default_rng(7000 + seed)
    p = rng.random(kshape) + 0.05
    centre = tuple(k // 2 for k in kshape)
    if symmetric:
        p = p + p[::-1, ::-1, ::-1]
        tap = centre
    else:
        tap = tuple(max(c - 1, 0) for c in centre)
    p *= 0.4 / p.sum()
    p[tap] += 0.6
    p = p.astype(np.float32)
    if symmetric:
        assert np.array_equal(p, p[::-1, ::-1, ::-1])
    else:
        assert not np.allclose(p, p[::-1, ::-1, ::-1], rtol=1e-2)
    if shape is not None:
        assert_not_lowpass(otf_rl(p, shape))
    return p


def assert_not_lowpass(H):
    mag = np.abs(H)
    assert mag.min() >= 0.3 * mag.max(), (H.shape, float(mag.min()), float(mag.max()))


def otf_rl(psf, shape):
    """The OTF of an RL context on the circular rule: deconFFT's placement (decon.m:131-133)."""
    return R.otf_from_psf(psf, shape)


def otf_convn(ker, shape):
    """The OTF of ``mi_conv3d`` on the circular rule, which is centred like convn: the transform of the kernel's response to a delta
    at the origin.  (The response is taken on the smallest grid that holds the kernel without wrapping onto itself and moved, by
    signed index, onto the full grid: the same array as ndimage.convolve on the full grid, tests/test_spectral_probe_host.py.)"""
    small = tuple(min(n, 2 * k) for n, k in zip(shape, ker.shape))
    delta = np.zeros(small)
    delta[0, 0, 0] = 1.0
    resp = ndimage.convolve(delta, ker.astype(np.float64), mode="wrap")
    if small == tuple(shape):
        return _fftn64(resp)
    full = np.zeros(shape)
    idx = [np.where(np.arange(s) < (s + 1) // 2, np.arange(s), np.arange(s) - s) % n for s, n in zip(small, shape)]
    full[np.ix_(*idx)] = resp
    return _fftn64(full)


def transfer_error(got, x32, H, X=None):
    """|fftn(float64(got)) / X - H| / |H| per bin (the full array), X = fftn(float64(x32)) (``X``: that array, where the caller
    has it already).  No bin of the probe may be dead."""
    if X is None:
        X = _fftn64(x32)
    n = float(np.prod(x32.shape))
    assert np.abs(X).min() > 0.5 * np.sqrt(n), "the probe has a dead bin"
    G = _fftn64(got)
    G /= X
    G -= H
    return np.abs(G) / np.abs(H)


def dc_lines(shape):
    """Mask of the bins with at least two zero frequency coordinates: the three lines through DC."""
    z, y, x = ((np.arange(n) == 0).astype(np.int8) for n in shape)
    return (z[:, None, None] + y[None, :, None] + x[None, None, :]) >= 2


def conv64(x32, H):
    """real(ifftn(fftn(x) .* H)) in float64."""
    return sfft.ifftn(_fftn64(x32) * H, workers=WORKERS).real


def dc_probe(w32, psf, H):
    """The probe of the RL context, whose half-steps clamp or take abs: x = dc + w with dc = 1.25 * max |conv64(w)| / sum(psf)."""
    dc = 1.25 * float(np.abs(conv64(w32, H)).max()) / float(psf.astype(np.float64).sum())
    return np.ascontiguousarray((w32.astype(np.float64) + dc).astype(np.float32))


def conv_complex64(x32, H):
    """The float32 yardstick: the same convolution through scipy.fft in complex64, H cast to complex64."""
    X = sfft.fftn(x32.astype(np.complex64), workers=WORKERS)
    assert X.dtype == np.complex64
    X *= H.astype(np.complex64)
    return np.ascontiguousarray(sfft.ifftn(X, workers=WORKERS).real.astype(np.float32))


def yardstick_forward(shape, symmetric):
    """max transfer error of the complex64 convolution on the case (shape, PSF) of the forward test."""
    x, ker, H = forward_case(shape, symmetric)
    return float(transfer_error(conv_complex64(x, H), x, H).max())


def yardstick_ctx(shape, symmetric):
    """(max outside dc_lines, max inside) of the complex64 convolution on the DC-carrying probe of the context test."""
    x, psf, H = ctx_case(shape, symmetric)
    err = transfer_error(conv_complex64(x, H), x, H)
    lines = dc_lines(shape)
    return float(err[~lines].max()), float(err[lines].max())


def case_seed(shape, symmetric):
    return shape[0] * 1000003 + shape[1] * 1009 + shape[2] + int(symmetric)


def forward_case(shape, symmetric, otf=otf_convn):
    """(probe, kernel, float64 OTF) of one forward case."""
    seed = case_seed(shape, symmetric)
    ker = probe_psf(KSHAPE, seed, symmetric)
    H = otf(ker, shape)
    assert_not_lowpass(H)
    return flat_probe(shape, seed), ker, H


def ctx_case(shape, symmetric):
    """(DC-carrying probe, PSF, float64 OTF) of one RL-context case."""
    seed = case_seed(shape, symmetric)
    psf = probe_psf(KSHAPE, seed, symmetric)
    H = otf_rl(psf, shape)
    assert_not_lowpass(H)
    return dc_probe(flat_probe(shape, seed), psf, H), psf, H


def freq2pos(k, n):
    """Where the pipeline keeps frequency k of an axis of length n = r * 2^l (r in 1, 3, 5, 9; fft_native_dev.h, freq2pos): one
    radix-r decimation-in-frequency stage, then r bit-reversed power-of-two transforms."""
    r = next(r for r in (1, 3, 5, 9) if n % r == 0 and (n // r) & (n // r - 1) == 0)
    l2 = (n // r).bit_length() - 1
    k2, k1 = divmod(k, r)
    return (k1 << l2) + (int(format(k2, "b").zfill(l2)[::-1], 2) if l2 else 0)


def permuted_position(bin_zyx, shape):
    """(pz, py, px) of a bin in the pipeline's arrays; x: the plane xk = min(kx, Nx - kx) of the half spectrum on Hx = Nx / 2
    complex points (working index of xk mod Hx, and the rotated order of Hx = 1024, 2048), which it shares with its mirror partner."""
    kz, ky, kx = (int(v) for v in bin_zyx)
    nz, ny, nx = shape
    hx = nx // 2
    w = freq2pos(min(kx, nx - kx) % hx, hx)
    if hx in (1024, 2048):
        w = ((w & 7) << (hx.bit_length() - 4)) | (w >> 3)
    return freq2pos(kz, nz), freq2pos(ky, ny), w


def describe_worst(err, shape):
    """The worst bin of an error array, for assertion messages."""
    b = np.unravel_index(int(np.argmax(err)), err.shape)
    return f"{float(err[b]):.3e} at bin (kz, ky, kx) = {tuple(int(v) for v in b)}, permuted position {permuted_position(b, shape)}"
