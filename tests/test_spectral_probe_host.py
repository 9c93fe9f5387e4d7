"""CPU: the per-bin transfer-function metric of tests/spectral_util.py.  It catches mistakes confined to a few frequency bins, its
bounds are margins over a measured float32 FFT (scipy.fft in complex64), and the list of lengths it sweeps on the GPU
(tests/test_gpu_fft_spectral.py) is the library's."""
import numpy as np
import pytest
import scipy.fft as sfft
from scipy import ndimage

from tests import spectral_util as S


def _seeded(P, mistake):
    """The float64 product spectrum P = X .* H with one mistake; Hermitian symmetry is kept, as a real pipeline keeps it."""
    nz, ny, nx = P.shape
    Q = P.copy()
    if mistake == "conj_plane":            # the self-mirrored plane kx = Nx / 2
        Q[:, :, nx // 2] = np.conj(Q[:, :, nx // 2])
    elif mistake == "pair_scaled":         # one bin and its mirror partner
        b = (nz // 2 - 1, ny // 4 + 1, nx // 4 + 1)
        Q[b] *= 1.5
        Q[tuple((-k) % n for k, n in zip(b, P.shape))] *= 1.5
    elif mistake == "bin_zeroed":
        Q[nz // 2, ny // 2, nx // 2] = 0.0
    elif mistake == "line_rotated":        # one z line of bins and its mirror line
        ky, kx = ny // 4 + 1, nx // 2 - 1
        Q[:, ky, kx] *= np.exp(0.3j)
        Q[:, -ky, -kx] *= np.exp(-0.3j)
    else:
        raise ValueError(mistake)
    return Q


@pytest.mark.parametrize("shape", [(8, 8, 16), (96, 288, 64), (2304, 16, 16), (8, 8, 9216)])
def test_metric_catches_mistakes_confined_to_a_few_bins(shape):
    for symmetric in (False, True):
        x, ker, H = S.forward_case(shape, symmetric)
        P = sfft.fftn(x.astype(np.float64)) * H
        clean = sfft.ifftn(P).real.astype(np.float32)
        assert S.transfer_error(clean, x, H).max() < S.FWD_BOUND / 8     # the float32 rounding of the result alone
        for mistake in ("conj_plane", "pair_scaled", "bin_zeroed", "line_rotated"):
            got = sfft.ifftn(_seeded(P, mistake)).real.astype(np.float32)
            worst = float(S.transfer_error(got, x, H).max())
            print(shape, symmetric, mistake, f"{worst:.3e}")
            assert worst >= 100 * S.FWD_BOUND, (mistake, worst)
            # the DC-carrying probe sees it as well, on bins outside the lines through DC
            assert worst >= 100 * S.CTX_BOUND_FINE, (mistake, worst)


@pytest.mark.parametrize("shape", S.AXIS_SHAPES + S.MIXED_SHAPES, ids=str)
def test_float32_yardstick_of_the_forward_cases(shape):
    """scipy.fft in complex64 on the same probe stays under an eighth of FWD_BOUND."""
    for symmetric in (False, True):
        y = S.yardstick_forward(shape, symmetric)
        print("yardstick fwd", shape, symmetric, f"{y:.3e}")
        assert y <= S.FWD_BOUND / 8


@pytest.mark.parametrize("shape", S.ROCFFT_ONLY_SHAPES, ids=str)
def test_float32_yardstick_of_the_rocfft_only_cases(shape):
    for symmetric in (False, True):
        y = S.yardstick_forward(shape, symmetric)
        print("yardstick fwd", shape, symmetric, f"{y:.3e}")
        assert y <= S.FWD_BOUND / 8


@pytest.mark.parametrize("shape", S.CTX_SHAPES, ids=str)
def test_float32_yardstick_of_the_context_cases(shape):
    """The DC-carrying probe: a large DC bin costs a float32 FFT accuracy on the three lines of bins through DC, so these carry a
    bound of their own."""
    for symmetric in (False, True):
        fine, lines = S.yardstick_ctx(shape, symmetric)
        print("yardstick ctx", shape, symmetric, f"fine {fine:.3e} lines {lines:.3e}")
        assert fine <= S.CTX_BOUND_FINE / 8
        assert lines <= S.CTX_BOUND_LINES / 8


def test_dc_probe_keeps_both_half_steps_positive():
    for shape in [(8, 8, 16), (96, 288, 64)]:
        for symmetric in (False, True):
            x, psf, H = S.ctx_case(shape, symmetric)
            assert S.conv64(x, H).min() > 0.25 and S.conv64(x, np.conj(H)).min() > 0.25


def test_probe_and_masks():
    shape = (12, 10, 16)
    x = S.flat_probe(shape, 3)
    assert x.dtype == np.float32 and x.shape == shape
    mag = np.abs(np.fft.fftn(x.astype(np.float64))) / np.sqrt(x.size)
    assert np.abs(mag - 1.0).max() < 1e-5
    assert abs(abs(float(x.astype(np.float64).mean())) - 1.0 / np.sqrt(x.size)) < 1e-6
    m = S.dc_lines(shape)
    assert m.sum() == sum(shape) - 2 and m[0, 0, 5] and m[3, 0, 0] and m[0, 7, 0] and not m[0, 1, 1]
    X = np.fft.fftn(x.astype(np.float64))
    X[2, 5, 3] = X[-2, -5, -3] = 0.0
    with pytest.raises(AssertionError, match="dead bin"):
        S.transfer_error(x, np.fft.ifftn(X).real.astype(np.float32), np.ones(shape))


@pytest.mark.parametrize("shape", [(8, 8, 16), (16, 288, 64), (40, 16, 18)])
def test_convn_otf_is_the_response_to_a_delta_at_the_origin(shape):
    rng = np.random.default_rng(5)
    ker = rng.random(S.KSHAPE).astype(np.float32)
    delta = np.zeros(shape)
    delta[0, 0, 0] = 1.0
    want = np.fft.fftn(ndimage.convolve(delta, ker.astype(np.float64), mode="wrap"))
    assert np.abs(S.otf_convn(ker, shape) - want).max() < 1e-12
    # and it is the operator of scipy's circular convolution
    x = rng.standard_normal(shape)
    conv = ndimage.convolve(x, ker.astype(np.float64), mode="wrap")
    assert np.abs(np.fft.ifftn(np.fft.fftn(x) * want).real - conv).max() < 1e-12


def test_permuted_positions():
    assert [S.freq2pos(k, 8) for k in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7]
    assert sorted(S.freq2pos(k, 96) for k in range(96)) == list(range(96))
    assert S.freq2pos(4, 96) == (1 << 5) + 16 and S.freq2pos(7, 160) == (2 << 5) + 16      # k = k1 + r * k2 -> (k1 << l) + brev(k2)
    assert S.permuted_position((0, 0, 0), (8, 8, 4096)) == (0, 0, 0)
    assert S.permuted_position((1, 1, 4096 - 1), (8, 8, 4096)) == (4, 4, ((1024 & 7) << 8) | (1024 >> 3))


def test_native_lengths_are_the_librarys():
    """mi_fft_good_size(n, axis) == n exactly for the lengths of NATIVE_LENGTHS; past the longest one the answer is 0."""
    from ipp_amd import capi
    g = capi.lib().mi_fft_good_size
    assert [len(S.NATIVE_LENGTHS[a]) for a in "xyz"] == [20, 24, 18]
    for axis, name in enumerate("xyz"):
        lengths = set(S.NATIVE_LENGTHS[name])
        assert len(lengths) == len(S.NATIVE_LENGTHS[name])
        for n in range(1, 9301):
            m = g(n, axis)
            assert (m == n) == (n in lengths), (name, n, m)
            larger = [v for v in lengths if v >= n]
            assert m == (min(larger) if larger else 0), (name, n, m)
