"""CPU: what dropping the imaginary part of an almost-real OTF costs, in float64, on the PSF family of the GPU test
(tests/test_gpu_real_otf_decision.py).  Whenever the library's criterion would keep the real part only, the float64 result of doing so
stays within one fifth of every bound the GPU test applies -- the other four fifths are there for float32."""
import numpy as np
import pytest

from tests import real_otf_util as U

SHAPES = [U.PAIRED_SHAPE, U.PLAIN_SHAPE, (128, 32, 64)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def sweep(request):
    """Per eps: (ratio, errors of the forward result, errors of the adjoint result) of the real-only OTF against the full one."""
    shape = request.param
    a, b = U.operands(shape)
    fa, fb = np.fft.fftn(a.astype(np.float64)), np.fft.fftn(b.astype(np.float64))
    rows = []
    for eps in U.EPS:
        # in the frame of the centre sample, where the library takes the real part; placing the PSF as the reference does multiplies
        # both OTFs by one phase ramp, a circular shift of both results alike
        ratio, otf = U.imag_ratio(U.psf_family(eps), shape)
        full = (np.real(np.fft.ifftn(fa * otf)), np.real(np.fft.ifftn(fb * np.conj(otf))))
        real = (np.real(np.fft.ifftn(fa * otf.real)), np.real(np.fft.ifftn(fb * otf.real)))
        rows.append((eps, ratio, U.errors(real[0], full[0]), U.errors(real[1], full[1])))
    return shape, rows


def test_real_only_otf_below_the_threshold_stays_within_a_fifth_of_the_gpu_bounds(sweep):
    shape, rows = sweep
    for eps, ratio, ef, ea in rows:
        print(f"{shape} eps {eps:g}: ratio {ratio:.2e}  fwd max {ef[0]:.2e} l2 {ef[1]:.2e} pt {ef[2]:.2f}x  adj max {ea[0]:.2e} l2 {ea[1]:.2e} pt {ea[2]:.2f}x")
    for eps, ratio, ef, ea in rows:
        if ratio <= U.THRESHOLD:
            for e in (ef, ea):
                assert e[0] <= U.BOUNDS["rel"] / 5, (eps, ratio, e)
                assert e[1] <= U.BOUNDS["rel_l2"] / 5, (eps, ratio, e)
                assert e[2] <= 1 / 5, (eps, ratio, e)


def test_family_brackets_the_threshold(sweep):
    """The sweep has PSFs on both sides of the criterion and the ratio grows with eps: eps = 0 is rounding noise, eps >= 1e-4 lies
    an order of magnitude past the threshold (where the GPU test asserts the complex form)."""
    _, rows = sweep
    ratios = [r[1] for r in rows]
    assert ratios[0] < 1e-3 * U.THRESHOLD
    assert all(x < y for x, y in zip(ratios[1:], ratios[2:]))
    assert ratios[U.EPS.index(3e-6)] < U.THRESHOLD < ratios[U.EPS.index(1e-5)]
    assert ratios[U.EPS.index(1e-4)] > 10 * U.THRESHOLD
