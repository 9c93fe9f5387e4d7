"""GPU: what process_img gained beside the automatic clips -- ``down_sample_method='median'`` (block_reduce with numpy.median: zero
padding to a block multiple, division by flat first, the mean of the two middle values of an even block), ``new_size`` and
``threshold``.  The median has no rounding of its own (a middle value, or half the sum of two float32 values taken in float64), so
the results equal the restatement of tests/autoclips_util.py exactly.
"""
import numpy as np
import pytest

from tests import autoclips_util as A
from tests import pystripe_util as U
from tests import thresholds_util as T

pytestmark = pytest.mark.gpu

BLOCKS = [(2, 2), (3, 2), (1, 5), (8, 8)]
SHAPES = [(37, 50), (64, 64)]


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


def tile(shape, kind, seed):
    if kind == "f32":
        return A.float_tile(shape, seed)
    return T.four_mode_image(shape, seed, np.uint8 if kind == "u8" else np.uint16)


@pytest.mark.parametrize("kind", ["u8", "u16", "f32", "u16_flat"])
@pytest.mark.parametrize("shape", SHAPES)
def test_median_equals_block_reduce(ps, dev, shape, kind):
    img = tile(shape, kind.split("_")[0], 50)
    flat = A.flat_field(shape) if kind.endswith("flat") else None
    for block in BLOCKS:
        kw = dict(down_sample=block, down_sample_method="median")
        assert ps.derive(shape, img.dtype, ps.make_params(img.dtype, flat=flat is not None, extended=True, **kw)).integer_kind == 0
        want, _ = A.process_img(img.copy(), flat=flat, **kw)
        got = ps.process_img(img.copy(), flat=flat, device=dev, extended=True, **kw)
        assert got.dtype == want.dtype and got.shape == want.shape == U.down_sampled_size(shape, block)
        assert np.array_equal(got, want), (kind, shape, block, np.abs(got.astype(np.float64) - want).max())
        # the float tile itself, halves included
        want32 = A.reduced(img, flat, block, "median").astype(np.float32)
        got32 = ps.process_img(img.copy(), flat=flat, d_type=np.float32, device=dev, extended=True, **kw)
        assert np.array_equal(got32, want32), (kind, shape, block)
    if kind == "u16":
        assert (A.reduced(img, None, (2, 2), "median") % 1 == 0.5).any()      # even blocks do produce halves


def test_median_in_a_stack_and_with_the_tail(ps, dev):
    stack = np.stack([T.four_mode_image((37, 50), 51 + i) for i in range(3)])
    kw = dict(down_sample=(3, 2), down_sample_method="Median", dark=120, convert_to_8bit=True, bit_shift_to_right=4, rotate=90)
    got = ps.process_img(stack, device=dev, extended=True, **kw)
    for i in range(3):
        want, _ = A.process_img(stack[i].copy(), **dict(kw, down_sample_method="median"))
        assert np.array_equal(got[i], want)


def test_median_block_of_more_than_64_samples_is_refused_by_name(ps, dev):
    img = T.four_mode_image((37, 50), 52)
    with pytest.raises(NotImplementedError, match="down_sample=\\(9, 8\\).*median"):
        ps.process_img(img, down_sample=(9, 8), down_sample_method="median", extended=True, device=dev)
    ps.process_img(img, down_sample=(9, 8), down_sample_method="mean", device=dev)


def test_new_size_in_process_img(ps, dev):
    img = T.four_mode_image((37, 41), 53)
    for kw in (dict(), dict(dark=100, convert_to_8bit=True, bit_shift_to_right=5, rotate=90), dict(sigma=(8, 8), wavelet="db9", padding_mode="reflect")):
        tail = {k: kw[k] for k in ("convert_to_8bit", "bit_shift_to_right", "rotate") if k in kw}
        head = {k: v for k, v in kw.items() if k not in tail}
        want = ps.process_img(ps.resize_tiles(ps.process_img(img.copy(), device=dev, **head), (53, 61), device=dev), device=dev, **tail)
        got = ps.process_img(img.copy(), new_size=(53, 61), device=dev, extended=True, **kw)
        assert got.dtype == want.dtype and np.array_equal(got, want), kw
        assert got.shape == ((61, 53) if kw.get("rotate") == 90 else (53, 61))
    assert np.array_equal(ps.process_img(img.copy(), new_size=(37, 41), extended=True, device=dev), img)
    uniform = ps.process_img(np.full((37, 41), 9, np.uint16), new_size=(53, 61), rotate=90, extended=True, device=dev)
    assert uniform.shape == (61, 53) and not uniform.any()
    with pytest.raises(NotImplementedError, match="new_size"):
        ps.process_img(img.copy(), new_size=(53, 30), extended=True, device=dev)       # below as a tuple, and an axis shrinks


def test_threshold_is_accepted(ps, dev):
    img = U.synthetic_tile((75, 101), 54, np.uint16)
    pipe = dict(wavelet="db9", padding_mode="reflect", bidirectional=True, device=dev, extended=True)
    plain = ps.process_img(img.copy(), sigma=(8, 16), **pipe)
    assert np.array_equal(ps.process_img(img.copy(), sigma=(8, 16), threshold=5.0, **pipe), plain)
    assert np.array_equal(ps.filter_streaks(img.copy(), sigma=(8, 16), threshold=5.0, **pipe), ps.filter_streaks(img.copy(), sigma=(8, 16), **pipe))
    single = ps.process_img(img.copy(), sigma=(8, 8), **pipe)
    assert not np.array_equal(single, plain)
    assert np.array_equal(ps.process_img(img.copy(), sigma=(8, 16), threshold=-1.0, **pipe), single)
    assert np.array_equal(ps.filter_streaks(img.copy(), sigma=(8, 16), threshold=0, **pipe), ps.filter_streaks(img.copy(), sigma=(8, 8), **pipe))
    with pytest.raises(NotImplementedError, match="threshold"):
        ps.process_img(img.copy(), sigma=(0, 16), threshold=-1.0, **pipe)
