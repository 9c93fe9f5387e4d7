"""GPU: the slice estimates (include/mi_thresholds.h, ipp_amd.thresholds) against numpy itself and the numpy restatement of
threshold_multiotsu (tests/thresholds_util.py): equal counts, edges and indices and bit-equal thresholds, no tolerance anywhere."""
import functools

import numpy as np
import pytest

from tests import thresholds_util as tu

pytestmark = pytest.mark.gpu

# less than one work-group; a few; odd with a vector tail; many work-groups
SHAPES = [(7, 9), (48, 80), (67, 131), (513, 1027)]
UP, DOWN = np.float32(np.inf), np.float32(-np.inf)


@functools.lru_cache(maxsize=None)
def log_image(shape):
    img = np.log1p(tu.four_mode_image(shape), dtype=np.float32)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(shape):
    """(histogram, {classes: indices}) of the restatement; asserts on the CPU that the image sits far from a tie: the indices do not
    change when every log sample moves one ulp up or down"""
    img = log_image(shape)
    hist = np.histogram(img.reshape(-1), 256)[0]
    idx = {c: tu.multiotsu_indices(hist, c)[0] for c in (2, 3, 4)}
    for moved in (np.nextafter(img, UP), np.nextafter(img, DOWN)):
        assert tu.multiotsu_indices(np.histogram(moved.reshape(-1), 256)[0], 4)[0].tolist() == idx[4].tolist()
    return hist, idx


def _hist_cases():
    rng = np.random.default_rng(21)
    cases = {f"log-{s[0]}x{s[1]}": lambda s=s: log_image(s)[None] for s in SHAPES}
    uniform = (rng.random((67, 131)) * 9 - 3).astype(np.float32)
    cases["uniform-random"] = lambda: uniform[None]
    # 67 * 131 is odd: the second and third image start off a 16-byte boundary as well
    cases["batch-of-three-ranges"] = lambda: np.stack([log_image((67, 131)), uniform, (uniform * 1e-3 + 40).astype(np.float32)])
    cases["constant"] = lambda: np.full((1, 48, 80), 3.25, np.float32)

    def on_the_edges():
        edges = np.histogram(uniform.reshape(-1), 256)[1]
        return np.clip(np.concatenate([edges, np.nextafter(edges, UP), np.nextafter(edges, DOWN)]), edges[0], edges[-1])[None]
    cases["every-sample-on-or-beside-an-edge"] = on_the_edges

    def one_bin():
        draw = np.random.default_rng(22)
        img = np.full(513 * 1027, 1.0, np.float32)
        elsewhere = draw.random(img.size) < 0.01
        img[elsewhere] = (draw.random(int(elsewhere.sum())) * 10).astype(np.float32)
        return img[None]
    cases["99-percent-in-one-bin"] = one_bin
    return cases


HIST_CASES = _hist_cases()


def _check_hist(images, got):
    rng, bad, edges, counts = got
    for k, img in enumerate(images):
        want_counts, want_edges = np.histogram(img.reshape(-1), 256)
        assert not bad[k]
        assert rng[k].tolist() == [img.min(), img.max()]
        assert np.array_equal(edges[k], want_edges), np.flatnonzero(edges[k] != want_edges)
        assert np.array_equal(counts[k], want_counts), np.flatnonzero(counts[k] != want_counts)


@pytest.mark.parametrize("case", list(HIST_CASES))
def test_hist256_equals_numpy(dev, case):
    from ipp_amd import thresholds as th
    images = HIST_CASES[case]()
    if case == "99-percent-in-one-bin":
        assert np.histogram(images[0], 256)[0].max() >= 0.98 * images[0].size
    _check_hist(images, th.hist256(images, dev))


def test_hist256_unaligned_base(dev):
    import torch
    from ipp_amd import thresholds as th
    img = log_image((67, 131)).reshape(-1)
    for offset in (1, 2, 3):
        buf = torch.zeros(img.size + 8, dtype=torch.float32, device=dev)
        view = buf[offset:offset + img.size]
        view.copy_(torch.from_numpy(img.copy()))
        assert view.data_ptr() % 16 == 4 * offset
        _check_hist(img[None], th.hist256(view.reshape(1, -1)))


def test_hist256_flags_what_is_not_finite(dev):
    from ipp_amd import thresholds as th
    imgs = np.stack([log_image((48, 80))] * 3).copy()
    imgs[0, 5, 7] = np.nan
    imgs[2, 47, 79] = np.inf
    rng, bad, edges, counts = th.hist256(imgs, dev)
    assert bad.tolist() == [1, 0, 1]
    _check_hist(imgs[1:2], (rng[1:2], bad[1:2], edges[1:2], counts[1:2]))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_code_hist_equals_bincount(dev, dtype):
    import torch
    from ipp_amd import thresholds as th
    ncodes = 256 if dtype == np.uint8 else 65536
    for shape in SHAPES:
        img = tu.four_mode_image(shape, dtype=dtype)
        assert np.array_equal(th.code_hist(img[None], dev)[0], np.bincount(img.reshape(-1), minlength=ncodes))
    rng = np.random.default_rng(3)
    # every code of the range, three images of an odd size (so the later ones start off a 16-byte boundary)
    stack = rng.integers(0, ncodes, (3, 67, 131)).astype(dtype)
    stack[1] = tu.four_mode_image((67, 131), seed=4, dtype=dtype)
    got = th.code_hist(stack, dev)
    for k in range(3):
        assert np.array_equal(got[k], np.bincount(stack[k].reshape(-1), minlength=ncodes))
    flat = stack[0].reshape(-1)
    for offset in (1, 3):
        buf = torch.zeros(flat.size + 16, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
        view = buf[offset:offset + flat.size]
        view.copy_(torch.from_numpy(flat.copy()))
        assert view.data_ptr() % 16 == offset * np.dtype(dtype).itemsize
        assert np.array_equal(th.code_hist(view.reshape(1, -1))[0], np.bincount(flat, minlength=ncodes))


@pytest.mark.parametrize("classes", [2, 3, 4])
def test_search_indices_equal_the_restatement(dev, classes):
    from ipp_amd import capi, thresholds as th
    hists = np.stack([reference(s)[0] for s in SHAPES])
    idx, nvalues, status = th.multiotsu_search(hists, classes, dev)
    assert status.tolist() == [capi.OTSU_OK] * len(SHAPES)
    assert nvalues.tolist() == [int(np.count_nonzero(h)) for h in hists]
    for k, s in enumerate(SHAPES):
        print(s, classes, idx[k])
        assert idx[k].tolist() == reference(s)[1][classes].tolist()


def test_search_shortcut_and_too_few_values(dev):
    from ipp_amd import capi, thresholds as th
    rng = np.random.default_rng(8)
    four = rng.choice(np.array([0.5, 2.0, 2.25, 9.0], np.float32), (48, 80))
    three = rng.choice(np.array([0.5, 2.0, 9.0], np.float32), (48, 80))
    hists = np.stack([np.histogram(four.reshape(-1), 256)[0], np.histogram(three.reshape(-1), 256)[0]])
    idx, nvalues, status = th.multiotsu_search(hists, 4, dev)
    assert nvalues.tolist() == [4, 3]
    assert status.tolist() == [capi.OTSU_VALUES_ARE_CLASSES, capi.OTSU_TOO_FEW_VALUES]
    assert idx[0].tolist() == tu.multiotsu_indices(hists[0], 4)[0].tolist()
    assert np.array_equal(th.threshold_multiotsu(four, classes=4), tu.threshold_multiotsu(four, 4))
    with pytest.raises(ValueError, match="only 3 different values"):
        th.threshold_multiotsu(three, classes=4)
    # the same three values split into three classes by the shortcut, into two by the search
    for classes in (3, 2):
        assert np.array_equal(th.threshold_multiotsu(three, classes=classes), tu.threshold_multiotsu(three, classes))


@pytest.mark.parametrize("classes", [2, 3, 4])
def test_search_returns_the_first_of_equal_optima(dev, classes):
    from ipp_amd import thresholds as th
    hist = reference((48, 80))[0]
    mirrored = hist + hist[::-1]       # two mirror-symmetric optima
    sparse = np.zeros(256, np.int64)   # empty bins between the occupied ones: every threshold inside a gap gives the same bits
    sparse[[9, 30, 31, 90, 150, 151, 240]] = [40, 7, 9, 25, 3, 11, 6]
    hists = np.stack([mirrored, sparse])
    idx, _, _ = th.multiotsu_search(hists, classes, dev)
    for k in range(2):
        assert idx[k].tolist() == tu.multiotsu_indices(hists[k], classes)[0].tolist()
    # the tie is real: moving the last threshold of the sparse histogram up inside its gap leaves sigma bit-equal
    _, P1, S1, _ = tu.moments(sparse)
    first = [np.array([v], np.intp) for v in idx[1]]
    later = first[:-1] + [first[-1] + 1]
    assert sparse[idx[1][-1] + 1] == 0 and tu.sigmas(P1, S1, first) == tu.sigmas(P1, S1, later)


def test_threshold_multiotsu_is_bit_equal(dev):
    import torch
    from ipp_amd import thresholds as th
    for shape in ((7, 9), (67, 131)):
        img = log_image(shape)
        want = tu.threshold_multiotsu(img, 4)
        got = th.threshold_multiotsu(img.copy(), classes=4)
        assert got.dtype == np.float32 and got.shape == (3,) and np.array_equal(got, want)
        assert np.array_equal(th.threshold_multiotsu(torch.from_numpy(img.copy()).to(dev), classes=4), want)
    img = log_image((67, 131))
    assert np.array_equal(th.threshold_multiotsu(img.copy()), tu.threshold_multiotsu(img, 3))   # skimage's default: three classes
    assert np.array_equal(th.threshold_multiotsu(img.reshape(-1).copy(), classes=2), tu.threshold_multiotsu(img, 2))   # any shape
    stack = np.stack([img, (img * np.float32(0.5)).astype(np.float32)])
    got = th.threshold_multiotsu_batch(stack, 4)
    assert got.shape == (2, 3)
    assert np.array_equal(got, np.stack([tu.threshold_multiotsu(s, 4) for s in stack]))
    bad = img.copy()
    bad[3, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        th.threshold_multiotsu(bad, classes=4)


def test_estimate_bit_shift(dev):
    import torch
    from ipp_amd import thresholds as th
    img = log_image((67, 131))
    clip_max = tu.threshold_multiotsu(img, 4)[2]
    for threshold, percentile in ((clip_max, 99.99), (clip_max, 99.9), (np.float32(4.0), 50), (np.float32(20.0), 99.9)):
        want = tu.estimate_bit_shift(img, threshold, percentile)[0]
        assert th.estimate_bit_shift(img.copy(), threshold, percentile) == want
        assert th.estimate_bit_shift(torch.from_numpy(img.copy()).to(dev), threshold, percentile) == want


@functools.lru_cache(maxsize=None)
def slice_stack():
    stack = np.stack([tu.four_mode_image((67, 131), seed=100 + z) for z in range(12)])
    stack[6] = 1234     # uniform: the 50 % index must move on to 7
    stack.setflags(write=False)
    return stack


def test_estimate_slice_params(dev, tmp_path):
    import torch
    from ipp_amd import pystripe, thresholds as th
    stack = slice_stack()
    want = tu.estimate_slice_params(stack)
    # an ulp cannot flip the bit shift: every upper bound is at least 2 counts away from every 256 * 2^b
    assert all(abs(bound - 256 * 2 ** b) >= 2 for bound in want["upper_bounds"] for b in range(9)), want["upper_bounds"]
    params = th.estimate_slice_params(stack)
    print(dict(params), params.slices, want)
    assert params.slices == [3, 7, 9] and want["slices"] == [3, 7, 9]
    clips = [params[name] for name in pystripe.BLEACH_CLIPS]
    assert all(type(c) is float for c in clips)
    assert np.array_equal(np.array(clips, np.float32), want["clips"]) and [float(np.float32(c)) for c in clips] == clips
    assert params["dark"] == want["dark"] and type(params["dark"]) is int
    assert params["bit_shift_to_right"] == want["bit_shift_to_right"]
    # ready for process_img
    out = pystripe.process_img(stack[3].copy(), sigma=(0, 0), bleach_correction_frequency=1 / 64, **params)
    assert out.shape == stack[3].shape and out.dtype == stack.dtype
    # a device tensor and a folder of TIFFs give the same
    as_tensor = th.estimate_slice_params(torch.from_numpy(stack.copy()).to(dev))
    assert dict(as_tensor) == dict(params) and as_tensor.slices == params.slices
    for z in range(stack.shape[0]):
        pystripe.imsave_tif(tmp_path / f"img_{z:06d}.tif", stack[z])
    from_folder = th.estimate_slice_params(tmp_path)
    assert dict(from_folder) == dict(params) and from_folder.slices == params.slices
    no_bleach = th.estimate_slice_params(stack, need_bleach_correction=False)
    assert no_bleach["dark"] == 0 and no_bleach["bit_shift_to_right"] == params["bit_shift_to_right"]


def test_estimate_slice_params_runs_out_of_slices(dev):
    from ipp_amd import thresholds as th
    with pytest.raises(ValueError, match="no slice"):
        th.estimate_slice_params(np.full((4, 16, 16), 7, np.uint16))
    # u8 slices of differing content go the same way
    stack = np.stack([tu.four_mode_image((48, 80), seed=z, dtype=np.uint8) for z in range(4)])
    want = tu.estimate_slice_params(stack)
    got = th.estimate_slice_params(stack)
    assert got.slices == want["slices"] and got["dark"] == want["dark"] and got["bit_shift_to_right"] == want["bit_shift_to_right"]
    assert np.array_equal(np.array([got[k] for k in ("bleach_correction_clip_min", "bleach_correction_clip_med", "bleach_correction_clip_max")],
                                   np.float32), want["clips"])
