"""GPU: the value padding modes of the stripe filter (padding_mode constant / linear_ramp / maximum / mean / median / minimum with
``extended=True``; csrc/pystripe_pad.hip) against the restatement of tests/pystripe_pad_util.py, which pads with numpy's own ``pad``.

Standards, the ones of tests/test_gpu_pystripe.py:
  * log domain: max |device - float64 restatement| <= 4 E_ref, E_ref = the float32 restatement's own distance from the float64 one;
  * integer results: every pixel within 1 + ceil(5 E_ref (v + 1)) counts of the float32 restatement, at most 1 % of the pixels differ;
  * float results: |device - restatement| <= 5 E_ref (|v| + 1).
Every measured figure is printed before it is asserted.  Every test here but the one of the four index maps raises
NotImplementedError on a build without the feature.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import destripe_oracle as O
from tests import autoclips_util as A
from tests import pystripe_pad_util as PU
from tests import pystripe_util as U
from tests import thresholds_util as T
from tests.conftest import ROOT
from tests.test_gpu_pystripe import check_against, report, run_abi

pytestmark = pytest.mark.gpu

INDEX_GOLDEN = os.path.join(ROOT, "tests", "golden", "pystripe_padmodes", "index_modes.npz")
AUTO = dict(bleach_correction_frequency=1 / 32)     # all three clips None: estimated per tile


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


@functools.lru_cache(maxsize=None)
def tile(shape, dtype, seed=7, stripes="rows"):
    img = U.synthetic_tile(shape, seed, np.dtype(dtype), stripes)
    img.setflags(write=False)
    return img


def check_case(ps, dev, name, img, rec_lo=None, wavelet="db9", **kw):
    """log domain and final result of one tile against the restatement; returns (device log image, float64 log image, E_ref)"""
    r32, l64, e_ref = PU.reference(img, rec_lo=rec_lo, **kw)
    log = ps.filter_streaks(img.copy(), wavelet=wavelet, device=dev, log_output=True, extended=True, **kw)
    assert log.dtype == np.float32 and log.shape == l64.shape
    err = float(np.abs(log.astype(np.float64) - l64).max())
    report(f"{name}: log domain, device vs float64 restatement {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f} (allowed 4)")
    assert err <= 4 * e_ref
    check_against(name, ps.process_img(img.copy(), wavelet=wavelet, device=dev, extended=True, **kw), r32, e_ref)
    return log, l64, e_ref


@pytest.mark.parametrize("bidirectional", [False, True])
@pytest.mark.parametrize("mode", PU.VALUE_MODES)
def test_every_mode_in_one_and_two_directions(ps, dev, mode, bidirectional):
    check_case(ps, dev, f"{mode} (97, 128) uint16 bidirectional={bidirectional}", tile((97, 128), "uint16"), sigma=(8, 8), padding_mode=mode,
               bidirectional=bidirectional)


@pytest.mark.parametrize("mode", PU.VALUE_MODES)
def test_odd_extents_pad_one_more_at_the_end(ps, dev, mode):
    """(129, 131): pad_y = pad_x = 1, so the two ramps of an axis differ in length and the end corners are wider than the front ones"""
    img = tile((129, 131), "uint8")
    info = ps.derive(img.shape, img.dtype, ps.make_params(img.dtype, sigma=(8, 8), padding_mode=mode, extended=True))
    assert (info.pad_y, info.pad_x) == (1, 1) and info.base_pad > 0
    check_case(ps, dev, f"{mode} (129, 131) uint8", img, sigma=(8, 8), padding_mode=mode, bidirectional=True)


@pytest.mark.parametrize("mode", ["mean", "median", "linear_ramp"])
def test_the_34_sample_rule(ps, dev, mode):
    img = tile((9, 21), "float32")
    info = ps.derive(img.shape, img.dtype, ps.make_params(img.dtype, sigma=(2, 2), padding_mode=mode, extended=True))
    assert (info.padded_ny, info.padded_nx) == (34, 34) and info.pad_y > 1 and info.pad_x > 1
    check_case(ps, dev, f"{mode} (9, 21) float32", img, sigma=(2, 2), padding_mode=mode, bidirectional=True)


@pytest.mark.parametrize("mode", ["mean", "constant"])
def test_two_passes_pad_once(ps, dev, mode):
    """sigma (6, 20): the second pass reads the image the first one left.  Padding it again would put the statistics of the FIRST
    pass's input around the second pass's, which the restatement does not do."""
    extra = dict(bleach_correction_clip_min=5.3) if mode == "constant" else {}
    check_case(ps, dev, f"{mode} two passes", tile((97, 128), "uint16"), sigma=(6, 20), padding_mode=mode, bidirectional=True, **extra)


@pytest.mark.parametrize("mode", ["median", "maximum"])
@pytest.mark.parametrize("wavelet,order", [("haar", 1), ("db4", 4)])
def test_the_generic_wavelet_route(ps, dev, wavelet, order, mode):
    check_case(ps, dev, f"{mode} {wavelet}", tile((97, 130), "uint8"), rec_lo=O.db_filters(order)[2], wavelet=wavelet, sigma=(6, 6),
               padding_mode=mode, bidirectional=True)


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("n", [PU.LDS_LINE, PU.LDS_LINE + 1])
def test_median_on_either_side_of_the_lds_limit(ps, dev, n, transpose):
    """Lines of PU.LDS_LINE samples (even; the keys stay in LDS) and of one more (odd; radix passes over global memory), as rows and,
    transposed, as columns; the other axis has 4 samples, and the corner is the median of the long vector of medians.  uint8: many
    samples tie."""
    from ipp_amd import capi
    assert capi.PS_PAD_LDS_LINE == PU.LDS_LINE
    img = tile((4, n), "uint8")
    assert np.unique(img).size * 50 < img.size
    if transpose:
        img = np.ascontiguousarray(img.T)
    check_case(ps, dev, f"median {img.shape} uint8", img, sigma=(2, 2), padding_mode="median", bidirectional=True)


def run_plan(ps, dev, stack, **kw):
    import torch
    plan = ps.Plan(dev, stack.shape[1:], stack.dtype, ps.make_params(stack.dtype, max_batch=stack.shape[0], extended=True, **kw))
    try:
        out = plan.run(torch.from_numpy(np.ascontiguousarray(stack)).to(dev))
        torch.cuda.synchronize(dev)
        clips = plan.clips() if plan.params.bleach_frequency else None
        return out.cpu().numpy(), clips
    finally:
        plan.close()


@pytest.mark.parametrize("mode", ["median", "constant"])
def test_tiles_of_a_batch_do_not_see_each_other(ps, dev, mode):
    """Three different tiles through one launch equal, bit for bit, what each gets alone: statistics and constants are per tile.
    The constant is each tile's own log1p(lb) (automatic clips)."""
    shape = (45, 70)
    tiles = np.stack([T.four_mode_image(shape, 30), (T.four_mode_image(shape, 31) // 3).astype(np.uint16),
                      np.clip(T.four_mode_image(shape, 32) * 2.5, 0, 65535).astype(np.uint16)])
    kw = dict(sigma=(8, 8), padding_mode=mode, bidirectional=True, **(AUTO if mode == "constant" else {}))
    for log in (False, True):
        together, clips = run_plan(ps, dev, tiles, log_output=log, **kw)
        for i in range(3):
            alone, _ = run_plan(ps, dev, tiles[i:i + 1], log_output=log, **kw)
            assert np.array_equal(together[i].view(np.uint8), alone[0].view(np.uint8)), (mode, log, i)
        assert not np.array_equal(together[0], together[1])
    if mode == "constant":
        lbs = [float(A.triple(t, **kw)[0]) for t in tiles]
        assert len(set(lbs)) == 3 and clips[1].tolist() == [0, 0, 0]
    for i in range(3):
        _, l64, e_ref = PU.reference(tiles[i], **kw)
        err = float(np.abs(together[i].astype(np.float64) - l64).max())
        report(f"batch {mode} tile {i}: log domain {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f}")
        assert err <= 4 * e_ref


def test_constant_without_a_clip_pads_with_zero(ps, dev):
    img = tile((97, 128), "uint16")
    kw = dict(sigma=(8, 8), padding_mode="constant", bidirectional=True)
    log, l64, e_ref = check_case(ps, dev, "constant 0", img, **kw)
    # ... and not with anything else: the restatement padded with log1p(5.3) is far from both
    _, other, _ = PU.reference(img, constant=PU.pad_constant(5.3), **kw)
    assert np.abs(other - l64).max() > 100 * e_ref and np.abs(log - other).max() > 100 * e_ref


def test_constant_takes_clip_min_without_a_frequency(ps, dev):
    img = tile((97, 128), "uint16")
    kw = dict(sigma=(8, 8), padding_mode="constant", bidirectional=True, bleach_correction_clip_min=5.3)
    log, l64, e_ref = check_case(ps, dev, "constant log1p(5.3), no frequency", img, **kw)
    _, zero, _ = PU.reference(img, constant=0.0, **kw)
    assert np.abs(zero - l64).max() > 100 * e_ref and np.abs(log - zero).max() > 100 * e_ref
    # the other two clips alone change nothing
    same = ps.filter_streaks(img.copy(), wavelet="db9", device=dev, log_output=True, extended=True, bleach_correction_clip_med=6.0,
                             bleach_correction_clip_max=7.0, **kw)
    assert np.array_equal(same, log)


def test_constant_with_a_frequency_and_all_three_clips(ps, dev):
    img = tile((97, 128), "uint16")
    clips = {k: v for k, v in zip(A.CLIP_KEYS, (5.3, 6.4, 8.1))}
    check_case(ps, dev, "constant log1p(5.3), bleach correction", img, sigma=(8, 8), padding_mode="constant", bidirectional=True,
               bleach_correction_frequency=1 / 32, **clips)


def test_constant_with_an_estimated_minimum_is_the_unraised_one(ps, dev):
    """A frequency and clip_min None: the pad is log1p(lb) of this tile's own multi-Otsu threshold lb, as the reference pads BEFORE
    correct_bleaching raises its minimum to log1p(1).  The tile's lb lies far below log1p(1); Plan.clips() reports the raised one."""
    img = PU.low_floor_tile((97, 128), 3)
    kw = dict(sigma=(8, 8), padding_mode="constant", bidirectional=True, **AUTO)
    lb = float(A.triple(img, **kw)[0])
    assert 0 < lb < 0.1 * PU.LOG2
    log, l64, e_ref = check_case(ps, dev, f"constant log1p(lb), lb = {lb:.4g}", img, **kw)
    out, (clips, status) = run_plan(ps, dev, img[None], log_output=True, **kw)
    assert status[0] == 0 and clips[0, 0] == np.float32(PU.LOG2) and np.array_equal(out[0], log)
    assert np.array_equal(clips[0], A.used_triple(A.triple(img, **kw)))
    _, raised, _ = PU.reference(img, constant=PU.pad_constant(float(clips[0, 0])), **kw)
    gap = float(np.abs(raised - l64).max())
    report(f"padded with the raised minimum instead, the restatement moves by {gap:.3g} = {gap / e_ref:.0f} E_ref")
    assert gap > 100 * e_ref and np.abs(log - raised).max() > 100 * e_ref


def test_index_maps_give_the_bits_they_gave_before(ps, dev):
    """reflect / wrap / symmetric / edge on one shape, one and two passes: the results recorded on the commit before the value modes
    existed (tests/golden/pystripe_padmodes/index_modes.npz)."""
    z = np.load(INDEX_GOLDEN)
    img = z["img"]
    assert np.array_equal(img, tile((97, 128), "uint16", 77))
    for mode in PU.INDEX_MODES:
        for name, sigma in (("one", (8, 8)), ("two", (8, 24))):
            kw = dict(sigma=sigma, wavelet="db9", padding_mode=mode, bidirectional=True, device=dev)
            assert np.array_equal(ps.process_img(img.copy(), **kw), z[f"{mode}_{name}_out"]), (mode, name)
            log = ps.filter_streaks(img.copy(), log_output=True, **kw)
            assert np.array_equal(log.view(np.uint32), z[f"{mode}_{name}_log"].view(np.uint32)), (mode, name)


def test_through_the_c_abi_alone(ps, dev):
    from ipp_amd import capi
    img = tile((129, 131), "uint8")
    kw = dict(sigma=(8, 8), padding_mode="median", bidirectional=True)
    r32, l64, e_ref = PU.reference(img, **kw)
    stack = np.stack([img, img[::-1].copy()])
    got, info = run_abi(dev, stack, ps.make_params(img.dtype, log_output=True, max_batch=2, extended=True, **kw))
    err = float(np.abs(got[0].astype(np.float64) - l64).max())
    report(f"C ABI, median: log domain {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f}")
    assert got.dtype == np.float32 and err <= 4 * e_ref and (info.pad_y, info.pad_x) == (1, 1)
    out, _ = run_abi(dev, stack, ps.make_params(img.dtype, max_batch=2, extended=True, **kw))
    check_against("C ABI, median", out[0], r32, e_ref)
    # a code outside mi_pystripe_padding
    prm = ps.make_params(img.dtype, extended=True, **kw)
    prm.padding_mode = 10
    h = C.c_void_p()
    rc = capi.lib().mi_pystripe_plan_create(dev.index or 0, 129, 131, capi.PS_U8, C.byref(prm), C.byref(h))
    assert rc == capi.MI_ERR_INVALID and not h.value
    with pytest.raises(capi.MiError, match="padding_mode"):
        capi.check(rc)
