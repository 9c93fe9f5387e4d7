"""CPU: the restatement of the foreground mask (tests/mask_util.py) against scipy's own filters, the properties include/mi_tile_mask.h
states (one window for both operators, the one-sample shift of an even box, the border rule, the kept border region), and what the
Python layer decides without a device (the keyword gate, the connectivity, the code bound of the threshold)."""
import numpy as np
import pytest

from tests import mask_util as M


@pytest.fixture(scope="module")
def ps():
    from ipp_amd import pystripe
    return pystripe


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 50])
def test_window_loops_equal_the_scipy_filters(k):
    for seed, shape in enumerate([(40, 61), (1, 70), (70, 1), (33, 33)]):
        m = M.blobs(shape, seed, density=0.3 + 0.1 * seed, smooth=seed % 3)
        for other in (1, 3, k):
            assert np.array_equal(M.close_open(m, k, other), M.close_open_scipy(m, k, other)), (shape, k, other)
            assert np.array_equal(M.close_open(m, other, k), M.close_open_scipy(m, other, k)), (shape, other, k)
        for axis in (0, 1):
            assert np.array_equal(M.dilate1d(m, k, axis), M._scipy1d(m, k, axis, True))
            assert np.array_equal(M.erode1d(m, k, axis), M._scipy1d(m, k, axis, False))


def test_k1_is_the_identity_and_a_huge_k_covers_the_line():
    m = M.blobs((23, 31), 5)
    assert np.array_equal(M.close_open(m, 1, 1), m)
    assert M.dilate(m, 500).all() and not M.erode(m, 500).any()
    assert np.array_equal(M.erode(np.ones_like(m), 500), np.ones_like(m))


@pytest.mark.parametrize("k", [2, 4])
def test_an_even_box_moves_a_single_pixel_by_one(k):
    m = np.zeros((21, 23), bool)
    m[9, 11] = True
    closed = M.erode(M.dilate(m, k), k)
    assert closed.sum() == 1 and closed[10, 12]
    for odd in (3, 5):
        assert np.array_equal(M.erode(M.dilate(m, odd), odd), m)


def test_border_rule_outside_is_0_for_dilation_and_1_for_erosion():
    ones = np.ones((9, 12), bool)
    assert M.erode(ones, 5).all()            # an erosion does not eat into a full tile from its border
    m = np.zeros((9, 12), bool)
    m[:, :3] = True                          # a band on the border survives an opening of its own width
    assert np.array_equal(M.dilate(M.erode(m, 3), 3), m)
    assert not M.dilate(np.zeros((9, 12), bool), 5).any()


def test_border_region_without_a_corner_is_kept_and_corner_regions_go():
    m = np.ones((20, 24), bool)
    m[:4, :5] = False            # holds the corner (0, 0): removed
    m[8:12, 10:14] = False       # enclosed hole: filled
    m[-3:, 9:15] = False         # touches the bottom edge, no corner: kept, so it becomes foreground
    got = M.fill(m, 4)
    want = np.ones_like(m)
    want[:4, :5] = False
    assert np.array_equal(got, want)
    assert M.fill(np.ones((5, 5), bool)).all() and not M.fill(np.zeros((5, 5), bool)).any()


def test_diagonal_gap_leaks_with_connectivity_8_only():
    m = np.ones((12, 12), bool)
    m[:3, :3] = False            # corner region
    m[3:6, 3:6] = False          # touches it at one diagonal step
    assert M.fill(m, 4)[4, 4] and not M.fill(m, 8)[4, 4]


def test_the_gate_still_refuses_masking_without_extended(ps):
    tile = np.zeros((40, 40), np.uint16)
    with pytest.raises(NotImplementedError, match="enable_masking"):
        ps.filter_streaks(tile, sigma=(8, 8), enable_masking=True)
    with pytest.raises(NotImplementedError, match="OpenCV / scikit-image semantics"):
        ps.filter_streaks(tile, sigma=(8, 8), enable_masking=True, close_steps=3, open_steps=3)


@pytest.mark.parametrize("flag", [0, 5, 16, 4 | 256 | 1, 255, True, 4.0])
def test_a_flood_fill_flag_that_is_neither_4_nor_8_names_itself(ps, flag):
    with pytest.raises(ValueError, match="flood_fill_flag"):
        ps.get_img_mask(np.zeros((8, 8), np.uint8), 0, flood_fill_flag=flag)


def test_the_low_byte_of_the_flag_is_the_connectivity(ps):
    assert ps.check_flood_fill_flag(4) == 4 and ps.check_flood_fill_flag(8 | (255 << 8)) == 8 and ps.check_flood_fill_flag(np.int32(4)) == 4


@pytest.mark.parametrize("name, value", [("close_steps", 0), ("open_steps", -2), ("close_steps", 2.5)])
def test_a_box_below_1_names_itself(ps, name, value):
    with pytest.raises(ValueError, match=name):
        ps.get_img_mask(np.zeros((8, 8), np.uint8), 0, **{name: value})


def test_code_bound_equals_the_brute_force_compare_over_all_codes(ps):
    from ipp_amd.thresholds import log_table
    for ncodes in (256, 65536):
        table = log_table(ncodes)
        clips = [-1.0, 0.0, 1e-9, float(table[1]), 0.6931, 0.6932, 2.5, 5.545, float(table[ncodes - 1]), 12.0]
        clips += [float(np.nextafter(table[c], np.float32(d))) for c in (1, 7, 200, ncodes - 2) for d in (-np.inf, np.inf)]
        clips += [float(table[c]) for c in (7, 200, ncodes - 2)]
        for clip in clips:
            bound = ps.mask_code_bound(clip, ncodes)
            assert -1 <= bound <= ncodes - 1
            assert np.array_equal(np.arange(ncodes) > bound, table > np.float32(clip)), (ncodes, clip, bound)


def _mirrored(m, close_steps, open_steps):
    """the morphology with the window of an even box shifted the other way"""
    return M.close_open(m[::-1, ::-1], close_steps, open_steps)[::-1, ::-1]


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_gpu_morphology_cases_carry_content(shape):
    """The expectations of tests/test_gpu_tile_mask.py on the patterns of ``structures``: neither empty nor full for every box below an
    extent, and different from what three wrong morphologies give -- none at all, the even window shifted the other way, a box capped
    at 9.  On a 2-D tile the fill adds next to nothing, so the mask is the morphology's result; on a line it closes every gap."""
    for boxes in M.BOXES:
        m = M.structures(shape, max(boxes))
        morph = M.close_open(m, *boxes)
        want = M.fill(morph)
        if max(boxes) >= max(shape):
            assert want.all()       # the box covers the tile from every sample: see extreme_stack
            continue
        assert want.any() and not want.all(), (shape, boxes)
        if min(shape) > 1:
            assert int((want != morph).sum()) <= 2, (shape, boxes)
        if boxes != (1, 1):
            assert not np.array_equal(M.fill(m), want), (shape, boxes)
        if boxes[0] % 2 == 0 or boxes[1] % 2 == 0:
            assert not np.array_equal(M.fill(_mirrored(m, *boxes)), want), (shape, boxes)
        if max(boxes) > 9:
            assert not np.array_equal(M.fill(M.close_open(m, min(boxes[0], 9), min(boxes[1], 9))), want), (shape, boxes)


def test_boxes_beyond_both_extents_tell_any_from_all():
    """a box beyond both extents makes a dilation "any sample" and an erosion "every sample" of the tile"""
    for shape in M.SHAPES:
        t = M.extreme_stack(shape)
        for boxes, full in (((500, 500), [0, 1, 1, 1]), ((500, 1), [0, 1, 1, 1]), ((1, 500), [0, 0, 0, 1])):
            for tile, one in zip(t, full):
                want = M.fill(M.close_open(tile, *boxes))
                assert want.all() if one else not want.any(), (shape, boxes)


def test_constant_padding_with_an_estimated_minimum_is_refused_under_masking(ps):
    """Plan.clips() reports the minimum raised to log1p(1); the constant is the one before.  Refused from the values, before a device."""
    tile = np.zeros((40, 40), np.uint16)
    kw = dict(sigma=(8, 8), padding_mode="constant", enable_masking=True, close_steps=3, open_steps=3, extended=True)
    with pytest.raises(NotImplementedError, match=r"enable_masking=True: padding_mode='constant' with an estimated bleach_correction_clip_min"):
        ps.filter_streaks(tile, bleach_correction_frequency=1 / 32, **kw)
    with pytest.raises(NotImplementedError, match="give bleach_correction_clip_min"):
        ps.filter_streaks(tile, bleach_correction_frequency=1 / 32, bleach_correction_clip_med=5.0, bleach_correction_clip_max=7.0, **kw)
