"""Host: the facts that tests/test_gpu_edgetaper.py relies on -- which tiles of the direct engine lie wholly on the taper's plateau,
where the plateaus of short axes are, and that the oracle's replicate convolution is the reference's loop for even PSF extents --
so that a later change of the cases cannot silently stop covering a branch of csrc/edgetaper.hip."""
import numpy as np
import pytest

from oracle import rl_oracle as R
from tests import edgetaper_util as U


def test_tile_grid_is_the_direct_engines():
    assert U.TILE == (2, 16, 128)
    tiles = U.tile_grid((5, 40, 264))
    assert len(tiles) == 3 * 3 * 3
    assert tiles[0] == ((0, 2), (0, 16), (0, 128)) and tiles[-1] == ((4, 5), (32, 40), (256, 264))
    # the tiles partition the block
    cover = np.zeros((5, 40, 264), np.int32)
    for (z0, z1), (y0, y1), (x0, x1) in tiles:
        cover[z0:z1, y0:y1, x0:x1] += 1
    assert (cover == 1).all()


@pytest.mark.parametrize("kshape", [(7, 9, 9), (4, 6, 8), (2, 2, 2), (6, 3, 4), (1, 1, 1), (16, 16, 16), (15, 16, 3)])
def test_264_columns_have_exactly_one_skipped_tile(kshape):
    """Any PSF of extents <= 16 has the taper width 8: plateaus [8, 11), [8, 33), [8, 257)."""
    assert U.plateaus((18, 40, 264), kshape) == [(8, 11), (8, 33), (8, 257)]
    assert U.skipped_tiles((18, 40, 264), kshape) == [((8, 10), (16, 32), (128, 256))]
    assert U.tile_centre(U.skipped_tiles((18, 40, 264), kshape)[0]) == (9, 24, 192)


def test_262_columns_have_none():
    """A tile [128, 256) inside the x plateau [8, nx - 7) needs nx >= 263: one column less and nothing is skipped."""
    assert U.plateaus((18, 40, 263), (7, 9, 9))[2] == (8, 256) and len(U.skipped_tiles((18, 40, 263), (7, 9, 9))) == 1
    assert U.plateaus((18, 40, 262), (7, 9, 9))[2] == (8, 255)
    assert U.skipped_tiles((18, 40, 262), (7, 9, 9)) == []
    assert U.skipped_tiles((40, 50, 140), (21, 9, 9)) == []   # the widest block of the older route test


def test_600_columns_skip_three_tiles_and_three_strides():
    shape, kshape, _ = U.CASES["three_strides_600"]
    assert U.plateaus(shape, kshape)[2] == (8, 593)
    skipped = U.skipped_tiles(shape, kshape)
    assert len(skipped) >= 3 and [t[2] for t in skipped] == [(128, 256), (256, 384), (384, 512)]
    assert {t[:2] for t in skipped} == {((8, 10), (16, 32))}
    # k_taper_blend: a lane at x inside the plateau [x_lo, x_hi) goes on at x + ceil((x_hi - x) / 256) * 256; on this row the
    # lanes jump two or three strides, some land inside the block (the upper ramp), others leave it
    x_lo, x_hi = U.plateaus(shape, kshape)[2]
    landings = {}
    for lane in range(256):
        x = lane if lane >= x_lo else lane + 256
        landings[lane] = x + -(-(x_hi - x) // 256) * 256
    assert all(v >= x_hi and v - 256 < x_hi for v in landings.values())
    assert any(v < shape[2] for v in landings.values()) and any(v >= shape[2] for v in landings.values())
    jumps = {lane: v - (lane if lane >= x_lo else lane + 256) for lane, v in landings.items()}
    assert set(jumps.values()) == {512, 768}
    assert {jumps[lane] for lane, v in landings.items() if v < shape[2]} == {512}   # x = 81 .. 87 go on at 593 .. 599


@pytest.mark.parametrize("n,want", [(1, (0, 1)), (2, (1, 2)), (3, (1, 3)), (15, (7, 9)), (16, (8, 9)), (17, (8, 10)), (40, (8, 33))])
def test_plateaus_of_short_axes_at_width_8(n, want):
    assert U.plateau(R.make_taper(n, 8)) == want


def test_wide_ramp_is_12_samples():
    shape, kshape, _ = U.CASES["wide_ramp"]
    assert R.taper_widths(kshape) == [12, 8, 8]
    assert U.plateaus(shape, kshape) == [(12, 29), (8, 13), (8, 17)]
    tz = R.edgetaper_mask_vectors(shape, kshape)[0]
    assert tz[0] == 0 and tz[11] == np.float32(11 / 12) and tz[39] == np.float32(1 / 12)


def test_mask_is_one_exactly_on_the_three_plateaus():
    for name in ("tile_skip_264", "degenerate_2_17_16", "degenerate_1_20_33", "psf_larger_than_block"):
        shape, kshape, _ = U.CASES[name]
        m = U.mask(shape, kshape)
        inside = np.zeros(shape, bool)
        (z0, z1), (y0, y1), (x0, x1) = U.plateaus(shape, kshape)
        inside[z0:z1, y0:y1, x0:x1] = True
        assert m.dtype == np.float32 and np.array_equal(m == 1.0, inside) and inside.any() and not inside.all()
        assert 0.0 <= m.min() and m.max() == 1.0


def test_cases_are_the_ones_the_branches_need():
    assert len(U.CASES) == 14 and len(U.ODD_CASES) == 8 and len(U.EVEN_CASES) == 6
    for name, (shape, kshape, _) in U.CASES.items():
        assert int(np.prod(shape)) < 500_000, name
    # direct-route witnesses: the odd cases and the even ones of the long block have skipped tiles
    assert len(U.skipped_tiles(*U.CASES["tile_skip_264"][:2])) == 1
    assert all(len(U.skipped_tiles(*U.CASES[n][:2])) == 1 for n in U.EVEN_CASES if U.CASES[n][0] == (18, 40, 264))
    assert sum(U.CASES[n][0] == (18, 40, 264) for n in U.EVEN_CASES) == 3
    # no other case has one: everything there is shell, or touched by it
    for name in set(U.CASES) - {"tile_skip_264", "three_strides_600"} - set(U.EVEN_CASES):
        assert U.skipped_tiles(*U.CASES[name][:2]) == [], name
    # degenerate tapers: a plateau of one sample on some axis, an axis of two samples, an axis without a taper
    assert U.plateaus(*U.CASES["degenerate_15_16_17"][:2]) == [(7, 9), (8, 9), (8, 10)]
    assert U.plateaus(*U.CASES["degenerate_17_15_16"][:2]) == [(8, 10), (7, 9), (8, 9)]
    assert U.plateaus(*U.CASES["degenerate_2_17_16"][:2]) == [(1, 2), (8, 10), (8, 9)]
    assert U.plateaus(*U.CASES["degenerate_1_20_33"][:2]) == [(0, 1), (8, 13), (8, 26)]
    assert U.plateaus(*U.CASES["psf_larger_than_block"][:2]) == [(3, 4), (3, 5), (2, 4)]


def test_case_inputs_are_in_range_and_shared():
    bl, psf, want, m = U.case("degenerate_15_16_17")
    assert bl.dtype == psf.dtype == want.dtype == m.dtype == np.float32
    assert 0.0 <= bl.min() and bl.max() < 1.0 and (psf >= 0).all() and abs(float(psf.sum()) - 1.0) > 0.5   # un-normalised
    assert U.case("degenerate_15_16_17")[0] is bl and not bl.flags.writeable
    assert np.array_equal(want[m == 1.0], bl[m == 1.0]) and not np.array_equal(want, bl)
    assert not np.allclose(psf, psf[::-1, ::-1, ::-1], rtol=1e-2)


@pytest.mark.parametrize("shape,kshape", [((6, 9, 11), (4, 6, 8)), ((7, 8, 9), (2, 2, 2)), ((5, 6, 7), (6, 3, 4))])
def test_oracle_convolution_is_the_reference_loop_for_even_extents(shape, kshape):
    rng = np.random.default_rng(11)
    a = rng.random(shape, dtype=np.float32)
    h = rng.random(kshape, dtype=np.float32)
    assert np.array_equal(R.conv3d_replicate(a, h), R.conv3d_replicate_loops(a, h))
    # and the even offset is visible: the window of convn's centre (k / 2 before, ndimage's default) gives another result
    from scipy import ndimage
    other = ndimage.convolve(a.astype(np.float64), h.astype(np.float64), mode="nearest").astype(np.float32)
    assert np.abs(other - R.conv3d_replicate(a, h)).max() > 100 * U.BOUND
