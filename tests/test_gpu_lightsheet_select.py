"""GPU: ``row_percentile_kernel`` and ``box_percentile_kernel`` (csrc/lightsheet.hip) on ties, signs, edges and routes, through
``ipp_amd.pystripe.local_percentile`` and ``LightsheetPlan``.  The reference is ``numpy.percentile`` per window
(tests/lightsheet_util.percentile_grid / row_grid) and every comparison is equality.  The windows come from
tests/lightsheet_select_util.py; tests/test_lightsheet_select_host.py proves on a host model which branches of the kernels they reach.
"""
import numpy as np
import pytest

from tests import lightsheet_select_util as S
from tests import lightsheet_util as L

pytestmark = pytest.mark.gpu
NAMES = [np.dtype(d).name for d in S.DTYPES]


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


def on_device(ps, dev, array, p, **kw):
    """local_percentile(interpolate=None) of a device tensor, back as numpy"""
    return ps.local_percentile(array, p, interpolate=None, **kw).cpu().numpy()


def first_difference(got, want, names=None):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if not len(bad):
        return None
    i = tuple(bad[0])
    return (i, names[i[0]] if names else None, got[i], want[i], len(bad))


# ---------------------------------------------------------------------------------------------------------------------------------
# box kernel: one window per tile

@pytest.mark.parametrize("dtype", NAMES)
@pytest.mark.parametrize("n", S.BOX_SIZES)
def test_box_whole_tile_windows(ps, dev, n, dtype):
    import torch
    names, stack = S.family_stack(n, dtype)
    tiles, kw = S.whole_tile_stack(stack)
    t = torch.from_numpy(tiles).to(dev)
    for p in S.percentiles_for(n, dtype == "float32"):
        got = on_device(ps, dev, t, p, **kw)
        assert got.shape == (len(stack), 1, 1) and got.dtype == stack.dtype
        want = np.zeros(len(stack), stack.dtype)
        want[...] = np.percentile(stack, 100 * p, axis=1)         # the store truncates into an integer grid
        assert np.array_equal(got[:, 0, 0], want), (n, dtype, p, first_difference(got[:, 0, 0], want, names))


def test_box_window_past_the_limit_is_refused(ps, dev):
    from ipp_amd import capi
    n = S.MAX_WINDOW + 1
    with pytest.raises(capi.MiError) as e:
        ps.local_percentile(np.zeros((1, n), np.uint8), 0.5, selem=(2, 2 * n), spacing=(1, n), interpolate=None, device=dev)
    assert e.value.code == capi.MI_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------------
# row kernel

@pytest.mark.parametrize("dtype", NAMES)
@pytest.mark.parametrize("length", S.ROW_LENGTHS)
def test_row_runs(ps, dev, length, dtype):
    import torch
    names, stack = S.family_stack(length, dtype)
    tiles, index = S.row_stack(stack, length)
    assert tiles.shape[1] * (tiles.shape[2] // length) == index.shape[1] * index.shape[2]
    t = torch.from_numpy(tiles).to(dev)
    for p in S.percentiles_for(length, dtype == "float32"):
        got = on_device(ps, dev, t, p, selem=(1, length))
        want = np.stack([L.row_grid(tile, p, length) for tile in tiles])
        assert got.shape == want.shape and got.dtype == want.dtype
        bad = np.argwhere(got != want)
        assert not len(bad), (length, dtype, p, names[index[tuple(bad[0])]], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


# ---------------------------------------------------------------------------------------------------------------------------------
# routes: the same (1, L) windows through the row kernel and, with a spacing of their own or a step, through the box kernel

def route_image(dtype, shape, seed):
    """two images of one shape: shuffled samples of the whole range, and two values only"""
    rng = np.random.default_rng(seed)
    shuffled = S.generic_samples(rng, shape[0] * shape[1], dtype).reshape(shape)
    lo_v, hi_v = (np.float32(-0.75), np.float32(2.5000002)) if dtype == "float32" else (7, 200)
    two = np.where(rng.random(shape) < 0.4, lo_v, hi_v).astype(dtype)
    return shuffled, two


ROUTE_P = (0.0, 1.0, 0.25, 2 / 3, 0.999)


@pytest.mark.parametrize("dtype", NAMES)
@pytest.mark.parametrize("length", (64, 257, 1000))
def test_routes_of_a_row_window(ps, dev, length, dtype):
    import torch
    family_tiles = S.row_stack(S.family_stack(length, dtype)[1], length)[0]         # the runs of test_row_runs, three tiles of them
    for img in route_image(dtype, (4, S.ROW_PAD + 3 * length), length) + tuple(family_tiles[:3]):
        t = torch.from_numpy(img).to(dev)
        for p in ROUTE_P:
            for kw in (dict(spacing=(1, length)), dict(spacing=(1, length + 3)), dict(step=(1, 2))):
                got = on_device(ps, dev, t, p, selem=(1, length), **kw)
                want = L.percentile_grid(img, p, (1, length), kw.get("spacing"), kw.get("step"))
                assert got.shape == want.shape and np.array_equal(got, want), (length, dtype, p, kw, first_difference(got, want))


@pytest.mark.parametrize("dtype", NAMES)
def test_row_window_past_the_row_kernel(ps, dev, dtype):
    """(1, 5000) on a 10007-wide image: longer than the row kernel takes, so the box kernel ranks it"""
    import torch
    for img in route_image(dtype, (3, 10007), 5000):
        t = torch.from_numpy(img).to(dev)
        for p in ROUTE_P:
            got = on_device(ps, dev, t, p, selem=(1, 5000))
            want = L.percentile_grid(img, p, (1, 5000))
            assert got.shape == (3, 2) and np.array_equal(got, want), (dtype, p, first_difference(got, want))


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry: rectangular windows, clipped at all four borders, stepped, larger than the image

GEOMETRY = [(selem, spacing, step) for selem in ((40, 50), (7, 6), (200, 300)) for spacing in ((7, 9), (70, 90)) for step in ((1, 1), (2, 3), (3, 2))]


@pytest.mark.parametrize("dtype", NAMES)
def test_rectangular_clipped_and_stepped_windows(ps, dev, dtype):
    import torch
    for img in route_image(dtype, (70, 90), 7090):
        t = torch.from_numpy(img).to(dev)
        for selem, spacing, step in GEOMETRY:
            for p in (0.25, 2 / 3, 1.0):
                got = on_device(ps, dev, t, p, selem=selem, spacing=spacing, step=step)
                want = L.percentile_grid(img, p, selem, spacing, step)
                assert got.shape == want.shape and np.array_equal(got, want), (dtype, selem, spacing, step, p, first_difference(got, want))


# ---------------------------------------------------------------------------------------------------------------------------------
# the grid's own type

def test_output_types(ps, dev):
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (70, 90)).astype(np.uint8)
    f32 = (rng.random((70, 90)) * 60000).astype(np.float32)
    f32_small = (rng.random((70, 90)) * 255).astype(np.float32)
    for img, out in ((u8, np.float32), (f32, np.uint16), (f32_small, np.uint8), (f32_small, np.uint16)):
        for selem, spacing, step in (((7, 6), (7, 9), (1, 1)), ((40, 50), (7, 9), (2, 3)), ((1, 30), (1, 30), (1, 1))):
            for p in (0.25, 2 / 3, 1.0):
                got = ps.local_percentile(img, p, selem=selem, spacing=spacing, step=step, interpolate=None, dtype=out, device=dev)
                want = L.percentile_grid(img, p, selem, spacing, step, dtype=out)
                assert got.dtype == want.dtype and np.array_equal(got, want), (img.dtype, out, selem, p, first_difference(got, want))


# ---------------------------------------------------------------------------------------------------------------------------------
# chunking

CHUNK = dict(artifact_length=64, background_window_size=100)


@pytest.fixture(scope="module")
def chunk_tiles():
    tiles = np.stack([L.bead_and_stripe_tile((64, 320), 300 + i, np.uint16) for i in range(11)])
    return tiles, [L.correct_lightsheet(t, **CHUNK)[:3] for t in tiles]


@pytest.mark.parametrize("maps", (False, True))
@pytest.mark.parametrize("in_place", (False, True))
def test_plan_runs_more_tiles_than_one_launch_holds(ps, dev, chunk_tiles, maps, in_place):
    """max_batch = 4: 3 tiles (one short chunk), 11 (chunks 4, 4, 3; the scratch grows behind a stream sync), then 2 again"""
    import torch
    tiles, want = chunk_tiles
    plan = ps.LightsheetPlan(dev, (64, 320), np.uint16, ps.make_lightsheet_params(np.uint16, max_batch=4, **CHUNK))
    try:
        assert plan.info.max_batch == 4
        for first, count in ((0, 3), (0, 11), (5, 2)):
            t = torch.from_numpy(tiles[first:first + count]).to(dev)
            out, ls, bg = plan.run(t, None if in_place else torch.empty_like(t), return_lightsheet=maps, return_background=maps)
            torch.cuda.synchronize(dev)
            assert (out.data_ptr() == t.data_ptr()) == in_place and (ls is None) == (not maps) and (bg is None) == (not maps)
            if not in_place:
                assert np.array_equal(t.cpu().numpy(), tiles[first:first + count])
            for i in range(count):
                w = want[first + i]
                assert np.array_equal(out[i].cpu().numpy(), w[0]), (count, i)
                if maps:
                    assert np.array_equal(ls[i].cpu().numpy(), w[1]) and np.array_equal(bg[i].cpu().numpy(), w[2]), (count, i)
    finally:
        plan.close()


def test_interpolated_percentile_past_one_chunk(ps, dev):
    """70 tiles through local_percentile(interpolate=1): chunks of 64 and 6"""
    rng = np.random.default_rng(9)
    tiles = rng.integers(0, 256, (70, 30, 40)).astype(np.uint8)
    tiles[3] = 255
    tiles[66] = 0
    got = ps.local_percentile(tiles, 1 / 3, selem=(9, 12), spacing=(5, 7), step=(1, 2), interpolate=1, device=dev)
    assert got.shape == tiles.shape and got.dtype == np.uint8
    for i, tile in enumerate(tiles):
        assert np.array_equal(got[i], L.zoom1(L.percentile_grid(tile, 1 / 3, (9, 12), (5, 7), (1, 2)), tile.shape)), i


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 samples must be finite (include/mi_lightsheet.h); a NaN stays inside the windows that hold it

def test_a_nan_touches_only_the_windows_that_hold_it(ps, dev):
    img = route_image("float32", (70, 90), 11)[0].copy()
    img[0, 0] = np.nan
    for kw in (dict(selem=(9, 12), spacing=(7, 9)), dict(selem=(40, 50), spacing=(7, 9), step=(2, 3)), dict(selem=(1, 30))):
        got = ps.local_percentile(img, 0.25, interpolate=None, device=dev, **kw)
        want = L.percentile_grid(img, 0.25, kw["selem"], kw.get("spacing"), kw.get("step"))
        clean = ~np.isnan(want)                        # numpy: NaN in every window that holds the sample
        assert 0 < (~clean).sum() < clean.size and not clean[0, 0]
        assert np.array_equal(got[clean], want[clean]), kw
