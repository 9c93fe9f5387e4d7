"""GPU: the foreground mask of filter_streaks (csrc/pystripe_mask.hip, include/mi_tile_mask.h; ``get_img_mask`` and
``filter_streaks(enable_masking=True, extended=True)``) against the numpy restatement of tests/mask_util.py.

Every comparison of a mask asks for ALL samples equal to the restatement; the results through ``filter_streaks`` are bit-equal to the
existing un-masked call on the tile zeroed with the restatement's mask.  Every test here fails on a build without the feature.
tests/test_tile_mask_host.py checks on the CPU that the morphology cases expect masks with content."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mask_util as M

pytestmark = pytest.mark.gpu

SHAPES, BOXES = M.SHAPES, M.BOXES
LEVELS = {"uint8": (10, 200, 100), "uint16": (100, 3000, 1000), "float32": (0.25, 0.75, 0.5)}   # background, foreground, threshold


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


def image_of(m, dtype, seed=0):
    """a tile of ``dtype`` whose samples above LEVELS' threshold are exactly ``m``; a float tile carries NaNs on background samples"""
    lo, hi, _ = LEVELS[dtype]
    rng = np.random.default_rng(seed)
    img = np.where(m, hi, lo).astype(dtype)
    if dtype == "float32":
        img += (rng.random(m.shape, dtype=np.float32) - 0.5) * np.float32(0.2)
        zeros = np.flatnonzero(~m.ravel())
        if zeros.size:
            img.ravel()[zeros[:: max(1, zeros.size // 7)]] = np.nan
    else:
        img += rng.integers(0, 9, m.shape).astype(dtype)
    return img


def run_plan(ps, dev, tiles, thr, close_steps, open_steps, connectivity=4, max_batch=0, log_domain=False, masked=None):
    """(masks bool [n, ny, nx], fill rounds, masked tiles or None) of a numpy stack through MaskPlan"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(tiles)).to(dev)
    plan = ps.MaskPlan(dev, tiles.shape[1:], tiles.dtype, close_steps, open_steps, connectivity, max_batch)
    try:
        got = plan.run(t, thr, log_domain, masked=t if masked == "alias" else masked)
        torch.cuda.synchronize(dev)
        rounds = plan.fill_rounds
    finally:
        plan.close()
    mask, out = got if isinstance(got, tuple) else (got, None)
    assert mask.dtype == torch.uint8 and int(mask.max()) <= 1
    return mask.cpu().numpy().astype(bool), rounds, None if out is None else out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def pattern(shape):
    m = M.framed(M.blobs(shape, seed=shape[0] + shape[1], density=0.45, smooth=1))
    m.setflags(write=False)
    return m


def check_types(ps, dev, m, boxes, want):
    """the tile of every type whose samples above the threshold are ``m``: all samples of the mask equal to ``want``"""
    for dtype in LEVELS:
        img = image_of(m, dtype)
        assert np.array_equal(M.threshold(img, LEVELS[dtype][2]), m)
        got, _, _ = run_plan(ps, dev, img[None], LEVELS[dtype][2], *boxes)
        assert np.array_equal(got[0], want), f"{dtype} {m.shape} {boxes}: {int((got[0] != want).sum())} samples differ"
        assert np.array_equal(ps.get_img_mask(img, LEVELS[dtype][2], *boxes, device=dev), want)


@pytest.mark.parametrize("boxes", BOXES, ids=lambda b: f"close{b[0]}-open{b[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_morphology_on_every_type(ps, dev, shape, boxes):
    """Solid structures on a background that is one region holding corners (``structures``): the fill removes exactly the background,
    so the mask is the morphology's result -- on a line tile, where the fill closes every gap, the span it leaves.  Every box below the
    tile's extents must leave a mask that is neither empty nor full; tests/test_tile_mask_host.py holds these expectations against
    wrong morphologies.  Structures lie across the wave edge (63 / 64) and the work-group edge (255 / 256), on the borders, and a gap
    of 25 apart, which only the boxes of 50 and more close."""
    m = M.structures(shape, max(boxes))
    morph = M.close_open(m, *boxes)
    want = M.fill(morph, 4)
    if max(boxes) < max(shape):
        assert want.any() and not want.all()
        assert min(shape) == 1 or int((want != morph).sum()) <= 2
    check_types(ps, dev, m, boxes, want)


@pytest.mark.parametrize("boxes", BOXES, ids=lambda b: f"close{b[0]}-open{b[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_morphology_inside_a_frame(ps, dev, shape, boxes):
    """Random blobs inside a frame of set border samples.  No background region then holds a corner, so the fill closes EVERY hole:
    where the frame survives the boxes the expected mask is all ones, and only the cases where the opening breaks the frame carry
    content.  Kept for the random fine structure of those cases."""
    m = pattern(shape)
    check_types(ps, dev, m, boxes, M.fill(M.close_open(m, *boxes), 4))


@pytest.mark.parametrize("boxes", [(500, 500), (500, 1), (1, 500)], ids=lambda b: f"close{b[0]}-open{b[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_boxes_beyond_both_extents(ps, dev, shape, boxes):
    """an empty tile, one sample, a full tile but one sample, a full tile, in one stack: with the window over the whole tile a
    dilation is "any sample" and an erosion "every sample", so the four masks differ from tile to tile"""
    t = M.extreme_stack(shape)
    want = np.stack([M.fill(M.close_open(x, *boxes)) for x in t])
    assert [bool(w.all()) for w in want] == ([False, False, False, True] if boxes == (1, 500) else [False, True, True, True])
    assert not want[0].any()
    for dtype in ("uint8", "float32"):
        tiles = np.stack([image_of(x, dtype, seed=k) for k, x in enumerate(t)])
        got, _, _ = run_plan(ps, dev, tiles, LEVELS[dtype][2], *boxes)
        assert np.array_equal(got, want), (dtype, [int((g != w).sum()) for g, w in zip(got, want)])


def test_morphology_without_a_frame(ps, dev):
    """no frame: the morphology's border rule and the fill act together"""
    m = M.blobs((129, 257), 3, density=0.4, smooth=2)
    for boxes in [(3, 4), (2, 1), (5, 8)]:
        got, _, _ = run_plan(ps, dev, image_of(m, "uint16")[None], 1000, *boxes)
        assert np.array_equal(got[0], M.fill(M.close_open(m, *boxes)))


def fill_only(ps, dev, m, connectivity=4):
    got, rounds, _ = run_plan(ps, dev, m.astype(np.uint8)[None], 0, 1, 1, connectivity)
    return got[0], rounds


def test_fill_follows_a_serpentine_corridor(ps, dev):
    m = M.serpentine(65, 67)
    want = M.fill(m, 4)
    assert np.array_equal(want, m)     # the corridor is one region and holds a corner: all of it is removed
    got, rounds = fill_only(ps, dev, m)
    print(f"serpentine 65 x 67: {rounds} fill rounds")
    assert np.array_equal(got, want)
    assert rounds > 8
    got8, _ = fill_only(ps, dev, m, 8)
    assert np.array_equal(got8, M.fill(m, 8))


def test_fill_leaks_through_a_diagonal_gap_with_connectivity_8_only(ps, dev):
    m = np.ones((70, 131), bool)
    m[:30, :64] = False          # holds the corner (0, 0); its last column is the last bit of a word
    m[30:50, 64:100] = False     # one diagonal step away, in the next word and the next row
    m[66:, 128:] = False         # the same at the far corner
    m[60:66, 120:128] = False
    for conn in (4, 8):
        want = M.fill(m, conn)
        got, _ = fill_only(ps, dev, m, conn)
        assert np.array_equal(got, want), conn
    assert M.fill(m, 4)[40, 80] and not M.fill(m, 8)[40, 80]
    assert np.array_equal(ps.get_img_mask(m.astype(np.uint8), 0, 1, 1, flood_fill_flag=8 | (255 << 8), device=dev), M.fill(m, 8))


def test_fill_edge_cases(ps, dev):
    inside = np.zeros((33, 65), bool)
    inside[:5, :5] = inside[-5:, -5:] = inside[:5, -5:] = inside[-5:, :5] = True    # every corner lies in the foreground: nothing is removed
    hole = np.ones((40, 70), bool)
    hole[-6:, 30:36] = False      # touches the border mid-edge and no corner: kept, so it becomes foreground
    hole[:3, :3] = False
    for m in (inside, np.zeros((17, 19), bool), np.ones((17, 19), bool), hole, np.zeros((1, 1), bool), np.ones((1, 1), bool),
              M.blobs((1, 300), 1), M.blobs((300, 1), 2), M.blobs((129, 130), 4, density=0.6, smooth=0)):
        for conn in (4, 8):
            got, _ = fill_only(ps, dev, m, conn)
            assert np.array_equal(got, M.fill(m, conn)), (m.shape, conn)
    assert M.fill(inside).all() and M.fill(hole)[-1, 32] and not M.fill(hole)[0, 0]


def test_stacks_rounds_and_the_aliased_output(ps, dev):
    tiles = np.stack([image_of(M.blobs((70, 130), s, density=0.35 + 0.1 * s, smooth=2), "uint16", s) for s in range(5)])
    tiles[3] = image_of(M.serpentine(70, 130), "uint16")
    want = np.stack([M.get_img_mask(t, 1000, 3, 4) for t in tiles])
    together, _, _ = run_plan(ps, dev, tiles[:3], 1000, 3, 4)
    for k in range(3):
        alone, _, _ = run_plan(ps, dev, tiles[k:k + 1], 1000, 3, 4)
        assert np.array_equal(alone[0], together[k]) and np.array_equal(alone[0], want[k])
    got, rounds, masked = run_plan(ps, dev, tiles, 1000, 3, 4, max_batch=2, masked=True)      # count above max_batch: three rounds of tiles
    assert np.array_equal(got, want)
    assert np.array_equal(masked, np.where(want, tiles, 0).astype(tiles.dtype))
    got, _, aliased = run_plan(ps, dev, tiles, 1000, 3, 4, max_batch=2, masked="alias")
    assert np.array_equal(got, want) and np.array_equal(aliased, masked)
    f32 = tiles.astype(np.float32)
    got, _, masked = run_plan(ps, dev, f32, float(np.log1p(np.float32(1000))), 3, 4, log_domain=True, masked=True)
    want_log = np.stack([M.get_img_mask(t, float(np.log1p(np.float32(1000))), 3, 4, log_domain=True) for t in f32])
    assert np.array_equal(got, want_log) and np.array_equal(masked, np.where(want_log, f32, 0).astype(np.float32))


# ---- through filter_streaks -----------------------------------------------------------------------------------------------------

BOX = dict(close_steps=5, open_steps=9)
FILTER = dict(sigma=(8, 8), level=0, wavelet="db9", padding_mode="reflect", bidirectional=True)


@functools.lru_cache(maxsize=None)
def specimen(dtype):
    """a bright body with holes and specks on a dark background with stripes, (130, 150)"""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[:130, :150]
    body = ((yy - 62) / 45.0) ** 2 + ((xx - 77) / 58.0) ** 2 < 1
    body &= ~(((yy - 60) ** 2 + (xx - 70) ** 2) < 36)            # a ventricle
    img = np.where(body, 2400.0, 90.0) * (1 + 0.15 * rng.standard_normal(body.shape)) + 25 * np.sin(yy / 3.0)
    img[rng.random(body.shape) < 0.004] = 3000.0                 # specks in the background and the body
    img = np.clip(img, 1, 60000)
    img = np.rint(img).astype(np.uint16) if dtype == "uint16" else (img + 0.37).astype(np.float32)
    img.setflags(write=False)
    return img


def log_mask(img, clip_med):
    """the restatement's mask of the log image; a float tile must keep 4 float32 ulps between every log1p and the clip, so the device's
    log1pf cannot move a sample across"""
    log = np.log1p(img, dtype=np.float32)
    if img.dtype.kind == "f":
        gap = np.abs(log.astype(np.float64) - float(np.float32(clip_med))).min()
        print(f"closest log1p to clip_med={clip_med}: {gap:.3g} = {gap / np.spacing(np.float32(clip_med)):.1f} ulps (more than 4 asked)")
        assert gap > 4 * np.spacing(np.float32(clip_med))
    mask = M.get_img_mask(log, clip_med, BOX["close_steps"], BOX["open_steps"])
    assert 0.2 < mask.mean() < 0.8 and not np.array_equal(mask, log > np.float32(clip_med))    # the boxes and the fill do act
    return mask


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_filter_streaks_with_explicit_clips(ps, dev, dtype):
    img = specimen(dtype)
    clips = dict(bleach_correction_clip_min=float(np.log1p(60)), bleach_correction_clip_med=float(np.log1p(700.25)),
                 bleach_correction_clip_max=float(np.log1p(3500)))
    mask = log_mask(img, clips["bleach_correction_clip_med"])
    zeroed = np.where(mask, img, 0).astype(img.dtype)
    for extra in (dict(bleach_correction_frequency=1 / 32, **clips), dict(bleach_correction_clip_med=clips["bleach_correction_clip_med"])):
        want = ps.filter_streaks(zeroed.copy(), device=dev, log_output=True, extended=True, **FILTER, **extra)
        got = ps.filter_streaks(img.copy(), device=dev, log_output=True, extended=True, enable_masking=True, **BOX, **FILTER, **extra)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        plain = ps.filter_streaks(img.copy(), device=dev, log_output=True, extended=True, **FILTER, **extra)
        assert not np.array_equal(got, plain)
        for none in ("close_steps", "open_steps"):     # the reference skips the mask when a box is None
            off = ps.filter_streaks(img.copy(), device=dev, log_output=True, extended=True, enable_masking=True, **FILTER, **extra,
                                    **dict(BOX, **{none: None}))
            assert np.array_equal(off, plain)
    same = ps.filter_streaks(img.copy(), sigma=(0, 0), enable_masking=True, extended=True, device=dev, **BOX)
    assert np.array_equal(same, img)     # the early return comes first: nothing is masked


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_filter_streaks_with_estimated_clips(ps, dev, dtype):
    import torch
    img = specimen(dtype)
    auto = dict(bleach_correction_frequency=1 / 32)
    plan = ps.Plan(dev, img.shape, img.dtype, ps.make_params(img.dtype, log_output=True, keep_uniform=True, extended=True, **FILTER, **auto))
    try:
        plan.run(torch.from_numpy(img.copy()).to(dev)[None])
        torch.cuda.synchronize(dev)
        triples, status = plan.clips()
    finally:
        plan.close()
    assert status[0] == 0
    lo, med, hi = (float(v) for v in triples[0])
    print(f"{dtype}: the un-masked run reports clips {lo}, {med}, {hi}")
    mask = log_mask(img, med)
    zeroed = np.where(mask, img, 0).astype(img.dtype)
    want = ps.filter_streaks(zeroed, device=dev, log_output=True, extended=True, **FILTER, **auto, bleach_correction_clip_min=lo,
                             bleach_correction_clip_med=med, bleach_correction_clip_max=hi)
    got = ps.filter_streaks(img.copy(), device=dev, log_output=True, extended=True, enable_masking=True, **BOX, **FILTER, **auto)
    assert np.array_equal(got, want)
    # a stack of two different tiles: each gets its own clips and its own mask
    other = np.ascontiguousarray(img[::-1] // 2 if dtype == "uint16" else img[::-1] * np.float32(0.5))
    both = ps.filter_streaks(np.stack([img, other]), device=dev, log_output=True, extended=True, enable_masking=True, **BOX, **FILTER, **auto)
    alone = ps.filter_streaks(other.copy(), device=dev, log_output=True, extended=True, enable_masking=True, **BOX, **FILTER, **auto)
    assert np.array_equal(both[0], want) and np.array_equal(both[1], alone)
    # without a frequency only the median is estimated, and it is the same one
    med_only = ps.filter_streaks(img.copy(), device=dev, log_output=True, extended=True, enable_masking=True, **BOX, **FILTER)
    assert np.array_equal(med_only, ps.filter_streaks(zeroed, device=dev, log_output=True, extended=True, **FILTER))


# ---- the C ABI alone ------------------------------------------------------------------------------------------------------------

def test_abi_refusals_name_the_argument(dev):
    import torch
    from ipp_amd import capi
    lib = capi.lib()
    good = dict(dev=0, ny=8, nx=9, dtype=capi.PS_U16, close_steps=3, open_steps=3, connectivity=4, max_batch=2)
    for name, value in [("ny", 0), ("nx", 0), ("nx", (1 << 30) + 1), ("dtype", 7), ("close_steps", 0), ("open_steps", -1), ("connectivity", 6),
                        ("connectivity", 0)]:
        h = C.c_void_p()
        rc = lib.mi_tile_mask_plan_create(*dict(good, **{name: value}).values(), C.byref(h))
        assert rc == capi.MI_ERR_INVALID and name in capi.last_error() and not h.value, (name, capi.last_error())
    h = C.c_void_p()
    capi.check(lib.mi_tile_mask_plan_create(*good.values(), C.byref(h)))
    try:
        info = capi.TileMaskInfo()
        capi.check(lib.mi_tile_mask_plan_info(h, C.byref(info)))
        assert info.max_batch == 2 and info.fill_rounds == 0 and info.scratch_bytes > 0
        tiles = torch.from_numpy(np.zeros((1, 8, 9), np.uint16)).to(dev)
        mask = torch.empty((1, 8, 9), dtype=torch.uint8, device=dev)
        stream = capi.current_stream_ptr(dev)
        for name, args in [("in", (None, 1.0, 0, mask.data_ptr(), None, 1)), ("mask", (tiles.data_ptr(), 1.0, 0, None, None, 1)),
                           ("count", (tiles.data_ptr(), 1.0, 0, mask.data_ptr(), None, -1)),
                           ("log_domain", (tiles.data_ptr(), 1.0, 1, mask.data_ptr(), None, 1)),
                           ("threshold", (tiles.data_ptr(), float("nan"), 0, mask.data_ptr(), None, 1))]:
            rc = lib.mi_tile_mask_run(h, stream, *args)
            assert rc == capi.MI_ERR_INVALID and name in capi.last_error(), (name, capi.last_error())
        capi.check(lib.mi_tile_mask_run(h, stream, tiles.data_ptr(), 1.0, 0, mask.data_ptr(), None, 0))
        capi.check(lib.mi_tile_mask_run(h, stream, tiles.data_ptr(), 1.0, 0, mask.data_ptr(), None, 1))
        torch.cuda.synchronize(dev)
        assert int(mask.sum()) == 0      # an all-background tile: every sample hangs on a corner
        capi.check(lib.mi_tile_mask_plan_info(h, C.byref(info)))
        assert info.fill_rounds >= 1
    finally:
        capi.check(lib.mi_tile_mask_plan_destroy(h))
    assert lib.mi_tile_mask_plan_destroy(None) == capi.MI_OK
