"""GPU: the tile resize of pystripe's batch_filter (include/mi_tile_resize.h, ipp_amd.pystripe) against scipy's zoom and clip
(tests/tile_resize_util.py: ``zoom_ref``, the restatement of ``resize(..., anti_aliasing=False)`` of DESIGN.md section 14).

Standards: a float32 tile is bit-equal to ``zoom_ref``; an integer tile goes through ``check_integer`` (samples whose float64
interpolant lies further than 2^-30 from an integer are trunc(v) exactly, the others rint(v) or rint(v) - 1 inside the tile's range;
at least half of every case's samples are of the first kind).  Through ``Pipeline`` and ``batch_filter`` the tile that enters the
resize is the device's own (the same options without ``new_size`` and without conversion, flip and rotation), so what is compared
is the resize and what follows it, not the stripe filter."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import tile_resize_util as U

pytestmark = pytest.mark.gpu

PIPE = dict(sigma=(8, 8), wavelet="db9", padding_mode="reflect", bidirectional=True)
T0, N0 = (64, 48), (80, 60)


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


@functools.lru_cache(maxsize=None)
def batch(T, dtype_name, seeds=U.SEEDS):
    stack = np.stack([U.pattern(T, np.dtype(dtype_name), s) for s in seeds])
    stack.setflags(write=False)
    return stack


def check_tile(got, tile, N, what, **kw):
    if tile.dtype == np.float32:
        want = U.zoom_ref(tile, N)
        assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
        diff = got != want
        assert not diff.any(), f"{what}: {int(diff.sum())} float32 samples differ from zoom_ref, max {np.abs(got - want).max():g}"
    else:
        U.check_integer(got, tile, N, what, **kw)


def run_abi(dev, stack, N, max_batch):
    """through the C ABI alone: plan_create / run / destroy on torch's current stream"""
    import torch
    from ipp_amd import capi
    lib = capi.lib()
    n, ny, nx = stack.shape
    code = {np.dtype(np.uint8): capi.PS_U8, np.dtype(np.uint16): capi.PS_U16, np.dtype(np.float32): capi.PS_F32}[stack.dtype]
    h = C.c_void_p()
    capi.check(lib.mi_tile_resize_plan_create(dev.index or 0, ny, nx, N[0], N[1], code, max_batch, C.byref(h)))
    try:
        tin = torch.from_numpy(np.ascontiguousarray(stack)).to(dev)
        out = torch.empty((n,) + tuple(N), dtype=tin.dtype, device=dev)
        capi.check(lib.mi_tile_resize_run(h, capi.current_stream_ptr(dev), tin.data_ptr(), out.data_ptr(), n))
        torch.cuda.synchronize(dev)
        return out.cpu().numpy()
    finally:
        capi.check(lib.mi_tile_resize_plan_destroy(h))


@pytest.mark.parametrize("T,N", U.CASES)
def test_abi_and_resize_tiles(dev, ps, T, N):
    for dtype in U.DTYPES:
        stack = batch(T, np.dtype(dtype).name)
        # two tiles per round: three tiles take two rounds, and the tiles of an odd shape start at every alignment
        for name, got in (("abi", run_abi(dev, stack, N, 2)), ("resize_tiles", ps.resize_tiles(np.array(stack), N, device=dev))):
            assert got.shape == (len(stack),) + tuple(N) and got.dtype == stack.dtype
            for k, tile in enumerate(stack):
                check_tile(got[k], tile, N, f"{name} {T} -> {N} {stack.dtype.name} tile {k}")


def test_resize_tiles_containers_and_copy(dev, ps):
    import torch
    tile = np.array(batch((37, 41), "uint16")[0])
    one = ps.resize_tiles(tile, (53, 60), device=dev)
    assert isinstance(one, np.ndarray) and one.shape == (53, 60) and one.dtype == np.uint16
    t = ps.resize_tiles(torch.from_numpy(tile).to(dev), (53, 60))
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), one)
    for name in ("uint8", "uint16", "float32"):   # equal shapes: the copy
        stack = np.array(batch((37, 41), name))
        assert np.array_equal(run_abi(dev, stack, (37, 41), 2), stack)


@pytest.mark.parametrize("name", ["uint16", "float32"])
def test_a_tile_does_not_depend_on_its_batch(dev, ps, name):
    for T, N in (((37, 41), (53, 60)), ((45, 70), (19, 33))):
        stack = np.array(batch(T, name, (0, 1, 2, 3, 4)))
        together = run_abi(dev, stack, N, 0)
        for k in range(len(stack)):
            alone = run_abi(dev, stack[k:k + 1], N, 0)[0]
            assert np.array_equal(together[k], alone), (T, N, k)
        assert np.array_equal(run_abi(dev, stack[::-1], N, 3)[::-1], together)


def test_offsets_past_2_31_samples(dev, ps):
    """One launch over more than 2^31 input and output samples (520 uint8 tiles of 2048^2 -> 2049 x 2047): the tiles past the
    32-bit range equal the same tiles run alone, and the last one passes the check against zoom_ref."""
    import torch
    T, N, count = (2048, 2048), (2049, 2047), 520
    assert count * T[0] * T[1] > 2 ** 31 and count * N[0] * N[1] > 2 ** 31
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    tiles = torch.randint(0, 256, (count,) + T, dtype=torch.uint8, device=dev, generator=g)
    plan = ps.ResizePlan(dev, T, N, np.uint8, max_batch=count)
    try:
        out = plan.run(tiles)
        for k in (0, 511, 512, count - 1):
            assert torch.equal(plan.run(tiles[k:k + 1].contiguous())[0], out[k]), k
        last = out[count - 1].cpu().numpy()
    finally:
        plan.close()
    U.check_integer(last, tiles[count - 1].cpu().numpy(), N, "tile 519 of 520")


def _mid_tiles(ps, dev, stack, **opts):
    """what enters the resize, from the device itself: the same head options without new_size and without the tail options"""
    import torch
    plan = ps.Pipeline(dev, stack.shape[1:], stack.dtype, **opts)
    try:
        out = plan.run(torch.from_numpy(stack).to(dev)).cpu().numpy()
    finally:
        plan.close()
    return out


PIPELINE_CASES = {
    "dark": (dict(dark=100), {}),
    "filter": (dict(PIPE), {}),
    "to8": ({}, dict(convert_to_8bit=True, bit_shift_to_right=3)),
    "rot90_flip": ({}, dict(rotate=90, flip_upside_down=True)),
    "all": (dict(PIPE, dark=100), dict(convert_to_8bit=True, bit_shift_to_right=3, rotate=90, flip_upside_down=True)),
}


@pytest.mark.parametrize("case", sorted(PIPELINE_CASES))
def test_through_pipeline(dev, ps, case):
    import torch
    head, tail = PIPELINE_CASES[case]
    stack = np.array(batch(T0, "uint16"))
    stack[1] = 777   # a uniform tile
    mid = _mid_tiles(ps, dev, stack, **head)
    assert mid.dtype == np.uint16 and mid.shape == stack.shape and not mid[1].any()
    plan = ps.Pipeline(dev, T0, np.uint16, new_size=N0, **head, **tail)
    try:
        assert plan.resize is not None and (plan.tail is not None) == bool(tail)
        got = plan.run(torch.from_numpy(stack).to(dev)).cpu().numpy()
    finally:
        plan.close()

    def convert(a):
        return ps.convert_to_8bit_fun(a, tail["bit_shift_to_right"]) if tail.get("convert_to_8bit") else a

    def place(a):
        a = np.flipud(a) if tail.get("flip_upside_down") else a
        return np.rot90(a, tail.get("rotate", 0) // 90)

    out_shape = N0[::-1] if tail.get("rotate") == 90 else N0
    assert got.shape == (3,) + out_shape and got.dtype == (np.uint8 if tail.get("convert_to_8bit") else np.uint16)
    assert not got[1].any()   # the uniform tile: zeros of new_size, rotated, in the converted type
    for k in (0, 2):
        U.check_integer(got[k], mid[k], N0, f"pipeline {case} tile {k}", convert=convert, place=place)
    # equal shapes build no step
    same = ps.Pipeline(dev, T0, np.uint16, new_size=T0, **head, **tail)
    try:
        assert same.resize is None
    finally:
        same.close()


def test_batch_filter_end_to_end(dev, ps, tmp_path):
    src, n_tiles = tmp_path / "in", 6
    tiles = {}
    for k in range(n_tiles):
        tile = U.pattern(T0, np.uint16, 10 + k) if k != 3 else np.full(T0, 500, np.uint16)
        rel = f"{'a' if k < 3 else 'b'}/tile_{k}.tif"
        (src / rel).parent.mkdir(parents=True, exist_ok=True)
        assert ps.imsave_tif(src / rel, tile)
        tiles[rel] = tile
    (src / "b" / "broken.tif").write_bytes(b"II*\x00 not a tiff at all")
    tiles["b/broken.tif"] = np.zeros(T0, np.uint16)
    files = ps.find_tiles(src)
    assert len(files) == n_tiles + 1
    for run, (down, new) in enumerate(((None, N0), ((2, 2), (27, 20)))):
        dst, stats = tmp_path / f"out{run}", {}
        kw = dict(files_list=files, workers=8, continue_process=False, print_input_file_names=False, timeout=None, gaussian_filter_2d=False,
                  bleach_correction_frequency=None, bleach_correction_max_method=False, sigma=(8, 8), level=0, wavelet="db9", crossover=10,
                  threshold=None, padding_mode="reflect", bidirectional=True, lightsheet=False, down_sample=down, tile_size=T0, new_size=new,
                  d_type="uint16", convert_to_8bit=False, bit_shift_to_right=8, compression=("ADOBE_DEFLATE", 1), threads_per_gpu=8)
        assert ps.batch_filter(src, dst, stats=stats, device=dev, **kw) == 0
        assert stats["written"] == n_tiles + 1 and stats["zero_tiles"] == 1
        stack = np.stack(list(tiles.values()))
        mid = _mid_tiles(ps, dev, stack, down_sample=down, **PIPE)
        assert mid.shape[1:] == (T0 if down is None else (32, 24))
        for k, rel in enumerate(tiles):
            got = ps.imread_tif_raw_png(dst / rel)
            assert got is not None and got.shape == new and got.dtype == np.uint16, rel
            if rel.endswith(("tile_3.tif", "broken.tif")):
                assert not got.any(), rel
            else:
                U.check_integer(got, mid[k], new, f"batch_filter {rel} -> {new}")
        stats = {}
        kw["continue_process"] = True
        assert ps.batch_filter(src, dst, stats=stats, device=dev, **kw) == 0
        assert stats["written"] == 0 and stats["skipped_existing"] == n_tiles + 1
