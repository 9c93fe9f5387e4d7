"""CPU: the tile resize of pystripe's batch_filter (include/mi_tile_resize.h) without a device: the library's tables
against the numpy tables of the recipe, the recipe against scipy's zoom (tests/tile_resize_util.py) on every shape pair the GPU
tests use, the decision rule from the shapes alone, and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from tests import tile_resize_util as U


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


@pytest.mark.parametrize("n,m", [(37, 53), (41, 60), (70, 33), (9, 20), (1, 4), (3, 2), (2048, 2560), (1024, 853)])
def test_library_tables_equal_the_recipe(ps, n, m):
    i0, i1, t = ps.tile_resize_tables(n, m)
    w0, w1, wt = U.tables(n, m)
    assert np.array_equal(i0, w0) and np.array_equal(i1, w1)
    assert t.dtype == np.float64 and np.array_equal(t, wt)   # bit for bit
    assert i0.min() >= 0 and max(i0.max(), i1.max()) <= n - 1 and i1.min() >= 0
    assert (t >= 0).all() and (t < 1).all()


@pytest.mark.parametrize("T,N", U.CASES)
def test_recipe_against_zoom(T, N):
    for dtype in U.DTYPES:
        for seed in U.SEEDS:
            tile = U.pattern(T, dtype, seed)
            got = U.recipe(tile, N)
            if dtype == np.float32:
                want = U.zoom_ref(tile, N)
                assert got.dtype == np.float32 and np.array_equal(got, want), (T, N, seed)
            else:
                share = U.check_integer(got, tile, N, f"{T} -> {N} {np.dtype(dtype).name} seed {seed}")
                assert share >= 0.5


def test_decision_rule_from_the_shapes_alone(ps):
    with pytest.raises(NotImplementedError, match="new_size"):
        ps.resize_decision((37, 41), (53, 29))
    assert ps.resize_decision((40, 50), (30, 64)) == (30, 64)      # T > N as tuples: no filter
    assert ps.resize_decision((33, 10), (33, 25)) == (33, 25)
    assert ps.resize_decision((64, 48), (80, 60)) == (80, 60)
    assert ps.resize_decision((32, 24), (27, 20)) == (27, 20)
    assert ps.resize_decision((33, 25), (33, 10)) == (33, 10)      # T > N: a shrinking axis without a filter
    assert ps.resize_decision((64, 48), (64, 48)) is None          # equal shapes build no step
    assert ps.resize_decision((64, 48), np.array([64, 48])) is None
    assert ps.resize_decision((64, 48), None) is None
    for bad in ((0, 5), (5, -1), (5,), (5, 6, 7), (5.0, 6), "ab", 7, (True, 5)):
        with pytest.raises(ValueError, match="new_size"):
            ps.resize_decision((8, 8), bad)
        with pytest.raises(ValueError, match="new_size"):
            ps.batch_filter("in", "out", new_size=bad)
    # through the entries, before a device is looked for
    with pytest.raises(NotImplementedError, match="new_size"):
        ps.Pipeline(None, (37, 41), np.uint16, new_size=(53, 29))
    with pytest.raises(NotImplementedError, match="new_size"):
        ps.Pipeline(None, (74, 82), np.uint16, new_size=(53, 29), down_sample=(2, 2))
    with pytest.raises(NotImplementedError, match="new_size"):
        ps.batch_filter("in", "out", tile_size=(37, 41), new_size=(53, 29))
    with pytest.raises(NotImplementedError, match="new_size"):
        ps.Pipeline(None, (64, 48), np.uint16, new_size=(80, 60), d_type="float32")   # the fractions of the float64 image would stay
    with pytest.raises(NotImplementedError, match="new_size"):
        ps.process_img(np.zeros((8, 8), np.uint16), new_size=(4, 4))


def test_command_line_takes_both_sizes_or_none(ps):
    a = ps._parse_args(["--input", "x", "--size_y", "80", "--size_x", "60"])
    assert ps._cli_new_size(a) == (80, 60)
    assert ps._cli_new_size(ps._parse_args(["--input", "x"])) is None
    for argv in (["--size_y", "80"], ["--size_x", "60"]):
        with pytest.raises(RuntimeError, match="both new_size_x and new_size_y are needed"):
            ps.main(["--input", "x"] + argv)


def test_c_abi_refusals_name_the_argument(ps):
    from ipp_amd import capi
    lib = capi.lib()
    h = C.c_void_p()
    for args, word in (((0, 5, 4, 4, capi.PS_U16), "ny=0"), ((5, 0, 4, 4, capi.PS_U16), "nx=0"), ((5, 5, 0, 4, capi.PS_U16), "my=0"),
                       ((5, 5, 4, -3, capi.PS_U16), "mx=-3"), ((5, 5, 4, 4, 7), "dtype=7")):
        assert lib.mi_tile_resize_plan_create(0, *args, 1, C.byref(h)) == capi.MI_ERR_INVALID
        assert word in capi.last_error() and not h
    buf_i, buf_t = (C.c_int * 4)(), (C.c_double * 4)()
    assert lib.mi_tile_resize_tables(0, 4, buf_i, buf_i, buf_t) == capi.MI_ERR_INVALID and "n=0" in capi.last_error()
    assert lib.mi_tile_resize_tables(4, 0, buf_i, buf_i, buf_t) == capi.MI_ERR_INVALID and "m=0" in capi.last_error()
    with pytest.raises(TypeError, match="dtype"):
        ps.ResizePlan(None, (5, 5), (4, 4), np.float64)
