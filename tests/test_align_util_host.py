"""CPU: the guarded offset buffers of tests/align_util.py -- the base residues they promise, and that the guard check sees a write
one element outside the view on either side and nothing else."""
import numpy as np
import pytest

from tests import align_util as A

CASES = [(dt, off) for dt, offs in A.OFFSETS.items() for off in offs]


@pytest.mark.parametrize("dtype,off", CASES)
def test_base_address_has_the_requested_residue(dtype, off):
    isz = np.dtype(dtype).itemsize
    fill = (np.arange(3 * 5 * 8) % 251).astype(dtype).reshape(3, 5, 8)
    v, check = A.offset_numpy((3, 5, 8), dtype, off, fill)
    assert v.dtype == np.dtype(dtype) and v.shape == (3, 5, 8) and v.flags["C_CONTIGUOUS"]
    assert v.ctypes.data % 16 == off * isz % 16
    assert (v.ctypes.data - off * isz) % 256 == 0
    assert np.array_equal(v, fill)
    check()
    v[...] = 0          # writing every element of the view is not a guard violation
    check()


def test_offsets_cover_the_residues_the_kernels_distinguish():
    res = {dt: sorted(off * np.dtype(dt).itemsize % 16 for off in offs) for dt, offs in A.OFFSETS.items()}
    assert res == {"float32": [4, 8, 12], "uint16": [2, 8], "uint8": [1, 8]}


@pytest.mark.parametrize("dtype,off", CASES)
@pytest.mark.parametrize("where", ["before", "after"])
def test_one_element_outside_the_view_fails_the_guard_check(dtype, off, where):
    v, check = A.offset_numpy((4, 16), dtype, off, np.zeros((4, 16), dtype))
    import ctypes
    # the element just in front of the view / just behind it, reached through its address (both lie inside the guarded buffer)
    addr = v.ctypes.data + (-v.itemsize if where == "before" else v.nbytes)
    one = np.ctypeslib.as_array((ctypes.c_ubyte * v.itemsize).from_address(addr))
    saved = one.copy()
    one[:] = 0
    with pytest.raises(AssertionError, match="in front of the view" if where == "before" else "behind the view"):
        check()
    one[:] = saved
    check()


def test_sentinel_is_finite_and_seen_through_the_integer_view():
    v, check = A.offset_numpy((8,), np.float32, 1)
    assert np.isfinite(v).all() and (v.view(np.uint32) == A.sentinel_bits(4)).all()
    # a NaN in the guard differs from the sentinel bit-wise (a float comparison would call NaN != NaN for any pattern)
    import ctypes
    one = np.ctypeslib.as_array((ctypes.c_float * 1).from_address(v.ctypes.data + v.nbytes))
    one[0] = np.nan
    with pytest.raises(AssertionError):
        check()
