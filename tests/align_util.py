"""Guarded buffers whose base address is offset from a 256-byte boundary by a chosen number of elements.

Every fresh device allocation is 256-byte aligned or better, so a kernel's fallback for a pointer that is only element-aligned
never runs unless a test builds such a pointer on purpose.  ``offset_numpy`` / ``offset_tensor`` cut a contiguous view out of
one flat buffer

    [ guard | off | payload (numel) | guard ]        (guard: a multiple of 64 elements, all of it a sentinel bit pattern)

starting at element ``guard + off``, and hand back a checker that asserts both guard regions (the ``off`` elements in front of the
view included) are still bit-for-bit the sentinel -- compared through an integer view of the element's width, so a NaN written
there is seen too."""
import numpy as np

GUARD = 64  # elements; a multiple of 64

# offsets (elements) worth running, per element type: float32 4 / 8 / 12 bytes -- 8 is what float2-safe but float4-unsafe code gets
# wrong --, uint16 2 / 8 bytes, uint8 1 / 8 bytes
OFFSETS = {"float32": (1, 2, 3), "uint16": (1, 4), "uint8": (1, 8)}

# sentinel bit patterns per element width; the 4-byte one is a finite float32 (-6.26e18)
_SENTINEL = {1: 0xA5, 2: 0xA5C3, 4: 0xDEADBEEF}
_INT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def sentinel_bits(itemsize):
    return _INT[itemsize](_SENTINEL[itemsize])


def _layout(shape, off, guard):
    assert guard > 0 and guard % 64 == 0, "guard must be a multiple of 64 elements"
    assert off >= 0
    numel = int(np.prod(shape, dtype=np.int64))
    return numel, guard + off + numel + guard


def _aligned_start(base_addr, itemsize, guard):
    """Elements to skip so that the front guard of the flat buffer ends on a 256-byte boundary."""
    skip = (-(base_addr + guard * itemsize)) % 256
    assert skip % itemsize == 0
    return skip // itemsize


def offset_numpy(shape, dtype, off, fill=None, guard=GUARD):
    """(view, check): a C-contiguous numpy array of ``shape`` whose first element lies ``off`` elements past a 256-byte boundary."""
    dtype = np.dtype(dtype)
    isz = dtype.itemsize
    numel, total = _layout(shape, off, guard)
    raw = np.empty(total + 256 // isz, dtype=_INT[isz])
    s = _aligned_start(raw.ctypes.data, isz, guard)
    flat = raw[s:s + total]
    flat[:] = sentinel_bits(isz)
    view = flat[guard + off:guard + off + numel].view(dtype).reshape(shape)
    if fill is not None:
        view[...] = np.asarray(fill, dtype=dtype).reshape(shape)
    assert view.flags["C_CONTIGUOUS"]
    assert view.ctypes.data % 16 == (off * isz) % 16, (view.ctypes.data % 16, off, isz)
    assert (view.ctypes.data - off * isz) % 256 == 0

    def check(what=""):
        want = sentinel_bits(isz)
        front, back = flat[:guard + off], flat[guard + off + numel:]
        assert back.size == guard
        bad = np.flatnonzero(front != want)
        assert bad.size == 0, f"{what} wrote {bad.size} element(s) in front of the view, the nearest {guard + off - int(bad[-1])} before it"
        bad = np.flatnonzero(back != want)
        assert bad.size == 0, f"{what} wrote {bad.size} element(s) behind the view, the nearest {int(bad[0])} past its end"

    return view, check


def offset_tensor(shape, dtype, off, device, fill=None, guard=GUARD):
    """(view, check) like ``offset_numpy`` for a contiguous device tensor.  ``dtype`` is a torch dtype (float32, uint16, int16,
    uint8); ``fill`` a numpy array / tensor of ``shape`` (left as the sentinel when None)."""
    import torch
    isz = torch.empty((), dtype=dtype).element_size()
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[isz]
    numel, total = _layout(shape, off, guard)
    raw = torch.empty(total + 256 // isz, dtype=idt, device=device)
    s = _aligned_start(raw.data_ptr(), isz, guard)
    flat = raw[s:s + total]
    bits = int(np.array(_SENTINEL[isz], dtype=_INT[isz]).view({1: np.uint8, 2: np.int16, 4: np.int32}[isz]))
    flat.fill_(bits)
    view = flat[guard + off:guard + off + numel].view(dtype).view(tuple(shape))
    if fill is not None:
        src = torch.from_numpy(np.ascontiguousarray(fill)) if isinstance(fill, np.ndarray) else fill
        assert tuple(src.shape) == tuple(shape) and src.element_size() == isz
        view.view(idt).copy_(src.contiguous().view(idt))
    assert view.is_contiguous()
    assert view.data_ptr() % 16 == (off * isz) % 16, (view.data_ptr() % 16, off, isz)
    assert (view.data_ptr() - off * isz) % 256 == 0

    def check(what=""):
        front = flat[:guard + off].cpu().numpy()
        back = flat[guard + off + numel:].cpu().numpy()
        assert back.size == guard
        bad = np.flatnonzero(front != bits)
        assert bad.size == 0, f"{what} wrote {bad.size} element(s) in front of the view, the nearest {guard + off - int(bad[-1])} before it"
        bad = np.flatnonzero(back != bits)
        assert bad.size == 0, f"{what} wrote {bad.size} element(s) behind the view, the nearest {int(bad[0])} past its end"

    return view, check


def payload_is_sentinel(view):
    """True when every element of a device view made with ``fill=None`` still holds the sentinel (an output a refused call must
    leave alone)."""
    import torch
    isz = view.element_size()
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[isz]
    got = view.view(idt).cpu().numpy().view(_INT[isz])
    return bool((got == sentinel_bits(isz)).all())
