"""GPU: the device route of the tree writer (csrc/tiff3d_lzw_enc.hip).  The LZW stream of a strip is determined by its bytes and
the schedule, so everything here is byte equality: the batch encoder against ``lzw_util.encode`` (the corpus of
tests/lzw_enc_util.py, strided and unaligned sources, a slot one byte short), the block files of ``mi_tiff3d_write_blocks_device``
against those of ``mi_tiff3d_write_blocks``, and the trees of ``teraconverter --lzw_encoder=device`` against the host route's and
the reference binary's goldens."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import lzw_enc_util as eu
from tests import lzw_util as lu
from tests import terafly_util as tu
from tests.test_gpu_terafly import BASE, _check_against_golden, _series, _tree

pytestmark = pytest.mark.gpu

I64P, I32P, VPP = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_void_p)
CANARY = 0xCD


def _encode(dev, src_ptrs, rows, rowb, stride, slots=None):
    """mi_tiff_lzw_encode_strips_device -> (rc, packed bytes, out_off, lengths, status); slots = (tensor, slot_off, slot_cap)"""
    from ipp_amd import capi
    lib = capi.lib()
    n = len(src_ptrs)
    src = np.ascontiguousarray(src_ptrs, np.uint64)
    rows = np.ascontiguousarray(rows, np.int32)
    rowb = np.ascontiguousarray(rowb, np.int32)
    stride = np.ascontiguousarray(stride, np.int64)
    cap = int((rows.astype(np.int64) * rowb * 3 // 2 + 16 + 3).sum())
    out = np.full(cap + 64, CANARY, np.uint8)
    out_off, lengths, status = np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int32)
    used = C.c_int64(-1)
    if slots is None:
        so, sc, ds, dsn = None, None, None, 0
    else:
        t, off, caps = slots
        off, caps = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(caps, np.int64)
        so, sc, ds, dsn = off.ctypes.data_as(I64P), caps.ctypes.data_as(I64P), t.data_ptr(), t.numel()
    rc = lib.mi_tiff_lzw_encode_strips_device(dev.index, capi.current_stream_ptr(dev), n, src.ctypes.data_as(VPP), rows.ctypes.data_as(I32P),
                                              rowb.ctypes.data_as(I32P), stride.ctypes.data_as(I64P), so, sc, ds, dsn, out.ctypes.data, cap,
                                              out_off.ctypes.data_as(I64P), lengths.ctypes.data_as(I64P), status.ctypes.data_as(I32P),
                                              C.byref(used))
    assert (out[cap:] == CANARY).all()
    return rc, out[:cap], out_off, lengths, status, used.value


def _check_packed(strips, out, out_off, lengths, status, used):
    """every stream is the Python encoder's, at its documented place; nothing else in the packed buffer"""
    at = 0
    align = eu.pack_align()
    for k, data in enumerate(strips):
        want = eu.reference(data)
        assert status[k] == 0, k
        assert lengths[k] == len(want), (k, len(data))
        assert out_off[k] == at, k
        assert out[at:at + len(want)].tobytes() == want, (k, len(data))
        end = at + len(want)
        at = (end + align - 1) // align * align
        assert not out[end:at].any(), k
    assert used == at
    assert (out[at:] == CANARY).all()


def test_the_corpus_in_one_batch(dev):
    """3000 short noise strips in front of the corpus: the three table classes and the packing offsets are all in play"""
    import torch
    strips = eu.noise_strips(3000, 500) + list(eu.corpus().values())
    flat = np.frombuffer(b"".join(strips), np.uint8)
    t = torch.from_numpy(flat.copy()).to(dev)
    sizes = np.array([len(s) for s in strips], np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rc, out, out_off, lengths, status, used = _encode(dev, t.data_ptr() + starts, np.ones(len(strips)), sizes, sizes)
    assert rc == 0
    _check_packed(strips, out, out_off, lengths, status, used)
    assert (t.cpu().numpy() == flat).all()


LEVELS = {
    # dtype: (shape, blocks (z0, y0, x0, nz, ny, nx)): odd first columns and rows; 30 and 31 rows leave a short last strip of 4
    np.uint8: ((7, 37, 301), [(1, 3, 5, 3, 30, 131), (0, 1, 151, 2, 33, 150), (4, 5, 1, 3, 31, 299)]),
    np.uint16: ((5, 33, 259), [(1, 1, 3, 3, 31, 129), (0, 3, 131, 2, 30, 128), (2, 1, 1, 3, 32, 257)]),
}


@pytest.mark.parametrize("rps", [1, 4, 64])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_strided_and_unaligned_sources(dev, dtype, rps):
    import torch
    shape, blocks = LEVELS[dtype]
    item = np.dtype(dtype).itemsize
    rng = np.random.default_rng(5)
    # smooth rows with noise in the low bits: strings of several bytes and literals
    level = ((np.arange(np.prod(shape)).reshape(shape) // 7) % 200 + rng.integers(0, 3, shape)).astype(dtype)
    guard = 4096 + 1                                     # the level begins at an odd byte of the buffer (uint8)
    if item == 2:
        guard = 4096 + 2
    buf = np.full(guard + level.nbytes + 4096, CANARY, np.uint8)
    buf[guard:guard + level.nbytes] = level.view(np.uint8).ravel()
    t = torch.from_numpy(buf.copy()).to(dev)
    base = t.data_ptr() + guard
    ptrs, rows, rowb, strips = [], [], [], []
    for z0, y0, x0, nz, ny, nx in blocks:
        assert x0 % 2 == 1 and y0 % 2 == 1
        for p in range(nz):
            for r in range(0, ny, rps):
                ptrs.append(base + (((z0 + p) * shape[1] + y0 + r) * shape[2] + x0) * item)
                rows.append(min(rps, ny - r))
                rowb.append(nx * item)
        strips += eu.strips_of_block(level, z0, y0, x0, nz, ny, nx, rps)
    if rps == 4:
        assert min(rows) < 4
    if rps == 64:
        assert len(rows) == sum(b[3] for b in blocks)   # one strip per page
    n = len(ptrs)
    # slots of the caller with gaps between them
    caps = np.array([r * b * 3 // 2 + 16 for r, b in zip(rows, rowb)], np.int64)
    gaps = 32
    off = np.zeros(n, np.int64)
    at = gaps
    for k in range(n):
        off[k] = at
        at += (caps[k] + 3) // 4 * 4 + gaps
    slots = torch.full((int(at),), CANARY, dtype=torch.uint8, device=dev)
    rc, out, out_off, lengths, status, used = _encode(dev, ptrs, rows, rowb, [shape[2] * item] * n, (slots, off, caps))
    assert rc == 0
    _check_packed(strips, out, out_off, lengths, status, used)
    assert (t.cpu().numpy() == buf).all()
    got = slots.cpu().numpy()
    inside = np.zeros(got.size, bool)
    for k in range(n):
        inside[off[k]:off[k] + caps[k]] = True
        assert got[off[k]:off[k] + lengths[k]].tobytes() == eu.reference(strips[k]), k
    assert (got[~inside] == CANARY).all()


def test_a_slot_one_byte_short(dev):
    """the bounded path: the status word, the whole stream's length, MI_ERR_NOMEM, and not a byte behind the slot"""
    import torch
    from ipp_amd import capi
    strips = eu.noise_strips(3, 500, seed0=77)
    want = [eu.reference(s) for s in strips]
    t = torch.from_numpy(np.frombuffer(b"".join(strips), np.uint8).copy()).to(dev)
    caps = np.array([len(want[0]), len(want[1]) - 1, len(want[2])], np.int64)
    off = np.array([64, 64 + 1024, 64 + 2048], np.int64)
    slots = torch.full((4096,), CANARY, dtype=torch.uint8, device=dev)
    rc, out, out_off, lengths, status, used = _encode(dev, t.data_ptr() + np.arange(3) * 500, [1] * 3, [500] * 3, [500] * 3, (slots, off, caps))
    assert rc == capi.MI_ERR_NOMEM
    assert "larger than its bound" in capi.last_error()
    assert list(status) == [0, 1, 0]
    assert list(lengths) == [len(w) for w in want]
    got = slots.cpu().numpy()
    inside = np.zeros(got.size, bool)
    for k in range(3):
        inside[off[k]:off[k] + caps[k]] = True
        assert got[off[k]:off[k] + caps[k]].tobytes() == want[k][:caps[k]], k
    assert (got[~inside] == CANARY).all()
    for k in (0, 2):
        assert out[out_off[k]:out_off[k] + lengths[k]].tobytes() == want[k]


def _write_blocks(dev, folder, vol, device, bigtiff, rps, calls):
    """the blocks of `vol` written in `calls` appends by the host or the device route; the files' bytes by name"""
    import torch
    from ipp_amd import capi
    lib = capi.lib()
    folder.mkdir()
    nz, ny, nx = vol.shape
    t = torch.from_numpy(vol).to(dev) if device else None
    item = vol.dtype.itemsize
    cuts = [(1, 1, 150, 131), (1, 151, 100, 140), (101, 3, 90, 255)]      # (y0, x0, ny, nx)
    z_at = 0
    for n_pages in calls:
        paths, first, strides, dims, page0, total = [], [], [], [], [], []
        for b, (y0, x0, h, w) in enumerate(cuts):
            paths.append(os.fsencode(str(folder / f"block{b}.tif")))
            at = ((z_at * ny + y0) * nx + x0) * item
            first.append((t.data_ptr() if device else vol.ctypes.data) + at)
            strides += [ny * nx, nx]
            dims += [w, h, n_pages]
            page0.append(z_at)
            total.append(nz)
        m = len(paths)
        args = (m, (C.c_char_p * m)(*paths), (C.c_void_p * m)(*first), (C.c_int64 * (2 * m))(*strides), (C.c_int * (3 * m))(*dims),
                (C.c_int * m)(*page0), (C.c_int * m)(*total), item, 1, rps, 1 if bigtiff else 0, 4)
        if device:
            capi.check(lib.mi_tiff3d_write_blocks_device(dev.index, capi.current_stream_ptr(dev), *args))
        else:
            capi.check(lib.mi_tiff3d_write_blocks(*args))
        z_at += n_pages
    return {f: (folder / f).read_bytes() for f in sorted(os.listdir(folder))}


@pytest.mark.parametrize("bigtiff", [0, 1])
@pytest.mark.parametrize("dtype,rps", [(np.uint16, 1), (np.uint8, 7)])
def test_block_files_equal_the_host_route(dev, tmp_path, dtype, rps, bigtiff):
    """one call from device memory, one from host memory: classic and BigTIFF, a second call appending to the same files"""
    rng = np.random.default_rng(9)
    shape = (6, 200, 300)
    vol = ((np.arange(np.prod(shape)).reshape(shape) // 5) % 251 + rng.integers(0, 4, shape)).astype(dtype)
    host = _write_blocks(dev, tmp_path / "host", vol, False, bigtiff, rps, [4, 2])
    device = _write_blocks(dev, tmp_path / "device", vol, True, bigtiff, rps, [4, 2])
    assert sorted(host) == sorted(device) and len(host) == 3
    for f in host:
        assert host[f] == device[f], f
        pages, _ = lu.tiff_pages(str(tmp_path / "device" / f))
        assert len(pages) == 6 and pages[5][297] == (5, 6)


def _convert(g, src, out, extra):
    from ipp_amd import teraconverter
    out.mkdir()
    return teraconverter.main(BASE + [str(f) for f in g["flags"]] + [f"-s={src}", f"-d={out}"] + extra)


def _same_files(a, b):
    assert _tree(a) == _tree(b)
    for f in _tree(a):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


@pytest.mark.parametrize("name", tu.golden_runs())
def test_device_route_writes_the_host_routes_tree(name, tmp_path, dev, capsys):
    from ipp_amd import capi, terafly
    g = tu.load_golden(name)
    src = tmp_path / "src"
    _series(tu.golden_input(g), src)
    if any("uncompress" in str(f) for f in g["flags"]):
        # the device route writes LZW: asking for it with an uncompressed tree is refused by name
        assert _convert(g, src, tmp_path / "device", ["--lzw_encoder=device"]) == 2
        assert "uncompressed tree" in capsys.readouterr().err
        return
    before = dict(terafly.route_counts), capi.lib().mi_tiff_lzw_encode_device_batches()
    assert _convert(g, src, tmp_path / "host", ["--lzw_encoder=host"]) == 0
    assert capi.lib().mi_tiff_lzw_encode_device_batches() == before[1] and terafly.route_counts["host"] == before[0]["host"] + 1
    assert _convert(g, src, tmp_path / "device", ["--lzw_encoder=device"]) == 0
    assert capi.lib().mi_tiff_lzw_encode_device_batches() > before[1] and terafly.route_counts["device"] == before[0]["device"] + 1
    _check_against_golden(g, tmp_path / "device")
    _same_files(tmp_path / "host", tmp_path / "device")


def test_strips_collected_over_several_bands(tmp_path, dev):
    g = tu.load_golden("u16_tiled")
    src = tmp_path / "src"
    _series(tu.golden_input(g), src)
    assert _convert(g, src, tmp_path / "host", ["--lzw_encoder=host"]) == 0
    for rows in (8, 24):
        out = tmp_path / f"device{rows}"
        assert _convert(g, src, out, ["--lzw_encoder=device", f"--slab_rows={rows}"]) == 0
        _check_against_golden(g, out)
        _same_files(tmp_path / "host", out)


def test_routes_and_refusals(tmp_path, dev, monkeypatch):
    from ipp_amd import capi, terafly
    g = tu.load_golden("u16_tiled")
    src = tmp_path / "src"
    _series(tu.golden_input(g), src)
    o = tu.parse_flags([str(f) for f in g["flags"]])
    kw = dict(resolutions=o["resolutions"], halve=o["halve"], block=(o["height"], o["width"], o["depth"]), isotropic=o["isotropic"],
              fixed_tiling=o["fixed_tiling"], sub=tuple(o[k] for k in ("V0", "V1", "H0", "H1", "D0", "D1")))
    batches = capi.lib().mi_tiff_lzw_encode_device_batches

    def run(name, **more):
        out = tmp_path / name
        out.mkdir()
        before = dict(terafly.route_counts), batches()
        terafly.convert(src, out, **kw, **more)
        took = [r for r in terafly.ENCODERS if terafly.route_counts[r] == before[0][r] + 1]
        assert len(took) == 1 and (batches() > before[1]) == (took[0] == "device")
        return took[0], out

    monkeypatch.delenv("MI_TERAFLY_WRITE_DEVICE", raising=False)
    assert run("unset")[0] == terafly.DEFAULT_ENCODER
    monkeypatch.setenv("MI_TERAFLY_WRITE_DEVICE", "1")
    route, by_env = run("env1")
    assert route == "device"
    assert run("env1_host", encoder="host")[0] == "host"            # the argument wins
    monkeypatch.setenv("MI_TERAFLY_WRITE_DEVICE", "0")
    route, host = run("env0")
    assert route == "host"
    assert run("env0_device", encoder="device")[0] == "device"
    _same_files(host, by_env)
    # an uncompressed tree and strips that may cross a band: refused when asked for by name, the host route quietly otherwise
    with pytest.raises(ValueError, match="uncompressed tree"):
        run("raw_device", encoder="device", compression=False)
    with pytest.raises(ValueError, match="row bands"):
        run("rps_device", encoder="device", rows_per_strip=4, slab_rows=8)
    monkeypatch.setenv("MI_TERAFLY_WRITE_DEVICE", "1")
    assert run("raw_env", compression=False)[0] == "host"
    route, banded = run("rps_env_bands", rows_per_strip=4, slab_rows=8)
    assert route == "host"
    # one band over the whole height takes strips of several rows
    route, whole = run("rps_device_one_band", encoder="device", rows_per_strip=4, slab_rows=100000)
    assert route == "device"
    _same_files(banded, whole)
    with pytest.raises(ValueError, match="host or device"):
        run("bad", encoder="gpu")
