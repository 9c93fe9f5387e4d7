"""Trees for the tests of the TeraFly tree reader, assembled on the CPU: the numpy restatement of the conversion
(tests/terafly_util.py) gives every block file's pages and the mdata.bin bytes, ``mi_tiff3d_write_blocks`` writes the files.  Also the
levels those files add up to, the boxes every tree is read with, and an editor of TIFF directory entries for the refusals."""
import ctypes as C
import os
import struct

import numpy as np

from tests import terafly_util as tu

# name -> (dtype, (D, V, H), flags of the restatement, LZW, rows per strip (0: the whole page), BigTIFF)
TREES = {
    "u16_lzw_rps1_tiled": ("uint16", (24, 510, 505), ["--resolutions=012", "--height=250", "--width=250", "--depth=12"], True, 1, False),
    "u8_lzw_rps8_tiled": ("uint8", (24, 503, 510), ["--resolutions=01", "--height=250", "--width=250", "--depth=12"], True, 8, False),
    "u16_raw_page": ("uint16", (10, 260, 270), ["--resolutions=01"], False, 0, False),
    "u8_raw_rps1_big": ("uint8", (10, 260, 270), ["--resolutions=012"], False, 1, True),
    "u16_lzw_page_big": ("uint16", (9, 263, 271), ["--resolutions=01", "--halve=max"], True, 0, True),
    "u16_raw_rps8": ("uint16", (10, 261, 270), ["--resolutions=0"], False, 8, False),
}


def volume(dtype, shape, seed):
    """compressible and not trivial: a ramp, blobs of noise, a constant region"""
    rng = np.random.default_rng(seed)
    D, V, H = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(V), np.arange(H), indexing="ij")
    top = np.iinfo(dtype).max
    vol = ((7 * z + y // 3 + x // 5) % (top + 1)).astype(dtype)
    noisy = rng.random(shape) < 0.15
    vol[noisy] = rng.integers(0, top + 1, int(noisy.sum())).astype(dtype)
    vol[:, V // 3:V // 2, H // 4:H // 2] = top // 3
    return vol


def write_tree(root, name):
    """Writes tree `name` under root; returns [level volumes (z, y, x), largest first]"""
    from ipp_amd import capi
    dtype, shape, flags, lzw, rps, big = TREES[name]
    vol = volume(dtype, shape, sorted(TREES).index(name) + 50)
    files, mdata = tu.convert(vol, flags)
    lib = capi.lib()
    names = sorted(files)
    pages = [np.ascontiguousarray(files[k]) for k in names]
    for k in names:
        os.makedirs(os.path.dirname(os.path.join(root, k)), exist_ok=True)
    m = len(names)
    strides, dims = [], []
    for p in pages:
        strides += [p.shape[1] * p.shape[2], p.shape[2]]
        dims += [p.shape[2], p.shape[1], p.shape[0]]
    capi.check(lib.mi_tiff3d_write_blocks(m, (C.c_char_p * m)(*[os.fsencode(os.path.join(root, k)) for k in names]),
                                          (C.c_void_p * m)(*[p.ctypes.data for p in pages]), (C.c_int64 * (2 * m))(*strides),
                                          (C.c_int * (3 * m))(*dims), (C.c_int * m)(*([0] * m)), (C.c_int * m)(*[p.shape[0] for p in pages]),
                                          vol.dtype.itemsize, 1 if lzw else 0, rps if rps else 1 << 20, 1 if big else 0, 4))
    for res, b in mdata.items():
        with open(os.path.join(root, res, "mdata.bin"), "wb") as f:
            f.write(b)
    return levels_of(files)


def levels_of(files):
    """The level volumes that {relative name: pages} add up to, largest first: directories sorted are rows and columns, files sorted are
    the blocks along D"""
    out = []
    for res in sorted({k.split("/")[0] for k in files}, key=lambda r: -int(r[4:].split("x")[0])):
        tree = {}
        for k in sorted(files):
            if k.startswith(res + "/"):
                _, vd, hd, f = k.split("/")
                tree.setdefault(vd, {}).setdefault(hd, []).append(files[k])
        out.append(np.concatenate([np.concatenate([np.concatenate(tree[vd][hd], axis=0) for hd in sorted(tree[vd])], axis=2) for vd in sorted(tree)],
                                  axis=1))
    return out


def boxes(shape, seams):
    """(z0, z1, y0, y1, x0, x1): the whole level, one voxel, a box with odd offsets across every seam (`seams` = (zs, ys, xs): the
    first voxel of every block but the first, per axis), a box inside one row"""
    D, V, H = shape
    out = [(0, D, 0, V, 0, H), (D - 1, D, V // 2, V // 2 + 1, H - 1, H)]
    lo = [max(1, (min(s) if s else n // 2) - 3) for s, n in zip(seams, shape)]
    hi = [min(n - 1, (max(s) if s else n // 2) + 4) for s, n in zip(seams, shape)]
    lo = [v | 1 for v in lo]
    out.append((lo[0], max(hi[0], lo[0] + 1), lo[1], max(hi[1], lo[1] + 1), lo[2], max(hi[2], lo[2] + 1)))
    out.append((D // 2, D // 2 + 1, V // 3, V // 3 + 1, 5, min(H, 37)))
    return out


def seams_of(level):
    """(zs, ys, xs) of a TreeLevel: where its blocks begin, but for the first"""
    b = level.mdata["blocks"]
    return (level.z_start[1:-1], sorted({q["abs_v"] for q in b} - {0}), sorted({q["abs_h"] for q in b} - {0}))


# ------------------------------------------------------------------------------------------------------------------ directory editor
def entries(path):
    """[{tag: (entry offset, type, count, offset of the value field)}] per page of a classic little-endian TIFF, and next-IFD offsets"""
    b = open(path, "rb").read()
    assert b[:4] == b"II*\0", "the editor takes classic files"
    off, = struct.unpack_from("<I", b, 4)
    pages = []
    while off:
        n, = struct.unpack_from("<H", b, off)
        tags = {}
        for k in range(n):
            at = off + 2 + 12 * k
            tag, typ, cnt = struct.unpack_from("<HHI", b, at)
            tags[tag] = (at, typ, cnt, at + 8)
        pages.append(tags)
        off, = struct.unpack_from("<I", b, off + 2 + 12 * n)
    return pages


def poke(path, at, fmt, *values):
    with open(path, "r+b") as f:
        f.seek(at)
        f.write(struct.pack(fmt, *values))


def strip_tiff(path, stream, width, rows=1, compression=5):
    """A classic one-page TIFF of `rows` x `width` bytes whose only strip is `stream`, taken as it is"""
    body = stream + (b"\0" if len(stream) % 2 else b"")
    tags = [(254, 4, 2), (256, 4, width), (257, 4, rows), (258, 3, 8), (259, 3, compression), (262, 3, 1), (273, 4, 8), (277, 3, 1),
            (278, 4, rows), (279, 4, len(stream)), (284, 3, 1)]
    ifd = struct.pack("<H", len(tags)) + b"".join(struct.pack("<HHII", t, ty, 1, v) for t, ty, v in tags) + struct.pack("<I", 0)
    with open(path, "wb") as f:
        f.write(b"II*\0" + struct.pack("<I", 8 + len(body)) + body + ifd)
    return str(path)


def multi_strip_tiff(path, streams, width, rows_each, compression=5, gap_bytes=0):
    """A classic one-page TIFF of len(streams) * rows_each x `width` bytes whose strips are `streams`, taken as they are and laid out
    back to back from file offset 8, strip k behind gap_bytes[k] bytes (a number: the same gap everywhere) that belong to no strip
    and are not zero.  Strips so begin at any byte; the directory is put on an even offset behind them."""
    n = len(streams)
    gaps = [gap_bytes] * n if isinstance(gap_bytes, int) else list(gap_bytes)
    assert len(gaps) == n
    body, offs = bytearray(), []
    for g, s in zip(gaps, streams):
        body += b"\xa5" * g
        offs.append(8 + len(body))
        body += s
    body += b"\xa5" * (len(body) % 2)
    cnts = [len(s) for s in streams]
    at = 8 + len(body)
    if n > 1:
        body += struct.pack(f"<{n}I", *offs) + struct.pack(f"<{n}I", *cnts)
    tags = [(254, 4, 1, 2), (256, 4, 1, width), (257, 4, 1, n * rows_each), (258, 3, 1, 8), (259, 3, 1, compression), (262, 3, 1, 1),
            (273, 4, n, at if n > 1 else offs[0]), (277, 3, 1, 1), (278, 4, 1, rows_each), (279, 4, n, at + 4 * n if n > 1 else cnts[0]),
            (284, 3, 1, 1)]
    ifd = struct.pack("<H", len(tags)) + b"".join(struct.pack("<HHII", *t) for t in tags) + struct.pack("<I", 0)
    with open(path, "wb") as f:
        f.write(b"II*\0" + struct.pack("<I", 8 + len(body)) + body + ifd)
    return str(path)
