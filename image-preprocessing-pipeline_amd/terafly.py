"""The TeraFly conversion: a folder of 2-D TIFF slices to the multi-resolution "TIFF (tiled, 3D)" tree that Vaa3D / TeraFly open.

    convert(src, dst, resolutions="012345", halve="mean", ...)

restates ``teraconverter --sfmt="TIFF (series, 2D)" --dfmt="TIFF (tiled, 3D)"`` (VolumeConverter::generateTilesVaa3DRaw,
VolumeConverter.cpp:1840-2520) for single-channel 8- and 16-bit series:

    <dst>/RES(<V>x<H>x<D>)/<V0>/<V0>_<H0>/<V0>_<H0>_<D0>.tif       one multi-page TIFF per block, LZW, RowsPerStrip 1
    <dst>/RES(<V>x<H>x<D>)/mdata.bin                               TiledVolume::save of the level

The volume is walked in z-groups of ``z_max_res = max(min(64, block_depth / 2), 2^halve_pow2[last])`` slices; each group is halved
on its own (``mi_pyramid_slab``, include/mi_pyramid.h), so a group loses its odd last slice at every 3-D level -- why
RES(...x9) of 37 slices holds 8 pages.  The level names still say ``depth / 2^h``.  A group's slices go to the device in row
bands sized from the free device memory (band heights are multiples of 2^deepest level, so the bands halve as the whole plane
does); each level's pages are appended to their block files (``mi_tiff3d_write_blocks``, LZW on a host thread pool) as soon as
the group is done, as appendSlice2Tiff3DFile does.  With ``encoder="device"`` the strips are encoded on the GPU from the band's
levels instead (``mi_tiff_lzw_encode_strips_device``; only the streams come back) and the pages appended from the collected
streams (``mi_tiff3d_write_blocks_encoded``): the same files, byte for byte.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import struct
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

STANDARD_BLOCK_DEPTH = 64        # IM_config.h
TMITREE_MIN_BLOCK_DIM = 250      # IM_config.h:151
MAX_LEVELS = 10                  # S_MAX_MULTIRES: the levels --resolutions can name
HALVE = {"mean": 0, "max": 1}    # mi_halve_method


def _tiles(total, block, fixed):
    """Block sizes along one axis: ``ceil(total / block)`` blocks as uniform as possible, or (fixed tiling) ``block`` each and a
    smaller last one (VolumeConverter.cpp:1925-1955)."""
    n = int(math.ceil(total / np.float32(block)))
    if fixed:
        return [block if k < n - 1 else (block if total % block == 0 else total % block) for k in range(n)]
    return [total // n + (1 if k < total % n else 0) for k in range(n)]


def _name6(v):
    return str(int(v)).rjust(6, "0")


@dataclass
class Plan:
    """Every decision of the conversion that does not depend on voxel values."""
    depth: int
    height: int
    width: int
    V0: int
    H0: int
    D0: int
    selected: list
    hp: list                 # halve_pow2[i]: D is halved 2^hp[i] times at level i
    rows: list               # rows[i]: block heights at level i
    cols: list
    deps: list               # deps[i]: nominal block depths at level i
    z_max_res: int
    bytes: int = 2
    n_res: int = field(init=False)

    def __post_init__(self):
        self.n_res = len(self.hp)

    def level_shape(self, i):
        return self.depth // 2 ** self.hp[i], self.height // 2 ** i, self.width // 2 ** i

    def res_dir(self, i):
        d, v, h = self.level_shape(i)
        return f"RES({v}x{h}x{d})"

    def v_name(self, i, r0):
        return _name6((self.V0 + r0 * 2 ** i) * 10)

    def h_name(self, i, c0):
        return _name6((self.H0 + c0 * 2 ** i) * 10)

    def d_name(self, i, s):
        return _name6(self.D0 * 10 + 2 ** self.hp[i] * s * 10)

    def blocks(self, i):
        """[(row start, rows, col start, cols, "V/V_H")] of level i."""
        out, r0 = [], 0
        for nr in self.rows[i]:
            c0 = 0
            for nc in self.cols[i]:
                vn, hn = self.v_name(i, r0), self.h_name(i, c0)
                out.append((r0, nr, c0, nc, f"{vn}/{vn}_{hn}"))
                c0 += nc
            r0 += nr
        return out

    def groups(self):
        """[(z, z_size)]: the z-groups, relative to D0 (z_size of the leftover group = depth % z_max_res)."""
        z_ratio = self.depth // self.z_max_res
        return [(z, self.z_max_res if g + 1 <= z_ratio else self.depth % self.z_max_res)
                for g, z in enumerate(range(0, self.depth, self.z_max_res))]

    def appends(self):
        """Per group, per selected level: [(level, D-block index, first group page, pages)] -- the reference's block walk
        (stack_block / slice_start / slice_end, one block change at most per group)."""
        blk = [0] * self.n_res
        s_end = [self.deps[i][0] - 1 for i in range(self.n_res)]
        out = []
        for z, z_size in self.groups():
            g = []
            for i in range(self.n_res):
                h = 2 ** self.hp[i]
                if z // h > s_end[i]:
                    blk[i] += 1
                    s_end[i] += self.deps[i][blk[i]] if blk[i] < len(self.deps[i]) else 0
                n = z_size // h
                if not self.selected[i] or n <= 0:
                    continue
                split = n
                for bz in range(n):
                    if z // h + bz > s_end[i]:
                        split = bz
                        break
                if split > 0:
                    g.append((i, blk[i], 0, split))
                if split < n:
                    g.append((i, blk[i] + 1, split, n - split))
            out.append(g)
        return out

    def d_block_start(self, i, k):
        return sum(self.deps[i][:k])


def plan(shape, resolutions="0", block=(-1, -1, -1), isotropic=False, fixed_tiling=False, sub=(-1, -1, -1, -1, -1, -1),
         bytes_per_sample=2) -> Plan:
    """The plan of a series of ``shape`` = (D, V, H) slices; ``block`` = (--height, --width, --depth), -1 = the whole extent;
    ``sub`` = (--V0, --V1, --H0, --H1, --D0, --D1), -1 = unset (D1 / V1 / H1 excluded)."""
    D, V, H = shape
    V0, V1, H0, H1, D0, D1 = sub
    V0 = max(V0, 0)
    H0 = max(H0, 0)
    D0 = max(D0, 0)
    V1 = V if V1 < 0 or V1 > V else V1
    H1 = H if H1 < 0 or H1 > H else H1
    D1 = D if D1 < 0 or D1 > D else D1
    if V0 >= V1 or H0 >= H1 or D0 >= D1:
        raise ValueError(f"empty subvolume [{V0},{V1}) x [{H0},{H1}) x [{D0},{D1}) of a {V} x {H} x {D} series")
    height, width, depth = V1 - V0, H1 - H0, D1 - D0
    bh, bw, bd = (height if block[0] < 0 else block[0], width if block[1] < 0 else block[1], depth if block[2] < 0 else block[2])
    if bh < TMITREE_MIN_BLOCK_DIM or bw < TMITREE_MIN_BLOCK_DIM:
        raise ValueError(f"blocks of {bh} x {bw}: the minimum dimension for block height and width is {TMITREE_MIN_BLOCK_DIM} "
                         "(VolumeConverter::generateTilesVaa3DRaw)")
    if bd <= 0:
        raise ValueError(f"block depth {bd}")
    selected = [str(i) in str(resolutions) for i in range(MAX_LEVELS)]
    if not any(selected):
        raise ValueError(f"--resolutions={resolutions!r} selects no level (digits 0..{MAX_LEVELS - 1})")
    n_res = max(i + 1 for i in range(MAX_LEVELS) if selected[i])
    if isotropic:
        # a 2-D series has unit voxels (SimpleVolume): D is halved whenever VXL_D <= 2 max(VXL_V, VXL_H) at that level
        hp = [0] * n_res
        vx2, hx2, vd = np.float32(2), np.float32(2), np.float32(1)
        for i in range(1, n_res):
            hp[i] = hp[i - 1]
            if vd <= max(vx2, hx2):
                hp[i] += 1
                vd *= 2
            vx2 *= 2
            hx2 *= 2
    else:
        hp = list(range(n_res))
    rows = [_tiles(height // 2 ** i, bh, fixed_tiling) for i in range(n_res)]
    cols = [_tiles(width // 2 ** i, bw, fixed_tiling) for i in range(n_res)]
    deps = []
    for i in range(n_res):
        t = depth // 2 ** hp[i]
        n = int(math.ceil(t / np.float32(bd)))
        if fixed_tiling:   # the reference sizes the last block from depth / 2^i whatever halve_pow2 says (VolumeConverter.cpp:1930)
            last = depth // 2 ** i
            deps.append([bd if k < n - 1 else (bd if last % bd == 0 else last % bd) for k in range(n)])
        else:
            deps.append([t // n + (1 if k < t % n else 0) for k in range(n)])
    for i in range(n_res):
        if min(height // 2 ** i, width // 2 ** i) <= 0 or not deps[i]:
            raise ValueError(f"level {i} of a {height} x {width} x {depth} volume is empty")
    z_max_res = max(min(STANDARD_BLOCK_DEPTH, bd // 2), 2 ** hp[n_res - 1])
    if z_max_res > 1 and z_max_res > bd // 2:
        raise ValueError(f"too much resolutions({n_res}): too much slices ({z_max_res}) in the buffer "
                         f"(block depth {bd}: VolumeConverter::generateTilesVaa3DRaw)")
    return Plan(depth, height, width, V0, H0, D0, selected, hp, rows, cols, deps, z_max_res, bytes_per_sample)


def mdata_bytes(p: Plan, i: int) -> bytes:
    """RES(...)/mdata.bin of level i (TiledVolume::save + Block::binarizeInto; MDATA_BIN_FILE_VERSION 2, reference system
    {1,2,3}, voxels 2^i x 2^i x 2^hp[i] um, origin from the first block's file name in 0.1 um / 1e4)."""
    written = {k for g in p.appends() for (lv, k, _, _) in g if lv == i}
    dblocks = sorted(written)
    bl = p.blocks(i)
    nrows, ncols = len(p.rows[i]), len(p.cols[i])
    first_d = p.d_name(i, p.d_block_start(i, dblocks[0]))
    org = [np.float32(np.float32(int(v)) / np.float32(10000.0)) for v in (p.v_name(i, 0), p.h_name(i, 0), first_d)]
    sv, sd = float(2 ** i), float(2 ** p.hp[i])
    dim_d = sum(p.deps[i][k] for k in dblocks)
    b = struct.pack("<f3i", 2.0, 1, 2, 3) + struct.pack("<6f", sv, sv, sd, sv, sv, sd) + struct.pack("<3f", *org)
    b += struct.pack("<3I2H", sum(p.rows[i]), sum(p.cols[i]), dim_d, nrows, ncols)
    for r0, nr, c0, nc, dirname in bl:
        vh = dirname.split("/")[1]
        b += struct.pack("<5I2i", nr, nc, dim_d, len(dblocks), 1, r0, c0)
        b += struct.pack("<H", len(dirname) + 1) + dirname.encode() + b"\0"
        absd = 0
        for k in dblocks:
            f = f"{vh}_{p.d_name(i, p.d_block_start(i, k))}.tif"
            b += struct.pack("<H", len(f) + 1) + f.encode() + b"\0" + struct.pack("<Ii", p.deps[i][k], absd)
            absd += p.deps[i][k]
        b += struct.pack("<I", p.bytes)
    assert ncols * nrows == len(bl)
    return b


def output_files(p: Plan):
    """Every file the conversion writes, relative to dst, sorted."""
    names = set()
    for g in p.appends():
        for i, k, _, _ in g:
            for _, _, _, _, dirname in p.blocks(i):
                vh = dirname.split("/")[1]
                names.add(f"{p.res_dir(i)}/{dirname}/{vh}_{p.d_name(i, p.d_block_start(i, k))}.tif")
    names |= {f"{p.res_dir(i)}/mdata.bin" for i in range(p.n_res) if p.selected[i]}
    return sorted(names)


# ------------------------------------------------------------------------------------------------------------------ source
class Series:
    """A folder of single-channel 2-D TIFF slices, sorted by name (as the reference's SimpleVolume lists them)."""

    def __init__(self, folder):
        from . import brickio
        self.files = brickio.list_tiff_series(folder)
        if not self.files:
            raise ValueError(f"no *.tif slices in {folder}")
        info = brickio.tiff_info(self.files[0])
        self.fast = bool(info is not None and info[2])
        if info is not None and info[1] is not None:
            (ny, nx), dt = info[0], np.dtype(info[1])
        else:
            first = np.asarray(brickio._pil().open(self.files[0]))
            if first.ndim != 2:
                raise ValueError(f"{self.files[0]}: {first.shape[-1] if first.ndim == 3 else first.ndim}-channel slices: multi-channel "
                                 "and RGB sources are not supported (one channel of 8 or 16 bits)")
            (ny, nx), dt = first.shape, first.dtype
        if dt not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise ValueError(f"{self.files[0]}: {dt} samples; the TeraFly conversion takes 8- or 16-bit single-channel slices")
        if not self.fast:
            first = np.asarray(brickio._pil().open(self.files[0]))
            if first.ndim != 2:
                raise ValueError(f"{self.files[0]}: multi-channel and RGB sources are not supported (one channel of 8 or 16 bits)")
        self.shape = (len(self.files), ny, nx)
        self.dtype = dt

    def read(self, z0, z1, y0, y1, x0, x1, threads=0):
        from . import brickio
        files = self.files[z0:z1]
        if self.fast:
            try:
                return brickio.read_tiff_box(files, self.shape[1:], self.dtype, y0, y1, x0, x1, threads=threads)
            except Exception:
                pass   # a slice the native reader does not take: Pillow decides
        Image = brickio._pil()
        out = np.empty((len(files), y1 - y0, x1 - x0), self.dtype)
        for k, f in enumerate(files):
            a = np.asarray(Image.open(f))
            if a.shape != self.shape[1:] or a.dtype != self.dtype:
                raise ValueError(f"{f}: {a.dtype} {a.shape} differs from the first slice ({self.dtype} {self.shape[1:]})")
            out[k] = a[y0:y1, x0:x1]
        return out


# ------------------------------------------------------------------------------------------------------------------ device
def pyramid_slab(slab, n_levels, halve_d, method, outs):
    """``mi_pyramid_slab`` on torch tensors: ``slab`` (nz, ny, nx) uint8 / uint16 on the device, ``outs[k]`` the buffer of level
    k+1 (or None where the level is not needed)."""
    from . import capi
    hd = (C.c_int * n_levels)(*[int(v) for v in halve_d])
    ptrs = (C.c_void_p * n_levels)(*[None if o is None or o.numel() == 0 else o.data_ptr() for o in outs])
    nz, ny, nx = slab.shape
    capi.check(capi.lib().mi_pyramid_slab(slab.device.index, capi.current_stream_ptr(slab.device), slab.data_ptr(),
                                          slab.element_size(), nx, ny, nz, HALVE[method], n_levels, hd, ptrs))


def level_shapes(shape, n_levels, halve_d):
    """(nz, ny, nx) of levels 1..n_levels of a slab of ``shape``."""
    nz, ny, nx = shape
    out = []
    for k in range(n_levels):
        nz, ny, nx = (nz // 2 if halve_d[k] else nz), ny // 2, nx // 2
        out.append((nz, ny, nx))
    return out


def _band_rows(p: Plan, nbytes, device, slab_rows=None):
    """Rows of level 0 per device band: a multiple of 2^(deepest level) whose group band plus its levels fit in half the free
    device memory (or ``slab_rows``, rounded to that multiple)."""
    import torch
    unit = 2 ** (p.n_res - 1)
    if slab_rows is None:
        free, _ = torch.cuda.mem_get_info(device)
        per_row = p.z_max_res * p.width * nbytes * 2      # the band and (at most 1/4 + 1/16 + ...) its levels
        slab_rows = max(1, int(free // 2 // max(per_row, 1)))
    return max(unit, (int(slab_rows) // unit) * unit)


ENCODERS = ("host", "device")
DEFAULT_ENCODER = "host"         # what an unset MI_TERAFLY_WRITE_DEVICE means (DESIGN section 23 holds the measurement that decides it)
route_counts = {"host": 0, "device": 0}   # conversions per route in this process: the route report of the tests


def _encoder_route(encoder, compression, rows_per_strip, one_band):
    """"host" or "device" for a conversion.  ``encoder`` "host" / "device" is taken at its word (and "device" refused where the
    device route does not go); None reads MI_TERAFLY_WRITE_DEVICE (1: device, 0: host, unset: DEFAULT_ENCODER) and quietly takes the
    host route where the device route does not go."""
    if encoder is not None and encoder not in ENCODERS:
        raise ValueError(f"encoder={encoder!r}: host or device")
    why = None
    if not compression:
        why = "the device route writes LZW strips: an uncompressed tree (--libtiff_uncompress) is written on the host"
    elif rows_per_strip > 1 and not one_band:
        why = (f"strips of {rows_per_strip} rows may cross the row bands of the device: the device route takes them only when one "
               "band covers the whole height (a larger --slab_rows, or --libtiff_rowsperstrip=1)")
    if encoder == "device" and why:
        raise ValueError(f"encoder=device: {why}")
    if encoder is None:
        env = os.environ.get("MI_TERAFLY_WRITE_DEVICE", "")
        if env not in ("", "0", "1"):
            raise ValueError(f"MI_TERAFLY_WRITE_DEVICE={env}: 0 (host) or 1 (device)")
        encoder = {"": DEFAULT_ENCODER, "0": "host", "1": "device"}[env]
    return "host" if why else encoder


def _encode_band(lib, capi, dev, entries, levels, rps, bytes_, strip_ptr, strip_len, keep):
    """The strips of the group's blocks that lie in one row band, encoded from the band's device tensors.  ``entries``:
    [(level, first group page, pages, block row0, block rows, block col0, block cols, first strip)]; ``levels[i]`` = (tensor of
    level i for the band, its first row in the level).  The streams' addresses and lengths go to strip_ptr / strip_len at the
    strips' places in (block, page, strip) order; ``keep`` holds the buffers they point into."""
    src, rows, gidx, rowb, stride = [], [], [], [], []
    for i, g0, n, r0b, nr, c0, nc, strip0 in entries:
        t, a = levels[i]
        hb, W = t.shape[1], t.shape[2]
        spp = (nr + rps - 1) // rps
        s_lo = max(0, (a - r0b + rps - 1) // rps)
        s_hi = min(spp, (a + hb - r0b + rps - 1) // rps)
        if s_hi <= s_lo or n <= 0:
            continue
        s_idx = np.arange(s_lo, s_hi, dtype=np.int64)
        pp = np.arange(n, dtype=np.int64)[:, None]
        y = r0b + s_idx * rps - a                           # the strip's first row in the band's tensor
        src.append((np.uint64(t.data_ptr()) + (((g0 + pp) * hb + y[None, :]) * W + c0).astype(np.uint64) * np.uint64(bytes_)).ravel())
        gidx.append((strip0 + pp * spp + s_idx[None, :]).ravel())
        rows.append(np.broadcast_to(np.minimum(rps, nr - s_idx * rps)[None, :], (n, s_idx.size)).ravel())
        rowb.append(np.full(n * s_idx.size, nc * bytes_, np.int32))
        stride.append(np.full(n * s_idx.size, W * bytes_, np.int64))
    if not src:
        return
    src = np.ascontiguousarray(np.concatenate(src), np.uint64)
    gidx = np.concatenate(gidx)
    rows = np.ascontiguousarray(np.concatenate(rows), np.int32)
    rowb = np.concatenate(rowb)
    stride = np.concatenate(stride)
    m = src.size
    raw = rows.astype(np.int64) * rowb
    out = np.empty(int((raw * 3 // 2 + 16 + 3).sum()), np.uint8)      # every stream at its bound, each from a multiple of 4
    out_off = np.empty(m, np.int64)
    lengths = np.empty(m, np.int64)
    status = np.empty(m, np.int32)
    used = C.c_int64()
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    capi.check(lib.mi_tiff_lzw_encode_strips_device(
        dev.index, capi.current_stream_ptr(dev), m, src.ctypes.data_as(C.POINTER(C.c_void_p)), rows.ctypes.data_as(i32p),
        rowb.ctypes.data_as(i32p), stride.ctypes.data_as(i64p), None, None, None, 0, out.ctypes.data, out.size,
        out_off.ctypes.data_as(i64p), lengths.ctypes.data_as(i64p), status.ctypes.data_as(i32p), C.byref(used)))
    strip_ptr[gidx] = np.uint64(out.ctypes.data) + out_off.astype(np.uint64)
    strip_len[gidx] = lengths
    keep.append(out)


def convert(src, dst, resolutions="0", halve="mean", block=(-1, -1, -1), isotropic=False, fixed_tiling=False,
            sub=(-1, -1, -1, -1, -1, -1), compression=True, rows_per_strip=1, bigtiff=False, device=None, slab_rows=None,
            threads=0, progress=None, encoder=None):
    """Writes the TeraFly tree of the 2-D series in ``src`` under ``dst`` (an existing folder); ``slab_rows`` fixes the rows of
    a device band (default: from the free device memory).  ``encoder``: "host" encodes the LZW strips on a host thread pool,
    "device" on the GPU from the levels where the pyramid kernel left them (only the streams come back; the files are the same
    bytes); None takes MI_TERAFLY_WRITE_DEVICE (1 / 0) or, unset, DEFAULT_ENCODER.  Returns the Plan."""
    import torch
    from . import capi
    if halve not in HALVE:
        raise ValueError(f"--halve={halve}: mean or max")
    if encoder is not None and encoder not in ENCODERS:
        raise ValueError(f"encoder={encoder!r}: host or device")
    dst = Path(dst)
    if not dst.is_dir():
        raise ValueError(f"destination {dst} is not an existing folder (teraconverter -d must exist)")
    series = Series(src)
    p = plan(series.shape, resolutions, block, isotropic, fixed_tiling, sub, series.dtype.itemsize)
    capi.require_gpu()
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    tdtype = {1: torch.uint8, 2: torch.uint16}[p.bytes]
    n_lv = p.n_res - 1
    halve_d = [1 if p.hp[i] == p.hp[i - 1] + 1 else 0 for i in range(1, p.n_res)]
    band = _band_rows(p, p.bytes, dev, slab_rows)
    route = _encoder_route(encoder, compression, int(rows_per_strip), band >= p.height)
    route_counts[route] += 1
    for i in range(p.n_res):
        if p.selected[i]:
            for _, _, _, _, dirname in p.blocks(i):
                (dst / p.res_dir(i) / dirname).mkdir(parents=True, exist_ok=True)
    pages_in = {}                  # path -> pages written so far
    appends = p.appends()
    lib = capi.lib()
    all_groups = p.groups()
    for gi, (z, z_size) in enumerate(all_groups):
        if not appends[gi]:
            continue
        if route == "device":
            _device_group(lib, capi, series, p, dst, dev, tdtype, z, z_size, appends[gi], pages_in, band, halve, halve_d,
                          int(rows_per_strip), bigtiff, threads)
            if progress:
                progress(gi + 1, len(all_groups))
            continue
        host = [None] * p.n_res
        host[0] = series.read(p.D0 + z, p.D0 + z + z_size, p.V0, p.V0 + p.height, p.H0, p.H0 + p.width, threads)
        shapes = level_shapes(host[0].shape, n_lv, halve_d)
        for i in range(1, p.n_res):
            host[i] = np.empty(shapes[i - 1], host[0].dtype)
        need = [p.selected[k + 1] or (k % 2 == 1 and k + 1 < n_lv) for k in range(n_lv)]
        if n_lv > 0:
            for r0 in range(0, p.height, band):
                r1 = min(p.height, r0 + band)
                slab = torch.from_numpy(host[0][:, r0:r1]).to(dev)
                bshapes = level_shapes(slab.shape, n_lv, halve_d)
                outs = [torch.empty(s, dtype=tdtype, device=dev) if need[k] else None for k, s in enumerate(bshapes)]
                pyramid_slab(slab, n_lv, halve_d, halve, outs)
                for k, o in enumerate(outs):
                    if o is not None and p.selected[k + 1] and o.numel():
                        a = r0 >> (k + 1)
                        host[k + 1][:, a:a + o.shape[1]] = o.cpu().numpy()
                del slab, outs
        # pages of this group, appended to their block files in one call
        paths, first, strides, dims, page0, total = [], [], [], [], [], []
        for i, k, g0, n in appends[gi]:
            lv = host[i]
            for r0, nr, c0, nc, dirname in p.blocks(i):
                vh = dirname.split("/")[1]
                path = str(dst / p.res_dir(i) / dirname / f"{vh}_{p.d_name(i, p.d_block_start(i, k))}.tif")
                view = lv[g0:g0 + n, r0:r0 + nr, c0:c0 + nc]
                paths.append(os.fsencode(path))
                first.append(view.ctypes.data)
                strides += [lv.shape[1] * lv.shape[2], lv.shape[2]]
                dims += [nc, nr, n]
                page0.append(pages_in.get(path, 0))
                total.append(p.deps[i][k])
                pages_in[path] = pages_in.get(path, 0) + n
        m = len(paths)
        capi.check(lib.mi_tiff3d_write_blocks(m, (C.c_char_p * m)(*paths), (C.c_void_p * m)(*first), (C.c_int64 * (2 * m))(*strides),
                                              (C.c_int * (3 * m))(*dims), (C.c_int * m)(*page0), (C.c_int * m)(*total), p.bytes,
                                              1 if compression else 0, int(rows_per_strip), 1 if bigtiff else 0, int(threads)))
        if progress:
            progress(gi + 1, len(all_groups))
    write_mdata(p, dst)
    return p


def _device_group(lib, capi, series, p, dst, dev, tdtype, z, z_size, group, pages_in, band, halve, halve_d, rps, bigtiff, threads):
    """One z-group on the device route: every row band is uploaded and halved as on the host route, the strips of every selected
    level that lie in the band are encoded from the device tensors, and after the last band the group's pages are appended to
    their block files from the collected streams."""
    import torch
    n_lv = p.n_res - 1
    need = [p.selected[k + 1] or (k % 2 == 1 and k + 1 < n_lv) for k in range(n_lv)]
    level0 = series.read(p.D0 + z, p.D0 + z + z_size, p.V0, p.V0 + p.height, p.H0, p.H0 + p.width, threads)
    paths, dims, page0, total, entries = [], [], [], [], []
    nstrips = 0
    for i, k, g0, n in group:
        for r0, nr, c0, nc, dirname in p.blocks(i):
            vh = dirname.split("/")[1]
            path = str(dst / p.res_dir(i) / dirname / f"{vh}_{p.d_name(i, p.d_block_start(i, k))}.tif")
            paths.append(os.fsencode(path))
            dims += [nc, nr, n]
            page0.append(pages_in.get(path, 0))
            total.append(p.deps[i][k])
            pages_in[path] = pages_in.get(path, 0) + n
            entries.append((i, g0, n, r0, nr, c0, nc, nstrips))
            nstrips += n * ((nr + rps - 1) // rps)
    strip_ptr = np.zeros(nstrips, np.uint64)
    strip_len = np.zeros(nstrips, np.int64)
    keep = []
    for r0 in range(0, p.height, band):
        r1 = min(p.height, r0 + band)
        slab = torch.from_numpy(level0[:, r0:r1]).to(dev)
        levels = {0: (slab, r0)}
        if n_lv > 0:
            bshapes = level_shapes(slab.shape, n_lv, halve_d)
            outs = [torch.empty(s, dtype=tdtype, device=dev) if need[k] else None for k, s in enumerate(bshapes)]
            pyramid_slab(slab, n_lv, halve_d, halve, outs)
            for k, o in enumerate(outs):
                if o is not None and p.selected[k + 1] and o.numel():
                    levels[k + 1] = (o, r0 >> (k + 1))
        _encode_band(lib, capi, dev, [e for e in entries if e[0] in levels], levels, rps, p.bytes, strip_ptr, strip_len, keep)
        del slab, levels
    if nstrips and not strip_len.all():
        raise RuntimeError("terafly.convert: a strip of the group lies in no row band")
    m = len(paths)
    capi.check(lib.mi_tiff3d_write_blocks_encoded(m, (C.c_char_p * m)(*paths), (C.c_int * (3 * m))(*dims), (C.c_int * m)(*page0),
                                                  (C.c_int * m)(*total), p.bytes, rps, 1 if bigtiff else 0,
                                                  strip_ptr.ctypes.data_as(C.POINTER(C.c_void_p)), strip_len.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  int(threads)))


def write_mdata(p: Plan, dst):
    for i in range(p.n_res):
        if p.selected[i]:
            (Path(dst) / p.res_dir(i) / "mdata.bin").write_bytes(mdata_bytes(p, i))


# ------------------------------------------------------------------------------------------------------------------ reading a tree
class _Cursor:
    def __init__(self, b):
        self.b, self.at = bytes(b), 0

    def take(self, fmt, field):
        n = struct.calcsize(fmt)
        if self.at + n > len(self.b):
            raise ValueError(f"mdata.bin: truncated at {field} (byte {self.at} of {len(self.b)})")
        v = struct.unpack_from(fmt, self.b, self.at)
        self.at += n
        return v

    def name(self, field):
        n, = self.take("<H", f"{field} (length)")
        if self.at + n > len(self.b):
            raise ValueError(f"mdata.bin: truncated at {field} (byte {self.at} of {len(self.b)})")
        s = self.b[self.at:self.at + n]
        self.at += n
        return s.split(b"\0", 1)[0].decode()


def parse_mdata(b) -> dict:
    """The inverse of ``mdata_bytes`` (TiledVolume::load + Block::unBinarizeFrom, MDATA_BIN_FILE_VERSION 2)::

        version, reference_system (3 ints), voxel_123, voxel (V, H, D), origin (V, H, D), extents (V, H, D), n_rows, n_cols,
        blocks[row * n_cols + col] = {dir, height, width, depth, abs_v, abs_h, files, depths, abs_d, n_chans}, bytes_per_channel

    ``ValueError`` naming the field for a version other than 2, more than one channel or a truncated file."""
    c = _Cursor(b)
    version, = c.take("<f", "MDATA_BIN_FILE_VERSION")
    if version != 2.0:
        raise ValueError(f"mdata.bin: MDATA_BIN_FILE_VERSION is {version:g}: version 2 is read")
    ref = c.take("<3i", "reference_system")
    v123 = c.take("<3f", "VXL_1 / VXL_2 / VXL_3")
    vox = c.take("<3f", "VXL_V / VXL_H / VXL_D")
    org = c.take("<3f", "ORG_V / ORG_H / ORG_D")
    dim = c.take("<3I", "DIM_V / DIM_H / DIM_D")
    n_rows, n_cols = c.take("<2H", "N_ROWS / N_COLS")
    blocks, nbytes = [], None
    for k in range(n_rows * n_cols):
        where = f"block ({k // n_cols}, {k % n_cols})"
        h, w, d, nb, nch = c.take("<5I", f"{where}: HEIGHT / WIDTH / DEPTH / N_BLOCKS / N_CHANS")
        if nch != 1:
            raise ValueError(f"mdata.bin: {where}: N_CHANS is {nch}: single-channel trees are read")
        abs_v, abs_h = c.take("<2i", f"{where}: ABS_V / ABS_H")
        dirname = c.name(f"{where}: DIR_NAME")
        files, depths, abs_d = [], [], []
        for q in range(nb):
            files.append(c.name(f"{where}: FILENAMES[{q}]"))
            size, a = c.take("<Ii", f"{where}: BLOCK_SIZE / BLOCK_ABS_D[{q}]")
            depths.append(size)
            abs_d.append(a)
        nby, = c.take("<I", f"{where}: N_BYTESxCHAN")
        if nbytes is not None and nby != nbytes:
            raise ValueError(f"mdata.bin: {where}: N_BYTESxCHAN is {nby}, the block before has {nbytes}")
        nbytes = nby
        blocks.append({"dir": dirname, "height": h, "width": w, "depth": d, "abs_v": abs_v, "abs_h": abs_h, "files": files, "depths": depths,
                       "abs_d": abs_d, "n_chans": nch})
    if not blocks:
        raise ValueError("mdata.bin: N_ROWS x N_COLS is 0: no block")
    return {"version": version, "reference_system": tuple(ref), "voxel_123": tuple(v123), "voxel": tuple(vox), "origin": tuple(org),
            "extents": tuple(dim), "n_rows": n_rows, "n_cols": n_cols, "blocks": blocks, "bytes_per_channel": nbytes}


class TreeLevel:
    """One ``RES(VxHxD)`` directory.  ``shape`` (D, V, H) is what exists: D is the number of pages of the block files, which is less
    than ``mdata.bin`` and the directory name say wherever the conversion dropped a group's odd last slice (the module text above;
    ``nominal_depth`` is what they say).  ``voxel`` and ``origin`` are in the same (D, V, H) order."""

    def __init__(self, path, md, pages):
        self.path, self.mdata, self.name = Path(path), md, Path(path).name
        self.pages = list(pages)                              # pages of the k-th file along D
        self.z_start = [0]
        for n in self.pages:
            self.z_start.append(self.z_start[-1] + n)
        self.nominal_depth = int(md["extents"][2])
        self.shape = (self.z_start[-1], int(md["extents"][0]), int(md["extents"][1]))
        self.voxel = (md["voxel"][2], md["voxel"][0], md["voxel"][1])
        self.origin = (md["origin"][2], md["origin"][0], md["origin"][1])


def tiff3d_info(path):
    """``mi_tiff3d_info``: {nx, ny, pages, bytes, compression, rows_per_strip, bigtiff} of a block file (MiError for a file the
    readers refuse)."""
    from . import capi
    v = [C.c_int() for _ in range(7)]
    capi.check(capi.lib().mi_tiff3d_info(os.fsencode(str(path)), *[C.byref(x) for x in v]))
    return dict(zip(("nx", "ny", "pages", "bytes", "compression", "rows_per_strip", "bigtiff"), (int(x.value) for x in v)))


class TeraFlyTree:
    """A TeraFly tree opened for reading (``open_tree``): ``levels`` (largest first), ``dtype``, ``imread`` and ``imread_device``."""

    def __init__(self, root):
        self.root = Path(root)
        found = []
        for d in sorted(self.root.iterdir()) if self.root.is_dir() else []:
            if d.is_dir() and d.name.startswith("RES(") and (d / "mdata.bin").is_file():
                md = parse_mdata((d / "mdata.bin").read_bytes())
                missing = [str(d / b["dir"] / f) for b in md["blocks"] for f in b["files"] if not (d / b["dir"] / f).is_file()]
                if missing:
                    raise ValueError(f"{missing[0]}: named by {d / 'mdata.bin'} and not there ({len(missing)} of the level's block files are "
                                     "missing; sparse trees are not read)")
                first = md["blocks"][0]
                infos = [tiff3d_info(d / first["dir"] / f) for f in first["files"]]
                if any(i["bytes"] != md["bytes_per_channel"] for i in infos):
                    raise ValueError(f"{d / first['dir'] / first['files'][0]}: samples of {infos[0]['bytes']} bytes, {d / 'mdata.bin'} says "
                                     f"{md['bytes_per_channel']}")
                found.append(TreeLevel(d, md, [i["pages"] for i in infos]))
        if not found:
            raise ValueError(f"{root}: no RES(VxHxD) directory with an mdata.bin")
        self.levels = sorted(found, key=lambda lv: -lv.shape[1] * lv.shape[2])
        nb = {lv.mdata["bytes_per_channel"] for lv in self.levels}
        if len(nb) != 1 or nb.pop() not in (1, 2):
            raise ValueError(f"{root}: levels of {sorted(lv.mdata['bytes_per_channel'] for lv in self.levels)} bytes per sample (1 or 2, all equal)")
        self.dtype = np.dtype({1: np.uint8, 2: np.uint16}[self.levels[0].mdata["bytes_per_channel"]])

    def _jobs(self, box, level):
        from . import capi
        if not 0 <= int(level) < len(self.levels):
            raise ValueError(f"level {level}: the tree has levels 0..{len(self.levels) - 1}")
        lv = self.levels[int(level)]
        if hasattr(box, "z0"):   # ipp_amd.tsv.VExtent
            box = (box.z0, box.z1, box.y0, box.y1, box.x0, box.x1)
        z0, z1, y0, y1, x0, x1 = (int(v) for v in box)
        D, V, H = lv.shape
        if not (0 <= z0 < z1 <= D and 0 <= y0 < y1 <= V and 0 <= x0 < x1 <= H):
            raise ValueError(f"box [{z0}, {z1}) x [{y0}, {y1}) x [{x0}, {x1}) outside level {level} of {D} x {V} x {H} (z, y, x)")
        jobs = []
        for b in lv.mdata["blocks"]:
            r0, c0 = b["abs_v"], b["abs_h"]
            ya, yb, xa, xb = max(y0, r0), min(y1, r0 + b["height"]), max(x0, c0), min(x1, c0 + b["width"])
            if ya >= yb or xa >= xb:
                continue
            for k, f in enumerate(b["files"]):
                za, zb = max(z0, lv.z_start[k]), min(z1, lv.z_start[k + 1])
                if za < zb:
                    jobs.append((os.fsencode(str(lv.path / b["dir"] / f)), za - lv.z_start[k], zb - lv.z_start[k], ya - r0, yb - r0, xa - c0,
                                 xb - c0, za - z0, ya - y0, xa - x0))
        arr = (capi.Tiff3dJob * len(jobs))(*[capi.Tiff3dJob(*j) for j in jobs])
        return arr, len(jobs), (z1 - z0, y1 - y0, x1 - x0)

    def imread(self, box, level=0, out=None, threads=0):
        """The voxels of ``box`` = (z0, z1, y0, y1, x0, x1) (half-open, in the level's own voxels; or an ``ipp_amd.tsv.VExtent``) as a
        numpy ``[z, y, x]`` array; only the strips the box touches are read and decoded (``mi_tiff3d_read_box``)."""
        from . import capi
        jobs, n, shape = self._jobs(box, level)
        if out is None:
            out = np.empty(shape, self.dtype)
        if not (isinstance(out, np.ndarray) and out.shape == shape and out.dtype == self.dtype and out.flags.c_contiguous):
            raise ValueError(f"imread: out must be a C-contiguous {self.dtype} array of shape {shape}")
        capi.check(capi.lib().mi_tiff3d_read_box(jobs, n, shape[0], shape[1], shape[2], self.dtype.itemsize, out.ctypes.data, int(threads)))
        return out

    def imread_device(self, box, level=0, device=None, route=None, threads=0):
        """``imread`` with the box as a device tensor, ordered on torch's current stream.  ``route="device"``: the strips cross as
        they are in the files and are decoded on the device (``mi_tiff3d_read_box_device``); ``route="host"``: decoded on the host
        threads and uploaded.  ``route=None`` takes the measured default, the device route (1.8 to 2.8 times the
        host route on noise, smooth and sparse trees), unless ``MI_TERAFLY_READ_DEVICE=0`` is set (read per call)."""
        import torch
        from . import capi
        capi.require_gpu()
        if route is None:
            route = "host" if os.environ.get("MI_TERAFLY_READ_DEVICE") == "0" else "device"
        if route not in ("host", "device"):
            raise ValueError(f"route={route!r}: 'host' or 'device'")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if route == "host":
            return torch.from_numpy(self.imread(box, level, threads=threads)).to(dev, non_blocking=False)
        jobs, n, shape = self._jobs(box, level)
        out = torch.empty(shape, dtype={1: torch.uint8, 2: torch.uint16}[self.dtype.itemsize], device=dev)
        with torch.cuda.device(dev):
            capi.check(capi.lib().mi_tiff3d_read_box_device(dev.index, capi.current_stream_ptr(dev), jobs, n, shape[0], shape[1], shape[2],
                                                            self.dtype.itemsize, out.data_ptr(), int(threads)))
        return out


def open_tree(root) -> TeraFlyTree:
    """Opens the TeraFly tree under ``root`` (what ``convert`` or the reference's teraconverter wrote) for reading."""
    return TeraFlyTree(root)
