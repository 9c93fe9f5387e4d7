"""Stitching step 6 (``terastitcher -6`` at resolution 0): the placed stacks of a project merged into a TiledXY|2Dseries tree.

    merge_tiles(project, volout, slice_height, slice_width, D0, D1, blending, device)

The output is walked in z-slabs sized by the free device memory.  For every slab each stack's slices go to the device (shifted by
its ABS_D, the integer samples as they are in the files), ``mi_merge_slab`` (include/mi_stitch.h) merges each output tile of the
slab straight into its own buffer, and the device TIFF writer (``mi_tiff_write_series_device``) deflates and writes its slices.

The layout is VolumeConverter::generateTiles' (VolumeConverter.cpp:568-1000) with the default tiling (as uniform as possible):

    <volout>/RES(<V>x<H>x<D>)/<V0>/<V0>_<H0>/<V0>_<H0>_<D>.tif

with every position in 0.1 um, six digits (getMultiresABS_V / _H / _D, VolumeConverter.cpp:2568-2605; the absolute position of a
pixel is iim::round(ORG * 1000 + pixel * VXL) in float, VirtualVolume.h:176-178).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np

TMITREE_MIN_BLOCK_DIM = 250      # IM_config.h:151: VolumeConverter refuses smaller slices
BLENDINGS = {"SINBLEND": 0, "NOBLEND": 1}


def _iim_round(x):
    x = np.float32(x)
    return int(x + np.float32(0.5)) if x > 0 else int(x - np.float32(0.5))


def _abs_pos(org, vxl, offs, pixel):
    """VirtualVolume::getABS_V/H/D (VirtualVolume.h:176-178) of the UnstitchedVolume: round(ORG * 1000 + pixel * VXL) with its origin
    moved to the stitched volume's first voxel, ORG += offs * VXL / 1000.0f (UnstitchedVolume.cpp:207-209); float arithmetic."""
    f = np.float32
    org = f(f(org) + f(f(f(offs) * f(vxl)) / f(1000.0)))
    return _iim_round(f(f(org * f(1000)) + f(f(pixel) * f(vxl))))


def _name6(v):
    """std::stringstream with width(6) and fill('0'): a negative position is padded in front of its sign ("000-10")."""
    return str(int(v)).rjust(6, "0")


def _tile_sizes(total, size):
    """VolumeConverter::generateTiles without --fixed_tiling: ceil(total / size) tiles as uniform as possible."""
    n = int(math.ceil(total / np.float32(size)))
    return [total // n + (1 if k < total % n else 0) for k in range(n)]


@dataclass
class Geometry:
    """The grid's placement and the stitched volume (mi_merge_volume_dims)."""
    n_rows: int
    n_cols: int
    abs_v: np.ndarray
    abs_h: np.ndarray
    abs_d: np.ndarray
    height: int
    width: int
    n_slices: int
    dims: tuple    # v0, v1, h0, h1, d0, d1 in the stacks' frame

    @property
    def offsets(self):
        """The stitched volume's first voxel (V, H, D) in the stacks' frame."""
        return self.dims[0], self.dims[2], self.dims[4]

    @property
    def shape(self):
        v0, v1, h0, h1, d0, d1 = self.dims
        return d1 - d0, v1 - v0, h1 - h0


def geometry(project) -> Geometry:
    from . import capi
    R, Cc = project.N_ROWS, project.N_COLS
    get = lambda k: np.array([[getattr(project.STACKS[r][c], k) for c in range(Cc)] for r in range(R)], dtype=np.int32)
    av, ah, ad = get("ABS_V"), get("ABS_H"), get("ABS_D")
    Hs, Ws, N = project.getStacksHeight(), project.getStacksWidth(), project.N_SLICES
    dims = (C.c_int * 6)()
    ip = C.POINTER(C.c_int)
    capi.check(capi.lib().mi_merge_volume_dims(R, Cc, av.ctypes.data_as(ip), ah.ctypes.data_as(ip), ad.ctypes.data_as(ip), Hs, Ws, N,
                                               dims))
    return Geometry(R, Cc, av, ah, ad, Hs, Ws, N, tuple(int(v) for v in dims))


def output_layout(project, shape, slice_height, slice_width, D0=0, offs=(0, 0, 0)):
    """(RES directory name, [(row start, rows, V name)], [(col start, cols, H name)], slice name of output slice k) of a volume of
    ``shape`` = (D, V, H) output slices, the first of which is slice D0 of the stitched volume; ``offs`` = the stitched volume's
    first voxel (V, H, D) in the stacks' frame (Geometry.offsets)."""
    D, V, H = shape
    res = f"RES({V}x{H}x{D})"
    rows, cols = [], []
    start = 0
    for n in _tile_sizes(V, slice_height):
        rows.append((start, n, _name6(_abs_pos(project.ORG_V, project.VXL_V, offs[0], start) * 10)))
        start += n
    start = 0
    for n in _tile_sizes(H, slice_width):
        cols.append((start, n, _name6(_abs_pos(project.ORG_H, project.VXL_H, offs[1], start) * 10)))
        start += n
    d_base = _abs_pos(project.ORG_D, project.VXL_D, offs[2], D0) * 10

    def d_name(k):
        return _name6(int(np.float32(d_base) + np.float32(np.float32(k) * np.float32(project.VXL_D)) * np.float32(10)))
    return res, rows, cols, d_name


def output_files(project, shape, slice_height, slice_width, D0=0, offs=(0, 0, 0)):
    """Every file name (relative to volout) of the tree, sorted: what the reference's -6 writes."""
    res, rows, cols, d_name = output_layout(project, shape, slice_height, slice_width, D0, offs)
    names = []
    for _, _, vn in rows:
        for _, _, hn in cols:
            names += [f"{res}/{vn}/{vn}_{hn}/{vn}_{hn}_{d_name(k)}.tif" for k in range(shape[0])]
    return sorted(names)


def check_slice_dims(slice_height, slice_width):
    if slice_height < TMITREE_MIN_BLOCK_DIM or slice_width < TMITREE_MIN_BLOCK_DIM:
        raise ValueError(f"slices of {slice_height} x {slice_width}: at least {TMITREE_MIN_BLOCK_DIM} x {TMITREE_MIN_BLOCK_DIM} "
                         "(TMITREE_MIN_BLOCK_DIM, as VolumeConverter::generateTiles)")


def merge_slab(geo: Geometry, stacks, dtype, blending, D0, D1, V0, V1, H0, H1, out):
    """``mi_merge_slab`` on device tensors: ``stacks[r][c]`` hold output slices [D0, D1) of each stack, ``out`` is the
    (D1-D0, V1-V0, H1-H0) output box (same integer type)."""
    from . import capi
    ip = C.POINTER(C.c_int)
    ptrs = (C.c_void_p * (geo.n_rows * geo.n_cols))(*[stacks[r][c].data_ptr() for r in range(geo.n_rows) for c in range(geo.n_cols)])
    capi.check(capi.lib().mi_merge_slab(out.device.index, capi.current_stream_ptr(out.device), geo.n_rows, geo.n_cols,
                                        geo.abs_v.ctypes.data_as(ip), geo.abs_h.ctypes.data_as(ip), geo.abs_d.ctypes.data_as(ip),
                                        geo.height, geo.width, geo.n_slices, ptrs, np.dtype(dtype).itemsize, int(blending),
                                        D0, D1, V0, V1, H0, H1, out.data_ptr()))


def _check_stacks(project, geo):
    for row in project.STACKS:
        for s in row:
            if len(s.z_ranges) != 1 or s.z_ranges[0] != (0, project.N_SLICES):
                raise ValueError(f"stack [{s.ROW_INDEX},{s.COL_INDEX}] ({s.DIR_NAME}) has Z_RANGES "
                                 f"{';'.join('[%d,%d)' % r for r in s.z_ranges)}: the merge takes complete stacks only "
                                 f"([0,{project.N_SLICES})); sparse stacks are not merged")


def _slab_depth(geo, bytes_per_sample, device, n_slices, slice_height, slice_width):
    """Output slices per slab: the stacks' slices plus one output tile's box must fit in half the free device memory."""
    import torch
    free, _ = torch.cuda.mem_get_info(device)
    per_slice = bytes_per_sample * (geo.n_rows * geo.n_cols * geo.height * geo.width + min(slice_height, geo.shape[1]) *
                                    min(slice_width, geo.shape[2]))
    return max(1, min(n_slices, int(free // 2 // max(per_slice, 1))))


def merge_tiles(project, volout, slice_height, slice_width, D0=None, D1=None, blending="SINBLEND", device=None, slab=None,
                out_D0=None, out_D1=None):
    """Writes the stitched volume of ``project`` (placed: ABS_V/H/D set by step 5) under ``volout``.  D0 / D1 select output slices
    of the stitched volume (as --D0 / --D1); out_D0 / out_D1 restrict which of those this call writes (a rank's share; the names
    and the RES() directory stay those of the whole [D0, D1) range).  Returns the number of files written."""
    import torch
    from . import capi
    capi.require_gpu()
    if blending not in BLENDINGS:
        raise ValueError(f"blending \"{blending}\": SINBLEND or NOBLEND")
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    geo = geometry(project)
    _check_stacks(project, geo)
    depth, V, H = geo.shape
    D0 = 0 if D0 is None or D0 < 0 else D0
    D1 = depth if D1 is None or D1 < 0 or D1 > depth else D1
    if D0 >= D1:
        raise ValueError(f"empty D range [{D0},{D1}) of a volume of {depth} slices")
    a = D0 if out_D0 is None else max(D0, out_D0)
    b = D1 if out_D1 is None else min(D1, out_D1)
    res, rows, cols, d_name = output_layout(project, (D1 - D0, V, H), slice_height, slice_width, D0, geo.offsets)
    base = Path(volout) / res
    for _, _, vn in rows:
        for _, _, hn in cols:
            (base / vn / f"{vn}_{hn}").mkdir(parents=True, exist_ok=True)
    if a >= b:
        return 0
    first = project._read_slices(project.STACKS[0][0], 0, 0)
    dtype = first.dtype
    tdtype = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16}[np.dtype(dtype)]
    step = slab or _slab_depth(geo, dtype.itemsize, dev, b - a, slice_height, slice_width)
    written = 0
    d0v = geo.dims[4]
    for z0 in range(a, b, step):
        z1 = min(b, z0 + step)
        stacks = []
        for r in range(geo.n_rows):
            row = []
            for c in range(geo.n_cols):
                s = project.STACKS[r][c]
                sz = z0 + d0v - s.ABS_D
                raw = project._read_slices(s, sz, sz + (z1 - z0) - 1)
                if raw.dtype != dtype:
                    raise ValueError(f"stack [{r},{c}]: {raw.dtype} samples, stack [0,0] has {dtype}")
                row.append(torch.from_numpy(np.ascontiguousarray(raw)).to(dev))
            stacks.append(row)
        for v0, nv, vn in rows:
            for h0, nh, hn in cols:
                out = torch.empty((z1 - z0, nv, nh), dtype=tdtype, device=dev)
                merge_slab(geo, stacks, dtype, BLENDINGS[blending], z0, z1, v0, v0 + nv, h0, h0 + nh, out)
                folder = base / vn / f"{vn}_{hn}"
                paths = (C.c_char_p * (z1 - z0))(*[os.fsencode(str(folder / f"{vn}_{hn}_{d_name(z - D0)}.tif")) for z in range(z0, z1)])
                made = C.c_int(0)
                capi.check(capi.lib().mi_tiff_write_series_device(dev.index, capi.current_stream_ptr(dev), paths, z1 - z0, out.data_ptr(),
                                                                  {1: 1, 2: 2}[dtype.itemsize], nh, nv, 0, C.byref(made)))
                written += int(made.value)
        del stacks
    return written
