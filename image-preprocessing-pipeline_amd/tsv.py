#!/usr/bin/env python3
"""tsv/volume.py on the MI355X: the TSVVolume of a TeraStitcher project, the pipeline's live tile merge.

    from ipp_amd.tsv import TSVVolume, VExtent
    volume = TSVVolume("xml_import.xml", alt_stack_dir=None, cosine_blending=True)
    planes = volume.imread_device(VExtent(x0, x1, y0, y1, z0, z1))     # device tensor [z, y, x]
    planes = volume.imread(volume.volume, volume.dtype)                # numpy, as the reference's

    python tsv.py --projin XML --output DIR [--alt_stack_dir D --cosine_blending --ignore_z_offsets --z0 a --z1 b]

What is kept of the reference (tsv/volume.py):

* placement (make_stacks, :730-797): stack (0,0) at the origin, a stack of row 0 at its west neighbour's offset minus the FIRST
  WEST_displacements entry's H / V / D ``displ``, every other stack at its north neighbour's minus the first NORTH_displacements
  entry; D dropped with ``ignore_z_offsets``; all offsets rebased to minima of 0 (``mi_tsv_place``).  ABS_* take no part.
* a stack's x / y extent is its first slice's shape, its z count the number of indices in Z_RANGES (:334-352), its slices the
  files the ordering pattern ``[^0-9]*(\\d+).*\\.tiff?`` matches, filtered by IMG_REGEX, ordered by the extracted integer (:361-375).
* the volume is the union of the stacks (:671-682); voxels no stack covers are 0.
* ``cosine_blending=False``: the maximum over the covering stacks (:633-645), exact.  ``True``: the float16 blend (:592-631) in the
  reference's numpy branch (USE_NUMEXPR = False), every operation and the order of the sums kept (``mi_tsv_merge``).

Refused by name: ``input_plugin="raw"``, TSVSimpleVolume, make_diagnostic_img, samples other than uint8 / uint16, a ``dtype`` other
than the volume's own, stacks of different shapes, a missing slice (the reference writes dummy files, :378-398), and under cosine
blending two stacks on the same XY rectangle.  Departure: a float16 result that is inf / nan (a uint16 sample >= 65520 under
cosine blending) saturates to 65535; the reference's cast of it is undefined.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import sys
from pathlib import Path
from xml.etree import ElementTree

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = "ipp_amd"

from . import capi  # noqa: E402

ORDERING_PATTERN = "[^0-9]*(\\d+).*\\.tiff?"     # tsv/volume.py:355
_DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16))


def _refuse(name, value, why):
    raise NotImplementedError(f"{name}={value!r}: {why}")


class VExtent:
    """A volume extent in voxels, [x0, x1) x [y0, y1) x [z0, z1) (tsv/volume.py:65-197)."""

    def __init__(self, x0, x1, y0, y1, z0, z1):
        self.x0, self.x1, self.y0, self.y1, self.z0, self.z1 = (int(v) for v in (x0, x1, y0, y1, z0, z1))

    @property
    def shape(self):
        """voxels along z, y and x"""
        return self.z1 - self.z0, self.y1 - self.y0, self.x1 - self.x0

    def intersects(self, other):
        return (self.x0 < other.x1 and self.x1 > other.x0 and self.y0 < other.y1 and self.y1 > other.y0
                and self.z0 < other.z1 and self.z1 > other.z0)

    def intersection(self, other):
        return VExtent(max(self.x0, other.x0), min(self.x1, other.x1), max(self.y0, other.y0), min(self.y1, other.y1),
                       max(self.z0, other.z0), min(self.z1, other.z1))

    def contains(self, other):
        return (self.x0 <= other.x0 and self.x1 >= other.x1 and self.y0 <= other.y0 and self.y1 >= other.y1
                and self.z0 <= other.z0 and self.z1 >= other.z1)

    def start(self, idx):
        return (self.z0, self.y0, self.x0)[idx]

    def end(self, idx):
        return (self.z1, self.y1, self.x1)[idx]

    def __eq__(self, other):
        return isinstance(other, VExtent) and all(getattr(self, k) == getattr(other, k) for k in ("x0", "x1", "y0", "y1", "z0", "z1"))

    __hash__ = None

    def __repr__(self):
        return f"VExtent(x0={self.x0}, x1={self.x1}, y0={self.y0}, y1={self.y1}, z0={self.z0}, z1={self.z1})"


class Location:
    """A stack's offset (tsv/volume.py:43-62); index 0 / 1 / 2 = z / y / x."""

    def __init__(self, x, y, z):
        self.x, self.y, self.z = int(x), int(y), int(z)

    def __getitem__(self, item):
        return (self.z, self.y, self.x)[item]

    def __eq__(self, other):
        return isinstance(other, Location) and (self.x, self.y, self.z) == (other.x, other.y, other.z)

    __hash__ = None

    def __repr__(self):
        return f"{{x={self.x:d}, y={self.y:d}, z={self.z:d}}}"


def parse_z_ranges(z_ranges):
    """Z_RANGES "[a,b);[c,d)" -> the indices into the sorted slice files, the ranges concatenated (tsv/volume.py:337-352,
    with its handling of "(a,b]": an open start adds 1, and the end adds 1 unless the WHOLE attribute ends with ")")."""
    idxs = []
    if len(z_ranges) == 0:
        return idxs
    for part in z_ranges.split(";"):
        a, b = (int(v) for v in part[1:-1].split(","))
        if not part.startswith("["):
            a += 1
        if not z_ranges.endswith(")"):
            b += 1
        idxs += list(range(a, b))
    return idxs


class TSVStack(VExtent):
    """One <Stack> element placed at ``offset`` (tsv/volume.py:304-400).  ``paths[k]`` is the file of the stack's plane k."""

    def __init__(self, element, offset, root_dir):
        self.row, self.column = int(element.attrib["ROW"]), int(element.attrib["COL"])
        self.n_chans = int(element.attrib["N_CHANS"])
        self.bytes_per_chan = int(element.attrib["N_BYTESxCHAN"])
        self.dir_name = element.attrib["DIR_NAME"]
        self.img_regex = element.attrib["IMG_REGEX"]
        self.root_dir = str(root_dir)
        self.idxs_to_keep = parse_z_ranges(element.attrib["Z_RANGES"])
        self.z0slice, self.z1slice = 0, len(self.idxs_to_keep)
        self._paths = None
        self.height = self.width = self.dtype = None
        super().__init__(offset.x, offset.x, offset.y, offset.y, offset.z, offset.z + self.z1slice)

    @property
    def directory(self):
        return os.path.join(self.root_dir, self.dir_name)

    @property
    def paths(self):
        if self._paths is None:
            directory = self.directory
            if not os.path.isdir(directory):
                raise ValueError(f"stack [{self.row},{self.column}]: no folder {directory}")
            found = []
            for filename in sorted(os.listdir(directory)):
                match = re.match(ORDERING_PATTERN, filename)
                if not match:
                    continue
                if self.img_regex != "" and not re.match(self.img_regex, filename):
                    continue
                found.append((int(match.groups()[0]), os.path.join(directory, filename)))
            found = [f[1] for f in sorted(found)]
            if self.idxs_to_keep and (max(self.idxs_to_keep) >= len(found) or min(self.idxs_to_keep) < 0):
                raise ValueError(f"stack [{self.row},{self.column}]: Z_RANGES asks for slice {max(self.idxs_to_keep)} and {directory} holds "
                                 f"{len(found)} slices; missing slices are not replaced by dummy files here")
            self._paths = [found[i] for i in self.idxs_to_keep]
        return self._paths

    def set_size(self, width, height, dtype):
        self.height, self.width, self.dtype = int(height), int(width), np.dtype(dtype)
        self.x1, self.y1 = self.x0 + self.width, self.y0 + self.height

    def read_plane(self, k):
        from .pystripe import imread_tif_raw_png
        img = imread_tif_raw_png(Path(self.paths[k]))
        if img is None:
            raise ValueError(f"stack [{self.row},{self.column}]: {self.paths[k]} cannot be read")
        if self.height is not None and (img.shape != (self.height, self.width) or img.dtype != self.dtype):
            raise ValueError(f"stack [{self.row},{self.column}]: {self.paths[k]} holds {img.dtype} {img.shape}, the stacks "
                             f"{self.dtype} {(self.height, self.width)}")
        return img

    def read_planes(self, k0, k1):
        """planes [k0, k1) of the stack as one [k1 - k0, height, width] array"""
        out = np.empty((k1 - k0, self.height, self.width), self.dtype)
        for k in range(k0, k1):
            out[k - k0] = self.read_plane(k)
        return out

    def read_planes_device(self, k0, k1, dev):
        """``read_planes`` as a device tensor.  With ``MI_TIFF_READ_DEVICE=1`` in the environment (read per call) and files the
        native TIFF reader decodes, the strips are inflated on the device (``brickio.read_tiff_box_device``); else the planes are
        read on the host and uploaded.  Only the first file of the range is probed: with the switch on, a later plane that the
        native reader does not decode, or of another shape or type, raises the device reader's ``capi.MiError`` where
        ``read_plane`` would have read it through the general reader or raised its ``ValueError``."""
        import torch
        if os.environ.get("MI_TIFF_READ_DEVICE") == "1" and k1 > k0:
            from . import brickio
            files = self.paths[k0:k1]
            info = brickio.tiff_info(files[0])
            if info is not None and info[2] and info[0] == (self.height, self.width) and np.dtype(info[1]) == self.dtype:
                return brickio.read_tiff_box_device(files, (self.height, self.width), self.dtype, 0, self.height, 0, self.width, device=dev)
        return torch.from_numpy(self.read_planes(k0, k1)).to(dev)


class TSVSimpleVolume:
    """tsv/volume.py:810-860 (a volume from a directory parse): not built."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("TSVSimpleVolume: a volume from a directory parse is not built (TSVVolume on a project XML is)")


class TSVVolume:
    """tsv.volume.TSVVolume (tsv/volume.py:685-807) with ``imread`` on the GPU.  ``device``: where ``imread_device`` works (default:
    torch's current device)."""

    def __init__(self, tree_xml_path, ignore_z_offsets=False, alt_stack_dir=None, cosine_blending=False, device=None):
        root = ElementTree.parse(str(tree_xml_path)).getroot()
        if root.tag != "TeraStitcher":
            raise ValueError(f"tree_xml_path={str(tree_xml_path)!r}: the root element is <{root.tag}>, not <TeraStitcher>")
        self.input_plugin = root.attrib["input_plugin"]
        if self.input_plugin == "raw":
            _refuse("input_plugin", "raw", "stacks of .raw slices are not built (tiff2D is)")
        self.volume_format = root.attrib["volume_format"]
        dims = root.find("dimensions")
        self.stack_rows, self.stack_columns = int(dims.attrib["stack_rows"]), int(dims.attrib["stack_columns"])
        self.stack_slices = int(dims.attrib["stack_slices"])
        self.voxel_dims = tuple(float(root.find("voxel_dims").attrib[k]) for k in "DVH")   # z, y, x
        self.origin = tuple(float(root.find("origin").attrib[k]) for k in "DVH")
        self.stacks_dir = root.find("stacks_dir").attrib["value"] if alt_stack_dir is None else str(alt_stack_dir)
        md = root.find("mechanical_displacements")
        self.mechanical_displacement_x, self.mechanical_displacement_y = float(md.attrib["H"]), float(md.attrib["V"])
        self.ignore_z_offsets, self.cosine_blending, self.device = bool(ignore_z_offsets), bool(cosine_blending), device
        self._make_stacks(root)

    def _make_stacks(self, root):
        R, Cc = self.stack_rows, self.stack_columns
        elements = [[None] * Cc for _ in range(R)]
        for child in root.find("STACKS").iter(tag="Stack"):
            elements[int(child.attrib["ROW"])][int(child.attrib["COL"])] = child
        north, west = np.zeros((R * Cc, 3), np.int32), np.zeros((R * Cc, 3), np.int32)
        nz = np.zeros(R * Cc, np.int32)
        for r in range(R):
            for c in range(Cc):
                child = elements[r][c]
                if child is None:
                    raise ValueError(f"the project has no <Stack> at ROW {r}, COL {c}")
                nz[r * Cc + c] = len(parse_z_ranges(child.attrib["Z_RANGES"]))
                if r == 0 and c == 0:
                    continue
                # the FIRST entry of the list (tsv/volume.py:752, :763), whatever else the list holds
                name, into = ("NORTH_displacements", north) if r > 0 else ("WEST_displacements", west)
                entries = list(child.find(name))
                if not entries:
                    raise ValueError(f"stack [{r},{c}] has no {name} entry: the project is not aligned (steps 2-4)")
                into[r * Cc + c] = [int(entries[0].find(k).attrib["displ"]) for k in "HVD"]
        if nz.min() < 1:
            s = int(np.argmin(nz))
            raise ValueError(f"stack [{s // Cc},{s % Cc}] has an empty Z_RANGES: every stack must hold slices")
        # x / y of every stack from its first slice; one shape and one sample type
        first = TSVStack(elements[0][0], Location(0, 0, 0), self.stacks_dir).read_plane(0)
        if first.ndim != 2 or first.dtype not in _DTYPES:
            _refuse("dtype", f"{first.dtype} {first.shape}", "2-D uint8 and uint16 slices are built")
        self._dtype = first.dtype
        height, width = first.shape
        x0, y0, z0 = (np.zeros(R * Cc, np.int32) for _ in range(3))
        extent = (C.c_int * 6)()
        ip = C.POINTER(C.c_int)
        capi.check(capi.lib().mi_tsv_place(R, Cc, north.ctypes.data_as(ip), west.ctypes.data_as(ip), int(self.ignore_z_offsets),
                                           nz.ctypes.data_as(ip), height, width, x0.ctypes.data_as(ip), y0.ctypes.data_as(ip),
                                           z0.ctypes.data_as(ip), extent))
        self._extent = VExtent(*extent)
        self.offsets = [[Location(x0[r * Cc + c], y0[r * Cc + c], z0[r * Cc + c]) for c in range(Cc)] for r in range(R)]
        self.stacks = [[TSVStack(elements[r][c], self.offsets[r][c], self.stacks_dir) for c in range(Cc)] for r in range(R)]
        for stack in self.flattened_stacks():
            stack.set_size(width, height, self._dtype)
            stack.read_plane(0)   # refuses another shape or sample type
            if stack.bytes_per_chan != self._dtype.itemsize:
                raise ValueError(f"stack [{stack.row},{stack.column}]: N_BYTESxCHAN={stack.bytes_per_chan} and {self._dtype} slices")
        if self.cosine_blending:
            seen = {}
            for stack in self.flattened_stacks():
                other = seen.setdefault((stack.x0, stack.y0), stack)
                if other is not stack:
                    raise ValueError(f"cosine_blending=True: stacks [{other.row},{other.column}] and [{stack.row},{stack.column}] lie on the "
                                     "same XY rectangle; the reference's weights then depend on the requested box and are not built")
        self._x0, self._y0, self._z0, self._nz = x0, y0, z0, nz

    def flattened_stacks(self):
        """the stacks in row-major order: the order of the blend"""
        return sum(self.stacks, [])

    @property
    def dtype(self):
        return self._dtype.type

    @property
    def volume(self):
        """the union of the stacks (tsv/volume.py:671-682)"""
        return self._extent

    def make_diagnostic_img(self, volume):
        raise NotImplementedError("make_diagnostic_img: the diagnostic image with one channel per stack is not built")

    def _device(self):
        import torch
        capi.require_gpu()
        if self.device is not None:
            return torch.device(self.device)
        return torch.device("cuda", torch.cuda.current_device())

    def imread_device(self, volume):
        """``imread(volume, self.dtype)`` as a device tensor [z, y, x]: the planes of every stack that meets the box go to the device
        as they are in the files and ``mi_tsv_merge`` makes the box in one launch."""
        import torch
        dev = self._device()
        tdtype = torch.uint8 if self._dtype.itemsize == 1 else torch.uint16
        shape = tuple(max(int(v), 0) for v in volume.shape)
        out = torch.empty(shape, dtype=tdtype, device=dev)
        if min(shape) == 0:
            return out
        stacks = self.flattened_stacks()
        held, ptrs = [], (C.c_void_p * len(stacks))()
        for k, stack in enumerate(stacks):
            if not stack.intersects(volume):
                continue
            zlo, zhi = max(stack.z0, volume.z0), min(stack.z1, volume.z1)
            planes = stack.read_planes_device(zlo - stack.z0, zhi - stack.z0, dev)
            held.append(planes)
            ptrs[k] = planes.data_ptr()
        merge_device(dev, self._x0, self._y0, self._z0, self._nz, stacks[0].height, stacks[0].width, ptrs, self._dtype.itemsize,
                     self.cosine_blending, volume, out)
        del held   # stream-ordered: torch keeps the blocks until the launch on this stream is past them
        return out

    def imread(self, volume, dtype):
        """The box as a numpy array of ``volume.shape`` (tsv/volume.py:575-647).  ``dtype`` must be the volume's own."""
        if np.dtype(dtype) != self._dtype:
            _refuse("dtype", np.dtype(dtype).name, f"only the volume's own sample type ({self._dtype.name}) is built")
        return self.imread_device(volume).cpu().numpy()


def merge_device(dev, x0, y0, z0, nz, height, width, ptrs, itemsize, cosine, box, out):
    """``mi_tsv_merge`` on torch's current stream of ``dev``; x0 / y0 / z0 / nz: int32 arrays, ptrs: c_void_p array."""
    import torch
    ip = C.POINTER(C.c_int)
    arr = [np.ascontiguousarray(a, dtype=np.int32) for a in (x0, y0, z0, nz)]
    try:
        with torch.cuda.device(dev):
            capi.check(capi.lib().mi_tsv_merge(dev.index or 0, capi.current_stream_ptr(dev), len(arr[0]), *[a.ctypes.data_as(ip) for a in arr],
                                               int(height), int(width), ptrs, int(itemsize), int(bool(cosine)), box.x0, box.x1, box.y0, box.y1,
                                               box.z0, box.z1, out.data_ptr()))
    except capi.MiError as e:
        if e.code == capi.MI_ERR_INVALID:
            raise ValueError(str(e)) from None
        raise


# ---------------------------------------------------------------------------------------------------------------------------------
# command line: the merged 2-D series

def _slab_depth(volume, depth, device):
    """Output planes per slab: every stack's planes plus the merged ones must fit in half the free device memory."""
    import torch
    free, _ = torch.cuda.mem_get_info(device)
    stack = volume.stacks[0][0]
    per_plane = np.dtype(volume.dtype).itemsize * (volume.stack_rows * volume.stack_columns * stack.height * stack.width
                                                   + volume.volume.shape[1] * volume.volume.shape[2])
    return max(1, min(depth, int(free // 2 // max(per_plane, 1))))


def write_series(volume, output, z0=None, z1=None, slab=None, tif_prefix="img"):
    """Planes [z0, z1) of ``volume`` as ``<output>/<tif_prefix>_<z:06>.tif`` through the device TIFF writer, in z slabs sized by the
    free device memory.  Returns the number of files written."""
    import torch
    ext = volume.volume
    z0 = ext.z0 if z0 is None else max(int(z0), ext.z0)
    z1 = ext.z1 if z1 is None else min(int(z1), ext.z1)
    if z0 >= z1:
        raise ValueError(f"empty z range [{z0},{z1}) of a volume of planes [{ext.z0},{ext.z1})")
    output = Path(output)
    output.mkdir(parents=True, exist_ok=True)
    dev = volume._device()
    step = slab or _slab_depth(volume, z1 - z0, dev)
    _, ny, nx = ext.shape
    written = 0
    for a in range(z0, z1, step):
        b = min(z1, a + step)
        planes = volume.imread_device(VExtent(ext.x0, ext.x1, ext.y0, ext.y1, a, b))
        paths = (C.c_char_p * (b - a))(*[os.fsencode(str(output / f"{tif_prefix}_{z:06}.tif")) for z in range(a, b)])
        made = C.c_int(0)
        with torch.cuda.device(dev):
            capi.check(capi.lib().mi_tiff_write_series_device(dev.index or 0, capi.current_stream_ptr(dev), paths, b - a, planes.data_ptr(),
                                                              np.dtype(volume.dtype).itemsize, nx, ny, 0, C.byref(made)))
        written += int(made.value)
    return written


def _parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="tsv.py", allow_abbrev=False, description="the merged 2-D series of a TeraStitcher project on the GPU")
    p.add_argument("--projin", required=True, help="project XML with displacements (steps 2-4)")
    p.add_argument("--output", required=True, help="folder of the merged slices img_<z>.tif")
    p.add_argument("--alt_stack_dir", default=None, help="stacks folder of another channel")
    p.add_argument("--cosine_blending", action="store_true")
    p.add_argument("--ignore_z_offsets", action="store_true")
    p.add_argument("--z0", type=int, default=None)
    p.add_argument("--z1", type=int, default=None)
    return p.parse_args(argv)


def main(argv=None):
    a = _parse_args(argv)
    volume = TSVVolume(a.projin, ignore_z_offsets=a.ignore_z_offsets, alt_stack_dir=a.alt_stack_dir, cosine_blending=a.cosine_blending)
    n = write_series(volume, a.output, a.z0, a.z1)
    print(f"tsv: {n} slices of {volume.volume.shape[1]} x {volume.volume.shape[2]} in {a.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
