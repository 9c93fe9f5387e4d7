"""parallel_image_processor.py on the MI355X: the per-slice pass of the pipeline (``fun`` on every slice of a folder, rotation, the
full-resolution TIFFs) and its isotropic down-sampled volume (the plane of every z group, ``<name>_zyx<target>um.npz``).

    python parallel_image_processor.py --input DIR|PROJECT.xml --output DIR --voxel_size Z Y X --voxel_size_target T
           [--downsampled_path DIR --rotation 0|90|180|270 --down_sampled_dtype float32|uint16|uint8 --no-alternating --rename]
           [--alt_stack_dir DIR --cosine_blending --ignore_z_offsets]      (with a project XML: the TSVVolume of ipp_amd.tsv)

The down-sampling runs on the device (include/mi_isodown.h): a slice is read there once by the halving kernel, which leaves a plane
some hundred times smaller; resize, z reduction and the final 3-D resize work on those.  When ``fun`` is
``ipp_amd.pystripe.process_img`` a whole z group goes through it as one device stack and stays on the device for rotation and
down-sampling; only the full-resolution result comes back, for writing.  Any other callable is called per slice on numpy arrays.
A ``source`` that is an ``ipp_amd.tsv.TSVVolume`` is merged on the device (``imread_device``, one call per z group with
``process_img``): the stitched planes never exist on the host or on disk before ``fun``.

Built to the restatement of DESIGN section 14 (scikit-image's resize / block_reduce / resize_local_mean written against scipy).
Not built, refused by name: Imaris (.ims) sources and any TSVVolume that is not ``ipp_amd.tsv.TSVVolume``.  ``timeout``, ``max_processors``, ``needed_memory`` and
``progress_bar_name`` are accepted and ignored.  Under ``torchrun`` every rank takes every WORLD_SIZE-th z group on its LOCAL_RANK
device; rank 0 waits for the planes of the others and builds the npz.  Departures from the reference: INTEGRATION section 4e.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import sys
import time
from pathlib import Path

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = "ipp_amd"

from . import capi, pystripe  # noqa: E402

SUPPORTED_EXTENSIONS = (".tif", ".tiff", ".raw", ".png")
_METHOD_NAMES = {capi.HALVE_MEAN: "mean", capi.HALVE_MAX: "max"}


# ---------------------------------------------------------------------------------------------------------------------------------
# host bookkeeping of the reference

def natural_sorted(names):
    """file names ordered with their digit runs compared as numbers (tifffile.natural_sorted)"""
    return sorted(names, key=lambda s: [int(c) if c.isdigit() else c for c in re.split(r"(\d+)", str(s))])


def scaled_voxel(source_shape, source_voxel, new_shape, is_rotated):
    """Voxel sizes (z, y, x) of a processed slice of ``new_shape``: a ``fun`` that changed the shape changed the y / x voxel sizes by
    source extent / new extent; for 90 / 270 the source's y pairs with the new x and the two sizes swap (:159-168)."""
    vz, vy, vx = (float(v) for v in source_voxel)
    if is_rotated:
        vy, vx = vx * (source_shape[1] / new_shape[0]), vy * (source_shape[0] / new_shape[1])
    else:
        vy, vx = vy * (source_shape[0] / new_shape[0]), vx * (source_shape[1] / new_shape[1])
    return vz, vy, vx


def derive(shape, voxel_yx, target_voxel, alternating=True):
    """The plan of one slice shape without a device (``mi_isodown_derive``) as a dict: target_shape, steps [(axis, method, extent
    before)], halved_shape, sigma, radius, taps, tile, scratch_bytes_per_slice.  ValueError when a target extent rounds to 0."""
    info = capi.IsodownInfo()
    try:
        capi.check(capi.lib().mi_isodown_derive(int(shape[0]), int(shape[1]), float(voxel_yx[0]), float(voxel_yx[1]), float(target_voxel),
                                                int(bool(alternating)), C.byref(info)))
    except capi.MiError as e:
        if e.code == capi.MI_ERR_INVALID:
            raise ValueError(str(e)) from None
        raise
    return info_dict(info)


def info_dict(info):
    return dict(target_shape=(info.target_ny, info.target_nx), rounds=(info.rounds_y, info.rounds_x),
                steps=[(info.step_axis[i], _METHOD_NAMES[info.step_method[i]], info.step_extent[i]) for i in range(info.nsteps)],
                halved_shape=(info.halved_ny, info.halved_nx), sigma=(info.sigma_y, info.sigma_x), radius=(info.radius_y, info.radius_x),
                taps=(info.taps_y, info.taps_x), tile=(info.tile_ny, info.tile_nx), lds_steps=info.lds_steps,
                scratch_bytes_per_slice=int(info.scratch_bytes_per_slice))


def z_steps(target_voxel, voxel_z):
    return max(1, math.floor(target_voxel / voxel_z))


def z_rounds(target_voxel, voxel_z):
    return math.ceil(math.sqrt(target_voxel / voxel_z))


def z_groups(count, steps):
    """Consecutive runs of ``steps`` slice indices.  The last group holds the slices that exist (the reference gives it one index past
    the end when count mod steps == steps - 1)."""
    return [list(range(i, min(i + steps, count))) for i in range(0, count, steps)]


def planes_left(n, rounds):
    for _ in range(rounds):
        if n > 1:
            n = (n + 1) // 2
    return n


def check_z_geometry(count, target_voxel, voxel_z):
    """ValueError for a geometry on which the reference's ``assert z_stack.shape[0] == 1`` stops (target / voxel_z == 9: 9 planes,
    3 rounds)."""
    steps, rounds = z_steps(target_voxel, voxel_z), z_rounds(target_voxel, voxel_z)
    for n in {len(g) for g in z_groups(count, steps)}:
        if planes_left(n, rounds) != 1:
            raise ValueError(f"target_voxel / voxel_z = {target_voxel / voxel_z:g}: {rounds} halving rounds along z leave "
                             f"{planes_left(n, rounds)} of the {n} planes of a group (the reference stops on this geometry)")


def volume_target_shape(count, shape, source_voxel, target_voxel, rotation=0):
    """Shape of the final volume: Python's round on the source slice shape, y / x swapped for 90 / 270 (:697-703)."""
    t = [int(round(count / (target_voxel / source_voxel[0]))), int(round(shape[0] / (target_voxel / source_voxel[1]))),
         int(round(shape[1] / (target_voxel / source_voxel[2])))]
    if rotation in (90, 270):
        t[1], t[2] = t[2], t[1]
    if min(t) < 1:
        raise ValueError(f"the down-sampled volume of {count} slices of {tuple(shape)} would have the shape {t}")
    return t


def local_mean_first(values, m):
    """Element 0 of skimage.transform.resize_local_mean(values, (m,)): the overlap-weighted mean of the inputs over [0, n / m)."""
    values = np.asarray(values, np.float64)
    n = len(values)
    j = np.arange(n, dtype=np.float64)
    weights = np.maximum(np.minimum(n / m, j + 1) - j, 0)
    weights /= weights.sum()
    return float((weights * values).sum())


def generate_voxel_spacing(shape, source_voxel, target_shape, target_voxel):
    """The three coordinate vectors saved as ``xI`` (:459-472), quirks included: callers pass the unrotated shape."""
    out = []
    for n, v, m in zip(shape, source_voxel, target_shape):
        locations = np.arange(n) * v - (n - 1) / 2.0 * v
        start = np.round(local_mean_first(locations, int(m)))
        out.append(np.array([start + target_voxel * k for k in range(int(m))], dtype=np.float64))
    return out


def downsampled_dir(downsampled_path, destination, steps, voxel_z, target_voxel):
    return Path(downsampled_path) / f"{Path(destination).stem}_z{steps * voxel_z:.1f}_yx{target_voxel:.1f}um"


def npz_path(downsampled_path, destination, target_voxel):
    return Path(downsampled_path) / f"{Path(destination).stem}_zyx{target_voxel:.1f}um.npz"


def tif_save_path(destination, images, idx, rename=False, tif_prefix="img"):
    """Full-resolution output of slice ``idx``: the source's name with .raw / .png becoming .tif, or ``{tif_prefix}_{idx:06}.tif``."""
    if rename:
        return Path(destination) / f"{tif_prefix}_{idx:06}.tif"
    file = Path(images[idx])
    if file.suffix.lower() in (".png", ".raw"):
        return Path(destination) / (file.name[0:-4] + ".tif")
    return Path(destination) / file.name


def _refuse_source(source):
    from .tsv import TSVVolume
    if isinstance(source, TSVVolume):
        return
    if type(source).__name__ == "TSVVolume":
        raise NotImplementedError("source=TSVVolume: a TSVVolume source is not built (a folder of 2-D slices is)")
    if isinstance(source, (str, Path)) and Path(source).suffix.lower() == ".ims":
        raise NotImplementedError(f"source={str(source)!r}: an Imaris (.ims) source is not built (a folder of 2-D slices is)")


# ---------------------------------------------------------------------------------------------------------------------------------
# device

def _np_dtype(t):
    return np.dtype(str(t.dtype).replace("torch.", ""))


def _layout(t):
    """the tensor with uint16 samples seen as int16: layout operations (stack, rot90) are not built for uint16 everywhere"""
    import torch
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _stack(tensors):
    import torch
    out = torch.stack([_layout(t) for t in tensors])
    return out.view(torch.uint16) if tensors[0].dtype == torch.uint16 else out


class Plan:
    """mi_isodown plan for processed slices of one shape and dtype.  ``run(stack)``: a dense [n, ny, nx] device tensor of one z group ->
    (plane tensor of ``out_dtype``, uniform flag tensor); ``planes(stack)`` -> [n, target_ny, target_nx] float32; ``halve(stack)`` ->
    (halved planes, per-slice differs flags)."""

    def __init__(self, device, shape, in_dtype, voxel_yx, target_voxel, alternating=True, z_rounds=0, out_dtype="float32", max_group=16):
        import torch
        capi.require_gpu()
        self.device = torch.device(device if device is not None else "cuda:0")
        self.shape, self.in_dtype, self.out_dtype = (int(shape[0]), int(shape[1])), np.dtype(in_dtype), np.dtype(out_dtype)
        p = capi.IsodownParams()
        p.voxel_y, p.voxel_x, p.target_voxel = float(voxel_yx[0]), float(voxel_yx[1]), float(target_voxel)
        p.alternating, p.z_rounds, p.max_group = int(bool(alternating)), int(z_rounds), int(max_group)
        p.out_dtype = pystripe._dtype_code(self.out_dtype, "down_sampled_dtype")
        self.params = p
        self._h = C.c_void_p()
        capi.check(capi.lib().mi_isodown_plan_create(self.device.index or 0, self.shape[0], self.shape[1], pystripe._dtype_code(self.in_dtype, "dtype"),
                                                     C.byref(p), C.byref(self._h)))
        info = capi.IsodownInfo()
        capi.check(capi.lib().mi_isodown_plan_info(self._h, C.byref(info)))
        self.info = info_dict(info)
        self.target_shape, self.halved_shape = self.info["target_shape"], self.info["halved_shape"]

    def _check(self, stack):
        import torch
        if not (isinstance(stack, torch.Tensor) and stack.is_cuda and stack.is_contiguous() and stack.dim() == 3
                and _np_dtype(stack) == self.in_dtype and tuple(stack.shape[1:]) == self.shape):
            raise ValueError(f"isodown plan: a contiguous [n, {self.shape[0]}, {self.shape[1]}] {self.in_dtype.name} device tensor is expected")
        return int(stack.shape[0])

    def halve(self, stack):
        import torch
        n = self._check(stack)
        halved = torch.empty((n,) + self.halved_shape, dtype=torch.float32, device=stack.device)
        differs = torch.empty((n,), dtype=torch.int32, device=stack.device)
        with torch.cuda.device(stack.device):
            capi.check(capi.lib().mi_isodown_halve(self._h, capi.current_stream_ptr(stack.device), stack.data_ptr(), n, halved.data_ptr(),
                                                   differs.data_ptr()))
        return halved, differs

    def planes(self, stack):
        import torch
        n = self._check(stack)
        out = torch.empty((n,) + self.target_shape, dtype=torch.float32, device=stack.device)
        with torch.cuda.device(stack.device):
            capi.check(capi.lib().mi_isodown_planes(self._h, capi.current_stream_ptr(stack.device), stack.data_ptr(), n, out.data_ptr()))
        return out

    def run(self, stack):
        import torch
        n = self._check(stack)
        plane = torch.empty(self.target_shape, dtype=getattr(torch, self.out_dtype.name), device=stack.device)
        uniform = torch.zeros((1,), dtype=torch.int32, device=stack.device)
        with torch.cuda.device(stack.device):
            capi.check(capi.lib().mi_isodown_run(self._h, capi.current_stream_ptr(stack.device), stack.data_ptr(), n, plane.data_ptr(),
                                                 uniform.data_ptr()))
        return plane, uniform

    def close(self):
        if self._h:
            capi.lib().mi_isodown_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reduce_z(stack, rounds, out_dtype="float32", processed_dtype=np.uint16):
    """The plane of one group from its float32 device stack [n, ny, nx] (which is overwritten) -> (plane tensor, uniform flag tensor)."""
    import torch
    out_dtype = np.dtype(out_dtype)
    if not (stack.is_cuda and stack.is_contiguous() and stack.dim() == 3 and stack.dtype == torch.float32):
        raise ValueError("reduce_z: a contiguous float32 [n, ny, nx] device tensor is expected")
    n, ny, nx = (int(v) for v in stack.shape)
    plane = torch.empty((ny, nx), dtype=getattr(torch, out_dtype.name), device=stack.device)
    uniform = torch.zeros((1,), dtype=torch.int32, device=stack.device)
    try:
        with torch.cuda.device(stack.device):
            capi.check(capi.lib().mi_isodown_reduce_z(stack.device.index or 0, capi.current_stream_ptr(stack.device), stack.data_ptr(), n, ny, nx,
                                                      int(rounds), int(np.dtype(processed_dtype) == np.uint8),
                                                      pystripe._dtype_code(out_dtype, "down_sampled_dtype"), plane.data_ptr(), uniform.data_ptr()))
    except capi.MiError as e:
        if e.code == capi.MI_ERR_INVALID:
            raise ValueError(str(e)) from None
        raise
    return plane, uniform


def resize_antialias(a, out_shape, device=None):
    """resize(a, out_shape, preserve_range=True, anti_aliasing=True) of a 2-D or 3-D float32 array on the device (numpy in, numpy out;
    a device tensor in, a device tensor out)."""
    import torch
    is_tensor = isinstance(a, torch.Tensor)
    if not is_tensor:
        capi.require_gpu()
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.device(device if device is not None else "cuda:0"))
    a = a.contiguous()
    if a.dtype != torch.float32 or a.dim() not in (2, 3) or len(out_shape) != a.dim():
        raise ValueError("resize_antialias: a 2-D or 3-D float32 array and an output shape of as many axes are expected")
    if min(int(v) for v in out_shape) < 1:
        raise ValueError(f"resize_antialias: output shape {tuple(out_shape)}")
    out = torch.empty(tuple(int(v) for v in out_shape), dtype=torch.float32, device=a.device)
    nd = a.dim()
    si, so = (C.c_int * nd)(*[int(v) for v in a.shape]), (C.c_int * nd)(*[int(v) for v in out_shape])
    with torch.cuda.device(a.device):
        capi.check(capi.lib().mi_resize_antialias(a.device.index or 0, capi.current_stream_ptr(a.device), a.data_ptr(), nd, si, so, out.data_ptr()))
    return out if is_tensor else out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# folder -> folder

def _call(fun, img, args, kwargs):
    if args is not None and kwargs is not None:
        return fun(img, *args, **kwargs)
    if args is not None:
        return fun(img, *args)
    if kwargs is not None:
        return fun(img, **kwargs)
    return fun(img)


def _device_kind(t):
    """(shape, dtype) of a slice that can go to the device as it is"""
    return tuple(int(v) for v in t.shape), _np_dtype(t)


def parallel_image_processor(source, destination, fun=None, args=None, kwargs=None, rename=False, tif_prefix="img", channel=0,
                             source_voxel=None, target_voxel=None, downsampled_path=None, down_sampled_dtype="float32",
                             alternating_downsampling_method=True, rotation=0, timeout=None, max_processors=None,
                             progress_bar_name=" ImgProc", compression=("ADOBE_DEFLATE", 1), resume=True, needed_memory=None,
                             save_images=True, return_downsampled_path=False):
    """parallel_image_processor.py:489 on the GPU, the reference's keywords and defaults.  Returns 0, or (0, down-sampled folder) with
    ``return_downsampled_path``."""
    import torch
    from .tsv import TSVVolume, VExtent
    _refuse_source(source)
    is_tsv = isinstance(source, TSVVolume)
    destination = Path(destination)
    if not is_tsv:
        source = Path(source)
        if not source.is_dir():
            raise RuntimeError("source can be either a tsv volume, an ims file path, or a 2D tiff series folder (the folder and the "
                               "tsv volume are built)")
    destination.mkdir(exist_ok=True)
    downsampled_path = destination if downsampled_path is None else Path(downsampled_path)
    out_dtype = np.dtype(down_sampled_dtype)
    if out_dtype not in (np.float32, np.uint16, np.uint8):
        raise RuntimeError(f"requested downsampled format is not supported: down_sampled_dtype={down_sampled_dtype!r}")

    if is_tsv:   # :578-590: the slices are the volume's planes, named {tif_prefix}_{idx:06}.tif (:194-199)
        images, rename = None, True
        whole = source.volume
        num_images = whole.shape[0]
        assert num_images > 0, "the TSVVolume holds no plane"
    else:
        images = natural_sorted([str(f) for f in source.iterdir() if f.is_file() and f.suffix.lower() in SUPPORTED_EXTENSIONS])
        num_images = len(images)
        assert num_images > 0, f"no .tif / .tiff / .raw / .png file in {source}"

    def read_planes(first, last):
        """planes [first, last] of the TSVVolume as one device stack (one merge launch)"""
        return source.imread_device(VExtent(whole.x0, whole.x1, whole.y0, whole.y1, whole.z0 + first, whole.z0 + last + 1))

    def read_source(idx):
        if is_tsv:
            return read_planes(idx, idx)[0].cpu().numpy()
        img = pystripe.imread_tif_raw_png(Path(images[idx]))
        if img is None:
            raise RuntimeError(f"cannot read {images[idx]}")
        if img.ndim == 3 and 0 <= channel < 3:
            img = img[:, :, channel]
        return img

    shape = tuple(whole.shape[1:3]) if is_tsv else tuple(read_source(0).shape)
    rotated = rotation in (90, 270)
    need_down_sampling = source_voxel is not None and target_voxel is not None
    steps, rounds, t3 = 1, 0, None
    if need_down_sampling:
        source_voxel = tuple(float(v) for v in source_voxel)
        steps, rounds = z_steps(target_voxel, source_voxel[0]), z_rounds(target_voxel, source_voxel[0])
        # everything the reference would fail on half-way is refused before any work
        check_z_geometry(num_images, target_voxel, source_voxel[0])
        t3 = volume_target_shape(num_images, shape, source_voxel, target_voxel, rotation)
        first_shape = (shape[1], shape[0]) if rotated else shape
        derive(first_shape, scaled_voxel(shape, source_voxel, first_shape, rotated)[1:], target_voxel, alternating_downsampling_method)
        downsampled_path = downsampled_dir(downsampled_path, destination, steps, source_voxel[0], target_voxel)
        downsampled_path.mkdir(parents=True, exist_ok=True)
    groups = z_groups(num_images, steps)

    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    capi.require_gpu()
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)) % max(torch.cuda.device_count(), 1))
    if is_tsv and source.device is not None and torch.device(source.device) != device:
        raise ValueError(f"source.device={source.device!r}: the per-slice pass of this rank works on {device}")
    on_device = fun is pystripe.process_img
    writes_images = save_images and (is_tsv or fun is not None or rotation in (90, 180, 270))   # :355
    plans = {}

    def plan_for(kind):
        if kind not in plans:
            vy, vx = scaled_voxel(shape, source_voxel, kind[0], rotated)[1:]
            plans[kind] = Plan(device, kind[0], kind[1], (vy, vx), target_voxel, alternating_downsampling_method, rounds, out_dtype,
                               max_group=steps)
        return plans[kind]

    def rotate(img):
        if rotation not in (90, 180, 270):
            return img
        if isinstance(img, torch.Tensor):
            turned = torch.rot90(_layout(img), rotation // 90, dims=(-2, -1)).contiguous()
            return turned.view(torch.uint16) if img.dtype == torch.uint16 else turned
        return np.rot90(img, rotation // 90)

    def to_device(img):
        """a processed slice as a device tensor of a type the kernels read (anything else becomes float32, as the reference's astype)"""
        if isinstance(img, torch.Tensor):
            return img if _np_dtype(img) in pystripe._NP_CODES else img.to(torch.float32)
        img = np.ascontiguousarray(img)
        if img.dtype not in pystripe._NP_CODES:
            img = img.astype(np.float32)
        return torch.from_numpy(img).to(device)

    def save_plane(path, plane):
        part = path.with_name(path.name + ".part")
        pystripe.imsave_tif(part, plane, compression)
        os.replace(part, path)   # another rank never sees half a file

    def process_group(group_idx, indices):
        plane_path = downsampled_path / f"{tif_prefix}_{group_idx:06}.tif" if need_down_sampling else None
        out_paths = [tif_save_path(destination, images, idx, rename, tif_prefix) for idx in indices]
        if need_down_sampling and resume and plane_path.exists() and all(p.exists() for p in out_paths):
            return
        slices = [None] * len(indices)   # processed slices: device tensors, or None where nothing is to be done
        todo = []
        for k, (idx, path) in enumerate(zip(indices, out_paths)):
            if resume and path.exists():
                if need_down_sampling:   # read back instead of computed again
                    img = pystripe.imread_tif_raw_png(path)
                    slices[k] = None if img is None else to_device(img)
            else:
                todo.append(k)
        if todo and on_device and is_tsv:   # the planes of the group from ONE merge; they stay on the device
            with torch.cuda.device(device):
                stack = read_planes(indices[todo[0]], indices[todo[-1]])
            if len(todo) != todo[-1] - todo[0] + 1:   # resumed: some planes in between exist already
                stack = _stack([stack[k - todo[0]] for k in todo])
            for k, r in zip(todo, list(rotate(_call(fun, stack, args, kwargs)))):
                slices[k] = r
        elif todo and on_device:
            src = [read_source(indices[k]) for k in todo]
            if len({(s.shape, s.dtype) for s in src}) == 1:   # the whole group through every launch together
                stack = torch.from_numpy(np.stack(src)).to(device)
                done = rotate(_call(fun, stack, args, kwargs))
                results = list(done)
            else:
                results = [rotate(_call(fun, torch.from_numpy(np.ascontiguousarray(s)).to(device), args, kwargs)) for s in src]
            for k, r in zip(todo, results):
                slices[k] = r
        else:
            for k in todo:
                img = read_source(indices[k])
                if fun is not None:
                    img = _call(fun, img, args, kwargs)
                slices[k] = rotate(img)
        if writes_images:
            for k in todo:
                img = slices[k]
                pystripe.imsave_tif(out_paths[k], img.cpu().numpy() if isinstance(img, torch.Tensor) else np.ascontiguousarray(img), compression)
        if not need_down_sampling:
            return
        present = [to_device(s).contiguous() for s in slices if s is not None]
        if not present:
            return
        kinds = {_device_kind(t) for t in present}
        processed_dtype = _np_dtype(present[-1])
        if len(kinds) == 1 and len(present) == len(indices):
            plane, uniform = plan_for(next(iter(kinds))).run(_stack(present))
        else:   # slices of several kinds, or a slice that could not be read back (its plane stays zero): plane by plane
            target_shape = plan_for(_device_kind(present[-1])).target_shape
            stack = torch.zeros((len(indices),) + target_shape, dtype=torch.float32, device=device)
            for k, s in enumerate(slices):
                if s is not None:
                    p = plan_for(_device_kind(to_device(s)))
                    if p.target_shape != target_shape:
                        raise ValueError(f"slices of one z group give planes of {p.target_shape} and {target_shape}")
                    stack[k] = p.planes(to_device(s).contiguous()[None])[0]
            plane, uniform = reduce_z(stack, rounds, out_dtype, processed_dtype)
        if int(uniform.item()):
            save_plane(plane_path, np.zeros(tuple(plane.shape), np.float32))   # the reference's zeros are float32 whatever the dtype
        else:
            save_plane(plane_path, plane.cpu().numpy())

    try:
        for group_idx, indices in list(enumerate(groups))[rank::world] if world > 1 else enumerate(groups):
            process_group(group_idx, indices)
        torch.cuda.synchronize(device)
    finally:
        for p in plans.values():
            p.close()

    if need_down_sampling and rank == 0:
        npz_file = npz_path(downsampled_path.parent, destination, target_voxel)
        if not (resume and npz_file.exists()):
            wanted = [downsampled_path / f"{tif_prefix}_{g:06}.tif" for g in range(len(groups))]
            while world > 1 and not all(p.exists() for p in wanted):   # the other ranks' planes
                time.sleep(0.2)
            files = sorted(downsampled_path.glob("*.tif"))
            stack = np.stack([pystripe.imread_tif_raw_png(f) for f in files])
            volume = resize_antialias(np.ascontiguousarray(stack, dtype=np.float32), t3, device)
            if stack.dtype != np.float32:
                volume = volume.astype(np.float64)   # the reference resizes an integer stack in float64
            spacing = generate_voxel_spacing((num_images, shape[0], shape[1]), source_voxel, t3, target_voxel)
            xI = np.empty(3, dtype=object)
            xI[:] = spacing
            np.savez_compressed(npz_file, I=volume, xI=xI)
    if return_downsampled_path:
        return 0, downsampled_path
    return 0


# ---------------------------------------------------------------------------------------------------------------------------------
# command line

def _parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="parallel_image_processor.py", allow_abbrev=False,
                                description="isotropic down-sampling of a folder of 2-D slices on the GPU")
    p.add_argument("--input", "-i", required=True, help="folder of 2-D .tif / .tiff / .raw / .png slices, or a TeraStitcher project "
                   ".xml with displacements (merged on the device: ipp_amd.tsv.TSVVolume)")
    p.add_argument("--output", "-o", required=True, help="destination folder (rotated slices are written here)")
    p.add_argument("--voxel_size", type=float, nargs=3, required=True, metavar=("Z", "Y", "X"))
    p.add_argument("--voxel_size_target", type=float, required=True, metavar="T")
    p.add_argument("--downsampled_path", default=None, help="parent of the down-sampled folder and the npz (default: --output)")
    p.add_argument("--rotation", type=int, default=0, choices=(0, 90, 180, 270))
    p.add_argument("--down_sampled_dtype", default="float32", choices=("float32", "uint16", "uint8"))
    p.add_argument("--no-alternating", dest="alternating", action="store_false", help="every halving round is mean / mean")
    p.add_argument("--rename", action="store_true", help="full-resolution outputs are named img_000000.tif, ...")
    p.add_argument("--alt_stack_dir", default=None, help="project XML: stacks folder of another channel")
    p.add_argument("--cosine_blending", action="store_true", help="project XML: the float16 cosine blend instead of the maximum")
    p.add_argument("--ignore_z_offsets", action="store_true", help="project XML: the D displacements are dropped")
    return p.parse_args(argv)


def main(argv=None):
    a = _parse_args(argv)
    source = a.input
    if str(a.input).lower().endswith(".xml"):
        from .tsv import TSVVolume
        source = TSVVolume(a.input, ignore_z_offsets=a.ignore_z_offsets, alt_stack_dir=a.alt_stack_dir, cosine_blending=a.cosine_blending)
    elif a.alt_stack_dir is not None or a.cosine_blending or a.ignore_z_offsets:
        raise SystemExit("--alt_stack_dir, --cosine_blending and --ignore_z_offsets go with a project .xml as --input")
    rc, folder = parallel_image_processor(source, a.output, source_voxel=tuple(a.voxel_size), target_voxel=a.voxel_size_target,
                                          downsampled_path=a.downsampled_path, rotation=a.rotation, down_sampled_dtype=a.down_sampled_dtype,
                                          alternating_downsampling_method=a.alternating, rename=a.rename, return_downsampled_path=True)
    print(f"parallel_image_processor: down-sampled planes in {folder}")
    return rc


if __name__ == "__main__":
    sys.exit(main())
