"""Test infrastructure: the isotropic down-sampling of parallel_image_processor.py restated in plain numpy + scipy.

scikit-image is not a dependency: ``resize``, ``block_reduce`` and ``resize_local_mean`` are the restatements below, written against
scipy.  Everything here works on host arrays and is the yardstick of tests/test_isodown_host.py and tests/test_gpu_isodown.py.
"""
import math

import numpy as np
from scipy import ndimage

# the cases of the GPU test: name -> (slice shape, (vy, vx), target)
CASES = {
    "A": ((45, 70), (1.0, 0.5), 5.0),
    "B": ((37, 41), (0.7, 0.7), 10.0),
    "C": ((10, 33), (1.0, 1.0), 1.5),
    "D": ((90, 100), (1.0, 1.0), 30.0),
    "E": ((9, 7), (2.0, 2.0), 1.0),
    "F": ((300, 3), (0.5, 1.0), 2.9),
    # additions: rows whose bytes are a multiple of 16 (the kernel's vector loads) and more than one work-group per axis
    "V": ((37, 48), (0.7, 0.7), 10.0),
    "W": ((150, 1104), (1.0, 1.0), 5.0),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# resize

def resize(a, out_shape):
    """resize(a, out_shape, preserve_range=True, anti_aliasing=True) of a float32 array"""
    a = np.asarray(a, np.float32)
    out_shape = tuple(int(v) for v in out_shape)
    f = np.array(a.shape, float) / np.array(out_shape, float)
    cur = a
    if np.any(f > 1):
        cur = ndimage.gaussian_filter(a, np.maximum(0, (f - 1) / 2), mode="mirror", cval=0)
    out = ndimage.zoom(cur, [1 / v for v in f], order=1, mode="mirror", grid_mode=True)
    assert out.shape == out_shape and out.dtype == np.float32, (out.shape, out_shape, out.dtype)
    return np.clip(out, a.min(), a.max())


def gaussian_taps(sigma):
    radius = int(4 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def mirror_index(i, n):
    """d c b | a b c d | c b a, of any reach"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def resize_separable(a, out_shape, acc=np.float64):
    """``resize`` as the kernels compute it: per-axis Gaussian taps on all axes (accumulated in ``acc``, float32 between the axes),
    then per-axis two-point interpolation on all axes, then the clip."""
    a = np.asarray(a, np.float32)
    f = np.array(a.shape, float) / np.array(out_shape, float)
    cur = a
    if np.any(f > 1):
        for ax, fa in enumerate(f):
            sigma = max(0.0, (fa - 1) / 2)
            if sigma <= 1e-15:
                continue
            taps = gaussian_taps(sigma)
            r = len(taps) // 2
            n = cur.shape[ax]
            idx = mirror_index(np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :], n)
            moved = np.moveaxis(cur, ax, -1)[..., idx].astype(acc)
            total = np.zeros(moved.shape[:-1], acc)
            for k in range(len(taps)):
                total = total + moved[..., k] * acc(taps[k])
            cur = np.moveaxis(total.astype(np.float32), -1, ax)
    for ax, (n, m) in enumerate(zip(a.shape, out_shape)):
        c = (np.arange(m) + 0.5) * n / m - 0.5
        fl = np.floor(c)
        t = (c - fl).astype(acc)
        moved = np.moveaxis(cur, ax, -1)
        lo, hi = moved[..., mirror_index(fl, n)].astype(acc), moved[..., mirror_index(fl + 1, n)].astype(acc)
        cur = np.moveaxis((lo * (1 - t) + hi * t).astype(np.float32), -1, ax)
    return np.clip(cur, a.min(), a.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# block_reduce

def halve(a, axis, method):
    """block_reduce(a, 2 along ``axis``, max / mean): zeros behind an odd extent, (a + b) / 2 in float32"""
    a = np.asarray(a, np.float32)
    if a.shape[axis] % 2:
        pad = [(0, 0)] * a.ndim
        pad[axis] = (0, 1)
        a = np.pad(a, pad)
    first, second = np.take(a, range(0, a.shape[axis], 2), axis), np.take(a, range(1, a.shape[axis], 2), axis)
    if method == "max":
        return np.maximum(first, second)
    assert method == "mean", method
    return ((first + second) / np.float32(2)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan of one slice shape

def scaled_voxel(source_shape, source_voxel, new_shape, is_rotated):
    """voxel sizes (z, y, x) of a processed slice of ``new_shape`` whose source had ``source_shape``"""
    vz, vy, vx = (float(v) for v in source_voxel)
    if is_rotated:
        vy *= source_shape[0] / new_shape[1]
        vx *= source_shape[1] / new_shape[0]
        vy, vx = vx, vy
    else:
        vy *= source_shape[0] / new_shape[0]
        vx *= source_shape[1] / new_shape[1]
    return vz, vy, vx


def plan(shape, voxel_yx, target, alternating=True):
    """target shape, the rounds [(y method, x method)] and the halvings that run [(axis, method, extent before)] with the halved
    shape"""
    times = target / np.array(voxel_yx, float)
    target_shape = tuple(int(v) for v in (np.array(shape) / times).round().astype(int))
    factors = np.floor(np.sqrt(times)).astype(int)
    my = ["max" if i % 2 == 0 else "mean" for i in range(factors[0])]
    mx = ["mean" if i % 2 == 0 else "max" for i in range(factors[1])]
    most = max(len(my), len(mx))
    my += [None] * (most - len(my))
    mx += [None] * (most - len(mx))
    rounds = list(zip(my, mx))
    if not alternating:
        rounds = [("mean", "mean")] * len(rounds)
    steps = []
    h, w = int(shape[0]), int(shape[1])
    for y_method, x_method in rounds:
        if y_method is not None and math.ceil(h / 2) >= target_shape[0]:
            steps.append((0, y_method, h))
            h = (h + 1) // 2
        if x_method is not None and math.ceil(w / 2) >= target_shape[1]:
            steps.append((1, x_method, w))
            w = (w + 1) // 2
    return dict(target_shape=target_shape, rounds=rounds, steps=steps, halved_shape=(h, w), factors=tuple(int(v) for v in factors))


def halve_chain(img, p):
    img = np.asarray(img).astype(np.float32)
    for axis, method, extent in p["steps"]:
        assert img.shape[axis] == extent
        img = halve(img, axis, method)
    assert img.shape == p["halved_shape"]
    return img


def is_uniform(a):
    a = np.asarray(a)
    return bool((a == a.flat[0]).all())


def slice_plane(img, p):
    """the float32 plane of one processed slice"""
    if is_uniform(img):
        return np.zeros(p["target_shape"], np.float32)
    return resize(halve_chain(img, p), p["target_shape"]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# z

def z_steps(target, voxel_z):
    return max(1, math.floor(target / voxel_z))


def z_rounds(target, voxel_z):
    return math.ceil(math.sqrt(target / voxel_z))


def z_groups(count, steps):
    """consecutive runs of ``steps`` slice indices; the last one holds the slices that are left"""
    return [list(range(i, min(i + steps, count))) for i in range(0, count, steps)]


def z_groups_of_the_reference(start, end, steps):
    """what calculate_downsampling_z_ranges returns: the last group is trimmed only when its last index is larger than ``end``, so
    a group that ends exactly at index ``end`` keeps that index, one past the last slice"""
    groups = []
    for first in range(start, end, steps):
        group = list(range(first, first + steps))
        if group[-1] > end:
            group = [i for i in group if i < end]
        groups.append(group)
    return groups


def convert_to_16bit(img):
    return np.minimum(np.maximum(img, 0), 65535).astype(np.uint16)


def convert_to_8bit(img, shift=8):
    wide = img if img.dtype == np.uint16 else convert_to_16bit(img)
    out = np.minimum(wide >> shift, 255).astype(np.uint8)
    out[(wide > 0) & (out == 0)] = 1
    return out


def z_reduce(stack, rounds, out_dtype="float32", processed_dtype=np.uint16):
    """the plane of one group from its stack of planes [n, ny, nx]"""
    stack = np.asarray(stack, np.float32)
    if is_uniform(stack):
        return np.zeros(stack.shape[1:], np.float32)
    for i in range(rounds):
        if stack.shape[0] > 1:
            stack = halve(stack, 0, "max" if i % 2 == 0 else "mean")
    if stack.shape[0] != 1:
        raise ValueError(f"{rounds} rounds leave {stack.shape[0]} planes")
    img = stack[0]
    out_dtype = np.dtype(out_dtype)
    if out_dtype == np.uint16:
        img = convert_to_16bit(img)
    elif out_dtype == np.uint8:
        img = img.astype(np.uint8) if np.dtype(processed_dtype) == np.uint8 else convert_to_8bit(img)
    return img


# ---------------------------------------------------------------------------------------------------------------------------------
# the final volume

def local_mean_first(values, m):
    """element 0 of resize_local_mean(values, (m,)): the overlap-weighted mean of the inputs over [0, n / m)"""
    values = np.asarray(values, np.float64)
    n = len(values)
    j = np.arange(n, dtype=np.float64)
    weights = np.maximum(np.minimum(n / m, j + 1) - j, 0)
    weights /= weights.sum()
    return float((weights * values).sum())


def generate_voxel_spacing(shape, source_voxel, target_shape, target_voxel):
    out = []
    for n, v, m in zip(shape, source_voxel, target_shape):
        locations = np.arange(n) * v - (n - 1) / 2.0 * v
        start = np.round(local_mean_first(locations, int(m)))
        out.append(np.array([start + target_voxel * k for k in range(int(m))], dtype=np.float64))
    return out


def volume_target_shape(count, shape, source_voxel, target, rotation=0):
    t = [int(round(count / (target / source_voxel[0]))), int(round(shape[0] / (target / source_voxel[1]))),
         int(round(shape[1] / (target / source_voxel[2])))]
    if rotation in (90, 270):
        t[1], t[2] = t[2], t[1]
    return t


def final_volume(planes, target_shape_3d):
    stack = np.stack(planes)
    if stack.dtype == np.float32:
        return resize(stack, target_shape_3d)
    return resize(stack.astype(np.float32), target_shape_3d).astype(np.float64)


def run_folder(slices, source_voxel, target, fun=None, rotation=0, alternating=True, out_dtype="float32"):
    """The whole stage on host arrays: ``slices`` (equally shaped 2-D arrays) -> dict(processed=[...], planes=[...], I=..., xI=[...])."""
    shape = slices[0].shape
    rotated = rotation in (90, 270)
    steps, rounds = z_steps(target, source_voxel[0]), z_rounds(target, source_voxel[0])
    processed, planes = [], []
    for group in z_groups(len(slices), steps):
        stack = []
        for idx in group:
            img = slices[idx]
            if fun is not None:
                img = fun(img)
            if rotation in (90, 180, 270):
                img = np.rot90(img, rotation // 90)
            processed.append(img)
            p = plan(img.shape, scaled_voxel(shape, source_voxel, img.shape, rotated)[1:], target, alternating)
            stack.append(slice_plane(img, p))
        planes.append(z_reduce(np.stack(stack), rounds, out_dtype, processed[-1].dtype))
    t3 = volume_target_shape(len(slices), shape, source_voxel, target, rotation)
    return dict(processed=processed, planes=planes, I=final_volume(planes, t3),
                xI=generate_voxel_spacing((len(slices),) + tuple(shape), source_voxel, t3, target), target_shape_3d=t3)


def pattern(shape, dtype, seed=0):
    """a slice with structure at every scale and a differing last sample"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    a = 900.0 + 600.0 * np.sin(0.37 * y) * np.cos(0.23 * x) + rng.uniform(0, 500, shape)
    if np.dtype(dtype) == np.uint8:
        return (a / 8).astype(np.uint8)
    if np.dtype(dtype) == np.uint16:
        return (a * 20).astype(np.uint16)
    return (a - 1000.0).astype(np.float32)   # negative values too
