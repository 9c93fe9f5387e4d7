"""TEST INFRASTRUCTURE for the lightsheet correction (tests/test_lightsheet_host.py, tests/test_gpu_lightsheet.py, the golden maker).

A plain numpy restatement of ``pystripe/lightsheet_correct.py`` as ``process_img`` calls it, written from the description of the
stage: window bookkeeping, ``numpy.percentile`` for the selection, an order-1 resampling of its own (NOT a call to scipy: the tests
compare it with ``scipy.ndimage.zoom``) and the combination rule with its integer wrap.  It must reproduce every golden of
tests/golden/lightsheet on the CPU, and it is the live comparison for shapes that have no golden.
"""
from __future__ import annotations

import numpy as np

GOLDEN_SUBDIR = "lightsheet"
BG_SPACING, BG_STEP = 25, 2


# ---------------------------------------------------------------------------------------------------------------------------------
# bookkeeping

def centres(extent, spacing):
    """(count, first centre) along one axis: ``extent // spacing`` centres, the remainder split in front and behind."""
    n = extent // spacing
    return n, (extent - (n - 1) * spacing) // 2 if n else 0


def window(centre, selem, extent):
    """[start, stop) of the window of ``selem`` samples around ``centre``, clipped to the axis."""
    left = selem // 2
    return max(0, centre - left), min(centre + (selem - left), extent)


def zoom_axis(n_in, n_out):
    """Per output index of an order-1 resampling n_in -> n_out samples: (lower node, weight of it, weight of the next, outside flag)."""
    scale = np.float64(n_in - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(1.0)
    c = np.arange(n_out, dtype=np.float64) * scale
    f = np.floor(c)
    w0 = 1.0 - (c - f)
    w1 = 1.0 - w0
    return f.astype(np.int64), w0, w1, c > n_in - 1


def bookkeeping(shape, artifact_length=150, background_window_size=200, spacing=BG_SPACING, step=BG_STEP):
    """What ``mi_lightsheet_derive`` reports, from the formulas above."""
    ny, nx = shape
    L, W = artifact_length, background_window_size
    ls_nx, ls_left = centres(nx, L)
    by, bly = centres(ny, spacing)
    bx, blx = centres(nx, spacing)
    out = dict(ls_ny=ny, ls_nx=ls_nx, ls_left_y=0, ls_left_x=ls_left, bg_ny=by, bg_nx=bx, bg_left_y=bly, bg_left_x=blx)
    for name, n, left, extent in (("y", by, bly, ny), ("x", bx, blx, nx)):
        first, last = window(left, W, extent), window(left + (n - 1) * spacing, W, extent)
        out.update({f"bg_first_{name}0": first[0], f"bg_first_{name}1": first[1], f"bg_last_{name}0": last[0], f"bg_last_{name}1": last[1]})
        out[f"_most_{name}"] = max(-(-(b - a) // step) for a, b in (window(left + i * spacing, W, extent) for i in range(n)))
    out["max_window_samples"] = max(out.pop("_most_y") * out.pop("_most_x"), L)
    out["ls_zero_last_row"] = 0
    out["ls_zero_last_col"] = int(zoom_axis(ls_nx, nx)[3][-1])
    out["bg_zero_last_row"] = int(zoom_axis(by, ny)[3][-1])
    out["bg_zero_last_col"] = int(zoom_axis(bx, nx)[3][-1])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the three steps

def percentile_grid(img, percentile, selem, spacing=None, step=None, dtype=None):
    """The sub-grid of local percentiles (``local_percentile(..., interpolate=None)``) of a 2-D image."""
    spacing = selem if spacing is None else spacing
    step = (1, 1) if step is None else tuple(1 if s is None else s for s in step)
    ny, nx = img.shape
    (cy, ly), (cx, lx) = centres(ny, spacing[0]), centres(nx, spacing[1])
    grid = np.zeros((cy, cx), img.dtype if dtype is None else dtype)
    q = 100 * percentile
    for i in range(cy):
        y0, y1 = window(ly + i * spacing[0], selem[0], ny)
        rows = img[y0:y1:step[0]]
        for j in range(cx):
            x0, x1 = window(lx + j * spacing[1], selem[1], nx)
            data = rows[:, x0:x1:step[1]].ravel()
            grid[i, j] = np.percentile(data, q) if data.size else 0     # the store truncates for an integer grid
    return grid


def row_grid(img, percentile, length, dtype=None):
    """``percentile_grid(img, percentile, (1, length))`` in one numpy.percentile call over the window axis."""
    ny, nx = img.shape
    cx, left = centres(nx, length)
    x0 = left - length // 2
    runs = img[:, x0:x0 + cx * length].reshape(ny, cx, length)
    grid = np.zeros((ny, cx), img.dtype if dtype is None else dtype)
    grid[...] = np.percentile(runs, 100 * percentile, axis=2)
    return grid


def zoom1(grid, shape):
    """Order-1 resampling of a 2-D grid to ``shape`` with scipy.ndimage.zoom's arithmetic (mode 'constant'): float64, the four
    products summed in a fixed order, integer output rounded half up and clamped, the line past the last node set to zero."""
    fy, wy0, wy1, oy = zoom_axis(grid.shape[0], shape[0])
    fx, wx0, wx1, ox = zoom_axis(grid.shape[1], shape[1])
    g = grid.astype(np.float64)
    fy1, fx1 = np.minimum(fy + 1, grid.shape[0] - 1), np.minimum(fx + 1, grid.shape[1] - 1)
    fy, fx = np.minimum(fy, grid.shape[0] - 1), np.minimum(fx, grid.shape[1] - 1)
    wy0, wy1 = wy0[:, None], wy1[:, None]
    v = (g[fy][:, fx] * wy0) * wx0
    v = v + (g[fy][:, fx1] * wy0) * wx1
    v = v + (g[fy1][:, fx] * wy1) * wx0
    v = v + (g[fy1][:, fx1] * wy1) * wx1
    v[oy, :] = 0
    v[:, ox] = 0
    if grid.dtype.kind in "ui":
        info = np.iinfo(grid.dtype)
        v = np.clip(np.floor(v + 0.5), info.min, info.max)
    return v.astype(grid.dtype)


def combine(img, ls, bg, lightsheet_vs_background=2.0):
    """img - min(img, min(ls, bg * factor)) with the reference's types: all-integer operands use the truncated factor and wrap."""
    if isinstance(lightsheet_vs_background, float) and all(a.dtype in (np.uint8, np.uint16) for a in (img, ls, bg)):
        return img - np.minimum(img, np.minimum(ls, bg * int(lightsheet_vs_background)))
    return img - np.minimum(img, np.minimum(ls, bg * lightsheet_vs_background)).astype(img.dtype)


def correct_lightsheet(img, percentile=0.25, artifact_length=150, background_window_size=200, lightsheet_vs_background=2.0,
                       d_type=None, spacing=BG_SPACING, step=BG_STEP, fast_rows=False):
    """(corrected image, lightsheet map, background map, lightsheet sub-grid, background sub-grid)"""
    d_type = img.dtype if d_type is None else np.dtype(d_type)
    ny, nx = img.shape
    if nx < artifact_length or ny < spacing or nx < spacing:
        raise NotImplementedError("lightsheet: the tile is smaller than one window")
    if fast_rows:
        ls_grid = row_grid(img, percentile, artifact_length, d_type)
    else:
        ls_grid = percentile_grid(img, percentile, (1, artifact_length), dtype=d_type)
    bg_grid = percentile_grid(img, percentile, (background_window_size,) * 2, (spacing,) * 2, (step,) * 2, dtype=d_type)
    ls, bg = zoom1(ls_grid, img.shape), zoom1(bg_grid, img.shape)
    return combine(img, ls, bg, lightsheet_vs_background), ls, bg, ls_grid, bg_grid


def process_img_tail(img, convert_to_16bit=False, convert_to_8bit=False, bit_shift_to_right=8, d_type=None, flip_upside_down=False,
                     rotate=0, **ignored):
    """The end of process_img after the lightsheet step: conversion, flip, rotation."""
    from tests import pystripe_util as P
    d_type = np.dtype(img.dtype if d_type is None else d_type)
    if convert_to_16bit and img.dtype != np.uint16:
        img = np.clip(img, 0, 65535).astype(np.uint16)
    elif convert_to_8bit and img.dtype != np.uint8:
        img = P.convert_to_8bit_fun(img, bit_shift_to_right)
    elif d_type.kind in "ui":
        img = np.clip(img, np.iinfo(d_type).min, np.iinfo(d_type).max).astype(d_type)
    else:
        img = img.astype(d_type)
    if flip_upside_down:
        img = np.flipud(img)
    if rotate in (90, 180, 270):
        img = np.rot90(img, rotate // 90)
    return np.ascontiguousarray(img)


def process_img(img, lightsheet=True, artifact_length=150, background_window_size=200, percentile=0.25, lightsheet_vs_background=2.0,
                **kw):
    """process_img WITHOUT the stripe filter and with the lightsheet step: tests/pystripe_util.process_img up to ``dark`` (no
    conversion, flip or rotation), the step above, then the tail."""
    from tests import pystripe_util as P
    entry_type = np.dtype(img.dtype if kw.get("d_type") is None else kw["d_type"])
    if (img == img.flat[0]).all():
        return P.process_img(img, **kw)[0]
    head = {k: v for k, v in kw.items() if k in ("flat", "down_sample", "down_sample_method", "dark", "flat_on_integers")}
    pre = _head(img, **head)
    out = correct_lightsheet(pre, percentile, artifact_length, background_window_size, lightsheet_vs_background, entry_type)[0]
    return process_img_tail(out, **dict(kw, d_type=entry_type))


def _head(img, flat=None, down_sample=None, down_sample_method="max", dark=0, flat_on_integers=False):
    """flat, down_sample and dark of process_img, leaving the tile in the type it has at that point."""
    from tests import pystripe_util as P
    if flat is not None and flat.shape == img.shape:
        if img.dtype.kind in "ui":
            if not flat_on_integers:
                raise TypeError("in-place divide of an integer tile by a float flat field")
            img = img.astype(np.float32)
        img = img / flat
    if down_sample is not None:
        func = {"max": np.max, "min": np.min, "mean": np.mean}[down_sample_method.lower()]
        img = P.block_reduce(img, tuple(down_sample), func)
    if dark and dark > 0:
        img = ((img > dark) * (img - dark)).astype(img.dtype)
    return img


def bead_and_stripe_tile(shape, seed, dtype=np.uint16):
    """A seeded tile with a smooth background, row-aligned lightsheet streaks and bright beads."""
    rng = np.random.default_rng(seed)
    ny, nx = shape
    yy = np.arange(ny, dtype=np.float32)[:, None]
    xx = np.arange(nx, dtype=np.float32)[None, :]
    img = 400 + 250 * np.sin(yy / 97.0) * np.cos(xx / 131.0) + rng.poisson(30, (ny, nx)).astype(np.float32)
    img += (300 * rng.random(ny, dtype=np.float32) ** 4)[:, None] * (0.6 + 0.4 * np.cos(xx / 400.0))
    n_beads = max(ny * nx // 4000, 4)
    img[rng.integers(0, ny, n_beads), rng.integers(0, nx, n_beads)] += rng.integers(500, 30000, n_beads)
    if np.dtype(dtype) == np.uint8:
        return np.clip(img / 8.0, 0, 255).astype(np.uint8)
    if np.dtype(dtype) == np.uint16:
        return np.clip(img, 0, 65535).astype(np.uint16)
    return np.floor(img).astype(np.float32) + rng.integers(0, 16, (ny, nx)).astype(np.float32) / 16
