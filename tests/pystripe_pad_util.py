"""TEST INFRASTRUCTURE for the value padding modes of the pystripe stage (tests/test_pystripe_padmodes_host.py,
tests/test_gpu_pystripe_padmodes.py).

The restatement of ``filter_streaks`` for ``padding_mode`` constant / linear_ramp / maximum / mean / median / minimum: numpy's float
``log1p``, then numpy's own ``pad`` -- the reference's call (pystripe/core.py:1100-1110) -- with the widths of ``pystripe_util.geometry``,
then the stripe filter of tests/pystripe_util.py (db9) or tests/wavelet_util.py (any ``rec_lo``), the bleach correction of
tests/bleach_util.py and the tail of ``pystripe_util.process_img``; in float32 or float64.
"""
from __future__ import annotations

import math

import numpy as np

from tests import autoclips_util as A
from tests import bleach_util as B
from tests import pystripe_util as U
from tests import wavelet_util as W

VALUE_MODES = ("constant", "linear_ramp", "maximum", "mean", "median", "minimum")
INDEX_MODES = U.PADDING_MODES
# keys of a line that stay in LDS beside the selection's 256 digit counts and 16 control words, in a quarter of a CU's 160 KiB: 9968
LDS_LINE = 160 * 1024 // 4 // 4 - 256 - 16
LOG2 = math.log1p(1.0)


def pad_log(x, widths, mode, constant=0.0):
    """numpy.pad of the log image ``x`` as filter_streaks calls it: ``constant_values`` for 'constant', defaults otherwise."""
    if mode == "constant":
        return np.pad(x, widths, mode="constant", constant_values=x.dtype.type(constant))
    return np.pad(x, widths, mode=mode)


def pad_constant(clip_min):
    """The value 'constant' pads with: 0 without a clip_min, else log1p of it -- the clip is in log units already and the reference
    takes the logarithm once more (pystripe/core.py:1104)."""
    return 0.0 if clip_min is None else float(np.log1p(np.float64(clip_min)))


def filter_streaks_log(img, sigma, padding_mode, level=0, bidirectional=False, dt=np.float32, constant=0.0, rec_lo=None):
    """The log-domain image of filter_streaks just before the bleach correction / expm1 (cropped to the tile)."""
    s1, s2 = sigma
    x = np.log1p(img.astype(dt))
    ny, nx = x.shape
    taps = 18 if rec_lo is None else len(rec_lo)
    bp, py, px, _, _, _ = W.geometry(x.shape, sigma, taps, level)
    x = pad_log(x, ((bp, bp + py), (bp, bp + px)), padding_mode, constant)
    axes = (-1, -2) if bidirectional else (-1,)
    for s in ((s1,) if s1 == s2 else (s1, s2)):
        x = U.filter_subband(x, s, level, axes, dt) if rec_lo is None else W.filter_subband(x, W.filters_from_rec_lo(rec_lo), s, level, axes, dt)
    return x[bp:bp + ny, bp:bp + nx]


def process_img(img, sigma, padding_mode, dt=np.float32, level=0, bidirectional=False, rec_lo=None, constant=None, **kw):
    """(result, log-domain image just before expm1).  ``kw``: the bleach keywords of process_img (a clip that is None is the
    restatement's multi-Otsu estimate of this tile) and the tail options of ``pystripe_util.process_img``.  ``constant``: the padded
    value; None derives it as the reference does, from the clip_min it ends up with BEFORE that is raised to log1p(1)."""
    kw = A.filled(img, **kw)
    bleach, tail = B.split_kwargs(kw)
    if constant is None:
        constant = pad_constant(kw.get("bleach_correction_clip_min"))
    tail.pop("wavelet", None)
    kind = img.dtype
    L = filter_streaks_log(img, tuple(sigma), padding_mode, level, bidirectional, dt, constant, rec_lo)
    if bleach is not None:
        L = B.correct_bleaching(L, dt=dt, **bleach)
    f = np.expm1(L).astype(dt)
    if kind.kind in "ui":
        f = np.clip(np.rint(f), np.iinfo(kind).min, np.iinfo(kind).max)
    out, _ = U.process_img(f.astype(kind), dt=dt, **tail)
    return out, L


def reference(img, **kw):
    """(float32 result, float64 log image, E_ref): E_ref is the float32 restatement's own distance from the float64 one."""
    r32, l32 = process_img(img.copy(), dt=np.float32, **kw)
    _, l64 = process_img(img.copy(), dt=np.float64, **kw)
    return r32, l64, float(np.abs(l32.astype(np.float64) - l64).max())


def low_floor_tile(shape, seed, dtype=np.uint8):
    """Four populations in smooth regions, the darkest of them exact zeros: the lowest multi-Otsu threshold of the log image falls
    into the empty range above 0, far below log1p(1)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    field = np.cos(2 * np.pi * yy / shape[0] + 0.3) + np.cos(4 * np.pi * xx / shape[1]) + 0.5 * np.cos(2 * np.pi * (yy + xx) / sum(shape))
    level = np.searchsorted(np.quantile(field, [.4, .7, .9]), field)
    img = np.choose(level, [np.zeros(shape), rng.integers(6, 10, shape), rng.integers(40, 60, shape), rng.integers(180, 250, shape)])
    return img.astype(dtype)
