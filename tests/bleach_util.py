"""TEST INFRASTRUCTURE for the bleach correction of the pystripe stage (tests/test_bleach_host.py, tests/test_gpu_bleach.py, the
golden maker tests/golden/make_bleach_golden.py).

The restatement of ``correct_bleaching`` and of ``process_img`` with it, in float32 or float64, written from the description of the
step: the stripe filter comes from tests/pystripe_util.py, the row filter is ``scipy.signal.sosfiltfilt`` on ``butter(1, f, 'sos')``.
``lowpass_explicit`` is the same row filter as the plain recurrence the kernels run.
"""
from __future__ import annotations

import glob
import json
import math
import os

import numpy as np
from scipy.signal import butter, sosfiltfilt

from tests import pystripe_util as U

GOLDEN_SUBDIR = "bleach"
PADLEN = 6                                   # sosfiltfilt's default for one section: 3 * (2 * 1 + 1 - 1) = 6
# The row filter keeps a row of n samples in LDS as n + 12 doubles beside the 16 wave totals (16 bytes each) of its scan; the kernel
# may ask for all 160 KiB of a compute unit's LDS.  Longer rows take the segmented route.
LDS_BYTES, SCAN_TOTALS_BYTES = 160 * 1024, 16 * 16
LDS_ROW = (LDS_BYTES - SCAN_TOTALS_BYTES) // 8 - 2 * PADLEN    # 20436
BLEACH_KEYS = ("bleach_correction_frequency", "bleach_correction_max_method", "bleach_correction_clip_min", "bleach_correction_clip_med",
               "bleach_correction_clip_max")


def golden_dir(root):
    return os.path.join(root, "tests", "golden", GOLDEN_SUBDIR)


def golden_cases(root):
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(golden_dir(root), "*.npz"))
                  if not p.endswith("refusals.npz"))


def load_case(root, name):
    z = np.load(os.path.join(golden_dir(root), name + ".npz"))
    kwargs = json.loads(str(z["kwargs"]))
    for k in ("sigma", "down_sample"):
        if kwargs.get(k) is not None:
            kwargs[k] = tuple(kwargs[k])
    return z, kwargs


def coefficients(frequency, from_scipy=False):
    """(b, a) of the section: y[i] = b u[i] + z, then z = b u[i] + a y[i]."""
    if from_scipy:
        sos = butter(1, frequency, output="sos")[0]     # [b0, b1, 0, 1, a1, 0] with b0 == b1
        return float(sos[0]), float(-sos[4])
    k = math.tan(math.pi * frequency / 2)
    return k / (1 + k), (1 - k) / (1 + k)


def lowpass(x, frequency):
    """butter_lowpass_filter without its cast: float64."""
    return sosfiltfilt(butter(1, frequency, output="sos"), x)


def lowpass_explicit(x, frequency, from_scipy=False):
    """The same along the last axis as the recurrence itself: odd extension by 6 samples per side, a forward pass from
    z = (1 - b) u[0], the same pass over the reversed result, the extension dropped.  float64."""
    b, a = coefficients(frequency, from_scipy)
    x = np.asarray(x, np.float64)
    rows = np.atleast_2d(x)
    n = rows.shape[1]
    if n <= PADLEN:
        raise ValueError("The length of the input vector x must be greater than padlen, which is 6.")
    u = np.concatenate([2 * rows[:, :1] - rows[:, PADLEN:0:-1], rows, 2 * rows[:, -1:] - rows[:, -2:-2 - PADLEN:-1]], axis=1)

    def run(u):
        y = np.empty_like(u)
        z = (1 - b) * u[:, 0]
        for i in range(u.shape[1]):
            y[:, i] = b * u[:, i] + z
            z = b * u[:, i] + a * y[:, i]
        return y

    y = run(run(u)[:, ::-1])[:, ::-1]
    return y[:, PADLEN:-PADLEN].reshape(x.shape)


def correct_bleaching(L, frequency, clip_min, clip_med, clip_max, max_method=False, dt=np.float32, row_filter=lowpass):
    """L' = (L / F) * max F with F the low-passed clipped copy of L (rows), or the outer product of the low-passed clipped row and
    column maxima of L.  Everything but the row filter (float64) in ``dt``."""
    dt = np.dtype(dt).type
    L = np.asarray(L, dt)
    lo, med, hi = dt(max(clip_min, math.log1p(1))), dt(clip_med), dt(clip_max)

    def clipped(v):
        g = v.copy()
        g[g == 0] = med
        return np.clip(g, lo, hi)

    if max_method:
        ry = row_filter(clipped(L.max(axis=1)), frequency).astype(dt)
        cx = row_filter(clipped(L.max(axis=0)), frequency).astype(dt)
        F = ry[:, None] * cx[None, :]
    else:
        F = row_filter(clipped(L), frequency).astype(dt)
    return ((L / F) * F.max()).astype(dt)


def split_kwargs(kw):
    """(bleach arguments of correct_bleaching or None, everything else)"""
    rest = {k: v for k, v in kw.items() if k not in BLEACH_KEYS}
    if kw.get("bleach_correction_frequency") is None:
        return None, rest
    return dict(frequency=kw["bleach_correction_frequency"], clip_min=kw["bleach_correction_clip_min"],
                clip_med=kw["bleach_correction_clip_med"], clip_max=kw["bleach_correction_clip_max"],
                max_method=kw.get("bleach_correction_max_method", False)), rest


def process_img(img, dt=np.float32, row_filter=lowpass, **kw):
    """Restatement of process_img with the bleach correction.  Returns (result, log-domain image just before expm1)."""
    bleach, kw = split_kwargs(kw)
    if bleach is None or (img == img.flat[0]).all():
        return U.process_img(img, dt=dt, **kw)
    d_type = np.dtype(img.dtype if kw.get("d_type") is None else kw["d_type"])
    flat, down_sample, sigma = kw.pop("flat", None), kw.pop("down_sample", None), tuple(kw.pop("sigma", (0, 0)))
    method = kw.pop("down_sample_method", "max")
    stripe = {k: kw.pop(k) for k in ("level", "padding_mode", "bidirectional") if k in kw}
    kw.pop("wavelet", None)
    if flat is not None and flat.shape == img.shape:
        img = img.astype(np.float32) / flat
    if down_sample is not None:
        img = U.block_reduce(img, tuple(down_sample), {"max": np.max, "min": np.min, "mean": np.mean}[method.lower()])
    kind = img.dtype
    if sigma > (0, 0):
        L = U.filter_streaks_log(img, sigma, dt=dt, **dict(dict(level=0, padding_mode="wrap", bidirectional=False), **stripe))
    else:
        L = np.log1p(img.astype(dt))
    L = correct_bleaching(L, dt=dt, row_filter=row_filter, **bleach)
    f = np.expm1(L).astype(dt)
    if kind.kind in "ui":
        f = np.clip(np.rint(f), np.iinfo(kind).min, np.iinfo(kind).max)
    out, _ = U.process_img(f.astype(kind), dt=dt, **dict(kw, d_type=d_type))     # the tail: dark, conversions, flip, rotation
    return out, L


def e_ref_floor(log64):
    """One float32 spacing at the largest |log64|: no float32 image lies closer to a float64 one than its own rounding."""
    return float(np.spacing(np.float32(np.abs(log64).max())))


def clips_for(img, fractions=(0.25, 0.6, 0.9)):
    """Three log1p-domain clips inside the tile's range, as Python floats: quantiles of the non-zero samples."""
    v = np.log1p(img[img > 0].astype(np.float64))
    lo, med, hi = (float(np.quantile(v, q)) for q in fractions)
    return dict(bleach_correction_clip_min=lo, bleach_correction_clip_med=med, bleach_correction_clip_max=hi)
