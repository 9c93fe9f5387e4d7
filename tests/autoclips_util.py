"""TEST INFRASTRUCTURE for the per-tile automatic bleach clips and the median down-sampling of the pystripe stage
(tests/test_autoclips_host.py, tests/test_gpu_autoclips.py, tests/test_gpu_median.py, tests/golden/make_autoclips_golden.py).

The restatement is the composition of two that exist: ``threshold_multiotsu(log1p(tile), classes=4)`` of tests/thresholds_util.py
fills the clips that are None, tests/bleach_util.py does the rest.  The log image is the float32 ``log1p`` of the tile after flat
and ``down_sample``, before padding and the stripe filter (pystripe/core.py:1062-1077).
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np

from tests import bleach_util as B
from tests import pystripe_util as U
from tests import thresholds_util as T

GOLDEN_SUBDIR = "autoclips"
CLIP_KEYS = B.BLEACH_KEYS[2:]
REDUCERS = {"max": np.max, "min": np.min, "mean": np.mean, "median": np.median}
LOG2 = float(np.log1p(1.0))


def golden_dir(root):
    return os.path.join(root, "tests", "golden", GOLDEN_SUBDIR)


def golden_cases(root):
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(golden_dir(root), "*.npz")))


def load_case(root, name):
    z = np.load(os.path.join(golden_dir(root), name + ".npz"))
    kwargs = json.loads(str(z["kwargs"]))
    for k in ("sigma", "down_sample"):
        if kwargs.get(k) is not None:
            kwargs[k] = tuple(kwargs[k])
    return z, kwargs


def reduced(img, flat=None, down_sample=None, down_sample_method="max"):
    """The tile after flat (float32 divide) and ``down_sample`` (block_reduce, zero padding); a median of integers is float64."""
    if flat is not None and flat.shape == img.shape:
        img = img.astype(np.float32) / flat
    if down_sample is not None:
        img = U.block_reduce(img, tuple(1 if d is None else d for d in down_sample), REDUCERS[down_sample_method.lower()])
    return img


def log_image(img, **kw):
    """What filter_streaks hands to threshold_multiotsu: numpy's float32 log1p of the reduced tile."""
    return np.log1p(reduced(img, kw.get("flat"), kw.get("down_sample"), kw.get("down_sample_method", "max")).astype(np.float32), dtype=np.float32)


def log_histogram(log):
    hist, edges = np.histogram(log.reshape(-1), 256)
    return hist, edges, (edges[:-1] + edges[1:]) / 2


def estimate(log):
    """(float32 thresholds [3], indices [3]) of the restatement for a float32 log image; ValueError as threshold_multiotsu."""
    hist, _, centers = log_histogram(log)
    idx, _ = T.multiotsu_indices(hist, 4)
    return centers[idx].astype(np.float32), idx


def triple(img, **kw):
    """The three clips the reference ends up with (float32; given ones keep their slot), min not yet raised to log1p(1)."""
    est, _ = estimate(log_image(img, **kw))
    return np.array([est[i] if kw.get(k) is None else kw[k] for i, k in enumerate(CLIP_KEYS)], np.float32)


def used_triple(t):
    """the triple as the bleach kernels use it: min raised to log1p(1) (float64 comparison, float32 result)"""
    t = np.array(t, np.float32)
    t[0] = np.float32(max(float(t[0]), LOG2))
    return t


def check_order(t):
    lo, med, hi = (float(v) for v in t)
    assert lo >= 0 and med > lo and hi > lo and hi > med, f"clips {tuple(t)}: 0 <= min < med < max is expected"


def filled(img, clips=None, **kw):
    """kw with every clip that is None replaced: by ``clips`` (a triple, e.g. the device's) or by the restatement's estimate."""
    if kw.get("bleach_correction_frequency") is None or all(kw.get(k) is not None for k in CLIP_KEYS):
        return kw
    t = triple(img, **kw) if clips is None else clips
    check_order(t)
    return dict(kw, **{k: float(np.float32(t[i])) for i, k in enumerate(CLIP_KEYS)})


def process_img(img, dt=np.float32, clips=None, **kw):
    """Restatement of process_img with automatic clips and the median: (result, log-domain image just before expm1).  A median is
    reduced here and goes on as the float tile it is (bleach_util knows max / min / mean), with the tile's own d_type."""
    uniform = (img == img.flat[0]).all()
    if not uniform:
        kw = filled(img, clips, **kw)
    if kw.get("down_sample") is not None and str(kw.get("down_sample_method", "max")).lower() == "median" and not uniform:
        d_type = np.dtype(img.dtype if kw.get("d_type") is None else kw["d_type"])
        tile = reduced(img, kw.pop("flat", None), kw.pop("down_sample"), kw.pop("down_sample_method")).astype(np.float32)
        return B.process_img(tile, dt=dt, **dict(kw, d_type=d_type))
    if kw.get("down_sample_method") == "median":
        kw = dict(kw, down_sample_method="max")      # a uniform tile: only the shape matters
    if kw.get("flat") is not None and img.dtype.kind in "ui":
        kw = dict(kw, flat_on_integers=True)
    return B.process_img(img, dt=dt, **kw)


def live_reference(img, clips=None, **kw):
    """(float32 result, float64 log image, E_ref) of the restatement, as tests/test_gpu_bleach.py's live_reference"""
    r32, l32 = process_img(img.copy(), dt=np.float32, clips=clips, **kw)
    _, l64 = process_img(img.copy(), dt=np.float64, clips=clips, **kw)
    return r32, l64, max(float(np.abs(l32.astype(np.float64) - l64).max()), B.e_ref_floor(l64))


def indices_are_stable(log):
    """True when the restatement's threshold indices do not change with every log sample moved by one float32 ulp either way: the
    device's log1pf may differ from numpy's by that much on a float tile."""
    _, idx = estimate(log)
    for toward in (np.float32(np.inf), np.float32(-np.inf)):
        _, moved = estimate(np.nextafter(log, toward))
        if not np.array_equal(idx, moved):
            return False
    return True


def float_tile(shape, seed):
    """four_mode_image as float32 with fractional parts, so that log1p is not a table of codes"""
    rng = np.random.default_rng(seed + 1000)
    return (T.four_mode_image(shape, seed).astype(np.float32) + rng.random(shape, dtype=np.float32)).astype(np.float32)


def flat_field(shape, seed=5):
    rng = np.random.default_rng(seed)
    f = 0.6 + 0.4 * rng.random(shape)
    return (f / f.max()).astype(np.float32)
