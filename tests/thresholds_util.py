"""TEST INFRASTRUCTURE for the slice estimates (tests/test_thresholds_host.py, tests/test_gpu_thresholds.py).

scikit-image is installed on neither machine, so the yardstick is a numpy restatement of ``skimage.filters.threshold_multiotsu``
written from its description together with numpy's own ``np.histogram`` / ``np.percentile``:

* histogram: ``np.histogram(image.reshape(-1), nbins)`` on the float32 image, centers ``(edges[:-1] + edges[1:]) / 2``;
* ``prob = (hist / hist.sum()).astype(float32)`` (float64 division, then rounded); fewer occupied bins than classes: ValueError;
  exactly as many: the occupied bins but the last;
* float32 prefix sums taken one after the other: ``P[i] = P[i-1] + prob[i]``, ``S[i] = S[i-1] + fl32(i) * prob[i]``, ``S[0] = 0``;
* ``H(i, j) = (s * s) / p`` in float32 with ``p = P[j] - P[i-1]``, ``s = S[j] - S[i-1]`` (0 below bin 0), 0 where ``p <= 0``;
* thresholds ``t0 < t1 < ...``, index k of m below ``nbins - m + k``; ``sigma = ((H(0, t0) + H(t_last + 1, nbins - 1)) + H(t0 + 1, t1))
  + H(t1 + 1, t2)`` in that order; the winner is the first tuple in lexicographic order whose sigma is strictly greater than every
  earlier one, starting from 0.
"""
from __future__ import annotations

import math

import numpy as np

_TUPLES = {}


def four_mode_image(shape, seed=7, dtype=np.uint16):
    """Four intensity populations with 8 % multiplicative noise, limited to the dtype's range (u8: the levels divided by 100)."""
    rng = np.random.default_rng(seed)
    img = rng.choice([110, 400, 2500, 20000], p=[.55, .25, .15, .05], size=shape) * (1 + 0.08 * rng.standard_normal(shape))
    if np.dtype(dtype) == np.uint8:
        return np.clip(img / 100.0, 0, 255).astype(np.uint8)
    return np.clip(img, 0, 65535).astype(np.uint16)


def moments(hist):
    """(prob, P1, S1, nvalues): P1[k], S1[k] are the float32 sums over the bins below k, taken one after the other."""
    hist = np.asarray(hist)
    prob = (hist / hist.sum()).astype(np.float32)
    n = prob.size
    P1, S1 = np.zeros(n + 1, np.float32), np.zeros(n + 1, np.float32)
    p = s = np.float32(0)
    for i in range(n):
        if i == 0:
            p, s = prob[0], np.float32(0)
        else:
            p = np.float32(p + prob[i])
            s = np.float32(s + np.float32(np.float32(i) * prob[i]))
        P1[i + 1], S1[i + 1] = p, s
    return prob, P1, S1, int(np.count_nonzero(prob))


def class_term(P1, S1, i, j, dt=np.float32):
    """H(i, j) for index arrays i <= j, in ``dt``"""
    P1, S1 = P1.astype(dt), S1.astype(dt)
    p = P1[j + 1] - P1[i]
    s = S1[j + 1] - S1[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, (s * s) / p, dt(0)).astype(dt)


def threshold_tuples(nbins, m):
    """every admissible tuple of m thresholds in lexicographic order, one array per threshold"""
    if (nbins, m) not in _TUPLES:
        axes = np.meshgrid(*[np.arange(nbins - m + k, dtype=np.int32) for k in range(m)], indexing="ij", sparse=True)
        ok = np.ones((), bool)
        for k in range(1, m):
            ok = ok & (axes[k - 1] < axes[k])
        _TUPLES[(nbins, m)] = tuple(t.astype(np.intp) for t in np.nonzero(np.broadcast_to(ok, tuple(nbins - m + k for k in range(m)))))
    return _TUPLES[(nbins, m)]


def sigmas(P1, S1, t, dt=np.float32):
    """between-class variance of every tuple of ``t`` with the sums in the restatement's order, in ``dt``"""
    nbins = P1.size - 1
    sigma = class_term(P1, S1, np.zeros_like(t[0]), t[0], dt) + class_term(P1, S1, t[-1] + 1, np.full_like(t[0], nbins - 1), dt)
    for k in range(len(t) - 1):
        sigma = (sigma + class_term(P1, S1, t[k] + 1, t[k + 1], dt)).astype(dt)
    return sigma


def multiotsu_indices(hist, classes):
    """threshold indices of the restatement for a histogram of any length; (indices, sigma of the winner or None)"""
    prob, P1, S1, nvalues = moments(hist)
    if nvalues < classes:
        raise ValueError(f"After discretization into bins, the input image has only {nvalues} different values. "
                         f"It cannot be thresholded in {classes} classes.")
    if nvalues == classes:
        return np.flatnonzero(prob)[:-1], None
    t = threshold_tuples(prob.size, classes - 1)
    sigma = sigmas(P1, S1, t)
    best = int(np.argmax(sigma))          # the first of the largest: what a strict > from 0 keeps
    if not sigma[best] > 0:
        return np.zeros(classes - 1, np.intp), np.float32(0)
    return np.array([tk[best] for tk in t], np.intp), sigma[best]


def threshold_multiotsu(image, classes=3, nbins=256):
    """the restatement end to end: float32 thresholds of a float32 image"""
    image = np.asarray(image)
    assert image.dtype == np.float32
    hist, edges = np.histogram(image.reshape(-1), nbins)
    centers = (edges[:-1] + edges[1:]) / 2
    idx, _ = multiotsu_indices(hist, classes)
    return centers[idx]


def estimate_bit_shift(img_log, threshold, percentile=99.9):
    """process_images.py:320-331; returns (bit shift, upper bound in counts)"""
    above = img_log[img_log > threshold]
    upper_bound = np.percentile(above, percentile) if above.size else np.max(img_log)
    upper_bound = int(np.round(np.expm1(upper_bound)))
    shift = 8
    for b in range(9):
        if 256 * 2 ** b >= upper_bound:
            shift = b
            break
    return shift, upper_bound


def estimate_slice_params(stack, need_bleach_correction=True):
    """process_images.py:594-655 on numpy's own log1p: dict of clips (float32), bit shift, dark, slices and the upper bounds"""
    nz = stack.shape[0]
    z = [math.floor(nz * 0.25), math.floor(nz * 0.5), math.floor(nz * 0.75)]
    shifts, bounds, clips = [], [], None
    for i in range(3):
        while True:
            try:
                img = stack[z[i]]
                assert not (img == img.flat[0]).all()
                img = np.log1p(img, dtype=np.float32)
                clips = threshold_multiotsu(img, classes=4)
                shift, bound = estimate_bit_shift(img, clips[2], 99.99)
                shifts.append(shift)
                bounds.append(bound)
                break
            except (ValueError, AssertionError):
                z[i] += 1
    return dict(clips=clips, bit_shift_to_right=max(shifts), dark=int(np.round(np.expm1(clips[0]))) if need_bleach_correction else 0,
                slices=z, upper_bounds=bounds)
