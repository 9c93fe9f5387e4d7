"""TEST INFRASTRUCTURE for the stripe filter with any orthogonal wavelet (tests/test_wavelets_host.py,
tests/test_gpu_pystripe_wavelets.py).

* the restatement: ``filter_streaks``' log-domain image in float32 or float64 for ANY filter set, from the pieces that exist:
  ``tests/pystripe_util`` (pad size, padding, the packed-position notch, the tail of process_img, the standards) and
  ``oracle.destripe_oracle``'s ``dwt_axis`` / ``idwt_axis``, which are written for any filter length and extend symmetrically over
  any distance.  PyWavelets' bookkeeping for L taps: an extent n gives (n + L - 1) / 2 coefficients, m coefficients give back
  2 m - L + 2 samples, the automatic level is min over both extents of floor(log2(n / (L - 1))) and 0 below L - 1 samples -- the
  approximation alone comes back and the image is unchanged.
* ``lattice_filter``: a seeded orthonormal low-pass of any even length from a paraunitary lattice.  It stands in for the LENGTH of
  wavelets whose tables are not on these machines (coif15: 90 taps); it has none of their vanishing moments.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import destripe_oracle as _o
from tests import bleach_util as B
from tests import pystripe_util as U


def filters_from_rec_lo(rec_lo):
    """(Lo_D, Hi_D, Lo_R, Hi_R), float64, by the quadrature-mirror rule: Hi_R[t] = (-1)^t Lo_R[L - 1 - t], decomposition = reversed"""
    lo_r = np.asarray(rec_lo, dtype=np.float64)
    hi_r = lo_r[::-1].copy()
    hi_r[1::2] = -hi_r[1::2]
    return lo_r[::-1].copy(), hi_r[::-1].copy(), lo_r, hi_r


def orthonormality_residual(h):
    h = np.asarray(h, dtype=np.float64)
    return max(abs(float(np.dot(h[:len(h) - 2 * k], h[2 * k:])) - (1.0 if k == 0 else 0.0)) for k in range(len(h) // 2))


def lattice_filter(taps, seed):
    """Orthonormal low-pass of ``taps`` (even) coefficients: taps / 2 rotations R_i by angles uniform in +-0.5 rad, the first shifted
    so that they sum to pi / 4 (then sum h = sqrt(2)), E(z) = R_K diag(1, 1/z) R_{K-1} ... diag(1, 1/z) R_0, and
    h[2 i] = E_00[i], h[2 i + 1] = E_01[i].  Every factor is paraunitary, so sum_n h[n] h[n + 2 k] = delta_k to rounding."""
    assert taps >= 2 and taps % 2 == 0
    rng = np.random.default_rng(seed)
    angles = rng.uniform(-0.5, 0.5, taps // 2)
    angles[0] += math.pi / 4 - angles.sum()

    def rot(a):
        return np.array([[math.cos(a), math.sin(a)], [-math.sin(a), math.cos(a)]])

    E = rot(angles[0])[:, :, None]                      # E[r, c, power of 1/z]
    for a in angles[1:]:
        D = np.zeros((2, 2, E.shape[2] + 1))
        D[0, :, :-1] = E[0]                             # diag(1, 1/z): the second row moves one power on
        D[1, :, 1:] = E[1]
        E = np.einsum("ij,jkp->ikp", rot(a), D)
    h = np.empty(taps)
    h[0::2], h[1::2] = E[0, 0], E[0, 1]
    return h


def max_level(n, taps):
    return max(int(math.floor(math.log2(n / (taps - 1)))), 0) if taps > 1 and n >= taps - 1 else 0


def geometry(shape, sigma, taps, level=0):
    """(base_pad, pad_y, pad_x, padded shape, levels, [detail shapes finest first]) for a wavelet of ``taps`` coefficients: the pad
    and the 34-sample rule do not depend on it."""
    ny, nx = shape
    bp = U.calculate_pad_size(shape, max(sigma))
    py, px = ny % 2, nx % 2
    if ny + 2 * bp + py < 34:
        py = 34 - (ny + 2 * bp)
    if nx + 2 * bp + px < 34:
        px = 34 - (nx + 2 * bp)
    H, W = ny + 2 * bp + py, nx + 2 * bp + px
    lev = level if level else min(max_level(H, taps), max_level(W, taps))
    shapes, h, w = [], H, W
    for _ in range(lev):
        h, w = (h + taps - 1) // 2, (w + taps - 1) // 2
        shapes.append((h, w))
    return bp, py, px, (H, W), lev, shapes


def filter_subband(img, F, sigma, level, axes, dt):
    H, W = img.shape
    L = len(F[0])
    lev = level if level else min(max_level(H, L), max_level(W, L))
    a, det = img, []
    for _ in range(lev):
        lo1, hi1 = _o.dwt_axis(a, F[0], 1), _o.dwt_axis(a, F[1], 1)
        A, cH = _o.dwt_axis(lo1, F[0], 0), _o.dwt_axis(lo1, F[1], 0)
        cV, cD = _o.dwt_axis(hi1, F[0], 0), _o.dwt_axis(hi1, F[1], 0)
        det.append((cH, cV, cD))
        a = A
    for cH, cV, cD in det[::-1]:
        if -1 in axes:
            cH = U.filter_coefficient(cH, sigma / H, -1, dt)
        if -2 in axes:
            cV = U.filter_coefficient(cV, sigma / W, -2, dt)
        a = a[:cH.shape[0], :cH.shape[1]]
        s0, s1 = 2 * cH.shape[0] - L + 2, 2 * cH.shape[1] - L + 2
        lo1 = _o.idwt_axis(a, cH, F[2], F[3], s0, 0)
        hi1 = _o.idwt_axis(cV, cD, F[2], F[3], s0, 0)
        a = _o.idwt_axis(lo1, hi1, F[2], F[3], s1, 1)
    return a.astype(dt)


def filter_streaks_log(img, rec_lo, sigma, level=0, padding_mode="reflect", bidirectional=False, dt=np.float32):
    """The log-domain image of filter_streaks just before expm1 (cropped to the tile) for the wavelet ``rec_lo``."""
    F = filters_from_rec_lo(rec_lo)
    s1, s2 = sigma
    x = np.log1p(img.astype(dt))
    bp, py, px, _, _, _ = geometry(x.shape, sigma, len(rec_lo), level)
    ny, nx = x.shape
    x = np.pad(x, ((bp, bp + py), (bp, bp + px)), mode=padding_mode)
    axes = (-1, -2) if bidirectional else (-1,)
    x = filter_subband(x, F, s1, level, axes, dt)
    if s1 != s2:
        x = filter_subband(x, F, s2, level, axes, dt)
    return x[bp:bp + ny, bp:bp + nx]


def process_img(img, rec_lo, sigma, level=0, padding_mode="wrap", bidirectional=False, dt=np.float32, bleach=None, **tail):
    """(result, log-domain image): the stripe filter with ``rec_lo``, the bleach correction (``bleach``: the keywords of
    ``bleach_util.correct_bleaching``), expm1, rint + clip for integer tiles, then the tail of ``pystripe_util.process_img`` (dark,
    conversions, flip, rotation)."""
    kind = img.dtype
    L = filter_streaks_log(img, rec_lo, sigma, level, padding_mode, bidirectional, dt)
    if bleach is not None:
        L = B.correct_bleaching(L, dt=dt, **bleach)
    f = np.expm1(L).astype(dt)
    if kind.kind in "ui":
        f = np.clip(np.rint(f), np.iinfo(kind).min, np.iinfo(kind).max)
    out, _ = U.process_img(f.astype(kind), dt=dt, **tail)
    return out, L


def reference(img, rec_lo, **kw):
    """(float32 result, float64 log image, E_ref): E_ref is the float32 restatement's own distance from the float64 one."""
    r32, l32 = process_img(img.copy(), rec_lo, dt=np.float32, **kw)
    _, l64 = process_img(img.copy(), rec_lo, dt=np.float64, **kw)
    return r32, l64, float(np.abs(l32.astype(np.float64) - l64).max())
