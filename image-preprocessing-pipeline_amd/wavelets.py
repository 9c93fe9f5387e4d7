"""Orthogonal wavelets for the stripe filter of ``ipp_amd.pystripe``: what ``wavelet=`` may be and how it becomes coefficients.

A wavelet is its reconstruction low-pass ``rec_lo`` (PyWavelets' name), an even number of taps between 2 and ``MAX_TAPS``.  The
high-pass and the decomposition pair follow by the quadrature-mirror rule on the device side (include/mi_pystripe.h, "Wavelets").

    "db9"                                the pipeline's wavelet: the library's own kernels for 18 taps (``resolve`` returns None)
    "haar", "db1" .. "db20"              built here by spectral factorisation (``daubechies``)
    an object with a ``rec_lo`` attribute, or a 1-D sequence / array of rec_lo
                                         e.g. ``pywt.Wavelet("coif15")`` on the caller's side; PyWavelets is never imported here
    any other string                     NotImplementedError: the library holds no table for it (coiflets and symlets cannot be
                                         derived in closed form), and the message says that the coefficients can be passed instead
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

MAX_TAPS = 128              # MI_PS_MAX_TAPS
ORTHONORMAL_BOUND = 1e-6    # on max_k |sum_n h[n] h[n + 2 k] - delta_k|; rounding a true table to float32 moves it by about 1.2e-7
MAX_DAUBECHIES = 20         # the factorisation's own residual is <= 2.7e-13 up to here and 2.4e-7 at N = 38


@dataclass(frozen=True)
class OrthogonalWavelet:
    """The reconstruction low-pass of an orthogonal wavelet as a tuple of floats.  Equality and hash go by the coefficient values
    alone (never by identity, never by name), so it can key a cache of plans."""
    rec_lo: tuple
    name: str = field(default=None, compare=False)

    @property
    def taps(self):
        return len(self.rec_lo)

    def array(self):
        return np.array(self.rec_lo, dtype=np.float64)


def orthonormality_residual(rec_lo):
    """max over k of |sum_n h[n] h[n + 2 k] - delta_k|"""
    h = np.asarray(rec_lo, dtype=np.float64)
    worst = 0.0
    for k in range(len(h) // 2):
        s = float(np.dot(h[:len(h) - 2 * k], h[2 * k:]))
        worst = max(worst, abs(s - (1.0 if k == 0 else 0.0)))
    return worst


def orthogonal_wavelet(rec_lo, name=None):
    """The immutable object used inside for the wavelet with the reconstruction low-pass ``rec_lo``.  ValueError naming ``wavelet``
    for an odd or empty length, more than MAX_TAPS taps, a value that is not finite, or a low-pass that is not orthonormal under
    double shifts (a biorthogonal one is not)."""
    try:
        h = np.array(rec_lo, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"wavelet: rec_lo is not a sequence of numbers ({e})") from None
    if h.ndim != 1:
        raise ValueError(f"wavelet: rec_lo must be one-dimensional, got shape {h.shape}")
    if h.size < 2 or h.size % 2 or h.size > MAX_TAPS:
        raise ValueError(f"wavelet: rec_lo has {h.size} taps; an even number between 2 and {MAX_TAPS} is built")
    if not np.isfinite(h).all():
        raise ValueError("wavelet: rec_lo holds a value that is not finite")
    residual = orthonormality_residual(h)
    if residual > ORTHONORMAL_BOUND:
        raise ValueError(f"wavelet: rec_lo is not the low-pass of an orthogonal wavelet: max_k |sum_n h[n] h[n + 2 k] - delta_k| = "
                         f"{residual:.3g}, allowed {ORTHONORMAL_BOUND:g} (biorthogonal wavelets are not built)")
    return OrthogonalWavelet(tuple(float(v) for v in h), None if name is None else str(name))


def daubechies(N):
    """rec_lo of the Daubechies wavelet with N vanishing moments (2 N taps), float64: the extremal-phase spectral factor of the
    half-band polynomial P(y) = sum_k C(N - 1 + k, k) y^k, y = (2 - z - 1 / z) / 4, times (1 + z)^N, scaled to sum sqrt(2)."""
    N = int(N)
    if N < 1:
        raise ValueError(f"wavelet: db{N} does not exist")
    if N == 1:
        return np.array([1.0, 1.0]) / math.sqrt(2.0)
    inside = []
    for y in np.roots([math.comb(N - 1 + k, k) for k in range(N)][::-1]):
        b = 2.0 - 4.0 * y                                  # z^2 - b z + 1 = 0: the root inside the unit circle
        d = np.sqrt(b * b - 4.0 + 0j)
        z = (b + d) / 2.0
        inside.append(z if abs(z) < 1 else (b - d) / 2.0)
    h = np.real(np.poly(np.concatenate([np.full(N, -1.0), np.array(inside)])))
    return h * (math.sqrt(2.0) / h.sum())


def _refuse_name(name):
    raise NotImplementedError(f"wavelet={name!r}: the library holds no table for this name (built in: 'haar', 'db1' .. 'db{MAX_DAUBECHIES}'); "
                              f"pass the coefficients instead, e.g. wavelet=pywt.Wavelet({name!r}) on the caller's side: any object with a "
                              f"rec_lo attribute, or the reconstruction low-pass itself as a sequence of up to {MAX_TAPS} values, is taken")


_built = {}


def resolve(wavelet):
    """None for "db9" (the library's own 18-tap kernels), else the OrthogonalWavelet that ``wavelet`` stands for.  Needs no device."""
    if isinstance(wavelet, OrthogonalWavelet):
        return wavelet
    if isinstance(wavelet, str):
        name = wavelet.lower()
        if name == "db9":
            return None
        order = 1 if name == "haar" else int(name[2:]) if name.startswith("db") and name[2:].isdigit() else 0
        if not 1 <= order <= MAX_DAUBECHIES:
            _refuse_name(wavelet)
        if order not in _built:
            _built[order] = orthogonal_wavelet(daubechies(order), f"db{order}")
        return _built[order]
    if wavelet is None:
        raise ValueError("wavelet=None: a name, an object with rec_lo, or the coefficients are expected")
    if hasattr(wavelet, "rec_lo"):
        return orthogonal_wavelet(wavelet.rec_lo, getattr(wavelet, "name", None))
    return orthogonal_wavelet(wavelet)


def load_file(path):
    """rec_lo from a ``.npy`` file or a text file of numbers (any white space or commas between them)."""
    path = str(path)
    if path.lower().endswith(".npy"):
        values = np.load(path, allow_pickle=False)
    else:
        with open(path) as f:
            values = np.array([float(v) for v in f.read().replace(",", " ").split()])
    return orthogonal_wavelet(np.ravel(values), name=path)
