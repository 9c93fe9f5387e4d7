"""TEST INFRASTRUCTURE for the pystripe stage (tests/test_pystripe_host.py, tests/test_gpu_pystripe.py, the golden maker).

Two halves:

* ``install_standins`` / ``import_reference`` -- used by tests/golden/make_pystripe_golden.py ALONE (the reference tree is not
  present where the GPU tests run).  The reference's ``pystripe.core`` needs PyWavelets, scikit-image, OpenCV, numexpr, numba,
  tifffile, dcimg and imageio, none of which is installed; small stand-ins go into ``sys.modules`` so that its own
  ``process_img`` / ``filter_streaks`` / ``filter_subband`` / ``np_filter_coefficient`` run unmodified on the CPU (scipy.fftpack is
  present).  ``pywt.wavedec2 / waverec2`` are built from ``oracle.destripe_oracle``'s ``dwt_axis`` / ``idwt_axis`` and
  ``skimage.measure.block_reduce`` is six lines: these two are restatements (DWT parity unpinned, like the MATLAB destripe).

* the restatement -- plain numpy / scipy code written from the description of the stage (float32 or float64), with a
  vectorised db9 transform of its own (so it is independent of the loop-built one behind the goldens).  It must reproduce every
  golden on the CPU, and it is the live comparison for shapes that have no golden.
"""
from __future__ import annotations

import math
import sys
import types

import numpy as np
from scipy.fftpack import irfft, rfft

from oracle import destripe_oracle as _o

GOLDEN_SUBDIR = "pystripe"
PADDING_MODES = ("reflect", "wrap", "symmetric", "edge")


# ---------------------------------------------------------------------------------------------------------------------------------
# stand-ins (golden maker only)

def install_standins():
    def mod(name, **kw):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules[name] = m
        return m

    def missing(*a, **k):
        raise NotImplementedError("not available on this machine")

    def jit(*a, **k):
        if a and callable(a[0]):
            return a[0]
        return lambda f: f

    def evaluate(expr, out=None, casting=None, local_dict=None):
        f = sys._getframe(1)
        ns = dict(f.f_globals)
        ns.update(f.f_locals)
        ns.update(where=np.where, exp=np.exp, tanh=np.tanh, log1p=np.log1p, expm1=np.expm1)
        r = eval(expr, {}, ns)
        if out is not None:
            out[...] = np.asarray(r).astype(out.dtype)
            return out
        return r

    class Wavelet:
        def __init__(self, name):
            if name != "db9":
                raise ValueError("only db9 has a stand-in")
            self.dec_len = 18
            self.name = name

    def dwt_max_level(n, flen):
        if isinstance(flen, Wavelet):
            flen = flen.dec_len
        return max(int(math.floor(math.log2(n / (flen - 1)))), 0) if n >= flen - 1 else 0

    F = _o.db_filters(9)

    def wavedec2(data, wavelet, mode="symmetric", level=None, axes=(-2, -1)):
        assert mode == "symmetric" and tuple(axes) == (-2, -1)
        if level is None:
            level = min(dwt_max_level(s, 18) for s in data.shape[-2:])
        a, out = data, []
        for _ in range(level):
            lo1, hi1 = _o.dwt_axis(a, F[0], 1), _o.dwt_axis(a, F[1], 1)
            A, cH = _o.dwt_axis(lo1, F[0], 0), _o.dwt_axis(lo1, F[1], 0)
            cV, cD = _o.dwt_axis(hi1, F[0], 0), _o.dwt_axis(hi1, F[1], 0)
            out.append((cH, cV, cD))
            a = A
        return [a] + out[::-1]

    def waverec2(coeffs, wavelet, mode="symmetric", axes=(-2, -1)):
        a = coeffs[0]
        for cH, cV, cD in coeffs[1:]:
            a = a[:cH.shape[0], :cH.shape[1]]
            s0, s1 = 2 * cH.shape[0] - 16, 2 * cH.shape[1] - 16
            lo1 = _o.idwt_axis(a, cH, F[2], F[3], s0, 0)
            hi1 = _o.idwt_axis(cV, cD, F[2], F[3], s0, 0)
            a = _o.idwt_axis(lo1, hi1, F[2], F[3], s1, 1)
        return a

    mod("cv2", morphologyEx=missing, MORPH_CLOSE=0, MORPH_OPEN=1, floodFill=missing, GaussianBlur=lambda img, **k: None)
    mod("dcimg", DCIMGFile=object)
    mod("imageio")
    mod("imageio.v3", imread=missing)
    mod("numba", jit=jit, njit=jit)
    mod("numexpr", evaluate=evaluate)
    mod("ptwt", wavedec2=missing, waverec2=missing)
    mod("pywt", wavedec2=wavedec2, waverec2=waverec2, Wavelet=Wavelet, dwt_max_level=dwt_max_level)
    mod("skimage")
    mod("skimage.filters", threshold_otsu=missing, threshold_multiotsu=missing)
    mod("skimage.measure", block_reduce=block_reduce)
    mod("skimage.transform", resize=missing)
    mod("tifffile", imwrite=missing, imread=missing)
    mod("tifffile.tifffile", TiffFileError=OSError)


def import_reference(reference_root):
    install_standins()
    if reference_root not in sys.path:
        sys.path.insert(0, reference_root)
    import pystripe.core as pc
    return pc


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement

def block_reduce(img, block_size, func, cval=0):
    """skimage.measure.block_reduce: pad with ``cval`` up to a multiple of the block, reduce every block."""
    by, bx = block_size
    ny, nx = img.shape
    p = np.pad(img, ((0, (-ny) % by), (0, (-nx) % bx)), constant_values=cval)
    return func(p.reshape(p.shape[0] // by, by, p.shape[1] // bx, bx), axis=(1, 3))


def calculate_pad_size(shape, sigma, rise=0.5):
    """Padding of filter_streaks: the distance at which the notch 1 - exp(-j^2 / (2 sigma^2)) has risen to ``level``, to the nearest
    integer, made even downwards; ``level`` is ``rise`` or, if lower, the memory-bound level (budget 5e14) less 0.01."""
    if sigma == 0:
        return 0
    ny, nx = shape
    spread = math.hypot(nx - ny, 2 * math.sqrt(5e14))          # sqrt((nx - ny)^2 + 4 * 5e14)
    bound = round(-math.expm1((nx + ny + 2 - spread) / (4 * sigma * sigma)), 2) - 0.01
    distance = sigma * math.sqrt(-2 * math.log1p(-min(bound, rise)))
    return int(distance + 0.5) & ~1


def dwt_max_level(n, flen=18):
    return max(int(math.floor(math.log2(n / (flen - 1)))), 0) if n >= flen - 1 else 0


def geometry(shape, sigma, level=0):
    """(base_pad, pad_y, pad_x, padded shape, levels, [detail shapes finest first]) of filter_streaks for a tile of ``shape``."""
    ny, nx = shape
    bp = calculate_pad_size(shape, max(sigma))
    py, px = ny % 2, nx % 2
    if ny + 2 * bp + py < 34:
        py = 34 - (ny + 2 * bp)
    if nx + 2 * bp + px < 34:
        px = 34 - (nx + 2 * bp)
    H, W = ny + 2 * bp + py, nx + 2 * bp + px
    lev = level if level else min(dwt_max_level(H), dwt_max_level(W))
    shapes, h, w = [], H, W
    for _ in range(lev):
        h, w = (h + 17) // 2, (w + 17) // 2
        shapes.append((h, w))
    return bp, py, px, (H, W), lev, shapes


def down_sampled_size(shape, down_sample):
    return tuple(int(math.ceil(s / d)) for s, d in zip(shape, down_sample))


def _sym(j, n):
    j = np.mod(j, 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def _dwt_last(x, F):
    """analysis along the last axis: out[i] = sum_t F[t] x[sym(2 i + 1 - t)], one gather for all taps."""
    n = x.shape[-1]
    m = (n + 17) // 2
    ext = x[..., _sym(np.arange(-16, 2 * m), n)]            # ext[q] = x[sym(q - 16)]
    out = np.zeros(x.shape[:-1] + (m,), x.dtype)
    for t in range(18):
        out += x.dtype.type(F[t]) * ext[..., 17 - t:17 - t + 2 * m:2]
    return out


def _idwt_last(a, d, lo_r, hi_r):
    """synthesis along the last axis to 2 m - 16 samples: out[2p + e] = sum_q a[p + q] Lo_R[16 + e - 2 q] + d[p + q] Hi_R[...]."""
    m = a.shape[-1]
    P = m - 8
    out = np.zeros(a.shape[:-1] + (2 * P,), a.dtype)
    T = a.dtype.type
    for q in range(9):
        aa, dd = a[..., q:q + P], d[..., q:q + P]
        out[..., 0::2] += aa * T(lo_r[16 - 2 * q]) + dd * T(hi_r[16 - 2 * q])
        out[..., 1::2] += aa * T(lo_r[17 - 2 * q]) + dd * T(hi_r[17 - 2 * q])
    return out


def _t(x):
    return np.ascontiguousarray(np.swapaxes(x, -1, -2))


def notch(n, sigma, dt):
    g = np.arange(n, dtype=dt)
    return (dt(1) - np.exp(-g ** 2 / (dt(2) * dt(sigma) ** 2))).astype(dt)


def filter_coefficient(c, width_frac, axis, dt):
    """np_filter_coefficient: the notch multiplies scipy.fftpack.rfft's PACKED spectrum [r0, r1, i1, r2, i2, ...] by position."""
    sigma = c.shape[axis + 1] * width_frac
    g = notch(c.shape[axis], sigma, dt)
    if axis == -2:
        g = g.reshape(-1, 1)
    return irfft(rfft(c, axis=axis) * g, axis=axis).astype(dt)


def filter_subband(img, sigma, level, axes, dt):
    F = _o.db_filters(9)
    H, W = img.shape
    lev = level if level else min(dwt_max_level(H), dwt_max_level(W))
    a, det = img, []
    for _ in range(lev):
        lo1, hi1 = _dwt_last(a, F[0]), _dwt_last(a, F[1])                  # axis -1
        A, cH = _t(_dwt_last(_t(lo1), F[0])), _t(_dwt_last(_t(lo1), F[1]))  # axis -2
        cV, cD = _t(_dwt_last(_t(hi1), F[0])), _t(_dwt_last(_t(hi1), F[1]))
        det.append((cH, cV, cD))
        a = A
    for cH, cV, cD in det[::-1]:
        if -1 in axes:
            cH = filter_coefficient(cH, sigma / H, -1, dt)
        if -2 in axes:
            cV = filter_coefficient(cV, sigma / W, -2, dt)
        a = a[:cH.shape[0], :cH.shape[1]]
        lo1 = _t(_idwt_last(_t(a), _t(cH), F[2], F[3]))
        hi1 = _t(_idwt_last(_t(cV), _t(cD), F[2], F[3]))
        a = _idwt_last(lo1, hi1, F[2], F[3])
    return a.astype(dt)


def filter_streaks_log(img, sigma, level=0, padding_mode="reflect", bidirectional=False, dt=np.float32):
    """The log-domain image of filter_streaks just before expm1 (cropped to the tile)."""
    s1, s2 = sigma
    if (s1 > 0) != (s2 > 0):
        raise ValueError("np_notch: sigma must be positive")
    if padding_mode not in PADDING_MODES:
        raise RuntimeError(f"Unsupported padding mode: {padding_mode}")
    x = np.log1p(img.astype(dt))
    bp, py, px, _, _, _ = geometry(x.shape, sigma, level)
    ny, nx = x.shape
    x = np.pad(x, ((bp, bp + py), (bp, bp + px)), mode=padding_mode)
    axes = (-1, -2) if bidirectional else (-1,)
    x = filter_subband(x, s1, level, axes, dt)
    if s1 != s2:
        x = filter_subband(x, s2, level, axes, dt)
    return x[bp:bp + ny, bp:bp + nx]


def convert_to_8bit_fun(img, bit_shift_to_right=8):
    """8-bit conversion through a 65536-entry table: value >> shift limited to 255, except that 1 .. 2^shift - 1 map to 1."""
    if img.dtype == np.uint8:
        return img
    shift = 8 if bit_shift_to_right is None else bit_shift_to_right
    if shift < 0 or shift > 8:
        raise RuntimeError("right shift should be between 0 and 8")
    table = np.minimum(np.arange(65536) >> shift, 255).astype(np.uint8)
    table[1:1 << shift] = 1
    index = img if img.dtype == np.uint16 else np.clip(img, 0, 65535).astype(np.uint16)
    return table[index]


def process_img(img, flat=None, down_sample=None, down_sample_method="max", sigma=(0, 0), level=0, padding_mode="wrap",
                bidirectional=False, dark=0, rotate=0, flip_upside_down=False, convert_to_16bit=False, convert_to_8bit=False,
                bit_shift_to_right=8, d_type=None, dt=np.float32, flat_on_integers=False, **ignored):
    """Restatement of process_img for the options this project builds.  Returns (result, log-domain image or None).
    ``flat_on_integers``: divide an integer tile by the flat field in float32 (the project's stated departure; the reference raises)."""
    d_type = np.dtype(img.dtype if d_type is None else d_type)
    shape = img.shape
    if (img == img.flat[0]).all():
        if down_sample is not None:
            shape = down_sampled_size(shape, down_sample)
        if rotate in (90, 270):
            shape = shape[::-1]
        out_t = np.uint16 if convert_to_16bit else np.uint8 if convert_to_8bit else d_type
        return np.zeros(shape, out_t), None
    if flat is not None and flat.shape == img.shape:
        if img.dtype.kind in "ui":
            if not flat_on_integers:
                raise TypeError("in-place divide of an integer tile by a float flat field")
            img = img.astype(np.float32)
        img = img / flat
    if down_sample is not None:
        func = {"max": np.max, "min": np.min, "mean": np.mean}[down_sample_method.lower()]
        img = block_reduce(img, tuple(down_sample), func)
    logimg = None
    if tuple(sigma) > (0, 0):
        kind = img.dtype
        logimg = filter_streaks_log(img, tuple(sigma), level, padding_mode, bidirectional, dt)
        f = np.expm1(logimg).astype(dt)
        if kind.kind in "ui":
            f = np.clip(np.rint(f), np.iinfo(kind).min, np.iinfo(kind).max)
        img = f.astype(kind)
    if dark:
        above = img > dark
        img = (above * (img - dark)).astype(img.dtype) if dark > 0 else img
    if convert_to_16bit and img.dtype != np.uint16:
        img = np.clip(img, 0, 65535).astype(np.uint16)
    elif convert_to_8bit and img.dtype != np.uint8:
        img = convert_to_8bit_fun(img, bit_shift_to_right)
    elif d_type.kind in "ui":
        img = np.clip(img, np.iinfo(d_type).min, np.iinfo(d_type).max).astype(d_type)
    else:
        img = img.astype(d_type)
    if flip_upside_down:
        img = np.flipud(img)
    if rotate in (90, 180, 270):
        img = np.rot90(img, rotate // 90)
    return np.ascontiguousarray(img), logimg


# ---------------------------------------------------------------------------------------------------------------------------------
# the standards of the issue

def integer_allowance(golden, e_ref):
    """per-pixel allowance in counts: 1 + ceil(5 E_ref (v + 1))"""
    return 1 + np.ceil(5.0 * float(e_ref) * (golden.astype(np.float64) + 1.0))


def synthetic_tile(shape, seed, dtype=np.uint16, stripes="rows", amplitude=0.3):
    """A smooth blob on a pedestal with Poisson noise and a multiplicative gain per row (or column)."""
    rng = np.random.default_rng(seed)
    ny, nx = shape
    yy, xx = np.mgrid[:ny, :nx]
    img = 300 + 4000 * np.exp(-((yy - ny / 2) ** 2 + (xx - nx / 2) ** 2) / (0.03 * ny * nx + 1)) + rng.poisson(40, (ny, nx))
    if stripes == "rows":
        img = img * (1 + amplitude * rng.standard_normal(ny))[:, None]
    elif stripes == "cols":
        img = img * (1 + amplitude * rng.standard_normal(nx))[None, :]
    if np.dtype(dtype) == np.uint8:
        return np.clip(img / 20.0, 0, 255).astype(np.uint8)
    if np.dtype(dtype) == np.uint16:
        return np.clip(img, 0, 65535).astype(np.uint16)
    return np.clip(img, 0, None).astype(np.float32)
