#!/usr/bin/env python3
"""pystripe tile preprocessing on the GPU: ``pystripe.core`` of the reference for the options ``process_images.py`` uses
(``process_images.py:420-447`` on raw tiles, ``:702-724`` on merged slices).

    from ipp_amd.pystripe import batch_filter
    batch_filter(input_path, output_path, sigma=(250, 250), wavelet="db9", padding_mode="reflect", bidirectional=True, ...)

``batch_filter`` is the drop-in boundary: the reference's keyword names and defaults, returns 0.  ``process_img`` and
``filter_streaks`` take one 2-D tile (numpy array or device tensor) like the reference, or a stack ``[n, ny, nx]`` of equally shaped
tiles, which go through every kernel launch together (include/mi_pystripe.h).  There is no CPU path: a missing library or device is
an error.

What is computed (reference line numbers in include/mi_pystripe.h): uniform tile -> zeros; flat field; ``down_sample`` (max / min /
mean / median, zero-padded blocks like skimage's ``block_reduce``); ``filter_streaks`` = log1p, numpy padding (reflect / wrap / symmetric /
edge as index maps of the first wavelet level; with ``extended=True`` also constant / linear_ramp / maximum / mean / median / minimum,
for which the row and column statistics of the log image and the padded image itself are made on the device; the constant is 0 or
log1p of ``bleach_correction_clip_min`` -- given, or the tile's own estimate), wavelet decomposition (``wavelet=``: 'db9', the pipeline's choice; 'haar' / 'db1' .. 'db20'; or any orthogonal wavelet of up
to 128 taps as an object with ``rec_lo`` -- ``pywt.Wavelet("coif15")`` -- or the coefficients themselves; ``wavelets.py``), the
packed-position Gaussian notch on cH (and cV when ``bidirectional``), reconstruction, crop,
bleach correction (``bleach_correction_frequency`` with the three clips in log1p units, each given or, when None, estimated per tile
on the device by the four-class multi-Otsu of the log image as the reference does: the log-domain image divided by a
zero-phase first-order Butterworth low-pass of its clipped copy -- row by row, or, with ``bleach_correction_max_method``, the outer
product of the filtered row and column maxima -- and rescaled by that copy's maximum; it also runs alone, at ``sigma=(0, 0)``),
expm1, rint + clip for integer tiles; ``dark``; ``lightsheet`` (pystripe/lightsheet_correct.py: local percentiles on two sub-grids,
order-1 resampling, subtraction; include/mi_lightsheet.h); in ``batch_filter`` the resize to ``new_size`` (order-1 zoom and clip,
include/mi_tile_resize.h; ``resize_tiles`` runs it alone); 8 / 16-bit conversion; flip; rotation.

Departures, all stated in INTEGRATION.md:
  * ``flat`` on an integer tile: the reference's in-place divide raises; here the tile is divided in float32 and is a float tile from
    there on (the float32-tile case matches the reference);
  * ``gaussian_filter_2d`` is accepted and does nothing, as in the reference (its GaussianBlur result is discarded);
  * ``lightsheet=True`` on a tile narrower than ``artifact_length`` or with an extent below 25 is refused (the reference returns
    zeros for a uniform such tile and divides by zero otherwise);
  * ``extended=True`` (``process_img``, ``filter_streaks``, ``batch_filter``, ``make_params``; default False) opens what these entry
    points refused by name before it existed and still refuse without it: a frequency without all three clips (the missing ones are
    then estimated per tile), ``down_sample_method='median'``, ``new_size`` in ``process_img``, a ``threshold``, the six value modes
    of ``padding_mode``, ``enable_masking`` in ``filter_streaks`` (``get_img_mask``: threshold at ``bleach_correction_clip_med``, close,
    open, corner flood fill; include/mi_tile_mask.h states the box window -- an even box moves content by one sample, as OpenCV's
    documented formula does; agreement with cv2 itself is not verified);
  * refused by name also with it: ``exclude_dark_edges_set_them_to_zero``,
    a ``new_size`` that needs skimage's Gaussian pre-filter (the tile
    shape below ``new_size`` as tuples with an axis that shrinks) or meets an integer tile with a float ``d_type``, ``.dcimg`` input,
    a median ``down_sample`` over blocks of more than 64 samples, a wavelet NAME without a built-in table (``'coif15'``: hand in
    the coefficients instead), biorthogonal wavelets, ``padding_mode='empty'``, a ``threshold`` of 0 or less with ``sigma1 == 0``
    (a ``threshold`` above 0 has no effect: ``use_thresholding`` is never set on this path, nor has ``crossover``; 0 or less runs the
    single ``sigma1`` pass);
  * accepted and ignored: ``workers``, ``threads_per_gpu``, ``timeout``, ``gpu_semaphore``, ``z_step``, ``print_input_file_names``,
    ``verbose``.
The command line takes the reference's LONG option names with plain ``store_true`` flags (the bleach options, which the reference's
parser lacks, are named after the keywords); the reference's own parser cannot be built
(``-w`` is given to two options), so the CLI is not claimed as a byte-for-byte drop-in.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys
import warnings
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = "ipp_amd"

from . import capi, wavelets  # noqa: E402

_NP_CODES = {np.dtype(np.uint8): capi.PS_U8, np.dtype(np.uint16): capi.PS_U16, np.dtype(np.float32): capi.PS_F32}
_CODE_NP = {v: k for k, v in _NP_CODES.items()}
SUPPORTED_EXTENSIONS = (".tif", ".tiff", ".raw", ".png")


# ---------------------------------------------------------------------------------------------------------------------------------
# small host functions of the reference

def calculate_pad_size(shape, sigma, rise=0.5):
    """Rows / columns of padding around a tile of ``shape`` = (ny, nx) for a notch of width ``sigma`` (what pystripe/core.py:681 and
    :670 compute; ``mi_pystripe_pad_size`` is the same in C).  The Gaussian notch ``1 - exp(-j^2 / (2 sigma^2))`` reaches the level
    ``r`` at ``j = sigma * sqrt(-2 ln(1 - r))``; the pad is that distance rounded to the nearest integer and then down to an even
    one.  ``r`` is ``rise`` unless the reference's memory bound is lower: with ``u = nx + 1``, ``v = ny + 1`` and the budget 5e14,
    ``1 - exp((u + v - sqrt((u - v)^2 + 4 * 5e14)) / (4 sigma^2))`` rounded to two decimals, less 0.01."""
    if not sigma:
        return 0
    u, v, budget = shape[1] + 1, shape[0] + 1, 5e14
    exponent = (u + v - math.sqrt((u - v) ** 2 + 4 * budget)) / (4 * sigma ** 2)
    level = min(rise, round(1 - math.exp(exponent), 2) - 0.01)
    reach = math.sqrt(-2 * sigma ** 2 * math.log(1 - level))
    return 2 * (int(reach + 0.5) // 2)


def calculate_down_sampled_size(tile_size, down_sample):
    """Shape after ``down_sample``: every extent divided by its block, rounded up (pystripe/core.py:1162)."""
    return tuple(int(s) if d is None else -(-int(s) // int(d)) for s, d in zip(tile_size, down_sample))


def normalize_flat(flat):
    """The flat field as float32 with its largest value scaled to 1 (pystripe/core.py:2047)."""
    out = np.array(flat, dtype=np.float32)
    np.divide(out, out.max(), out=out)
    return out


def convert_to_16bit_fun(img):
    """Values limited to 0 .. 65535, then truncated to uint16 (pystripe/core.py:397)."""
    return np.minimum(np.maximum(img, 0), 65535).astype(np.uint16)


def convert_to_8bit_fun(img, bit_shift_to_right=8):
    """A uint16 image (anything else goes through ``convert_to_16bit_fun`` first) shifted right by 0 .. 8 bits and limited to 255; a
    value that is not zero never becomes zero: it becomes 1 (pystripe/core.py:402).  uint8 input is returned as it is.  Host arrays;
    the device path does the same inside its store."""
    shift = 8 if bit_shift_to_right is None else int(bit_shift_to_right)
    if img is None or img.dtype == np.uint8:
        return img
    if shift not in range(9):
        raise RuntimeError(f"right shift should be between 0 and 8 (bit_shift_to_right={bit_shift_to_right})")
    wide = img if img.dtype == np.uint16 else convert_to_16bit_fun(img)
    out = np.minimum(wide >> shift, 255).astype(np.uint8)
    out[(wide > 0) & (out == 0)] = 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# options -> mi_pystripe_params

def _refuse(name, value, why):
    raise NotImplementedError(f"{name}={value!r}: {why}")


def _check_padding(padding_mode, extended):
    """Raises NotImplementedError for a mode of numpy.pad this build does not do: 'empty' always (the reference then filters
    uninitialised memory), the six value modes without ``extended=True``."""
    mode = padding_mode.lower() if isinstance(padding_mode, str) else padding_mode
    if mode == "empty" or (mode in capi.PS_VALUE_PADDING and not extended):
        _refuse("padding_mode", padding_mode, "reflect, wrap, symmetric and edge are built" if not extended else
                "the reference pads with uninitialised memory; every other mode of numpy.pad is built")


def _check_unsupported(kw):
    """Raises NotImplementedError naming the first option this build does not do.  Without ``extended=True`` that includes what the
    entry points refused before the option existed: a frequency without all three clips, ``new_size`` in ``process_img``, a
    ``threshold``."""
    if not kw.get("extended"):
        if kw.get("bleach_correction_frequency") is not None and any(kw.get(name) is None for name in BLEACH_CLIPS):
            _refuse("bleach_correction_frequency", kw["bleach_correction_frequency"],
                    "bleach_correction_clip_min / _med / _max must be given: the clips that are left out are estimated per tile "
                    "(threshold_multiotsu of the log image) with extended=True only")
        if kw.get("new_size") is not None:
            _refuse("new_size", kw["new_size"], "process_img resizes with extended=True only; batch_filter (and resize_tiles) do")
        if kw.get("threshold") is not None:
            _refuse("threshold", kw["threshold"], "accepted with extended=True only (the thresholding dual-band path is not built)")
    for name in ("enable_masking", "exclude_dark_edges_set_them_to_zero"):
        if kw.get(name) and not (name == "enable_masking" and kw.get("extended")):
            _refuse(name, kw[name], "not built (needs OpenCV / scikit-image semantics)")
    threshold = kw.get("threshold")
    if threshold is not None and threshold <= 0 and "sigma" in kw:
        s1, s2 = _sigma_pair(kw["sigma"])
        if s1 == 0 and s2 != 0:
            _refuse("threshold", threshold, f"with sigma={kw['sigma']!r} the reference runs filter_subband at sigma 0; not built")
    if "padding_mode" in kw and _sigma_pair(kw.get("sigma", (0, 0))) > (0, 0):
        _check_padding(kw["padding_mode"], kw.get("extended"))
    if kw.get("log1p_normalization_needed") is False:
        _refuse("log1p_normalization_needed", False, "only the log1p path is built")


BLEACH_CLIPS = ("bleach_correction_clip_min", "bleach_correction_clip_med", "bleach_correction_clip_max")
_FLOATS = (float, np.float32, np.float64)


def check_bleach(shape, frequency, clip_min, clip_med, clip_max, max_method=False, down_sample=None):
    """What the reference raises for these bleach-correction arguments on a tile of ``shape``, from the values alone: the asserts of
    correct_bleaching (pystripe/core.py:524-528) as AssertionError, then butter's ValueError for a frequency of 1 or more, then
    sosfiltfilt's for a filtered line of 6 samples or fewer (the rows; with ``max_method`` also the column of row maxima).  A clip
    that is None is estimated per tile on the device (``threshold_multiotsu`` of the log image): the checks that involve it run
    there, on the estimate; those between given clips run here."""
    def require(ok, what):
        if not ok:
            raise AssertionError(what)
    require(isinstance(frequency, _FLOATS) and frequency > 0, f"bleach_correction_frequency={frequency!r}: a float above 0 is expected")
    if clip_min is not None:
        require(isinstance(clip_min, _FLOATS) and clip_min >= 0, f"bleach_correction_clip_min={clip_min!r}: a float, 0 or more, is expected")
    if clip_med is not None:
        require(isinstance(clip_med, _FLOATS) and (clip_min is None or clip_med > clip_min),
                f"bleach_correction_clip_med={clip_med!r}: a float above bleach_correction_clip_min={clip_min!r} is expected")
    if clip_max is not None:
        require(isinstance(clip_max, _FLOATS) and (clip_min is None or clip_max > clip_min),
                f"bleach_correction_clip_max={clip_max!r}: a float above bleach_correction_clip_min={clip_min!r} is expected")
        require(clip_med is None or clip_max > clip_med,
                f"bleach_correction_clip_max={clip_max!r} is not above bleach_correction_clip_med={clip_med!r}")
    if not frequency < 1:
        raise ValueError(f"Digital filter critical frequencies must be 0 < Wn < 1 (bleach_correction_frequency={frequency!r})")
    shape = tuple(int(v) for v in shape[-2:])
    if down_sample is not None:
        shape = calculate_down_sampled_size(shape, down_sample)
    for n in (shape if max_method else shape[1:]):
        if n <= 6:
            raise ValueError(f"The length of the input vector x must be greater than padlen, which is 6. (bleach correction filters a "
                             f"line of {n} samples of a tile of shape {shape})")


def _bleach_opts(shape, down_sample, frequency, max_method, clip_min, clip_med, clip_max):
    """The bleach keywords of make_params, after the checks that need no device.  Without a frequency only a given ``clip_min``
    is kept: padding_mode='constant' pads with it whether or not the correction runs."""
    if frequency is None:
        return {} if clip_min is None else dict(bleach_correction_clip_min=clip_min)
    check_bleach(shape, frequency, clip_min, clip_med, clip_max, max_method, down_sample)
    return dict(bleach_correction_frequency=frequency, bleach_correction_max_method=max_method, bleach_correction_clip_min=clip_min,
                bleach_correction_clip_med=clip_med, bleach_correction_clip_max=clip_max)


def _sigma_pair(sigma):
    """(sigma1, sigma2) as floats; a single number stands for both."""
    try:
        first, second = sigma
    except TypeError:
        first = second = sigma
    return float(first), float(second)


def _early_wavelet(sigma, wavelet):
    """``wavelet`` as make_params will take it, resolved from the values alone before anything touches the device: "db9" stays the
    name (the library's own route), everything else becomes its OrthogonalWavelet or raises.  Without a filter nothing is looked at."""
    if _sigma_pair(sigma) > (0, 0):
        found = wavelets.resolve(wavelet)
        return "db9" if found is None else found
    return wavelet


def _dtype_code(dt, what):
    dt = np.dtype(dt)
    if dt not in _NP_CODES:
        raise TypeError(f"{what}={dt.name}: uint8, uint16 and float32 are built")
    return _NP_CODES[dt]


def make_params(in_dtype, flat=False, down_sample=None, down_sample_method="max", sigma=(0, 0), level=0, wavelet="db9",
                padding_mode="reflect", bidirectional=False, dark=0, rotate=0, flip_upside_down=False, convert_to_16bit=False,
                convert_to_8bit=False, bit_shift_to_right=8, d_type=None, log_output=False, keep_uniform=False, max_batch=0,
                bleach_correction_frequency=None, bleach_correction_max_method=False, bleach_correction_clip_min=None,
                bleach_correction_clip_med=None, bleach_correction_clip_max=None, extended=False):
    """mi_pystripe_params for process_img's options.  Everything the C side cannot name itself is refused here.  ``extended=True``
    takes a clip that is None (NaN in the struct: estimated per tile), the median down-sampling and the value modes of numpy.pad
    (``padding_mode`` 'constant', 'linear_ramp', 'maximum', 'mean', 'median', 'minimum'; ``bleach_correction_clip_min`` is the constant's
    source also without a frequency)."""
    s1, s2 = _sigma_pair(sigma)
    filt = (s1, s2) > (0, 0)
    wobj = None
    if filt:
        wobj = wavelets.resolve(wavelet)   # None: 'db9', the library's own 18-tap kernels
        if (s1 > 0) != (s2 > 0) or s1 < 0 or s2 < 0:
            raise ValueError(f"np_notch: sigma must be positive (sigma={sigma!r})")
        mode = padding_mode.lower() if isinstance(padding_mode, str) else padding_mode
        _check_padding(padding_mode, extended)
        if mode not in capi.PS_PADDING:
            print(f"Unsupported padding mode: {padding_mode}")
            raise RuntimeError(f"Unsupported padding mode: padding_mode={padding_mode!r}")
    else:
        s1 = s2 = 0.0
        mode = "reflect"
    p = capi.PystripeParams()
    p.sigma1, p.sigma2, p.level = s1, s2, int(level)
    p.padding_mode = capi.PS_PADDING[mode]
    if mode == "constant" and bleach_correction_clip_min is not None:
        # the C side pads with log1p of this field also without a frequency (the clip is in log units already: the reference's double
        # log, pystripe/core.py:1101-1105, is mirrored).  With a frequency the field is set below: NaN for a minimum estimated per tile
        if not float(bleach_correction_clip_min) >= 0:
            raise ValueError(f"bleach_correction_clip_min={bleach_correction_clip_min!r}: padding_mode='constant' pads with log1p of it; "
                             "0 or more is expected")
        p.bleach_clip_min = float(bleach_correction_clip_min)
    p.bidirectional = int(bool(bidirectional))
    if down_sample is not None:
        method = str(down_sample_method).lower()
        if method == "median" and not extended:
            _refuse("down_sample_method", down_sample_method, "max, min and mean are built; the median with extended=True")
        if method not in capi.PS_DOWN:
            print(f"unsupported down-sampling method: {down_sample_method}")
            raise RuntimeError(f"unsupported down-sampling method: down_sample_method={down_sample_method!r}")
        p.down_y, p.down_x = (int(d) if d is not None else 1 for d in down_sample)
        p.down_method = capi.PS_DOWN[method]
        if method == "median" and p.down_y * p.down_x > capi.PS_MEDIAN_MAX_BLOCK:
            _refuse("down_sample", down_sample, f"down_sample_method='median' is built for blocks of up to {capi.PS_MEDIAN_MAX_BLOCK} samples")
    p.use_flat = int(bool(flat))
    p.dark = float(dark) if dark is not None and dark > 0 else 0.0
    if convert_to_16bit and convert_to_8bit:
        raise TypeError("convert_to_16bit and convert_to_8bit are both set")
    bit_shift_to_right = 8 if bit_shift_to_right is None else bit_shift_to_right
    if convert_to_8bit and bit_shift_to_right not in range(9):
        raise RuntimeError(f"right shift should be between 0 and 8 (bit_shift_to_right={bit_shift_to_right})")
    p.convert_to_16bit, p.convert_to_8bit, p.bit_shift = int(bool(convert_to_16bit)), int(bool(convert_to_8bit)), int(bit_shift_to_right)
    if rotate not in (0, 90, 180, 270):
        rotate = 0   # the reference rotates for 90 / 180 / 270 and leaves every other value alone
    p.rotate, p.flip_upside_down = int(rotate), int(bool(flip_upside_down))
    if convert_to_16bit:
        out = np.uint16
    elif convert_to_8bit:
        out = np.uint8
    else:
        out = in_dtype if d_type is None else d_type
    p.out_dtype = _dtype_code(out, "d_type")
    p.log_output, p.keep_uniform, p.max_batch = int(bool(log_output)), int(bool(keep_uniform)), int(max_batch)
    if bleach_correction_frequency is not None:
        clips = dict(bleach_correction_clip_min=bleach_correction_clip_min, bleach_correction_clip_med=bleach_correction_clip_med,
                     bleach_correction_clip_max=bleach_correction_clip_max)
        _check_unsupported(dict(clips, bleach_correction_frequency=bleach_correction_frequency, extended=extended))
        p.bleach_frequency = float(bleach_correction_frequency)
        p.bleach_clip_min, p.bleach_clip_med, p.bleach_clip_max = (math.nan if clips[name] is None else float(clips[name]) for name in BLEACH_CLIPS)
        p.bleach_max_method = int(bool(bleach_correction_max_method))
    p.wavelet = wobj   # a Python attribute beside the C fields: None, or the OrthogonalWavelet that derive / Plan hand to the C side
    return p


def orthogonal_wavelet(rec_lo, name=None):
    """The small immutable object ``wavelet=`` stands for inside (``wavelets.OrthogonalWavelet``), from the reconstruction low-pass
    coefficients -- what ``pywt.Wavelet(name).rec_lo`` holds.  ValueError naming ``wavelet`` when they are not an orthogonal wavelet
    of 2 .. 128 taps."""
    return wavelets.orthogonal_wavelet(rec_lo, name)


def plan_key(shape, in_dtype, params):
    """What identifies a plan: shape, dtype, every field of ``params`` and the wavelet's coefficient VALUES (two objects with equal
    coefficients give equal keys; the object's identity and name do not enter)."""
    w = getattr(params, "wavelet", None)
    return (int(shape[0]), int(shape[1])), np.dtype(in_dtype).name, bytes(params), None if w is None else w.rec_lo


def derive(shape, in_dtype, params):
    """The bookkeeping of a plan without a device (pad, padded shape, levels, coefficient shapes, output shape and type)."""
    info = capi.PystripeInfo()
    w = getattr(params, "wavelet", None)
    args = (int(shape[0]), int(shape[1]), _dtype_code(in_dtype, "dtype"), C.byref(params))
    if w is None:
        capi.check(capi.lib().mi_pystripe_derive(*args, C.byref(info)))
    else:
        capi.check(capi.lib().mi_pystripe_derive_wavelet(*args, w.taps, C.byref(info)))
    return info


class Plan:
    """mi_pystripe plan for tiles of one shape and dtype.  ``run(tiles[, flat])``: [n, ny, nx] device tensor -> result tensor."""

    def __init__(self, device, shape, in_dtype, params):
        import torch
        capi.require_gpu()
        self.device = torch.device(device if device is not None else "cuda:0")
        self.shape, self.in_dtype, self.params = (int(shape[0]), int(shape[1])), np.dtype(in_dtype), params
        self._h = C.c_void_p()
        self.wavelet = getattr(params, "wavelet", None)
        args = (self.device.index or 0, self.shape[0], self.shape[1], _dtype_code(in_dtype, "dtype"), C.byref(params))
        if self.wavelet is None:
            capi.check(capi.lib().mi_pystripe_plan_create(*args, C.byref(self._h)))
        else:
            rec_lo = (C.c_double * self.wavelet.taps)(*self.wavelet.rec_lo)
            capi.check(capi.lib().mi_pystripe_plan_create_wavelet(*args, rec_lo, self.wavelet.taps, C.byref(self._h)))
        self.info = capi.PystripeInfo()
        capi.check(capi.lib().mi_pystripe_plan_info(self._h, C.byref(self.info)))
        self.out_shape = (self.info.out_ny, self.info.out_nx)
        self.out_dtype = _CODE_NP[self.info.out_dtype]
        self._last_n = 0
        if params.bleach_auto and self.info.integer_kind:
            # numpy's float32 log1p of every code decides the bins of the automatic clips, not the device's log1pf
            from .thresholds import log_table
            table = np.ascontiguousarray(log_table(256 if self.in_dtype == np.uint8 else 65536), dtype=np.float32)
            capi.check(capi.lib().mi_pystripe_plan_set_log_table(self._h, table.ctypes.data, table.size))

    def notch_routes(self):
        """The notch kernel's route per (pass, level, axis) as mi_pystripe_plan_notch_routes reports it, in the plan's order: dicts
        of capi.PS_NOTCH_ROUTE (``R`` lines per work-group, ``lds`` bytes), and ``lines``, the lines of ``n`` samples the launch
        covers (the other axis' ``n`` at that level).  Axis 1 is listed also when the plan is not bidirectional."""
        width = len(capi.PS_NOTCH_ROUTE)
        buf = (C.c_int * (2 * 2 * capi.PS_MAX_LEVELS * width))()   # two passes, two axes per level
        count = capi.lib().mi_pystripe_plan_notch_routes(self._h, buf, len(buf))
        if count < 0:
            capi.check(count)
        routes = [dict(zip(capi.PS_NOTCH_ROUTE, buf[i * width:(i + 1) * width])) for i in range(count)]
        for i, r in enumerate(routes):
            r["lines"] = routes[i ^ 1]["n"]
        return routes

    def clips(self, n=None):
        """(clips float32 [n, 3], status int32 [n]) of the first ``n`` tiles (default: all) of the last ``run``: the triple
        (min, med, max) in log1p units the bleach correction used -- min raised to log1p(1) -- and capi.PS_CLIPS_*.  The caller has
        synchronised the stream of that run."""
        n = self._last_n if n is None else int(n)
        clips, status = np.empty((n, 3), np.float32), np.empty((n,), np.int32)
        capi.check(capi.lib().mi_pystripe_plan_clips(self._h, clips.ctypes.data, status.ctypes.data, n))
        return clips, status

    def run(self, tiles, flat=None, out=None):
        import torch
        tdt = getattr(torch, self.in_dtype.name)
        if not (isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.is_contiguous() and tiles.dim() == 3 and tiles.dtype == tdt
                and tuple(tiles.shape[1:]) == self.shape):
            raise ValueError(f"Plan.run: a contiguous [n, {self.shape[0]}, {self.shape[1]}] {self.in_dtype.name} device tensor is expected")
        n = int(tiles.shape[0])
        if out is None:
            out = torch.empty((n,) + self.out_shape, dtype=getattr(torch, self.out_dtype.name), device=tiles.device)
        fp = None
        if self.params.use_flat:
            if flat is None or tuple(flat.shape) != self.shape or flat.dtype != torch.float32 or not flat.is_contiguous():
                raise ValueError("Plan.run: the plan divides by a flat field: a contiguous float32 tensor of the tile's shape is expected")
            fp = flat.data_ptr()
        with torch.cuda.device(tiles.device):
            capi.check(capi.lib().mi_pystripe_run(self._h, capi.current_stream_ptr(tiles.device), tiles.data_ptr(), fp, out.data_ptr(), n))
        self._last_n = n
        return out

    def close(self):
        if self._h:
            capi.lib().mi_pystripe_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _as_stack(img, device):
    """img: 2-D tile or [n, ny, nx] stack, numpy or device tensor -> (contiguous device stack, single, is_tensor, numpy dtype)"""
    import torch
    is_tensor = isinstance(img, torch.Tensor)
    if is_tensor:
        tiles = img
        in_dtype = np.dtype(str(img.dtype).replace("torch.", ""))
    else:
        img = np.asarray(img)
        in_dtype = img.dtype
        _dtype_code(in_dtype, "img.dtype")
        capi.require_gpu()
        tiles = torch.from_numpy(np.ascontiguousarray(img)).to(torch.device(device if device is not None else "cuda:0"))
    single = tiles.dim() == 2
    if tiles.dim() not in (2, 3):
        raise ValueError(f"a 2-D tile or a stack [n, ny, nx] is expected, got shape {tuple(tiles.shape)}")
    return (tiles[None] if single else tiles).contiguous(), single, is_tensor, in_dtype


# ---------------------------------------------------------------------------------------------------------------------------------
# lightsheet correction (pystripe/lightsheet_correct.py; include/mi_lightsheet.h)

BACKGROUND_SPACING, BACKGROUND_STEP = 25, 2   # process_img's choice (pystripe/core.py:1343-1346)


def check_lightsheet_shape(shape, artifact_length=150, spacing=BACKGROUND_SPACING):
    """Raises NotImplementedError when a tile of ``shape`` holds no window centre: the reference then divides by zero in zoom (or
    returns zeros when the tile is uniform); this build refuses it from the shape alone."""
    ny, nx = int(shape[-2]), int(shape[-1])
    if nx < artifact_length or ny < spacing or nx < spacing:
        raise NotImplementedError(f"lightsheet=True: a tile of shape {(ny, nx)} is narrower than artifact_length={artifact_length} or has "
                                  f"an extent below the background spacing {spacing}: no window centre fits (the reference fails here too)")


def make_lightsheet_params(map_dtype, artifact_length=150, background_window_size=200, percentile=0.25, lightsheet_vs_background=2.0,
                           spacing=BACKGROUND_SPACING, step=BACKGROUND_STEP, along_y=False, max_batch=0):
    """mi_lightsheet_params for process_img's lightsheet options."""
    if isinstance(percentile, (tuple, list, np.ndarray)):
        _refuse("percentile", percentile, "one percentile is built, not a list")
    if not 0 <= float(percentile) <= 1:
        raise ValueError(f"Percentiles must be in the range [0, 100] (percentile={percentile!r} stands for {100 * percentile})")
    p = capi.LightsheetParams()
    p.artifact_length, p.artifact_along_y = int(artifact_length), int(bool(along_y))
    p.background_window_size, p.background_spacing, p.background_step = int(background_window_size), int(spacing), int(step)
    p.percentile, p.lightsheet_vs_background = float(percentile), float(lightsheet_vs_background)
    p.factor_is_integer = int(isinstance(lightsheet_vs_background, (int, np.integer)) and not isinstance(lightsheet_vs_background, bool))
    p.map_dtype, p.max_batch = _dtype_code(map_dtype, "d_type"), int(max_batch)
    return p


def derive_lightsheet(shape, in_dtype, params):
    """The bookkeeping of a lightsheet plan without a device (centres, window bounds, largest window, zero lines, scratch)."""
    info = capi.LightsheetInfo()
    capi.check(capi.lib().mi_lightsheet_derive(int(shape[0]), int(shape[1]), _dtype_code(in_dtype, "dtype"), C.byref(params), C.byref(info)))
    return info


class LightsheetPlan:
    """mi_lightsheet plan for tiles of one shape and dtype.  ``run(tiles)`` corrects a [n, ny, nx] device tensor (in place unless
    ``out`` is given) and returns (out, lightsheet maps or None, background maps or None)."""

    def __init__(self, device, shape, in_dtype, params):
        import torch
        capi.require_gpu()
        self.device = torch.device(device if device is not None else "cuda:0")
        self.shape, self.in_dtype, self.params = (int(shape[0]), int(shape[1])), np.dtype(in_dtype), params
        self.map_dtype = _CODE_NP[params.map_dtype]
        self._h = C.c_void_p()
        capi.check(capi.lib().mi_lightsheet_plan_create(self.device.index or 0, self.shape[0], self.shape[1], _dtype_code(in_dtype, "dtype"),
                                                        C.byref(params), C.byref(self._h)))
        self.info = capi.LightsheetInfo()
        capi.check(capi.lib().mi_lightsheet_plan_info(self._h, C.byref(self.info)))

    def run(self, tiles, out=None, return_lightsheet=False, return_background=False):
        import torch
        tdt = getattr(torch, self.in_dtype.name)
        if not (isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.is_contiguous() and tiles.dim() == 3 and tiles.dtype == tdt
                and tuple(tiles.shape[1:]) == self.shape):
            raise ValueError(f"LightsheetPlan.run: a contiguous [n, {self.shape[0]}, {self.shape[1]}] {self.in_dtype.name} device tensor "
                             "is expected")
        out = tiles if out is None else out
        if out.shape != tiles.shape or out.dtype != tiles.dtype or not out.is_contiguous():
            raise ValueError("LightsheetPlan.run: out must look like the input")
        mdt = getattr(torch, self.map_dtype.name)
        ls = torch.empty(tiles.shape, dtype=mdt, device=tiles.device) if return_lightsheet else None
        bg = torch.empty(tiles.shape, dtype=mdt, device=tiles.device) if return_background else None
        with torch.cuda.device(tiles.device):
            capi.check(capi.lib().mi_lightsheet_run(self._h, capi.current_stream_ptr(tiles.device), tiles.data_ptr(), out.data_ptr(),
                                                    None if ls is None else ls.data_ptr(), None if bg is None else bg.data_ptr(),
                                                    int(tiles.shape[0])))
        return out, ls, bg

    def close(self):
        if self._h:
            capi.lib().mi_lightsheet_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pair(value, name, default=None):
    """(y, x) of a 2- or 3-tuple of the reference (its images carry a third axis of one sample)."""
    if value is None:
        return default
    if isinstance(value, np.ndarray):
        _refuse(name, "array", "only rectangular windows given as a tuple are built")
    v = tuple(1 if e is None else int(e) for e in value)
    if len(v) == 3 and v[2] == 1:
        v = v[:2]
    if len(v) != 2:
        raise ValueError(f"Dimension mismatch in the parameters! ({name}={value!r} for a 2-D image)")
    return v


def local_percentile(source, percentile, selem=(50, 50), spacing=None, step=None, interpolate=1, mask=None, dtype=None, device=None):
    """pystripe/lightsheet_correct.py:245 on the GPU for one percentile and a rectangular window: the local percentiles on the
    sub-grid (``interpolate=None``) or resampled to the image shape (``interpolate=1``).  ``source``: a 2-D image or a stack
    [n, ny, nx], numpy or device tensor.  Tuples may carry the reference's third entry of 1."""
    import torch
    if mask is not None:
        _refuse("mask", "array", "masked windows are not built")
    if isinstance(percentile, (tuple, list, np.ndarray)):
        _refuse("percentile", percentile, "one percentile is built, not a list")
    if interpolate not in (None, 0, 1) or interpolate is False:
        _refuse("interpolate", interpolate, "order 1 and None (the sub-grid) are built")
    if not 0 <= float(percentile) <= 1:
        raise ValueError(f"Percentiles must be in the range [0, 100] (percentile={percentile!r} stands for {100 * percentile})")
    selem = _pair(selem, "selem")
    spacing = _pair(spacing, "spacing", selem)
    step = _pair(step, "step", (1, 1))
    tiles, single, is_tensor, in_dtype = _as_stack(source, device)
    n, ny, nx = (int(v) for v in tiles.shape)
    out_dtype = np.dtype(in_dtype if dtype is None else dtype)
    if ny < spacing[0] or nx < spacing[1]:
        raise NotImplementedError(f"local_percentile: an image of shape {(ny, nx)} holds no centre at spacing={spacing}")
    shape = (n, ny, nx) if interpolate else (n, ny // spacing[0], nx // spacing[1])
    out = torch.empty(shape, dtype=getattr(torch, out_dtype.name), device=tiles.device)
    with torch.cuda.device(tiles.device):
        capi.check(capi.lib().mi_lightsheet_local_percentile(
            tiles.device.index or 0, capi.current_stream_ptr(tiles.device), tiles.data_ptr(), _dtype_code(in_dtype, "source.dtype"), ny, nx, n,
            selem[0], selem[1], spacing[0], spacing[1], step[0], step[1], float(percentile), int(bool(interpolate)), out.data_ptr(),
            _dtype_code(out_dtype, "dtype")))
    out = out[0] if single else out
    return out if is_tensor else out.cpu().numpy()


def correct_lightsheet(img, percentile=0.25, mask=None, lightsheet=dict(selem=(150, 1, 1)),
                       background=dict(selem=(200, 200, 1), spacing=(25, 25, 1), interpolate=1, dtype=None, step=(2, 2, 1)),
                       lightsheet_vs_background=2.0, return_lightsheet=False, return_background=False, device=None):
    """pystripe/lightsheet_correct.py:31 on the GPU: ``img - min(img, min(ls, bg * lightsheet_vs_background))`` with ``ls`` the local
    percentile in a window along the lightsheet and ``bg`` the one in a square window, both resampled to the image.  ``img``: a 2-D
    tile or a stack [n, ny, nx], numpy or device tensor; the result is new (the reference works in place).  Built: a ``lightsheet``
    window (1, L) or (L, 1) at its own spacing, a square ``background`` window with one spacing and one step, ``interpolate=1``."""
    import torch
    if mask is not None:
        _refuse("mask", "array", "masked windows are not built")
    ls_kw = dict(dict(selem=(50, 50), spacing=None, step=None, interpolate=1, mask=None, dtype=None), **lightsheet)
    bg_kw = dict(dict(selem=(50, 50), spacing=None, step=None, interpolate=1, mask=None, dtype=None), **background)
    for name, kw in (("lightsheet", ls_kw), ("background", bg_kw)):
        if kw["mask"] is not None:
            _refuse(f"{name}['mask']", "array", "masked windows are not built")
        if kw["interpolate"] != 1:
            _refuse(f"{name}['interpolate']", kw["interpolate"], "order 1 is built")
    ls_sel, bg_sel = _pair(ls_kw["selem"], "lightsheet['selem']"), _pair(bg_kw["selem"], "background['selem']")
    ls_space, bg_space = _pair(ls_kw["spacing"], "lightsheet['spacing']", ls_sel), _pair(bg_kw["spacing"], "background['spacing']", bg_sel)
    ls_step, bg_step = _pair(ls_kw["step"], "lightsheet['step']", (1, 1)), _pair(bg_kw["step"], "background['step']", (1, 1))
    if min(ls_sel) != 1 or ls_space != ls_sel or ls_step != (1, 1):
        _refuse("lightsheet", lightsheet, "a window (1, L) or (L, 1) at its own spacing without a step is built")
    if bg_sel[0] != bg_sel[1] or bg_space[0] != bg_space[1] or bg_step[0] != bg_step[1]:
        _refuse("background", background, "a square window with one spacing and one step is built")
    tiles, single, is_tensor, in_dtype = _as_stack(img, device)
    map_dtype = np.dtype(in_dtype if ls_kw["dtype"] is None else ls_kw["dtype"])
    if np.dtype(in_dtype if bg_kw["dtype"] is None else bg_kw["dtype"]) != map_dtype:
        _refuse("background['dtype']", bg_kw["dtype"], "one dtype for both estimates is built")
    along_y = ls_sel[1] == 1 and ls_sel[0] != 1
    length = max(ls_sel)
    ny, nx = (int(v) for v in tiles.shape[1:])
    if (ny if along_y else nx) < length or ny < bg_space[0] or nx < bg_space[0]:
        raise NotImplementedError(f"lightsheet: a tile of shape {(ny, nx)} holds no window centre for selem={ls_sel}, spacing={bg_space}")
    prm = make_lightsheet_params(map_dtype, length, bg_sel[0], percentile, lightsheet_vs_background, bg_space[0], bg_step[0], along_y,
                                 max_batch=min(int(tiles.shape[0]), 16))
    plan = LightsheetPlan(tiles.device, (ny, nx), in_dtype, prm)
    try:
        got = plan.run(tiles, torch.empty_like(tiles), return_lightsheet, return_background)
        torch.cuda.synchronize(tiles.device)
    finally:
        plan.close()
    got = [g if is_tensor else g.cpu().numpy() for g in ((a[0] if single else a) for a in got if a is not None)]
    return got[0] if len(got) == 1 else tuple(got)


# ---------------------------------------------------------------------------------------------------------------------------------
# resize to new_size (pystripe/core.py:1356-1359; include/mi_tile_resize.h)

def check_new_size(new_size):
    """``new_size`` as a tuple of two positive Python integers, or ValueError naming it."""
    try:
        pair = tuple(new_size)
    except TypeError:
        pair = ()
    ok = len(pair) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and v >= 1 for v in pair)
    if not ok:
        raise ValueError(f"new_size={new_size!r}: two positive integers (rows, columns) are expected")
    return int(pair[0]), int(pair[1])


def resize_decision(tile_shape, new_size):
    """What process_img does with a tile of ``tile_shape`` (after ``down_sample``) for ``new_size``, from the shapes alone: None when
    nothing is resized (no ``new_size``, or equal shapes), else ``new_size`` as a tuple.  The reference compares the two shapes as
    tuples: below ``new_size`` it resizes with ``anti_aliasing=True``, above it without.  The Gaussian pre-filter of the first case
    acts on an axis that shrinks only; that mixed case is refused (NotImplementedError naming ``new_size``), every other one is the
    plain order-1 zoom."""
    if new_size is None:
        return None
    N = check_new_size(new_size)
    T = (int(tile_shape[-2]), int(tile_shape[-1]))
    if T == N:
        return None
    if T < N and (N[0] < T[0] or N[1] < T[1]):
        _refuse("new_size", N, f"a tile of shape {T} is below it as a tuple, so the reference resizes with anti_aliasing=True, and an axis "
                               "shrinks: the Gaussian pre-filter on float64 is not built")
    return N


def tile_resize_tables(n, m):
    """(i0, i1, t) of one axis of the resize, n samples -> m samples, from the library's own host function (no device needed)."""
    i0, i1, t = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float64)
    capi.check(capi.lib().mi_tile_resize_tables(int(n), int(m), i0.ctypes.data_as(C.POINTER(C.c_int)), i1.ctypes.data_as(C.POINTER(C.c_int)),
                                                t.ctypes.data_as(C.POINTER(C.c_double))))
    return i0, i1, t


class ResizePlan:
    """mi_tile_resize plan for tiles of one shape and dtype.  ``run(tiles)``: [n, ny, nx] device tensor -> [n, my, mx] of the same type."""

    def __init__(self, device, shape, new_size, dtype, max_batch=0):
        import torch
        self.shape, self.out_shape, self.dtype = (int(shape[0]), int(shape[1])), check_new_size(new_size), np.dtype(dtype)
        code = _dtype_code(dtype, "dtype")
        capi.require_gpu()
        self.device = torch.device(device if device is not None else "cuda:0")
        self._h = C.c_void_p()
        capi.check(capi.lib().mi_tile_resize_plan_create(self.device.index or 0, self.shape[0], self.shape[1], self.out_shape[0], self.out_shape[1],
                                                         code, int(max_batch), C.byref(self._h)))

    def run(self, tiles, out=None):
        import torch
        tdt = getattr(torch, self.dtype.name)
        if not (isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.is_contiguous() and tiles.dim() == 3 and tiles.dtype == tdt
                and tuple(tiles.shape[1:]) == self.shape):
            raise ValueError(f"ResizePlan.run: a contiguous [n, {self.shape[0]}, {self.shape[1]}] {self.dtype.name} device tensor is expected")
        n = int(tiles.shape[0])
        if out is None:
            out = torch.empty((n,) + self.out_shape, dtype=tdt, device=tiles.device)
        elif tuple(out.shape) != (n,) + self.out_shape or out.dtype != tdt or not out.is_contiguous() or out.device != tiles.device:
            raise ValueError("ResizePlan.run: out must be a contiguous tensor of the result's shape and the input's type")
        with torch.cuda.device(tiles.device):
            capi.check(capi.lib().mi_tile_resize_run(self._h, capi.current_stream_ptr(tiles.device), tiles.data_ptr(), out.data_ptr(), n))
        return out

    def close(self):
        if self._h:
            capi.lib().mi_tile_resize_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resize_tiles(img, new_size, device=None):
    """``skimage.transform.resize(img, new_size, preserve_range=True, anti_aliasing=False)`` as process_img uses it
    (pystripe/core.py:1359) on the GPU: scipy's order-1 zoom (mode 'mirror', grid_mode) and a clip to the tile's own [min, max].
    ``img``: a 2-D tile or a stack [n, ny, nx], numpy or device tensor, uint8 / uint16 / float32; the same container and dtype come
    back (an integer tile is the truncated float64 result, which is what process_img's astype makes of it)."""
    import torch
    N = check_new_size(new_size)
    tiles, single, is_tensor, in_dtype = _as_stack(img, device)
    plan = ResizePlan(tiles.device, tuple(int(v) for v in tiles.shape[1:]), N, in_dtype, max_batch=min(int(tiles.shape[0]), 16))
    try:
        out = plan.run(tiles)
        torch.cuda.synchronize(tiles.device)
    finally:
        plan.close()
    out = out[0] if single else out
    return out if is_tensor else out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# foreground mask (pystripe/core.py:475-489; include/mi_tile_mask.h)

def check_flood_fill_flag(flood_fill_flag):
    """The connectivity cv2.floodFill reads from its flags (``flood_fill_flag & 0xff``): 4 or 8, or ValueError naming the argument."""
    ok = isinstance(flood_fill_flag, (int, np.integer)) and not isinstance(flood_fill_flag, (bool, np.bool_))
    if not ok or (int(flood_fill_flag) & 0xff) not in (4, 8):
        raise ValueError(f"flood_fill_flag={flood_fill_flag!r}: its low byte is the connectivity, 4 or 8")
    return int(flood_fill_flag) & 0xff


def check_mask_steps(close_steps, open_steps):
    """(close_steps, open_steps) as Python integers of 1 or more, or ValueError naming the one that is not."""
    for name, k in (("close_steps", close_steps), ("open_steps", open_steps)):
        if not isinstance(k, (int, np.integer)) or isinstance(k, (bool, np.bool_)) or k < 1:
            raise ValueError(f"{name}={k!r}: the side of the box, an integer of 1 or more, is expected")
    return int(close_steps), int(open_steps)


def mask_code_bound(clip_med, ncodes):
    """The code bound of the mask's threshold on an integer tile: the largest integer ``b`` (-1 .. ncodes - 1) with
    ``code > b  <=>  log_table(ncodes)[code] > float32(clip_med)`` for every code, from the numpy log1p table that also decides the
    bins of the automatic clips.  The table does not decrease, so the codes above the clip are a tail of it."""
    from .thresholds import log_table
    return int(np.searchsorted(log_table(int(ncodes)), np.float32(clip_med), side="right")) - 1


class MaskPlan:
    """mi_tile_mask plan for tiles of one shape and dtype.  ``run(tiles, threshold)``: [n, ny, nx] device tensor -> uint8 masks
    [n, ny, nx] (0 / 1), and with ``masked=True`` also the tiles zeroed outside the mask (``masked`` may be a tensor to write to,
    the input itself included).  ``fill_rounds`` is the number of fill rounds of the last run."""

    def __init__(self, device, shape, dtype, close_steps=50, open_steps=500, connectivity=4, max_batch=0):
        import torch
        self.shape, self.dtype = (int(shape[0]), int(shape[1])), np.dtype(dtype)
        code = _dtype_code(dtype, "dtype")
        capi.require_gpu()
        self.device = torch.device(device if device is not None else "cuda:0")
        self._h = C.c_void_p()
        capi.check(capi.lib().mi_tile_mask_plan_create(self.device.index or 0, self.shape[0], self.shape[1], code, int(close_steps), int(open_steps),
                                                       int(connectivity), int(max_batch), C.byref(self._h)))

    @property
    def info(self):
        info = capi.TileMaskInfo()
        capi.check(capi.lib().mi_tile_mask_plan_info(self._h, C.byref(info)))
        return info

    @property
    def fill_rounds(self):
        return int(self.info.fill_rounds)

    def run(self, tiles, threshold, log_domain=False, masked=None):
        import torch
        tdt = getattr(torch, self.dtype.name)
        if not (isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.is_contiguous() and tiles.dim() == 3 and tiles.dtype == tdt
                and tuple(tiles.shape[1:]) == self.shape):
            raise ValueError(f"MaskPlan.run: a contiguous [n, {self.shape[0]}, {self.shape[1]}] {self.dtype.name} device tensor is expected")
        n = int(tiles.shape[0])
        mask = torch.empty(tiles.shape, dtype=torch.uint8, device=tiles.device)
        if masked is True:
            masked = torch.empty_like(tiles)
        elif masked is not None and (masked.shape != tiles.shape or masked.dtype != tdt or not masked.is_contiguous() or masked.device != tiles.device):
            raise ValueError("MaskPlan.run: masked must look like the input")
        with torch.cuda.device(tiles.device):
            capi.check(capi.lib().mi_tile_mask_run(self._h, capi.current_stream_ptr(tiles.device), tiles.data_ptr(), float(threshold),
                                                   int(bool(log_domain)), mask.data_ptr(), None if masked is None else masked.data_ptr(), n))
        return mask if masked is None else (mask, masked)

    def close(self):
        if self._h:
            capi.lib().mi_tile_mask_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_MASK_SCRATCH_BUDGET = 2 << 30   # device bytes one mask plan may own: sizes its batch


def _mask_batch(n, shape):
    """tiles of one round of a mask plan: at most 16, and as many as keep the plan's scratch (about 6 bytes per sample) in budget"""
    return int(max(1, min(n, 16, _MASK_SCRATCH_BUDGET // (6 * shape[0] * shape[1] + 1))))


def get_img_mask(img, threshold, close_steps=50, open_steps=500, flood_fill_flag=4, device=None):
    """pystripe/core.py:475 on the GPU: ``img > threshold``, closed with a ``close_steps`` box, opened with an ``open_steps`` box, with
    the background regions that hold a corner removed and every other hole filled (include/mi_tile_mask.h states the windows, the
    border rule and the one-sample shift of an even box).  ``img``: a 2-D tile or a stack [n, ny, nx], numpy or device tensor, uint8 /
    uint16 / float32; a bool mask in the same kind of container comes back.  Raw values are compared: no logarithm is taken."""
    import torch
    connectivity = check_flood_fill_flag(flood_fill_flag)
    close_steps, open_steps = check_mask_steps(close_steps, open_steps)
    if threshold != threshold:
        raise ValueError(f"threshold={threshold!r}: a number is expected")
    tiles, single, is_tensor, in_dtype = _as_stack(img, device)
    shape = tuple(int(v) for v in tiles.shape[1:])
    plan = MaskPlan(tiles.device, shape, in_dtype, close_steps, open_steps, connectivity, _mask_batch(int(tiles.shape[0]), shape))
    try:
        mask = plan.run(tiles, threshold).to(torch.bool)
    finally:
        plan.close()
    mask = mask[0] if single else mask
    return mask if is_tensor else mask.cpu().numpy()


def _unmasked_clips(tiles, in_dtype, frequency, max_method, clips, verbose):
    """float32 [n, 3]: the triple (min, med, max) of every tile with the clips that are None estimated from the tile as it is, as the
    automatic-clip route of the plan reports them (``Plan.clips``; the given ones keep their slot).  Raises as ``raise_for_clips``."""
    import torch
    shape = tuple(int(v) for v in tiles.shape[1:])
    # The plan's own route, also when no correction is asked for (the frequency is then a stand-in and the corrected image is dropped):
    # the mask must be cut at exactly the median an un-masked run of the tile reports, and that one comes from the plan's kernels --
    # numpy's log1p table for integer tiles, the device's log1pf and its two-pass histogram for float tiles.  threshold_multiotsu of a
    # log image made by other arithmetic can put a float sample into the neighbouring bin and move the median by a bin.
    if frequency is None:   # only the median is needed: estimate the whole triple, which is ordered by construction
        clips = (None, None, None)
    opts = dict(zip(BLEACH_CLIPS, clips))
    prm = make_params(in_dtype, log_output=True, keep_uniform=True, max_batch=min(int(tiles.shape[0]), 16), extended=True,
                      bleach_correction_frequency=0.5 if frequency is None else frequency, bleach_correction_max_method=max_method, **opts)
    plan = Plan(tiles.device, shape, in_dtype, prm)
    try:
        plan.run(tiles)
        torch.cuda.synchronize(tiles.device)
        raise_for_clips(plan, verbose)
        triples, _ = plan.clips()
    finally:
        plan.close()
    return triples


def _filter_streaks_masked(img, device, close_steps, open_steps, frequency, max_method, clips, verbose, **opts):
    """filter_streaks with ``enable_masking``: the clips that are missing come from the un-masked tile, the mask from ``clip_med`` on
    the log image, and the tile zeroed outside the mask (log1p(0) = 0, so this is ``log_image *= mask``) goes through the plan with
    its clips given, never estimated again.  Tiles of a stack whose triples differ run one by one."""
    import torch
    tiles, single, is_tensor, in_dtype = _as_stack(img, device)
    n, shape = int(tiles.shape[0]), tuple(int(v) for v in tiles.shape[1:])
    need = clips[1] is None or (frequency is not None and any(c is None for c in clips))
    if need:
        triples = _unmasked_clips(tiles, in_dtype, frequency, max_method, clips, verbose)
    else:
        triples = np.tile(np.array([np.nan if c is None else c for c in clips], np.float32), (n, 1))
    same = all(np.array_equal(triples[t], triples[0], equal_nan=True) for t in range(n))
    groups = [list(range(n))] if same else [[t] for t in range(n)]
    plan = MaskPlan(tiles.device, shape, in_dtype, close_steps, open_steps, 4, _mask_batch(1 if len(groups) > 1 else n, shape))
    outs = []
    try:
        for group in groups:
            lo, med, hi = (None if v != v else float(v) for v in triples[group[0]])
            sub = tiles[group[0]:group[-1] + 1]
            if med is None:   # a uniform tile has no estimate and no mask: it takes the plan's own route for uniform tiles
                masked = sub
            elif in_dtype.kind == "u":
                _, masked = plan.run(sub, mask_code_bound(med, 256 if in_dtype == np.uint8 else 65536), False, masked=True)
            else:
                _, masked = plan.run(sub, float(np.float32(med)), True, masked=True)
            if frequency is not None:
                bleach = dict(bleach_correction_frequency=frequency, bleach_correction_max_method=max_method,
                              bleach_correction_clip_min=lo, bleach_correction_clip_med=med, bleach_correction_clip_max=hi)
            else:
                bleach = {} if clips[0] is None else dict(bleach_correction_clip_min=clips[0])
            outs.append(_run_tiles(masked, None, device, verbose=verbose, **opts, **bleach))
    finally:
        plan.close()
    out = outs[0] if len(outs) == 1 else torch.cat(outs)
    out = out[0] if single else out
    return out if is_tensor else out.cpu().numpy()


class Pipeline:
    """process_img for tiles of one shape and dtype: one pystripe plan, or -- with ``lightsheet`` (a dict of artifact_length,
    background_window_size, percentile, lightsheet_vs_background) or a ``new_size`` that differs from the tile's shape after
    ``down_sample`` -- up to four steps that stay on the device: the pystripe plan up to and including ``dark`` in the tile's own
    kind, the lightsheet plan in place, the resize plan, and a filter-less pystripe plan for conversion, flip and rotation (left
    out when it would change nothing).  A uniform tile leaves the first step as zeros and stays zeros through the others."""

    def __init__(self, device, shape, in_dtype, flat=False, lightsheet=None, new_size=None, max_batch=0, **opts):
        in_dtype = np.dtype(in_dtype)
        self.tail = self.ls = self.resize = None
        down = opts.get("down_sample")
        resize_to = resize_decision(shape if down is None else calculate_down_sampled_size(shape, down), new_size)
        if lightsheet is None and resize_to is None:
            self.head = Plan(device, shape, in_dtype, make_params(in_dtype, flat=flat, max_batch=max_batch, **opts))
            return
        tail_names = ("rotate", "flip_upside_down", "convert_to_16bit", "convert_to_8bit", "bit_shift_to_right")
        entry_type = np.dtype(in_dtype if opts.get("d_type") is None else opts["d_type"])
        head_opts = {k: v for k, v in opts.items() if k not in tail_names}
        prm = make_params(in_dtype, flat=flat, max_batch=max_batch, **dict(head_opts, d_type=in_dtype))
        info = derive(shape, in_dtype, prm)
        mid_type = in_dtype if info.integer_kind else np.dtype(np.float32)   # the kind the tile has after ``dark``
        prm.out_dtype = _dtype_code(mid_type, "dtype")
        mid_shape = (info.ny, info.nx)
        ls_prm = None
        if lightsheet is not None:
            check_lightsheet_shape(mid_shape, lightsheet.get("artifact_length", 150))
            ls_prm = make_lightsheet_params(entry_type, max_batch=max_batch, **lightsheet)
        tail_shape = mid_shape if resize_to is None else resize_to
        tail_prm = make_params(mid_type, max_batch=max_batch, keep_uniform=True, d_type=entry_type, **{k: opts[k] for k in tail_names if k in opts})
        tail_info = derive(tail_shape, mid_type, tail_prm)
        out_type = _CODE_NP[tail_info.out_dtype]
        if resize_to is not None and mid_type.kind == "u" and out_type.kind == "f":
            _refuse("new_size", resize_to, f"a {mid_type.name} tile with d_type={out_type.name}: the reference keeps the fractions of the "
                                           "float64 image there; the resize of an integer tile is built with the truncation that follows it")
        self.head = Plan(device, shape, in_dtype, prm)
        try:
            if ls_prm is not None:
                self.ls = LightsheetPlan(device, mid_shape, mid_type, ls_prm)
            if resize_to is not None:
                self.resize = ResizePlan(device, mid_shape, resize_to, mid_type, max_batch=max_batch)
            changes = tail_prm.rotate or tail_prm.flip_upside_down or out_type != mid_type
            if changes:
                self.tail = Plan(device, tail_shape, mid_type, tail_prm)
        except Exception:
            self.close()
            raise

    def run(self, tiles, flat=None):
        out = self.head.run(tiles, flat)
        if self.ls is not None:
            self.ls.run(out)
        if self.resize is not None:
            out = self.resize.run(out)
        if self.tail is not None:
            out = self.tail.run(out)
        return out

    def close(self):
        for plan in (self.head, self.ls, self.resize, self.tail):
            if plan is not None:
                plan.close()


def _lightsheet_opts(lightsheet, shape, down_sample, artifact_length, background_window_size, percentile, lightsheet_vs_background):
    """None, or the options of the lightsheet step after the shape check that needs no device."""
    if not lightsheet:
        return None
    shape = tuple(int(v) for v in shape[-2:])
    if down_sample is not None:
        shape = calculate_down_sampled_size(shape, down_sample)
    check_lightsheet_shape(shape, artifact_length)
    return dict(artifact_length=artifact_length, background_window_size=background_window_size, percentile=percentile,
                lightsheet_vs_background=lightsheet_vs_background)


def raise_for_clips(plan, verbose=False):
    """After a synchronised run of ``plan`` (a Plan with automatic clips): what the reference raises for the first tile whose clips
    could not be used -- threshold_multiotsu's / numpy.histogram's ValueError, the AssertionError of correct_bleaching -- naming the
    tile's index in the stack and the triple.  ``verbose`` prints every tile's triple through expm1, as filter_streaks does."""
    clips, status = plan.clips()
    for t, (triple, st) in enumerate(zip(clips, status)):
        what = f"tile {t}: bleach_correction_clip_min, _med, _max = {tuple(float(v) for v in triple)}"
        if st == capi.PS_CLIPS_TOO_FEW:
            raise ValueError(f"{what}: after discretization into bins, the log image has fewer than 4 different values; it cannot be "
                             "thresholded in 4 classes")
        if st == capi.PS_CLIPS_NONFINITE:
            raise ValueError(f"{what}: autodetected range of the log image is not finite")
        if st == capi.PS_CLIPS_ORDER:
            raise AssertionError(f"{what}: 0 <= clip_min < clip_med < clip_max is expected (correct_bleaching)")
        if verbose and st == capi.PS_CLIPS_OK:
            lo, med, hi = (float(np.expm1(v)) for v in triple)
            print(f"bleach correction is applied: tile {t}, clip_min={lo}, clip_med={med}, clip_max={hi}")


def _run_tiles(img, flat, device, lightsheet=None, verbose=False, **opts):
    """img: 2-D tile or [n, ny, nx] stack, numpy or device tensor -> the same kind of container."""
    import torch
    tiles, single, is_tensor, in_dtype = _as_stack(img, device)
    shape = tuple(int(v) for v in tiles.shape[1:])
    flat_t = None
    if flat is not None:
        if tuple(flat.shape) == shape:
            flat_t = flat if isinstance(flat, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float32))
            flat_t = flat_t.to(tiles.device, torch.float32).contiguous()
        else:
            warnings.warn("warning: image and flat arrays had different shapes")
    plan = Pipeline(tiles.device, shape, in_dtype, flat=flat_t is not None, lightsheet=lightsheet, max_batch=min(int(tiles.shape[0]), 16), **opts)
    try:
        out = plan.run(tiles, flat_t)
        torch.cuda.synchronize(tiles.device)
        if plan.head.params.bleach_auto:
            raise_for_clips(plan.head, verbose)
    finally:
        plan.close()
    out = out[0] if single else out
    return out if is_tensor else out.cpu().numpy()


def _single_band(sigma, threshold):
    """``sigma`` as filter_streak_dual_band (pystripe/core.py:943) uses it on this path, where use_thresholding is never set:
    unchanged for ``threshold`` None or above 0; a threshold of 0 or less runs the single sigma1 pass."""
    s1, s2 = _sigma_pair(sigma)
    if threshold is None or threshold > 0 or s1 == s2:
        return sigma
    return (s1, s1)


def filter_streaks(img, sigma=(250, 250), level=0, wavelet="db9", crossover=10, threshold=None, padding_mode="wrap",
                   bidirectional=False, gpu_semaphore=None, bleach_correction_frequency=None, bleach_correction_max_method=False,
                   bleach_correction_clip_min=None, bleach_correction_clip_med=None, bleach_correction_clip_max=None,
                   log1p_normalization_needed=True, enable_masking=False, close_steps=50, open_steps=500, verbose=False, device=None,
                   log_output=False, extended=False):
    """pystripe/core.py:982 on the GPU.  ``crossover`` has no effect on this path (as in the reference).  ``log_output=True`` returns
    the float32 image just before ``expm1`` (an addition, for tests).  The bleach correction takes the three clips in log1p units; one
    left None is estimated per tile (``threshold_multiotsu(log1p(img), classes=4)``) and a tile it cannot be estimated for raises as in
    the reference (``raise_for_clips``).  With ``sigma=(0, 0)`` the correction runs alone.  ``enable_masking`` (with ``extended=True``)
    zeroes the log image outside ``get_img_mask(log image, bleach_correction_clip_med, close_steps, open_steps)`` before the filter, as
    the reference does (:1079-1080); a clip that is missing is then estimated from the un-masked tile and handed to the plan
    explicitly; with ``close_steps`` or ``open_steps`` None the run is the un-masked one."""
    _check_unsupported(dict(bleach_correction_frequency=bleach_correction_frequency, bleach_correction_clip_min=bleach_correction_clip_min,
                            bleach_correction_clip_med=bleach_correction_clip_med, bleach_correction_clip_max=bleach_correction_clip_max,
                            enable_masking=enable_masking, threshold=threshold, sigma=sigma, extended=extended, padding_mode=padding_mode,
                            log1p_normalization_needed=log1p_normalization_needed))
    s1, s2 = _sigma_pair(_single_band(sigma, threshold))
    if s1 == s2 == 0 and bleach_correction_frequency is None:
        return img
    wavelet = _early_wavelet((s1, s2), wavelet)
    bleach = _bleach_opts(img.shape, None, bleach_correction_frequency, bleach_correction_max_method, bleach_correction_clip_min,
                          bleach_correction_clip_med, bleach_correction_clip_max)
    if enable_masking and close_steps is not None and open_steps is not None:
        close_steps, open_steps = check_mask_steps(close_steps, open_steps)
        if (bleach_correction_frequency is not None and bleach_correction_clip_min is None and (s1, s2) > (0, 0)
                and str(padding_mode).lower() == "constant"):
            _refuse("enable_masking", True, "padding_mode='constant' with an estimated bleach_correction_clip_min pads with the minimum before "
                                            "it is raised to log1p(1), which the masked route does not carry: give bleach_correction_clip_min")
        if bleach_correction_clip_med is not None and bleach_correction_clip_med != bleach_correction_clip_med:
            raise ValueError(f"bleach_correction_clip_med={bleach_correction_clip_med!r}: the mask's threshold, a number, is expected")
        return _filter_streaks_masked(img, device, close_steps, open_steps, bleach_correction_frequency, bleach_correction_max_method,
                                      (bleach_correction_clip_min, bleach_correction_clip_med, bleach_correction_clip_max), verbose,
                                      sigma=(s1, s2), level=level, wavelet=wavelet, padding_mode=padding_mode, bidirectional=bidirectional,
                                      keep_uniform=True, log_output=log_output, extended=extended)
    return _run_tiles(img, None, device, sigma=(s1, s2), level=level, wavelet=wavelet, padding_mode=padding_mode, bidirectional=bidirectional,
                      keep_uniform=True, log_output=log_output, verbose=verbose, extended=extended, **bleach)


def process_img(img, flat=None, gaussian_filter_2d=False, down_sample=None, down_sample_method="max", tile_size=None, new_size=None,
                exclude_dark_edges_set_them_to_zero=False, sigma=(0, 0), level=0, wavelet="coif15", crossover=10, threshold=None,
                padding_mode="wrap", bidirectional=False, gpu_semaphore=None, bleach_correction_frequency=None,
                bleach_correction_clip_min=None, bleach_correction_clip_med=None, bleach_correction_clip_max=None,
                bleach_correction_max_method=False, log1p_normalization_needed=True, dark=0, lightsheet=False, artifact_length=150,
                background_window_size=200, percentile=0.25, lightsheet_vs_background=2.0, rotate=0, flip_upside_down=False,
                convert_to_16bit=False, convert_to_8bit=False, bit_shift_to_right=8, d_type=None, verbose=False, device=None,
                extended=False):
    """pystripe/core.py:1190 on the GPU, the reference's keywords and defaults (so ``wavelet`` must be given when ``sigma`` asks for the
    filter: the default NAME 'coif15' has no table here; ``wavelet=pywt.Wavelet("coif15")`` or its ``rec_lo`` is taken).
    ``gaussian_filter_2d`` does nothing, as in the reference, whose GaussianBlur result is discarded.  ``img`` may be
    a stack [n, ny, nx] of equally shaped tiles (an addition): they go through every launch together.  ``lightsheet=True`` runs
    ``correct_lightsheet`` after ``dark`` as the reference does; a tile too small for one window is refused from its shape alone.
    The clips of ``bleach_correction_frequency`` are in log1p units; one left None is estimated per tile on the device.  ``new_size``
    resizes after ``dark`` / ``lightsheet`` as ``batch_filter`` does; ``threshold``: see the module's text."""
    _check_unsupported(dict(bleach_correction_frequency=bleach_correction_frequency, bleach_correction_clip_min=bleach_correction_clip_min,
                            bleach_correction_clip_med=bleach_correction_clip_med, bleach_correction_clip_max=bleach_correction_clip_max,
                            exclude_dark_edges_set_them_to_zero=exclude_dark_edges_set_them_to_zero, threshold=threshold, sigma=sigma,
                            new_size=new_size, extended=extended, padding_mode=padding_mode,
                            log1p_normalization_needed=log1p_normalization_needed))
    sigma = _single_band(sigma, threshold)
    if new_size is not None:   # the values and the shapes, before anything touches the device
        shape = tuple(int(v) for v in img.shape[-2:])
        resize_decision(shape if down_sample is None else calculate_down_sampled_size(shape, down_sample), check_new_size(new_size))
    wavelet = _early_wavelet(sigma, wavelet)
    ls = _lightsheet_opts(lightsheet, img.shape, down_sample, artifact_length, background_window_size, percentile, lightsheet_vs_background)
    bleach = _bleach_opts(img.shape, down_sample, bleach_correction_frequency, bleach_correction_max_method, bleach_correction_clip_min,
                          bleach_correction_clip_med, bleach_correction_clip_max)
    return _run_tiles(img, flat, device, lightsheet=ls, down_sample=down_sample, down_sample_method=down_sample_method, sigma=sigma, level=level,
                      wavelet=wavelet, padding_mode=padding_mode, bidirectional=bidirectional, dark=dark, rotate=rotate,
                      flip_upside_down=flip_upside_down, convert_to_16bit=convert_to_16bit, convert_to_8bit=convert_to_8bit,
                      bit_shift_to_right=bit_shift_to_right, d_type=d_type, new_size=new_size, verbose=verbose, extended=extended, **bleach)


# ---------------------------------------------------------------------------------------------------------------------------------
# folder -> folder

def find_tiles(path, extensions=SUPPORTED_EXTENSIONS):
    """Every file under ``path``, at any depth, whose suffix is one of ``extensions`` in either letter case -- the files the
    reference's ``glob_re`` walk (pystripe/core.py:1603) hands to batch_filter.  Directories reached through links are not entered."""
    found = []
    for folder, _, names in os.walk(path, followlinks=False):
        found.extend(Path(folder) / name for name in names if os.path.splitext(name)[1].lower() in extensions)
    return sorted(found)


def raw_imread(path):
    """tsv/raw.py:9: 8-byte header (width, height as uint32, endianness by the smaller width), uint16 samples."""
    head = np.fromfile(path, dtype=np.uint8, count=8)
    w_be, h_be = head.view(">u4")
    w_le, h_le = head.view("<u4")
    (w, h, dt) = (w_le, h_le, "<u2") if w_le < w_be else (w_be, h_be, ">u2")
    return np.fromfile(path, dtype=dt, offset=8, count=int(w) * int(h)).reshape(int(h), int(w)).astype(np.uint16)


def imread_tif_raw_png(path, dtype=None, shape=None):
    """One tile, or None when the file cannot be read (pystripe/core.py:200 without its repair attempts).  TIFFs the library's reader
    takes go through it (mi_tiffio.h); every other TIFF and PNG through Pillow."""
    from . import brickio
    path = Path(path)
    ext = path.suffix.lower()
    try:
        if ext == ".raw":
            return raw_imread(path)
        if ext == ".dcimg":
            _refuse("input", path.name, ".dcimg input is not built")
        if ext in (".tif", ".tiff"):
            info = brickio.tiff_info(path)
            if info is not None and info[2] and info[1] is not None:
                (ny, nx), dt, _ = info
                return brickio.read_tiff_box([path], (ny, nx), dt, 0, ny, 0, nx)[0]
        if ext in (".tif", ".tiff", ".png"):
            from PIL import Image
            with Image.open(path) as handle:
                return np.asarray(handle).copy()
        print(f"Unsupported file format: {ext}")
    except NotImplementedError:
        raise
    except Exception as e:   # a damaged file: the caller decides (zero tile or skip)
        print(f"file: {path.name} failed to read: {type(e).__name__} - {e}")
    return None


def imsave_tif(path, img, compression=("ADOBE_DEFLATE", 1)):
    """One 2-D TIFF with the library's writer (Adobe deflate at the given level, or uncompressed)."""
    _write_tiles([Path(path)], np.ascontiguousarray(img)[None], compression)
    return True


def _write_tiles(paths, stack, compression):
    lib = capi.lib()
    n = len(paths)
    for p in paths:
        p.parent.mkdir(parents=True, exist_ok=True)
        if p.exists():
            p.unlink()       # the writer leaves an existing file alone; here the caller has already decided to replace it
    level = 1
    comp = 1
    if compression is None:
        comp = 0
    elif str(compression[0]).upper() not in ("ADOBE_DEFLATE", "DEFLATE", "ZLIB"):
        _refuse("compression", compression, "ADOBE_DEFLATE or None")
    else:
        level = min(max(int(compression[1]), 1), 9)
    code = {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.float32): 4}[stack.dtype]
    arr = (C.c_char_p * n)(*[os.fsencode(str(p)) for p in paths])
    capi.check(lib.mi_tiff_write_series(arr, n, stack.ctypes.data, code, stack.shape[2], stack.shape[1], comp, level, 0, None))


def split_for_rank(files, rank=None, world=None):
    """The share of ``files`` of this torchrun rank (RANK / WORLD_SIZE): every world-th file, so the ranks cover every file once."""
    rank = int(os.environ.get("RANK", 0)) if rank is None else int(rank)
    world = int(os.environ.get("WORLD_SIZE", 1)) if world is None else int(world)
    return list(files)[rank::world] if world > 1 else list(files)


def batch_filter(input_path, output_path, files_list=None, workers=None, threads_per_gpu=8, flat=None, gaussian_filter_2d=False,
                 sigma=(0, 0), level=0, wavelet="db9", crossover=10, threshold=None, padding_mode="reflect", bidirectional=False,
                 bleach_correction_frequency=None, bleach_correction_max_method=True, bleach_correction_clip_min=None,
                 bleach_correction_clip_med=None, bleach_correction_clip_max=None, dark=0, z_step=None, rotate=0, flip_upside_down=False,
                 lightsheet=False, artifact_length=150, background_window_size=200, percentile=.25, lightsheet_vs_background=2.0,
                 convert_to_16bit=False, convert_to_8bit=False, bit_shift_to_right=8, continue_process=False, d_type=None, tile_size=None,
                 down_sample=None, new_size=None, print_input_file_names=False, timeout=None, compression=("ADOBE_DEFLATE", 1),
                 down_sample_method="max", device=None, max_batch=None, stats=None, extended=False):
    """pystripe/core.py:1806: every .tif / .tiff / .raw / .png under ``input_path`` (or ``files_list``) -> the same relative path
    under ``output_path`` with a ``.tif`` suffix.  Returns 0.

    Tiles of equal shape and dtype are grouped into batches sized from the free device memory (``max_batch`` overrides); the next
    batch is read and the previous one written on host threads while the device works on the current one.  Under ``torchrun`` every
    rank takes every WORLD_SIZE-th file on its LOCAL_RANK device.  ``continue_process``: a file whose output exists is skipped.  A file
    that cannot be read becomes a zero tile when ``d_type`` and ``tile_size`` are given, else it is skipped with a warning.
    The clips of ``bleach_correction_frequency`` are in log1p units, one left None is estimated per tile;
    ``bleach_correction_max_method`` defaults to True here, as in the reference.  ``new_size``: every tile whose own shape after ``down_sample`` differs from it is resized to it after ``dark`` /
    ``lightsheet`` and before the conversion (``resize_decision``, ``resize_tiles``); outputs have that shape, swapped under
    ``rotate`` 90 / 270.  A tile whose shape differs from ``tile_size`` is not resized to ``tile_size``, as in the reference.  ``workers``, ``threads_per_gpu``, ``timeout``, ``z_step``, ``print_input_file_names`` are accepted and ignored.  ``stats`` (a dict)
    receives the seconds spent reading, computing and writing and the file counts."""
    import time
    import torch
    if convert_to_16bit and convert_to_8bit:
        raise TypeError("convert_to_16bit and convert_to_8bit are both set: choose one output format")
    _check_unsupported(dict(bleach_correction_frequency=bleach_correction_frequency, bleach_correction_clip_min=bleach_correction_clip_min,
                            bleach_correction_clip_med=bleach_correction_clip_med, bleach_correction_clip_max=bleach_correction_clip_max,
                            threshold=threshold, sigma=sigma, extended=extended, padding_mode=padding_mode))
    sigma = _single_band(sigma, threshold)
    if new_size is not None:   # the values, and the shapes where they are known, before anything touches the device
        new_size = check_new_size(new_size)
        if tile_size is not None:
            known = tuple(int(v) for v in tile_size)
            resize_decision(known if down_sample is None else calculate_down_sampled_size(known, down_sample), new_size)
    bleach_args =(bleach_correction_frequency, bleach_correction_max_method, bleach_correction_clip_min, bleach_correction_clip_med,
                   bleach_correction_clip_max)
    _bleach_opts((7, 7), None, *bleach_args)   # the values alone; every tile shape is checked when it is met
    wavelet = _early_wavelet(sigma, wavelet)
    input_path, output_path = Path(input_path), Path(output_path)
    if input_path.suffix.lower() == ".dcimg":
        _refuse("input_path", str(input_path), ".dcimg input is not built")
    if files_list is None:
        if input_path.is_file():
            files_list, input_path = [input_path], input_path.parent
        else:
            files_list = find_tiles(input_path)
    files = [Path(f) if Path(f).is_absolute() or Path(f).exists() else input_path / f for f in files_list]
    files = split_for_rank(files)
    capi.require_gpu()
    if device is None:
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)) % max(torch.cuda.device_count(), 1))
    device = torch.device(device)
    if flat is not None:
        flat = normalize_flat(flat)
    if tile_size is not None:
        tile_size = tuple(int(v) for v in tile_size)
    opts = dict(down_sample=down_sample, down_sample_method=down_sample_method, sigma=sigma, level=level, wavelet=wavelet,
                padding_mode=padding_mode, bidirectional=bidirectional, dark=dark, rotate=rotate, flip_upside_down=flip_upside_down,
                convert_to_16bit=convert_to_16bit, convert_to_8bit=convert_to_8bit, bit_shift_to_right=bit_shift_to_right, d_type=d_type,
                extended=extended, **_bleach_opts((7, 7), None, *bleach_args))

    st = dict(read_s=0.0, compute_s=0.0, write_s=0.0, files=len(files), written=0, skipped_existing=0, skipped_unreadable=0, zero_tiles=0)
    todo = []
    for f in files:
        try:
            rel = f.relative_to(input_path)
        except ValueError:
            rel = Path(f.name)
        o = (output_path / rel).with_suffix(".tif")
        if continue_process and o.exists():
            st["skipped_existing"] += 1
            continue
        todo.append((f, o))

    def read_many(paths):
        """{path: tile}: the TIFFs the library's reader takes go through it together (one call decodes them on all cores); what is left
        -- other TIFFs, .raw, .png, and every file of a call that failed -- is read one by one."""
        from . import brickio
        got, kinds = {}, {}
        for f in paths:
            if f.suffix.lower() in (".tif", ".tiff"):
                info = brickio.tiff_info(f)
                if info is not None and info[2] and info[1] is not None:
                    kinds.setdefault((info[0], np.dtype(info[1])), []).append(f)
        for ((ny, nx), dt), fs in kinds.items():
            try:
                stack = brickio.read_tiff_box(fs, (ny, nx), dt, 0, ny, 0, nx)
                got.update(zip(fs, stack))
            except Exception:   # a damaged file among them: the one-by-one route finds it
                pass
        for f in paths:
            if f not in got:
                got[f] = imread_tif_raw_png(f, dtype=d_type, shape=tile_size)
        return got

    def read_group(items):
        t0 = time.perf_counter()
        out = []
        tiles = read_many([f for f, _ in items])
        for f, o in items:
            img = tiles[f]
            if img is not None and (img.ndim != 2 or img.dtype not in _NP_CODES):
                print(f"file: {f.name}: a 2-D uint8 / uint16 / float32 image is expected, got {img.dtype} {img.shape}")
                img = None
            can_substitute = d_type is not None and tile_size is not None
            if img is None and can_substitute:
                print(f"warning: could not read {f}: the output is a dummy zeros tile of shape {tile_size} and type {d_type}")
                img = np.zeros(tile_size, np.dtype(d_type))
                st["zero_tiles"] += 1
            elif img is None:
                print(f"warning: could not read {f}: skipped (a dummy tile of zeros needs tile_size and d_type)")
                st["skipped_unreadable"] += 1
                continue
            out.append((img, o))
        st["read_s"] += time.perf_counter() - t0
        return out

    def write_group(paths, stack):
        t0 = time.perf_counter()
        _write_tiles(paths, stack, compression)
        st["write_s"] += time.perf_counter() - t0
        st["written"] += len(paths)

    plans = {}

    def compute(group):
        """tiles of one read group, any mix of shapes -> [(paths, host stack)]"""
        t0 = time.perf_counter()
        by_kind = {}
        for img, o in group:
            by_kind.setdefault((img.shape, img.dtype), []).append((img, o))
        results = []
        for (shape, dt), members in by_kind.items():
            use_flat = flat is not None and flat.shape == shape
            if flat is not None and not use_flat:
                print("warning: image and flat arrays had different shapes")
            # an OrthogonalWavelet compares and hashes by its coefficient values (without a filter the argument is not looked at)
            key = (shape, dt, use_flat, wavelet if isinstance(wavelet, (str, wavelets.OrthogonalWavelet)) else None)
            if key not in plans:
                _bleach_opts(shape, down_sample, *bleach_args)
                ls = _lightsheet_opts(lightsheet, shape, down_sample, artifact_length, background_window_size, percentile,
                                      lightsheet_vs_background)
                plans[key] = (Pipeline(device, shape, dt, flat=use_flat, lightsheet=ls, new_size=new_size, max_batch=chunk, **opts),
                              torch.from_numpy(flat).to(device) if use_flat else None)
            plan, flat_t = plans[key]
            stack = torch.from_numpy(np.stack([m[0] for m in members])).to(device)
            out = plan.run(stack, flat_t).cpu().numpy()
            if plan.head.params.bleach_auto:
                raise_for_clips(plan.head)
            results.append(([m[1] for m in members], out))
        st["compute_s"] += time.perf_counter() - t0
        return results

    # batch size: the scratch of a batch plus its input and output must fit a quarter of the free device memory
    chunk = 16
    if max_batch is not None:
        chunk = max(int(max_batch), 1)
    elif todo:
        first = imread_tif_raw_png(todo[0][0]) if tile_size is None else np.zeros(tile_size, np.dtype(d_type or np.uint16))
        if first is not None and first.ndim == 2 and first.dtype in _NP_CODES:
            _bleach_opts(first.shape, down_sample, *bleach_args)
            info = derive(first.shape, first.dtype, make_params(first.dtype, flat=False, **opts))
            per_tile = info.scratch_bytes_per_tile + 2 * first.size * 4 + (2 * new_size[0] * new_size[1] * 4 if new_size else 0)
            with torch.cuda.device(device):
                free = torch.cuda.mem_get_info()[0]
            chunk = int(min(max(free // 4 // max(per_tile, 1), 1), 64))
    groups = [todo[i:i + chunk] for i in range(0, len(todo), chunk)]
    with ThreadPoolExecutor(1) as reader, ThreadPoolExecutor(1) as writer:
        pending_writes = []
        nxt = reader.submit(read_group, groups[0]) if groups else None
        for gi in range(len(groups)):
            group = nxt.result()
            nxt = reader.submit(read_group, groups[gi + 1]) if gi + 1 < len(groups) else None
            for paths, stack in compute(group):
                pending_writes.append(writer.submit(write_group, paths, stack))
            while len(pending_writes) > 2:
                pending_writes.pop(0).result()
        for w in pending_writes:
            w.result()
    for plan, _ in plans.values():
        plan.close()
    if stats is not None:
        stats.update(st)
    return 0


# ---------------------------------------------------------------------------------------------------------------------------------
# command line

def _parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="pystripe.py", allow_abbrev=False,
                                description="pystripe tile preprocessing on the GPU (the reference's long option names, plain store_true flags)")
    p.add_argument("--input", "-i", required=True, help="folder (searched recursively) or one image file")
    p.add_argument("--output", "-o", default="", help="output folder (default: <input>_destriped)")
    p.add_argument("--sigma1", "-s1", type=float, default=0, help="foreground bandwidth [pixels]")
    p.add_argument("--sigma2", "-s2", type=float, default=0, help="background bandwidth [pixels]")
    p.add_argument("--level", "-l", type=int, default=0)
    which = p.add_mutually_exclusive_group()
    which.add_argument("--wavelet", default="db9", help="'db9' (default), 'haar' or 'db1' .. 'db20'")
    which.add_argument("--wavelet_file", default=None, metavar="FILE",
                       help="any other orthogonal wavelet of up to 128 taps: its reconstruction low-pass (PyWavelets' rec_lo) as a .npy file "
                            "or a text file of numbers")
    p.add_argument("--threshold", type=float, default=None)
    p.add_argument("--crossover", type=float, default=10)
    p.add_argument("--padding_mode", default="reflect")
    p.add_argument("--bidirectional", action="store_true")
    p.add_argument("--workers", type=int, default=None, help="accepted and ignored")
    p.add_argument("--chunks", type=int, default=1, help="accepted and ignored")
    p.add_argument("--compression_method", default="ADOBE_DEFLATE")
    p.add_argument("--compression_level", type=int, default=1)
    p.add_argument("--flat", default=None, help="flat-field reference image (TIFF)")
    p.add_argument("--dark", type=float, default=0)
    p.add_argument("--zstep", type=float, default=None, help="accepted and ignored (.dcimg only)")
    p.add_argument("--rotate", type=int, default=0)
    p.add_argument("--flip_upside_down", action="store_true")
    p.add_argument("--lightsheet", action="store_true", help="lightsheet correction (background subtraction) after --dark")
    p.add_argument("--artifact_length", type=int, default=150, help="length of the lightsheet window along x [pixels]")
    p.add_argument("--background_window_size", type=int, default=200, help="side of the background window [pixels]")
    p.add_argument("--percentile", type=float, default=0.25, help="percentile of both estimates, in [0, 1]")
    p.add_argument("--lightsheet_vs_background", type=float, default=2.0, help="factor on the background estimate")
    p.add_argument("--down_sample", type=int, nargs=2, default=None, metavar=("DY", "DX"))
    p.add_argument("--down_sample_method", default="max")
    p.add_argument("--convert_to_16bit", action="store_true")
    p.add_argument("--convert_to_8bit", action="store_true")
    p.add_argument("--bit_shift_to_right", type=int, default=8)
    p.add_argument("--continue_process", action="store_true")
    p.add_argument("--dtype", default=None)
    p.add_argument("--tile_size", type=int, nargs=2, default=None, metavar=("NY", "NX"))
    p.add_argument("--size_y", type=int, default=None, help="new image size in Y axis (with --size_x): every tile is resized to it")
    p.add_argument("--size_x", type=int, default=None, help="new image size in X axis (with --size_y)")
    p.add_argument("--gaussian_filter_2d", action="store_true", help="accepted; does nothing, as in the reference")
    p.add_argument("--max_batch", type=int, default=None, help="tiles per launch (default: from the free device memory)")
    p.add_argument("--bleach_correction_frequency", type=float, default=None,
                   help="bleach correction: cutoff of the low-pass as a fraction of the Nyquist frequency, in (0, 1); 1 / tile size is usual")
    for name, what in (("min", "background vs foreground threshold"), ("med", "intermediate foreground value (it also replaces exact zeros)"),
                       ("max", "largest foreground value")):
        p.add_argument(f"--bleach_correction_clip_{name}", type=float, default=None,
                       help=f"bleach correction: {what}, in log1p units (log1p of the intensity); all three clips are required unless --estimate_clips fills them or --extended estimates them per tile")
    p.add_argument("--bleach_correction_max_method", action=argparse.BooleanOptionalAction, default=True,
                   help="bleach correction from the filtered row and column maxima (default) rather than from every filtered row")
    p.add_argument("--extended", action="store_true",
                   help="batch_filter(extended=True): a bleach clip that is not given is estimated per tile, --down_sample_method median, "
                        "--threshold and the --padding_mode values constant, linear_ramp, maximum, mean, median and minimum are accepted")
    p.add_argument("--estimate_clips", action="store_true",
                   help="with --bleach_correction_frequency: take the clips that are not given from the slices of --input at 25 %%, 50 %% and "
                        "75 %% of the depth (four-class multi-Otsu of the log1p image, as process_images.py does) and print them")
    a = p.parse_args(argv)
    if a.estimate_clips and a.bleach_correction_frequency is None:
        p.error("--estimate_clips fills the bleach-correction clips: --bleach_correction_frequency must be given")
    return a


def _estimated_clips(a, estimate=None):
    """The three clips of the command line; with --estimate_clips those not given come from ``estimate_slice_params`` on --input."""
    clips = {name: getattr(a, name) for name in BLEACH_CLIPS}
    if a.estimate_clips and any(v is None for v in clips.values()):
        if estimate is None:
            from .thresholds import estimate_slice_params as estimate
        found = estimate(a.input, need_bleach_correction=True, need_16bit_to_8bit_conversion=False)
        clips = {name: found[name] if value is None else value for name, value in clips.items()}
        print("pystripe: " + ", ".join(f"--{name}={value!r}" for name, value in clips.items()))
    return clips


def _cli_wavelet(a):
    """``wavelet=`` of the command line: the name, or the coefficients of --wavelet_file."""
    return wavelets.load_file(a.wavelet_file) if a.wavelet_file else a.wavelet


def _cli_new_size(a):
    """``new_size=`` of the command line: (--size_y, --size_x), None without both; one alone is the reference's error."""
    if (a.size_y is None) != (a.size_x is None):
        print("both new_size_x and new_size_y are needed!")
        raise RuntimeError("both new_size_x and new_size_y are needed! (--size_y and --size_x go together)")
    return None if a.size_y is None else (a.size_y, a.size_x)


def main(argv=None):
    a = _parse_args(argv)
    new_size = _cli_new_size(a)
    inp = Path(a.input)
    out = Path(a.output) if a.output else inp.parent / (inp.name + "_destriped")
    flat = None
    if a.flat:
        flat = imread_tif_raw_png(Path(a.flat))
        if flat is None:
            raise SystemExit(f"--flat={a.flat}: cannot be read")
    clips = _estimated_clips(a)
    stats = {}
    rc = batch_filter(inp, out, flat=flat, gaussian_filter_2d=a.gaussian_filter_2d, sigma=(a.sigma1, a.sigma2), level=a.level,
                      wavelet=_cli_wavelet(a), crossover=a.crossover, threshold=a.threshold, padding_mode=a.padding_mode,
                      bidirectional=a.bidirectional, bleach_correction_frequency=a.bleach_correction_frequency,
                      bleach_correction_max_method=a.bleach_correction_max_method, dark=a.dark, rotate=a.rotate, flip_upside_down=a.flip_upside_down,
                      lightsheet=a.lightsheet, artifact_length=a.artifact_length, background_window_size=a.background_window_size,
                      percentile=a.percentile, lightsheet_vs_background=a.lightsheet_vs_background, convert_to_16bit=a.convert_to_16bit, convert_to_8bit=a.convert_to_8bit,
                      bit_shift_to_right=a.bit_shift_to_right, continue_process=a.continue_process, d_type=a.dtype,
                      tile_size=tuple(a.tile_size) if a.tile_size else None, down_sample=tuple(a.down_sample) if a.down_sample else None,
                      new_size=new_size, down_sample_method=a.down_sample_method, compression=(a.compression_method, a.compression_level),
                      max_batch=a.max_batch, stats=stats, extended=a.extended, **clips)
    print("pystripe: {files} files, {written} written, {skipped_existing} already there, {skipped_unreadable} unreadable, "
          "{zero_tiles} zero tiles; read {read_s:.2f} s, compute {compute_s:.2f} s, write {write_s:.2f} s".format(**stats))
    return rc


if __name__ == "__main__":
    sys.exit(main())
