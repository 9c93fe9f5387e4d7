#!/usr/bin/env python3
"""The slice estimates of the pipeline on the GPU: multi-Otsu clips, the bit shift of the 8-bit conversion and ``dark``
(``process_images.py:594-655``, ``estimate_img_related_params``, and ``:320-331``, ``estimate_bit_shift``).

    from ipp_amd.thresholds import estimate_slice_params
    params = estimate_slice_params("stitched_slices/")        # or a [nz, ny, nx] u8 / u16 array or device tensor
    process_img(tile, bleach_correction_frequency=1 / 64, **params)

``threshold_multiotsu`` has scikit-image's signature for the case the pipeline uses: a float32 image, 256 bins, up to four
classes.  Parity is with a numpy restatement of scikit-image's function and with ``numpy.histogram`` /
``numpy.percentile`` themselves, not with scikit-image, which is installed on neither machine: the threshold *indices* are equal to
the restatement's and the thresholds bit-equal.  Refused by name: ``hist=``, ``nbins`` other than 256, more than four classes,
integer and float64 images (scikit-image bins integers by value).

``estimate_slice_params`` counts the codes of the u8 / u16 slices on the device (``mi_code_hist``); everything in log units then
comes from those counts and the table ``numpy.log1p(arange(n), dtype=float32)`` with numpy's own arithmetic on the host (the range,
``numpy.histogram``'s 256 bins, the percentile of the samples above ``clip_max``), so that the device's ``log1pf`` never enters, and
the search runs on the device again (``mi_multiotsu_search``).  There is no CPU path for the counting and the search.
"""
from __future__ import annotations

import math
import os
import sys
from pathlib import Path

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = "ipp_amd"

from . import capi  # noqa: E402

NBINS = 256          # MI_HIST_BINS
MAX_CLASSES = 4      # MI_OTSU_MAX_CLASSES
_CODES = {np.dtype(np.uint8): (capi.CODES_U8, 256), np.dtype(np.uint16): (capi.CODES_U16, 65536)}
_TABLES = {}


def _refuse(name, value, why):
    raise NotImplementedError(f"{name}={value!r}: {why}")


def _too_few(nvalues, classes):
    return ValueError(f"After discretization into bins, the input image has only {nvalues} different values. "
                      f"It cannot be thresholded in {classes} classes.")


def _check_multiotsu(image, classes, nbins, hist):
    """The refusals and errors of threshold_multiotsu that need no device."""
    if hist is not None:
        _refuse("hist", "<given>", "a precomputed histogram is not built; pass the image")
    if image is None:
        raise ValueError("Either `image` or `hist` must be provided.")
    if nbins != NBINS:
        _refuse("nbins", nbins, f"only {NBINS} bins are built")
    if int(classes) != classes or classes < 2:
        raise ValueError(f"classes={classes!r}: an integer, 2 or more, is expected")
    if classes > MAX_CLASSES:
        _refuse("classes", classes, f"up to {MAX_CLASSES} classes are built")
    name = str(image.dtype).replace("torch.", "")
    if name != "float32":
        _refuse("image.dtype", name, "only float32 images are built (scikit-image bins integer images by value; the pipeline "
                "passes the float32 log1p image)")


# ---------------------------------------------------------------------------------------------------------------------------------
# the three device entries (include/mi_thresholds.h)

def _to_device(a, device):
    """numpy array or tensor -> contiguous device tensor (a contiguous view keeps its own, possibly unaligned, base)"""
    import torch
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            capi.require_gpu()
            a = a.to(torch.device(device if device is not None else "cuda:0"))
        return a.contiguous()
    capi.require_gpu()
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(torch.device(device if device is not None else "cuda:0"))


def _index(t):
    return t.device.index or 0


def hist256(images, device=None):
    """``numpy.histogram(image, 256)`` of every float32 image of ``images`` [n, ...] on the device (``mi_hist256_f32``).
    Returns numpy arrays: range [n, 2], nonfinite [n], edges [n, 257], counts [n, 256] (int64)."""
    import torch
    t = _to_device(images, device)
    if t.dtype != torch.float32 or t.dim() < 2 or t[0].numel() == 0:
        raise ValueError("hist256: a float32 stack [n, ...] of non-empty images is expected")
    n = int(t.shape[0])
    rng = torch.empty((n, 2), dtype=torch.float32, device=t.device)
    bad = torch.empty((n,), dtype=torch.int32, device=t.device)
    edges = torch.empty((n, NBINS + 1), dtype=torch.float32, device=t.device)
    counts = torch.empty((n, NBINS), dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        capi.check(capi.lib().mi_hist256_f32(_index(t), capi.current_stream_ptr(t.device), t.data_ptr(), n, t[0].numel(), rng.data_ptr(),
                                             bad.data_ptr(), edges.data_ptr(), counts.data_ptr()))
    return rng.cpu().numpy(), bad.cpu().numpy(), edges.cpu().numpy(), counts.cpu().numpy()


def code_hist(images, device=None):
    """Occurrences of every code of the u8 / u16 images ``images`` [n, ...] (``mi_code_hist``): int64 [n, 256] or [n, 65536]."""
    import torch
    t = _to_device(images, device)
    dt = np.dtype(str(t.dtype).replace("torch.", ""))
    if dt not in _CODES or t.dim() < 2 or t[0].numel() == 0:
        raise ValueError(f"code_hist: a uint8 or uint16 stack [n, ...] of non-empty images is expected, got {dt} {tuple(t.shape)}")
    code, ncodes = _CODES[dt]
    n = int(t.shape[0])
    counts = torch.empty((n, ncodes), dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        capi.check(capi.lib().mi_code_hist(_index(t), capi.current_stream_ptr(t.device), t.data_ptr(), code, n, t[0].numel(), counts.data_ptr()))
    return counts.cpu().numpy()


def multiotsu_search(counts, classes, device=None):
    """The multi-Otsu search over histograms ``counts`` [n, 256] (``mi_multiotsu_search``).  Returns numpy arrays: indices
    [n, classes - 1], nvalues [n], status [n] (capi.OTSU_*)."""
    import torch
    if not isinstance(counts, torch.Tensor):
        counts = np.ascontiguousarray(counts, dtype=np.int64)
    t = _to_device(counts, device)
    if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != NBINS:
        raise ValueError(f"multiotsu_search: int64 counts [n, {NBINS}] are expected")
    n = int(t.shape[0])
    idx = torch.empty((n, MAX_CLASSES - 1), dtype=torch.int32, device=t.device)
    nvalues = torch.empty((n,), dtype=torch.int32, device=t.device)
    status = torch.empty((n,), dtype=torch.int32, device=t.device)
    work = torch.empty((n,), dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        capi.check(capi.lib().mi_multiotsu_search(_index(t), capi.current_stream_ptr(t.device), t.data_ptr(), n, int(classes), idx.data_ptr(),
                                                  nvalues.data_ptr(), status.data_ptr(), work.data_ptr()))
    return idx.cpu().numpy()[:, :classes - 1].astype(np.intp), nvalues.cpu().numpy(), status.cpu().numpy()


def bin_centers(edges):
    """centers of numpy.histogram's bins as scikit-image takes them: (edges[:-1] + edges[1:]) / 2, float32 for float32 edges"""
    return (edges[..., :-1] + edges[..., 1:]) / 2


# ---------------------------------------------------------------------------------------------------------------------------------
# scikit-image's entry

def threshold_multiotsu_batch(stack, classes=3, device=None):
    """``threshold_multiotsu`` of every image of the float32 stack [n, ...] in one pass: float32 [n, classes - 1].  An addition."""
    _check_multiotsu(stack, classes, NBINS, None)
    _, bad, edges, counts = hist256(stack, device)
    if bad.any():
        raise ValueError(f"autodetected range of image {int(np.flatnonzero(bad)[0])} is not finite")
    idx, nvalues, status = multiotsu_search(counts, classes, device)
    short = np.flatnonzero(status == capi.OTSU_TOO_FEW_VALUES)
    if short.size:
        raise _too_few(int(nvalues[short[0]]), classes)
    return np.take_along_axis(bin_centers(edges), idx, axis=1).astype(np.float32)


def threshold_multiotsu(image=None, classes=3, nbins=256, *, hist=None, device=None):
    """``skimage.filters.threshold_multiotsu`` for a float32 image of any shape, numpy or device tensor: the ``classes - 1``
    thresholds as a float32 numpy array.  ValueError as there (fewer occupied bins than classes, a range that is not finite)."""
    _check_multiotsu(image, classes, nbins, hist)
    if int(np.prod(tuple(image.shape))) == 0:
        raise ValueError("threshold_multiotsu: the image is empty")
    return threshold_multiotsu_batch(image.reshape(1, -1), classes, device)[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# host arithmetic on code counts (numpy's own; no device)

def log_table(ncodes):
    """log1p of every code as numpy takes it in float32: the log image of an integer slice holds these values and no others"""
    if ncodes not in _TABLES:
        _TABLES[ncodes] = np.log1p(np.arange(ncodes), dtype=np.float32)
    return _TABLES[ncodes]


def log_histogram_of_codes(code_counts):
    """``numpy.histogram(numpy.log1p(img, dtype=float32), 256)`` from the counts per code of ``img``: (int64 counts, float32 edges).
    The range is the table's value at the first and last occupied code, and numpy bins the table itself, weighted by the counts
    (exact in float64 below 2^53)."""
    counts = np.asarray(code_counts)
    table = log_table(counts.size)
    occupied = np.flatnonzero(counts)
    if occupied.size == 0:
        raise ValueError("log_histogram_of_codes: no sample")
    lo, hi = table[occupied[0]], table[occupied[-1]]
    hist, edges = np.histogram(table, NBINS, range=(lo, hi), weights=counts.astype(np.float64))
    return np.rint(hist).astype(np.int64), edges


def percentile_of_sorted(order_statistic, n, percentile):
    """``numpy.percentile(a, percentile)`` (method 'linear') of a float32 array of ``n`` samples known only through
    ``order_statistic(k)``, its k-th smallest value -- numpy's arithmetic step by step: for float32 data the quantile and the
    virtual index are float32 too, which is coarse for many samples, and this keeps that."""
    q = np.asanyarray(np.true_divide(percentile, np.float32(100)))
    if not (0 <= q <= 1):
        raise ValueError("Percentiles must be in the range [0, 100]")
    virtual = np.asanyarray((n - 1) * q)
    previous = np.floor(virtual)
    if virtual >= n - 1:
        k0 = k1 = n - 1
        previous = np.float32(-1)   # as numpy's index -1; the two neighbours are equal, so gamma does not matter
    elif virtual < 0:
        k0 = k1 = 0
        previous = np.float32(0)
    else:
        k0 = int(previous)
        k1 = k0 + 1
    gamma = np.asanyarray(virtual - np.intp(previous), dtype=virtual.dtype)
    a, b = np.float32(order_statistic(k0)), np.float32(order_statistic(k1))
    diff = np.subtract(b, a)
    if gamma >= 0.5:
        return np.float32(np.subtract(b, diff * (1 - gamma)))
    return np.float32(np.add(a, diff * gamma))


def masked_percentile_of_codes(code_counts, threshold, percentile):
    """``numpy.percentile(img_log[img_log > threshold], percentile)`` from the counts per code, ``numpy.max(img_log)`` when no sample
    lies above the threshold (process_images.py:320-324)."""
    counts = np.asarray(code_counts)
    table = log_table(counts.size)
    occupied = np.flatnonzero(counts)
    codes = occupied[table[occupied] > threshold]
    if codes.size == 0:
        return table[occupied[-1]]
    ends = np.cumsum(counts[codes].astype(np.int64))   # samples up to and including each code
    return percentile_of_sorted(lambda k: table[codes[np.searchsorted(ends, k, side="right")]], int(ends[-1]), percentile)


def bit_shift_of_upper_bound(upper_bound_log):
    """the smallest b in 0 .. 8 with 256 * 2^b >= round(expm1(upper bound)), 8 when there is none (process_images.py:325-331)"""
    upper_bound = int(np.round(np.expm1(upper_bound_log)))
    for b in range(9):
        if 256 * 2 ** b >= upper_bound:
            return b
    return 8


def estimate_bit_shift(img, threshold, percentile=99.9, device=None):
    """``estimate_bit_shift`` of process_images.py on a float32 log image, numpy or device tensor."""
    import torch
    name = str(img.dtype).replace("torch.", "")
    if name != "float32":
        _refuse("img.dtype", name, "only float32 log images are built")
    rng, bad, _, _ = hist256(img.reshape(1, -1), device)
    # This general entry takes the exact percentile of the samples above the threshold on the host with numpy; the device gives
    # the range.  The pipeline's path (estimate_slice_params) never copies a slice back: it works from the code counts.
    host = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    above = host[host > threshold]
    upper = np.percentile(above, percentile) if above.size else (np.float32(np.nan) if bad[0] else rng[0, 1])
    return bit_shift_of_upper_bound(upper)


# ---------------------------------------------------------------------------------------------------------------------------------
# process_images.py:594-655

class SliceParams(dict):
    """The keywords ``process_img`` / ``batch_filter`` take (so ``**params`` works), with the slices they came from beside them."""
    slices = ()

    def as_json(self):
        return dict(self, slices=list(self.slices))


class _Slices:
    """A folder of 2-D slices (natural order, the library's TIFF reader), a [nz, ny, nx] array / tensor or an ``ipp_amd.tsv.TSVVolume``
    (process_images.py:610-615; its planes are merged on the device and stay there), one slice at a time."""

    def __init__(self, source):
        from .tsv import TSVVolume
        self.files = self.stack = self.volume = None
        if isinstance(source, TSVVolume):
            self.volume = source
        elif isinstance(source, (str, os.PathLike)):
            from .parallel_image_processor import natural_sorted
            from .pystripe import SUPPORTED_EXTENSIONS
            path = Path(source)
            names = [path] if path.is_file() else [f for f in path.iterdir() if f.is_file() and f.suffix.lower() in SUPPORTED_EXTENSIONS]
            self.files = [Path(f) for f in natural_sorted([str(f) for f in names])]
            if not self.files:
                raise ValueError(f"estimate_slice_params: no .tif / .tiff / .raw / .png file in {source}")
        else:
            if len(source.shape) != 3:
                raise ValueError(f"estimate_slice_params: a folder or a stack [nz, ny, nx] is expected, got shape {tuple(source.shape)}")
            self.stack = source

    def __len__(self):
        if self.volume is not None:
            return int(self.volume.volume.shape[0])
        return len(self.files) if self.files is not None else int(self.stack.shape[0])

    def __getitem__(self, z):
        if self.volume is not None:
            from .tsv import VExtent
            v = self.volume.volume
            return self.volume.imread_device(VExtent(v.x0, v.x1, v.y0, v.y1, v.z0 + z, v.z0 + z + 1))[0]
        if self.stack is not None:
            return self.stack[z]
        from .pystripe import imread_tif_raw_png
        img = imread_tif_raw_png(self.files[z])
        if img is None:
            raise ValueError(f"estimate_slice_params: {self.files[z]} cannot be read")
        return img


def _stacked(images):
    """equally shaped slices -> one [n, ny, nx] array, or tensor when every slice is one (copied with copy_, which every dtype has)"""
    import torch
    if all(isinstance(i, torch.Tensor) for i in images):
        out = torch.empty((len(images),) + tuple(images[0].shape), dtype=images[0].dtype, device=images[0].device)
        for k, img in enumerate(images):
            out[k].copy_(img)
        return out
    return np.stack([i.detach().cpu().numpy() if isinstance(i, torch.Tensor) else np.asarray(i) for i in images])


def _estimate_from_counts(code_counts, device):
    """[(clips float32[3], bit shift) or None] for every row of counts per code; None where the reference would move on to the next
    slice: a uniform slice, or fewer than four occupied bins."""
    results = [None] * len(code_counts)
    rows, hists, centers = [], [], []
    for k, counts in enumerate(code_counts):
        if np.count_nonzero(counts) < 2:   # is_uniform_2d
            continue
        hist, edges = log_histogram_of_codes(counts)
        rows.append(k)
        hists.append(hist)
        centers.append(bin_centers(edges))
    if rows:
        idx, _, status = multiotsu_search(np.stack(hists), MAX_CLASSES, device)
        for j, k in enumerate(rows):
            if status[j] == capi.OTSU_TOO_FEW_VALUES:
                continue
            clips = centers[j][idx[j]].astype(np.float32)
            upper = masked_percentile_of_codes(code_counts[k], clips[2], 99.99)
            results[k] = (clips, bit_shift_of_upper_bound(upper))
    return results


def estimate_slice_params(source, need_bleach_correction=True, need_16bit_to_8bit_conversion=True, device=None):
    """``estimate_img_related_params`` of process_images.py: four-class multi-Otsu of the log1p image of the slices at 25 %, 50 % and
    75 % of the depth, the bit shift of each at the 99.99th percentile of the samples above ``clip_max``.  A uniform slice, or one
    multi-Otsu cannot split, moves that index up by one (past the last slice: ValueError).  Returns the largest bit shift, the
    clips of the LAST slice (the reference overwrites them in its loop) and ``dark = round(expm1(clip_min))`` as the keywords of
    ``process_img``; ``.slices`` are the three indices used.  ``source``: a folder of u8 / u16 slices, a [nz, ny, nx] array / tensor, or an
    ``ipp_amd.tsv.TSVVolume``."""
    params = SliceParams(bleach_correction_clip_min=None, bleach_correction_clip_med=None, bleach_correction_clip_max=None,
                         bit_shift_to_right=8, dark=0)
    if not (need_16bit_to_8bit_conversion or need_bleach_correction):
        return params
    slices = _Slices(source)
    nz = len(slices)
    z = [math.floor(nz * 0.25), math.floor(nz * 0.5), math.floor(nz * 0.75)]

    def check(img, at):
        dt = np.dtype(str(img.dtype).replace("torch.", ""))
        if dt not in _CODES or len(img.shape) != 2:
            _refuse("slice", f"{dt} {tuple(img.shape)} at index {at}", "2-D uint8 or uint16 slices are built")
        return img

    def one(img):
        return _estimate_from_counts(code_hist(_stacked([img]), device), device)[0]

    images = [check(slices[i], i) for i in z]
    if len({(tuple(i.shape), str(i.dtype)) for i in images}) == 1:   # the usual case: one launch for the three
        found = _estimate_from_counts(code_hist(_stacked(images), device), device)
    else:
        found = [one(img) for img in images]
    for i in range(3):
        while found[i] is None:
            z[i] += 1
            if z[i] >= nz:
                raise ValueError(f"estimate_slice_params: no slice from index {z[i] - 1} on can be split into four classes")
            found[i] = one(check(slices[z[i]], z[i]))
    clips = found[2][0]
    params.update(bleach_correction_clip_min=float(clips[0]), bleach_correction_clip_med=float(clips[1]),
                  bleach_correction_clip_max=float(clips[2]), bit_shift_to_right=max(f[1] for f in found))
    if need_bleach_correction:
        params["dark"] = int(np.round(np.expm1(clips[0])))
    params.slices = list(z)
    return params


def _parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="thresholds.py", allow_abbrev=False,
                                description="clips, bit shift and dark of a folder of stitched slices, as JSON")
    p.add_argument("--input", "-i", required=True, help="folder of 2-D uint8 / uint16 slices")
    p.add_argument("--no_bleach_correction", action="store_true", help="dark stays 0")
    p.add_argument("--device", default=None)
    return p.parse_args(argv)


def main(argv=None):
    import json
    a = _parse_args(argv)
    print(json.dumps(estimate_slice_params(a.input, need_bleach_correction=not a.no_bleach_correction, device=a.device).as_json()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
