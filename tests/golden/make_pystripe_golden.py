#!/usr/bin/env python3
"""Golden fixtures of the pystripe stage from the reference's OWN ``pystripe.core`` (build container only: it reads the reference tree).

The reference imports PyWavelets, scikit-image, OpenCV, numexpr, numba, tifffile, dcimg and imageio, none of which is installed;
``tests/pystripe_util.install_standins`` puts small stand-ins into ``sys.modules`` and the reference's ``process_img`` /
``filter_streaks`` / ``filter_subband`` / ``np_filter_coefficient`` / ``calculate_pad_size`` / ``convert_to_8bit_fun`` then run
unmodified.  PARITY: pinned to the reference's code for everything except the DWT primitive (``pywt.wavedec2 / waverec2``, built
from oracle/destripe_oracle.py) and ``skimage.measure.block_reduce``, which are restatements.

tests/golden/pystripe/<case>.npz:
    img, flat         the input tile (and the normalised flat field, when the case has one)
    kwargs            JSON of the keyword arguments given to process_img
    out               the reference's result
    log32             the reference's log-domain image just before expm1 (its float32 run), when the case filters
    log64             the same from the float64 run of the restatement (tests/pystripe_util.py)
    e_ref             max |log32 - log64|
    frac_ref          share of pixels on which the reference's result differs from the float64 restatement's (asserted < 0.5 %)
    base_pad, padded, levels, coef_shapes     the bookkeeping seen inside the reference run
tests/golden/pystripe/host.npz: calculate_pad_size / convert_to_8bit_fun / normalize_flat samples and the calls the reference
itself refuses (exception type and message).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import pystripe_util as U  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", U.GOLDEN_SUBDIR)
PIPE = dict(wavelet="db9", padding_mode="reflect", bidirectional=True)

# name -> (shape, dtype, seed, stripes, kwargs)
CASES = {
    "u16_big_pipeline": ((201, 256), "uint16", 3, "rows", dict(PIPE, sigma=(32, 32))),
    "u16_odd_even": ((97, 128), "uint16", 4, "rows", dict(PIPE, sigma=(16, 16))),
    "u16_odd_odd_one_dir": ((75, 101), "uint16", 5, "rows", dict(PIPE, sigma=(16, 16), bidirectional=False)),
    "u16_dual_sigma_wrap": ((97, 128), "uint16", 6, "rows", dict(PIPE, sigma=(8, 24), padding_mode="wrap", bidirectional=False)),
    "u16_dual_sigma_bidir": ((96, 111), "uint16", 7, "cols", dict(PIPE, sigma=(24, 12))),
    "u16_symmetric": ((97, 128), "uint16", 8, "rows", dict(PIPE, sigma=(16, 16), padding_mode="symmetric")),
    "u16_edge": ((97, 128), "uint16", 9, "rows", dict(PIPE, sigma=(16, 16), padding_mode="edge")),
    "u16_level2": ((97, 128), "uint16", 10, "rows", dict(PIPE, sigma=(16, 16), level=2)),
    "u16_small34": ((21, 27), "uint16", 11, "rows", dict(PIPE, sigma=(2, 2))),
    "u16_small34b": ((9, 11), "uint16", 12, "rows", dict(PIPE, sigma=(1, 1))),
    "u8_tile": ((97, 128), "uint8", 13, "rows", dict(PIPE, sigma=(16, 16))),
    "f32_tile": ((97, 128), "float32", 14, "rows", dict(PIPE, sigma=(16, 16))),
    "f32_to16": ((97, 128), "float32", 15, "rows", dict(PIPE, sigma=(16, 16), convert_to_16bit=True)),
    "f32_flat": ((97, 128), "float32", 16, "rows", dict(PIPE, sigma=(16, 16), flat=True)),
    "u16_down_max": ((97, 128), "uint16", 17, "rows", dict(PIPE, sigma=(16, 16), down_sample=(2, 3))),
    "u16_down_min": ((97, 128), "uint16", 18, "rows", dict(PIPE, sigma=(16, 16), down_sample=(3, 2), down_sample_method="min")),
    "u16_down_mean": ((97, 128), "uint16", 19, "rows", dict(PIPE, sigma=(16, 16), down_sample=(3, 2), down_sample_method="mean")),
    "u16_dark": ((97, 128), "uint16", 20, "rows", dict(PIPE, sigma=(16, 16), dark=120)),
    "u16_dark_fraction": ((97, 128), "uint16", 21, "rows", dict(PIPE, sigma=(8, 8), dark=2.5)),
    "u16_8bit_shift0": ((97, 128), "uint16", 22, "rows", dict(PIPE, sigma=(16, 16), convert_to_8bit=True, bit_shift_to_right=0)),
    "u16_8bit_shift4": ((97, 128), "uint16", 23, "rows", dict(PIPE, sigma=(16, 16), convert_to_8bit=True, bit_shift_to_right=4)),
    "u16_8bit_shift8": ((97, 128), "uint16", 24, "rows", dict(PIPE, sigma=(16, 16), convert_to_8bit=True, bit_shift_to_right=8)),
    "u16_flip": ((97, 128), "uint16", 25, "rows", dict(PIPE, sigma=(16, 16), flip_upside_down=True)),
    "u16_rot90": ((97, 128), "uint16", 26, "rows", dict(PIPE, sigma=(16, 16), rotate=90)),
    "u16_rot180": ((97, 128), "uint16", 27, "rows", dict(PIPE, sigma=(16, 16), rotate=180)),
    "u16_flip_rot270": ((97, 128), "uint16", 28, "rows", dict(PIPE, sigma=(16, 16), flip_upside_down=True, rotate=270)),
    "u16_all": ((97, 128), "uint16", 29, "rows", dict(PIPE, sigma=(16, 16), dark=100, convert_to_8bit=True, bit_shift_to_right=4,
                                                        rotate=90, down_sample=(2, 2))),
    "u16_uniform": ((30, 40), "uint16", 30, "uniform", dict(PIPE, sigma=(16, 16), rotate=90, convert_to_8bit=True, down_sample=(2, 2))),
    "u16_nofilter": ((97, 128), "uint16", 31, "rows", dict(dark=50, convert_to_8bit=True, bit_shift_to_right=3, rotate=270,
                                                             down_sample=(2, 2), down_sample_method="mean")),
    "u16_col_stripes_one_dir": ((97, 128), "uint16", 32, "cols", dict(PIPE, sigma=(16, 16), bidirectional=False)),
    "u16_col_stripes_bidir": ((97, 128), "uint16", 32, "cols", dict(PIPE, sigma=(16, 16))),
}


def make_input(shape, dtype, seed, stripes):
    if stripes == "uniform":
        return np.full(shape, 7, np.dtype(dtype))
    return U.synthetic_tile(shape, seed, np.dtype(dtype), stripes)


def main():
    pc = U.import_reference("/root/reference")
    import pywt
    os.makedirs(OUT, exist_ok=True)
    seen = {}
    real_expm1, real_wavedec2 = pc.expm1_jit, pywt.wavedec2

    def watch_expm1(img, *a, **k):
        seen["log32"] = np.array(img, copy=True)
        return real_expm1(img, *a, **k)

    def watch_wavedec2(data, *a, **k):
        c = real_wavedec2(data, *a, **k)
        seen.setdefault("padded", data.shape)
        seen.setdefault("coef_shapes", [d[0].shape for d in c[1:]][::-1])
        return c

    pc.expm1_jit = watch_expm1
    pc.wavedec2 = watch_wavedec2
    total = 0
    for name, (shape, dtype, seed, stripes, kw) in CASES.items():
        seen.clear()
        img = make_input(shape, dtype, seed, stripes)
        kwargs = dict(kw)
        arrays = {}
        flat = None
        if kwargs.pop("flat", False):
            rng = np.random.default_rng(seed + 1000)
            flat = pc.normalize_flat(0.5 + 0.5 * rng.random(shape))
            arrays["flat"] = flat
        out = pc.process_img(img.copy(), flat=None if flat is None else flat.copy(), **kwargs)
        r32, l32 = U.process_img(img.copy(), flat=flat, dt=np.float32, **kwargs)
        r64, l64 = U.process_img(img.copy(), flat=flat, dt=np.float64, **kwargs)
        assert out.shape == r64.shape and out.dtype == r64.dtype, (name, out.shape, out.dtype, r64.shape, r64.dtype)
        arrays.update(img=img, out=out, kwargs=np.array(json.dumps(kwargs)))
        frac = float((out.astype(np.float64) != r64.astype(np.float64)).mean())
        maxd = float(np.abs(out.astype(np.float64) - r64.astype(np.float64)).max())
        line = f"{name:26s} out {out.shape} {out.dtype} ref-vs-f64 differ {100 * frac:.3f} % max {maxd:g}"
        if out.dtype.kind in "ui":
            assert frac < 0.005, line
        arrays["frac_ref"] = np.float64(frac)
        if "log32" in seen:
            e_ref = float(np.abs(seen["log32"].astype(np.float64) - l64).max())
            own = float(np.abs(l32.astype(np.float64) - l64).max())
            arrays.update(log32=seen["log32"], log64=l64, e_ref=np.float64(e_ref), padded=np.array(seen["padded"]),
                          coef_shapes=np.array(seen["coef_shapes"]), levels=np.int64(len(seen["coef_shapes"])))
            pre_shape = l64.shape
            arrays["base_pad"] = np.int64(pc.calculate_pad_size(shape=pre_shape, sigma=max(kwargs["sigma"])))
            line += f" | E_ref {e_ref:.3g} (restatement f32 {own:.3g}) padded {tuple(seen['padded'])} levels {len(seen['coef_shapes'])}"
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        total += size
        assert size < 1 << 20, (name, size)
        print(line, f"| {size / 1024:.0f} KiB")

    # host-side samples and the calls the reference itself refuses
    host = {}
    shapes = [(2048, 2048), (301, 400), (97, 128), (21, 27), (9, 11), (1850, 1850), (4096, 2304), (64, 5000)]
    sigmas = [0, 1, 2, 8, 16, 32, 100, 128, 250, 256, 512, 2000]
    host["pad_shapes"] = np.array(shapes)
    host["pad_sigmas"] = np.array(sigmas)
    host["pad_sizes"] = np.array([[pc.calculate_pad_size(shape=s, sigma=g) for g in sigmas] for s in shapes])
    ramp = np.arange(0, 65536, 7, dtype=np.uint16).reshape(-1, 3)
    host["ramp"] = ramp
    for sh in range(9):
        host[f"to8_shift{sh}"] = pc.convert_to_8bit_fun(ramp.copy(), bit_shift_to_right=sh)
    framp = np.linspace(-10, 70000, 4001).astype(np.float32).reshape(-1, 1)
    host["framp"] = framp
    host["framp_to8_shift4"] = pc.convert_to_8bit_fun(framp.copy(), bit_shift_to_right=4)
    rng = np.random.default_rng(77)
    fl = (rng.random((5, 7)) * 1000).astype(np.uint16)
    host["flat_raw"] = fl
    host["flat_norm"] = pc.normalize_flat(fl)
    tile = make_input((97, 128), "uint16", 40, "rows")
    refusals = {}

    def refuse(name, f):
        try:
            f()
            refusals[name] = ["", ""]
        except Exception as e:  # noqa: BLE001
            refusals[name] = [type(e).__name__, str(e)]

    flat = pc.normalize_flat(0.5 + 0.5 * rng.random(tile.shape))
    refuse("sigma_0_8", lambda: pc.process_img(tile.copy(), sigma=(0, 8), **PIPE))
    refuse("sigma_8_0", lambda: pc.process_img(tile.copy(), sigma=(8, 0), **PIPE))
    refuse("flat_on_u16", lambda: pc.process_img(tile.copy(), flat=flat, sigma=(8, 8), **PIPE))
    refuse("shift_9", lambda: pc.process_img(tile.copy(), sigma=(8, 8), convert_to_8bit=True, bit_shift_to_right=9, **PIPE))
    refuse("padding_bogus", lambda: pc.process_img(tile.copy(), sigma=(8, 8), wavelet="db9", padding_mode="bogus"))
    refuse("down_bogus", lambda: pc.process_img(tile.copy(), down_sample=(2, 2), down_sample_method="bogus"))
    host["refusals"] = np.array(json.dumps(refusals))
    np.savez_compressed(os.path.join(OUT, "host.npz"), **host)
    print(json.dumps(refusals, indent=1))
    print(f"total {total / 1e6:.2f} MB in {len(CASES)} cases")


if __name__ == "__main__":
    main()
