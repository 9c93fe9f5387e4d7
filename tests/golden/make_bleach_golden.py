#!/usr/bin/env python3
"""Golden fixtures of the bleach correction from the reference's OWN ``pystripe.core`` (build container only: it reads the reference
tree through ``tests/pystripe_util.import_reference``, whose stand-ins are described in tests/golden/make_pystripe_golden.py;
scipy's ``butter`` and ``sosfiltfilt`` are the installed ones).

tests/golden/bleach/<case>.npz, fields as in tests/golden/pystripe:
    img, kwargs, out    the input tile, the JSON of the keyword arguments given to process_img, the reference's result
    log32               the reference's log-domain image just before expm1 (after correct_bleaching)
    log64               the same from the float64 run of the restatement (tests/bleach_util.py)
    e_ref               max |log32 - log64|, floored at one float32 spacing of the largest |log64| (e_ref_raw: before the floor)
    frac_ref            share of pixels on which the reference's result differs from the float64 restatement's (asserted < 0.5 %)
tests/golden/bleach/refusals.npz: the calls the reference itself refuses (exception type and message).
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import bleach_util as B  # noqa: E402
from tests import pystripe_util as U  # noqa: E402

OUT = B.golden_dir(ROOT)
PIPE = dict(wavelet="db9", padding_mode="reflect", bidirectional=True)


def tile(shape, seed, dtype="uint16", stripes="rows"):
    return U.synthetic_tile(shape, seed, np.dtype(dtype), stripes)


def zero_block():
    img = tile((41, 60), 57)
    img[10:25, 20:45] = 0
    img[30, :] = 0          # a whole row of zeros as well
    return img


def bleach(frequency, max_method=False, **clips):
    return dict(bleach_correction_frequency=frequency, bleach_correction_max_method=max_method, **clips)


# name -> (input, keyword arguments without the clips, overrides of the clips)
CASES = {}
for mm in (False, True):
    tag = "max" if mm else "rows"
    CASES[f"u16_nofilter_{tag}"] = (tile((37, 53), 51), dict(sigma=(0, 0), **bleach(1 / 32, mm)), {})
    CASES[f"u16_filter_{tag}"] = (tile((97, 128), 52), dict(PIPE, sigma=(16, 16), **bleach(1 / 64, mm)), {})
CASES.update({
    "u16_odd_padding": (tile((75, 101), 53), dict(PIPE, sigma=(16, 16), **bleach(1 / 64)), {}),
    "u16_min_row": (tile((9, 7), 54), dict(sigma=(0, 0), **bleach(1 / 4)), {}),
    "u16_min_column_max": (tile((7, 11), 55), dict(sigma=(0, 0), **bleach(1 / 4, True)), {}),
    "u16_zero_block": (zero_block(), dict(sigma=(0, 0), **bleach(1 / 32)), {}),
    "u16_zero_block_max": (zero_block(), dict(sigma=(0, 0), **bleach(1 / 32, True)), {}),
    "u16_clip_min_zero": (tile((37, 53), 51), dict(sigma=(0, 0), **bleach(1 / 32)), dict(bleach_correction_clip_min=0.0)),
    "u16_row64_half": (tile((1, 64), 58, stripes="cols"), dict(sigma=(0, 0), **bleach(0.5)), {}),
    "u16_row64_long_memory": (tile((1, 64), 58, stripes="cols"), dict(sigma=(0, 0), **bleach(1 / 2000)), {}),
    "f32_tail": (tile((37, 53), 59, "float32"), dict(sigma=(0, 0), dark=150, convert_to_8bit=True, bit_shift_to_right=4, rotate=90,
                                                     **bleach(1 / 32)), {}),
    "u8_tile": (tile((37, 53), 60, "uint8"), dict(sigma=(0, 0), **bleach(1 / 32)), {}),
})


def main():
    pc = U.import_reference("/root/reference")
    os.makedirs(OUT, exist_ok=True)
    seen = {}
    real_expm1 = pc.expm1_jit

    def watch_expm1(img, *a, **k):
        seen["log32"] = np.array(img, copy=True)
        return real_expm1(img, *a, **k)

    pc.expm1_jit = watch_expm1
    total = 0
    for name, (img, kw, override) in CASES.items():
        seen.clear()
        kwargs = dict(kw, **dict(B.clips_for(img), **override))
        assert kwargs["bleach_correction_clip_min"] < kwargs["bleach_correction_clip_med"] < kwargs["bleach_correction_clip_max"], name
        out = pc.process_img(img.copy(), **kwargs)
        r32, l32 = B.process_img(img.copy(), dt=np.float32, **kwargs)
        r64, l64 = B.process_img(img.copy(), dt=np.float64, **kwargs)
        assert out.shape == r64.shape and out.dtype == r64.dtype, (name, out.shape, out.dtype, r64.shape, r64.dtype)
        frac = float((out.astype(np.float64) != r64.astype(np.float64)).mean())
        raw = float(np.abs(seen["log32"].astype(np.float64) - l64).max())
        own = float(np.abs(l32.astype(np.float64) - l64).max())
        e_ref = max(raw, B.e_ref_floor(l64))
        line = (f"{name:26s} out {out.shape} {out.dtype} ref-vs-f64 differ {100 * frac:.3f} % | E_ref {raw:.3g} floored {e_ref:.3g} "
                f"(restatement f32 {own:.3g}; f32 restatement == reference: {np.array_equal(l32, seen['log32'])})")
        assert frac < 0.005, line
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, img=img, out=out, kwargs=np.array(json.dumps(kwargs)), log32=seen["log32"], log64=l64,
                            e_ref=np.float64(e_ref), e_ref_raw=np.float64(raw), frac_ref=np.float64(frac))
        size = os.path.getsize(path)
        total += size
        assert size < 1 << 20, (name, size)
        print(line, f"| {size / 1024:.0f} KiB")

    # what the reference itself refuses
    img = tile((37, 53), 51)
    clips = B.clips_for(img)
    refusals = {}

    def refuse(name, f):
        try:
            f()
            refusals[name] = ["", ""]
        except Exception as e:  # noqa: BLE001
            refusals[name] = [type(e).__name__, str(e)]

    run = lambda im=img, **k: pc.process_img(im.copy(), **dict(dict(sigma=(0, 0), **bleach(1 / 32), **clips), **k))  # noqa: E731
    refuse("int_clip", lambda: run(bleach_correction_clip_max=9))
    refuse("int_frequency", lambda: run(bleach_correction_frequency=1))
    refuse("med_not_above_min", lambda: run(bleach_correction_clip_med=clips["bleach_correction_clip_min"]))
    refuse("max_not_above_med", lambda: run(bleach_correction_clip_max=clips["bleach_correction_clip_med"]))
    refuse("negative_min", lambda: run(bleach_correction_clip_min=-0.5))
    refuse("frequency_one", lambda: run(bleach_correction_frequency=1.0))
    refuse("frequency_above_one", lambda: run(bleach_correction_frequency=1.5))
    refuse("nx_6", lambda: run(tile((9, 6), 61)))
    refuse("nx_7", lambda: run(tile((9, 7), 61)))
    refuse("ny_6_max_method", lambda: run(tile((6, 9), 62), bleach_correction_max_method=True))
    refuse("ny_6_rows", lambda: run(tile((6, 9), 62)))
    np.savez_compressed(os.path.join(OUT, "refusals.npz"), refusals=np.array(json.dumps(refusals)))
    print(json.dumps(refusals, indent=1))
    print(f"total {total / 1e3:.0f} kB in {len(CASES)} cases; float32 spacing floor, LDS row limit {B.LDS_ROW}, log1p(1) = {math.log1p(1):.6f}")


if __name__ == "__main__":
    main()
