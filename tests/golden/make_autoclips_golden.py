#!/usr/bin/env python3
"""Golden fixtures of the bleach correction with automatic clips from the reference's OWN ``pystripe.core`` (build container only: it
reads the reference tree through ``tests/pystripe_util.import_reference``, whose stand-ins are described in
tests/golden/make_pystripe_golden.py).  scikit-image is not installed: ``threshold_multiotsu`` inside the reference is the numpy
restatement of tests/thresholds_util.py, which tests/test_thresholds_host.py holds to scikit-image's description.

tests/golden/autoclips/<case>.npz, fields as in tests/golden/bleach:
    img, kwargs, out    the input tile, the JSON of the keyword arguments given to process_img (a clip that is null is automatic),
                        the reference's result
    triple              the three clips correct_bleaching received (float32), before min is raised to log1p(1)
    log32, log64        the reference's log-domain image just before expm1; the same from the float64 restatement
                        (tests/autoclips_util.py) fed the same triple
    e_ref               max |log32 - log64|, floored at one float32 spacing of the largest |log64| (e_ref_raw: before the floor)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import autoclips_util as A  # noqa: E402
from tests import bleach_util as B  # noqa: E402
from tests import pystripe_util as U  # noqa: E402
from tests import thresholds_util as T  # noqa: E402

OUT = A.golden_dir(ROOT)
PIPE = dict(wavelet="db9", padding_mode="reflect", bidirectional=True)
AUTO = dict(bleach_correction_clip_min=None, bleach_correction_clip_med=None, bleach_correction_clip_max=None)
MED = dict(bleach_correction_clip_min=5.0, bleach_correction_clip_med=None, bleach_correction_clip_max=9.0)


def bleach(frequency, max_method=False, **clips):
    return dict(bleach_correction_frequency=frequency, bleach_correction_max_method=max_method, **clips)


CASES = {}
for mm in (False, True):
    tag = "max" if mm else "rows"
    CASES[f"u16_nofilter_{tag}"] = (T.four_mode_image((37, 53), 11), dict(sigma=(0, 0), **bleach(1 / 32, mm, **AUTO)))
    CASES[f"u16_filter_{tag}"] = (T.four_mode_image((40, 72), 12), dict(PIPE, sigma=(8, 8), **bleach(1 / 64, mm, **AUTO)))
    CASES[f"u16_med_only_{tag}"] = (T.four_mode_image((37, 53), 13), dict(sigma=(0, 0), **bleach(1 / 32, mm, **MED)))
CASES.update({
    "u8_nofilter_rows": (T.four_mode_image((37, 53), 14, np.uint8), dict(sigma=(0, 0), **bleach(1 / 32, **AUTO))),
    "u8_filter_max": (T.four_mode_image((40, 72), 15, np.uint8), dict(PIPE, sigma=(8, 8), **bleach(1 / 64, True, **AUTO))),
    "f32_nofilter_rows": (A.float_tile((37, 53), 16), dict(sigma=(0, 0), **bleach(1 / 32, **AUTO))),
    "f32_filter_rows": (A.float_tile((40, 72), 17), dict(PIPE, sigma=(8, 8), **bleach(1 / 64, **AUTO))),
    "f32_med_only_max": (A.float_tile((37, 53), 18), dict(sigma=(0, 0), **bleach(1 / 32, True, **MED))),
    "u16_tail": (T.four_mode_image((96, 128), 19), dict(sigma=(0, 0), dark=100, convert_to_8bit=True, bit_shift_to_right=4, rotate=90,
                                                        **bleach(1 / 128, **AUTO))),
})


def main():
    pc = U.import_reference("/root/reference")
    pc.threshold_multiotsu = T.threshold_multiotsu
    os.makedirs(OUT, exist_ok=True)
    seen = {}
    real_expm1, real_bleach = pc.expm1_jit, pc.correct_bleaching

    def watch_expm1(img, *a, **k):
        seen["log32"] = np.array(img, copy=True)
        return real_expm1(img, *a, **k)

    def watch_bleach(img, frequency, clip_min, clip_med, clip_max, **k):
        seen["triple"] = np.array([clip_min, clip_med, clip_max], np.float32)
        return real_bleach(img, frequency, clip_min, clip_med, clip_max, **k)

    pc.expm1_jit, pc.correct_bleaching = watch_expm1, watch_bleach
    total = 0
    for name, (img, kwargs) in CASES.items():
        seen.clear()
        out = pc.process_img(img.copy(), **kwargs)
        want = A.triple(img, **kwargs)
        assert np.array_equal(seen["triple"], want), (name, seen["triple"], want)
        if img.dtype == np.float32:
            assert A.indices_are_stable(A.log_image(img, **kwargs)), name
        r32, l32 = A.process_img(img.copy(), dt=np.float32, **kwargs)
        r64, l64 = A.process_img(img.copy(), dt=np.float64, **kwargs)
        assert out.shape == r64.shape and out.dtype == r64.dtype, (name, out.shape, out.dtype, r64.shape, r64.dtype)
        frac = float((out.astype(np.float64) != r64.astype(np.float64)).mean())
        raw = float(np.abs(seen["log32"].astype(np.float64) - l64).max())
        e_ref = max(raw, B.e_ref_floor(l64))
        line = (f"{name:22s} out {out.shape} {out.dtype} triple {tuple(float(v) for v in want)} ref-vs-f64 differ {100 * frac:.3f} % | "
                f"E_ref {raw:.3g} floored {e_ref:.3g} (f32 restatement == reference: {np.array_equal(l32, seen['log32'])})")
        # a sanity check of the maker, not a standard: the populations at 2500 and 20000 counts turn a log-domain difference of E_ref
        # into up to 0.05 counts, so a few pixels per thousand round the other way
        assert frac < 0.01 or out.dtype.kind == "f", line
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, img=img, out=out, kwargs=np.array(json.dumps(kwargs)), triple=seen["triple"], log32=seen["log32"], log64=l64,
                            e_ref=np.float64(e_ref), e_ref_raw=np.float64(raw), frac_ref=np.float64(frac))
        size = os.path.getsize(path)
        total += size
        assert size < 1 << 20, (name, size)
        print(line, f"| {size / 1024:.0f} KiB")
    print(f"total {total / 1e3:.0f} kB in {len(CASES)} cases")


if __name__ == "__main__":
    main()
