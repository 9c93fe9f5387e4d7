#!/usr/bin/env python3
"""Golden fixtures of the lightsheet correction from the reference's OWN ``pystripe/lightsheet_correct.py`` and ``process_img``
(build container only: it reads the reference tree; ``tests/pystripe_util.install_standins`` supplies ``numba.njit`` and the other
missing imports, none of which takes part in this step).

tests/golden/lightsheet/<case>.npz:
    img, flat         the input tile (and the normalised flat field, when the case has one)
    kind              'correct' (the reference's correct_lightsheet as process_img calls it) or 'process' (its process_img)
    kwargs            JSON of the keyword arguments
    out               the reference's result
    ls, bg            'correct' cases: its full-size lightsheet and background maps
    ls_grid, bg_grid  'correct' cases: the two sub-grids (local_percentile(..., interpolate=None))
    e_out, e_ls, e_bg float32 cases ('process': e_out alone): the reference's own largest distance from the restatement run on the float64 copy of the tile
                      (E_ref of the float standard; the tests recompute the float64 run)
tests/golden/lightsheet/<case>_maps.npz: ``ls`` and ``bg`` of a float32 case (a file of their own to stay under 1 MB)
Every case is also run through the restatement of tests/lightsheet_util.py, which must equal the reference exactly.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import lightsheet_util as L  # noqa: E402
from tests import pystripe_util as U  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", L.GOLDEN_SUBDIR)

# name -> (shape, dtype, seed, keyword arguments of correct_lightsheet in process_img's terms)
CORRECT = {
    "u16_301x457": ((301, 457), "uint16", 1, {}),
    "u8_128x150_one_centre": ((128, 150), "uint8", 2, {}),
    "u16_130x310_wrap": ((130, 310), "uint16", 3, {}),
    "u16_300x634_zero_lines": ((300, 634), "uint16", 4, {}),
    "u16_25x150_one_row": ((25, 150), "uint16", 5, {}),
    "u16_49x1897_thin": ((49, 1897), "uint16", 6, {}),
    "u16_608x170_thin": ((608, 170), "uint16", 7, {}),
    "f32_97x331": ((97, 331), "float32", 8, {}),
    "f32_257x449": ((257, 449), "float32", 9, {}),
    "u16_factor_2p9": ((213, 600), "uint16", 10, dict(lightsheet_vs_background=2.9)),
    "f32_factor_2p9": ((97, 331), "float32", 11, dict(lightsheet_vs_background=2.9)),
    "u16_percentile_0p5": ((213, 600), "uint16", 12, dict(percentile=0.5)),
    "u16_percentile_0p03": ((213, 600), "uint16", 13, dict(percentile=0.03)),
    "u16_length_64": ((213, 600), "uint16", 14, dict(artifact_length=64)),
    "u16_length_151": ((213, 600), "uint16", 15, dict(artifact_length=151)),
    "u16_window_100": ((213, 600), "uint16", 16, dict(background_window_size=100)),
    "u16_window_51": ((213, 600), "uint16", 17, dict(background_window_size=51)),
}
# process_img without the stripe filter
PROCESS = {
    "pi_dark_120": ((257, 449), "uint16", 20, dict(dark=120)),
    "pi_dark_2p5": ((257, 449), "uint16", 21, dict(dark=2.5)),
    "pi_8bit_shift4": ((257, 449), "uint16", 22, dict(convert_to_8bit=True, bit_shift_to_right=4)),
    "pi_rot90_flip": ((257, 449), "uint16", 23, dict(rotate=90, flip_upside_down=True)),
    "pi_down_2x2": ((301, 700), "uint16", 24, dict(down_sample=(2, 2))),
    "pi_f32_flat": ((257, 449), "float32", 25, dict(flat=True)),
    "pi_uniform": ((60, 320), "uint16", 26, dict(rotate=90)),
}


def make_input(name, shape, dtype, seed):
    if name == "pi_uniform":
        return np.full(shape, 7, np.dtype(dtype))
    img = L.bead_and_stripe_tile(shape, seed, np.dtype(dtype))
    if "factor" in name:           # rows whose lightsheet estimate exceeds twice the background, so that the factor decides
        img[::7] += 1500
    if name.endswith("_wrap"):     # a background above 32767: bg * 2 wraps in uint16
        img = (40000 + (img.astype(np.int64) * 7) % 20000).astype(np.uint16)
    return img


def reference_correct(lc, img, percentile=0.25, artifact_length=150, background_window_size=200, lightsheet_vs_background=2.0):
    d_type = img.dtype
    ls_kw = dict(selem=(1, artifact_length, 1), dtype=d_type)
    bg_kw = dict(selem=(background_window_size, background_window_size, 1), spacing=(25, 25, 1), interpolate=1, dtype=d_type, step=(2, 2, 1))
    out, ls, bg = lc.correct_lightsheet(img.copy(), percentile=percentile, lightsheet=ls_kw, background=bg_kw,
                                        lightsheet_vs_background=lightsheet_vs_background, return_lightsheet=True, return_background=True)
    cube = img.reshape(img.shape + (1,))
    ls_grid = lc.local_percentile(cube, percentile=percentile, **dict(ls_kw, interpolate=None))
    bg_grid = lc.local_percentile(cube, percentile=percentile, **dict(bg_kw, interpolate=None))
    return out, ls[..., 0], bg[..., 0], ls_grid[..., 0], bg_grid[..., 0]


def main():
    pc = U.import_reference("/root/reference")
    import pystripe.lightsheet_correct as lc
    os.makedirs(OUT, exist_ok=True)
    total = 0

    def save(name, arrays):
        nonlocal total
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size < 1 << 20, (name, size)
        total += size
        return size

    for name, (shape, dtype, seed, kw) in CORRECT.items():
        img = make_input(name, shape, dtype, seed)
        out, ls, bg, ls_grid, bg_grid = reference_correct(lc, img, **kw)
        mine = L.correct_lightsheet(img.copy(), **kw)
        for got, want, what in zip(mine, (out, ls, bg, ls_grid, bg_grid), ("out", "ls", "bg", "ls_grid", "bg_grid")):
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, what)
        arrays = dict(img=img, kind=np.array("correct"), kwargs=np.array(json.dumps(kw)), out=out, ls=ls, bg=bg, ls_grid=ls_grid,
                      bg_grid=bg_grid)
        line = f"{name:26s} {dtype} {shape} grids {ls_grid.shape} {bg_grid.shape} changed {100 * float((out != img).mean()):.1f} %"
        if dtype == "float32":
            o64, l64, b64 = L.correct_lightsheet(img.astype(np.float64), **kw)[:3]
            e = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in ((out, o64), (ls, l64), (bg, b64))]
            arrays.update(e_out=np.float64(e[0]), e_ls=np.float64(e[1]), e_bg=np.float64(e[2]))
            save(name + "_maps", dict(ls=arrays.pop("ls"), bg=arrays.pop("bg")))
            line += f" | E_ref out {e[0]:.3g} ls {e[1]:.3g} bg {e[2]:.3g}"
        print(line, f"| {save(name, arrays) / 1024:.0f} KiB")

    for name, (shape, dtype, seed, kw) in PROCESS.items():
        img = make_input(name, shape, dtype, seed)
        kwargs = dict(kw, lightsheet=True)
        arrays, flat = {}, None
        if kwargs.pop("flat", False):
            flat = pc.normalize_flat(0.5 + 0.5 * np.random.default_rng(seed + 1000).random(shape))
            arrays["flat"] = flat
        out = pc.process_img(img.copy(), flat=None if flat is None else flat.copy(), **kwargs)
        mine = L.process_img(img.copy(), flat=flat, **kwargs)
        assert mine.dtype == out.dtype and np.array_equal(mine, out), name
        arrays.update(img=img, kind=np.array("process"), kwargs=np.array(json.dumps(kwargs)), out=out)
        if dtype == "float32":
            o64 = L.process_img(img.astype(np.float64), flat=flat, **kwargs)
            arrays["e_out"] = np.float64(np.abs(out.astype(np.float64) - o64).max())
        print(f"{name:26s} {dtype} {shape} -> {out.dtype} {out.shape} | {save(name, arrays) / 1024:.0f} KiB")
    print(f"total {total / 1e6:.2f} MB in {len(CORRECT) + len(PROCESS)} cases")


if __name__ == "__main__":
    main()
