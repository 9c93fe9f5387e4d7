#!/usr/bin/env python3
"""Golden fixtures of the TeraFly conversion from the reference's OWN ``teraconverter`` binary (build container only).

Every run writes a seeded 2-D TIFF series (one file per slice, ``slice_NNNN.tif``) and converts it with

    teraconverter --sfmt="TIFF (series, 2D)" --dfmt="TIFF (tiled, 3D)" --clist=0 --noprogressbar -s=SRC -d=OUT <flags>

Stored under tests/golden/terafly/, one ``<run>.npz`` per run:

    recipe        dtype name, (D, V, H) of the series, seed: the test regenerates the input with
                  ``np.random.default_rng(seed).integers(0, 2**bits, (D, V, H))``
    input_sha     SHA-256 of the regenerated series (guards the generator)
    flags         the extra teraconverter flags of the run
    files         every file name the run wrote, relative to OUT, sorted
    mdata/<RES>   the bytes of RES(...)/mdata.bin
    pages/<file>  number of pages of each .tif, page shape, compression tag, SHA-256 of its decoded pages (C order)
    sample/<file> a seeded subset of each .tif's decoded pages (indices in sample_idx/<file>), to show a mismatch

``refused.npz`` records a run the binary refuses (too many resolutions for the volume's depth): its flags and message (the
binary prints "ERROR: ..." and still exits with status 0, leaving the empty RES directories behind).
Only data is committed: arrays, hashes, name lists and the mdata.bin bytes the binary wrote.
"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image, ImageSequence

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TC = "/root/reference/TeraStitcher/Linux/AVX2/teraconverter"
OUT = os.path.join(ROOT, "tests", "golden", "terafly")
BASE = ["--sfmt=TIFF (series, 2D)", "--dfmt=TIFF (tiled, 3D)", "--clist=0", "--noprogressbar"]

# name -> (dtype, (D, V, H), seed, flags)
RUNS = {
    "u16_012345": ("uint16", (70, 251, 263), 11, ["--resolutions=012345", "--halve=mean"]),
    "u16_tiled": ("uint16", (45, 521, 509), 12, ["--resolutions=0123", "--height=250", "--width=250", "--depth=20"]),
    "u16_max": ("uint16", (37, 271, 301), 13, ["--resolutions=0123", "--halve=max"]),
    "u8_mean": ("uint8", (45, 271, 301), 14, ["--resolutions=0123", "--halve=mean"]),
    "u8_max_tiled": ("uint8", (37, 263, 517), 15, ["--resolutions=012", "--halve=max", "--height=250", "--width=250",
                                                    "--depth=16"]),
    "u16_iso": ("uint16", (37, 271, 301), 16, ["--resolutions=0123", "--isotropic"]),
    "u16_sub": ("uint16", (45, 271, 301), 17, ["--resolutions=0123", "--V0=5", "--H0=7", "--D0=3", "--D1=40"]),
    "u16_fixed": ("uint16", (45, 521, 509), 18, ["--resolutions=012", "--height=250", "--width=250", "--depth=20",
                                                  "--fixed_tiling"]),
    "u16_uncompressed": ("uint16", (37, 271, 301), 19, ["--resolutions=0123", "--libtiff_uncompress"]),
}
REFUSED = ("uint16", (37, 256, 256), 20, ["--resolutions=012345"])
SAMPLE_PAGES = 2
SAMPLE_BUDGET = 600_000   # bytes of sample pages per run


def make_series(dtype, shape, seed):
    bits = np.dtype(dtype).itemsize * 8
    return np.random.default_rng(seed).integers(0, 2 ** bits, shape, dtype=dtype)


def write_series(vol, folder):
    os.makedirs(folder)
    for k in range(vol.shape[0]):
        Image.fromarray(vol[k]).save(os.path.join(folder, f"slice_{k:04d}.tif"))


def run(flags, src, out):
    cmd = [TC] + BASE + flags + [f"-s={src}", f"-d={out}"]
    print(" ".join(cmd), flush=True)
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def read_pages(path):
    im = Image.open(path)
    pages = np.stack([np.asarray(p) for p in ImageSequence.Iterator(im)])
    return pages, int(im.tag_v2.get(259))


def main():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    with tempfile.TemporaryDirectory() as tmp:
        for name, (dtype, shape, seed, flags) in RUNS.items():
            vol = make_series(dtype, shape, seed)
            src, out = os.path.join(tmp, name, "src"), os.path.join(tmp, name, "out")
            write_series(vol, src)
            os.makedirs(out)
            p = run(flags, src, out)
            if p.returncode != 0 or "ERROR" in p.stdout:   # the binary reports some refusals with exit status 0
                print(p.stdout[-3000:])
                raise SystemExit(f"teraconverter failed with {p.returncode}")
            files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
            rec = {"recipe_dtype": np.array(dtype), "recipe_shape": np.array(shape), "recipe_seed": np.array(seed),
                   "input_sha": np.array(hashlib.sha256(vol.tobytes()).hexdigest()), "flags": np.array(flags),
                   "files": np.array(files)}
            rng = np.random.default_rng(seed + 1000)
            budget = SAMPLE_BUDGET
            for f in files:
                full = os.path.join(out, f)
                if f.endswith("mdata.bin"):
                    rec[f"mdata/{f}"] = np.frombuffer(open(full, "rb").read(), dtype=np.uint8)
                    continue
                pages, comp = read_pages(full)
                rec[f"pages/{f}"] = np.array([pages.shape[0], pages.shape[1], pages.shape[2], comp])
                rec[f"sha/{f}"] = np.array(hashlib.sha256(np.ascontiguousarray(pages).tobytes()).hexdigest())
                k = min(SAMPLE_PAGES, pages.shape[0])
                if budget - k * pages[0].nbytes >= 0:
                    idx = np.sort(rng.choice(pages.shape[0], k, replace=False))
                    rec[f"sample_idx/{f}"] = idx
                    rec[f"sample/{f}"] = pages[idx]
                    budget -= k * pages[0].nbytes
            np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **rec)
            print(f"{name}: {len(files)} files, {os.path.getsize(os.path.join(OUT, name + '.npz'))} bytes")
        dtype, shape, seed, flags = REFUSED
        vol = make_series(dtype, shape, seed)
        src, out = os.path.join(tmp, "refused", "src"), os.path.join(tmp, "refused", "out")
        write_series(vol, src)
        os.makedirs(out)
        p = run(flags, src, out)
        msg = [ln for ln in p.stdout.splitlines() if "too much resolutions" in ln]
        assert msg, "the binary accepted a run it is expected to refuse"
        np.savez_compressed(os.path.join(OUT, "refused.npz"), recipe_dtype=np.array(dtype), recipe_shape=np.array(shape),
                            flags=np.array(flags), message=np.array(msg[0] if msg else p.stdout[-500:]))


if __name__ == "__main__":
    sys.exit(main())
