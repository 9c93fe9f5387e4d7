#!/usr/bin/env python3
"""Golden fixtures of the TeraFly tree READER from the reference's OWN ``teraconverter`` binary (build container only).

The fixtures of tests/golden/terafly are noise, which LZW cannot compress and which uses almost no dictionary string.  These three
series compress, so the block files the binary writes through libtiff hold long strings, KwKwK codes and table growth -- the only
libtiff-encoded LZW streams of the suite.  Every run writes a seeded 2-D TIFF series and converts it with

    teraconverter --sfmt="TIFF (series, 2D)" --dfmt="TIFF (tiled, 3D)" --clist=0 --noprogressbar --resolutions=01 -s=SRC -d=OUT

Stored under tests/golden/terafly_read/:

    <run>/RES(...)/...    the tree exactly as the binary wrote it: block .tif files and mdata.bin (data written by the program)
    <run>.npz             recipe (name, dtype, shape, seed), SHA-256 of the input series, the flags, the list of files

The test regenerates the input with ``series(name, shape, seed)`` below (restated in tests/test_terafly_read_host.py) and checks the
hash before it trusts it.
"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TC = "/root/reference/TeraStitcher/Linux/AVX2/teraconverter"
OUT = os.path.join(ROOT, "tests", "golden", "terafly_read")
BASE = ["--sfmt=TIFF (series, 2D)", "--dfmt=TIFF (tiled, 3D)", "--clist=0", "--noprogressbar"]
FLAGS = ["--resolutions=01"]

# name -> (kind, dtype, (D, V, H), seed)
RUNS = {
    "ramp_u16": ("ramp", "uint16", (12, 260, 270), 31),   # 12 slices: the block file of 20 passes the size of a fixture
    "sparse_u16": ("sparse", "uint16", (20, 260, 270), 32),
    "planes_u8": ("planes", "uint8", (20, 260, 270), 33),
}


def series(kind, dtype, shape, seed):
    rng = np.random.default_rng(seed)
    D, V, H = shape
    if kind == "ramp":      # a smooth ramp with noise of one bit in one voxel of 25 (more noise passes the size of a fixture)
        z, y, x = np.meshgrid(np.arange(D), np.arange(V), np.arange(H), indexing="ij")
        return (1000 + 16 * z + 4 * (y // 8) + 4 * (x // 16) + (rng.random(shape) < 0.04)).astype(dtype)
    if kind == "sparse":    # 95 % zeros and a few blobs
        vol = np.zeros(shape, dtype)
        for _ in range(6):
            c = [int(rng.integers(3, n - 3)) for n in shape]
            r = int(rng.integers(3, 9))
            z, y, x = np.ogrid[:D, :V, :H]
            m = (z - c[0]) ** 2 * 4 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r * 4
            vol[m] = rng.integers(200, 60000, int(m.sum())).astype(dtype)
        return vol
    if kind == "planes":    # constant planes
        return np.broadcast_to(rng.integers(0, 256, (D, 1, 1)).astype(dtype), shape).copy()
    raise ValueError(kind)


def main():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    with tempfile.TemporaryDirectory() as tmp:
        for name, (kind, dtype, shape, seed) in RUNS.items():
            vol = series(kind, dtype, shape, seed)
            src, out = os.path.join(tmp, name, "src"), os.path.join(OUT, name)
            os.makedirs(src)
            for k in range(vol.shape[0]):
                Image.fromarray(vol[k]).save(os.path.join(src, f"slice_{k:04d}.tif"))
            os.makedirs(out)
            cmd = [TC] + BASE + FLAGS + [f"-s={src}", f"-d={out}"]
            print(" ".join(cmd), flush=True)
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0 or "ERROR" in p.stdout:
                print(p.stdout[-3000:])
                raise SystemExit(f"teraconverter failed with {p.returncode}")
            files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
            np.savez_compressed(os.path.join(OUT, f"{name}.npz"), recipe_kind=np.array(kind), recipe_dtype=np.array(dtype),
                                recipe_shape=np.array(shape), recipe_seed=np.array(seed),
                                input_sha=np.array(hashlib.sha256(vol.tobytes()).hexdigest()), flags=np.array(FLAGS), files=np.array(files))
            total = sum(os.path.getsize(os.path.join(out, f)) for f in files)
            print(f"{name}: {len(files)} files, {total} bytes")


if __name__ == "__main__":
    sys.exit(main())
