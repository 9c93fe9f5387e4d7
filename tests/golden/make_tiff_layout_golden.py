#!/usr/bin/env python3
"""SHA-256 sums of the slice files the TIFF series writers make (tests/golden/tiff_layout_sums.json), recorded from the build of the
commit BEFORE a change to the writers, so that tests/test_tiff_layout_host.py and tests/test_gpu_tiff_device.py can tell that every
byte of a file -- strips, even-byte padding, strip tables, the arrays in front of the directory, the directory, the header -- is what
it was.  Only the sums are stored, never the files.

    python tests/golden/make_tiff_layout_golden.py            # key "host":   mi_tiff_write_series / mi_tiff_write_rgb_series, uncompressed
    python tests/golden/make_tiff_layout_golden.py --device   # key "device": mi_tiff_write_series_device (needs the GPU)

The host cases are uncompressed, so the sums depend on no deflate library.  The device's Huffman code is the project's own and
deterministic, so the sums of its deflated files are meaningful.  A key that is already recorded is not overwritten unless --force
is given.  The samples come from integer arithmetic alone (no random generator whose stream could change between numpy versions).
"""
import argparse
import hashlib
import json
import os
import struct
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff_layout_sums.json")

# name: (gray / rgb, dtype, (nz, ny, nx), strips per slice)
HOST_CASES = {
    "gray_u8_2x5x7": ("gray", "uint8", (2, 5, 7), 1),
    "gray_u16_2x5x7": ("gray", "uint16", (2, 5, 7), 1),
    "gray_f32_2x5x7": ("gray", "float32", (2, 5, 7), 1),
    "gray_u16_1x600x1000": ("gray", "uint16", (1, 600, 1000), 2),   # rows of 2000 bytes: 524 rows per strip; out-of-line strip tables
    "gray_u8_1x3x5": ("gray", "uint8", (1, 3, 5), 1),               # 15 bytes of samples: the padding byte
    "rgb_u8_1x5x7": ("rgb", "uint8", (1, 5, 7), 1),
    "rgb_f32_1x300x400": ("rgb", "float32", (1, 300, 400), 2),      # rows of 4800 bytes: 218 rows per strip
}
# name: (dtype, (nz, ny, nx), strips per slice, smooth first slice)
DEVICE_CASES = {
    "u8_2x64x96": ("uint8", (2, 64, 96), 1, False),
    "u16_2x64x96": ("uint16", (2, 64, 96), 1, False),
    "u16_2x600x1000": ("uint16", (2, 600, 1000), 2, True),   # slice 0 smooth: predictor 2 and tag 317; slice 1 noise: no tag 317
}


def noise(n):
    """n words of 64 well-mixed bits (the splitmix64 finaliser of 0 .. n - 1)"""
    x = np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def volume(dtype, shape, smooth_first=False):
    n = int(np.prod(shape))
    if dtype == "float32":
        v = ((noise(n) >> np.uint64(40)).astype(np.float32) / np.float32(1 << 24)).reshape(shape)
    elif dtype == "uint16":   # noise on a narrow range, as a camera's: differencing it widens the range, so the device keeps predictor 1
        v = ((noise(n) >> np.uint64(17)) % np.uint64(3000) + np.uint64(200)).astype(dtype).reshape(shape)
    else:
        v = (noise(n) >> np.uint64(17)).astype(dtype).reshape(shape)
    if smooth_first:
        y, x = np.mgrid[0:shape[-2], 0:shape[-1]]
        v[0] = (3 * y + 5 * x).astype(dtype)
    return np.ascontiguousarray(v)


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def directory(path):
    """{tag: (type, count, value)} of the first directory of a classic little-endian TIFF"""
    with open(path, "rb") as f:
        b = f.read()
    assert b[:4] == b"II*\0"
    at, = struct.unpack_from("<I", b, 4)
    n, = struct.unpack_from("<H", b, at)
    return {t: (ty, c, v) for t, ty, c, v in (struct.unpack_from("<HHII", b, at + 2 + 12 * k) for k in range(n))}


def write_host(name, folder, compression=None):
    """the files of a host case, in slice order"""
    from ipp_amd import align_images, brickio
    kind, dtype, shape, _ = HOST_CASES[name]
    os.makedirs(folder, exist_ok=True)
    paths = [os.path.join(str(folder), f"img_{k + 1:06d}.tif") for k in range(shape[0])]
    if kind == "gray":
        assert brickio._native() is not None, "the native library is not built"
        assert brickio.save_tiff_series(folder, volume(dtype, shape), compression=compression) == shape[0]
    else:
        assert align_images.write_rgb_series(paths, volume(dtype, shape + (3,)), compression=compression) == shape[0]
    return paths


def write_device(name, folder):
    import torch
    from ipp_amd import brickio
    dtype, shape, _, smooth = DEVICE_CASES[name]
    vol = torch.from_numpy(volume(dtype, shape, smooth)).to(torch.device("cuda", 0))
    assert brickio.save_tiff_series_device(folder, vol) == shape[0]
    return [os.path.join(str(folder), f"img_{k + 1:06d}.tif") for k in range(shape[0])]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", action="store_true", help="record the key \"device\" (on the GPU) instead of \"host\"")
    ap.add_argument("--force", action="store_true", help="overwrite a key that is already recorded")
    a = ap.parse_args()
    golden = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            golden = json.load(f)
    key = "device" if a.device else "host"
    if key in golden and not a.force:
        sys.exit(f"{GOLDEN}: the key \"{key}\" is already recorded; --force overwrites it")
    with tempfile.TemporaryDirectory() as tmp:
        if a.device:
            golden[key] = {n: [sha(p) for p in write_device(n, os.path.join(tmp, n))] for n in DEVICE_CASES}
        else:
            golden[key] = {n: [sha(p) for p in write_host(n, os.path.join(tmp, n))] for n in HOST_CASES}
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: recorded \"{key}\" ({len(golden[key])} cases)")


if __name__ == "__main__":
    main()
