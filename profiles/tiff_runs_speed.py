#!/usr/bin/env python3
"""Throughput of the device TIFF writer (mi_tiff_write_series_device) on a 2048 x 2048 x 64 uint16 volume that lies in device memory,
files written to /dev/shm: noise, a smooth field (the one of tests/test_gpu_tiff_device.py's size test) and a sparse one (a noisy
disc on zero, tests/deflate_util.sparse_disc).  GB/s are the samples' bytes over the wall time of the call (it ends in a stream
synchronise), `reps` repeats after one warm-up call each.

    python profiles/tiff_runs_speed.py [--lib OTHER/libmi_ipp.so] [--reps 5] [--nz 64] [--content noise,smooth,sparse] [--out FILE.json]

--lib times another build of the library (the parent commit's, for a comparison on the same box: alternate the two commands);
--reps 0 writes every content once with no warm-up -- the form to put under `rocprofv3 --kernel-trace --stats`."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def volumes(nz, n, dev, which):
    import torch
    g = torch.Generator(device=dev).manual_seed(12)
    rand = lambda *s: torch.rand(*s, generator=g, device=dev)       # noqa: E731
    randn = lambda *s: torch.randn(*s, generator=g, device=dev)     # noqa: E731
    u16 = lambda t: ((t.to(torch.int32) + 32768) % 65536 - 32768).to(torch.int16).contiguous()   # noqa: E731  (the bits of uint16)
    if "noise" in which:
        yield "noise", u16(rand(nz, n, n) * 65535)
    if "smooth" in which:
        yield "smooth", u16((torch.cumsum(randn(nz, n, n), dim=2) * 6 + 3000 + rand(nz, n, n) * 40).clamp(0, 65535))
    if "sparse" in which:
        y, x = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
        inside = (y - n * 0.47) ** 2 + (x - n * 0.55) ** 2 < (n * 0.3) ** 2
        yield "sparse", u16(torch.where(inside[None], (randn(nz, n, n) * 240 + 1500).clamp(1, 3000), torch.zeros((), device=dev)))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "image-preprocessing-pipeline_amd", "libmi_ipp.so"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nz", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--content", default="noise,smooth,sparse")
    ap.add_argument("--dir", default="/dev/shm/tiff_runs_speed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    lib = C.CDLL(a.lib)
    lib.mi_tiff_write_series_device.restype = C.c_int
    lib.mi_tiff_write_series_device.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(C.c_int)]
    lib.mi_last_error.restype = C.c_char_p
    paths = (C.c_char_p * a.nz)(*[os.fsencode(os.path.join(a.dir, f"img_{k:06d}.tif")) for k in range(a.nz)])
    stream = torch.cuda.current_stream(dev).cuda_stream

    def write(t):
        shutil.rmtree(a.dir, ignore_errors=True)
        os.makedirs(a.dir)
        made = C.c_int(0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rc = lib.mi_tiff_write_series_device(0, stream, paths, a.nz, t.data_ptr(), 2, a.size, a.size, 0, C.byref(made))
        dt = time.perf_counter() - t0
        assert rc == 0 and made.value == a.nz, lib.mi_last_error()
        return dt

    result = {"lib": a.lib, "shape": [a.nz, a.size, a.size], "reps": a.reps, "MI_TIFF_DEVICE_RUNS": os.environ.get("MI_TIFF_DEVICE_RUNS")}
    for name, t in volumes(a.nz, a.size, dev, a.content.split(",")):
        nbytes = t.numel() * 2
        if a.reps > 0:
            write(t)
        times = [write(t) for _ in range(max(1, a.reps))]
        size = sum(os.path.getsize(os.path.join(a.dir, f)) for f in os.listdir(a.dir))
        from ipp_amd import brickio
        import numpy as np
        same = bool(np.array_equal(brickio.load_tiff_series(a.dir, 0, 2).view(np.int16), t[:2].cpu().numpy()))
        result[name] = {"GB_per_s": [nbytes / x / 1e9 for x in times], "s": times, "file_bytes": size, "of_the_samples": size / nbytes,
                        "first_slices_identical": same}
        print(name, json.dumps(result[name]), flush=True)
        assert same
        del t
    shutil.rmtree(a.dir, ignore_errors=True)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
