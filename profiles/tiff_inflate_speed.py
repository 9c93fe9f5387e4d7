#!/usr/bin/env python3
"""Throughput of the device TIFF reader (mi_tiff_read_box_device) against the host route it mirrors (mi_tiff_read_box on 16 threads,
then ``.to(device)``) on a 2048 x 2048 x 64 uint16 volume whose files lie in /dev/shm.  Contents: noise, a smooth field and a
sparse one (profiles/tiff_runs_speed.py's); each from two file makers: mi_tiff_write_series (the host's deflate at level 1, full
LZ77) and mi_tiff_write_series_device (one dynamic block per strip: literals, or runs as matches at distance 1).  GB/s are the
samples' bytes over the wall time from the call to the box lying in device memory (both routes end in a synchronise).  The two
routes alternate, `reps` times after one warm-up each; ranges and medians are printed, since the box is shared.

    python profiles/tiff_inflate_speed.py [--parent-lib OTHER/libmi_ipp.so] [--reps 5] [--nz 64] [--content noise,smooth,sparse]
                                          [--threads 16] [--out FILE.json]

--parent-lib: the host route calls mi_tiff_read_box of another build of the library (the parent commit's), so that the parent's
code and this commit's alternate on the same box in one process;

--reps 0 reads every folder once through the device route only, with no warm-up -- the form to put under
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import numpy as np
    import torch
    from ipp_amd import brickio
    from tiff_runs_speed import volumes
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nz", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--content", default="noise,smooth,sparse")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--dir", default="/dev/shm/tiff_inflate_speed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    shape = (a.size, a.size)

    parent = None
    if a.parent_lib:
        import ctypes as C
        parent = C.CDLL(a.parent_lib)
        parent.mi_tiff_read_box.restype = C.c_int
        parent.mi_tiff_read_box.argtypes = [C.POINTER(C.c_char_p)] + [C.c_int] * 8 + [C.c_void_p, C.c_int]

    def read_host(files):
        if parent is None:
            return brickio.read_tiff_box(files, shape, np.uint16, 0, a.size, 0, a.size, threads=a.threads)
        out = np.empty((len(files), a.size, a.size), np.uint16)      # (what brickio.read_tiff_box does, on the other library)
        paths = (C.c_char_p * len(files))(*[os.fsencode(str(f)) for f in files])
        rc = parent.mi_tiff_read_box(paths, len(files), a.size, a.size, 2, 0, a.size, 0, a.size, out.ctypes.data, a.threads)
        assert rc == 0, rc
        return out

    def host_route(files):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        t = torch.from_numpy(read_host(files)).to(dev)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, t

    def device_route(files):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        t = brickio.read_tiff_box_device(files, shape, np.uint16, 0, a.size, 0, a.size, device=dev, threads=a.threads)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, t

    def stats(times, nbytes):
        g = sorted(nbytes / x / 1e9 for x in times)
        return {"GB_per_s_min": g[0], "GB_per_s_median": statistics.median(g), "GB_per_s_max": g[-1], "s": times}

    result = {"shape": [a.nz, a.size, a.size], "reps": a.reps, "threads": a.threads, "parent_lib": a.parent_lib}
    shutil.rmtree(a.dir, ignore_errors=True)
    for name, t in volumes(a.nz, a.size, dev, a.content.split(",")):
        nbytes = t.numel() * 2
        vol = t.view(torch.uint16)
        for maker in ("host_level1", "device"):
            folder = os.path.join(a.dir, f"{name}_{maker}")
            if maker == "device":
                brickio.save_tiff_series_device(folder, vol)
            else:
                brickio.save_tiff_series(folder, vol.cpu().numpy())
            files = brickio.list_tiff_series(folder)
            size = sum(os.path.getsize(f) for f in files)
            entry = {"file_bytes": size, "of_the_samples": size / nbytes}
            if a.reps > 0:
                host_route(files)
                device_route(files)
            th, td = [], []
            for _ in range(max(1, a.reps)):
                if a.reps > 0:
                    dt, _t = host_route(files)
                    th.append(dt)
                    assert bool(torch.equal(_t.view(torch.int16), vol.view(torch.int16))), (name, maker, "host route")
                    del _t
                dt, got = device_route(files)
                td.append(dt)
                same = bool(torch.equal(got.view(torch.int16), vol.view(torch.int16)))
                del got
                assert same, (name, maker)
            if th:
                entry["host_then_upload"] = stats(th, nbytes)
            entry["device"] = stats(td, nbytes)
            if th:
                entry["device_over_host_median"] = entry["device"]["GB_per_s_median"] / entry["host_then_upload"]["GB_per_s_median"]
            result[f"{name}/{maker}"] = entry
            print(name, maker, json.dumps(entry), flush=True)
            shutil.rmtree(folder, ignore_errors=True)
        del t, vol
    shutil.rmtree(a.dir, ignore_errors=True)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
