#!/usr/bin/env python3
"""Throughput of the TeraFly conversion (terafly.convert, --resolutions=012345, LZW) by two routes that alternate in one process:

    host     the LZW strips encoded on --threads host threads (mi_tiff3d_write_blocks) -- through --parent-lib when given, the
             library of the commit before the device encoder, so that the comparison is with what was there
    device   encoder="device": the strips encoded on the GPU from the levels (k_strip_lzw_encode), only the streams return

The series: --nz x --ny x --nx uint16 slices in /dev/shm, contents noise, a smooth field and a sparse one (profiles/tiff_runs_speed.py's);
the tree goes to /dev/shm too and is removed after every run.  Blocks: --block 0 (the default blocks: one per level) or N (N x N x 64).
Mvoxel/s are the voxels of level 0 over the wall time of convert(); after one warm-up per route, `reps` repeats alternate; min / median /
max are printed, since the box is shared.  After the last repeat the two trees are compared file by file.

    python profiles/terafly_write_speed.py [--reps 5] [--nz 64] [--ny 2048] [--nx 2048] [--block 0] [--content noise,smooth,sparse]
                                           [--threads 16] [--parent-lib PATH] [--out FILE.json]

--reps 0 converts every series once through the device route only, with no warm-up -- the form to put under
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the raw rows in and the stream bytes out are printed."""
import argparse
import ctypes as C
import glob
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
    import torch
    from ipp_amd import brickio, capi, terafly
    from tiff_runs_speed import volumes
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nz", type=int, default=64)
    ap.add_argument("--ny", type=int, default=2048)
    ap.add_argument("--nx", type=int, default=2048)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--content", default="noise,smooth,sparse")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--dir", default="/dev/shm/terafly_write_speed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    own = capi.lib()
    parent = None
    if a.parent_lib:
        parent = C.CDLL(a.parent_lib)
        for name, (res, args) in capi.SIGNATURES.items():
            if hasattr(parent, name):
                f = getattr(parent, name)
                f.restype, f.argtypes = res, args
        assert not hasattr(parent, "mi_tiff3d_write_blocks_device"), "--parent-lib already has the device route"
    block = (a.block, a.block, 64) if a.block > 0 else (-1, -1, -1)

    def run(route, src, dst):
        shutil.rmtree(dst, ignore_errors=True)
        os.makedirs(dst)
        capi._lib = parent if (route == "host" and parent is not None) else own
        try:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            terafly.convert(src, dst, resolutions="012345", block=block, threads=a.threads, encoder=route)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0
        finally:
            capi._lib = own

    def digest(dst):
        import hashlib
        out = {}
        for f in sorted(glob.glob(os.path.join(dst, "**", "*"), recursive=True)):
            if os.path.isfile(f):
                out[os.path.relpath(f, dst)] = hashlib.sha256(open(f, "rb").read()).hexdigest()
        return out

    def stats(times, voxels):
        g = sorted(voxels / x / 1e6 for x in times)
        return {"Mvoxel_per_s_min": g[0], "Mvoxel_per_s_median": statistics.median(g), "Mvoxel_per_s_max": g[-1], "s": times}

    result = {"shape": [a.nz, a.ny, a.nx], "block": a.block, "reps": a.reps, "threads": a.threads, "parent_lib": bool(parent)}
    shutil.rmtree(a.dir, ignore_errors=True)
    voxels = a.nz * a.ny * a.nx
    for name, t in volumes(a.nz, max(a.ny, a.nx), dev, a.content.split(",")):
        vol = t.view(torch.uint16)[:, :a.ny, :a.nx].contiguous()
        del t
        src, dst = os.path.join(a.dir, f"{name}_series"), os.path.join(a.dir, f"{name}_tree")
        brickio.save_tiff_series(src, vol.cpu().numpy(), first_index=0)
        del vol
        torch.cuda.empty_cache()
        entry = {}
        times = {"host": [], "device": []}
        if a.reps > 0:
            run("host", src, dst)
            run("device", src, dst)
        digests = {}
        for rep in range(max(1, a.reps)):
            for route in times:
                if a.reps == 0 and route != "device":
                    continue
                times[route].append(run(route, src, dst))
                if rep == max(1, a.reps) - 1:
                    digests[route] = digest(dst)
                    files = glob.glob(os.path.join(dst, "RES*", "*", "*", "*.tif"))
                    entry["files"] = len(files)
                    entry["file_bytes"] = sum(os.path.getsize(f) for f in files)
        if len(digests) == 2:
            assert digests["host"] == digests["device"], name
            entry["trees_identical"] = True
        # every level's raw rows: 1 + 1/8 + 1/64 + ... of level 0 (3-D halving)
        entry["raw_row_bytes"] = int(sum(2 * (a.nz >> k) * (a.ny >> k) * (a.nx >> k) for k in range(6)))
        for k, v in times.items():
            if v:
                entry[k] = stats(v, voxels)
        if times["host"]:
            entry["device_over_host_median"] = entry["device"]["Mvoxel_per_s_median"] / entry["host"]["Mvoxel_per_s_median"]
            entry["device_slowest_beats_host_fastest"] = entry["device"]["Mvoxel_per_s_min"] > entry["host"]["Mvoxel_per_s_max"]
        result[name] = entry
        print(name, json.dumps(entry), flush=True)
        shutil.rmtree(dst, ignore_errors=True)
        shutil.rmtree(src, ignore_errors=True)
    shutil.rmtree(a.dir, ignore_errors=True)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
