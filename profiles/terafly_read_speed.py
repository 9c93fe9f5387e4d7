#!/usr/bin/env python3
"""Throughput of reading level 0 of a TeraFly tree into device memory, by three routes that alternate in one process:

    pillow   what the commit before the tree reader could do: Pillow page by page over every block file, then ``.to(device)``
    host     TeraFlyTree.imread (mi_tiff3d_read_box on --threads host threads), then ``.to(device)``
    device   TeraFlyTree.imread_device(route="device") (mi_tiff3d_read_box_device: k_strip_lzw, k_tree_place)

The tree: 64 x 2048 x 2048 uint16, written by terafly.convert (LZW, RowsPerStrip 1) into /dev/shm in blocks of --block x --block x 64
(256: strips of 512 bytes, 2^20 of them; 0: one block, strips of 4096 bytes).  Contents: noise, a smooth field and a sparse one
(profiles/tiff_runs_speed.py's).  GB/s are the samples' bytes over the wall time from the call to the box lying in device memory
(every route ends in a synchronise).  `reps` repeats after one warm-up each (Pillow: at most two, no warm-up -- it takes seconds);
ranges and medians are printed, since the box is shared.

    python profiles/terafly_read_speed.py [--reps 5] [--nz 64] [--size 2048] [--block 256] [--content noise,smooth,sparse]
                                          [--threads 16] [--out FILE.json]

--reps 0 reads every tree once through the device route only, with no warm-up -- the form to put under
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters)."""
import argparse
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
    import numpy as np
    import torch
    from PIL import Image, ImageSequence
    from ipp_amd import brickio, terafly
    from tiff_runs_speed import volumes
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nz", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--content", default="noise,smooth,sparse")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/terafly_read_speed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)

    def pillow_route(tree):
        lv = tree.levels[0]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = np.empty(lv.shape, tree.dtype)
        for b in lv.mdata["blocks"]:
            for k, f in enumerate(b["files"]):
                im = Image.open(lv.path / b["dir"] / f)
                for p, page in enumerate(ImageSequence.Iterator(im)):
                    out[lv.z_start[k] + p, b["abs_v"]:b["abs_v"] + b["height"], b["abs_h"]:b["abs_h"] + b["width"]] = np.asarray(page)
        t = torch.from_numpy(out).to(dev)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, t

    def host_route(tree):
        D, V, H = tree.levels[0].shape
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        t = torch.from_numpy(tree.imread((0, D, 0, V, 0, H), threads=a.threads)).to(dev)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, t

    def device_route(tree):
        D, V, H = tree.levels[0].shape
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        t = tree.imread_device((0, D, 0, V, 0, H), device=dev, route="device", threads=a.threads)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, t

    def stats(times, nbytes):
        g = sorted(nbytes / x / 1e9 for x in times)
        return {"GB_per_s_min": g[0], "GB_per_s_median": statistics.median(g), "GB_per_s_max": g[-1], "s": times}

    result = {"shape": [a.nz, a.size, a.size], "block": a.block, "reps": a.reps, "threads": a.threads}
    shutil.rmtree(a.dir, ignore_errors=True)
    for name, t in volumes(a.nz, a.size, dev, a.content.split(",")):
        nbytes = t.numel() * 2
        vol = t.view(torch.uint16)
        src, dst = os.path.join(a.dir, f"{name}_series"), os.path.join(a.dir, f"{name}_tree")
        brickio.save_tiff_series(src, vol.cpu().numpy(), first_index=0)
        os.makedirs(dst)
        block = (a.block, a.block, a.nz) if a.block > 0 else (-1, -1, -1)
        terafly.convert(src, dst, resolutions="0", block=block, threads=a.threads)
        shutil.rmtree(src, ignore_errors=True)
        files = glob.glob(os.path.join(dst, "RES*", "*", "*", "*.tif"))
        size = sum(os.path.getsize(f) for f in files)
        tree = terafly.open_tree(dst)
        entry = {"files": len(files), "file_bytes": size, "of_the_samples": size / nbytes}
        routes = {"pillow": pillow_route, "host": host_route, "device": device_route}
        times = {k: [] for k in routes}
        if a.reps > 0:
            host_route(tree)
            device_route(tree)
        for rep in range(max(1, a.reps)):
            for k, fn in routes.items():
                if a.reps == 0 and k != "device":
                    continue
                if k == "pillow" and rep >= 2:
                    continue
                dt, got = fn(tree)
                times[k].append(dt)
                same = bool(torch.equal(got.view(torch.int16), vol.view(torch.int16)))
                del got
                assert same, (name, k)
        for k, v in times.items():
            if v:
                entry[k] = stats(v, nbytes)
        if times["host"]:
            entry["device_over_host_median"] = entry["device"]["GB_per_s_median"] / entry["host"]["GB_per_s_median"]
        result[name] = entry
        print(name, json.dumps(entry), flush=True)
        shutil.rmtree(dst, ignore_errors=True)
        del t, vol
    shutil.rmtree(a.dir, ignore_errors=True)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
