"""Throughput of the isotropic down-sampling (include/mi_isodown.h) on one device.

    python profiles/isodown_bench.py [--size 16384] [--slices 4] [--reps 7] [--folder-size 4096] [--folder-slices 28] [--out FILE.json]

  halve    the halving kernel alone on a stack of --slices slices of --size x --size samples (uint16 and float32) with the plan of
           10 um from 0.7 um (three rounds on both axes): source bytes / time, next to a plain device read of the same buffer (an
           int32 max reduction over the same bytes).  The stack is larger than the 256-MB last-level cache.
  group    mi_isodown_run of the same stack (halving, resize, z reduction).
  folder   parallel_image_processor folder -> folder (fun=None) on --folder-slices uint16 slices of --folder-size, wall time, and the
           device time of the same groups' runs alone (the share of the wall time spent in kernels).

Device events around every timed window, one warm-up, the median of --reps repeats.  A run without a GPU fails.
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, reps):
    """median milliseconds of fn() between two device events, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--folder-size", type=int, default=4096)
    ap.add_argument("--folder-slices", type=int, default=28)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ipp_amd import capi, parallel_image_processor as pip, pystripe
    capi.require_gpu()
    dev = torch.device("cuda", 0)
    voxel, target = (0.7, 0.7, 0.7), 10.0
    rounds = pip.z_rounds(target, voxel[0])
    result = dict(size=a.size, slices=a.slices, reps=a.reps, device=torch.cuda.get_device_name(0))
    for name, tdt in (("uint16", torch.int16), ("float32", torch.float32)):
        if tdt == torch.float32:
            stack = torch.rand((a.slices, a.size, a.size), device=dev) * 4000
        else:
            stack = torch.randint(0, 30000, (a.slices, a.size, a.size), device=dev, dtype=torch.int16).view(torch.uint16)
        plan = pip.Plan(dev, (a.size, a.size), name, voxel[1:], target, True, z_rounds=rounds, max_group=a.slices)
        src_bytes = stack.numel() * stack.element_size()
        words = stack.view(torch.int32)
        t_read = timed(torch, lambda: words.max(), a.reps)
        t_halve = timed(torch, lambda: plan.halve(stack), a.reps)
        t_group = timed(torch, lambda: plan.run(stack), a.reps)
        row = dict(source_bytes=src_bytes, steps=plan.info["steps"], halved_shape=plan.halved_shape, target_shape=plan.target_shape,
                   tile=plan.info["tile"], plain_read_ms=t_read, halve_ms=t_halve, group_run_ms=t_group,
                   plain_read_TBps=src_bytes / t_read[0] / 1e9, halve_TBps=src_bytes / t_halve[0] / 1e9,
                   group_run_TBps=src_bytes / t_group[0] / 1e9)
        result[name] = row
        print(f"[isodown_bench] {name} {a.slices} x {a.size}^2 ({src_bytes / 2 ** 30:.2f} GiB): plain read {t_read[0]:.3f} ms "
              f"({row['plain_read_TBps']:.2f} TB/s), halving {t_halve[0]:.3f} ms ({row['halve_TBps']:.2f} TB/s, "
              f"{t_halve[1]:.3f} .. {t_halve[2]:.3f}), whole group {t_group[0]:.3f} ms ({row['group_run_TBps']:.2f} TB/s)", flush=True)
        plan.close()
        del stack, words
        torch.cuda.empty_cache()

    # folder -> folder
    rng = np.random.default_rng(0)
    n, size = a.folder_slices, a.folder_size
    with tempfile.TemporaryDirectory() as tmp:
        src, dest = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        os.makedirs(src)
        slices = [rng.integers(0, 30000, (size, size), dtype=np.uint16) for _ in range(n)]
        for i, s in enumerate(slices):
            pystripe.imsave_tif(os.path.join(src, f"s_{i:04}.tif"), s)
        t0 = time.perf_counter()
        pip.parallel_image_processor(src, dest, source_voxel=voxel, target_voxel=target)
        wall = time.perf_counter() - t0
    steps = pip.z_steps(target, voxel[0])
    plan = pip.Plan(dev, (size, size), "uint16", voxel[1:], target, True, z_rounds=rounds, max_group=steps)
    device_ms = 0.0
    for g in pip.z_groups(n, steps):
        stack = torch.from_numpy(np.stack([slices[i] for i in g])).to(dev)
        device_ms += timed(torch, lambda: plan.run(stack), 3)[0]
    plan.close()
    result["folder"] = dict(slices=n, size=size, wall_s=wall, device_ms=device_ms, kernel_share=device_ms / 1e3 / wall)
    print(f"[isodown_bench] folder of {n} uint16 slices of {size}^2 -> planes + npz: {wall:.2f} s wall, {device_ms:.2f} ms in kernels "
          f"({100 * device_ms / 1e3 / wall:.1f} % of the wall time; the rest is TIFF reading, upload and the writer)", flush=True)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
