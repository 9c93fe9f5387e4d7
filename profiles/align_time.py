#!/usr/bin/env python3
"""Device and wall time of the entries of include/mi_align.h.  `python profiles/align_time.py [--reps 5 --out FILE.json]`

* one ECC iteration's sums (mi_ecc_sums: the sum kernel and the single-work-group total) at 256^2, 1024^2 and 4096^2: device events
  around the entry alone, the median of `reps` after one warm-up call; bytes are the four float32 planes read once;
* the loop (mi_ecc_translation_run) with eps = 0 for a fixed 512 iterations at batch sizes 1 .. 512: wall time per iteration, which
  is what the batch size is chosen by (the state is read once per batch);
* a full get_transformation_matrix (prepare, loop to eps = 1e-10, inverse) on a 1024^2 pair: wall time and iterations;
* mi_channel_composite of one group of 8 slices of 2048^2, u16 in and out: device events; bytes are three reads and one write."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pair(n, shift=(2.3, -1.7)):
    """a smooth plane and the same scene shifted, from outer products (cheap at 4096^2)"""
    x = np.arange(n, dtype=np.float64)

    def scene(dx, dy):
        a = np.outer(np.cos((x + dy) / 53.0), np.sin((x + dx) / 37.0)) + np.outer(np.sin((x + dy) / 11.0), np.cos((x + dx) / 17.0))
        return (100.0 * a + 300.0).astype(np.float32)
    return scene(0.0, 0.0), scene(*shift)


def device_ms(call, reps, torch, dev):
    call()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize(dev)
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), times


def main():
    import torch
    from ipp_amd import align_images as ai, capi
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    capi.require_gpu()
    dev = torch.device("cuda", 0)
    lib = capi.lib()
    stream = capi.current_stream_ptr(dev)
    result = {"reps": a.reps}

    for n in (256, 1024, 4096):
        tmpl, subj = pair(n)
        planes = ai.ecc_prepare(torch.from_numpy(tmpl).to(dev), torch.from_numpy(subj).to(dev))
        ptrs = [p.data_ptr() for p in planes]
        sums = torch.empty(capi.ECC_NSUMS, dtype=torch.float64, device=dev)
        scratch = torch.empty(capi.ECC_SCRATCH_BYTES // 8, dtype=torch.float64, device=dev)
        state = torch.empty(6, dtype=torch.float64, device=dev)
        ms, every = device_ms(lambda: capi.check(lib.mi_ecc_sums(0, stream, *ptrs, n, n, 0.4, -0.3, scratch.data_ptr(), sums.data_ptr())), a.reps,
                              torch, dev)
        nbytes = 4 * 4 * n * n
        result[f"ecc_sums_{n}"] = {"ms_median": ms, "ms_all": every, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6}
        print(f"ecc_sums_{n}", result[f"ecc_sums_{n}"], flush=True)
        out = capi.EccState()
        per_iteration = {}
        for batch in (1, 4, 16, 32, 64, 128, 512):
            def run():
                capi.check(lib.mi_ecc_translation_run(0, stream, *ptrs, n, n, 0.0, 0.0, 512, 0.0, batch, state.data_ptr(), scratch.data_ptr(),
                                                      C.byref(out)))
            run()
            walls = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                run()
                walls.append(time.perf_counter() - t0)
            if out.iteration != 512 or out.status != capi.ECC_OK:   # the loop ended early: the figure would be of empty launches
                per_iteration[batch] = {"iterations": out.iteration, "status": out.status}
                continue
            per_iteration[batch] = float(np.median(walls)) / 512 * 1e6
        result[f"ecc_loop_{n}_us_per_iteration_by_batch"] = per_iteration
        print(f"ecc_loop_{n}_us_per_iteration_by_batch", per_iteration, flush=True)

    tmpl, subj = pair(1024)
    d0, d1 = torch.from_numpy(tmpl).to(dev), torch.from_numpy(subj).to(dev)
    ai.get_transformation_matrix(d0, d1, verbose=False)
    t0 = time.perf_counter()
    m = ai.get_transformation_matrix(d0, d1, verbose=False)
    result["get_transformation_matrix_1024"] = {"wall_s": time.perf_counter() - t0, "iterations": ai.ecc_translation(d0, d1)[3],
                                                "translation": [float(m[0, 2]), float(m[1, 2])]}
    print("get_transformation_matrix_1024", result["get_transformation_matrix_1024"], flush=True)

    n, size = 8, 2048
    rng = np.random.default_rng(3)
    sources = [torch.from_numpy(rng.integers(0, 65535, (n, size, size)).astype(np.uint16)).to(dev) for _ in range(3)]
    maps = [(0, 0, 0), (0, 4, -6), (0, -4, 2)]
    ms, every = device_ms(lambda: ai.channel_composite(sources, [0, 0, 0], maps, 0, n, (size, size), "uint16"), a.reps, torch, dev)
    nbytes = 2 * 2 * 3 * n * size * size
    result["channel_composite_8x2048"] = {"ms_median": ms, "ms_all": every, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6}
    print("channel_composite_8x2048", result["channel_composite_8x2048"], flush=True)

    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
