#!/usr/bin/env python3
"""Device time of the three entries of include/mi_thresholds.h on one u16 slice, and the host time of the numpy restatement
(tests/thresholds_util.py) on the same slice.  `python profiles/thresholds_time.py [--size 16384 --reps 5 --out FILE.json]`

Device times are device events around the entry alone (buffers allocated before, nothing copied), the median of `reps` after one
warm-up call; bytes are what the algorithm must read.  The host figure is the wall time of log1p + threshold_multiotsu(classes=4) +
estimate_bit_shift in numpy, once."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from ipp_amd import capi, thresholds as th
    from tests import thresholds_util as tu
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no_host", action="store_true")
    a = ap.parse_args()
    capi.require_gpu()
    dev = torch.device("cuda", 0)
    lib = capi.lib()
    img = tu.four_mode_image((a.size, a.size), seed=7)
    n = img.size
    d16 = torch.from_numpy(img).to(dev)
    d32 = torch.from_numpy(np.log1p(img, dtype=np.float32)).to(dev)
    rng = torch.empty((1, 2), dtype=torch.float32, device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    edges = torch.empty((1, 257), dtype=torch.float32, device=dev)
    counts = torch.empty((1, 256), dtype=torch.int64, device=dev)
    codes = torch.empty((1, 65536), dtype=torch.int64, device=dev)
    idx = torch.empty((1, 3), dtype=torch.int32, device=dev)
    nv = torch.empty((1,), dtype=torch.int32, device=dev)
    st = torch.empty((1,), dtype=torch.int32, device=dev)
    work = torch.empty((1,), dtype=torch.int64, device=dev)
    stream = capi.current_stream_ptr(dev)
    calls = {
        "mi_hist256_f32": (lambda: lib.mi_hist256_f32(0, stream, d32.data_ptr(), 1, n, rng.data_ptr(), bad.data_ptr(), edges.data_ptr(),
                                                      counts.data_ptr()), 2 * 4 * n),   # two passes over the float32 image
        "mi_code_hist_u16": (lambda: lib.mi_code_hist(0, stream, d16.data_ptr(), capi.CODES_U16, 1, n, codes.data_ptr()), 2 * 2 * n),
        "mi_multiotsu_search": (lambda: lib.mi_multiotsu_search(0, stream, counts.data_ptr(), 1, 4, idx.data_ptr(), nv.data_ptr(),
                                                                st.data_ptr(), work.data_ptr()), 0),
    }
    result = {"size": a.size, "samples": n, "reps": a.reps}
    for name, (call, nbytes) in calls.items():
        capi.check(call())
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.check(call())
            e1.record()
            torch.cuda.synchronize(dev)
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        result[name] = {"ms_median": ms, "ms_all": times, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6 if nbytes else None}
        print(name, result[name], flush=True)
    assert np.array_equal(codes.cpu().numpy()[0], np.bincount(img.reshape(-1), minlength=65536))
    result["device_indices"] = idx.cpu().numpy()[0].tolist()
    t0 = time.perf_counter()
    params = th.estimate_slice_params(d16[None])   # nz = 1: the three indices are slice 0, one batch of three
    torch.cuda.synchronize(dev)
    result["estimate_slice_params_wall_s_three_slices_on_device"] = time.perf_counter() - t0
    result["params"] = params.as_json()
    if not a.no_host:
        t0 = time.perf_counter()
        log_img = np.log1p(img, dtype=np.float32)
        clips = tu.threshold_multiotsu(log_img, classes=4)
        shift, _ = tu.estimate_bit_shift(log_img, clips[2], 99.99)
        result["numpy_restatement_wall_s_one_slice"] = time.perf_counter() - t0
        result["restatement"] = {"clips": [float(c) for c in clips], "bit_shift_to_right": shift}
        assert [params[k] for k in ("bleach_correction_clip_min", "bleach_correction_clip_med", "bleach_correction_clip_max")] == result["restatement"]["clips"]
        assert params["bit_shift_to_right"] == shift
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
