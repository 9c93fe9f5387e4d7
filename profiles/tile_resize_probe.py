"""The tile resize of pystripe's batch_filter (include/mi_tile_resize.h) on the GPU.

    python profiles/tile_resize_probe.py kernel          mi_tile_resize_run alone (events around the call, warm, median of 5) for the two
                                                         shapes of an isotropic run: 16 uint16 tiles 2048^2 -> 2560^2 (z finer than xy)
                                                         and 1024^2 -> 853^2 (z coarser, after down_sample (2, 2)); ms, the bytes that
                                                         must cross (input read once + output written once) per second, and a device
                                                         copy of the same bytes
    python profiles/tile_resize_probe.py trace           one warm-up and one run of both shapes -- for
                                                         rocprofv3 --kernel-trace --stats -- python3 profiles/tile_resize_probe.py trace
    python profiles/tile_resize_probe.py e2e DIR [tiles] `tiles` (default 32) deflate TIFF tiles of 2048 x 2048 uint16 under DIR/in, then
                                                         batch_filter with process_images.py's keywords at sigma (250, 250), without and
                                                         with new_size for both cases: seconds per tile (read / compute / write)
"""
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from profiles.pystripe_probe import PIPE, tiles_u16, timed  # noqa: E402

CASES = (((2048, 2048), (2560, 2560)), ((1024, 1024), (853, 853)))


def kernel(count=16, trace=False):
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    full = tiles_u16(count, dev)
    for T, N in CASES:
        x = full[:, :T[0], :T[1]].contiguous()
        plan = ps.ResizePlan(dev, T, N, np.uint16, max_batch=count)
        out = torch.empty((count,) + N, dtype=torch.uint16, device=dev)
        plan.run(x, out=out)
        if trace:
            plan.run(x, out=out)
            torch.cuda.synchronize()
            plan.close()
            continue
        ms = timed(lambda: plan.run(x, out=out))
        must = count * 2 * (T[0] * T[1] + N[0] * N[1])
        src = torch.empty(must // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        mc = timed(lambda: dst.copy_(src))
        print(f"{count} uint16 tiles {T} -> {N}: {ms:.4f} ms ({ms / count:.4f} per tile), {must / 1e6:.1f} MB must cross = "
              f"{must / ms / 1e9:.3f} TB/s; a device copy of the same bytes: {mc:.4f} ms = {must / mc / 1e9:.3f} TB/s")
        plan.close()


def e2e(folder, n):
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    src = os.path.join(folder, "in")
    shutil.rmtree(folder, ignore_errors=True)
    base = tiles_u16(16, dev).cpu().numpy()
    for i in range(n):
        ps.imsave_tif(os.path.join(src, f"{i // 64:06d}", f"tile_{i:06d}.tif"), np.roll(base[i % 16], i, axis=1))
    kw = dict(sigma=(250, 250), level=0, crossover=10, threshold=None, lightsheet=False, tile_size=(2048, 2048), d_type="uint16", convert_to_8bit=False,
              bit_shift_to_right=8, bleach_correction_frequency=None, bleach_correction_max_method=False, device=dev, **PIPE)
    for down, new in ((None, None), (None, (2560, 2560)), ((2, 2), None), ((2, 2), (853, 853))):
        dst, stats = os.path.join(folder, "out"), {}
        shutil.rmtree(dst, ignore_errors=True)
        t0 = time.perf_counter()
        ps.batch_filter(src, dst, down_sample=down, new_size=new, stats=stats, **kw)
        dt = time.perf_counter() - t0
        print(f"batch_filter down_sample={down} new_size={new}: {n} tiles in {dt:.2f} s = {dt / n:.4f} s per tile; read {stats['read_s'] / n:.4f}, "
              f"compute (upload + kernels + download) {stats['compute_s'] / n:.4f}, write {stats['write_s'] / n:.4f} s per tile (the three overlap)")
    shutil.rmtree(folder, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        kernel()
    elif mode == "trace":
        kernel(trace=True)
    elif mode == "e2e":
        e2e(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 32)
    else:
        raise SystemExit(__doc__)
