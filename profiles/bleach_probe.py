"""The bleach correction of the pystripe stage (ipp_amd.pystripe) on the GPU.

    python profiles/bleach_probe.py tiles [B ...]   ms per 2048 x 2048 uint16 tile, batches B (default 32 1): sigma (0, 0) with the bleach
                                                    correction, row method and max method; sigma (250, 250) without and with it (the
                                                    difference is the price of the step); beside each a device copy of the bytes the
                                                    step must move
    python profiles/bleach_probe.py slice [NY NX]   one uint16 slice (default 20000 x 15000, rows of 15000) at batch 1, both methods,
                                                    and the same samples as rows of 30000 (the segmented long-row route)
    python profiles/bleach_probe.py trace [B]       one warm-up and one run of batch B, row method, sigma (0, 0) -- for
                                                    rocprofv3 --kernel-trace --stats -- python3 profiles/bleach_probe.py trace 32
Device time by events, median of 5 after a warm-up.
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from profiles.pystripe_probe import PIPE, tiles_u16, timed  # noqa: E402

CLIPS = dict(bleach_correction_clip_min=math.log1p(200.0), bleach_correction_clip_med=math.log1p(1000.0),
             bleach_correction_clip_max=math.log1p(3000.0))


def copy_ms(nbytes, dev):
    """a device copy that moves nbytes in all (half read, half written)"""
    import torch
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src))


def run_case(label, dev, x, must_bytes, **kw):
    import torch
    from ipp_amd import pystripe as ps
    b, ny, nx = x.shape
    plan = ps.Plan(dev, (ny, nx), np.uint16, ps.make_params(np.uint16, max_batch=b, **kw))
    out = torch.empty((b, ny, nx), dtype=torch.uint16, device=dev)
    plan.run(x, out=out)
    ms = timed(lambda: plan.run(x, out=out))
    info = plan.info
    line = f"{label:44s} batch {b:3d}: {ms / b:8.3f} ms per tile, scratch {info.scratch_bytes_per_tile / 1e6:7.1f} MB per tile, long rows {info.bleach_long_rows}"
    if must_bytes:
        mc = copy_ms(b * ny * nx * must_bytes, dev)
        line += f"; must move {must_bytes} B per pixel, device copy of them {mc / b:.3f} ms per tile ({ms / mc:.1f} x)"
    print(line, flush=True)
    plan.close()
    return ms / b


def tiles(batches):
    import torch
    dev = torch.device("cuda", 0)
    tin = tiles_u16(max(batches), dev)
    for b in batches:
        x = tin[:b].contiguous()
        # rows: read tile 2, write F 4, read tile 2, read F 4, write result 2; max method: read tile 2 (maxima), read tile 2, write 2
        run_case("sigma (0, 0) + bleach, rows", dev, x, 14, sigma=(0, 0), bleach_correction_frequency=1 / 2048, **CLIPS)
        run_case("sigma (0, 0) + bleach, max method", dev, x, 6, sigma=(0, 0), bleach_correction_frequency=1 / 2048,
                 bleach_correction_max_method=True, **CLIPS)
        base = run_case("sigma (250, 250)", dev, x, 0, sigma=(250, 250), **PIPE)
        # behind the stripe filter L is a float32 image: rows write L 4, read L 4, write F 4, read L 4, read F 4 (the result's 2 bytes were
        # the filter's before); max method write L 4, read L 4, read L 4
        rows = run_case("sigma (250, 250) + bleach, rows", dev, x, 20, sigma=(250, 250), bleach_correction_frequency=1 / 2048, **CLIPS, **PIPE)
        mm = run_case("sigma (250, 250) + bleach, max method", dev, x, 12, sigma=(250, 250), bleach_correction_frequency=1 / 2048,
                      bleach_correction_max_method=True, **CLIPS, **PIPE)
        print(f"price of the step behind sigma (250, 250) at batch {b}: rows {rows - base:.3f} ms per tile, max method {mm - base:.3f} ms per tile", flush=True)


def slice_(ny, nx):
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    x = (300 + 3000 * torch.rand((1, ny, nx), generator=g, device=dev)).to(torch.int32).to(torch.uint16)
    f = 1 / min(ny, nx)
    run_case(f"{ny} x {nx} slice, rows", dev, x, 14, sigma=(0, 0), bleach_correction_frequency=f, **CLIPS)
    run_case(f"{ny} x {nx} slice, max method", dev, x, 6, sigma=(0, 0), bleach_correction_frequency=f, bleach_correction_max_method=True, **CLIPS)
    wide = x.reshape(1, ny * nx // 30000, 30000).contiguous() if (ny * nx) % 30000 == 0 else None
    if wide is not None:
        # the long-row route adds the float64 forward row: written 8, read 8
        run_case(f"{wide.shape[1]} x 30000 (same samples), rows", dev, wide, 30, sigma=(0, 0), bleach_correction_frequency=f, **CLIPS)
        run_case(f"{wide.shape[1]} x 30000 (same samples), max method", dev, wide, 6, sigma=(0, 0), bleach_correction_frequency=f,
                 bleach_correction_max_method=True, **CLIPS)


def trace(b):
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    x = tiles_u16(b, dev)
    plan = ps.Plan(dev, (2048, 2048), np.uint16, ps.make_params(np.uint16, sigma=(0, 0), bleach_correction_frequency=1 / 2048, max_batch=b, **CLIPS))
    for _ in range(2):
        plan.run(x)
    torch.cuda.synchronize()
    plan.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "tiles"
    if mode == "tiles":
        tiles([int(v) for v in sys.argv[2:]] or [32, 1])
    elif mode == "slice":
        slice_(*([int(v) for v in sys.argv[2:4]] or [20000, 15000]))
    elif mode == "trace":
        trace(int(sys.argv[2]) if len(sys.argv) > 2 else 32)
    else:
        raise SystemExit(__doc__)
