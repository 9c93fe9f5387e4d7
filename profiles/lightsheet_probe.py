"""The lightsheet correction (ipp_amd.pystripe, include/mi_lightsheet.h) on the GPU.

    python profiles/lightsheet_probe.py plan             ms per tile of the lightsheet plan alone at the defaults (L 150, W 200,
                                                         percentile 0.25): 2048 x 2048 uint16 at batch 1 and 32 and one
                                                         15000 x 20000 uint16 slice; device time by events (median of 5), each as a
                                                         multiple of a device-to-device copy of the tile's bytes in the same process
    python profiles/lightsheet_probe.py stage            process_img(sigma=(250, 250), db9, reflect, bidirectional) on 2048 x 2048
                                                         uint16 with and without lightsheet=True (batch 1 and 32), same process
    python profiles/lightsheet_probe.py trace [B]        one warm-up and one run of the plan on a batch of B (default 32) -- for
                                                         rocprofv3 --kernel-trace --stats -- python3 profiles/lightsheet_probe.py trace
    python profiles/lightsheet_probe.py slice            the same for the 15000 x 20000 slice
    python profiles/lightsheet_probe.py cpu              the restatement of tests/lightsheet_util.py (the reference's loop of
                                                         numpy.percentile calls) on one 2048 x 2048 tile, one core
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

PIPE = dict(sigma=(250, 250), wavelet="db9", padding_mode="reflect", bidirectional=True)


def tiles_u16(n, ny, nx, dev):
    """smooth background + row streaks + noise, made on the device"""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    yy = torch.arange(ny, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(nx, device=dev, dtype=torch.float32)[None, :]
    base = 400 + 250 * torch.sin(yy / 97.0) * torch.cos(xx / 131.0)
    out = torch.empty((n, ny, nx), dtype=torch.uint16, device=dev)
    for i in range(n):
        streak = 300 * torch.rand((ny, 1), generator=g, device=dev) ** 4
        noise = 30 + 6 * torch.randn((ny, nx), generator=g, device=dev)
        out[i] = (base + streak + noise).clamp(0, 65535).to(torch.int32).to(torch.uint16)
    return out


def timed(fn, reps=5):
    import torch
    ts = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts[1:]))


def make_plan(ps, dev, shape, batch):
    return ps.LightsheetPlan(dev, shape, np.uint16, ps.make_lightsheet_params(np.uint16, max_batch=batch))


def plan_times():
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    for shape, batches in (((2048, 2048), (1, 32)), ((15000, 20000), (1,))):
        x = tiles_u16(max(batches), shape[0], shape[1], dev)
        for b in batches:
            plan = make_plan(ps, dev, shape, b)
            xb, out = x[:b].contiguous(), torch.empty_like(x[:b])
            plan.run(xb, out)
            ms = timed(lambda: plan.run(xb, out))
            dst = torch.empty_like(xb)
            mc = timed(lambda: dst.copy_(xb))
            i = plan.info
            print(f"{shape[0]} x {shape[1]} uint16 batch {b:2d}: {ms / b:8.3f} ms per tile; grids {i.ls_ny} x {i.ls_nx} and {i.bg_ny} x {i.bg_nx}, "
                  f"largest window {i.max_window_samples}; device copy of the tile's {xb[0].numel() * 2 / 1e6:.1f} MB: {mc / b:.4f} ms "
                  f"-> the plan is {ms / mc:.0f} x a copy")
            plan.close()
        del x


def stage():
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    x = tiles_u16(32, 2048, 2048, dev)
    for b in (1, 32):
        xb = x[:b].contiguous()
        for ls in (False, True):
            pipe = ps.Pipeline(dev, (2048, 2048), np.uint16, max_batch=b, lightsheet=dict() if ls else None, **PIPE)
            pipe.run(xb)
            ms = timed(lambda: pipe.run(xb))
            print(f"process_img sigma (250, 250) db9 reflect bidirectional, 2048 x 2048 uint16, batch {b:2d}, lightsheet={ls}: "
                  f"{ms / b:8.3f} ms per tile")
            pipe.close()


def trace(shape, b):
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    x = tiles_u16(b, shape[0], shape[1], dev)
    plan = make_plan(ps, dev, shape, b)
    for _ in range(2):
        plan.run(x)
    torch.cuda.synchronize()
    plan.close()


def cpu():
    from tests import lightsheet_util as L
    img = L.bead_and_stripe_tile((2048, 2048), 60, np.uint16)
    t0 = time.perf_counter()
    L.correct_lightsheet(img)
    print(f"CPU restatement (the reference's loop of numpy.percentile calls), 2048 x 2048 uint16, one core: {time.perf_counter() - t0:.2f} s per tile")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "plan"
    if mode == "plan":
        plan_times()
    elif mode == "stage":
        stage()
    elif mode == "trace":
        trace((2048, 2048), int(sys.argv[2]) if len(sys.argv) > 2 else 32)
    elif mode == "slice":
        trace((15000, 20000), 1)
    elif mode == "cpu":
        cpu()
    else:
        raise SystemExit(__doc__)
