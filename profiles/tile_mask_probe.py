"""The foreground mask of filter_streaks (ipp_amd.pystripe.MaskPlan, include/mi_tile_mask.h) on the GPU.

    python profiles/tile_mask_probe.py            one 2048 x 2048 uint16 slice (a bright body with holes on a dark, speckled
                                                  background): ms of the whole mask at the defaults (close 50, open 500) with its
                                                  fill rounds; of threshold + fill alone (boxes 1, 1); of close = open = 5 and
                                                  close = open = 500 (the morphology's share is the difference to boxes 1, 1); and a
                                                  device-to-device copy of the tile for scale.  Device time by events around
                                                  MaskPlan.run, which waits for the fill's flags itself; median of 5 after a warm-up.
                                                  Every mask is compared with the restatement of tests/mask_util.py first.
                                                  Then the morphology alone: the same slice inside a 600-sample frame of foreground,
                                                  which survives every box, so no corner is background and the fill settles in its
                                                  first round whatever the boxes are; boxes (k, k) minus boxes (1, 1) on that tile
                                                  is the eight passes of the morphology, whose work does not depend on the content.
    python profiles/tile_mask_probe.py trace      one warm-up and one run at the defaults -- for
                                                  rocprofv3 --kernel-trace --stats -- python3 profiles/tile_mask_probe.py trace
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def slice_u16(ny=2048, nx=2048, seed=5):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:ny, :nx]
    body = ((yy - 0.52 * ny) / (0.36 * ny)) ** 2 + ((xx - 0.48 * nx) / (0.41 * nx)) ** 2 < 1 + 0.08 * np.sin(yy / 37.0) * np.cos(xx / 53.0)
    for cy, cx, r in ((0.45, 0.40, 0.035), (0.45, 0.56, 0.035), (0.62, 0.48, 0.02)):     # ventricles
        body &= ((yy - cy * ny) ** 2 + (xx - cx * nx) ** 2) > (r * ny) ** 2
    img = np.where(body, 2400.0, 90.0) * (1 + 0.2 * rng.standard_normal((ny, nx)))
    img[rng.random((ny, nx)) < 0.002] = 4000.0
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16)


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


def main(mode):
    import torch
    from ipp_amd import pystripe as ps
    from tests import mask_util as M
    dev = torch.device("cuda", 0)
    img = slice_u16()
    x = torch.from_numpy(img).to(dev)[None].contiguous()
    thr = 700
    cases = [(50, 500)] if mode == "trace" else [(50, 500), (1, 1), (5, 5), (500, 500)]
    for close_steps, open_steps in cases:
        plan = ps.MaskPlan(dev, img.shape, img.dtype, close_steps, open_steps, 4, 1)
        mask = plan.run(x, thr)
        torch.cuda.synchronize()
        rounds = plan.fill_rounds
        if mode == "trace":
            plan.run(x, thr)
            torch.cuda.synchronize()
            plan.close()
            return
        want = M.fill(M.close_open_scipy(img > thr, close_steps, open_steps))
        same = bool(np.array_equal(mask[0].cpu().numpy().astype(bool), want))
        ms = timed(lambda: plan.run(x, thr))
        print(f"2048 x 2048 uint16, close {close_steps:3d}, open {open_steps:3d}: {ms:7.3f} ms, {rounds} fill rounds, foreground {want.mean():.3f}, "
              f"equal to the restatement: {same}, scratch {plan.info.scratch_bytes / 1e6:.1f} MB")
        plan.close()
    framed = img.copy()
    framed[:600, :] = framed[-600:, :] = 4000
    framed[:, :600] = framed[:, -600:] = 4000
    xf = torch.from_numpy(framed).to(dev)[None].contiguous()
    base = None
    for k in (1, 5, 50, 500):
        plan = ps.MaskPlan(dev, img.shape, img.dtype, k, k, 4, 1)
        mask = plan.run(xf, thr)
        torch.cuda.synchronize()
        same = bool(np.array_equal(mask[0].cpu().numpy().astype(bool), M.fill(M.close_open_scipy(framed > thr, k, k))))
        ms = timed(lambda: plan.run(xf, thr))
        base = ms if base is None else base
        print(f"framed slice, close = open = {k:3d}: {ms:7.3f} ms, {plan.fill_rounds} fill round(s), equal to the restatement: {same}"
              + ("" if k == 1 else f"; morphology = {ms - base:6.3f} ms"))
        plan.close()
    dst = torch.empty_like(x)
    print(f"device copy of the tile's {x.numel() * 2 / 1e6:.1f} MB: {timed(lambda: dst.copy_(x)):.4f} ms")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "times")
