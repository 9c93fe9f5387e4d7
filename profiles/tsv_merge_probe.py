"""The TSVVolume merge on a 4 x 4 grid of 2048^2 uint16 tiles, 10 % overlap, jittered placement, stacks already on the device.

    python profiles/tsv_merge_probe.py [slices] [out.txt]

Per variant one window of REPS launches between two events, after a warm-up launch, three windows, the median: mi_tsv_merge with
`max` and with the cosine blend, mi_merge_slab (terastitcher -6 semantics, SINBLEND) on the same placement, and a device copy of
the output's bytes.  GB/s are output bytes written per second (the figure a user sees: stitched voxels per second); the bytes the
kernel must also read (every output sample once from each covering tile) are listed beside them.
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

R = Cc = 4
HS = WS = 2048
OV = int(0.10 * 2048)
REPS = 10


def placement(seed=4, unit=1):
    """jitter of -3 .. 3 units; with unit = 8 every x offset is a multiple of 8 samples: all tile rows and output rows on 16 bytes"""
    rng = np.random.default_rng(seed)
    jit = lambda r, c: 0 if (r, c) == (0, 0) else unit * int(rng.integers(-3, 4))  # noqa: E731
    step = (WS - OV) // unit * unit
    y0 = np.array([[r * (HS - OV) + jit(r, c) for c in range(Cc)] for r in range(R)], np.int32)
    x0 = np.array([[c * step + jit(r, c) for c in range(Cc)] for r in range(R)], np.int32)
    return x0 - x0.min(), y0 - y0.min()


def timed(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3 / REPS)
    return float(np.median(ts)), ts


def main(n_slices, report):
    import torch
    from ipp_amd import merge, tsv
    from tests import stitch_util as U
    dev = torch.device("cuda", 0)
    x0, y0 = placement()
    z0 = np.zeros(R * Cc, np.int32)
    nz = np.full(R * Cc, n_slices, np.int32)
    g = torch.Generator(device=dev).manual_seed(1)
    stacks = [torch.randint(0, 65520, (n_slices, HS, WS), generator=g, device=dev, dtype=torch.int32).to(torch.uint16) for _ in range(R * Cc)]
    ptrs = (C.c_void_p * (R * Cc))(*[t.data_ptr() for t in stacks])
    ext = tsv.VExtent(0, int(x0.max()) + WS, 0, int(y0.max()) + HS, 0, n_slices)
    out = torch.empty(ext.shape, dtype=torch.uint16, device=dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    out_b = out.numel() * 2
    covered = sum(int((min(ext.x1, x + WS) - x) * (min(ext.y1, y + HS) - y)) for x, y in zip(x0.reshape(-1), y0.reshape(-1))) * n_slices * 2
    say(f"{R}x{Cc} tiles of {HS}x{WS}x{n_slices} uint16, overlap {OV}, jitter +-3 -> volume {ext.shape}: {out_b / 1e9:.2f} GB written, "
        f"{covered / 1e9:.2f} GB of tile samples read (every tile sample lies in the volume)")
    results = {}
    for name, cosine in (("max", False), ("cosine", True)):
        t, ts = timed(lambda: tsv.merge_device(dev, x0.reshape(-1), y0.reshape(-1), z0, nz, HS, WS, ptrs, 2, cosine, ext, out))
        results[name] = t
        say(f"mi_tsv_merge {name:6s}: {t * 1e3:8.2f} ms per launch (windows {', '.join(f'{v * 1e3:.2f}' for v in ts)}) = {out_b / t / 1e9:7.0f} GB/s "
            f"written, {(out_b + covered) / t / 1e9:7.0f} GB/s read + written")
    # terastitcher -6 semantics on the same placement
    av, ah, ad = y0.astype(np.int32), x0.astype(np.int32), np.zeros((R, Cc), np.int32)
    geo = merge.Geometry(R, Cc, av, ah, ad, HS, WS, n_slices, U.volume_dims(av, ah, ad, HS, WS, n_slices))
    D, V, H = geo.shape
    out6 = torch.empty((D, V, H), dtype=torch.uint16, device=dev)
    grid = [[stacks[r * Cc + c] for c in range(Cc)] for r in range(R)]
    t, ts = timed(lambda: merge.merge_slab(geo, grid, np.uint16, 0, 0, D, 0, V, 0, H, out6))
    say(f"mi_merge_slab SINBLEND: {t * 1e3:6.2f} ms per launch (windows {', '.join(f'{v * 1e3:.2f}' for v in ts)}) = {out6.numel() * 2 / t / 1e9:7.0f} GB/s "
        f"written ({D}x{V}x{H})")
    # a device copy of the output's bytes: the least a pass that writes them can take
    a = torch.empty_like(out)
    t, ts = timed(lambda: a.copy_(out))
    say(f"device copy of the output: {t * 1e3:6.2f} ms (windows {', '.join(f'{v * 1e3:.2f}' for v in ts)}) = {out_b / t / 1e9:7.0f} GB/s written, "
        f"{2 * out_b / t / 1e9:7.0f} GB/s read + written")
    for name in ("max", "cosine"):
        say(f"mi_tsv_merge {name}: the copy's time is {t / results[name]:.2f} of its time")
    # the same grid with every x offset a multiple of 8 samples: every run of every tile is one 16-byte load, no cell thinner than 8
    x8, y8 = placement(unit=8)
    ext8 = tsv.VExtent(0, int(x8.max()) + WS, 0, int(y8.max()) + HS, 0, n_slices)
    out8 = torch.empty(ext8.shape, dtype=torch.uint16, device=dev)
    for name, cosine in (("max", False), ("cosine", True)):
        t, ts = timed(lambda: tsv.merge_device(dev, x8.reshape(-1), y8.reshape(-1), z0, nz, HS, WS, ptrs, 2, cosine, ext8, out8))
        say(f"x offsets in multiples of 8, volume {ext8.shape}: mi_tsv_merge {name:6s}: {t * 1e3:8.2f} ms per launch "
            f"(windows {', '.join(f'{v * 1e3:.2f}' for v in ts)}) = {out8.numel() * 2 / t / 1e9:7.0f} GB/s written")
    if report:
        os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
        with open(report, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 16, sys.argv[2] if len(sys.argv) > 2 else None)
