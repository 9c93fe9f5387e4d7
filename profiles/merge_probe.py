"""Stitching step 6 on a C5-like grid: 8 x 8 stacks of 2048^2 uint16, 15 % overlap, jittered placement.

    python profiles/merge_probe.py kernel [slices]      mi_merge_slab over the whole volume, stacks already on the device: kernel
                                                        time (events, median of 3), bytes (tile bytes read + output bytes written)
                                                        and the fraction of a device-to-device copy of the same byte count
    python profiles/merge_probe.py e2e DIR [slices]     a TIFF tree (deflate slices) of the grid under DIR, then merge_tiles from
                                                        that tree to a TIFF tree out: Mvoxel/s of output
    python profiles/merge_probe.py tree DIR [slices]    only writes the input tree and its project (for terastitcher -6)
"""
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

R = C = 8
HS = WS = 2048
OV = int(0.15 * 2048)


def placement(seed=8):
    rng = np.random.default_rng(seed)
    jit = lambda r, c: 0 if (r, c) == (0, 0) else int(rng.integers(-3, 4))
    av = np.array([[r * (HS - OV) + jit(r, c) for c in range(C)] for r in range(R)], np.int32)
    ah = np.array([[c * (WS - OV) + jit(r, c) for c in range(C)] for r in range(R)], np.int32)
    ad = np.zeros((R, C), np.int32)
    return av, ah, ad


def kernel(n_slices):
    import torch
    from ipp_amd import merge
    from tests import stitch_util as U
    dev = torch.device("cuda", 0)
    av, ah, ad = placement()
    dims = U.volume_dims(av, ah, ad, HS, WS, n_slices)
    geo = merge.Geometry(R, C, av, ah, ad, HS, WS, n_slices, dims)
    D, V, H = geo.shape
    g = torch.Generator(device=dev).manual_seed(1)
    stacks = [[torch.randint(0, 65536, (n_slices, HS, WS), generator=g, device=dev, dtype=torch.int32).to(torch.uint16)
               for _ in range(C)] for _ in range(R)]
    out = torch.empty((D, V, H), dtype=torch.uint16, device=dev)
    ts = []
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        merge.merge_slab(geo, stacks, np.uint16, 0, 0, D, 0, V, 0, H, out)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    t = float(np.median(ts[1:]))
    read_b = R * C * n_slices * HS * WS * 2
    write_b = out.numel() * 2
    # the achievable: a device-to-device copy moving the same bytes (read + write)
    n = (read_b + write_b) // 4
    a = torch.empty(n, dtype=torch.uint16, device=dev)
    b = torch.empty(n, dtype=torch.uint16, device=dev)
    cs = []
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        cs.append(e0.elapsed_time(e1) / 1e3)
    tc = float(np.median(cs[1:]))
    bw, cbw = (read_b + write_b) / t / 1e9, 4 * n / tc / 1e9
    print(f"merge kernel: {R}x{C} stacks of {HS}x{WS}x{n_slices} u16 -> {H}x{V}x{D}: {t * 1e3:.1f} ms, "
          f"{read_b / 1e9:.1f} GB tile samples read + {write_b / 1e9:.1f} GB written = {bw:.0f} GB/s; "
          f"device copy of the same bytes {tc * 1e3:.1f} ms = {cbw:.0f} GB/s; fraction {bw / cbw:.2f}")


def write_tree(root, n_slices):
    from ipp_amd import brickio, tsproject
    av, ah, ad = placement()
    rng = np.random.default_rng(2)
    p = tsproject.Project(root, R, C, n_slices, VXL=(0.5, 0.5, 2.0), MEC=((HS - OV) * 0.5, (WS - OV) * 0.5))
    for r in range(R):
        for c in range(C):
            d = f"{r * 10000:06d}/{r * 10000:06d}_{c * 10000:06d}"
            vol = rng.integers(600, 700, size=(n_slices, HS, WS), dtype=np.uint16)
            idx = rng.integers(0, vol.size, size=vol.size // 2000)
            vol.reshape(-1)[idx] = rng.integers(5000, 60000, size=idx.size, dtype=np.uint16)
            brickio.save_tiff_series(os.path.join(root, d), vol)
            p.STACKS[r][c] = tsproject.Stack(r, c, d, ABS_V=int(av[r, c]), ABS_H=int(ah[r, c]), ABS_D=0, N_BYTESxCHAN=2,
                                             stitchable=True, z_ranges=[(0, n_slices)])
    p.save(os.path.join(root, "xml_merging.xml"))
    return p


def e2e(root, n_slices):
    import torch
    from ipp_amd import merge
    shutil.rmtree(root, ignore_errors=True)
    t0 = time.perf_counter()
    p = write_tree(os.path.join(root, "tiles"), n_slices)
    t_gen = time.perf_counter() - t0
    out = os.path.join(root, "out")
    geo = merge.geometry(p)
    D, V, H = geo.shape
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    made = merge.merge_tiles(p, out, 100000, 100000, device=torch.device("cuda", 0))
    t = time.perf_counter() - t0
    in_b = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(root, "tiles")) for f in fs if f.endswith(".tif"))
    out_b = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(out) for f in fs)
    print(f"merge end to end: TIFF tree of {R}x{C} stacks x {n_slices} slices ({in_b / 1e9:.2f} GB deflate, written in {t_gen:.0f} s) "
          f"-> {made} slices {H}x{V} ({out_b / 1e9:.2f} GB): {t:.2f} s = {D * V * H / t / 1e6:.0f} Mvoxel/s")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 64)
    elif mode == "e2e":
        e2e(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 8)
    else:
        shutil.rmtree(sys.argv[2], ignore_errors=True)
        write_tree(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 8)
