"""The TeraFly conversion (ipp_amd.terafly) on the GPU.

    python profiles/terafly_probe.py kernel                 mi_pyramid_slab on a 64 x 4096 x 8192 uint16 group (levels 1..5, mean):
                                                            kernel time (events, median of 5), bytes (level 0 read + levels written)
                                                            and the fraction of a device-to-device copy of the same byte count
    python profiles/terafly_probe.py e2e DIR [slices]       a 2-D series of `slices` uncompressed 4096 x 8192 uint16 slices under DIR,
                                                            then the pipeline's conversion (--resolutions=012345, mean) with
                                                            --libtiff_uncompress and with LZW: Mvoxel/s of level 0
    python profiles/terafly_probe.py series DIR [slices]    only writes the series (for the reference teraconverter)
"""
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

NY, NX = 4096, 8192


def kernel():
    import torch
    from ipp_amd import terafly
    dev = torch.device("cuda", 0)
    nz, hd = 64, [1, 1, 1, 1, 1]
    slab = torch.randint(0, 65536, (nz, NY, NX), dtype=torch.int32, device=dev).to(torch.uint16)
    shapes = terafly.level_shapes(tuple(slab.shape), len(hd), hd)
    outs = [torch.empty(s, dtype=torch.uint16, device=dev) for s in shapes]
    nbytes = slab.numel() * 2 + sum(o.numel() * 2 for o in outs)
    src = torch.empty(nbytes // 2, dtype=torch.uint16, device=dev)
    dst = torch.empty_like(src)

    def timed(fn, reps=5):
        ts = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / 1e3)
        return float(np.median(ts[1:]))
    tk = timed(lambda: terafly.pyramid_slab(slab, len(hd), hd, "mean", outs))
    tc = timed(lambda: dst.copy_(src))
    print(f"kernel: group {nz} x {NY} x {NX} uint16, levels 1..5 mean: {tk * 1e3:.3f} ms, {nbytes / tk / 1e9:.0f} GB/s "
          f"(read {slab.numel() * 2 / 1e9:.2f} GB + wrote {(nbytes - slab.numel() * 2) / 1e9:.2f} GB)")
    print(f"device copy of the same {nbytes / 1e9:.2f} GB: {tc * 1e3:.3f} ms, {nbytes / tc / 1e9:.0f} GB/s; "
          f"kernel / copy = {tc / tk:.2f}")


def series(folder, n):
    import torch
    from ipp_amd import brickio
    os.makedirs(folder, exist_ok=True)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    for z0 in range(0, n, 16):
        z1 = min(n, z0 + 16)
        # smooth-ish content with noise: compresses like a real stitched volume more than white noise does
        base = torch.randint(0, 2000, (z1 - z0, NY // 16, NX // 16), dtype=torch.int32, device=dev, generator=g).float()
        vol = torch.nn.functional.interpolate(base[None, None], size=(z1 - z0, NY, NX), mode="trilinear")[0, 0]
        vol = (vol + torch.randint(0, 64, vol.shape, device=dev, generator=g)).to(torch.int32).to(torch.uint16).cpu().numpy()
        brickio.save_tiff_series(folder, vol, first_index=z0 + 1, compression=None)
    return n * NY * NX


def e2e(folder, n):
    from ipp_amd import terafly
    t0 = time.perf_counter()
    vox = series(os.path.join(folder, "src"), n)
    print(f"series: {n} slices of {NY} x {NX} uint16 = {vox * 2 / 1e9:.2f} GB written in {time.perf_counter() - t0:.1f} s")
    for lzw in (False, True):
        out = os.path.join(folder, "lzw" if lzw else "raw")
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        t0 = time.perf_counter()
        terafly.convert(os.path.join(folder, "src"), out, "012345", "mean", compression=lzw)
        dt = time.perf_counter() - t0
        size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(out) for f in fs)
        print(f"e2e {'LZW' if lzw else 'uncompressed'}: {dt:.1f} s, {vox / dt / 1e6:.0f} Mvoxel/s of level 0, tree {size / 1e9:.2f} GB")
        shutil.rmtree(out, ignore_errors=True)


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "kernel":
        kernel()
    elif what == "e2e":
        e2e(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 128)
    elif what == "series":
        series(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 128)
