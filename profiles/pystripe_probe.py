"""The pystripe stage (ipp_amd.pystripe) on the GPU.

    python profiles/pystripe_probe.py kernel [B ...]     ms per 2048 x 2048 uint16 tile at the pipeline's sigma settings ((100, 100),
                                                         (128, 256), (250, 250); db9, reflect, bidirectional), batches B (default 1 8 32):
                                                         device time by events (median of 5), the bytes a tile must cross (read +
                                                         write), and a device copy of the same bytes
    python profiles/pystripe_probe.py trace [B]          one warm-up and one run of batch B at sigma (250, 250) -- for
                                                         rocprofv3 --kernel-trace --stats -- python3 profiles/pystripe_probe.py trace 8
    python profiles/pystripe_probe.py wavelet [B ...]    sigma (250, 250) with "db9" by name, the 18 db9 coefficients (the kernels for any
                                                         tap count) and a 90-tap orthonormal filter, batches B (default 32 1): ms per
                                                         tile, five runs of the median of 5 and their spread
    python profiles/pystripe_probe.py wavelet_trace K [B]  one warm-up and one run of choice K (0, 1, 2 in that order), batch B -- for
                                                         rocprofv3 --kernel-trace --stats, which gives the wavelet passes' share
    python profiles/pystripe_probe.py padmodes [MODE ...]  sigma (250, 250), batch 16, one plan per padding mode (default: reflect and the six
                                                         value modes): ms per tile by a host clock around 10 synchronised runs, seven
                                                         such rounds: their median, least and largest.  One MODE under rocprofv3
                                                         --kernel-trace --stats gives the share of the pad_* kernels
    python profiles/pystripe_probe.py e2e DIR [tiles]   `tiles` (default 256) deflate TIFF tiles of 2048 x 2048 uint16 under DIR/in,
                                                         then batch_filter -> DIR/out: tiles/s and the read / compute / write seconds
    python profiles/pystripe_probe.py cpu                the numpy / scipy restatement of tests/pystripe_util.py on one tile (context
                                                         only: it is not the reference's implementation, which needs PyWavelets)
"""
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

NY = NX = 2048
SIGMAS = [(100, 100), (128, 256), (250, 250)]
PIPE = dict(wavelet="db9", padding_mode="reflect", bidirectional=True)


def tiles_u16(n, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    yy = torch.arange(NY, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(NX, device=dev, dtype=torch.float32)[None, :]
    blob = 300 + 4000 * torch.exp(-((yy - NY / 2) ** 2 + (xx - NX / 2) ** 2) / (0.03 * NY * NX))
    out = torch.empty((n, NY, NX), dtype=torch.uint16, device=dev)
    for i in range(n):
        gain = 1 + 0.3 * torch.randn((NY, 1), generator=g, device=dev)
        noise = 40 + 6 * torch.randn((NY, NX), generator=g, device=dev)
        out[i] = ((blob + noise) * gain).clamp(0, 65535).to(torch.int32).to(torch.uint16)
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


def kernel(batches):
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    nb = max(batches)
    tin = tiles_u16(nb, dev)
    must = 2 * NY * NX * 2
    for sigma in SIGMAS:
        for b in batches:
            prm = ps.make_params(np.uint16, sigma=sigma, max_batch=b, **PIPE)
            plan = ps.Plan(dev, (NY, NX), np.uint16, prm)
            out = torch.empty((b, NY, NX), dtype=torch.uint16, device=dev)
            x = tin[:b].contiguous()
            plan.run(x, out=out)
            ms = timed(lambda: plan.run(x, out=out))
            info = plan.info
            print(f"sigma {sigma} batch {b:3d}: {ms / b:8.3f} ms per tile ({ms:9.3f} ms per batch), padded {info.padded_ny} x {info.padded_nx}, "
                  f"{info.levels} levels, scratch {info.scratch_bytes_per_tile / 1e6:.0f} MB per tile")
            plan.close()
    src = torch.empty(nb * must // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    mc = timed(lambda: dst.copy_(src))
    print(f"a tile must cross {must / 1e6:.1f} MB (read {must / 2e6:.1f} + write {must / 2e6:.1f}); device copy of {nb} x {must / 2e6:.1f} MB: "
          f"{mc / nb:.4f} ms per tile")


def lattice_rec_lo(taps, seed=1):
    """an orthonormal low-pass of any even length (the paraunitary lattice of tests/wavelet_util.py): stands in for coif15's 90 taps"""
    from tests import wavelet_util as W
    return W.lattice_filter(taps, seed)


def wavelet_choices():
    from ipp_amd import wavelets
    return [("db9 by name (18-tap kernels)", "db9"), ("db9 as 18 coefficients (any-length kernels)", wavelets.daubechies(9)),
            ("90 taps (any-length kernels)", lattice_rec_lo(90))]


def wavelet(batches, runs=5):
    """2048^2 uint16, sigma (250, 250), reflect, bidirectional: ms per tile for each wavelet choice; `runs` runs of the median-of-5
    each, whose spread is the run-to-run spread.  The share of the wavelet passes comes from `wavelet_trace` under rocprofv3."""
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    tin = tiles_u16(max(batches), dev)
    for label, w in wavelet_choices():
        for b in batches:
            prm = ps.make_params(np.uint16, sigma=(250, 250), max_batch=b, **dict(PIPE, wavelet=w))
            plan = ps.Plan(dev, (NY, NX), np.uint16, prm)
            out = torch.empty((b, NY, NX), dtype=torch.uint16, device=dev)
            x = tin[:b].contiguous()
            plan.run(x, out=out)
            ms = [timed(lambda: plan.run(x, out=out)) / b for _ in range(runs)]
            print(f"{label}, batch {b:3d}: {np.median(ms):7.3f} ms per tile (runs {' '.join(f'{v:.3f}' for v in ms)}; spread "
                  f"{100 * (max(ms) - min(ms)) / np.median(ms):.1f} %), {plan.info.levels} levels")
            plan.close()


def wavelet_trace(which, b):
    """one warm-up and one run of batch b with wavelet choice `which` (0, 1, 2 of wavelet_choices) -- for rocprofv3 --kernel-trace --stats"""
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    x = tiles_u16(b, dev)
    label, w = wavelet_choices()[which]
    plan = ps.Plan(dev, (NY, NX), np.uint16, ps.make_params(np.uint16, sigma=(250, 250), max_batch=b, **dict(PIPE, wavelet=w)))
    for _ in range(2):
        plan.run(x)
    torch.cuda.synchronize()
    plan.close()
    print(label)


def trace(b):
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    x = tiles_u16(b, dev)
    plan = ps.Plan(dev, (NY, NX), np.uint16, ps.make_params(np.uint16, sigma=(250, 250), max_batch=b, **PIPE))
    for _ in range(2):
        plan.run(x)
    torch.cuda.synchronize()
    plan.close()


def padmodes(modes, rounds=7, reps=10, batch=16):
    import torch
    from ipp_amd import pystripe as ps
    from tests import pystripe_util as U
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(np.stack([U.synthetic_tile((NY, NX), 100 + i, np.uint16) for i in range(batch)])).to(dev)
    for mode in modes:
        plan = ps.Plan(dev, (NY, NX), np.uint16, ps.make_params(np.uint16, sigma=(250, 250), max_batch=batch, extended=True,
                                                                **dict(PIPE, padding_mode=mode)))
        out = plan.run(x)
        for _ in range(3):
            plan.run(x, out=out)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            for _ in range(reps):
                plan.run(x, out=out)
            torch.cuda.synchronize(dev)
            ms.append((time.perf_counter() - t0) / reps / batch * 1e3)
        print(f"{mode:12s} batch {batch}: {np.median(ms):.4f} ms per tile ({rounds} rounds of {reps} runs: {min(ms):.4f} .. {max(ms):.4f}), "
              f"scratch {plan.info.scratch_bytes_per_tile / 1e6:.0f} MB per tile", flush=True)
        plan.close()


def e2e(folder, n):
    import torch
    from ipp_amd import pystripe as ps
    dev = torch.device("cuda", 0)
    src, dst = os.path.join(folder, "in"), os.path.join(folder, "out")
    shutil.rmtree(folder, ignore_errors=True)
    t0 = time.perf_counter()
    base = tiles_u16(16, dev).cpu().numpy()
    for i in range(n):
        ps.imsave_tif(os.path.join(src, f"{i // 64:06d}", f"tile_{i:06d}.tif"), np.roll(base[i % 16], i, axis=1))
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(src) for f in fs)
    print(f"wrote {n} tiles ({size / 1e9:.2f} GB of deflate TIFF) in {time.perf_counter() - t0:.1f} s")
    stats = {}
    t0 = time.perf_counter()
    ps.batch_filter(src, dst, sigma=(250, 250), stats=stats, device=dev, **PIPE)
    dt = time.perf_counter() - t0
    busy = stats["read_s"] + stats["compute_s"] + stats["write_s"]
    print(f"batch_filter: {n} tiles in {dt:.2f} s = {n / dt:.1f} tiles/s ({n * NY * NX / dt / 1e6:.0f} Mvoxel/s); read {stats['read_s']:.2f} s, "
          f"compute (upload + kernels + download) {stats['compute_s']:.2f} s, write {stats['write_s']:.2f} s "
          f"(shares {stats['read_s'] / busy:.2f} / {stats['compute_s'] / busy:.2f} / {stats['write_s'] / busy:.2f}; the three overlap)")
    shutil.rmtree(folder, ignore_errors=True)


def cpu():
    from tests import pystripe_util as U
    img = U.synthetic_tile((NY, NX), 11, np.uint16)
    for sigma in SIGMAS:
        t0 = time.perf_counter()
        U.process_img(img.copy(), sigma=sigma, dt=np.float32, **PIPE)
        print(f"CPU restatement (numpy / scipy, float32) sigma {sigma}: {time.perf_counter() - t0:.2f} s per tile")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        kernel([int(v) for v in sys.argv[2:]] or [1, 8, 32])
    elif mode == "wavelet":
        wavelet([int(v) for v in sys.argv[2:]] or [32, 1])
    elif mode == "wavelet_trace":
        wavelet_trace(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 32)
    elif mode == "trace":
        trace(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    elif mode == "padmodes":
        padmodes(sys.argv[2:] or ["reflect", "constant", "linear_ramp", "maximum", "mean", "median", "minimum", "reflect"])
    elif mode == "e2e":
        e2e(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 256)
    elif mode == "cpu":
        cpu()
    else:
        raise SystemExit(__doc__)
