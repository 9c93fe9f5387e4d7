"""Full-grid form of the paired z pass against the predicated form (MI_FFT_Z_GENERAL=1), one process, one workload of bench.py:

    python profiles/zpass_diet_ab.py [c3|c2] [rounds, default 3]

Two contexts -- a plan keeps the switches of the moment it was created --, time_pass("z_conv") over 10 launches each, alternating.
Isolates the plane bounds; everything else of the diet (literal LDS addresses, the z ramp as contiguous loads, the plane twiddle from a
table) is in both, so the total comes from fresh-process runs of bench.py, parent against change."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from ipp_amd import capi, decon  # noqa: E402


def main():
    workload = sys.argv[1] if len(sys.argv) > 1 else "c3"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    vshape, kshape = bench.WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    psf = bench.make_psf(kshape)
    ctxs = {}
    for name, env in (("full", None), ("general", "MI_FFT_Z_GENERAL")):
        if env:
            os.environ[env] = "1"
        os.environ["MI_FFT_PLACE_CANDIDATES"] = "1"   # (two contexts side by side: no placement trial)
        ctxs[name] = decon.RLContext(vshape, psf, None, boundary=capi.BOUNDARY_CIRCULAR, engine=capi.ENGINE_FFT, device=dev)
        if env:
            del os.environ[env]
        print(name, "z_full_grid", ctxs[name].z_full_grid, ctxs[name].otf_form, flush=True)
    assert ctxs["full"].z_full_grid and not ctxs["general"].z_full_grid
    bl = bench.make_volume(vshape, dev)
    for c in ctxs.values():
        c.time_pass("z_conv", bl, reps=3)   # warm
    got = {k: [] for k in ctxs}
    for _ in range(rounds):
        for name, c in ctxs.items():
            got[name].append(c.time_pass("z_conv", bl, reps=10))
    for name, v in got.items():
        print(f"z launch, ms   {name:8s}" + "  ".join(f"{x:.4f}" for x in v), flush=True)


if __name__ == "__main__":
    main()
