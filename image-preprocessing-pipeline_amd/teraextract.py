#!/usr/bin/env python3
"""Extracts a sub-volume of a TeraFly tree ("TIFF (tiled, 3D)") as a 2-D TIFF series, through the device (ipp_amd.terafly.open_tree):

    teraextract.py --src=<tree> --dst=<folder> [--level=K] [--V0= --V1= --H0= --H1= --D0= --D1=]

The job of the reference's ``subvolextractor`` (and of ``teraconverter --sfmt="TIFF (tiled, 3D)" --dfmt="TIFF (series, 2D)"``) for
single-channel trees.  --V0/--V1 (rows), --H0/--H1 (columns) and --D0/--D1 (slices) are TemplateCLI's names, half-open, in the
voxels of the chosen level (0: the largest); unset means the level's edge.  Slice z of the level becomes ``img_<z:06>.tif``,
written by the library's device series writer in z slabs sized from the free device memory.  Slices that exist are kept.
"""
import argparse
import os
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parser():
    p = argparse.ArgumentParser(prog="teraextract.py", description=__doc__.split("\n\n")[0], allow_abbrev=False)
    p.add_argument("-s", "--src", required=True)
    p.add_argument("-d", "--dst", required=True)
    p.add_argument("--level", type=int, default=0)
    for k in ("V0", "V1", "H0", "H1", "D0", "D1"):
        p.add_argument(f"--{k}", type=int, default=-1)
    p.add_argument("--route", choices=("host", "device"), default=None, help="where the strips are decoded (default: the library's)")
    p.add_argument("--slab", type=int, default=None, help="slices per slab (default: from the free device memory)")
    return p


def slab_slices(shape_yx, itemsize, device, slab=None):
    """Slices per slab: the box and the writer's scratch beside it in a third of the free device memory"""
    import torch
    if slab is not None:
        return max(1, int(slab))
    free, _ = torch.cuda.mem_get_info(device)
    return max(1, int(free // 3 // max(1, shape_yx[0] * shape_yx[1] * itemsize)))


def extract(src, dst, level=0, sub=(-1, -1, -1, -1, -1, -1), route=None, slab=None, device=None):
    """Writes the series; returns (slices written, the box (z0, z1, y0, y1, x0, x1))."""
    import torch
    from ipp_amd import brickio, capi, terafly
    t = terafly.open_tree(src)
    if not 0 <= level < len(t.levels):
        raise ValueError(f"--level={level}: the tree has levels 0..{len(t.levels) - 1}")
    D, V, H = t.levels[level].shape
    V0, V1, H0, H1, D0, D1 = sub
    box = (max(D0, 0), D if D1 < 0 else D1, max(V0, 0), V if V1 < 0 else V1, max(H0, 0), H if H1 < 0 else H1)
    z0, z1, y0, y1, x0, x1 = box
    if not (z0 < z1 <= D and y0 < y1 <= V and x0 < x1 <= H):
        raise ValueError(f"sub-volume [{y0}, {y1}) x [{x0}, {x1}) x [{z0}, {z1}) outside level {level} of {V} x {H} x {D} (V x H x D)")
    capi.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    step = slab_slices((y1 - y0, x1 - x0), t.dtype.itemsize, dev, slab)
    made = 0
    for a in range(z0, z1, step):
        b = min(z1, a + step)
        vol = t.imread_device((a, b, y0, y1, x0, x1), level, device=dev, route=route)
        made += brickio.save_tiff_series_device(dst, vol, first_index=a)
        del vol
    return made, box


def main(argv=None):
    a = parser().parse_args(sys.argv[1:] if argv is None else list(argv))
    try:
        made, box = extract(a.src, a.dst, a.level, (a.V0, a.V1, a.H0, a.H1, a.D0, a.D1), a.route, a.slab)
    except ValueError as e:
        print(f"teraextract.py: {e}", file=sys.stderr)
        return 2
    print(f"wrote {made} slices of {box[3] - box[2]} x {box[5] - box[4]} (slices {box[0]}..{box[1] - 1} of level {a.level}) under {a.dst}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
