#!/usr/bin/env python3
"""``teraconverter`` for the pipeline's TeraFly step, on the GPU (ipp_amd.terafly):

    teraconverter.py --sfmt="TIFF (series, 2D)" --dfmt="TIFF (tiled, 3D)" --resolutions="012345" --clist=0 --halve=mean \\
                     -s=<slices> -d=<existing folder>

Takes the reference's flag spelling (TemplateCLI.cpp) for this subset: -s/--src, -d/--dst, --sfmt, --dfmt, --resolutions,
--halve=mean|max, --clist=0, --height/--width/--depth, --isotropic, --fixed_tiling, --libtiff_uncompress, --libtiff_rowsperstrip,
--libtiff_bigtiff, --V0/--V1/--H0/--H1/--D0/--D1, --noprogressbar (and --mdata_fname, which the reference ignores for this
destination).  Of its own: --slab_rows (rows of a device band) and --lzw_encoder=host|device (where the LZW strips are encoded).  Other source / destination formats, a --clist other than 0 and multi-channel slices are refused by name.
"""
import argparse
import os
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SFMT = "TIFF (series, 2D)"
DFMT = "TIFF (tiled, 3D)"


def parser():
    p = argparse.ArgumentParser(prog="teraconverter.py", description=__doc__.split("\n\n")[0], allow_abbrev=False)
    p.add_argument("-s", "--src", required=True)
    p.add_argument("-d", "--dst", required=True)
    p.add_argument("--sfmt", required=True)
    p.add_argument("--dfmt", required=True)
    p.add_argument("--resolutions", default="0")
    p.add_argument("--halve", default="mean")
    p.add_argument("--clist", default="")
    p.add_argument("--height", type=int, default=-1)
    p.add_argument("--width", type=int, default=-1)
    p.add_argument("--depth", type=int, default=-1)
    p.add_argument("--isotropic", action="store_true")
    p.add_argument("--fixed_tiling", action="store_true")
    p.add_argument("--libtiff_uncompress", action="store_true")
    p.add_argument("--libtiff_rowsperstrip", type=int, default=1)
    p.add_argument("--libtiff_bigtiff", action="store_true")
    for k in ("V0", "V1", "H0", "H1", "D0", "D1"):
        p.add_argument(f"--{k}", type=int, default=-1)
    p.add_argument("--noprogressbar", action="store_true")
    p.add_argument("--mdata_fname", default="")
    p.add_argument("--slab_rows", type=int, default=None, help="rows of a device band (default: from the free device memory)")
    p.add_argument("--lzw_encoder", choices=("host", "device"), default=None,
                   help="where the LZW strips are encoded (default: MI_TERAFLY_WRITE_DEVICE, else the host)")
    return p


def check_args(a):
    """Raises ValueError for what this converter does not do (before touching the source or the GPU)."""
    if a.sfmt != SFMT:
        raise ValueError(f'--sfmt="{a.sfmt}": only "{SFMT}" is supported')
    if a.dfmt != DFMT:
        raise ValueError(f'--dfmt="{a.dfmt}": only "{DFMT}" is supported')
    if a.clist not in ("", "0"):
        raise ValueError(f"--clist={a.clist}: single-channel sources only (--clist=0)")
    if a.halve not in ("mean", "max"):
        raise ValueError(f"--halve={a.halve}: mean or max")
    if a.libtiff_rowsperstrip == -1:
        raise ValueError("--libtiff_rowsperstrip=-1 (whole image per strip) is not supported; give a row count")
    if a.libtiff_rowsperstrip < 1:
        raise ValueError(f"--libtiff_rowsperstrip={a.libtiff_rowsperstrip}")


def _split_short(argv):
    """TCLAP takes ``-s=PATH``; argparse would read the value as "=PATH"."""
    out = []
    for v in argv:
        if len(v) > 3 and v[0] == "-" and v[1] in "sd" and v[2] == "=":
            out += [v[:2], v[3:]]
        else:
            out.append(v)
    return out


def main(argv=None):
    a = parser().parse_args(_split_short(sys.argv[1:] if argv is None else list(argv)))
    try:
        check_args(a)
    except ValueError as e:
        print(f"teraconverter.py: {e}", file=sys.stderr)
        return 2
    from ipp_amd import terafly

    def progress(k, n):
        print(f"\rgroup {k} of {n}", end="" if k < n else "\n", flush=True)
    try:
        p = terafly.convert(a.src, a.dst, a.resolutions, a.halve, (a.height, a.width, a.depth), a.isotropic, a.fixed_tiling,
                            (a.V0, a.V1, a.H0, a.H1, a.D0, a.D1), not a.libtiff_uncompress, a.libtiff_rowsperstrip,
                            a.libtiff_bigtiff, slab_rows=a.slab_rows, progress=None if a.noprogressbar else progress,
                            encoder=a.lzw_encoder)
    except ValueError as e:
        print(f"teraconverter.py: {e}", file=sys.stderr)
        return 2
    print(f"wrote {sum(p.selected[:p.n_res])} resolutions of {p.height} x {p.width} x {p.depth} under {a.dst}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
