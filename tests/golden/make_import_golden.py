#!/usr/bin/env python3
"""Golden fixtures of stitching step 1 (import) from the reference's OWN binary (build container only; /root/reference never
travels).

For every case of CASES a small two-level tile folder is written (tiles of 10 x 14 pixels: the import reads names and one TIFF
header per stack, no pixel), ``/root/reference/TeraStitcher/Linux/AVX2/terastitcher -1`` is run on it the way the reference's
process_images.py does (process_images.py:460-476), and tests/golden/stitch_import/ receives

    cases.json               per case: the folder (directory and file names), tile size, bit depth, channels, flags
    <case>.xml               the project the binary wrote, its absolute folder replaced by TILES_DIR
    <case>.err               for a case the binary refuses: its error line

A folder is described as {first-level name: {second-level name: [file names]}}; a name that maps to null is a plain file.
``mdata.bin`` is never written by this script: the binary writes its own, and one left by an earlier run would be loaded in
place of the scan -- each case gets a fresh folder.  (tests/test_stitch_import_host.py does create the ``mdata.bin`` a case
lists, with arbitrary bytes: our import must ignore it.)

A second part writes tests/golden/stitch_import/chain_hvd/: the ``terastitcher_8bit`` tiles of make_terastitcher_golden.py in a
folder whose FIRST level is the H coordinate, imported with the pipeline's default ``--ref1=H --ref2=V --ref3=D --sparse_data``
and taken through the binary's steps 2-4 (tiles.npz and the four project files, like tests/golden/terastitcher_8bit/), then
through its ``-5`` and ``-6`` (NOBLEND): xml_merging.xml and merged_names.txt, the file names of the merged tree.
chain_negH_negV/ holds the same files (without tiles.npz: the folder is the same) for ``--ref1=-H --ref2=-V``.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_terastitcher_golden as T  # noqa: E402  (tile generator and the binary's path)

OUT = os.path.join(HERE, "stitch_import")
TILE = (10, 14)                       # height, width: different on purpose


def folder(first, second, zs, missing=None, short_names=False):
    """{<a>: {<a>_<b>: [<a>_<b>_<z>.tif ...]}} for the first / second coordinates and z coordinates (0.1 um, six digits);
    ``missing`` = {(i, j): z indices without a file}; ``short_names`` = the second file-name format of name2coordZ, <z>.tif."""
    tree = {}
    for i, a in enumerate(first):
        row = tree[f"{a:06d}"] = {}
        for j, b in enumerate(second):
            gone = (missing or {}).get((i, j), ())
            row[f"{a:06d}_{b:06d}"] = [f"{z:06d}.tif" if short_names else f"{a:06d}_{b:06d}_{z:06d}.tif"
                                       for k, z in enumerate(zs) if k not in gone]
    return tree


def case(tree, ref="V H D", vxl=(0.8, 0.8, 2.0), sparse=True, bits=8, chans=1):
    return dict(tree=tree, ref=ref.split(), vxl=list(vxl), sparse=sparse, tile=list(TILE), bits=bits, chans=chans)


def with_entries(tree, extra):
    """A copy of ``tree`` with the entries of ``extra`` merged in ({name: None} = a file, {dir: {...}} = merged one level down)."""
    out = {k: (dict(v) if isinstance(v, dict) else v) for k, v in tree.items()}
    for k, v in extra.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k].update(v)
        else:
            out[k] = v
    return out


V2, H3, Z5 = [0, 64], [0, 80, 160], [0, 20, 40, 60, 80]
grid_vh = folder(V2, H3, Z5)              # first level = V: a 2 x 3 grid
grid_hv = folder(H3, V2, Z5)              # first level = H: the same grid for H V D
last, middle, empty, nofirst = {(0, 1): {4}}, {(1, 0): {1, 2}}, {(1, 2): set(range(5))}, {(0, 0): {0}}

CASES = {
    # 1. the two supported systems on a complete 2 x 3 grid
    "vhd_2x3": case(grid_vh, sparse=False),
    "hvd_2x3": case(grid_hv, "H V D", sparse=False),
    "hvd_2x3_sparse_flag": case(grid_hv, "H V D"),
    # 2. negative axes: the mirrors and the origin correction (and a negative voxel size on a positive axis: the sign fix)
    "negV_H": case(grid_vh, "-V H D"),
    "V_negH": case(grid_vh, "V -H D"),
    "H_negV": case(grid_hv, "H -V D"),
    "negH_V": case(grid_hv, "-H V D"),
    "negH_negV": case(grid_hv, "-H -V D"),
    "negV_negH_numbers": case(grid_vh, "-1 -2 3"),
    "V_H_negative_vxl": case(grid_vh, vxl=(-0.8, 0.8, -2.0)),
    # 3. single rows / columns: MEC falls back to extent * VXL
    "grid_1x3": case(folder([0], H3, Z5)),
    "grid_3x1": case(folder([0, 64, 128], [0], Z5)),
    "grid_1x1": case(folder([0], [0], Z5), vxl=(0.351, 1.626, 5.0)),
    "hvd_first_level_1": case(folder([0], V2, Z5), "H V D", vxl=(0.351, 1.626, 5.0)),
    # 4. sparse data
    "sparse_last": case(folder(V2, H3, Z5, last)),
    "sparse_middle": case(folder(V2, H3, Z5, middle)),
    "sparse_empty": case(folder(V2, H3, Z5, empty)),
    "sparse_mixed_hvd": case(folder(H3, V2, Z5, {(0, 1): {4}, (1, 0): {1, 2}, (2, 1): set(range(5))}), "H V D"),
    "sparse_no_first_z": case(folder(V2, H3, Z5, nofirst)),
    "sparse_no_first_z_hvd_neg": case(folder(H3, V2, Z5, {(2, 0): {0}}), "-H V D"),
    "nosparse_last": case(folder(V2, H3, Z5, last), sparse=False),
    "nosparse_middle": case(folder(V2, H3, Z5, middle), sparse=False),
    "nosparse_empty": case(folder(V2, H3, Z5, empty), sparse=False),
    "nosparse_no_first_z": case(folder(V2, H3, Z5, nofirst), sparse=False),
    # 5. a first coordinate other than zero: the origin
    "origin": case(folder([1000, 1064], [2000, 2080, 2160], [300, 320, 340])),
    "origin_hvd_negH_negV": case(folder([2000, 2080, 2160], [1000, 1064], [300, 320, 340]), "-H -V D"),
    # 6. voxel sizes: float -> %g
    "vxl_0351": case(folder([0, 35], [0, 130], Z5), vxl=(0.351, 1.626, 5.0)),
    "vxl_0351_hvd": case(folder([0, 35, 70], [0, 130], [0, 50, 100]), "H V D", vxl=(0.351, 1.626, 5.0)),
    # 7. sample formats
    "bits16": case(grid_vh, bits=16),
    "rgb8": case(grid_vh, chans=3),
    # 8. stray entries
    "stray": case(with_entries(grid_vh, {"notes.txt": None, "mdata.bin": None,
                                        "000000": {"000000_000080 copy": ["000000_000080_000000.tif"]},
                                        "000064": {"000064_000000": grid_vh["000064"]["000064_000000"] + ["Thumbs.db"],
                                                   "old 000064_000080": []}})),
    "unequal_columns": case(with_entries(grid_vh, {"000064": {"000064_000240": ["000064_000240_000000.tif"]}})),
    "empty_folder": case({}),
    "only_files": case({"notes.txt": None}),
    # 9. the second file-name format of name2coordZ
    "short_names": case(folder(V2, H3, Z5, short_names=True)),
    "short_names_sparse": case(folder(V2, H3, Z5, {(0, 2): {2}, (1, 1): {3, 4}}, short_names=True)),
    # refused reference systems
    "ref_V_D_H": case(grid_vh, "V D H"),
    "ref_V_H_negD": case(grid_vh, "V H -D"),
}


def write_folder(root, c):
    """The folder of a case.  ``.tif`` names become TIFFs of the case's size and sample format, other files are empty;
    ``mdata.bin`` is left to the binary."""
    h, w = c["tile"]
    mode = "RGB" if c["chans"] == 3 else ("I;16" if c["bits"] == 16 else "L")
    img = Image.new(mode, (w, h))

    def put(path, name):
        if name == "mdata.bin":
            return
        if name.endswith(".tif"):
            img.save(os.path.join(path, name))
        else:
            open(os.path.join(path, name), "wb").close()

    os.makedirs(root)
    for n1, lev2 in c["tree"].items():
        if lev2 is None:
            put(root, n1)
            continue
        os.makedirs(os.path.join(root, n1))
        for n2, files in lev2.items():
            if files is None:
                put(os.path.join(root, n1), n2)
                continue
            os.makedirs(os.path.join(root, n1, n2))
            for f in files:
                put(os.path.join(root, n1, n2), f)


def import_command(c, vol, xml):
    cmd = [T.TS, "-1", f"--ref1={c['ref'][0]}", f"--ref2={c['ref'][1]}", f"--ref3={c['ref'][2]}", f"--vxl1={c['vxl'][0]}",
           f"--vxl2={c['vxl'][1]}", f"--vxl3={c['vxl'][2]}"]
    return cmd + (["--sparse_data"] if c["sparse"] else []) + [f"--volin={vol}", f"--projout={xml}", "--noprogressbar"]


def generate_cases():
    for f in os.listdir(OUT):
        if f.endswith((".xml", ".err")):
            os.remove(os.path.join(OUT, f))
    for name, c in CASES.items():
        work = tempfile.mkdtemp(prefix="ts_import_")
        try:
            vol, xml = os.path.join(work, "tiles"), os.path.join(work, "import.xml")
            write_folder(vol, c)
            p = subprocess.run(import_command(c, vol, xml), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode == 0 and os.path.exists(xml):
                with open(os.path.join(OUT, f"{name}.xml"), "w") as f:
                    f.write(open(xml).read().replace(vol, "TILES_DIR"))
                c["result"] = "xml"
            else:
                lines = [ln.strip() for ln in p.stdout.splitlines() if " in " in f" {ln}" and "::" in ln]
                if not lines:
                    print(p.stdout[-3000:])
                    raise SystemExit(f"{name}: terastitcher failed with {p.returncode} and no error line")
                with open(os.path.join(OUT, f"{name}.err"), "w") as f:
                    f.write(lines[-1].replace(vol, "TILES_DIR") + "\n")
                c["result"] = "error"
            print(name, c["result"], flush=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(CASES, f, indent=1, sort_keys=True)
        f.write("\n")


def write_chain_tree(root, tiles, cfg):
    """<root>/<H>/<H>_<V>/<H>_<V>_<D>.tif: the tiles of make_terastitcher_golden.write_tree with H as the first level."""
    TILE_, VXL = cfg["TILE"], cfg["VXL"]
    step_v, step_h = TILE_[0] - cfg["OV"][0], TILE_[1] - cfg["OV"][1]
    for (r, c), vol in tiles.items():
        v = int(round(r * step_v * VXL[0] * 10))
        h = int(round(c * step_h * VXL[1] * 10))
        d = os.path.join(root, f"{h:06d}", f"{h:06d}_{v:06d}")
        os.makedirs(d, exist_ok=True)
        for z in range(vol.shape[0]):
            Image.fromarray(vol[z]).save(os.path.join(d, f"{h:06d}_{v:06d}_{int(round(z * VXL[2] * 10)):06d}.tif"))


def generate_chain(name, ref1, ref2, with_tiles):
    cfg = T.DATASETS["terastitcher_8bit"]
    out = os.path.join(OUT, name)
    os.makedirs(out, exist_ok=True)
    VXL, SEARCH, SUBVOL, THRESHOLD = cfg["VXL"], cfg["SEARCH"], cfg["SUBVOL"], cfg["THRESHOLD"]
    tiles = T.make_tiles(cfg)
    work = tempfile.mkdtemp(prefix="ts_import_chain_")
    try:
        vol = os.path.join(work, "tiles")
        write_chain_tree(vol, tiles, cfg)
        x = {k: os.path.join(work, f"xml_{k}.xml") for k in ("import", "displcomp", "displproj", "displthres", "merging")}
        T.run([T.TS, "-1", f"--ref1={ref1}", f"--ref2={ref2}", "--ref3=D", f"--vxl1={VXL[1]}", f"--vxl2={VXL[0]}", f"--vxl3={VXL[2]}",
               "--sparse_data", f"--volin={vol}", f"--projout={x['import']}", "--noprogressbar"])
        T.run([T.TS, "-2", f"--sV={SEARCH[0]}", f"--sH={SEARCH[1]}", f"--sD={SEARCH[2]}", f"--subvoldim={SUBVOL}",
               f"--threshold={THRESHOLD}", f"--projin={x['import']}", f"--projout={x['displcomp']}", "--noprogressbar"])
        T.run([T.TS, "-3", f"--projin={x['displcomp']}", f"--projout={x['displproj']}", "--noprogressbar"])
        T.run([T.TS, "-4", f"--threshold={THRESHOLD}", f"--projin={x['displproj']}", f"--projout={x['displthres']}",
               "--noprogressbar"])
        # steps 5 and 6 as well: the placed project and the NAMES of the merged tree (the voxels are not kept)
        T.run([T.TS, "-5", f"--projin={x['displthres']}", f"--projout={x['merging']}", "--noprogressbar"])
        merged = os.path.join(work, "OUT")
        os.makedirs(merged)
        T.run([T.TS, "-6", f"--projin={x['merging']}", f"--volout={merged}", "--volout_plugin=TiledXY|2Dseries",
               "--slicewidth=100000", "--sliceheight=150000", "--resolutions=0", "--algorithm=NOBLEND", "--noprogressbar"])
        names = sorted(os.path.relpath(os.path.join(d, f), merged) for d, _, fs in os.walk(merged) for f in fs if f.endswith(".tif"))
        with open(os.path.join(out, "merged_names.txt"), "w") as f:
            f.write("\n".join(names) + "\n")
        for k, path in x.items():
            with open(os.path.join(out, f"xml_{k}.xml"), "w") as f:
                f.write(open(path).read().replace(vol, "TILES_DIR"))
        if with_tiles:
            np.savez_compressed(os.path.join(out, "tiles.npz"), rows=cfg["ROWS"], cols=cfg["COLS"], vxl=np.array(VXL),
                                search=np.array(SEARCH), subvoldim=SUBVOL, threshold=THRESHOLD, overlap=np.array(cfg["OV"]),
                                **{f"tile_{r}_{c}": v for (r, c), v in tiles.items()})
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print("wrote", name, sorted(os.listdir(out)))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    generate_cases()
    generate_chain("chain_hvd", "H", "V", with_tiles=True)
    generate_chain("chain_negH_negV", "-H", "-V", with_tiles=False)      # the same folder (chain_hvd/tiles.npz), both axes inverted
