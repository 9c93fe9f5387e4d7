#!/usr/bin/env python3
"""Golden fixtures of stitching steps 5 (placement) and 6 (merge) from the reference's OWN binary (build container only).

For both committed tile sets (tests/golden/terastitcher, tests/golden/terastitcher_8bit) the TIFF tree is recreated as
make_terastitcher_golden.py wrote it, and ``terastitcher -5`` / ``-6`` run on the committed step-4 project:

    terastitcher -5 --projin=xml_displthres.xml --projout=xml_merging.xml
    terastitcher -6 --projin=xml_merging.xml --volout=OUT --volout_plugin="TiledXY|2Dseries" --slicewidth=.. --sliceheight=..
                    [--D0=.. --D1=..]

Stored under tests/golden/merge/:

    <set>/xml_merging.xml        the -5 project (stacks_dir -> TILES_DIR)
    <set>/<run>.npz              the -6 output of one run: the stitched volume of a seeded subset of slices (the tiles of
                                 the tree put back together), the slice indices, the RES() shape
    <set>/<run>.txt              every file name the run wrote, relative to OUT, sorted
    place_<name>/xml_in.xml      a fabricated step-4 project (random reliabilities, zero-reliability links, equal-weight ties)
    place_<name>/xml_out.xml     what ``terastitcher -5`` made of it
    offsets/                     a placed 2x3 grid whose stitched volume starts at negative V / H and positive D in the stacks'
                                 frame (the output names carry the offsets): tiles.npz, xml_merging.xml, default.npz / .txt

Only data is committed: arrays, the XML the binary wrote and name lists.
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ipp_amd import crossmips, tsproject  # noqa: E402
from tests.test_gpu_terastitcher_golden import write_tiff_tree  # noqa: E402

TS = "/root/reference/TeraStitcher/Linux/AVX2/terastitcher"
OUT = os.path.join(ROOT, "tests", "golden", "merge")
# run name -> extra -6 flags (the binary refuses slices under 250 x 250: TMITREE_MIN_BLOCK_DIM); slice subsets keep each
# file well under 1 MiB
RUNS = {
    "default": ["--slicewidth=100000", "--sliceheight=150000"],
    "tiled": ["--slicewidth=250", "--sliceheight=250"],
    "d0d1": ["--slicewidth=100000", "--sliceheight=150000", "--D0=5", "--D1=17"],
}
N_KEEP = 6
PLACEMENTS = {"1x5": (1, 5, 11), "4x1": (4, 1, 12), "5x7": (5, 7, 13)}


def run(cmd):
    print(" ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit(f"terastitcher failed with {p.returncode}")
    return p.stdout


def read_tree(out_dir):
    """(sorted relative file names, RES shape (V, H, D), {slice index: stitched 2-D slice}) of a TiledXY|2Dseries tree."""
    names = sorted(os.path.relpath(os.path.join(d, f), out_dir) for d, _, fs in os.walk(out_dir) for f in fs if f.endswith(".tif"))
    res = [n for n in os.listdir(out_dir) if n.startswith("RES(")]
    assert len(res) == 1, res
    V, H, D = (int(v) for v in res[0][4:-1].split("x"))
    rows = sorted(n for n in os.listdir(os.path.join(out_dir, res[0])) if os.path.isdir(os.path.join(out_dir, res[0], n)))
    slices = {}
    for rdir in rows:
        cols = sorted(os.listdir(os.path.join(out_dir, res[0], rdir)))
        for cdir in cols:
            files = sorted(os.listdir(os.path.join(out_dir, res[0], rdir, cdir)))
            for k, f in enumerate(files):
                slices.setdefault(k, {})[(rdir, cdir)] = np.asarray(Image.open(os.path.join(out_dir, res[0], rdir, cdir, f)))
    vols = {}
    for k, tiles in slices.items():
        rows_img = []
        for rdir in rows:
            rows_img.append(np.concatenate([tiles[(rdir, c)] for c in sorted(os.listdir(os.path.join(out_dir, res[0], rdir)))], axis=1))
        vols[k] = np.concatenate(rows_img, axis=0)
        assert vols[k].shape == (V, H), (vols[k].shape, V, H)
    return names, (V, H, D), vols


def merge_goldens(name):
    gold = os.path.join(ROOT, "tests", "golden", name)
    dst = os.path.join(OUT, name)
    os.makedirs(dst, exist_ok=True)
    work = tempfile.mkdtemp(prefix="merge_golden_")
    try:
        tiles = os.path.join(work, "tiles")
        write_tiff_tree(tiles, np.load(os.path.join(gold, "tiles.npz")))
        x4, x5 = os.path.join(work, "xml_displthres.xml"), os.path.join(work, "xml_merging.xml")
        with open(x4, "w") as f:
            f.write(open(os.path.join(gold, "xml_displthres.xml")).read().replace("TILES_DIR", tiles))
        run([TS, "-5", f"--projin={x4}", f"--projout={x5}", "--noprogressbar"])
        with open(os.path.join(dst, "xml_merging.xml"), "w") as f:
            f.write(open(x5).read().replace(tiles, "TILES_DIR"))
        for rname, flags in RUNS.items():
            out = os.path.join(work, f"OUT_{rname}")
            os.makedirs(out)
            run([TS, "-6", f"--projin={x5}", f"--volout={out}", "--volout_plugin=TiledXY|2Dseries", *flags, "--noprogressbar"])
            names, shape, vols = read_tree(out)
            rng = np.random.default_rng(shape[2] * 100 + len(rname))
            keep = np.sort(rng.choice(shape[2], size=min(N_KEEP, shape[2]), replace=False))
            np.savez_compressed(os.path.join(dst, f"{rname}.npz"), shape=np.array(shape), slices=keep,
                                volume=np.stack([vols[int(k)] for k in keep]), flags=np.array(flags))
            with open(os.path.join(dst, f"{rname}.txt"), "w") as f:
                f.write("\n".join(names) + "\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print("wrote", dst, sorted(os.listdir(dst)))


def fabricated_project(rows, cols, seed, stacks_dir):
    """A step-4 project on a rows x cols grid of tiny 8-bit tiles: random displacements and reliabilities, some links with
    reliability 0 (weight S_UNRELIABLE_WEIGHT) and groups of links with the same reliability (equal-weight paths)."""
    rng = np.random.default_rng(seed)
    TILE, STEP, SLICES = (12, 14), (10, 11), 3
    for r in range(rows):
        for c in range(cols):
            d = os.path.join(stacks_dir, f"{r * STEP[0] * 10:06d}", f"{r * STEP[0] * 10:06d}_{c * STEP[1] * 10:06d}")
            os.makedirs(d, exist_ok=True)
            for z in range(SLICES):
                Image.fromarray(rng.integers(1, 255, TILE, dtype=np.uint8)).save(
                    os.path.join(d, f"{r * STEP[0] * 10:06d}_{c * STEP[1] * 10:06d}_{z * 10:06d}.tif"))
    p = tsproject.Project(stacks_dir, rows, cols, SLICES, VXL=(1.0, 1.0, 1.0), MEC=(STEP[0], STEP[1]))
    for r in range(rows):
        for c in range(cols):
            s = tsproject.Stack(r, c, f"{r * STEP[0] * 10:06d}/{r * STEP[0] * 10:06d}_{c * STEP[1] * 10:06d}",
                                ABS_V=r * STEP[0], ABS_H=c * STEP[1], N_BYTESxCHAN=1, z_ranges=[(0, SLICES)])
            p.STACKS[r][c] = s
    tie_peaks = [0.5, 0.75]

    def record(nominal):
        peaks, widths, coords = [], [], []
        for k in range(3):
            u = rng.random()
            if u < 0.2:       # unreliable: reliability 0
                peaks.append(0.0)
                widths.append(crossmips.S_NCC_WIDTH_MAX)
            elif u < 0.55:    # ties
                peaks.append(float(rng.choice(tie_peaks)))
                widths.append(crossmips.S_NCC_WIDTH_MAX)
            else:
                peaks.append(float(np.float32(rng.uniform(0.3, 0.99))))
                widths.append(int(rng.integers(1, crossmips.S_NCC_WIDTH_MAX)))
            coords.append(nominal[k] + int(rng.integers(-3, 4)))
        d = crossmips.DisplacementMIPNCC(coords, peaks, widths, [3, 3, 2], [crossmips.S_NCC_WIDTH_MAX - 1] * 3,
                                         [crossmips.S_NCC_WIDTH_MAX] * 3)
        return d
    for r in range(rows):
        for c in range(cols):
            if c + 1 < cols:
                p.insertDisplacement(p.STACKS[r][c], p.STACKS[r][c + 1], record((0, STEP[1], 0)))
            if r + 1 < rows:
                p.insertDisplacement(p.STACKS[r][c], p.STACKS[r + 1][c], record((STEP[0], 0, 0)))
    thr = np.float32(0.65)
    for r in range(rows):
        for c in range(cols):
            s = p.STACKS[r][c]
            s.stitchable = any(np.float32(d.getReliability(k)) >= thr for side in tsproject._SIDES for d in getattr(s, side)
                               for k in range(3))
    # the top-left stack is not always stitchable: the MST source then moves
    if seed % 2:
        p.STACKS[0][0].stitchable = False
    return p


def placement_goldens(name, rows, cols, seed):
    dst = os.path.join(OUT, f"place_{name}")
    os.makedirs(dst, exist_ok=True)
    work = tempfile.mkdtemp(prefix="place_golden_")
    try:
        tiles = os.path.join(work, "tiles")
        p = fabricated_project(rows, cols, seed, tiles)
        xin, xout = os.path.join(work, "in.xml"), os.path.join(work, "out.xml")
        p.save(xin)
        run([TS, "-5", f"--projin={xin}", f"--projout={xout}", "--noprogressbar"])
        for src, fname in ((xin, "xml_in.xml"), (xout, "xml_out.xml")):
            with open(os.path.join(dst, fname), "w") as f:
                f.write(open(src).read().replace(tiles, "TILES_DIR"))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print("wrote", dst)


def offsets_golden():
    """-6 on a placed grid with negative ABS_V / ABS_H in the first row / column and ABS_D of both signs."""
    dst = os.path.join(OUT, "offsets")
    os.makedirs(dst, exist_ok=True)
    work = tempfile.mkdtemp(prefix="offsets_golden_")
    try:
        rng = np.random.default_rng(21)
        R, Cc, TILE, N = 2, 3, (40, 44), 6
        av = np.array([[0, -3, 1], [31, 33, 29]])
        ah = np.array([[0, 35, 71], [-2, 33, 70]])
        ad = np.array([[0, 1, -1], [2, 0, 1]])
        tiles_dir = os.path.join(work, "tiles")
        p = tsproject.Project(tiles_dir, R, Cc, N, VXL=(0.7, 0.9, 3.0), ORG=(0.25, -0.5, 0.125), MEC=(28.0, 31.5))
        stacks = {}
        for r in range(R):
            for c in range(Cc):
                d = f"{r:06d}/{r:06d}_{c:06d}"
                os.makedirs(os.path.join(tiles_dir, d))
                vol = rng.integers(1, 65535, size=(N,) + TILE, dtype=np.uint16)
                vol[rng.random(vol.shape) < 0.05] = 0
                for z in range(N):
                    Image.fromarray(vol[z]).save(os.path.join(tiles_dir, d, f"{r:06d}_{c:06d}_{z:06d}.tif"))
                stacks[f"tile_{r}_{c}"] = vol
                p.STACKS[r][c] = tsproject.Stack(r, c, d, ABS_V=int(av[r, c]), ABS_H=int(ah[r, c]), ABS_D=int(ad[r, c]),
                                                 N_BYTESxCHAN=2, stitchable=True, z_ranges=[(0, N)])
        x5 = os.path.join(work, "xml_merging.xml")
        p.save(x5)
        with open(os.path.join(dst, "xml_merging.xml"), "w") as f:
            f.write(open(x5).read().replace(tiles_dir, "TILES_DIR"))
        np.savez_compressed(os.path.join(dst, "tiles.npz"), **stacks)
        out = os.path.join(work, "OUT")
        os.makedirs(out)
        flags = ["--slicewidth=100000", "--sliceheight=150000"]
        run([TS, "-6", f"--projin={x5}", f"--volout={out}", "--volout_plugin=TiledXY|2Dseries", *flags, "--noprogressbar"])
        names, shape, vols = read_tree(out)
        keep = np.arange(shape[2])
        np.savez_compressed(os.path.join(dst, "default.npz"), shape=np.array(shape), slices=keep,
                            volume=np.stack([vols[int(k)] for k in keep]), flags=np.array(flags))
        with open(os.path.join(dst, "default.txt"), "w") as f:
            f.write("\n".join(names) + "\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print("wrote", dst, sorted(os.listdir(dst)))


if __name__ == "__main__":
    for n in ("terastitcher", "terastitcher_8bit"):
        merge_goldens(n)
    for n, (r, c, s) in PLACEMENTS.items():
        placement_goldens(n, r, c, s)
    offsets_golden()
