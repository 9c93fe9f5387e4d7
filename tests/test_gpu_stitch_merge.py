"""GPU: stitching step 6 (``process_images.py -6`` / ``mi_merge_slab``) against the reference's OWN binary and against the numpy
restatement tests/stitch_util.py (itself checked against the binary's voxels in tests/test_stitch_placement.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import stitch_util as U
from tests.test_gpu_terastitcher_golden import write_tiff_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MERGE = os.path.join(GOLD, "merge")
SETS = ("terastitcher", "terastitcher_8bit")
RUNS = ("default", "tiled", "d0d1")


def read_tree(out_dir):
    """(sorted file names relative to out_dir, RES shape (V, H, D), (D, V, H) volume put back together from its tiles)."""
    from PIL import Image
    names = sorted(os.path.relpath(os.path.join(d, f), out_dir) for d, _, fs in os.walk(out_dir) for f in fs if f.endswith(".tif"))
    res = [n for n in os.listdir(out_dir) if n.startswith("RES(")]
    assert len(res) == 1, res
    V, H, D = (int(v) for v in res[0][4:-1].split("x"))
    top = os.path.join(out_dir, res[0])
    rows = []
    for rdir in sorted(os.listdir(top)):
        cols = []
        for cdir in sorted(os.listdir(os.path.join(top, rdir))):
            files = sorted(os.listdir(os.path.join(top, rdir, cdir)))
            cols.append(np.stack([np.asarray(Image.open(os.path.join(top, rdir, cdir, f))) for f in files]))
        rows.append(np.concatenate(cols, axis=2))
    vol = np.concatenate(rows, axis=1)
    return names, (V, H, D), vol


def diff_report(got, want):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    return int((d > 0).sum()), int(d.max()) if d.size else 0


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """The TIFF trees of both golden tile sets and their projects after our step 5."""
    from ipp_amd import process_images
    out = {}
    for name in SETS:
        t = tmp_path_factory.mktemp(name)
        tiles = t / "tiles"
        write_tiff_tree(str(tiles), np.load(os.path.join(GOLD, name, "tiles.npz")))
        x4 = t / "xml_displthres.xml"
        x4.write_text(open(os.path.join(GOLD, name, "xml_displthres.xml")).read().replace("TILES_DIR", str(tiles)))
        x5 = t / "xml_merging.xml"
        assert process_images.main(["-5", f"--projin={x4}", f"--projout={x5}"]) == 0
        out[name] = (t, x5)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", SETS)
@pytest.mark.parametrize("run", RUNS)
def test_steps_5_6_reproduce_the_binary_tree(dev, trees, dataset, run):
    from ipp_amd import process_images
    t, x5 = trees[dataset]
    g = np.load(os.path.join(MERGE, dataset, f"{run}.npz"))
    out = t / f"OUT_{run}"
    assert process_images.main(["-6", f"--projin={x5}", f"--volout={out}", "--volout_plugin=TiledXY|2Dseries",
                                *[str(f) for f in g["flags"]]]) == 0
    names, shape, vol = read_tree(str(out))
    assert names == open(os.path.join(MERGE, dataset, f"{run}.txt")).read().split()
    assert shape == tuple(int(v) for v in g["shape"])
    n, mx = diff_report(vol[g["slices"]], g["volume"])
    assert n == 0, f"{n} voxels differ from terastitcher -6, largest difference {mx}"


def _rand_grid(rng, R, C, Hs, Ws, N, ov_v, ov_h, dtype, zero_frac=0.05):
    """A placed R x C grid with jittered ABS_* (negative ABS_D included) and some zero samples."""
    full = 65535 if dtype == np.uint16 else 255
    av = np.zeros((R, C), np.int32)
    ah = np.zeros((R, C), np.int32)
    ad = np.zeros((R, C), np.int32)
    for r in range(R):
        for c in range(C):
            if (r, c) == (0, 0):
                continue
            av[r, c] = r * (Hs - ov_v) + int(rng.integers(-1, 2)) * (ov_v > 2)
            ah[r, c] = c * (Ws - ov_h) + int(rng.integers(-1, 2)) * (ov_h > 2)
            ad[r, c] = int(rng.integers(-2, 3))
    stacks = []
    for r in range(R):
        row = []
        for c in range(C):
            a = rng.integers(1, full + 1, size=(N, Hs, Ws)).astype(dtype)
            a[rng.random(a.shape) < zero_frac] = 0
            row.append(a)
        stacks.append(row)
    return stacks, av, ah, ad


def _gpu_merge(dev, stacks, av, ah, ad, blending, box):
    import torch
    from ipp_amd import merge
    R, C = av.shape
    N, Hs, Ws = stacks[0][0].shape
    geo = merge.Geometry(R, C, av.astype(np.int32), ah.astype(np.int32), ad.astype(np.int32), Hs, Ws, N,
                         U.volume_dims(av, ah, ad, Hs, Ws, N))
    D0, D1, V0, V1, H0, H1 = box
    d0v = geo.dims[4]
    dt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16}[stacks[0][0].dtype]
    dst = [[torch.from_numpy(np.ascontiguousarray(stacks[r][c][D0 + d0v - ad[r, c]:D1 + d0v - ad[r, c]])).to(dev) for c in range(C)]
           for r in range(R)]
    out = torch.full((D1 - D0, V1 - V0, H1 - H0), 7, dtype=dt, device=dev)
    merge.merge_slab(geo, dst, stacks[0][0].dtype, blending, D0, D1, V0, V1, H0, H1, out)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


CASES = [  # (R, C, Hs, Ws, ov_v, ov_h)
    (1, 1, 20, 24, 0, 0),
    (1, 4, 18, 21, 0, 6),
    (4, 1, 17, 22, 5, 0),
    (3, 4, 19, 23, 7, 6),
    (3, 4, 16, 18, 1, 2),
    (2, 3, 15, 17, 2, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c[:2])) + f"_ov{c[4]}-{c[5]}" for c in CASES])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("blending", [U.SINBLEND, U.NOBLEND], ids=["sin", "noblend"])
def test_merge_slab_matches_the_restatement(dev, case, dtype, blending):
    R, C, Hs, Ws, ov_v, ov_h = case
    rng = np.random.default_rng(100 * CASES.index(case) + 10 * np.dtype(dtype).itemsize + blending)
    stacks, av, ah, ad = _rand_grid(rng, R, C, Hs, Ws, 7, ov_v, ov_h, dtype)
    V0, V1, H0, H1, D0, D1 = U.volume_dims(av, ah, ad, Hs, Ws, 7)
    want = U.merge_volume(stacks, av, ah, ad, blending)
    full = (0, D1 - D0, 0, V1 - V0, 0, H1 - H0)
    got = _gpu_merge(dev, stacks, av, ah, ad, blending, full)
    n, mx = diff_report(got, want)
    assert n == 0, f"{n} voxels differ, largest difference {mx}"
    # boxes that start inside an overlap (and end inside another one)
    for _ in range(3):
        b0 = int(rng.integers(0, D1 - D0))
        b1 = int(rng.integers(b0 + 1, D1 - D0 + 1))
        v0 = max(0, Hs - ov_v - 1 + int(rng.integers(0, 2))) if R > 1 else int(rng.integers(0, V1 - V0))
        h0 = max(0, Ws - ov_h - 1 + int(rng.integers(0, 2))) if C > 1 else int(rng.integers(0, H1 - H0))
        v0, h0 = min(v0, V1 - V0 - 1), min(h0, H1 - H0 - 1)
        v1 = int(rng.integers(v0 + 1, V1 - V0 + 1))
        h1 = int(rng.integers(h0 + 1, H1 - H0 + 1))
        got = _gpu_merge(dev, stacks, av, ah, ad, blending, (b0, b1, v0, v1, h0, h1))
        n, mx = diff_report(got, want[b0:b1, v0:v1, h0:h1])
        assert n == 0, f"box {(b0, b1, v0, v1, h0, h1)}: {n} voxels differ, largest difference {mx}"


@pytest.mark.gpu
def test_merge_slab_refuses_bad_boxes(dev):
    import torch
    from ipp_amd import capi, merge
    rng = np.random.default_rng(3)
    stacks, av, ah, ad = _rand_grid(rng, 2, 2, 16, 16, 4, 4, 4, np.uint16)
    ad[:] = 0
    geo = merge.Geometry(2, 2, av, ah, ad, 16, 16, 4, U.volume_dims(av, ah, ad, 16, 16, 4))
    dst = [[torch.zeros((4, 16, 16), dtype=torch.uint16, device=dev) for _ in range(2)] for _ in range(2)]
    out = torch.zeros((1, 1, 1), dtype=torch.uint16, device=dev)
    with pytest.raises(capi.MiError, match="outside the volume"):
        merge.merge_slab(geo, dst, np.uint16, 0, 0, 1, 0, 1, 0, 10_000, out)
    with pytest.raises(capi.MiError, match="blending"):
        merge.merge_slab(geo, dst, np.uint16, 5, 0, 1, 0, 1, 0, 1, out)


def _write_grid_tree(root, stacks, vxl=(1.0, 1.0, 1.0)):
    from PIL import Image
    for r, row in enumerate(stacks):
        for c, vol in enumerate(row):
            d = os.path.join(root, f"{r:06d}", f"{r:06d}_{c:06d}")
            os.makedirs(d, exist_ok=True)
            for z in range(vol.shape[0]):
                Image.fromarray(vol[z]).save(os.path.join(d, f"{r:06d}_{c:06d}_{z:06d}.tif"))


def _placed_project(root, stacks, av, ah, ad):
    from ipp_amd import tsproject
    R, C = av.shape
    N = stacks[0][0].shape[0]
    p = tsproject.Project(root, R, C, N, VXL=(0.5, 0.5, 2.0), MEC=(1.0, 1.0))
    for r in range(R):
        for c in range(C):
            p.STACKS[r][c] = tsproject.Stack(r, c, f"{r:06d}/{r:06d}_{c:06d}", ABS_V=int(av[r, c]), ABS_H=int(ah[r, c]),
                                             ABS_D=int(ad[r, c]), N_BYTESxCHAN=stacks[0][0].dtype.itemsize, stitchable=True,
                                             z_ranges=[(0, N)])
    return p


@pytest.mark.gpu
def test_slab_size_does_not_change_the_tree(dev, tmp_path):
    from ipp_amd import merge
    rng = np.random.default_rng(11)
    stacks, av, ah, ad = _rand_grid(rng, 3, 3, 120, 140, 17, 20, 24, np.uint16)
    _write_grid_tree(str(tmp_path / "tiles"), stacks)
    p = _placed_project(str(tmp_path / "tiles"), stacks, av, ah, ad)
    trees = []
    for slab in (1, 7, None):
        out = tmp_path / f"out_{slab}"
        merge.merge_tiles(p, out, 250, 250, device=dev, slab=slab or 10_000)
        trees.append(read_tree(str(out)))
    for names, shape, vol in trees[1:]:
        assert names == trees[0][0] and shape == trees[0][1]
        assert np.array_equal(vol, trees[0][2])
    want = U.merge_volume(stacks, av, ah, ad)
    n, mx = diff_report(trees[0][2], want)
    assert n == 0, f"{n} voxels differ from the restatement, largest difference {mx}"


@pytest.mark.gpu
def test_two_processes_split_the_z_range(dev, tmp_path):
    """-6 under two ranks (RANK / WORLD_SIZE as torchrun sets them, no collective) writes the tree of one process."""
    from ipp_amd import process_images
    rng = np.random.default_rng(5)
    stacks, av, ah, ad = _rand_grid(rng, 2, 3, 90, 100, 13, 15, 18, np.uint8)
    _write_grid_tree(str(tmp_path / "tiles"), stacks)
    x5 = tmp_path / "xml_merging.xml"
    _placed_project(str(tmp_path / "tiles"), stacks, av, ah, ad).save(x5)
    one = tmp_path / "one"
    assert process_images.main(["-6", f"--projin={x5}", f"--volout={one}"]) == 0
    two = tmp_path / "two"
    cmd = [sys.executable, os.path.join(ROOT, "image-preprocessing-pipeline_amd", "process_images.py"), "-6", f"--projin={x5}",
           f"--volout={two}"]
    procs = [subprocess.Popen(cmd, cwd=ROOT, env={**os.environ, "RANK": str(k), "WORLD_SIZE": "2", "LOCAL_RANK": "0"})
             for k in range(2)]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    a, b = read_tree(str(one)), read_tree(str(two))
    assert a[0] == b[0] and a[1] == b[1]
    assert np.array_equal(a[2], b[2])


@pytest.mark.gpu
def test_large_grid_past_2_31_bytes(dev):
    """8 x 8 stacks of 2048^2 u16, 15 % overlap: the output slab passes 2^31 bytes; rows across every seam of the last slice
    (whose offsets are past 2^31) against the restatement."""
    import torch
    from ipp_amd import merge
    R = C = 8
    Hs = Ws = 2048
    ov = int(0.15 * 2048)
    N = 8
    rng = np.random.default_rng(8)
    av = np.array([[r * (Hs - ov) + (int(rng.integers(-3, 4)) if (r, c) != (0, 0) else 0) for c in range(C)] for r in range(R)], np.int32)
    ah = np.array([[c * (Ws - ov) + (int(rng.integers(-3, 4)) if (r, c) != (0, 0) else 0) for c in range(C)] for r in range(R)], np.int32)
    ad = np.array([[0 if (r, c) == (0, 0) else int(rng.integers(-1, 2)) for c in range(C)] for r in range(R)], np.int32)
    V0, V1, H0, H1, D0, D1 = U.volume_dims(av, ah, ad, Hs, Ws, N)
    depth = D1 - D0
    assert depth * (V1 - V0) * (H1 - H0) * 2 > 2 ** 31
    geo = merge.Geometry(R, C, av, ah, ad, Hs, Ws, N, (V0, V1, H0, H1, D0, D1))
    g = torch.Generator(device=dev).manual_seed(1)
    dst = [[torch.randint(0, 65536, (depth, Hs, Ws), generator=g, device=dev, dtype=torch.int32).to(torch.uint16) for _ in range(C)]
           for _ in range(R)]
    out = torch.empty((depth, V1 - V0, H1 - H0), dtype=torch.uint16, device=dev)
    merge.merge_slab(geo, dst, np.uint16, U.SINBLEND, 0, depth, 0, V1 - V0, 0, H1 - H0, out)
    torch.cuda.synchronize(dev)
    z = depth - 1
    got = out[z].cpu().numpy()
    tiles = [[U.to_float(dst[r][c][z].cpu().numpy()) for c in range(C)] for r in range(R)]
    want = U.to_samples(U.merge_slice(tiles, av, ah, Hs, Ws), np.uint16)
    rows = sorted({int(v) for r in range(1, R) for v in (av[r].min() - V0 + 3, av[r - 1].max() + Hs - V0 - 4)} |
                  {5, (V1 - V0) // 2, V1 - V0 - 1})
    n, mx = diff_report(got[rows], want[rows])
    assert n == 0, f"{n} voxels differ in rows {rows}, largest difference {mx}"
    cols = sorted({int(h) for c in range(1, C) for h in (ah[:, c].min() - H0 + 2, ah[:, c - 1].max() + Ws - H0 - 3)})
    n, mx = diff_report(got[:, cols], want[:, cols])
    assert n == 0, f"{n} voxels differ in columns {cols}, largest difference {mx}"


@pytest.mark.gpu
def test_step6_reproduces_the_binary_off_the_origin(dev, tmp_path):
    """A placed grid whose stitched volume starts at negative V / H and positive D: names and voxels of terastitcher -6."""
    from PIL import Image
    from ipp_amd import process_images
    npz = np.load(os.path.join(MERGE, "offsets", "tiles.npz"))
    tiles = tmp_path / "tiles"
    for key in npz.files:
        r, c = (int(v) for v in key.split("_")[1:])
        d = tiles / f"{r:06d}" / f"{r:06d}_{c:06d}"
        d.mkdir(parents=True)
        for z, sl in enumerate(npz[key]):
            Image.fromarray(sl).save(d / f"{r:06d}_{c:06d}_{z:06d}.tif")
    x5 = tmp_path / "xml_merging.xml"
    x5.write_text(open(os.path.join(MERGE, "offsets", "xml_merging.xml")).read().replace("TILES_DIR", str(tiles)))
    g = np.load(os.path.join(MERGE, "offsets", "default.npz"))
    out = tmp_path / "OUT"
    assert process_images.main(["-6", f"--projin={x5}", f"--volout={out}", *[str(f) for f in g["flags"]]]) == 0
    names, shape, vol = read_tree(str(out))
    assert names == open(os.path.join(MERGE, "offsets", "default.txt")).read().split()
    n, mx = diff_report(vol, g["volume"])
    assert n == 0, f"{n} voxels differ from terastitcher -6, largest difference {mx}"
