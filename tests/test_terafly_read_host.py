"""CPU: reading TeraFly trees on the host -- ``terafly.parse_mdata``, ``terafly.open_tree`` and ``TeraFlyTree.imread`` over
``mi_tiff3d_read_box`` (csrc/tiff3d_read.hip: the directory parser for multi-page classic and BigTIFF files, the LZW decoder of
csrc/tiff_lzw_dev.h on host threads).

References: ``terafly.plan`` for what an mdata.bin must say, the numpy restatement of the conversion (tests/terafly_util.py) for the
voxels of every level, Pillow for the pages of the block files the reference's converter wrote through libtiff
(tests/golden/terafly_read).

Depth of a level.  mdata.bin and the directory name carry the nominal depth ``D / 2^h``; the block files hold fewer pages wherever a
z-group of the conversion had an odd number of slices at a level (ipp_amd/terafly.py, module text).  The binary's goldens show it:
u16_max, level 2, is named ...x9, its mdata.bin says 9 and its file has 8 pages (asserted below).  So ``TreeLevel.shape[0]`` is the
page count and ``nominal_depth`` is what mdata.bin says."""
import glob
import os
import shutil

import numpy as np
import pytest

from tests import lzw_util as lu
from tests import terafly_read_util as ru
from tests import terafly_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_READ = os.path.join(ROOT, "tests", "golden", "terafly_read")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def trees(lib, tmp_path_factory):
    """name -> (root, [level volumes]); written once"""
    out = {}
    for name in ru.TREES:
        root = str(tmp_path_factory.mktemp(name))
        out[name] = (root, ru.write_tree(root, name))
    return out


def _plan_of(shape, flags, nbytes):
    from ipp_amd import terafly
    o = tu.parse_flags(flags)
    return terafly.plan(shape, o["resolutions"], (o["height"], o["width"], o["depth"]), o["isotropic"], o["fixed_tiling"],
                        (o["V0"], o["V1"], o["H0"], o["H1"], o["D0"], o["D1"]), nbytes)


def _check_against_plan(md, p, i):
    written = sorted({k for g in p.appends() for (lv, k, _, _) in g if lv == i})
    assert md["version"] == 2.0 and md["reference_system"] == (1, 2, 3) and md["bytes_per_channel"] == p.bytes
    assert md["voxel"] == md["voxel_123"] == (2.0 ** i, 2.0 ** i, 2.0 ** p.hp[i])
    assert md["extents"] == (sum(p.rows[i]), sum(p.cols[i]), sum(p.deps[i][k] for k in written))
    assert (md["n_rows"], md["n_cols"]) == (len(p.rows[i]), len(p.cols[i]))
    assert md["origin"][:2] == tuple(float(np.float32(np.float32(v * 10) / np.float32(10000.0))) for v in (p.V0, p.H0))
    for b, (r0, nr, c0, nc, dirname) in zip(md["blocks"], p.blocks(i)):
        assert (b["dir"], b["height"], b["width"], b["abs_v"], b["abs_h"], b["n_chans"]) == (dirname, nr, nc, r0, c0, 1)
        vh = dirname.split("/")[1]
        assert b["files"] == [f"{vh}_{p.d_name(i, p.d_block_start(i, k))}.tif" for k in written]
        assert b["depths"] == [p.deps[i][k] for k in written] and b["depth"] == sum(b["depths"])
        assert b["abs_d"] == [sum(b["depths"][:q]) for q in range(len(written))]


@pytest.mark.parametrize("run", tu.golden_runs())
def test_parse_mdata_of_the_binarys_files_equals_the_plan(run):
    from ipp_amd import terafly
    g = tu.load_golden(run)
    shape = tuple(int(v) for v in g["recipe_shape"])
    p = _plan_of(shape, [str(f) for f in g["flags"]], np.dtype(str(g["recipe_dtype"])).itemsize)
    seen = 0
    for i in range(p.n_res):
        if p.selected[i]:
            b = g[f"mdata/{p.res_dir(i)}/mdata.bin"].tobytes()
            md = terafly.parse_mdata(b)
            _check_against_plan(md, p, i)
            assert terafly.parse_mdata(terafly.mdata_bytes(p, i)) == md
            seen += 1
    assert seen == sum(p.selected[:p.n_res]) >= 3


def test_parse_mdata_of_the_new_goldens_and_their_page_counts():
    from ipp_amd import terafly
    runs = sorted(f[:-4] for f in os.listdir(GOLDEN_READ) if f.endswith(".npz"))
    assert runs == ["planes_u8", "ramp_u16", "sparse_u16"]
    for run in runs:
        g = np.load(os.path.join(GOLDEN_READ, f"{run}.npz"))
        shape = tuple(int(v) for v in g["recipe_shape"])
        p = _plan_of(shape, [str(f) for f in g["flags"]], np.dtype(str(g["recipe_dtype"])).itemsize)
        for i in range(p.n_res):
            md = terafly.parse_mdata(open(os.path.join(GOLDEN_READ, run, p.res_dir(i), "mdata.bin"), "rb").read())
            _check_against_plan(md, p, i)


def test_the_binarys_mdata_promises_more_slices_than_its_files_hold():
    """the goldens named in the module text: nominal depth against pages, per level"""
    from ipp_amd import terafly
    differ = {}
    for run in ("u16_max", "u16_iso", "u16_012345"):
        g = tu.load_golden(run)
        shape = tuple(int(v) for v in g["recipe_shape"])
        p = _plan_of(shape, [str(f) for f in g["flags"]], 2)
        for i in range(p.n_res):
            md = terafly.parse_mdata(g[f"mdata/{p.res_dir(i)}/mdata.bin"].tobytes())
            b = md["blocks"][0]
            pages = sum(int(g[f"pages/{p.res_dir(i)}/{b['dir']}/{f}"][0]) for f in b["files"])
            assert pages <= md["extents"][2]
            differ[(run, i)] = (md["extents"][2], pages)
    assert differ[("u16_max", 2)] == (9, 8)
    assert differ[("u16_max", 0)] == (37, 37)
    assert any(a != b for a, b in differ.values())


def test_parse_mdata_names_what_it_refuses():
    from ipp_amd import terafly
    import struct
    p = _plan_of((20, 260, 270), ["--resolutions=01"], 2)
    good = terafly.mdata_bytes(p, 0)
    with pytest.raises(ValueError, match="MDATA_BIN_FILE_VERSION"):
        terafly.parse_mdata(struct.pack("<f", 1.0) + good[4:])
    at = 4 + 12 + 24 + 12 + 12 + 4 + 16                       # N_CHANS of the first block
    with pytest.raises(ValueError, match="N_CHANS"):
        terafly.parse_mdata(good[:at] + struct.pack("<I", 3) + good[at + 4:])
    with pytest.raises(ValueError, match="truncated at .*N_BYTESxCHAN"):
        terafly.parse_mdata(good[:-2])
    with pytest.raises(ValueError, match="truncated at .*FILENAMES"):
        terafly.parse_mdata(good[:-16])
    with pytest.raises(ValueError, match="truncated at DIM_V"):
        terafly.parse_mdata(good[:60])


@pytest.mark.parametrize("name", sorted(ru.TREES))
def test_imread_equals_the_restatement(trees, name):
    from ipp_amd import terafly
    root, levels = trees[name]
    dtype, shape, flags, lzw, rps, big = ru.TREES[name]
    t = terafly.open_tree(root)
    assert t.dtype == np.dtype(dtype) and len(t.levels) == len(levels) <= 3
    f0 = sorted(glob.glob(os.path.join(root, t.levels[0].name, "*", "*", "*.tif")))[0]
    info = terafly.tiff3d_info(f0)
    assert (info["bigtiff"], info["compression"], info["bytes"]) == (int(big), 5 if lzw else 1, np.dtype(dtype).itemsize)
    assert info["rows_per_strip"] == (rps if rps else info["ny"])
    for k, (lv, want) in enumerate(zip(t.levels, levels)):
        assert lv.shape == want.shape and lv.nominal_depth >= lv.shape[0]
        for box in ru.boxes(lv.shape, ru.seams_of(lv)):
            z0, z1, y0, y1, x0, x1 = box
            got = t.imread(box, k)
            assert got.dtype == want.dtype and got.shape == (z1 - z0, y1 - y0, x1 - x0)
            assert got.tobytes() == want[z0:z1, y0:y1, x0:x1].tobytes(), (name, k, box)
    if "tiled" in name:
        zs, ys, xs = ru.seams_of(t.levels[0])
        assert len(zs) >= 1 and len(ys) >= 1 and len(xs) >= 1          # the seam box spans 2 x 2 x 2 blocks
        assert t.levels[-1].nominal_depth > t.levels[-1].shape[0] or len(t.levels) < 3
    # an ipp_amd.tsv.VExtent is taken as a box; out= is filled
    from ipp_amd.tsv import VExtent
    want = levels[0]
    out = np.zeros((2, 3, 4), want.dtype)
    assert t.imread(VExtent(5, 9, 2, 5, 1, 3), out=out) is out and out.tobytes() == want[1:3, 2:5, 5:9].tobytes()


def test_every_golden_block_file_equals_pillow():
    from PIL import Image, ImageSequence
    from ipp_amd import terafly
    for run in ("planes_u8", "ramp_u16", "sparse_u16"):
        t = terafly.open_tree(os.path.join(GOLDEN_READ, run))
        assert len(t.levels) == 2
        for k, lv in enumerate(t.levels):
            f, = glob.glob(os.path.join(str(lv.path), "*", "*", "*.tif"))
            pages = np.stack([np.asarray(p) for p in ImageSequence.Iterator(Image.open(f))])
            got = t.imread((0, lv.shape[0], 0, lv.shape[1], 0, lv.shape[2]), k)
            assert got.dtype == pages.dtype and got.tobytes() == pages.tobytes(), (run, k)
            assert t.imread((1, 3, 7, 20, 3, 250 // (k + 1)), k).tobytes() == pages[1:3, 7:20, 3:250 // (k + 1)].tobytes()


@pytest.fixture()
def small_tree(trees, tmp_path):
    """a copy of the classic uncompressed tree with strips of 8 rows, to be damaged"""
    root = str(tmp_path / "tree")
    shutil.copytree(trees["u16_raw_rps8"][0], root)
    f, = glob.glob(os.path.join(root, "RES*", "*", "*", "*.tif"))
    return root, f


def test_refusals_name_the_file_the_page_and_the_tag(small_tree):
    from ipp_amd import capi, terafly
    root, f = small_tree
    good = open(f, "rb").read()
    whole = (0, 10, 0, 261, 0, 270)

    def refused(match):
        with pytest.raises(capi.MiError, match=match) as e:
            terafly.open_tree(root).imread(whole)
        assert os.path.basename(f) in str(e.value)
        open(f, "wb").write(good)
        assert terafly.open_tree(root).imread(whole).shape == (10, 261, 270)

    e = ru.entries(f)
    assert len(e) == 10
    # predictor 2: the PlanarConfiguration entry of page 3 becomes a Predictor entry
    ru.poke(f, e[3][284][0], "<HHIHH", 317, 3, 1, 2, 0)
    refused(r"page 3: tag 317 \(Predictor\) is 2")
    ru.poke(f, e[0][277][3], "<H", 2)
    refused(r"page 0: tag 277 \(SamplesPerPixel\) is 2")
    ru.poke(f, e[1][257][3], "<I", 260)
    refused(r"page 1: tags 256 / 257 .* differ from page 0")
    offs_at, = __import__("struct").unpack_from("<I", good, e[2][273][3])
    ru.poke(f, offs_at + 4 * 5, "<I", len(good) - 100)
    refused(r"page 2: strip 5: tags 273 / 279 .* outside the file")
    ru.poke(f, e[4][259][3], "<H", 8)
    refused(r"page 4: tag 259 \(Compression\) is 8")


def test_missing_block_file_and_box_outside_the_level(small_tree, trees):
    from ipp_amd import terafly
    root, f = small_tree
    t = terafly.open_tree(root)
    for box in ((0, 11, 0, 261, 0, 270), (0, 10, 0, 262, 0, 270), (0, 10, 0, 261, -1, 270), (4, 4, 0, 261, 0, 270)):
        with pytest.raises(ValueError, match="outside level 0 of 10 x 261 x 270"):
            t.imread(box)
    with pytest.raises(ValueError, match="level 1"):
        t.imread((0, 1, 0, 1, 0, 1), level=1)
    os.remove(f)
    with pytest.raises(ValueError, match=os.path.basename(f) + ".*not there"):
        terafly.open_tree(root)
    with pytest.raises(ValueError, match="no RES"):
        terafly.open_tree(os.path.dirname(f))


def test_a_bad_lzw_strip_names_page_strip_and_status(trees, tmp_path):
    from ipp_amd import capi, terafly
    root = str(tmp_path / "tree")
    shutil.copytree(trees["u16_lzw_page_big"][0], root)
    t = terafly.open_tree(root)
    f, = glob.glob(os.path.join(str(t.levels[1].path), "*", "*", "*.tif"))
    pages, b = lu.tiff_pages(f)
    at = pages[2][273]                        # one strip per page: the offset is the entry's value
    ru.poke(f, at, "<BBB", 0x80, 0x40, 0x80)   # Clear, then code 258: the first code after Clear is no literal
    with pytest.raises(capi.MiError, match=r"page 2: strip 0 does not decode to its rows \(status 2: first code is not a literal\)"):
        t.imread((0, 4, 0, 10, 0, 10), 1)
    assert t.imread((0, 2, 0, 10, 0, 10), 1).shape == (2, 10, 10)     # pages the box does not touch are not decoded
