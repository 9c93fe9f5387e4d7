"""GPU: the stitching chain from OUR import.  ``process_images.py -1`` on the TIFF trees of the step 2-4 goldens, then
``-2 -> -3 -> -4`` on its project, must reproduce the files the reference's binary made from ITS import -- for the two
``V, H, D`` datasets of tests/golden/terastitcher*/ and for tests/golden/stitch_import/chain_hvd/, the same tiles in a folder
whose first level is the H coordinate, imported with the pipeline's default ``--ref1=H --ref2=V --ref3=D`` (generator:
tests/golden/make_import_golden.py).  The standard is test_gpu_terastitcher_golden.compare: integers exact, peaks and
reliabilities to float tolerance."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from tests import stitch_import_util as U
from tests import stitch_util
from tests.test_gpu_stitch_merge import read_tree
from tests.test_gpu_terastitcher_golden import DATASETS, GOLD_ROOT, compare, stack_flags, write_tiff_tree

CHAIN_HVD = os.path.join(U.GOLD, "chain_hvd")


def placement(path):
    """{(row, col): (DIR_NAME, ABS_V, ABS_H, ABS_D)} of a project file."""
    return {(int(st.get("ROW")), int(st.get("COL"))): (st.get("DIR_NAME"),) + tuple(int(st.get(k)) for k in ("ABS_V", "ABS_H", "ABS_D"))
            for st in ET.parse(path).getroot().find("STACKS")}


def run_chain(tmp_path, gold, npz, tiles_dir, ref1, ref2, vxl1, vxl2, n_step2, n_step34):
    """-1 ... -4 with the search radii, subvoldim and threshold of the golden run; every file against the binary's."""
    from ipp_amd import process_images
    x1, x2, x3, x4 = (tmp_path / f"xml_{k}.xml" for k in ("import", "displcomp", "displproj", "displthres"))
    assert process_images.main(["-1", f"--ref1={ref1}", f"--ref2={ref2}", "--ref3=D", f"--vxl1={vxl1}", f"--vxl2={vxl2}",
                                f"--vxl3={float(npz['vxl'][2])}", "--sparse_data", f"--volin={tiles_dir}", f"--projout={x1}",
                                "--noprogressbar"]) == 0
    U.assert_same_xml(x1, U.golden_text(os.path.join(gold, "xml_import.xml"), tiles_dir), "step 1")
    sv, sh, sd = (int(v) for v in npz["search"])
    thr = float(npz["threshold"])
    assert process_images.main(["-2", f"--sV={sv}", f"--sH={sh}", f"--sD={sd}", f"--subvoldim={int(npz['subvoldim'])}",
                                f"--threshold={thr}", f"--projin={x1}", f"--projout={x2}"]) == 0
    assert compare(x2, os.path.join(gold, "xml_displcomp.xml"), "step 2") == n_step2
    assert process_images.main(["-3", f"--projin={x2}", f"--projout={x3}"]) == 0
    assert compare(x3, os.path.join(gold, "xml_displproj.xml"), "step 3") == n_step34
    assert process_images.main(["-4", f"--threshold={thr}", f"--projin={x3}", f"--projout={x4}"]) == 0
    assert compare(x4, os.path.join(gold, "xml_displthres.xml"), "step 4") == n_step34
    assert stack_flags(x4) == stack_flags(os.path.join(gold, "xml_displthres.xml"))
    return x4


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", sorted(DATASETS))
def test_steps_1_to_4_from_our_import(dev, tmp_path, dataset):
    gold = os.path.join(GOLD_ROOT, dataset)
    npz = np.load(os.path.join(gold, "tiles.npz"))
    tiles_dir = tmp_path / "tiles"
    write_tiff_tree(str(tiles_dir), npz)
    run_chain(tmp_path, gold, npz, tiles_dir, "V", "H", float(npz["vxl"][0]), float(npz["vxl"][1]), *DATASETS[dataset])


@pytest.mark.gpu
def test_steps_1_to_6_in_the_default_reference_system(dev, tmp_path):
    """H, V, D: the stacks are transposed by the import, the images are not.  Steps 1-4 against the binary's files and step 5 against its
    placement; of the binary's step 6 (NOBLEND, whole volume) only the file names are kept: ours must give the volume the placed
    project implies, under those names, and give it again."""
    from ipp_amd import process_images, tsproject
    npz = np.load(os.path.join(CHAIN_HVD, "tiles.npz"))
    tiles_dir = tmp_path / "tiles"
    U.write_hvd_tiff_tree(str(tiles_dir), npz)
    x4 = run_chain(tmp_path, CHAIN_HVD, npz, tiles_dir, "H", "V", float(npz["vxl"][1]), float(npz["vxl"][0]),
                   *DATASETS["terastitcher_8bit"])
    proj = tsproject.Project.load(x4)
    rows, cols = int(npz["rows"]), int(npz["cols"])
    assert (proj.N_ROWS, proj.N_COLS, proj.ref_sys) == (rows, cols, (2, 1, 3))
    n, height, width = npz["tile_0_0"].shape
    step_v, step_h = height - int(npz["overlap"][0]), width - int(npz["overlap"][1])
    for r in range(rows):                                   # row = V index, column = H index, although H is the first level
        for c in range(cols):
            v, h = int(round(r * step_v * npz["vxl"][0] * 10)), int(round(c * step_h * npz["vxl"][1] * 10))
            assert proj.STACKS[r][c].DIR_NAME == f"{h:06d}/{h:06d}_{v:06d}"
    x5 = tmp_path / "xml_merging.xml"
    assert process_images.main(["-5", f"--projin={x4}", f"--projout={x5}"]) == 0
    assert placement(x5) == placement(os.path.join(CHAIN_HVD, "xml_merging.xml"))                       # the binary's -5
    placed = tsproject.Project.load(x5)
    get = lambda k: [[getattr(s, k) for s in row] for row in placed.STACKS]
    v0, v1, h0, h1, d0, d1 = stitch_util.volume_dims(get("ABS_V"), get("ABS_H"), get("ABS_D"), height, width, n)
    runs = []
    for k in ("one", "two"):
        out = tmp_path / k
        assert process_images.main(["-6", f"--projin={x5}", f"--volout={out}", "--volout_plugin=TiledXY|2Dseries",
                                    "--algorithm=NOBLEND"]) == 0
        runs.append(read_tree(str(out)))
    names, shape, vol = runs[0]
    assert shape == (v1 - v0, h1 - h0, d1 - d0)
    assert vol.shape == (d1 - d0, v1 - v0, h1 - h0) and vol.dtype == npz["tile_0_0"].dtype
    assert len(names) == d1 - d0 and vol.any()
    assert names == open(os.path.join(CHAIN_HVD, "merged_names.txt")).read().split()                   # the tree of the binary's -6
    assert runs[1][0] == names and runs[1][1] == shape and np.array_equal(runs[1][2], vol)


@pytest.mark.gpu
def test_steps_1_to_5_with_both_axes_inverted(dev, tmp_path):
    """The same folder as ``-H -V D``: rows and columns reversed on top of the transposition, negative voxel sizes and
    mechanical displacements.  Every record of the binary's steps 2-4 and its placed project."""
    from ipp_amd import process_images
    gold = os.path.join(U.GOLD, "chain_negH_negV")
    npz = np.load(os.path.join(CHAIN_HVD, "tiles.npz"))
    tiles_dir = tmp_path / "tiles"
    U.write_hvd_tiff_tree(str(tiles_dir), npz)
    x4 = run_chain(tmp_path, gold, npz, tiles_dir, "-H", "-V", float(npz["vxl"][1]), float(npz["vxl"][0]),
                   *DATASETS["terastitcher_8bit"])
    x5 = tmp_path / "xml_merging.xml"
    assert process_images.main(["-5", f"--projin={x4}", f"--projout={x5}"]) == 0
    assert placement(x5) == placement(os.path.join(gold, "xml_merging.xml"))
