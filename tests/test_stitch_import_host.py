"""CPU: stitching step 1 against the reference's OWN binary.  tests/golden/stitch_import/ holds, per case, the project file (or
the error line) that ``terastitcher -1`` gave for a small tile folder (generator: tests/golden/make_import_golden.py, build
container only); ``Project.from_folder`` on the same folder, saved and reloaded, must give the same file element by element
(StackedVolume::init, Stack::init, applyReferenceSystem: vmStackedVolume.cpp:277-560, vmStack.cpp:165-250,792-846)."""
import os

import numpy as np
import pytest

from tests import stitch_import_util as U
from tests.test_gpu_terastitcher_golden import GOLD_ROOT, write_tiff_tree

CASES = U.load_cases()
XML_CASES = sorted(k for k, c in CASES.items() if c["result"] == "xml")
ERROR_CASES = sorted(k for k, c in CASES.items() if c["result"] == "error")
# what the issue lists: every rule of the import has a case, and each kind of refusal
REQUIRED = {"vhd_2x3", "hvd_2x3", "negV_H", "V_negH", "H_negV", "negH_V", "negH_negV", "grid_1x3", "grid_3x1", "grid_1x1",
            "sparse_last", "sparse_middle", "sparse_empty", "sparse_no_first_z", "nosparse_last", "nosparse_middle",
            "nosparse_empty", "nosparse_no_first_z", "origin", "vxl_0351", "bits16", "rgb8", "stray", "unequal_columns",
            "empty_folder", "short_names"}


def from_folder(case, tiles_dir):
    from ipp_amd import tsproject
    return tsproject.Project.from_folder(tiles_dir, U.ref_codes(case), case["vxl"], sparse_data=case["sparse"])


def test_the_golden_set_is_complete():
    assert REQUIRED <= set(CASES)
    for name in XML_CASES:
        assert os.path.exists(os.path.join(U.GOLD, f"{name}.xml")), name
    for name in ERROR_CASES:
        assert os.path.exists(os.path.join(U.GOLD, f"{name}.err")), name
    assert {"sparse_no_first_z", "nosparse_last", "nosparse_empty", "unequal_columns", "empty_folder"} <= set(ERROR_CASES)


@pytest.mark.parametrize("name", XML_CASES)
def test_import_reproduces_the_reference_binary(tmp_path, name):
    from ipp_amd import tsproject
    case, tiles_dir = CASES[name], tmp_path / "tiles"
    U.write_folder(str(tiles_dir), case)
    want = U.golden_text(os.path.join(U.GOLD, f"{name}.xml"), tiles_dir)
    proj = from_folder(case, tiles_dir)
    x1, x2 = tmp_path / "import.xml", tmp_path / "reloaded.xml"
    proj.save(x1)
    U.assert_same_xml(x1, want, name)
    assert x1.read_text() == want                           # and, with TinyXML's layout and %g, the same text
    tsproject.Project.load(x1).save(x2)                     # saved and reloaded: still the binary's file
    U.assert_same_xml(x2, want, f"{name} (reloaded)")
    assert all(not getattr(s, side) for row in proj.STACKS for s in row for side in ("NORTH", "EAST", "SOUTH", "WEST"))
    assert not os.path.exists(tiles_dir / "mdata.bin") or "mdata.bin" in case["tree"]      # never written


@pytest.mark.parametrize("name", ERROR_CASES)
def test_import_refuses_what_the_reference_binary_refuses(tmp_path, name):
    case, tiles_dir = CASES[name], tmp_path / "tiles"
    U.write_folder(str(tiles_dir), case)
    line = U.golden_text(os.path.join(U.GOLD, f"{name}.err"), tiles_dir).strip()
    message = line[line.index("in ") + 3:]
    assert "::" in message
    with pytest.raises(ValueError) as e:
        from_folder(case, tiles_dir)
    assert message in str(e.value), (str(e.value), message)


@pytest.mark.parametrize("dataset", ["terastitcher", "terastitcher_8bit"])
def test_the_committed_import_files_are_reproduced(tmp_path, dataset):
    """The xml_import.xml the binary wrote for the step 2-4 goldens, from the TIFF tree rebuilt out of their tiles.npz."""
    from ipp_amd import tsproject
    gold = os.path.join(GOLD_ROOT, dataset)
    npz = np.load(os.path.join(gold, "tiles.npz"))
    tiles_dir = tmp_path / "tiles"
    write_tiff_tree(str(tiles_dir), npz)
    proj = tsproject.Project.from_folder(tiles_dir, (1, 2, 3), [float(v) for v in npz["vxl"]], sparse_data=True)
    x1 = tmp_path / "xml_import.xml"
    proj.save(x1)
    U.assert_same_xml(x1, U.golden_text(os.path.join(gold, "xml_import.xml"), tiles_dir), dataset)


CHAINS = {"chain_hvd": ("H", "V"), "chain_negH_negV": ("-H", "-V")}


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_host_steps_on_a_transposed_or_mirrored_grid(tmp_path, chain):
    """tests/golden/stitch_import/chain_*: one H-first folder imported as ``H V D`` and as ``-H -V D`` and taken through the
    binary's steps 2-6.  The stacks are permuted, the images are not transposed -- and nothing after step 1 looks at ref_sys:
    our import gives the binary's project, and from the binary's step-2 file the host steps 3, 4 and 5 give its files (step 5 to
    the letter), the output names of step 6 its tree."""
    from ipp_amd import merge, process_images, tsproject
    from tests import stitch_util
    from tests.test_gpu_terastitcher_golden import compare, stack_flags
    gold = os.path.join(U.GOLD, chain)
    npz = np.load(os.path.join(U.GOLD, "chain_hvd", "tiles.npz"))
    tiles_dir = tmp_path / "tiles"
    U.write_hvd_tiff_tree(str(tiles_dir), npz)
    ref1, ref2 = CHAINS[chain]
    x1 = tmp_path / "x1.xml"
    assert process_images.main(["-1", f"--ref1={ref1}", f"--ref2={ref2}", "--ref3=D", f"--vxl1={float(npz['vxl'][1])}",
                                f"--vxl2={float(npz['vxl'][0])}", f"--vxl3={float(npz['vxl'][2])}", "--sparse_data",
                                f"--volin={tiles_dir}", f"--projout={x1}", "--noprogressbar"]) == 0
    assert x1.read_text() == U.golden_text(os.path.join(gold, "xml_import.xml"), tiles_dir)
    n = npz["tile_0_0"].shape[0]
    thr = float(npz["threshold"])
    proj = tsproject.Project.load(os.path.join(gold, "xml_displcomp.xml"))
    y3, y4, y5 = (tmp_path / f"y{k}.xml" for k in (3, 4, 5))
    proj.projectDisplacements()
    proj.save(y3)
    compare(y3, os.path.join(gold, "xml_displproj.xml"), "step 3")
    proj.thresholdDisplacements(thr)
    proj.save(y4)
    compare(y4, os.path.join(gold, "xml_displthres.xml"), "step 4")
    assert stack_flags(y4) == stack_flags(os.path.join(gold, "xml_displthres.xml"))
    placed = tsproject.Project.load(os.path.join(gold, "xml_displthres.xml"))
    placed.computeTilesPlacement()
    placed.save(y5)
    assert y5.read_text() == open(os.path.join(gold, "xml_merging.xml")).read()
    get = lambda k: [[getattr(s, k) for s in row] for row in placed.STACKS]
    v0, v1, h0, h1, d0, d1 = stitch_util.volume_dims(get("ABS_V"), get("ABS_H"), get("ABS_D"), *npz["tile_0_0"].shape[1:], n)
    names = merge.output_files(placed, (d1 - d0, v1 - v0, h1 - h0), v1 - v0, h1 - h0, 0, (v0, h0, d0))
    assert names == open(os.path.join(gold, "merged_names.txt")).read().split()


def reference_command_line(case, tiles_dir, projout):
    """The argument list of the reference's process_images.py:461-474, the program name left out."""
    return ["-1", f"--ref1={case['ref'][0]}", f"--ref2={case['ref'][1]}", f"--ref3={case['ref'][2]}", f"--vxl1={case['vxl'][0]:.3f}",
            f"--vxl2={case['vxl'][1]:.3f}", f"--vxl3={case['vxl'][2]}", "--sparse_data", f"--volin={tiles_dir}",
            f"--projout={projout}", "--noprogressbar"]


@pytest.mark.parametrize("name", ["vxl_0351_hvd", "sparse_mixed_hvd", "negH_negV", "negV_negH_numbers", "vhd_2x3"])
def test_command_line_writes_the_same_file_as_the_python_call(tmp_path, name):
    from ipp_amd import process_images
    case, tiles_dir = dict(CASES[name], sparse=True), tmp_path / "tiles"
    U.write_folder(str(tiles_dir), case)
    x_cli, x_py = tmp_path / "cli.xml", tmp_path / "py.xml"
    assert process_images.main(reference_command_line(case, tiles_dir, x_cli)) == 0
    from_folder(case, tiles_dir).save(x_py)
    assert x_cli.read_text() == x_py.read_text()
    if CASES[name]["sparse"]:
        U.assert_same_xml(x_cli, U.golden_text(os.path.join(U.GOLD, f"{name}.xml"), tiles_dir), name)


def test_command_line_takes_the_plugins_it_has_and_names_the_flag_of_the_others(tmp_path):
    from ipp_amd import process_images
    case, tiles_dir = CASES["hvd_2x3"], tmp_path / "tiles"
    U.write_folder(str(tiles_dir), case)
    line = reference_command_line(case, tiles_dir, tmp_path / "x.xml")
    assert process_images.main(line + ["--volin_plugin=TiledXY|2Dseries", "--imin_plugin=tiff2D"]) == 0
    for flag, value in (("--volin_plugin", "TiledXY|3Dseries"), ("--imin_plugin", "opencv2D")):
        with pytest.raises(SystemExit) as e:
            process_images.main(line + [f"--{flag[2:]}={value}"])
        assert flag in str(e.value) and value in str(e.value)
    with pytest.raises(SystemExit) as e:                    # an error of the import itself: the reference's message
        process_images.main(reference_command_line(CASES["unequal_columns"], tmp_path / "nowhere", tmp_path / "y.xml"))
    assert "in StackedVolume::init(...): Unable to open directory" in str(e.value)
    with pytest.raises(SystemExit) as e:                    # an axis name str2axis does not know
        process_images.main([a.replace("--ref1=H", "--ref1=Q") for a in line])
    assert "invalid importing parameters" in str(e.value)


def test_a_stale_mdata_bin_changes_nothing(tmp_path):
    case, tiles_dir = CASES["sparse_mixed_hvd"], tmp_path / "tiles"
    U.write_folder(str(tiles_dir), case)
    a, b = tmp_path / "a.xml", tmp_path / "b.xml"
    from_folder(case, tiles_dir).save(a)
    stale = tiles_dir / "mdata.bin"
    stale.write_bytes(b"\x00\x01 left by an earlier run of another tool")
    from_folder(case, tiles_dir).save(b)
    assert a.read_text() == b.read_text()
    assert stale.read_bytes() == b"\x00\x01 left by an earlier run of another tool"        # neither read nor rewritten


def test_axis_names_are_parsed_like_str2axis():
    from ipp_amd import tsproject
    for text, code in (("V", 1), ("v", 1), ("Y", 1), ("1", 1), ("vertical", 1), ("-V", -1), ("-1", -1), ("inv_vertical", -1),
                       ("H", 2), ("X", 2), ("-H", -2), ("-x", -2), ("D", 3), ("z", 3), ("-D", -3), ("inv_depth", -3),
                       ("", 0), ("Q", 0), ("-", 0), ("--V", 0), ("-vertical", 0), ("4", 0)):
        assert tsproject.str2axis(text) == code, text
