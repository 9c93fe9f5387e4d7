"""CPU: stitching step 5 (global placement, TPAlgoMST::execute) and the host side of step 6 against the reference's OWN binary.

tests/golden/merge/ holds what ``terastitcher -5`` / ``-6`` wrote (generator: tests/golden/make_merge_golden.py, build
container only): the placement of the two committed tile sets and of three fabricated grids (1x5, 4x1, 5x7 with random
reliabilities, zero-reliability links and equal-weight ties), the output trees' file names and a subset of their slices."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from tests import stitch_util as U
from tests.test_gpu_terastitcher_golden import records

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MERGE = os.path.join(GOLD, "merge")
SETS = ("terastitcher", "terastitcher_8bit")
RUNS = ("default", "tiled", "d0d1")
PLACEMENTS = {"1x5": "place_1x5", "4x1": "place_4x1", "5x7": "place_5x7"}


def placement_cases():
    out = [(os.path.join(MERGE, d, "xml_in.xml"), os.path.join(MERGE, d, "xml_out.xml")) for d in PLACEMENTS.values()]
    out += [(os.path.join(GOLD, s, "xml_displthres.xml"), os.path.join(MERGE, s, "xml_merging.xml")) for s in SETS]
    return out


def abs_coords(path):
    return {(int(s.get("ROW")), int(s.get("COL"))): tuple(int(s.get(k)) for k in ("ABS_V", "ABS_H", "ABS_D"))
            for s in ET.parse(path).getroot().find("STACKS")}


@pytest.mark.parametrize("src,want", placement_cases(), ids=[os.path.basename(os.path.dirname(w)) for _, w in placement_cases()])
def test_placement_reproduces_the_binary(src, want):
    from ipp_amd import tsproject
    p = tsproject.Project.load(src)
    p.computeTilesPlacement("MST")
    got = {(s.ROW_INDEX, s.COL_INDEX): (s.ABS_V, s.ABS_H, s.ABS_D) for row in p.STACKS for s in row}
    assert got == abs_coords(want)


def test_placement_goldens_cover_sources_ties_and_unreliable_links():
    """The fabricated projects do what they are for: some links have reliability 0, some equal reliabilities, and one grid's
    top-left stack is not stitchable (the MST source moves)."""
    from ipp_amd import tsproject
    rels, sources = [], []
    for d in PLACEMENTS.values():
        p = tsproject.Project.load(os.path.join(MERGE, d, "xml_in.xml"))
        rels += [s.EAST[0].rel_factors[k] for row in p.STACKS for s in row if s.EAST for k in range(3)]
        rels += [s.SOUTH[0].rel_factors[k] for row in p.STACKS for s in row if s.SOUTH for k in range(3)]
        sources.append(p.computeTilesPlacement())
    assert rels.count(0.0) >= 5
    vals, counts = np.unique([r for r in rels if r > 0], return_counts=True)
    assert counts.max() >= 3
    assert any(s != (0, 0) for s in sources)


@pytest.mark.parametrize("dataset", SETS)
def test_step5_cli_round_trips_the_project(tmp_path, dataset):
    """process_images.py -5 writes the project terastitcher -5 wrote: same coordinates, same records, same flags."""
    from ipp_amd import process_images
    out = tmp_path / "xml_merging.xml"
    assert process_images.main(["-5", f"--projin={os.path.join(GOLD, dataset, 'xml_displthres.xml')}", f"--projout={out}"]) == 0
    want = os.path.join(MERGE, dataset, "xml_merging.xml")
    assert abs_coords(out) == abs_coords(want)
    g, w = records(out), records(want)
    assert g.keys() == w.keys()
    for k in w:
        assert len(g[k]) == len(w[k])
        for a, b in zip(g[k], w[k]):
            for ax in "VHD":
                for f in ("displ", "default_displ", "nccWidth", "nccWRangeThr", "nccInvWidth", "delay"):
                    assert int(a[ax][f]) == int(b[ax][f]), (k, ax, f)
                for f in ("reliability", "nccPeak"):
                    assert float(a[ax][f]) == pytest.approx(float(b[ax][f]), rel=1e-6, abs=1e-7)
    flags = lambda p: {(s.get("ROW"), s.get("COL")): (s.get("STITCHABLE"), s.get("DIR_NAME"), s.get("Z_RANGES"))
                       for s in ET.parse(p).getroot().find("STACKS")}
    assert flags(out) == flags(want)


@pytest.mark.parametrize("dataset", SETS)
@pytest.mark.parametrize("run", RUNS)
def test_output_names_reproduce_the_binary(dataset, run):
    from ipp_amd import merge, tsproject
    g = np.load(os.path.join(MERGE, dataset, f"{run}.npz"))
    flags = {f.split("=")[0]: int(f.split("=")[1]) for f in g["flags"]}
    p = tsproject.Project.load(os.path.join(MERGE, dataset, "xml_merging.xml"))
    V, H, D = (int(v) for v in g["shape"])
    names = merge.output_files(p, (D, V, H), min(flags["--sliceheight"], V), min(flags["--slicewidth"], H), flags.get("--D0", 0))
    want = open(os.path.join(MERGE, dataset, f"{run}.txt")).read().split()
    assert names == want


def _golden_grid(dataset):
    from ipp_amd import tsproject
    npz = np.load(os.path.join(GOLD, dataset, "tiles.npz"))
    p = tsproject.Project.load(os.path.join(MERGE, dataset, "xml_merging.xml"))
    R, C = p.N_ROWS, p.N_COLS
    get = lambda k: np.array([[getattr(p.STACKS[r][c], k) for c in range(C)] for r in range(R)])
    return [[npz[f"tile_{r}_{c}"] for c in range(C)] for r in range(R)], get("ABS_V"), get("ABS_H"), get("ABS_D")


@pytest.mark.parametrize("dataset", SETS)
@pytest.mark.parametrize("run", RUNS)
def test_restatement_reproduces_the_binary(dataset, run):
    """tests/stitch_util.py, the yardstick of the GPU merge, against the binary's own output voxels."""
    stacks, av, ah, ad = _golden_grid(dataset)
    g = np.load(os.path.join(MERGE, dataset, f"{run}.npz"))
    D0 = 5 if run == "d0d1" else 0
    got = np.stack([U.merge_volume(stacks, av, ah, ad, D0=D0 + int(k), D1=D0 + int(k) + 1)[0] for k in g["slices"]])
    assert got.shape == g["volume"].shape
    d = np.abs(got.astype(np.int64) - g["volume"].astype(np.int64))
    assert int((d > 0).sum()) == 0, f"{int((d > 0).sum())} voxels differ, largest difference {int(d.max())}"


def test_volume_dims_follow_the_binary():
    for dataset in SETS:
        stacks, av, ah, ad = _golden_grid(dataset)
        n, h, w = stacks[0][0].shape
        V0, V1, H0, H1, D0, D1 = U.volume_dims(av, ah, ad, h, w, n)
        V, H, D = (int(v) for v in np.load(os.path.join(MERGE, dataset, "default.npz"))["shape"])
        assert (V1 - V0, H1 - H0, D1 - D0) == (V, H, D)


def test_step5_refuses_other_algorithms_and_the_npy_mode(tmp_path):
    from ipp_amd import process_images, tsproject
    src = os.path.join(GOLD, "terastitcher", "xml_displthres.xml")
    for algo in ("LQP", "SCANV", "SCANH"):
        with pytest.raises(SystemExit, match="only MST"):
            process_images.main(["-5", f"--projin={src}", f"--projout={tmp_path / 'x.xml'}", f"--algorithm={algo}"])
        with pytest.raises(ValueError, match="only MST"):
            tsproject.Project.load(src).computeTilesPlacement(algo)
    np.save(tmp_path / "tile_0_0.npy", np.zeros((2, 4, 4), np.uint16))
    with pytest.raises(SystemExit, match="npy mode"):
        process_images.main(["-5", f"--input={tmp_path}", f"--projout={tmp_path / 'x.xml'}"])
    assert not (tmp_path / "x.xml").exists()


def test_step6_refusals(tmp_path):
    from ipp_amd import merge, process_images, tsproject
    src = os.path.join(MERGE, "terastitcher", "xml_merging.xml")
    base = ["-6", f"--projin={src}", f"--volout={tmp_path / 'out'}"]
    with pytest.raises(SystemExit, match="only resolution 0"):
        process_images.main(base + ["--resolutions=01"])
    with pytest.raises(SystemExit, match="only resolution 0"):
        process_images.main(base + ["--resolutions=1"])
    with pytest.raises(SystemExit, match="SINBLEND or NOBLEND"):
        process_images.main(base + ["--algorithm=MAXBLEND"])
    with pytest.raises(SystemExit, match="TiledXY"):
        process_images.main(base + ["--volout_plugin=TiledXY|3Dseries"])
    with pytest.raises(SystemExit, match="npy mode"):
        process_images.main(["-6", f"--input={tmp_path}", f"--volout={tmp_path / 'out'}"])
    with pytest.raises(ValueError, match="at least 250"):
        merge.check_slice_dims(100, 300)
    p = tsproject.Project.load(src)
    p.STACKS[1][2].z_ranges = [(0, 10), (12, 44)]
    with pytest.raises(ValueError, match=r"Z_RANGES \[0,10\);\[12,44\)"):
        merge._check_stacks(p, None)
    assert not (tmp_path / "out").exists()


def _offsets_grid():
    from ipp_amd import tsproject
    npz = np.load(os.path.join(MERGE, "offsets", "tiles.npz"))
    p = tsproject.Project.load(os.path.join(MERGE, "offsets", "xml_merging.xml"))
    R, C = p.N_ROWS, p.N_COLS
    get = lambda k: np.array([[getattr(p.STACKS[r][c], k) for c in range(C)] for r in range(R)])
    return p, [[npz[f"tile_{r}_{c}"] for c in range(C)] for r in range(R)], get("ABS_V"), get("ABS_H"), get("ABS_D")


def test_names_and_voxels_of_a_volume_off_the_origin():
    """A stitched volume that starts at negative V / H and positive D in the stacks' frame: the names carry the offsets
    (UnstitchedVolume moves its origin, and the stream pads "-10" to "000-10"), the voxels follow the restatement."""
    from ipp_amd import merge
    p, stacks, av, ah, ad = _offsets_grid()
    n, h, w = stacks[0][0].shape
    V0, V1, H0, H1, D0, D1 = U.volume_dims(av, ah, ad, h, w, n)
    assert V0 < 0 and H0 < 0 and D0 > 0
    g = np.load(os.path.join(MERGE, "offsets", "default.npz"))
    assert tuple(int(v) for v in g["shape"]) == (V1 - V0, H1 - H0, D1 - D0)
    names = merge.output_files(p, (D1 - D0, V1 - V0, H1 - H0), V1 - V0, H1 - H0, 0, (V0, H0, D0))
    assert names == open(os.path.join(MERGE, "offsets", "default.txt")).read().split()
    got = U.merge_volume(stacks, av, ah, ad)
    d = np.abs(got.astype(np.int64) - g["volume"].astype(np.int64))
    assert int((d > 0).sum()) == 0, f"{int((d > 0).sum())} voxels differ, largest difference {int(d.max())}"
