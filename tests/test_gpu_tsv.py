"""GPU: the TSVVolume merge (include/mi_tsv.h, ipp_amd.tsv) against goldens made by the reference's own ``TSVVolume.imread``
(tests/golden/make_tsv_golden.py) and against the numpy restatement (tests/tsv_util.py).  Everything is exact except case E (a
260-column overlap), whose bound is stated at its test."""
import functools
import subprocess
import sys

import numpy as np
import pytest

from tests import tsv_util as T

pytestmark = pytest.mark.gpu
BLENDS = ("max", "cosine")


@pytest.fixture(scope="module")
def projects(tmp_path_factory):
    """case name -> the XML path of the case, tiles written once per module from their seeds"""
    from ipp_amd import pystripe
    root = tmp_path_factory.mktemp("tsv")
    made = {}

    def get(name):
        if name not in made:
            case = T.CASES[name]
            made[name] = case.write(root / name, lambda path, plane: pystripe.imsave_tif(path, plane, None), case.stored_xml())
        return made[name]
    return get


@pytest.fixture(scope="module")
def volumes(projects, dev):
    """(case name, blend) -> (TSVVolume, its full read on the host)"""
    from ipp_amd import tsv
    made = {}

    def get(name, blend):
        if (name, blend) not in made:
            case = T.CASES[name]
            vol = tsv.TSVVolume(projects(name), ignore_z_offsets=case.ignore_z_offsets, cosine_blending=blend == "cosine", device=dev)
            full = vol.imread(vol.volume, vol.dtype)
            full.setflags(write=False)
            made[name, blend] = (vol, full)
        return made[name, blend]
    return get


@functools.lru_cache(maxsize=None)
def golden(name):
    g = T.load_golden(T.CASES[name])
    for a in g.values():
        a.setflags(write=False)
    return g


@pytest.mark.parametrize("blend", BLENDS)
@pytest.mark.parametrize("name", T.EXACT_CASES)
def test_full_read_equals_the_reference(volumes, name, blend):
    vol, full = volumes(name, blend)
    want = golden(name)[blend]
    assert full.dtype == want.dtype and full.shape == want.shape
    differ = int((full != want).sum())
    print(f"{name} {blend}: {differ} of {want.size} voxels differ")
    assert differ == 0


def test_wide_overlap_within_one_float16_step(volumes):
    """Case E, weights up to d = od = 260: every voxel within one float16 step of the reference's, at most 0.1 % of the overlap voxels
    different at all (with the weight in double rounded once, none is expected to be)."""
    vol, full = volumes("E", "cosine")
    want = golden("E")["cosine"]
    assert full.shape == want.shape
    case = T.CASES["E"]
    x0 = golden("E")["x0"].reshape(-1)
    overlap = (x0.min() + case.width - x0.max()) * min(case.height, want.shape[1]) * want.shape[0]
    differ = full != want
    # one float16 step at the reference's value: the spacing of float16 there (the result was a float16 before the cast)
    with np.errstate(over="ignore"):   # the spacing at float16's largest values is inf
        step = np.maximum(np.spacing(want.astype(np.float16)).astype(np.float64), 1.0)
    excess = np.abs(full.astype(np.float64) - want.astype(np.float64)) - step
    print(f"E cosine: {int(differ.sum())} of {overlap} overlap voxels differ, largest |difference| - step = {excess.max()}")
    assert excess.max() <= 0
    assert differ.sum() <= 0.001 * overlap


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_offsets_and_extent_equal_the_reference(volumes, name):
    case = T.CASES[name]
    vol, _ = volumes(name, case.blends[-1])
    g = golden(name)
    v = vol.volume
    assert (v.x0, v.x1, v.y0, v.y1, v.z0, v.z1) == tuple(g["extent"].tolist())
    assert v.shape == g[case.blends[-1]].shape
    for key in ("x0", "y0", "z0"):
        got = [[getattr(vol.offsets[r][c], key[0]) for c in range(case.cols)] for r in range(case.rows)]
        assert got == g[key].tolist(), key
    assert (vol.stack_rows, vol.stack_columns) == (case.rows, case.cols) and vol.dtype == case.dtype.type
    assert vol.voxel_dims == (5.0, 2.0, 2.0)
    s = vol.stacks[case.rows - 1][case.cols - 1]
    assert (s.x0, s.y0, s.z0) == (g["x0"][-1, -1], g["y0"][-1, -1], g["z0"][-1, -1]) and s.x1 - s.x0 == case.width


@pytest.mark.parametrize("blend", BLENDS)
@pytest.mark.parametrize("name", ("A", "C", "F_z_ranges"))
def test_sub_boxes_equal_the_slice_of_the_full_read(volumes, name, blend):
    from ipp_amd import tsv
    vol, _ = volumes(name, blend)
    g = golden(name)
    extent = tuple(g["extent"].tolist())
    for box in T.sub_boxes(extent):
        got = vol.imread(tsv.VExtent(*box), vol.dtype)
        assert np.array_equal(got, T.slice_of(g[blend], extent, box)), box
    outside = T.sub_boxes(extent)[2]
    assert not vol.imread(tsv.VExtent(*outside), vol.dtype).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# mi_tsv_merge itself on synthetic device stacks

def _merge(dev, stacks, x0, y0, z0, box, cosine, odd_addresses=False):
    """mi_tsv_merge on copies of ``stacks``; ``odd_addresses``: every stack and the output start one sample past a 16-byte boundary"""
    import ctypes as C
    import torch
    from ipp_amd import tsv
    dtype = stacks[0].dtype
    tdtype = torch.uint8 if dtype == np.uint8 else torch.uint16
    H, W = stacks[0].shape[1:]
    held, ptrs = [], (C.c_void_p * len(stacks))()
    pad = 1 if odd_addresses else 0
    for k, s in enumerate(stacks):
        zlo, zhi = max(int(z0[k]), box[4]), min(int(z0[k]) + s.shape[0], box[5])
        if zlo >= zhi:
            continue
        part = np.ascontiguousarray(s[zlo - int(z0[k]):zhi - int(z0[k])]).reshape(-1)
        t = torch.empty(part.size + pad, dtype=tdtype, device=dev)
        t[pad:].copy_(torch.from_numpy(part))
        held.append(t)
        ptrs[k] = t.data_ptr() + pad * dtype.itemsize
    shape = (box[5] - box[4], box[3] - box[2], box[1] - box[0])
    n = int(np.prod(shape))
    flat = torch.empty(n + pad, dtype=tdtype, device=dev)
    out = flat[pad:]
    tsv.merge_device(dev, x0, y0, z0, [s.shape[0] for s in stacks], H, W, ptrs, dtype.itemsize, cosine, tsv.VExtent(*box), out)
    return out.cpu().numpy().reshape(shape)


def _grid(rng, dtype, rows, cols, H, W, nz, overlap, top):
    x0 = np.array([c * (W - overlap) + int(rng.integers(0, 4)) for r in range(rows) for c in range(cols)])
    y0 = np.array([r * (H - overlap) + int(rng.integers(0, 4)) for r in range(rows) for c in range(cols)])
    z0 = np.array([int(rng.integers(0, 3)) for _ in range(rows * cols)])
    stacks = [rng.integers(0, top, size=(nz, H, W)).astype(dtype) for _ in range(rows * cols)]
    extent = (int(x0.min()), int(x0.max()) + W, int(y0.min()), int(y0.max()) + H, int(z0.min()), int(z0.max()) + nz)
    return stacks, x0, y0, z0, extent


# odd sizes with several cells per group row; a cell wider than one group's 2048 columns (two pieces along x) and 8-bit samples;
# four-stack corners at addresses off every vector boundary
SYNTHETIC = {
    "u16-3x2-odd": dict(dtype=np.uint16, rows=3, cols=2, H=37, W=53, nz=3, overlap=11, top=60000, odd_addresses=False),
    "u8-1x2-wide": dict(dtype=np.uint8, rows=1, cols=2, H=9, W=2301, nz=2, overlap=190, top=256, odd_addresses=False),
    "u16-2x2-odd-addresses": dict(dtype=np.uint16, rows=2, cols=2, H=33, W=47, nz=2, overlap=15, top=4000, odd_addresses=True),
    "u8-2x2-odd-addresses": dict(dtype=np.uint8, rows=2, cols=2, H=21, W=35, nz=2, overlap=9, top=256, odd_addresses=True),
}


@pytest.mark.parametrize("cosine", (False, True), ids=BLENDS)
@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_merge_entry_equals_the_restatement(dev, name, cosine):
    cfg = dict(SYNTHETIC[name])
    odd = cfg.pop("odd_addresses")
    stacks, x0, y0, z0, extent = _grid(np.random.default_rng(len(name)), **cfg)
    # the whole extent with a margin of uncovered voxels around it (odd origin, odd width)
    box = (extent[0] - 3, extent[1] + 2, extent[2] - 1, extent[3] + 4, extent[4], extent[5] + 1)
    got = _merge(dev, stacks, x0, y0, z0, box, cosine, odd)
    want = T.merge_restatement(stacks, x0, y0, z0, box, cosine)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("cosine", (False, True), ids=BLENDS)
def test_a_sample_of_65535_outside_any_overlap_stays(dev, cosine):
    """Under cosine blending 65535 is inf in float16 and the reference's cast of it is undefined; here it saturates (the departure)."""
    rng = np.random.default_rng(5)
    stacks, x0, y0, z0, extent = _grid(rng, np.uint16, 1, 2, 20, 40, 1, 8, 1000)
    z0[:] = 0
    stacks[0][0, 3, 2] = 65535      # columns 0 .. 31 of stack 0 are its own
    stacks[1][0, 7, 39] = 65535
    box = (extent[0], extent[1], extent[2], extent[3], 0, 1)
    got = _merge(dev, stacks, x0, y0, z0, box, cosine)
    assert got[0, y0[0] - extent[2] + 3, x0[0] - extent[0] + 2] == 65535
    assert got[0, y0[1] - extent[2] + 7, x0[1] - extent[0] + 39] == 65535
    assert np.array_equal(got, T.merge_restatement(stacks, x0, y0, z0, box, cosine))


def test_merge_entry_refuses_by_name(dev):
    stacks, x0, y0, z0, extent = _grid(np.random.default_rng(1), np.uint16, 1, 2, 8, 8, 1, 2, 100)
    box = (extent[0], extent[1], extent[2], extent[3], extent[4], extent[5])
    with pytest.raises(ValueError, match="same XY rectangle"):
        _merge(dev, stacks, np.array([0, 0]), np.array([0, 0]), np.array([0, 0]), (0, 8, 0, 8, 0, 1), True)
    import ctypes as C
    import torch
    from ipp_amd import tsv
    out = torch.zeros(64, dtype=torch.uint16, device=dev)
    none = (C.c_void_p * 2)()
    with pytest.raises(ValueError, match="empty box"):
        tsv.merge_device(dev, x0, y0, z0, [1, 1], 8, 8, none, 2, False, tsv.VExtent(box[0], box[0], box[2], box[3], box[4], box[5]), out)
    with pytest.raises(ValueError, match="stack 0 meets the box and has no samples"):
        tsv.merge_device(dev, x0, y0, z0, [1, 1], 8, 8, none, 2, False, tsv.VExtent(*box), out)
    with pytest.raises(ValueError, match="3 bytes per sample"):
        tsv.merge_device(dev, x0, y0, z0, [1, 1], 8, 8, none, 3, False, tsv.VExtent(*box), out)


# ---------------------------------------------------------------------------------------------------------------------------------
# the pipeline around it

def test_parallel_image_processor_on_a_tsv_volume_equals_the_folder_of_its_planes(volumes, tmp_path):
    """The per-slice pass with process_img on case A: the same slice files, down-sampled planes and npz from the TSVVolume as from a
    folder that holds the planes of its ``imread``."""
    from ipp_amd import parallel_image_processor as pip
    from ipp_amd import pystripe
    vol, full = volumes("A", "max")
    folder = tmp_path / "planes"
    folder.mkdir()
    for z, plane in enumerate(full):
        pystripe.imsave_tif(folder / f"img_{z:06}.tif", plane, None)
    common = dict(fun=pystripe.process_img, kwargs={"dark": 100}, source_voxel=(5.0, 2.0, 2.0), target_voxel=10.0)
    rc_a, down_a = pip.parallel_image_processor(vol, tmp_path / "out_tsv", return_downsampled_path=True, **common)
    rc_b, down_b = pip.parallel_image_processor(folder, tmp_path / "out_folder", return_downsampled_path=True, **common)
    assert rc_a == 0 and rc_b == 0

    def series(path):
        files = sorted(p.name for p in path.glob("*.tif"))
        return files, [pystripe.imread_tif_raw_png(path / f) for f in files]

    names_a, slices_a = series(tmp_path / "out_tsv")
    names_b, slices_b = series(tmp_path / "out_folder")
    assert names_a == names_b == [f"img_{z:06}.tif" for z in range(full.shape[0])]
    for a, b, plane in zip(slices_a, slices_b, full):
        assert a.dtype == b.dtype and np.array_equal(a, b)
        assert a.shape == plane.shape and not np.array_equal(a, plane)       # process_img took the dark level off the merged plane
    names_a, planes_a = series(down_a)
    names_b, planes_b = series(down_b)
    assert names_a == names_b and len(names_a) == 5
    for a, b in zip(planes_a, planes_b):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    with np.load(tmp_path / "out_tsv" / "out_tsv_zyx10.0um.npz", allow_pickle=True) as fa, \
            np.load(tmp_path / "out_folder" / "out_folder_zyx10.0um.npz", allow_pickle=True) as fb:
        assert fa["I"].dtype == fb["I"].dtype and np.array_equal(fa["I"], fb["I"])
        for a, b in zip(fa["xI"], fb["xI"]):
            assert np.array_equal(a, b)


def test_estimate_slice_params_on_a_tsv_volume_equals_the_stacked_array(dev, tmp_path):
    """Three slices a four-class multi-Otsu can split: a 2 x 2 grid of four-mode tiles, read through imread_device."""
    from ipp_amd import pystripe, thresholds, tsv
    from tests import thresholds_util as tu
    case = T.Case("modes", np.uint16, 2, 2, 48, 64, 8, 12, seed=31)
    rng = np.random.default_rng(31)
    case.tile = lambda r, c: np.stack([tu.four_mode_image((48, 64), seed=int(rng.integers(1 << 30))) for _ in range(8)]).astype(np.uint16)
    xml = case.write(tmp_path, lambda path, plane: pystripe.imsave_tif(path, plane, None))
    vol = tsv.TSVVolume(xml, device=dev)
    full = vol.imread(vol.volume, vol.dtype)
    want = thresholds.estimate_slice_params(full, device=dev)
    got = thresholds.estimate_slice_params(vol, device=dev)
    assert dict(got) == dict(want) and got.slices == want.slices
    assert got["bleach_correction_clip_max"] is not None


@pytest.mark.parametrize("cosine", (False, True), ids=BLENDS)
def test_command_line_writes_the_series_of_imread(volumes, projects, tmp_path, cosine):
    from ipp_amd import pystripe
    import ipp_amd
    vol, full = volumes("C", BLENDS[cosine])
    out = tmp_path / "series"
    cmd = [sys.executable, str(ipp_amd.PACKAGE_DIR) + "/tsv.py", "--projin", str(projects("C")), "--output", str(out), "--z0", "1"]
    done = subprocess.run(cmd + (["--cosine_blending"] if cosine else []), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    files = sorted(p.name for p in out.glob("*.tif"))
    assert files == [f"img_{z:06}.tif" for z in range(1, full.shape[0])]
    for z in range(1, full.shape[0]):
        assert np.array_equal(pystripe.imread_tif_raw_png(out / f"img_{z:06}.tif"), full[z])
