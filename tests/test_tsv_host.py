"""No GPU: the host half of the TSVVolume merge (ipp_amd.tsv, mi_tsv_place) -- the numpy restatement against the goldens made by the
reference's own ``TSVVolume.imread``, the placement, the XML and file bookkeeping, and every refusal."""
import ctypes as C

import numpy as np
import pytest

from tests import tsv_util as T


def _imsave(path, plane):
    from ipp_amd import pystripe
    pystripe.imsave_tif(path, plane, None)


@pytest.fixture(scope="module")
def project_c(tmp_path_factory):
    return T.CASES["C"].write(tmp_path_factory.mktemp("tsv_host"), _imsave, T.CASES["C"].stored_xml())


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_restatement_equals_the_reference(name):
    """every case, both blends, bit for bit -- case E too: the restatement computes the reference's own weight formula"""
    case = T.CASES[name]
    g = T.load_golden(case)
    stacks, x0, y0, z0, extent = T.case_stacks(case)
    assert extent == tuple(g["extent"].tolist())
    assert np.array_equal(x0.reshape(case.rows, case.cols), g["x0"]) and np.array_equal(y0.reshape(case.rows, case.cols), g["y0"])
    assert np.array_equal(z0.reshape(case.rows, case.cols), g["z0"])
    assert sorted(k for k in g if k in ("max", "cosine")) == sorted(case.blends)
    for blend in case.blends:
        got = T.merge_restatement(stacks, x0, y0, z0, extent, blend == "cosine")
        assert got.dtype == g[blend].dtype and np.array_equal(got, g[blend]), blend
        if blend == "cosine" and case.dtype == np.uint16:
            assert max(int(s.max()) for s in stacks) < 65520     # finite in float16: the goldens hold no undefined cast
    assert case.stored_xml() == case.xml()


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_placement_entry_equals_the_reference(name):
    from ipp_amd import capi
    case = T.CASES[name]
    g = T.load_golden(case)
    n = case.rows * case.cols
    north = np.array([case.north[r, c] for r in range(case.rows) for c in range(case.cols)], np.int32)
    west = np.array([case.west[r, c] for r in range(case.rows) for c in range(case.cols)], np.int32)
    nz = np.array([len(case.kept_indices(r, c)) for r in range(case.rows) for c in range(case.cols)], np.int32)
    x0, y0, z0 = (np.full(n, -7, np.int32) for _ in range(3))
    extent = (C.c_int * 6)()
    ip = C.POINTER(C.c_int)
    capi.check(capi.lib().mi_tsv_place(case.rows, case.cols, north.ctypes.data_as(ip), west.ctypes.data_as(ip), int(case.ignore_z_offsets),
                                       nz.ctypes.data_as(ip), case.height, case.width, x0.ctypes.data_as(ip), y0.ctypes.data_as(ip),
                                       z0.ctypes.data_as(ip), extent))
    assert list(extent) == g["extent"].tolist()
    for got, key in ((x0, "x0"), (y0, "y0"), (z0, "z0")):
        assert got.reshape(case.rows, case.cols).tolist() == g[key].tolist(), key


def test_volume_of_a_project(project_c):
    """construction needs no device: offsets, extent, stacks and the slice order by the integer in the name"""
    from ipp_amd import tsv
    case, g = T.CASES["C"], T.load_golden(T.CASES["C"])
    vol = tsv.TSVVolume(project_c, cosine_blending=True)
    v = vol.volume
    assert (v.x0, v.x1, v.y0, v.y1, v.z0, v.z1) == tuple(g["extent"].tolist()) and v.shape == g["max"].shape
    assert vol.dtype is np.uint8 and (vol.stack_rows, vol.stack_columns) == (2, 2)
    assert [[o.x for o in row] for row in vol.offsets] == g["x0"].tolist()
    stack = vol.stacks[1][0]
    assert [p.rsplit("/", 1)[1] for p in stack.paths] == ["t0.tif", "t50.tif", "t100.tif"]
    assert np.array_equal(stack.read_planes(0, 3), case.tile(1, 0))
    assert stack.contains(stack.intersection(v)) and vol.stacks[0][0].intersects(vol.stacks[1][1])


def test_z_ranges():
    from ipp_amd import tsv
    assert tsv.parse_z_ranges("[0,3);[4,5)") == [0, 1, 2, 4]
    assert tsv.parse_z_ranges("") == []
    assert tsv.parse_z_ranges("(1,3]") == [2, 3]     # an open start and a closed end, as the reference codes them


def test_refusals_name_the_argument(project_c, tmp_path):
    from ipp_amd import tsv
    text = T.CASES["C"].stored_xml().replace(T.PLACEHOLDER, str(project_c.parent / "tiles"))

    def project(name, changed):
        assert changed != text
        path = tmp_path / name
        path.write_text(changed)
        return path

    with pytest.raises(NotImplementedError, match="input_plugin='raw'"):
        tsv.TSVVolume(project("raw.xml", text.replace('input_plugin="tiff2D"', 'input_plugin="raw"')))
    with pytest.raises(NotImplementedError, match="TSVSimpleVolume"):
        tsv.TSVSimpleVolume(str(tmp_path), 1.0, 1.0, 1.0)
    vol = tsv.TSVVolume(project_c)
    with pytest.raises(NotImplementedError, match="make_diagnostic_img"):
        vol.make_diagnostic_img(vol.volume)
    with pytest.raises(NotImplementedError, match="dtype='uint16'"):
        vol.imread(vol.volume, np.uint16)
    with pytest.raises(NotImplementedError, match="dtype='float32'"):
        vol.imread(vol.volume, "float32")
    # a missing slice names the folder and writes nothing into it
    with pytest.raises(ValueError, match="000000_001000"):
        tsv.TSVVolume(project("missing.xml", text.replace('DIR_NAME="000000/000000_001000" Z_RANGES="[0,3)"',
                                                          'DIR_NAME="000000/000000_001000" Z_RANGES="[0,4)"'))).stacks[0][1].paths
    assert sorted(p.name for p in (project_c.parent / "tiles" / "000000" / "000000_001000").iterdir()) == ["t0.tif", "t100.tif", "t50.tif"]
    # two stacks on one XY rectangle: refused under cosine blending only
    case = T.Case("same", np.uint16, 2, 1, 16, 16, 1, 4, seed=4)
    case.north[1, 0] = (0, 0, 0)
    same = case.write(tmp_path / "same", _imsave)
    assert tsv.TSVVolume(same).volume.shape == (1, 16, 16)
    with pytest.raises(ValueError, match="cosine_blending=True.*same XY rectangle"):
        tsv.TSVVolume(same, cosine_blending=True)


def test_refused_sample_types_and_shapes(tmp_path):
    from ipp_amd import tsv
    case = T.Case("f32", np.uint16, 1, 2, 16, 16, 1, 4, seed=3)
    real_tile = case.tile
    case.tile = lambda r, c: real_tile(r, c).astype(np.float32)
    with pytest.raises(NotImplementedError, match="dtype='float32"):
        tsv.TSVVolume(case.write(tmp_path / "f32", _imsave))
    case.tile = lambda r, c: real_tile(r, c)[:, :, :16 - c]
    with pytest.raises(ValueError, match=r"stack \[0,1\]"):
        tsv.TSVVolume(case.write(tmp_path / "shapes", _imsave))
    case.tile = lambda r, c: real_tile(r, c).astype(np.uint8 if c else np.uint16)
    with pytest.raises(ValueError, match=r"stack \[0,1\]"):
        tsv.TSVVolume(case.write(tmp_path / "types", _imsave))


def test_only_this_volume_is_a_source():
    """any other class that is merely named TSVVolume stays refused by the per-slice pass"""
    from ipp_amd import parallel_image_processor as pip
    from ipp_amd import tsv

    class TSVVolume:
        pass
    with pytest.raises(NotImplementedError, match="TSVVolume"):
        pip._refuse_source(TSVVolume())
    assert pip._refuse_source(object.__new__(tsv.TSVVolume)) is None
