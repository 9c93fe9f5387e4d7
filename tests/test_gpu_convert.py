"""GPU: ``ipp_amd.convert`` end to end on six 40 x 56 uint16 slices -- the processed series equals ``process_img`` on every slice with
``build_kwargs``' dictionary, then the rotation; ``--teraFly`` equals a direct ``terafly.convert`` of the written series (on a series
large enough for six resolutions); ``--resume`` rewrites nothing; a project ``.xml`` as input gives the planes of its ``TSVVolume``."""
import os

import numpy as np
import pytest

from tests import thresholds_util as T
from tests import tsv_util

pytestmark = pytest.mark.gpu

ARGV = ["--bleach-correction", "--bleach-correction-period", "40", "--bleach-correction-clip-min", "3", "--bleach-correction-clip-max", "9",
        "--downsample-x", "2", "--downsample-y", "2", "--downsample-method", "median", "--convert-to-8bit", "--bit-shift", "4", "--rotation", "90"]


@pytest.fixture(scope="module")
def series(dev, tmp_path_factory):
    """(convert module, source folder, the six slices, output folder of the processed series)"""
    from ipp_amd import convert, pystripe
    root = tmp_path_factory.mktemp("convert")
    src, out = root / "slices", root / "out"
    src.mkdir()
    slices = [T.four_mode_image((40, 56), 60 + z) for z in range(6)]
    for z, img in enumerate(slices):
        pystripe.imsave_tif(src / f"slice_{z:03d}.tif", img)
    assert convert.main(convert.parse_args(["--input", str(src), "--tif", str(out)] + ARGV)) is None
    return convert, src, slices, out


def tree(folder):
    return {os.path.relpath(os.path.join(d, f), folder): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(folder) for f in fs}


def test_every_slice_equals_process_img_then_the_rotation(series, dev):
    from ipp_amd import pystripe
    convert, src, slices, out = series
    process, pip = convert.build_kwargs(convert.parse_args(["--input", str(src), "--tif", str(out)] + ARGV))
    assert process["bleach_correction_clip_min"] == 3.0 and "bleach_correction_clip_med" not in process and pip["rotation"] == 90
    assert sorted(p.name for p in out.iterdir()) == [f"slice_{z:03d}.tif" for z in range(6)]
    for z, img in enumerate(slices):
        want = np.rot90(pystripe.process_img(img.copy(), device=dev, extended=True, **process), 1)
        got = pystripe.imread_tif_raw_png(out / f"slice_{z:03d}.tif")
        assert got.dtype == np.uint8 and got.shape == (28, 20) and np.array_equal(got, want), z
    assert len({pystripe.imread_tif_raw_png(p).tobytes() for p in out.iterdir()}) == 6 and got.any()


def test_resume_rewrites_nothing(series):
    convert, src, slices, out = series
    before = {p.name: (p.stat().st_mtime_ns, p.read_bytes()) for p in out.iterdir()}
    (out / "slice_002.tif").unlink()
    convert.main(convert.parse_args(["--input", str(src), "--tif", str(out), "--resume"] + ARGV))
    after = {p.name: (p.stat().st_mtime_ns, p.read_bytes()) for p in out.iterdir()}
    assert sorted(after) == sorted(before)
    for name in before:
        assert after[name][1] == before[name][1]
        assert (after[name][0] == before[name][0]) == (name != "slice_002.tif"), name


def test_terafly_of_the_result_equals_a_direct_conversion(series, tmp_path):
    """TeraFly with six resolutions needs planes of 250 samples a side and 64 slices (VolumeConverter's limits, which
    ``terafly.plan`` keeps), so the 28 x 20 x 6 result above is refused -- by ``convert`` with the words of the direct call -- and the
    comparison runs on 64 slices of 502 x 526 through the same options: 263 x 251 x 64."""
    from ipp_amd import pystripe, terafly
    convert, src, slices, out = series
    with pytest.raises(ValueError, match="minimum dimension for block height and width is 250") as direct_error:
        terafly.convert(out, tmp_path, resolutions="012345", halve="mean")
    with pytest.raises(ValueError) as convert_error:
        convert.main(convert.parse_args(["--input", str(out), "--teraFly", str(tmp_path / "small")]))
    assert str(convert_error.value) == str(direct_error.value)
    big = tmp_path / "big"
    big.mkdir()
    base = T.four_mode_image((502, 526), 70)
    for z in range(64):
        pystripe.imsave_tif(big / f"slice_{z:03d}.tif", np.roll(base, 7 * z, axis=1), None)
    plan = convert.main(convert.parse_args(["--input", str(big), "--tif", str(tmp_path / "tif"), "--teraFly", str(tmp_path / "fly")] + ARGV))
    (tmp_path / "direct").mkdir()
    direct = terafly.convert(tmp_path / "tif", tmp_path / "direct", resolutions="012345", halve="mean")
    a, b = tree(tmp_path / "fly"), tree(tmp_path / "direct")
    assert sorted(a) == sorted(b) == terafly.output_files(direct) and len(a) > 6
    assert all(a[k] == b[k] for k in a)
    assert (plan.height, plan.width, plan.depth) == (direct.height, direct.width, direct.depth) == (263, 251, 64)
    # the series alone, a plain folder with nothing to do, goes straight to the same tree
    convert.main(convert.parse_args(["--input", str(tmp_path / "tif"), "--teraFly", str(tmp_path / "fly2")]))
    assert tree(tmp_path / "fly2") == a


def test_project_xml_gives_the_planes_of_its_volume(series, dev, tmp_path):
    from ipp_amd import pystripe, tsv
    convert = series[0]
    case = tsv_util.CASES["A"]
    xml = case.write(tmp_path / "project", lambda path, plane: pystripe.imsave_tif(path, plane, None), case.stored_xml())
    vol = tsv.TSVVolume(str(xml), device=dev)
    full = vol.imread(vol.volume, vol.dtype)
    convert.main(convert.parse_args(["--input", str(xml), "--tif", str(tmp_path / "planes")]))
    files = sorted(p.name for p in (tmp_path / "planes").glob("*.tif"))
    assert files == [f"img_{z:06}.tif" for z in range(full.shape[0])]
    for z in range(full.shape[0]):
        assert np.array_equal(pystripe.imread_tif_raw_png(tmp_path / "planes" / f"img_{z:06}.tif"), full[z])
