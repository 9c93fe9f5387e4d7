"""GPU: the acquisition driver (ipp_amd.acquisition.main) on the synthetic acquisition of tests/acquisition_util.py: three channels of a
3 x 3 grid of 128 x 128 x 16 tiles.  Every test makes one ``main([...])`` call; the products must equal what the stages give when they are
called by hand with arguments spelled out here."""
import shutil
import xml.etree.ElementTree as ET
from argparse import Namespace
from pathlib import Path

import numpy as np
import pytest

from ipp_amd import acquisition as A
from tests import acquisition_util as U
from tests.channel_align_util import read_tiff
from tests.test_gpu_terastitcher_golden import compare

pytestmark = pytest.mark.gpu
ONE, TWO, THREE = U.CHANNELS


@pytest.fixture(scope="module")
def acquisition(tmp_path_factory):
    """the acquisition, written once and only read: (folder, jy, jx)"""
    root = tmp_path_factory.mktemp("acquisition") / "brain"
    jy, jx = U.write_acquisition(root)
    return root, jy, jx


def folders(tmp_path):
    made = [tmp_path / name for name in ("tmp", "out", "rgb")]
    for folder in made:
        folder.mkdir()
    return made


def argv_of(acq, tmp, out, *more):
    return ["--objective", "15x", "--input", str(acq), "--tmptif", str(tmp), "--stitched", str(out), "--skipconf", "--tile_size", "128",
            "128", "--bleach_wavelet", "db9", *more]


def tree(root):
    """{relative path: (modification time in ns, size)} of every file under ``root``"""
    return {str(f.relative_to(root)): (f.stat().st_mtime_ns, f.stat().st_size) for f in sorted(Path(root).rglob("*")) if f.is_file()}


def read(path):
    from ipp_amd import pystripe
    img = pystripe.imread_tif_raw_png(path)
    assert img is not None, path
    return img


def same_series(got_dir, want_dir, dtype=None):
    got, want = sorted(f.name for f in Path(got_dir).iterdir()), sorted(f.name for f in Path(want_dir).iterdir())
    assert got == want and got, (got_dir, want_dir)
    for name in got:
        g, w = read(Path(got_dir) / name), read(Path(want_dir) / name)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (got_dir, name)
        assert dtype is None or g.dtype == dtype
    return len(got)


def pages(path):
    from PIL import Image, ImageSequence
    with Image.open(path) as im:
        return np.stack([np.array(page) for page in ImageSequence.Iterator(im)])


def placement(path):
    """{(row, col): (ABS_V, ABS_H, ABS_D)} of a project file"""
    return {(int(s.get("ROW")), int(s.get("COL"))): tuple(int(s.get(k)) for k in ("ABS_V", "ABS_H", "ABS_D"))
            for s in ET.parse(path).getroot().find("STACKS")}


def by_hand_channel(dev, acq, channel, work, planes_dtype):
    """One channel through the stages, every argument spelled out: -> (tiles, step-5 project, slices, down-sampled planes)."""
    from ipp_amd import process_images, pystripe, thresholds
    from ipp_amd.parallel_image_processor import parallel_image_processor
    from ipp_amd.tsv import TSVVolume
    tiles = work / "tiles" / channel
    assert pystripe.batch_filter(acq / channel, tiles, gaussian_filter_2d=True, sigma=(250, 250), level=0, wavelet="db9", crossover=10,
                                 threshold=None, padding_mode="reflect", bidirectional=True, bleach_correction_frequency=None,
                                 bleach_correction_max_method=False, lightsheet=False, down_sample=None, tile_size=(128, 128), new_size=None,
                                 d_type="uint16", convert_to_8bit=False, bit_shift_to_right=8, compression=("ADOBE_DEFLATE", 1)) == 0
    x = [work / f"{channel}_step_{k}.xml" for k in (1, 2, 3, 4, 5)]
    assert process_images.main(["-1", "--ref1=H", "--ref2=V", "--ref3=D", "--vxl1=0.410", "--vxl2=0.410", "--vxl3=2.0", "--sparse_data",
                                f"--volin={tiles}", f"--projout={x[0]}", "--noprogressbar"]) == 0
    for k in (2, 3, 4, 5):
        assert process_images.main([f"-{k}", "--sD=10", "--subvoldim=16", "--threshold=0.65", f"--projin={x[k - 2]}", f"--projout={x[k - 1]}"]) == 0
    volume = TSVVolume(x[4], alt_stack_dir=str(tiles), cosine_blending=False)
    found = thresholds.estimate_slice_params(volume, need_bleach_correction=True, need_16bit_to_8bit_conversion=True)
    slices = work / f"{channel}_tif"
    slices.mkdir()
    (work / "Downsampled").mkdir(exist_ok=True)
    rc, planes = parallel_image_processor(
        source=volume, destination=slices, fun=pystripe.process_img,
        kwargs=dict(sigma=(256, 256), wavelet="db9", padding_mode="wrap", gpu_semaphore=None, bidirectional=True,
                    threshold=found["bleach_correction_clip_med"], bleach_correction_frequency=None,
                    bleach_correction_clip_min=found["bleach_correction_clip_min"], bleach_correction_clip_med=found["bleach_correction_clip_med"],
                    bleach_correction_clip_max=found["bleach_correction_clip_max"], bleach_correction_max_method=False, dark=found["dark"],
                    lightsheet=False, percentile=0.25, rotate=0, convert_to_8bit=True, bit_shift_to_right=found["bit_shift_to_right"],
                    tile_size=tuple(volume.volume.shape[1:3]), d_type=volume.dtype, extended=True),
        source_voxel=(2.0, 0.41, 0.41), target_voxel=10, downsampled_path=work / "Downsampled", rotation=90,
        compression=("ADOBE_DEFLATE", 1), resume=True, return_downsampled_path=True, down_sampled_dtype=planes_dtype)
    assert rc == 0
    return tiles, x[4], slices, planes


def test_whole_run(dev, acquisition, tmp_path, capsys):
    """Three channels, ``--terafly_channels Ex_561_Em_600 --composite``, defaults otherwise.  Integer images and the ``I`` of the npz are
    compared exactly (the stages are deterministic; their own GPU tests compare exactly too); the project files through
    ``tests.test_gpu_terastitcher_golden.compare``: integers exact, peaks and reliabilities at rel 2e-5 / abs 2e-6.  Two arguments of the
    by-hand calls are not the reference's: the planes' ``down_sampled_dtype="uint16"`` (``align_images`` refuses float32 planes) and
    TeraFly levels "0123" (16 slices hold no more)."""
    from ipp_amd import align_images, terafly
    acq, jy, jx = acquisition
    tmp, out, rgb = folders(tmp_path)
    assert A.main(argv_of(acq, tmp, out, "--terafly_channels", TWO, "--composite", str(rgb))) == 0
    pre, stitched, composite = tmp / "brain_tif", out / "brain_stitched", rgb / "brain_composite"
    text = capsys.readouterr().out
    assert "stitching started" in text and "--nthreads" in text and "accepted and ignored" in text and "done." in text
    log = (stitched / "log.txt").read_text()
    assert "stitching started" in log and f"Channels: {list(U.CHANNELS)}" in log and "--enable_axis_correction=False: accepted and ignored" in log
    assert log.index(f"{TWO}: started preprocessing") < log.index(f"{ONE}: started preprocessing") < log.index(f"{THREE}: started preprocessing")

    hand = tmp_path / "hand"
    hand.mkdir()
    want_yx = {(r, c): (r * U.STEP + int(jy[r, c]), c * U.STEP + int(jx[r, c])) for r in range(U.GRID) for c in range(U.GRID)}
    shapes = []
    for channel in U.CHANNELS:
        tiles, x5, slices, planes = by_hand_channel(dev, acq, channel, hand, "uint16")   # (--composite: integer planes)
        # the preprocessed tiles
        got_tiles = sorted(str(f.relative_to(pre / channel)) for f in (pre / channel).rglob("*.tif"))
        assert got_tiles == sorted(str(f.relative_to(tiles)) for f in tiles.rglob("*.tif")) and len(got_tiles) == 9 * U.SLICES
        for rel in got_tiles:
            g, w = read(pre / channel / rel), read(tiles / rel)
            assert g.dtype == np.uint16 and g.shape == (128, 128) and np.array_equal(g, w), (channel, rel)
        # the step-5 project, the only one left; the placements recover the jitter to the pixel
        mine = stitched / f"{channel}_xml_import_step_5.xml"
        assert sorted(f.name for f in stitched.glob(f"{channel}_xml_import_step_*.xml")) == [mine.name]
        assert compare(mine, x5, f"{channel} step 5") > 0
        placed = placement(mine)
        assert placed == placement(x5)
        v0, h0, d0 = placed[(0, 0)]
        assert {k: (v - v0, h - h0) for k, (v, h, _) in placed.items()} == want_yx, channel
        assert {d for _, _, d in placed.values()} == {d0}
        # the stitched slices, the down-sampled planes and the npz
        assert same_series(stitched / f"{channel}_tif", slices, np.uint8) == U.SLICES
        down = stitched / "Downsampled" / f"{channel}_tif_z10.0_yx10.0um"
        assert planes == hand / "Downsampled" / down.name and same_series(down, planes, np.uint16) == 4
        got, want = (np.load(d / f"{channel}_tif_zyx10.0um.npz", allow_pickle=True) for d in (stitched / "Downsampled", hand / "Downsampled"))
        assert got["I"].dtype == want["I"].dtype and got["I"].shape == want["I"].shape == (3, 13, 13) and np.array_equal(got["I"], want["I"])
        assert all(np.array_equal(a, b) for a, b in zip(got["xI"], want["xI"]))
        shapes.append(read(stitched / f"{channel}_tif" / "img_000000.tif").shape)
    assert len(set(shapes)) == 1   # (rotated, and the extent depends on the jitter: only equality is asked)

    # TeraFly: only the chosen channel, the file list and every page
    assert sorted(f.name for f in stitched.glob("*_TeraFly")) == [f"{TWO}_TeraFly"]
    hand_tf = hand / "terafly"
    hand_tf.mkdir()
    with pytest.raises(ValueError, match="level 5"):                                         # the reference's six levels: refused at 16 slices
        terafly.convert(hand / f"{TWO}_tif", hand_tf, resolutions="012345", halve="mean")
    # level k needs 2^k slices in half the block depth: 2^k <= 16 // 2, so levels 0 .. 3 of the six
    assert A.terafly_resolutions((U.SLICES, 320, 320)) == "0123" and A.terafly_resolutions((64, 320, 320)) == "012345"
    terafly.convert(hand / f"{TWO}_tif", hand_tf, resolutions="0123", halve="mean")
    assert "resolutions: 0123 (of 012345" in log
    got_tf, want_tf = tree(stitched / f"{TWO}_TeraFly"), tree(hand_tf)
    assert sorted(got_tf) == sorted(want_tf) and any(name.endswith(".tif") for name in got_tf)
    for rel in got_tf:
        if rel.endswith(".tif"):
            assert np.array_equal(pages(stitched / f"{TWO}_TeraFly" / rel), pages(hand_tf / rel)), rel
        else:
            assert (stitched / f"{TWO}_TeraFly" / rel).read_bytes() == (hand_tf / rel).read_bytes(), rel

    # the composite: the reference channel (the first found) as red, every stitched folder with its own down-sampled folder
    def pair(channel):
        return stitched / f"{channel}_tif", stitched / "Downsampled" / f"{channel}_tif_z10.0_yx10.0um"
    hand_rgb = hand / "composite"
    align_images.main(Namespace(red=pair(ONE), green=pair(TWO), blue=pair(THREE), output=hand_rgb, write_alignments=True, generate_ims=False,
                                max_iterations=10, reference="red", num_threads=8, save_singles=False, dtype="uint32", dx=(0.41, 0.41),
                                dy=(0.41, 0.41), dz=(2.0, 2.0)))
    assert (composite / "alignments.txt").read_text() == (hand_rgb / "alignments.txt").read_text()
    for series in ("original/RGB", "downsampled/RGB"):
        got_files, want_files = sorted((composite / series).iterdir()), sorted((hand_rgb / series).iterdir())
        assert [f.name for f in got_files] == [f.name for f in want_files] and got_files, series
        for g, w in zip(got_files, want_files):
            (g_img, _), (w_img, _) = read_tiff(g), read_tiff(w)
            assert g_img.dtype == w_img.dtype and g_img.shape == w_img.shape and g_img.shape[-1] == 3 and np.array_equal(g_img, w_img), (series, g.name)
    assert len(list((composite / "original/RGB").iterdir())) == U.SLICES


def test_resume_rewrites_nothing(dev, acquisition, tmp_path):
    """A second identical call returns 0 and leaves every tile, project, slice, plane and npz as it is (modification times and sizes)."""
    acq, _, _ = acquisition
    tmp, out, _ = folders(tmp_path)
    argv = argv_of(acq, tmp, out)
    assert A.main(argv) == 0
    keep = lambda root: {k: v for k, v in tree(root).items() if not k.endswith("log.txt")}
    before_tiles, before_out = tree(tmp), keep(out)
    assert len(before_tiles) == 3 * 9 * U.SLICES
    for channel in U.CHANNELS:
        assert f"brain_stitched/{channel}_xml_import_step_5.xml" in before_out
        assert sum(k.startswith(f"brain_stitched/{channel}_tif/") for k in before_out) == U.SLICES
        assert f"brain_stitched/Downsampled/{channel}_tif_zyx10.0um.npz" in before_out
    assert A.main(argv) == 0
    assert tree(tmp) == before_tiles and keep(out) == before_out


def test_shared_alignment(dev, acquisition, tmp_path):
    """--stitch_based_on_reference_channel_alignment: only the reference channel has project files, and all three stitched volumes have
    its shape."""
    acq, _, _ = acquisition
    tmp, out, _ = folders(tmp_path)
    assert A.main(argv_of(acq, tmp, out, "--stitch_based_on_reference_channel_alignment", "--reference_channel", TWO)) == 0
    stitched = out / "brain_stitched"
    assert sorted(f.name for f in stitched.glob("*.xml")) == [f"{TWO}_xml_import_step_5.xml"]
    log = (stitched / "log.txt").read_text()
    assert log.count("aligning tiles") == 1 and f"{TWO}: aligning tiles" in log
    shapes = set()
    for channel in U.CHANNELS:
        files = sorted((stitched / f"{channel}_tif").iterdir())
        assert len(files) == U.SLICES
        shapes.add(read(files[0]).shape + (read(files[0]).dtype.name,))
    assert len(shapes) == 1
    # the other channels were merged from their own tiles: the slices differ
    assert not np.array_equal(read(stitched / f"{ONE}_tif" / "img_000008.tif"), read(stitched / f"{TWO}_tif" / "img_000008.tif"))


def test_missing_tile(dev, acquisition, tmp_path, capsys):
    """One tile file deleted: the inspection warns, the preprocessed folder holds a zero tile of --tile_size and uint16 in its place, and
    the run completes."""
    acq, _, _ = acquisition
    tmp, out, _ = folders(tmp_path)
    copy = tmp_path / "copy" / "brain"
    shutil.copytree(acq, copy)
    gone = Path(U.tile_dir(copy, ONE, 1, 2)) / U.z_name(5)
    gone.unlink()
    assert A.main(argv_of(copy, tmp, out)) == 0
    text = capsys.readouterr().out
    assert "warning: following folders might have missing tiles:" in text and f"folders having {U.SLICES - 1} tiles" in text
    assert str(gone.parent) in text
    made = tmp / "brain_tif" / gone.relative_to(copy)
    tile = read(made)
    assert tile.dtype == np.uint16 and tile.shape == (128, 128) and not tile.any()
    assert read(made.with_name(U.z_name(4))).any()
    assert len(list((out / "brain_stitched" / f"{ONE}_tif").iterdir())) == U.SLICES
