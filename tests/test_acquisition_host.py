"""CPU: the host half of the acquisition driver (ipp_amd.acquisition): the parser against a table written out here, and the decisions of
``plan()`` on folders of empty files against values worked out by hand from the rules of the reference's process_images.py."""
import argparse
import sys
from argparse import Namespace
from pathlib import Path

import pytest

from ipp_amd import acquisition as A
from tests import acquisition_util as U

FLAG = argparse.BooleanOptionalAction
# dest -> (option strings, default, choices or None, is a --x / --no-x flag)
PARSER_TABLE = {
    "objective": (["--objective"], None, ["15x", "9x", "8x", "4x", "40x"], False),
    "input": (["--input", "-i"], None, None, False),
    "tmptif": (["--tmptif", "-t"], None, None, False),
    "stitched": (["--stitched", "-s"], None, None, False),
    "composite": (["--composite"], None, None, False),
    "reference_channel": (["--reference_channel"], "", None, False),
    "stitch_based_on_reference_channel_alignment": (["--stitch_based_on_reference_channel_alignment"], False, None, True),
    "imaris": (["--imaris", "-o"], None, None, False),
    "terafly_channels": (["--terafly_channels", "-f"], [], None, False),
    "terafly_path": (["--terafly_path"], "", None, False),
    "nthreads": (["--nthreads", "-n"], "ANY", None, False),
    "stitch_mip": (["--stitch_mip"], False, None, True),
    "need_raw_png_to_tiff_conversion": (["--need_raw_png_to_tiff_conversion"], True, None, True),
    "gaussian": (["--gaussian", "-g"], True, None, True),
    "de_stripe": (["--de_stripe"], True, None, True),
    "padding_mode": (["--padding_mode"], "wrap", ["constant", "edge", "linear_ramp", "maximum", "mean", "median", "minimum", "reflect",
                                                  "symmetric", "wrap", "empty"], False),
    "isotropic": (["--isotropic"], False, None, True),
    "bleach_correction": (["--bleach_correction"], True, None, True),
    "bleach_correction_channels": (["--bleach_correction_channels"], [], None, False),
    "background_subtraction": (["--background_subtraction"], False, None, True),
    "background_subtraction_channels": (["--background_subtraction_channels"], [], None, False),
    "convert_to_8bit": (["--convert_to_8bit"], True, None, True),
    "rot90": (["--rot90"], True, None, True),
    "compression_method": (["--compression_method", "-zm"], "ADOBE_DEFLATE", ["ADOBE_DEFLATE", "LZW", "PackBits"], False),
    "compression_level": (["--compression_level", "-zl"], 1, list(range(10)), False),
    "voxel_size_target": (["--voxel_size_target", "-dt"], 10, None, False),
    "resume": (["--resume"], True, None, True),
    "timeout": (["--timeout"], None, None, False),
    "skipconf": (["--skipconf"], False, None, True),
    "skip_inspection": (["--skip_inspection"], False, None, True),
    "exclude_gpus": (["--exclude_gpus"], [], None, False),
    "vram_mem_fraction_gpu0": (["--vram_mem_fraction_gpu0"], 1.0, None, False),
    "enable_axis_correction": (["--enable_axis_correction"], False, None, True),
    "cosine_blending": (["--cosine_blending"], False, None, True),
    # without a counterpart in the reference
    "tile_size": (["--tile_size"], None, None, False),
    "voxel_size_z": (["--voxel_size_z"], None, None, False),
    "bleach_wavelet": (["--bleach_wavelet"], "coif15", None, False),
}
REQUIRED = {"objective", "input", "tmptif", "stitched"}


def test_parser_names_defaults_and_choices():
    actions = {a.dest: a for a in A.build_parser()._actions if a.dest != "help"}
    assert set(actions) == set(PARSER_TABLE)
    for dest, (strings, default, choices, is_flag) in PARSER_TABLE.items():
        a = actions[dest]
        want = strings + ([f"--no-{strings[0][2:]}"] if is_flag else [])
        assert sorted(a.option_strings) == sorted(want), dest
        if default != "ANY":
            assert a.default == default and type(a.default) is type(default), dest
        assert (None if a.choices is None else list(a.choices)) == choices, dest
        assert isinstance(a, FLAG) == is_flag, dest
        assert a.required == (dest in REQUIRED), dest
    assert actions["nthreads"].type is int and actions["nthreads"].default >= 1
    assert actions["tile_size"].nargs == 2 and actions["tile_size"].type is int
    for dest in ("terafly_channels", "bleach_correction_channels", "background_subtraction_channels", "exclude_gpus"):
        assert actions[dest].nargs == "+", dest
    with pytest.raises(SystemExit):
        A.build_parser().parse_args(["--objective", "10x", "-i", "a", "-t", "b", "-s", "c"])     # in the table, not among the choices


@pytest.fixture
def roots(tmp_path):
    for name in ("tmp", "out", "rgb", "tf"):
        (tmp_path / name).mkdir()
    return tmp_path


def untouched(roots, *names):
    return all(not list((roots / n).iterdir()) for n in names)


def parse(roots, acq, *more, objective="15x"):
    return A.build_parser().parse_args(["--objective", objective, "-i", str(acq), "-t", str(roots / "tmp"), "-s", str(roots / "out"),
                                        "--bleach_wavelet", "db9", *more])


def make(roots, channels=U.CHANNELS[:1], name="acq", **kw):
    acq = roots / name
    U.write_empty_acquisition(acq, channels, **kw)
    return acq


@pytest.mark.parametrize("objective, voxel, tile", [("4x", 1.809, (1600, 2000)), ("8x", 0.82, (2000, 2000)), ("9x", 0.72, (2000, 2000)),
                                                     ("15x", 0.41, (2000, 2000)), ("40x", 0.14, (2048, 2048))])
def test_every_objective(roots, objective, voxel, tile):
    acq = make(roots, z_step=8)
    p = A.plan(parse(roots, acq, objective=objective))
    assert (p.voxel_size_x, p.voxel_size_y, p.voxel_size_z, p.tile_size) == (voxel, voxel, 0.8, tile)
    assert (p.down_sampling_factor, p.new_tile_size) == (None, None)
    q = A.plan(parse(roots, acq, "--tile_size", "100", "120", "--voxel_size_z", "1.5", objective=objective))
    assert (q.tile_size, q.voxel_size_z) == ((100, 120), 1.5)
    assert A.OBJECTIVES["10x"] == (0.62, 0.62, (2000, 2000))


def test_z_step_from_names_and_without_a_terminal(roots, monkeypatch):
    assert A.plan(parse(roots, make(roots, z_step=20))).voxel_size_z == 2.0
    named = roots / "named"
    U.write_empty_acquisition(named, U.CHANNELS[:1], name="img_{z:06d}")                     # stems that are no integers
    monkeypatch.setattr(sys, "stdin", open("/dev/null"))
    with pytest.raises(RuntimeError, match="--voxel_size_z"):
        A.plan(parse(roots, named))
    assert A.plan(parse(roots, named, "--voxel_size_z", "0.8")).voxel_size_z == 0.8
    single = roots / "single"
    U.write_empty_acquisition(single, U.CHANNELS[:1], slices=1)                              # one file per stack: no difference to take
    with pytest.raises(RuntimeError, match="--voxel_size_z"):
        A.plan(parse(roots, single))


def test_isotropic_branches(roots):
    acq = make(roots, z_step=20)
    # z = 2.0 coarser than 0.41: the tiles shrink; 128 * 0.41 / 2 = 26.24 -> 26, factor = 2.0 // 0.41 = 4
    p = A.plan(parse(roots, acq, "--isotropic", "--tile_size", "128", "128"))
    assert (p.down_sampling_factor, p.new_tile_size) == ((4, 4), (26, 26))
    assert (p.voxel_size_x, p.voxel_size_y, p.voxel_size_z) == (2.0, 2.0, 2.0)
    b = p.channels[0].batch_filter
    assert (b["down_sample"], b["new_size"], b["tile_size"]) == ((4, 4), (26, 26), (128, 128))
    assert p.channels[0].bleach_sigma == (52, 52)
    assert p.channels[0].steps[0][4:7] == ["--vxl1=2.000", "--vxl2=2.000", "--vxl3=2.0"]
    ns = p.align_namespace(["a", "b"], ["c", "d"])
    assert (ns.dx, ns.dy, ns.dz) == ((2.0, 8.0), (2.0, 8.0), (2.0, 2.0))
    # the same without --isotropic: nothing changes
    p = A.plan(parse(roots, acq, "--tile_size", "128", "128"))
    assert (p.down_sampling_factor, p.new_tile_size, p.voxel_size_x) == (None, None, 0.41)
    assert p.channels[0].bleach_sigma == (256, 256)
    # z = 0.6 coarser than 0.41 but less than twice: factor (1, 1) -> None, the resize stays: 2000 * 0.41 / 0.6 = 1366.67 -> 1367
    p = A.plan(parse(roots, acq, "--isotropic", "--voxel_size_z", "0.6"))
    assert (p.down_sampling_factor, p.new_tile_size, p.voxel_size_x) == (None, (1367, 1367), 0.6)
    assert p.channels[0].preprocess and p.channels[0].batch_filter["new_size"] == (1367, 1367)
    # z = 0.2 finer than 0.41: the tiles grow, 2000 * 0.41 / 0.2 = 4100, no factor
    p = A.plan(parse(roots, acq, "--isotropic", "--voxel_size_z", "0.2"))
    assert (p.down_sampling_factor, p.new_tile_size, p.voxel_size_y) == (None, (4100, 4100), 0.2)
    # z equal: nothing, and the warning
    p = A.plan(parse(roots, acq, "--isotropic", "--voxel_size_z", "0.41"))
    assert (p.down_sampling_factor, p.new_tile_size) == (None, None)
    assert any("make sure voxel sizes are really equal" in n for n in p.notes)
    # the asserts on the target voxel size
    with pytest.raises(AssertionError):
        A.plan(parse(roots, acq, "--voxel_size_target", "1.5"))                              # z = 2.0 is not below it
    with pytest.raises(AssertionError):
        A.plan(parse(roots, acq, "--voxel_size_target", "0.5", "--voxel_size_z", "0.3"))     # the target itself below 1


def test_select_channels_and_reorderings(roots):
    acq = make(roots, U.CHANNELS)
    one, two, three = U.CHANNELS
    p = A.plan(parse(roots, acq))
    assert p.all_channels == list(U.CHANNELS) == p.order and p.reference_channel == one
    assert p.bleach_correction_channels == list(U.CHANNELS) and p.background_subtraction_channels == [] and p.terafly_channels == []
    assert p.channel_colors == {one: "b", two: "g", three: "r"} and p.order_of_colors() == "bgr"
    p = A.plan(parse(roots, acq, "--bleach_correction_channels", three, "--background_subtraction", "--background_subtraction_channels",
                     two, one, "--terafly_channels", three, two))
    assert p.bleach_correction_channels == [three] and p.background_subtraction_channels == [two, one]
    assert p.order == [three, two, one]                                                      # TeraFly channels first, as given
    assert [c.channel for c in p.channels] == p.order and [c.terafly is not None for c in p.channels] == [True, True, False]
    assert [(c.need_bleach_correction, c.need_lightsheet_cleaning) for c in p.channels] == [(True, False), (False, True), (False, True)]
    assert [c.bleach_sigma for c in p.channels] == [(4000, 4000), (0, 0), (0, 0)]
    # --background_subtraction_channels without --background_subtraction selects nothing
    assert A.plan(parse(roots, acq, "--background_subtraction_channels", two)).background_subtraction_channels == []
    # then the reference channel, when alignments are shared
    p = A.plan(parse(roots, acq, "--terafly_channels", three, "--stitch_based_on_reference_channel_alignment", "--reference_channel", two))
    assert p.order == [two, three, one] and p.order_of_colors() == "grb"
    assert {c.channel_for_alignment for c in p.channels} == {two}
    p = A.plan(parse(roots, acq, "--terafly_channels", three, "--reference_channel", two))
    assert p.order == [three, one, two] and [c.channel_for_alignment for c in p.channels] == p.order
    for option, word in (("--bleach_correction_channels", "bleach correction"), ("--terafly_channels", "terafly conversion")):
        with pytest.raises(RuntimeError, match=f"{word} channel Ex_000 is not among"):
            A.plan(parse(roots, acq, option, "Ex_000"))
    with pytest.raises(RuntimeError, match="--reference_channel should be among"):
        A.plan(parse(roots, acq, "--reference_channel", "Ex_000"))
    # a single channel: it is selected whatever is named, and its name is not checked
    p = A.plan(parse(roots, make(roots, name="solo"), "--terafly_channels", "Ex_000", "--composite", str(roots / "rgb")))
    assert p.terafly_channels == [one] and not p.need_composite_image and p.composite_path == roots / "tmp"


def test_mip_discovery_and_paths(roots):
    acq = roots / "brain"
    one, two, _ = U.CHANNELS
    U.write_empty_acquisition(acq, [one, two, "Ex_999_Em_1"], z_step=20)
    U.write_empty_acquisition(acq, [one + "_MIP", "Ex_642_Ch2_MIP"], z_step=4000)
    p = A.plan(parse(roots, acq, "--composite", str(roots / "rgb"), "--terafly_channels", two, "--terafly_path", str(roots / "tf")))
    assert p.all_channels == [one, two]
    assert p.preprocessed_path == roots / "tmp" / "brain_tif" and p.stitched_path == roots / "out" / "brain_stitched"
    assert p.composite_path == roots / "rgb" / "brain_composite" and p.need_composite_image
    assert p.downsampled_path == roots / "out" / "brain_stitched" / "Downsampled"
    assert p.log_file == roots / "out" / "brain_stitched" / "log.txt" and p.terafly_path == roots / "tf"
    assert p.mkdirs() == [p.preprocessed_path, p.stitched_path, p.composite_path, p.downsampled_path]
    c = p.channels[0]
    assert c.channel == two and c.stitched_tif_path == p.stitched_path / f"{two}_tif"
    assert c.terafly == dict(src=c.stitched_tif_path, dst=roots / "tf" / f"{two}_TeraFly", resolutions="012345", halve="mean")
    assert c.batch_filter["input_path"] == acq / two and c.batch_filter["output_path"] == p.preprocessed_path / two
    assert c.projects == [p.stitched_path / f"{two}_xml_import_step_{k}.xml" for k in (1, 2, 3, 4, 5)]
    assert c.tsv == dict(tree_xml_path=c.projects[4], alt_stack_dir=str(p.preprocessed_path / two), cosine_blending=False)
    assert c.image_processor["downsampled_path"] == p.downsampled_path
    # nothing was made
    assert sorted(f.name for f in roots.iterdir()) == ["brain", "out", "rgb", "tf", "tmp"]
    assert untouched(roots, "out", "rgb", "tf", "tmp")
    m = A.plan(parse(roots, acq, "--stitch_mip", "--composite", str(roots / "rgb")))
    assert m.all_channels == [one + "_MIP", "Ex_642_Ch2_MIP"] and m.channel_colors == {one + "_MIP": "b", "Ex_642_Ch2_MIP": "r"}
    assert m.composite_path == roots / "rgb" / "brain_composite_MIP" and m.log_file.name == "log_mip.txt"
    assert m.voxel_size_z == 400.0                                                           # no assert against the target under --stitch_mip
    assert [c.image_processor["target_voxel"] for c in m.channels] == [None, None]
    # the RuntimeError cases
    for argv, word in ((["-i", str(roots / "nothing")], "does not exist"), (["-i", str(roots / "brain" / one / "000000" / "000000_000000" / "000000.tif")], "should be a folder"),
                       (["-t", str(roots / "no_tmp")], "--tmptif"), (["-s", str(roots / "no_out")], "--stitched"),
                       (["--composite", str(roots / "no_rgb")], "composite path")):
        with pytest.raises(RuntimeError, match=word):
            A.plan(parse(roots, acq, *argv))
    (roots / "empty").mkdir()
    with pytest.raises(RuntimeError, match="could not find unstitched files"):
        A.plan(parse(roots, roots / "empty"))
    with pytest.raises(ValueError, match="--vram_mem_fraction_gpu0"):
        A.plan(parse(roots, acq, "--vram_mem_fraction_gpu0", "0"))


def test_imaris_is_refused_with_nothing_created(roots):
    acq = make(roots, name="has-dash")
    with pytest.raises(NotImplementedError, match="--imaris"):
        A.plan(parse(roots, acq, "--imaris", str(roots / "out" / "brain.ims")), rename=True)
    assert sorted(f.name for f in roots.iterdir()) == ["has-dash", "out", "rgb", "tf", "tmp"]   # not even renamed
    assert untouched(roots, "out", "rgb", "tf", "tmp")


def test_rename_only_on_request(roots):
    acq = make(roots, name="brain-1-left")
    p = A.plan(parse(roots, acq))
    assert p.source_path == acq and acq.exists() and p.stitched_path.name == "brain-1-left_stitched"
    p = A.plan(parse(roots, acq), rename=True)
    assert p.source_path == roots / "brain_1_left" and p.source_path.exists() and not acq.exists()
    assert p.preprocessed_path == roots / "tmp" / "brain_1_left_tif"
    assert any("renamed" in n for n in p.notes)


@pytest.mark.parametrize("objective, more, slices, want", [
    ("15x", [], 36, ("--sD=10", "--subvoldim=36")),
    ("15x", [], 250, ("--sD=10", "--subvoldim=100")),
    ("40x", [], 250, ("--sD=0", "--subvoldim=10")),
    ("40x", [], 4, ("--sD=0", "--subvoldim=10")),
    ("15x", ["--stitch_mip"], 36, ("--sD=0", "--subvoldim=1")),
    ("15x", ["--skip_inspection"], 36, ("--sD=10", "--subvoldim=100")),
])
def test_search_depth_and_subvolume(roots, objective, more, slices, want):
    channel = U.CHANNELS[0] + ("_MIP" if "--stitch_mip" in more else "")
    acq = make(roots, [channel], grid=(1, 2), slices=slices, z_step=8)
    c = A.plan(parse(roots, acq, *more, objective=objective)).channels[0]
    for k in (2, 3, 4, 5):
        step = c.steps[k - 1]
        assert step[0] == f"-{k}" and tuple(step[1:3]) == want and step[3] == "--threshold=0.65"
        assert step[4:] == [f"--projin={c.projects[k - 2]}", f"--projout={c.projects[k - 1]}"]
    assert c.subvolume_depth == (100 if "--skip_inspection" in more else slices)
    assert (c.files_list is None) == ("--skip_inspection" in more)


def test_step_1_arguments_for_40x_against_15x(roots):
    acq = make(roots, z_step=8)
    for objective, want in (("15x", ["--ref1=H", "--ref2=V", "--ref3=D", "--vxl1=0.410", "--vxl2=0.410", "--vxl3=0.8"]),
                            ("40x", ["--ref1=V", "--ref2=H", "--ref3=D", "--vxl1=0.140", "--vxl2=0.140", "--vxl3=0.8"]),
                            ("4x", ["--ref1=H", "--ref2=V", "--ref3=D", "--vxl1=1.809", "--vxl2=1.809", "--vxl3=0.8"])):
        p = A.plan(parse(roots, acq, objective=objective))
        c = p.channels[0]
        assert c.steps[0] == ["-1"] + want + ["--sparse_data", f"--volin={p.preprocessed_path / c.channel}", f"--projout={c.projects[0]}",
                                              "--noprogressbar"]


def test_batch_filter_keywords_and_whether_the_stage_runs(roots):
    acq = make(roots, z_step=8)
    for objective, sigma in (("15x", (250, 250)), ("4x", (100, 100)), ("40x", (128, 256)), ("8x", (250, 250))):
        p = A.plan(parse(roots, acq, "--timeout", "30", "-n", "5", objective=objective))
        c = p.channels[0]
        assert c.preprocess and c.tiles == p.preprocessed_path / c.channel
        assert c.batch_filter == dict(
            input_path=acq / c.channel, output_path=p.preprocessed_path / c.channel, files_list=c.files_list, workers=5, continue_process=True,
            print_input_file_names=False, timeout=30.0, gaussian_filter_2d=True, bleach_correction_frequency=None,
            bleach_correction_max_method=False, sigma=sigma, level=0, wavelet="db9", crossover=10, threshold=None, padding_mode="reflect",
            bidirectional=True, lightsheet=False, down_sample=None, tile_size=p.tile_size, new_size=None, d_type="uint16",
            convert_to_8bit=False, bit_shift_to_right=8, compression=("ADOBE_DEFLATE", 1), threads_per_gpu=8)
        assert sorted(c.files_list) == sorted(acq.glob("*/*/*/*.tif")) and len(c.files_list) == 12
    p = A.plan(parse(roots, acq, "--no-de_stripe", "--no-resume", "-zl", "0"))
    b = p.channels[0].batch_filter
    assert (b["sigma"], b["continue_process"], b["compression"]) == ((0, 0), False, None) and p.channels[0].preprocess
    # nothing asked of the stage: it does not run and the stitch reads the source folder
    p = A.plan(parse(roots, acq, "--no-de_stripe", "--no-gaussian", "--no-need_raw_png_to_tiff_conversion"))
    c = p.channels[0]
    assert not c.preprocess and c.tiles == acq / c.channel and c.tsv["alt_stack_dir"] == str(acq / c.channel)
    assert c.steps[0][8] == f"--volin={acq / c.channel}"
    # ... unless the isotropic resize needs it
    assert A.plan(parse(roots, acq, "--no-de_stripe", "--no-gaussian", "--no-need_raw_png_to_tiff_conversion", "--isotropic")).channels[0].preprocess


FAKE_ESTIMATE = dict(bleach_correction_clip_min=5.25, bleach_correction_clip_med=6.5, bleach_correction_clip_max=8.75, bit_shift_to_right=3, dark=190)


@pytest.mark.parametrize("bleach", [True, False])
@pytest.mark.parametrize("eight_bit", [True, False])
def test_per_slice_keywords(roots, bleach, eight_bit):
    acq = make(roots, z_step=20)
    p = A.plan(parse(roots, acq, "--tile_size", "128", "128", "--padding_mode", "reflect", "--bleach_correction" if bleach else "--no-bleach_correction",
                     "--convert_to_8bit" if eight_bit else "--no-convert_to_8bit", "--no-rot90", "-dt", "12.5", "--cosine_blending"))
    c = p.channels[0]
    assert c.process_img_kwargs(FAKE_ESTIMATE, (320, 318), "uint16") == dict(
        sigma=(256, 256) if bleach else (0, 0), wavelet="db9", padding_mode="reflect", gpu_semaphore=None, bidirectional=bleach, threshold=6.5,
        bleach_correction_frequency=None, bleach_correction_clip_min=5.25, bleach_correction_clip_med=6.5, bleach_correction_clip_max=8.75,
        bleach_correction_max_method=False, dark=190, lightsheet=False, percentile=0.25, rotate=0, convert_to_8bit=eight_bit,
        bit_shift_to_right=3, tile_size=(320, 318), d_type="uint16")
    assert (c.need_bleach_correction, c.need_16bit_to_8bit_conversion) == (bleach, eight_bit)
    assert c.image_processor == dict(
        source_voxel=(2.0, 0.41, 0.41), target_voxel=12.5, downsampled_path=p.downsampled_path, rotation=0, timeout=None,
        max_processors=p.args.nthreads, progress_bar_name="TSV", compression=("ADOBE_DEFLATE", 1), resume=True, needed_memory=None,
        return_downsampled_path=True, down_sampled_dtype="float32")
    assert c.tsv["cosine_blending"] is True
    assert A.plan(parse(roots, acq)).channels[0].image_processor["rotation"] == 90


def test_align_namespace(roots):
    acq = make(roots, U.CHANNELS, z_step=20)
    one, two, three = U.CHANNELS
    p = A.plan(parse(roots, acq, "--composite", str(roots / "rgb"), "--terafly_channels", two))
    assert p.order == [two, one, three] and p.reference_channel == one
    # the planes align_images will read are integers; without a composite (and with one channel, which has none) they stay float32
    assert {c.image_processor["down_sampled_dtype"] for c in p.channels} == {"uint16"}
    assert {c.image_processor["down_sampled_dtype"] for c in A.plan(parse(roots, acq)).channels} == {"float32"}
    tifs =[Path(f"/s/{c}_tif") for c in p.order]
    downs = [Path(f"/d/{c}") for c in p.order]
    assert p.align_namespace(tifs, downs) == Namespace(
        red=(tifs[1], downs[1]), green=(tifs[0], downs[0]), blue=(tifs[2], downs[2]), output=roots / "rgb" / "acq_composite",
        write_alignments=True, generate_ims=False, max_iterations=10, reference="red", num_threads=8, save_singles=False, dtype="uint32",
        dx=(0.41, 0.41), dy=(0.41, 0.41), dz=(2.0, 2.0))
    # two channels: what align_images takes for an absent one; four: the first three
    ns = p.align_namespace(tifs[:2], downs[:2])
    assert (ns.red, ns.green, ns.blue) == ((tifs[1], downs[1]), (tifs[0], downs[0]), (None, None))
    ns = p.align_namespace(tifs + [Path("/s/Ex_642_Em_2_tif")], downs + [Path("/d/x")])
    assert (ns.red, ns.green, ns.blue) == ((tifs[1], downs[1]), (tifs[0], downs[0]), (tifs[2], downs[2]))


def test_bleach_wavelet(roots, monkeypatch, tmp_path):
    acq = make(roots, z_step=20)
    monkeypatch.setitem(sys.modules, "pywt", None)                                           # PyWavelets cannot be imported
    argv = ["--objective", "15x", "-i", str(acq), "-t", str(roots / "tmp"), "-s", str(roots / "out")]
    with pytest.raises(NotImplementedError, match=r"--bleach_wavelet='coif15'.*--bleach_wavelet FILE"):
        A.plan(A.build_parser().parse_args(argv))                                            # the default
    with pytest.raises(NotImplementedError, match="--bleach_wavelet='sym8'"):
        A.plan(A.build_parser().parse_args(argv + ["--bleach_wavelet", "sym8"]))
    # no channel is bleach-corrected: the wavelet is not looked at
    assert A.plan(A.build_parser().parse_args(argv + ["--no-bleach_correction"])).channels[0].bleach_wavelet == "coif15"
    assert A.plan(A.build_parser().parse_args(argv + ["--bleach_wavelet", "db9"])).channels[0].bleach_wavelet == "db9"
    from ipp_amd import wavelets
    haar = A.plan(A.build_parser().parse_args(argv + ["--bleach_wavelet", "haar"])).channels[0].bleach_wavelet
    assert haar == wavelets.resolve("db1") and haar.taps == 2
    table = tmp_path / "db4.txt"
    table.write_text(" ".join(repr(float(v)) for v in wavelets.daubechies(4)))
    got = A.plan(A.build_parser().parse_args(argv + ["--bleach_wavelet", str(table)])).channels[0].bleach_wavelet
    assert got == wavelets.resolve("db4")

    class FakePywt:                                                                          # a name goes through PyWavelets when it imports
        @staticmethod
        def Wavelet(name):
            return Namespace(rec_lo=list(wavelets.daubechies(3)), name=name)
    monkeypatch.setitem(sys.modules, "pywt", FakePywt)
    assert A.plan(A.build_parser().parse_args(argv)).channels[0].bleach_wavelet == wavelets.resolve("db3")


def stack_folders(root, counts):
    """<root>/<k>/<k>_0 with counts[k] empty .tif files"""
    folders = []
    for k, n in enumerate(counts):
        folder = root / f"{k:06d}" / f"{k:06d}_000000"
        folder.mkdir(parents=True)
        for z in range(n):
            (folder / f"{z * 20:06d}.tif").touch()
        (folder / "notes.txt").touch()                                                       # not a tile
        folders.append(folder)
    return folders


def test_inspection(tmp_path):
    lines = []
    stack_folders(tmp_path / "equal", [5, 5, 5])
    files, largest = A.inspect_for_missing_tiles_get_files_list(tmp_path / "equal", log=lines.append)
    assert largest == 5 and len(files) == 15 and all(f.suffix == ".tif" for f in files)
    assert len(lines) == 1 and "inspecting channel equal" in lines[0]
    assert A.missing_slices(files) == []

    lines.clear()
    folders = stack_folders(tmp_path / "short", [5, 3, 5])
    files, largest = A.inspect_for_missing_tiles_get_files_list(tmp_path / "short", log=lines.append)
    assert largest == 5 and len(files) == 13
    assert lines[1:3] == ["[3, 5]", "warning: following folders might have missing tiles:"]
    assert lines[3] == f"\tfolders having 3 tiles: \n\t\t{folders[1]}" and len(lines) == 4
    assert A.missing_slices(files) == [folders[1] / "000060.tif", folders[1] / "000080.tif"]

    # a count of 1 beside one other count is no warning (a stack that holds a single file is not a short stack) ...
    lines.clear()
    stack_folders(tmp_path / "single", [1, 5, 5])
    files, largest = A.inspect_for_missing_tiles_get_files_list(tmp_path / "single", log=lines.append)
    assert largest == 5 and len(files) == 11 and len(lines) == 1
    # ... beside two others it is, and the folders with one file are not listed
    lines.clear()
    folders = stack_folders(tmp_path / "single3", [1, 4, 5])
    files, largest = A.inspect_for_missing_tiles_get_files_list(tmp_path / "single3", log=lines.append)
    assert largest == 5 and lines[1] == "[1, 4, 5]" and len(lines) == 4 and lines[3].endswith(str(folders[1]))
    assert A.inspect_for_missing_tiles_get_files_list(tmp_path / "nowhere", skip=True) == (None, 100)


def test_missing_slices_keep_the_folder_s_own_spelling(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    files = [a / "000100_000200_000000.tif", a / "000100_000200_000020.tif", b / "000300_000200_000020.tif"]
    assert A.missing_slices(files) == [b / "000300_000200_000000.tif"]


def test_device_choice_and_rank_mode(roots, monkeypatch):
    assert A.pick_device((), 2) == 0 and A.pick_device((0,), 2) == 1 and A.pick_device((1, 0), 3) == 2
    with pytest.raises(RuntimeError, match="--exclude_gpus: 2 is not a valid gpu index"):
        A.pick_device((2,), 2)
    with pytest.raises(RuntimeError, match="--exclude_gpus"):
        A.pick_device((0,), 1)
    p = A.plan(parse(roots, make(roots, z_step=20), "--exclude_gpus", "3", "1"))
    assert p.exclude_gpus == (3, 1)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="WORLD_SIZE=2"):
        A.run(p)
    assert untouched(roots, "out", "tmp")


def test_terafly_levels_a_volume_can_hold():
    """level k needs 2^k slices within half a block of the depth (terafly.plan): six levels from 64 slices on"""
    for depth, want in ((1, "0"), (2, "0"), (4, "01"), (16, "0123"), (36, "01234"), (63, "01234"), (64, "012345"), (2000, "012345")):
        assert A.terafly_resolutions((depth, 320, 320)) == want, depth


def test_the_host_half_imports_no_torch():
    import subprocess
    code = "import sys; from ipp_amd import acquisition as A; A.build_parser(); assert 'torch' not in sys.modules, 'torch was imported'"
    root = Path(__file__).resolve().parent.parent
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0
