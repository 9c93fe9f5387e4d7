"""CPU: ``ipp_amd.convert`` -- the options, ``build_kwargs`` against the dictionaries the reference's convert.py builds for the same
command lines (written out here from convert.py:95-131), the messages of its decision tree, and the refusals, which come before
anything on disk is touched."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def cv():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import convert
    return convert


def process_dict(**changes):
    """the process_img dictionary of convert.py:95-116 at the defaults of its parser"""
    base = dict(gaussian_filter_2d=False, down_sample=None, down_sample_method="mean", new_size=None, sigma=(0, 0), padding_mode="reflect",
                bidirectional=True, dark=0, lightsheet=False, bleach_correction_frequency=None, bleach_correction_max_method=False,
                bleach_correction_clip_min=20.0, bleach_correction_clip_max=255.0, exclude_dark_edges_set_them_to_zero=False, rotate=0,
                flip_upside_down=False, convert_to_16bit=False, convert_to_8bit=False, bit_shift_to_right=8, gpu_semaphore=None)
    assert set(changes) <= set(base)
    return dict(base, **changes)


def pip_dict(nthreads, **changes):
    """the parallel_image_processor keywords of convert.py:117-131 at the defaults of its parser"""
    base = dict(rename=False, max_processors=nthreads, channel=0, compression=("ADOBE_DEFLATE", 1), timeout=None, source_voxel=(1.0, 1.0, 1.0),
                target_voxel=None, rotation=0, resume=False, needed_memory=1024 ** 3, save_images=True, downsampled_path="",
                alternating_downsampling_method=False, down_sampled_dtype="float32")
    assert set(changes) <= set(base)
    return dict(base, **changes)


COMMAND_LINES = [
    (["-i", "in", "-t", "out"], {}, {}),
    (["--input", "in", "--tif", "out", "--bleach-correction", "--bleach-correction-period", "40", "--bleach-correction-clip-min", "3",
      "--bleach-correction-clip-max", "9", "--downsample-x", "2", "--downsample-y", "2", "--downsample-method", "median", "--convert-to-8bit",
      "--bit-shift", "4", "--rotation", "90"],
     dict(down_sample=(2, 2), down_sample_method="median", bleach_correction_frequency=1 / 40, bleach_correction_clip_min=3.0,
          bleach_correction_clip_max=9.0, convert_to_8bit=True, bit_shift_to_right=4),
     dict(rotation=90)),
    (["-i", "in", "-t", "out", "--destripe", "-w", "wrap", "-dsx", "3", "-nsx", "100", "-nsy", "80", "-d", "120", "--background-subtraction", "-g",
      "--flip-upside-down", "--convert-to-16bit", "-zl", "0", "-dx", "0.5", "-dy", "0.6", "-dz", "2", "-dt", "10", "-dsdt", "uint8", "-dsp", "down",
      "--rename", "--resume", "--no-save-images", "--needed-memory", "3", "--timeout", "7.5", "-n", "5"],
     dict(gaussian_filter_2d=True, down_sample=(1, 3), new_size=(80, 100), sigma=(250, 250), padding_mode="wrap", dark=120, lightsheet=True,
          flip_upside_down=True, convert_to_16bit=True),
     dict(rename=True, max_processors=5, compression=None, timeout=7.5, source_voxel=(2.0, 0.6, 0.5), target_voxel=10.0, resume=True,
          needed_memory=3 * 1024 ** 3, save_images=False, downsampled_path="down", down_sampled_dtype="uint8")),
    (["-i", "in", "-t", "out", "-c", "-1", "-dsm", "", "-zm", "LZW", "-zl", "5", "-r", "270"], None,
     dict(channel=-1, compression=("LZW", 5), rotation=270, alternating_downsampling_method=True)),
]


@pytest.mark.parametrize("argv,process,pip", COMMAND_LINES[:3])
def test_build_kwargs_equals_the_references_dictionaries(cv, argv, process, pip):
    args = cv.parse_args(argv)
    got_process, got_pip = cv.build_kwargs(args)
    assert got_process == process_dict(**process)
    assert got_pip == pip_dict(args.nthreads, **pip)
    assert list(got_process) == list(process_dict()) and list(got_pip) == list(pip_dict(0))
    # every keyword is one process_img takes
    import inspect
    from ipp_amd import pystripe
    from ipp_amd.parallel_image_processor import parallel_image_processor
    assert set(got_process) <= set(inspect.signature(pystripe.process_img).parameters)
    assert set(got_pip) <= set(inspect.signature(parallel_image_processor).parameters)


def test_negative_channel_has_no_process_img_dictionary(cv):
    argv, _, pip = COMMAND_LINES[3]
    args = cv.parse_args([a for a in argv if a not in ("-dsm", "")])
    process, got = cv.build_kwargs(args)
    assert process is None
    assert got == pip_dict(args.nthreads, **dict(pip, alternating_downsampling_method=False))
    # an empty method name is the reference's RuntimeError (it is not one of the four)
    with pytest.raises(RuntimeError, match="unsupported down-sampling method"):
        cv.build_kwargs(cv.parse_args(argv))


def test_defaults_and_short_names(cv):
    a = cv.parse_args(["-i", "x"])
    assert (a.tif, a.teraFly, a.fnt, a.imaris, a.movie, a.channel) == ("", "", "", "", "", 0)
    assert (a.bleach_correction_period, a.bleach_correction_clip_min, a.bleach_correction_clip_max) == (2000, 20, 255)
    assert (a.downsample_method, a.downsample_dtype, a.padding_mode, a.bit_shift, a.compression_level, a.compression_method) == \
        ("mean", "float32", "reflect", 8, 1, "ADOBE_DEFLATE")
    assert (a.save_images, a.resume, a.rename, a.threads_per_gpu, a.needed_memory, a.voxel_size_target) == (True, False, False, 1, 1, None)
    b = cv.parse_args(["-i", "x", "-t", "t", "-f", "f", "-fnt", "n", "-o", "o", "-m", "m", "-n", "3", "-c", "2", "-b", "5", "-r", "180"])
    assert (b.tif, b.teraFly, b.fnt, b.imaris, b.movie, b.nthreads, b.channel, b.bit_shift, b.rotation) == ("t", "f", "n", "o", "m", 3, 2, 5, 180)
    with pytest.raises(SystemExit):
        cv.parse_args(["-t", "out"])          # --input is required


def test_messages_of_the_decision_tree(cv, tmp_path, capsys):
    src = tmp_path / "slices"
    src.mkdir()
    with pytest.raises(RuntimeError, match="Input path is not valid"):
        cv.main(cv.parse_args(["-i", str(tmp_path / "nothing")]))
    with pytest.raises(RuntimeError, match="tif path is needed to continue."):
        cv.main(cv.parse_args(["-i", str(src), "--convert-to-8bit"]))
    assert "tif path is needed to continue." in capsys.readouterr().out
    for one in (["-nsx", "64"], ["-nsy", "64"]):
        with pytest.raises(RuntimeError, match="both new_size_x and new_size_y are needed!"):
            cv.main(cv.parse_args(["-i", str(src), "-t", str(tmp_path / "out")] + one))
    with pytest.raises(RuntimeError, match="unsupported down-sampling method: mode"):
        cv.main(cv.parse_args(["-i", str(src), "-t", str(tmp_path / "out"), "-dsm", "mode"]))
    assert not (tmp_path / "out").exists()
    # when processing is needed, and when process_img runs (a new size, a rotation or a target voxel alone do not call it)
    for argv, want in (([], (False, False)), (["--dark", "5"], (True, True)), (["-nsx", "4", "-nsy", "4"], (True, False)),
                       (["-r", "90"], (True, False)), (["-dt", "10"], (True, False)), (["--bleach-correction"], (True, True)),
                       (["-dsy", "2"], (True, True)), (["-g"], (True, True)), (["--convert-to-16bit"], (False, False))):
        assert cv.needs_processing(cv.parse_args(["-i", "x"] + argv)) == want, argv


def test_plain_folder_goes_straight_to_terafly(cv, tmp_path, monkeypatch):
    from ipp_amd import terafly
    src = tmp_path / "slices"
    src.mkdir()
    seen = {}

    def fake(s, d, **kw):
        seen.update(src=s, dst=d, **kw)
        return "plan"
    monkeypatch.setattr(terafly, "convert", fake)
    assert cv.main(cv.parse_args(["-i", str(src), "-f", str(tmp_path / "fly")])) == "plan"
    assert seen == dict(src=src, dst=tmp_path / "fly", resolutions="012345", halve="mean") and (tmp_path / "fly").is_dir()
    assert cv.main(cv.parse_args(["-i", str(src)])) is None


def test_refusals_come_before_the_filesystem(cv, tmp_path):
    src = tmp_path / "slices"
    src.mkdir()
    out = tmp_path / "out"
    base = ["-i", str(src), "-t", str(out), "--dark", "5"]
    for extra, word in ((["--imaris", str(tmp_path / "a.ims")], "--imaris"), (["-fnt", str(tmp_path / "fnt")], "--fnt"),
                        (["--movie", str(tmp_path / "m.mp4")], "--movie"), (["-f", str(tmp_path / "fly"), "-c", "1"], "--channel=1"),
                        (["-f", str(tmp_path / "fly"), "-c", "-1"], "--channel=-1")):
        with pytest.raises(NotImplementedError, match=word):
            cv.main(cv.parse_args(base + extra))
    with pytest.raises(NotImplementedError, match=r"\.ims"):
        cv.main(cv.parse_args(["-i", str(tmp_path / "volume.ims"), "-t", str(out)]))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["slices"]
