#!/usr/bin/env python3
"""convert.py on the MI355X: an existing slice folder (or a stitched TeraStitcher project) is destriped, bleach-corrected, background
subtracted, down-sampled, resized and converted to 8 bits slice by slice on the GPU, then turned into a TeraFly tree.

    python convert.py --input SLICES --tif OUT --bleach-correction --bleach-correction-period 2000 \\
           --bleach-correction-clip-min 5 --bleach-correction-clip-max 10 --downsample-x 2 --downsample-y 2 --convert-to-8bit --bit-shift 4
    python convert.py --input OUT --teraFly TERAFLY

The reference's option names, long and short, and its defaults (convert.py:301-400).  ``build_kwargs`` makes the ``process_img``
keywords and the ``parallel_image_processor`` keywords of convert.py:95-131; ``main`` follows its decision tree (:61-135).  The
per-slice pass is ``ipp_amd.parallel_image_processor`` with ``ipp_amd.pystripe.process_img``: a z group goes through every kernel
launch as one device stack.  ``--teraFly`` runs ``ipp_amd.terafly.convert`` in this process with resolutions "012345" and the mean
(the reference starts paraconverter under mpiexec with these arguments).

The clips go through as given, in log1p units, and ``bleach_correction_clip_med`` is never given: it is estimated per slice on the
device (four-class multi-Otsu of the log image).  With the reference's defaults of 20 and 255 that estimate lies below clip_min
and the assert of correct_bleaching fires, here as there: give clips in log1p units.

``--padding-mode`` takes every mode of ``numpy.pad`` but ``empty`` (the per-slice filter runs with ``extended=True``).
Additions and refusals: a project ``.xml`` as ``--input`` is opened as ``ipp_amd.tsv.TSVVolume`` (the reference hands
the path itself to a function that rejects it).  Refused by name before any folder is made: ``--imaris``, ``--fnt``, ``--movie``, an
``.ims`` input, ``--channel`` other than 0 together with ``--teraFly``.  ``--nthreads``, ``--timeout``, ``--needed-memory`` and
``--threads-per-gpu`` are accepted and ignored.  ``main`` adds ``extended=True`` to the ``process_img`` keywords (automatic clips,
median, ``new_size``) and ``wavelet="db9"`` when it destripes (``process_img``'s default name has no table here).
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = "ipp_amd"

DOWNSAMPLE_METHODS = ("min", "max", "mean", "median")
DESTRIPE_SIGMA = (250, 250)
TERAFLY_RESOLUTIONS, TERAFLY_HALVE = "012345", "mean"


def make_parser():
    p = argparse.ArgumentParser(prog="convert.py", allow_abbrev=False,
                                description="2-D series (or stitched project) to processed TIFF series and TeraFly, on the GPU")
    flag = dict(default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("--input", "-i", type=str, required=True, help="a folder of 2-D tif / tiff / png / raw slices, or a TeraStitcher project .xml")
    p.add_argument("--tif", "-t", type=str, default="", help="folder of the processed TIFF slices")
    p.add_argument("--teraFly", "-f", type=str, default="", help="folder of the TeraFly tree")
    p.add_argument("--fnt", "-fnt", type=str, default="", help="not built")
    p.add_argument("--imaris", "-o", type=str, default="", help="not built")
    p.add_argument("--movie", "-m", type=str, default="", help="not built")
    p.add_argument("--nthreads", "-n", type=int, default=os.cpu_count() or 1, help="accepted and ignored")
    p.add_argument("--channel", "-c", type=int, default=0, help="channel of RGB slices; negative: the slices are copied unprocessed")
    p.add_argument("--gaussian", "-g", help="accepted; does nothing, as in the reference's process_img", **flag)
    p.add_argument("--destripe", help="stripe filter at sigma (250, 250), bidirectional", **flag)
    p.add_argument("--padding-mode", "-w", type=str, default="reflect", help="padding of the stripe filter: reflect, wrap, symmetric, edge, constant, linear_ramp, maximum, mean, median, minimum")
    p.add_argument("--downsample-x", "-dsx", type=int, default=0, help="2-D down-sampling factor along x")
    p.add_argument("--downsample-y", "-dsy", type=int, default=0, help="2-D down-sampling factor along y")
    p.add_argument("--downsample-method", "-dsm", type=str, default="mean", help="max, min, mean or median")
    p.add_argument("--downsample-dtype", "-dsdt", type=str, default="float32", help="type of the isotropic down-sampled volume")
    p.add_argument("--downsample-path", "-dsp", type=str, default="", help="folder of the isotropic down-sampled volume")
    p.add_argument("--new-size-x", "-nsx", type=int, default=0, help="columns every slice is resized to (with --new-size-y)")
    p.add_argument("--new-size-y", "-nsy", type=int, default=0, help="rows every slice is resized to (with --new-size-x)")
    p.add_argument("--dark", "-d", type=int, default=0, help="value subtracted from every sample above it; the others become 0")
    p.add_argument("--background-subtraction", help="lightsheet background subtraction", **flag)
    p.add_argument("--bleach-correction", help="bleach correction; clip_med is estimated per slice", **flag)
    p.add_argument("--bleach-correction-period", type=float, default=2000, help="inverse of the low-pass frequency; the camera tile size is usual")
    p.add_argument("--bleach-correction-clip-min", type=float, default=20, help="foreground vs background threshold, in log1p units")
    p.add_argument("--bleach-correction-clip-max", type=float, default=255, help="largest value without outliers, in log1p units")
    p.add_argument("--convert-to-16bit", **flag)
    p.add_argument("--convert-to-8bit", **flag)
    p.add_argument("--bit-shift", "-b", type=int, default=8, help="right shift of the 8-bit conversion, 0 .. 8")
    p.add_argument("--rotation", "-r", type=int, default=0, help="0, 90, 180 or 270")
    p.add_argument("--flip-upside-down", **flag)
    p.add_argument("--compression-level", "-zl", type=int, default=1, help="0: uncompressed")
    p.add_argument("--compression-method", "-zm", type=str, default="ADOBE_DEFLATE")
    p.add_argument("--movie-start", type=int, default=0)
    p.add_argument("--movie-end", type=int, default=None)
    p.add_argument("--movie-frame-duration", type=int, default=5)
    p.add_argument("--voxel-size-x", "-dx", type=float, default=1)
    p.add_argument("--voxel-size-y", "-dy", type=float, default=1)
    p.add_argument("--voxel-size-z", "-dz", type=float, default=1)
    p.add_argument("--voxel-size-target", "-dt", type=float, default=None, help="voxel size of the isotropic down-sampled volume")
    p.add_argument("--timeout", type=float, default=None, help="accepted and ignored")
    p.add_argument("--rename", help="outputs are named img_000000.tif, ...", **flag)
    p.add_argument("--resume", help="slices whose output exists are left alone", **flag)
    p.add_argument("--needed-memory", type=int, default=1, help="accepted and ignored")
    p.add_argument("--save-images", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--threads-per-gpu", type=int, default=1, help="accepted and ignored")
    return p


def parse_args(argv=None):
    return make_parser().parse_args(argv)


def _fail(message):
    print(message)
    raise RuntimeError(message)


def _down_sample(args):
    if args.downsample_y > 0 or args.downsample_x > 0:
        return (args.downsample_y or 1, args.downsample_x or 1)
    return None


def _new_size(args):
    if args.new_size_y and args.new_size_x:
        return (args.new_size_y, args.new_size_x)
    if args.new_size_y or args.new_size_x:
        _fail("both new_size_x and new_size_y are needed!")
    return None


def build_kwargs(args):
    """(process_img keywords or None, parallel_image_processor keywords) for the parsed options: the dicts of convert.py:95-116 and
    :117-131.  A pure function of ``args``; raises the reference's RuntimeError for an unknown down-sampling method and for one
    new size without the other.  ``gpu_semaphore`` is None: there is no queue of devices here."""
    if args.downsample_method.lower() not in DOWNSAMPLE_METHODS:
        _fail(f"unsupported down-sampling method: {args.downsample_method}")
    process = None
    if args.channel >= 0:
        process = dict(
            gaussian_filter_2d=args.gaussian, down_sample=_down_sample(args), down_sample_method=args.downsample_method, new_size=_new_size(args),
            sigma=DESTRIPE_SIGMA if args.destripe else (0, 0), padding_mode=args.padding_mode, bidirectional=True, dark=args.dark,
            lightsheet=args.background_subtraction,
            bleach_correction_frequency=1 / args.bleach_correction_period if args.bleach_correction else None,
            bleach_correction_max_method=False, bleach_correction_clip_min=args.bleach_correction_clip_min,
            bleach_correction_clip_max=args.bleach_correction_clip_max, exclude_dark_edges_set_them_to_zero=False, rotate=0,
            flip_upside_down=args.flip_upside_down, convert_to_16bit=args.convert_to_16bit, convert_to_8bit=args.convert_to_8bit,
            bit_shift_to_right=args.bit_shift, gpu_semaphore=None)
    else:
        _new_size(args)
    pip = dict(
        rename=args.rename, max_processors=args.nthreads, channel=args.channel,
        compression=(args.compression_method, args.compression_level) if args.compression_level > 0 else None, timeout=args.timeout,
        source_voxel=(args.voxel_size_z, args.voxel_size_y, args.voxel_size_x), target_voxel=args.voxel_size_target, rotation=args.rotation,
        resume=args.resume, needed_memory=args.needed_memory * 1024 ** 3, save_images=args.save_images, downsampled_path=args.downsample_path,
        alternating_downsampling_method=not args.downsample_method, down_sampled_dtype=args.downsample_dtype)
    return process, pip


def needs_processing(args, is_dir=True):
    """(the slices go through parallel_image_processor, process_img runs on them): convert.py:61-77."""
    down, size = _down_sample(args), _new_size(args)
    wanted = bool(args.dark > 0 or args.convert_to_8bit or size or down or args.voxel_size_target or args.rotation or args.flip_upside_down
                  or args.gaussian or args.background_subtraction or args.destripe or args.bleach_correction)
    pre = bool(args.dark > 0 or args.convert_to_8bit or down or args.flip_upside_down or args.gaussian or args.background_subtraction
               or args.destripe or args.bleach_correction)
    return (wanted if is_dir else True), pre


def check_unsupported(args):
    """NotImplementedError naming the first option this build does not do; nothing on disk has been touched."""
    for name in ("imaris", "fnt", "movie"):
        if getattr(args, name):
            raise NotImplementedError(f"--{name}={getattr(args, name)!r}: the {name} output is not built (--tif and --teraFly are)")
    if Path(args.input).suffix.lower() == ".ims":
        raise NotImplementedError(f"--input={args.input!r}: an Imaris (.ims) input is not built (a folder of 2-D slices and a project .xml are)")
    if args.teraFly and args.channel != 0:
        raise NotImplementedError(f"--channel={args.channel} with --teraFly: the TeraFly conversion is built for single-channel series (--channel 0)")


def main(args):
    """The reference's main(args) for the built outputs.  Returns the TeraFly plan, or None without ``--teraFly``."""
    check_unsupported(args)
    input_path = Path(args.input)
    if not args.input or not input_path.exists():
        _fail("Input path is not valid.")
    process, pip = build_kwargs(args)
    is_xml = input_path.is_file() and input_path.suffix.lower() == ".xml"
    through, pre = needs_processing(args, input_path.is_dir())
    tif_folder = Path(args.tif)
    if is_xml or (input_path.is_dir() and through):
        if not args.tif:
            _fail("tif path is needed to continue.")
        from . import pystripe
        from .parallel_image_processor import parallel_image_processor
        tif_folder.mkdir(parents=True, exist_ok=True)
        source = input_path
        if is_xml:
            from .tsv import TSVVolume
            source = TSVVolume(str(input_path))
        if process is not None:   # what this build's process_img needs beside the reference's keywords
            process = dict(process, extended=True, **(dict(wavelet="db9") if process["sigma"] != (0, 0) else {}))
        pip = dict(pip, downsampled_path=pip["downsampled_path"] or None)
        rc = parallel_image_processor(source=source, destination=tif_folder, fun=pystripe.process_img if pre else None, kwargs=process, **pip)
        assert rc == 0
    elif input_path.is_dir():
        tif_folder = input_path
    else:
        _fail("Input path is not valid: a folder of 2-D slices or a project .xml is expected.")
    if not args.teraFly:
        return None
    from . import terafly
    dst = Path(args.teraFly)
    dst.mkdir(parents=True, exist_ok=True)
    start = time.time()
    plan = terafly.convert(tif_folder, dst, resolutions=TERAFLY_RESOLUTIONS, halve=TERAFLY_HALVE)
    print(f"elapsed time = {round((time.time() - start) / 60, 1)}")
    return plan


if __name__ == "__main__":
    main(parse_args())
    sys.exit(0)
