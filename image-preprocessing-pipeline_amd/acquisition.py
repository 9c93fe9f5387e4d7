#!/usr/bin/env python3
"""The acquisition driver: every stage of the reference's ``process_images.py`` in one run.

    python image-preprocessing-pipeline_amd/acquisition.py --input ACQ --tmptif TMP --stitched OUT --objective 15x [...]

``ACQ`` is a raw acquisition folder, one sub-folder per channel (``Ex_488_Em_525/<H>/<H>_<V>/<z>.tif``, coordinates in 0.1 um).  Per
channel the run preprocesses the tiles (``pystripe.batch_filter``), aligns them (``process_images.py -1 ... -5``), merges and
post-processes the slices (``tsv.TSVVolume``, ``thresholds.estimate_slice_params``, ``parallel_image_processor`` with
``pystripe.process_img``) and converts the chosen channels to TeraFly (``terafly.convert``); then it aligns the channels into an RGB
series (``align_images.main``).  The options are the reference's, with their names, short names, defaults and choices
(process_images.py:1629-1725); what each stage receives is what ``main`` and ``process_channel`` of the reference decide
(:1062-1487, :334-786).

The module has two halves.  ``build_parser()`` and ``plan(args)`` are host code: no torch, no device, no directory made; the
``AcquisitionPlan`` they return spells every stage's arguments as plain data.  ``run(plan)`` executes it in this process, calling the
stages' Python entry points in the reference's order; the data moves between the stages through the files the reference also writes.
No kernel belongs to this module.

Departures from the reference:
  * the stages run in this process, one after the other: no subprocess, no MPI, no pool.  The TeraFly conversion of a channel, which
    the reference starts in the background, runs before the next channel;
  * options without a counterpart: ``--tile_size``, ``--voxel_size_z``, ``--bleach_wavelet``;
  * a two-channel composite: the reference indexes a third path that does not exist; here ``align_images`` gets ``(None, None)`` for
    the absent blue channel, which it accepts;
  * the composite pairs every stitched folder with its own down-sampled folder (the reference reorders only the first list);
  * with ``--composite`` the down-sampled planes are uint16 (``down_sampled_dtype``), not the reference's float32: ``align_images``
    composes integer channels only and refuses float32 planes by name;
  * a slice that other stacks of a channel hold and one stack lacks is handed to ``batch_filter`` as well, which writes the zero tile
    of ``tile_size`` and uint16 it writes for a file it cannot read (the reference writes such dummy slices later, in its TSVVolume);
  * the TeraFly conversion asks for the leading levels of "012345" that the volume can hold (``terafly_resolutions``): the reference's
    fixed six levels are refused by its converter, and by ``terafly.convert``, for fewer than 64 slices;
  * when no preprocessing is asked for, the stitch reads the source folder;
  * ``--nthreads``, ``--timeout``, ``--vram_mem_fraction_gpu0`` and ``--enable_axis_correction`` are accepted and ignored.
Refused by name: ``--imaris`` (NotImplementedError, before anything is created) and a run under ``WORLD_SIZE`` > 1 (RuntimeError: the
stages' rank modes are not composed here).  A stage's own refusal propagates unchanged: of ``--padding_mode`` the per-slice filter
does every choice but ``empty``.
"""
from __future__ import annotations

import argparse
import os
import platform
import re
import sys
import time
from argparse import Namespace
from dataclasses import dataclass, field
from datetime import datetime, timedelta
from pathlib import Path

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = "ipp_amd"

# (channel folder name, colour of the composite), process_images.py:52-57
ALL_CHANNELS = (
    ("Ex_488_Em_525", "b"), ("Ex_561_Em_600", "g"), ("Ex_647_Em_690", "r"), ("Ex_642_Em_690", "r"),
    ("Ex_488_Em_1", "b"), ("Ex_561_Em_1", "g"), ("Ex_642_Em_1", "r"),
    ("Ex_488_Ch0", "b"), ("Ex_561_Ch1", "g"), ("Ex_642_Ch2", "r"),
    ("Ex_488_Em_2", "b"), ("Ex_561_Em_2", "g"), ("Ex_642_Em_2", "r"), ("Ex_642_Em_680", "r"),
)
# objective -> (voxel size x, voxel size y, tile size (y, x)), get_voxel_sizes (:58-63, :89-110).  10x has a table entry and is no choice
# of --objective, as in the reference.
OBJECTIVES = {
    "4x": (1.809, 1.809, (1600, 2000)),
    "8x": (0.82, 0.82, (2000, 2000)),
    "9x": (0.72, 0.72, (2000, 2000)),
    "10x": (0.62, 0.62, (2000, 2000)),
    "15x": (0.41, 0.41, (2000, 2000)),
    "40x": (0.14, 0.14, (2048, 2048)),
}
OBJECTIVE_CHOICES = ("15x", "9x", "8x", "4x", "40x")
PADDING_MODES = ("constant", "edge", "linear_ramp", "maximum", "mean", "median", "minimum", "reflect", "symmetric", "wrap", "empty")
COMPRESSION_METHODS = ("ADOBE_DEFLATE", "LZW", "PackBits")
SUPPORTED_EXTENSIONS = (".png", ".tif", ".tiff", ".raw")
MAX_SUBVOLUME_DEPTH = 100
STITCH_THRESHOLD = 0.65
TERAFLY_RESOLUTIONS, TERAFLY_HALVE = "012345", "mean"
DEFAULT_BLEACH_WAVELET = "coif15"
COMPOSITE_PLANE_DTYPE = "uint16"
IGNORED_OPTIONS = ("nthreads", "timeout", "vram_mem_fraction_gpu0", "enable_axis_correction")


# ---------------------------------------------------------------------------------------------------------------------------------
# command line

def build_parser():
    """The reference's parser (process_images.py:1629-1725) and three options of this module's own."""
    flag = argparse.BooleanOptionalAction
    p = argparse.ArgumentParser(prog="acquisition.py", description="raw light-sheet acquisition -> stitched, post-processed slices, "
                                                                   "TeraFly trees and the RGB series, on the GPU")
    p.add_argument("--objective", type=str, required=True, choices=OBJECTIVE_CHOICES, help="objective the acquisition was imaged with")
    p.add_argument("--input", "-i", type=str, required=True, help="acquisition folder: one sub-folder of tiles per channel")
    p.add_argument("--tmptif", "-t", type=str, required=True, help="existing folder that receives <input name>_tif, the preprocessed tiles")
    p.add_argument("--stitched", "-s", type=str, required=True, help="existing folder that receives <input name>_stitched")
    p.add_argument("--composite", type=str, required=False, help="existing folder that receives the RGB series; given: the channels are "
                                                                 "aligned and composed")
    p.add_argument("--reference_channel", type=str, required=False, default="", help="channel the others are aligned to (default: the first)")
    p.add_argument("--stitch_based_on_reference_channel_alignment", default=False, action=flag,
                   help="stitch every channel with the reference channel's project files")
    p.add_argument("--imaris", "-o", type=str, required=False, help="refused: the Imaris conversion is not built")
    p.add_argument("--terafly_channels", "-f", required=False, nargs="+", default=[], help="channels converted to TeraFly")
    p.add_argument("--terafly_path", type=str, required=False, default="", help="folder of the TeraFly trees (default: the stitched folder)")
    p.add_argument("--nthreads", "-n", type=int, default=os.cpu_count() or 1, help="accepted and ignored")
    p.add_argument("--stitch_mip", default=False, action=flag, help="stitch the <channel>_MIP folders")
    p.add_argument("--need_raw_png_to_tiff_conversion", default=True, action=flag, help="preprocessing: the tiles are rewritten as TIFF")
    p.add_argument("--gaussian", "-g", default=True, action=flag, help="preprocessing: the Gaussian switch of batch_filter")
    p.add_argument("--de_stripe", default=True, action=flag, help="preprocessing: stripe filter of the tiles")
    p.add_argument("--padding_mode", type=str, default="wrap", choices=PADDING_MODES, help="padding of the per-slice stripe filter")
    p.add_argument("--isotropic", default=False, action=flag, help="preprocessing: resize the tiles so that xy voxels equal the z step")
    p.add_argument("--bleach_correction", default=True, action=flag, help="post-processing: bleach correction of the stitched slices")
    p.add_argument("--bleach_correction_channels", required=False, nargs="+", default=[], help="channels that get it (default: all)")
    p.add_argument("--background_subtraction", default=False, action=flag, help="post-processing: lightsheet background subtraction")
    p.add_argument("--background_subtraction_channels", required=False, nargs="+", default=[], help="channels that get it (default: all)")
    p.add_argument("--convert_to_8bit", default=True, action=flag, help="post-processing: 8-bit slices, bit shift estimated from the data")
    p.add_argument("--rot90", default=True, action=flag, help="post-processing: rotate the stitched slices by 90 degrees")
    p.add_argument("--compression_method", "-zm", type=str, default="ADOBE_DEFLATE", choices=COMPRESSION_METHODS,
                   help="TIFF compression of tiles and slices")
    p.add_argument("--compression_level", "-zl", type=int, default=1, choices=range(0, 10), metavar="[0-9]", help="0: uncompressed")
    p.add_argument("--voxel_size_target", "-dt", type=float, default=10, help="voxel size of the isotropic down-sampled volume, um")
    p.add_argument("--resume", default=True, action=flag, help="leave alone the tiles, projects and slices that exist")
    p.add_argument("--timeout", type=float, default=None, help="accepted and ignored")
    p.add_argument("--skipconf", default=False, action=flag, help="do not wait for Enter after the summary")
    p.add_argument("--skip_inspection", default=False, action=flag, help="do not look for missing tiles")
    p.add_argument("--exclude_gpus", required=False, nargs="+", default=[], help="device indices that must not be used")
    p.add_argument("--vram_mem_fraction_gpu0", required=False, type=float, default=1.0, help="accepted and ignored")
    p.add_argument("--enable_axis_correction", default=False, action=flag, help="accepted and ignored (Imaris sources only)")
    p.add_argument("--cosine_blending", default=False, action=flag, help="cosine blend of the tile seams instead of the maximum")
    own = p.add_argument_group("options without a counterpart in the reference")
    own.add_argument("--tile_size", type=int, nargs=2, default=None, metavar=("Y", "X"),
                     help="camera tile size (default: the objective's table entry, which the reference hard-codes)")
    own.add_argument("--voxel_size_z", type=float, default=None, metavar="UM",
                     help="z step (default: from the file names; the reference prompts when that fails)")
    own.add_argument("--bleach_wavelet", type=str, default=DEFAULT_BLEACH_WAVELET, metavar="NAME|FILE",
                     help="wavelet of the per-slice stripe filter: a name (default coif15, through PyWavelets when it has no built-in "
                          "table) or a file with rec_lo as pystripe.py --wavelet_file takes it")
    return p


# ---------------------------------------------------------------------------------------------------------------------------------
# host functions of the reference

def _now():
    return datetime.now().isoformat(timespec="seconds", sep=" ")


def _fail(message, kind=RuntimeError):
    print(message)
    raise kind(message)


def get_list_of_files(folder, extensions=SUPPORTED_EXTENSIONS):
    extensions = tuple(e.lower() for e in extensions)
    return [f for f in Path(folder).iterdir() if f.suffix.lower() in extensions]


def inspect_for_missing_tiles_get_files_list(channel_path, skip=False, log=print):
    """(every tile file of the channel, the largest file count of a stack folder), process_images.py:160-193.  Folders with fewer files
    than the largest count are reported through ``log`` -- unless the only smaller count is 1 (a stack that holds one file is not
    counted as short; with a 1 among the counts a third count is needed for the warning).  ``skip``: ``(None, 100)``, what the
    reference uses under --skip_inspection."""
    if skip:
        return None, MAX_SUBVOLUME_DEPTH
    channel_path = Path(channel_path)
    log(f"{_now()}: inspecting channel {channel_path.name} for missing files.")
    folders = [y for x in channel_path.iterdir() if x.is_dir() for y in x.iterdir() if y.is_dir()]
    by_count, files = {}, []
    for folder in folders:
        found = get_list_of_files(folder)
        by_count.setdefault(len(found), []).append(str(folder))
        files += found
    counts = sorted(by_count)
    if (len(counts) > 1 and counts[0] != 1) or (len(counts) > 2 and counts[0] == 1):
        log(str(counts))
        log("warning: following folders might have missing tiles:")
        for count in counts[:-1]:
            if count != 1:
                log(f"\tfolders having {count} tiles: \n\t\t" + "\n\t\t".join(by_count[count]))
    return files, counts[-1]


def missing_slices(files):
    """The paths a channel lacks: for every stack folder of ``files``, the z positions (the last run of digits of a file's stem) that
    another folder holds and this one does not, spelled like the folder's own files.  No counterpart in the reference, which writes
    dummy slices for them in its TSVVolume; here ``batch_filter`` writes its zero tile for each."""
    def z_key(path):
        runs = re.findall(r"\d+", path.stem)
        return runs[-1] if runs else None
    folders = {}
    for f in files:
        folders.setdefault(f.parent, {})[z_key(f)] = f
    every = {k for held in folders.values() for k in held if k is not None}
    missing = []
    for folder, held in folders.items():
        template = next((f for k, f in sorted(held.items(), key=lambda kv: str(kv[0])) if k is not None), None)
        if template is None:
            continue
        key = z_key(template)
        head, tail = template.stem.rsplit(key, 1)
        for k in sorted(every - set(held)):
            missing.append(folder / f"{head}{k}{tail}{template.suffix}")
    return missing


def voxel_size_z_from_names(path):
    """The z step in um from the first stack folder that holds two files whose stems are integers in 0.1 um (:123-140), or None."""
    for y_folder in sorted(Path(path).iterdir()):
        if not y_folder.is_dir():
            continue
        for x_folder in sorted(y_folder.iterdir()):
            if not x_folder.is_dir():
                continue
            try:
                files = sorted(f for f in x_folder.iterdir() if f.suffix.lower() in SUPPORTED_EXTENSIONS and f.is_file())
                if len(files) > 1:
                    return (int(files[1].stem) - int(files[0].stem)) / 10
            except (ValueError, OSError) as e:
                print(e)
    return None


def get_voxel_sizes(objective, path, is_mip, tile_size=None, voxel_size_z=None):
    """(voxel size x, y, z, tile size (y, x)) of process_images.py:89-148.  ``tile_size`` and ``voxel_size_z`` override the table and the
    file names.  Without a z step from either, the reference prompts: here only when stdin is a terminal, else RuntimeError."""
    if objective not in OBJECTIVES:
        _fail("Error: unsupported objective")
    voxel_size_x, voxel_size_y, table_tile = OBJECTIVES[objective]
    tile_size = table_tile if tile_size is None else (int(tile_size[0]), int(tile_size[1]))
    if voxel_size_z is None:
        voxel_size_z = voxel_size_z_from_names(path)
    if voxel_size_z is None:
        if not sys.stdin.isatty():
            _fail(f"the z step cannot be read from the file names under {path} and there is no terminal to ask on: give --voxel_size_z UM")
        hint = "400" if is_mip else "typically 0.8"
        while voxel_size_z is None:
            try:
                answer = float(input(f"what is the z-step size in um? (hint: {hint} um for the {'MIP' if is_mip else 'main'} images)\n"))
            except ValueError:
                continue
            if 0.001 <= answer <= 1000:
                voxel_size_z = answer
    return voxel_size_x, voxel_size_y, float(voxel_size_z), tile_size


def isotropic_decisions(voxel_size_x, voxel_size_y, voxel_size_z, tile_size, isotropic):
    """(voxel sizes x, y, z after the decision, down_sampling_factor, new_tile_size, voxels were equal): the three branches of
    process_images.py:1163-1190.  z finer than xy: the tiles are enlarged; z coarser: they shrink and the factor is the integer ratio,
    with (1, 1) becoming None; equal: nothing, and the caller warns."""
    factor = new_tile = None
    equal = False
    resized = (int(round(tile_size[0] * voxel_size_y / voxel_size_z, 0)), int(round(tile_size[1] * voxel_size_x / voxel_size_z, 0)))
    if voxel_size_z < voxel_size_x or voxel_size_z < voxel_size_y:
        if isotropic:
            new_tile = resized
            voxel_size_x = voxel_size_y = voxel_size_z
    elif voxel_size_z > voxel_size_x or voxel_size_z > voxel_size_y:
        if isotropic:
            new_tile = resized
            factor = (int(voxel_size_z // voxel_size_y), int(voxel_size_z // voxel_size_x))
            voxel_size_x = voxel_size_y = voxel_size_z
            if factor == (1, 1):
                factor = None
    else:
        equal = True
    return voxel_size_x, voxel_size_y, voxel_size_z, factor, new_tile, equal


def select_channels(needed, channels, message, all_channels):
    """process_images.py:1192-1207: nothing unless ``needed``; the only channel; the named ones, each of which must exist; or all."""
    if not needed:
        return []
    if len(all_channels) == 1 or not channels:
        return list(all_channels)
    for channel in channels:
        if channel not in all_channels:
            _fail(f"{message} channel {channel} is not among {all_channels}")
    return list(channels)


def reorder_list(a, b):
    """``b`` first, then what is left of ``a`` (:279-282)"""
    return list(b) + [c for c in a if c not in b]


def destripe_sigma(objective, need_destriping):
    """sigma of the tile stripe filter (:397-404)"""
    if not need_destriping:
        return (0, 0)
    return {"4x": (100, 100), "40x": (128, 256)}.get(objective, (250, 250))


def stitch_depth(objective, stitch_mip, subvolume_depth):
    """(--sD, --subvoldim) of steps 2-5 (:481-527, :562-564).  The reference starts from ``10 if 40x else min(depth, 100)`` and halves
    that only while it is above 100 (:509-520), so its loops never run: subvoldim is exactly that value, or 1 under --stitch_mip."""
    depth = int(10 if objective == "40x" else min(subvolume_depth, MAX_SUBVOLUME_DEPTH))
    return (0 if objective == "40x" or stitch_mip else 10), (1 if stitch_mip else depth)


def resolve_bleach_wavelet(value):
    """``wavelet=`` of the per-slice stripe filter from --bleach_wavelet: an existing file holds rec_lo (``wavelets.load_file``); a name
    with a built-in table stays a name or becomes its coefficients; any other name goes through PyWavelets when that imports."""
    from . import wavelets
    if os.path.isfile(value):
        return wavelets.load_file(value)
    try:
        found = wavelets.resolve(value)
        return value if found is None else found
    except NotImplementedError:
        pass
    try:
        import pywt
    except ImportError:
        raise NotImplementedError(f"--bleach_wavelet={value!r}: the library holds no table for this name and PyWavelets cannot be imported; "
                                  "give --bleach_wavelet FILE, a file with the wavelet's rec_lo (as pystripe.py --wavelet_file), or a "
                                  "built-in name ('db9', 'haar', 'db1' .. 'db20')") from None
    return wavelets.resolve(pywt.Wavelet(value))


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan

@dataclass
class ChannelPlan:
    """Everything one channel's stages receive, as plain data."""
    channel: str
    channel_for_alignment: str
    color: str
    files_list: list             # of the inspection (None under --skip_inspection)
    subvolume_depth: int
    preprocess: bool             # whether batch_filter runs (:380-382)
    batch_filter: dict           # its keywords (:420-447), input_path and output_path included
    tiles: Path                  # the folder TSVVolume reads as alt_stack_dir
    projects: list               # <channel_for_alignment>_xml_import_step_{1..5}.xml
    steps: list                  # argv of process_images.main for steps 1..5
    tsv: dict                    # TSVVolume(**tsv) (:587-591)
    need_bleach_correction: bool
    need_lightsheet_cleaning: bool
    need_16bit_to_8bit_conversion: bool
    bleach_sigma: tuple          # sigma of the per-slice filter: 2 * min(tile) twice, (0, 0) without bleach correction (:635-643)
    bleach_wavelet: object
    padding_mode: str
    stitched_tif_path: Path
    image_processor: dict        # keywords of parallel_image_processor but source, destination, fun and kwargs (:727-739)
    terafly: dict = None         # terafly.convert(**terafly), or None (:751-774)

    def process_img_kwargs(self, estimate, shape_yx, d_type):
        """The keywords of ``process_img`` (:706-726) from the slice estimates (``estimate_slice_params``), the volume's plane shape and
        its sample type.  ``gpu_semaphore`` is None: there is no queue of devices here."""
        clip_min, clip_med, clip_max = (estimate[f"bleach_correction_clip_{k}"] for k in ("min", "med", "max"))
        return dict(
            sigma=self.bleach_sigma, wavelet=self.bleach_wavelet, padding_mode=self.padding_mode, gpu_semaphore=None,
            bidirectional=bool(self.need_bleach_correction), threshold=clip_med, bleach_correction_frequency=None,
            bleach_correction_clip_min=clip_min, bleach_correction_clip_med=clip_med, bleach_correction_clip_max=clip_max,
            bleach_correction_max_method=False, dark=estimate["dark"], lightsheet=self.need_lightsheet_cleaning, percentile=0.25, rotate=0,
            convert_to_8bit=self.need_16bit_to_8bit_conversion, bit_shift_to_right=estimate["bit_shift_to_right"],
            tile_size=tuple(shape_yx), d_type=d_type)


@dataclass
class AcquisitionPlan:
    args: Namespace
    source_path: Path
    objective: str
    stitch_mip: bool
    all_channels: list           # as found, in the table's order
    order: list                  # as processed: TeraFly channels first, then the reference channel when alignments are shared
    reference_channel: str
    channel_colors: dict
    preprocessed_path: Path
    stitched_path: Path
    composite_path: Path
    downsampled_path: Path
    terafly_path: Path
    log_file: Path
    need_composite_image: bool
    voxel_size_x: float          # after the isotropic decision
    voxel_size_y: float
    voxel_size_z: float
    tile_size: tuple
    down_sampling_factor: tuple
    new_tile_size: tuple
    bleach_correction_channels: list
    background_subtraction_channels: list
    terafly_channels: list
    exclude_gpus: tuple
    channels: list = field(default_factory=list)     # ChannelPlan, in ``order``
    notes: list = field(default_factory=list)        # what planning printed; run() copies it into the log

    def mkdirs(self):
        """the folders the reference makes before it starts (:1090-1148)"""
        return [self.preprocessed_path, self.stitched_path] + ([self.composite_path] if self.need_composite_image else []) + [self.downsampled_path]

    def align_namespace(self, stitched_tif_paths, downsampled_subpaths):
        """The Namespace ``align_images.main`` gets (:1376-1408) from the channels' stitched and down-sampled folders in processing
        order: the folders whose name holds the reference channel's first, at most three channels, ``(None, None)`` for an absent
        one.  A stitched folder keeps its own down-sampled folder."""
        ref = self.reference_channel.lower()
        pairs = list(zip(stitched_tif_paths, downsampled_subpaths))
        pairs = [p for p in pairs if ref in Path(p[0]).name.lower()] + [p for p in pairs if ref not in Path(p[0]).name.lower()]
        pairs = (pairs + [(None, None)] * 3)[:3]
        f = self.down_sampling_factor
        vx, vy, vz = self.voxel_size_x, self.voxel_size_y, self.voxel_size_z
        return Namespace(red=pairs[0], green=pairs[1], blue=pairs[2], output=self.composite_path, write_alignments=True, generate_ims=False,
                         max_iterations=10, reference="red", num_threads=8, save_singles=False, dtype="uint32",
                         dx=(vx, vx * f[0] if f else vx), dy=(vy, vy * f[1] if f else vy), dz=(vz, vz))

    def order_of_colors(self):
        return self.channel_colors[self.reference_channel] + "".join(self.channel_colors[c] for c in self.order if c != self.reference_channel)


def plan(args, rename=False):
    """The decisions of the reference's ``main`` and ``process_channel`` for the parsed options, without a device and without making a
    directory.  ``rename=True`` renames an --input folder whose name holds '-' as the reference does (:1066-1068); the command line
    passes it."""
    notes = []

    def note(text):
        print(text)
        notes.append(str(text))

    if args.imaris:
        raise NotImplementedError(f"--imaris={args.imaris!r}: the Imaris conversion is not built (it needs HDF5); the stitched TIFF series, "
                                  "--terafly_channels and --composite are")
    source_path = Path(args.input)
    if rename and source_path.exists() and "-" in source_path.name:
        source_path = source_path.rename(source_path.parent / source_path.name.replace("-", "_"))
        note("--input path renamed to replace '-' with '_'")
    if not source_path.exists():
        _fail(f"--input path {source_path} does not exist!")
    if not source_path.is_dir():
        _fail(f"--input path {source_path} should be a folder!")
    suffix = "_MIP" if args.stitch_mip else ""
    all_channels = [c + suffix for c, _ in ALL_CHANNELS if source_path.joinpath(c + suffix).exists()]
    if not all_channels:
        _fail(f"could not find unstitched files. --input path should have at least one of these folders {[c + suffix for c, _ in ALL_CHANNELS]}!")
    if not Path(args.tmptif).exists():
        _fail(f"--tmptif path {args.tmptif} does not exist!")
    preprocessed_path = Path(args.tmptif) / (source_path.name + "_tif")
    if not Path(args.stitched).exists():
        _fail(f"--stitched path {args.stitched} does not exist!")
    stitched_path = Path(args.stitched) / (source_path.name + "_stitched")

    need_composite_image = False
    reference_channel = all_channels[0]
    composite_path = Path(args.tmptif)
    if len(all_channels) > 1:
        if args.composite:
            need_composite_image = True
            composite_path = Path(args.composite)
            if not composite_path.exists():
                _fail(f"composite path {composite_path} did not exist.")
            composite_path = composite_path / (source_path.name + "_composite" + suffix)
        if args.reference_channel:
            reference_channel = args.reference_channel
        if reference_channel not in all_channels:
            _fail(f"provided --reference_channel should be among: {all_channels}")
    colors = {c + suffix: color for c, color in ALL_CHANNELS}
    channel_colors = {c: colors[c] for c in all_channels}
    downsampled_path = stitched_path / "Downsampled"
    log_file = stitched_path / ("log_mip.txt" if args.stitch_mip else "log.txt")

    objective = args.objective.lower()
    vx, vy, vz, tile_size = get_voxel_sizes(objective, source_path / all_channels[0], args.stitch_mip, args.tile_size, args.voxel_size_z)
    if not args.stitch_mip:
        assert 1 <= args.voxel_size_target
        assert vx < args.voxel_size_target
        assert vy < args.voxel_size_target
        assert vz < args.voxel_size_target
    vx, vy, vz, factor, new_tile_size, equal = isotropic_decisions(vx, vy, vz, tile_size, args.isotropic)
    if equal:
        note(f"voxel_size_x = {vx}\nvoxel_size_y = {vy}\nvoxel_size_z = {vz}\nmake sure voxel sizes are really equal!")

    bleach = select_channels(args.bleach_correction, args.bleach_correction_channels, "bleach correction", all_channels)
    background = select_channels(args.background_subtraction, args.background_subtraction_channels, "background subtraction", all_channels)
    terafly_channels = select_channels(bool(args.terafly_channels), args.terafly_channels, "terafly conversion", all_channels)
    terafly_path = stitched_path
    if terafly_channels and args.terafly_path:
        terafly_path = Path(args.terafly_path)
        if not terafly_path.exists():
            note(f"--terafly_path {args.terafly_path} does not exits!")
    exclude_gpus = tuple(map(int, args.exclude_gpus))
    if not 0 < args.vram_mem_fraction_gpu0 <= 1:
        _fail("--vram_mem_fraction_gpu0 should be a float between 0 and 1!", ValueError)
    bleach_wavelet = resolve_bleach_wavelet(args.bleach_wavelet) if bleach else args.bleach_wavelet

    order = reorder_list(all_channels, terafly_channels)
    if args.stitch_based_on_reference_channel_alignment:
        order = reorder_list(order, [reference_channel])

    result = AcquisitionPlan(
        args=args, source_path=source_path, objective=objective, stitch_mip=bool(args.stitch_mip), all_channels=all_channels, order=order,
        reference_channel=reference_channel, channel_colors=channel_colors, preprocessed_path=preprocessed_path, stitched_path=stitched_path,
        composite_path=composite_path, downsampled_path=downsampled_path, terafly_path=terafly_path, log_file=log_file,
        need_composite_image=need_composite_image, voxel_size_x=vx, voxel_size_y=vy, voxel_size_z=vz, tile_size=tile_size,
        down_sampling_factor=factor, new_tile_size=new_tile_size, bleach_correction_channels=bleach,
        background_subtraction_channels=background, terafly_channels=terafly_channels, exclude_gpus=exclude_gpus, notes=notes)

    compression = (args.compression_method, args.compression_level) if args.compression_level > 0 else None
    preprocess = bool(args.gaussian or args.de_stripe or args.need_raw_png_to_tiff_conversion or factor not in (None, (1, 1))
                      or new_tile_size is not None)
    tiles_root = preprocessed_path if preprocess else source_path   # without the stage the stitch reads the source folder
    swap = objective == "40x"
    s_d, subvoldim_of = None, None
    for channel in order:
        files, depth = inspect_for_missing_tiles_get_files_list(source_path / channel, skip=args.skip_inspection, log=note)
        if files is not None and preprocess:
            files = files + missing_slices(files)
        for_alignment = reference_channel if args.stitch_based_on_reference_channel_alignment else channel
        batch = dict(
            input_path=source_path / channel, output_path=preprocessed_path / channel, files_list=files, workers=args.nthreads,
            continue_process=args.resume, print_input_file_names=False, timeout=args.timeout, gaussian_filter_2d=args.gaussian,
            bleach_correction_frequency=None, bleach_correction_max_method=False, sigma=destripe_sigma(objective, args.de_stripe), level=0,
            wavelet="db9", crossover=10, threshold=None, padding_mode="reflect", bidirectional=True, lightsheet=False, down_sample=factor,
            tile_size=tile_size, new_size=new_tile_size, d_type="uint16", convert_to_8bit=False, bit_shift_to_right=8,
            compression=compression, threads_per_gpu=8)
        projects = [stitched_path / f"{for_alignment}_xml_import_step_{k}.xml" for k in range(1, 6)]
        s_d, subvoldim = stitch_depth(objective, args.stitch_mip, depth)
        steps = [["-1", f"--ref1={'V' if swap else 'H'}", f"--ref2={'H' if swap else 'V'}", "--ref3=D",
                  f"--vxl1={vy if swap else vx:.3f}", f"--vxl2={vx if swap else vy:.3f}", f"--vxl3={vz}", "--sparse_data",
                  f"--volin={tiles_root / for_alignment}", f"--projout={projects[0]}", "--noprogressbar"]]
        for k in (2, 3, 4, 5):
            steps.append([f"-{k}", f"--sD={s_d}", f"--subvoldim={subvoldim}", f"--threshold={STITCH_THRESHOLD}",
                          f"--projin={projects[k - 2]}", f"--projout={projects[k - 1]}"])
        need_bleach = channel in bleach
        sigma = (0, 0)
        if need_bleach:   # (:635-640; a factor is only ever set together with a new tile size, so the middle branch there is dead)
            sigma = (int(min(new_tile_size if new_tile_size is not None else tile_size) * 2),) * 2
        stitched_tif_path = stitched_path / f"{channel}_tif"
        processor = dict(
            source_voxel=(vz, vy, vx), target_voxel=None if args.stitch_mip else args.voxel_size_target, downsampled_path=downsampled_path,
            rotation=90 if args.rot90 else 0, timeout=args.timeout, max_processors=args.nthreads, progress_bar_name="TSV",
            compression=compression, resume=args.resume, needed_memory=None, return_downsampled_path=True,
            # align_images composes integer channels only: the planes it will read are written as uint16, which holds the processed
            # slices' 8 or 16 bits; without a composite they are the reference's float32
            down_sampled_dtype=COMPOSITE_PLANE_DTYPE if need_composite_image else "float32")
        terafly = None
        if channel in terafly_channels:
            terafly = dict(src=stitched_tif_path, dst=terafly_path / f"{channel}_TeraFly", resolutions=TERAFLY_RESOLUTIONS, halve=TERAFLY_HALVE)
        result.channels.append(ChannelPlan(
            channel=channel, channel_for_alignment=for_alignment, color=channel_colors[channel], files_list=files, subvolume_depth=depth,
            preprocess=preprocess, batch_filter=batch, tiles=tiles_root / channel, projects=projects, steps=steps,
            tsv=dict(tree_xml_path=projects[4], alt_stack_dir=str(tiles_root / channel), cosine_blending=args.cosine_blending),
            need_bleach_correction=need_bleach, need_lightsheet_cleaning=channel in background,
            need_16bit_to_8bit_conversion=bool(args.convert_to_8bit), bleach_sigma=sigma, bleach_wavelet=bleach_wavelet,
            padding_mode=args.padding_mode, stitched_tif_path=stitched_tif_path, image_processor=processor, terafly=terafly))
    return result


def summary(p):
    """the text the reference prints and logs before it starts (:1243-1284)"""
    a = p.args
    return (
        f"{_now()}:  stitching started"
        f"\n\tRun on computer: {platform.node()}"
        f"\n\tLogical CPU core count: {os.cpu_count()}"
        f"\n\tRequested CPU core count: {a.nthreads}"
        f"\n\tcompression: {(a.compression_method, a.compression_level)}"
        f"\n\tSource folder path:\n\t\t{p.source_path}"
        f"\n\t\tChannels: {p.all_channels}"
        f"\n\t\tObjective: {p.objective}"
        f"\n\t\ttile size: {p.tile_size}"
        f"\n\t\tVoxel size x: {p.voxel_size_x} um"
        f"\n\t\tVoxel size y: {p.voxel_size_y} um"
        f"\n\t\tVoxel size z: {p.voxel_size_z} um"
        f"\n\tPreprocessed folder path:\n\t\t{p.preprocessed_path}"
        f"\n\t\tpreprocessing, gaussian: {a.gaussian}"
        f"\n\t\tpreprocessing, down sampling factors (y, x): {p.down_sampling_factor}"
        f"\n\t\tpreprocessing, new tile size (y, x): {p.new_tile_size}"
        f"\n\t\tpreprocessing, tile destriping: {a.de_stripe}"
        f"\n\t\tpreprocessing, tif conversion: {a.need_raw_png_to_tiff_conversion}"
        f"\n\tStitched folder path:\n\t\t{p.stitched_path}"
        f"\n\t\tpostprocessing, bleach correction: {a.bleach_correction}"
        f"\n\t\tpostprocessing, bleach correction channels: {p.bleach_correction_channels}"
        f"\n\t\tpostprocessing, bleach correction padding mode: {a.padding_mode}"
        f"\n\t\tpostprocessing, bleach correction wavelet: {a.bleach_wavelet}"
        f"\n\t\tpostprocessing, background subtraction: {a.background_subtraction}"
        f"\n\t\tpostprocessing, background subtraction channels: {p.background_subtraction_channels}"
        f"\n\t\tpostprocessing, conversion to 8-bit: {a.convert_to_8bit}"
        f"\n\t\tpostprocessing, 90 degree rotation: {a.rot90}"
        f"\n\tTerafly path:\n\t\t{p.terafly_path}"
        f"\n\t\tChannels need terafly conversion: {p.terafly_channels}"
        f"\n\tComposite folder path:\n\t\t{p.composite_path}"
        f"\n\t\tReference channel:{p.reference_channel}"
        f"\n\t\tChannel colors:{p.channel_colors}"
        f"\n\tDownsampled path:\n\t\t{p.downsampled_path}"
        f"\n\tImaris conversion: False"
        f"\n\ttimeout: {a.timeout}"
        f"\n\tresume: {a.resume}"
        f"\n\tskipconf: {a.skipconf}")


# ---------------------------------------------------------------------------------------------------------------------------------
# execution

class _Log:
    """prints, and writes the same text to the log file (rewritten by every run, :1150-1152)"""

    def __init__(self, path):
        self.handle = open(path, "w")

    def __call__(self, text):
        text = str(text)
        print(text)
        self.handle.write(text + "\n")
        self.handle.flush()

    def close(self):
        self.handle.close()


def pick_device(exclude_gpus, count):
    """Index of the first device not in ``exclude_gpus``; an excluded index the host lacks is the reference's RuntimeError (:1228-1233)."""
    for gpu in exclude_gpus:
        if gpu not in range(count):
            _fail(f"--exclude_gpus: {gpu} is not a valid gpu index. Choose among {range(count)}")
    for gpu in range(count):
        if gpu not in exclude_gpus:
            return gpu
    _fail(f"--exclude_gpus: {list(exclude_gpus)} leaves none of the {count} devices")


def terafly_resolutions(shape, wanted=TERAFLY_RESOLUTIONS):
    """The leading levels of ``wanted`` that ``terafly.plan`` admits for a series of ``shape`` (z, y, x).  The reference always asks for
    "012345", which its converter refuses for a volume of fewer than 64 slices (level k needs 2^k slices in half a block of the
    depth); a shallow acquisition, a MIP among them, then gets the pyramid it can hold.  With one level left, the stage's own refusal
    is raised."""
    from . import terafly
    while len(wanted) > 1:
        try:
            terafly.plan(tuple(int(v) for v in shape), wanted)
            break
        except ValueError:
            wanted = wanted[:-1]
    return wanted


def _run_channel(p, c, device, log):
    from . import process_images, pystripe, terafly, thresholds
    from .parallel_image_processor import parallel_image_processor
    from .tsv import TSVVolume
    a = p.args
    assert (p.source_path / c.channel).exists()
    assert p.downsampled_path.exists()
    if c.preprocess:
        k = c.batch_filter
        log(f"{_now()}: {c.channel}: started preprocessing tile images and converting them to tif.\n"
            f"\tsource: {k['input_path']}\n\tdestination: {k['output_path']}\n\tcompression: {k['compression']}\n"
            f"\tgaussian: {k['gaussian_filter_2d']}\n\ttile de-striping sigma: {k['sigma']}\n\ttile size: {k['tile_size']}\n"
            f"\tdown sampling factor on xy-plane: {k['down_sample']}\n\tresizing target on xy-plane: {k['new_size']}")
        rc = pystripe.batch_filter(device=device, **k)
        if rc != 0:
            return rc, None, None, None
    inspect_for_missing_tiles_get_files_list(c.tiles, log=log)

    if not c.projects[4].exists() or not a.resume:
        log(f"{_now()}: {c.channel_for_alignment}: aligning tiles ...")
        for k, argv in enumerate(c.steps, start=1):
            log(f"\tstep {k}: process_images.py " + " ".join(argv))
            if k > 1:
                assert c.projects[k - 2].exists()
            rc = process_images.main(list(argv))
            if rc != 0:
                return rc, None, None, None
            if not c.projects[k - 1].exists():
                _fail(f"{c.channel_for_alignment}: step {k} of stitching wrote no project file.")
            if k > 1:
                c.projects[k - 2].unlink()

    c.stitched_tif_path.mkdir(exist_ok=True)
    volume = TSVVolume(device=device, **c.tsv)
    shape = tuple(volume.volume.shape)   # z, y, x
    estimate = thresholds.estimate_slice_params(volume, need_bleach_correction=c.need_bleach_correction,
                                                need_16bit_to_8bit_conversion=c.need_16bit_to_8bit_conversion, device=device)
    kwargs = c.process_img_kwargs(estimate, shape[1:3], volume.dtype)
    shown = {k: v for k, v in kwargs.items() if k != "wavelet"}
    log(f"{_now()}: {c.channel}: merging tiles into 2D tif series and postprocessing the stitched images ...\n"
        f"\tsource: {c.tsv['tree_xml_path']}\n\ttiles: {c.tsv['alt_stack_dir']}\n\tdestination: {c.stitched_tif_path}\n"
        f"\ttsv volume shape (zyx): {shape}\n\ttsv volume data type: {volume.dtype.__name__}\n\tslices of the estimates: {list(estimate.slices)}\n"
        f"\tper-slice keywords: {shown}\n\trotate: {c.image_processor['rotation']}")
    rc, downsampled_subpath = parallel_image_processor(source=volume, destination=c.stitched_tif_path, fun=pystripe.process_img,
                                                       kwargs=dict(kwargs, extended=True), **c.image_processor)
    if c.image_processor["rotation"]:
        shape = (shape[0], shape[2], shape[1])
    if rc != 0:
        return rc, None, None, None

    if c.terafly is not None:
        Path(c.terafly["dst"]).mkdir(exist_ok=True)
        resolutions = terafly_resolutions(shape, c.terafly["resolutions"])
        log(f"{_now()}: {c.channel}: starting to convert to TeraFly format ...\n\tsource: {c.terafly['src']}\n\tdestination: {c.terafly['dst']}\n"
            f"\tresolutions: {resolutions}" + ("" if resolutions == c.terafly["resolutions"] else
                                               f" (of {c.terafly['resolutions']}: a volume of {shape} holds no more levels)"))
        terafly.convert(device=device, **dict(c.terafly, resolutions=resolutions))
    return 0, c.stitched_tif_path, shape, downsampled_subpath


def run(p, device=None):
    """Executes the plan in this process, in the reference's order.  ``device``: a device index or torch device (default: the first one
    not in --exclude_gpus).  Returns 0, or the first non-zero code of a stage."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError(f"WORLD_SIZE={os.environ['WORLD_SIZE']}: the acquisition driver runs in one process; the stages' rank modes "
                           "(torchrun) are not composed here")
    import torch
    from . import capi
    capi.require_gpu()
    if device is None:
        device = pick_device(p.exclude_gpus, torch.cuda.device_count())
    device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    index = device.index or 0
    for folder in p.mkdirs():
        folder.mkdir(exist_ok=True)
    probe = p.terafly_path / "test"   # the reference's check that the TeraFly folder can be written (:1225-1226)
    probe.touch(exist_ok=False)
    probe.unlink()
    a = p.args
    log = _Log(p.log_file)
    # the per-slice pass and step 2 work on the device LOCAL_RANK names: it is set for the length of the run
    before = os.environ.get("LOCAL_RANK")
    os.environ["LOCAL_RANK"] = str(index)
    try:
        with torch.cuda.device(device):
            for text in p.notes:
                log.handle.write(text + "\n")
            log(summary(p))
            log(f"\tdevice: {device}")
            for name in IGNORED_OPTIONS:
                log(f"\t--{name}={getattr(a, name)}: accepted and ignored")
            if not a.skipconf:
                input("press enter to continue if everything is OK ... ")
            start = time.time()
            stitched_tif_paths, shapes, downsampled_subpaths = [], [], []
            for c in p.channels:
                rc, stitched_tif_path, shape, downsampled_subpath = _run_channel(p, c, device, log)
                if rc != 0:
                    return rc
                stitched_tif_paths.append(stitched_tif_path)
                shapes.append(shape)
                downsampled_subpaths.append(downsampled_subpath)
            if shapes.count(shapes[0]) != len(shapes):
                log("warning: channels had different shapes:\n\t" + "\n\t".join(
                    f"channel {c}: volume shape={s}" for c, s in zip(p.order, shapes)))
            if p.need_composite_image and len(stitched_tif_paths) > 1:
                from . import align_images
                log(f"{_now()}: merging channels to composite RGB started ...\n\ttime elapsed so far {timedelta(seconds=time.time() - start)}")
                if len(stitched_tif_paths) >= 4:
                    log("Warning: since number of channels are more than 3 merging the first 3 channels only.")
                namespace = p.align_namespace(stitched_tif_paths, downsampled_subpaths)
                log(f"\talign_images: {namespace}")
                align_images.main(namespace)
            log(f"\n{_now()}: done.\n\tTime elapsed: {timedelta(seconds=time.time() - start)}")
    finally:
        log.close()
        if before is None:
            os.environ.pop("LOCAL_RANK", None)
        else:
            os.environ["LOCAL_RANK"] = before
    return 0


def main(argv=None):
    return run(plan(build_parser().parse_args(argv), rename=True))


if __name__ == "__main__":
    sys.exit(main())
