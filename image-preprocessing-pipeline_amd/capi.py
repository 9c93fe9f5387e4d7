"""ctypes binding of libmi_ipp.so (the C ABI declared in include/*.h).

This is the only door between the Python host code and the HIP kernels.  There is no CPU fallback:
if the shared library is missing or a symbol is absent, importing ``lib()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI_IPP_PROBES=1 (profiles/ only): the build with the experiment switches compiled in (make -C csrc probes)
LIB_PATH = os.path.join(_HERE, "libmi_ipp_probes.so" if os.environ.get("MI_IPP_PROBES") == "1" else "libmi_ipp.so")

MI_OK = 0
IPC_HANDLE_BYTES = 64  # MI_IPC_HANDLE_BYTES
# mi_boundary / mi_engine (include/mi_lsdeconv.h)
BOUNDARY_ZERO, BOUNDARY_REPLICATE, BOUNDARY_CIRCULAR = 0, 1, 2
ENGINE_AUTO, ENGINE_DIRECT, ENGINE_FFT = 0, 1, 2
NORTH_SOUTH, WEST_EAST = 0, 1
SINBLEND, NOBLEND = 0, 1   # mi_blending (include/mi_stitch.h)
HALVE_MEAN, HALVE_MAX = 0, 1   # mi_halve_method (include/mi_pyramid.h)
PS_U8, PS_U16, PS_F32 = 0, 1, 2   # mi_pystripe_dtype (include/mi_pystripe.h)
# mi_pystripe_padding: four index maps, then the value modes (PS_VALUE_PADDING; the Python layer takes them with extended=True)
PS_PADDING = {"reflect": 0, "wrap": 1, "symmetric": 2, "edge": 3, "constant": 4, "linear_ramp": 5, "maximum": 6, "mean": 7, "median": 8,
              "minimum": 9}
PS_VALUE_PADDING = ("constant", "linear_ramp", "maximum", "mean", "median", "minimum")
PS_DOWN = {"max": 0, "min": 1, "mean": 2, "median": 3}   # mi_pystripe_down
PS_MEDIAN_MAX_BLOCK = 64  # MI_PS_MEDIAN_MAX_BLOCK
PS_NOTCH_ROUTE = ("pass", "level", "axis", "n", "kp", "kb", "R", "threads", "lds")   # a record of mi_pystripe_plan_notch_routes
PS_AUTO_MIN, PS_AUTO_MED, PS_AUTO_MAX = 1, 2, 4   # bits of PystripeParams.bleach_auto (MI_PS_AUTO_*)
PS_CLIPS_UNIFORM, PS_CLIPS_OK, PS_CLIPS_TOO_FEW, PS_CLIPS_ORDER, PS_CLIPS_NONFINITE = -1, 0, 1, 2, 3   # mi_pystripe_clip_status
CODES_U8, CODES_U16 = 0, 1   # mi_code_dtype (include/mi_thresholds.h)
OTSU_OK, OTSU_TOO_FEW_VALUES, OTSU_VALUES_ARE_CLASSES = 0, 1, 2   # mi_otsu_status


MI_ERR_INVALID, MI_ERR_HIP, MI_ERR_FFT, MI_ERR_NOMEM, MI_ERR_UNSUPPORTED, MI_ERR_INTERNAL = -1, -2, -3, -4, -5, -6  # include/mi_common.h


class MiError(RuntimeError):
    """A C-ABI call returned a negative mi_status; the message is mi_last_error()."""

    def __init__(self, code: int, message: str):
        super().__init__(f"[mi_status {code}] {message}")
        self.code = code


class RlOptions(C.Structure):
    """mi_rl_options (include/mi_lsdeconv.h)."""
    _fields_ = [("niter", C.c_int), ("lambda_", C.c_float), ("stop_criterion", C.c_float),
                ("regularize_interval", C.c_int), ("engine", C.c_int), ("skip_edgetaper", C.c_int),
                ("gauss_taps", C.c_int), ("psf_grid", C.c_int * 3)]


class NccParams(C.Structure):
    """mi_ncc_params == NCC_parms_t without the enhance tables (CrossMIPs.h:65-86)."""
    _fields_ = [("enhance", C.c_int), ("maxIter", C.c_int), ("maxThr", C.c_float), ("widthThr", C.c_float),
                ("wRangeThr_i", C.c_int), ("wRangeThr_j", C.c_int), ("wRangeThr_k", C.c_int),
                ("minPoints", C.c_int), ("minDim_NCCsrc", C.c_int), ("minDim_NCCmap", C.c_int),
                ("UNR_NCC", C.c_float), ("INF_W", C.c_int), ("INV_COORD", C.c_int)]


class NccDescr(C.Structure):
    """mi_ncc_descr == NCC_descr_t (CrossMIPs.h:58-62)."""
    _fields_ = [("coord", C.c_int * 3), ("NCC_maxs", C.c_float * 3), ("NCC_widths", C.c_int * 3)]


class PystripeParams(C.Structure):
    """mi_pystripe_params (include/mi_pystripe.h)."""
    _fields_ = [("sigma1", C.c_double), ("sigma2", C.c_double), ("level", C.c_int), ("padding_mode", C.c_int),
                ("bidirectional", C.c_int), ("down_y", C.c_int), ("down_x", C.c_int), ("down_method", C.c_int),
                ("use_flat", C.c_int), ("dark", C.c_float), ("convert_to_16bit", C.c_int), ("convert_to_8bit", C.c_int),
                ("bit_shift", C.c_int), ("out_dtype", C.c_int), ("flip_upside_down", C.c_int), ("rotate", C.c_int),
                ("log_output", C.c_int), ("max_batch", C.c_int), ("keep_uniform", C.c_int), ("bleach_frequency", C.c_double),
                ("bleach_clip_min", C.c_double), ("bleach_clip_med", C.c_double), ("bleach_clip_max", C.c_double),
                ("bleach_max_method", C.c_int)]

    @property
    def bleach_auto(self):
        """PS_AUTO_* bits of the clips that are NaN: those the plan estimates per tile (0 without a bleach_frequency)"""
        if not self.bleach_frequency:
            return 0
        clips = (self.bleach_clip_min, self.bleach_clip_med, self.bleach_clip_max)
        return sum(bit for bit, v in zip((PS_AUTO_MIN, PS_AUTO_MED, PS_AUTO_MAX), clips) if v != v)


PS_MAX_LEVELS = 24  # MI_PS_MAX_LEVELS
PS_MAX_TAPS = 128  # MI_PS_MAX_TAPS
PS_BLEACH_LDS_ROW = 20436  # MI_PS_BLEACH_LDS_ROW
PS_PAD_LDS_LINE = 9968  # MI_PS_PAD_LDS_LINE


class PystripeInfo(C.Structure):
    """mi_pystripe_info (include/mi_pystripe.h)."""
    _fields_ = [("ny", C.c_int), ("nx", C.c_int), ("base_pad", C.c_int), ("pad_y", C.c_int), ("pad_x", C.c_int),
                ("padded_ny", C.c_int), ("padded_nx", C.c_int), ("levels", C.c_int), ("coef_ny", C.c_int * PS_MAX_LEVELS),
                ("coef_nx", C.c_int * PS_MAX_LEVELS), ("out_ny", C.c_int), ("out_nx", C.c_int), ("out_dtype", C.c_int),
                ("integer_kind", C.c_int), ("max_batch", C.c_int), ("scratch_bytes_per_tile", C.c_size_t), ("bleach_long_rows", C.c_int)]


class LightsheetParams(C.Structure):
    """mi_lightsheet_params (include/mi_lightsheet.h)."""
    _fields_ = [("artifact_length", C.c_int), ("artifact_along_y", C.c_int), ("background_window_size", C.c_int), ("background_spacing", C.c_int),
                ("background_step", C.c_int), ("percentile", C.c_double), ("lightsheet_vs_background", C.c_double),
                ("factor_is_integer", C.c_int), ("map_dtype", C.c_int), ("max_batch", C.c_int)]


class LightsheetInfo(C.Structure):
    """mi_lightsheet_info (include/mi_lightsheet.h)."""
    _fields_ = [(name, C.c_int) for name in (
        "ny", "nx", "ls_ny", "ls_nx", "ls_left_y", "ls_left_x", "bg_ny", "bg_nx", "bg_left_y", "bg_left_x", "bg_first_y0", "bg_first_y1", "bg_last_y0",
        "bg_last_y1", "bg_first_x0", "bg_first_x1", "bg_last_x0", "bg_last_x1", "max_window_samples", "ls_zero_last_row", "ls_zero_last_col",
        "bg_zero_last_row", "bg_zero_last_col", "integer_mode", "max_batch")] + [("scratch_bytes_per_tile", C.c_size_t)]


class TileMaskInfo(C.Structure):
    """mi_tile_mask_info (include/mi_tile_mask.h)."""
    _fields_ = [("scratch_bytes", C.c_size_t), ("max_batch", C.c_int), ("fill_rounds", C.c_int)]


ISO_MAX_STEPS = 32  # MI_ISO_MAX_STEPS


class FftRoute(C.Structure):
    """mi_fft_route (include/mi_lsdeconv.h)"""
    _fields_ = [(name, C.c_int) for name in ("native", "paired", "z_kernel", "real_otf", "x_pipelined", "x_splits", "x_dynamic", "z_dynamic",
                                              "pruned", "ty", "tc", "tl", "z_full_grid")]


class IsodownParams(C.Structure):
    """mi_isodown_params (include/mi_isodown.h)."""
    _fields_ = [("voxel_y", C.c_double), ("voxel_x", C.c_double), ("target_voxel", C.c_double), ("alternating", C.c_int),
                ("z_rounds", C.c_int), ("out_dtype", C.c_int), ("max_group", C.c_int)]


class IsodownInfo(C.Structure):
    """mi_isodown_info (include/mi_isodown.h)."""
    _fields_ = [("ny", C.c_int), ("nx", C.c_int), ("target_ny", C.c_int), ("target_nx", C.c_int), ("rounds_y", C.c_int),
                ("rounds_x", C.c_int), ("nsteps", C.c_int), ("step_axis", C.c_int * ISO_MAX_STEPS), ("step_method", C.c_int * ISO_MAX_STEPS),
                ("step_extent", C.c_int * ISO_MAX_STEPS), ("ky", C.c_int), ("kx", C.c_int), ("halved_ny", C.c_int), ("halved_nx", C.c_int),
                ("sigma_y", C.c_double), ("sigma_x", C.c_double), ("radius_y", C.c_int), ("radius_x", C.c_int), ("taps_y", C.c_int),
                ("taps_x", C.c_int), ("tile_ny", C.c_int), ("tile_nx", C.c_int), ("lds_steps", C.c_int), ("scratch_bytes_per_slice", C.c_size_t)]


ECC_NSUMS, ECC_SCRATCH_BYTES, ECC_DEFAULT_BATCH = 16, 1024 * 16 * 8, 32   # MI_ECC_NSUMS, MI_ECC_SCRATCH_BYTES, MI_ECC_DEFAULT_BATCH
ECC_OK, ECC_NAN, ECC_MINIMIZED = 0, 1, 2   # mi_ecc_status
ECC_SUM_NAMES = ("n", "sw", "sww", "st", "stt", "swt", "hxx", "hxy", "hyy", "gxw", "gyw", "mgx", "mgy", "gxt", "gyt")   # mi_ecc_sum
RGB_U8, RGB_U16, RGB_U32, RGB_F32 = 1, 2, 3, 4   # mi_rgb_dtype; also the dtype of mi_tiff_write_rgb_series


class EccState(C.Structure):
    """mi_ecc_state (include/mi_align.h)."""
    _fields_ = [("tx", C.c_double), ("ty", C.c_double), ("rho", C.c_double), ("rho_last", C.c_double), ("iteration", C.c_int),
                ("status", C.c_int), ("done", C.c_int), ("reserved", C.c_int)]


class CompositeChannel(C.Structure):
    """mi_composite_channel (include/mi_align.h)."""
    _fields_ = [("src", C.c_void_p), ("count", C.c_int), ("first", C.c_int), ("ny", C.c_int), ("nx", C.c_int), ("dz", C.c_int),
                ("dy", C.c_int), ("dx", C.c_int), ("reserved", C.c_int)]


class Tiff3dJob(C.Structure):
    """mi_tiff3d_job (include/mi_tiff3d.h): pages [p0, p1) x rows [y0, y1) x columns [x0, x1) of a block file land at (oz, oy, ox) of the box."""
    _fields_ = [("path", C.c_char_p)] + [(name, C.c_int) for name in ("p0", "p1", "y0", "y1", "x0", "x1", "oz", "oy", "ox")]


LZW_OK, LZW_CODE, LZW_FIRST, LZW_INPUT, LZW_OUTPUT, LZW_OLD_STYLE, LZW_TABLE = range(7)   # mi_lzw_status (include/mi_tiff3d.h)

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_ip = C.POINTER(C.c_int)

# name -> (restype, argtypes); every symbol declared in include/*.h
SIGNATURES = {
    # mi_common.h
    "mi_last_error": (C.c_char_p, []),
    "mi_device_count": (_i, []),
    "mi_abi_version": (_i, []),
    "mi_stream_synchronize": (_i, [_i, _vp]),
    # mi_lsdeconv.h
    "mi_conv3d_replicate": (_i, [_i, _vp, _vp, _vp, _vp] + [_i] * 6),
    "mi_conv3d": (_i, [_i, _vp, _vp, _vp, _vp] + [_i] * 8),
    "mi_gauss3d_inplace": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, C.POINTER(C.c_float), _ip]),
    "mi_gauss3d_route": (_i, [_i, _i, _i, C.POINTER(C.c_float), _ip]),
    "mi_edgetaper3d": (_i, [_i, _vp, _vp, _vp, _vp] + [_i] * 6),
    "mi_otf": (_i, [_i, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _f]),
    "mi_u16_to_f32": (_i, [_i, _vp, _vp, _vp, _sz, _f]),
    "mi_subtract_dark": (_i, [_i, _vp, _vp, _vp, _sz, _f]),
    "mi_norm2": (_i, [_i, _vp, _vp, _sz, C.POINTER(C.c_double)]),
    "mi_release_cached_memory": (_sz, [_i]),
    "mi_cached_memory_bytes": (_sz, []),
    "mi_rl_fuses": (_i, [_vp]),
    "mi_rl_otf_is_real": (_i, [_vp]),
    "mi_rl_otf_form": (_i, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mi_rl_fft_route": (_i, [_vp, C.POINTER(FftRoute)]),
    "mi_rl_sharded_begin": (_i, [_vp, _vp, _vp]),
    "mi_rl_sharded_ratio": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_int)]),
    "mi_rl_sharded_update": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(C.c_int)]),
    "mi_rl_spectrum_rows": (_i, [_vp, _vp, _i, _i, _vp, _i]),
    "mi_rl_spectrum_row_floats": (_sz, [_vp]),
    "mi_rl_sharded_stage": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "mi_rl_spectrum_rows_z": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i]),
    "mi_rl_z_granule": (_i, [_vp]),
    "mi_rl_set_overlap": (_i, [_vp, _i, _i]),
    "mi_rl_overlap_probe": (_i, [_vp, _vp, _vp, _ip, _i, _f, _i, C.POINTER(C.c_float)]),
    "mi_prctile": (_i, [_i, _vp, _vp, _sz, C.POINTER(C.c_double), _i, C.POINTER(C.c_float)]),
    "mi_rescale_block": (_i, [_i, _vp, _vp, _vp, _sz, _i, _f, _f, _f, _f]),
    "mi_pad_center": (_i, [_i, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i]),
    "mi_crop_center": (_i, [_i, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i]),
    "mi_rl_create": (_i, [_i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "mi_rl_create_ex": (_i, [_i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _ip, _ip, _i, C.POINTER(_vp)]),
    "mi_rl_destroy": (_i, [_vp]),
    "mi_rl_engine": (_i, [_vp]),
    "mi_rl_separable": (_i, [_vp]),
    "mi_rl_sep_route": (_i, [_vp, _i, _ip]),
    "mi_rl_pair_layout": (_i, [_vp]),
    "mi_rl_device_bytes": (_sz, [_vp]),
    "mi_rl_forward_ratio": (_i, [_vp, _vp, _vp, _vp]),
    "mi_rl_adjoint_update": (_i, [_vp, _vp, _vp, _vp, _f, _vp]),
    "mi_rl_iterate": (_i, [_vp, _vp, _vp, _vp, _i]),
    "mi_rl_time_pass": (_i, [_vp, _vp, _i, _vp, _i, C.POINTER(C.c_float)]),
    "mi_rl_fft_spectrum_bytes": (_sz, [_vp]),
    "mi_rl_time_between": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, C.POINTER(C.c_float)]),
    "mi_rl_fft_placement": (_i, [_vp, C.POINTER(C.c_float), _i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mi_rl_reg_term": (_i, [_i, _vp, _vp, _vp, _i, _i, _i]),
    "mi_rl_spatial": (_i, [_i, _vp, _vp, _vp, _vp] + [_i] * 6 + [C.POINTER(RlOptions), _ip]),
    "mi_rl_fft": (_i, [_i, _vp, _vp, _vp] + [_i] * 9 + [C.POINTER(RlOptions), _ip]),
    "mi_rl_fft_wiener": (_i, [_i, _vp, _vp, _vp] + [_i] * 9 + [C.POINTER(RlOptions), _ip]),
    "mi_decon_plan_create": (_i, [_i, C.POINTER(_vp)]),
    "mi_decon_plan_run": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 6 + [C.POINTER(RlOptions), _i, _ip, _i, _ip]),
    "mi_decon_plan_destroy": (_i, [_vp]),
    "mi_load_block": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _vp] + [_i] * 6),
    "mi_destripe_z": (_i, [_i, _vp, _vp, _i, _i, _i, _f, _i]),
    "mi_destripe_max_levels": (_i, [_i, _i]),
    "mi_decon": (_i, [_i, _vp, _vp, _vp, _vp] + [_i] * 6 + [C.POINTER(RlOptions), _i, _ip, _i, _ip]),
    "mi_engine_select": (_i, [_i] * 7),
    "mi_next_fast_len": (_i, [_i]),
    "mi_fft_good_size": (_i, [_i, _i]),
    "mi_pack_rows": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mi_unpack_rows": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mi_tiff_codec": (C.c_char_p, []),
    "mi_tiff_info": (_i, [C.c_char_p, _ip, _ip, _ip, _ip]),
    "mi_tiff_read_box": (_i, [C.POINTER(C.c_char_p), _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i]),
    "mi_tiff_write_series": (_i, [C.POINTER(C.c_char_p), _i, _vp, _i, _i, _i, _i, _i, _i, _ip]),
    "mi_tiff_write_rgb_series": (_i, [C.POINTER(C.c_char_p), _i, _vp, _i, _i, _i, _i, _i, _i, _ip]),
    "mi_tiff_write_series_device":(_i, [_i, _vp, C.POINTER(C.c_char_p), _i, _vp, _i, _i, _i, _i, _ip]),
    "mi_tiff_read_box_device": (_i, [_i, _vp, C.POINTER(C.c_char_p), _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i]),
    "mi_peer_link_create": (_i, [_i, _sz, C.POINTER(_vp), C.c_char_p, C.c_char_p]),
    "mi_peer_link_connect": (_i, [_vp, _i, C.c_char_p, C.c_char_p, _i]),
    "mi_peer_link_begin": (_i, [_vp, _vp, C.c_uint, _i]),
    "mi_peer_link_send": (_i, [_vp, _vp, C.c_uint, _i, _i, _sz, _sz, _vp, _vp]),
    "mi_peer_link_recv": (_i, [_vp, _vp, C.c_uint, _i, _i, _i, C.POINTER(_vp)]),
    "mi_peer_exchange": (_i, [_vp, _vp, C.c_uint, _i, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "mi_peer_link_status": (_i, [_vp, C.POINTER(_i)]),
    "mi_peer_link_disconnect": (_i, [_vp]),
    "mi_peer_link_destroy": (_i, [_vp]),
    # mi_stitch.h
    "mi_merge_volume_dims": (_i, [_i, _i, _ip, _ip, _ip, _i, _i, _i, _ip]),
    "mi_merge_slab": (_i, [_i, _vp, _i, _i, _ip, _ip, _ip, _i, _i, _i, C.POINTER(_vp), _i, _i] + [_i] * 6 + [_vp]),
    # mi_tsv.h
    "mi_tsv_place": (_i, [_i, _i, _ip, _ip, _i, _ip, _i, _i, _ip, _ip, _ip, _ip]),
    "mi_tsv_merge": (_i, [_i, _vp, _i, _ip, _ip, _ip, _ip, _i, _i, C.POINTER(_vp), _i, _i] + [_i] * 6 + [_vp]),
    # mi_pyramid.h
    "mi_pyramid_slab": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _i, _i, _ip, C.POINTER(_vp)]),
    "mi_tiff3d_write_blocks": (_i, [_i, C.POINTER(C.c_char_p), C.POINTER(_vp), C.POINTER(C.c_int64), _ip, _ip, _ip, _i, _i, _i, _i,
                                    _i]),
    "mi_tiff_deflate_strip_host": (_i, [_vp, C.c_size_t, _i, C.c_size_t, _i, _i, _vp, C.c_size_t, C.POINTER(C.c_size_t), _ip]),
    "mi_tiff_lzw_encode": (_i, [_vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "mi_tiff_lzw_encode_strips_device": (_i, [_i, _vp, C.c_int64, C.POINTER(_vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int64), _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "mi_tiff3d_write_blocks_device": (_i, [_i, _vp, _i, C.POINTER(C.c_char_p), C.POINTER(_vp), C.POINTER(C.c_int64), _ip, _ip, _ip, _i, _i, _i,
                                           _i, _i]),
    "mi_tiff3d_write_blocks_encoded": (_i, [_i, C.POINTER(C.c_char_p), _ip, _ip, _ip, _i, _i, _i, C.POINTER(_vp), C.POINTER(C.c_int64), _i]),
    "mi_tiff_lzw_encode_device_batches": (C.c_int64, []),
    # mi_tiff3d.h
    "mi_tiff3d_info": (_i, [C.c_char_p] + [_ip] * 7),
    "mi_tiff_lzw_decode": (_i, [_vp, C.c_int64, _vp, C.c_int64, _ip]),
    "mi_tiff3d_read_box": (_i, [C.POINTER(Tiff3dJob), _i, _i, _i, _i, _i, _vp, _i]),
    "mi_tiff3d_read_box_device": (_i, [_i, _vp, C.POINTER(Tiff3dJob), _i, _i, _i, _i, _i, _vp, _i]),
    # mi_pystripe.h
    "mi_pystripe_plan_create": (_i, [_i, _i, _i, _i, C.POINTER(PystripeParams), C.POINTER(_vp)]),
    "mi_pystripe_plan_create_wavelet": (_i, [_i, _i, _i, _i, C.POINTER(PystripeParams), C.POINTER(C.c_double), _i, C.POINTER(_vp)]),
    "mi_pystripe_derive_wavelet": (_i, [_i, _i, _i, C.POINTER(PystripeParams), _i, C.POINTER(PystripeInfo)]),
    "mi_pystripe_plan_destroy": (_i, [_vp]),
    "mi_pystripe_plan_info": (_i, [_vp, C.POINTER(PystripeInfo)]),
    "mi_pystripe_plan_notch_routes": (_i, [_vp, _ip, _i]),
    "mi_pystripe_derive": (_i, [_i, _i, _i, C.POINTER(PystripeParams), C.POINTER(PystripeInfo)]),
    "mi_pystripe_run": (_i, [_vp, _vp, _vp, _vp, _vp, C.c_int64]),
    "mi_pystripe_pad_size": (_i, [_i, _i, C.c_double]),
    "mi_pystripe_plan_set_log_table": (_i, [_vp, _vp, _i]),
    "mi_pystripe_plan_clips": (_i, [_vp, _vp, _vp, _i]),
    # mi_lightsheet.h
    "mi_lightsheet_derive": (_i, [_i, _i, _i, C.POINTER(LightsheetParams), C.POINTER(LightsheetInfo)]),
    "mi_lightsheet_plan_create": (_i, [_i, _i, _i, _i, C.POINTER(LightsheetParams), C.POINTER(_vp)]),
    "mi_lightsheet_plan_destroy": (_i, [_vp]),
    "mi_lightsheet_plan_info": (_i, [_vp, C.POINTER(LightsheetInfo)]),
    "mi_lightsheet_run": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int64]),
    "mi_lightsheet_local_percentile": (_i, [_i, _vp, _vp, _i, _i, _i, C.c_int64] + [_i] * 6 + [C.c_double, _i, _vp, _i]),
    # mi_tile_resize.h
    "mi_tile_resize_tables": (_i, [_i, _i, _ip, _ip, C.POINTER(C.c_double)]),
    "mi_tile_resize_plan_create": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "mi_tile_resize_run": (_i, [_vp, _vp, _vp, _vp, C.c_int64]),
    "mi_tile_resize_plan_destroy": (_i, [_vp]),
    # mi_tile_mask.h
    "mi_tile_mask_plan_create": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "mi_tile_mask_run": (_i, [_vp, _vp, _vp, C.c_double, _i, _vp, _vp, C.c_int64]),
    "mi_tile_mask_plan_info": (_i, [_vp, C.POINTER(TileMaskInfo)]),
    "mi_tile_mask_plan_destroy": (_i, [_vp]),
    # mi_isodown.h
    "mi_isodown_derive": (_i, [_i, _i, C.c_double, C.c_double, C.c_double, _i, C.POINTER(IsodownInfo)]),
    "mi_isodown_plan_create": (_i, [_i, _i, _i, _i, C.POINTER(IsodownParams), C.POINTER(_vp)]),
    "mi_isodown_plan_destroy": (_i, [_vp]),
    "mi_isodown_plan_info": (_i, [_vp, C.POINTER(IsodownInfo)]),
    "mi_isodown_halve": (_i, [_vp, _vp, _vp, C.c_int64, _vp, _vp]),
    "mi_isodown_planes": (_i, [_vp, _vp, _vp, C.c_int64, _vp]),
    "mi_isodown_run": (_i, [_vp, _vp, _vp, C.c_int64, _vp, _vp]),
    "mi_isodown_reduce_z": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "mi_resize_antialias": (_i, [_i, _vp, _vp, _i, _ip, _ip, _vp]),
    # mi_thresholds.h
    "mi_hist256_f32": (_i, [_i, _vp, _vp, _i, C.c_int64, _vp, _vp, _vp, _vp]),
    "mi_code_hist": (_i, [_i, _vp, _vp, _i, _i, C.c_int64, _vp]),
    "mi_multiotsu_search": (_i, [_i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    # mi_align.h
    "mi_sobel2d_f32": (_i, [_i, _vp, _vp, _i, _i, _vp]),
    "mi_ecc_prepare": (_i, [_i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "mi_ecc_sums": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_double, C.c_double, _vp, _vp]),
    "mi_ecc_translation_run": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_double, C.c_double, _i, C.c_double, _i, _vp, _vp,
                                    C.POINTER(EccState)]),
    "mi_channel_composite": (_i, [_i, _vp, C.POINTER(CompositeChannel), _i, _i, _i, _i, _i, _vp, _i]),
    # mi_crossmips.h
    "mi_ncc_default_params": (None, [_i, _i, _i, C.POINTER(NccParams)]),
    "mi_ncc_mips": (_i, [_i, _vp, _vp, _vp] + [_i] * 10 + [C.POINTER(NccParams), C.POINTER(NccDescr)]),
    "mi_ncc_mips_host": (_i, [_i, _vp, _vp, _vp] + [_i] * 10 + [C.POINTER(NccParams), C.POINTER(NccDescr)]),
    "mi_ncc_mips_batch_begin": (_i, [_i, _vp, _i, C.POINTER(_vp), _i, _f, _ip, _ip, _i, _i, _i, _ip, _ip, _i, _i, _i, _ip, C.POINTER(NccParams),
                                     C.POINTER(_vp)]),
    "mi_ncc_mips_batch_end": (_i, [_vp, C.POINTER(NccParams), C.POINTER(NccDescr)]),
    "mi_ncc_mips_batch": (_i, [_i, _vp, _i, C.POINTER(_vp), _ip, _ip, _i, _i, _i, _ip, _ip, _i, _i, _i, _ip,
                               C.POINTER(NccParams), C.POINTER(NccDescr)]),
    "mi_ncc_mips_batch_u16": (_i, [_i, _vp, _i, C.POINTER(_vp), C.c_float, _ip, _ip, _i, _i, _i, _ip, _ip, _i, _i, _i, _ip,
                                   C.POINTER(NccParams), C.POINTER(NccDescr)]),
    "mi_ncc_mips_batch_u8": (_i, [_i, _vp, _i, C.POINTER(_vp), C.c_float, _ip, _ip, _i, _i, _i, _ip, _ip, _i, _i, _i, _ip,
                                  C.POINTER(NccParams), C.POINTER(NccDescr)]),
    "mi_ncc_time_mips": (_i, [_i, _vp, _i, C.POINTER(_vp), _ip, _ip, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_float)]),
    "mi_ncc_time_mips_u8": (_i, [_i, _vp, _i, C.POINTER(_vp), C.c_float, _ip, _ip, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_float)]),
    "mi_ncc_time_mips_u16": (_i, [_i, _vp, _i, C.POINTER(_vp), C.c_float, _ip, _ip, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_float)]),
    "mi_ncc_stats": (None, [C.POINTER(C.c_longlong), _i]),
    "mi_ncc_compute_mips": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i] + [_vp] * 6),
    "mi_ncc_compute_map": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mi_ncc_compute_map_lag": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
}

_lib = None


def lib() -> C.CDLL:
    """Loads libmi_ipp.so once and binds every declared symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            f"(python -c 'import __graft_entry__ as g; g.build()' or make -C {os.path.join(_HERE, 'csrc')}). "
            "There is no CPU fallback.")
    # One HIP / HSA runtime per process: PyTorch ships its own copies of libamdhip64 / libhsa-runtime64.  When they are loaded
    # first, this library binds to them (same sonames); the other way round the process ends up with the system's HIP runtime
    # under this library and torch's HSA runtime under torch, and torch then finds "No HIP GPUs".  The host layer uses torch
    # for device memory and streams anyway, so it goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    handle = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(handle, name)  # AttributeError if the library does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = handle
    return handle


def last_error() -> str:
    return lib().mi_last_error().decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc != MI_OK:
        raise MiError(rc, last_error())


def require_gpu() -> None:
    """Fail loudly when no HIP device is visible (the product path never computes on the CPU)."""
    n = lib().mi_device_count()
    if n <= 0:
        raise RuntimeError(f"no HIP device available (mi_device_count() = {n}: {last_error()}); "
                           "the MI355X path has no CPU fallback")


def release_cached_memory(device=None) -> int:
    """Gives the device memory the library keeps for reuse back to the driver (``mi_release_cached_memory``); returns bytes."""
    return int(lib().mi_release_cached_memory(-1 if device is None else int(device)))


def current_stream_ptr(device) -> int:
    """hipStream_t of torch's current stream on ``device`` as an integer for the void* parameter."""
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)
