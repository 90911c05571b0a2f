"""ctypes binding of libs2sr.so (include/s2sr.h).

This is the only place Python touches the native library.  There is NO fallback: if the
shared object is missing or no gfx950 device is visible, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref
from pathlib import Path
from typing import List, NamedTuple, Optional

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("S2SR_LIB", _HERE.parent / "csrc" / "libs2sr.so"))

PREC_F16, PREC_F16_HP, PREC_FP8 = 0, 1, 2
_ERR = {-1: "invalid argument", -2: "HIP error", -3: "weights not loaded", -4: "bad weight blob",
        -5: "no gfx950 device (no CPU fallback exists)", -6: "buffer too small", -7: "file could not be written"}


class S2srError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("num_block", C.c_int32), ("num_feat", C.c_int32), ("num_grow", C.c_int32), ("scale", C.c_int32),
                ("precision", C.c_int32), ("device", C.c_int32), ("group", C.c_int32), ("arch", C.c_int32)]


class Window(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("y1", "y2", "x1", "x2", "crop_top", "crop_bottom", "crop_left",
                                         "crop_right", "oy1", "oy2", "ox1", "ox2")]


class PPParams(C.Structure):
    _fields_ = [("clahe_clip", C.c_float), ("clahe_grid", C.c_int32), ("blur_sigma", C.c_float),
                ("w_img", C.c_float), ("w_blur", C.c_float), ("hue_lo", C.c_int32), ("hue_hi", C.c_int32),
                ("sat_gain", C.c_float), ("stages", C.c_int32)]


class Mask(C.Structure):                   # s2sr_mask
    _fields_ = [("valid", C.c_void_p), ("radius", C.c_int32), ("out_nodata", C.c_int32)]


class EnhanceArgs(C.Structure):            # s2sr_enhance_args: one whole-image call
    _fields_ = [("size", C.c_uint32), ("bits", C.c_int32), ("img", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("H", "W", "tile", "pad", "lo", "hi")] + \
               [("prm", C.POINTER(PPParams)), ("swap_rb", C.c_int32), ("blend", C.c_int32), ("force_tiled", C.c_int32),
                ("mask", C.POINTER(Mask)), ("consistency", C.c_int32), ("out", C.c_void_p), ("out_f32", C.c_void_p), ("inexact", C.c_void_p)]


class Enhanced(NamedTuple):                # Engine.enhance's result; None for what was not asked
    q: Optional[np.ndarray]                # the quantised image
    f32: Optional[np.ndarray]              # the unquantised HWC float32 image
    inexact: Optional[np.ndarray]          # uint64 [3], with a consistency pass


class DebugConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("precision", "group", "trunk_w4", "lo_exp", "fp8_form", "fp8_x_exp", "fp8_g_exp",
                                         "fp8_hp_tail", "graphs_on", "trunk_wino")] + [("reserved", C.c_int32 * 6)]


class DebugTrunkArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "form", "N", "Cin", "H", "W")] + \
               [(n, C.c_void_p) for n in ("x", "weight", "bias", "lo", "skip", "y", "y_aux")]


TAP_NAMES = ("P0", "F", "TRUNK_HI", "TRUNK_LO", "T8", "U0", "U1", "U2", "U3", "U0LO", "U1LO", "U2LO", "U3LO")   # S2SR_TAP_*
# channels and scale (0: 1x, 1: 2x, 2: 4x) of each tap
TAP_SHAPE = {"P0": (16, 0), "F": (64, 0), "TRUNK_HI": (64, 0), "TRUNK_LO": (64, 0), "T8": (128, 0), "U0": (64, 0), "U1": (64, 1),
             "U2": (64, 2), "U3": (64, 2), "U0LO": (128, 0), "U1LO": (128, 1), "U2LO": (128, 2), "U3LO": (128, 2)}


class DebugTaps(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(n, C.c_int32 * 3) for n in ("H", "W", "Hp", "Wp")] + \
               [(n, C.c_int32) for n in ("mos_kx", "mos_ky", "mos_wh", "mos_ww", "mos_count", "trunk_lo_exp", "avail")] + \
               [("reserved", C.c_int32 * 4), ("tap", C.c_void_p * len(TAP_NAMES)), ("out_f32", C.c_void_p), ("out_u8", C.c_void_p)]


TRUNK_FORM_FIELDS = ("kernel", "ct", "rows", "ring", "full", "pl", "prod", "wgl", "loe", "wv", "npl", "epi")   # s2sr_debug_trunk_form


class DebugTrunkForm(C.Structure):
    _fields_ = [(n, C.c_int32) for n in TRUNK_FORM_FIELDS]


class DebugTrunkFields(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("first", "count", "n", "H", "W", "Hp", "Wp", "mos_kx", "mos_ky", "mos_wh", "mos_ww",
                                         "mos_count", "fp8", "lo_exp", "x_exp", "g_exp")] + [("reserved", C.c_int32 * 4)] + \
               [(n, C.c_void_p) for n in ("x_hi", "x_lo", "growth", "skip_hi", "skip_lo", "entry_lo", "form", "out_f32", "out_u8")]


class KStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


# constants of the two post-process variants (reference wow_sr.py:191-205, farm_sr.py:100,170-178)
def pp_wow() -> PPParams:
    return PPParams(2.5, 8, 1.2, 1.4, -0.4, 35, 85, 1.2, 7)


def pp_farm() -> PPParams:
    return PPParams(2.5, 8, 1.5, 2.2, -1.2, 35, 85, 1.3, 7)


PP_ORDER_BGR, PP_ORDER_SWAP_OUT = 1, 2      # s2sr_pp_band_begin_dev `order` bits


COMPACT_TAPS_MAX = 8
COMPACT_GROUP = 16          # engine.hip kCompactGroup (the sweep of tools/bench_compact.py)
ARCH_RRDB, ARCH_COMPACT = 0, 1
_ARCH = {"rrdb": ARCH_RRDB, "compact": ARCH_COMPACT}


class DebugCompactFields(C.Structure):     # s2sr_debug_compact_fields
    _fields_ = [("nlayers", C.c_int32), ("layers", C.c_int32 * COMPACT_TAPS_MAX)] + \
               [(n, C.c_int32) for n in ("n", "H", "W", "Hp", "Wp", "mos_kx", "mos_ky", "mos_wh", "mos_ww", "mos_count")] + \
               [("reserved", C.c_int32 * 4), ("act", C.c_void_p * COMPACT_TAPS_MAX), ("p0", C.c_void_p), ("out_f32", C.c_void_p),
                ("out_u8", C.c_void_p)]


_lib = None

_PROTOS = {
    "s2sr_version": (C.c_char_p, []),
    "s2sr_device_count": (C.c_int, []),
    "s2sr_create": (C.c_int, [C.POINTER(_Config), C.POINTER(C.c_void_p)]),
    "s2sr_destroy": (None, [C.c_void_p]),
    "s2sr_last_error": (C.c_char_p, [C.c_void_p]),
    "s2sr_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "s2sr_host_free": (C.c_int, [C.c_void_p]),
    "s2sr_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "s2sr_expected_blob_floats": (C.c_size_t, [C.c_int32]),
    "s2sr_expected_blob_floats_scale": (C.c_size_t, [C.c_int32, C.c_int32]),
    "s2sr_expected_blob_floats_cfg": (C.c_size_t, [C.POINTER(_Config)]),
    "s2sr_load_weights_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "s2sr_calibrate_fp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32)]),
    "s2sr_plan_tiles": (C.c_int, [C.c_int32] * 5 + [C.POINTER(Window), C.c_int32, C.POINTER(C.c_int32)]),
    "s2sr_forward_batch_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_forward_batch_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p]),
    "s2sr_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_forward_batch_u16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "s2sr_forward_batch_u16_dev": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "s2sr_enhance": (C.c_int, [C.c_void_p, C.POINTER(EnhanceArgs)]),
    "s2sr_enhance_u16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]),
    "s2sr_enhance_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_enhance_blend_u8": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(PPParams), C.c_int32, C.c_void_p, C.c_void_p]),
    "s2sr_enhance_blend_u16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]),
    "s2sr_fill_nodata_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_fill_nodata_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_enhance_masked_u8": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(PPParams), C.c_int32, C.c_int32, C.POINTER(Mask),
                                         C.c_void_p]),
    "s2sr_enhance_masked_u16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.POINTER(Mask), C.c_void_p]),
    "s2sr_consistency_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "s2sr_consistency_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p, C.c_void_p]),
    "s2sr_enhance_consistent_u8": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(PPParams), C.c_int32, C.c_int32, C.POINTER(Mask),
                                             C.c_int32, C.c_void_p, C.c_void_p]),
    "s2sr_enhance_consistent_u16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.POINTER(Mask), C.c_int32, C.c_void_p, C.c_void_p]),
    "s2sr_display_hist_u16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p]),
    "s2sr_display_apply_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "s2sr_carry_band_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "s2sr_index_nd_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p, C.c_int32, C.c_void_p,
                                    C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 5),
    "s2sr_index_render_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "s2sr_zones_rasterize_u16": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "s2sr_fields_segment_i16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.c_int64, C.c_int32] + [C.c_void_p] * 3),
    "s2sr_labels_trace_u16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 3 + [C.c_uint64] * 2 + [C.c_void_p] * 4),
    "s2sr_debug_fields_stage_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "s2sr_fields_split_i16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.c_int64, C.c_int32] + [C.c_void_p] * 6),
    "s2sr_debug_fields_split_stage_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "s2sr_zones_kmeans_i16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] + [C.c_int32] * 3 + [C.c_int64] + [C.c_int32] * 2 +
                              [C.c_void_p] * 5),
    "s2sr_debug_mzones_stage_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "s2sr_enhance_job_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PPParams), C.c_void_p]),
    "s2sr_enhance_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_tile_process_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_cut_windows_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]),
    "s2sr_stitch_windows_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
    "s2sr_stitch_rows_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]),
    "s2sr_forward_part_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
    "s2sr_copy_to_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "s2sr_postprocess_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(PPParams), C.c_void_p]),
    "s2sr_postprocess_batch_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                C.POINTER(PPParams), C.c_void_p, C.c_void_p]),
    "s2sr_pp_band_begin_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(PPParams), C.c_int32, C.c_void_p]),
    "s2sr_pp_band_hist_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_pp_band_lut_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "s2sr_pp_band_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "s2sr_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "s2sr_get_kernel_stats": (C.c_int, [C.c_void_p, C.POINTER(KStat), C.c_int32, C.POINTER(C.c_int32)]),
    "s2sr_reset_kernel_stats": (C.c_int, [C.c_void_p]),
    "s2sr_synchronize": (C.c_int, [C.c_void_p]),
    "s2sr_debug_f32_to_e4m3": (C.c_uint8, [C.c_float]),
    "s2sr_debug_pack_f8_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "s2sr_debug_pack_f8": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "s2sr_warp_bilinear_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_warp_bilinear_masked_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p] +
                                     [C.c_int32] * 5 + [C.c_void_p]),
    "s2sr_tiles_base_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_tiles_overview_u8": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p]),
    "s2sr_tiles_resample_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + ([C.c_void_p] * 3 + [C.c_int32]) * 2 +
                               [C.c_int32, C.c_int32, C.c_void_p]),
    "s2sr_tiles_write_png": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_int32)]),
    "s2sr_tiles_write_png_xyz": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                           C.POINTER(C.c_int32)]),
    "s2sr_tiff_lzw_encode": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "s2sr_tiff_lzw_decode": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "s2sr_png_bound": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "s2sr_png_encode": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "s2sr_png_idat_band": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]),
    "s2sr_png_write_tiles": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.POINTER(C.c_char_p), C.c_int32,
                                       C.POINTER(C.c_int32)]),
    "s2sr_graph_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "s2sr_debug_conv": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p] +
                        [C.c_int32] * 3 + [C.c_void_p]),
    "s2sr_debug_pick_mosaic": (C.c_int, [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 2),
    "s2sr_debug_mosaic_patches": (C.c_int, [C.c_int32] * 3 + [C.POINTER(C.c_int64)] * 2),
    "s2sr_debug_plan_chunks": (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]),
    "s2sr_debug_plan_windows": (C.c_int, [C.c_int32] * 6 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "s2sr_debug_plan_blend": (C.c_int, [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]),
    "s2sr_debug_plan_bands": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "s2sr_debug_get_config": (C.c_int, [C.c_void_p, C.POINTER(DebugConfig)]),
    "s2sr_debug_conv_trunk": (C.c_int, [C.c_void_p, C.POINTER(DebugTrunkArgs)]),
    "s2sr_debug_forward_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(DebugTaps)]),
    "s2sr_debug_trunk_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(DebugTrunkFields)]),
    "s2sr_debug_compact_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(DebugCompactFields)]),
    "s2sr_debug_mfma_ceiling": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_float)]),
    "s2sr_debug_bench_conv": (C.c_int, [C.c_void_p] + [C.c_int32] * 6 + [C.POINTER(C.c_float), C.c_void_p, C.c_int32]),
    "s2sr_debug_rdb_persistent": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32)]),
    "s2sr_debug_redzone": (C.c_int, [C.c_int64]),
    "s2sr_debug_redzone_bytes": (C.c_int64, []),
    "s2sr_debug_redzone_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "s2sr_debug_redzone_poke": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    "s2sr_debug_poison": (C.c_int, [C.c_int32]),
    "s2sr_debug_poison_pattern": (C.c_int32, []),
    "s2sr_debug_poison_scratch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "s2sr_debug_scratch_peek": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]),
    "s2sr_debug_delay": (C.c_int, [C.c_int32, C.c_int32]),
    "s2sr_debug_delay_mode": (C.c_int32, []),
    "s2sr_debug_delay_usec": (C.c_int32, []),
    "s2sr_debug_delay_drop": (C.c_int, [C.c_int32]),
    "s2sr_debug_delay_dropped": (C.c_int32, []),
    "s2sr_debug_stall": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "s2sr_debug_stream_touch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "s2sr_debug_grid_cap": (C.c_int, [C.c_int32]),
    "s2sr_debug_grid_cap_workgroups": (C.c_int32, []),
    "s2sr_debug_grid_cap_stats": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32)]),
    "s2sr_debug_grid_cap_stats_reset": (None, []),
    "s2sr_debug_grid_cap_family": (C.c_char_p, [C.c_int32]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)
FIELDS_STAGES = ("mask_morphology", "local", "border", "flatten", "count", "scan", "apply", "labels")   # S2SR_FIELDS_STAGE_*
MZONES_STAGES = ("statistics", "iterations", "assign", "smoothing", "table")                            # S2SR_MZONES_*
FSPLIT_STAGES = ("edge", "distance", "cores", "grow_interior", "grow_edges", "remap", "numbering")      # S2SR_FSPLIT_*


def _mapped_hip_runtimes() -> set:
    """Real paths of every libamdhip64 mapped into this process (Linux; empty when /proc is not readable)."""
    out = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    out.add(os.path.realpath(line.split()[-1]))
    except OSError:
        pass
    return out


def load_library():
    """dlopen libs2sr.so and attach prototypes.  Raises if it is not built: no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise S2srError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"or `make -C {LIB_PATH.parent}`.  There is no CPU fallback.")
    # ONE HIP runtime per process.  libs2sr.so is linked against `libamdhip64.so.<N>` (RUNPATH /opt/rocm/lib) and the
    # PyTorch-ROCm wheel bundles a runtime with the same SONAME.  The dynamic loader resolves a DT_NEEDED entry against
    # already loaded objects by SONAME first, so when torch is imported BEFORE this dlopen, libs2sr binds to torch's
    # bundled runtime and both sides share one HIP context, one set of streams and device pointers (which is what the
    # `*_dev` entry points and the RCCL path need).  The other order maps the system runtime first and leaves torch with
    # "No HIP GPUs are available".  So: import torch first when it exists, then verify that exactly one libamdhip64 is
    # mapped -- two would mean the SONAMEs diverged (e.g. a ROCm major bump on one side) and device pointers could not
    # be shared; that is an error, not something to limp along with.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(str(LIB_PATH))
    hips = _mapped_hip_runtimes()
    if len(hips) > 1:
        raise S2srError(f"two HIP runtimes are mapped into this process ({sorted(hips)}): libs2sr.so and PyTorch must share one "
                        "libamdhip64 (same SONAME) -- rebuild libs2sr.so against the ROCm major version of the torch wheel")
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)          # AttributeError here == ABI drift, let it surface
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def tiff_lzw_encode(data) -> bytes:
    """Host call (no GPU): raw strip bytes -> TIFF LZW.  ctypes drops the GIL: strips encode in parallel."""
    lib = load_library()
    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).ravel()
    cap = buf.size * 3 // 2 + 16
    out = np.empty(cap, np.uint8)
    n = C.c_size_t(0)
    rc = lib.s2sr_tiff_lzw_encode(buf.ctypes.data_as(C.c_void_p), buf.size, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    if rc:
        raise S2srError(f"s2sr_tiff_lzw_encode: {_ERR.get(rc, rc)}")
    return out[:n.value].tobytes()


def _png_rows(img: np.ndarray):
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"expected HxWx3 or HxWx4 uint8, got {img.shape} {img.dtype}")
    if img.strides[2] != 1 or img.strides[1] != img.shape[2] or img.strides[0] < img.shape[1] * img.shape[2]:
        img = np.ascontiguousarray(img)
    return img, img.shape[0], img.shape[1], img.shape[2], img.strides[0]


_PNG_TLS = threading.local()


def _png_out(cap: int) -> np.ndarray:
    """Output staging of the calling thread (a fresh 300-KB array per tile is an mmap / munmap pair per call)."""
    buf = getattr(_PNG_TLS, "buf", None)
    if buf is None or buf.size < cap or buf.size > max(4 * cap, 1 << 22):
        buf = _PNG_TLS.buf = np.empty(cap, np.uint8)
    return buf


def png_encode(img: np.ndarray) -> bytes:
    """Host call (no GPU): HxWx3 / HxWx4 uint8 -> a complete PNG file (Sub filter, run-length deflate, dynamic Huffman).
    ctypes drops the GIL: tiles encode in parallel on threads."""
    lib = load_library()
    img, h, w, c, stride = _png_rows(img)
    cap = lib.s2sr_png_bound(w, h, c)
    out = _png_out(cap)
    n = C.c_size_t(0)
    rc = lib.s2sr_png_encode(img.ctypes.data_as(C.c_void_p), w, h, c, stride, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    if rc:
        raise S2srError(f"s2sr_png_encode: {_ERR.get(rc, rc)}")
    return out[:n.value].tobytes()


def png_idat_band(rows: np.ndarray, first: bool, last: bool):
    """Host call (no GPU): a band of rows of a big image -> (one complete IDAT chunk, Adler-32 of the band's filtered bytes,
    their count); see s2sr_png_idat_band in include/s2sr.h for how the bands make a file."""
    lib = load_library()
    rows, h, w, c, stride = _png_rows(rows)
    cap = lib.s2sr_png_bound(w, h, c)
    out = _png_out(cap)
    n, adler, raw_n = C.c_size_t(0), C.c_uint32(0), C.c_size_t(0)
    rc = lib.s2sr_png_idat_band(rows.ctypes.data_as(C.c_void_p), w, h, c, stride, int(first), int(last), out.ctypes.data_as(C.c_void_p),
                                cap, C.byref(n), C.byref(adler), C.byref(raw_n))
    if rc:
        raise S2srError(f"s2sr_png_idat_band: {_ERR.get(rc, rc)}")
    return out[:n.value].tobytes(), int(adler.value), int(raw_n.value)


def png_write_tiles(tiles_arr: np.ndarray, paths, skip_transparent: bool = True) -> np.ndarray:
    """Host call (no GPU): [n, S, S, 3|4] uint8 tiles -> PNG files at `paths` (str / Path, None = skip), parent directories made on
    demand, fully transparent RGBA tiles skipped.  Returns the 0/1 array of files written.  The whole loop runs without the GIL."""
    lib = load_library()
    if tiles_arr.dtype != np.uint8 or tiles_arr.ndim != 4 or tiles_arr.shape[1] != tiles_arr.shape[2] or tiles_arr.shape[3] not in (3, 4):
        raise ValueError(f"expected [n, S, S, 3|4] uint8, got {tiles_arr.shape} {tiles_arr.dtype}")
    n, size, _, c = tiles_arr.shape
    if len(paths) != n:
        raise ValueError(f"{n} tiles, {len(paths)} paths")
    if tiles_arr.strides[1:] != (size * c, c, 1) or tiles_arr.strides[0] < size * size * c:
        tiles_arr = np.ascontiguousarray(tiles_arr)
    cp = (C.c_char_p * n)(*[None if p is None else os.fsencode(p) for p in paths])
    written = np.zeros(n, np.int32)
    rc = lib.s2sr_png_write_tiles(tiles_arr.ctypes.data_as(C.c_void_p), n, size, c, tiles_arr.strides[0] if n else size * size * c, cp,
                                  int(skip_transparent), written.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc:
        raise S2srError(f"s2sr_png_write_tiles: {_ERR.get(rc, rc)}" + (f" ({os.strerror(C.get_errno())})" if rc == -7 and C.get_errno() else ""))
    return written


def tiff_lzw_decode(data: bytes, expected: int) -> bytes:
    """Host call (no GPU): TIFF LZW strip/tile -> raw bytes (at most `expected`)."""
    lib = load_library()
    out = C.create_string_buffer(max(int(expected), 1))
    n = C.c_size_t(0)
    rc = lib.s2sr_tiff_lzw_decode(data, len(data), out, int(expected), C.byref(n))
    if rc:
        raise S2srError(f"s2sr_tiff_lzw_decode: {_ERR.get(rc, rc)}")
    return out.raw[:n.value]


def tiff_lzw_decode_into(src: np.ndarray, offset: int, count: int, dst: np.ndarray) -> int:
    """Host call (no GPU): the LZW stream src[offset : offset + count] (a uint8 array over the file) decoded straight into the
    C-contiguous array `dst` (at most dst.nbytes) -> bytes produced.  No intermediate buffers: a strip of a chunky GeoTIFF lands in
    the rows of the image it belongs to."""
    lib = load_library()
    if not dst.flags["C_CONTIGUOUS"] or not dst.flags["WRITEABLE"] or offset < 0 or count < 0 or offset + count > src.size:
        raise ValueError("tiff_lzw_decode_into: a C-contiguous writable destination and a stream inside the source are required")
    n = C.c_size_t(0)
    rc = lib.s2sr_tiff_lzw_decode(C.c_void_p(src.ctypes.data + offset), count, dst.ctypes.data_as(C.c_void_p), dst.nbytes, C.byref(n))
    if rc:
        raise S2srError(f"s2sr_tiff_lzw_decode: {_ERR.get(rc, rc)}")
    return int(n.value)


def plan_tiles(H: int, W: int, tile: int = 256, pad: int = 10, scale: int = 4) -> List[Window]:
    """Pure host call (works without a GPU): window plan of `_tile_process`."""
    lib = load_library()
    n = C.c_int32(0)
    rc = lib.s2sr_plan_tiles(H, W, tile, pad, scale, None, 0, C.byref(n))
    if rc:
        raise S2srError(f"s2sr_plan_tiles: {_ERR.get(rc, rc)}")
    arr = (Window * n.value)()
    rc = lib.s2sr_plan_tiles(H, W, tile, pad, scale, arr, n.value, C.byref(n))
    if rc:
        raise S2srError(f"s2sr_plan_tiles: {_ERR.get(rc, rc)}")
    return list(arr)


def pick_mosaic(B: int, th: int, tw: int) -> tuple:
    """(kx, ky): windows per launch image the engine would use for B windows of th x tw (host arithmetic)."""
    kx, ky = C.c_int32(0), C.c_int32(0)
    rc = load_library().s2sr_debug_pick_mosaic(B, th, tw, C.byref(kx), C.byref(ky))
    if rc:
        raise S2srError(f"s2sr_debug_pick_mosaic failed ({_ERR.get(rc, rc)})")
    return int(kx.value), int(ky.value)


def mosaic_patches(B: int, th: int, tw: int) -> tuple:
    """(launched, plain): 32x32 patches the engine launches for B windows of th x tw, and what B plain images would cost."""
    a, b = C.c_int64(0), C.c_int64(0)
    rc = load_library().s2sr_debug_mosaic_patches(B, th, tw, C.byref(a), C.byref(b))
    if rc:
        raise S2srError(f"s2sr_debug_mosaic_patches failed ({_ERR.get(rc, rc)})")
    return int(a.value), int(b.value)


def plan_chunks(units: int, u_max: int, unit_windows: int, per: int, pimg: int, ncu: int = 256) -> List[int]:
    """Chunk sizes (row units, front to back) s2sr_enhance_u8 would use; host arithmetic, works without a GPU."""
    lib = load_library()
    n = C.c_int32(0)
    buf = (C.c_int32 * max(1, units))()
    rc = lib.s2sr_debug_plan_chunks(units, u_max, unit_windows, per, pimg, ncu, buf, max(1, units), C.byref(n))
    if rc:
        raise S2srError(f"s2sr_debug_plan_chunks failed ({_ERR.get(rc, rc)})")
    return [int(buf[i]) for i in range(n.value)]


def plan_windows(PH: int, PW: int, tile: int, pad: int, scale: int = 4, tiled: bool = True) -> tuple:
    """(nx, ny, wh, ww, rects[nx * ny, 4], rm[scale * PH, 2], cm[scale * PW, 2]): the distinct windows enhance runs the net on and
    its paste maps (window row / column, row / column inside the window's output); host arithmetic, works without a GPU."""
    cap = ((PH + tile - 1) // tile) * ((PW + tile - 1) // tile)
    dims, rects = np.zeros(4, np.int32), np.zeros((cap, 4), np.int32)
    rm, cm = np.zeros((scale * PH, 2), np.int32), np.zeros((scale * PW, 2), np.int32)
    rc = load_library().s2sr_debug_plan_windows(PH, PW, tile, pad, scale, int(tiled), _ptr(dims), _ptr(rects), cap, _ptr(rm), _ptr(cm))
    if rc:
        raise S2srError(f"s2sr_debug_plan_windows failed ({_ERR.get(rc, rc)})")
    nx, ny, wh, ww = (int(v) for v in dims)
    return nx, ny, wh, ww, rects[:nx * ny if tiled else 0], rm, cm


def plan_blend(PH: int, PW: int, tile: int, pad: int, scale: int = 4, tiled: bool = True) -> tuple:
    """(rows[scale * PH, 6], cols[scale * PW, 6]): the blend tables of enhance_blend_* for plan_windows' job, per output row /
    column {a, ia, b, ib, num, den} -- the two windows, the row / column inside each one's output and the weight num / den of b
    (0 / 1 outside the ramps, where a == b); host arithmetic, works without a GPU."""
    rows, cols = np.zeros((scale * PH, 6), np.int32), np.zeros((scale * PW, 6), np.int32)
    rc = load_library().s2sr_debug_plan_blend(PH, PW, tile, pad, scale, int(tiled), _ptr(rows), _ptr(cols))
    if rc:
        raise S2srError(f"s2sr_debug_plan_blend failed ({_ERR.get(rc, rc)})")
    return rows, cols


def plan_bands(chunk_r0, ny: int, OH: int, last_row) -> np.ndarray:
    """bands[nchunks, 2]: the output rows [yb, ye) each chunk of a whole-image call makes final.  chunk_r0: the first window row of
    each chunk, then ny; last_row[OH]: the last window row every output row reads (plan_windows' rm[:, 0], plan_blend's
    rows[:, 2]); host arithmetic, works without a GPU."""
    r0, last = np.ascontiguousarray(chunk_r0, np.int32), np.ascontiguousarray(last_row[:OH], np.int32)
    if r0.ndim != 1 or len(r0) < 2 or last.shape != (OH,):
        raise ValueError("chunk_r0 holds nchunks + 1 window rows, last_row at least OH rows")
    bands = np.zeros((len(r0) - 1, 2), np.int32)
    rc = load_library().s2sr_debug_plan_bands(_ptr(r0), len(r0) - 1, ny, OH, _ptr(last), _ptr(bands))
    if rc:
        raise S2srError(f"s2sr_debug_plan_bands failed ({_ERR.get(rc, rc)})")
    return bands


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class _PinnedPool:
    """Page-locked output arrays (s2sr_host_alloc).  `RealESRGAN.enhance` returns a fresh numpy array per call
    (cnn_super_resolution.py:231-233); a fresh pageable array costs the device-to-host path a staging copy and a page fault per
    4 KB (805 MB: 130 ms), a page-locked one is filled by the DMA engines (20 ms).  Pinning is slow (hundreds of ms for 800 MB), so
    buffers are recycled: an array handed out here returns its buffer to the pool when the last view of it is garbage collected.
    Buffers come in 16-MB size classes, so images of nearby sizes share them (r03 ADVICE: exact-size keys pinned a new buffer
    per distinct image size).  Two caps: S2SR_PINNED_POOL_MB (default 4096) of IDLE buffers are kept, and S2SR_PINNED_MAX_MB
    (default 16384) bounds all page-locked bytes, in use and idle -- beyond it `empty` hands out ordinary pageable arrays (the
    library then takes its staged route).  A service that RETAINS results (job tables, caches) should copy them (`.copy()`) or
    set S2SR_PINNED_OUT=0: a retained result keeps its page-locked buffer."""
    BUCKET = 16 << 20

    def __init__(self):
        import threading
        self._lock = threading.Lock()
        self._free = {}          # bucket bytes -> [address, ...]
        self._idle = 0
        self._total = 0          # page-locked bytes alive, in use + idle
        self._cap = int(os.environ.get("S2SR_PINNED_POOL_MB", "4096")) << 20
        self._max = int(os.environ.get("S2SR_PINNED_MAX_MB", "16384")) << 20
        self.on = os.environ.get("S2SR_PINNED_OUT", "1") != "0"
        self.hits = self.misses = self.refused = 0

    def empty(self, shape, dtype) -> np.ndarray:
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        if not self.on or n < (8 << 20):
            return np.empty(shape, dtype=dtype)
        nb = -(-n // self.BUCKET) * self.BUCKET
        lib = load_library()
        with self._lock:
            lst = self._free.get(nb)
            addr = lst.pop() if lst else None
            if addr is not None:
                self._idle -= nb
                self.hits += 1
            elif self._total + nb > self._max:
                self.refused += 1
                return np.empty(shape, dtype=dtype)
            else:
                self._total += nb           # reserved before the (slow) allocation, outside the lock
                self.misses += 1
        if addr is None:
            p = C.c_void_p()
            if lib.s2sr_host_alloc(nb, C.byref(p)) or not p.value:
                with self._lock:
                    self._total -= nb
                return np.empty(shape, dtype=dtype)      # no page-locked memory to be had: the pageable route still works
            addr = p.value
        buf = (C.c_uint8 * nb).from_address(addr)
        weakref.finalize(buf, self._give, addr, nb)       # runs when the last numpy view of `buf` is gone
        return np.frombuffer(buf, dtype=np.uint8, count=n).view(dtype).reshape(shape)

    def _give(self, addr, nb):
        with self._lock:
            if self._idle + nb <= self._cap:
                self._free.setdefault(nb, []).append(addr)
                self._idle += nb
                return
            self._total -= nb
        try:
            load_library().s2sr_host_free(C.c_void_p(addr))
        except Exception:
            pass

    def trim(self):
        """Release every idle buffer."""
        with self._lock:
            addrs = [(a, nb) for nb, lst in self._free.items() for a in lst]
            self._free.clear()
            self._idle = 0
            self._total -= sum(nb for _, nb in addrs)
        for a, _ in addrs:
            load_library().s2sr_host_free(C.c_void_p(a))


pinned_pool = _PinnedPool()


def warp_mask(rgb_shape, valid, valid_scale) -> np.ndarray:
    """The mask of Engine.warp_bilinear_u8 as the library takes it, or ValueError: uint8 [ceil(H / valid_scale), ceil(W / valid_scale)]
    for an [H, W, 3] raster, valid_scale an integer >= 1 (host arithmetic: refused before the engine is touched)."""
    vs = valid_scale
    if isinstance(vs, bool) or not isinstance(vs, (int, np.integer)) or vs < 1:
        raise ValueError(f"valid_scale {vs!r}: an integer of at least 1")
    valid = np.ascontiguousarray(valid)
    rgb_shape = tuple(rgb_shape)
    if len(rgb_shape) != 3 or rgb_shape[2] != 3:
        raise ValueError(f"expected an [H, W, 3] raster, got {rgb_shape}")
    want = (-(-rgb_shape[0] // int(vs)), -(-rgb_shape[1] // int(vs)))
    if valid.dtype != np.uint8 or valid.shape != want:
        raise ValueError(f"valid: expected uint8 {want} for a {rgb_shape} raster at valid_scale {vs}, got {valid.dtype} {valid.shape}")
    return valid


class Engine:
    """One native handle == one GPU.  Thread-safe (the library serialises calls per handle)."""

    def __init__(self, num_block: int = 23, precision: int = PREC_F16, device: int = 0, group: int = 0, scale: int = 4,
                 arch: str = "rrdb"):
        """scale 4, or 2 = RealESRGAN_x2plus (include/s2sr.h s2sr_config.scale): every output is `scale` x the input.
        arch "compact" = SRVGGNetCompact (realesr-general-x4v3 and kin): `num_block` carries num_conv (16 or 32), scale 4 only;
        PREC_F16 and PREC_F16_HP run the same arithmetic there, PREC_FP8 is refused."""
        self._lib = load_library()
        self._h = C.c_void_p()
        # held by callers across calls that depend on what the call before left on the device (enhance_u16 -> display_*_u16 with
        # img=None): the library serialises single calls, not such pairs
        self.chain_lock = threading.RLock()
        if arch not in _ARCH:
            raise ValueError(f"arch {arch!r}: 'rrdb' or 'compact'")
        self.arch = arch
        self.num_block = num_block
        self.precision, self.group = precision, group
        self.scale = int(scale)
        cfg = _Config(num_block, 64, 32, self.scale, precision, device, group, _ARCH[arch])
        rc = self._lib.s2sr_create(C.byref(cfg), C.byref(self._h))
        if rc:
            msg = self._lib.s2sr_last_error(None)
            raise S2srError(f"s2sr_create failed ({_ERR.get(rc, rc)}): {msg.decode() if msg else ''}")

    def group_images(self) -> int:
        """Images per launch group (engine.hip group_size: 16, 32 for the fp8 trunk, or what the constructor was given)."""
        if self.group <= 0 and self.arch == "compact":
            return COMPACT_GROUP
        return self.group if self.group > 0 else (32 if self.precision == PREC_FP8 else 16)

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc:
            msg = self._lib.s2sr_last_error(self._h)
            raise S2srError(f"{what} failed ({_ERR.get(rc, rc)}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.s2sr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights ----------------------------------------------------------------------------
    def load_blob(self, blob: np.ndarray):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._check(self._lib.s2sr_load_weights(self._h, _ptr(blob), blob.size), "s2sr_load_weights")

    def load_blob_dev(self, d_blob: int, n_floats: int, stream: int = 0):
        """Device pointer to the fp32 blob (e.g. the tensor an RCCL broadcast filled)."""
        self._check(self._lib.s2sr_load_weights_dev(self._h, C.c_void_p(d_blob), n_floats, C.c_void_p(stream)),
                    "s2sr_load_weights_dev")

    def load_state_dict(self, sd):
        from .weights import flatten_state_dict, infer_arch
        arch = infer_arch(sd.keys())[0]
        if arch != self.arch:
            raise ValueError(f"state dict is a {arch} net, this engine was created with arch={self.arch!r}")
        self.load_blob(flatten_state_dict(sd, self.num_block, scale=self.scale, arch=arch))

    def calibrate_fp8(self, tiles: np.ndarray, headroom: float = 2.0) -> tuple:
        """PREC_FP8 engines: set the trunk's activation scales from representative tiles -> (x_exp, g_exp)."""
        tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
        B, h, w, c = tiles.shape
        assert c == 3
        xe, ge = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.s2sr_calibrate_fp8(self._h, _ptr(tiles), B, h, w, headroom, C.byref(xe), C.byref(ge)), "s2sr_calibrate_fp8")
        return int(xe.value), int(ge.value)

    # -- forward ----------------------------------------------------------------------------
    def forward_batch_u8(self, tiles: np.ndarray) -> np.ndarray:
        tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
        B, h, w, c = tiles.shape
        assert c == 3
        S = self.scale
        out = pinned_pool.empty((B, S * h, S * w, 3), np.uint8)
        self._check(self._lib.s2sr_forward_batch_u8(self._h, _ptr(tiles), B, h, w, _ptr(out)), "s2sr_forward_batch_u8")
        return out

    def forward_batch_u8_dev(self, d_in: int, B: int, h: int, w: int, d_out: int, stream: int = 0):
        """Device pointers (ints, e.g. torch.Tensor.data_ptr()); asynchronous on `stream`."""
        self._check(self._lib.s2sr_forward_batch_u8_dev(self._h, d_in, B, h, w, d_out, C.c_void_p(stream)),
                    "s2sr_forward_batch_u8_dev")

    def forward_f32(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        N, c, H, W = x.shape
        assert c == 3
        y = np.empty((N, 3, self.scale * H, self.scale * W), dtype=np.float32)
        self._check(self._lib.s2sr_forward_f32(self._h, _ptr(x), N, H, W, _ptr(y)), "s2sr_forward_f32")
        return y

    # -- the whole-image door (include/s2sr.h s2sr_enhance_args: every keyword below is the field of that name) ------------------
    def enhance(self, img: np.ndarray, *, tile: int = 256, pad: int = 10, lo: int = 0, hi: int = 65535, prm: Optional[PPParams] = None,
                swap_rb: bool = False, blend: bool = False, force_tiled: bool = False, valid=None, radius: int = 32, out_nodata: int = 0,
                consistency: int = 0, quantised: bool = True, want_f32: bool = False) -> Enhanced:
        """HxWx3 uint8 or uint16 (bits from the dtype) through s2sr_enhance with the options that are on -> Enhanced(q, f32,
        inexact).  valid (uint8 [H, W], nonzero = valid; None: not masked) with radius and out_nodata is the record's mask;
        quantised / want_f32 choose the outputs.  Which combinations exist is the library's to say (S2srError with its text)."""
        img = np.asarray(img)
        if img.dtype not in (np.uint8, np.uint16):
            raise TypeError(f"enhance takes a uint8 or uint16 image, got {img.dtype}")
        img = np.ascontiguousarray(img)
        H, W, c = img.shape
        assert c == 3
        shape = (self.scale * H, self.scale * W, 3)
        m = None
        if valid is not None:
            valid = self._valid(valid, H, W, "enhance")      # (valid and m stay alive to the end of the call)
            m = Mask(valid.ctypes.data, int(radius), int(out_nodata))
        q = pinned_pool.empty(shape, img.dtype) if quantised else None
        f = np.empty(shape, dtype=np.float32) if want_f32 else None
        bad = np.zeros(3, np.uint64) if consistency else None
        data = lambda a: None if a is None else a.ctypes.data
        args = EnhanceArgs(C.sizeof(EnhanceArgs), 8 * img.itemsize, img.ctypes.data, H, W, int(tile), int(pad), int(lo), int(hi),
                           None if prm is None else C.pointer(prm), int(bool(swap_rb)), int(bool(blend)), int(bool(force_tiled)),
                           None if m is None else C.pointer(m), int(consistency), data(q), data(f), data(bad))
        self._check(self._lib.s2sr_enhance(self._h, C.byref(args)), "s2sr_enhance")
        return Enhanced(q, f, bad)

    # The forms: the doors from before the record, each a spelling of `enhance` (include/s2sr.h lists the fields each sets).
    def enhance_u8(self, img: np.ndarray, tile: int = 256, pad: int = 10) -> np.ndarray:
        return self.enhance(np.ascontiguousarray(img, dtype=np.uint8), tile=tile, pad=pad).q

    def enhance_job_u8(self, rgb: np.ndarray, prm: Optional[PPParams] = None, tile: int = 256, pad: int = 10) -> np.ndarray:
        """RGB in -> (BGR) net -> RGB -> post-process `prm` (None: none) -> RGB out: a job's device work in one call."""
        return self.enhance(np.ascontiguousarray(rgb, dtype=np.uint8), prm=prm, swap_rb=True, tile=tile, pad=pad).q

    def enhance_f32(self, img: np.ndarray, tile: int = 256, pad: int = 10) -> np.ndarray:
        return self.enhance(np.ascontiguousarray(img, dtype=np.uint8), tile=tile, pad=pad, quantised=False, want_f32=True).f32

    def tile_process_f32(self, img: np.ndarray, tile: int = 256, pad: int = 10) -> np.ndarray:
        return self.enhance(np.ascontiguousarray(img, dtype=np.uint8), tile=tile, pad=pad, force_tiled=True, quantised=False,
                            want_f32=True).f32

    # -- the 16-bit door (include/s2sr.h: uint16 in, uint16 x4 out, value range lo, hi) ---------
    def forward_batch_u16(self, tiles: np.ndarray, lo: int = 0, hi: int = 65535, want_f32: bool = False):
        """[B,h,w,3] uint16 -> [B,4h,4w,3] uint16 = lo + rint(clip(y, 0, 1) * (hi - lo)); want_f32: (that, the unquantised net
        output [B,3,4h,4w] float32)."""
        if np.asarray(tiles).dtype != np.uint16:
            raise TypeError(f"forward_batch_u16 takes uint16 tiles, got {np.asarray(tiles).dtype}")
        tiles = np.ascontiguousarray(tiles)
        B, h, w, c = tiles.shape
        assert c == 3
        out = pinned_pool.empty((B, 4 * h, 4 * w, 3), np.uint16)
        f = np.empty((B, 3, 4 * h, 4 * w), dtype=np.float32) if want_f32 else None
        self._check(self._lib.s2sr_forward_batch_u16(self._h, _ptr(tiles), B, h, w, int(lo), int(hi), _ptr(out), _ptr(f) if want_f32 else None),
                    "s2sr_forward_batch_u16")
        return (out, f) if want_f32 else out

    def forward_batch_u16_dev(self, d_in: int, B: int, h: int, w: int, d_out: int, lo: int = 0, hi: int = 65535, stream: int = 0):
        """Device pointers (ints): [B,h,w,3] uint16 -> [B,4h,4w,3] uint16; asynchronous on `stream`."""
        self._check(self._lib.s2sr_forward_batch_u16_dev(self._h, d_in, B, h, w, int(lo), int(hi), d_out, C.c_void_p(stream)),
                    "s2sr_forward_batch_u16_dev")

    @staticmethod
    def _u16(img, what: str):
        if np.asarray(img).dtype != np.uint16:
            raise TypeError(f"{what} takes a uint16 image, got {np.asarray(img).dtype}")
        return img

    def enhance_u16(self, img: np.ndarray, lo: int = 0, hi: int = 65535, tile: int = 256, pad: int = 10, want_f32: bool = False):
        """HxWx3 uint16 -> 4Hx4Wx3 uint16 (whole / tiled as enhance_u8); want_f32: (that, the unquantised HWC float32 image)."""
        r = self.enhance(self._u16(img, "enhance_u16"), lo=lo, hi=hi, tile=tile, pad=pad, want_f32=want_f32)
        return (r.q, r.f32) if want_f32 else r.q

    # -- the seam-blended stitch (include/s2sr.h: the default doors' windows, cross-faded where they overlap) -------------------
    def enhance_blend_u8(self, img: np.ndarray, prm: Optional[PPParams] = None, swap_rb: bool = False, tile: int = 256, pad: int = 10,
                         want_f32: bool = False):
        """enhance_u8 (prm None, swap_rb False) or enhance_job_u8 (swap_rb True) with the blended paste; want_f32 (plain calls
        only): (the u8 image, the unquantised HWC float32 image)."""
        r = self.enhance(np.ascontiguousarray(img, dtype=np.uint8), prm=prm, swap_rb=swap_rb, blend=True, tile=tile, pad=pad, want_f32=want_f32)
        return (r.q, r.f32) if want_f32 else r.q

    def enhance_blend_u16(self, img: np.ndarray, lo: int = 0, hi: int = 65535, tile: int = 256, pad: int = 10, want_f32: bool = False):
        """enhance_u16 with the blended paste."""
        r = self.enhance(self._u16(img, "enhance_blend_u16"), lo=lo, hi=hi, blend=True, tile=tile, pad=pad, want_f32=want_f32)
        return (r.q, r.f32) if want_f32 else r.q

    # -- nodata-aware enhance (include/s2sr.h, DESIGN.md 7.4: fill the invalid pixels in front of the net, mask behind everything) ----
    @staticmethod
    def _valid(valid, H: int, W: int, what: str) -> np.ndarray:
        v = np.asarray(valid)
        if v.shape != (H, W):
            raise ValueError(f"{what}: valid must be [H, W] = {(H, W)}, got shape {v.shape}")
        return np.ascontiguousarray(v != 0, dtype=np.uint8) if v.dtype != np.uint8 else np.ascontiguousarray(v)

    def fill_nodata(self, img: np.ndarray, valid: np.ndarray, radius: int = 32) -> np.ndarray:
        """HxWx3 uint8 or uint16 -> the same image with every invalid pixel (valid == 0) replaced by its nearest valid neighbour
        within `radius` (ties: the upper, then the left one); no weights needed."""
        img = np.asarray(img)
        if img.dtype not in (np.uint8, np.uint16):
            raise TypeError(f"fill_nodata takes a uint8 or uint16 image, got {img.dtype}")
        img = np.ascontiguousarray(img)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"fill_nodata: expected HxWx3, got shape {img.shape}")
        H, W, _ = img.shape
        valid = self._valid(valid, H, W, "fill_nodata")
        out = np.empty_like(img)
        fn, name = (self._lib.s2sr_fill_nodata_u8, "s2sr_fill_nodata_u8") if img.dtype == np.uint8 else \
                   (self._lib.s2sr_fill_nodata_u16, "s2sr_fill_nodata_u16")
        self._check(fn(self._h, _ptr(img), _ptr(valid), H, W, int(radius), _ptr(out)), name)
        return out

    def enhance_masked_u8(self, img: np.ndarray, valid: np.ndarray, radius: int = 32, out_nodata: int = 0, prm: Optional[PPParams] = None,
                          swap_rb: bool = False, blend: bool = False, tile: int = 256, pad: int = 10) -> np.ndarray:
        """enhance_u8 / enhance_job_u8 (swap_rb) / enhance_blend_u8 (blend) on the filled image, out_nodata written over the output
        pixels of the invalid input pixels."""
        if valid is None:
            raise ValueError("enhance_masked_u8: valid must be [H, W], got None")
        return self.enhance(np.ascontiguousarray(img, dtype=np.uint8), valid=valid, radius=radius, out_nodata=out_nodata, prm=prm,
                            swap_rb=swap_rb, blend=blend, tile=tile, pad=pad).q

    def enhance_masked_u16(self, img: np.ndarray, valid: np.ndarray, lo: int = 0, hi: int = 65535, radius: int = 32, out_nodata: int = 0,
                           blend: bool = False, tile: int = 256, pad: int = 10) -> np.ndarray:
        """enhance_u16 / enhance_blend_u16 (blend) on the filled image, masked as enhance_masked_u8."""
        if valid is None:
            raise ValueError("enhance_masked_u16: valid must be [H, W], got None")
        return self.enhance(self._u16(img, "enhance_masked_u16"), valid=valid, lo=lo, hi=hi, radius=radius, out_nodata=out_nodata,
                            blend=blend, tile=tile, pad=pad).q

    # -- radiometric consistency (include/s2sr.h, DESIGN.md 7.5: block means of the output reproduce the input pixels) ------------
    def consistency(self, sr: np.ndarray, img: np.ndarray, mode: int = 1, lo: int = 0, hi: int = 65535, band_rows: int = 0):
        """The pass alone: sr [S H, S W, 3] and img [H, W, 3], both uint8 or both uint16 (lo, hi: the 16-bit range), S = 2 or 4
        from the shapes -> (the consistent image, inexact uint64 [3]); mode 1 exact, 2 smooth; no weights needed."""
        sr, img = np.asarray(sr), np.asarray(img)
        if sr.dtype != img.dtype or sr.dtype not in (np.uint8, np.uint16):
            raise TypeError(f"consistency takes two uint8 or two uint16 images, got {sr.dtype} and {img.dtype}")
        if sr.ndim != 3 or img.ndim != 3 or sr.shape[2] != 3 or img.shape[2] != 3:
            raise ValueError(f"consistency: expected [S H, S W, 3] and [H, W, 3], got {sr.shape} and {img.shape}")
        H, W, _ = img.shape
        S = sr.shape[0] // H if H else 0
        if S not in (2, 4) or sr.shape[:2] != (S * H, S * W):
            raise ValueError(f"consistency: sr {sr.shape} is not 2x or 4x img {img.shape}")
        sr, img = np.ascontiguousarray(sr), np.ascontiguousarray(img)
        out = np.empty_like(sr)
        bad = np.zeros(3, np.uint64)
        if sr.dtype == np.uint8:
            self._check(self._lib.s2sr_consistency_u8(self._h, _ptr(sr), _ptr(img), H, W, S, int(mode), int(band_rows), _ptr(out), _ptr(bad)),
                        "s2sr_consistency_u8")
        else:
            self._check(self._lib.s2sr_consistency_u16(self._h, _ptr(sr), _ptr(img), H, W, S, int(lo), int(hi), int(mode), int(band_rows),
                                                       _ptr(out), _ptr(bad)), "s2sr_consistency_u16")
        return out, bad

    consistency_u8 = consistency
    consistency_u16 = consistency

    @staticmethod
    def _mode(mode, what: str) -> int:
        if mode not in (1, 2):                         # (0 means "off" in the record: the consistent forms do not offer it)
            raise S2srError(f"{what} failed (invalid argument): consistency: mode must be 1 or 2, got {mode}")
        return int(mode)

    def enhance_consistent_u8(self, img: np.ndarray, mode: int = 1, prm: Optional[PPParams] = None, swap_rb: bool = False, blend: bool = False,
                              valid=None, radius: int = 32, out_nodata: int = 0, tile: int = 256, pad: int = 10):
        """enhance_u8 / enhance_job_u8 (swap_rb) / enhance_blend_u8 (blend) / enhance_masked_u8 (valid) with the consistency pass
        behind the paste -> (the image, inexact uint64 [3])."""
        r = self.enhance(np.ascontiguousarray(img, dtype=np.uint8), consistency=self._mode(mode, "enhance_consistent_u8"), prm=prm,
                         swap_rb=swap_rb, blend=blend, valid=valid, radius=radius, out_nodata=out_nodata, tile=tile, pad=pad)
        return r.q, r.inexact

    def enhance_consistent_u16(self, img: np.ndarray, lo: int = 0, hi: int = 65535, mode: int = 1, blend: bool = False, valid=None,
                               radius: int = 32, out_nodata: int = 0, tile: int = 256, pad: int = 10):
        """enhance_u16 / enhance_blend_u16 (blend) / enhance_masked_u16 (valid) with the consistency pass -> (the image, inexact)."""
        r = self.enhance(self._u16(img, "enhance_consistent_u16"), consistency=self._mode(mode, "enhance_consistent_u16"), lo=lo, hi=hi,
                         blend=blend, valid=valid, radius=radius, out_nodata=out_nodata, tile=tile, pad=pad)
        return r.q, r.inexact

    # -- display rendering of 16-bit images (include/s2sr.h; policy between the two passes: s2sr/display.py) ---------------------
    @staticmethod
    def _display_source(img, shape, what: str):
        if img is None:
            if shape is None:
                raise ValueError(f"{what}: img=None (the device copy) needs shape=(H, W)")
            return None, int(shape[0]), int(shape[1])
        if np.asarray(img).dtype != np.uint16:
            raise TypeError(f"{what} takes a uint16 image, got {np.asarray(img).dtype}")
        img = np.ascontiguousarray(img)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"{what}: expected HxWx3, got shape {img.shape}")
        return img, img.shape[0], img.shape[1]

    def display_hist_u16(self, img: Optional[np.ndarray], nodata: int = -1, band_rows: int = 0, shape=None) -> np.ndarray:
        """HxWx3 uint16 -> uint64 [3][65536]: samples per channel and value, those equal to nodata (-1: none) left out.  img None: the
        uint16 image of `shape` (H, W) the previous call on this engine left on the device (enhance_u16 / enhance_blend_u16: their
        4H x 4W output; a display call: its upload)."""
        img, H, W = self._display_source(img, shape, "display_hist_u16")
        hist = np.empty((3, 65536), np.uint64)
        self._check(self._lib.s2sr_display_hist_u16(self._h, _ptr(img) if img is not None else None, H, W, int(nodata), int(band_rows),
                                                    _ptr(hist)), "s2sr_display_hist_u16")
        return hist

    def display_apply_u16(self, img: Optional[np.ndarray], lut: np.ndarray, band_rows: int = 0, shape=None) -> np.ndarray:
        """out[y, x, c] = lut[c][img[y, x, c]], lut uint8 [3][65536]; img None as in display_hist_u16."""
        img, H, W = self._display_source(img, shape, "display_apply_u16")
        lut = np.ascontiguousarray(lut)
        if lut.dtype != np.uint8 or lut.shape != (3, 65536):
            raise ValueError(f"display_apply_u16: lut must be uint8 [3][65536], got {lut.dtype} {lut.shape}")
        out = np.empty((H, W, 3), np.uint8) if H > 0 and W > 0 else np.empty((1,), np.uint8)
        self._check(self._lib.s2sr_display_apply_u16(self._h, _ptr(img) if img is not None else None, H, W, _ptr(lut), int(band_rows),
                                                     _ptr(out)), "s2sr_display_apply_u16")
        return out

    # -- carrying an extra band to the SR grid (include/s2sr.h; defaults and argument checks: s2sr/bands.py) -----------
    def carry_band_u16(self, band: np.ndarray, S: int, sr: Optional[np.ndarray] = None, lo: int = 0, hi: int = 65535, weights=(1, 1, 1),
                       r: int = 2, eps: int = 1, valid=None, fill: int = 0, band_rows: int = 0):
        """band [H, W] uint16 -> (the band on the SR grid, uint16 [S H, S W], inexact): guided upsampling against sr [S H, S W, 3]
        uint16, or (sr None) against the S H x S W uint16 image the previous call on this engine left on the device, which stays
        there for the next band or a display call.  No weights needed."""
        band = np.asarray(band)
        if band.dtype != np.uint16:
            raise TypeError(f"carry_band_u16 takes a uint16 band, got {band.dtype}")
        if band.ndim != 2:
            raise ValueError(f"carry_band_u16: expected a band [H, W], got shape {band.shape}")
        band = np.ascontiguousarray(band)
        H, W = band.shape
        S = int(S)
        if sr is not None:
            if np.asarray(sr).dtype != np.uint16:
                raise TypeError(f"carry_band_u16 takes a uint16 image, got {np.asarray(sr).dtype}")
            sr = np.ascontiguousarray(sr)
            if sr.shape != (S * H, S * W, 3):
                raise ValueError(f"carry_band_u16: sr {sr.shape} is not [S H, S W, 3] = {(S * H, S * W, 3)}")
        if valid is not None:
            valid = self._valid(valid, H, W, "carry_band_u16")
        w = np.array([int(x) for x in weights], np.int32)
        if w.shape != (3,):
            raise ValueError(f"carry_band_u16: three guide weights are required, got {weights!r}")
        out = pinned_pool.empty((S * H, S * W), np.uint16) if H > 0 and W > 0 and S > 0 else np.empty((1,), np.uint16)
        bad = np.zeros(1, np.uint64)
        self._check(self._lib.s2sr_carry_band_u16(self._h, _ptr(sr) if sr is not None else None, _ptr(band), H, W, S, int(lo), int(hi), _ptr(w),
                                                  int(r), int(eps), _ptr(valid) if valid is not None else None, int(fill), int(band_rows),
                                                  _ptr(out), _ptr(bad)), "s2sr_carry_band_u16")
        return out, int(bad[0])

    # -- normalised-difference indices (include/s2sr.h; presets, ramps, statistics and argument checks: s2sr/index.py) --
    @staticmethod
    def _plane(p, what: str):
        """a uint16 plane [H, W] or [H, W, c] -> (the contiguous array, H, W, c)"""
        p = np.asarray(p)
        if p.dtype != np.uint16:
            raise TypeError(f"{what} takes uint16 planes, got {p.dtype}")
        if p.ndim not in (2, 3):
            raise ValueError(f"{what}: expected a plane [H, W] or [H, W, c], got shape {p.shape}")
        p = np.ascontiguousarray(p)
        return p, p.shape[0], p.shape[1], (p.shape[2] if p.ndim == 3 else 1)

    @staticmethod
    def _cells(m, H: int, W: int, scale: int, dtype, what: str) -> np.ndarray:
        m = np.asarray(m)
        scale = int(scale)
        want = (-(-H // scale), -(-W // scale)) if scale >= 1 else None
        if want is not None and m.shape != want:
            raise ValueError(f"{what} must be [ceil(H / {scale}), ceil(W / {scale})] = {want}, got shape {m.shape}")
        if dtype == np.uint8 and m.dtype != np.uint8:
            m = m != 0
        return np.ascontiguousarray(m, dtype=dtype)

    @staticmethod
    def _index_lut(lut, what: str) -> np.ndarray:
        lut = np.ascontiguousarray(lut)
        if lut.dtype != np.uint8 or lut.shape != (65536, 4):
            raise ValueError(f"{what}: lut must be uint8 [65536][4], got {lut.dtype} {lut.shape}")
        return lut

    def index_nd_u16(self, a: Optional[np.ndarray], b: np.ndarray, ca: int = 0, cb: int = 0, offset: int = 0, L: int = 0, K: int = 10000,
                     valid=None, valid_scale: int = 1, zones=None, zone_scale: int = 1, Z: int = 0, lut=None, band_rows: int = 0,
                     want=("index",)) -> dict:
        """v = round_half_away(K (a' - b') / (a' + b' + L)), a' = max(a - offset, 0), of channel ca of a and channel cb of b (uint16
        [H, W] or [H, W, 3]); a None: channel ca of the H x W x 3 uint16 image the previous call on this engine left on the device,
        which stays there.  `want` names the outputs: "index" (int16 [H, W], nodata -32768), "hist" (uint64 [2 K + 1]), "rgba"
        (uint8 [H, W, 4] through lut, uint8 [65536][4]), "zonal" (int64 [Z + 1][3] over the uint16 labels `zones`).  Returns a dict
        of those and "undefined" (the unmasked pixels whose denominator is zero).  No weights needed."""
        what = "index_nd_u16"
        b, H, W, bc = self._plane(b, what)
        ac = 3
        if a is not None:
            a, Ha, Wa, ac = self._plane(a, what)
            if (Ha, Wa) != (H, W):
                raise ValueError(f"{what}: a is {Ha} x {Wa}, b is {H} x {W}")
        want = set(want)
        if not want <= {"index", "hist", "rgba", "zonal"}:
            raise ValueError(f"{what}: outputs are index, hist, rgba, zonal; got {sorted(want)}")
        if valid is not None:
            valid = self._cells(valid, H, W, valid_scale, np.uint8, f"{what}: valid")
        if zones is not None:
            zones = self._cells(zones, H, W, zone_scale, np.uint16, f"{what}: zones")
        if lut is not None:
            lut = self._index_lut(lut, what)
        K, Z = int(K), int(Z)
        ok = H > 0 and W > 0
        out = pinned_pool.empty((H, W), np.int16) if "index" in want and ok else None
        rgba = pinned_pool.empty((H, W, 4), np.uint8) if "rgba" in want and ok else None
        hist = np.zeros(2 * K + 1 if 1 <= K <= 16383 else 1, np.uint64) if "hist" in want else None
        zonal = np.zeros((Z + 1 if 0 <= Z <= 65535 else 1, 3), np.int64) if "zonal" in want else None
        undef = np.zeros(1, np.uint64)
        p = lambda x: _ptr(x) if x is not None else None
        self._check(self._lib.s2sr_index_nd_u16(self._h, p(a), ac, int(ca), _ptr(b), bc, int(cb), H, W, int(offset), int(L), K, p(valid),
                                                int(valid_scale), p(zones), int(zone_scale), Z, p(lut), int(band_rows), p(out), p(hist), p(zonal),
                                                p(rgba), _ptr(undef)), "s2sr_index_nd_u16")
        res = {"undefined": int(undef[0])}
        for k, v in (("index", out), ("hist", hist), ("rgba", rgba), ("zonal", zonal)):
            if k in want:
                res[k] = v
        return res

    def index_render_i16(self, idx: np.ndarray, lut: np.ndarray, band_rows: int = 0) -> np.ndarray:
        """int16 [H, W] -> uint8 [H, W, 4] = lut[(uint16)(idx + 32768)], -32768 (nodata) -> 0, 0, 0, 0."""
        idx = np.asarray(idx)
        if idx.dtype != np.int16 or idx.ndim != 2:
            raise TypeError(f"index_render_i16 takes an int16 raster [H, W], got {idx.dtype} {idx.shape}")
        idx = np.ascontiguousarray(idx)
        lut = self._index_lut(lut, "index_render_i16")
        H, W = idx.shape
        out = pinned_pool.empty((H, W, 4), np.uint8) if H > 0 and W > 0 else np.empty((1,), np.uint8)
        self._check(self._lib.s2sr_index_render_i16(self._h, _ptr(idx), H, W, _ptr(lut), int(band_rows), _ptr(out)), "s2sr_index_render_i16")
        return out

    def zones_rasterize_u16(self, xy, ring_start, feat_start, label, Z: int, shape, band_rows: int = 0, want_area: bool = True):
        """Features made of rings -> (uint16 labels [H, W], uint64 area [Z + 1] or None) on the label grid shape = (H, W)
        (include/s2sr.h s2sr_zones_rasterize_u16).  xy: int32 [V, 2] in 1/256 of a label pixel; ring_start: int32
        [R + 1] into xy; feat_start: int32 [F + 1] into the rings; label: uint16 [F] in 1..Z.  The later feature wins a pixel two
        features hold; 0 where none does.  The call voids whatever the call before it kept on the device.  No weights needed."""
        what = "zones_rasterize_u16"
        tabs = []
        for name, t, dt in (("xy", xy, np.int32), ("ring_start", ring_start, np.int32), ("feat_start", feat_start, np.int32), ("label", label, np.uint16)):
            t = np.asarray(t)
            if t.dtype != dt:
                raise TypeError(f"{what}: {name} must be {np.dtype(dt).name}, got {t.dtype}")
            tabs.append(np.ascontiguousarray(t))
        xy, ring_start, feat_start, label = tabs
        if xy.ndim != 2 or xy.shape[1] != 2 or ring_start.ndim != 1 or feat_start.ndim != 1 or label.ndim != 1:
            raise ValueError(f"{what}: xy is [V, 2], ring_start [R + 1], feat_start [F + 1], label [F]")
        F = len(feat_start) - 1
        if len(ring_start) < 1 or F < 0 or len(label) != F:
            raise ValueError(f"{what}: {len(feat_start)} feature starts, {len(label)} labels and {len(ring_start)} ring starts do not fit together")
        # what the library cannot know: the tables' lengths.  Every start must point inside the table it indexes
        if F >= 0 and len(feat_start) and (feat_start.min(initial=0) < 0 or feat_start.max(initial=0) > len(ring_start) - 1):
            raise ValueError(f"{what}: feat_start points outside the {len(ring_start) - 1} rings")
        if ring_start.min(initial=0) < 0 or ring_start.max(initial=0) > len(xy):
            raise ValueError(f"{what}: ring_start points outside the {len(xy)} vertices")
        try:
            H, W = (int(v) for v in shape)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: shape is (H, W), got {shape!r}") from None
        Z = int(Z)
        ok = H > 0 and W > 0 and H * W < 2 ** 31
        out = pinned_pool.empty((H, W), np.uint16) if ok else np.empty((1,), np.uint16)
        area = np.zeros(Z + 1 if 0 <= Z <= 65535 else 1, np.uint64) if want_area else None
        self._check(self._lib.s2sr_zones_rasterize_u16(self._h, _ptr(xy), _ptr(ring_start), _ptr(feat_start), _ptr(label), F, Z, H, W, int(band_rows),
                                                       _ptr(out), _ptr(area) if area is not None else None), "s2sr_zones_rasterize_u16")
        return out, area

    def fields_segment_i16(self, idx, lo: int, hi: int, r_open: int = 0, r_close: int = 0, conn: int = 4, min_pixels: int = 1, Z: int = 65535):
        """An int16 index raster [H, W] (nodata -32768) -> (uint16 labels [H, W], int64 fields [Z + 1][6] = pixels, key, x0, y0,
        x1, y1, found) (include/s2sr.h s2sr_fields_segment_i16): the mask lo <= idx <= hi, opened and closed with
        squares of radius r_open and r_close, split into components under conn (4 or 8); those of at least min_pixels pixels are
        numbered 1, 2, ... by their first pixel.  The call voids whatever the call before it kept on the device.  No weights needed."""
        idx = np.asarray(idx)
        if idx.dtype != np.int16 or idx.ndim != 2:
            raise TypeError(f"fields_segment_i16 takes an int16 raster [H, W], got {idx.dtype} {idx.shape}")
        idx = np.ascontiguousarray(idx)
        H, W = idx.shape
        Z = int(Z)
        ok = H > 0 and W > 0 and H * W < 2 ** 31
        labels = pinned_pool.empty((H, W), np.uint16) if ok else np.empty((1,), np.uint16)
        fields = np.zeros((Z + 1 if 0 <= Z <= 65535 else 1, 6), np.int64)
        found = np.zeros(1, np.uint64)
        self._check(self._lib.s2sr_fields_segment_i16(self._h, _ptr(idx), H, W, int(lo), int(hi), int(r_open), int(r_close), int(conn), int(min_pixels), Z,
                                                      _ptr(labels), _ptr(fields), _ptr(found)), "s2sr_fields_segment_i16")
        return labels, fields, int(found[0])

    def _stage_ms(self, hook: str, stages, *more) -> dict:
        """{stage: (ms, launches)} from one of the s2sr_debug_*_stage_ms hooks; more: what the hook takes behind ms and launches"""
        ms, n = np.zeros(len(stages), np.float64), np.zeros(len(stages), np.int32)
        self._check(getattr(self._lib, hook)(self._h, _ptr(ms), _ptr(n), *more), hook)
        return {name: (float(ms[k]), int(n[k])) for k, name in enumerate(stages)}

    def fields_stage_ms(self) -> dict:
        """What the stages of the last fields_segment_i16 took by HIP events, {stage: (ms, launches)} in the order of FIELDS_STAGES
        (include/s2sr.h s2sr_debug_fields_stage_ms): zeros unless that call ran under set_profiling(1)."""
        return self._stage_ms("s2sr_debug_fields_stage_ms", FIELDS_STAGES)

    def fields_split_i16(self, idx, lo: int, hi: int, r_open: int = 0, r_close: int = 0, conn: int = 4, min_pixels: int = 1, Z: int = 65535,
                         split=None, want=()):
        """fields_segment_i16 with touching fields cut apart (include/s2sr.h s2sr_fields_split_i16).  split: None (the
        bytes of fields_segment_i16) or {"core_q": 1..1000, "core_px": 0..255, "edge": 0..32767, "edge_r": 0..4} (defaults 500, 2, 0,
        1).  Returns (labels, fields, found) and, with want=("dist2", "cores") or one of them, those planes behind them in that
        order: uint16 [H, W] squared distances capped at 255^2, uint8 [H, W] core pixels (zeros without a split).  The call voids
        whatever the call before it kept on the device.  No weights needed."""
        idx = np.asarray(idx)
        if idx.dtype != np.int16 or idx.ndim != 2:
            raise TypeError(f"fields_split_i16 takes an int16 raster [H, W], got {idx.dtype} {idx.shape}")
        unknown = set(want) - {"dist2", "cores"}
        if unknown:
            raise ValueError(f"fields_split_i16: unknown output(s) {sorted(unknown)}; known are dist2, cores")
        idx = np.ascontiguousarray(idx)
        H, W = idx.shape
        Z = int(Z)
        ok = H > 0 and W > 0 and H * W < 2 ** 31
        labels = pinned_pool.empty((H, W), np.uint16) if ok else np.empty((1,), np.uint16)
        fields = np.zeros((Z + 1 if 0 <= Z <= 65535 else 1, 6), np.int64)
        found = np.zeros(1, np.uint64)
        rec = None
        if split is not None:
            unknown = set(split) - {"core_q", "core_px", "edge", "edge_r"}
            if unknown:
                raise ValueError(f"fields_split_i16: split has unknown key(s) {sorted(unknown)}; known are core_q, core_px, edge, edge_r")
            rec = np.array([split.get("core_q", 500), split.get("core_px", 2), split.get("edge", 0), split.get("edge_r", 1)], np.int32)
        dist2 = np.zeros((H, W), np.uint16) if "dist2" in want else None
        cores = np.zeros((H, W), np.uint8) if "cores" in want else None
        self._check(self._lib.s2sr_fields_split_i16(self._h, _ptr(idx), H, W, int(lo), int(hi), int(r_open), int(r_close), int(conn), int(min_pixels), Z,
                                                    _ptr(rec) if rec is not None else None, _ptr(labels), _ptr(fields), _ptr(found),
                                                    _ptr(dist2) if dist2 is not None else None, _ptr(cores) if cores is not None else None),
                    "s2sr_fields_split_i16")
        return (labels, fields, int(found[0])) + tuple(v for v in (dist2, cores) if v is not None)

    def fields_split_stage_ms(self) -> dict:
        """What the stages of the last fields_split_i16 with a split took by HIP events, {stage: (ms, launches)} in the order of
        FSPLIT_STAGES, and under "rounds" the launches its two growths took (include/s2sr.h s2sr_debug_fields_split_stage_ms): the
        times are zeros unless that call ran under set_profiling(1)."""
        rounds = np.zeros(2, np.int32)
        out = self._stage_ms("s2sr_debug_fields_split_stage_ms", FSPLIT_STAGES, _ptr(rounds))
        out["rounds"] = (int(rounds[0]), int(rounds[1]))
        return out

    def zones_kmeans_i16(self, feats, labels, Z: int, k: int = 3, iters: int = 32, min_per_zone: int = 10, smooth: int = 0, band_rows: int = 0) -> dict:
        """Integer k-means inside every field (include/s2sr.h s2sr_zones_kmeans_i16).  feats: int16 [D, H, W] (or
        [H, W]: one raster), nodata -32768; labels: uint16 [H, W], 0 = no field, above Z = no field.  Returns {"zone": uint8 [H, W]
        (0: no zone; 1 the lowest class of the first raster), "table": int64 [Z + 1, k, 1 + 2 D] = pixels, then sum and sum of
        squares per raster, "centres": int32 [Z + 1, k, D] in zone order, "status": uint8 [Z + 1] (0 absent, 1 skipped, 2 zoned),
        "iterations": int}.  The call voids whatever the call before it kept on the device.  No weights needed."""
        feats, labels = np.asarray(feats), np.asarray(labels)
        if feats.dtype == np.int16 and feats.ndim == 2:
            feats = feats[None]
        if feats.dtype != np.int16 or feats.ndim != 3:
            raise TypeError(f"zones_kmeans_i16 takes int16 rasters [D, H, W], got {feats.dtype} {feats.shape}")
        if labels.dtype != np.uint16 or labels.ndim != 2 or labels.shape != feats.shape[1:]:
            raise TypeError(f"zones_kmeans_i16 takes uint16 labels {feats.shape[1:]}, got {labels.dtype} {labels.shape}")
        feats, labels = np.ascontiguousarray(feats), np.ascontiguousarray(labels)
        D, H, W = feats.shape
        Z, k = int(Z), int(k)
        ok = H > 0 and W > 0 and H * W < 2 ** 31
        rows, kk, dd = (Z + 1 if 0 <= Z <= 65535 else 1), (k if 2 <= k <= 8 else 1), (D if 1 <= D <= 4 else 1)
        zone = pinned_pool.empty((H, W), np.uint8) if ok else np.empty((1,), np.uint8)
        table, centres = np.zeros((rows, kk, 1 + 2 * dd), np.int64), np.zeros((rows, kk, dd), np.int32)
        status, iterations = np.zeros(rows, np.uint8), np.zeros(1, np.uint32)
        self._check(self._lib.s2sr_zones_kmeans_i16(self._h, _ptr(feats), D, H, W, _ptr(labels), Z, k, int(iters), int(min_per_zone), int(smooth),
                                                    int(band_rows), _ptr(zone), _ptr(table), _ptr(centres), _ptr(status), _ptr(iterations)),
                    "s2sr_zones_kmeans_i16")
        return {"zone": zone, "table": table, "centres": centres, "status": status, "iterations": int(iterations[0])}

    def mzones_stage_ms(self) -> dict:
        """What the stages of the last zones_kmeans_i16 took by HIP events, {stage: (ms, launches)} in the order of MZONES_STAGES
        (include/s2sr.h s2sr_debug_mzones_stage_ms): zeros unless that call ran under set_profiling(1)."""
        return self._stage_ms("s2sr_debug_mzones_stage_ms", MZONES_STAGES)

    def labels_trace_u16(self, labels, Z: int):
        """A uint16 label raster [H, W] -> (xy int32 [V, 2] in pixel corners, ring_start int32 [R + 1], ring_label uint16 [R]): the
        rings around the labels 1..Z (include/s2sr.h s2sr_labels_trace_u16; csrc/ring_trace.h), exteriors counterclockwise on a
        north-up map, holes clockwise, ordered by label and start vertex.  Host code; no weights needed."""
        labels = np.asarray(labels)
        if labels.dtype != np.uint16 or labels.ndim != 2:
            raise TypeError(f"labels_trace_u16 takes a uint16 raster [H, W], got {labels.dtype} {labels.shape}")
        labels = np.ascontiguousarray(labels)
        H, W = labels.shape
        counts = np.zeros(2, np.uint64)
        self._check(self._lib.s2sr_labels_trace_u16(self._h, _ptr(labels), H, W, int(Z), 0, 0, None, None, None, _ptr(counts)), "s2sr_labels_trace_u16")
        V, R = int(counts[0]), int(counts[1])
        xy, ring_start, ring_label = np.zeros((V, 2), np.int32), np.zeros(R + 1, np.int32), np.zeros(R, np.uint16)
        if R:
            self._check(self._lib.s2sr_labels_trace_u16(self._h, _ptr(labels), H, W, int(Z), V, R, _ptr(xy), _ptr(ring_start), _ptr(ring_label),
                                                        _ptr(counts)), "s2sr_labels_trace_u16")
        return xy, ring_start, ring_label

    # -- multi-GPU building blocks (device pointers) ------------------------------------------
    def cut_windows_u8_dev(self, d_img: int, H: int, W: int, tile: int, pad: int, first: int, count: int,
                           d_tiles: int, stream: int = 0):
        self._check(self._lib.s2sr_cut_windows_u8_dev(self._h, d_img, H, W, tile, pad, first, count, d_tiles,
                                                      C.c_void_p(stream)), "s2sr_cut_windows_u8_dev")

    def stitch_windows_u8_dev(self, d_tiles: int, H: int, W: int, tile: int, pad: int, d_out: int, stream: int = 0):
        self._check(self._lib.s2sr_stitch_windows_u8_dev(self._h, d_tiles, H, W, tile, pad, d_out, C.c_void_p(stream)),
                    "s2sr_stitch_windows_u8_dev")

    def stitch_rows_u8_dev(self, d_tiles: int, H: int, W: int, tile: int, pad: int, oy0: int, oy1: int, d_out: int, stream: int = 0):
        """Output rows [oy0, oy1) of the paste; d_out is the whole [S H, S W, 3] image (S = self.scale)."""
        self._check(self._lib.s2sr_stitch_rows_u8_dev(self._h, d_tiles, H, W, tile, pad, oy0, oy1, d_out, C.c_void_p(stream)),
                    "s2sr_stitch_rows_u8_dev")

    def forward_part_u8_dev(self, d_in: int, B: int, h: int, w: int, job_windows: int, d_out: int, stream: int = 0):
        """B windows that are a part of a job of `job_windows` (one mosaic plan and workspace for the whole job)."""
        self._check(self._lib.s2sr_forward_part_u8_dev(self._h, d_in, B, h, w, job_windows, d_out, C.c_void_p(stream)),
                    "s2sr_forward_part_u8_dev")

    def copy_to_host(self, dst: np.ndarray, d_src: int, stream: int = 0):
        """Device -> the (C-contiguous) host array `dst`, behind everything on `stream`; blocks until the bytes are there."""
        assert dst.flags["C_CONTIGUOUS"]
        self._check(self._lib.s2sr_copy_to_host(self._h, _ptr(dst), C.c_void_p(d_src), dst.nbytes, C.c_void_p(stream)), "s2sr_copy_to_host")

    # -- post-process -----------------------------------------------------------------------
    def postprocess_u8(self, rgb: np.ndarray, prm: PPParams) -> np.ndarray:
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        H, W, c = rgb.shape
        assert c == 3
        out = np.empty_like(rgb)
        self._check(self._lib.s2sr_postprocess_u8(self._h, _ptr(rgb), H, W, C.byref(prm), _ptr(out)),
                    "s2sr_postprocess_u8")
        return out

    def postprocess_batch_u8_dev(self, d_in: int, B: int, H: int, W: int, prm: PPParams, d_out: int, stream: int = 0):
        self._check(self._lib.s2sr_postprocess_batch_u8_dev(self._h, d_in, B, H, W, C.byref(prm), d_out,
                                                            C.c_void_p(stream)), "s2sr_postprocess_batch_u8_dev")

    # the same over ONE device image in row bands (include/s2sr.h: begin, hist over every row, lut, rows from row 0 on)
    def pp_band_begin_dev(self, H: int, W: int, prm: PPParams, order: int = 0, stream: int = 0):
        self._check(self._lib.s2sr_pp_band_begin_dev(self._h, H, W, C.byref(prm), order, C.c_void_p(stream)), "s2sr_pp_band_begin_dev")

    def pp_band_hist_dev(self, d_img: int, y0: int, y1: int, stream: int = 0):
        self._check(self._lib.s2sr_pp_band_hist_dev(self._h, C.c_void_p(d_img), y0, y1, C.c_void_p(stream)), "s2sr_pp_band_hist_dev")

    def pp_band_lut_dev(self, stream: int = 0):
        self._check(self._lib.s2sr_pp_band_lut_dev(self._h, C.c_void_p(stream)), "s2sr_pp_band_lut_dev")

    def pp_band_rows_dev(self, d_img: int, y0: int, y1: int, d_out: int, stream: int = 0):
        self._check(self._lib.s2sr_pp_band_rows_dev(self._h, C.c_void_p(d_img), y0, y1, C.c_void_p(d_out), C.c_void_p(stream)),
                    "s2sr_pp_band_rows_dev")

    def mfma_ceiling(self, mode: int, stages: int, launches: int) -> dict:
        """csrc/ceiling.hip: mode 0 bare MFMA loop, 1 + LDS operand reads, 2 + LDS-DMA ring refill (3 half the bytes, 4 from cache, 5 conv1-4's
        traffic mix, 6 conv5's, 7 / 8 from a 100-MB / 200-MB source inside the Infinity Cache) -> TFLOP/s over `launches` launches."""
        fl, by, ms = C.c_double(0), C.c_double(0), C.c_float(0)
        self._check(self._lib.s2sr_debug_mfma_ceiling(self._h, mode, stages, launches, C.byref(fl), C.byref(by), C.byref(ms)),
                    "s2sr_debug_mfma_ceiling")
        return {"ms": float(ms.value), "launches": launches, "us_per_launch": float(ms.value) * 1e3 / launches,
                "TFLOP_per_s": fl.value * launches / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0,
                "dma_GB_per_s": by.value * launches / (ms.value * 1e-3) / 1e9 if ms.value > 0 else 0.0}

    def rdb_persistent(self, variant: int, grid: int, P: int, rdbs: int, launches: int) -> dict:
        """csrc/persist.hip (diagnostic prototype): the RDB-shaped loop whose workgroups stay across layers -> TFLOP/s, dependency-wait timeouts.
        variant: bit 0 device-scope plane loads + written-through stores, bit 1 the deeper ring (32-KiB stages, three stages of look-ahead);
        4 / 5: variant 0 / 1 with every handed-over piece checked (halo_mismatches, own_mismatches)."""
        fl, ms, to, mm = C.c_double(0), C.c_float(0), C.c_int32(0), (C.c_int32 * 2)(0, 0)
        self._check(self._lib.s2sr_debug_rdb_persistent(self._h, int(variant), grid, P, rdbs, launches, C.byref(fl), C.byref(ms), C.byref(to), mm),
                    "s2sr_debug_rdb_persistent")
        return {"ms": float(ms.value), "launches": launches, "timeouts": int(to.value), "halo_mismatches": int(mm[0]), "own_mismatches": int(mm[1]), "working_set_MB": grid * P * (0.46875 if int(variant) & 2 else 0.5),
                "TFLOP_per_s": fl.value * launches / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0}

    # -- measurement ------------------------------------------------------------------------
    def set_profiling(self, every: int):
        """0/False: off; N>=1: HIP-event pair around every N-th launch of each kernel family."""
        self._check(self._lib.s2sr_set_profiling(self._h, int(every)), "s2sr_set_profiling")

    def reset_kernel_stats(self):
        self._check(self._lib.s2sr_reset_kernel_stats(self._h), "s2sr_reset_kernel_stats")

    def kernel_stats(self) -> dict:
        n = C.c_int32(0)
        self._check(self._lib.s2sr_get_kernel_stats(self._h, None, 0, C.byref(n)), "s2sr_get_kernel_stats")
        arr = (KStat * n.value)()
        self._check(self._lib.s2sr_get_kernel_stats(self._h, arr, n.value, C.byref(n)), "s2sr_get_kernel_stats")
        return {s.name.decode(): {"launches": s.launches, "total_ms": s.total_ms, "flops": s.flops, "bytes": s.bytes}
                for s in arr}

    # -- XYZ tile pyramid -----------------------------------------------------------------
    def warp_bilinear_u8(self, rgb: np.ndarray, grid: np.ndarray, step: int, out_h: int, out_w: int, valid: Optional[np.ndarray] = None,
                         valid_scale: int = 1) -> np.ndarray:
        """valid (uint8 [ceil(H / valid_scale), ceil(W / valid_scale)], nonzero = valid; None: the plain warp): source pixel (y, x)
        counts iff valid[y // valid_scale, x // valid_scale]; output pixels that lean on invalid ones by half their weight or more
        come out (0, 0, 0, 0) (s2sr_warp_bilinear_masked_u8)."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        grid = np.ascontiguousarray(grid, np.float32)
        if valid is not None:
            valid = warp_mask(rgb.shape, valid, valid_scale)
        out = pinned_pool.empty((out_h, out_w, 4), np.uint8)        # (page-locked when large: the raster comes back with one DMA)
        if valid is not None:
            self._check(self._lib.s2sr_warp_bilinear_masked_u8(self._h, _ptr(rgb), rgb.shape[0], rgb.shape[1], _ptr(valid), int(valid_scale),
                                                               _ptr(grid), grid.shape[0], grid.shape[1], step, out_h, out_w, _ptr(out)),
                        "s2sr_warp_bilinear_masked_u8")
            return out
        self._check(self._lib.s2sr_warp_bilinear_u8(self._h, _ptr(rgb), rgb.shape[0], rgb.shape[1], _ptr(grid), grid.shape[0],
                                                    grid.shape[1], step, out_h, out_w, _ptr(out)), "s2sr_warp_bilinear_u8")
        return out

    def tiles_base_u8(self, rgba, col_lo, col_hi, row_lo, row_hi, fetch: bool = True, on_device: bool = False) -> Optional[np.ndarray]:
        """fetch=False: the level is computed and left on the device (for tiles_write_png / the next overview); returns None.
        on_device: the raster is the one the previous call on this engine -- warp_bilinear_u8 -- produced and nothing else ran on the
        engine since: its device copy is used instead of an upload; `rgba` is then only read for its shape (array or (H, W))."""
        if on_device:
            H, W = rgba.shape[:2] if hasattr(rgba, "shape") else rgba
            src = None
        else:
            rgba = np.ascontiguousarray(rgba, np.uint8)
            H, W = rgba.shape[:2]
            src = _ptr(rgba)
        t = [np.ascontiguousarray(a, np.int32) for a in (col_lo, col_hi, row_lo, row_hi)]
        nx, ny = t[0].size // 256, t[2].size // 256
        out = np.empty((ny, nx, 256, 256, 4), np.uint8) if fetch else None
        self._check(self._lib.s2sr_tiles_base_u8(self._h, src, H, W, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]),
                                                 _ptr(t[3]), nx, ny, _ptr(out) if fetch else None), "s2sr_tiles_base_u8")
        return out

    def tiles_overview_u8(self, child, ox: int, oy: int, pnx: int, pny: int, on_device: bool = False,
                          fetch: bool = True) -> Optional[np.ndarray]:
        """on_device: the children are the level the previous tiles_base_u8 / tiles_overview_u8 call on this engine produced and
        nothing else ran on the engine since: its device copy is used instead of an upload; `child` is then only read for its
        shape (the array, or a (cny, cnx) pair).  fetch=False: the new level stays on the device, returns None."""
        out = np.empty((pny, pnx, 256, 256, 4), np.uint8) if fetch else None
        if on_device:
            cny, cnx = child.shape[:2] if hasattr(child, "shape") else child
            src = None
        else:
            child = np.ascontiguousarray(child, np.uint8)
            cny, cnx = child.shape[:2]
            src = _ptr(child)
        self._check(self._lib.s2sr_tiles_overview_u8(self._h, src, cnx, cny, ox, oy, pnx, pny, _ptr(out) if fetch else None),
                    "s2sr_tiles_overview_u8")
        return out

    def tiles_resample_u8(self, src, cols, rows, nx: int, ny: int, level_shape=None, on_device: bool = False,
                          fetch: bool = True) -> Optional[np.ndarray]:
        """A level through tap tables (s2sr_tiles_resample_u8): cols / rows = (first, count, coef[, K]) of nx*256 / ny*256 samples,
        as s2sr.tiles.plan_resample_axis returns them.  src: an RGBA raster [H, W, 4], or a level [cny, cnx, 256, 256, 4].
        on_device: the source is what the previous call on this engine left on the device -- the raster of warp_bilinear_u8, or with
        level_shape = (cny, cnx) the level of a tiles call -- and `src` is then only read for its shape (an array, (H, W), or
        None with level_shape).  fetch=False: the level stays on the device, returns None."""
        is_level = level_shape is not None or (hasattr(src, "ndim") and src.ndim == 5)
        if on_device:
            sa, sb = level_shape if level_shape is not None else (src.shape[:2] if hasattr(src, "shape") else src)
            ptr = None
        else:
            src = np.ascontiguousarray(src, np.uint8)
            if src.shape[-1] != 4 or (is_level and src.shape[2:4] != (256, 256)) or (level_shape is not None and tuple(level_shape) != src.shape[:2]):
                raise ValueError(f"expected [H, W, 4] or [cny, cnx, 256, 256, 4] uint8, got {src.shape}")
            sa, sb = src.shape[:2]
            ptr = _ptr(src)
        t = []
        for first, count, coef in (cols[:3], rows[:3]):
            first, count, coef = (np.ascontiguousarray(a, np.int32) for a in (first, count, coef))
            if coef.ndim != 2 or first.shape != (coef.shape[0],) or count.shape != first.shape:
                raise ValueError(f"tap tables: first {first.shape}, count {count.shape}, coef {coef.shape}")
            t.append((first, count, coef))
        if t[0][0].size != nx * 256 or t[1][0].size != ny * 256:
            raise ValueError(f"{nx} x {ny} tiles, tables of {t[0][0].size} columns and {t[1][0].size} rows")
        out = np.empty((ny, nx, 256, 256, 4), np.uint8) if fetch else None
        self._check(self._lib.s2sr_tiles_resample_u8(self._h, ptr, 1 if is_level else 0, int(sa), int(sb),
                                                     _ptr(t[0][0]), _ptr(t[0][1]), _ptr(t[0][2]), t[0][2].shape[1],
                                                     _ptr(t[1][0]), _ptr(t[1][1]), _ptr(t[1][2]), t[1][2].shape[1],
                                                     nx, ny, _ptr(out) if fetch else None), "s2sr_tiles_resample_u8")
        return out

    def tiles_write_png(self, nx: int, ny: int, paths, skip_transparent: bool = True, host_encoder: bool = False,
                        row_threads: bool = False, small_groups: bool = False) -> np.ndarray:
        """The PNG files of the level the previous tiles call left on the device, encoded there (s2sr_tiles_write_png): `paths` has
        ny * nx entries in the tile array's order (None = skip).  Returns the 0/1 array [ny, nx] of files written."""
        if len(paths) != nx * ny:
            raise ValueError(f"{nx * ny} tiles, {len(paths)} paths")
        cp = (C.c_char_p * (nx * ny))(*[None if p is None else os.fsencode(p) for p in paths])
        written = np.zeros(nx * ny, np.int32)
        self._check(self._lib.s2sr_tiles_write_png(self._h, nx, ny, cp, int(skip_transparent) | (2 if host_encoder else 0) | (4 if row_threads else 0)
                                                   | (8 if small_groups else 0), written.ctypes.data_as(C.POINTER(C.c_int32))),
                    "s2sr_tiles_write_png")
        return written.reshape(ny, nx)

    def tiles_write_png_xyz(self, nx: int, ny: int, directory, zoom: int, x0: int, y_rows, skip_transparent: bool = True) -> np.ndarray:
        """tiles_write_png for the XYZ layout: tile (j, i) -> <directory>/<zoom>/<x0 + i>/<y_rows[j]>.png; the paths are built natively."""
        rows = np.ascontiguousarray(y_rows, np.int32)
        if rows.size != ny:
            raise ValueError(f"{ny} tile rows, {rows.size} row numbers")
        written = np.zeros(nx * ny, np.int32)
        self._check(self._lib.s2sr_tiles_write_png_xyz(self._h, nx, ny, os.fsencode(str(directory)), zoom, x0, _ptr(rows),
                                                       1 if skip_transparent else 0, written.ctypes.data_as(C.POINTER(C.c_int32))),
                    "s2sr_tiles_write_png_xyz")
        return written.reshape(ny, nx)

    def synchronize(self):
        self._check(self._lib.s2sr_synchronize(self._h), "s2sr_synchronize")

    def graph_stats(self) -> tuple[int, int]:
        """(groups captured into hipGraphs, graph replays) since the engine was created."""
        c, r = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.s2sr_graph_stats(self._h, C.byref(c), C.byref(r)), "s2sr_graph_stats")
        return int(c.value), int(r.value)

    # -- test hook --------------------------------------------------------------------------
    def debug_conv(self, x: np.ndarray, weight: np.ndarray, bias: np.ndarray, upsample: bool = False,
                   act: bool = False, backwards: bool = False) -> np.ndarray:
        # backwards: the launch walks its patches back to front (bit 8 of the hook's `act`; same bytes)
        x = np.ascontiguousarray(x, dtype=np.float32)
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        N, cin, H, W = x.shape
        cout = weight.shape[0]
        assert weight.shape == (cout, cin, 3, 3) and bias.shape == (cout,)
        s = 2 if upsample else 1
        y = np.empty((N, cout, s * H, s * W), dtype=np.float32)
        self._check(self._lib.s2sr_debug_conv(self._h, _ptr(x), N, cin, H, W, _ptr(weight), _ptr(bias), cout,
                                              int(upsample), int(act) | (WALK_BACKWARDS if backwards else 0), _ptr(y)), "s2sr_debug_conv")
        return y


TRUNK_F16_CONV14, TRUNK_F16_CONV5, TRUNK_F16_CONV5_RRDB, TRUNK_F8_CONV14, TRUNK_F8_CONV5, TRUNK_F8_CONV5_RRDB = range(6)
WALK_BACKWARDS = 0x100      # bit 8 of s2sr_debug_conv_trunk's `form` / s2sr_debug_conv's `act`: the launch's patches back to front


def _debug_config(self) -> dict:
    """What s2sr_create read from the environment for this handle (kernel forms, scales)."""
    c = DebugConfig()
    self._check(self._lib.s2sr_debug_get_config(self._h, C.byref(c)), "s2sr_debug_get_config")
    d = {n: int(getattr(c, n)) for n, _ in DebugConfig._fields_ if n != "reserved"}
    d["mosaic_on"] = int(c.reserved[0])
    d["f16_loader"] = int(c.reserved[1])
    d["last_fold"] = int(c.reserved[2])
    d["tail_w4"] = int(c.reserved[3])
    d["f16_full"] = int(c.reserved[4])
    d["serpentine"] = int(c.fp8_form)       # the launch-order mask travels in the retired fp8_form slot
    d["ws_allocs"] = int(c.reserved[5])
    return d


def _debug_conv_trunk(self, kind, x, weight, bias, lo=None, skip=None, form=0, backwards=False):
    """One RDB-shaped conv through conv_trunk_f16 / conv_trunk_f8 (include/s2sr.h: s2sr_debug_conv_trunk).
    backwards: the launch walks its patches back to front (WALK_BACKWARDS in `form`; same bytes).
    Returns y, or (y, y_aux) for the fp8 conv5 kinds."""
    x = np.ascontiguousarray(x, np.float32)
    weight = np.ascontiguousarray(weight, np.float32)
    bias = np.ascontiguousarray(bias, np.float32)
    N, cin, H, W = x.shape
    cout = weight.shape[0]
    assert weight.shape == (cout, cin, 3, 3) and bias.shape == (cout,)
    y = np.empty((N, cout, H, W), np.float32)
    aux = np.empty((N, 64, H, W), np.float32) if kind in (TRUNK_F8_CONV5, TRUNK_F8_CONV5_RRDB) else None
    lo = None if lo is None else np.ascontiguousarray(lo, np.float32)
    skip = None if skip is None else np.ascontiguousarray(skip, np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    args = DebugTrunkArgs(kind, form | (WALK_BACKWARDS if backwards else 0), N, cin, H, W, p(x), p(weight), p(bias), p(lo), p(skip), p(y), p(aux))
    self._check(self._lib.s2sr_debug_conv_trunk(self._h, C.byref(args)), "s2sr_debug_conv_trunk")
    return y if aux is None else (y, aux)


def _debug_forward_taps(self, tiles=None, x=None, job_windows=0):
    """One batch through the production forward, eagerly, then every tensor the head / tail convs read or write
    (include/s2sr.h: s2sr_debug_forward_taps).  Pass u8 `tiles` [B, th, tw, 3] or fp32 `x` [B, 3, th, tw].
    Returns (geometry dict, {tap name: fp32 [n, C, Hp, Wp]} of the taps this mode has, out_f32 [B, 3, 4th, 4tw], out_u8 [B, 4th, 4tw, 3])."""
    assert (tiles is None) != (x is None)
    if tiles is not None:
        tiles = np.ascontiguousarray(tiles, np.uint8)
        B, th, tw, c = tiles.shape
        assert c == 3
    else:
        x = np.ascontiguousarray(x, np.float32)
        B, c, th, tw = x.shape
        assert c == 3
    t = DebugTaps()
    call = lambda: self._check(self._lib.s2sr_debug_forward_taps(self._h, None if tiles is None else _ptr(tiles), None if x is None else _ptr(x),
                                                                 B, th, tw, int(job_windows), C.byref(t)), "s2sr_debug_forward_taps")
    call()                                  # geometry only
    geo = {"n": t.n, "H": list(t.H), "W": list(t.W), "Hp": list(t.Hp), "Wp": list(t.Wp), "mos_kx": t.mos_kx, "mos_ky": t.mos_ky,
           "mos_wh": t.mos_wh, "mos_ww": t.mos_ww, "mos_count": t.mos_count, "trunk_lo_exp": t.trunk_lo_exp}
    taps = {}
    for i, name in enumerate(TAP_NAMES):
        if t.avail >> i & 1:
            ch, k = TAP_SHAPE[name]
            taps[name] = np.zeros((t.n, ch, t.Hp[k], t.Wp[k]), np.float32)
            t.tap[i] = taps[name].ctypes.data
    S = self.scale
    out_f32 = np.zeros((B, 3, S * th, S * tw), np.float32)
    out_u8 = np.zeros((B, S * th, S * tw, 3), np.uint8)
    t.out_f32, t.out_u8 = out_f32.ctypes.data, out_u8.ctypes.data
    call()
    return geo, taps, out_f32, out_u8


def _debug_trunk_taps(self, first, count, tiles=None, x=None, job_windows=0):
    """One batch through the production forward, eagerly, with the trunk fields of the RDBs [first, first + count) copied out at
    every RDB boundary (include/s2sr.h: s2sr_debug_trunk_taps).  Input as debug_forward_taps.
    Returns (geometry dict, fields, forms, out_f32 [B, 3, 4th, 4tw], out_u8 [B, 4th, 4tw, 3]).  fields (fp32, padded extent):
    x_hi / x_lo [count + 1, n, 64, Hp, Wp], growth [count, n, 128, Hp, Wp], skip_hi / skip_lo [count, n, 64, Hp, Wp] (zero
    where the RDB is no rdb3), entry_lo [n, 64, Hp, Wp] (first == 0, fp16 path; else zero).  forms: [count][5] dicts of
    TRUNK_FORM_FIELDS, conv1..conv5 of each RDB."""
    assert (tiles is None) != (x is None)
    if tiles is not None:
        tiles = np.ascontiguousarray(tiles, np.uint8)
        B, th, tw, c = tiles.shape
    else:
        x = np.ascontiguousarray(x, np.float32)
        B, c, th, tw = x.shape
    assert c == 3
    t = DebugTrunkFields()
    t.first, t.count = int(first), int(count)
    call = lambda: self._check(self._lib.s2sr_debug_trunk_taps(self._h, None if tiles is None else _ptr(tiles), None if x is None else _ptr(x),
                                                               B, th, tw, int(job_windows), C.byref(t)), "s2sr_debug_trunk_taps")
    call()                                  # geometry only
    geo = {k: getattr(t, k) for k in ("n", "H", "W", "Hp", "Wp", "mos_kx", "mos_ky", "mos_wh", "mos_ww", "mos_count", "fp8",
                                       "lo_exp", "x_exp", "g_exp")}
    n, Hp, Wp = t.n, t.Hp, t.Wp
    fields = {"x_hi": np.zeros((count + 1, n, 64, Hp, Wp), np.float32), "x_lo": np.zeros((count + 1, n, 64, Hp, Wp), np.float32),
              "growth": np.zeros((count, n, 128, Hp, Wp), np.float32), "skip_hi": np.zeros((count, n, 64, Hp, Wp), np.float32),
              "skip_lo": np.zeros((count, n, 64, Hp, Wp), np.float32), "entry_lo": np.zeros((n, 64, Hp, Wp), np.float32)}
    for k, a in fields.items():
        setattr(t, k, a.ctypes.data)
    forms = (DebugTrunkForm * (5 * count))()
    t.form = C.addressof(forms)
    out_f32 = np.zeros((B, 3, 4 * th, 4 * tw), np.float32)
    out_u8 = np.zeros((B, 4 * th, 4 * tw, 3), np.uint8)
    t.out_f32, t.out_u8 = out_f32.ctypes.data, out_u8.ctypes.data
    call()
    fl = [[{k: getattr(forms[5 * i + c5], k) for k in TRUNK_FORM_FIELDS} for c5 in range(5)] for i in range(count)]
    return geo, fields, fl, out_f32, out_u8


def _debug_compact_taps(self, layers, tiles=None, x=None, job_windows=0):
    """Compact engines: one batch through the production forward, eagerly, with the fp16 activation copied out behind each layer
    of `layers` (ascending; 0 = the first conv, k = body conv k; include/s2sr.h: s2sr_debug_compact_taps).  Input as
    debug_forward_taps.  Returns (geometry dict, {layer: [n, 64, Hp, Wp] fp32}, p0 [n, 16, Hp, Wp], out_f32, out_u8)."""
    assert (tiles is None) != (x is None)
    if tiles is not None:
        tiles = np.ascontiguousarray(tiles, np.uint8)
        B, th, tw, c = tiles.shape
    else:
        x = np.ascontiguousarray(x, np.float32)
        B, c, th, tw = x.shape
    assert c == 3
    layers = [int(v) for v in layers]
    t = DebugCompactFields()
    t.nlayers = len(layers)
    for k, v in enumerate(layers):
        t.layers[k] = v
    call = lambda: self._check(self._lib.s2sr_debug_compact_taps(self._h, None if tiles is None else _ptr(tiles), None if x is None else _ptr(x),
                                                                 B, th, tw, int(job_windows), C.byref(t)), "s2sr_debug_compact_taps")
    call()                                  # geometry only
    geo = {k: getattr(t, k) for k in ("n", "H", "W", "Hp", "Wp", "mos_kx", "mos_ky", "mos_wh", "mos_ww", "mos_count")}
    acts = {v: np.zeros((t.n, 64, t.Hp, t.Wp), np.float32) for v in layers}
    for k, v in enumerate(layers):
        t.act[k] = acts[v].ctypes.data
    p0 = np.zeros((t.n, 16, t.Hp, t.Wp), np.float32)
    out_f32 = np.zeros((B, 3, 4 * th, 4 * tw), np.float32)
    out_u8 = np.zeros((B, 4 * th, 4 * tw, 3), np.uint8)
    t.p0, t.out_f32, t.out_u8 = p0.ctypes.data, out_f32.ctypes.data, out_u8.ctypes.data
    call()
    return geo, acts, p0, out_f32, out_u8


def redzone(nbytes: int):
    """Red zones of `nbytes` (0: off; a multiple of 4096) around every device allocation the library makes from now on
    (include/s2sr.h: s2sr_debug_redzone).  Process-wide; a diagnostic."""
    rc = load_library().s2sr_debug_redzone(int(nbytes))
    if rc:
        raise S2srError(f"s2sr_debug_redzone({nbytes}) failed ({_ERR.get(rc, rc)}): 0 or a multiple of 4096")


def redzone_bytes() -> int:
    """The zone size in force (0: off): what a caller that switches the mode puts back."""
    return int(load_library().s2sr_debug_redzone_bytes())


def _redzone_check(self) -> tuple:
    """(zoned allocations this engine owns, damaged zones in the process since the last check, the first damage's description or
    ""): include/s2sr.h s2sr_debug_redzone_check."""
    n, bad = C.c_int64(0), C.c_int64(0)
    self._check(self._lib.s2sr_debug_redzone_check(self._h, C.byref(n), C.byref(bad)), "s2sr_debug_redzone_check")
    msg = self._lib.s2sr_last_error(self._h) if bad.value else b""
    return int(n.value), int(bad.value), (msg or b"").decode()


def _redzone_poke(self, slot: int, offset: int):
    """The negative control: one wrong byte into the back (offset >= 0) or front (offset < 0) zone of scratch buffer `slot`."""
    self._check(self._lib.s2sr_debug_redzone_poke(self._h, int(slot), int(offset)), "s2sr_debug_redzone_poke")


Engine.redzone_check = _redzone_check
Engine.redzone_poke = _redzone_poke

SCRATCH_SLOTS, TRASH_BYTES = 8, 8192            # include/s2sr.h S2SR_SCRATCH_SLOTS, S2SR_TRASH_BYTES


def poison(pattern: int):
    """Fill every device and page-locked allocation the library makes from now on with a pattern (include/s2sr.h:
    s2sr_debug_poison): 0 off, 1 every byte 0xFF, 2 a position-dependent non-zero byte.  Process-wide; a diagnostic."""
    rc = load_library().s2sr_debug_poison(int(pattern))
    if rc:
        raise S2srError(f"s2sr_debug_poison({pattern}) failed ({_ERR.get(rc, rc)}): 0, 1 or 2")


def poison_pattern() -> int:
    """The pattern in force (0: off): what a caller that switches the mode puts back."""
    return int(load_library().s2sr_debug_poison_pattern())


def poison_byte(pattern: int, i):
    """Byte(s) i of a range poisoned with `pattern` (csrc/redzone.h poison::byte_at), for the controls."""
    i = np.asarray(i, dtype=np.uint64)
    if pattern == 1:
        return np.full(i.shape, 0xFF, np.uint8)
    return (((i * np.uint64(167) + (i >> np.uint64(8)) * np.uint64(13) + np.uint64(0x5B)) & np.uint64(0xFF)) | np.uint64(1)).astype(np.uint8)


def _poison_scratch(self) -> dict:
    """Fill this engine's scratch slots and trash page with the pattern in force and forget what the last call left there
    (include/s2sr.h s2sr_debug_poison_scratch).  Returns {slot: capacity in bytes} of the slots filled."""
    mask, cap = C.c_int64(0), (C.c_int64 * SCRATCH_SLOTS)()
    self._check(self._lib.s2sr_debug_poison_scratch(self._h, C.byref(mask), cap), "s2sr_debug_poison_scratch")
    return {i: int(cap[i]) for i in range(SCRATCH_SLOTS) if mask.value >> i & 1}


def _scratch_peek(self, slot: int, offset: int, n: int) -> np.ndarray:
    """n bytes at `offset` of scratch slot `slot` (-1: the trash page): include/s2sr.h s2sr_debug_scratch_peek."""
    out = np.empty(int(n), np.uint8)
    self._check(self._lib.s2sr_debug_scratch_peek(self._h, int(slot), int(offset), int(n), out.ctypes.data), "s2sr_debug_scratch_peek")
    return out


Engine.poison_scratch = _poison_scratch
Engine.scratch_peek = _scratch_peek

STALL_MAX_USEC = 20000                          # include/s2sr.h S2SR_DEBUG_STALL_MAX_USEC
# the ordering sites whose waits s2sr_debug_delay_drop accepts (include/s2sr.h S2SR_SITE_*)
SITE_BATCH_GROUP_D2H, SITE_CHUNK_BAND_D2H, SITE_DISPLAY_BAND_D2H, SITE_COPY_TO_HOST = 0, 2, 6, 7
DROPPABLE_SITES = (SITE_BATCH_GROUP_D2H, SITE_CHUNK_BAND_D2H, SITE_DISPLAY_BAND_D2H, SITE_COPY_TO_HOST)


def delay(mode: int, usec: int = 0):
    """Stall the compute side (mode bit 1) and / or the copy side (bit 2) for `usec` microseconds at the head of every stream
    segment (include/s2sr.h: s2sr_debug_delay); 0 turns the mode off.  Process-wide; a diagnostic."""
    rc = load_library().s2sr_debug_delay(int(mode), int(usec))
    if rc:
        raise S2srError(f"s2sr_debug_delay({mode}, {usec}) failed ({_ERR.get(rc, rc)}): mode 0..3, 1..{STALL_MAX_USEC} microseconds")


def delay_mode() -> tuple:
    """(mode, microseconds) in force ((0, 0): off): what a caller that switches the mode puts back."""
    lib = load_library()
    return int(lib.s2sr_debug_delay_mode()), int(lib.s2sr_debug_delay_usec())


def delay_drop(site: int):
    """The negative control: while the mode is on, skip the stream-waits of one droppable ordering site (-1: none)."""
    rc = load_library().s2sr_debug_delay_drop(int(site))
    if rc:
        raise S2srError(f"s2sr_debug_delay_drop({site}) failed ({_ERR.get(rc, rc)}): only a wait in front of a copy of finished pixels can be dropped")


def delay_dropped() -> int:
    return int(load_library().s2sr_debug_delay_dropped())


def _stall(self, which: int, usec: int, stream: int = 0):
    """One stall of `usec` microseconds on the engine's stream (which 0), its copy stream (1) or `stream` (2)."""
    self._check(self._lib.s2sr_debug_stall(self._h, int(which), C.c_void_p(stream), int(usec)), "s2sr_debug_stall")


def _stream_touch(self, which: int, stream: int = 0, wait: bool = True):
    """A 64-byte memset on that stream (which as in stall); wait: returns when the stream is idle."""
    self._check(self._lib.s2sr_debug_stream_touch(self._h, int(which), C.c_void_p(stream), int(bool(wait))), "s2sr_debug_stream_touch")


Engine.stall = _stall
Engine.stream_touch = _stream_touch


def expected_blob_floats_cfg(num_block: int, scale: int = 4, arch: str = "rrdb") -> int:
    cfg = _Config(num_block, 64, 32, scale, PREC_F16, 0, 0, _ARCH[arch])
    return int(load_library().s2sr_expected_blob_floats_cfg(C.byref(cfg)))


Engine.debug_compact_taps = _debug_compact_taps
Engine.debug_config = _debug_config
Engine.debug_trunk_taps = _debug_trunk_taps
Engine.debug_conv_trunk = _debug_conv_trunk
Engine.debug_forward_taps = _debug_forward_taps


def _bench_conv(self, N, H, W, cin, cout, iters=20, trace_wgs=0):
    """Diagnostic: (avg launch us, trace[wgs,24] of s_memtime ticks or None)."""
    us = C.c_float(0)
    tr = np.zeros((max(trace_wgs, 1), 24), dtype=np.uint64)
    self._check(self._lib.s2sr_debug_bench_conv(self._h, N, H, W, cin, cout, iters, C.byref(us),
                                                _ptr(tr) if trace_wgs else None, trace_wgs), "s2sr_debug_bench_conv")
    return float(us.value), (tr if trace_wgs else None)


Engine.bench_conv = _bench_conv


def device_count() -> int:
    return int(load_library().s2sr_device_count())

GRID_CAP_MAX, GRID_CAP_FAMILIES = 1048576, 11   # include/s2sr.h S2SR_DEBUG_GRID_CAP_MAX, S2SR_GRID_CAP_FAMILIES


def grid_cap(workgroups: int):
    """At most `workgroups` workgroups for every launch whose kernel loops over its grid (include/s2sr.h: s2sr_debug_grid_cap; the
    conv kernels take max(8, workgroups & ~7)); 0 turns the mode off.  Read when a launch is enqueued: a captured graph keeps its
    grids.  Process-wide; a diagnostic."""
    rc = load_library().s2sr_debug_grid_cap(int(workgroups))
    if rc:
        raise S2srError(f"s2sr_debug_grid_cap({workgroups}) failed ({_ERR.get(rc, rc)}): 0 or 1..{GRID_CAP_MAX}")


def grid_cap_workgroups() -> int:
    """The cap in force (0: off): what a caller that switches the mode puts back."""
    return int(load_library().s2sr_debug_grid_cap_workgroups())


def grid_cap_families() -> tuple:
    """the launcher families of grid_cap_stats, in the library's order"""
    lib = load_library()
    return tuple(lib.s2sr_debug_grid_cap_family(i).decode() for i in range(GRID_CAP_FAMILIES))


def grid_cap_stats(reset: bool = False) -> dict:
    """{family: (launches the cap made smaller, the largest ceil(work items / workgroups) among them)} since the last reset
    (include/s2sr.h s2sr_debug_grid_cap_stats); reset: start counting afresh afterwards."""
    lib = load_library()
    launches, trips, n = (C.c_int64 * GRID_CAP_FAMILIES)(), (C.c_int64 * GRID_CAP_FAMILIES)(), C.c_int32(0)
    rc = lib.s2sr_debug_grid_cap_stats(launches, trips, GRID_CAP_FAMILIES, C.byref(n))
    if rc or n.value != GRID_CAP_FAMILIES:
        raise S2srError(f"s2sr_debug_grid_cap_stats failed ({_ERR.get(rc, rc)}; {n.value} families)")
    if reset:
        lib.s2sr_debug_grid_cap_stats_reset()
    return {name: (int(launches[i]), int(trips[i])) for i, name in enumerate(grid_cap_families())}
