"""ctypes binding of libcenternet_amd.so -- the C ABI declared in include/centernet_amd.h.

There is no fallback: if the HIP library has not been built (``python -c
"import __graft_entry__ as g; g.build()"`` or ``make -C centernet_amd/csrc``) every
entry point raises.  PyTorch is used only for device memory and streams; tensors
cross this boundary as raw device pointers.
"""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CENTERNET_AMD_LIB: another build of the same library (A/B measurements, tools/build_variant.sh)
LIB_PATH = os.environ.get("CENTERNET_AMD_LIB") or os.path.join(_HERE, "libcenternet_amd.so")
CSRC = os.path.join(_HERE, "csrc")

CN_OK = 0
LAYOUT_NCHW = 0
LAYOUT_NHWC = 1
DTYPE_F32 = 0
DTYPE_F16 = 1
DTYPE_F32S = 2        # fp32 values as fp16 (high, low) pairs: three fp16 MFMAs per product
CONV_X_PLAIN, CONV_Y_PLAIN, CONV_R_PLAIN, CONV_STEM_F32S, CONV_STEM_MAXPOOL = 1, 2, 4, 8, 16
CONV_STEM_Y_F32S = 32
MERGE_MAX_ROWS = 2048       # CN_MERGE_MAX_ROWS: S * K rows per image that the merge kernels take
MERGE_MAX_CLASSES = 1024    # CN_MERGE_MAX_CLASSES
TILES_MAX_ROWS = 65536      # CN_TILES_MAX_ROWS: T * K rows per frame that cn_ctdet_tiles_merge_f32 takes
POSE_TILES_MAX_ROWS = 5120  # CN_POSE_TILES_MAX_ROWS: survivors per frame that cn_multi_pose_tiles_merge_f32 holds
POSE_TILES_ONE_WAVE_ROWS = 256   # CN_POSE_TILES_ONE_WAVE_ROWS: up to there its soft-NMS runs on one wave
# flag bits of the decode entries: the #defines of the same names in include/centernet_amd.h
# (tests/test_decode_route_host.py compares them)
DECODE_SIGMOID = 1          # CN_DECODE_SIGMOID
DECODE_NO_PEAK_TEST = 512   # CN_DECODE_NO_PEAK_TEST: rank every cell (plain topk)
DECODE_PER_BAND = 2048      # CN_DECODE_PER_BAND: force the per-band select (tests / A-B)
DECODE_STATE_CLEAN = 4096   # CN_DECODE_STATE_CLEAN: the caller owns the workspace, its image state words are zero
DECODE_TWO_LAUNCHES = 8192  # CN_DECODE_TWO_LAUNCHES: the two-launch image-level form (tests / A-B)
DECODE_DDD_RAW_DEPTH = 16384    # CN_DECODE_DDD_RAW_DEPTH: cn_ddd_decode_f32 transforms the gathered depths
DECODE_MAX_K = 128          # CN_DECODE_MAX_K: where cn_ctdet_decode_f32 / cn_topk_f32 stop
DECODE_LARGE_MAX_K = 1024   # CN_DECODE_LARGE_MAX_K: cn_ctdet_decode_large_f32 / cn_topk_large_f32
EXCT_STORED_MAX_K = 64      # cn_exct_decode_f32 / cn_agnex_ct_decode_f32: K^4 scores in memory
EXCT_STREAM_MAX_K = 128     # cn_exct_decode_stream_f32 / cn_agnex_ct_decode_stream_f32
EXCT_CLAMP_ONE = 2          # CN_EXCT_CLAMP_ONE (cn_exct_decode_f32): clamp the peak-tested edge maps to 1
# forms and flags of cn_dcn_v2_route: the #defines CN_<name> of the header (tests/test_dcn_route_host.py compares them)
DCN_GATHER, DCN_GATHER_PAD, DCN_WINDOW, DCN_TEAM_T, DCN_TEAM_N, DCN_WIDE4, DCN_WIDE8 = range(7)
DCNH_WINDOW = 7      # CN_DCNH_WINDOW: the LDS-window form of DTYPE_F16 calls
DCN_FLAG_PREFETCH, DCN_FLAG_STAGGER, DCN_FLAG_TILE2D, DCN_FLAG_VEC_OUT = 1, 2, 4, 8
DCN_FORM_NAMES = ("gather", "gather_pad", "window", "team_t", "team_n", "wide4", "wide8")
# routes and variants of cn_conv2d_route: the #defines CN_<name> of the header (tests/test_conv_route_cases_host.py
# compares them)
(ROUTE_NONE, ROUTE_STEM_POOL, ROUTE_STEM, ROUTE_CONV16, ROUTE_CONV16S, ROUTE_CONV16H, ROUTE_OFFCONV, ROUTE_HALO,
 ROUTE_S2P, ROUTE_PROJ, ROUTE_IGEMM) = range(11)
CONV_ROUTE_NAMES = ("none", "stem_pool", "stem", "conv16", "conv16s", "conv16h", "offconv", "halo", "s2p", "proj",
                    "igemm")
STEM_NONE, STEM_WINDOW, STEM_PERSIST, STEM_PERSIST_F32S, STEM_16S = range(5)
C3_PERSIST, C3_TILE = 1, 2
C3_TW32, C3_WAVES8, C3_OCC4, C3_KSKIP, C3_WREG, C3_HREG = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200


def c3_prefetch(variant):
    """CN_C3_PREFETCH: taps of weight prefetch of an f32s tile kernel with an LDS weight tile."""
    return (variant >> 12) & 3


def conv_route_name(route):
    """Readable name of cn_conv_route_info.route."""
    return CONV_ROUTE_NAMES[route]


def dcn_form_name(form):
    """Readable name of cn_dcn_route_info.form, the fp16 forms included."""
    return "window_f16" if form == DCNH_WINDOW else DCN_FORM_NAMES[form]


# cn_image_desc, one image of a mixed-size batch (cn_warp_normalize_u8_f32_ragged / cn_resize_bilinear_u8_ragged)
IMAGE_DESC = np.dtype([("offset", np.uint64), ("H", np.int32), ("W", np.int32), ("pitch", np.int32),
                       ("reserved", np.int32), ("dst_to_src", np.float64, (6,)), ("scale", np.float64, (2,))])
assert IMAGE_DESC.itemsize == 88
# cn_tile_box_desc, one tile of a tile pyramid (cn_tile_box_normalize_u8_f32)
TILE_BOX_DESC = np.dtype([("offset", np.uint64), ("H", np.int32), ("W", np.int32), ("pitch", np.int32),
                          ("level", np.int32), ("y0", np.int32), ("x0", np.int32)])
assert TILE_BOX_DESC.itemsize == 32

_lib = None


class NativeError(RuntimeError):
    pass


class F32sCtl(ctypes.Structure):
    """Mirror of ``cn_f32s_ctl``: range control of the f32s kernels (multipliers that carry the
    per-tensor exponents + the device words that receive the largest |value| a launch split)."""
    _fields_ = [("x_mul", ctypes.c_float), ("res_mul", ctypes.c_float), ("range", ctypes.c_void_p)]


class DcnRouteInfo(ctypes.Structure):
    """Mirror of ``cn_dcn_route_info``: the kernel form, grid and K split of a cn_dcn_v2_forward_nhwc call."""
    _fields_ = [(n, ctypes.c_int) for n in ("form", "grid_x", "grid_y", "ksplit", "flags")]


class ConvRouteInfo(ctypes.Structure):
    """Mirror of ``cn_conv_route_info``: the kernel, its form, tile and K split of a cn_conv2d call."""
    _fields_ = [(n, ctypes.c_int) for n in ("route", "n_tile", "m_tile", "ksplit", "want", "variant", "grid_x",
                                            "grid_y")]


class ConvDesc(ctypes.Structure):
    """Mirror of ``cn_conv_desc`` (include/centernet_amd.h)."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "B", "H", "W", "Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad_h", "pad_w",
        "dil", "in_layout", "in_pitch", "out_layout", "out_pitch", "OH", "OW", "oy_mul",
        "oy_add", "ox_mul", "ox_add", "relu", "dtype", "flags", "res_pitch")] + [("ctl", F32sCtl)]


class HeadOut(ctypes.Structure):
    """Mirror of ``cn_head_out`` (include/centernet_amd.h)."""
    _fields_ = [("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("cout", ctypes.c_int), ("reserved", ctypes.c_int), ("oscale", ctypes.c_void_p),
                ("w_frag", ctypes.c_void_p)]


class CellHeadGroup(ctypes.Structure):
    """Mirror of ``cn_cell_head_group`` (include/centernet_amd.h): one group of consecutive heads of
    ``cn_ddd_heads_at_cells_f32``."""
    _fields_ = [("w1_packed", ctypes.c_void_p), ("bias1", ctypes.c_void_p), ("w2", ctypes.c_void_p),
                ("bias2", ctypes.c_void_p), ("n_heads", ctypes.c_int), ("reserved", ctypes.c_int)]


CELL_GROUP_MAX_HEADS = 3    # heads of one cn_cell_head_group
CELL_GROUPS_MAX = 5         # groups of one cn_ddd_heads_at_cells_f32 call


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        args.append("-B")
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(args, stdout=out)
    if not os.path.exists(LIB_PATH):
        raise NativeError("build did not produce %s" % LIB_PATH)
    return LIB_PATH


def _declare(lib):
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.cn_version.restype = i
    lib.cn_status_string.restype = ctypes.c_char_p
    lib.cn_status_string.argtypes = [i]
    lib.cn_arch.restype = ctypes.c_char_p
    lib.cn_set_tuning.restype = i
    lib.cn_set_tuning.argtypes = [i, i]
    lib.cn_get_tuning.restype = i
    lib.cn_get_tuning.argtypes = [i, ctypes.POINTER(i)]
    lib.cn_reset_tuning.restype = i
    lib.cn_dcn_v2_forward_workspace_bytes.restype = sz
    lib.cn_dcn_v2_forward_workspace_bytes.argtypes = [i] * 8
    lib.cn_dcn_v2_forward_f32.restype = i
    lib.cn_dcn_v2_forward_f32.argtypes = [vp] * 6 + [i] * 15 + [vp, sz, vp]
    lib.cn_dcn_v2_forward_nhwc_f32.restype = i
    lib.cn_dcn_v2_forward_nhwc_f32.argtypes = [vp, vp, vp, vp, i, vp, vp, vp] + [i] * 7 + [vp, sz, vp]
    lib.cn_dcn_v2_forward_nhwc_workspace_bytes.restype = sz
    lib.cn_dcn_v2_forward_nhwc_workspace_bytes.argtypes = [i] * 5
    lib.cn_f32_to_f32s.restype = i
    lib.cn_f32_to_f32s.argtypes = [vp, vp, sz, i, i, i, vp]
    lib.cn_f32s_to_f32.restype = i
    lib.cn_f32s_to_f32.argtypes = [vp, vp, sz, i, i, i, vp]
    f = ctypes.c_float
    ctl = ctypes.POINTER(F32sCtl)
    lib.cn_f32_to_f32s_scaled.restype = i
    lib.cn_f32_to_f32s_scaled.argtypes = [vp, vp, sz, i, i, i, f, vp, vp]
    lib.cn_f32s_to_f32_scaled.restype = i
    lib.cn_f32s_to_f32_scaled.argtypes = [vp, vp, sz, i, i, i, f, vp]
    lib.cn_absmax_f32.restype = i
    lib.cn_absmax_f32.argtypes = [vp, sz, i, i, vp, vp]
    lib.cn_range_fold.restype = i
    lib.cn_range_fold.argtypes = [vp, vp, vp, i, vp]
    lib.cn_range_fold_digest.restype = i
    lib.cn_range_fold_digest.argtypes = [vp, vp, vp, vp, i, vp]
    lib.cn_packed_head_w2_bytes.restype = sz
    lib.cn_packed_head_w2_bytes.argtypes = [i]
    lib.cn_pack_head_w2_f32s.restype = i
    lib.cn_pack_head_w2_f32s.argtypes = [vp, vp, i, vp]
    lib.cn_flip_average_f32.restype = i
    lib.cn_flip_average_f32.argtypes = [vp, vp, i, i, i, vp, vp, i, vp]
    lib.cn_flip_average_f32_batch.restype = i
    lib.cn_flip_average_f32_batch.argtypes = [vp, vp, i, i, i, i, vp, vp, i, i, vp]
    lib.cn_calib_mfma_f16.restype = ctypes.c_double
    lib.cn_calib_mfma_f16.argtypes = [vp, i, vp]
    lib.cn_calib_mfma_shape.restype = ctypes.c_double
    lib.cn_calib_mfma_shape.argtypes = [vp, vp, vp, i, i, i, vp]
    lib.cn_calib_copy.restype = i
    lib.cn_calib_copy.argtypes = [vp, vp, sz, vp]
    lib.cn_calib_clock.restype = i
    lib.cn_calib_clock.argtypes = [vp, i, vp]
    lib.cn_calib_latency.restype = i
    lib.cn_calib_latency.argtypes = [vp, ctypes.c_uint32, i, vp, vp, vp]
    lib.cn_maxpool_nhwc_f32s.restype = i
    lib.cn_maxpool_nhwc_f32s.argtypes = [vp, vp, i, i, i, i, i, i, i, i, i, f, vp, vp]
    lib.cn_maxpool_nhwc_f16.restype = i
    lib.cn_maxpool_nhwc_f16.argtypes = [vp, vp, i, i, i, i, i, i, i, i, i, vp]
    lib.cn_maxpool_nhwc_scaled.restype = i
    lib.cn_maxpool_nhwc_scaled.argtypes = [vp, vp, i, i, i, i, i, i, i, i, f, vp]
    lib.cn_dcn_v2_forward_nhwc.restype = i
    lib.cn_dcn_v2_forward_nhwc.argtypes = [vp, vp, vp, vp, i, vp, vp, vp] + [i] * 10 + [ctl, vp, sz, vp]
    lib.cn_dcn_v2_route.restype = i
    lib.cn_dcn_v2_route.argtypes = lib.cn_dcn_v2_forward_nhwc.argtypes + [ctypes.POINTER(DcnRouteInfo)]
    lib.cn_dcn_v2_forward_nhwc_f16.restype = i
    lib.cn_dcn_v2_forward_nhwc_f16.argtypes = [vp, vp, vp, vp, i, vp, vp, vp] + [i] * 8 + [vp, sz, vp]
    lib.cn_dcn_v2_forward_nhwc_f16_rects.restype = i
    lib.cn_dcn_v2_forward_nhwc_f16_rects.argtypes = [vp, vp, vp, vp, i, vp, vp, vp] + [i] * 8 + [vp, sz, vp, i, vp]
    lib.cn_dcn_v2_route_f16.restype = i
    lib.cn_dcn_v2_route_f16.argtypes = lib.cn_dcn_v2_forward_nhwc_f16.argtypes + [ctypes.POINTER(DcnRouteInfo)]
    lib.cn_pack_deconv4x4s2_weight.restype = i
    lib.cn_pack_deconv4x4s2_weight.argtypes = [vp, vp, i, i, i, vp]
    lib.cn_conv_transpose4x4s2.restype = i
    lib.cn_conv_transpose4x4s2.argtypes = [vp, vp, vp, vp, vp] + [i] * 10 + [ctl, vp]
    lib.cn_heads3x3_1x1.restype = i
    lib.cn_heads3x3_1x1.argtypes = [vp, i, i, i, i, i, vp, vp, vp, i, i, vp, i, i, ctl, vp]
    lib.cn_conv_transpose4x4s2_route.restype = i
    lib.cn_conv_transpose4x4s2_route.argtypes = lib.cn_conv_transpose4x4s2.argtypes + [ctypes.POINTER(ConvRouteInfo)]
    lib.cn_heads3x3_1x1_route.restype = i
    lib.cn_heads3x3_1x1_route.argtypes = lib.cn_heads3x3_1x1.argtypes + [ctypes.POINTER(ConvRouteInfo)]
    lib.cn_packed_conv_weight_floats.restype = sz
    lib.cn_packed_conv_weight_floats.argtypes = [i] * 4
    lib.cn_pack_conv_weight_f32.restype = i
    lib.cn_pack_conv_weight_f32.argtypes = [vp, vp, i, i, i, i, vp]
    lib.cn_stem_maxpool_supported.restype = i
    lib.cn_stem_maxpool_supported.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.cn_stem_f32s_supported.restype = i
    lib.cn_stem_f32s_supported.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.cn_conv16_f16_supported.restype = i
    lib.cn_conv16_f16_supported.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.cn_conv2d_f32.restype = i
    lib.cn_conv2d_f32.argtypes = [ctypes.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp]
    lib.cn_packed_conv_weight_elems.restype = sz
    lib.cn_packed_conv_weight_elems.argtypes = [i] * 5
    lib.cn_pack_conv_weight.restype = i
    lib.cn_pack_conv_weight.argtypes = [vp, vp, i, i, i, i, i, vp]
    lib.cn_conv2d_res_pitch_supported.restype = i
    lib.cn_conv2d_res_pitch_supported.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.cn_conv2d_workspace_bytes.restype = sz
    lib.cn_conv2d_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.cn_conv2d.restype = i
    lib.cn_conv2d.argtypes = [ctypes.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.cn_conv2d_route.restype = i
    lib.cn_conv2d_route.argtypes = lib.cn_conv2d.argtypes + [ctypes.POINTER(ConvRouteInfo)]
    lib.cn_upsample2x_add_f16.restype = i
    lib.cn_upsample2x_add_f16.argtypes = [vp, vp, vp, i, i, i, i, vp]
    lib.cn_packed_deconv4x4s2_weight_floats.restype = sz
    lib.cn_packed_deconv4x4s2_weight_floats.argtypes = [i, i]
    lib.cn_pack_deconv4x4s2_weight_f32.restype = i
    lib.cn_pack_deconv4x4s2_weight_f32.argtypes = [vp, vp, i, i, vp]
    lib.cn_conv_transpose4x4s2_f32.restype = i
    lib.cn_conv_transpose4x4s2_f32.argtypes = [vp] * 5 + [i] * 8 + [vp]
    lib.cn_maxpool3x3s2_nhwc_f32.restype = i
    lib.cn_maxpool3x3s2_nhwc_f32.argtypes = [vp, vp, i, i, i, i, vp]
    lib.cn_maxpool_nhwc_f32.restype = i
    lib.cn_maxpool_nhwc_f32.argtypes = [vp, vp, i, i, i, i, i, i, i, vp]
    lib.cn_maxpool_nhwc.restype = i
    lib.cn_maxpool_nhwc.argtypes = [vp, vp, i, i, i, i, i, i, i, i, vp]
    lib.cn_dw_conv_transpose_f32.restype = i
    lib.cn_dw_conv_transpose_f32.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp]
    lib.cn_copy_channels_f32.restype = i
    lib.cn_copy_channels_f32.argtypes = [vp, i, vp, i, sz, i, vp]
    lib.cn_dw_conv_transpose_f16.restype = i
    lib.cn_dw_conv_transpose_f16.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp]
    lib.cn_copy_channels_f16.restype = i
    lib.cn_copy_channels_f16.argtypes = [vp, i, vp, i, sz, i, vp]
    lib.cn_upsample2x_add_f32.restype = i
    lib.cn_upsample2x_add_f32.argtypes = [vp, vp, vp, i, i, i, i, vp]
    lib.cn_mask_rects_f32.restype = i
    lib.cn_mask_rects_f32.argtypes = [vp, i, i, i, i, i, i, vp, i, vp]
    lib.cn_mask_rects_f16.restype = i
    lib.cn_mask_rects_f16.argtypes = [vp, i, i, i, i, i, i, vp, i, vp]
    lib.cn_mask_rects_nchw_f32.restype = i
    lib.cn_mask_rects_nchw_f32.argtypes = [vp, i, i, i, i, vp, i, f, vp]
    lib.cn_heads3x3_1x1_f32.restype = i
    lib.cn_heads3x3_1x1_f32.argtypes = [vp, i, i, i, i, i, vp, vp, i, i, ctypes.POINTER(HeadOut), vp]
    lib.cn_warp_normalize_u8_f32.restype = i
    lib.cn_warp_normalize_u8_f32.argtypes = [vp, i, i, i, ctypes.POINTER(ctypes.c_double), i, i,
                                             ctypes.POINTER(ctypes.c_float),
                                             ctypes.POINTER(ctypes.c_float), i, vp, vp]
    lib.cn_warp_normalize_u8_f32_batch.restype = i
    lib.cn_warp_normalize_u8_f32_batch.argtypes = [vp, i, sz, i, i, i, ctypes.POINTER(ctypes.c_double), i, i,
                                                   ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                                   i, vp, vp]
    lib.cn_warp_normalize_u8_f32_ragged.restype = i
    lib.cn_warp_normalize_u8_f32_ragged.argtypes = [vp, vp, i, i, i, ctypes.POINTER(ctypes.c_float),
                                                    ctypes.POINTER(ctypes.c_float), i, vp, vp]
    lib.cn_resize_bilinear_u8_ragged.restype = i
    lib.cn_resize_bilinear_u8_ragged.argtypes = [vp, vp, vp, vp, i, i, i, vp]
    lib.cn_warp_table_u8_f32_batch.restype = i
    lib.cn_warp_table_u8_f32_batch.argtypes = [vp, i, sz, i, i, i, ctypes.POINTER(ctypes.c_double), i, i, vp, vp, vp]
    lib.cn_warp_table_u8_f32_ragged.restype = i
    lib.cn_warp_table_u8_f32_ragged.argtypes = [vp, vp, i, i, i, vp, vp, vp]
    lib.cn_ddd_post_process_f32.restype = i
    lib.cn_ddd_post_process_f32.argtypes = [vp, i, i, i, i, vp, i, vp, ctypes.c_float, vp, vp, vp, vp]
    lib.cn_ctdet_post_process_f32.restype = i
    lib.cn_ctdet_post_process_f32.argtypes = [vp, i, i, i, vp, i, ctypes.c_float, vp, vp, vp]
    lib.cn_ctdet_merge_f32.restype = i
    lib.cn_ctdet_merge_f32.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp, vp]
    lib.cn_ctdet_tiles_merge_workspace_bytes.restype = sz
    lib.cn_ctdet_tiles_merge_workspace_bytes.argtypes = [i, i, i, i]
    lib.cn_ctdet_tiles_merge_f32.restype = i
    lib.cn_ctdet_tiles_merge_f32.argtypes = [vp, vp, i, i, i, i, vp, i, i, vp, vp, vp, vp, sz, vp]
    lib.cn_ctdet_tiles_merge_gated_workspace_bytes.restype = sz
    lib.cn_ctdet_tiles_merge_gated_workspace_bytes.argtypes = [i, i, i, i]
    lib.cn_ctdet_tiles_merge_gated_f32.restype = i
    lib.cn_ctdet_tiles_merge_gated_f32.argtypes = [vp, vp, i, i, i, i, vp, vp, i, i, vp, vp, vp, vp, sz, vp]
    lib.cn_tile_box_normalize_u8_f32.restype = i
    lib.cn_tile_box_normalize_u8_f32.argtypes = [vp, vp, i, i, i, ctypes.POINTER(ctypes.c_float),
                                                 ctypes.POINTER(ctypes.c_float), vp, vp]
    lib.cn_exdet_post_process_f32.restype = i
    lib.cn_exdet_post_process_f32.argtypes = [vp, i, i, i, i, vp, i, ctypes.c_float, vp, vp, vp]
    lib.cn_exdet_merge_f32.restype = i
    lib.cn_exdet_merge_f32.argtypes = [vp, vp, i, i, i, i, i, vp, vp, vp, vp]
    lib.cn_multi_pose_post_process_f32.restype = i
    lib.cn_multi_pose_post_process_f32.argtypes = [vp, i, i, vp, i, ctypes.c_float, vp, vp]
    lib.cn_multi_pose_merge_f32.restype = i
    lib.cn_multi_pose_merge_f32.argtypes = [vp, i, i, i, i, vp, vp]
    lib.cn_multi_pose_tiles_merge_workspace_bytes.restype = sz
    lib.cn_multi_pose_tiles_merge_workspace_bytes.argtypes = [i, i, i]
    lib.cn_multi_pose_tiles_merge_f32.restype = i
    lib.cn_multi_pose_tiles_merge_f32.argtypes = [vp, i, i, i, vp, i, i, ctypes.c_float, vp, vp, vp, vp, sz, vp]
    lib.cn_resize_bilinear_u8.restype = i
    lib.cn_resize_bilinear_u8.argtypes = [vp, i, i, i, i, i, vp, vp]
    lib.cn_warp_affine_u8_host.restype = i
    lib.cn_warp_affine_u8_host.argtypes = [vp, i, i, i, ctypes.POINTER(ctypes.c_double), i, i, vp]
    lib.cn_resize_linear_u8_host.restype = i
    lib.cn_resize_linear_u8_host.argtypes = [vp, i, i, i, i, i, vp]
    lib.cn_nv12_to_bgr_u8_batch.restype = i
    lib.cn_nv12_to_bgr_u8_batch.argtypes = [vp, i, sz, i, i, i, vp, vp]
    lib.cn_nv12_to_bgr_u8_host.restype = i
    lib.cn_nv12_to_bgr_u8_host.argtypes = [vp, i, i, i, vp]
    lib.cn_normalize_u8_chw_f32_host.restype = i
    lib.cn_normalize_u8_chw_f32_host.argtypes = [vp, i, i, vp, vp, vp]
    lib.cn_soft_nms_f32.restype = i
    lib.cn_soft_nms_f32.argtypes = [vp, i, i, ctypes.c_float, ctypes.c_float, ctypes.c_float, i]
    lib.cn_nchw_to_nhwc_f32.restype = i
    lib.cn_nchw_to_nhwc_f32.argtypes = [vp, vp, i, i, i, i, i, vp]
    lib.cn_nhwc_to_nchw_f32.restype = i
    lib.cn_nhwc_to_nchw_f32.argtypes = [vp, vp, i, i, i, i, i, vp]
    lib.cn_ctdet_decode_workspace_bytes.restype = sz
    lib.cn_ctdet_decode_workspace_bytes.argtypes = [i] * 5
    lib.cn_decode_state_region.restype = i
    lib.cn_decode_state_region.argtypes = [i] * 5 + [ctypes.POINTER(ctypes.c_size_t)] * 2
    lib.cn_ctdet_decode_f32.restype = i
    lib.cn_ctdet_decode_f32.argtypes = [vp, vp, vp] + [i] * 7 + [vp, vp, vp, sz, vp]
    lib.cn_nms_topk_channel_f32.restype = i
    lib.cn_nms_topk_channel_f32.argtypes = [vp] + [i] * 6 + [vp, vp, vp, sz, vp]
    lib.cn_topk_f32.restype = i
    lib.cn_topk_f32.argtypes = [vp] + [i] * 6 + [vp, vp, vp, vp, sz, vp]
    lib.cn_ctdet_decode_large_workspace_bytes.restype = sz
    lib.cn_ctdet_decode_large_workspace_bytes.argtypes = [i] * 5
    lib.cn_ctdet_decode_large_f32.restype = i
    lib.cn_ctdet_decode_large_f32.argtypes = lib.cn_ctdet_decode_f32.argtypes
    lib.cn_topk_large_f32.restype = i
    lib.cn_topk_large_f32.argtypes = lib.cn_topk_f32.argtypes
    lib.cn_pack_cell_heads_w1.restype = i
    lib.cn_pack_cell_heads_w1.argtypes = [vp, vp, i, i, vp]
    lib.cn_ctdet_heads_at_cells_f32.restype = i
    lib.cn_ctdet_heads_at_cells_f32.argtypes = [vp, i, i, i, i, i, i, ctypes.c_float, vp, vp, vp, i, vp, vp, i, i,
                                                vp, vp, vp, vp, vp]
    lib.cn_multi_pose_heads_at_cells_f32.restype = i
    lib.cn_multi_pose_heads_at_cells_f32.argtypes = [vp, i, i, i, i, i, i, ctypes.c_float, vp, vp, vp, i, vp, vp,
                                                     i, i, i, vp, vp, vp, vp, vp]
    lib.cn_ddd_heads_at_cells_f32.restype = i
    lib.cn_ddd_heads_at_cells_f32.argtypes = [vp, i, i, i, i, i, i, ctypes.c_float, vp, vp, vp, i, i, i,
                                              ctypes.POINTER(CellHeadGroup), i, i, i, vp, vp, vp]
    lib.cn_gather_feat_f32.restype = i
    lib.cn_gather_feat_f32.argtypes = [vp, vp, vp] + [i] * 5 + [vp]
    lib.cn_ddd_decode_workspace_bytes.restype = sz
    lib.cn_ddd_decode_workspace_bytes.argtypes = [i] * 5
    lib.cn_ddd_decode_f32.restype = i
    lib.cn_ddd_decode_f32.argtypes = [vp] * 6 + [i] * 6 + [vp, vp, sz, vp]
    lib.cn_exct_decode_workspace_bytes.restype = sz
    lib.cn_exct_decode_workspace_bytes.argtypes = [i] * 5
    lib.cn_exct_aggregate_f32.restype = i
    lib.cn_exct_aggregate_f32.argtypes = [vp, vp, i, i, i, i, i, ctypes.c_float, vp]
    lib.cn_exct_decode_f32.restype = i
    lib.cn_exct_decode_f32.argtypes = [vp] * 9 + [i] * 5 + [ctypes.c_float, ctypes.c_float, i, i,
                                                        vp, vp, sz, vp]
    lib.cn_agnex_ct_decode_workspace_bytes.restype = sz
    lib.cn_agnex_ct_decode_workspace_bytes.argtypes = [i] * 5
    lib.cn_agnex_ct_decode_f32.restype = i
    lib.cn_agnex_ct_decode_f32.argtypes = [vp] * 9 + [i] * 5 + [ctypes.c_float, ctypes.c_float, i, i,
                                                            vp, vp, sz, vp]
    for name in ("cn_exct_decode_stream", "cn_agnex_ct_decode_stream"):    # the forms without the K^4 array
        getattr(lib, name + "_workspace_bytes").restype = sz
        getattr(lib, name + "_workspace_bytes").argtypes = [i] * 5
        getattr(lib, name + "_f32").restype = i
        getattr(lib, name + "_f32").argtypes = lib.cn_exct_decode_f32.argtypes
    lib.cn_multi_pose_decode_workspace_bytes.restype = sz
    lib.cn_multi_pose_decode_workspace_bytes.argtypes = [i] * 6
    lib.cn_multi_pose_decode_f32.restype = i
    lib.cn_multi_pose_decode_f32.argtypes = [vp] * 6 + [i] * 7 + [vp, vp, sz, vp]
    lib.cn_multi_pose_match_f32.restype = i
    lib.cn_multi_pose_match_f32.argtypes = [vp, vp] + [i] * 6 + [vp, vp, sz, vp]


def lib():
    """Load the HIP library; raise loudly if it is missing (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                "%s is missing: build it with `make -C %s` (hipcc, gfx950). "
                "centernet_amd has no CPU or PyTorch fallback." % (LIB_PATH, CSRC))
        l = ctypes.CDLL(LIB_PATH)
        _declare(l)
        _lib = l
    return _lib


def check(rc, what):
    if rc != CN_OK:
        raise NativeError("%s failed: %s (%d)" % (what, lib().cn_status_string(rc).decode(), rc))


@contextlib.contextmanager
def tuning(knobs):
    """Run a block with ``cn_set_tuning`` keys set: ``with native.tuning({23: 2, 5: 1}): ...``.

    The values the keys had on entry are put back on exit, also when the block raises.  A key or value
    the library refuses raises NativeError (keys set before it are restored).
    """
    l = lib()
    before = {}
    for key in knobs:
        v = ctypes.c_int()
        check(l.cn_get_tuning(key, ctypes.byref(v)), "cn_get_tuning(%d)" % key)
        before[key] = v.value
    try:
        for key, value in knobs.items():
            check(l.cn_set_tuning(key, value), "cn_set_tuning(%d, %d)" % (key, value))
        yield
    finally:
        for key, value in before.items():
            l.cn_set_tuning(key, value)


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Raw device pointer of a CUDA/HIP fp32/int32 tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise NativeError("centernet_amd kernels need tensors on a HIP device (got %s); "
                          "there is no CPU path" % t.device)
    if not t.is_contiguous():
        raise NativeError("tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def require_f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise NativeError("fp32 tensors required, got %s" % t.dtype)
