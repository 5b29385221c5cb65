"""ctypes binding of libwct_hip.so (the C ABI declared in include/wct_hip.h).

The product path has no CPU fallback: if the HIP library is missing or a call fails this module raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# WCT_LIB_PATH: load an instrumented build of the same library (tools/experiments/sp_timing.sh); default = the in-tree build
LIB_PATH = os.environ.get("WCT_LIB_PATH") or os.path.join(_PKG, "libwct_hip.so")

WCT_OK, WCT_ERR_INVALID, WCT_ERR_HIP, WCT_ERR_NOMEM, WCT_ERR_STATE, WCT_ERR_RANGE = 0, -1, -2, -3, -4, -5
KIND_ENC, KIND_DEC = 0, 1
LAYOUT_NHWC, LAYOUT_NCHW = 0, 1

# every symbol include/wct_hip.h declares (tests check that the built library exports all of them)
SYMBOLS = [
    "wct_version", "wct_create", "wct_destroy", "wct_last_error", "wct_set_stream", "wct_sync", "wct_saturation_count", "wct_range_poll", "wct_range_flag_f64", "wct_debug_set", "wct_debug_get",
    "wct_load_module", "wct_feature_shape", "wct_encode", "wct_decode", "wct_moments", "wct_solve",
    "wct_apply", "wct_transform", "wct_decode_affine", "wct_style_transfer_level", "wct_stylize",
    "wct_style_prepare", "wct_content_encode", "wct_content_solve", "wct_content_decode",
    "wct_comm_load", "wct_comm_library", "wct_comm_unique_id", "wct_comm_init", "wct_comm_attach", "wct_comm_destroy", "wct_level_sharded",
    "wct_comm_attach_collectives", "wct_comm_info", "wct_comm_selftest", "wct_shard_geometry", "wct_stylize_sharded", "wct_style_moments", "wct_style_solve",
    "wct_style_prepare_levels", "wct_style_stats_count", "wct_style_export", "wct_style_import", "wct_stylize_prepared",
    "wct_u8_to_planar", "wct_planar_to_u8", "wct_stylize_u8", "wct_resize_shape", "wct_resize_u8", "wct_resize_u8_to_planar",
    "wct_moments_labeled", "wct_apply_labeled", "wct_stylize_regions",
    "wct_noise_uniform", "wct_synthesize", "wct_resize_u8_filter",
    "wct_stylize_interp", "wct_style_blend", "wct_stylize_blend", "wct_moments_weighted", "wct_apply_mixed",
    "wct_workspace_bytes", "wct_reserve", "wct_set_conv_mode", "wct_set_numpy_variant", "wct_set_overlap", "wct_profile_enable", "wct_profile_reset", "wct_profile_read",
]

# every symbol include/wct_hip_color.h declares (colour preservation); bound from the same libwct_hip.so
SYMBOLS_COLOR = ["wct_color_moments", "wct_color_solve", "wct_color_apply", "wct_color_match", "wct_luma_merge", "wct_stylize_color"]
COLOR_MATCH, COLOR_LUMA = 1, 2                                      # WCT_COLOR_*: the mode mask of wct_stylize_color
COLOR_MODES = {"match": COLOR_MATCH, "luma": COLOR_LUMA, "match+luma": COLOR_MATCH | COLOR_LUMA}
COLOR_EPS = 1e-5                                                    # WCT_COLOR_EPS

# every symbol include/wct_hip_smooth.h declares (guided-filter smoothing by the content image); bound from the same libwct_hip.so
SYMBOLS_SMOOTH = ["wct_guided_filter", "wct_stylize_smooth"]
SMOOTH_MAX_RADIUS = 2048                                            # WCT_SMOOTH_MAX_RADIUS
SMOOTH_EPS = 1e-3                                                   # WCT_SMOOTH_EPS

# every symbol include/wct_hip_transform.h declares (the choice of feature transform); bound from the same libwct_hip.so
SYMBOLS_TRANSFORM = ["wct_set_transform", "wct_get_transform", "wct_transform_solve"]
TRANSFORM_WCT, TRANSFORM_OT, TRANSFORM_ADAIN = 0, 1, 2              # WCT_TRANSFORM_*
TRANSFORMS = {"wct": TRANSFORM_WCT, "ot": TRANSFORM_OT, "adain": TRANSFORM_ADAIN}
ADAIN_EPS = 1e-5                                                    # WCT_ADAIN_EPS

# every symbol include/wct_hip_swap.h declares (patch-based style swap at one cascade level); bound from the same libwct_hip.so
SYMBOLS_SWAP = ["wct_patch_match", "wct_patch_assemble", "wct_swap_level", "wct_stylize_swap"]
SWAP_WHITENED, SWAP_RAW = 0, 1                                      # WCT_SWAP_*: the match mode
SWAP_MATCHES = {"whitened": SWAP_WHITENED, "raw": SWAP_RAW}
SWAP_EPS = 1e-12                                                    # WCT_SWAP_EPS
SWAP_KEY_CHUNK = 8192                                               # WCT_SWAP_KEY_CHUNK
SWAP_LEVELS = (2, 3, 4, 5)

# every symbol include/wct_hip_attn.h declares (attention-weighted style statistics at one cascade level); bound from the same libwct_hip.so
SYMBOLS_ATTN = ["wct_attn_project", "wct_attn_stats", "wct_attn_apply", "wct_attn_level", "wct_stylize_attn"]
ATTN_STANDARD, ATTN_WHITENED = 0, 1                                 # WCT_ATTN_*: the match domain
ATTN_MATCHES = {"attention": ATTN_STANDARD, "attention_whitened": ATTN_WHITENED}   # --swap_match names -> domain
ATTN_EPS = 1e-12                                                    # WCT_ATTN_EPS
ATTN_MAX_TEMP = 32                                                  # WCT_ATTN_MAX_TEMP
ATTN_QUERY_TILE, ATTN_KEY_TILE, ATTN_QUERY_CHUNK = 64, 32, 32768    # WCT_ATTN_QUERY_TILE, WCT_ATTN_KEY_TILE, WCT_ATTN_QUERY_CHUNK
ATTN_TEMP = 8.0                                                     # the command line's default --swap_temp

# every symbol include/wct_hip_scale.h declares (scale control: the coarse-to-fine cascade on a device image pyramid); bound from the same libwct_hip.so
SYMBOLS_SCALE = ["wct_scale_shape", "wct_resample_planar", "wct_pyramid_merge", "wct_stylize_scaled"]
SCALE_MAX_DIVISOR = 16                                              # WCT_SCALE_MAX_DIVISOR
SCALE_MAX_SHRINK = 32                                               # WCT_SCALE_MAX_SHRINK
SCALE_DETAIL = 1.0                                                  # WCT_SCALE_DETAIL

# every symbol include/wct_hip_guided.h declares (region-to-region transfer: style label maps, k-means feature regions); bound from the same libwct_hip.so
SYMBOLS_GUIDED = ["wct_stylize_guided", "wct_kmeans_assign", "wct_kmeans_seed", "wct_feature_regions"]
GUIDED_MAX_REGIONS = 8                                              # WCT_GUIDED_MAX_REGIONS
GUIDED_MAX_STYLES = 8                                               # WCT_GUIDED_MAX_STYLES
KMEANS_MAX_K = 8                                                    # WCT_KMEANS_MAX_K
KMEANS_MAX_ITERS = 64                                               # WCT_KMEANS_MAX_ITERS
KMEANS_DEAD_VARIANCE = 1e-12                                        # WCT_KMEANS_DEAD_VARIANCE

# every symbol include/wct_hip_video.h declares (video mode: tracked statistics and the temporal blend of a frame sequence); bound from the same libwct_hip.so
SYMBOLS_VIDEO = ["wct_clip_bytes", "wct_clip_create", "wct_clip_destroy", "wct_clip_reset", "wct_clip_export", "wct_moments_track", "wct_temporal_blend",
                 "wct_stylize_clip"]
CLIP_MAX_RADIUS = 8                                                 # WCT_CLIP_MAX_RADIUS
CLIP_RATE, CLIP_CUT, CLIP_BLEND, CLIP_SIGMA, CLIP_RADIUS = 0.25, 0.5, 0.6, 0.05, 2   # WCT_CLIP_*: the command line's defaults

# every symbol include/wct_hip_motion.h declares (motion compensation for video mode: block matching, the warped blend); bound from the same libwct_hip.so
SYMBOLS_MOTION = ["wct_motion_shape", "wct_motion_luma", "wct_motion_estimate", "wct_motion_blend", "wct_motion_attach", "wct_motion_export"]
MOTION_BLOCK, MOTION_MAX_LEVELS, MOTION_MAX_RANGE = 8, 4, 7         # WCT_MOTION_BLOCK, WCT_MOTION_MAX_LEVELS, WCT_MOTION_MAX_RANGE
MOTION_LEVELS, MOTION_RANGE, MOTION_PENALTY = 4, 4, 4               # WCT_MOTION_*: the command line's defaults

# every symbol include/wct_hip_diverse.h declares (seeded style variations: a rotation inside the colouring step); bound from the same libwct_hip.so
SYMBOLS_DIVERSE = ["wct_rotation_make", "wct_style_diversify", "wct_stylize_diverse"]
DIVERSE_MAX_STRENGTH = 8                                            # WCT_DIVERSE_MAX_STRENGTH
DIVERSE_LEVELS = (5,)                                               # the command line's default --diversity_levels

# every symbol include/wct_hip_bgrid.h declares (proxy mode: stylise reduced, apply at full size by bilateral grid); bound from the same libwct_hip.so
SYMBOLS_BGRID = ["wct_bgrid_shape", "wct_bgrid_fit", "wct_bgrid_slice", "wct_stylize_proxy"]
BGRID_MAX_XY, BGRID_MAX_Z, BGRID_MAX_SMOOTH = 256, 32, 4            # WCT_BGRID_MAX_*
BGRID_FIT_ROWS, BGRID_TILE_W, BGRID_TILE_H, BGRID_LDS_VERTICES = 64, 128, 8, 320   # WCT_BGRID_FIT_ROWS, WCT_BGRID_TILE_*, WCT_BGRID_LDS_VERTICES
BGRID_CELL, BGRID_BINS, BGRID_EPS, BGRID_SMOOTH = 16, 8, 1e-2, 1    # WCT_BGRID_*: the command line's defaults

# every symbol include/wct_hip_jpeg.h declares (the device JPEG encoder behind --device_jpeg); bound from the same libwct_hip.so
SYMBOLS_JPEG = ["wct_jpeg_header", "wct_jpeg_bound", "wct_jpeg_blocks", "wct_jpeg_pack", "wct_jpeg_encode"]
JPEG_HEADER_BYTES, JPEG_MAX_DIM, JPEG_BLOCK_MAX_BITS = 623, 65500, 1728   # WCT_JPEG_HEADER_BYTES, WCT_JPEG_MAX_DIM, WCT_JPEG_BLOCK_MAX_BITS
JPEG_SEG_MCUS, JPEG_SCAN_TILE, JPEG_SCAN_CHUNK, JPEG_PACK_SPAN, JPEG_STUFF_CHUNK = 8, 256, 256, 64, 1024   # WCT_JPEG_*: the launchers' units
JPEG_OVERFLOW = 0xFFFFFFFFFFFFFFFF                                  # WCT_JPEG_OVERFLOW
JPEG_QUALITY = 75                                                   # Pillow's default, and the command line's

# every symbol include/wct_hip_jdec.h declares (the device JPEG decoder behind --device_decode); bound from the same libwct_hip.so
SYMBOLS_JDEC = ["wct_jdec_parse", "wct_jdec_num_blocks", "wct_jdec_coefficients", "wct_jdec_pixels", "wct_jdec_decode"]
JDEC_UNSUPPORTED = 1                                                # WCT_JDEC_UNSUPPORTED
JDEC_STATUS_OK, JDEC_STATUS_UNSYNC, JDEC_STATUS_CORRUPT = 0, 1, 2   # WCT_JDEC_STATUS_*
JDEC_SUBSEQ_BITS, JDEC_SYNC_THREADS, JDEC_LAUNCHES, JDEC_ROUNDS, JDEC_MAX_ROUNDS = 1024, 256, 4, 32, 4096   # WCT_JDEC_*: the schedule
JDEC_CHUNK, JDEC_SCAN_CHUNK, JDEC_DC_TILE, JDEC_MAX_DIM, JDEC_MAX_SCAN_BYTES = 1024, 256, 256, 65500, 0x0FFFFFFF   # the launchers' units and the limits


class WctJdecInfo(ctypes.Structure):
    """include/wct_hip_jdec.h wct_jdec_info."""
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("hs", ctypes.c_int32 * 3), ("vs", ctypes.c_int32 * 3), ("tq", ctypes.c_int32 * 3), ("td", ctypes.c_int32 * 3),
                ("ta", ctypes.c_int32 * 3), ("reserved", ctypes.c_int32), ("scan_offset", ctypes.c_uint64), ("scan_length", ctypes.c_uint64),
                ("qt", (ctypes.c_uint8 * 64) * 4), ("dc_counts", (ctypes.c_uint8 * 16) * 2), ("dc_vals", (ctypes.c_uint8 * 16) * 2),
                ("ac_counts", (ctypes.c_uint8 * 16) * 2), ("ac_vals", (ctypes.c_uint8 * 256) * 2)]


class WctLayer(ctypes.Structure):
    _fields_ = [("cin", c_int), ("cout", c_int), ("pool_after", c_int), ("up_after", c_int),
                ("weight", POINTER(c_float)), ("bias", POINTER(c_float))]


class WctProfEntry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("ms", c_double), ("flops", c_double), ("bytes", c_double),
                ("launches", c_long)]


class WctP2P(ctypes.Structure):
    _fields_ = [("peer", c_int), ("is_send", c_int), ("buf", c_void_p), ("bytes", c_size_t)]


class WctClipParams(ctypes.Structure):
    """include/wct_hip_video.h wct_clip_params."""
    _fields_ = [("rate", c_double), ("cut", c_double), ("blend", c_float), ("sigma", c_float), ("radius", c_int)]


class WctMotionParams(ctypes.Structure):
    """include/wct_hip_motion.h wct_motion_params."""
    _fields_ = [("levels", c_int), ("range", c_int), ("penalty", c_int)]


ALL_REDUCE_FN =ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_size_t, c_void_p)          # (user, buf, count, stream)
BROADCAST_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p)    # (user, buf, bytes, root, stream)
SENDRECV_FN = ctypes.CFUNCTYPE(c_int, c_void_p, POINTER(WctP2P), c_int, c_void_p)        # (user, ops, n_ops, stream)


class WctCollectives(ctypes.Structure):
    """include/wct_hip.h wct_collectives: the transport table of wct_stylize_sharded (wct_comm_attach_collectives)."""
    _fields_ = [("user", c_void_p), ("all_reduce_sum_f64", ALL_REDUCE_FN), ("broadcast", BROADCAST_FN), ("sendrecv", SENDRECV_FN)]


HALO_MODES = {"auto": 0, "recompute": 1, "exchange": 2}
STYLE_MODES = {"auto": 0, "owner": 1, "strips": 2, "replicate": 3}
SHARD_BROADCAST_MAP = 1
SHARD_FAST_FOLD = 2
RESIZE_FILTERS = {"bilinear": 0, "bicubic": 1}      # WCT_FILTER_*


class WctError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libwct_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load() -> ctypes.CDLL:
    """dlopen the in-tree library.  Raises ImportError when it has not been built
    (`python -c 'import __graft_entry__ as g; g.build()'` or collaborative-distillation_amd/build.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libwct_hip.so not found at %s -- build it with collaborative-distillation_amd/build.sh; "
                          "there is no CPU fallback" % LIB_PATH)
    # torch first: it brings its own HIP runtime, and both must resolve to ONE libamdhip64 in the process -- with this
    # library loaded before torch, wct_create later fails with a HIP error (seen when build() and smoke() share a process)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    fp, dp, ip = POINTER(c_float), POINTER(c_double), POINTER(c_int)
    vp = c_void_p  # device pointers travel as integers
    lib.wct_version.restype = c_int
    lib.wct_create.argtypes = [c_int, POINTER(c_void_p)]
    lib.wct_destroy.argtypes = [c_void_p]
    lib.wct_destroy.restype = None
    lib.wct_last_error.argtypes = [c_void_p]
    lib.wct_last_error.restype = c_char_p
    lib.wct_set_stream.argtypes = [c_void_p, c_void_p]
    lib.wct_sync.argtypes = [c_void_p]
    lib.wct_saturation_count.argtypes = [c_void_p, c_int, POINTER(ctypes.c_ulonglong)]
    lib.wct_range_poll.argtypes = [c_void_p, POINTER(ctypes.c_ulonglong)]
    lib.wct_range_flag_f64.argtypes = [c_void_p, vp]
    lib.wct_debug_get.argtypes = [c_void_p, c_char_p, POINTER(ctypes.c_double)]
    lib.wct_debug_set.argtypes = [c_void_p, c_char_p, c_double]
    lib.wct_load_module.argtypes = [c_void_p, c_int, c_int, c_int, POINTER(WctLayer), fp, fp]
    lib.wct_feature_shape.argtypes = [c_void_p, c_int, c_int, c_int, ip, ip, ip]
    lib.wct_encode.argtypes = [c_void_p, c_int, vp, c_int, c_int, vp, c_int]
    lib.wct_decode.argtypes = [c_void_p, c_int, vp, c_int, c_int, c_int, vp]
    lib.wct_moments.argtypes = [c_void_p, vp, c_int, c_int, c_int, c_int, c_int, vp, vp]
    lib.wct_solve.argtypes = [c_void_p, c_int, c_double, vp, vp, c_double, vp, vp, c_double, vp, vp, ip]
    lib.wct_apply.argtypes = [c_void_p, vp, c_int, c_int, c_int, c_int, vp, vp, vp]
    lib.wct_transform.argtypes = [c_void_p, vp, c_int, c_int, c_int, vp, c_int, c_int, c_float, c_int, vp]
    lib.wct_decode_affine.argtypes = [c_void_p, c_int, vp, c_int, c_int, vp, vp, vp]
    lib.wct_style_transfer_level.argtypes = [c_void_p, c_int, vp, c_int, c_int, vp, c_int, c_int, c_float, vp, ip, ip]
    lib.wct_stylize.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_float, c_int, vp, ip, ip]
    lib.wct_style_prepare.argtypes = [c_void_p, vp, c_int, c_int]
    lib.wct_content_encode.argtypes = [c_void_p, c_int, vp, c_int, c_int, c_int, c_int, vp, vp, ip, ip]
    lib.wct_content_solve.argtypes = [c_void_p, c_int, c_double, vp, vp, c_float, vp, vp]
    lib.wct_content_decode.argtypes = [c_void_p, c_int, vp, vp, vp, ip, ip]
    lib.wct_comm_load.argtypes = [c_char_p]
    lib.wct_comm_library.restype = c_char_p
    lib.wct_comm_attach_collectives.argtypes = [c_void_p, POINTER(WctCollectives), c_int, c_int]
    lib.wct_comm_info.argtypes = [c_void_p, ip, ip]
    lib.wct_comm_selftest.argtypes = [c_void_p]
    lib.wct_shard_geometry.argtypes = [c_int, c_int, c_int, c_int, ip, ip, ip, ip, ip]
    lib.wct_stylize_sharded.argtypes = [c_void_p, vp, c_int, c_int, c_int, c_int, vp, c_int, c_int, c_float, c_int, c_int, c_int, vp, ip, ip, vp]
    lib.wct_style_moments.argtypes = [c_void_p, c_int, vp, c_int, c_int, c_int, c_int, vp, vp]
    lib.wct_style_solve.argtypes = [c_void_p, c_int, c_double, vp, vp]
    lib.wct_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.wct_comm_init.argtypes = [c_void_p, c_int, c_int, ctypes.c_char_p]
    lib.wct_comm_attach.argtypes = [c_void_p, c_void_p, c_int, c_int]
    lib.wct_comm_destroy.argtypes = [c_void_p]
    lib.wct_level_sharded.argtypes = [c_void_p, c_int, vp, c_int, c_int, c_int, c_int, c_double, c_float, vp, ip, ip, vp]
    lib.wct_style_prepare_levels.argtypes = [c_void_p, vp, c_int, c_int, ctypes.c_uint]
    lib.wct_style_stats_count.argtypes = [c_void_p, c_int, POINTER(c_size_t)]
    lib.wct_style_export.argtypes = [c_void_p, c_int, vp]
    lib.wct_style_import.argtypes = [c_void_p, c_int, vp]
    lib.wct_stylize_prepared.argtypes = [c_void_p, vp, c_int, c_int, c_float, c_int, vp, ip, ip]
    lib.wct_moments_labeled.argtypes = [c_void_p, vp, c_int, c_int, c_int, vp, c_int, vp, vp, vp]
    lib.wct_apply_labeled.argtypes = [c_void_p, vp, c_int, c_int, c_int, c_int, vp, c_int, vp, vp, vp]
    lib.wct_stylize_regions.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, POINTER(c_void_p), ip, ip, fp, c_int, vp, ip, ip]
    lib.wct_stylize_interp.argtypes = [c_void_p, vp, c_int, c_int, c_int, POINTER(c_void_p), ip, ip, fp, c_float, c_int, vp, ip, ip]
    lib.wct_style_blend.argtypes = [c_void_p, c_int, c_int, vp, fp]
    lib.wct_stylize_blend.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, POINTER(c_void_p), ip, ip, fp, c_int, vp, ip, ip]
    lib.wct_moments_weighted.argtypes = [c_void_p, vp, c_int, c_int, c_int, vp, c_int, vp, vp]
    lib.wct_apply_mixed.argtypes = [c_void_p, vp, c_int, c_int, c_int, c_int, vp, c_int, vp, vp, vp]
    lib.wct_u8_to_planar.argtypes = [c_void_p, vp, c_int, c_int, vp]
    lib.wct_planar_to_u8.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int]
    lib.wct_stylize_u8.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_float, c_int, vp, ip, ip, c_int]
    lib.wct_resize_shape.argtypes = [c_int, c_int, c_int, ip, ip]
    lib.wct_resize_u8.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int]
    lib.wct_resize_u8_to_planar.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int]
    lib.wct_resize_u8_filter.argtypes = [c_void_p, vp, c_int, c_int, vp, vp, c_int, c_int, c_int]
    lib.wct_noise_uniform.argtypes = [c_void_p, ctypes.c_uint64, ctypes.c_uint32, c_int, c_int, vp]
    lib.wct_synthesize.argtypes = [c_void_p, vp, c_int, c_int, c_int, c_int, ctypes.c_uint64, ctypes.c_uint32, c_float, c_int, vp, ip, ip]
    lib.wct_color_moments.argtypes = [c_void_p, vp, c_int, c_int, vp, vp]
    lib.wct_color_solve.argtypes = [c_void_p, c_double, vp, vp, c_double, vp, vp, c_double, vp, vp]
    lib.wct_color_apply.argtypes = [c_void_p, vp, c_int, c_int, vp, vp, vp]
    lib.wct_color_match.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, vp]
    lib.wct_luma_merge.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, vp, vp, c_int]
    lib.wct_stylize_color.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_float, c_int, c_int, vp, ip, ip]
    lib.wct_guided_filter.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_int, c_double, vp, vp, c_int]
    lib.wct_stylize_smooth.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_float, c_int, c_int, c_int, c_double, vp, ip, ip]
    lib.wct_patch_match.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_int, vp, vp]
    lib.wct_patch_assemble.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_int, vp, c_float, vp]
    lib.wct_swap_level.argtypes = [c_void_p, c_int, vp, c_int, c_int, vp, c_int, c_int, c_int, c_float, vp, ip, ip]
    lib.wct_stylize_swap.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_int, c_int, c_float, c_int, vp, ip, ip]
    lib.wct_attn_project.argtypes = [c_void_p, vp, c_int, c_int, c_int, c_int, vp, vp]
    lib.wct_attn_stats.argtypes = [c_void_p, vp, c_int, vp, vp, c_int, c_int, c_float, vp, vp]
    lib.wct_attn_apply.argtypes = [c_void_p, vp, vp, vp, vp, c_int, c_int, vp, vp, c_float, vp]
    lib.wct_attn_level.argtypes = [c_void_p, c_int, vp, c_int, c_int, vp, c_int, c_int, c_int, c_float, c_float, vp, ip, ip]
    lib.wct_stylize_attn.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_int, c_int, c_float, c_float, c_int, vp, ip, ip]
    lib.wct_scale_shape.argtypes = [c_int, c_int, c_int, ip, ip]
    lib.wct_resample_planar.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_int]
    lib.wct_pyramid_merge.argtypes = [c_void_p, vp, vp, c_int, c_int, vp, c_int, c_int, c_float, vp]
    lib.wct_stylize_scaled.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_float, c_int, ip, c_float, vp, ip, ip]
    lib.wct_stylize_guided.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, POINTER(c_void_p), ip, ip, POINTER(c_void_p), ip, fp, c_int, vp, ip, ip]
    lib.wct_kmeans_assign.argtypes = [c_void_p, vp, c_int, c_int, c_int, vp, vp, vp, c_int, vp, vp, vp, vp, vp]
    lib.wct_kmeans_seed.argtypes = [c_void_p, vp, c_int, c_int, c_int, vp, vp, c_int, vp, vp]
    lib.wct_feature_regions.argtypes = [c_void_p, c_int, vp, c_int, c_int, vp, c_int, c_int, c_int, c_int, vp, vp, vp]
    lib.wct_clip_bytes.argtypes = [c_int, c_int, ip, POINTER(c_size_t)]
    lib.wct_clip_create.argtypes = [c_void_p, c_int, c_int, POINTER(WctClipParams), POINTER(c_void_p)]
    lib.wct_clip_destroy.argtypes = [c_void_p, c_void_p]
    lib.wct_clip_destroy.restype = None
    lib.wct_clip_reset.argtypes = [c_void_p, c_void_p]
    lib.wct_clip_export.argtypes = [c_void_p, c_void_p, c_int, vp, vp, vp]
    lib.wct_moments_track.argtypes = [c_void_p, c_void_p, c_int, c_int, vp, vp]
    lib.wct_temporal_blend.argtypes = [c_void_p, vp, c_int, c_int, vp, vp, vp, c_int, c_int, c_float, c_float, c_int, vp, vp, vp, c_int]
    lib.wct_stylize_clip.argtypes = [c_void_p, c_void_p, vp, c_int, c_int, c_float, vp, vp, c_int, ip, ip]
    lib.wct_motion_shape.argtypes = [c_int, c_int, ip, ip]
    lib.wct_motion_luma.argtypes = [c_void_p, vp, c_int, c_int, c_int, c_int, c_int, vp]
    lib.wct_motion_estimate.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, POINTER(WctMotionParams), vp]
    lib.wct_motion_blend.argtypes = [c_void_p, vp, c_int, c_int, vp, vp, vp, c_int, c_int, c_float, c_float, c_int, vp, vp, vp, c_int, vp]
    lib.wct_motion_attach.argtypes = [c_void_p, c_void_p, POINTER(WctMotionParams)]
    lib.wct_motion_export.argtypes = [c_void_p, c_void_p, vp]
    lib.wct_rotation_make.argtypes = [c_void_p, c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint, c_double, vp, vp]
    lib.wct_style_diversify.argtypes = [c_void_p, ctypes.c_uint, c_double, ctypes.c_uint64, ctypes.c_uint32]
    lib.wct_stylize_diverse.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, ctypes.c_uint, c_double, ctypes.c_uint64, ctypes.c_uint32, c_float, c_int,
                                        vp, ip, ip]
    lib.wct_bgrid_shape.argtypes = [c_int, c_int, c_int, ip, ip]
    lib.wct_bgrid_fit.argtypes = [c_void_p, vp, vp, c_int, c_int, c_int, c_int, c_int, c_double, c_int, vp]
    lib.wct_bgrid_slice.argtypes = [c_void_p, vp, c_int, c_int, c_int, vp, c_int, c_int, vp, vp, c_int]
    lib.wct_stylize_proxy.argtypes = [c_void_p, vp, c_int, c_int, vp, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_double, c_int, vp, vp, c_int]
    u8p, u16p, u64p = POINTER(ctypes.c_uint8), POINTER(ctypes.c_uint16), POINTER(ctypes.c_uint64)
    lib.wct_jpeg_header.argtypes = [c_int, c_int, c_int, u8p, u16p, u16p]
    lib.wct_jpeg_bound.argtypes = [c_int, c_int, u64p]
    lib.wct_jpeg_blocks.argtypes = [c_void_p, vp, c_int, c_int, c_int, vp]
    lib.wct_jpeg_pack.argtypes = [c_void_p, vp, c_int, c_int, vp, ctypes.c_uint64, vp]
    lib.wct_jpeg_encode.argtypes = [c_void_p, vp, c_int, c_int, c_int, vp, ctypes.c_uint64, vp]
    jip = POINTER(WctJdecInfo)
    lib.wct_jdec_parse.argtypes = [c_void_p, c_size_t, jip]
    lib.wct_jdec_num_blocks.argtypes = [jip, u64p]
    lib.wct_jdec_coefficients.argtypes = [c_void_p, vp, jip, c_int, vp, vp]
    lib.wct_jdec_pixels.argtypes = [c_void_p, vp, jip, vp]
    lib.wct_jdec_decode.argtypes = [c_void_p, vp, jip, c_int, vp, vp]
    lib.wct_set_transform.argtypes = [c_void_p, c_int]
    lib.wct_get_transform.argtypes = [c_void_p, ip]
    lib.wct_transform_solve.argtypes = [c_void_p, c_int, c_int, c_double, vp, vp, vp, c_double, vp, vp, ip]
    lib.wct_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int, c_int]
    lib.wct_workspace_bytes.restype = c_size_t
    lib.wct_reserve.argtypes = [c_void_p, c_int, c_int, c_int, c_int]
    lib.wct_set_conv_mode.argtypes = [c_void_p, c_int]
    lib.wct_set_numpy_variant.argtypes = [c_void_p, c_int]
    lib.wct_set_overlap.argtypes = [c_void_p, c_int]
    lib.wct_profile_enable.argtypes = [c_void_p, c_int]
    lib.wct_profile_reset.argtypes = [c_void_p]
    lib.wct_profile_read.argtypes = [c_void_p, POINTER(WctProfEntry), c_int, ip]
    _lib = lib
    return lib


def check(lib, ctx, rc):
    if rc != WCT_OK:
        msg = lib.wct_last_error(ctx).decode("utf-8", "replace") if ctx else "no context"
        if rc == WCT_ERR_INVALID:
            raise ValueError("libwct_hip: " + msg)
        if rc == WCT_ERR_RANGE:
            raise OverflowError("libwct_hip: " + msg)
        raise WctError(rc, msg)
