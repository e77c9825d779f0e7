"""ctypes binding of libftk_hip.so (C ABI in include/ftk.h).

The library is built in-tree by ``feature_tracker_amd/csrc/Makefile`` (hipcc, gfx950).  Loading
fails loudly when it is missing: there is no Python / CPU fallback for any compute entry point.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(_PKG_DIR, "csrc")
LIB_PATH = os.path.join(CSRC_DIR, "libftk_hip.so")

FTK_OK = 0
FTK_MAX_LEVELS = 12
FTK_CORR_MAX_LEVELS = 16
FTK_CORR_MAX_RADIUS = 64
FTK_FLOW_UPSAMPLE_TILE = 32
FTK_FLOW_POINTS_TILE = 64
FTK_FLOW_WARM_TILE = 256
FTK_FLOW_WARM_MAX_PIXELS = 1 << 20
FTK_FLOW_WARM_MAX_SPLITS = 32
# masked Harris detection and the track table (include/ftk.h)
FTK_HARRIS_DEVICE_MAX_SURVIVORS = 65536
FTK_HARRIS_RANK_TILE = 256
FTK_TRACK_TABLE_MAX_SLOTS = 65536
FTK_TRACK_TABLE_BLOCK = 1024
# two-view outlier rejection (include/ftk.h)
FTK_EPIPOLAR_MAX_HYPOTHESES = 4096
FTK_EPIPOLAR_SAMPLE = 8
FTK_EPIPOLAR_MAX_ATTEMPTS = 16
FTK_EPIPOLAR_SCORE_TILE = 256
# the same with a choice of model (include/ftk.h)
FTK_TWO_VIEW_FUNDAMENTAL = 0
FTK_TWO_VIEW_HOMOGRAPHY = 1
FTK_TWO_VIEW_AUTO = 2
FTK_TWO_VIEW_HOMOGRAPHY_SAMPLE = 4
TWO_VIEW_MODES = {"fundamental": 0, "homography": 1, "auto": 2}
# relative pose and landmarks from two-view inliers (include/ftk.h)
FTK_POSE_JACOBI_SWEEPS = 7
FTK_POSE_TILE = 256
# PnpRansac (include/ftk.h)
FTK_PNP_SAMPLE = 6
FTK_PNP_MODEL_FLOATS = 12
FTK_PNP_MAX_REFINE_ITERATIONS = 16
FTK_PNP_SAMPLE_DLT6 = 0
FTK_PNP_SAMPLE_P3P = 1
FTK_PNP_P3P_SAMPLE = 4
# the keypoint decoder (include/ftk.h)
FTK_KEYPOINT_DECODE_CELL = 8
FTK_KEYPOINT_DECODE_MAX_KEYPOINTS = 65536
FTK_KEYPOINT_DECODE_MAX_CHANNELS = 1024
# the assignment head (include/ftk.h)
FTK_MATCH_ASSIGNMENT_MAX_ROWS = 4096
FTK_MATCH_ASSIGNMENT_MAX_DIM = 1024
# the transformer layer (include/ftk.h)
FTK_TRANSFORMER_MAX_ROWS = 4096
FTK_TRANSFORMER_MAX_DIM = 1024
FTK_TRANSFORMER_MAX_HEAD_DIM = 128
# the adaptive pass (include/ftk.h)
FTK_LIGHTGLUE_MAX_LAYERS = 64
FTK_LIGHTGLUE_STATE_WORDS = 4  # live0, live1, stopped, stop_layer
# the landmark table (include/ftk.h)
FTK_MATCH_TABLE_MAX_SLOTS = 4096
FTK_MATCH_TABLE_MAX_DIM = 1024
# TrackOdometry's landmark table (include/ftk.h): the counters' indices and the end entry's modes
FTK_LANDMARK_TABLE_BLOCK = 256
FTK_LANDMARK_TABLE_COUNTERS = 8
FTK_LANDMARK_TABLE_VALID, FTK_LANDMARK_TABLE_N_NEW, FTK_LANDMARK_TABLE_N_ANCHORED = 0, 1, 2
FTK_LANDMARK_TABLE_N_LANDMARKS, FTK_LANDMARK_TABLE_N_DROPPED, FTK_LANDMARK_TABLE_LOST = 3, 4, 5
FTK_LANDMARK_TABLE_STEADY, FTK_LANDMARK_TABLE_BOOTSTRAP = 0, 1
# SepConvGru (include/ftk.h): the supported sizes and the packed weight layout
FTK_SEP_CONV_GRU_MAX_PARTS = 3
FTK_SEP_CONV_GRU_MAX_H_CHANNELS = 1024
FTK_SEP_CONV_GRU_MAX_IN_CHANNELS = 4096
FTK_SEP_CONV_GRU_CHUNK = 16
FTK_SEP_CONV_GRU_KERNEL_SIZES = (3, 5)
# conv2d (UpdateBlock's stock layers; include/ftk.h): the supported sizes and, per kernel size, the chunk of input channels
FTK_CONV2D_MAX_PARTS = 3
FTK_CONV2D_MAX_OUT_CHANNELS = 1024
FTK_CONV2D_MAX_IN_CHANNELS = 4096
FTK_CONV2D_CHUNK = {1: 32, 3: 8, 7: 2}  # FTK_CONV2D_CHUNK_1 / _3 / _7
FTK_CONV2D_KERNEL_SIZES = (1, 3, 7)
FTK_CONV2D_STRIDES = {1: (1, 3, 7), 2: (1, 3)}  # ftk_conv2d_strided_device: the kernel sizes of each stride
FTK_CONV2D_POOL_KERNEL_SIZES = (1, 3)  # ftk_conv2d_pool_device
ERROR_NAMES = {0: "FTK_OK", -1: "FTK_E_INVALID_ARGUMENT", -2: "FTK_E_NO_DEVICE", -3: "FTK_E_HIP", -4: "FTK_E_UNSUPPORTED",
               -5: "FTK_E_OUT_OF_MEMORY"}

MODELS = {"basic": 0, "affine": 1, "lssd": 2}
METHODS = {"inverse": 0, "direct": 1, "fast": 2, "sse": 3, "neon": 4}

# every symbol include/ftk.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "ftk_abi_version", "ftk_build_info", "ftk_device_count", "ftk_context_create", "ftk_context_destroy", "ftk_last_error", "ftk_synchronize", "ftk_warmup", "ftk_set_reduction_mode", "ftk_context_refresh_env", "ftk_pyramid_update",
    "ftk_default_klt_options", "ftk_pyramid_upload", "ftk_pyramid_wrap_device", "ftk_pyramid_build", "ftk_pyramid_levels",
    "ftk_pyramid_level", "ftk_pyramid_download_level", "ftk_pyramid_destroy", "ftk_klt_track", "ftk_klt_track_device",
    "ftk_extract_extend_patch", "ftk_hamming_match", "ftk_hamming_match_device", "ftk_cosine_match", "ftk_cosine_match_device", "ftk_ldlt6_solve", "ftk_default_direct_options", "ftk_direct_track", "ftk_direct_track_batch_device", "ftk_fill_matched_pixels",
    "ftk_brief_compute", "ftk_brief_compute_device", "ftk_harris_detect", "ftk_harris_response",
    "ftk_shard_bounds", "ftk_klt_shard_bytes", "ftk_comm_unique_id", "ftk_comm_create", "ftk_comm_destroy", "ftk_comm_rank", "ftk_comm_world",
    "ftk_klt_track_sharded_device", "ftk_klt_track_sharded", "ftk_klt_track_shard_device", "ftk_klt_unpack_shards_device", "ftk_hamming_match_sharded_device",
    "ftk_default_dense_flow_options", "ftk_dense_flow_gaussian", "ftk_dense_flow", "ftk_dense_flow_device", "ftk_dense_flow_level",
    "ftk_corr_pyramid_layout", "ftk_corr_pyramid_build_device", "ftk_corr_pyramid_lookup_device", "ftk_flow_upsample_device", "ftk_flow_track_points_device", "ftk_flow_warm_splits", "ftk_flow_warm_device",
    "ftk_corr_ondemand_layout", "ftk_corr_ondemand_prepare_device", "ftk_corr_ondemand_lookup_device",
    "ftk_sep_conv_gru_packed_elements", "ftk_sep_conv_gru_gates_device", "ftk_sep_conv_gru_blend_device",
    "ftk_conv2d_packed_elements", "ftk_conv2d_device", "ftk_conv2d_strided_device", "ftk_conv2d_pool_device", "ftk_channel_normalise_device",
    "ftk_nn_match_scores_device", "ftk_nn_match_scores", "ftk_nn_match_list_device", "ftk_nn_match_list", "ftk_nn_fill_pixels_device",
    "ftk_harris_detect_device", "ftk_track_table_retire_device", "ftk_track_table_fill_device",
    "ftk_epipolar_workspace_bytes", "ftk_epipolar_ransac_device",
    "ftk_two_view_workspace_bytes", "ftk_two_view_ransac_device",
    "ftk_two_view_pose_workspace_bytes", "ftk_two_view_pose_device",
    "ftk_pnp_ransac_workspace_bytes", "ftk_pnp_ransac_device", "ftk_pnp_ransac_sampled_device",
    "ftk_landmark_table_begin_device", "ftk_landmark_table_end_device",
    "ftk_keypoint_decode_workspace_bytes", "ftk_keypoint_decode_device",
    "ftk_match_assignment_workspace_bytes", "ftk_match_assignment_device",
    "ftk_transformer_layer_workspace_bytes", "ftk_attention_device", "ftk_linear_device", "ftk_transformer_layer_device",
    "ftk_lightglue_adaptive_workspace_bytes", "ftk_transformer_layer_adaptive_device", "ftk_lightglue_confidence_device",
    "ftk_lightglue_adapt_step_device", "ftk_lightglue_finish_device",
    "ftk_match_table_workspace_bytes", "ftk_match_table_query_device", "ftk_match_table_update_device",
]
UNIQUE_ID_BYTES = 128


class FtkError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32)]


class KltOptions(C.Structure):
    """OpticalFlowOptions (optical_flow.h:20-28)."""
    _fields_ = [
        ("max_track_points", C.c_uint32), ("max_iteration", C.c_uint32), ("max_tolerance_large_step", C.c_uint32),
        ("half_rows", C.c_int32), ("half_cols", C.c_int32), ("max_converge_step", C.c_float), ("method", C.c_int32),
    ]


class DirectOptions(C.Structure):
    """DirectMethodOptions (direct_method_tracker.h:20-28)."""
    _fields_ = [
        ("max_track_points", C.c_uint32), ("max_iteration", C.c_uint32), ("half_rows", C.c_int32), ("half_cols", C.c_int32),
        ("max_converge_step", C.c_float), ("max_converge_residual", C.c_float), ("method", C.c_int32),
    ]


class DenseFlowOptions(C.Structure):
    """DenseOpticalFlow::Options (dense_optical_flow.h:15-20) + the object's {k2, k4, k22} for half patch 0."""
    _fields_ = [
        ("max_iteration", C.c_int32), ("half_patch", C.c_int32), ("max_converge_step", C.c_float), ("max_delta_flow_step", C.c_float),
        ("k_moments", C.c_float * 3),
    ]


class DirectProblem(C.Structure):
    """ftk_direct_problem: one pose problem of a batched launch (device pointers)."""
    _fields_ = [
        ("ref", C.c_void_p), ("cur", C.c_void_p), ("K", C.c_float * 4), ("d_p_c_in_ref", C.c_void_p), ("d_ref_uv", C.c_void_p),
        ("d_cur_uv", C.c_void_p), ("n", C.c_int32), ("d_pose", C.c_void_p), ("d_status", C.c_void_p), ("status_valid", C.c_int32),
        ("d_iterations", C.c_void_p),
    ]


class GruPart(C.Structure):
    """ftk_gru_part: one tensor of SepConvGru's ``x`` (a device pointer and its channel count)."""
    _fields_ = [("data", C.c_void_p), ("channels", C.c_int32)]


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile libftk_hip.so for gfx950 with the committed Makefile (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC_DIR, f) for f in os.listdir(CSRC_DIR) if f.endswith((".cpp", ".hip", ".h"))]
    srcs.append(os.path.join(os.path.dirname(_PKG_DIR), "include", "ftk.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        cmd = ["make", "-C", CSRC_DIR, "-j4"] + (["-B"] if force else []) + ["libftk_hip.so"]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("building libftk_hip.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
        if verbose:
            print(res.stdout)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """The loaded library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own HIP / HSA runtime.  Two runtimes in one process do not share
    # the device, so when torch is installed it must be loaded FIRST: libftk_hip.so then binds to
    # the same libamdhip64.so.7 (same SONAME) and device pointers / streams are interchangeable.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = os.environ.get("FTK_LIB_PATH", LIB_PATH)  # e.g. a library built with other compiler flags
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP extension must be built first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C feature_tracker_amd/csrc). "
            "feature_tracker_amd has no CPU fallback.")
    l = C.CDLL(path)
    vp, i32, u32p = C.c_void_p, C.c_int32, C.POINTER(C.c_uint32)
    l.ftk_abi_version.restype = C.c_int
    l.ftk_build_info.restype = C.c_char_p
    l.ftk_device_count.restype = C.c_int
    l.ftk_context_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    l.ftk_context_destroy.argtypes = [vp]
    l.ftk_context_destroy.restype = None
    l.ftk_last_error.argtypes = [vp]
    l.ftk_last_error.restype = C.c_char_p
    l.ftk_synchronize.argtypes = [vp]
    l.ftk_warmup.argtypes = [vp, C.c_uint]
    l.ftk_set_reduction_mode.argtypes = [vp, C.c_int]
    l.ftk_context_refresh_env.argtypes = [vp]
    l.ftk_pyramid_update.argtypes = [vp, vp, vp, C.c_int]
    l.ftk_default_klt_options.argtypes = [C.POINTER(KltOptions)]
    l.ftk_default_klt_options.restype = None
    l.ftk_pyramid_upload.argtypes = [vp, C.POINTER(Image), i32, C.POINTER(vp)]
    l.ftk_pyramid_wrap_device.argtypes = [vp, C.POINTER(Image), i32, C.POINTER(vp)]
    l.ftk_pyramid_build.argtypes = [vp, vp, i32, i32, i32, C.c_int, C.POINTER(vp)]
    l.ftk_pyramid_levels.argtypes = [vp]
    l.ftk_pyramid_level.argtypes = [vp, i32, C.POINTER(Image)]
    l.ftk_pyramid_download_level.argtypes = [vp, vp, i32, vp]
    l.ftk_pyramid_destroy.argtypes = [vp]
    l.ftk_pyramid_destroy.restype = None
    l.ftk_klt_track.argtypes = [vp, C.c_int, C.POINTER(KltOptions), vp, vp, vp, vp, vp, i32, vp, C.c_int, C.c_int, vp]
    l.ftk_klt_track_device.argtypes = [vp, C.c_int, C.POINTER(KltOptions), vp, vp, vp, vp, vp, vp, vp, i32, vp, C.c_int, C.c_int, vp]
    l.ftk_extract_extend_patch.argtypes = [vp, vp, i32, C.c_float, C.c_float, i32, i32, vp, vp, u32p]
    l.ftk_hamming_match.argtypes = [vp, vp, i32, vp, i32, i32, i32, C.c_float, vp, vp, i32, i32, vp, C.POINTER(C.c_int)]
    l.ftk_hamming_match_device.argtypes = [vp, vp, i32, vp, i32, i32, i32, C.c_float, vp, vp, i32, i32, vp, vp]
    l.ftk_cosine_match.argtypes = [vp, vp, i32, vp, i32, i32, C.c_float, vp, vp, i32, i32, vp, C.POINTER(C.c_int)]
    l.ftk_cosine_match_device.argtypes = [vp, vp, i32, vp, i32, i32, C.c_float, vp, vp, i32, i32, vp]
    l.ftk_ldlt6_solve.argtypes = [vp, vp, vp, vp, i32]
    l.ftk_default_direct_options.argtypes = [C.POINTER(DirectOptions)]
    l.ftk_default_direct_options.restype = None
    l.ftk_direct_track.argtypes = [vp, C.POINTER(DirectOptions), vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, C.c_int, u32p]
    l.ftk_direct_track_batch_device.argtypes = [vp, C.POINTER(DirectOptions), C.POINTER(DirectProblem), i32]
    l.ftk_fill_matched_pixels.argtypes = [vp, i32, vp, i32, vp, vp]
    l.ftk_brief_compute.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp]
    l.ftk_brief_compute_device.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp]
    l.ftk_harris_detect.argtypes = [vp, vp, i32, i32, i32, C.c_float, vp, C.POINTER(C.c_int32)]
    l.ftk_harris_response.argtypes = [vp, vp, i32, vp]
    l.ftk_shard_bounds.argtypes = [i32, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    l.ftk_shard_bounds.restype = None
    l.ftk_klt_shard_bytes.argtypes = [i32, i32]
    l.ftk_klt_shard_bytes.restype = C.c_size_t
    l.ftk_comm_unique_id.argtypes = [vp]
    l.ftk_comm_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    l.ftk_comm_destroy.argtypes = [vp]
    l.ftk_comm_destroy.restype = None
    l.ftk_comm_rank.argtypes = [vp]
    l.ftk_comm_world.argtypes = [vp]
    l.ftk_klt_track_sharded_device.argtypes = [vp, vp, C.c_int, C.POINTER(KltOptions), vp, vp, vp, vp, vp, vp, vp, i32, vp, C.c_int, C.c_int, vp]
    l.ftk_klt_track_sharded.argtypes = [vp, vp, C.c_int, C.POINTER(KltOptions), vp, vp, vp, vp, vp, i32, vp, C.c_int, C.c_int, vp]
    l.ftk_klt_track_shard_device.argtypes = [vp, i32, i32, C.c_int, C.POINTER(KltOptions), vp, vp, vp, vp, vp, i32, vp, C.c_int, C.c_int, vp, vp]
    l.ftk_klt_unpack_shards_device.argtypes = [vp, vp, i32, i32, vp, vp]
    l.ftk_hamming_match_sharded_device.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, C.c_float, vp, vp, i32, i32, vp]
    l.ftk_default_dense_flow_options.argtypes = [C.POINTER(DenseFlowOptions)]
    l.ftk_default_dense_flow_options.restype = None
    l.ftk_dense_flow_gaussian.argtypes = [i32, vp, vp]
    l.ftk_dense_flow.argtypes = [vp, C.POINTER(DenseFlowOptions), vp, vp, vp, vp]
    l.ftk_dense_flow_device.argtypes = [vp, C.POINTER(DenseFlowOptions), vp, vp, vp, vp]
    l.ftk_dense_flow_level.argtypes = [vp, C.POINTER(DenseFlowOptions), vp, vp, i32, vp, vp, i32]
    i64p = C.POINTER(C.c_int64)
    l.ftk_corr_pyramid_layout.argtypes = [i32, i32, i32, i32, i64p, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    l.ftk_corr_pyramid_build_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    l.ftk_corr_pyramid_lookup_device.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32]
    l.ftk_corr_ondemand_layout.argtypes = [i32, i32, i32, i32, i32, i64p, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    l.ftk_corr_ondemand_prepare_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    l.ftk_corr_ondemand_lookup_device.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32]
    l.ftk_flow_upsample_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, vp]
    l.ftk_flow_track_points_device.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float, vp, vp, vp, vp]
    l.ftk_flow_warm_splits.argtypes = [i32, i32, i32, C.POINTER(C.c_int32)]
    l.ftk_flow_warm_device.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp]
    i64, f32 = C.c_int64, C.c_float
    parts = C.POINTER(GruPart)
    l.ftk_sep_conv_gru_packed_elements.argtypes = [i32, i32, i32, i64p]
    l.ftk_sep_conv_gru_gates_device.argtypes = [vp, vp, parts, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    l.ftk_sep_conv_gru_blend_device.argtypes = [vp, vp, parts, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    l.ftk_conv2d_packed_elements.argtypes = [i32, i32, i32, i64p]
    l.ftk_conv2d_device.argtypes = [vp, vp, parts, i32, vp, vp, i32, i32, i32, f32, i32, i32, i32, vp]
    l.ftk_conv2d_strided_device.argtypes = [vp, vp, parts, i32, vp, vp, i32, i32, i32, i32, f32, vp, i32, i32, i32, i32, vp]
    l.ftk_conv2d_pool_device.argtypes = [vp, vp, parts, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    l.ftk_channel_normalise_device.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    l.ftk_nn_match_scores_device.argtypes = [vp, vp, vp, i32, i32, i32, i64, i64, f32, vp, vp]
    l.ftk_nn_match_scores.argtypes = [vp, vp, i32, i32, i32, i64, i64, f32, vp, vp, C.POINTER(C.c_int)]
    l.ftk_nn_match_list_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    l.ftk_nn_match_list.argtypes = [vp, vp, i32, i32, i32, vp, vp, C.POINTER(C.c_int)]
    l.ftk_nn_fill_pixels_device.argtypes = [vp, vp, vp, i32, vp, i32, vp]
    l.ftk_harris_detect_device.argtypes = [vp, vp, i32, i32, i32, f32, vp, vp, i32, vp, vp]
    l.ftk_track_table_retire_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp]
    l.ftk_track_table_fill_device.argtypes = [vp, vp, i32, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    l.ftk_epipolar_workspace_bytes.argtypes = [i32, i32, i64p]
    l.ftk_epipolar_ransac_device.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    l.ftk_two_view_workspace_bytes.argtypes = [i32, i32, i32, i64p]
    l.ftk_two_view_ransac_device.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, C.c_uint32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    l.ftk_two_view_pose_workspace_bytes.argtypes = [i32, i64p]
    l.ftk_two_view_pose_device.argtypes = [vp, vp, vp, vp, vp, i32] + [f32] * 10 + [vp] * 7
    l.ftk_pnp_ransac_workspace_bytes.argtypes = [i32, i32, i32, i64p]
    l.ftk_pnp_ransac_device.argtypes = [vp, vp, vp, vp, vp, i32] + [f32] * 5 + [i32, i32, C.c_uint32] + [vp] * 7
    l.ftk_pnp_ransac_sampled_device.argtypes = [vp, vp, vp, vp, vp, i32] + [f32] * 5 + [i32, i32, C.c_uint32, i32] + [vp] * 7
    l.ftk_landmark_table_begin_device.argtypes = [vp, vp, vp, i32] + [vp] * 6
    l.ftk_landmark_table_end_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32] + [f32] * 6 + [vp] * 6
    l.ftk_keypoint_decode_workspace_bytes.argtypes = [i32, i32, i32, i32, i64p]
    l.ftk_keypoint_decode_device.argtypes = [vp, vp, vp, i32, i32, vp, i32, C.c_int64, C.c_int64, C.c_int64, i32, f32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    l.ftk_match_assignment_workspace_bytes.argtypes = [i32, i32, i32, i32, i64p]
    l.ftk_match_assignment_device.argtypes = [vp, vp, vp, i32, vp, i32, i32, vp, vp, f32, vp, vp, vp, vp, C.c_int64]
    l.ftk_transformer_layer_workspace_bytes.argtypes = [i32, i32, i32, i32, i64p]
    l.ftk_attention_device.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, vp, f32, f32, vp]
    l.ftk_linear_device.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, vp]
    l.ftk_transformer_layer_device.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    l.ftk_lightglue_adaptive_workspace_bytes.argtypes = [i32, i32, i32, i32, i64p]
    l.ftk_transformer_layer_adaptive_device.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    l.ftk_lightglue_confidence_device.argtypes = [vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    l.ftk_lightglue_adapt_step_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, f32, f32, f32, i32] + [vp] * 15
    l.ftk_lightglue_finish_device.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp]
    l.ftk_match_table_workspace_bytes.argtypes = [i32, i32, i32, i64p]
    l.ftk_match_table_query_device.argtypes = [vp, vp, i32, i32] + [vp] * 7
    l.ftk_match_table_update_device.argtypes = [vp, vp, i32, i32] + [vp] * 15 + [i32, vp, i32, vp, vp]
    _lib = l
    return l


def loaded():
    """The library if it has been loaded, else None: what a destructor frees a handle through.  A destructor runs whenever the collector
    decides, so it must neither load a library nor talk to whatever stands in for ``lib`` at that moment (a test's recording stand-in)."""
    return _lib


def build_info() -> dict:
    """ftk_build_info() as a dict: source_hash, compiler, arch, mllvm (accepted internal LLVM options), mllvm_rejected."""
    text = lib().ftk_build_info().decode()
    return {k.strip(): v.strip() for k, v in (item.split("=", 1) for item in text.split(";") if "=" in item)}


def check(rc: int, ctx_handle=None) -> None:
    if rc != FTK_OK:
        msg = lib().ftk_last_error(ctx_handle)
        raise FtkError(rc, msg.decode() if msg else "")


def corr_pyramid_layout(B: int, H: int, W: int, levels: int):
    """ftk_corr_pyramid_layout (host only): (elements, [offset_l], [(H_l, W_l)]) of a correlation volume; FtkError when a level would be
    empty or the sizes are out of range."""
    n = max(int(levels), 0)
    elements = C.c_int64()
    off = (C.c_int64 * max(n, 1))()
    lh = (C.c_int32 * max(n, 1))()
    lw = (C.c_int32 * max(n, 1))()
    check(lib().ftk_corr_pyramid_layout(int(B), int(H), int(W), int(levels), C.byref(elements), off, lh, lw), None)
    return elements.value, [off[i] for i in range(n)], [(lh[i], lw[i]) for i in range(n)]


def corr_ondemand_layout(B: int, C_: int, H: int, W: int, levels: int):
    """ftk_corr_ondemand_layout (host only): (elements, [offset_l], [(H_l, W_l)]) of an on-demand correlation workspace, fmap0 transposed at
    element 0 and fmap1's level l channel-last at offset_l; elements = B * C * (H * W + sum_l H_l * W_l).  FtkError as corr_pyramid_layout."""
    n = max(int(levels), 0)
    elements = C.c_int64()
    off = (C.c_int64 * max(n, 1))()
    lh = (C.c_int32 * max(n, 1))()
    lw = (C.c_int32 * max(n, 1))()
    check(lib().ftk_corr_ondemand_layout(int(B), int(C_), int(H), int(W), int(levels), C.byref(elements), off, lh, lw), None)
    return elements.value, [off[i] for i in range(n)], [(lh[i], lw[i]) for i in range(n)]


def flow_warm_splits(B: int, H: int, W: int) -> int:
    """ftk_flow_warm_splits (host only): the number of source ranges ftk_flow_warm_device should scan at these sizes; FtkError for a
    non-positive size or H * W above FTK_FLOW_WARM_MAX_PIXELS."""
    splits = C.c_int32()
    check(lib().ftk_flow_warm_splits(int(B), int(H), int(W), C.byref(splits)), None)
    return splits.value


def _up16(v: int) -> int:
    """v rounded up to a multiple of 16: what a block of v bytes occupies in a caller-owned workspace (csrc/ftk_layout.h's 16-byte slots)."""
    return (v + 15) & ~15


def _ransac_workspace_bytes(n: int, hypotheses: int, slots: int) -> int:
    """csrc/two_view_plan.cpp's workspace: M, then the participants' normalised coordinates, their indices, and per slot counts, models and
    validity flags, each block rounded up to 16 bytes."""
    n, k = int(n), slots * int(hypotheses)
    return 16 + _up16(16 * n) + _up16(4 * n) + _up16(4 * k) + _up16(36 * k) + _up16(k)


def epipolar_workspace_bytes(n: int, hypotheses: int) -> int:
    """Bytes of workspace ftk_epipolar_ransac_device needs, the value ftk_epipolar_workspace_bytes returns (pure Python: argument checks
    need no library): the plan's layout with one slot."""
    return _ransac_workspace_bytes(n, hypotheses, 1)


def two_view_workspace_bytes(n: int, hypotheses: int, mode: int = FTK_TWO_VIEW_AUTO) -> int:
    """Bytes of workspace ftk_two_view_ransac_device needs, the value ftk_two_view_workspace_bytes returns (pure Python): the plan's layout
    with the slots of two models, the same for every mode."""
    return _ransac_workspace_bytes(n, hypotheses, 2)


def two_view_pose_workspace_bytes(n: int) -> int:
    """Bytes of workspace ftk_two_view_pose_device needs, the value ftk_two_view_pose_workspace_bytes returns (pure Python;
    csrc/two_view_pose_plan.cpp): M, the participants' calibrated coordinates, 45 totals per tile of FTK_POSE_TILE points, the model block."""
    n = int(n)
    return 16 + _up16(16 * n) + _up16(4 * 45 * -(-n // FTK_POSE_TILE)) + 128


def pnp_ransac_workspace_bytes(n: int, hypotheses: int, refine_iterations: int = 0) -> int:
    """Bytes of workspace ftk_pnp_ransac_device needs, the value ftk_pnp_ransac_workspace_bytes returns (pure Python; csrc/pnp_plan.cpp): M,
    the participants' (x, y, X, Y), Z and indices, per hypothesis a count, a model of 12 floats and a validity flag, per tile of
    FTK_POSE_TILE points 27 totals and an inlier count, the pose and the flags.  The same for every refine_iterations."""
    n, k = int(n), int(hypotheses)
    tiles = -(-n // FTK_POSE_TILE)
    return 16 + _up16(16 * n) + 2 * _up16(4 * n) + _up16(4 * k) + _up16(4 * FTK_PNP_MODEL_FLOATS * k) + _up16(k) + _up16(4 * 27 * tiles) + _up16(4 * tiles) + 32 + 16


def keypoint_decode_workspace_bytes(cell_rows: int, cell_cols: int, min_distance: int, n_occupied: int = 0) -> int:
    """Bytes of workspace ftk_keypoint_decode_device needs, the value ftk_keypoint_decode_workspace_bytes returns (pure Python;
    csrc/keypoint_decode_plan.cpp): three 64-bit planes of the 8 cell_rows x 8 cell_cols image, the survivor list and its count, and with
    occupied points two byte planes."""
    px = 64 * int(cell_rows) * int(cell_cols)
    d = max(int(min_distance), 1)
    capacity = -(-8 * int(cell_rows) // d) * -(-8 * int(cell_cols) // d)
    return 3 * _up16(8 * px) + _up16(8 * capacity) + 16 + (2 * _up16(px) if int(n_occupied) > 0 else 0)


def match_assignment_workspace_bytes(rows0: int, rows1: int, dim: int, with_weights: bool) -> int:
    """Bytes of workspace ftk_match_assignment_device needs, the value ftk_match_assignment_workspace_bytes returns (pure Python;
    csrc/match_assignment_plan.cpp): the two normalisers, and with weights the projected descriptors, z and ls(z), ls(-z) of both sides."""
    m, n, d = int(rows0), int(rows1), int(dim)
    own = _up16(4 * m) + _up16(4 * n)
    return own + (_up16(4 * (m + n) * d) + _up16(4 * (m + n)) + _up16(8 * m) + _up16(8 * n) if with_weights else 0)


def transformer_layer_workspace_bytes(rows0: int, rows1: int, dim: int, heads: int = 4) -> int:
    """Bytes of workspace ftk_transformer_layer_device needs, the value ftk_transformer_layer_workspace_bytes returns (pure Python;
    csrc/transformer_plan.cpp): with R = rows0 + rows1 the q | k | v planes [3][R][D], the attention output, the message and the self
    block's result [R][D] each, and the hidden rows [R][2 D].  ValueError for a shape the library refuses."""
    m, n, d, h = int(rows0), int(rows1), int(dim), int(heads)
    if not (1 <= m <= FTK_TRANSFORMER_MAX_ROWS and 1 <= n <= FTK_TRANSFORMER_MAX_ROWS):
        raise ValueError(f"rows must be in 1 .. FTK_TRANSFORMER_MAX_ROWS = {FTK_TRANSFORMER_MAX_ROWS} per side (got {m} and {n})")
    if not 1 <= d <= FTK_TRANSFORMER_MAX_DIM:
        raise ValueError(f"dim must be in 1 .. FTK_TRANSFORMER_MAX_DIM = {FTK_TRANSFORMER_MAX_DIM} (got {d})")
    if h < 1 or d % h != 0:
        raise ValueError(f"heads = {h} must divide dim = {d}")
    if (d // h) % 2 != 0 or not 2 <= d // h <= FTK_TRANSFORMER_MAX_HEAD_DIM:
        raise ValueError(f"the head dimension must be even and in 2 .. FTK_TRANSFORMER_MAX_HEAD_DIM = {FTK_TRANSFORMER_MAX_HEAD_DIM} (got {d // h})")
    r = m + n
    return _up16(12 * r * d) + 3 * _up16(4 * r * d) + _up16(8 * r * d)


def lightglue_adaptive_workspace_bytes(rows0: int, rows1: int, dim: int, heads: int = 4) -> int:
    """Bytes of workspace the adaptive pass needs, the value ftk_lightglue_adaptive_workspace_bytes returns (pure Python;
    csrc/lightglue_adaptive_plan.cpp): the layer's workspace, the assignment head's, the selected head [D + 1][D] and [D + 1], the gather
    maps [M] and [N], and the matcher's index and status [M].  ValueError for a shape the library refuses."""
    m, n, d = int(rows0), int(rows1), int(dim)
    return (_up16(transformer_layer_workspace_bytes(m, n, d, heads)) + _up16(match_assignment_workspace_bytes(m, n, d, True)) + _up16(4 * (d + 1) * d)
            + _up16(4 * (d + 1)) + 2 * _up16(4 * m) + _up16(4 * n) + _up16(m))


def match_table_workspace_bytes(n_slots: int, rows_cur: int, dim: int) -> int:
    """Bytes of workspace ftk_match_table_update_device needs, the value ftk_match_table_workspace_bytes returns (pure Python;
    csrc/match_table_plan.h): the current rows' slots, int32 [rows_cur], rounded up to 16 bytes."""
    return (4 * int(rows_cur) + 15) & ~15


def transformer_layer_weight_offsets(dim: int):
    """(float offsets of the self block's ten tensors, of the cross block's, the total) in ftk_transformer_layer_device's packed weights
    (csrc/transformer_plan.cpp): per block the input Linear and bias, the output Linear and bias, ffn.0 and bias, LayerNorm's weight and
    bias, ffn.3 and bias."""
    d, at, blocks = int(dim), 0, []
    for in_outs in (3 * d, 2 * d):
        offsets = []
        for size in (in_outs * d, in_outs, d * d, d, 4 * d * d, 2 * d, 2 * d, 2 * d, 2 * d * d, d):
            offsets.append(at)
            at += size
        blocks.append(tuple(offsets))
    return blocks[0], blocks[1], at


def _gemm_k_steps(in_channels: int, chunk: int, taps: int) -> int:
    """MFMA k-steps of a packed weight matrix (include/ftk.h): whole chunks of ``chunk`` input channels of ``taps`` k each, two k per step."""
    return -(-int(in_channels) // chunk) * (chunk * taps // 2)


def sep_conv_gru_k_steps(in_channels: int, kernel_size: int) -> int:
    """MFMA k-steps of a packed SepConvGru weight matrix: chunks of FTK_SEP_CONV_GRU_CHUNK input channels, ``kernel_size`` taps."""
    return _gemm_k_steps(in_channels, FTK_SEP_CONV_GRU_CHUNK, int(kernel_size))


def sep_conv_gru_packed_elements(out_channels: int, in_channels: int, kernel_size: int) -> int:
    """Floats of the packed matrix, the value ftk_sep_conv_gru_packed_elements returns (pure Python: argument checks need no library)."""
    return -(-int(out_channels) // 32) * sep_conv_gru_k_steps(in_channels, kernel_size) * 64


def conv2d_k_steps(in_channels: int, kernel_size: int) -> int:
    """MFMA k-steps of a packed conv2d weight matrix: chunks of FTK_CONV2D_CHUNK[kernel_size] input channels, ``kernel_size`` squared taps."""
    return _gemm_k_steps(in_channels, FTK_CONV2D_CHUNK[int(kernel_size)], int(kernel_size) ** 2)


def conv2d_packed_elements(out_channels: int, in_channels: int, kernel_size: int) -> int:
    """Floats of the packed matrix, the value ftk_conv2d_packed_elements returns (pure Python: argument checks need no library)."""
    return -(-int(out_channels) // 32) * conv2d_k_steps(in_channels, kernel_size) * 64


def part_list(parts, noun: str, limit: int) -> list:
    """``parts`` as a list of 1 .. ``limit`` tensors; ``noun`` is what the refusal calls them.  Shared by _device_sep_conv_gru.py and _device_raft_conv.py."""
    parts = list(parts)
    if not 1 <= len(parts) <= limit:
        raise ValueError(f"{noun} must be 1 .. {limit} tensors (got {len(parts)})")
    return parts


def checked_channels(label: str, parts, B: int, H: int, W: int, dev) -> int:
    """``device._check`` of every part as a contiguous float32 [B, C_i >= 1, H, W] tensor on ``dev``; the sum of the C_i."""
    from . import device as D

    channels = 0
    for i, part in enumerate(parts):
        D._check(f"{label}[{i}]", part, D._F32, (B, None, H, W), dev)
        if int(part.shape[1]) < 1:
            raise ValueError(f"{label}[{i}] must have at least one channel (got {list(part.shape)})")
        channels += int(part.shape[1])
    return channels


def part_array(parts):
    """The ftk_gru_part array of parts that passed ``checked_channels``."""
    return (GruPart * len(parts))(*[GruPart(C.c_void_p(p.data_ptr()), int(p.shape[1])) for p in parts])
