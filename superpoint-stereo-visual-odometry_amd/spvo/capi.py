"""ctypes binding of the C ABI in include/spvo.h (used by tests/ and bench.py).

There is no CPU path: `load()` raises if libspvo.so has not been built
(`python __graft_entry__.py` or `make -C superpoint-stereo-visual-odometry_amd`).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.environ.get("SPVO_LIB_DIR") or os.path.dirname(_HERE), "libspvo.so")   # SPVO_LIB_DIR: a side build (make BUILD=... OUT=variants/x) for A/B measurements


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("net_height", C.c_int), ("net_width", C.c_int),
                ("max_batch", C.c_int), ("conf_thresh", C.c_float), ("dist_thresh", C.c_int),
                ("border_remove", C.c_int), ("max_keypoints", C.c_int), ("bug_compat_p", C.c_int)]


class Features(C.Structure):
    _fields_ = [("n", C.c_int), ("xy", C.POINTER(C.c_float)), ("desc", C.POINTER(C.c_float))]


class ClassicOpts(C.Structure):
    _fields_ = [("kind", C.c_int), ("nfeatures", C.c_int), ("max_corners", C.c_int), ("quality_level", C.c_double), ("min_distance", C.c_double), ("block_size", C.c_int),
                ("fast_threshold", C.c_int), ("fast_nonmax", C.c_int), ("slot_capacity", C.c_int)]


class ClassicFeatures(C.Structure):
    _fields_ = [("n", C.c_int), ("kp", C.c_void_p), ("desc", C.c_void_p), ("cap", C.c_int)]


CLASSIC_KINDS = {"ORB": 0, "ShiTomasi": 1, "GFTT": 1, "FAST": 2, "ShiTomasi+BRISK": 3, "GFTT+BRISK": 3, "FAST+BRISK": 4}
CLASSIC_BRISK_KINDS = (3, 4)          # spvo_classic_kind values whose rows are 64 bytes
CLASSIC_SIFT_KINDS = {"ShiTomasi": 5, "GFTT": 5, "FAST": 6}   # spvo_classic_kind values of spvo_classic_sift_pair, by detector


class BriskFeatures(C.Structure):          # spvo_brisk_features
    _fields_ = [("n", C.c_int), ("kp", C.c_void_p), ("desc", C.c_void_p), ("cap", C.c_int)]


class AkazeFeatures(C.Structure):          # spvo_akaze_features
    _fields_ = [("n", C.c_int), ("kp", C.c_void_p), ("desc", C.c_void_p), ("cap", C.c_int)]


class SiftFeatures(C.Structure):
    _fields_ = [("n", C.c_int), ("kp", C.c_void_p), ("desc", C.c_void_p), ("cap", C.c_int)]


class AkazeSiftFeatures(C.Structure):      # spvo_akaze_sift_features: AKAZE records (28 bytes), rows of 128 floats
    _fields_ = [("n", C.c_int), ("kp", C.c_void_p), ("desc", C.c_void_p), ("cap", C.c_int)]


class DetectMirrors(C.Structure):
    _fields_ = [("n", C.c_int * 2), ("xy", C.POINTER(C.c_float) * 2), ("desc", C.POINTER(C.c_float) * 2), ("resized", C.POINTER(C.c_uint8) * 2), ("token", C.c_int)]


class RansacOpts(C.Structure):
    _fields_ = [("iterations", C.c_int), ("reproj_error", C.c_double), ("confidence", C.c_double),
                ("seed", C.c_uint32)]


class RefineOpts(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("huber_delta", C.c_double)]


class RefineSummary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("usable", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double)]


class SolveInput(C.Structure):
    _fields_ = [("n", C.c_int), ("xy_cl", C.c_void_p), ("xy_cr", C.c_void_p), ("xy_pl", C.c_void_p), ("xy_pr", C.c_void_p),
                ("prev_xyz", C.c_void_p), ("prev_valid", C.c_void_p), ("P_l", C.c_double * 12), ("P_r", C.c_double * 12),
                ("rvec_pred", C.c_double * 3), ("tvec_pred", C.c_double * 3), ("frame_count", C.c_int),
                ("refinement_degree", C.c_int), ("ransac", RansacOpts), ("refine", RefineOpts), ("prev_index", C.c_void_p), ("late_prior", C.c_int)]


class SolveOutput(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("rvec", C.c_double * 3), ("tvec", C.c_double * 3),
                ("pnp_ok", C.c_int), ("accepted", C.c_int), ("refined", C.c_int), ("n_inliers", C.c_int),
                ("summary", RefineSummary)]


SIFT_KP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32), ("octave", np.int32)])   # spvo_sift_keypoint
BRISK_KP_DTYPE = SIFT_KP_DTYPE   # spvo_brisk_keypoint: octave is the layer 0..5, angle is -1
AKAZE_KP_DTYPE = np.dtype(SIFT_KP_DTYPE.descr + [("class_id", np.int32)])   # spvo_akaze_keypoint: class_id is the level 0..15, angle is 0
AKAZE_CAND_DTYPE = np.dtype([("level", np.int32), ("row", np.int32), ("col", np.int32), ("response", np.float32), ("ok", np.int32)])   # spvo_akaze_candidate
AKAZE_DESC_BYTES = 61                                                       # SPVO_AKAZE_DESC_BYTES: the full MLDB descriptor, 486 bits
OBS_DTYPE = np.dtype([("X", np.float32, 3), ("uv", np.float32, 2), ("cam", np.int32), ("inverse", np.int32)])

# every symbol include/spvo.h declares
SYMBOLS = [
    "spvo_default_config", "spvo_create", "spvo_destroy", "spvo_last_error", "spvo_load_weights", "spvo_engine_precision", "spvo_set_fp32_split", "spvo_set_int8_general",
    "spvo_preprocess", "spvo_forward", "spvo_debug_tensor", "spvo_heatmap", "spvo_nms",
    "spvo_sample_descriptors", "spvo_detect", "spvo_detect_dev", "spvo_detect_dev_submit", "spvo_detect_wait", "spvo_set_trunk_pairing", "spvo_detect_submit", "spvo_detect_collect", "spvo_detect_collect_mirrors", "spvo_detect_mirrors_wait", "spvo_match", "spvo_match_slots", "spvo_set_prematch", "spvo_set_match_fp8", "spvo_get_match_fp8", "spvo_match_last_form",
    "spvo_match_hamming", "spvo_default_classic_opts", "spvo_classic_detect", "spvo_classic_slot_rows", "spvo_match_hamming_slots", "spvo_orb_detect", "spvo_orb_tables", "spvo_gftt_detect", "spvo_gftt_last_rounds", "spvo_fast_detect", "spvo_orb_describe", "spvo_orb_describe_octaves", "spvo_brisk_describe", "spvo_brisk_tables", "spvo_brisk_detect", "spvo_brisk_detect_debug_layer", "spvo_brisk_detect_pair", "spvo_akaze_detect", "spvo_akaze_debug_level", "spvo_akaze_last_contrast", "spvo_akaze_tables", "spvo_akaze_describe", "spvo_akaze_detect_pair", "spvo_akaze_suppress_debug", "spvo_brisk_orb_pair", "spvo_akaze_orb_pair", "spvo_akaze_brisk_pair", "spvo_orb_octaves_link_debug", "spvo_sift_detect", "spvo_sift_debug_level", "spvo_sift_describe", "spvo_sift_detect_pair", "spvo_classic_sift_pair", "spvo_brisk_sift_pair", "spvo_akaze_sift_pair", "spvo_orb_brisk_pair", "spvo_orb_sift_pair", "spvo_sift_brisk_pair", "spvo_sift_records_debug", "spvo_sift_link_debug", "spvo_sift_slot_rows", "spvo_match_l2_slots", "spvo_sift_order_debug", "spvo_classic_slot_fill_debug", "spvo_match_l2", "spvo_match_l2_u8", "spvo_match_l2_u8_slots", "spvo_set_binary_prematch_norm", "spvo_triangulate", "spvo_pnp_ransac", "spvo_pnp_refine", "spvo_solve_stereo_odometry", "spvo_solve_submit", "spvo_solve_wait", "spvo_solve_wait_prior", "spvo_solve_pending", "spvo_stream", "spvo_synchronize",
    "spvo_profile_enable", "spvo_profile_reset", "spvo_profile_only", "spvo_profile_count", "spvo_profile_get", "spvo_profile_stage_kernel", "spvo_profile_stage_variant", "spvo_profile_stage_fused",
    "spvo_set_tuning", "spvo_get_tuning", "spvo_clear_tuning",
    "spvo_comm_unique_id", "spvo_comm_available", "spvo_comm_create", "spvo_comm_create_host", "spvo_comm_rank", "spvo_comm_world", "spvo_comm_destroy",
    "spvo_pose_allgather", "spvo_pose_allgather_n",
]

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build the HIP library first "
                           "(python __graft_entry__.py); there is no CPU path")
    lib = C.CDLL(LIB_PATH)
    vp, ip, fp, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)
    lib.spvo_default_config.argtypes = [C.POINTER(Config)]
    lib.spvo_default_config.restype = None
    lib.spvo_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.spvo_destroy.argtypes = [vp]
    lib.spvo_destroy.restype = None
    lib.spvo_last_error.argtypes = [vp]
    lib.spvo_last_error.restype = C.c_char_p
    lib.spvo_load_weights.argtypes = [vp, C.c_char_p]
    lib.spvo_set_int8_general.argtypes = [vp, C.c_int]
    lib.spvo_preprocess.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, dp, vp]
    lib.spvo_forward.argtypes = [vp, vp, C.c_int, vp, vp]
    lib.spvo_debug_tensor.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    lib.spvo_heatmap.argtypes = [vp, vp, vp]
    lib.spvo_nms.argtypes = [vp, vp, vp, ip]
    lib.spvo_sample_descriptors.argtypes = [vp, vp, vp, C.c_int, vp]
    lib.spvo_detect.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, dp, dp, C.c_int, C.c_int,
                                C.POINTER(Features), C.POINTER(Features), vp, vp]
    lib.spvo_detect_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, dp, dp, C.c_int, C.c_int,
                                    C.POINTER(Features), C.POINTER(Features)]
    lib.spvo_detect_dev_submit.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int]
    lib.spvo_detect_wait.argtypes = [vp, dp, dp, C.POINTER(Features), C.POINTER(Features)]
    lib.spvo_detect_submit.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int]
    lib.spvo_detect_collect.argtypes = [vp, dp, dp, C.POINTER(Features), C.POINTER(Features), vp, vp]
    lib.spvo_detect_collect_mirrors.argtypes = [vp, dp, dp, C.POINTER(DetectMirrors)]
    lib.spvo_detect_mirrors_wait.argtypes = [vp, C.POINTER(DetectMirrors)]
    lib.spvo_set_tuning.argtypes = [C.c_char_p, C.c_int]
    lib.spvo_get_tuning.argtypes = [C.c_char_p, C.c_int]
    lib.spvo_get_tuning.restype = C.c_int
    lib.spvo_clear_tuning.argtypes = []
    lib.spvo_clear_tuning.restype = None
    lib.spvo_match.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
    lib.spvo_match_slots.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
    lib.spvo_match_last_form.argtypes = [vp, ip]
    lib.spvo_match_hamming.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
    lib.spvo_orb_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, vp, vp, C.c_int, ip]
    lib.spvo_orb_tables.argtypes = [vp, vp]
    lib.spvo_gftt_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp, C.c_int, ip]
    lib.spvo_gftt_last_rounds.argtypes = [vp, vp, ip]
    lib.spvo_fast_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, vp, C.c_int, ip]
    lib.spvo_orb_describe.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, vp, vp, vp, ip]
    lib.spvo_orb_describe_octaves.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_int, vp, vp, vp, ip]
    lib.spvo_brisk_describe.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_int, vp, vp, vp, vp, ip]
    lib.spvo_brisk_tables.argtypes = [C.c_int, vp, vp, vp, vp, vp]
    lib.spvo_brisk_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, ip]
    lib.spvo_brisk_detect_debug_layer.argtypes = [vp, C.c_int, C.c_int, vp, ip, ip]
    lib.spvo_brisk_detect_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BriskFeatures), C.POINTER(BriskFeatures)]
    lib.spvo_akaze_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_float, vp, C.c_int, ip]
    lib.spvo_akaze_debug_level.argtypes = [vp, C.c_int, C.c_int, vp, ip, ip]
    lib.spvo_akaze_last_contrast.argtypes = [vp, vp, ip]
    lib.spvo_akaze_tables.argtypes = [C.c_int, C.c_int, ip, vp, vp, vp, vp, vp, C.c_int, ip, vp, vp]
    lib.spvo_akaze_describe.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, vp, vp]
    lib.spvo_akaze_detect_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(AkazeFeatures), C.POINTER(AkazeFeatures)]
    lib.spvo_akaze_suppress_debug.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, ip]
    lib.spvo_brisk_orb_pair.argtypes = lib.spvo_brisk_detect_pair.argtypes
    lib.spvo_akaze_orb_pair.argtypes = lib.spvo_akaze_brisk_pair.argtypes = lib.spvo_akaze_detect_pair.argtypes
    lib.spvo_orb_octaves_link_debug.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, ip]
    lib.spvo_sift_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_int, ip]
    lib.spvo_sift_debug_level.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, ip, ip]
    lib.spvo_sift_describe.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, C.c_int, vp]
    lib.spvo_sift_detect_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(SiftFeatures), C.POINTER(SiftFeatures)]
    lib.spvo_brisk_sift_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SiftFeatures), C.POINTER(SiftFeatures)]
    lib.spvo_akaze_sift_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(AkazeSiftFeatures), C.POINTER(AkazeSiftFeatures)]
    lib.spvo_orb_brisk_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BriskFeatures), C.POINTER(BriskFeatures)]
    lib.spvo_orb_sift_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SiftFeatures), C.POINTER(SiftFeatures)]
    lib.spvo_sift_brisk_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(BriskFeatures), C.POINTER(BriskFeatures)]
    lib.spvo_sift_records_debug.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, vp, C.c_int, ip]
    lib.spvo_sift_link_debug.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, ip]
    lib.spvo_classic_sift_pair.argtypes = [vp, C.POINTER(ClassicOpts), vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(SiftFeatures), C.POINTER(SiftFeatures)]
    lib.spvo_sift_slot_rows.argtypes = [vp, C.c_int, ip]
    lib.spvo_match_l2_slots.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
    lib.spvo_sift_order_debug.argtypes = [vp, vp, C.c_int, vp, ip]
    lib.spvo_match_l2.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
    lib.spvo_set_prematch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_float]
    lib.spvo_default_classic_opts.argtypes = [C.POINTER(ClassicOpts), C.c_int]
    lib.spvo_default_classic_opts.restype = None
    lib.spvo_classic_detect.argtypes = [vp, C.POINTER(ClassicOpts), vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(ClassicFeatures), C.POINTER(ClassicFeatures)]
    lib.spvo_classic_slot_rows.argtypes = [vp, C.c_int, ip]
    lib.spvo_classic_slot_fill_debug.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int]
    lib.spvo_match_hamming_slots.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
    lib.spvo_match_l2_u8.argtypes = lib.spvo_match_hamming.argtypes
    lib.spvo_match_l2_u8_slots.argtypes = lib.spvo_match_hamming_slots.argtypes
    lib.spvo_set_binary_prematch_norm.argtypes = [vp, C.c_int]
    lib.spvo_triangulate.argtypes = [vp, dp, dp, vp, vp, C.c_int, vp]
    lib.spvo_pnp_ransac.argtypes = [vp, dp, vp, vp, C.c_int, C.POINTER(RansacOpts), dp, dp, vp, ip, ip]
    lib.spvo_pnp_refine.argtypes = [vp, dp, dp, vp, C.c_int, C.POINTER(RefineOpts), dp, dp,
                                    C.POINTER(RefineSummary)]
    lib.spvo_solve_stereo_odometry.argtypes = [vp, C.POINTER(SolveInput), C.POINTER(SolveOutput), vp, vp]
    lib.spvo_solve_submit.argtypes = [vp, C.POINTER(SolveInput)]
    lib.spvo_solve_wait.argtypes = [vp, C.POINTER(SolveOutput), vp, vp]
    lib.spvo_solve_wait_prior.argtypes = [vp, vp, vp, C.c_int, C.POINTER(SolveOutput), vp, vp]
    lib.spvo_solve_pending.argtypes = [vp]
    lib.spvo_stream.argtypes = [vp]
    lib.spvo_stream.restype = vp
    lib.spvo_synchronize.argtypes = [vp]
    lib.spvo_profile_enable.argtypes = [vp, C.c_int]
    lib.spvo_profile_reset.argtypes = [vp]
    lib.spvo_profile_only.argtypes = [vp, C.c_char_p]
    lib.spvo_profile_count.argtypes = [vp]
    lib.spvo_profile_get.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t, dp, C.POINTER(C.c_longlong), dp, dp]
    lib.spvo_profile_stage_kernel.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t, dp]
    lib.spvo_profile_stage_variant.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
    lib.spvo_profile_stage_fused.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
    lib.spvo_comm_unique_id.argtypes = [vp]
    lib.spvo_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    lib.spvo_comm_create_host.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    lib.spvo_comm_rank.argtypes = [vp]
    lib.spvo_comm_world.argtypes = [vp]
    lib.spvo_comm_destroy.argtypes = [vp]
    lib.spvo_comm_destroy.restype = None
    lib.spvo_pose_allgather.argtypes = [vp, dp, dp]
    lib.spvo_pose_allgather_n.argtypes = [vp, dp, C.c_int, dp]
    _lib = lib
    return lib


class SpvoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"spvo error {code}: {msg}")
        self.code = code


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u8_rows(img) -> np.ndarray:
    """a 2-D u8 image whose rows are contiguous; a strided view (rows of a larger image) is passed as it is, with its row stride"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1 or img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img, np.uint8)
    return img


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Context:
    """Thin object wrapper: one method per C entry point, numpy in / numpy out."""

    def __init__(self, **kw):
        self.lib = load()
        self.cfg = Config()
        self.lib.spvo_default_config(C.byref(self.cfg))
        for k, v in kw.items():
            if not hasattr(self.cfg, k):
                raise TypeError(k)
            setattr(self.cfg, k, v)
        self.h = C.c_void_p()
        rc = self.lib.spvo_create(C.byref(self.cfg), C.byref(self.h))
        if rc:
            raise SpvoError(rc, self.lib.spvo_last_error(None).decode())
        self.H, self.W = self.cfg.net_height, self.cfg.net_width
        self.Hc, self.Wc = self.H // 8, self.W // 8
        self.cap = self.cfg.max_keypoints

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.spvo_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc:
            raise SpvoError(rc, self.lib.spvo_last_error(self.h).decode())

    def load_weights(self, path: str):
        self._check(self.lib.spvo_load_weights(self.h, path.encode()))

    def preprocess(self, img: np.ndarray, P: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        img = np.ascontiguousarray(img, np.uint8)
        P2 = np.ascontiguousarray(P, np.float64).reshape(12).copy()
        out = np.empty((self.H, self.W), np.uint8)
        self._check(self.lib.spvo_preprocess(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0],
                                             _dptr(P2), _ptr(out)))
        return out, P2.reshape(3, 4)

    def forward(self, x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        x = np.ascontiguousarray(x, np.float32)
        b = x.shape[0]
        assert x.shape == (b, 1, self.H, self.W)
        det = np.empty((b, 65, self.Hc, self.Wc), np.float32)
        desc = np.empty((b, self.Hc, self.Wc, 256), np.float32)
        self._check(self.lib.spvo_forward(self.h, _ptr(x), b, _ptr(det), _ptr(desc)))
        return det, desc

    def debug_tensor(self, tid: int, batch: int, channels: int, level: int) -> np.ndarray:
        out = np.empty((batch, channels, self.H >> level, self.W >> level), np.float32)
        self._check(self.lib.spvo_debug_tensor(self.h, tid, batch, _ptr(out), out.size))
        return out

    def heatmap(self, det: np.ndarray) -> np.ndarray:
        det = np.ascontiguousarray(det, np.float32)
        assert det.shape == (65, self.Hc, self.Wc)
        heat = np.empty((self.H, self.W), np.float32)
        self._check(self.lib.spvo_heatmap(self.h, _ptr(det), _ptr(heat)))
        return heat

    def nms(self, heat: np.ndarray) -> np.ndarray:
        heat = np.ascontiguousarray(heat, np.float32)
        assert heat.shape == (self.H, self.W)
        xy = np.zeros((self.cap, 2), np.int32)
        n = C.c_int(0)
        self._check(self.lib.spvo_nms(self.h, _ptr(heat), _ptr(xy), C.byref(n)))
        return xy[:n.value].copy()

    def sample_descriptors(self, desc_nhwc: np.ndarray, xy: np.ndarray) -> np.ndarray:
        desc_nhwc = np.ascontiguousarray(desc_nhwc, np.float32)
        assert desc_nhwc.shape == (self.Hc, self.Wc, 256)
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        out = np.empty((len(xy), 256), np.float32)
        self._check(self.lib.spvo_sample_descriptors(self.h, _ptr(desc_nhwc), _ptr(xy), len(xy), _ptr(out)))
        return out

    def _features(self, want_desc=True):
        xy = np.zeros((self.cap, 2), np.float32)
        desc = np.zeros((self.cap, 256), np.float32) if want_desc else None
        f = Features(0, xy.ctypes.data_as(C.POINTER(C.c_float)),
                     desc.ctypes.data_as(C.POINTER(C.c_float)) if want_desc else None)
        return f, xy, desc

    def detect(self, img_l: np.ndarray, img_r: np.ndarray, P_l, P_r, slot_l=2, slot_r=3, want_resized=False):
        img_l = np.ascontiguousarray(img_l, np.uint8)
        img_r = np.ascontiguousarray(img_r, np.uint8)
        assert img_l.shape == img_r.shape and img_l.strides == img_r.strides
        Pl = np.ascontiguousarray(P_l, np.float64).reshape(12).copy()
        Pr = np.ascontiguousarray(P_r, np.float64).reshape(12).copy()
        fl, xyl, dl = self._features()
        fr, xyr, dr = self._features()
        rl = np.empty((self.H, self.W), np.uint8) if want_resized else None
        rr = np.empty((self.H, self.W), np.uint8) if want_resized else None
        self._check(self.lib.spvo_detect(self.h, _ptr(img_l), _ptr(img_r), img_l.shape[0], img_l.shape[1],
                                         img_l.strides[0], _dptr(Pl), _dptr(Pr), slot_l, slot_r,
                                         C.byref(fl), C.byref(fr), _ptr(rl), _ptr(rr)))
        out = dict(xy_l=xyl[:fl.n].copy(), desc_l=dl[:fl.n].copy(), xy_r=xyr[:fr.n].copy(),
                   desc_r=dr[:fr.n].copy(), P_l=Pl.reshape(3, 4), P_r=Pr.reshape(3, 4))
        if want_resized:
            out["resized_l"], out["resized_r"] = rl, rr
        return out

    def detect_dev(self, d_img_l: int, d_img_r: int, rows: int, cols: int, stride: int, P_l, P_r,
                   slot_l=2, slot_r=3, want_desc=False):
        Pl = np.ascontiguousarray(P_l, np.float64).reshape(12).copy()
        Pr = np.ascontiguousarray(P_r, np.float64).reshape(12).copy()
        fl, xyl, dl = self._features(want_desc)
        fr, xyr, dr = self._features(want_desc)
        self._check(self.lib.spvo_detect_dev(self.h, C.c_void_p(d_img_l), C.c_void_p(d_img_r), rows, cols, stride,
                                             _dptr(Pl), _dptr(Pr), slot_l, slot_r, C.byref(fl), C.byref(fr)))
        return dict(xy_l=xyl[:fl.n], xy_r=xyr[:fr.n], desc_l=None if dl is None else dl[:fl.n],
                    desc_r=None if dr is None else dr[:fr.n], P_l=Pl.reshape(3, 4), P_r=Pr.reshape(3, 4))

    def set_fp32_split(self, enable: bool):
        """FP32 engines loaded after this call evaluate their convolutions on the bf16x3 split kernels (include/spvo.h)."""
        self._check(self.lib.spvo_set_fp32_split(self.h, int(enable)))

    def set_int8_general(self, enable: bool):
        """INT8 engines loaded after this call may hold a stand-alone max-pool and convolutions whose cin is 16 more than a multiple
        of 32: the squeeze graph (include/spvo.h).  Overrides the process-wide tuning "int8_general" for this context."""
        self._check(self.lib.spvo_set_int8_general(self.h, int(enable)))

    def set_match_fp8(self, enable: bool):
        self._check(self.lib.spvo_set_match_fp8(self.h, int(enable)))

    def match_fp8(self) -> bool:
        rc = self.lib.spvo_get_match_fp8(self.h)
        self._check(min(rc, 0))
        return rc == 1

    def match_last_form(self) -> dict:
        """Which kernels the most recent L2 match ran (spvo_match_last_form): fp8 / fused as bool, nch 4 or 0, jobs (0: none yet)."""
        info = (C.c_int * 4)()
        self._check(self.lib.spvo_match_last_form(self.h, info))
        return dict(fp8=bool(info[0]), fused=bool(info[1]), nch=int(info[2]), jobs=int(info[3]))

    def engine_precision(self) -> str:
        rc = self.lib.spvo_engine_precision(self.h)
        if rc < 0:
            raise SpvoError(rc, "no weights loaded")
        return {0: "FP32", 1: "FP16", 2: "INT8"}[rc]

    def detect_dev_submit(self, d_img_l: int, d_img_r: int, rows: int, cols: int, stride: int, slot_l: int, slot_r: int):
        """Enqueue a detector pass (at most six may be in flight); complete them oldest-first with detect_wait."""
        self._check(self.lib.spvo_detect_dev_submit(self.h, C.c_void_p(d_img_l), C.c_void_p(d_img_r), rows, cols, stride, slot_l, slot_r))

    def set_trunk_pairing(self, on: bool):
        self._check(self.lib.spvo_set_trunk_pairing(self.h, int(on)))

    def detect_submit(self, img_l: np.ndarray, img_r: np.ndarray, slot_l: int, slot_r: int, extras: int = 3):
        """Asynchronous detector pass on HOST images (spvo_detect_submit); complete with detect_collect."""
        img_l = np.ascontiguousarray(img_l, np.uint8)
        img_r = np.ascontiguousarray(img_r, np.uint8)
        self._check(self.lib.spvo_detect_submit(self.h, _ptr(img_l), _ptr(img_r), img_l.shape[0], img_l.shape[1], img_l.strides[0], slot_l, slot_r, extras))

    def detect_collect(self, P_l, P_r, want_desc=True, want_resized=True):
        Pl = np.ascontiguousarray(P_l, np.float64).reshape(12).copy()
        Pr = np.ascontiguousarray(P_r, np.float64).reshape(12).copy()
        fl, xyl, dl = self._features(want_desc)
        fr, xyr, dr = self._features(want_desc)
        rl = np.empty((self.H, self.W), np.uint8) if want_resized else None
        rr = np.empty((self.H, self.W), np.uint8) if want_resized else None
        self._check(self.lib.spvo_detect_collect(self.h, _dptr(Pl), _dptr(Pr), C.byref(fl), C.byref(fr), _ptr(rl), _ptr(rr)))
        out = dict(xy_l=xyl[:fl.n].copy(), xy_r=xyr[:fr.n].copy(), P_l=Pl.reshape(3, 4), P_r=Pr.reshape(3, 4))
        if want_desc:
            out["desc_l"], out["desc_r"] = dl[:fl.n].copy(), dr[:fr.n].copy()
        if want_resized:
            out["resized_l"], out["resized_r"] = rl, rr
        return out

    def detect_collect_mirrors(self, P_l, P_r):
        """spvo_detect_collect_mirrors: numpy VIEWS of the submission's pinned mirrors (valid until seven more submissions)"""
        Pl = np.ascontiguousarray(P_l, np.float64).reshape(12).copy()
        Pr = np.ascontiguousarray(P_r, np.float64).reshape(12).copy()
        m = DetectMirrors()
        self._check(self.lib.spvo_detect_collect_mirrors(self.h, _dptr(Pl), _dptr(Pr), C.byref(m)))
        self._check(self.lib.spvo_detect_mirrors_wait(self.h, C.byref(m)))      # the descriptors arrive beside the matches
        out = dict(P_l=Pl.reshape(3, 4), P_r=Pr.reshape(3, 4))
        for i, side in enumerate("lr"):
            n = m.n[i]
            out["xy_" + side] = np.ctypeslib.as_array(m.xy[i], (max(n, 1), 2))[:n]
            out["desc_" + side] = np.ctypeslib.as_array(m.desc[i], (max(n, 1), 256))[:n] if m.desc[i] else None
            out["resized_" + side] = np.ctypeslib.as_array(m.resized[i], (self.H, self.W)) if m.resized[i] else None
        return out

    def detect_wait(self, P_l, P_r):
        Pl = np.ascontiguousarray(P_l, np.float64).reshape(12).copy()
        Pr = np.ascontiguousarray(P_r, np.float64).reshape(12).copy()
        fl, xyl, _ = self._features(False)
        fr, xyr, _ = self._features(False)
        self._check(self.lib.spvo_detect_wait(self.h, _dptr(Pl), _dptr(Pr), C.byref(fl), C.byref(fr)))
        return dict(xy_l=xyl[:fl.n], xy_r=xyr[:fr.n], P_l=Pl.reshape(3, 4), P_r=Pr.reshape(3, 4))

    def orb(self, img: np.ndarray, nfeatures=2000):
        """ORB keypoints + descriptors of one u8 image (spvo_orb_detect): dict of xy [n,2], angle, response, octave, desc [n,32]."""
        img = np.ascontiguousarray(img, np.uint8)
        kp = np.zeros((nfeatures, 5), np.float32)          # x, y, angle, response, octave (int32 bits)
        desc = np.zeros((nfeatures, 32), np.uint8)
        n = C.c_int(0)
        self._check(self.lib.spvo_orb_detect(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], nfeatures, _ptr(kp), _ptr(desc), nfeatures, C.byref(n)))
        k = min(n.value, nfeatures)
        return dict(xy=kp[:k, :2].copy(), angle=kp[:k, 2].copy(), response=kp[:k, 3].copy(), octave=kp[:k, 4].copy().view(np.int32), desc=desc[:k].copy())

    def orb_tables(self):
        pat = np.zeros(1024, np.float32)
        taps = np.zeros(7, np.float32)
        self._check(self.lib.spvo_orb_tables(_ptr(pat), _ptr(taps)))
        return pat, taps

    def gftt(self, img: np.ndarray, max_corners=1000, quality=0.03, min_distance=7.5, block_size=5):
        """Shi-Tomasi corners of one u8 image (spvo_gftt_detect): dict of xy [n,2] in the order they were kept, response [n]."""
        img = _u8_rows(img)
        cap = max_corners if max_corners > 0 else img.shape[0] * img.shape[1]
        xy = np.zeros((cap, 2), np.float32)
        resp = np.zeros(cap, np.float32)
        n = C.c_int(0)
        self._check(self.lib.spvo_gftt_detect(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], max_corners, quality, min_distance, block_size,
                                              _ptr(xy), _ptr(resp), cap, C.byref(n)))
        self._resident_shape = img.shape
        k = min(n.value, cap)
        return dict(xy=xy[:k].copy(), response=resp[:k].copy())

    def gftt_rounds(self):
        """(undecided candidates after each round launch, rounds of the finish kernel) of the last gftt() call"""
        rem = np.zeros(3, np.int32)
        fin = C.c_int(0)
        self._check(self.lib.spvo_gftt_last_rounds(self.h, _ptr(rem), C.byref(fin)))
        return rem, fin.value

    def fast(self, img: np.ndarray, threshold=10, nonmax_suppression=True):
        """FAST-9/16 corners of one u8 image in raster order (spvo_fast_detect): dict of xy [n,2], response [n]; all of them (no cap)."""
        img = _u8_rows(img)
        cap = (img.shape[0] // 2 + 1) * (img.shape[1] // 2 + 1) if nonmax_suppression else img.shape[0] * img.shape[1]
        xy = np.zeros((cap, 2), np.float32)
        resp = np.zeros(cap, np.float32)
        n = C.c_int(0)
        self._check(self.lib.spvo_fast_detect(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], threshold, int(bool(nonmax_suppression)), _ptr(xy), _ptr(resp),
                                              cap, C.byref(n)))
        assert n.value <= cap
        self._resident_shape = img.shape
        return dict(xy=xy[:n.value].copy(), response=resp[:n.value].copy())

    def orb_describe(self, img, xy: np.ndarray, shape=None):
        """ORB descriptors of given level-0 keypoints (spvo_orb_describe).  img = None: the image of the last gftt() / fast() /
        orb_describe() of this context, still on the device (shape: its (rows, cols), by default the one this object remembers).
        -> dict of kept [m] (indices into xy that survived the 31-pixel border rule), angle [m] rad, desc [m,32]."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        kept = np.zeros(max(n, 1), np.int32)
        angle = np.zeros(max(n, 1), np.float32)
        desc = np.zeros((max(n, 1), 32), np.uint8)
        m = C.c_int(0)
        if img is None:
            rows, cols = shape if shape is not None else getattr(self, "_resident_shape", (0, 0))
            ptr, stride = None, 0
            if rows <= 0 or cols <= 0:
                rows = cols = 1            # nothing remembered: let the library answer (SPVO_ERR_STATE)
        else:
            img = _u8_rows(img)
            (rows, cols), ptr, stride = img.shape, _ptr(img), img.strides[0]
        self._check(self.lib.spvo_orb_describe(self.h, ptr, rows, cols, stride, _ptr(xy), n, _ptr(kept), _ptr(angle), _ptr(desc), C.byref(m)))
        if img is not None:
            self._resident_shape = img.shape
        return dict(kept=kept[:m.value].copy(), angle=angle[:m.value].copy(), desc=desc[:m.value].copy())

    def orb_describe_octaves(self, img, xy: np.ndarray, octave, shape=None):
        """ORB descriptors of given keypoints on the pyramid level their octave names (spvo_orb_describe_octaves); octave: per keypoint,
        or one for all.  img = None: the image the last detector or describe call of this context left on the device (shape as in
        orb_describe).  -> dict of kept [m] (indices into xy that survived the 31-pixel border rule at level 0, grouped by octave), angle [m]
        rad, desc [m,32]."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        octave = np.ascontiguousarray(np.broadcast_to(np.asarray(octave, np.int32), (n,)))
        kept = np.zeros(max(n, 1), np.int32)
        angle = np.zeros(max(n, 1), np.float32)
        desc = np.zeros((max(n, 1), 32), np.uint8)
        m = C.c_int(0)
        if img is None:
            rows, cols = shape if shape is not None else getattr(self, "_resident_shape", (0, 0))
            ptr, stride = None, 0
            if rows <= 0 or cols <= 0:
                rows = cols = 1            # nothing remembered: let the library answer (SPVO_ERR_STATE)
        else:
            img = _u8_rows(img)
            (rows, cols), ptr, stride = img.shape, _ptr(img), img.strides[0]
        self._check(self.lib.spvo_orb_describe_octaves(self.h, ptr, rows, cols, stride, _ptr(xy), _ptr(octave), n, _ptr(kept), _ptr(angle), _ptr(desc), C.byref(m)))
        if img is not None:
            self._resident_shape = img.shape
        return dict(kept=kept[:m.value].copy(), angle=angle[:m.value].copy(), desc=desc[:m.value].copy())

    def brisk_describe(self, img, xy: np.ndarray, size, shape=None, values0=False):
        """BRISK descriptors of given keypoints (spvo_brisk_describe); size: per keypoint, or one for all.  img = None: the image of the
        last gftt() / fast() / orb_describe() / brisk_describe() of this context, still on the device (shape as in orb_describe).
        -> dict of kept [m] (indices into xy that survived the border rule), angle [m] degrees, desc [m,64] and, with values0, the 60
        intensities at rotation 0 [m,60]."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        size = np.ascontiguousarray(np.broadcast_to(np.asarray(size, np.float32), (n,)))
        kept = np.zeros(max(n, 1), np.int32)
        angle = np.zeros(max(n, 1), np.float32)
        desc = np.zeros((max(n, 1), 64), np.uint8)
        v0 = np.zeros((max(n, 1), 60), np.int32) if values0 else None
        m = C.c_int(0)
        if img is None:
            rows, cols = shape if shape is not None else getattr(self, "_resident_shape", (0, 0))
            ptr, stride = None, 0
            if rows <= 0 or cols <= 0:
                rows = cols = 1            # nothing remembered: let the library answer (SPVO_ERR_STATE)
        else:
            img = _u8_rows(img)
            (rows, cols), ptr, stride = img.shape, _ptr(img), img.strides[0]
        self._check(self.lib.spvo_brisk_describe(self.h, ptr, rows, cols, stride, _ptr(xy), _ptr(size), n, _ptr(kept), _ptr(angle), _ptr(desc),
                                                 _ptr(v0) if values0 else None, C.byref(m)))
        if img is not None:
            self._resident_shape = img.shape
        out = dict(kept=kept[:m.value].copy(), angle=angle[:m.value].copy(), desc=desc[:m.value].copy())
        if values0:
            out["values0"] = v0[:m.value].copy()
        return out

    def brisk_detect(self, img: np.ndarray, threshold: int = 30, octaves: int = 3, cap: Optional[int] = None):
        """BRISK keypoints of one u8 image (spvo_brisk_detect): dict of kp [m] (BRISK_KP_DTYPE records: x, y, size, angle = -1, response,
        octave = layer 0..5) and n, the number found; m = min(n, cap).  cap = None: all of them (a second call when the first buffer was too
        small).  The image stays on the device for a brisk_describe(None, ..., shape=img.shape) that follows."""
        img = _u8_rows(img)
        want = 4096 if cap is None else int(cap)
        while True:
            kp = np.zeros(max(want, 1), BRISK_KP_DTYPE)
            n = C.c_int(0)
            self._check(self.lib.spvo_brisk_detect(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], int(threshold), int(octaves), _ptr(kp), want, C.byref(n)))
            if cap is not None or n.value <= want:
                return dict(kp=kp[:min(n.value, want)].copy(), n=n.value)
            want = n.value

    def brisk_detect_layer(self, layer: int, what: int = 0) -> np.ndarray:
        """A layer of the last brisk_detect()'s scale space (spvo_brisk_detect_debug_layer): what = 0 the image, 1 the AGAST 9-16 score map,
        2 (layer 0 only) the 5-8 score map."""
        rows, cols = C.c_int(0), C.c_int(0)
        self._check(self.lib.spvo_brisk_detect_debug_layer(self.h, layer, what, None, C.byref(rows), C.byref(cols)))
        out = np.zeros((rows.value, cols.value), np.uint8)
        self._check(self.lib.spvo_brisk_detect_debug_layer(self.h, layer, what, _ptr(out), C.byref(rows), C.byref(cols)))
        return out

    def akaze_detect(self, img: np.ndarray, threshold: float = 0.001, cap: Optional[int] = None):
        """AKAZE keypoints of one u8 image (spvo_akaze_detect): dict of kp [m] (AKAZE_KP_DTYPE records: x, y, size, angle = 0, response,
        octave, class_id = level) in the order the suppression leaves them, and n, the number found; m = min(n, cap).  cap = None: all of
        them (a second call when the first buffer was too small).  The image stays on the device for a brisk_describe(None, ...,
        shape=img.shape) that follows, its scale space for an akaze_describe(None, kp)."""
        img = _u8_rows(img)
        want = 4096 if cap is None else int(cap)
        while True:
            kp = np.zeros(max(want, 1), AKAZE_KP_DTYPE)
            n = C.c_int(0)
            self._check(self.lib.spvo_akaze_detect(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], float(threshold), _ptr(kp), want, C.byref(n)))
            if cap is not None or n.value <= want:
                self._resident_shape = img.shape
                return dict(kp=kp[:min(n.value, want)].copy(), n=n.value)
            want = n.value

    def akaze_level(self, level: int, what: int = 0) -> np.ndarray:
        """A level of the last akaze_detect()'s scale space (spvo_akaze_debug_level): what = 0 Lt, 1 Lsmooth, 2 Lflow, 3 Ldet."""
        rows, cols = C.c_int(0), C.c_int(0)
        self._check(self.lib.spvo_akaze_debug_level(self.h, level, what, None, C.byref(rows), C.byref(cols)))
        out = np.zeros((rows.value, cols.value), np.float32)
        self._check(self.lib.spvo_akaze_debug_level(self.h, level, what, _ptr(out), C.byref(rows), C.byref(cols)))
        return out

    def akaze_last_contrast(self) -> np.ndarray:
        """The contrast factor of every octave of the last akaze_detect() (spvo_akaze_last_contrast)."""
        k, n = np.zeros(4, np.float32), C.c_int(0)
        self._check(self.lib.spvo_akaze_last_contrast(self.h, _ptr(k), C.byref(n)))
        return k[:n.value].copy()

    def akaze_describe(self, img: Optional[np.ndarray], kp: np.ndarray, shape=None):
        """Orientation and MLDB descriptor of AKAZE keypoints (spvo_akaze_describe): kp [n] AKAZE_KP_DTYPE records (class_id = level; the
        angle that comes in is ignored) -> dict of angle [n] float32 degrees and desc [n, 61] uint8; no keypoint is dropped.  img None:
        on the scale space the last akaze_detect() / akaze_describe(img, ...) left on the device (shape: that image's, default the
        remembered one); otherwise the scale space of img is built first and stays."""
        kp = np.ascontiguousarray(kp, AKAZE_KP_DTYPE)
        n = len(kp)
        angle = np.zeros(max(n, 1), np.float32)
        desc = np.zeros((max(n, 1), AKAZE_DESC_BYTES), np.uint8)
        if img is None:
            rows, cols = shape if shape is not None else getattr(self, "_resident_shape", (0, 0))
            ptr, stride = None, 0
            if rows <= 0 or cols <= 0:
                rows = cols = 16           # nothing remembered: let the library answer (SPVO_ERR_STATE)
        else:
            img = _u8_rows(img)
            (rows, cols), ptr, stride = img.shape, _ptr(img), img.strides[0]
        self._check(self.lib.spvo_akaze_describe(self.h, ptr, rows, cols, stride, _ptr(kp), n, _ptr(angle), _ptr(desc)))
        if img is not None:
            self._resident_shape = img.shape
        return dict(angle=angle[:n].copy(), desc=desc[:n].copy())

    def brisk_detect_pair(self, img_l, img_r, slot_l: int, slot_r: int, threshold: int = 30, octaves: int = 3, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the BRISK detector + extractor into two binary feature slots of 64-byte rows (spvo_brisk_detect_pair).
        -> (left, right): dicts of kp [m] (BRISK_KP_DTYPE records: the detector's, with the extractor's angle in degrees), desc [m, 64] uint8
        and n, the rows the slot holds; m = min(n, cap), cap = None: slot_capacity.  Strided views are accepted.
        On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .n_l, .n_r (and .counts)."""
        want = int(slot_capacity) if cap is None else int(cap)
        return self._pair_call(self.lib.spvo_brisk_detect_pair, (), (int(threshold), int(octaves), slot_l, slot_r, int(slot_capacity)), img_l, img_r, BRISK_KP_DTYPE, (np.uint8, 64),
                               BriskFeatures, want, resident=False)

    def _pair_call(self, call, head, tail, img_l, img_r, kp_dtype, row_dtype, features, want, resident):
        """The Python side of one stereo-pair call, whichever entry point it is: call(ctx, *head, left, right, rows, cols, stride, *tail,
        out_l, out_r).  Both images as u8 rows of one shape and stride; per image a buffer of max(want, 1) records (kp_dtype) and as many
        rows (row_dtype, e.g. (np.uint8, 64)) behind a `features` struct of cap = want; on failure an SpvoError that carries the two counts
        as .n_l, .n_r and .counts.  resident: the call leaves the right image resident, which the *_describe(None, ...) methods and the
        debug hooks look up as _resident_shape.  -> (left, right): dicts of kp [m], desc [m, ...] and n, m = min(n, want)."""
        l, r = _u8_rows(img_l), _u8_rows(img_r)
        if l.shape != r.shape or l.strides[0] != r.strides[0]:
            l, r = np.ascontiguousarray(l), np.ascontiguousarray(r)
            if l.shape != r.shape:
                raise ValueError("the two images of a pair must have one shape")
        bufs = [(np.zeros(max(want, 1), np.dtype(kp_dtype)), np.zeros(max(want, 1), np.dtype(row_dtype))) for _ in range(2)]
        feats = [features(0, kp.ctypes.data, desc.ctypes.data, want) for kp, desc in bufs]
        rc = call(self.h, *head, _ptr(l), _ptr(r), l.shape[0], l.shape[1], l.strides[0], *tail, C.byref(feats[0]), C.byref(feats[1]))
        if rc:
            e = SpvoError(rc, self.lib.spvo_last_error(self.h).decode())
            e.n_l, e.n_r = feats[0].n, feats[1].n
            e.counts = (e.n_l, e.n_r)
            raise e
        if resident:
            self._resident_shape = r.shape
        return tuple(dict(kp=kp[:min(f.n, max(want, 0))].copy(), desc=desc[:min(f.n, max(want, 0))].copy(), n=f.n) for (kp, desc), f in zip(bufs, feats))

    def akaze_detect_pair(self, img_l, img_r, slot_l: int, slot_r: int, threshold: float = 0.001, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the AKAZE detector + descriptor into two binary feature slots of 61-byte rows (spvo_akaze_detect_pair).
        -> (left, right): dicts of kp [m] (AKAZE_KP_DTYPE records: the detector's, with the descriptor's angle in degrees), desc [m, 61] uint8
        and n, the rows the slot holds; m = min(n, cap), cap = None: slot_capacity.  Strided views are accepted.  Afterwards the right
        image and its scale space are resident (akaze_describe(None, ...), akaze_level).
        On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .n_l, .n_r (and .counts)."""
        want = int(slot_capacity) if cap is None else int(cap)
        return self._pair_call(self.lib.spvo_akaze_detect_pair, (), (float(threshold), slot_l, slot_r, int(slot_capacity)), img_l, img_r, AKAZE_KP_DTYPE, (np.uint8, AKAZE_DESC_BYTES),
                               AkazeFeatures, want, resident=True)

    def _octave_pair(self, call, kp_dtype, features, desc_bytes, img_l, img_r, params, slot_l, slot_r, slot_capacity, cap):
        """brisk_detect_pair's protocol around one of the three pair calls whose extractor is another algorithm's."""
        want = int(slot_capacity) if cap is None else int(cap)
        return self._pair_call(call, (), (*params, slot_l, slot_r, int(slot_capacity)), img_l, img_r, kp_dtype, (np.uint8, desc_bytes), features, want, resident=True)

    def brisk_orb_pair(self, img_l, img_r, slot_l: int, slot_r: int, threshold: int = 30, octaves: int = 3, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the BRISK detector and the ORB extractor at the keypoints' octaves into two binary feature slots of
        32-byte rows (spvo_brisk_orb_pair).  -> (left, right): dicts of kp [m] (BRISK_KP_DTYPE records: the detector's that survived the
        extractor's border rule, grouped by octave, with the extractor's angle in radians), desc [m, 32] uint8 and n, as brisk_detect_pair.
        Afterwards the right image is resident.  On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .n_l, .n_r (and .counts)."""
        return self._octave_pair(self.lib.spvo_brisk_orb_pair, BRISK_KP_DTYPE, BriskFeatures, 32, img_l, img_r, (int(threshold), int(octaves)), slot_l, slot_r, slot_capacity, cap)

    def akaze_orb_pair(self, img_l, img_r, slot_l: int, slot_r: int, threshold: float = 0.001, slot_capacity: int = 8192, cap: Optional[int] = None):
        """The same behind the AKAZE detector (spvo_akaze_orb_pair): kp [m] AKAZE_KP_DTYPE records with the extractor's angle in radians,
        desc [m, 32].  Afterwards the right image and its scale space are resident."""
        return self._octave_pair(self.lib.spvo_akaze_orb_pair, AKAZE_KP_DTYPE, AkazeFeatures, 32, img_l, img_r, (float(threshold),), slot_l, slot_r, slot_capacity, cap)

    def akaze_brisk_pair(self, img_l, img_r, slot_l: int, slot_r: int, threshold: float = 0.001, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the AKAZE detector and the BRISK extractor into two binary feature slots of 64-byte rows
        (spvo_akaze_brisk_pair): kp [m] AKAZE_KP_DTYPE records that survived the extractor's border rule, in the detector's order, with the
        extractor's angle in degrees, desc [m, 64].  Afterwards the right image and its scale space are resident."""
        return self._octave_pair(self.lib.spvo_akaze_brisk_pair, AKAZE_KP_DTYPE, AkazeFeatures, 64, img_l, img_r, (float(threshold),), slot_l, slot_r, slot_capacity, cap)

    def orb_octaves_link_debug(self, xy: np.ndarray, octave, keep=None, max_octave: int = 7, shape=None):
        """The ORB pairs' device link and describe kernel on a caller's list against the resident image (spvo_orb_octaves_link_debug):
        xy [n, 2], octave per keypoint (or one for all), keep [n] flags or None, shape as in orb_describe.  -> dict of kept [m] (indices
        into xy), angle [m] rad, desc [m, 32], as orb_describe_octaves(None, ...) on the list without its keep == 0 records."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(xy)
        octave = np.ascontiguousarray(np.broadcast_to(np.asarray(octave, np.int32), (n,)))
        flags = None if keep is None else np.ascontiguousarray(np.asarray(keep) != 0, np.uint8).reshape(n)
        kept = np.zeros(max(n, 1), np.int32)
        angle = np.zeros(max(n, 1), np.float32)
        desc = np.zeros((max(n, 1), 32), np.uint8)
        m = C.c_int(0)
        rows, cols = shape if shape is not None else getattr(self, "_resident_shape", (0, 0))
        if rows <= 0 or cols <= 0:
            rows = cols = 64               # nothing remembered: let the library answer (SPVO_ERR_STATE)
        self._check(self.lib.spvo_orb_octaves_link_debug(self.h, int(rows), int(cols), _ptr(xy), _ptr(octave), None if flags is None else _ptr(flags), n, int(max_octave), _ptr(kept),
                                                         _ptr(angle), _ptr(desc), C.byref(m)))
        return dict(kept=kept[:m.value].copy(), angle=angle[:m.value].copy(), desc=desc[:m.value].copy())

    def akaze_suppress_debug(self, rows: int, cols: int, cand: np.ndarray) -> np.ndarray:
        """The device suppression of akaze_detect_pair on a candidate list (spvo_akaze_suppress_debug): cand [n] AKAZE_CAND_DTYPE records
        (level, row, col, response, ok), level by level, for the level tables of a rows x cols image -> the indices that stay, in output order."""
        cand = np.ascontiguousarray(cand, AKAZE_CAND_DTYPE)
        keep, n = np.zeros(max(len(cand), 1), np.int32), C.c_int(0)
        self._check(self.lib.spvo_akaze_suppress_debug(self.h, int(rows), int(cols), _ptr(cand), len(cand), _ptr(keep), C.byref(n)))
        return keep[:n.value].copy()

    def sift_detect(self, img: np.ndarray, cap: Optional[int] = None):
        """SIFT keypoints + descriptors of one u8 image (spvo_sift_detect): dict of kp [m] (SIFT_KP_DTYPE records), desc [m, 128] float32 (integers
        0..255) and n, the number found; m = min(n, cap).  cap = None: all of them (a second call when the first buffer was too small)."""
        img = _u8_rows(img)
        want = 4096 if cap is None else int(cap)
        while True:
            kp = np.zeros(max(want, 1), SIFT_KP_DTYPE)
            desc = np.zeros((max(want, 1), 128), np.float32)
            n = C.c_int(0)
            self._check(self.lib.spvo_sift_detect(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], _ptr(kp), _ptr(desc), want, C.byref(n)))
            if cap is not None or n.value <= want:
                m = min(n.value, want)
                return dict(kp=kp[:m].copy(), desc=desc[:m].copy(), n=n.value)
            want = n.value

    def sift_describe(self, img, kp: np.ndarray, shape=None) -> np.ndarray:
        """SIFT descriptors of given keypoints (spvo_sift_describe): kp [n] SIFT_KP_DTYPE records (x, y, size, angle in degrees, response,
        packed octave) -> desc [n, 128] float32 (integers 0..255), row i for record i; nothing is erased.  img = None: the image of the last
        gftt() / fast() / brisk_detect() / akaze_detect() / *_describe(img) of this context, still on the device (shape as in brisk_describe)."""
        kp = np.ascontiguousarray(kp, SIFT_KP_DTYPE).reshape(-1)
        n = len(kp)
        desc = np.zeros((max(n, 1), 128), np.float32)
        if img is None:
            rows, cols = shape if shape is not None else getattr(self, "_resident_shape", (0, 0))
            ptr, stride = None, 0
            if rows <= 0 or cols <= 0:
                rows = cols = 1            # nothing remembered: let the library answer
        else:
            img = _u8_rows(img)
            (rows, cols), ptr, stride = img.shape, _ptr(img), img.strides[0]
        self._check(self.lib.spvo_sift_describe(self.h, ptr, rows, cols, stride, _ptr(kp), n, _ptr(desc)))
        if img is not None:
            self._resident_shape = img.shape
        return desc[:n].copy()

    def sift_level(self, octave: int, layer: int, dog: bool = False) -> np.ndarray:
        """A Gaussian (layer 0..5) or difference-of-Gaussians (dog: 0..4) level of the last sift_detect()'s pyramid (spvo_sift_debug_level); after
        sift_describe() a Gaussian level of ITS pyramid, octave 0 being that call's first octave (dog: SPVO_ERR_STATE)."""
        rows, cols = C.c_int(0), C.c_int(0)
        self._check(self.lib.spvo_sift_debug_level(self.h, octave, layer, int(bool(dog)), None, C.byref(rows), C.byref(cols)))
        out = np.zeros((rows.value, cols.value), np.float32)
        self._check(self.lib.spvo_sift_debug_level(self.h, octave, layer, int(bool(dog)), _ptr(out), C.byref(rows), C.byref(cols)))
        return out

    def sift_detect_pair(self, img_l, img_r, slot_l: int, slot_r: int, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the SIFT detector + descriptor into two SIFT slots (spvo_sift_detect_pair) -> (left, right): dicts like
        sift_detect's -- the host's copy of what the slots hold; cap: rows the host buffers take (None: slot_capacity, i.e. all).
        On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .counts."""
        want = max(int(slot_capacity), 1) if cap is None else int(cap)   # (at least 1: a slot_capacity the library refuses is refused as that, not as a bad buffer)
        return self._pair_call(self.lib.spvo_sift_detect_pair, (), (slot_l, slot_r, int(slot_capacity)), img_l, img_r, SIFT_KP_DTYPE, (np.float32, 128), SiftFeatures, want, resident=False)

    def classic_sift_pair(self, img_l, img_r, slot_l: int, slot_r: int, kind="FAST", cap: Optional[int] = None, **opts):
        """One stereo pair through the Shi-Tomasi ("ShiTomasi") or FAST ("FAST") detector and the SIFT extractor into two SIFT slots
        (spvo_classic_sift_pair); kind may also be a spvo_classic_kind number.  opts: fields of spvo_classic_opts that differ from the
        reference's parameters (slot_capacity among them); cap: rows the host buffers take (None: slot_capacity, i.e. all).
        -> (left, right): dicts like sift_detect's -- kp [m] SIFT_KP_DTYPE records {x, y, 5 or 7, -1, response, 0} in the detector's order,
        desc [m, 128], n -- the host's copy of what the slots hold.  On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .counts."""
        o = ClassicOpts()
        self.lib.spvo_default_classic_opts(C.byref(o), CLASSIC_SIFT_KINDS[kind] if isinstance(kind, str) else int(kind))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(k)
            setattr(o, k, v)
        want = max(int(o.slot_capacity), 1) if cap is None else int(cap)   # (at least 1: as sift_detect_pair)
        return self._pair_call(self.lib.spvo_classic_sift_pair, (C.byref(o),), (slot_l, slot_r), img_l, img_r, SIFT_KP_DTYPE, (np.float32, 128), SiftFeatures, want, resident=True)

    def _sift_octave_pair(self, call, kp_dtype, features, img_l, img_r, params, slot_l, slot_r, slot_capacity, cap):
        """classic_sift_pair's protocol around one of the two pair calls whose detector reports an octave."""
        want = int(slot_capacity) if cap is None else int(cap)
        return self._pair_call(call, (), (*params, slot_l, slot_r, int(slot_capacity)), img_l, img_r, kp_dtype, (np.float32, 128), features, want, resident=True)

    def brisk_sift_pair(self, img_l, img_r, slot_l: int, slot_r: int, threshold: int = 30, octaves: int = 3, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the BRISK detector and the SIFT extractor into two SIFT slots (spvo_brisk_sift_pair).  -> (left, right):
        dicts of kp [m] (BRISK_KP_DTYPE: the detector's records, unchanged), desc [m, 128] float32 and n -- per image what brisk_detect()
        followed by sift_describe(None, its records) returns.  Afterwards the right image is resident.  On SPVO_ERR_CAPACITY the SpvoError
        carries the two counts as .counts."""
        return self._sift_octave_pair(self.lib.spvo_brisk_sift_pair, BRISK_KP_DTYPE, SiftFeatures, img_l, img_r, (int(threshold), int(octaves)), slot_l, slot_r, slot_capacity, cap)

    def akaze_sift_pair(self, img_l, img_r, slot_l: int, slot_r: int, threshold: float = 0.001, slot_capacity: int = 8192, cap: Optional[int] = None):
        """The same behind the AKAZE detector (spvo_akaze_sift_pair): kp [m] AKAZE_KP_DTYPE records, unchanged (class_id included), desc
        [m, 128] -- per image what akaze_detect() followed by sift_describe(None, its records without class_id) returns.  Afterwards the
        right image and its scale space are resident."""
        return self._sift_octave_pair(self.lib.spvo_akaze_sift_pair, AKAZE_KP_DTYPE, AkazeSiftFeatures, img_l, img_r, (float(threshold),), slot_l, slot_r, slot_capacity, cap)

    def orb_brisk_pair(self, img_l, img_r, slot_l: int, slot_r: int, nfeatures: int = 2000, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the ORB detector and the BRISK extractor into two binary feature slots of 64-byte rows
        (spvo_orb_brisk_pair).  -> (left, right): dicts of kp [m] (BRISK_KP_DTYPE: x, y, size 31 * 1.2^octave, the extractor's angle in
        degrees, response, octave -- the detector's records that survived the extractor's border rule, in the detector's order), desc
        [m, 64] uint8 and n -- per image what orb_detect() followed by brisk_describe(img, its xy, those sizes) returns.  Afterwards the
        right image is resident.  On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .n_l, .n_r (and .counts)."""
        return self._octave_pair(self.lib.spvo_orb_brisk_pair, BRISK_KP_DTYPE, BriskFeatures, 64, img_l, img_r, (int(nfeatures),), slot_l, slot_r, slot_capacity, cap)

    def orb_sift_pair(self, img_l, img_r, slot_l: int, slot_r: int, nfeatures: int = 2000, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the ORB detector and the SIFT extractor into two SIFT slots (spvo_orb_sift_pair).  -> (left, right):
        dicts of kp [m] (SIFT_KP_DTYPE: x, y, size 31 * 1.2^octave, the detector's angle in degrees, response, octave), desc [m, 128]
        float32 and n -- per image what orb_detect() followed by sift_describe(img, those records) returns; nothing is erased.
        Afterwards the right image is resident.  On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .counts."""
        return self._sift_octave_pair(self.lib.spvo_orb_sift_pair, SIFT_KP_DTYPE, SiftFeatures, img_l, img_r, (int(nfeatures),), slot_l, slot_r, slot_capacity, cap)

    def sift_brisk_pair(self, img_l, img_r, slot_l: int, slot_r: int, slot_capacity: int = 8192, cap: Optional[int] = None):
        """One stereo pair through the SIFT detector and the BRISK extractor into two binary feature slots of 64-byte rows
        (spvo_sift_brisk_pair).  -> (left, right): dicts of kp [m] (BRISK_KP_DTYPE: the detector's x, y, size, response and packed octave
        with the extractor's angle in degrees -- the records that survived the extractor's border rule, in the detector's order, one per
        orientation peak), desc [m, 64] uint8 and n -- per image what sift_detect() followed by brisk_describe(img, its xy, its sizes)
        returns.  Afterwards the right image is resident.  On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .n_l, .n_r (and
        .counts).  set_tuning("sift_brisk_recheck", 1): the second pass on the host's records, forced (diagnostic)."""
        return self._octave_pair(self.lib.spvo_sift_brisk_pair, BRISK_KP_DTYPE, BriskFeatures, 64, img_l, img_r, (), slot_l, slot_r, slot_capacity, cap)

    def sift_records_debug(self, img: np.ndarray, describe: bool = False, cap: Optional[int] = None) -> np.ndarray:
        """sift_brisk_pair's chain of one image up to the records the BRISK extractor's chain reads (spvo_sift_records_debug): kp [n]
        SIFT_KP_DTYPE in the detector's order, the detector's angle still in place.  describe: the describing form of the orientation
        kernel in the other's place (the records must not depend on it).  Afterwards the image is resident."""
        img = _u8_rows(img)
        want = 8192 if cap is None else int(cap)
        while True:
            kp = np.zeros(max(want, 1), SIFT_KP_DTYPE)
            n = C.c_int(0)
            self._check(self.lib.spvo_sift_records_debug(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], int(bool(describe)), _ptr(kp), want, C.byref(n)))
            self._resident_shape = img.shape
            if cap is not None or n.value <= want:
                return kp[:min(n.value, want)].copy()
            want = n.value

    def sift_link_debug(self, kp: np.ndarray, keep=None, max_octave: int = 5, shape=None):
        """The two calls' device link and describe launch on a caller's list against the resident image (spvo_sift_link_debug): kp [n]
        SIFT_KP_DTYPE records, keep [n] flags or None, shape as in sift_describe.  -> dict of kept [m] (indices into kp) and desc [m, 128],
        as sift_describe(None, kp[kept])."""
        kp = np.ascontiguousarray(kp, SIFT_KP_DTYPE).reshape(-1)
        n = len(kp)
        flags = None if keep is None else np.ascontiguousarray(np.asarray(keep) != 0, np.uint8).reshape(n)
        kept = np.zeros(max(n, 1), np.int32)
        desc = np.zeros((max(n, 1), 128), np.float32)
        m = C.c_int(0)
        rows, cols = shape if shape is not None else getattr(self, "_resident_shape", (0, 0))
        if rows <= 0 or cols <= 0:
            rows = cols = 64               # nothing remembered: let the library answer (SPVO_ERR_STATE)
        self._check(self.lib.spvo_sift_link_debug(self.h, int(rows), int(cols), _ptr(kp), None if flags is None else _ptr(flags), n, int(max_octave), _ptr(kept), _ptr(desc), C.byref(m)))
        return dict(kept=kept[:m.value].copy(), desc=desc[:m.value].copy())

    def sift_slot_rows(self, slot: int) -> int:
        n = C.c_int(0)
        self._check(self.lib.spvo_sift_slot_rows(self.h, slot, C.byref(n)))
        return n.value

    def match_l2_slots(self, slot_a: int, slot_b: int, selector="KNN", cross_check=False, ratio=0.8):
        """cv::BFMatcher(NORM_L2) between two SIFT slots, on the device (spvo_match_l2_slots)."""
        n = self.sift_slot_rows(slot_a)
        self.sift_slot_rows(slot_b)
        idx = np.full(max(n, 1), -1, np.int32)
        dist = np.zeros(max(n, 1), np.float32)
        self._check(self.lib.spvo_match_l2_slots(self.h, slot_a, slot_b, 1 if selector == "KNN" else 0, int(cross_check), ratio, _ptr(idx), _ptr(dist)))
        return idx[:n], dist[:n]

    def sift_order(self, rec: np.ndarray) -> np.ndarray:
        """The device ordering stage of sift_detect_pair alone on SIFT_KP_DTYPE records (spvo_sift_order_debug): the indices that stay, in output order."""
        rec = np.ascontiguousarray(rec, SIFT_KP_DTYPE)
        order = np.zeros(max(len(rec), 1), np.int32)
        n = C.c_int(0)
        self._check(self.lib.spvo_sift_order_debug(self.h, _ptr(rec), len(rec), _ptr(order), C.byref(n)))
        return order[:n.value].copy()

    def match_l2(self, a: np.ndarray, b: np.ndarray, selector="KNN", cross_check=False, ratio=0.8, dim: Optional[int] = None):
        """cv::BFMatcher(NORM_L2) on float rows of `dim` columns (spvo_match_l2); dim = None: the arrays' own width (128 when both are empty)."""
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        if dim is None:
            dim = a.shape[1] if a.ndim == 2 and a.shape[1] else (b.shape[1] if b.ndim == 2 and b.shape[1] else 128)
        if dim > 0:
            a, b = a.reshape(-1, dim), b.reshape(-1, dim)
        idx = np.full(len(a), -1, np.int32)
        dist = np.zeros(len(a), np.float32)
        self._check(self.lib.spvo_match_l2(self.h, _ptr(a), len(a), _ptr(b), len(b), dim, 1 if selector == "KNN" else 0, int(cross_check), ratio, _ptr(idx), _ptr(dist)))
        return idx, dist

    def classic_detect(self, img_l, img_r, slot_l: int, slot_r: int, kind="ORB", **opts):
        """One stereo pair through the classic front end's detector + extractor into two binary feature slots (spvo_classic_detect).
        kind "ORB", "ShiTomasi" or "FAST" (ORB extractor), "ShiTomasi+BRISK" or "FAST+BRISK"; opts: fields of spvo_classic_opts that differ
        from the reference's parameters.
        -> (left, right): dicts of xy [n,2], angle (radians; degrees for the BRISK kinds), response, octave, desc [n,32] ([n,64] for the BRISK
        kinds) -- the host's copy of what the slots hold.
        On SPVO_ERR_CAPACITY the SpvoError carries the two counts as .counts."""
        o = ClassicOpts()
        self.lib.spvo_default_classic_opts(C.byref(o), CLASSIC_KINDS[kind] if isinstance(kind, str) else int(kind))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(k)
            setattr(o, k, v)
        cap = max(int(o.slot_capacity), 1)
        kp_rec = (np.float32, 5)                          # x, y, angle, response, octave (int32 bits)
        pair = self._pair_call(self.lib.spvo_classic_detect, (C.byref(o),), (slot_l, slot_r), img_l, img_r, kp_rec, (np.uint8, 64 if o.kind in CLASSIC_BRISK_KINDS else 32), ClassicFeatures,
                               cap, resident=False)       # (a call that succeeds fits its slots, so every row comes back)
        return tuple(dict(xy=f["kp"][:, :2].copy(), angle=f["kp"][:, 2].copy(), response=f["kp"][:, 3].copy(), octave=f["kp"][:, 4].copy().view(np.int32), desc=f["desc"]) for f in pair)

    def classic_slot_rows(self, slot: int) -> int:
        n = C.c_int(0)
        self._check(self.lib.spvo_classic_slot_rows(self.h, slot, C.byref(n)))
        return n.value

    def classic_slot_fill(self, slot: int, desc: np.ndarray) -> None:
        """Caller-supplied rows [n,32] or [n,64] u8 into a binary feature slot (spvo_classic_slot_fill_debug, a test hook)."""
        desc = np.ascontiguousarray(desc, np.uint8)
        if desc.ndim != 2:
            raise ValueError("rows of 32 or 64 bytes expected: a 2-D array")
        self._check(self.lib.spvo_classic_slot_fill_debug(self.h, slot, _ptr(desc) if len(desc) else None, len(desc), desc.shape[1]))

    def match_hamming_slots(self, slot_a: int, slot_b: int, selector="KNN", cross_check=False, ratio=0.8):
        """cv::BFMatcher(NORM_HAMMING) between two binary feature slots, on the device (spvo_match_hamming_slots)."""
        n = self.classic_slot_rows(slot_a)
        self.classic_slot_rows(slot_b)
        idx = np.full(max(n, 1), -1, np.int32)
        dist = np.zeros(max(n, 1), np.float32)
        self._check(self.lib.spvo_match_hamming_slots(self.h, slot_a, slot_b, 1 if selector == "KNN" else 0, int(cross_check), ratio, _ptr(idx), _ptr(dist)))
        return idx[:n], dist[:n]

    def match_hamming(self, a: np.ndarray, b: np.ndarray, selector="KNN", cross_check=False, ratio=0.8):
        """cv::BFMatcher(NORM_HAMMING) on u8 descriptor rows (spvo_match_hamming)."""
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        nbytes = a.shape[1] if a.ndim == 2 and a.shape[1] else (b.shape[1] if b.ndim == 2 and b.shape[1] else 32)
        a = a.reshape(len(a), nbytes)
        b = b.reshape(len(b), nbytes)
        idx = np.full(len(a), -1, np.int32)
        dist = np.zeros(len(a), np.float32)
        self._check(self.lib.spvo_match_hamming(self.h, _ptr(a), len(a), _ptr(b), len(b), nbytes, 1 if selector == "KNN" else 0,
                                                int(cross_check), ratio, _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_l2_u8(self, a: np.ndarray, b: np.ndarray, selector="KNN", cross_check=False, ratio=0.8):
        """MatcherType::FLANN on u8 descriptor rows: the exact L2 nearest neighbours of the bytes as numbers (spvo_match_l2_u8)."""
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        nbytes = a.shape[1] if a.ndim == 2 and a.shape[1] else (b.shape[1] if b.ndim == 2 and b.shape[1] else 32)
        a = a.reshape(len(a), nbytes)
        b = b.reshape(len(b), nbytes)
        idx = np.full(len(a), -1, np.int32)
        dist = np.zeros(len(a), np.float32)
        self._check(self.lib.spvo_match_l2_u8(self.h, _ptr(a), len(a), _ptr(b), len(b), nbytes, 1 if selector == "KNN" else 0,
                                              int(cross_check), ratio, _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_l2_u8_slots(self, slot_a: int, slot_b: int, selector="KNN", cross_check=False, ratio=0.8):
        """spvo_match_l2_u8 between two binary feature slots, on the device (spvo_match_l2_u8_slots)."""
        n = self.classic_slot_rows(slot_a)
        self.classic_slot_rows(slot_b)
        idx = np.full(max(n, 1), -1, np.int32)
        dist = np.zeros(max(n, 1), np.float32)
        self._check(self.lib.spvo_match_l2_u8_slots(self.h, slot_a, slot_b, 1 if selector == "KNN" else 0, int(cross_check), ratio, _ptr(idx), _ptr(dist)))
        return idx[:n], dist[:n]

    def set_binary_prematch_norm(self, norm="HAMMING"):
        """Which matcher the binary pair calls enqueue behind their features (spvo_set_binary_prematch_norm): "HAMMING" (default) or "L2"."""
        self._check(self.lib.spvo_set_binary_prematch_norm(self.h, {"HAMMING": 0, "L2": 1}[norm]))

    def match(self, a: np.ndarray, b: np.ndarray, selector="KNN", cross_check=False, ratio=0.8):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 256)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 256)
        idx = np.full(len(a), -1, np.int32)
        dist = np.zeros(len(a), np.float32)
        self._check(self.lib.spvo_match(self.h, _ptr(a), len(a), _ptr(b), len(b), 1 if selector == "KNN" else 0,
                                        int(cross_check), ratio, _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_slots(self, slot_a: int, slot_b: int, n_a: int, selector="KNN", cross_check=False, ratio=0.8):
        idx = np.full(max(n_a, 1), -1, np.int32)
        dist = np.zeros(max(n_a, 1), np.float32)
        self._check(self.lib.spvo_match_slots(self.h, slot_a, slot_b, 1 if selector == "KNN" else 0,
                                              int(cross_check), ratio, _ptr(idx), _ptr(dist)))
        return idx[:n_a], dist[:n_a]

    def set_prematch(self, enable=True, selector="KNN", cross_check=False, ratio=0.8):
        self._check(self.lib.spvo_set_prematch(self.h, int(enable), 1 if selector == "KNN" else 0, int(cross_check), ratio))

    def triangulate(self, P_l, P_r, xy_l, xy_r) -> np.ndarray:
        Pl = np.ascontiguousarray(P_l, np.float64).reshape(12)
        Pr = np.ascontiguousarray(P_r, np.float64).reshape(12)
        a = np.ascontiguousarray(xy_l, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(xy_r, np.float32).reshape(-1, 2)
        out = np.zeros((len(a), 3), np.float32)
        self._check(self.lib.spvo_triangulate(self.h, _dptr(Pl), _dptr(Pr), _ptr(a), _ptr(b), len(a), _ptr(out)))
        return out

    def pnp_ransac(self, K, xyz, xy, rvec0, tvec0, iterations=500, reproj_error=2.0, seed=0):
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        r = np.ascontiguousarray(rvec0, np.float64).reshape(3).copy()
        t = np.ascontiguousarray(tvec0, np.float64).reshape(3).copy()
        inl = np.zeros(max(len(xyz), 1), np.int32)
        n_inl, ok = C.c_int(0), C.c_int(0)
        opts = RansacOpts(iterations, reproj_error, 0.999, seed)
        self._check(self.lib.spvo_pnp_ransac(self.h, _dptr(K), _ptr(xyz), _ptr(xy), len(xyz), C.byref(opts),
                                             _dptr(r), _dptr(t), _ptr(inl), C.byref(n_inl), C.byref(ok)))
        return bool(ok.value), r, t, inl[:n_inl.value].copy()

    def pnp_refine(self, P_l, P_r, obs: np.ndarray, q0, t0, max_iterations=40, huber_delta=1.0):
        Pl = np.ascontiguousarray(P_l, np.float64).reshape(12)
        Pr = np.ascontiguousarray(P_r, np.float64).reshape(12)
        obs = np.ascontiguousarray(obs, OBS_DTYPE)
        q = np.ascontiguousarray(q0, np.float64).reshape(4).copy()
        t = np.ascontiguousarray(t0, np.float64).reshape(3).copy()
        s = RefineSummary()
        opts = RefineOpts(max_iterations, huber_delta)
        self._check(self.lib.spvo_pnp_refine(self.h, _dptr(Pl), _dptr(Pr), _ptr(obs), len(obs), C.byref(opts),
                                             _dptr(q), _dptr(t), C.byref(s)))
        return q, t, s

    def solve(self, P_l, P_r, cl, cr, pl, pr, prev_xyz=None, prev_valid=None, rvec_pred=(0, 0, 0), tvec_pred=(0, 0, 0),
              frame_count=0, refinement_degree=4, seed=0, iterations=500, reproj_error=2.0, max_iterations=40, split=None, prev_index=None, late_prior=False):
        """spvo_solve_stereo_odometry, or (split="submit") spvo_solve_submit alone: complete with solve_wait(n) / solve_wait_prior(n, ...).
        prev_index: instead of prev_xyz / prev_valid, indices into the points of the previous submit on this context (-1: none);
        late_prior: the prior is handed to solve_wait_prior instead (the previous solve may still be in flight); 2: and the chain's last kernel
        is held back for the next submission's launch (include/spvo.h)."""
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 2) for a in (cl, cr, pl, pr)]
        n = len(arrs[0])
        si = SolveInput()
        si.n = n
        si.xy_cl, si.xy_cr, si.xy_pl, si.xy_pr = [a.ctypes.data for a in arrs]
        if prev_xyz is not None:
            px = np.ascontiguousarray(prev_xyz, np.float32).reshape(-1, 3)
            pv = np.ascontiguousarray(prev_valid, np.int32)
            si.prev_xyz, si.prev_valid = px.ctypes.data, pv.ctypes.data
        si.P_l[:] = np.asarray(P_l, np.float64).reshape(12).tolist()
        si.P_r[:] = np.asarray(P_r, np.float64).reshape(12).tolist()
        si.rvec_pred[:] = list(map(float, rvec_pred))
        si.tvec_pred[:] = list(map(float, tvec_pred))
        si.frame_count, si.refinement_degree = frame_count, refinement_degree
        si.ransac = RansacOpts(iterations, reproj_error, 0.999, seed)
        si.refine = RefineOpts(max_iterations, 1.0)
        if prev_index is not None:
            pi = np.ascontiguousarray(prev_index, np.int32)
            si.prev_index = pi.ctypes.data
        si.late_prior = int(late_prior)
        if split == "submit":      # spvo_solve_submit only: the inputs are staged, complete with solve_wait(n)
            self._check(self.lib.spvo_solve_submit(self.h, C.byref(si)))
            return n
        so = SolveOutput()
        xyz = np.zeros((max(n, 1), 3), np.float32)
        inl = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.spvo_solve_stereo_odometry(self.h, C.byref(si), C.byref(so), _ptr(xyz), _ptr(inl)))
        return self._solve_result(so, xyz, inl, n)

    def solve_wait(self, n):
        """Second half of solve(..., split="submit")."""
        so = SolveOutput()
        xyz = np.zeros((max(n, 1), 3), np.float32)
        inl = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.spvo_solve_wait(self.h, C.byref(so), _ptr(xyz), _ptr(inl)))
        return self._solve_result(so, xyz, inl, n)

    def solve_wait_prior(self, n, rvec_pred, tvec_pred, frame_count):
        """spvo_solve_wait_prior: the oldest pending solve, gated against the prior given NOW."""
        so = SolveOutput()
        xyz = np.zeros((max(n, 1), 3), np.float32)
        inl = np.zeros(max(n, 1), np.int32)
        r = np.ascontiguousarray(rvec_pred, np.float64).reshape(3)
        t = np.ascontiguousarray(tvec_pred, np.float64).reshape(3)
        self._check(self.lib.spvo_solve_wait_prior(self.h, _dptr(r), _dptr(t), int(frame_count), C.byref(so), _ptr(xyz), _ptr(inl)))
        return self._solve_result(so, xyz, inl, n)

    def solve_pending(self):
        return int(self.lib.spvo_solve_pending(self.h))

    @staticmethod
    def _solve_result(so, xyz, inl, n):
        return dict(q=np.array(so.q[:]), t=np.array(so.t[:]), rvec=np.array(so.rvec[:]), tvec=np.array(so.tvec[:]),
                    pnp_ok=bool(so.pnp_ok), accepted=bool(so.accepted), refined=bool(so.refined),
                    inliers=inl[:so.n_inliers].copy(), xyz=xyz[:n].copy(), iterations=so.summary.iterations,
                    converged=bool(so.summary.converged), final_cost=so.summary.final_cost)

    def stream(self) -> int:
        return self.lib.spvo_stream(self.h) or 0

    def synchronize(self):
        self._check(self.lib.spvo_synchronize(self.h))

    def profile_enable(self, on=True):
        self._check(self.lib.spvo_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self._check(self.lib.spvo_profile_reset(self.h))

    def profile_only(self, stage=None):
        """Time one stage only (e.g. "conv:1"); None = every stage."""
        self._check(self.lib.spvo_profile_only(self.h, stage.encode() if stage else None))

    def profile(self):
        out = {}
        n = self.lib.spvo_profile_count(self.h)
        for i in range(n):
            name = C.create_string_buffer(64)
            ms, fl, by = C.c_double(), C.c_double(), C.c_double()
            calls = C.c_longlong()
            self._check(self.lib.spvo_profile_get(self.h, i, name, 64, C.byref(ms), C.byref(calls), C.byref(fl), C.byref(by)))
            out[name.value.decode()] = dict(total_ms=ms.value, calls=calls.value, flops=fl.value, bytes=by.value)
        return out

    def stage_kernel(self, stage):
        """(kernel family, executed / algorithmic multiply-adds) of a "conv:<op index>" stage of the loaded engine."""
        name = C.create_string_buffer(64)
        f = C.c_double()
        self._check(self.lib.spvo_profile_stage_kernel(self.h, stage.encode(), name, 64, C.byref(f)))
        return name.value.decode(), f.value

    def stage_variant(self, stage):
        """Tile variant of a "conv:<op index>" stage of the loaded engine and the grid of its most recent launch: dict(ks, ck, wr, wc,
        pool, tiles, wgs), or None for a layer that runs no tile variant (Winograd, stem, merged sibling, fused block, fused heads)."""
        info = (C.c_int * 7)()
        self._check(self.lib.spvo_profile_stage_variant(self.h, stage.encode(), info))
        if info[0] == 0:
            return None
        return dict(ks=info[0], ck=info[1], wr=info[2], wc=info[3], pool=bool(info[4]), tiles=info[5], wgs=info[6])

    def stage_fused(self, stage):
        """What a fused launch last ran.  "conv:<pointwise op>": dict(G, STEM, POOL, EPI, co_tiles, tiles, wgs) of the INT8 block kernel's
        instance and grid; "heads": dict(kind = 1 fp32 / 2 fp16 / 3 int8 fused tail, tiles, wgs).  None where no fused launch ran (yet)."""
        info = (C.c_int * 8)()
        self._check(self.lib.spvo_profile_stage_fused(self.h, stage.encode(), info))
        if info[0] == 0:
            return None
        if stage == "heads":
            return dict(kind=info[1], tiles=info[6], wgs=info[7])
        return dict(G=info[1], STEM=info[2], POOL=info[3], EPI=info[4], co_tiles=info[5], tiles=info[6], wgs=info[7])


def set_tuning(name: str, value: int):
    """spvo_set_tuning: a diagnostic switch of the library (process-wide; contexts created / engines loaded afterwards).  The library
    reads no environment variable for these: tests and tools set them through this call."""
    rc = load().spvo_set_tuning(name.encode(), int(value))
    if rc:
        raise SpvoError(rc, f"unknown tuning name {name!r}")


def get_tuning(name: str, default: int) -> int:
    return load().spvo_get_tuning(name.encode(), int(default))


def clear_tuning():
    load().spvo_clear_tuning()


def tuning_from_env(prefix: str = "SPVO_TUNE_"):
    """tools/ only: SPVO_TUNE_<NAME>=<int> in the environment of a measurement script -> set_tuning (the script opts in by calling
    this; the library itself never looks)."""
    for k, v in os.environ.items():
        if k.startswith(prefix):
            set_tuning(k[len(prefix):].lower(), int(v))


COMM_ID_BYTES = 128


def comm_available() -> bool:
    """spvo_comm_available: librccl opens and has the entry points the library uses (no bootstrap state is created)"""
    return load().spvo_comm_available() == 0


def comm_unique_id() -> bytes:
    """rank 0: the RCCL id every rank passes to Comm.rccl (hand it over out of band)."""
    lib = load()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib.spvo_comm_unique_id(buf)
    if rc:
        raise SpvoError(rc, lib.spvo_last_error(None).decode())
    return buf.raw


class Comm:
    """spvo_comm: the pose all-gather of include/spvo.h (RCCL over xGMI; `host` = the file transport of the CPU tests)."""

    def __init__(self, handle, lib):
        self.h, self.lib = handle, lib
        self.rank, self.world = lib.spvo_comm_rank(handle), lib.spvo_comm_world(handle)

    @classmethod
    def rccl(cls, device: int, rank: int, world: int, unique_id: bytes) -> "Comm":
        lib = load()
        h = C.c_void_p()
        rc = lib.spvo_comm_create(device, rank, world, C.create_string_buffer(unique_id, COMM_ID_BYTES), C.byref(h))
        if rc:
            raise SpvoError(rc, lib.spvo_last_error(None).decode())
        return cls(h, lib)

    @classmethod
    def host(cls, directory: str, rank: int, world: int) -> "Comm":
        lib = load()
        h = C.c_void_p()
        rc = lib.spvo_comm_create_host(directory.encode(), rank, world, C.byref(h))
        if rc:
            raise SpvoError(rc, lib.spvo_last_error(None).decode())
        return cls(h, lib)

    def allgather(self, poses: np.ndarray) -> np.ndarray:
        """poses [n, 7] (or [7]) float64 -> [world, n, 7]"""
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        out = np.empty((self.world, len(p), 7), np.float64)
        rc = self.lib.spvo_pose_allgather_n(self.h, _dptr(p), len(p), _dptr(out))
        if rc:
            raise SpvoError(rc, self.lib.spvo_last_error(None).decode())
        return out

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.spvo_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def obs_array(X, uv, cam, inverse) -> np.ndarray:
    n = len(X)
    a = np.zeros(n, OBS_DTYPE)
    if n:
        a["X"] = np.asarray(X, np.float32).reshape(n, 3)
        a["uv"] = np.asarray(uv, np.float32).reshape(n, 2)
        a["cam"] = np.asarray(cam, np.int32)
        a["inverse"] = np.asarray(inverse, np.int32)
    return a


def akaze_tables(rows: int, cols: int):
    """The AKAZE detector's tables for a rows x cols image (spvo_akaze_tables; no context, no device), in the layout of
    tests/akaze_ref.py's make_tables: octave, esigma, sigma_size per level, nsteps per transition, tau (all step sizes), g0, g1."""
    lib = load()
    octave, esigma, sigma_size, nsteps = np.zeros(16, np.int32), np.zeros(16, np.float32), np.zeros(16, np.int32), np.zeros(15, np.int32)
    tau, g0, g1 = np.zeros(1024, np.float32), np.zeros(5, np.float32), np.zeros(3, np.float32)
    levels, n_tau = C.c_int(0), C.c_int(0)
    rc = lib.spvo_akaze_tables(int(rows), int(cols), C.byref(levels), _ptr(octave), _ptr(esigma), _ptr(sigma_size), _ptr(nsteps), _ptr(tau), len(tau), C.byref(n_tau), _ptr(g0), _ptr(g1))
    if rc or n_tau.value > len(tau):
        raise SpvoError(rc or -1, "spvo_akaze_tables failed")
    n = levels.value
    return dict(octave=octave[:n].copy(), esigma=esigma[:n].copy(), sigma_size=sigma_size[:n].copy(), nsteps=nsteps[:max(n - 1, 0)].copy(), tau=tau[:n_tau.value].copy(), g0=g0, g1=g1)


def brisk_tables(scales=range(64)):
    """The BRISK extractor's tables (spvo_brisk_tables; no context, no device): dict of points [64,1024,60,3] (x, y, sigma; the slices of
    `scales`, zeros elsewhere), short_pairs [512,2], long_pairs [870,4] (i, j, wdx, wdy), scale_list [64], size_list [64]."""
    lib = load()
    points = np.zeros((64, 1024, 60, 3), np.float32)
    short = np.zeros((512, 2), np.int32)
    long_ = np.zeros((870, 4), np.int32)
    scale_list = np.zeros(64, np.float32)
    size_list = np.zeros(64, np.int32)
    rc = lib.spvo_brisk_tables(0, None, _ptr(short), _ptr(long_), _ptr(scale_list), _ptr(size_list))
    for s in scales:
        rc = rc or lib.spvo_brisk_tables(int(s), points[s].ctypes.data, None, None, None, None)
    if rc:
        raise SpvoError(rc, (lib.spvo_last_error(None) or b"").decode())
    return dict(points=points, short_pairs=short, long_pairs=long_, scale_list=scale_list, size_list=size_list)
