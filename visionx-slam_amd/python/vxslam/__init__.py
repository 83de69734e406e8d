"""ctypes binding of libvxslam.so (include/vx_slam.h) for tests, smoke and bench.

There is no Python fallback: if the HIP library is missing or fails to load, every entry point
raises.  Names mirror the reference call surface: ``ORBExtractor.extract`` (FeatureExtractor::
Extract, core/feature/feature_extractor.h:15), ``ORBMatcher.match`` (FeatureMatcher::Match,
core/feature/feature_matcher.h:11-12) and ``LocalBA.optimize`` (LocalBA::Optimize,
core/backend/local_ba.h:23).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.environ.get("VX_LIB") or os.path.join(PKG_ROOT, "lib", "libvxslam.so")  # VX_LIB: trace build
HEADER_PATH = os.path.join(REPO_ROOT, "include", "vx_slam.h")

VX_OK, VX_ERR_INVALID, VX_ERR_HIP, VX_ERR_CAPACITY, VX_ERR_COMM, VX_ERR_STATE = 0, -1, -2, -3, -4, -5
MAX_SLOTS = 4
ORDER_STL, ORDER_RASTER = 0, 1  # vx_orb_set_order (include/vx_slam.h)
DEBUG_FAST_NO_BORDER, DEBUG_STAGES = 1, 2  # vx_orb_set_debug test hooks
CAND_DTYPE = np.dtype([("xy", "<u4"), ("score", "<i4"), ("harris", "<f4"), ("pad", "<i4")])

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("angle", "<f4"),
                           ("octave", "<i4")])
MATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])


class VxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"vx error {code}: {msg}")
        self.code = code


class OrbParams(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("fast_threshold", C.c_int32), ("edge_threshold", C.c_int32)]


class MapView(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kf_id", C.c_void_p), ("kf_pose", C.c_void_p),
                ("kf_intr", C.c_void_p), ("kf_has_cam", C.c_void_p), ("kf_feat_ptr", C.c_void_p),
                ("feat_uv", C.c_void_p), ("feat_lm_id", C.c_void_p), ("feat_flags", C.c_void_p),
                ("n_lm", C.c_int32), ("lm_id", C.c_void_p), ("lm_pos", C.c_void_p),
                ("lm_bad", C.c_void_p), ("lm_obs_ptr", C.c_void_p), ("obs_kf_id", C.c_void_p),
                ("obs_feat_idx", C.c_void_p)]


class BAOptions(C.Structure):
    _fields_ = [("window_size", C.c_int32), ("max_iterations", C.c_int32),
                ("min_pose_observations", C.c_int32), ("min_point_observations", C.c_int32),
                ("huber_delta", C.c_double), ("max_reproj_error", C.c_double)]


class BAStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("n_window_kf", C.c_int32), ("n_landmarks", C.c_int32),
                ("cost", C.c_double * 16), ("obs", C.c_int32 * 16), ("gate_margin", C.c_double),
                ("status", C.c_int32)]


class SBAOptions(C.Structure):
    _fields_ = [("window_size", C.c_int32), ("max_iterations", C.c_int32),
                ("min_point_observations", C.c_int32), ("fixed_keyframes", C.c_int32),
                ("huber_delta", C.c_double), ("max_reproj_error", C.c_double),
                ("lambda_init", C.c_double), ("rel_tol", C.c_double)]


class SBAStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("n_window_kf", C.c_int32),
                ("n_landmarks", C.c_int32), ("cost", C.c_double * 16), ("obs", C.c_int32 * 16),
                ("step", C.c_int32 * 16), ("lambda_", C.c_double), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("status", C.c_int32)]


EXPORTS = [
    "vx_version", "vx_create", "vx_destroy", "vx_host_alloc", "vx_host_free", "vx_last_error", "vx_stream", "vx_synchronize",
    "vx_stream_wait_ctx", "vx_event_create", "vx_event_record", "vx_event_wait", "vx_event_destroy",
    "vx_orb_default_params", "vx_orb_pattern", "vx_orb_extract", "vx_orb_extract_async",
    "vx_orb_fetch", "vx_orb_slot_device", "vx_match_knn2_ratio", "vx_match_slots_async",
    "vx_match_device_async", "vx_match_fetch", "vx_ba_default_options", "vx_ba_optimize_map", "vx_ba_plan_create",
    "vx_ba_plan_run_async", "vx_ba_plan_fetch", "vx_ba_plan_destroy", "vx_ba_plan_info", "vx_ba_plan_layout", "vx_ba_plan_persistent", "vx_ba_plan_fused_tables",
    "vx_ba_plan_inspect", "vx_ba_shard_of", "vx_comm_unique_id", "vx_comm_init", "vx_comm_info", "vx_prof_enable", "vx_prof_count", "vx_prof_name",
    "vx_prof_read", "vx_sba_default_options", "vx_sba_plan_create", "vx_sba_plan_run_async",
    "vx_sba_plan_fetch", "vx_sba_plan_destroy", "vx_sba_plan_info", "vx_sba_plan_system", "vx_sba_plan_step",
    "vx_sba_optimize_map", "vx_depth_landmarks", "vx_triangulate", "vx_graph_enable", "vx_graph_counts", "vx_create_ex", "vx_device_cus", "vx_ba_plan_create_ex",
    "vx_dmap_create", "vx_dmap_add_keyframe", "vx_dmap_add_landmarks", "vx_dmap_add_observations",
    "vx_dmap_remove_observations", "vx_dmap_remove_keyframe", "vx_dmap_remove_landmarks", "vx_dmap_set_features",
    "vx_dmap_set_landmark_bad", "vx_dmap_set_poses", "vx_dmap_counts", "vx_dmap_live_counts", "vx_dmap_download",
    "vx_ba_plan_create_dmap", "vx_ba_plan_apply_dmap", "vx_ba_shard_emulate_run", "vx_ba_optimize_dmap",
    "vx_ba_dmap_results", "vx_ba_dmap_results_view", "vx_dmap_prefetch_results", "vx_sba_plan_factor_work", "vx_sba_plan_create_dmap", "vx_sba_plan_rebuild_dmap", "vx_sba_shard_emulate_run", "vx_sba_plan_apply_dmap", "vx_seq_create", "vx_seq_destroy", "vx_seq_wait", "vx_seq_record", "vx_seq_extract",
    "vx_seq_match", "vx_seq_ba_run", "vx_seq_length", "vx_seq_run", "vx_seq_set_threads",
    "vx_orb_extract_batch_async", "vx_orb_batch_fetch", "vx_orb_batch_device", "vx_match_batch_async",
    "vx_match_batch_fetch", "vx_orb_extract_batch", "vx_match_knn2_ratio_batch", "vx_orb_set_order",
    "vx_orb_get_order", "vx_orb_set_debug", "vx_orb_debug_read", "vx_test_retain_best",
    "vx_track_default_options", "vx_orb_slot_keypoints", "vx_track_pnp_async", "vx_track_pnp_fetch", "vx_track_block", "vx_track_pnp_host_async",
    "vx_cull_default_options", "vx_dmap_cull_landmarks", "vx_dmap_keyframe_redundancy", "vx_dmap_cull_keyframes",
    "vx_dmap_cull_results", "vx_cull_block", "vx_cull_lds_keyframes",
    "vx_keyframe_default_options", "vx_dmap_create_keyframe", "vx_dmap_create_keyframe_host", "vx_dmap_create_results",
    "vx_dmap_keyframe_features", "vx_keyframe_block", "vx_prof_enable64",
    "vx_track_essential_default_options", "vx_track_essential_async", "vx_track_essential_host_async",
    "vx_track_essential_fetch",
    "vx_init_gate_default_options", "vx_init_gate_async", "vx_init_gate_host_async", "vx_init_gate_fetch",
    "vx_frame_create", "vx_frame_destroy", "vx_frame_capture_async", "vx_frame_extract_host_async",
    "vx_frame_upload_async", "vx_frame_device", "vx_frame_fetch", "vx_frame_fetch_ex",
    "vx_track_frame_async", "vx_track_frame_fetch", "vx_track_frame_pairs", "vx_track_frame_matches",
    "vx_dmap_create_keyframe_frame",
    "vx_frame_capture_batch_async", "vx_track_rig_async", "vx_track_rig_fetch", "vx_track_rig_pairs",
    "vx_track_rig_keypoints", "vx_track_rig_matches", "vx_track_rig_layout", "vx_track_rig_block",
    "vx_dmap_create_keyframes_rig",
    "vx_relocalize_async", "vx_relocalize_fetch", "vx_relocalize_matches", "vx_relocalize_table_limit",
]

DEPTH_TYPES = {np.dtype(np.uint16): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}

_lib = None


def build():
    subprocess.run(["make", "-s", "-C", PKG_ROOT, "-j8"], check=True)


def lib():
    """Load libvxslam.so (fails loudly: there is no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} missing: run __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        L.vx_last_error.restype = C.c_char_p
        L.vx_last_error.argtypes = [C.c_void_p]
        L.vx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.vx_destroy.argtypes = [C.c_void_p]
        L.vx_host_alloc.restype = C.c_void_p
        L.vx_host_alloc.argtypes = [C.c_size_t]
        L.vx_host_free.argtypes = [C.c_void_p]
        L.vx_stream.restype = C.c_void_p
        L.vx_stream.argtypes = [C.c_void_p]
        L.vx_synchronize.argtypes = [C.c_void_p]
        L.vx_set_grid_share.argtypes = [C.c_void_p, C.c_float]
        L.vx_orb_set_order.argtypes = [C.c_void_p, C.c_int]
        L.vx_orb_get_order.argtypes = [C.c_void_p]
        L.vx_orb_set_debug.argtypes = [C.c_void_p, C.c_int]
        L.vx_orb_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.vx_test_retain_best.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.POINTER(C.c_int)]
        L.vx_stream_wait_ctx.argtypes = [C.c_void_p, C.c_void_p]
        L.vx_event_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.vx_event_record.argtypes = [C.c_void_p, C.c_void_p]
        L.vx_event_wait.argtypes = [C.c_void_p, C.c_void_p]
        L.vx_event_destroy.argtypes = [C.c_void_p]
        L.vx_event_destroy.restype = None
        L.vx_orb_slot_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int32)]
        L.vx_match_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_float]
        L.vx_orb_extract_batch_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                                 C.c_int, C.c_int, C.c_int64, C.c_int]
        L.vx_orb_extract_batch.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int64, C.c_int]
        L.vx_orb_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
        L.vx_orb_batch_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_int)]
        L.vx_match_batch_async.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                           C.c_float]
        L.vx_match_batch_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.vx_match_knn2_ratio_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p,
                                                C.POINTER(C.c_void_p), C.c_void_p, C.c_float]
        L.vx_prof_name.restype = C.c_char_p
        L.vx_ba_plan_destroy.argtypes = [C.c_void_p]
        L.vx_dmap_destroy.argtypes = [C.c_void_p]
        L.vx_dmap_destroy.restype = None
        L.vx_ba_plan_destroy.restype = None
        L.vx_orb_default_params.restype = None
        L.vx_ba_default_options.restype = None
        L.vx_sba_plan_destroy.argtypes = [C.c_void_p]
        L.vx_sba_plan_destroy.restype = None
        L.vx_sba_default_options.restype = None
        L.vx_pnp_default_options.restype = None
        L.vx_essential_default_options.restype = None
        L.vx_seq_destroy.argtypes = [C.c_void_p]
        L.vx_seq_destroy.restype = None
        for f in ("vx_seq_wait", "vx_seq_record"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.vx_seq_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int64, C.c_int]
        L.vx_seq_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_float]
        L.vx_seq_ba_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.vx_seq_length.argtypes = [C.c_void_p]
        L.vx_seq_run.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.vx_seq_set_threads.argtypes = [C.c_void_p, C.c_int]
        L.vx_track_default_options.restype = None
        L.vx_track_default_options.argtypes = [C.c_void_p]
        L.vx_orb_slot_keypoints.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.vx_track_pnp_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.vx_track_pnp_host_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.vx_track_pnp_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.vx_track_essential_default_options.restype = None
        L.vx_track_essential_default_options.argtypes = [C.c_void_p]
        L.vx_track_essential_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.vx_track_essential_host_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vx_track_essential_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.vx_init_gate_default_options.restype = None
        L.vx_init_gate_default_options.argtypes = [C.c_void_p]
        L.vx_init_gate_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        L.vx_init_gate_host_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                              C.c_int64, C.c_int, C.c_void_p]
        L.vx_init_gate_fetch.argtypes = [C.c_void_p, C.c_void_p]
        L.vx_frame_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.vx_frame_destroy.argtypes = [C.c_void_p]
        L.vx_frame_destroy.restype = None
        L.vx_frame_capture_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.vx_frame_extract_host_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_int, C.c_int64]
        L.vx_frame_upload_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.vx_frame_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
        L.vx_frame_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.vx_frame_fetch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]
        L.vx_track_frame_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vx_track_frame_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.vx_track_frame_pairs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.vx_track_frame_matches.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_int32)]
        L.vx_frame_capture_batch_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vx_track_rig_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.vx_track_rig_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.vx_track_rig_pairs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.vx_track_rig_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.vx_track_rig_matches.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_int32)]
        L.vx_track_rig_layout.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.vx_track_rig_block.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int]
        L.vx_relocalize_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                          C.c_void_p]
        L.vx_relocalize_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.vx_relocalize_matches.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_int32)]
        L.vx_relocalize_table_limit.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.vx_cull_default_options.restype = None
        L.vx_cull_default_options.argtypes = [C.c_void_p]
        L.vx_dmap_cull_landmarks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.vx_dmap_keyframe_redundancy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.POINTER(C.c_int)]
        L.vx_dmap_cull_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                             C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.vx_dmap_cull_results.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int),
                                           C.POINTER(C.c_int)]
        L.vx_prof_enable64.argtypes = [C.c_void_p, C.c_uint64]
        L.vx_keyframe_default_options.restype = None
        L.vx_keyframe_default_options.argtypes = [C.c_void_p]
        L.vx_dmap_create_keyframe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                              C.c_uint64, C.c_void_p, C.c_void_p]
        L.vx_dmap_create_keyframe_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_int,
                                                   C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_uint64,
                                                   C.c_void_p, C.c_void_p]
        L.vx_dmap_create_results.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.vx_dmap_keyframe_features.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_int)]
        L.vx_dmap_create_keyframes_rig.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                                   C.c_void_p]
        L.vx_ba_shard_of.restype = C.c_uint32
        L.vx_ba_shard_of.argtypes = [C.c_uint64, C.c_int]
        _lib = L
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


# vx_pnp_options / vx_pnp_result (include/vx_slam.h) as numpy records
PNP_OPTIONS_DTYPE = np.dtype([("max_iterations", "<i4"), ("refine_iterations", "<i4"), ("reproj_error", "<f8"),
                              ("confidence", "<f8"), ("seed", "<u8")])
PNP_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("n_inliers", "<i4"), ("best_hypothesis", "<i4"),
                             ("hypotheses_run", "<i4"), ("refine_iterations", "<i4"), ("reserved", "<i4"),
                             ("rvec", "<f8", 3), ("tvec", "<f8", 3), ("pose", "<f8", 7), ("cost0", "<f8"),
                             ("cost", "<f8")])


EM_OPTIONS_DTYPE = np.dtype([("max_iterations", "<i4"), ("reserved", "<i4"), ("threshold", "<f8"),
                             ("confidence", "<f8"), ("distance_thresh", "<f8"), ("seed", "<u8")])
EM_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("n_inliers", "<i4"), ("n_ransac_inliers", "<i4"),
                            ("best_hypothesis", "<i4"), ("best_model", "<i4"), ("hypotheses_run", "<i4"),
                            ("pose_candidate", "<i4"), ("reserved", "<i4"), ("E", "<f8", 9), ("R", "<f8", 9),
                            ("t", "<f8", 3)])


def essential_options(max_iterations=None, threshold=None, confidence=None, distance_thresh=None, seed=None):
    """findEssentialMat(.., RANSAC, 0.999, 1.0, mask) + recoverPose (tracking.cpp:521-528) defaults,
    any field overridable."""
    o = np.zeros((), EM_OPTIONS_DTYPE)
    lib().vx_essential_default_options(_p(o))
    for k, v in (("max_iterations", max_iterations), ("threshold", threshold), ("confidence", confidence),
                 ("distance_thresh", distance_thresh), ("seed", seed)):
        if v is not None:
            o[k] = v
    return o


def pnp_options(n, max_iterations=None, reproj_error=2.0, confidence=0.99, seed=0x5EED, refine_iterations=20):
    """solvePnPRansac's arguments in Tracking::TrackWithPnP (tracking.cpp:420-423) for n pairs."""
    o = np.zeros((), PNP_OPTIONS_DTYPE)
    lib().vx_pnp_default_options(int(n), _p(o))
    if max_iterations is not None:
        o["max_iterations"] = max_iterations
    o["refine_iterations"] = refine_iterations
    o["reproj_error"] = reproj_error
    o["confidence"] = confidence
    o["seed"] = seed
    return o


# vx_track_options / vx_track_result (include/vx_slam.h; sizes pinned in csrc/track.hip)
TRACK_OPTIONS_DTYPE = np.dtype([("min_matches", "<i4"), ("min_inliers", "<i4"), ("pnp", PNP_OPTIONS_DTYPE)])
TRACK_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_matches", "<i4"), ("n_good_matches", "<i4"), ("n_pairs", "<i4"),
                               ("n_bad_index", "<i4"), ("min_distance", "<f4"), ("parallax", "<f8"),
                               ("pnp", PNP_RESULT_DTYPE)])
TRACK_OK, TRACK_FEW_MATCHES, TRACK_FEW_PAIRS, TRACK_PNP_FAILED, TRACK_BAD_ROTATION = range(5)


def track_options(min_matches=None, min_inliers=None, max_iterations=None, reproj_error=None, confidence=None,
                  seed=None, refine_iterations=None):
    """Tracking::Options + solvePnPRansac's arguments in Tracking::TrackWithPnP (tracking.h:27-29,
    tracking.cpp:420-423); max_iterations -1 (the default) = min(100, 2 * pairs), resolved on the device."""
    o = np.zeros((), TRACK_OPTIONS_DTYPE)
    lib().vx_track_default_options(_p(o))
    for k, v in (("min_matches", min_matches), ("min_inliers", min_inliers)):
        if v is not None:
            o[k] = v
    for k, v in (("max_iterations", max_iterations), ("reproj_error", reproj_error), ("confidence", confidence),
                 ("seed", seed), ("refine_iterations", refine_iterations)):
        if v is not None:
            o["pnp"][k] = v
    return o


# vx_track_essential_options / vx_track_essential_result (include/vx_slam.h; sizes pinned in csrc/track_ess.hip)
TRACK_ESS_OPTIONS_DTYPE = np.dtype([("min_matches", "<i4"), ("min_inliers", "<i4"), ("ess", EM_OPTIONS_DTYPE)])
TRACK_ESS_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_matches", "<i4"), ("n_good_matches", "<i4"), ("n_pairs", "<i4"),
                                   ("n_bad_index", "<i4"), ("min_distance", "<f4"), ("parallax", "<f8"),
                                   ("pose", "<f8", 7), ("ess", EM_RESULT_DTYPE)])
TRACK_ESSENTIAL_FAILED = 5


def track_essential_options(min_matches=None, min_inliers=None, max_iterations=None, threshold=None, confidence=None,
                            distance_thresh=None, seed=None):
    """Tracking::Options' gates + findEssentialMat / recoverPose's arguments in Tracking::TrackLastFrame
    (tracking.h:27-28, tracking.cpp:521-528), any field overridable."""
    o = np.zeros((), TRACK_ESS_OPTIONS_DTYPE)
    lib().vx_track_essential_default_options(_p(o))
    for k, v in (("min_matches", min_matches), ("min_inliers", min_inliers)):
        if v is not None:
            o[k] = v
    for k, v in (("max_iterations", max_iterations), ("threshold", threshold), ("confidence", confidence),
                 ("distance_thresh", distance_thresh), ("seed", seed)):
        if v is not None:
            o["ess"][k] = v
    return o


# vx_track_frame_result (include/vx_slam.h; layout pinned in csrc/track_frame.hip)
TRACK_FRAME_RESULT_DTYPE = np.dtype([("path", "<i4"), ("status", "<i4"), ("n_inliers", "<i4"), ("n_keypoints", "<i4"),
                                     ("parallax", "<f8"), ("pose", "<f8", 7), ("pnp_ran", "<i4"), ("ess_ran", "<i4"),
                                     ("pnp", TRACK_RESULT_DTYPE), ("ess", TRACK_ESS_RESULT_DTYPE)])
TRACK_PATH_NONE, TRACK_PATH_PNP, TRACK_PATH_ESSENTIAL = range(3)


MAX_RIG_CAMERAS = 16  # VX_MAX_RIG_CAMERAS

# vx_rig_camera (include/vx_slam.h): one camera of Context.track_rig_async
RIG_CAMERA_DTYPE = np.dtype([("last_kf_id", "<u8"), ("last_kf", "<u8"), ("last", "<u8"), ("curr", "<u8"),
                             ("pose_last7", "<u8"), ("intr4", "<u8")])


def rig_camera(curr, intr, last_kf_id=0, last_kf=None, last=None, pose_last=None):
    """one camera of Context.track_rig_async: Frame handles (last_kf: the frame holding keyframe
    last_kf_id's features, None: no last keyframe; last: None: the fallback fails), its intrinsics and
    T_lw of `last` (None: identity)"""
    return {"last_kf_id": int(last_kf_id), "last_kf": last_kf, "last": last, "curr": curr, "intr": intr,
            "pose_last": pose_last}


MAX_RELOC_CANDIDATES = 16  # VX_MAX_RELOC_CANDIDATES

# vx_reloc_candidate / vx_reloc_candidate_result / vx_reloc_result (include/vx_slam.h; sizes pinned in csrc/reloc.hip)
RELOC_CANDIDATE_DTYPE = np.dtype([("kf_id", "<u8"), ("frame", "<u8")])
RELOC_CANDIDATE_RESULT_DTYPE = np.dtype([("n_matches", "<i4"), ("n_good_matches", "<i4"), ("n_pairs", "<i4"),
                                         ("n_bad_index", "<i4"), ("open", "<i4"), ("n_kept", "<i4"), ("n_inliers", "<i4"),
                                         ("min_distance", "<f4"), ("parallax", "<f8")])
RELOC_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_cand", "<i4"), ("n_pool", "<i4"), ("best_cand", "<i4"),
                               ("parallax", "<f8"), ("pnp", PNP_RESULT_DTYPE),
                               ("cand", RELOC_CANDIDATE_RESULT_DTYPE, MAX_RELOC_CANDIDATES)])


def track_rig_layout(cap_pairs0, cap_pairs1, cap_kp):
    """(cam_offset int64[n], total_bytes) of vx_track_rig_fetch's packed block for these per-camera pair
    capacities of the two paths and keypoint capacities (vx_track_rig_layout: no context, no device)"""
    a, b, k = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (cap_pairs0, cap_pairs1, cap_kp))
    if not (len(a) == len(b) == len(k)):
        raise ValueError("track_rig_layout: one capacity of each kind per camera")
    off = np.zeros(max(len(a), 1), np.int64)
    total = C.c_int64(0)
    rc = lib().vx_track_rig_layout(len(a), _p(a), _p(b), _p(k), _p(off), C.byref(total))
    if rc != VX_OK:
        raise VxError(rc, f"vx_track_rig_layout: {len(a)} cameras / a negative capacity")
    return off[:len(a)].copy(), int(total.value)


def track_frame_block(cap_pairs0, cap_pairs1, cap_kp):
    """Offsets inside one camera's packed block (trk::FrameBlock, csrc/track_bodies.hpp): (pair_match0, mask0,
    pair_match1, mask1, keypoint rows, bytes) for the two paths' pair capacities and the keypoint capacity;
    every part begins on a 16-byte boundary"""
    a16 = lambda x: (int(x) + 15) & ~15
    o_pm0 = a16(TRACK_FRAME_RESULT_DTYPE.itemsize)
    o_m0 = o_pm0 + a16(cap_pairs0 * 4)
    o_pm1 = o_m0 + a16(cap_pairs0)
    o_m1 = o_pm1 + a16(cap_pairs1 * 4)
    o_kp = o_m1 + a16(cap_pairs1)
    return o_pm0, o_m0, o_pm1, o_m1, o_kp, o_kp + a16(cap_kp * KEYPOINT_DTYPE.itemsize)


def track_frame_options(min_matches=None, min_inliers=None, pnp=None, ess=None):
    """(TRACK_OPTIONS_DTYPE, TRACK_ESS_OPTIONS_DTYPE) for Context.track_frame_async: Tracking::Options'
    two gates (tracking.h:27-28) on both paths; pnp / ess: dicts of track_options /
    track_essential_options keywords for the rest."""
    return (track_options(min_matches, min_inliers, **(pnp or {})),
            track_essential_options(min_matches, min_inliers, **(ess or {})))


# vx_init_gate_options / vx_init_gate_result (include/vx_slam.h; sizes pinned in csrc/init_gate.hip)
INIT_GATE_OPTIONS_DTYPE = np.dtype([("min_features", "<i4"), ("grid_cols", "<i4"), ("grid_rows", "<i4"), ("pad", "<i4"),
                                    ("min_grid_frac", "<f8"), ("min_mean", "<f8"), ("max_mean", "<f8"),
                                    ("min_stddev", "<f8")])
INIT_GATE_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_features", "<i4"), ("valid_grids", "<i4"), ("grid_mask", "<u4"),
                                   ("n_pixels", "<i8"), ("sum", "<u8"), ("sum_sq", "<u8"), ("mean", "<f8"),
                                   ("stddev", "<f8")])
INIT_OK, INIT_FEW_FEATURES, INIT_POOR_DISTRIBUTION, INIT_POOR_IMAGE = range(4)


def init_gate_options(**fields):
    """Tracking::InitWithFirstFrame's constants (tracking.h:27, tracking.cpp:96-97, :117, :129-135), any field
    overridable: min_features, grid_cols, grid_rows, min_grid_frac, min_mean, max_mean, min_stddev."""
    o = np.zeros((), INIT_GATE_OPTIONS_DTYPE)
    lib().vx_init_gate_default_options(_p(o))
    for k, v in fields.items():
        o[k] = v
    return o


# vx_cull_options / vx_cull_landmark / vx_cull_feature (include/vx_slam.h; sizes pinned in csrc/cull.hip)
CULL_OPTIONS_DTYPE = np.dtype([("min_landmark_observations", "<i4"), ("min_landmarks_for_culling", "<i4"),
                               ("min_keyframes_for_culling", "<i4"), ("max_keyframes", "<i4"),
                               ("kf_min_shared_observations", "<i4"), ("reserved", "<i4"),
                               ("kf_redundant_ratio", "<f8"), ("landmark_max_reproj_error", "<f8")])
CULL_LANDMARK_DTYPE = np.dtype([("lm_id", "<u8"), ("row", "<i4"), ("reason", "<i4"), ("n_projected", "<i4"),
                                ("reserved", "<i4"), ("mean_err", "<f8")])
CULL_FEATURE_DTYPE = np.dtype([("kf_id", "<u8"), ("kf_row", "<i4"), ("feat_idx", "<i4")])
CULL_ALREADY_BAD, CULL_FEW_OBSERVATIONS, CULL_NO_PROJECTION, CULL_LARGE_ERROR, CULL_MEAN_ERROR = range(1, 6)


def cull_options(**fields):
    """Tracking::Options' map-culling fields (tracking.h:33-40) with the reference's defaults, any of
    them overridable by name."""
    o = np.zeros((), CULL_OPTIONS_DTYPE)
    lib().vx_cull_default_options(_p(o))
    for k, v in fields.items():
        if k not in CULL_OPTIONS_DTYPE.names or k == "reserved":
            raise TypeError(f"cull_options: unknown field {k!r}")
        o[k] = v
    return o


def cull_block() -> int:
    """landmark rows of one scan workgroup (the unit of the culled lists' ordered compaction)"""
    return int(lib().vx_cull_block())


def cull_lds_keyframes() -> int:
    """live keyframes up to which the landmark scan holds its keyframe table in LDS"""
    return int(lib().vx_cull_lds_keyframes())


# vx_keyframe_options / vx_keyframe_result / vx_keyframe_landmark (include/vx_slam.h; sizes pinned in csrc/keyframe.hip)
KEYFRAME_OPTIONS_DTYPE = np.dtype([("tri_min_angle_deg", "<f8"), ("tri_max_reproj_error", "<f8")])
KEYFRAME_RESULT_DTYPE = np.dtype([("n_feat", "<i4"), ("n_depth", "<i4"), ("n_triangulated", "<i4"), ("n_matches", "<i4"),
                                  ("first_landmark_id", "<u8"), ("next_landmark_id", "<u8"), ("error_bits", "<i4"),
                                  ("reserved", "<i4")])
KEYFRAME_LANDMARK_DTYPE = np.dtype([("lm_id", "<u8"), ("row", "<i4"), ("kind", "<i4"), ("feat_curr", "<i4"),
                                    ("feat_last", "<i4"), ("pw", "<f8", 3)])
KF_ERR_MATCH_RANGE, KF_ERR_DUP_QUERY, KF_ERR_KF_LIVE, KF_ERR_NO_LAST, KF_ERR_NO_CAMERA, KF_ERR_ID_RANGE = 1, 2, 4, 8, 16, 32
KF_ERR_RIG_REPEAT = 64
# vx_rig_keyframe (include/vx_slam.h; size pinned in csrc/keyframe_rig.hip): one camera of DMap.create_keyframes_rig
RIG_KEYFRAME_DTYPE = np.dtype({"names": ["kf_id", "pose7", "intr4", "curr", "has_last", "last_kf_id", "d_matches",
                                         "d_n_matches", "cap_matches", "depth", "depth_type", "rows", "cols",
                                         "row_stride"],
                               "formats": ["<u8", "<u8", "<u8", "<u8", "<i4", "<u8", "<u8", "<u8", "<i4", "<u8", "<i4",
                                           "<i4", "<i4", "<i8"],
                               "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88, 96], "itemsize": 104})


def keyframe_options(**fields):
    """Tracking::Options' triangulation fields (tracking.h:43-44) with the reference's defaults, either
    overridable by name."""
    o = np.zeros((), KEYFRAME_OPTIONS_DTYPE)
    lib().vx_keyframe_default_options(_p(o))
    for k, v in fields.items():
        if k not in KEYFRAME_OPTIONS_DTYPE.names:
            raise TypeError(f"keyframe_options: unknown field {k!r}")
        o[k] = v
    return o


def keyframe_block() -> int:
    """threads of the keyframe commit workgroup (the chunk of its two ordered compactions)"""
    return int(lib().vx_keyframe_block())


def track_block() -> int:
    """threads of the pair-gather workgroup (the chunk of its two compactions)"""
    return int(lib().vx_track_block())


def default_orb_params(n_features=1000, scale_factor=1.2, n_levels=8, fast_threshold=20,
                       edge_threshold=31):
    return OrbParams(n_features, scale_factor, n_levels, fast_threshold, edge_threshold)


def default_ba_options(window=5, iters=5, min_pose=20, min_point=2, huber=5.0, max_err=5.0):
    return BAOptions(window, iters, min_pose, min_point, huber, max_err)


def default_sba_options(window=5, iters=10, min_point=2, fixed=2, huber=5.0, max_err=5.0, lam=1e-4,
                        rel_tol=1e-6):
    return SBAOptions(window, iters, min_point, fixed, huber, max_err, lam, rel_tol)


def map_view(m) -> MapView:
    """MapView over the arrays of a synth.BAMap (kf_pose / lm_pos are written in place)."""
    v = MapView()
    for name, _ in MapView._fields_:
        if name == "n_kf":
            v.n_kf = int(m["kf_id"].shape[0])
        elif name == "n_lm":
            v.n_lm = int(m["lm_id"].shape[0])
        else:
            a = m[name]
            assert a.flags["C_CONTIGUOUS"], name
            setattr(v, name, a.ctypes.data)
    return v


def pattern() -> np.ndarray:
    out = np.zeros(1024, np.int32)
    rc = lib().vx_orb_pattern(_p(out))
    assert rc == 0
    return out


def ba_plan_inspect(m, opts=None, ref_kf_id=None, shard_rank=0, shard_count=1) -> dict:
    """Host-only dry run of vx_ba_plan_create (no device needed)."""
    opts = opts or default_ba_options(window=m.get("window", 5))
    ref = m.get("ref_kf_id") if ref_kf_id is None else ref_kf_id
    v = map_view(m)
    out = np.zeros(8, np.int64)
    lm = np.zeros(max(int(m["lm_id"].shape[0]), 1), np.int32)
    kf = np.zeros(max(int(m["kf_id"].shape[0]), 1), np.int32)
    rc = lib().vx_ba_plan_inspect(C.byref(v), C.c_uint64(0 if ref is None else int(ref)), 0 if ref is None else 1,
                                  C.byref(opts), shard_rank, shard_count, _p(out), _p(lm), len(lm), _p(kf), len(kf))
    if rc != VX_OK:
        raise VxError(rc, "vx_ba_plan_inspect failed")
    keys = ["status", "n_window_kf", "n_landmarks", "n_kf", "n_opt", "n_lm", "n_pose_obs", "n_lm_obs"]
    d = {k: int(x) for k, x in zip(keys, out)}
    d["lm_map_idx"] = lm[:d["n_lm"]].copy()
    d["kf_map_idx"] = kf[:d["n_kf"]].copy()
    return d


def ba_shard_of(lm_id: int, shard_count: int) -> int:
    return int(lib().vx_ba_shard_of(C.c_uint64(int(lm_id)), int(shard_count)))


class Event:
    """A device event (vx_event) for cross-context ordering."""

    def __init__(self, ctx: "Context"):
        self._h = C.c_void_p()
        ctx._check(lib().vx_event_create(ctx.handle, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().vx_event_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One vx_ctx = one device + one HIP stream (not thread-safe, like the reference's tracking
    thread owning the hot path, core/system/system.cpp:39-52)."""

    def __init__(self, device: int = 0, priority: int = 0, cu_mask=None):
        """cu_mask: iterable of compute-unit indices this context may use (None: all)."""
        self._h = C.c_void_p()
        self.device = int(device)
        words, nw = None, 0
        if cu_mask is not None:
            n = lib().vx_device_cus(int(device))
            nw = (n + 31) // 32
            words = (C.c_uint32 * nw)()
            for i in cu_mask:
                words[i // 32] |= 1 << (i % 32)
        rc = lib().vx_create_ex(int(device), int(priority), words, nw, C.byref(self._h))
        if rc != VX_OK:
            raise VxError(rc, f"vx_create(device={device}) failed")

    def close(self):
        if self._h:
            lib().vx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != VX_OK:
            raise VxError(rc, lib().vx_last_error(self._h).decode())
        return rc

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return lib().vx_stream(self._h)

    def synchronize(self):
        self._check(lib().vx_synchronize(self._h))

    def wait_for(self, other: "Context"):
        """Order later work on this context after everything enqueued on `other` (device-side)."""
        self._check(lib().vx_stream_wait_ctx(self._h, other._h))

    # ---------------------------------------------------------------- ORB
    def orb_extract(self, img: np.ndarray, params: OrbParams | None = None, cap: int | None = None):
        img = np.ascontiguousarray(img)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        params = params or default_orb_params()
        cap = cap or (2 * params.n_features + 256)
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        self._check(lib().vx_orb_extract(self._h, C.byref(params), _p(img), w, h, ch,
                                         C.c_int64(img.strides[0]), _p(kps), _p(desc), cap,
                                         C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def orb_extract_async(self, d_img_ptr: int, w: int, h: int, channels: int, row_stride: int,
                          slot: int, params: OrbParams | None = None):
        params = params or default_orb_params()
        self._check(lib().vx_orb_extract_async(self._h, C.byref(params), C.c_void_p(d_img_ptr), w, h,
                                               channels, C.c_int64(row_stride), slot))

    def orb_fetch(self, slot: int, cap: int = 8192):
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        self._check(lib().vx_orb_fetch(self._h, slot, _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def orb_extract_batch_async(self, d_imgs_ptr: int, n_frames: int, frame_stride: int, w: int, h: int,
                                channels: int, row_stride: int, bank: int = 0, params: OrbParams | None = None):
        """Extract n_frames device-resident images (frame f at d_imgs_ptr + f * frame_stride) in one
        launch per kernel; results stay in batch bank `bank`."""
        params = params or default_orb_params()
        self._check(lib().vx_orb_extract_batch_async(self._h, C.byref(params), C.c_void_p(d_imgs_ptr), n_frames,
                                                     C.c_int64(frame_stride), w, h, channels, C.c_int64(row_stride),
                                                     bank))

    def orb_batch_fetch(self, bank: int, frame: int, cap: int = 8192):
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        self._check(lib().vx_orb_batch_fetch(self._h, bank, frame, _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def batch_device(self, bank: int, frame: int):
        """(device descriptor pointer, device count pointer, row capacity) of a batch frame."""
        d, n, cap = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._check(lib().vx_orb_batch_device(self._h, bank, frame, C.byref(d), C.byref(n), C.byref(cap)))
        return d.value, n.value, cap.value

    def orb_extract_batch(self, imgs: np.ndarray, params: OrbParams | None = None, bank: int = 0):
        """Host convenience over vx_orb_extract_batch (host frames, uploaded by the library): a
        (B, H, W[, C]) stack extracted as one batch; returns a list of (keypoints, descriptors) per
        frame."""
        imgs = np.ascontiguousarray(imgs)
        b, h, w = imgs.shape[:3]
        ch = 1 if imgs.ndim == 3 else imgs.shape[3]
        params = params or default_orb_params()
        ptrs = (C.c_void_p * b)(*[C.c_void_p(imgs[f].ctypes.data) for f in range(b)])
        self._check(lib().vx_orb_extract_batch(self._h, C.byref(params), ptrs, b, w, h, ch, C.c_int64(imgs.strides[1]),
                                               bank))
        return [self.orb_batch_fetch(bank, f) for f in range(b)]

    # ---------------------------------------------------------------- matching
    def match(self, q: np.ndarray, t: np.ndarray, ratio: float = 0.8):
        q = np.ascontiguousarray(q, np.uint8)
        t = np.ascontiguousarray(t, np.uint8)
        cap = max(len(q), 1)
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_int(0)
        self._check(lib().vx_match_knn2_ratio(self._h, _p(q), len(q), _p(t), len(t),
                                              C.c_float(ratio), _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def match_slots_async(self, q_slot: int, t_slot: int, ratio: float = 0.8):
        self._check(lib().vx_match_slots_async(self._h, q_slot, t_slot, C.c_float(ratio)))

    def slot_device(self, slot: int):
        """(device descriptor pointer, device count pointer, row capacity) of an extraction slot."""
        d, n, cap = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._check(lib().vx_orb_slot_device(self._h, slot, C.byref(d), C.byref(n), C.byref(cap)))
        return d.value, n.value, cap.value

    def slot_keypoints(self, slot: int) -> int:
        """device pointer of an extraction slot's KEYPOINT_DTYPE rows (their count: slot_device()[1])"""
        d = C.c_void_p()
        self._check(lib().vx_orb_slot_keypoints(self._h, slot, C.byref(d)))
        return d.value

    def track_pnp_async(self, dmap: "DMap", last_kf_id: int, curr, intr, opts=None, matches=None):
        """Tracking::TrackWithPnP after the match (tracking.cpp:342-423, :449) on the device.  curr: an
        extraction slot of this context, or (device pointer of the first x, row stride in bytes,
        device pointer of the int32 row count); matches: None = this context's last match_*_async
        result, or (device pointer of MATCH_DTYPE rows, device pointer of the int32 count, capacity).
        Nothing synchronises; track_pnp_fetch() completes it."""
        if isinstance(curr, (int, np.integer)):
            curr = (self.slot_keypoints(int(curr)), KEYPOINT_DTYPE.itemsize, self.slot_device(int(curr))[1])
        xy, stride, n_ptr = curr
        m_ptr, mn_ptr, m_cap = matches if matches is not None else (None, None, 0)
        intr = np.ascontiguousarray(intr, np.float64)
        assert intr.size == 4
        opts = np.ascontiguousarray(track_options() if opts is None else opts, TRACK_OPTIONS_DTYPE)
        self._check(lib().vx_track_pnp_async(self._h, dmap.handle, int(last_kf_id), C.c_void_p(xy), int(stride),
                                             C.c_void_p(n_ptr), C.c_void_p(m_ptr), C.c_void_p(mn_ptr), int(m_cap),
                                             _p(intr), _p(opts)))

    def track_pnp_host_async(self, dmap: "DMap", last_kf_id: int, desc_kf, desc_curr, curr_xy, intr, opts=None,
                             ratio: float = 0.8):
        """The host-input form (vx_track_pnp_host_async, what visionx::PnPTracker calls): both frames'
        descriptor rows and the current positions uploaded in one copy, matched on the device, then
        as track_pnp_async on that match list."""
        q = np.ascontiguousarray(desc_kf, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(desc_curr, np.uint8).reshape(-1, 32)
        xy = np.ascontiguousarray(curr_xy, np.float32).reshape(-1, 2)
        assert len(xy) == len(t)
        intr = np.ascontiguousarray(intr, np.float64)
        opts = np.ascontiguousarray(track_options() if opts is None else opts, TRACK_OPTIONS_DTYPE)
        self._check(lib().vx_track_pnp_host_async(self._h, dmap.handle, int(last_kf_id), _p(q), len(q), _p(t), len(t),
                                                  _p(xy), ratio, _p(intr), _p(opts)))

    def track_pnp_fetch(self, cap: int = 8192):
        """(TRACK_RESULT_DTYPE record, pair_match int32[n_pairs], inlier mask uint8[n_pairs]) of the last
        track_pnp_async: one copy, one synchronisation."""
        out = np.zeros(1, TRACK_RESULT_DTYPE)
        pm = np.zeros(max(cap, 1), np.int32)
        mask = np.zeros(max(cap, 1), np.uint8)
        self._check(lib().vx_track_pnp_fetch(self._h, _p(out), _p(pm), _p(mask), cap))
        n = int(out[0]["n_pairs"])
        return out[0], pm[:n].copy(), mask[:n].copy()

    def _xy_rows(self, rows):
        """a slot number -> (device pointer of its first x, 20, device pointer of its count); a
        (pointer, stride, count pointer) triple as it is"""
        if isinstance(rows, (int, np.integer)):
            return self.slot_keypoints(int(rows)), KEYPOINT_DTYPE.itemsize, self.slot_device(int(rows))[1]
        return rows

    def track_essential_async(self, last, curr, intr, opts=None, matches=None, pose_last=None):
        """Tracking::TrackLastFrame after the match (tracking.cpp:291-325, :509-541) on the device.  last /
        curr: an extraction slot of this context, or (device pointer of the first x, row stride in
        bytes, device pointer of the int32 row count); matches: None = this context's last
        match_*_async result (query = last), or (device pointer of MATCH_DTYPE rows, device pointer of
        the int32 count, capacity); pose_last: T_lw as qx qy qz qw tx ty tz (None: identity).  Nothing
        synchronises; track_essential_fetch() completes it."""
        lxy, lstride, ln = self._xy_rows(last)
        cxy, cstride, cn = self._xy_rows(curr)
        m_ptr, mn_ptr, m_cap = matches if matches is not None else (None, None, 0)
        intr = np.ascontiguousarray(intr, np.float64)
        assert intr.size == 4
        pose = None if pose_last is None else np.ascontiguousarray(pose_last, np.float64)
        assert pose is None or pose.size == 7
        opts = np.ascontiguousarray(track_essential_options() if opts is None else opts, TRACK_ESS_OPTIONS_DTYPE)
        self._check(lib().vx_track_essential_async(self._h, C.c_void_p(lxy), int(lstride), C.c_void_p(ln),
                                                   C.c_void_p(cxy), int(cstride), C.c_void_p(cn), C.c_void_p(m_ptr),
                                                   C.c_void_p(mn_ptr), int(m_cap), None if pose is None else _p(pose),
                                                   _p(intr), _p(opts)))

    def track_essential_host_async(self, desc_last, last_xy, desc_curr, curr_xy, intr, opts=None, ratio: float = 0.8,
                                   pose_last=None):
        """The host-input form (vx_track_essential_host_async, what visionx::EssentialTracker calls): both
        frames' descriptor rows and positions uploaded in one copy, matched on the device (query =
        last), then as track_essential_async on that match list."""
        q = np.ascontiguousarray(desc_last, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(desc_curr, np.uint8).reshape(-1, 32)
        qxy = np.ascontiguousarray(last_xy, np.float32).reshape(-1, 2)
        txy = np.ascontiguousarray(curr_xy, np.float32).reshape(-1, 2)
        assert len(qxy) == len(q) and len(txy) == len(t)
        intr = np.ascontiguousarray(intr, np.float64)
        assert intr.size == 4
        pose = None if pose_last is None else np.ascontiguousarray(pose_last, np.float64)
        assert pose is None or pose.size == 7
        opts = np.ascontiguousarray(track_essential_options() if opts is None else opts, TRACK_ESS_OPTIONS_DTYPE)
        self._check(lib().vx_track_essential_host_async(self._h, _p(q), len(q), _p(qxy), _p(t), len(t), _p(txy), ratio,
                                                        None if pose is None else _p(pose), _p(intr), _p(opts)))

    def track_essential_fetch(self, cap: int = 8192):
        """(TRACK_ESS_RESULT_DTYPE record, pair_match int32[n_pairs], recoverPose mask uint8[n_pairs]) of
        the last track_essential_async: one copy, one synchronisation."""
        out = np.zeros(1, TRACK_ESS_RESULT_DTYPE)
        pm = np.zeros(max(cap, 1), np.int32)
        mask = np.zeros(max(cap, 1), np.uint8)
        self._check(lib().vx_track_essential_fetch(self._h, _p(out), _p(pm), _p(mask), cap))
        n = int(out[0]["n_pairs"])
        return out[0], pm[:n].copy(), mask[:n].copy()

    def track_frame_async(self, dmap, last_kf_id, last_kf, last, curr, intr, opts=None, ratio: float = 0.8,
                          pose_last=None):
        """Tracking::Track (tracking.cpp:267-279) over Frame handles in one enqueue: PnP against last_kf
        (a Frame holding keyframe last_kf_id's features; None: straight to the fallback), and, decided
        on the device, the essential fallback against `last` (None: the fallback fails).  opts: a
        track_frame_options() pair.  Nothing synchronises; track_frame_fetch() completes it."""
        po, eo = track_frame_options() if opts is None else opts
        po = np.ascontiguousarray(po, TRACK_OPTIONS_DTYPE)
        eo = np.ascontiguousarray(eo, TRACK_ESS_OPTIONS_DTYPE)
        intr = np.ascontiguousarray(intr, np.float64)
        assert intr.size == 4
        pose = None if pose_last is None else np.ascontiguousarray(pose_last, np.float64)
        assert pose is None or pose.size == 7
        h = lambda f: None if f is None else f.handle
        self._check(lib().vx_track_frame_async(self._h, None if dmap is None else dmap.handle, int(last_kf_id),
                                               h(last_kf), h(last), h(curr), ratio,
                                               None if pose is None else _p(pose), _p(intr), _p(po), _p(eo)))

    def track_frame_fetch(self, keypoints: bool = True, cap: int = 8192):
        """The last track_frame_async in one copy and one synchronisation: a dict of `result`
        (TRACK_FRAME_RESULT_DTYPE), `pnp` and `ess` ((pair_match, mask) of each path) and `keypoints`
        (the current frame's KEYPOINT_DTYPE rows; None with keypoints=False)."""
        out = np.zeros(1, TRACK_FRAME_RESULT_DTYPE)
        kp = np.zeros(max(cap, 1), KEYPOINT_DTYPE) if keypoints else None
        n = C.c_int(0)
        self._check(lib().vx_track_frame_fetch(self._h, _p(out), None if kp is None else _p(kp), cap, C.byref(n)))
        pairs = []
        for which, rec in ((0, out[0]["pnp"]), (1, out[0]["ess"])):
            k = int(rec["n_pairs"])
            pm, mask = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.uint8)
            self._check(lib().vx_track_frame_pairs(self._h, which, _p(pm), _p(mask), k))
            pairs.append((pm[:k].copy(), mask[:k].copy()))
        return {"result": out[0], "pnp": pairs[0], "ess": pairs[1],
                "keypoints": None if kp is None else kp[:n.value].copy()}

    def track_frame_matches(self, which: int):
        """(device pointer of MATCH_DTYPE rows, device pointer of the int32 count, capacity) of the PnP
        match (0) or the fallback match (1) of the last track_frame_async: what track_*_async and
        DMap.create_keyframe take as `matches`."""
        d, n, cap = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._check(lib().vx_track_frame_matches(self._h, int(which), C.byref(d), C.byref(n), C.byref(cap)))
        return d.value, n.value, cap.value

    def track_rig_async(self, dmap, cams, opts=None, ratio: float = 0.8):
        """Tracking::Track for every camera of a rig time step over one map in ONE enqueue
        (vx_track_rig_async): cams is a list of rig_camera() dicts, opts a track_frame_options() pair
        serving all of them.  Nothing synchronises; track_rig_fetch() completes it."""
        po, eo = track_frame_options() if opts is None else opts
        po = np.ascontiguousarray(po, TRACK_OPTIONS_DTYPE)
        eo = np.ascontiguousarray(eo, TRACK_ESS_OPTIONS_DTYPE)
        tab = np.zeros(max(len(cams), 1), RIG_CAMERA_DTYPE)
        keep = []  # the host arrays the table points to, alive until the call returns
        hv = lambda f: 0 if f is None else int(f.handle.value or 0)
        for r, k in zip(tab, cams):
            intr = np.ascontiguousarray(k["intr"], np.float64)
            assert intr.size == 4
            pose = None if k.get("pose_last") is None else np.ascontiguousarray(k["pose_last"], np.float64)
            assert pose is None or pose.size == 7
            keep += [intr, pose]
            r["last_kf_id"], r["last_kf"], r["last"], r["curr"] = k.get("last_kf_id", 0), hv(k.get("last_kf")), hv(k.get("last")), hv(k["curr"])
            r["intr4"] = intr.ctypes.data
            r["pose_last7"] = 0 if pose is None else pose.ctypes.data
        self._check(lib().vx_track_rig_async(self._h, None if dmap is None else dmap.handle, len(cams), _p(tab), ratio,
                                             _p(po), _p(eo)))

    def track_rig_fetch(self, keypoints: bool = True):
        """The last track_rig_async in one copy and one synchronisation: per camera the dict
        track_frame_fetch returns (`result`, `pnp`, `ess`, `keypoints`), sliced out of the packed block
        at vx_track_rig_layout's offsets."""
        n = C.c_int(0)
        self._check(lib().vx_track_rig_fetch(self._h, 1 if keypoints else 0, None, 0, C.byref(n)))
        b = n.value
        blk, nbytes = C.c_void_p(), C.c_int64(0)
        cp0, cp1, ckp = (np.zeros(b, np.int32) for _ in range(3))
        self._check(lib().vx_track_rig_block(self._h, C.byref(blk), C.byref(nbytes), _p(cp0), _p(cp1), _p(ckp), b))
        off, total = track_rig_layout(cp0, cp1, ckp)
        assert total == nbytes.value
        raw = np.ctypeslib.as_array(C.cast(blk, C.POINTER(C.c_uint8)), shape=(total,))
        out = []
        for i in range(b):
            o = int(off[i])
            res = raw[o:o + TRACK_FRAME_RESULT_DTYPE.itemsize].copy().view(TRACK_FRAME_RESULT_DTYPE)[0]
            o_pm0, o_m0, o_pm1, o_m1, o_kp = (o + x for x in track_frame_block(cp0[i], cp1[i], ckp[i])[:5])
            k0, k1, nk = int(res["pnp"]["n_pairs"]), int(res["ess"]["n_pairs"]), int(res["n_keypoints"])
            pairs = [(raw[opm:opm + 4 * k].copy().view(np.int32), raw[om:om + k].copy())
                     for opm, om, k in ((o_pm0, o_m0, k0), (o_pm1, o_m1, k1))]
            kp = raw[o_kp:o_kp + nk * KEYPOINT_DTYPE.itemsize].copy().view(KEYPOINT_DTYPE) if keypoints else None
            out.append({"result": res, "pnp": pairs[0], "ess": pairs[1], "keypoints": kp})
        return out

    def track_rig_matches(self, cam: int, which: int):
        """(device pointer of MATCH_DTYPE rows, device pointer of the int32 count, capacity) of camera
        cam's PnP match (0) or fallback match (1) of the last track_rig_async, as track_frame_matches"""
        d, n, cap = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._check(lib().vx_track_rig_matches(self._h, int(cam), int(which), C.byref(d), C.byref(n), C.byref(cap)))
        return d.value, n.value, cap.value

    def relocalize_async(self, dmap, cands, curr, intr, opts=None, ratio: float = 0.8):
        """TrackWithPnP against the landmarks of up to MAX_RELOC_CANDIDATES keyframes as ONE pooled PnP
        (vx_relocalize_async): cands is a list of (kf_id, Frame) pairs in the caller's order, curr the current
        Frame, opts a track_options() record.  Nothing synchronises; relocalize_fetch() completes it."""
        opts = np.ascontiguousarray(track_options() if opts is None else opts, TRACK_OPTIONS_DTYPE)
        intr = np.ascontiguousarray(intr, np.float64)
        assert intr.size == 4
        tab = np.zeros(max(len(cands), 1), RELOC_CANDIDATE_DTYPE)
        for r, (kf_id, frame) in zip(tab, cands):
            r["kf_id"], r["frame"] = int(kf_id), 0 if frame is None else int(frame.handle.value or 0)
        self._check(lib().vx_relocalize_async(self._h, None if dmap is None else dmap.handle, len(cands), _p(tab),
                                              None if curr is None else curr.handle, ratio, _p(intr), _p(opts)))

    def relocalize_fetch(self, cap: int = 8192):
        """The last relocalize_async in one copy and one synchronisation: a dict of `result` (RELOC_RESULT_DTYPE),
        `pool_cand` (uint8), `pool_match`, `pool_train` (int32) and `mask` (uint8), n_pool entries each."""
        out = np.zeros(1, RELOC_RESULT_DTYPE)
        pc, mask = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        pm, pt = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        self._check(lib().vx_relocalize_fetch(self._h, _p(out), _p(pc), _p(pm), _p(pt), _p(mask), cap))
        n = int(out[0]["n_pool"])
        return {"result": out[0], "pool_cand": pc[:n].copy(), "pool_match": pm[:n].copy(), "pool_train": pt[:n].copy(),
                "mask": mask[:n].copy()}

    def relocalize_matches(self, cand: int):
        """(device pointer of MATCH_DTYPE rows, device pointer of the int32 count, capacity) of candidate cand's
        Match(kf_cand, curr) of the last relocalize_async, as track_frame_matches"""
        d, n, cap = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._check(lib().vx_relocalize_matches(self._h, int(cand), C.byref(d), C.byref(n), C.byref(cap)))
        return d.value, n.value, cap.value

    def relocalize_table_limit(self) -> int:
        """the largest current-frame capacity relocalize_async accepts (k_reloc_pool's LDS table)"""
        n = C.c_int32(0)
        self._check(lib().vx_relocalize_table_limit(self._h, C.byref(n)))
        return int(n.value)

    def frame_capture_batch(self, bank: int, frames):
        """frames 0 .. len(frames) - 1 of a batch bank (orb_extract_batch*) into the Frame handles in ONE
        launch (vx_frame_capture_batch_async); no synchronisation"""
        hs = (C.c_void_p * max(len(frames), 1))(*[f.handle for f in frames])
        self._check(lib().vx_frame_capture_batch_async(self._h, int(bank), len(frames), hs))

    def init_gate_async(self, d_img_ptr: int, w: int, h: int, channels: int, row_stride: int, feats, opts=None,
                        cap_feat: int | None = None):
        """Tracking::InitWithFirstFrame's gates (tracking.cpp:177-197) on a device image.  feats: an
        extraction slot of this context, or (device pointer of the first x, row stride in bytes, device
        pointer of the int32 row count); cap_feat: at most that many rows (default: the slot's capacity;
        required with a triple).  Nothing synchronises; init_gate_fetch() completes it."""
        if isinstance(feats, (int, np.integer)) and cap_feat is None:
            cap_feat = self.slot_device(int(feats))[2]
        xy, stride, n_ptr = self._xy_rows(feats)
        assert cap_feat is not None
        opts = np.ascontiguousarray(init_gate_options() if opts is None else opts, INIT_GATE_OPTIONS_DTYPE)
        self._check(lib().vx_init_gate_async(self._h, C.c_void_p(d_img_ptr), int(w), int(h), int(channels),
                                             int(row_stride), C.c_void_p(xy), int(stride), C.c_void_p(n_ptr),
                                             int(cap_feat), _p(opts)))

    def init_gate_host(self, img: np.ndarray, xy, opts=None, fetch: bool = True):
        """The host-input form (vx_init_gate_host_async, what visionx::Tracking calls): image rows (H x W
        or H x W x C uint8, any row stride) and float2 positions uploaded in one copy.  Returns the
        fetched INIT_GATE_RESULT_DTYPE record (fetch=False: only enqueues)."""
        assert img.dtype == np.uint8 and img.ndim in (2, 3)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        if img.strides[1] != ch or (img.ndim == 3 and img.strides[2] != 1) or img.strides[0] < w * ch:
            img = np.ascontiguousarray(img)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        opts = np.ascontiguousarray(init_gate_options() if opts is None else opts, INIT_GATE_OPTIONS_DTYPE)
        self._check(lib().vx_init_gate_host_async(self._h, _p(img), w, h, ch, int(img.strides[0]), _p(xy), 8, len(xy),
                                                  _p(opts)))
        return self.init_gate_fetch() if fetch else None

    def init_gate_fetch(self):
        """the INIT_GATE_RESULT_DTYPE record of the last init_gate_async / init_gate_host: one copy, one
        synchronisation"""
        out = np.zeros(1, INIT_GATE_RESULT_DTYPE)
        self._check(lib().vx_init_gate_fetch(self._h, _p(out)))
        return out[0]

    def match_device_async(self, query, train, ratio: float = 0.8):
        """Match device descriptor sets given as slot_device() triples (possibly of another context)."""
        (dq, nq, cq), (dt, nt, ct) = query, train
        self._check(lib().vx_match_device_async(self._h, C.c_void_p(dq), C.c_void_p(nq), cq, C.c_void_p(dt),
                                                C.c_void_p(nt), ct, C.c_float(ratio)))

    def event(self) -> "Event":
        return Event(self)

    def record(self, ev: "Event"):
        self._check(lib().vx_event_record(self._h, ev._h))

    def wait_event(self, ev: "Event"):
        self._check(lib().vx_event_wait(self._h, ev._h))

    def match_batch_async(self, pairs, ratio: float = 0.8):
        """pairs: list of (query, train) device triples (slot_device() / batch_device())."""
        n = len(pairs)
        arr = lambda xs: (C.c_void_p * max(n, 1))(*[C.c_void_p(x) for x in xs])
        dq, nq, dt, nt = (arr([p[0][0] for p in pairs]), arr([p[0][1] for p in pairs]),
                          arr([p[1][0] for p in pairs]), arr([p[1][1] for p in pairs]))
        cq = max([p[0][2] for p in pairs], default=0)
        ct = max([p[1][2] for p in pairs], default=0)
        self._check(lib().vx_match_batch_async(self._h, n, dq, nq, cq, dt, nt, ct, C.c_float(ratio)))

    def match_batch_fetch(self, pair: int, cap: int = 8192):
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_int(0)
        self._check(lib().vx_match_batch_fetch(self._h, pair, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def match_batch(self, pairs, ratio: float = 0.8):
        """vx_match_knn2_ratio_batch: pairs is a list of (query, train) host descriptor arrays (either may be
        empty), matched in one batched call; returns one match array per pair."""
        n = len(pairs)
        qs = [np.ascontiguousarray(q, np.uint8).reshape(-1, 32) for q, _ in pairs]
        ts = [np.ascontiguousarray(t, np.uint8).reshape(-1, 32) for _, t in pairs]
        ptrs = lambda xs: (C.c_void_p * max(n, 1))(*[C.c_void_p(x.ctypes.data if len(x) else None) for x in xs])
        nq = np.array([len(q) for q in qs], np.int32)
        nt = np.array([len(t) for t in ts], np.int32)
        self._check(lib().vx_match_knn2_ratio_batch(self._h, n, ptrs(qs), _p(nq), ptrs(ts), _p(nt), C.c_float(ratio)))
        return [self.match_batch_fetch(i, max(len(q), 1)) for i, q in enumerate(qs)]

    def match_fetch(self, cap: int = 8192):
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_int(0)
        self._check(lib().vx_match_fetch(self._h, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    # ---------------------------------------------------------------- bundle adjustment
    def ba_optimize(self, m, opts: BAOptions | None = None, ref_kf_id=None) -> BAStats:
        opts = opts or default_ba_options(window=m.get("window", 5))
        ref = m.get("ref_kf_id") if ref_kf_id is None else ref_kf_id
        v = map_view(m)
        st = BAStats()
        self._check(lib().vx_ba_optimize_map(self._h, C.byref(v), C.c_uint64(0 if ref is None else int(ref)),
                                             0 if ref is None else 1, C.byref(opts), C.byref(st)))
        return st

    def ba_plan(self, m, opts: BAOptions | None = None, ref_kf_id=None, shard_rank=0, shard_count=1,
                host_build=False, global_poses=False):
        return BAPlan(self, m, opts, ref_kf_id, shard_rank, shard_count, host_build, global_poses)

    def graph_enable(self, on=True):
        self._check(lib().vx_graph_enable(self._h, 1 if on else 0))

    def set_grid_share(self, share: float):
        """vx_set_grid_share: size one-round grids for this share of the CUs (concurrent contexts)."""
        self._check(lib().vx_set_grid_share(self._h, C.c_float(share)))

    def set_order(self, order: int):
        """vx_orb_set_order: ORDER_STL (default: OpenCV's libstdc++ retainBest permutation) or
        ORDER_RASTER (the same keypoint set per level in raster order)."""
        self._check(lib().vx_orb_set_order(self._h, int(order)))

    @property
    def order(self) -> int:
        return lib().vx_orb_get_order(self._h)

    def set_debug(self, flags: int):
        """vx_orb_set_debug (test hook): DEBUG_FAST_NO_BORDER | DEBUG_STAGES."""
        self._check(lib().vx_orb_set_debug(self._h, int(flags)))

    def debug_read(self, level: int, what: int):
        """vx_orb_debug_read after orb_extract: 0 level bytes, 1 blurred level, 2 candidate records
        (raster order), 3 retainBest(2q) order (indices into 2), 4 final records (CAND_DTYPE)."""
        n = C.c_int64(0)
        rc = lib().vx_orb_debug_read(self._h, level, what, None, 0, C.byref(n))
        if rc not in (VX_OK, VX_ERR_CAPACITY):
            self._check(rc)
        dt = {0: np.uint8, 1: np.uint8, 2: CAND_DTYPE, 3: np.int32, 4: CAND_DTYPE}[what]
        out = np.zeros(max(n.value, 1), dt)
        self._check(lib().vx_orb_debug_read(self._h, level, what, _p(out), out.nbytes, C.byref(n)))
        return out[:n.value]

    def test_retain_best(self, keys, npts: int, wide: bool = False, use_lds: bool = True):
        """vx_test_retain_best: the device retainBest over bare keys; kept indices in output order."""
        keys = np.ascontiguousarray(keys, np.uint32)
        out = np.zeros(max(len(keys), 1), np.int32)
        n = C.c_int(0)
        self._check(lib().vx_test_retain_best(self._h, _p(keys), len(keys), int(npts), int(wide), int(use_lds),
                                              _p(out), C.byref(n)))
        return out[:n.value].copy()

    def graph_counts(self):
        """(graphs captured, graph launches) of this context's hipGraph replay."""
        cap, lau = C.c_int(0), C.c_int(0)
        self._check(lib().vx_graph_counts(self._h, C.byref(cap), C.byref(lau)))
        return cap.value, lau.value

    # ---------------------------------------------------------------- landmark creation
    def depth_landmarks(self, uv, has, depth, intr, pose):
        """Tracking::CreateLandmarksFromDepth on the GPU: (index per feature or -1, created points)."""
        uv = np.ascontiguousarray(uv, np.float64)
        has = np.ascontiguousarray(has, np.uint8)
        n = len(has)
        idx = np.full(max(n, 1), -1, np.int32)
        pw = np.zeros((max(n, 1), 3))
        cnt = C.c_int(0)
        if depth is None:
            dptr, dt, rows, cols, stride = None, 0, 0, 0, 0
        else:
            depth = np.ascontiguousarray(depth)
            dptr, dt = _p(depth), DEPTH_TYPES[depth.dtype]
            rows, cols, stride = depth.shape[0], depth.shape[1], depth.strides[0]
        intr = np.ascontiguousarray(intr, np.float64)
        pose = np.ascontiguousarray(pose, np.float64)
        self._check(lib().vx_depth_landmarks(self._h, _p(uv), _p(has), n, dptr, dt, rows, cols, C.c_int64(stride),
                                             _p(intr), _p(pose), _p(idx), _p(pw), C.byref(cnt)))
        return idx[:n].copy(), pw[:cnt.value].copy()

    def triangulate(self, d, min_angle_deg=1.0, max_err=5.0, intr1=None, intr2=None):
        """Tracking::TriangulateWithLastKeyFrame on the GPU for a synth.make_keyframe_pair dict."""
        m = np.ascontiguousarray(d["matches"])
        nm = len(m)
        idx = np.full(max(nm, 1), -1, np.int32)
        pw = np.zeros((max(nm, 1), 3))
        cnt = C.c_int(0)
        i1 = np.ascontiguousarray(d["intr"] if intr1 is None else intr1, np.float64)
        i2 = np.ascontiguousarray(d["intr"] if intr2 is None else intr2, np.float64)
        self._check(lib().vx_triangulate(self._h, _p(d["uv1"]), _p(d["has1"]), len(d["has1"]), _p(i1),
                                         _p(d["pose1"]), _p(d["uv2"]), _p(d["has2"]), len(d["has2"]), _p(i2),
                                         _p(d["pose2"]), _p(m), nm, C.c_double(min_angle_deg), C.c_double(max_err),
                                         _p(idx), _p(pw), C.byref(cnt)))
        return idx[:nm].copy(), pw[:cnt.value].copy()

    def pnp_ransac_batch(self, offsets, obj, img, intr, opts):
        """cv::solvePnPRansac (Tracking::TrackWithPnP, tracking.cpp:414-423) on the GPU for independent
        problems: problem p owns rows offsets[p]:offsets[p+1] of obj (float32 x3) / img (float32 x2),
        intr[p] = fx fy cx cy, opts[p] a PNP_OPTIONS_DTYPE record.  Returns (results[P], mask[N])."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
        img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        intr = np.ascontiguousarray(intr, np.float64).reshape(-1, 4)
        opts = np.ascontiguousarray(np.atleast_1d(opts), PNP_OPTIONS_DTYPE)
        P = len(offsets) - 1
        n = int(offsets[-1])
        assert len(obj) == n and len(img) == n and len(intr) == P and len(opts) == P
        out = np.zeros(max(P, 1), PNP_RESULT_DTYPE)
        mask = np.zeros(max(n, 1), np.uint8)
        self._check(lib().vx_pnp_ransac_batch(self._h, P, _p(offsets), _p(obj), _p(img), _p(intr), _p(opts),
                                              _p(mask), _p(out)))
        return out[:P].copy(), mask[:n].copy()

    def pnp_ransac(self, obj, img, intr, opt):
        """One solvePnPRansac call: (result record, inlier mask)."""
        obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
        img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        intr = np.ascontiguousarray(intr, np.float64)
        opt = np.ascontiguousarray(opt, PNP_OPTIONS_DTYPE)
        out = np.zeros(1, PNP_RESULT_DTYPE)
        mask = np.zeros(max(len(obj), 1), np.uint8)
        self._check(lib().vx_pnp_ransac(self._h, _p(obj), _p(img), len(obj), _p(intr), _p(opt), _p(mask), _p(out)))
        return out[0], mask[:len(obj)].copy()

    def essential_ransac_batch(self, offsets, pts_last, pts_curr, intr, opts):
        """cv::findEssentialMat + cv::recoverPose (Tracking::EstimatePoseByEssential,
        tracking.cpp:503-547) on the GPU for independent problems: (results[P], mask[N])."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        p1 = np.ascontiguousarray(pts_last, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts_curr, np.float32).reshape(-1, 2)
        intr = np.ascontiguousarray(intr, np.float64).reshape(-1, 4)
        opts = np.ascontiguousarray(np.atleast_1d(opts), EM_OPTIONS_DTYPE)
        P = len(offsets) - 1
        n = int(offsets[-1])
        assert len(p1) == n and len(p2) == n and len(intr) == P and len(opts) == P
        out = np.zeros(max(P, 1), EM_RESULT_DTYPE)
        mask = np.zeros(max(n, 1), np.uint8)
        self._check(lib().vx_essential_ransac_batch(self._h, P, _p(offsets), _p(p1), _p(p2), _p(intr), _p(opts),
                                                    _p(mask), _p(out)))
        return out[:P].copy(), mask[:n].copy()

    def essential_ransac(self, pts_last, pts_curr, intr, opt):
        """One findEssentialMat + recoverPose: (result record, recoverPose mask)."""
        p1 = np.ascontiguousarray(pts_last, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts_curr, np.float32).reshape(-1, 2)
        intr = np.ascontiguousarray(intr, np.float64)
        opt = np.ascontiguousarray(opt, EM_OPTIONS_DTYPE)
        out = np.zeros(1, EM_RESULT_DTYPE)
        mask = np.zeros(max(len(p1), 1), np.uint8)
        self._check(lib().vx_essential_ransac(self._h, _p(p1), _p(p2), len(p1), _p(intr), _p(opt), _p(mask),
                                              _p(out)))
        return out[0], mask[:len(p1)].copy()

    def sba_optimize(self, m, opts: SBAOptions | None = None, ref_kf_id=None) -> SBAStats:
        """Schur-complement joint BA (vx_sba_optimize_map) on a synth.BAMap, in place."""
        opts = opts or default_sba_options(window=m.get("window", 5))
        ref = m.get("ref_kf_id") if ref_kf_id is None else ref_kf_id
        v = map_view(m)
        st = SBAStats()
        self._check(lib().vx_sba_optimize_map(self._h, C.byref(v), C.c_uint64(0 if ref is None else int(ref)),
                                              0 if ref is None else 1, C.byref(opts), C.byref(st)))
        return st

    def sba_plan(self, m, opts: SBAOptions | None = None, ref_kf_id=None, shard_rank=0, shard_count=1):
        return SBAPlan(self, m, opts, ref_kf_id, shard_rank, shard_count)

    # ---------------------------------------------------------------- multi-GPU
    def sba_shard_emulate(self, plans):
        """vx_sba_shard_emulate_run: the Schur shard plans run on this one device as the ranks of a
        sharded Schur BA would, the all-reduce of the reduced system replaced by a rank-order sum."""
        arr = (C.c_void_p * len(plans))(*[pl._h.value for pl in plans])
        self._check(lib().vx_sba_shard_emulate_run(self._h, arr, len(plans)))

    def ba_shard_emulate(self, plans):
        """vx_ba_shard_emulate_run: the shard plans (rank r of len(plans)) run on this one device
        as the ranks of a sharded LocalBA would, the all-reduce replaced by a rank-order sum."""
        arr = (C.c_void_p * len(plans))(*[pl._h.value for pl in plans])
        self._check(lib().vx_ba_shard_emulate_run(self._h, arr, len(plans)))

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = lib().vx_comm_unique_id(buf)
        if rc != VX_OK:
            raise VxError(rc, "ncclGetUniqueId failed")
        return bytes(buf)

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(lib().vx_comm_init(self._h, buf, nranks, rank))

    def comm_info(self):
        """(nranks, rank) as RCCL reports them for this context's communicator (vx_comm_info)."""
        n, r = C.c_int(0), C.c_int(0)
        self._check(lib().vx_comm_info(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    # ---------------------------------------------------------------- profiling
    def prof_enable(self, on=True, stages=None):
        """on=False disables; stages=None brackets every stage, else an iterable of stage names."""
        if not on:
            mask = 0
        elif stages is None:
            mask = -1
        else:
            names = [lib().vx_prof_name(i).decode() for i in range(lib().vx_prof_count())]
            mask = 0
            for s in stages:
                mask |= 1 << names.index(s)
        self._check(lib().vx_prof_enable64(self._h, C.c_uint64(mask & 0xFFFFFFFFFFFFFFFF)))

    def prof_read(self, reset=True) -> dict:
        n = lib().vx_prof_count()
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        self._check(lib().vx_prof_read(self._h, ms, cnt, 1 if reset else 0))
        return {lib().vx_prof_name(i).decode(): (ms[i], cnt[i]) for i in range(n)}


class Frame:
    """A frame's keypoints, descriptors and count on the device for as long as the object lives
    (vx_frame): what Context.track_frame_async, match_device_async, track_*_async and
    DMap.create_keyframe read, without a slot that the next extraction overwrites."""

    def __init__(self, ctx: Context, cap: int):
        self._h = C.c_void_p()
        self.cap = int(cap)
        ctx._check(lib().vx_frame_create(ctx._h, int(cap), C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def capture(self, ctx: Context, slot: int):
        """an extraction slot of ctx -> this frame (one launch on ctx's stream, no synchronisation)"""
        ctx._check(lib().vx_frame_capture_async(ctx._h, int(slot), self._h))
        return self

    def extract_host(self, ctx: Context, img: np.ndarray, params: OrbParams | None = None):
        """ORBExtractor::Extract of a host image into this frame (upload, extraction, capture; no
        synchronisation): orb_extract's keypoints and descriptors, byte for byte"""
        img = np.ascontiguousarray(img)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        params = params or default_orb_params()
        ctx._check(lib().vx_frame_extract_host_async(ctx._h, self._h, C.byref(params), _p(img), w, h, ch,
                                                     C.c_int64(img.strides[0])))
        return self

    def upload(self, ctx: Context, xy, desc):
        """host float2 positions + 32-byte rows -> this frame in one copy (the other keypoint fields 0)"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert len(xy) == len(desc)
        ctx._check(lib().vx_frame_upload_async(ctx._h, self._h, _p(xy), _p(desc), len(xy)))
        return self

    def device(self):
        """dict of the device pointers the device-input forms take: xy (first x), stride (20), desc,
        count, cap; `rows` = the (xy, stride, count) triple of track_*_async, `desc_rows` = the
        (desc, count, cap) triple of match_device_async"""
        xy, st, d, n, cap = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int32()
        rc = lib().vx_frame_device(self._h, C.byref(xy), C.byref(st), C.byref(d), C.byref(n), C.byref(cap))
        if rc != VX_OK:
            raise VxError(rc, "vx_frame_device: no frame")
        return {"xy": xy.value, "stride": st.value, "desc": d.value, "count": n.value, "cap": cap.value,
                "rows": (xy.value, st.value, n.value), "desc_rows": (d.value, n.value, cap.value)}

    def fetch(self, ctx: Context, descriptors: bool = True, cap: int | None = None, overflow: bool = False):
        """(keypoints, descriptors) — descriptors None with descriptors=False — in one copy and one
        synchronisation of ctx; overflow=True appends the frame's overflow flag"""
        cap = self.cap if cap is None else cap
        kp = np.zeros(max(cap, 1), KEYPOINT_DTYPE)
        desc = np.zeros((max(cap, 1), 32), np.uint8) if descriptors else None
        n, ov = C.c_int(0), C.c_int(0)
        ctx._check(lib().vx_frame_fetch_ex(ctx._h, self._h, _p(kp), None if desc is None else _p(desc), cap,
                                           C.byref(n), C.byref(ov)))
        out = (kp[:n.value].copy(), None if desc is None else desc[:n.value].copy())
        return out + (ov.value,) if overflow else out

    def close(self):
        if self._h:
            lib().vx_frame_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BAPlan:
    """vx_ba_plan: host window selection + device CSR upload, repeatable device runs."""

    def __init__(self, ctx: Context, m, opts=None, ref_kf_id=None, shard_rank=0, shard_count=1, host_build=False,
                 global_poses=False):
        """host_build: the host reference build of the plan (VX_PLAN_HOST_BUILD) instead of the
        device build; global_poses: the large-window kernels at any window size
        (VX_PLAN_GLOBAL_POSES)."""
        self.ctx = ctx
        self.m = m
        self.opts = opts or default_ba_options(window=m.get("window", 5))
        ref = m.get("ref_kf_id") if ref_kf_id is None else ref_kf_id
        self._h = C.c_void_p()
        v = map_view(m)
        ctx._check(lib().vx_ba_plan_create_ex(ctx.handle, C.byref(v), C.c_uint64(0 if ref is None else int(ref)),
                                              0 if ref is None else 1, C.byref(self.opts), shard_rank,
                                              shard_count, (1 if host_build else 0) | (2 if global_poses else 0),
                                              C.byref(self._h)))

    def info(self):
        out = np.zeros(8, np.int64)
        rc = lib().vx_ba_plan_info(self._h, _p(out))
        assert rc == 0
        keys = ["n_kf", "n_lm", "n_pose_obs", "n_lm_obs", "n_opt", "n_split", "n_lm_blocks", "max_lm_obs"]
        return {k: int(v) for k, v in zip(keys, out)}

    def layout(self):
        """vx_ba_plan_layout: whether the plan has the fused k_ba_iter layout, and its shape."""
        out = np.zeros(4, np.int64)
        self.ctx._check(lib().vx_ba_plan_layout(self._h, _p(out)))
        return {k: int(v) for k, v in zip(["fused", "threads", "workgroups", "max_slots"], out)}

    def persistent(self) -> bool:
        """vx_ba_plan_persistent: runs are one persistent k_ba_win launch per window."""
        return bool(lib().vx_ba_plan_persistent(self._h))

    def fused_tables(self) -> bytes:
        """vx_ba_plan_fused_tables: the fused layout's index tables, back to back (test hook)."""
        n = C.c_size_t(0)
        self.ctx._check(lib().vx_ba_plan_fused_tables(self.ctx.handle, self._h, None, C.c_size_t(0), C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        self.ctx._check(lib().vx_ba_plan_fused_tables(self.ctx.handle, self._h, _p(buf), n, C.byref(n)))
        return buf.tobytes()

    def run_async(self):
        self.ctx._check(lib().vx_ba_plan_run_async(self.ctx.handle, self._h))

    def fetch(self, m=None) -> BAStats:
        st = BAStats()
        v = map_view(m) if m is not None else None
        self.ctx._check(lib().vx_ba_plan_fetch(self.ctx.handle, self._h, C.byref(v) if v is not None else None,
                                               C.byref(st)))
        return st

    def apply(self, dmap: "DMap"):
        """vx_ba_plan_apply_dmap: scatter the run's poses / positions into the resident map."""
        self.ctx._check(lib().vx_ba_plan_apply_dmap(self.ctx.handle, self._h, dmap.handle))

    def close(self):
        if self._h:
            lib().vx_ba_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Seq:
    """vx_seq: a recorded list of async calls replayed from C by run() (include/vx_slam.h)."""

    def __init__(self):
        self._h = C.c_void_p()
        if lib().vx_seq_create(C.byref(self._h)) != VX_OK:
            raise VxError(VX_ERR_INVALID, "vx_seq_create failed")
        self._ctxs = {}
        # every object whose raw handle or device memory a recorded call names (events, plans, the
        # tensors behind image pointers when given): the header requires them to outlive the
        # sequence, so the sequence holds them until close()
        self._keep = []

    def _add(self, rc, ctx, *keep):
        if rc != VX_OK:
            raise VxError(rc, "vx_seq: bad arguments")
        self._ctxs[len(self)] = ctx
        self._keep.extend(k for k in keep if k is not None)

    def wait(self, ctx, ev):
        self._add(lib().vx_seq_wait(self._h, ctx.handle, ev._h), ctx, ev)

    def record(self, ctx, ev):
        self._add(lib().vx_seq_record(self._h, ctx.handle, ev._h), ctx, ev)

    def extract(self, ctx, params, d_img, w, h, ch, stride, slot, owner=None):
        """d_img: a device pointer (int); owner: the object holding that memory (e.g. the torch
        tensor), kept alive with the sequence."""
        self._add(lib().vx_seq_extract(self._h, ctx.handle, C.byref(params), C.c_void_p(d_img), w, h, ch, stride, slot),
                  ctx, owner, params)

    def match(self, ctx, q, t, ratio=0.8):
        """q / t: (desc, count, cap) device triples (Context.slot_device)."""
        self._add(lib().vx_seq_match(self._h, ctx.handle, C.c_void_p(q[0]), C.c_void_p(q[1]), q[2], C.c_void_p(t[0]),
                                     C.c_void_p(t[1]), t[2], C.c_float(ratio)), ctx)

    def ba_run(self, ctx, plan):
        self._add(lib().vx_seq_ba_run(self._h, ctx.handle, plan._h), ctx, plan)

    def __len__(self):
        return lib().vx_seq_length(self._h)

    def set_threads(self, n: int):
        """vx_seq_set_threads: > 1 replays each context's calls on a host thread of its own."""
        if lib().vx_seq_set_threads(self._h, int(n)) != VX_OK:
            raise VxError(VX_ERR_INVALID, "vx_seq_set_threads")

    def run(self):
        bad = C.c_int(-1)
        rc = lib().vx_seq_run(self._h, C.byref(bad))
        if rc != VX_OK:
            ctx = self._ctxs.get(bad.value + 1)
            raise VxError(rc, f"vx_seq_run: call {bad.value}: " + (lib().vx_last_error(ctx.handle).decode() if ctx else ""))

    def close(self):
        if self._h:
            lib().vx_seq_destroy(self._h)
            self._h = C.c_void_p()
        self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DMap:
    """vx_dmap: visionx::Map resident on the device, updated incrementally (include/vx_slam.h)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()
        ctx._check(lib().vx_dmap_create(ctx.handle, C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def add_keyframe(self, kf_id, pose7, intr4, has_cam, feat_uv, feat_lm_id, feat_flags):
        uv = np.ascontiguousarray(feat_uv, np.float64).reshape(-1, 2)
        lm = np.ascontiguousarray(feat_lm_id, np.uint64)
        fl = np.ascontiguousarray(feat_flags, np.uint8)
        pose = np.ascontiguousarray(pose7, np.float64)
        intr = np.ascontiguousarray(intr4, np.float64)
        self.ctx._check(lib().vx_dmap_add_keyframe(self._h, C.c_uint64(int(kf_id)), _p(pose), _p(intr),
                                                   1 if has_cam else 0, len(fl), _p(uv), _p(lm), _p(fl)))

    def add_landmarks(self, ids, pos, bad=None):
        ids = np.ascontiguousarray(ids, np.uint64)
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        b = None if bad is None else np.ascontiguousarray(bad, np.uint8)
        self.ctx._check(lib().vx_dmap_add_landmarks(self._h, len(ids), _p(ids), _p(pos),
                                                    None if b is None else _p(b)))

    def add_observations(self, lm_ids, kf_ids, feat_idx):
        a = np.ascontiguousarray(lm_ids, np.uint64)
        k = np.ascontiguousarray(kf_ids, np.uint64)
        f = np.ascontiguousarray(feat_idx, np.uint64)
        self.ctx._check(lib().vx_dmap_add_observations(self._h, len(a), _p(a), _p(k), _p(f)))

    def remove_observations(self, lm_ids, kf_ids):
        """Landmark::RemoveObservation(kf_id) for each (landmark, keyframe) pair."""
        a = np.ascontiguousarray(lm_ids, np.uint64)
        k = np.ascontiguousarray(kf_ids, np.uint64)
        self.ctx._check(lib().vx_dmap_remove_observations(self._h, len(a), _p(a), _p(k)))

    def remove_keyframe(self, kf_id):
        """Map::RemoveKeyFrame(id)."""
        self.ctx._check(lib().vx_dmap_remove_keyframe(self._h, C.c_uint64(int(kf_id))))

    def remove_landmarks(self, lm_ids):
        """Map::RemoveLandmark(id) for each id."""
        a = np.ascontiguousarray(lm_ids, np.uint64)
        self.ctx._check(lib().vx_dmap_remove_landmarks(self._h, len(a), _p(a)))

    def live_counts(self):
        out = np.zeros(4, np.int64)
        self.ctx._check(lib().vx_dmap_live_counts(self._h, _p(out)))
        return dict(zip(["kf", "lm", "obs"], map(int, out[:3])))

    def set_features(self, kf_id, feat_idx, lm_ids, flags):
        i = np.ascontiguousarray(feat_idx, np.int32)
        lm = np.ascontiguousarray(lm_ids, np.uint64)
        fl = np.ascontiguousarray(flags, np.uint8)
        self.ctx._check(lib().vx_dmap_set_features(self._h, C.c_uint64(int(kf_id)), len(i), _p(i), _p(lm), _p(fl)))

    def set_landmark_bad(self, ids, bad):
        ids = np.ascontiguousarray(ids, np.uint64)
        b = np.ascontiguousarray(bad, np.uint8)
        self.ctx._check(lib().vx_dmap_set_landmark_bad(self._h, len(ids), _p(ids), _p(b)))

    def set_poses(self, kf_ids, poses):
        ids = np.ascontiguousarray(kf_ids, np.uint64)
        ps = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        self.ctx._check(lib().vx_dmap_set_poses(self._h, len(ids), _p(ids), _p(ps)))

    def counts(self):
        out = np.zeros(4, np.int64)
        self.ctx._check(lib().vx_dmap_counts(self._h, _p(out)))
        return dict(zip(["kf", "feat", "lm", "obs"], map(int, out)))

    def download(self):
        c = self.counts()
        pose = np.zeros((max(c["kf"], 1), 7))
        pos = np.zeros((max(c["lm"], 1), 3))
        self.ctx._check(lib().vx_dmap_download(self._h, _p(pose), _p(pos)))
        return pose[:c["kf"]], pos[:c["lm"]]

    def plan(self, opts, ref_kf_id=None, shard_rank=0, shard_count=1) -> "BAPlan":
        """vx_ba_plan_create_dmap: the LocalBA plan from the resident map."""
        plan = BAPlan.__new__(BAPlan)
        plan.ctx, plan.m, plan.opts = self.ctx, None, opts
        plan._h = C.c_void_p()
        self.ctx._check(lib().vx_ba_plan_create_dmap(self.ctx.handle, self._h,
                                                     C.c_uint64(0 if ref_kf_id is None else int(ref_kf_id)),
                                                     0 if ref_kf_id is None else 1, C.byref(opts), shard_rank,
                                                     shard_count, C.byref(plan._h)))
        return plan

    def optimize(self, opts, ref_kf_id=None) -> BAStats:
        """vx_ba_optimize_dmap: LocalBA::Optimize on the resident map in one call (plan, run and the
        scatter into the map; synchronises once, at its end)."""
        st = BAStats()
        self.ctx._check(lib().vx_ba_optimize_dmap(self.ctx.handle, self._h,
                                                  C.c_uint64(0 if ref_kf_id is None else int(ref_kf_id)),
                                                  0 if ref_kf_id is None else 1, C.byref(opts), C.byref(st)))
        return st

    def sba_plan(self, opts, ref_kf_id=None) -> "SBAPlan":
        """vx_sba_plan_create_dmap: the Schur-complement BA plan from the resident map."""
        plan = SBAPlan.__new__(SBAPlan)
        plan.ctx, plan.opts = self.ctx, opts
        plan._h = C.c_void_p()
        self.ctx._check(lib().vx_sba_plan_create_dmap(self.ctx.handle, self._h,
                                                      C.c_uint64(0 if ref_kf_id is None else int(ref_kf_id)),
                                                      0 if ref_kf_id is None else 1, C.byref(opts), C.byref(plan._h)))
        return plan

    def sba_plan_rebuild(self, plan: "SBAPlan", ref_kf_id=None) -> "SBAPlan":
        """vx_sba_plan_rebuild_dmap: rebuild a plan of this map in place (its buffers reused)."""
        self.ctx._check(lib().vx_sba_plan_rebuild_dmap(self.ctx.handle, self._h,
                                                       C.c_uint64(0 if ref_kf_id is None else int(ref_kf_id)),
                                                       0 if ref_kf_id is None else 1, plan._h))
        return plan

    def prefetch_results(self, on=True):
        """vx_dmap_prefetch_results: optimize() brings its results back with its one synchronisation."""
        self.ctx._check(lib().vx_dmap_prefetch_results(self._h, 1 if on else 0))

    def results(self):
        """vx_ba_dmap_results: (keyframe rows, their poses (n, 7), landmark rows, positions (n, 3)) the
        last optimize() changed."""
        nk, nl = C.c_int(0), C.c_int(0)
        rc = lib().vx_ba_dmap_results(self.ctx.handle, self._h, 0, None, None, 0, None, None, C.byref(nk),
                                      C.byref(nl))
        if rc not in (VX_OK, VX_ERR_CAPACITY):
            self.ctx._check(rc)
        kr, kp = np.zeros(max(nk.value, 1), np.int64), np.zeros((max(nk.value, 1), 7))
        lr, lp = np.zeros(max(nl.value, 1), np.int64), np.zeros((max(nl.value, 1), 3))
        self.ctx._check(lib().vx_ba_dmap_results(self.ctx.handle, self._h, len(kr), _p(kr), _p(kp), len(lr), _p(lr),
                                                 _p(lp), C.byref(nk), C.byref(nl)))
        return kr[:nk.value], kp[:nk.value], lr[:nl.value], lp[:nl.value]

    def results_view(self):
        """vx_ba_dmap_results_view (prefetching on): the same four arrays as results(), read from the
        pinned block the last optimize() filled (copied here; the C++ adapter reads them in place)."""
        kr, lr = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        kp, lp = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        nk, nl = C.c_int(0), C.c_int(0)
        self.ctx._check(lib().vx_ba_dmap_results_view(self.ctx.handle, self._h, C.byref(kr), C.byref(kp), C.byref(lr),
                                                      C.byref(lp), C.byref(nk), C.byref(nl)))
        n, m = nk.value, nl.value
        if n == 0 and m == 0:
            return (np.zeros(0, np.int64), np.zeros((0, 7)), np.zeros(0, np.int64), np.zeros((0, 3)))
        k_rows = np.ctypeslib.as_array(kr, (n,)).astype(np.int64)
        k_pose = np.ctypeslib.as_array(kp, (n, 8))[:, :7].copy()
        l_rows = np.ctypeslib.as_array(lr, (m,)).astype(np.int64)
        l_pos = np.ctypeslib.as_array(lp, (m, 4))[:, :3].copy()
        return k_rows, k_pose, l_rows, l_pos

    def _create_done(self, c, rc, res):
        self.last_create = res[0].copy()
        c._check(rc)
        return {"result": res[0], "landmarks": self.create_results()}

    def create_keyframe(self, kf_id, pose7, intr4, curr, *, last_kf_id=None, matches=None, depth=None,
                        first_landmark_id=0, opts=None, ctx=None):
        """vx_dmap_create_keyframe: Tracking::CreateKeyFrame (tracking.cpp:577-584) on the resident map
        from device inputs, one synchronisation.  curr: an extraction slot of the context, or (device
        pointer of the first x, row stride in bytes, device pointer of the int32 row count, row
        capacity); last_kf_id None = no triangulation; matches: None = the context's last match_*_async
        result, or (device pointer of MATCH_DTYPE rows, device pointer of the int32 count, capacity);
        depth: None, or (device pointer, VX_DEPTH_* type, rows, cols, row stride in bytes).  Returns
        {"result": KEYFRAME_RESULT_DTYPE record, "landmarks": KEYFRAME_LANDMARK_DTYPE records}; a
        rejected call raises VxError, its record (error_bits) is self.last_create."""
        c = self.ctx if ctx is None else ctx
        if isinstance(curr, (int, np.integer)):
            _, n_ptr, cap = c.slot_device(int(curr))
            curr = (c.slot_keypoints(int(curr)), KEYPOINT_DTYPE.itemsize, n_ptr, cap)
        xy, stride, n_ptr, cap = curr
        m_ptr, mn_ptr, m_cap = matches if matches is not None else (None, None, 0)
        d_ptr, d_type, rows, cols, d_stride = depth if depth is not None else (None, 0, 0, 0, 0)
        pose = np.ascontiguousarray(pose7, np.float64)
        intr = None if intr4 is None else np.ascontiguousarray(intr4, np.float64)
        o = np.ascontiguousarray(keyframe_options() if opts is None else opts, KEYFRAME_OPTIONS_DTYPE)
        res = np.zeros(1, KEYFRAME_RESULT_DTYPE)
        rc = lib().vx_dmap_create_keyframe(c.handle, self._h, C.c_uint64(int(kf_id)), _p(pose),
                                           None if intr is None else _p(intr), C.c_void_p(xy), int(stride),
                                           C.c_void_p(n_ptr), int(cap), 0 if last_kf_id is None else 1,
                                           C.c_uint64(0 if last_kf_id is None else int(last_kf_id)), C.c_void_p(m_ptr),
                                           C.c_void_p(mn_ptr), int(m_cap), C.c_void_p(d_ptr), int(d_type), int(rows),
                                           int(cols), int(d_stride), C.c_uint64(int(first_landmark_id)), _p(o), _p(res))
        return self._create_done(c, rc, res)

    def create_keyframe_host(self, kf_id, pose7, intr4, feat_uv, *, last_kf_id=None, matches=None, depth=None,
                             first_landmark_id=0, opts=None, ctx=None):
        """vx_dmap_create_keyframe_host: the same from host arrays (positions (n, 2) float64, a
        MATCH_DTYPE list, a 2-D depth image whose row stride is taken from the array), staged and
        uploaded in one copy.  Returns what create_keyframe returns."""
        c = self.ctx if ctx is None else ctx
        uv = np.ascontiguousarray(feat_uv, np.float64).reshape(-1, 2)
        mt = np.zeros(0, MATCH_DTYPE) if matches is None else np.ascontiguousarray(matches, MATCH_DTYPE)
        if depth is None:
            dptr, dt, rows, cols, dstride = None, 0, 0, 0, 0
        else:
            if depth.strides[1] != depth.itemsize or depth.strides[0] < depth.shape[1] * depth.itemsize:
                depth = np.ascontiguousarray(depth)
            # (a view with padded rows: the rows the call reads end inside its base buffer)
            dptr, dt = C.c_void_p(depth.ctypes.data), DEPTH_TYPES[depth.dtype]
            rows, cols, dstride = depth.shape[0], depth.shape[1], depth.strides[0]
        pose = np.ascontiguousarray(pose7, np.float64)
        intr = None if intr4 is None else np.ascontiguousarray(intr4, np.float64)
        o = np.ascontiguousarray(keyframe_options() if opts is None else opts, KEYFRAME_OPTIONS_DTYPE)
        res = np.zeros(1, KEYFRAME_RESULT_DTYPE)
        rc = lib().vx_dmap_create_keyframe_host(c.handle, self._h, C.c_uint64(int(kf_id)), _p(pose),
                                                None if intr is None else _p(intr), _p(uv), len(uv),
                                                0 if last_kf_id is None else 1,
                                                C.c_uint64(0 if last_kf_id is None else int(last_kf_id)), _p(mt),
                                                len(mt), dptr, int(dt), int(rows), int(cols), int(dstride),
                                                C.c_uint64(int(first_landmark_id)), _p(o), _p(res))
        return self._create_done(c, rc, res)

    def create_keyframe_frame(self, kf_id, pose7, intr4, frame, *, last_kf_id=None, matches=None, depth=None,
                              first_landmark_id=0, opts=None, ctx=None):
        """vx_dmap_create_keyframe_frame: the same over a Frame handle; matches: a device triple
        (Context.track_frame_matches / track_rig_matches) or None for the context's last match; depth: a
        host 2-D image or None.  Returns what create_keyframe returns."""
        c = self.ctx if ctx is None else ctx
        m_ptr, mn_ptr, m_cap = matches if matches is not None else (None, None, 0)
        if depth is None:
            dptr, dt, rows, cols, dstride = None, 0, 0, 0, 0
        else:
            depth = np.ascontiguousarray(depth)
            dptr, dt = C.c_void_p(depth.ctypes.data), DEPTH_TYPES[depth.dtype]
            rows, cols, dstride = depth.shape[0], depth.shape[1], depth.strides[0]
        pose = np.ascontiguousarray(pose7, np.float64)
        intr = None if intr4 is None else np.ascontiguousarray(intr4, np.float64)
        o = np.ascontiguousarray(keyframe_options() if opts is None else opts, KEYFRAME_OPTIONS_DTYPE)
        res = np.zeros(1, KEYFRAME_RESULT_DTYPE)
        rc = lib().vx_dmap_create_keyframe_frame(c.handle, self._h, C.c_uint64(int(kf_id)), _p(pose),
                                                 None if intr is None else _p(intr), frame.handle,
                                                 C.c_int(0 if last_kf_id is None else 1),
                                                 C.c_uint64(0 if last_kf_id is None else int(last_kf_id)),
                                                 C.c_void_p(m_ptr), C.c_void_p(mn_ptr), C.c_int(int(m_cap)), dptr,
                                                 C.c_int(int(dt)), C.c_int(int(rows)), C.c_int(int(cols)),
                                                 C.c_int64(int(dstride)), C.c_uint64(int(first_landmark_id)), _p(o), _p(res))
        return self._create_done(c, rc, res)

    def create_keyframes_rig(self, cams, first_landmark_id=0, opts=None, ctx=None):
        """vx_dmap_create_keyframes_rig: Tracking::CreateKeyFrame for every camera of a rig step that
        inserts a keyframe, in one call and one synchronisation.  cams: a list of dicts with
        create_keyframe_frame's per-camera arguments ("kf_id", "pose7", "intr4", "frame", and optionally
        "last_kf_id", "matches" (a device triple, Context.track_rig_matches(i, 0)), "depth" (a host 2-D
        image)).  Returns {"results": KEYFRAME_RESULT_DTYPE[n], "landmarks": all cameras' records in
        camera order}; camera i's slice follows from the results' counts.  A rejected call raises
        VxError and commits nothing; the per-camera records (error_bits) are self.last_create_rig."""
        c = self.ctx if ctx is None else ctx
        tab = np.zeros(max(len(cams), 1), RIG_KEYFRAME_DTYPE)
        keep = []  # the host arrays the table points to, alive until the call returns
        for r, k in zip(tab, cams):
            pose = np.ascontiguousarray(k["pose7"], np.float64)
            assert pose.size == 7
            intr = None if k.get("intr4") is None else np.ascontiguousarray(k["intr4"], np.float64)
            assert intr is None or intr.size == 4
            depth = None if k.get("depth") is None else np.ascontiguousarray(k["depth"])
            keep += [pose, intr, depth]
            m_ptr, mn_ptr, m_cap = k["matches"] if k.get("matches") is not None else (0, 0, 0)
            last = k.get("last_kf_id")
            r["kf_id"], r["pose7"], r["intr4"] = int(k["kf_id"]), pose.ctypes.data, 0 if intr is None else intr.ctypes.data
            r["curr"] = int(k["frame"].handle.value or 0)
            r["has_last"], r["last_kf_id"] = (0, 0) if last is None else (1, int(last))
            r["d_matches"], r["d_n_matches"], r["cap_matches"] = int(m_ptr or 0), int(mn_ptr or 0), int(m_cap)
            if depth is not None:
                r["depth"], r["depth_type"] = depth.ctypes.data, DEPTH_TYPES[depth.dtype]
                r["rows"], r["cols"], r["row_stride"] = depth.shape[0], depth.shape[1], depth.strides[0]
        o = np.ascontiguousarray(keyframe_options() if opts is None else opts, KEYFRAME_OPTIONS_DTYPE)
        res = np.zeros(max(len(cams), 1), KEYFRAME_RESULT_DTYPE)
        rc = lib().vx_dmap_create_keyframes_rig(c.handle, self._h, len(cams), _p(tab), C.c_uint64(int(first_landmark_id)),
                                                _p(o), _p(res))
        del keep
        self.last_create_rig = res[:len(cams)].copy()
        c._check(rc)
        return {"results": res[:len(cams)], "landmarks": self.create_results()}

    def create_results(self):
        """vx_dmap_create_results: the last create_keyframe*'s KEYFRAME_LANDMARK_DTYPE records."""
        n = C.c_int(0)
        self.ctx._check(lib().vx_dmap_create_results(self._h, 0, None, C.byref(n)))
        rec = np.zeros(max(n.value, 1), KEYFRAME_LANDMARK_DTYPE)
        self.ctx._check(lib().vx_dmap_create_results(self._h, len(rec), _p(rec), C.byref(n)))
        return rec[:n.value]

    def keyframe_features(self, kf_id):
        """vx_dmap_keyframe_features: (uv (n, 2), lm_id, flags) of a live keyframe, read from the device."""
        n = C.c_int(0)
        self.ctx._check(lib().vx_dmap_keyframe_features(self._h, C.c_uint64(int(kf_id)), 0, None, None, None,
                                                        C.byref(n)))
        k = max(n.value, 1)
        uv, lm, fl = np.zeros((k, 2)), np.zeros(k, np.uint64), np.zeros(k, np.uint8)
        self.ctx._check(lib().vx_dmap_keyframe_features(self._h, C.c_uint64(int(kf_id)), k, _p(uv), _p(lm), _p(fl),
                                                        C.byref(n)))
        return uv[:n.value], lm[:n.value], fl[:n.value]

    def cull_results(self):
        """vx_dmap_cull_results: the last cull call's (landmark records, feature records)."""
        nl, nf = C.c_int(0), C.c_int(0)
        self.ctx._check(lib().vx_dmap_cull_results(self._h, 0, None, 0, None, C.byref(nl), C.byref(nf)))
        lm = np.zeros(max(nl.value, 1), CULL_LANDMARK_DTYPE)
        ft = np.zeros(max(nf.value, 1), CULL_FEATURE_DTYPE)
        self.ctx._check(lib().vx_dmap_cull_results(self._h, len(lm), _p(lm), len(ft), _p(ft), C.byref(nl),
                                                   C.byref(nf)))
        return lm[:nl.value], ft[:nf.value]

    def cull_landmarks(self, opts=None, ctx=None):
        """vx_dmap_cull_landmarks: Tracking::CullLandmarks on the resident map (decision and edit on the
        device, one synchronisation).  Returns {"landmarks": CULL_LANDMARK_DTYPE records in ascending
        row, "features": CULL_FEATURE_DTYPE records of the features reset}.  `ctx`: another context
        of the same device to run on."""
        o = cull_options() if opts is None else opts
        c = self.ctx if ctx is None else ctx
        nl, nf = C.c_int(0), C.c_int(0)
        c._check(lib().vx_dmap_cull_landmarks(c.handle, self._h, _p(o), C.byref(nl), C.byref(nf)))
        lm, ft = self.cull_results()
        assert len(lm) == nl.value and len(ft) == nf.value
        return {"landmarks": lm, "features": ft}

    def keyframe_redundancy(self, opts=None, ctx=None):
        """vx_dmap_keyframe_redundancy: {"kf_id", "total", "redundant"} of every live keyframe in
        ascending id (the counts of Tracking::CullKeyFrames' loop); no edit."""
        o = cull_options() if opts is None else opts
        c = self.ctx if ctx is None else ctx
        cap = max(self.live_counts()["kf"], 1)
        ids, tot, red = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int(0)
        c._check(lib().vx_dmap_keyframe_redundancy(c.handle, self._h, _p(o), cap, _p(ids), _p(tot), _p(red),
                                                   C.byref(n)))
        return {"kf_id": ids[:n.value], "total": tot[:n.value], "redundant": red[:n.value]}

    def cull_keyframes(self, opts=None, protect=(), ctx=None):
        """vx_dmap_cull_keyframes: Tracking::CullKeyFrames (with RemoveKeyFrame and the trailing
        CullLandmarks) on the resident map.  `protect`: the ids of last_keyframe_, init_frame_ and the
        current frame.  Returns {"removed": bool, "kf_id", "ratio", "landmarks", "features"}."""
        o = cull_options() if opts is None else opts
        c = self.ctx if ctx is None else ctx
        pr = np.ascontiguousarray(list(protect), np.uint64)
        rem, nl, nf = C.c_int(0), C.c_int(0), C.c_int(0)
        kid, ratio = C.c_uint64(0), C.c_double(0.0)
        c._check(lib().vx_dmap_cull_keyframes(c.handle, self._h, _p(o), _p(pr) if len(pr) else None, len(pr),
                                              C.byref(rem), C.byref(kid), C.byref(ratio), C.byref(nl), C.byref(nf)))
        lm, ft = self.cull_results()
        assert len(lm) == nl.value and len(ft) == nf.value
        return {"removed": bool(rem.value), "kf_id": int(kid.value), "ratio": float(ratio.value), "landmarks": lm,
                "features": ft}

    def close(self):
        if self._h:
            lib().vx_dmap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SBAPlan:
    """vx_sba_plan: Schur-complement joint BA plan (window, observation / block / pair tables)."""

    def __init__(self, ctx: Context, m, opts=None, ref_kf_id=None, shard_rank=0, shard_count=1):
        self.ctx = ctx
        self.opts = opts or default_sba_options(window=m.get("window", 5))
        ref = m.get("ref_kf_id") if ref_kf_id is None else ref_kf_id
        self._h = C.c_void_p()
        v = map_view(m)
        ctx._check(lib().vx_sba_plan_create(ctx.handle, C.byref(v), C.c_uint64(0 if ref is None else int(ref)),
                                            0 if ref is None else 1, C.byref(self.opts), shard_rank,
                                            shard_count, C.byref(self._h)))

    def info(self):
        out = np.zeros(8, np.int64)
        assert lib().vx_sba_plan_info(self._h, _p(out)) == 0
        keys = ["n_kf", "n_opt", "n_obs", "n_pairs", "n_blocks", "n", "n_tiles", "n_comp"]
        return {k: int(v) for k, v in zip(keys, out)}

    def factor_work(self):
        """vx_sba_plan_factor_work: the dense pose solve's tiles and its FP64 flops per factorisation."""
        out = np.zeros(4, np.int64)
        assert lib().vx_sba_plan_factor_work(self._h, _p(out)) == 0
        d = dict(zip(["l_tiles", "updates", "diag", "panel"], (int(x) for x in out)))
        d["flops"] = 2 * 16 ** 3 * d["updates"] + 16 ** 3 * d["panel"] + (16 ** 3 // 3) * d["diag"]
        return d

    def run_async(self):
        self.ctx._check(lib().vx_sba_plan_run_async(self.ctx.handle, self._h))

    def fetch(self, m=None) -> SBAStats:
        st = SBAStats()
        v = map_view(m) if m is not None else None
        self.ctx._check(lib().vx_sba_plan_fetch(self.ctx.handle, self._h, C.byref(v) if v is not None else None,
                                                C.byref(st)))
        return st

    def apply(self, dmap):
        """vx_sba_plan_apply_dmap: the run's best state into the resident map (plans from DMap.sba_plan)."""
        self.ctx._check(lib().vx_sba_plan_apply_dmap(self.ctx.handle, self._h, dmap.handle))

    def system(self):
        """(S, rhs) of the last assembly (lower triangle of S meaningful, damping included)."""
        n = self.info()["n"]
        S = np.zeros((n, n))
        rhs = np.zeros(n)
        self.ctx._check(lib().vx_sba_plan_system(self.ctx.handle, self._h, _p(S), _p(rhs), n))
        return S, rhs

    def step(self):
        """vx_sba_plan_step: (dx, fail) — the pose step of the run's last solving iteration (S dx = rhs;
        6 per window keyframe, fixed ones 0) and whether any iteration's Cholesky failed."""
        n = self.info()["n"]
        dx = np.zeros(n)
        fail = C.c_int32(0)
        self.ctx._check(lib().vx_sba_plan_step(self.ctx.handle, self._h, _p(dx), n, C.byref(fail)))
        return dx, int(fail.value)

    def close(self):
        if self._h:
            lib().vx_sba_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dmap_load(dmap: DMap, m, kf_rows=None):
    """Insert a synth.BAMap into a DMap the way a running system builds its map: keyframes in
    ascending id order (``kf_rows`` limits it to those snapshot rows, in that order), each with its
    features; the landmarks first observed by that keyframe; then that keyframe's observations
    (Landmark::AddObservation, in landmark order).  Returns (kf_order, lm_order): the snapshot
    keyframe / landmark rows in the DMap's insertion order (landmarks never observed go last)."""
    ids = m["kf_id"]
    kf_order = np.argsort(ids, kind="stable") if kf_rows is None else np.asarray(kf_rows)
    optr = m["lm_obs_ptr"]
    obs_lm = np.repeat(np.arange(len(m["lm_id"])), np.diff(optr))
    obs_kf = m["obs_kf_id"]
    seen = np.zeros(len(m["lm_id"]), bool)
    lm_order = []
    for k in kf_order:
        f0, f1 = m["kf_feat_ptr"][k], m["kf_feat_ptr"][k + 1]
        dmap.add_keyframe(ids[k], m["kf_pose"].reshape(-1, 7)[k], m["kf_intr"].reshape(-1, 4)[k], m["kf_has_cam"][k],
                          m["feat_uv"].reshape(-1, 2)[f0:f1], m["feat_lm_id"][f0:f1], m["feat_flags"][f0:f1])
        sel = np.nonzero(obs_kf == ids[k])[0]  # observation rows of this keyframe, landmark order
        new = np.unique(obs_lm[sel][~seen[obs_lm[sel]]])
        if len(new):
            dmap.add_landmarks(m["lm_id"][new], m["lm_pos"].reshape(-1, 3)[new], m["lm_bad"][new])
            seen[new] = True
            lm_order.extend(new.tolist())
        if len(sel):
            dmap.add_observations(m["lm_id"][obs_lm[sel]], obs_kf[sel], m["obs_feat_idx"][sel])
    if kf_rows is None:
        rest = np.nonzero(~seen)[0]
        if len(rest):
            dmap.add_landmarks(m["lm_id"][rest], m["lm_pos"].reshape(-1, 3)[rest], m["lm_bad"][rest])
            lm_order.extend(rest.tolist())
    return np.asarray(kf_order), np.asarray(lm_order, np.int64)


def map_reorder(m, kf_order, lm_order):
    """The snapshot with its keyframe / landmark rows permuted (per-landmark observation lists kept);
    the result has the input's type (a synth.BAMap stays one, so its deep .copy() is kept)."""
    out = type(m)(m)
    fp = m["kf_feat_ptr"]
    cnt = np.diff(fp)[kf_order]
    out["kf_id"] = m["kf_id"][kf_order].copy()
    out["kf_pose"] = m["kf_pose"].reshape(-1, 7)[kf_order].copy()
    out["kf_intr"] = m["kf_intr"].reshape(-1, 4)[kf_order].copy()
    out["kf_has_cam"] = m["kf_has_cam"][kf_order].copy()
    out["kf_feat_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    fidx = np.concatenate([np.arange(fp[k], fp[k + 1]) for k in kf_order]) if len(kf_order) else np.zeros(0, int)
    out["feat_uv"] = m["feat_uv"].reshape(-1, 2)[fidx].copy()
    out["feat_lm_id"] = m["feat_lm_id"][fidx].copy()
    out["feat_flags"] = m["feat_flags"][fidx].copy()
    optr = m["lm_obs_ptr"]
    out["lm_id"] = m["lm_id"][lm_order].copy()
    out["lm_pos"] = m["lm_pos"].reshape(-1, 3)[lm_order].copy()
    out["lm_bad"] = m["lm_bad"][lm_order].copy()
    ocnt = np.diff(optr)[lm_order]
    out["lm_obs_ptr"] = np.concatenate([[0], np.cumsum(ocnt)]).astype(np.int64)
    oidx = np.concatenate([np.arange(optr[l], optr[l + 1]) for l in lm_order]) if len(lm_order) else np.zeros(0, int)
    out["obs_kf_id"] = m["obs_kf_id"][oidx].copy()
    out["obs_feat_idx"] = m["obs_feat_idx"][oidx].copy()
    return out
