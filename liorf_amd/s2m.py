"""Python binding of the C ABI in include/liorf_s2m.h (libliorf_s2m.so, HIP / gfx950).

`MapOptimizationS2M` mirrors the members and method names of the reference's
`mapOptimization` class that belong to the scan-to-map path (reference
src/mapOptmization.cpp:1069-1363): `transformTobeMapped`, `isDegenerate`,
`laserCloudSurfFromMapDS` / `laserCloudSurfLastDS` setters, `scan2MapOptimization()`.
Everything runs in the HIP library; there is no CPU fallback — a missing library or GPU
raises immediately.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("S2M_LIB") or os.path.join(_HERE, "libliorf_s2m.so")   # S2M_LIB: A/B measurements of two builds

S2M_OK = 0
S2M_ERR_CAPACITY = -5
S2M_ERR_BUSY = -6
S2M_ERR_FORMAT, S2M_ERR_CHECKSUM, S2M_ERR_IO = -7, -8, -9   # saving and loading a session
ERRORS = {-1: "S2M_ERR_INVALID_ARG", -2: "S2M_ERR_NO_DEVICE", -3: "S2M_ERR_HIP", -4: "S2M_ERR_NO_SCAN",
          -5: "S2M_ERR_CAPACITY", -6: "S2M_ERR_BUSY", -7: "S2M_ERR_FORMAT", -8: "S2M_ERR_CHECKSUM", -9: "S2M_ERR_IO"}

# every symbol include/liorf_s2m.h declares
ABI_SYMBOLS = [
    "s2m_version", "s2m_default_params", "s2m_create", "s2m_destroy", "s2m_last_error", "s2m_set_params", "s2m_get_params",
    "s2m_set_map", "s2m_set_map_device", "s2m_set_scan", "s2m_set_scan_device",
    "s2m_optimize", "s2m_optimize_resident", "s2m_optimize_launch", "s2m_optimize_collect",
    "s2m_optimize_batch", "s2m_batch_set_scan", "s2m_batch_set_scans", "s2m_slot_set_scan", "s2m_slot_optimize_launch", "s2m_slot_optimize_collect", "s2m_optimize_batch_launch", "s2m_optimize_batch_collect", "s2m_batch_get_trace",
    "s2m_get_trace", "s2m_surf_optimization", "s2m_normal_eq", "s2m_last_timing", "s2m_debug_deferred",
    "s2m_time_iteration_kernel", "s2m_time_iterations", "s2m_make_scancontext", "s2m_debug_wave_profile", "s2m_debug_time_steady", "s2m_time_loop_launches",
    "s2m_debug_scan_prep",
    "s2m_voxel_downsample", "s2m_voxel_downsample_device", "s2m_downsample_scan", "s2m_extract_cloud",
    "s2m_transform_cloud",
    "s2m_icp_default_params", "s2m_icp_align", "s2m_icp_align_guess", "s2m_debug_device_trig", "s2m_debug_device_hypot",
    "s2m_debug_lm_close", "s2m_debug_lm_close_check_args", "s2m_debug_lm_rows", "s2m_debug_lm_rows_check_args",
    "s2m_sc_reset", "s2m_sc_size", "s2m_sc_add_scan", "s2m_sc_add_descriptor", "s2m_sc_detect_loop", "s2m_sc_distance",
    "s2m_sc_query_default_params", "s2m_sc_query_check_args", "s2m_sc_query_key", "s2m_sc_query_descriptor", "s2m_sc_query_scan", "s2m_sc_query_projected",
    "s2m_sc_query_many_default_params", "s2m_sc_query_many_check_args", "s2m_sc_query_keys", "s2m_sc_query_descriptors", "s2m_sc_get_descriptors",
    "s2m_debug_sc_query_many_pass", "s2m_debug_sc_query_many_shape", "s2m_debug_sc_query_many_last",
    "s2m_sc_ring_default_params", "s2m_sc_ring_check_args", "s2m_sc_ring_neighbours_keys", "s2m_sc_ring_neighbours_descriptors",
    "s2m_sc_query_keys_ring", "s2m_sc_query_descriptors_ring", "s2m_debug_sc_ring_pass", "s2m_debug_sc_ring_shape", "s2m_debug_sc_ring_last",
    "s2m_kf_default_params", "s2m_kf_reset", "s2m_kf_size", "s2m_kf_add", "s2m_kf_set_poses", "s2m_extract_surrounding",
    "s2m_extract_surrounding_at",
    "s2m_loop_default_params", "s2m_loop_near_keyframes", "s2m_loop_align", "s2m_loop_closure_rs",
    "s2m_loop_align_launch", "s2m_loop_closure_rs_launch", "s2m_loop_poll", "s2m_loop_collect",
    "s2m_loop_verify_check_args", "s2m_loop_verify_launch", "s2m_loop_verify_poll", "s2m_loop_verify_collect", "s2m_loop_verify",
    "s2m_loop_verify_many_check_args", "s2m_loop_verify_many", "s2m_debug_icp_align_pairs_device",
    "s2m_debug_loop_verify_many_pass", "s2m_debug_loop_verify_many_last", "s2m_debug_loop_verify_many_plan", "s2m_debug_batch_last",
    "s2m_loop_detect_default_params", "s2m_loop_detect_keys_check_args", "s2m_loop_detect_keys",
    "s2m_debug_loop_detect_pass", "s2m_debug_loop_detect_shape", "s2m_debug_loop_detect_last", "s2m_debug_loop_detect_splits",
    "s2m_reloc_default_params", "s2m_relocalize_check_args", "s2m_relocalize_scan", "s2m_debug_icp_align_guess_many_device",
    "s2m_debug_icp_nearest", "s2m_debug_icp_time_nearest", "s2m_debug_icp_align_device", "s2m_debug_icp_align_many_device",
    "s2m_debug_icp_tuning", "s2m_debug_icp_grid_check_args", "s2m_debug_icp_grid",
    "s2m_debug_icp_close_check_args", "s2m_debug_icp_close", "s2m_debug_icp_sums_check_args", "s2m_debug_icp_sums",
    "s2m_gmap_default_params", "s2m_global_map", "s2m_kf_map_cloud",
    "s2m_scan_layout_preset", "s2m_project_default_params", "s2m_imu_deskew_info", "s2m_project_check_args", "s2m_project_scan",
    "s2m_downsample_projected", "s2m_sc_add_projected",
    "s2m_odom_deskew_info", "s2m_project_check_args_motion", "s2m_project_scan_motion", "s2m_guess_state_init", "s2m_update_initial_guess",
    "s2m_pg_default_params", "s2m_pg_check_args", "s2m_pg_reset", "s2m_pg_size", "s2m_pg_add_prior", "s2m_pg_add_between", "s2m_pg_add_gps",
    "s2m_pg_set_initial", "s2m_pg_add_odometry", "s2m_pg_optimize", "s2m_pg_get_poses", "s2m_pg_marginal", "s2m_pg_apply_to_store",
    "s2m_pg_marginals_check_args", "s2m_pg_marginals", "s2m_pg_joint_marginal",
    "s2m_pg_optimize_launch", "s2m_pg_optimize_poll", "s2m_pg_optimize_collect", "s2m_debug_pg_rebase",
    "s2m_debug_pg_set_estimate", "s2m_debug_pg_linearize", "s2m_debug_pg_apply", "s2m_debug_pg_apply_check_args", "s2m_debug_pg_cg",
    "s2m_debug_pg_retract",
    "s2m_pg_consistency_default_params", "s2m_pg_consistency_check_args", "s2m_pg_consistent_loops",
    "s2m_session_info_of", "s2m_session_save", "s2m_session_load", "s2m_session_save_file", "s2m_session_load_file", "s2m_session_check",
    "s2m_debug_session_chunk", "s2m_debug_sc_keys", "s2m_debug_kf_frame",
    "s2m_debug_kf_select_last", "s2m_debug_kf_select_last_check_args",
    "s2m_session_append_check_args", "s2m_session_append", "s2m_session_append_file", "s2m_session_place", "s2m_session_appended",
    "s2m_session_anchor_from_pairs", "s2m_relocalize_key",
]
S2M_SESSION_VERSION = 1
S2M_RING_U8, S2M_RING_U16, S2M_RING_I32 = 0, 1, 2
S2M_TIME_F32, S2M_TIME_U32_NS, S2M_TIME_U32, S2M_TIME_F64_REL = 0, 1, 2, 3
S2M_SENSOR_VELODYNE, S2M_SENSOR_LIVOX, S2M_SENSOR_OUSTER, S2M_SENSOR_MULRAN, S2M_SENSOR_ROBOSENSE = 0, 1, 2, 3, 4
S2M_IMU_QUEUE_LENGTH = 2000
S2M_KF_FROM_HOST, S2M_KF_FROM_DEVICE, S2M_KF_FROM_LAST_DOWNSAMPLE = 0, 1, 2
S2M_LOOP_NONE, S2M_LOOP_ALREADY_CLOSED, S2M_LOOP_TOO_FEW_POINTS, S2M_LOOP_REJECTED, S2M_LOOP_ACCEPTED = 0, 1, 2, 3, 4
S2M_LOOP_PENDING = 5                                     # a launched closure whose ICP is still queued or running
S2M_LOOP_MAX_CANDIDATES = 8                              # candidates of one verification: the slots of the device loop
S2M_LOOP_MANY_MAX_PAIRS = 64      # pairs of one pass of s2m_loop_verify_many
S2M_DEBUG_PREP_READ, S2M_DEBUG_PREP_NEW, S2M_DEBUG_PREP_LEGACY = -1, 0, 1   # chains of s2m_debug_scan_prep (liorf_s2m_debug.h)
S2M_ICP_RANGE = 8                                        # iterations the device loop queues at a time (liorf_s2m_debug.h)
S2M_DEBUG_ICP_GRID_MAX_CELLS = 1 << 18                   # most cells of a grid of the device loop's search (liorf_s2m_debug.h)
S2M_WARN_LEAF_TOO_SMALL = 1
S2M_DEBUG_KF_NARROW, S2M_DEBUG_KF_PRE, S2M_DEBUG_KF_WIDE = 0, 1, 2   # s2m_debug_kf_select_out::path (liorf_s2m_debug.h)
S2M_PG_PRIOR, S2M_PG_BETWEEN, S2M_PG_GPS, S2M_PG_INITIAL = 0, 1, 2, 3
S2M_PG_PENDING, S2M_PG_IDLE = 2, 3                       # s2m_pg_optimize_launch / _poll / _collect: queued or running; nothing pending
S2M_PG_BLOCK_COLUMNS = 24                                # right-hand sides per pass of the block solve
S2M_DEBUG_PG_FWD, S2M_DEBUG_PG_BWD, S2M_DEBUG_PG_K, S2M_DEBUG_PG_KT = 0, 1, 2, 3   # operators of s2m_debug_pg_apply
PG_MARGINALS_KEYS_PER_PASS = S2M_PG_BLOCK_COLUMNS // 6   # keys one pass of s2m_pg_marginals serves
S2M_PG_CONSISTENCY_MAX = 4096                            # candidates of one s2m_pg_consistent_loops: 64 words of 64 bits per row
S2M_SC_QUERY_MAX_K = 32
S2M_SC_ALIGN_SECTOR_KEY, S2M_SC_ALIGN_FULL = 0, 1        # s2m_sc_query_params::align: 7 shifts around the sector-key guess; all 60
SC_QUERY_MAX_GROUPS = 1024                               # kScQueryMaxGroups: workgroups of the query's distance kernel, 3 keys each per pass


class Params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device_id", C.c_int32), ("stream", C.c_void_p),
                ("k_neighbors", C.c_int32), ("gate_sq", C.c_double), ("plane_tol", C.c_double),
                ("weight_scale", C.c_double), ("weight_min", C.c_double), ("min_corr", C.c_int32),
                ("min_feats", C.c_int32), ("max_iter", C.c_int32), ("eig_thresh", C.c_float),
                ("conv_deg", C.c_double), ("conv_cm", C.c_double), ("z_tol", C.c_float), ("rot_tol", C.c_float),
                ("imu_type", C.c_int32), ("imu_rpy_weight", C.c_float), ("early_exit", C.c_int32)]


class ImuInit(C.Structure):
    _fields_ = [("imuAvailable", C.c_int64), ("imuRollInit", C.c_float), ("imuPitchInit", C.c_float),
                ("imuYawInit", C.c_float)]


class Result(C.Structure):
    _fields_ = [("iters_run", C.c_int32), ("converged", C.c_int32), ("is_degenerate", C.c_int32),
                ("n_sel_last", C.c_int32), ("skipped", C.c_int32), ("pose", C.c_float * 6),
                ("affine", C.c_float * 12)]


class IterTrace(C.Structure):
    _fields_ = [("n_sel", C.c_int32), ("stepped", C.c_int32), ("delta", C.c_float * 6),
                ("pose", C.c_float * 6), ("deltaR", C.c_float), ("deltaT", C.c_float)]


class LmCloseOut(C.Structure):
    """s2m_debug_lm_close_out (include/liorf_s2m_debug.h)."""
    _fields_ = [("AtA", C.c_float * 36), ("AtB", C.c_float * 6), ("n_sel_last", C.c_int32), ("trace", IterTrace),
                ("pose", C.c_float * 6), ("pose_next", C.c_float * 6), ("iters_run", C.c_int32), ("converged", C.c_int32),
                ("done", C.c_int32), ("stalled", C.c_int32), ("is_degenerate", C.c_int32), ("n_rows_active", C.c_int32),
                ("matP", C.c_float * 36)]


class LmRowsOut(C.Structure):
    """s2m_debug_lm_rows_out (include/liorf_s2m_debug.h)."""
    _fields_ = [("n_rows_active", C.c_int32), ("wpb", C.c_int32), ("nblocks", C.c_int32), ("n_waves", C.c_int32),
                ("pose_used", C.c_float * 6), ("done", C.c_int32)]


class ScMatch(C.Structure):
    _fields_ = [("min_dist", C.c_double), ("nn_idx", C.c_int32), ("nn_align", C.c_int32),
                ("cand_idx", C.c_int32 * 3), ("cand_d2", C.c_float * 3)]


class ScQueryParams(C.Structure):
    """s2m_sc_query_params: the searched keys [first, first+count) (count = -1: to the end) outside [exclude_lo, exclude_hi)."""
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("exclude_lo", C.c_int32), ("exclude_hi", C.c_int32),
                ("top_k", C.c_int32), ("align", C.c_int32), ("max_dist", C.c_double)]


class ScQueryManyParams(C.Structure):
    """s2m_sc_query_many_params: the single query's parameters per query, and for stored-key queries the relative window
    [key + rel_lo, key + rel_hi) that is left out as well."""
    _fields_ = [("q", ScQueryParams), ("rel_lo", C.c_int32), ("rel_hi", C.c_int32)]


class ScRingParams(C.Structure):
    """s2m_sc_ring_params: the many-query's parameters and the number of ring-key neighbours that go on to the column-by-column
    distance (1 .. S2M_SC_RING_MAX_CAND; 3 is the detector's NUM_CANDIDATES_FROM_TREE)."""
    _fields_ = [("m", ScQueryManyParams), ("n_candidates", C.c_int32), ("reserved", C.c_int32)]


class ScRingNeighbour(C.Structure):
    _fields_ = [("d2", C.c_float), ("key", C.c_int32)]


SC_RING_NEIGHBOUR_DTYPE = np.dtype([("d2", np.float32), ("key", np.int32)])
S2M_SC_RING_MAX_CAND = 256


class ScHit(C.Structure):
    _fields_ = [("dist", C.c_double), ("key", C.c_int32), ("shift", C.c_int32), ("yaw_diff_rad", C.c_float), ("reserved", C.c_int32)]


SC_HIT_DTYPE = np.dtype([("dist", np.float64), ("key", np.int32), ("shift", np.int32), ("yaw_diff_rad", np.float32), ("reserved", np.int32)])
assert SC_HIT_DTYPE.itemsize == C.sizeof(ScHit) == 24


class IcpParams(C.Structure):
    _fields_ = [("max_correspondence_distance", C.c_double), ("max_iterations", C.c_int32),
                ("transformation_epsilon", C.c_double), ("euclidean_fitness_epsilon", C.c_double)]


class IcpResult(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("converged", C.c_int32), ("iterations", C.c_int32), ("fitness_score", C.c_double)]


class IcpGridOut(C.Structure):
    """s2m_debug_icp_grid_out (include/liorf_s2m_debug.h)."""
    _fields_ = [("lo", C.c_float * 3), ("cell", C.c_float), ("inv", C.c_float), ("n", C.c_int32 * 3), ("n_fin", C.c_int32),
                ("usable", C.c_int32)]


class IcpLoopStateWords(C.Structure):
    """s2m_debug_icp_state (include/liorf_s2m_debug.h) as the 38 32-bit words it is made of: T 16 floats, T_step 16 floats,
    prev_mse (a double, two words), it, conv, similar, done."""
    _fields_ = [("w", C.c_uint32 * 38)]


class KfParams(C.Structure):
    _fields_ = [("search_radius", C.c_float), ("density", C.c_float), ("map_leaf", C.c_float), ("recent_window_s", C.c_double)]


class LoopParams(C.Structure):
    _fields_ = [("search_radius", C.c_float), ("time_diff_s", C.c_float), ("search_num", C.c_int32),
                ("fitness_score", C.c_float), ("icp_leaf", C.c_float)]


class LoopDetectParams(C.Structure):
    """s2m_loop_detect_params: radius and time gate, the searched range, the fixed and the relative window, top_k."""
    _fields_ = [("search_radius", C.c_float), ("time_diff_s", C.c_float), ("first", C.c_int32), ("count", C.c_int32),
                ("exclude_lo", C.c_int32), ("exclude_hi", C.c_int32), ("rel_lo", C.c_int32), ("rel_hi", C.c_int32),
                ("top_k", C.c_int32), ("reserved", C.c_int32)]


class LoopResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("key_cur", C.c_int32), ("key_pre", C.c_int32), ("n_cur", C.c_int32),
                ("n_prev", C.c_int32), ("icp", IcpResult), ("pose_from", C.c_float * 6), ("pose_to", C.c_float * 6)]


class RelocParams(C.Structure):
    """s2m_reloc_params: the place query, the loop's submap / ICP / gate settings, and whether the hit's yaw goes into the guess."""
    _fields_ = [("query", ScQueryParams), ("loop", LoopParams), ("use_yaw", C.c_int32), ("reserved", C.c_int32)]


class RelocCandidate(C.Structure):
    """s2m_reloc_candidate: one hit of the query with its alignment; icp.T maps the scan's frame into the map frame."""
    _fields_ = [("hit", ScHit), ("status", C.c_int32), ("n_src", C.c_int32), ("n_tgt", C.c_int32), ("guess", C.c_float * 16),
                ("icp", IcpResult), ("pose_xyzrpy", C.c_float * 6), ("pose_tobemapped", C.c_float * 6)]


class GmapParams(C.Structure):
    _fields_ = [("search_radius", C.c_float), ("pose_density", C.c_float), ("leaf", C.c_float)]


class ScanLayout(C.Structure):
    _fields_ = [("stride", C.c_uint32), ("off_x", C.c_uint32), ("off_intensity", C.c_uint32), ("off_ring", C.c_uint32),
                ("off_time", C.c_uint32), ("ring_type", C.c_int32), ("time_type", C.c_int32)]


class ProjectParams(C.Structure):
    _fields_ = [("n_scan", C.c_int32), ("downsample_rate", C.c_int32), ("point_filter_num", C.c_int32),
                ("lidar_min_range", C.c_float), ("lidar_max_range", C.c_float)]


class DeskewInfo(C.Structure):
    _fields_ = [("time_scan_cur", C.c_double), ("deskew", C.c_int32), ("imu_pointer_cur", C.c_int32),
                ("imu_time", C.POINTER(C.c_double)), ("imu_rot_x", C.POINTER(C.c_double)),
                ("imu_rot_y", C.POINTER(C.c_double)), ("imu_rot_z", C.POINTER(C.c_double))]


class OdomSample(C.Structure):
    _fields_ = [("time", C.c_double), ("px", C.c_double), ("py", C.c_double), ("pz", C.c_double), ("qx", C.c_double),
                ("qy", C.c_double), ("qz", C.c_double), ("qw", C.c_double), ("cov0", C.c_double)]


class OdomDeskew(C.Structure):
    _fields_ = [("odom_available", C.c_int32), ("odom_deskew_flag", C.c_int32), ("initial_guess", C.c_float * 6),
                ("odom_incre", C.c_float * 3), ("n_popped", C.c_int32)]


class MotionInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("time_scan_end", C.c_double), ("odom_incre", C.c_float * 3)]


class GuessState(C.Structure):
    _fields_ = [("last_imu_transformation", C.c_float * 12), ("last_imu_pre_transformation", C.c_float * 12),
                ("last_imu_pre_trans_available", C.c_int32)]


class GuessInfo(C.Structure):
    _fields_ = [("imuAvailable", C.c_int64), ("odomAvailable", C.c_int64), ("imuRollInit", C.c_float), ("imuPitchInit", C.c_float),
                ("imuYawInit", C.c_float), ("initialGuess", C.c_float * 6)]


class PgParams(C.Structure):
    _fields_ = [("prior_var", C.c_double * 6), ("odom_var", C.c_double * 6), ("sc_loop_var", C.c_double * 6),
                ("sc_loop_robust_k", C.c_double), ("relative_error_tol", C.c_double), ("absolute_error_tol", C.c_double),
                ("cg_rel_tol", C.c_double), ("max_iterations", C.c_int32), ("cg_max_iterations", C.c_int32)]


class PgResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("inner_iterations", C.c_int32), ("converged", C.c_int32), ("n_variables", C.c_int32),
                ("n_factors", C.c_int32), ("reserved", C.c_int32), ("error_before", C.c_double), ("error_after", C.c_double),
                ("robust_weight_min", C.c_double)]


class PgConsistencyParams(C.Structure):
    """s2m_pg_consistency_params: the tolerances at zero chain length and their growth per metre of chain (translation in metres,
    rotation as a chord 2 sin(angle / 2)).  The defaults are a starting point that has not been measured on real data."""
    _fields_ = [("tol_m", C.c_double), ("tol_chord", C.c_double), ("rate_m", C.c_double), ("rate_chord", C.c_double),
                ("reserved", C.c_int32 * 4)]


class PgConsistencyResult(C.Structure):
    """s2m_pg_consistency_result: the counts, the candidate the winning set was grown from, the set bits of the matrix / 2."""
    _fields_ = [("n_candidates", C.c_int32), ("n_selected", C.c_int32), ("start", C.c_int32), ("reserved", C.c_int32),
                ("n_consistent_pairs", C.c_int64)]


class PgCgOut(C.Structure):
    """s2m_debug_pg_cg_out (include/liorf_s2m_debug.h)."""
    _fields_ = [("rr", C.c_double), ("bb", C.c_double), ("iters", C.c_int32), ("stop", C.c_int32)]


class SessionInfo(C.Structure):
    """s2m_session_info: what a session blob holds."""
    _fields_ = [("version", C.c_uint32), ("n_keys", C.c_int32), ("n_descriptors", C.c_int32), ("n_loop_pairs", C.c_int32),
                ("n_variables", C.c_int32), ("n_factors", C.c_int32), ("n_points", C.c_uint64), ("bytes", C.c_uint64)]


class SessionAppendInfo(C.Structure):
    """s2m_session_append_info: what the appended blob held, the first new key, the junction's index in the factor list (-1: none)."""
    _fields_ = [("blob", SessionInfo), ("first_key", C.c_int32), ("junction_factor", C.c_int32)]


SESSION_WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
SESSION_READ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


class BatchLoop(C.Structure):
    """s2m_debug_batch_loop (include/liorf_s2m_debug.h)."""
    _fields_ = [("wpb", C.c_int32), ("nslots", C.c_int32), ("nblocks", C.c_int32), ("fused", C.c_int32), ("first_split", C.c_int32)]


class BatchLast(C.Structure):
    """s2m_debug_batch_last_out (include/liorf_s2m_debug.h)."""
    _fields_ = [("n_scans", C.c_int32), ("n_live", C.c_int32),
                ("ctx_launches", C.c_int32), ("init_launches", C.c_int32), ("prep_launches", C.c_int32),
                ("ranges_issued", C.c_int32), ("graph_cached", C.c_int32), ("n_loops", C.c_int32), ("loop", BatchLoop * 2)]


class KfSelectOut(C.Structure):
    """s2m_debug_kf_select_out (include/liorf_s2m_debug.h)."""
    _fields_ = [("path", C.c_int32), ("n_cand", C.c_int32), ("n_cent", C.c_int32), ("n_frames", C.c_int32), ("n_points", C.c_int64),
                ("cent_cap", C.c_size_t), ("cent", C.POINTER(C.c_float)), ("nn", C.POINTER(C.c_int32)),
                ("frames_cap", C.c_size_t), ("keys", C.POINTER(C.c_int32)), ("offsets", C.POINTER(C.c_int32))]


class S2MError(RuntimeError):
    """`code` is the status the library returned, where one did."""
    code = None


_LIB = None


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  The PyTorch-ROCm wheel ships its own libamdhip64.so (soname
    libamdhip64.so.7) and looks it up by file name; if libliorf_s2m.so has already pulled in
    /opt/rocm's copy, a later `import torch` loads a second runtime that sees no GPU.  Loading the
    wheel's copy first (without importing torch) makes both sides resolve to the same runtime, in
    either import order.  Without a PyTorch wheel the system runtime is used as linked."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(p):
        C.CDLL(p, mode=C.RTLD_GLOBAL)


def load_library(path: str | None = None) -> C.CDLL:
    """Load libliorf_s2m.so and declare the ABI. Raises if the HIP library is missing."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise S2MError(f"{p} not found: build it with __graft_entry__.build() "
                       f"(make -C liorf_amd/csrc); there is no CPU fallback")
    _share_hip_runtime_with_torch()
    L = C.CDLL(p)
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    L.s2m_version.restype = C.c_char_p
    L.s2m_last_error.restype = C.c_char_p
    L.s2m_last_error.argtypes = [vp]
    L.s2m_default_params.argtypes = [C.POINTER(Params)]
    L.s2m_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.s2m_destroy.argtypes = [vp]
    L.s2m_set_params.argtypes = [vp, C.POINTER(Params)]
    L.s2m_get_params.argtypes = [vp, C.POINTER(Params)]
    for n in ("s2m_set_map", "s2m_set_map_device", "s2m_set_scan", "s2m_set_scan_device"):
        getattr(L, n).argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.s2m_optimize.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, C.POINTER(ImuInit), C.POINTER(Result)]
    L.s2m_optimize_resident.argtypes = [vp, fp, C.POINTER(ImuInit), C.POINTER(Result)]
    L.s2m_optimize_launch.argtypes = [vp, fp]
    L.s2m_optimize_collect.argtypes = [vp, fp, C.POINTER(ImuInit), C.POINTER(Result)]
    L.s2m_get_trace.argtypes = [vp, C.POINTER(IterTrace), C.c_int]
    L.s2m_optimize_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, fp, C.POINTER(ImuInit), C.POINTER(Result)]
    L.s2m_batch_set_scan.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_int]
    L.s2m_slot_set_scan.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_int]
    L.s2m_slot_optimize_launch.argtypes = [vp, C.c_int, fp]
    L.s2m_slot_optimize_collect.argtypes = [vp, C.c_int, fp, C.POINTER(ImuInit), C.POINTER(Result)]
    L.s2m_batch_set_scans.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int]
    L.s2m_optimize_batch_launch.argtypes = [vp, C.c_int, fp]
    L.s2m_optimize_batch_collect.argtypes = [vp, C.c_int, fp, C.POINTER(ImuInit), C.POINTER(Result)]
    L.s2m_batch_get_trace.argtypes = [vp, C.c_int, C.POINTER(IterTrace), C.c_int]
    L.s2m_surf_optimization.argtypes = [vp, fp, C.POINTER(C.c_int32), fp, C.POINTER(C.c_uint8), fp]
    L.s2m_normal_eq.argtypes = [vp, fp, fp, fp, C.POINTER(C.c_int32)]
    L.s2m_last_timing.argtypes = [vp, fp, fp, fp]
    L.s2m_debug_deferred.argtypes = [vp, C.c_int]
    L.s2m_time_iteration_kernel.argtypes = [vp, fp, C.c_int, fp]
    L.s2m_time_iterations.argtypes = [vp, fp, C.c_int, fp, C.c_int]
    L.s2m_debug_wave_profile.argtypes = [vp, fp, C.c_int, C.POINTER(C.c_uint64), C.c_size_t]
    L.s2m_debug_time_steady.argtypes = [vp, fp, C.c_int, C.c_int, fp]
    L.s2m_time_loop_launches.argtypes = [vp, fp, C.c_int, fp]
    L.s2m_debug_scan_prep.argtypes = [vp, C.c_int32, fp, C.POINTER(C.c_int32), fp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.s2m_make_scancontext.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    szp = C.POINTER(C.c_size_t)
    for n in ("s2m_voxel_downsample", "s2m_voxel_downsample_device"):
        getattr(L, n).argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_float, vp, C.c_size_t, C.c_size_t, szp]
    L.s2m_downsample_scan.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, C.c_size_t, szp]
    L.s2m_extract_cloud.argtypes = [vp, C.c_int, C.POINTER(vp), szp, C.c_size_t, C.c_int, fp, C.c_float,
                                    vp, C.c_size_t, C.c_size_t, szp]
    L.s2m_transform_cloud.argtypes = [vp, vp, C.c_size_t, C.c_size_t, fp, vp, C.c_size_t]
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.s2m_debug_device_trig.argtypes = [vp, fp, C.c_size_t, fp, fp, fp]
    L.s2m_debug_device_hypot.argtypes = [vp, fp, fp, C.c_size_t, fp]
    L.s2m_debug_lm_close.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int, fp, C.c_int, fp, C.POINTER(LmCloseOut)]
    L.s2m_debug_lm_close_check_args.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, fp, fp, C.POINTER(LmCloseOut)]
    L.s2m_debug_lm_rows.argtypes = [vp, fp, C.c_int, dp, C.c_int, C.POINTER(LmRowsOut), i32p]
    L.s2m_debug_lm_rows_check_args.argtypes = [fp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.POINTER(LmRowsOut)]
    L.s2m_icp_default_params.argtypes = [C.POINTER(IcpParams)]
    L.s2m_icp_align.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.POINTER(IcpParams), C.POINTER(IcpResult)]
    L.s2m_icp_align_guess.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, fp, C.POINTER(IcpParams), C.POINTER(IcpResult)]
    L.s2m_sc_reset.argtypes = [vp]
    L.s2m_sc_size.argtypes = [vp]
    L.s2m_sc_add_scan.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.s2m_sc_add_descriptor.argtypes = [vp, dp]
    L.s2m_sc_detect_loop.argtypes = [vp, i32p, fp, C.POINTER(ScMatch)]
    L.s2m_sc_distance.argtypes = [vp, C.c_int32, i32p, C.c_int32, dp, i32p]
    qp, hp = C.POINTER(ScQueryParams), C.POINTER(ScHit)
    L.s2m_sc_query_default_params.argtypes = [qp]
    L.s2m_sc_query_check_args.argtypes = [C.c_int32, qp]
    L.s2m_sc_query_key.argtypes = [vp, C.c_int32, qp, hp, i32p]
    L.s2m_sc_query_descriptor.argtypes = [vp, dp, qp, hp, i32p]
    L.s2m_sc_query_scan.argtypes = [vp, vp, C.c_size_t, C.c_size_t, qp, hp, i32p]
    L.s2m_sc_query_projected.argtypes = [vp, qp, hp, i32p]
    mp = C.POINTER(ScQueryManyParams)
    L.s2m_sc_query_many_default_params.argtypes = [mp]
    L.s2m_sc_query_many_check_args.argtypes = [C.c_int32, C.c_int32, mp, C.c_int32]
    L.s2m_sc_query_keys.argtypes = [vp, i32p, C.c_int32, mp, hp, i32p]
    L.s2m_sc_query_descriptors.argtypes = [vp, dp, C.c_int32, mp, hp, i32p]
    L.s2m_sc_get_descriptors.argtypes = [vp, C.c_int32, C.c_int32, dp]
    L.s2m_debug_sc_query_many_pass.argtypes = [vp, C.c_int32]
    L.s2m_debug_sc_query_many_shape.argtypes = [i32p, i32p]
    L.s2m_debug_sc_query_many_last.argtypes = [vp, i32p, C.POINTER(C.c_size_t)]
    rp, nbp = C.POINTER(ScRingParams), C.POINTER(ScRingNeighbour)
    L.s2m_sc_ring_default_params.argtypes = [rp]
    L.s2m_sc_ring_check_args.argtypes = [C.c_int32, C.c_int32, rp, C.c_int32]
    L.s2m_sc_ring_neighbours_keys.argtypes = [vp, i32p, C.c_int32, rp, nbp, i32p]
    L.s2m_sc_ring_neighbours_descriptors.argtypes = [vp, dp, C.c_int32, rp, nbp, i32p]
    L.s2m_sc_query_keys_ring.argtypes = [vp, i32p, C.c_int32, rp, hp, i32p]
    L.s2m_sc_query_descriptors_ring.argtypes = [vp, dp, C.c_int32, rp, hp, i32p]
    L.s2m_debug_sc_ring_pass.argtypes = [vp, C.c_int32]
    L.s2m_debug_sc_ring_shape.argtypes = [i32p, i32p, i32p]
    L.s2m_debug_sc_ring_last.argtypes = [vp, i32p, C.POINTER(C.c_size_t)]
    L.s2m_kf_default_params.argtypes = [C.POINTER(KfParams)]
    L.s2m_kf_reset.argtypes = [vp]
    L.s2m_kf_size.argtypes = [vp]
    L.s2m_kf_add.argtypes = [vp, fp, C.c_double, vp, C.c_size_t, C.c_size_t, C.c_int]
    L.s2m_kf_set_poses.argtypes = [vp, C.c_int, C.c_int, fp]
    L.s2m_extract_surrounding.argtypes = [vp, C.c_double, C.POINTER(KfParams), vp, C.c_size_t, C.c_size_t, szp, i32p,
                                          C.c_size_t, szp]
    L.s2m_extract_surrounding_at.argtypes = [vp, fp, C.POINTER(KfParams), vp, C.c_size_t, C.c_size_t, szp, i32p, C.c_size_t, szp]
    L.s2m_loop_default_params.argtypes = [C.POINTER(LoopParams)]
    L.s2m_loop_near_keyframes.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_float, vp, C.c_size_t, C.c_size_t, szp]
    L.s2m_loop_align.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(LoopParams), C.POINTER(LoopResult)]
    L.s2m_loop_closure_rs.argtypes = [vp, C.c_double, C.POINTER(LoopParams), C.POINTER(LoopResult)]
    L.s2m_loop_align_launch.argtypes = L.s2m_loop_align.argtypes
    L.s2m_loop_closure_rs_launch.argtypes = L.s2m_loop_closure_rs.argtypes
    L.s2m_loop_poll.argtypes = [vp, C.POINTER(LoopResult)]
    L.s2m_loop_collect.argtypes = [vp, C.POINTER(LoopResult)]
    L.s2m_loop_verify_check_args.argtypes = [C.c_int32, C.c_int32, i32p, C.c_int32, C.c_int32, C.POINTER(LoopParams)]
    L.s2m_loop_verify_launch.argtypes = [vp, C.c_int32, i32p, C.c_int32, C.c_int32, C.POINTER(LoopParams), C.POINTER(LoopResult), i32p]
    L.s2m_loop_verify.argtypes = L.s2m_loop_verify_launch.argtypes
    L.s2m_loop_verify_poll.argtypes = [vp, C.POINTER(LoopResult), C.c_int32, i32p, i32p]
    L.s2m_loop_verify_collect.argtypes = L.s2m_loop_verify_poll.argtypes
    L.s2m_loop_verify_many_check_args.argtypes = [C.c_int32, i32p, i32p, i32p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(LoopParams)]
    L.s2m_loop_verify_many.argtypes = [vp, i32p, i32p, i32p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(LoopParams), C.POINTER(LoopResult), i32p]
    L.s2m_debug_icp_align_pairs_device.argtypes = [vp, C.POINTER(C.c_void_p), szp, C.POINTER(C.c_void_p), szp, C.c_int32, C.c_size_t,
                                                   C.POINTER(C.c_void_p), C.POINTER(IcpParams), C.POINTER(IcpResult)]
    L.s2m_debug_loop_verify_many_pass.argtypes = [vp, C.c_int32]
    L.s2m_debug_loop_verify_many_last.argtypes = [vp, i32p, i32p, szp]
    L.s2m_debug_loop_verify_many_plan.argtypes = [i32p, C.c_int32, C.c_int32, i32p, i32p]
    ldp = C.POINTER(LoopDetectParams)
    L.s2m_loop_detect_default_params.argtypes = [ldp]
    L.s2m_loop_detect_keys_check_args.argtypes = [C.c_int32, i32p, C.c_int32, C.c_int, ldp]
    L.s2m_loop_detect_keys.argtypes = [vp, i32p, dp, C.c_int32, ldp, i32p, fp, i32p]
    L.s2m_debug_loop_detect_pass.argtypes = [vp, C.c_int32]
    L.s2m_debug_loop_detect_splits.argtypes = [vp, C.c_int32]
    L.s2m_debug_loop_detect_shape.argtypes = [i32p, i32p, i32p]
    L.s2m_debug_loop_detect_last.argtypes = [vp, i32p, szp]
    L.s2m_debug_batch_last.argtypes = [vp, C.POINTER(BatchLast)]
    L.s2m_debug_icp_align_many_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_void_p), szp, C.c_int32, C.c_size_t, C.POINTER(IcpParams),
                                                  C.POINTER(IcpResult)]
    L.s2m_debug_icp_align_guess_many_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_void_p), szp, fp, C.c_int32, C.c_size_t,
                                                        C.POINTER(IcpParams), C.POINTER(IcpResult)]
    L.s2m_reloc_default_params.argtypes = [C.POINTER(RelocParams)]
    L.s2m_relocalize_check_args.argtypes = [C.c_int32, C.c_int32, C.POINTER(RelocParams)]
    L.s2m_relocalize_scan.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(RelocParams), C.POINTER(RelocCandidate), i32p, i32p]
    L.s2m_debug_icp_nearest.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int32, vp, C.POINTER(C.c_int32)]
    L.s2m_debug_icp_time_nearest.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, vp, C.POINTER(C.c_int32), fp, fp]
    L.s2m_debug_icp_align_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.POINTER(IcpParams), C.POINTER(IcpResult)]
    L.s2m_debug_icp_tuning.argtypes = [vp, C.c_float, C.c_int32, C.c_int32]
    L.s2m_debug_icp_close_check_args.argtypes = [C.c_int32, dp, vp, C.POINTER(IcpParams), vp]
    L.s2m_debug_icp_close.argtypes = [vp, C.c_int32, dp, vp, C.POINTER(IcpParams), vp]
    L.s2m_debug_icp_sums_check_args.argtypes = [C.POINTER(C.c_void_p), szp, C.POINTER(C.c_void_p), szp, C.c_int32, C.c_size_t, C.c_int32, dp,
                                                C.POINTER(C.c_int32)]
    L.s2m_debug_icp_sums.argtypes = [vp, C.POINTER(C.c_void_p), szp, C.POINTER(C.c_void_p), szp, C.c_int32, C.c_size_t, C.c_int32, C.c_double, dp,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.s2m_debug_icp_grid_check_args.argtypes = [C.POINTER(C.c_void_p), szp, C.c_int32, C.c_size_t, C.POINTER(IcpGridOut)]
    L.s2m_debug_icp_grid.argtypes = [vp, C.POINTER(C.c_void_p), szp, C.c_int32, C.c_size_t, C.POINTER(IcpGridOut), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.s2m_gmap_default_params.argtypes = [C.POINTER(GmapParams)]
    L.s2m_global_map.argtypes = [vp, C.POINTER(GmapParams), vp, C.c_size_t, C.c_size_t, szp, i32p, C.c_size_t, szp]
    L.s2m_kf_map_cloud.argtypes = [vp, C.c_int, C.c_int, C.c_float, vp, C.c_size_t, C.c_size_t, szp]
    L.s2m_scan_layout_preset.argtypes = [C.c_int32, C.POINTER(ScanLayout)]
    L.s2m_project_default_params.argtypes = [C.POINTER(ProjectParams)]
    L.s2m_imu_deskew_info.argtypes = [dp, C.c_size_t, C.c_double, C.c_double, dp, dp, dp, dp, i32p, i32p]
    L.s2m_project_check_args.argtypes = [C.POINTER(ScanLayout), C.POINTER(ProjectParams), C.POINTER(DeskewInfo)]
    L.s2m_project_scan.argtypes = [vp, vp, C.c_size_t, C.POINTER(ScanLayout), C.c_int, C.POINTER(ProjectParams),
                                   C.POINTER(DeskewInfo), vp, C.c_size_t, C.c_size_t, szp]
    L.s2m_downsample_projected.argtypes = [vp, C.c_float, vp, C.c_size_t, C.c_size_t, szp]
    L.s2m_sc_add_projected.argtypes = [vp]
    L.s2m_odom_deskew_info.argtypes = [C.POINTER(OdomSample), C.c_size_t, C.c_double, C.c_double, C.c_float, C.POINTER(OdomDeskew)]
    L.s2m_project_check_args_motion.argtypes = [C.POINTER(ScanLayout), C.POINTER(ProjectParams), C.POINTER(DeskewInfo), C.POINTER(MotionInfo)]
    L.s2m_project_scan_motion.argtypes = [vp, vp, C.c_size_t, C.POINTER(ScanLayout), C.c_int, C.POINTER(ProjectParams),
                                          C.POINTER(DeskewInfo), C.POINTER(MotionInfo), vp, C.c_size_t, C.c_size_t, szp]
    L.s2m_guess_state_init.argtypes = [C.POINTER(GuessState)]
    L.s2m_pg_default_params.argtypes = [C.POINTER(PgParams)]
    L.s2m_pg_check_args.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp, dp, C.c_double]
    L.s2m_pg_reset.argtypes = [vp]
    L.s2m_pg_size.argtypes = [vp, i32p, i32p]
    L.s2m_pg_add_prior.argtypes = [vp, C.c_int32, fp, dp]
    L.s2m_pg_add_between.argtypes = [vp, C.c_int32, C.c_int32, fp, dp, C.c_double]
    L.s2m_pg_add_gps.argtypes = [vp, C.c_int32, fp, dp]
    L.s2m_pg_set_initial.argtypes = [vp, C.c_int32, fp]
    L.s2m_pg_add_odometry.argtypes = [vp, fp]
    L.s2m_pg_optimize.argtypes = [vp, C.POINTER(PgParams), C.POINTER(PgResult)]
    L.s2m_pg_optimize_launch.argtypes = [vp, C.POINTER(PgParams), C.POINTER(PgResult)]
    L.s2m_pg_optimize_poll.argtypes = [vp, C.POINTER(PgResult)]
    L.s2m_pg_optimize_collect.argtypes = [vp, C.POINTER(PgResult)]
    L.s2m_debug_pg_rebase.argtypes = [dp, dp, dp]
    L.s2m_debug_pg_set_estimate.argtypes = [vp, C.c_int32, dp]
    L.s2m_debug_pg_linearize.argtypes = [vp, C.c_int32, C.c_int32] + [dp] * 10
    L.s2m_debug_pg_apply.argtypes = [vp, C.c_int32, C.c_int32, dp, dp]
    L.s2m_debug_pg_apply_check_args.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, dp]
    L.s2m_debug_pg_cg.argtypes = [vp, C.POINTER(PgParams), C.c_int32, dp, dp, C.POINTER(PgCgOut)]
    L.s2m_debug_pg_retract.argtypes = [vp, C.c_int32, dp, dp]
    L.s2m_pg_get_poses.argtypes = [vp, C.c_int32, C.c_int32, fp]
    L.s2m_pg_marginal.argtypes = [vp, C.c_int32, dp]
    L.s2m_pg_apply_to_store.argtypes = [vp, C.c_int32, C.c_int32]
    L.s2m_pg_marginals_check_args.argtypes = [C.c_int32, i32p, C.c_int32]
    L.s2m_pg_marginals.argtypes = [vp, i32p, C.c_int32, dp]
    L.s2m_pg_joint_marginal.argtypes = [vp, C.c_int32, C.c_int32, dp]
    L.s2m_pg_consistency_default_params.argtypes = [C.POINTER(PgConsistencyParams)]
    L.s2m_pg_consistency_check_args.argtypes = [C.c_int32, i32p, i32p, fp, C.c_int32, C.POINTER(PgConsistencyParams)]
    L.s2m_pg_consistent_loops.argtypes = [vp, i32p, i32p, fp, C.c_int32, C.POINTER(PgConsistencyParams), C.POINTER(C.c_uint8), i32p,
                                          C.POINTER(C.c_uint64), C.POINTER(PgConsistencyResult)]
    L.s2m_update_initial_guess.argtypes = [C.POINTER(GuessState), C.POINTER(C.c_float), C.c_int, C.POINTER(GuessInfo), C.c_int, C.c_int,
                                           C.POINTER(C.c_float)]
    L.s2m_session_info_of.argtypes = [vp, C.POINTER(SessionInfo)]
    L.s2m_session_save.argtypes = [vp, SESSION_WRITE_FN, vp]
    L.s2m_session_load.argtypes = [vp, SESSION_READ_FN, vp, C.POINTER(SessionInfo)]
    L.s2m_session_save_file.argtypes = [vp, C.c_char_p]
    L.s2m_session_load_file.argtypes = [vp, C.c_char_p, C.POINTER(SessionInfo)]
    L.s2m_session_check.argtypes = [vp, C.c_size_t, C.POINTER(SessionInfo)]
    L.s2m_debug_session_chunk.argtypes = [vp, C.c_size_t]
    L.s2m_session_append_check_args.argtypes = [C.POINTER(SessionInfo), C.POINTER(SessionInfo), fp, dp]
    L.s2m_session_append.argtypes = [vp, SESSION_READ_FN, vp, fp, dp, C.POINTER(SessionAppendInfo)]
    L.s2m_session_append_file.argtypes = [vp, C.c_char_p, fp, dp, C.POINTER(SessionAppendInfo)]
    L.s2m_session_place.argtypes = [vp, fp]
    L.s2m_relocalize_key.argtypes = [vp, C.c_int32, C.POINTER(RelocParams), C.POINTER(RelocCandidate), i32p, i32p]
    L.s2m_session_appended.argtypes = [vp, i32p, i32p]
    L.s2m_session_anchor_from_pairs.argtypes = [fp, fp, C.c_int32, C.c_double, C.c_double, fp, i32p, i32p]
    L.s2m_debug_sc_keys.argtypes = [vp, C.c_int32, C.c_int32, fp, dp]
    L.s2m_debug_kf_frame.argtypes = [vp, C.c_int32, fp, fp, fp, i32p]
    L.s2m_debug_kf_select_last.argtypes = [vp, C.POINTER(KfSelectOut)]
    L.s2m_debug_kf_select_last_check_args.argtypes = [C.POINTER(KfSelectOut)]
    if path is None:
        _LIB = L
    return L


def kernel_source_sha() -> str:
    """sha256 over the device code of the registration path (the kernel headers of liorf_amd/csrc): measurements kept under
    profiles/ are stamped with it so that bench.py can tell whether they were taken on the kernels it is running."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(_HERE, "csrc")
    for f in ("s2m_device.hpp", "s2m_prep.hpp", "s2m_kernels.hpp", "s2m_register.hpp", "s2m_types.h"):
        h.update(f.encode())
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def default_params(**kw) -> Params:
    p = Params()
    load_library().s2m_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def session_check(blob) -> SessionInfo:
    """s2m_session_check: structure, checksums and content of a session blob, on the host, without a handle or a GPU. Returns
    what it holds; raises S2MError (`code`: S2M_ERR_FORMAT or S2M_ERR_CHECKSUM) otherwise."""
    b = bytes(blob)
    out = SessionInfo()
    rc = load_library().s2m_session_check(b, len(b), C.byref(out))
    if rc != S2M_OK:
        e = S2MError(f"s2m_session_check: {ERRORS.get(rc, rc)}")
        e.code = rc
        raise e
    return out


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _opt_f32(v, n=6):
    """(keep-alive array, pointer) of an optional float vector: None stays NULL."""
    if v is None:
        return None, None
    a = np.ascontiguousarray(v, np.float32).reshape(n)
    return a, _fp(a)


def _opt_f64(v, n=6):
    if v is None:
        return None, None
    a = np.ascontiguousarray(v, np.float64).reshape(n)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def session_append_check_args(have: SessionInfo, blob_info: SessionInfo, anchor=None, junction_var=None) -> int:
    """s2m_session_append_check_args: the precondition verdict of s2m_session_append from what the handle holds and what the
    blob's header states (host only, no handle, no GPU): S2M_OK or S2M_ERR_INVALID_ARG."""
    _a, pa = _opt_f32(anchor)
    _v, pv = _opt_f64(junction_var)
    return load_library().s2m_session_append_check_args(C.byref(have) if have is not None else None,
                                                        C.byref(blob_info) if blob_info is not None else None, pa, pv)


def anchorFromPairs(pose_in_session, pose_in_map, tol_m: float = 1.0, tol_rad: float = 0.1):
    """s2m_session_anchor_from_pairs (host only): the anchor {x, y, z, roll, pitch, yaw} that most of the pairs (a pose of the
    session in its own frame, the same pose in the map's frame) agree on, its number of supporters and the pair it came from."""
    a = np.ascontiguousarray(pose_in_session, np.float32).reshape(-1, 6)
    b = np.ascontiguousarray(pose_in_map, np.float32).reshape(-1, 6)
    if a.shape != b.shape:
        raise ValueError("as many poses in the session as in the map")
    out = np.zeros(6, np.float32)
    n, chosen = C.c_int32(0), C.c_int32(-1)
    rc = load_library().s2m_session_anchor_from_pairs(_fp(a), _fp(b), a.shape[0], float(tol_m), float(tol_rad), _fp(out), C.byref(n), C.byref(chosen))
    if rc != S2M_OK:
        e = S2MError(f"s2m_session_anchor_from_pairs: {ERRORS.get(rc, rc)}")
        e.code = rc
        raise e
    return out, n.value, chosen.value


def _records(a) -> tuple[np.ndarray, int, int]:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("points must be (n, >=3) float32 records")
    return a, a.shape[0], a.shape[1] * 4


class MapOptimizationS2M:
    """The scan-to-map slice of the reference's mapOptimization node, on one MI355X."""

    def __init__(self, **params):
        self.lib = load_library()
        self.params = default_params(**params)
        h = C.c_void_p()
        rc = self.lib.s2m_create(C.byref(self.params), C.byref(h))
        if rc != S2M_OK:
            raise S2MError(f"s2m_create failed: {ERRORS.get(rc, rc)} (no gfx950 device or HIP error; no CPU fallback)")
        self.h = h
        self.transformTobeMapped = np.zeros(6, np.float32)     # reference :134
        self.isDegenerate = False                              # reference :139
        self.incrementalOdometryAffineBack = np.zeros((3, 4), np.float32)   # reference :157
        self.incrementalOdometryAffineFront = np.zeros((3, 4), np.float32)  # reference :156
        self.guessState = GuessState()                         # the three function statics of updateInitialGuess() (:904, :920-921)
        self.lib.s2m_guess_state_init(C.byref(self.guessState))
        self.laserCloudSurfLastDSNum = 0
        self.last_result: Result | None = None

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.s2m_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != S2M_OK:
            msg = self.lib.s2m_last_error(self.h)
            e = S2MError(f"{what}: {ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}")
            e.code = rc
            raise e

    def setParams(self, **kw):
        """s2m_set_params: the ParamServer values the path reads at every call in the reference
        (z_tol, rot_tol, imu_type, imu_rpy_weight) and the loop constants, changed after construction."""
        for k, v in kw.items():
            setattr(self.params, k, v)
        self._check(self.lib.s2m_set_params(self.h, C.byref(self.params)), "s2m_set_params")

    # -- inputs ------------------------------------------------------------
    def setInputCloud(self, laserCloudSurfFromMapDS):
        """kdtreeSurfFromMap->setInputCloud(laserCloudSurfFromMapDS) (reference :1302)."""
        a, n, st = _records(laserCloudSurfFromMapDS)
        self._check(self.lib.s2m_set_map(self.h, a.ctypes.data, n, st), "s2m_set_map")

    def setScan(self, laserCloudSurfLastDS):
        a, n, st = _records(laserCloudSurfLastDS)
        self._check(self.lib.s2m_set_scan(self.h, a.ctypes.data, n, st), "s2m_set_scan")
        self.laserCloudSurfLastDSNum = n

    def setScanDevice(self, d_ptr: int, n: int, stride_bytes: int):
        """s2m_set_scan_device: the scan already lives in HBM (asynchronous; the buffer must stay
        valid until the next synchronising call, e.g. collect())."""
        self._check(self.lib.s2m_set_scan_device(self.h, C.c_void_p(d_ptr), n, stride_bytes), "s2m_set_scan_device")
        self.laserCloudSurfLastDSNum = n

    def setInputCloudDevice(self, d_ptr: int, n: int, stride_bytes: int):
        self._check(self.lib.s2m_set_map_device(self.h, C.c_void_p(d_ptr), n, stride_bytes), "s2m_set_map_device")

    # -- the voxel-grid stages that feed the path -------
    def _check_voxel(self, rc: int, what: str) -> bool:
        """True when PCL's "leaf size is too small" case was hit (output = input)."""
        if rc == S2M_WARN_LEAF_TOO_SMALL:
            return True
        self._check(rc, what)
        return False

    def voxelGrid(self, cloud, leaf: float) -> np.ndarray:
        """downSizeFilter.setInputCloud(cloud); .filter(out): (m, 8) float32 PointXYZI records."""
        a, n, st = _records(cloud)
        out = np.zeros((max(n, 1), 8), np.float32)
        m = C.c_size_t(0)
        self.leaf_too_small = self._check_voxel(
            self.lib.s2m_voxel_downsample(self.h, a.ctypes.data, n, st, leaf, out.ctypes.data, 32, n, C.byref(m)),
            "s2m_voxel_downsample")
        return out[:m.value]

    def voxelGridDevice(self, d_in: int, n: int, stride_bytes: int, leaf: float, d_out: int, cap: int) -> int:
        """Both clouds in HBM (32-byte output records); returns the number of voxels."""
        m = C.c_size_t(0)
        self.leaf_too_small = self._check_voxel(
            self.lib.s2m_voxel_downsample_device(self.h, C.c_void_p(d_in), n, stride_bytes, leaf, C.c_void_p(d_out), 32,
                                                 cap, C.byref(m)), "s2m_voxel_downsample_device")
        return m.value

    def downsampleCurrentScan(self, laserCloudSurfLast, leaf: float, readback: bool = True, device_ptr=None):
        """Reference :1061-1067, fused with setScan: returns laserCloudSurfLastDS (or None if !readback).
        `device_ptr=(ptr, n, stride_bytes)` filters a cloud that already lives in HBM."""
        if device_ptr is not None:
            ptr, n, st = device_ptr
            src, on_dev = C.c_void_p(ptr), 1
        else:
            a, n, st = _records(laserCloudSurfLast)
            src, on_dev = a.ctypes.data, 0
        out = np.zeros((max(n, 1), 8), np.float32) if readback else None
        m = C.c_size_t(0)
        self.leaf_too_small = self._check_voxel(
            self.lib.s2m_downsample_scan(self.h, src, n, st, on_dev, leaf, out.ctypes.data if readback else None, 32,
                                         n if readback else 0, C.byref(m)), "s2m_downsample_scan")
        self.laserCloudSurfLastDSNum = m.value
        return out[:m.value] if readback else None

    def extractCloud(self, frames, poses_xyzrpy, leaf: float, readback: bool = True, device_frames=None):
        """Reference :1014-1039 for already selected key frames, fused with setInputCloud: transform every
        frame by its key pose {x, y, z, roll, pitch, yaw}, concatenate, voxel-filter, build the map index.
        `device_frames=[(ptr, n), ...]` with `frames=stride_bytes` uses clouds that already live in HBM."""
        poses = np.ascontiguousarray(poses_xyzrpy, np.float32).reshape(-1, 6)
        if device_frames is not None:
            st = int(frames)
            ptrs = (C.c_void_p * len(device_frames))(*[C.c_void_p(p) for p, _ in device_frames])
            sizes = (C.c_size_t * len(device_frames))(*[n for _, n in device_frames])
            nf, on_dev, keep = len(device_frames), 1, None
        else:
            keep = [_records(f) for f in frames]
            st = keep[0][2] if keep else 32
            if any(k[2] != st for k in keep):
                raise ValueError("all key-frame clouds must share one record stride")
            ptrs = (C.c_void_p * len(keep))(*[C.c_void_p(k[0].ctypes.data) for k in keep])
            sizes = (C.c_size_t * len(keep))(*[k[1] for k in keep])
            nf, on_dev = len(keep), 0
        if poses.shape[0] != nf:
            raise ValueError("one key pose per frame")
        total = int(sum(sizes))
        out = np.zeros((max(total, 1), 8), np.float32) if readback else None
        m = C.c_size_t(0)
        self.leaf_too_small = self._check_voxel(
            self.lib.s2m_extract_cloud(self.h, nf, ptrs, sizes, st, on_dev, _fp(poses), leaf,
                                       out.ctypes.data if readback else None, 32, total if readback else 0, C.byref(m)),
            "s2m_extract_cloud")
        self.laserCloudSurfFromMapDSNum = m.value
        return out[:m.value] if readback else None

    def transformPointCloud(self, cloudIn, pose_xyzrpy) -> np.ndarray:
        """Reference :310-329 (PointTypePose order x, y, z, roll, pitch, yaw)."""
        a, n, st = _records(cloudIn)
        out = np.zeros((max(n, 1), 8), np.float32)
        p = np.ascontiguousarray(pose_xyzrpy, np.float32)
        self._check(self.lib.s2m_transform_cloud(self.h, a.ctypes.data, n, st, _fp(p), out.ctypes.data, 32),
                    "s2m_transform_cloud")
        return out[:n]

    # -- the resident cloud_deskewed of an ImageProjectionS2M on this handle ------------------------------
    def downsampleCurrentScanProjected(self, leaf: float, readback: bool = True, cloud_num: int | None = None):
        """downsampleCurrentScan() (reference :1061-1067) on the cloud_deskewed the last projectPointCloud() left on the
        device (s2m_downsample_projected): returns laserCloudSurfLastDS, or None if !readback. cloud_num is that projection's
        count (the filter never returns more); ImageProjectionS2M.projectPointCloud() records it on this object."""
        m = C.c_size_t(0)
        if not readback:
            self.leaf_too_small = self._check_voxel(
                self.lib.s2m_downsample_projected(self.h, leaf, None, 32, 0, C.byref(m)), "s2m_downsample_projected")
            self.laserCloudSurfLastDSNum = m.value
            return None
        if cloud_num is None:
            cloud_num = getattr(self, "cloudDeskewedNum", None)
        if cloud_num is None:
            raise ValueError("cloud_num: the count of the projection (s2m_project_scan's n_out) sizes the host buffer")
        out = np.zeros((max(int(cloud_num), 1), 8), np.float32)
        self.leaf_too_small = self._check_voxel(
            self.lib.s2m_downsample_projected(self.h, leaf, out.ctypes.data, 32, int(cloud_num), C.byref(m)), "s2m_downsample_projected")
        self.laserCloudSurfLastDSNum = m.value
        return out[:m.value]

    def makeAndSaveScancontextAndKeysProjected(self):
        """makeAndSaveScancontextAndKeys(cloud_deskewed) (reference :1591-1594) from the resident buffer."""
        self._check(self.lib.s2m_sc_add_projected(self.h), "s2m_sc_add_projected")

    # -- the path ----------------------------------------------------------
    def updateInitialGuess(self, cloudInfo: GuessInfo, key_poses_empty: bool | None = None, useImuHeadingInitialization: bool = False) -> np.ndarray:
        """updateInitialGuess() (reference :899-958, s2m_update_initial_guess, host code): transformTobeMapped becomes the
        pose scan2MapOptimization() starts from and incrementalOdometryAffineFront the transform before the update.
        key_poses_empty defaults to the resident key-frame store being empty (cloudKeyPoses3D->points.empty(), :906)."""
        if key_poses_empty is None:
            key_poses_empty = self.kfSize() == 0
        pose = np.ascontiguousarray(self.transformTobeMapped, np.float32).copy()
        front = np.zeros(12, np.float32)
        self._check(self.lib.s2m_update_initial_guess(C.byref(self.guessState), _fp(pose), 1 if key_poses_empty else 0, C.byref(cloudInfo),
                                                      1 if useImuHeadingInitialization else 0, int(self.params.imu_type), _fp(front)),
                    "s2m_update_initial_guess")
        self.transformTobeMapped = pose
        self.incrementalOdometryAffineFront = front.reshape(3, 4)
        return pose

    def scan2MapOptimization(self, imu: ImuInit | None = None) -> Result:
        """Reference :1295-1321 on the resident scan and map; updates transformTobeMapped."""
        r = Result()
        pose = np.ascontiguousarray(self.transformTobeMapped, np.float32)
        self._check(self.lib.s2m_optimize_resident(self.h, _fp(pose), C.byref(imu) if imu is not None else None,
                                                   C.byref(r)), "s2m_optimize_resident")
        self.transformTobeMapped = pose
        self.isDegenerate = bool(r.is_degenerate)
        self.incrementalOdometryAffineBack = np.array(r.affine, np.float32).reshape(3, 4)
        self.last_result = r
        return r

    def optimize(self, scan, pose, imu: ImuInit | None = None) -> Result:
        """s2m_optimize on host buffers (upload + loop)."""
        a, n, st = _records(scan)
        p = np.ascontiguousarray(pose, np.float32).copy()
        r = Result()
        self._check(self.lib.s2m_optimize(self.h, a.ctypes.data, n, st, _fp(p),
                                          C.byref(imu) if imu is not None else None, C.byref(r)), "s2m_optimize")
        self.transformTobeMapped = p
        self.isDegenerate = bool(r.is_degenerate)
        self.laserCloudSurfLastDSNum = n
        self.last_result = r
        return r

    def launch(self, pose):
        p = np.ascontiguousarray(pose, np.float32)
        self._check(self.lib.s2m_optimize_launch(self.h, _fp(p)), "s2m_optimize_launch")

    def collect(self, imu: ImuInit | None = None) -> Result:
        r = Result()
        p = np.zeros(6, np.float32)
        self._check(self.lib.s2m_optimize_collect(self.h, _fp(p), C.byref(imu) if imu is not None else None,
                                                  C.byref(r)), "s2m_optimize_collect")
        self.transformTobeMapped = p
        self.isDegenerate = bool(r.is_degenerate)
        self.last_result = r
        return r

    # -- a batch of scans against the resident map (BASELINE config 4 on one GPU) ---------------------
    def batchSetScan(self, slot: int, scan=None, device_ptr=None):
        """Install scan `slot` of the batch: host records, or device_ptr=(ptr, n, stride_bytes)."""
        if device_ptr is not None:
            ptr, n, st = device_ptr
            self._check(self.lib.s2m_batch_set_scan(self.h, slot, C.c_void_p(ptr), n, st, 1), "s2m_batch_set_scan")
        else:
            a, n, st = _records(scan)
            self._check(self.lib.s2m_batch_set_scan(self.h, slot, a.ctypes.data, n, st, 0), "s2m_batch_set_scan")

    # -- a stream of scans: preparation of the next scan overlaps the loop of the current one (two slots) ------
    def slotSetScan(self, slot: int, scan=None, device_ptr=None):
        if device_ptr is not None:
            ptr, n, st = device_ptr
            self._check(self.lib.s2m_slot_set_scan(self.h, slot, C.c_void_p(ptr), n, st, 1), "s2m_slot_set_scan")
        else:
            a, n, st = _records(scan)
            self._check(self.lib.s2m_slot_set_scan(self.h, slot, a.ctypes.data, n, st, 0), "s2m_slot_set_scan")

    def slotLaunch(self, slot: int, pose):
        p = np.ascontiguousarray(pose, np.float32).reshape(6)
        self._check(self.lib.s2m_slot_optimize_launch(self.h, slot, _fp(p)), "s2m_slot_optimize_launch")

    def slotCollect(self, slot: int, imu=None):
        r = Result()
        p = np.zeros(6, np.float32)
        self._check(self.lib.s2m_slot_optimize_collect(self.h, slot, _fp(p), C.byref(imu) if imu is not None else None, C.byref(r)),
                    "s2m_slot_optimize_collect")
        return p, r

    def batchSetScans(self, scans=None, device_ptrs=None):
        """Install slots 0 .. n-1 at once (s2m_batch_set_scans): host records, or device_ptrs=[(ptr, n, stride_bytes), ...]."""
        if device_ptrs is not None:
            n = len(device_ptrs)
            st = device_ptrs[0][2]
            ptrs = (C.c_void_p * n)(*[C.c_void_p(d[0]) for d in device_ptrs])
            sizes = (C.c_size_t * n)(*[d[1] for d in device_ptrs])
            self._check(self.lib.s2m_batch_set_scans(self.h, n, ptrs, sizes, st, 1), "s2m_batch_set_scans")
        else:
            keep = [_records(sc) for sc in scans]
            n = len(keep)
            st = keep[0][2]
            if any(k[2] != st for k in keep):
                raise ValueError("all scans of a batch must share one record stride")
            ptrs = (C.c_void_p * n)(*[C.c_void_p(k[0].ctypes.data) for k in keep])
            sizes = (C.c_size_t * n)(*[k[1] for k in keep])
            self._check(self.lib.s2m_batch_set_scans(self.h, n, ptrs, sizes, st, 0), "s2m_batch_set_scans")

    def batchLaunch(self, poses):
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        self._batch_n = p.shape[0]
        self._check(self.lib.s2m_optimize_batch_launch(self.h, p.shape[0], _fp(p)), "s2m_optimize_batch_launch")

    def batchCollect(self, imus=None):
        n = self._batch_n
        poses = np.zeros((n, 6), np.float32)
        res = (Result * n)()
        im = None
        if imus is not None:
            im = (ImuInit * n)(*imus)
        self._check(self.lib.s2m_optimize_batch_collect(self.h, n, _fp(poses), im, res), "s2m_optimize_batch_collect")
        return poses, [res[k] for k in range(n)]

    def optimizeBatch(self, scans, poses, imus=None):
        """s2m_optimize_batch: n scan2MapOptimization() calls against the resident map in one graph; (poses, results)."""
        keep = [_records(sc) for sc in scans]
        n = len(keep)
        st = keep[0][2]
        if any(k[2] != st for k in keep):
            raise ValueError("all scans of a batch must share one record stride")
        ptrs = (C.c_void_p * n)(*[C.c_void_p(k[0].ctypes.data) for k in keep])
        sizes = (C.c_size_t * n)(*[k[1] for k in keep])
        p = np.ascontiguousarray(poses, np.float32).reshape(n, 6).copy()
        res = (Result * n)()
        im = (ImuInit * n)(*imus) if imus is not None else None
        self._check(self.lib.s2m_optimize_batch(self.h, n, ptrs, sizes, st, _fp(p), im, res), "s2m_optimize_batch")
        self._batch_n = n
        return p, [res[k] for k in range(n)]

    def batchLast(self) -> BatchLast:
        """s2m_debug_batch_last: what the last batchSetScans and batch launch / collect issued, noted where they issued it."""
        out = BatchLast()
        self._check(self.lib.s2m_debug_batch_last(self.h, C.byref(out)), "s2m_debug_batch_last")
        return out

    def batchTrace(self, slot: int) -> list[IterTrace]:
        buf = (IterTrace * 64)()
        n = self.lib.s2m_batch_get_trace(self.h, slot, buf, 64)
        return [buf[i] for i in range(max(n, 0))]

    def trace(self) -> list[IterTrace]:
        buf = (IterTrace * 64)()
        n = self.lib.s2m_get_trace(self.h, buf, 64)
        return [buf[i] for i in range(max(n, 0))]

    # -- observation hooks -----------------------------------------------------
    def surfOptimization(self, pose):
        """One surfOptimization() pass (reference :1074-1143); outputs in original scan order."""
        n = self.laserCloudSurfLastDSNum
        p = np.ascontiguousarray(pose, np.float32)
        idx = np.full((n, 5), -1, np.int32)
        d2 = np.zeros((n, 5), np.float32)
        flag = np.zeros(n, np.uint8)
        coeff = np.zeros((n, 4), np.float32)
        self._check(self.lib.s2m_surf_optimization(self.h, _fp(p), idx.ctypes.data_as(C.POINTER(C.c_int32)), _fp(d2),
                                                   flag.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(coeff)),
                    "s2m_surf_optimization")
        return idx, d2, flag, coeff

    def normal_eq(self, pose):
        p = np.ascontiguousarray(pose, np.float32)
        AtA = np.zeros((6, 6), np.float32)
        AtB = np.zeros(6, np.float32)
        n = C.c_int32(0)
        self._check(self.lib.s2m_normal_eq(self.h, _fp(p), _fp(AtA), _fp(AtB), C.byref(n)), "s2m_normal_eq")
        return AtA, AtB, n.value

    def deviceTrig(self, x):
        """Observation hook: (sinf, cosf, atanf) of the float32 array x as the device computes them."""
        a = np.ascontiguousarray(x, np.float32)
        sn, cs, at = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
        self._check(self.lib.s2m_debug_device_trig(self.h, _fp(a), a.size, _fp(sn), _fp(cs), _fp(at)), "s2m_debug_device_trig")
        return sn, cs, at

    def deviceHypot(self, x, y):
        """Observation hook: hypotf(x, y) of two float32 arrays as the device computes it in cv::eigen's rotations."""
        a, b = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
        assert a.shape == b.shape
        r = np.zeros_like(a)
        self._check(self.lib.s2m_debug_device_hypot(self.h, _fp(a), _fp(b), a.size, _fp(r)), "s2m_debug_device_hypot")
        return r

    def lmClose(self, form: int, it: int, rows, pose0, degen_in: int, matP_in) -> LmCloseOut:
        """Observation hook: close LM iteration `it` on the partial rows `rows` (n x 28 float64); see s2m_debug_lm_close."""
        r = np.ascontiguousarray(rows, np.float64).reshape(-1, 28)
        p = np.ascontiguousarray(pose0, np.float32).reshape(6)
        m = np.ascontiguousarray(matP_in, np.float32).reshape(36)
        out = LmCloseOut()
        self._check(self.lib.s2m_debug_lm_close(self.h, form, it, r.ctypes.data_as(C.POINTER(C.c_double)), r.shape[0], _fp(p),
                                                int(degen_in), _fp(m), C.byref(out)), "s2m_debug_lm_close")
        return out

    def lmRows(self, pose, launch: int = 0, table: bool = True):
        """Observation hook: the partial rows registration launch `launch` wrote (0: the first launch of a scan at `pose`;
        N > 0: launch N of a real loop from `pose`); see s2m_debug_lm_rows. Returns (rows (n_rows_active, 28) float64,
        LmRowsOut, wave table (n_waves, 2) int32 or None)."""
        p = np.ascontiguousarray(pose, np.float32).reshape(6)
        cap = 512                                              # (kMaxBlocks: no scan has more active workgroups)
        rows = np.zeros((cap, 28), np.float64)
        wt = np.zeros(((self.laserCloudSurfLastDSNum + 63) // 64 * 12 + 64, 2), np.int32) if table else None
        out = LmRowsOut()
        self._check(self.lib.s2m_debug_lm_rows(self.h, _fp(p), int(launch), rows.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(out),
                                               None if wt is None else wt.ctypes.data_as(C.POINTER(C.c_int32))), "s2m_debug_lm_rows")
        return rows[:out.n_rows_active].copy(), out, None if wt is None else wt[:out.n_waves].copy()

    def scanPrep(self, chain: int = 0, pose=None) -> dict:
        """Observation hook: run the preparation of the resident scan again (chain 0 = as setScan / launch do, 1 = the
        six-kernel chain, -1 = nothing) and read back what it left; see s2m_debug_scan_prep."""
        n = self.laserCloudSurfLastDSNum
        nc = (n + 63) // 64
        i32 = C.POINTER(C.c_int32)
        qperm = np.zeros(n, np.int32)
        qxyz = np.zeros((3, n), np.float32)
        parts, factor = np.zeros(nc, np.int32), np.zeros(nc, np.int32)
        table = np.zeros((nc * 12 + 64, 2), np.int32)
        nw = C.c_int32(0)
        p = None if pose is None else np.ascontiguousarray(pose, np.float32)
        self._check(self.lib.s2m_debug_scan_prep(self.h, int(chain), None if p is None else _fp(p), qperm.ctypes.data_as(i32), _fp(qxyz),
                                                 parts.ctypes.data_as(i32), factor.ctypes.data_as(i32), table.ctypes.data_as(i32),
                                                 C.byref(nw)), "s2m_debug_scan_prep")
        return dict(qperm=qperm, qxyz=qxyz, chunk_parts=parts, chunk_factor=factor, wave_table=table[:max(nw.value, 0)].copy(),
                    n_waves=nw.value)

    def timing(self):
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        self.lib.s2m_last_timing(self.h, C.byref(a), C.byref(b), C.byref(c))
        return dict(optimize_ms=a.value, set_map_ms=b.value, set_scan_ms=c.value)

    def time_iteration_kernel(self, pose, reps: int = 200) -> float:
        p = np.ascontiguousarray(pose, np.float32)
        ms = C.c_float(0)
        self._check(self.lib.s2m_time_iteration_kernel(self.h, _fp(p), reps, C.byref(ms)), "s2m_time_iteration_kernel")
        return ms.value

    def time_iterations(self, pose, reps: int = 10) -> np.ndarray:
        """Mean k_register duration (ms) of every launch of the loop, index = LM iteration."""
        p = np.ascontiguousarray(pose, np.float32)
        out = np.zeros(64, np.float32)
        self._check(self.lib.s2m_time_iterations(self.h, _fp(p), reps, _fp(out), 64), "s2m_time_iterations")
        return out[:self.params.max_iter]

    def time_loop_launches(self, pose, reps: int = 10) -> float:
        """Mean k_register launch duration (us) over whole LM loops, four HIP-event pairs per loop (s2m_time_loop_launches)."""
        p = np.ascontiguousarray(pose, np.float32)
        us = C.c_float(0)
        self._check(self.lib.s2m_time_loop_launches(self.h, _fp(p), reps, C.byref(us)), "s2m_time_loop_launches")
        return us.value

    def time_steady(self, pose, reps: int = 200, solve_prev: bool = True) -> float:
        """Diagnostics: microseconds per replayed steady-state launch (s2m_debug_time_steady)."""
        p = np.ascontiguousarray(pose, np.float32)
        us = C.c_float(0)
        self._check(self.lib.s2m_debug_time_steady(self.h, _fp(p), reps, 1 if solve_prev else 0, C.byref(us)), "s2m_debug_time_steady")
        return us.value

    def wave_profile(self, pose, launches: int = 3) -> np.ndarray:
        """Diagnostics: (n_waves, 32) uint64 per-wave stamps/stats of one k_register pass (include/liorf_s2m.h);
        launches < 0 records launch number -launches of a real LM loop."""
        p = np.ascontiguousarray(pose, np.float32)
        cap = (self.laserCloudSurfLastDSNum + 15) // 16 + 256
        out = np.zeros((cap, 32), np.uint64)
        n = self.lib.s2m_debug_wave_profile(self.h, _fp(p), launches, out.ctypes.data_as(C.POINTER(C.c_uint64)), cap)
        if n < 0:
            self._check(n, "s2m_debug_wave_profile")
        return out[:n]

    # -- ICP loop-closure alignment (reference src/mapOptmization.cpp:571-586), SURVEY.md section 8(f) row F4 --
    def icpAlign(self, cureKeyframeCloud, prevKeyframeCloud, **params):
        """icp.setInputSource(cure); icp.setInputTarget(prev); icp.align(): (T 4x4, hasConverged, getFitnessScore, iterations)."""
        a, na, st = _records(cureKeyframeCloud)
        b, nb, st2 = _records(prevKeyframeCloud)
        if st != st2:
            raise ValueError("both clouds must share one record stride")
        p = IcpParams()
        self.lib.s2m_icp_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        r = IcpResult()
        self._check(self.lib.s2m_icp_align(self.h, a.ctypes.data, na, b.ctypes.data, nb, st, C.byref(p), C.byref(r)), "s2m_icp_align")
        return np.array(r.T, np.float32).reshape(4, 4), bool(r.converged), r.fitness_score, r.iterations

    @staticmethod
    def _guess_arg(guess):
        """A row-major 4x4 as the float pointer s2m_icp_align_guess takes (None: a null pointer, the identity)."""
        if guess is None:
            return None, None
        g = np.ascontiguousarray(guess, np.float32).reshape(16)
        return g, _fp(g)

    def icpAlignGuess(self, cureKeyframeCloud, prevKeyframeCloud, guess=None, **params):
        """icp.align(output, guess): the alignment started at the 4x4 `guess` (None or the identity: icpAlign). The returned T
        includes the guess. (T 4x4, hasConverged, getFitnessScore, iterations)."""
        a, na, st = _records(cureKeyframeCloud)
        b, nb, st2 = _records(prevKeyframeCloud)
        if st != st2:
            raise ValueError("both clouds must share one record stride")
        p = IcpParams()
        self.lib.s2m_icp_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        r = IcpResult()
        g, gp = self._guess_arg(guess)
        self._check(self.lib.s2m_icp_align_guess(self.h, a.ctypes.data, na, b.ctypes.data, nb, st, gp, C.byref(p), C.byref(r)),
                    "s2m_icp_align_guess")
        return np.array(r.T, np.float32).reshape(4, 4), bool(r.converged), r.fitness_score, r.iterations

    # -- SCManager (reference include/Scancontext.cpp), SURVEY.md section 8(f) row F3 --------------
    def scReset(self):
        self._check(self.lib.s2m_sc_reset(self.h), "s2m_sc_reset")

    def scSize(self) -> int:
        return self.lib.s2m_sc_size(self.h)

    def makeAndSaveScancontextAndKeys(self, scan_down):
        """Reference :236-250: descriptor + ring key + sector key of the cloud, appended to the device store."""
        a, n, st = _records(scan_down)
        self._check(self.lib.s2m_sc_add_scan(self.h, a.ctypes.data, n, st), "s2m_sc_add_scan")

    def scAddDescriptor(self, desc):
        d = np.ascontiguousarray(desc, np.float64).reshape(20, 60)
        self._check(self.lib.s2m_sc_add_descriptor(self.h, d.ctypes.data_as(C.POINTER(C.c_double))), "s2m_sc_add_descriptor")

    def detectLoopClosureID(self):
        """Reference :253-344: (loop_id, yaw_diff_rad, ScMatch with the intermediate values)."""
        lid, yaw, m = C.c_int32(-1), C.c_float(0), ScMatch()
        self._check(self.lib.s2m_sc_detect_loop(self.h, C.byref(lid), C.byref(yaw), C.byref(m)), "s2m_sc_detect_loop")
        return lid.value, yaw.value, m

    def distanceBtnScanContext(self, query_idx: int, cand_idx):
        """Reference :116-148 for stored key frames, batched over the candidates: (dist[m], shift[m])."""
        c = np.ascontiguousarray(cand_idx, np.int32)
        dist = np.zeros(len(c), np.float64)
        shift = np.zeros(len(c), np.int32)
        self._check(self.lib.s2m_sc_distance(self.h, query_idx, c.ctypes.data_as(C.POINTER(C.c_int32)), len(c),
                                             dist.ctypes.data_as(C.POINTER(C.c_double)),
                                             shift.ctypes.data_as(C.POINTER(C.c_int32))), "s2m_sc_distance")
        return dist, shift

    # -- the place query: a descriptor against every stored key of a range, the K nearest under a threshold
    def _sc_query(self, fn, what, args, params, kw):
        p = params if params is not None else default_sc_query_params()
        if kw:
            p = default_sc_query_params(**{**{f: getattr(p, f) for f, _ in ScQueryParams._fields_}, **kw})
        hits = np.zeros(S2M_SC_QUERY_MAX_K, SC_HIT_DTYPE)
        n = C.c_int32(0)
        self._check(fn(self.h, *args, C.byref(p), hits.ctypes.data_as(C.POINTER(ScHit)), C.byref(n)), what)
        return hits[:n.value].copy()

    def scQueryKey(self, key: int, params: "ScQueryParams | None" = None, **kw):
        """s2m_sc_query_key: the hits (SC_HIT_DTYPE records, ascending (dist, key)) of stored key `key`; keyword arguments set
        fields of the parameters."""
        return self._sc_query(self.lib.s2m_sc_query_key, "s2m_sc_query_key", (int(key),), params, kw)

    def scQueryDescriptor(self, desc, params: "ScQueryParams | None" = None, **kw):
        d = np.ascontiguousarray(desc, np.float64).reshape(20, 60)
        return self._sc_query(self.lib.s2m_sc_query_descriptor, "s2m_sc_query_descriptor", (d.ctypes.data_as(C.POINTER(C.c_double)),), params, kw)

    def scQueryScan(self, scan, params: "ScQueryParams | None" = None, **kw):
        a, n, st = _records(scan)
        return self._sc_query(self.lib.s2m_sc_query_scan, "s2m_sc_query_scan", (a.ctypes.data, n, st), params, kw)

    def scQueryProjected(self, params: "ScQueryParams | None" = None, **kw):
        """The query with the descriptor of the cloud s2m_project_scan left on the device."""
        return self._sc_query(self.lib.s2m_sc_query_projected, "s2m_sc_query_projected", (), params, kw)

    # -- the place query for many queries at once
    @staticmethod
    def _sc_queries(queries, descs: bool):
        """The queries of a many-query call - stored keys, or (m, 20, 60) descriptors - as a contiguous array and its pointer."""
        a = np.ascontiguousarray(queries, np.float64).reshape(-1, 20, 60) if descs else np.ascontiguousarray(queries, np.int32).reshape(-1)
        return a, a.ctypes.data_as(C.POINTER(C.c_double if descs else C.c_int32))

    def _sc_query_rows(self, what, queries, descs, params, kw, defaults_fn, fields_fn, width_fn, rec_dtype, rec_ctype):
        """One row of at most width_fn(parameters) records per query from the library call `what`."""
        p = params if params is not None else defaults_fn()
        if kw:
            p = defaults_fn(**{**fields_fn(p), **kw})
        a, ptr = self._sc_queries(queries, descs)
        m = len(a)
        rows = np.zeros((max(m, 1), max(int(width_fn(p)), 1)), rec_dtype)
        n = np.zeros(max(m, 1), np.int32)
        self._check(getattr(self.lib, what)(self.h, ptr, m, C.byref(p), rows.ctypes.data_as(C.POINTER(rec_ctype)),
                                            n.ctypes.data_as(C.POINTER(C.c_int32))), what)
        return [rows[i, :n[i]].copy() for i in range(m)]

    def _sc_query_many(self, what, queries, descs, params, kw):
        return self._sc_query_rows(what, queries, descs, params, kw, default_sc_query_many_params, _sc_many_fields, lambda p: p.q.top_k,
                                   SC_HIT_DTYPE, ScHit)

    def scQueryKeys(self, keys, params: "ScQueryManyParams | None" = None, **kw):
        """s2m_sc_query_keys: for every stored key of `keys` its hits (SC_HIT_DTYPE records, ascending (dist, key)), each row what
        scQueryKey returns for the same searched set.  Keyword arguments set fields of the single query's parameters, and
        rel_lo / rel_hi the window around each query's own key that is left out as well."""
        return self._sc_query_many("s2m_sc_query_keys", keys, False, params, kw)

    def scQueryDescriptors(self, descs, params: "ScQueryManyParams | None" = None, **kw):
        """s2m_sc_query_descriptors: the same for descriptors from elsewhere, (m, 20, 60) doubles."""
        return self._sc_query_many("s2m_sc_query_descriptors", descs, True, params, kw)

    def scGetDescriptors(self, first: int = 0, count: "int | None" = None):
        """s2m_sc_get_descriptors: the stored descriptors first .. first+count-1 as (count, 20, 60) doubles, bit for bit what was added."""
        if count is None:
            count = self.scSize() - first
        out = np.zeros((max(count, 0), 20, 60), np.float64)
        self._check(self.lib.s2m_sc_get_descriptors(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_double))), "s2m_sc_get_descriptors")
        return out

    def _sessionLoopRows(self, gap, max_dist, top_k, align, ring_candidates):
        """Every stored key against the keys at least `gap` before it: exhaustively (ring_candidates=None), or against its
        ring_candidates ring-key neighbours among them."""
        keys = np.arange(self.scSize(), dtype=np.int32)
        kw = dict(top_k=top_k, align=align, max_dist=max_dist, rel_lo=1 - int(gap), rel_hi=2**31 - 1)
        if ring_candidates is None:
            return self.scQueryKeys(keys, **kw)
        return self.scQueryKeysRing(keys, n_candidates=int(ring_candidates), **kw)

    def findSessionLoops(self, gap: int = 30, max_dist: float = 0.3, top_k: int = 1, align: int = S2M_SC_ALIGN_FULL, ring_candidates=None):
        """Every stored key against the keys at least `gap` before it: the (key_cur, key_pre, dist, yaw_diff_rad) candidates a node
        hands to loopVerify, in key_cur order and per key in (dist, key_pre) order.  ring_candidates=C compares every key with its
        C ring-key neighbours only (scQueryKeysRing) instead of with all of them."""
        rows = self._sessionLoopRows(gap, max_dist, top_k, align, ring_candidates)
        return [(cur, int(h["key"]), float(h["dist"]), float(h["yaw_diff_rad"])) for cur, row in enumerate(rows) for h in row]

    # -- the place query behind a ring-key prefilter
    def _sc_ring(self, what, queries, descs, params, kw, both):
        """both: the rows of hits behind the prefilter; else the neighbour lists."""
        shape = (lambda p: p.m.q.top_k, SC_HIT_DTYPE, ScHit) if both else (lambda p: p.n_candidates, SC_RING_NEIGHBOUR_DTYPE, ScRingNeighbour)
        return self._sc_query_rows(what, queries, descs, params, kw, default_sc_ring_params, _sc_ring_fields, *shape)

    def scRingNeighboursKeys(self, keys, params: "ScRingParams | None" = None, **kw):
        """s2m_sc_ring_neighbours_keys: for every stored key of `keys` its n_candidates ring-key neighbours in its searched set
        (SC_RING_NEIGHBOUR_DTYPE records, ascending (d2, key)).  Keyword arguments set n_candidates and the many-query's fields."""
        return self._sc_ring("s2m_sc_ring_neighbours_keys", keys, False, params, kw, False)

    def scRingNeighboursDescriptors(self, descs, params: "ScRingParams | None" = None, **kw):
        """s2m_sc_ring_neighbours_descriptors: the same for descriptors from elsewhere, (m, 20, 60) doubles."""
        return self._sc_ring("s2m_sc_ring_neighbours_descriptors", descs, True, params, kw, False)

    def scQueryKeysRing(self, keys, params: "ScRingParams | None" = None, **kw):
        """s2m_sc_query_keys_ring: scQueryKeys with every query's searched set cut to its n_candidates ring-key neighbours."""
        return self._sc_ring("s2m_sc_query_keys_ring", keys, False, params, kw, True)

    def scQueryDescriptorsRing(self, descs, params: "ScRingParams | None" = None, **kw):
        """s2m_sc_query_descriptors_ring: the same for descriptors from elsewhere, (m, 20, 60) doubles."""
        return self._sc_ring("s2m_sc_query_descriptors_ring", descs, True, params, kw, True)

    def scRingPass(self, queries_per_pass: int):
        """s2m_debug_sc_ring_pass: at most this many queries per pass of the ring calls (0: the default)."""
        self._check(self.lib.s2m_debug_sc_ring_pass(self.h, queries_per_pass), "s2m_debug_sc_ring_pass")

    def scRingLast(self):
        """s2m_debug_sc_ring_last: (passes, device bytes of one pass) of the last ring call."""
        n, b = C.c_int32(0), C.c_size_t(0)
        self._check(self.lib.s2m_debug_sc_ring_last(self.h, C.byref(n), C.byref(b)), "s2m_debug_sc_ring_last")
        return n.value, b.value

    def scQueryManyPass(self, queries_per_pass: int):
        """s2m_debug_sc_query_many_pass: at most this many queries per pass (0: the default)."""
        self._check(self.lib.s2m_debug_sc_query_many_pass(self.h, queries_per_pass), "s2m_debug_sc_query_many_pass")

    def scQueryManyLast(self):
        """s2m_debug_sc_query_many_last: (passes, device bytes of one pass) of the last many-query."""
        n, b = C.c_int32(0), C.c_size_t(0)
        self._check(self.lib.s2m_debug_sc_query_many_last(self.h, C.byref(n), C.byref(b)), "s2m_debug_sc_query_many_last")
        return n.value, b.value

    def makeScancontext(self, scan):
        """SCManager::makeScancontext + makeRingkeyFromScancontext (reference include/Scancontext.cpp:151-211)."""
        a, n, st = _records(scan)
        desc = np.zeros((20, 60), np.float64)
        key = np.zeros(20, np.float64)
        self._check(self.lib.s2m_make_scancontext(self.h, a.ctypes.data, n, st,
                                                  desc.ctypes.data_as(C.POINTER(C.c_double)),
                                                  key.ctypes.data_as(C.POINTER(C.c_double))), "s2m_make_scancontext")
        return desc, key

    # -- the resident key-frame store and extractSurroundingKeyFrames() (reference :1046-1059) --------
    def kfReset(self):
        self._check(self.lib.s2m_kf_reset(self.h), "s2m_kf_reset")

    def kfSize(self) -> int:
        return self.lib.s2m_kf_size(self.h)

    def saveKeyFrame(self, pose_xyzrpy, time: float, cloud=None, device_ptr=None):
        """saveKeyFramesAndFactor() (reference :1549-1580): append a key frame with pose {x, y, z, roll, pitch, yaw}.
        cloud=None stores laserCloudSurfLastDS as the last downsampleCurrentScan left it (no copy through the host);
        `device_ptr=(ptr, n, stride_bytes)` copies records that live in HBM."""
        p = np.ascontiguousarray(pose_xyzrpy, np.float32).reshape(6)
        if device_ptr is not None:
            ptr, n, st = device_ptr
            rc = self.lib.s2m_kf_add(self.h, _fp(p), float(time), C.c_void_p(ptr), n, st, S2M_KF_FROM_DEVICE)
        elif cloud is None:
            rc = self.lib.s2m_kf_add(self.h, _fp(p), float(time), None, 0, 32, S2M_KF_FROM_LAST_DOWNSAMPLE)
        else:
            a, n, st = _records(cloud)
            rc = self.lib.s2m_kf_add(self.h, _fp(p), float(time), a.ctypes.data, n, st, S2M_KF_FROM_HOST)
        self._check(rc, "s2m_kf_add")

    def correctPoses(self, poses_xyzrpy, first: int = 0):
        """correctPoses() (reference :1611-1640): new poses for key frames first .. first + len(poses) - 1."""
        p = np.ascontiguousarray(poses_xyzrpy, np.float32).reshape(-1, 6)
        self._check(self.lib.s2m_kf_set_poses(self.h, first, p.shape[0], _fp(p)), "s2m_kf_set_poses")

    def extractSurroundingKeyFrames(self, timeLaserInfoCur: float, params: KfParams | None = None, readback: bool = True,
                                    return_map: bool = False):
        """Reference :1046-1059 on the resident store, fused with setInputCloud: returns the key id of every frame
        concatenated into the local map (or None if !readback); with return_map also laserCloudSurfFromMapDS."""
        n = max(self.kfSize(), 0)
        keys = np.zeros(2 * n + 1, np.int32)
        m, nk = C.c_size_t(0), C.c_size_t(0)
        pp = C.byref(params) if params is not None else None

        def run(out, cap):
            return self._check_voxel(
                self.lib.s2m_extract_surrounding(self.h, float(timeLaserInfoCur), pp, out, 32, cap, C.byref(m),
                                                 keys.ctypes.data_as(C.POINTER(C.c_int32)) if readback else None,
                                                 keys.size if readback else 0, C.byref(nk)), "s2m_extract_surrounding")
        self.leaf_too_small = run(None, 0)
        self.laserCloudSurfFromMapDSNum = m.value
        k = keys[:nk.value].copy() if readback else None
        if not return_map:
            return k
        out = np.zeros((max(m.value, 1), 8), np.float32)
        run(out.ctypes.data, m.value)                 # (the same selection again: deterministic, same map)
        return k, out[:m.value]

    def extractSurroundingKeyFramesAt(self, centre_xyz, params: KfParams | None = None, readback: bool = True, return_map: bool = False):
        """s2m_extract_surrounding_at: extractSurroundingKeyFrames around `centre_xyz` instead of the newest key, without the
        recent keys, installed as the local map. Returns as extractSurroundingKeyFrames does."""
        n = max(self.kfSize(), 0)
        keys = np.zeros(2 * n + 1, np.int32)
        m, nk = C.c_size_t(0), C.c_size_t(0)
        pp = C.byref(params) if params is not None else None
        c = np.ascontiguousarray(centre_xyz, np.float32).reshape(3)

        def run(out, cap):
            return self._check_voxel(
                self.lib.s2m_extract_surrounding_at(self.h, _fp(c), pp, out, 32, cap, C.byref(m),
                                                    keys.ctypes.data_as(C.POINTER(C.c_int32)) if readback else None,
                                                    keys.size if readback else 0, C.byref(nk)), "s2m_extract_surrounding_at")
        self.leaf_too_small = run(None, 0)
        self.laserCloudSurfFromMapDSNum = m.value
        k = keys[:nk.value].copy() if readback else None
        if not return_map:
            return k
        out = np.zeros((max(m.value, 1), 8), np.float32)
        run(out.ctypes.data, m.value)                 # (the same selection again: deterministic, same map)
        return k, out[:m.value]

    # -- relocalisation: a scan that is no key against the stored map ---------------------------------------------
    def relocalizeScan(self, scan, params: "RelocParams | None" = None, device_ptr=None):
        """s2m_relocalize_scan: (records, best). records are the query's hits in its order, each aligned from
        T(pose[key]) * Rz(-yaw); best is the accepted record with the least (fitness, position), or -1.
        `device_ptr=(ptr, n, stride_bytes)` takes a scan that already lives in HBM."""
        if device_ptr is not None:
            ptr, n, st = device_ptr
            src, on_dev = C.c_void_p(ptr), 1
        else:
            a, n, st = _records(scan)
            src, on_dev = a.ctypes.data, 0
        recs = (RelocCandidate * S2M_LOOP_MAX_CANDIDATES)()
        n_out, best = C.c_int32(0), C.c_int32(-1)
        pp = C.byref(params) if params is not None else None
        self._check(self.lib.s2m_relocalize_scan(self.h, src, n, st, on_dev, pp, recs, C.byref(n_out), C.byref(best)), "s2m_relocalize_scan")
        return [_copy_struct(recs[i]) for i in range(n_out.value)], best.value

    def relocalizeKey(self, key: int, params: "RelocParams | None" = None):
        """s2m_relocalize_key: relocalizeScan for a key the store holds - its stored descriptor as the query, its own records
        as the source, target submaps clamped to the query's searched range. (records, best)."""
        recs = (RelocCandidate * S2M_LOOP_MAX_CANDIDATES)()
        n_out, best = C.c_int32(0), C.c_int32(-1)
        pp = C.byref(params) if params is not None else None
        self._check(self.lib.s2m_relocalize_key(self.h, key, pp, recs, C.byref(n_out), C.byref(best)), "s2m_relocalize_key")
        return [_copy_struct(recs[i]) for i in range(n_out.value)], best.value

    def mergeSession(self, path_or_blob, probe_keys, reloc: "RelocParams | None" = None, tol_m: float = 1.0, tol_rad: float = 0.1,
                     junction_var=None, probe_poses=None):
        """The first half of the merge workflow: append the saved session unplaced, relocalise the
        keys `probe_keys` of it (indices in the appended session) against the keys the handle held, take the anchor most of
        the accepted ones agree on, and place the session by it. Returns (append info, anchor or None, supporters); with no
        accepted probe the session stays as stored (anchor None). probe_poses: the probes' poses in the session's own frame
        (None: the appended graph's estimates, which the blob must hold for them). The caller goes on with scQueryKeys of [N0, N) against
        first = 0, count = N0, loopVerifyMany, pgAddBetween, pgOptimize and pgApplyToStore."""
        if isinstance(path_or_blob, (bytes, bytearray, memoryview)):
            info = self.sessionAppend(blob=bytes(path_or_blob), junction_var=junction_var)
        else:
            info = self.sessionAppendFile(path_or_blob, junction_var=junction_var)
        n0 = info.first_key
        prm = reloc if reloc is not None else default_reloc_params()
        prm.query.first, prm.query.count = 0, n0
        in_session, in_map = [], []
        for i, k in enumerate(probe_keys):
            if probe_poses is None and int(k) >= info.blob.n_variables:
                raise ValueError("a probe key without a pose-graph variable needs probe_poses")
            recs, best = self.relocalizeKey(n0 + int(k), prm)
            if best >= 0:
                in_session.append(np.array(probe_poses[i] if probe_poses is not None else self.pgPoses(n0 + int(k), 1)[0], np.float32))
                in_map.append(np.array(recs[best].pose_xyzrpy, np.float32))
        if not in_session:
            return info, None, 0
        anchor, n_in, _ = anchorFromPairs(in_session, in_map, tol_m, tol_rad)
        self.sessionPlace(anchor)
        return info, anchor, n_in

    def localizeInStoredMap(self, scan, reloc: "RelocParams | None" = None, kf: KfParams | None = None):
        """Start (or recover) inside the stored map: relocalise `scan`, install the local map around the best pose and set
        transformTobeMapped to it, so that downsampleCurrentScan + scan2MapOptimization track from there. Returns
        (pose_tobemapped, records, best), the pose None when no hit was accepted (nothing is installed then)."""
        recs, best = self.relocalizeScan(scan, reloc)
        if best < 0:
            return None, recs, best
        pose = np.array(recs[best].pose_tobemapped, np.float32)
        self.extractSurroundingKeyFramesAt(pose[3:6], kf, readback=False)
        self.transformTobeMapped = pose.copy()
        return pose, recs, best

    # -- saving and loading a session: key frames, descriptors, loop pairs, pose graph ------------------------------
    def session_info(self) -> SessionInfo:
        """s2m_session_info_of: what session_save() would write now."""
        out = SessionInfo()
        self._check(self.lib.s2m_session_info_of(self.h, C.byref(out)), "s2m_session_info_of")
        return out

    def session_save(self, write=None) -> bytes | None:
        """s2m_session_save: the session blob as bytes, or, with `write` (a callable taking each chunk as bytes, in stream
        order; an exception or a true return value fails the save), nothing."""
        parts = []

        def cb(_user, data, n):
            try:
                chunk = C.string_at(data, n)
                if write is None:
                    parts.append(chunk)
                    return 0
                return 1 if write(chunk) else 0
            except Exception:                           # (no exception crosses the C boundary)
                return 1
        self._check(self.lib.s2m_session_save(self.h, SESSION_WRITE_FN(cb), None), "s2m_session_save")
        return b"".join(parts) if write is None else None

    def session_load(self, blob=None, read=None) -> SessionInfo:
        """s2m_session_load into this handle, whose stores and pose graph must be empty: from `blob` (bytes), or from `read`,
        a callable (n) -> n bytes in stream order (fewer bytes, an exception or None fail the load). A blob that ends
        early is S2M_ERR_FORMAT."""
        buf = (C.c_char * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0") if blob is not None else None
        at = [0]

        def cb(_user, data, n):
            try:
                if buf is not None:
                    if at[0] + n > len(blob):
                        return S2M_ERR_FORMAT            # the stream has ended
                    C.memmove(data, C.addressof(buf) + at[0], n)
                    at[0] += n
                    return 0
                chunk = read(n)
                if chunk is None or len(chunk) != n:
                    return 1
                C.memmove(data, bytes(chunk), n)
                return 0
            except Exception:
                return 1
        out = SessionInfo()
        self._check(self.lib.s2m_session_load(self.h, SESSION_READ_FN(cb), None, C.byref(out)), "s2m_session_load")
        return out

    @staticmethod
    def _read_callback(blob, read):
        buf = (C.c_char * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0") if blob is not None else None
        at = [0]

        def cb(_user, data, n):
            try:
                if buf is not None:
                    if at[0] + n > len(blob):
                        return S2M_ERR_FORMAT            # the stream has ended
                    C.memmove(data, C.addressof(buf) + at[0], n)
                    at[0] += n
                    return 0
                chunk = read(n)
                if chunk is None or len(chunk) != n:
                    return 1
                C.memmove(data, bytes(chunk), n)
                return 0
            except Exception:
                return 1
        return SESSION_READ_FN(cb)

    def sessionAppend(self, blob=None, read=None, anchor=None, junction_var=None) -> SessionAppendInfo:
        """s2m_session_append: a saved session (`blob`, or `read` as session_load takes it) behind the stored keys, placed by
        `anchor` {x, y, z, roll, pitch, yaw} (None: as stored); the junction factor's variances (None: 1.0 x 6)."""
        _a, pa = _opt_f32(anchor)
        _v, pv = _opt_f64(junction_var)
        out = SessionAppendInfo()
        cb = self._read_callback(blob, read)
        self._check(self.lib.s2m_session_append(self.h, cb, None, pa, pv, C.byref(out)), "s2m_session_append")
        return out

    def sessionAppendFile(self, path: str, anchor=None, junction_var=None) -> SessionAppendInfo:
        _a, pa = _opt_f32(anchor)
        _v, pv = _opt_f64(junction_var)
        out = SessionAppendInfo()
        self._check(self.lib.s2m_session_append_file(self.h, os.fsencode(path), pa, pv, C.byref(out)), "s2m_session_append_file")
        return out

    def sessionPlace(self, move):
        """s2m_session_place: moves the session appended last by `move` {x, y, z, roll, pitch, yaw}."""
        a, pa = _opt_f32(move)
        self._check(self.lib.s2m_session_place(self.h, pa), "s2m_session_place")

    def sessionAppended(self) -> tuple[int, int]:
        """s2m_session_appended: (first key, count) of the session appended last; (-1, 0): none."""
        first, count = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.s2m_session_appended(self.h, C.byref(first), C.byref(count)), "s2m_session_appended")
        return first.value, count.value

    def session_save_file(self, path: str):
        self._check(self.lib.s2m_session_save_file(self.h, os.fsencode(path)), "s2m_session_save_file")

    def session_load_file(self, path: str) -> SessionInfo:
        out = SessionInfo()
        self._check(self.lib.s2m_session_load_file(self.h, os.fsencode(path), C.byref(out)), "s2m_session_load_file")
        return out

    def sessionChunk(self, chunk_bytes: int):
        """s2m_debug_session_chunk: the staging chunk of session_save / session_load (0: the default)."""
        self._check(self.lib.s2m_debug_session_chunk(self.h, chunk_bytes), "s2m_debug_session_chunk")

    def scKeys(self, first: int = 0, count: int | None = None):
        """s2m_debug_sc_keys: (ring keys (count, 20) float32, sector keys (count, 60) float64) as the store holds them."""
        if count is None:
            count = self.scSize() - first
        ring, sector = np.zeros((max(count, 0), 20), np.float32), np.zeros((max(count, 0), 60), np.float64)
        self._check(self.lib.s2m_debug_sc_keys(self.h, first, count, _fp(ring), _dp(sector)), "s2m_debug_sc_keys")
        return ring, sector

    def kfFrame(self, key: int):
        """s2m_debug_kf_frame: (T of the host mirror, T of the device's frame table, device position, device point count)."""
        th, td, pos, n = np.zeros(12, np.float32), np.zeros(12, np.float32), np.zeros(4, np.float32), C.c_int32(0)
        self._check(self.lib.s2m_debug_kf_frame(self.h, key, _fp(th), _fp(td), _fp(pos), C.byref(n)), "s2m_debug_kf_frame")
        return th, td, pos, n.value

    def kfSelectLast(self):
        """s2m_debug_kf_select_last: the stages of the handle's last key-frame selection as a dict - path, n_cand, n_cent, n_frames,
        n_points, cent (n_cent x 3 fp32), nn (n_cent), keys (n_frames), offsets (n_frames + 1)."""
        n = max(self.kfSize(), 0)
        cent, nn = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        keys, off = np.zeros(2 * n + 1, np.int32), np.zeros(2 * n + 2, np.int32)
        i32 = C.POINTER(C.c_int32)
        o = KfSelectOut(cent_cap=n, cent=_fp(cent), nn=nn.ctypes.data_as(i32), frames_cap=keys.size,
                        keys=keys.ctypes.data_as(i32), offsets=off.ctypes.data_as(i32))
        self._check(self.lib.s2m_debug_kf_select_last(self.h, C.byref(o)), "s2m_debug_kf_select_last")
        return {"path": o.path, "n_cand": o.n_cand, "n_cent": o.n_cent, "n_frames": o.n_frames, "n_points": o.n_points,
                "cent": cent[:o.n_cent].copy(), "nn": nn[:o.n_cent].copy(), "keys": keys[:o.n_frames].copy(),
                "offsets": off[:o.n_frames + 1].copy()}

    # -- the pose graph beside the store (reference :1386-1534, :1611-1642) --------
    def pgReset(self):
        self._check(self.lib.s2m_pg_reset(self.h), "s2m_pg_reset")
        self.aLoopIsClosed = False

    def pgSize(self) -> tuple[int, int]:
        nv, nf = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.s2m_pg_size(self.h, C.byref(nv), C.byref(nf)), "s2m_pg_size")
        return nv.value, nf.value

    def pgAddPrior(self, key: int, pose_xyzrpy, var):
        p, v = np.ascontiguousarray(pose_xyzrpy, np.float32).reshape(6), np.ascontiguousarray(var, np.float64).reshape(6)
        self._check(self.lib.s2m_pg_add_prior(self.h, key, _fp(p), _dp(v)), "s2m_pg_add_prior")

    def pgAddBetween(self, key_from: int, key_to: int, rel_xyzrpy, var, robust_k: float = 0.0):
        p, v = np.ascontiguousarray(rel_xyzrpy, np.float32).reshape(6), np.ascontiguousarray(var, np.float64).reshape(6)
        self._check(self.lib.s2m_pg_add_between(self.h, key_from, key_to, _fp(p), _dp(v), float(robust_k)), "s2m_pg_add_between")

    def pgAddGps(self, key: int, xyz, var):
        p, v = np.ascontiguousarray(xyz, np.float32).reshape(3), np.ascontiguousarray(var, np.float64).reshape(3)
        self._check(self.lib.s2m_pg_add_gps(self.h, key, _fp(p), _dp(v)), "s2m_pg_add_gps")

    def pgSetInitial(self, key: int, pose_xyzrpy):
        p = np.ascontiguousarray(pose_xyzrpy, np.float32).reshape(6)
        self._check(self.lib.s2m_pg_set_initial(self.h, key, _fp(p)), "s2m_pg_set_initial")

    def addOdomFactor(self, pose_xyzrpy):
        """addOdomFactor() (reference :1386-1400)."""
        p = np.ascontiguousarray(pose_xyzrpy, np.float32).reshape(6)
        self._check(self.lib.s2m_pg_add_odometry(self.h, _fp(p)), "s2m_pg_add_odometry")

    def addLoopFactor(self, key_cur: int, key_pre: int, pose_from, pose_to, var, robust_k: float = 0.0, rel=None):
        """addLoopFactor() (reference :1513-1534) for one queued closure: the between factor poseFrom.between(poseTo) of a
        LoopResult (RS: var = six times icp.fitness_score; SC: default_pg_params().sc_loop_var and .sc_loop_robust_k)."""
        if rel is None:                                  # (rel: the between pose itself, when the caller already holds it)
            rel = between_xyzrpy(pose_from, pose_to)
        self.pgAddBetween(key_cur, key_pre, rel, var, robust_k)
        self.aLoopIsClosed = True

    def pgOptimize(self, params: PgParams | None = None) -> PgResult:
        out = PgResult()
        self._check(self.lib.s2m_pg_optimize(self.h, C.byref(params) if params is not None else None, C.byref(out)), "s2m_pg_optimize")
        return out

    def _pg_code(self, rc: int, what: str) -> int:
        if rc not in (S2M_OK, S2M_PG_PENDING, S2M_PG_IDLE):
            self._check(rc, what)
        return rc

    def pgOptimizeLaunch(self, params: PgParams | None = None) -> tuple[int, PgResult]:
        """s2m_pg_optimize_launch: (S2M_PG_PENDING, the early result) with the solve queued beside the scan handler, or
        (S2M_OK, the synchronous result) for an empty graph."""
        out = PgResult()
        rc = self.lib.s2m_pg_optimize_launch(self.h, C.byref(params) if params is not None else None, C.byref(out))
        return self._pg_code(rc, "s2m_pg_optimize_launch"), out

    def pgOptimizePoll(self) -> tuple[int, PgResult]:
        """s2m_pg_optimize_poll: never waits for the device. (S2M_PG_PENDING, untouched), (S2M_OK, the result) once, or
        (S2M_PG_IDLE, untouched) with nothing pending."""
        out = PgResult()
        return self._pg_code(self.lib.s2m_pg_optimize_poll(self.h, C.byref(out)), "s2m_pg_optimize_poll"), out

    def pgOptimizeCollect(self) -> tuple[int, PgResult]:
        """s2m_pg_optimize_collect: waits. (S2M_OK, the result) or (S2M_PG_IDLE, untouched)."""
        out = PgResult()
        return self._pg_code(self.lib.s2m_pg_optimize_collect(self.h, C.byref(out)), "s2m_pg_optimize_collect"), out

    def pgPoses(self, first: int = 0, count: int | None = None) -> np.ndarray:
        if count is None:
            count = self.pgSize()[0] - first
        out = np.zeros((max(count, 0), 6), np.float32)
        self._check(self.lib.s2m_pg_get_poses(self.h, first, count, _fp(out)), "s2m_pg_get_poses")
        return out

    def pgMarginal(self, key: int) -> np.ndarray:
        cov = np.zeros((6, 6), np.float64)
        self._check(self.lib.s2m_pg_marginal(self.h, key, _dp(cov)), "s2m_pg_marginal")
        return cov

    def pgMarginals(self, keys) -> np.ndarray:
        """The marginals of `keys` (they may repeat) in one block solve: (len(keys), 6, 6), block k bitwise pgMarginal(keys[k])."""
        k = np.ascontiguousarray(keys, np.int32).reshape(-1)
        cov = np.zeros((k.shape[0], 6, 6), np.float64)
        self._check(self.lib.s2m_pg_marginals(self.h, k.ctypes.data_as(C.POINTER(C.c_int32)), k.shape[0], _dp(cov)), "s2m_pg_marginals")
        return cov

    def pgJointMarginal(self, key_a: int, key_b: int) -> np.ndarray:
        """The joint covariance of two keys, 12x12 over [key_a's tangent, key_b's tangent], not symmetrised."""
        cov = np.zeros((12, 12), np.float64)
        self._check(self.lib.s2m_pg_joint_marginal(self.h, key_a, key_b, _dp(cov)), "s2m_pg_joint_marginal")
        return cov

    def pgApplyToStore(self, first: int = 0, count: int | None = None):
        if count is None:
            count = self.pgSize()[0] - first
        self._check(self.lib.s2m_pg_apply_to_store(self.h, first, count), "s2m_pg_apply_to_store")

    # -- observation hooks of the pose graph's stages (include/liorf_s2m_debug.h) --------
    def pgSetEstimate(self, key: int, R, t):
        """s2m_debug_pg_set_estimate: the estimate of `key` from a 3x3 rotation and a translation in fp64, taken as they are."""
        X = np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])
        self._check(self.lib.s2m_debug_pg_set_estimate(self.h, key, _dp(X)), "s2m_debug_pg_set_estimate")

    def pgLinearize(self) -> dict:
        """s2m_debug_pg_linearize at the current estimates: rc, Binv, Aof (chain, by key), Ji, Jj, rx (extra factors), ferr, fw
        (chain first), err, wmin."""
        n, nf = self.pgSize()
        m = nf - n
        o = dict(rc=np.zeros((n, 6)), Binv=np.zeros((n, 6, 6)), Aof=np.zeros((n, 6, 6)), Ji=np.zeros((m, 6, 6)), Jj=np.zeros((m, 6, 6)),
                 rx=np.zeros((m, 6)), ferr=np.zeros(n + m), fw=np.zeros(n + m))
        err, wmin = np.zeros(1), np.zeros(1)
        self._check(self.lib.s2m_debug_pg_linearize(self.h, n, m, *[_dp(o[k]) for k in ("rc", "Binv", "Aof", "Ji", "Jj", "rx", "ferr", "fw")],
                                                    _dp(err), _dp(wmin)), "s2m_debug_pg_linearize")
        o["err"], o["wmin"] = float(err[0]), float(wmin[0])
        return o

    def pgApply(self, op: int, v, block: bool = False) -> np.ndarray:
        """s2m_debug_pg_apply: one operator (S2M_DEBUG_PG_*) of the linearisation at the current estimates on the vector `v`
        (single form) or, with block=True, on the rows of `v` (1 .. S2M_PG_BLOCK_COLUMNS of them) in the block form."""
        n, nf = self.pgSize()
        m = nf - n
        a = np.ascontiguousarray(v, np.float64)
        cols = a.shape[0] if block else 0
        lin, lout = (6 * m if op == S2M_DEBUG_PG_KT else 6 * n), (6 * m if op == S2M_DEBUG_PG_K else 6 * n)
        a = a.reshape(max(cols, 1), lin)
        out = np.zeros((max(cols, 1), lout))
        self._check(self.lib.s2m_debug_pg_apply(self.h, op, cols, _dp(a), _dp(out)), "s2m_debug_pg_apply")
        return out if block else out[0]

    def pgCg(self, b, params: PgParams | None = None, block: bool = False):
        """s2m_debug_pg_cg: the CG on (I + K^T K) y = b at the current estimates; returns (y, [PgCgOut per column])."""
        n = self.pgSize()[0]
        a = np.ascontiguousarray(b, np.float64)
        cols = a.shape[0] if block else 0
        a = a.reshape(max(cols, 1), 6 * n)
        y = np.zeros_like(a)
        out = (PgCgOut * max(cols, 1))()
        self._check(self.lib.s2m_debug_pg_cg(self.h, C.byref(params) if params is not None else None, cols, _dp(a), _dp(y), out), "s2m_debug_pg_cg")
        return (y if block else y[0]), list(out)

    def pgRetract(self, delta) -> np.ndarray:
        """s2m_debug_pg_retract: (n, 12) states X (+) delta for the (n, 6) host `delta`; the estimates stay."""
        n = self.pgSize()[0]
        d = np.ascontiguousarray(delta, np.float64).reshape(n, 6)
        X = np.zeros((n, 12))
        self._check(self.lib.s2m_debug_pg_retract(self.h, n, _dp(d), _dp(X)), "s2m_debug_pg_retract")
        return X

    def saveKeyFramesAndFactor(self, pose_xyzrpy, time: float, cloud=None, loops=(), params: PgParams | None = None):
        """saveKeyFramesAndFactor() (reference :1536-1609) without the saveFrame() gate and the GPS queue, which stay with the
        caller: odometry factor, the queued loop factors `loops` (tuples for addLoopFactor), the update - and, as the
        reference runs isam->update() five more times after a closure, a second optimise - then the key frame with the
        graph's latest estimate.  Returns (PgResult, the stored pose)."""
        self.addOdomFactor(pose_xyzrpy)
        for lp in loops:
            self.addLoopFactor(*lp)
        res = self.pgOptimize(params)
        if getattr(self, "aLoopIsClosed", False):
            res = self.pgOptimize(params)
        n = self.pgSize()[0]
        latest = self.pgPoses(n - 1, 1)[0]
        self.saveKeyFrame(latest, time, cloud)
        return res, latest

    def correctPosesFromGraph(self) -> bool:
        """correctPoses() (reference :1611-1642): after a closure every key of the store takes the graph's estimate."""
        if self.kfSize() <= 0 or not getattr(self, "aLoopIsClosed", False):
            return False
        self.pgApplyToStore(0, self.kfSize())
        self.aLoopIsClosed = False
        return True

    # -- the global map and the saved map from the resident store (reference :453-502, :375-432) --------
    def publishGlobalMap(self, params: GmapParams | None = None, return_keys: bool = False):
        """publishGlobalMap() (reference :453-502) on the resident store: globalMapKeyFramesDS as (m, 8) float32 records;
        with return_keys also the key id of every frame concatenated into it, in order."""
        pp = C.byref(params) if params is not None else None
        n = max(self.kfSize(), 0)
        keys = np.zeros(max(n, 1), np.int32)
        m, nk = C.c_size_t(0), C.c_size_t(0)
        out = getattr(self, "_gmap_buf", None)
        if out is None:
            out = np.zeros((1, 8), np.float32)
        for _ in range(2):                            # a buffer too small for this call: grown to the count, and once more
            rc = self.lib.s2m_global_map(self.h, pp, out.ctypes.data, 32, out.shape[0], C.byref(m),
                                         keys.ctypes.data_as(C.POINTER(C.c_int32)), keys.size, C.byref(nk))
            if rc not in (S2M_OK, S2M_ERR_CAPACITY, S2M_WARN_LEAF_TOO_SMALL) or m.value <= out.shape[0]:
                break
            out = np.zeros((m.value, 8), np.float32)
        self._gmap_buf = out
        self.leaf_too_small = self._check_voxel(rc, "s2m_global_map")
        cloud = out[:m.value].copy()
        return (cloud, keys[:nk.value].copy()) if return_keys else cloud

    def globalMapCloud(self, first: int = 0, count: int | None = None, leaf: float = 0.0) -> np.ndarray:
        """saveMapService()'s globalSurfCloud (reference :395-398) for keys first .. first + count - 1, and with leaf > 0
        its downSizeFilterSurf at that resolution (:400-407): (m, 8) float32 records."""
        if count is None:
            count = max(self.kfSize(), 0) - first
        m = C.c_size_t(0)
        if leaf == 0.0:
            self._check(self.lib.s2m_kf_map_cloud(self.h, first, count, 0.0, None, 32, 0, C.byref(m)), "s2m_kf_map_cloud")
            out = np.zeros((max(m.value, 1), 8), np.float32)
            if m.value:
                self._check(self.lib.s2m_kf_map_cloud(self.h, first, count, 0.0, out.ctypes.data, 32, m.value, C.byref(m)),
                            "s2m_kf_map_cloud")
            self.leaf_too_small = False
            return out[:m.value]
        # filtered: the voxel count is known only after the filter; room for the unfiltered count never falls short
        self._check(self.lib.s2m_kf_map_cloud(self.h, first, count, 0.0, None, 32, 0, C.byref(m)), "s2m_kf_map_cloud")
        out = np.zeros((max(m.value, 1), 8), np.float32)
        self.leaf_too_small = self._check_voxel(
            self.lib.s2m_kf_map_cloud(self.h, first, count, float(leaf), out.ctypes.data, 32, out.shape[0], C.byref(m)),
            "s2m_kf_map_cloud")
        return out[:m.value]

    # -- loop closure against the resident key-frame store (reference :542-844) ----------------------
    def loopFindNearKeyframes(self, key: int, searchNum: int, loop_index: int = -1, leaf: float = 0.3) -> np.ndarray:
        """loopFindNearKeyframes(nearKeyframes, key, searchNum, loop_index) (reference :821-844) with downSizeFilterICP's
        leaf: (m, 8) float32 records."""
        m = C.c_size_t(0)
        rc = self.lib.s2m_loop_near_keyframes(self.h, key, searchNum, loop_index, leaf, None, 32, 0, C.byref(m))
        if rc != S2M_ERR_CAPACITY:
            self.leaf_too_small = self._check_voxel(rc, "s2m_loop_near_keyframes")
        out = np.zeros((max(m.value, 1), 8), np.float32)
        if m.value:                                   # (the same submap again, now with room for it)
            self.leaf_too_small = self._check_voxel(
                self.lib.s2m_loop_near_keyframes(self.h, key, searchNum, loop_index, leaf, out.ctypes.data, 32, m.value,
                                                 C.byref(m)), "s2m_loop_near_keyframes")
        return out[:m.value]

    def loopAlign(self, key_cur: int, key_pre: int, base_key: int = -1, params: LoopParams | None = None) -> LoopResult:
        """Extraction, gates, ICP and pose result for a given pair: base_key -1 is the RS form, >= 0 the SC form."""
        r = LoopResult()
        pp = C.byref(params) if params is not None else None
        self._check(self.lib.s2m_loop_align(self.h, key_cur, key_pre, base_key, pp, C.byref(r)), "s2m_loop_align")
        return r

    def performRSLoopClosure(self, timeLaserInfoCur: float, params: LoopParams | None = None) -> LoopResult:
        """performRSLoopClosure() (reference :542-622) with detectLoopClosureDistance() (:732-765) on the device."""
        r = LoopResult()
        pp = C.byref(params) if params is not None else None
        self._check(self.lib.s2m_loop_closure_rs(self.h, float(timeLaserInfoCur), pp, C.byref(r)), "s2m_loop_closure_rs")
        return r

    # -- the launched forms: the ICP runs on the handle's loop stream while the handle registers scans -----------
    def loopAlignLaunch(self, key_cur: int, key_pre: int, base_key: int = -1, params: LoopParams | None = None) -> LoopResult:
        """s2m_loop_align_launch: loopAlign up to the size gate; status S2M_LOOP_PENDING when the ICP was queued, else the
        final result (nothing pending). loopPoll() / loopCollect() bring the result."""
        r = LoopResult()
        pp = C.byref(params) if params is not None else None
        self._check(self.lib.s2m_loop_align_launch(self.h, key_cur, key_pre, base_key, pp, C.byref(r)), "s2m_loop_align_launch")
        return r

    def performRSLoopClosureLaunch(self, timeLaserInfoCur: float, params: LoopParams | None = None) -> LoopResult:
        """s2m_loop_closure_rs_launch: performRSLoopClosure() with the ICP queued instead of waited for."""
        r = LoopResult()
        pp = C.byref(params) if params is not None else None
        self._check(self.lib.s2m_loop_closure_rs_launch(self.h, float(timeLaserInfoCur), pp, C.byref(r)), "s2m_loop_closure_rs_launch")
        return r

    def loopPoll(self) -> LoopResult:
        """s2m_loop_poll: never waits for the device. S2M_LOOP_PENDING, the final result, or S2M_LOOP_NONE with nothing pending.
        The loop thread: lock, loopPoll(), unlock, sleep - until the status is not S2M_LOOP_PENDING."""
        r = LoopResult()
        self._check(self.lib.s2m_loop_poll(self.h, C.byref(r)), "s2m_loop_poll")
        return r

    def loopCollect(self) -> LoopResult:
        """s2m_loop_collect: loopPoll() with waits - the final result of the pending closure."""
        r = LoopResult()
        self._check(self.lib.s2m_loop_collect(self.h, C.byref(r)), "s2m_loop_collect")
        return r

    # -- verification: key_cur against several candidates, aligned in lockstep ----------------------------------
    def _verify_launch(self, fn, what, key_cur, key_pre, base_key, params):
        keys = (C.c_int32 * max(len(key_pre), 1))(*[int(k) for k in key_pre])
        recs = (LoopResult * S2M_LOOP_MAX_CANDIDATES)()
        best = C.c_int32(-1)
        pp = C.byref(params) if params is not None else None
        self._check(fn(self.h, int(key_cur), keys, len(key_pre), int(base_key), pp, recs, C.byref(best)), what)
        return [_copy_struct(recs[i]) for i in range(len(key_pre))], best.value

    def loopVerify(self, key_cur: int, key_pre, base_key: int = -1, params: LoopParams | None = None):
        """s2m_loop_verify: (records, best). records[i] is loopAlign(key_cur, key_pre[i], base_key) on a handle whose container does
        not hold key_cur; best is the position of the accepted record with the least (fitness, position), or -1. Only that pair
        goes into the container."""
        return self._verify_launch(self.lib.s2m_loop_verify, "s2m_loop_verify", key_cur, key_pre, base_key, params)

    def loopVerifyLaunch(self, key_cur: int, key_pre, base_key: int = -1, params: LoopParams | None = None):
        """s2m_loop_verify_launch: (early records, -1). Candidates that passed the gates carry S2M_LOOP_PENDING; if none did the
        records are final and nothing is pending."""
        return self._verify_launch(self.lib.s2m_loop_verify_launch, "s2m_loop_verify_launch", key_cur, key_pre, base_key, params)

    def _verify_poll(self, fn, what):
        recs = (LoopResult * S2M_LOOP_MAX_CANDIDATES)()
        n, best = C.c_int32(0), C.c_int32(-1)
        self._check(fn(self.h, recs, S2M_LOOP_MAX_CANDIDATES, C.byref(n), C.byref(best)), what)
        return [_copy_struct(recs[i]) for i in range(n.value)], best.value

    def loopVerifyPoll(self):
        """s2m_loop_verify_poll: never waits for the device. (records, best): pending records, the final ones, or ([], -1) with
        nothing pending."""
        return self._verify_poll(self.lib.s2m_loop_verify_poll, "s2m_loop_verify_poll")

    def loopVerifyCollect(self):
        """s2m_loop_verify_collect: loopVerifyPoll() with waits - the final records of the pending verification."""
        return self._verify_poll(self.lib.s2m_loop_verify_collect, "s2m_loop_verify_collect")

    # -- verification of many keys: the rows of scQueryKeys in one call ---------------------------
    def loopVerifyMany(self, rows, base_key: int = -1, params: LoopParams | None = None):
        """s2m_loop_verify_many: rows = [(key_cur, [key_pre...]), ...] -> (records per row, best per row), each row what
        loopVerify(key_cur, key_pre, base_key, params) gives in turn; a row without candidates gives ([], -1)."""
        key_cur, key_pre, n_cand, stride = _verify_many_rows(rows)
        m = len(rows)
        recs = (LoopResult * max(m * stride, 1))()
        best = (C.c_int32 * max(m, 1))(*([-1] * max(m, 1)))
        pp = C.byref(params) if params is not None else None
        self._check(self.lib.s2m_loop_verify_many(self.h, key_cur, key_pre, n_cand, m, stride, int(base_key), pp, recs, best), "s2m_loop_verify_many")
        return ([[_copy_struct(recs[r * stride + i]) for i in range(n_cand[r])] for r in range(m)], [best[r] for r in range(m)])

    def verifySessionLoops(self, gap: int = 30, max_dist: float = 0.3, top_k: int = 1, align: int = S2M_SC_ALIGN_FULL, base_key: int = 0,
                           params: LoopParams | None = None, rows_per_call: int = 64, ring_candidates=None):
        """findSessionLoops' query (ring_candidates as there) followed by loopVerifyMany in chunks of rows_per_call rows (a node
        releases its lock between chunks): the winning records, one per key that has an accepted candidate, in key_cur order."""
        top_k = min(int(top_k), S2M_LOOP_MAX_CANDIDATES)
        hits = self._sessionLoopRows(gap, max_dist, top_k, align, ring_candidates)
        rows = [(cur, [int(h["key"]) for h in row]) for cur, row in enumerate(hits) if len(row)]
        won = []
        for i in range(0, len(rows), max(int(rows_per_call), 1)):
            recs, best = self.loopVerifyMany(rows[i:i + max(int(rows_per_call), 1)], base_key, params)
            won += [r[b] for r, b in zip(recs, best) if b >= 0]
        return won

    # -- loop candidates by position for many keys -------------------------------------------------
    def loopDetectKeys(self, keys, time_cur=None, params: "LoopDetectParams | None" = None, **kw):
        """s2m_loop_detect_keys: for every stored key of `keys` its candidates by position, ascending (d2, key): (rows, d2 rows),
        rows = [(key, [key_pre...]), ...] as loopVerifyMany(rows, base_key=-1) takes them, d2 rows the fp32 squared distances
        alike.  time_cur: None (a query's time is its key's) or one time per key.  Keyword arguments set fields of the
        parameters (search_radius, time_diff_s, first, count, exclude_lo / _hi, rel_lo / _hi, top_k)."""
        p = default_loop_detect_params(**kw) if params is None else _copy_struct(params)
        if params is not None:
            for k, v in kw.items():
                if not hasattr(p, k):
                    raise AttributeError(k)
                setattr(p, k, v)
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1)
        m, K = len(keys), max(int(p.top_k), 0)
        tc = None if time_cur is None else np.ascontiguousarray(time_cur, np.float64).reshape(-1)
        if tc is not None and len(tc) != m:
            raise ValueError("time_cur: one time per key")
        key_pre = np.full((m, K), -1, np.int32)
        d2 = np.full((m, K), np.inf, np.float32)
        n = np.zeros(m, np.int32)
        self._check(self.lib.s2m_loop_detect_keys(self.h, keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  None if tc is None else tc.ctypes.data_as(C.POINTER(C.c_double)), m, C.byref(p),
                                                  key_pre.ctypes.data_as(C.POINTER(C.c_int32)), d2.ctypes.data_as(C.POINTER(C.c_float)),
                                                  n.ctypes.data_as(C.POINTER(C.c_int32))), "s2m_loop_detect_keys")
        return ([(int(keys[i]), [int(k) for k in key_pre[i, :n[i]]]) for i in range(m)], [d2[i, :n[i]].copy() for i in range(m)])

    def findSessionLoopsByDistance(self, radius: float = 10.0, time_diff: float = 30.0, top_k: int = 1, keys=None):
        """Every stored key, or `keys`, against the whole store by position: the (key_cur, key_pre, d2) candidates a node hands to
        loopVerifyMany(base_key=-1), in the order of the keys and per key in (d2, key_pre) order."""
        if keys is None:
            keys = np.arange(self.kfSize(), dtype=np.int32)
        rows, d2 = self.loopDetectKeys(keys, search_radius=radius, time_diff_s=time_diff, top_k=top_k)
        return [(cur, pre, float(d)) for (cur, pres), ds in zip(rows, d2) for pre, d in zip(pres, ds)]

    def verifySessionLoopsByDistance(self, radius: float = 10.0, time_diff: float = 30.0, top_k: int = 1, keys=None, base_key: int = -1,
                                     params: LoopParams | None = None, rows_per_call: int = 64):
        """findSessionLoopsByDistance's query followed by loopVerifyMany in chunks of rows_per_call rows (a node releases its lock
        between chunks): the winning records, one per key that has an accepted candidate, in the order of the keys.  `keys` must
        be distinct, as loopVerifyMany asks."""
        top_k = min(int(top_k), S2M_LOOP_MAX_CANDIDATES)
        if keys is None:
            keys = np.arange(self.kfSize(), dtype=np.int32)
        rows, _ = self.loopDetectKeys(keys, search_radius=radius, time_diff_s=time_diff, top_k=top_k)
        rows = [r for r in rows if len(r[1])]
        won = []
        for i in range(0, len(rows), max(int(rows_per_call), 1)):
            recs, best = self.loopVerifyMany(rows[i:i + max(int(rows_per_call), 1)], base_key, params)
            won += [r[b] for r, b in zip(recs, best) if b >= 0]
        return won

    # -- the mutually consistent loops among many candidates ---------------------------------------
    def pgConsistentLoops(self, key_from, key_to, rel, params: "PgConsistencyParams | None" = None, matrix: bool = False):
        """s2m_pg_consistent_loops: candidates as pgAddBetween would take them (key_from[i], key_to[i], rel[i] = the between
        pose) against the graph's current estimates.  Returns (selected (m,) bool, degree (m,) int32, PgConsistencyResult), and
        with matrix=True a fourth item, the (m, (m + 63) // 64) uint64 bit rows.  The set is the stated greedy rule's, not the
        maximum clique; nothing is added to the graph."""
        kf = np.ascontiguousarray(key_from, np.int32).reshape(-1)
        kt = np.ascontiguousarray(key_to, np.int32).reshape(-1)
        r = np.ascontiguousarray(rel, np.float32).reshape(-1, 6)
        m = len(kf)
        if len(kt) != m or len(r) != m:
            raise ValueError("key_from, key_to and rel: one entry per candidate")
        sel = np.zeros(max(m, 1), np.uint8)
        deg = np.zeros(max(m, 1), np.int32)
        mat = np.zeros((max(m, 1), max((m + 63) // 64, 1)), np.uint64) if matrix else None
        out = PgConsistencyResult()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.s2m_pg_consistent_loops(self.h, kf.ctypes.data_as(i32p), kt.ctypes.data_as(i32p), _fp(r), m,
                                                     C.byref(params) if params is not None else None,
                                                     sel.ctypes.data_as(C.POINTER(C.c_uint8)), deg.ctypes.data_as(i32p),
                                                     mat.ctypes.data_as(C.POINTER(C.c_uint64)) if matrix else None, C.byref(out)),
                    "s2m_pg_consistent_loops")
        res = (sel[:m].astype(bool), deg[:m], out)
        return res + (mat[:m, :(m + 63) // 64],) if matrix else res

    def selectConsistentLoops(self, records, params: "PgConsistencyParams | None" = None):
        """The records of verifySessionLoops / verifySessionLoopsByDistance (accepted LoopResults) that pgConsistentLoops keeps,
        in their order: each record is the candidate (key_cur, key_pre, pose_from.between(pose_to)) that addLoopFactor would
        add.  Between the verification and the graph: pass the kept ones to addLoopFactor."""
        records = list(records)
        if not records:
            return []
        rel = np.array([between_xyzrpy(np.array(r.pose_from), np.array(r.pose_to)) for r in records], np.float32)
        sel, _, _ = self.pgConsistentLoops([r.key_cur for r in records], [r.key_pre for r in records], rel, params)
        return [r for r, s in zip(records, sel) if s]

    def debugLoopDetectPass(self, queries_per_pass: int = 0):
        """s2m_debug_loop_detect_pass: at most this many queries per pass of loopDetectKeys (0: the default)."""
        self._check(self.lib.s2m_debug_loop_detect_pass(self.h, int(queries_per_pass)), "s2m_debug_loop_detect_pass")

    def debugLoopDetectSplits(self, max_splits: int = 0):
        """s2m_debug_loop_detect_splits: at most this many store splits per grid of loopDetectKeys (0: the plan's own)."""
        self._check(self.lib.s2m_debug_loop_detect_splits(self.h, int(max_splits)), "s2m_debug_loop_detect_splits")

    def debugLoopDetectLast(self):
        """s2m_debug_loop_detect_last: (passes, device bytes of one pass) of the last loopDetectKeys."""
        n, b = C.c_int32(0), C.c_size_t(0)
        self._check(self.lib.s2m_debug_loop_detect_last(self.h, C.byref(n), C.byref(b)), "s2m_debug_loop_detect_last")
        return n.value, b.value

    def debugLoopVerifyManyPass(self, pairs_per_pass: int = 0):
        """s2m_debug_loop_verify_many_pass: the pairs of a pass of loopVerifyMany (0: the default; clamped to [8, 64])."""
        self._check(self.lib.s2m_debug_loop_verify_many_pass(self.h, int(pairs_per_pass)), "s2m_debug_loop_verify_many_pass")

    def debugLoopVerifyManyLast(self):
        """s2m_debug_loop_verify_many_last: (passes, pairs aligned, bytes held for the submaps of a pass) of the last loopVerifyMany."""
        n, k, b = C.c_int32(0), C.c_int32(0), C.c_size_t(0)
        self._check(self.lib.s2m_debug_loop_verify_many_last(self.h, C.byref(n), C.byref(k), C.byref(b)), "s2m_debug_loop_verify_many_last")
        return n.value, k.value, b.value

    def debugIcpAlignPairsDevice(self, pairs, guesses=None, **params):
        """s2m_debug_icp_align_pairs_device: pairs = [(source, target), ...] through the table form of the device loop (no size
        gate), guesses None or one entry per pair (None or a 4x4): a list of (T 4x4, hasConverged, getFitnessScore, iterations)."""
        sr = [_records(a) for a, _ in pairs]
        tg = [_records(b) for _, b in pairs]
        st = sr[0][2] if sr else 0
        if any(t[2] != st for t in sr + tg):
            raise ValueError("all clouds must share one record stride")
        p = IcpParams()
        self.lib.s2m_icp_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        P = len(pairs)
        sp = (C.c_void_p * max(P, 1))(*[t[0].ctypes.data for t in sr])
        sn = (C.c_size_t * max(P, 1))(*[t[1] for t in sr])
        tp = (C.c_void_p * max(P, 1))(*[t[0].ctypes.data for t in tg])
        tn = (C.c_size_t * max(P, 1))(*[t[1] for t in tg])
        gs = None
        if guesses is not None:
            keep = [None if g is None else np.ascontiguousarray(g, np.float32).reshape(16) for g in guesses]
            gs = (C.c_void_p * max(P, 1))(*[None if g is None else g.ctypes.data for g in keep])
        out = (IcpResult * max(P, 1))()
        self._check(self.lib.s2m_debug_icp_align_pairs_device(self.h, sp, sn, tp, tn, P, st, gs, C.byref(p), out), "s2m_debug_icp_align_pairs_device")
        return [(np.array(r.T, np.float32).reshape(4, 4), bool(r.converged), r.fitness_score, r.iterations) for r in out[:P]]

    def debugIcpClose(self, sums, states, **params):
        """s2m_debug_icp_close: sums (n, 17) float64 and states (n, 38) uint32 (s2m_debug_icp_state word by word), n <= 64, closed
        by one launch of k_icp_close; keyword arguments are fields of the ICP parameters. Returns the outgoing states, (n, 38) uint32."""
        S = np.ascontiguousarray(sums, np.float64).reshape(-1, 17)
        w = np.ascontiguousarray(states, np.uint32).reshape(-1, 38)
        if S.shape[0] != w.shape[0]:
            raise ValueError("one state per row of sums")
        p = IcpParams()
        self.lib.s2m_icp_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        out = np.zeros_like(w)
        self._check(self.lib.s2m_debug_icp_close(self.h, S.shape[0], S.ctypes.data_as(C.POINTER(C.c_double)), w.ctypes.data, C.byref(p),
                                                 out.ctypes.data), "s2m_debug_icp_close")
        return out

    def debugIcpSums(self, pairs, table, max_correspondence_distance, want_parts=False, want_keys=False):
        """s2m_debug_icp_sums: pairs = [(source, target), ...]; table False: the slot form (every source the same array), True: the
        table form. Returns a list of dicts: sums (17 float64), rows, and where asked for parts (rows x 17) and keys (uint64 per source)."""
        sr = [_records(a) for a, _ in pairs]
        tg = [_records(b) for _, b in pairs]
        st = sr[0][2] if sr else 0
        if any(t[2] != st for t in sr + tg):
            raise ValueError("all clouds must share one record stride")
        if not table:
            if any(a is not pairs[0][0] for a, _ in pairs):
                raise ValueError("the slot form has one source")
            sr = [sr[0]] * len(sr)
        P = len(pairs)
        sp = (C.c_void_p * max(P, 1))(*[t[0].ctypes.data for t in sr])
        sn = (C.c_size_t * max(P, 1))(*[t[1] for t in sr])
        tp = (C.c_void_p * max(P, 1))(*[t[0].ctypes.data for t in tg])
        tn = (C.c_size_t * max(P, 1))(*[t[1] for t in tg])
        sums, rows = np.zeros((max(P, 1), 17)), np.zeros(max(P, 1), np.int32)
        parts = [np.zeros((256, 17)) for _ in range(P)] if want_parts else None
        keys = [np.zeros(t[1], np.uint64) for t in sr] if want_keys else None
        pp = (C.c_void_p * max(P, 1))(*[a.ctypes.data for a in parts]) if parts else None
        kp = (C.c_void_p * max(P, 1))(*[a.ctypes.data for a in keys]) if keys else None
        self._check(self.lib.s2m_debug_icp_sums(self.h, sp, sn, tp, tn, P, st, 1 if table else 0, float(max_correspondence_distance),
                                                sums.ctypes.data_as(C.POINTER(C.c_double)), rows.ctypes.data_as(C.POINTER(C.c_int32)), pp, kp),
                    "s2m_debug_icp_sums")
        out = []
        for k in range(P):
            d = dict(sums=sums[k].copy(), rows=int(rows[k]))
            if parts:
                d["parts"] = parts[k][:d["rows"]]
            if keys:
                d["keys"] = keys[k]
            out.append(d)
        return out

    def performSCLoopClosureVerified(self, top_k: int = 4, params: LoopParams | None = None, **query):
        """performSCLoopClosure() on the place query: the top_k <= S2M_LOOP_MAX_CANDIDATES hits of scQueryKey for the newest key
        (keyword arguments go to the query) verified in lockstep, SC form (base_key 0). The hits come ordered by descriptor
        distance; the verification re-ranks them by fitness. Returns (records, best, hits)."""
        n = self.kfSize()
        if n <= 0:
            return [], -1, np.zeros(0, SC_HIT_DTYPE)
        hits = self.scQueryKey(n - 1, top_k=int(top_k), **query)
        hits = hits[hits["key"] != n - 1][:S2M_LOOP_MAX_CANDIDATES]
        if len(hits) == 0:
            return [], -1, hits
        recs, best = self.loopVerify(n - 1, [int(k) for k in hits["key"]], 0, params)
        return recs, best, hits

    def debugIcpAlignManyDevice(self, cureKeyframeCloud, prevKeyframeClouds, **params):
        """s2m_debug_icp_align_many_device: one source against several targets by the slotted device loop (no size gate): a list of
        (T 4x4, hasConverged, getFitnessScore, iterations), one per target."""
        a, na, st = _records(cureKeyframeCloud)
        tg = [_records(t) for t in prevKeyframeClouds]
        if any(t[2] != st for t in tg):
            raise ValueError("all clouds must share one record stride")
        p = IcpParams()
        self.lib.s2m_icp_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        ptrs = (C.c_void_p * max(len(tg), 1))(*[t[0].ctypes.data for t in tg])
        ns = (C.c_size_t * max(len(tg), 1))(*[t[1] for t in tg])
        out = (IcpResult * max(len(tg), 1))()
        self._check(self.lib.s2m_debug_icp_align_many_device(self.h, a.ctypes.data, na, ptrs, ns, len(tg), st, C.byref(p), out),
                    "s2m_debug_icp_align_many_device")
        return [(np.array(r.T, np.float32).reshape(4, 4), bool(r.converged), r.fitness_score, r.iterations) for r in out[:len(tg)]]

    def debugIcpAlignGuessManyDevice(self, cureKeyframeCloud, prevKeyframeClouds, guesses, **params):
        """s2m_debug_icp_align_guess_many_device: debugIcpAlignManyDevice with a 4x4 guess per target (guesses=None: none); slot i
        gives what icpAlignGuess(cure, prev[i], guesses[i]) gives."""
        a, na, st = _records(cureKeyframeCloud)
        tg = [_records(t) for t in prevKeyframeClouds]
        if any(t[2] != st for t in tg):
            raise ValueError("all clouds must share one record stride")
        p = IcpParams()
        self.lib.s2m_icp_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        ptrs = (C.c_void_p * max(len(tg), 1))(*[t[0].ctypes.data for t in tg])
        ns = (C.c_size_t * max(len(tg), 1))(*[t[1] for t in tg])
        out = (IcpResult * max(len(tg), 1))()
        g = None if guesses is None else np.ascontiguousarray(guesses, np.float32).reshape(len(tg), 16)
        self._check(self.lib.s2m_debug_icp_align_guess_many_device(self.h, a.ctypes.data, na, ptrs, ns, None if g is None else _fp(g),
                                                                   len(tg), st, C.byref(p), out), "s2m_debug_icp_align_guess_many_device")
        return [(np.array(r.T, np.float32).reshape(4, 4), bool(r.converged), r.fitness_score, r.iterations) for r in out[:len(tg)]]

    def debugIcpNearest(self, src, tgt, mode: int, reps: int = 0):
        """s2m_debug_icp_nearest / s2m_debug_icp_time_nearest: (keys uint64 per source point, n_fallback[, us_build, us_search]);
        mode 0 = k_icp_nn, mode 1 = the grid search with its fallback."""
        a, na, st = _records(src)
        b, nb, st2 = _records(tgt)
        if st != st2:
            raise ValueError("both clouds must share one record stride")
        keys = np.zeros(max(na, 1), np.uint64)
        nf, ub, us = C.c_int32(0), C.c_float(0), C.c_float(0)
        self._check(self.lib.s2m_debug_icp_time_nearest(self.h, a.ctypes.data, na, b.ctypes.data, nb, st, mode, reps, keys.ctypes.data,
                                                        C.byref(nf), C.byref(ub), C.byref(us)), "s2m_debug_icp_time_nearest")
        return (keys[:na], nf.value) if reps == 0 else (keys[:na], nf.value, ub.value, us.value)

    def debugIcpAlignDevice(self, cureKeyframeCloud, prevKeyframeCloud, **params):
        """s2m_debug_icp_align_device: icpAlign() by the device loop (no size gate): (T 4x4, hasConverged, getFitnessScore, iterations)."""
        a, na, st = _records(cureKeyframeCloud)
        b, nb, st2 = _records(prevKeyframeCloud)
        if st != st2:
            raise ValueError("both clouds must share one record stride")
        p = IcpParams()
        self.lib.s2m_icp_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        r = IcpResult()
        self._check(self.lib.s2m_debug_icp_align_device(self.h, a.ctypes.data, na, b.ctypes.data, nb, st, C.byref(p), C.byref(r)),
                    "s2m_debug_icp_align_device")
        return np.array(r.T, np.float32).reshape(4, 4), bool(r.converged), r.fitness_score, r.iterations

    def debugIcpTuning(self, cell_in_leaves: float = 0.0, shell_cap: int = 0, use_grid: int = -1):
        """s2m_debug_icp_tuning: the grid's cell edge (in leaves), the shell cap, grid on / off for what follows (0, 0, -1 = built in)."""
        self._check(self.lib.s2m_debug_icp_tuning(self.h, cell_in_leaves, shell_cap, use_grid), "s2m_debug_icp_tuning")

    def debugIcpGrid(self, targets, tables: bool = True):
        """s2m_debug_icp_grid: the grids the device loop builds over 1 .. S2M_LOOP_MAX_CANDIDATES targets, one dict per target:
        lo (3 fp32), cell, inv (np.float32), n (3 ints), n_fin, usable and, with `tables` and where a grid was built, start and
        end (prod(n) int32: per cell its range in the sorted targets) and order (n_fin int32: the original index of each entry)."""
        tg = [_records(t) for t in targets]
        if any(t[2] != tg[0][2] for t in tg):
            raise ValueError("all clouds must share one record stride")
        K = len(tg)
        ptrs = (C.c_void_p * max(K, 1))(*[t[0].ctypes.data for t in tg])
        ns = (C.c_size_t * max(K, 1))(*[t[1] for t in tg])
        out = (IcpGridOut * max(K, 1))()
        bufs = [[np.full(S2M_DEBUG_ICP_GRID_MAX_CELLS, -1, np.int32), np.full(S2M_DEBUG_ICP_GRID_MAX_CELLS, -1, np.int32),
                 np.full(max(t[1], 1), -1, np.int32)] for t in tg] if tables else []
        arrs = [(C.c_void_p * max(K, 1))(*[b[j].ctypes.data for b in bufs]) if tables else None for j in range(3)]
        self._check(self.lib.s2m_debug_icp_grid(self.h, ptrs, ns, K, tg[0][2] if tg else 0, out, *arrs), "s2m_debug_icp_grid")
        res = []
        for k in range(K):
            o = out[k]
            g = dict(lo=np.array(o.lo, np.float32), cell=np.float32(o.cell), inv=np.float32(o.inv), n=tuple(int(v) for v in o.n),
                     n_fin=int(o.n_fin), usable=int(o.usable))
            if tables and g["usable"]:
                nc = g["n"][0] * g["n"][1] * g["n"][2]
                g.update(start=bufs[k][0][:nc], end=bufs[k][1][:nc], order=bufs[k][2][:g["n_fin"]])
            res.append(g)
        return res

    def performSCLoopClosure(self, params: LoopParams | None = None) -> LoopResult:
        """performSCLoopClosure() (reference :624-730): the ScanContext detector on this handle's SC store, then
        s2m_loop_align(kfSize() - 1, pre, 0, ..) (:634-655). yaw_diff is not used by the reference (:639)."""
        r = LoopResult()
        r.status, r.key_cur, r.key_pre = S2M_LOOP_NONE, -1, -1
        n = self.kfSize()
        if n <= 0:                                    # (:626-627): no detection either
            return r
        pre, _, _ = self.detectLoopClosureID()
        if pre == -1:
            return r
        return self.loopAlign(n - 1, pre, 0, params)


def between_xyzrpy(pose_from, pose_to) -> np.ndarray:
    """poseFrom.between(poseTo) of two {x, y, z, roll, pitch, yaw} poses (Rot3::RzRyRx), fp64, as a float pose vector."""
    def mat(p):
        p = np.asarray(p, np.float64)
        cr, sr, cp, sp, cy, sy = np.cos(p[3]), np.sin(p[3]), np.cos(p[4]), np.sin(p[4]), np.cos(p[5]), np.sin(p[5])
        return np.array([[cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr],
                         [sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr],
                         [-sp, cp * sr, cp * cr]]), p[:3]
    Ra, ta = mat(pose_from)
    Rb, tb = mat(pose_to)
    R, t = Ra.T @ Rb, Ra.T @ (tb - ta)
    return np.array([t[0], t[1], t[2], np.arctan2(R[2, 1], R[2, 2]), np.arcsin(np.clip(-R[2, 0], -1.0, 1.0)),
                     np.arctan2(R[1, 0], R[0, 0])], np.float32)


def default_pg_params(**kw) -> PgParams:
    p = PgParams()
    rc = load_library().s2m_pg_default_params(C.byref(p))
    if rc != S2M_OK:
        raise S2MError(rc, "s2m_pg_default_params")
    for k, v in kw.items():
        if isinstance(v, (list, tuple, np.ndarray)):
            v = (C.c_double * 6)(*[float(x) for x in v])
        setattr(p, k, v)
    return p


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def pg_check_args(kind: int, n_variables: int, key_a: int, key_b: int, values, var=None, robust_k: float = 0.0) -> int:
    """s2m_pg_check_args (host only, no GPU): the status code."""
    v = None if values is None else np.ascontiguousarray(values, np.float32)
    w = None if var is None else np.ascontiguousarray(var, np.float64)
    return load_library().s2m_pg_check_args(kind, n_variables, key_a, key_b, None if v is None else _fp(v),
                                            None if w is None else _dp(w), float(robust_k))


def default_pg_consistency_params(**kw) -> PgConsistencyParams:
    """s2m_pg_consistency_default_params; keyword arguments set fields."""
    p = PgConsistencyParams()
    rc = load_library().s2m_pg_consistency_default_params(C.byref(p))
    if rc != S2M_OK:
        raise S2MError(rc, "s2m_pg_consistency_default_params")
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def pg_consistency_check_args(n_variables: int, key_from, key_to, rel, params: "PgConsistencyParams | None" = None, m=None) -> int:
    """s2m_pg_consistency_check_args (host only, no GPU): the status code.  None for an array passes a null pointer; m defaults
    to len(key_from); params=None passes a null pointer (the defaults)."""
    kf = None if key_from is None else np.ascontiguousarray(key_from, np.int32).reshape(-1)
    kt = None if key_to is None else np.ascontiguousarray(key_to, np.int32).reshape(-1)
    r = None if rel is None else np.ascontiguousarray(rel, np.float32).reshape(-1)
    mm = m if m is not None else (0 if kf is None else len(kf))
    i32p = C.POINTER(C.c_int32)
    return load_library().s2m_pg_consistency_check_args(n_variables, None if kf is None else kf.ctypes.data_as(i32p),
                                                        None if kt is None else kt.ctypes.data_as(i32p), None if r is None else _fp(r),
                                                        mm, None if params is None else C.byref(params))


def pg_rebase(a_launch, a_now, X) -> np.ndarray:
    """s2m_debug_pg_rebase (host only, no GPU): the tail rule of a launched optimise, X <- (a_now a_launch^-1) X on states of
    12 doubles (R row-major, then t)."""
    a = np.ascontiguousarray(a_launch, np.float64).reshape(12)
    b = np.ascontiguousarray(a_now, np.float64).reshape(12)
    x = np.array(X, np.float64).reshape(12).copy()
    rc = load_library().s2m_debug_pg_rebase(_dp(a), _dp(b), _dp(x))
    if rc != S2M_OK:
        raise S2MError(rc, "s2m_debug_pg_rebase")
    return x


def pg_apply_check_args(n_variables: int, n_extra: int, op: int, cols: int, has_in: bool = True, has_out: bool = True) -> int:
    """s2m_debug_pg_apply_check_args (host only, no GPU): the status code."""
    a = np.zeros(1)
    return load_library().s2m_debug_pg_apply_check_args(n_variables, n_extra, op, cols, _dp(a) if has_in else None, _dp(a) if has_out else None)


def debug_icp_grid_check_args(targets, n_cand: int | None = None, stride: int | None = None, has_out: bool = True,
                              has_list: bool = True, has_counts: bool = True) -> int:
    """s2m_debug_icp_grid_check_args (host only, no GPU): the status code. targets: clouds, or None for a null entry."""
    tg = [None if t is None else _records(t) for t in targets]
    K = len(tg)
    ptrs = (C.c_void_p * max(K, 1))(*[None if t is None else t[0].ctypes.data for t in tg])
    ns = (C.c_size_t * max(K, 1))(*[1 if t is None else t[1] for t in tg])
    if stride is None:
        stride = next((t[2] for t in tg if t is not None), 16)
    out = (IcpGridOut * max(K, 1))()
    return load_library().s2m_debug_icp_grid_check_args(ptrs if has_list else None, ns if has_counts else None, K if n_cand is None else n_cand,
                                                        stride, out if has_out else None)


def pg_marginals_check_args(n_variables: int, keys, n_keys: int | None = None) -> int:
    """s2m_pg_marginals_check_args (host only, no GPU): the status code.  keys=None passes a null pointer."""
    k = None if keys is None else np.ascontiguousarray(keys, np.int32).reshape(-1)
    if n_keys is None:
        n_keys = 0 if k is None else k.shape[0]
    return load_library().s2m_pg_marginals_check_args(n_variables, None if k is None else k.ctypes.data_as(C.POINTER(C.c_int32)), n_keys)


def default_sc_query_params(**kw) -> ScQueryParams:
    p = ScQueryParams()
    load_library().s2m_sc_query_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _sc_many_fields(p) -> dict:
    return {**{f: getattr(p.q, f) for f, _ in ScQueryParams._fields_}, "rel_lo": p.rel_lo, "rel_hi": p.rel_hi}


def default_sc_query_many_params(**kw) -> ScQueryManyParams:
    """s2m_sc_query_many_default_params; keyword arguments set rel_lo, rel_hi and the fields of the single query's parameters."""
    p = ScQueryManyParams()
    load_library().s2m_sc_query_many_default_params(C.byref(p))
    for k, v in kw.items():
        tgt = p if k in ("rel_lo", "rel_hi") else p.q
        if not hasattr(tgt, k):
            raise AttributeError(k)
        setattr(tgt, k, v)
    return p


def sc_query_many_check_args(n_stored: int, m: int, params: "ScQueryManyParams | None", descriptor_query: bool = False) -> int:
    """s2m_sc_query_many_check_args (host only, no GPU): the status code.  params=None passes a null pointer (the defaults)."""
    return load_library().s2m_sc_query_many_check_args(n_stored, m, None if params is None else C.byref(params), int(descriptor_query))


def _sc_ring_fields(p) -> dict:
    return {**_sc_many_fields(p.m), "n_candidates": p.n_candidates, "reserved": p.reserved}


def default_sc_ring_params(**kw) -> ScRingParams:
    """s2m_sc_ring_default_params; keyword arguments set n_candidates, reserved and the fields of the many-query's parameters."""
    p = ScRingParams()
    load_library().s2m_sc_ring_default_params(C.byref(p))
    for k, v in kw.items():
        tgt = p if k in ("n_candidates", "reserved") else p.m if k in ("rel_lo", "rel_hi") else p.m.q
        if not hasattr(tgt, k):
            raise AttributeError(k)
        setattr(tgt, k, v)
    return p


def sc_ring_check_args(n_stored: int, m: int, params: "ScRingParams | None", descriptor_query: bool = False) -> int:
    """s2m_sc_ring_check_args (host only, no GPU): the status code.  params=None passes a null pointer (the defaults)."""
    return load_library().s2m_sc_ring_check_args(n_stored, m, None if params is None else C.byref(params), int(descriptor_query))


def sc_ring_shape():
    """s2m_debug_sc_ring_shape: (stored ring keys of a tile, queries of a block, words of a query's candidate buffer) of
    k_sc_ring_select."""
    t, b, w = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    load_library().s2m_debug_sc_ring_shape(C.byref(t), C.byref(b), C.byref(w))
    return t.value, b.value, w.value


def sc_query_many_shape():
    """s2m_debug_sc_query_many_shape: (stored descriptors of a tile, queries of a block) of k_sc_many_dist."""
    t, b = C.c_int32(0), C.c_int32(0)
    load_library().s2m_debug_sc_query_many_shape(C.byref(t), C.byref(b))
    return t.value, b.value


def _copy_struct(s):
    """A ctypes structure of its own (an element of a ctypes array is a view into the array)."""
    out = type(s)()
    C.memmove(C.byref(out), C.byref(s), C.sizeof(s))
    return out


def loop_verify_check_args(n_stored: int, key_cur: int, key_pre, base_key: int = -1, params: "LoopParams | None" = None, n_cand=None) -> int:
    """s2m_loop_verify_check_args (host only, no GPU): the status code. key_pre=None passes a null pointer; n_cand defaults to
    len(key_pre)."""
    keys = None if key_pre is None else (C.c_int32 * max(len(key_pre), 1))(*[int(k) for k in key_pre])
    n = n_cand if n_cand is not None else (0 if key_pre is None else len(key_pre))
    return load_library().s2m_loop_verify_check_args(n_stored, key_cur, keys, n, base_key, None if params is None else C.byref(params))


def _verify_many_rows(rows):
    """rows = [(key_cur, [key_pre...]), ...] as the arrays of s2m_loop_verify_many: (key_cur, key_pre, n_cand, row_stride)."""
    m = len(rows)
    stride = max([len(c) for _, c in rows] + [1])
    key_cur = (C.c_int32 * max(m, 1))(*[int(k) for k, _ in rows])
    n_cand = (C.c_int32 * max(m, 1))(*[len(c) for _, c in rows])
    key_pre = (C.c_int32 * max(m * stride, 1))()
    for r, (_, c) in enumerate(rows):
        for i, k in enumerate(c):
            key_pre[r * stride + i] = int(k)
    return key_cur, key_pre, n_cand, stride


def loop_verify_many_check_args(n_stored: int, rows, base_key: int = -1, params: "LoopParams | None" = None, m=None, row_stride=None,
                                n_cand=None) -> int:
    """s2m_loop_verify_many_check_args (host only, no GPU): the status code. rows as loopVerifyMany takes them (None: null
    arrays); m, row_stride and n_cand override what the rows imply."""
    if rows is None:
        key_cur = key_pre = nc = None
        mm, stride = 0, 1
    else:
        key_cur, key_pre, nc, stride = _verify_many_rows(rows)
        mm = len(rows)
    if n_cand is not None:
        nc = (C.c_int32 * max(len(n_cand), 1))(*[int(v) for v in n_cand])
    return load_library().s2m_loop_verify_many_check_args(n_stored, key_cur, key_pre, nc, mm if m is None else m,
                                                          stride if row_stride is None else row_stride, base_key,
                                                          None if params is None else C.byref(params))


def loop_verify_many_plan(n_cand, pairs_per_pass: int = 0):
    """s2m_debug_loop_verify_many_plan (host only, no GPU): the first row of every pass and, last, m."""
    m = len(n_cand)
    nc = (C.c_int32 * max(m, 1))(*[int(v) for v in n_cand])
    first = (C.c_int32 * (m + 1))()
    n_pass = C.c_int32(0)
    rc = load_library().s2m_debug_loop_verify_many_plan(nc, m, int(pairs_per_pass), first, C.byref(n_pass))
    if rc != 0:
        raise RuntimeError(f"s2m_debug_loop_verify_many_plan failed ({rc})")
    return [first[k] for k in range(n_pass.value + 1)]


def default_loop_detect_params(**kw) -> LoopDetectParams:
    """s2m_loop_detect_default_params; keyword arguments set fields."""
    p = LoopDetectParams()
    load_library().s2m_loop_detect_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def loop_detect_keys_check_args(n_stored: int, keys, params: "LoopDetectParams | None" = None, m=None, has_time_cur: bool = False) -> int:
    """s2m_loop_detect_keys_check_args (host only, no GPU): the status code. keys=None passes a null pointer; m defaults to
    len(keys); params=None passes a null pointer (the defaults)."""
    arr = None if keys is None else (C.c_int32 * max(len(keys), 1))(*[int(k) for k in keys])
    mm = m if m is not None else (0 if keys is None else len(keys))
    return load_library().s2m_loop_detect_keys_check_args(n_stored, arr, mm, int(has_time_cur), None if params is None else C.byref(params))


def loop_detect_shape():
    """s2m_debug_loop_detect_shape: (stored keys of a tile, queries of a block, most store splits) of k_loop_detect_many."""
    t, b, s = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    load_library().s2m_debug_loop_detect_shape(C.byref(t), C.byref(b), C.byref(s))
    return t.value, b.value, s.value


def loop_verify_best(records) -> int:
    """The model of *best: the position of the S2M_LOOP_ACCEPTED record with the least (icp.fitness_score, position), or -1."""
    ranked = sorted((r.icp.fitness_score, i) for i, r in enumerate(records) if r.status == S2M_LOOP_ACCEPTED)
    return ranked[0][1] if ranked else -1


def default_reloc_params(**kw) -> RelocParams:
    """s2m_reloc_default_params; keyword arguments set fields, `query_*` and `loop_*` those of the two nested structures."""
    p = RelocParams()
    load_library().s2m_reloc_default_params(C.byref(p))
    for k, v in kw.items():
        tgt, name = (p.query, k[6:]) if k.startswith("query_") else (p.loop, k[5:]) if k.startswith("loop_") else (p, k)
        if not hasattr(tgt, name):
            raise AttributeError(k)
        setattr(tgt, name, v)
    return p


def relocalize_check_args(n_sc: int, n_kf: int, params: "RelocParams | None") -> int:
    """s2m_relocalize_check_args (host only, no GPU): the status code. params=None passes a null pointer (the defaults)."""
    return load_library().s2m_relocalize_check_args(n_sc, n_kf, None if params is None else C.byref(params))


def sc_query_check_args(n_stored: int, params: "ScQueryParams | None") -> int:
    """s2m_sc_query_check_args (host only, no GPU): the status code.  params=None passes a null pointer (the defaults)."""
    return load_library().s2m_sc_query_check_args(n_stored, None if params is None else C.byref(params))


def default_kf_params(**kw) -> KfParams:
    p = KfParams()
    load_library().s2m_kf_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_loop_params(**kw) -> LoopParams:
    p = LoopParams()
    load_library().s2m_loop_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_gmap_params(**kw) -> GmapParams:
    p = GmapParams()
    load_library().s2m_gmap_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---- imageProjection's point filter and IMU deskew (reference src/imageProjection.cpp) ------------------------------
def scan_layout_preset(sensor: int) -> ScanLayout:
    lay = ScanLayout()
    if load_library().s2m_scan_layout_preset(sensor, C.byref(lay)) != S2M_OK:
        raise ValueError(f"unknown sensor {sensor}")
    return lay


def default_project_params(**kw) -> ProjectParams:
    p = ProjectParams()
    load_library().s2m_project_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def imu_deskew_info(imu, time_scan_cur: float, time_scan_end: float):
    """s2m_imu_deskew_info (host code, no GPU): imu is (n, 4) float64 {time, wx, wy, wz}. Returns
    (rc, imuTime, imuRotX, imuRotY, imuRotZ, imuPointerCur, imuAvailable); the tables have S2M_IMU_QUEUE_LENGTH entries."""
    a = np.ascontiguousarray(imu, np.float64).reshape(-1, 4)
    tabs = [np.zeros(S2M_IMU_QUEUE_LENGTH, np.float64) for _ in range(4)]
    cur, avail = C.c_int32(0), C.c_int32(0)
    dp = C.POINTER(C.c_double)
    rc = load_library().s2m_imu_deskew_info(a.ctypes.data_as(dp), a.shape[0], float(time_scan_cur), float(time_scan_end),
                                            *[t.ctypes.data_as(dp) for t in tabs], C.byref(cur), C.byref(avail))
    return (rc, *tabs, cur.value, bool(avail.value))


def make_deskew_info(time_scan_cur: float, deskew: bool, imu_pointer_cur: int, imu_time, rot_x, rot_y, rot_z):
    """An s2m_deskew_info over the four arrays (kept alive on the returned object)."""
    dp = C.POINTER(C.c_double)
    keep = [np.ascontiguousarray(t, np.float64) for t in (imu_time, rot_x, rot_y, rot_z)]
    d = DeskewInfo(float(time_scan_cur), 1 if deskew else 0, int(imu_pointer_cur), *[k.ctypes.data_as(dp) for k in keep])
    d._keep = keep
    return d


def odom_deskew_info(odom, time_scan_cur: float, time_scan_end: float, imu_rate: float = 500.0) -> OdomDeskew:
    """s2m_odom_deskew_info (host code, no GPU): odom is (n, 9) float64 {time, px, py, pz, qx, qy, qz, qw, cov0} in queue order."""
    a = np.ascontiguousarray(odom, np.float64).reshape(-1, 9)
    out = OdomDeskew()
    rc = load_library().s2m_odom_deskew_info(a.ctypes.data_as(C.POINTER(OdomSample)), a.shape[0], float(time_scan_cur), float(time_scan_end),
                                             float(imu_rate), C.byref(out))
    if rc != S2M_OK:
        raise S2MError(f"s2m_odom_deskew_info: {ERRORS.get(rc, rc)}")
    return out


def make_motion_info(enabled: bool, time_scan_end: float, odom_incre) -> MotionInfo:
    return MotionInfo(1 if enabled else 0, float(time_scan_end), (C.c_float * 3)(*[float(v) for v in odom_incre]))


def make_guess_info(imuAvailable=0, odomAvailable=0, imu=(0.0, 0.0, 0.0), guess=(0.0,) * 6) -> GuessInfo:
    """The cloud_info fields updateInitialGuess() reads: imu = imuRollInit, imuPitchInit, imuYawInit; guess = initialGuessX, Y, Z,
    Roll, Pitch, Yaw."""
    return GuessInfo(int(imuAvailable), int(odomAvailable), float(imu[0]), float(imu[1]), float(imu[2]), (C.c_float * 6)(*[float(v) for v in guess]))


class ImageProjectionS2M:
    """The cloud path of the reference's ImageProjection node (src/imageProjection.cpp) over a MapOptimizationS2M's
    handle: imuDeskewInfo() on the host, projectPointCloud() on the device. The deskewed cloud stays resident on that
    handle for downsampleCurrentScanProjected() / makeAndSaveScancontextAndKeysProjected()."""

    def __init__(self, mapper: MapOptimizationS2M, sensor: int | None = S2M_SENSOR_VELODYNE, layout: ScanLayout | None = None,
                 **params):
        self.mapper = mapper
        self.lib = mapper.lib
        self.layout = layout if layout is not None else scan_layout_preset(sensor)
        self.params = default_project_params(**params)
        self.deskewFlag = 1                                    # (:310-323: 1 when the cloud has a time field, else -1)
        self.timeScanCur = 0.0
        self.timeScanEnd = 0.0
        self.imuTime = np.zeros(S2M_IMU_QUEUE_LENGTH, np.float64)
        self.imuRotX = np.zeros(S2M_IMU_QUEUE_LENGTH, np.float64)
        self.imuRotY = np.zeros(S2M_IMU_QUEUE_LENGTH, np.float64)
        self.imuRotZ = np.zeros(S2M_IMU_QUEUE_LENGTH, np.float64)
        self.imuPointerCur = 0
        self.imuAvailable = False
        self.fullCloud = None
        self.fullCloudNum = 0
        self._raw = None
        self.imuRate = 500.0                                   # include/utility.h:212
        self.positionalDeskew = False                          # findPosition() with its commented lines live (:526-533); off = the reference as shipped
        self.odomAvailable = False                             # cloudInfo.odomAvailable
        self.odomDeskewFlag = False
        self.odomIncre = np.zeros(3, np.float32)               # odomIncreX, Y, Z
        self.initialGuess = np.zeros(6, np.float32)            # cloudInfo.initialGuessX, Y, Z, Roll, Pitch, Yaw
        self.odomQueue = np.zeros((0, 9), np.float64)          # stand-in for odomQueue: rows {time, px, py, pz, qx, qy, qz, qw, cov0}

    def record_times(self, raw: np.ndarray) -> np.ndarray:
        """laserCloudIn->points[i].time of every record, as the conversion loops leave it (:216-274)."""
        lay, n = self.layout, raw.size // self.layout.stride
        rec = raw.reshape(n, lay.stride)
        b = rec[:, lay.off_time:lay.off_time + (8 if lay.time_type == S2M_TIME_F64_REL else 4)]
        if lay.time_type == S2M_TIME_F32:
            return np.ascontiguousarray(b).view(np.float32).reshape(n)
        if lay.time_type == S2M_TIME_U32_NS:
            return np.ascontiguousarray(b).view(np.uint32).reshape(n).astype(np.float32) * np.float32(1e-9)
        if lay.time_type == S2M_TIME_U32:
            return np.ascontiguousarray(b).view(np.uint32).reshape(n).astype(np.float32)
        ts = np.ascontiguousarray(b).view(np.float64).reshape(n)
        return (ts - ts[0]).astype(np.float32)

    def cachePointCloud(self, raw_bytes, stamp: float):
        """The part of cachePointCloud() (:206-343) that reaches the cloud path: keep the raw bytes as they are,
        timeScanCur = header stamp, timeScanEnd = timeScanCur + time of the last record (:282-283)."""
        raw = np.ascontiguousarray(np.frombuffer(raw_bytes, np.uint8) if not isinstance(raw_bytes, np.ndarray) else raw_bytes.view(np.uint8).reshape(-1))
        if raw.size % self.layout.stride:
            raise ValueError("the buffer is not a whole number of records")
        self._raw = raw
        self.timeScanCur = float(stamp)
        n = raw.size // self.layout.stride
        last = float(self.record_times(raw)[-1]) if n else 0.0
        self.timeScanEnd = self.timeScanCur + last

    def imuDeskewInfo(self, imu) -> bool:
        """imuDeskewInfo() (:350-409) on samples {time, wx, wy, wz} already popped to timeScanCur - 0.01."""
        rc, self.imuTime, self.imuRotX, self.imuRotY, self.imuRotZ, self.imuPointerCur, self.imuAvailable = \
            imu_deskew_info(imu, self.timeScanCur, self.timeScanEnd)
        if rc != S2M_OK:
            raise S2MError(f"s2m_imu_deskew_info: {ERRORS.get(rc, rc)}")
        return self.imuAvailable

    def odomDeskewInfo(self, odom=None) -> bool:
        """odomDeskewInfo() (:411-491) on odomQueue (or on `odom`, which then becomes the queue): pops the front of the queue as
        the reference does and sets odomAvailable, initialGuess, odomDeskewFlag and odomIncre. Like the reference's members,
        initialGuess and odomIncre keep their previous values where the reference does not write them."""
        if odom is not None:
            self.odomQueue = np.ascontiguousarray(odom, np.float64).reshape(-1, 9)
        r = odom_deskew_info(self.odomQueue, self.timeScanCur, self.timeScanEnd, self.imuRate)
        self.odomQueue = self.odomQueue[r.n_popped:]
        self.odomAvailable = bool(r.odom_available)
        if r.odom_available:
            self.initialGuess = np.array(r.initial_guess, np.float32)
            self.odomDeskewFlag = bool(r.odom_deskew_flag)
        if r.odom_deskew_flag:
            self.odomIncre = np.array(r.odom_incre, np.float32)
        return self.odomAvailable

    def motionInfo(self, positional: bool | None = None) -> MotionInfo:
        on = self.positionalDeskew if positional is None else positional
        return make_motion_info(bool(on and self.odomAvailable and self.odomDeskewFlag), self.timeScanEnd, self.odomIncre)

    def deskewInfo(self) -> DeskewInfo:
        on = self.deskewFlag == 1 and self.imuAvailable
        return make_deskew_info(self.timeScanCur, on, self.imuPointerCur if on else 0, self.imuTime, self.imuRotX, self.imuRotY,
                                self.imuRotZ)

    def projectPointCloud(self, readback: bool = True, device_ptr=None, positional: bool | None = None):
        """projectPointCloud() (:568-598) on the cached records (or device_ptr=(ptr, n) for records already in HBM):
        cloud_deskewed stays on the device; with readback fullCloud is its host copy, (m, 8) float32. positional (default: the
        positionalDeskew member) turns findPosition()'s commented lines on (s2m_project_scan_motion) when odomDeskewInfo() found
        odomAvailable and odomDeskewFlag."""
        lay = self.layout
        if device_ptr is not None:
            src, n, on_dev = C.c_void_p(device_ptr[0]), int(device_ptr[1]), 1
        else:
            n = self._raw.size // lay.stride
            src, on_dev = self._raw.ctypes.data, 0
        d = self.deskewInfo()
        m = C.c_size_t(0)
        cap = (n + self.params.point_filter_num - 1) // max(self.params.point_filter_num, 1) if readback else 0
        out = np.zeros((max(cap, 1), 8), np.float32) if readback else None
        mo = self.motionInfo(positional)
        if mo.enabled:
            self.mapper._check(self.lib.s2m_project_scan_motion(self.mapper.h, src, n, C.byref(lay), on_dev, C.byref(self.params), C.byref(d),
                                                                C.byref(mo), out.ctypes.data if readback else None, 32, cap, C.byref(m)),
                               "s2m_project_scan_motion")
        else:
            self.mapper._check(self.lib.s2m_project_scan(self.mapper.h, src, n, C.byref(lay), on_dev, C.byref(self.params), C.byref(d),
                                                         out.ctypes.data if readback else None, 32, cap, C.byref(m)), "s2m_project_scan")
        self.fullCloudNum = m.value
        self.mapper.cloudDeskewedNum = m.value                 # sizes downsampleCurrentScanProjected()'s host buffer
        self.fullCloud = out[:m.value] if readback else None
        return self.fullCloud
