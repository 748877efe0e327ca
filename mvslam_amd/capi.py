"""ctypes binding of libmvslam_hip.so (include/mvslam_hip.h).

Plumbing only: it forwards numpy buffers to the C ABI and never computes anything itself.
There is no CPU fallback -- if the HIP library is missing or no device is present the
calls raise.
"""
import ctypes as C
import os
import weakref

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libmvslam_hip.so")
# diagnostics build with the mvs_debug_* hooks (make -C mvslam_amd/csrc): never loaded by this package unless a tool asks
# for it explicitly with MVS_USE_DEBUG_LIB=1 (tools/margin_sweep.py) -- tests load it side by side through ctypes
DBG_LIB_PATH = os.path.join(_PKG, "lib", "libmvslam_hip_dbg.so")
if os.environ.get("MVS_USE_DEBUG_LIB") == "1":
    LIB_PATH = DBG_LIB_PATH

MVS_OK = 0
MVS_NO_MODEL = 1
MVS_ERR_INVALID_ARG, MVS_ERR_NO_DEVICE, MVS_ERR_HIP, MVS_ERR_CAPACITY, MVS_ERR_BAD_INTRINSICS = -1, -2, -3, -4, -5
SAMPLER_IDENTITY = 0
SAMPLER_PHILOX = 1

MATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


class Params(C.Structure):
    _fields_ = [
        ("ratio", C.c_double),
        ("max_dist", C.c_double),
        ("max_error_sq", C.c_double),
        ("num_hypotheses", C.c_int32),
        ("sampler", C.c_int32),
        ("seed", C.c_uint64),
        ("min_inliers", C.c_int32),
        ("reserved", C.c_int32),
    ]


class PairResult(C.Structure):
    _fields_ = [
        ("valid", C.c_int32),
        ("n_matches", C.c_int32),
        ("n_inliers", C.c_int32),
        ("n_points", C.c_int32),
        ("best_hyp", C.c_int32),
        ("best_count", C.c_int32),
        ("best_residual", C.c_double),
        ("F", C.c_double * 9),
        ("E", C.c_double * 9),
        ("R1to2", C.c_double * 9),
        ("t1to2", C.c_double * 3),
        ("R", C.c_double * 9),
        ("t", C.c_double * 3),
    ]


RESULT_DTYPE = np.dtype([
    ("valid", "<i4"), ("n_matches", "<i4"), ("n_inliers", "<i4"), ("n_points", "<i4"), ("best_hyp", "<i4"),
    ("best_count", "<i4"), ("best_residual", "<f8"), ("F", "<f8", (3, 3)), ("E", "<f8", (3, 3)),
    ("R1to2", "<f8", (3, 3)), ("t1to2", "<f8", (3,)), ("R", "<f8", (3, 3)), ("t", "<f8", (3,))])
assert RESULT_DTYPE.itemsize == C.sizeof(PairResult)


class PnpParams(C.Structure):
    _fields_ = [("num_hypotheses", C.c_int32), ("sampler", C.c_int32), ("seed", C.c_uint64),
                ("reproj_error", C.c_double), ("min_inliers", C.c_int32), ("refit", C.c_int32)]


TRACK_DTYPE = np.dtype([("ok", "<i4"), ("n_corr", "<i4"), ("n_inliers", "<i4"), ("best_hyp", "<i4"),
                        ("R", "<f8", (3, 3)), ("t", "<f8", (3,))])


class RefineParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved", C.c_int32), ("lambda_initial", C.c_double),
                ("lambda_factor", C.c_double), ("lambda_upper", C.c_double), ("rel_tol", C.c_double),
                ("abs_tol", C.c_double), ("anchor_sigma", C.c_double * 2), ("pose_sigma", C.c_double * 2),
                ("point_sigma", C.c_double)]


class BaProblem(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_points", C.c_int32), ("K", C.POINTER(C.c_double)),
                ("frame_pose", C.POINTER(C.c_double)), ("frame_prior_var", C.POINTER(C.c_double)),
                ("points", C.POINTER(C.c_double)), ("point_prior_cov", C.POINTER(C.c_double)),
                ("obs", C.POINTER(C.c_double) * 2), ("obs_cov", C.POINTER(C.c_double) * 2),
                ("obs_valid", C.POINTER(C.c_uint8) * 2)]


class BaWindow(C.Structure):
    """mvs_ba_window: BaProblem's fields with the per-frame arrays as arrays of n_frames pointers"""
    _fields_ = [("n_frames", C.c_int32), ("n_points", C.c_int32), ("K", C.POINTER(C.c_double)),
                ("frame_pose", C.POINTER(C.c_double)), ("frame_prior_var", C.POINTER(C.c_double)),
                ("points", C.POINTER(C.c_double)), ("point_prior_cov", C.POINTER(C.c_double)),
                ("obs", C.POINTER(C.POINTER(C.c_double))), ("obs_cov", C.POINTER(C.POINTER(C.c_double))),
                ("obs_valid", C.POINTER(C.POINTER(C.c_uint8)))]


class BaSparse(C.Structure):
    """mvs_ba_sparse: a bundle adjustment of up to 4096 frames with the observations as a CSR by point"""
    _fields_ = [("n_frames", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32), ("reserved", C.c_int32),
                ("K", C.POINTER(C.c_double)), ("frame_pose", C.POINTER(C.c_double)),
                ("frame_prior_var", C.POINTER(C.c_double)), ("points", C.POINTER(C.c_double)),
                ("point_prior_cov", C.POINTER(C.c_double)), ("obs_off", C.POINTER(C.c_int32)),
                ("obs_frame", C.POINTER(C.c_int32)), ("obs_uv", C.POINTER(C.c_double)), ("obs_cov", C.POINTER(C.c_double))]


class BaSparseResult(C.Structure):
    _fields_ = [("ok", C.c_int32), ("iterations", C.c_int32), ("rejected_steps", C.c_int32), ("failed_solves", C.c_int32),
                ("error_initial", C.c_double), ("error", C.c_double), ("envelope_blocks", C.c_int32),
                ("widest_row", C.c_int32), ("bad_frame", C.c_int32), ("reserved", C.c_int32)]


REFINE_DTYPE = np.dtype([("ok", "<i4"), ("iterations", "<i4"), ("error", "<f8"), ("R", "<f8", (3, 3)),
                         ("t", "<f8", (3,)), ("pose_cov", "<f8", (6, 6))])


class SeqWindowParams(C.Structure):
    _fields_ = [("window_frames", C.c_int32), ("stride", C.c_int32), ("max_points", C.c_int32), ("reserved", C.c_int32),
                ("sigma_px", C.c_double)]


class SeqWindowInfo(C.Structure):
    _fields_ = [("first_frame", C.c_int32), ("n_frames", C.c_int32), ("n_points", C.c_int32), ("n_tracks_found", C.c_int32)]


WINDOW_INFO_DTYPE = np.dtype([("first_frame", "<i4"), ("n_frames", "<i4"), ("n_points", "<i4"), ("n_tracks_found", "<i4")])


class SeqGlobalParams(C.Structure):
    """mvs_seq_global_params: max_track_frames 0 = uncut tracks, or 2 .. 4096"""
    _fields_ = [("max_track_frames", C.c_int32), ("reserved", C.c_int32), ("sigma_px", C.c_double)]


class SeqScaleParams(C.Structure):
    """mvs_seq_scale_params: rule SEQ_SCALE_CHAIN / SEQ_SCALE_DEPTH_RATIO; min_common >= 1"""
    _fields_ = [("rule", C.c_int32), ("min_common", C.c_int32)]


SEQ_SCALE_CHAIN, SEQ_SCALE_DEPTH_RATIO = 0, 1
SCALE_STEP_DTYPE = np.dtype([("n_common", "<i4"), ("n_used", "<i4"), ("flag", "<i4"), ("reserved", "<i4"), ("scale", "<f8")])


class VoParams(C.Structure):
    """mvs_vo_params: the tracking loop of Sequence.track"""
    _fields_ = [("init_pair", C.c_int32), ("use_refined_init", C.c_int32), ("min_pnp_point_count", C.c_int32),
                ("reserved", C.c_int32), ("max_error", C.c_double), ("anchor_var", C.c_double * 2),
                ("regulator_var", C.c_double * 2), ("point_sigma", C.c_double), ("sigma_px", C.c_double)]


TRACK_NOT_REACHED, TRACK_INIT, TRACK_TRACKED, TRACK_LOST_PNP, TRACK_LOST_FEW, TRACK_LOST_BA, TRACK_LOST_ERROR = range(7)
TRACK_INITIALIZING = 7   # Sequence.odometry only: processed while initialising, and did not initialise


class VoInitParams(C.Structure):
    """mvs_vo_init_params: the frame queue and the initialisation gates of Sequence.odometry"""
    _fields_ = [("frame_queue_size", C.c_int32), ("min_match_inlier_count", C.c_int32),
                ("max_rotation_magnitude", C.c_double), ("max_translation_z", C.c_double)]


ODO_FRAME_DTYPE = np.dtype([("mode_after", "<i4"), ("segment", "<i4"), ("init_base", "<i4"), ("queue_first", "<i4"),
                            ("n_updated", "<i4"), ("gate_fail", "<i4"), ("rot_sq", "<f8"), ("abs_tz", "<f8")])   # mvs_odo_frame
TRACK_FRAME_DTYPE = np.dtype([("state", "<i4"), ("n_cand", "<i4"), ("n_pnp_inliers", "<i4"), ("n_tracked", "<i4"),
                              ("n_new", "<i4"), ("pnp_best_hyp", "<i4"), ("iterations", "<i4"), ("reserved", "<i4"),
                              ("scale", "<f8"), ("error", "<f8"), ("R_pnp", "<f8", (3, 3)), ("t_pnp", "<f8", (3,)),
                              ("R", "<f8", (3, 3)), ("t", "<f8", (3,))])   # mvs_track_frame


class PoseGraph(C.Structure):
    """mvs_pose_graph: one pose graph, every pointer a host pointer"""
    _fields_ = [("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("node_pose", C.POINTER(C.c_double)),
                ("edge_src", C.POINTER(C.c_int32)), ("edge_dst", C.POINTER(C.c_int32)),
                ("edge_pose", C.POINTER(C.c_double)), ("edge_cov", C.POINTER(C.c_double)), ("anchor_node", C.c_int32)]


class PoseGraphParams(C.Structure):
    _fields_ = [("lm", RefineParams), ("anchor_sigma", C.c_double * 2), ("cg_rel_tol", C.c_double),
                ("cg_max_iterations", C.c_int32), ("cg_chunk_iterations", C.c_int32)]


class PoseGraphResult(C.Structure):
    _fields_ = [("ok", C.c_int32), ("iterations", C.c_int32), ("cg_iterations", C.c_int32),
                ("rejected_steps", C.c_int32), ("error_initial", C.c_double), ("error", C.c_double)]


class Sim3Graph(C.Structure):
    """mvs_sim3_graph: one pose graph over Sim(3), every pointer a host pointer"""
    _fields_ = [("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("node_sim3", C.POINTER(C.c_double)),
                ("edge_src", C.POINTER(C.c_int32)), ("edge_dst", C.POINTER(C.c_int32)),
                ("edge_sim3", C.POINTER(C.c_double)), ("edge_cov", C.POINTER(C.c_double)), ("anchor_node", C.c_int32)]


class Sim3GraphParams(C.Structure):
    _fields_ = [("lm", RefineParams), ("anchor_sigma", C.c_double * 3), ("cg_rel_tol", C.c_double),
                ("cg_max_iterations", C.c_int32), ("cg_chunk_iterations", C.c_int32)]


POSE_GRAPH_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("iterations", "<i4"), ("cg_iterations", "<i4"),
                                    ("rejected_steps", "<i4"), ("error_initial", "<f8"), ("error", "<f8")])
assert POSE_GRAPH_RESULT_DTYPE.itemsize == C.sizeof(PoseGraphResult)
POSE_GRAPH_DENSE_MAX_NODES, POSE_GRAPH_MAX_NODES, POSE_GRAPH_MAX_EDGES = 16, 4096, 65536
POSE_GRAPH_MARGINALS_INFO_DTYPE = np.dtype([("ok", "<i4"), ("envelope_blocks", "<i4"), ("bad_node", "<i4"), ("reserved", "<i4"),
                                            ("min_pivot", "<f8")])
POSE_GRAPH_MAX_ENVELOPE_BLOCKS = 1 << 21
MVS_PG_SOLVER_PCG, MVS_PG_SOLVER_DIRECT = 0, 1
MVS_PG_LOSS_NONE, MVS_PG_LOSS_HUBER, MVS_PG_LOSS_CAUCHY = 0, 1, 2
MVS_PG_LOSS_LOOP_EDGES = -1
MVS_BA_LOSS_NONE, MVS_BA_LOSS_HUBER, MVS_BA_LOSS_CAUCHY = 0, 1, 2
POSE_GRAPH_DIRECT_INFO_DTYPE = np.dtype([("envelope_blocks", "<i4"), ("widest_row", "<i4"), ("failed_solves", "<i4"),
                                         ("bad_node", "<i4"), ("min_pivot", "<f8"), ("failed_pivot", "<f8")])


def _marginals_args(n_nodes, queries, anchor_sigma, cov_out):
    """(sigma, n_query, query_i, query_j, cov_out, info) of the two marginals calls; queries None = every diagonal block"""
    sig = anchor_sigma if anchor_sigma is not None else (1e-4, 1e-4)   # mvs_pose_graph_params_default's
    sigma = (C.c_double * 2)(float(sig[0]), float(sig[1]))
    if queries is None:
        qi = qj = None
        n = 0
        rows = n_nodes
    else:
        q = np.asarray(queries, dtype=np.int32).reshape(-1, 2)
        qi, qj = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])
        n = rows = len(qi)
        if n == 0:
            raise ValueError("an empty query list: pass None for every diagonal block")
    if cov_out is None:
        cov_out = np.zeros((rows, 6, 6))
    assert cov_out.dtype == np.float64 and cov_out.flags.c_contiguous and cov_out.shape == (rows, 6, 6)
    return sigma, n, qi, qj, cov_out, np.zeros(1, dtype=POSE_GRAPH_MARGINALS_INFO_DTYPE)


class SeqGraphParams(C.Structure):
    """mvs_seq_graph_params: which resident lagged pairs become edges of the sequence's pose graph"""
    _fields_ = [("max_lag", C.c_int32), ("min_points", C.c_int32), ("max_error", C.c_double), ("chain_sigma", C.c_double * 2)]


SEQ_GRAPH_EDGE_MEASURED, SEQ_GRAPH_EDGE_CHAIN, SEQ_GRAPH_EDGE_LOOP = 0, 1, 2


class LoopSelectParams(C.Structure):
    """mvs_loop_select_params: which scored frame pairs become loop-closure candidates"""
    _fields_ = [("min_score", C.c_int32), ("top_k", C.c_int32), ("max_candidates", C.c_int32), ("reserved", C.c_int32)]


class LoopEdgeParams(C.Structure):
    """mvs_loop_edge_params: the gates and the extra covariance of the loop edges"""
    _fields_ = [("min_points", C.c_int32), ("reserved", C.c_int32), ("max_error", C.c_double), ("loop_sigma", C.c_double * 2)]


LOOP_CANDIDATE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("score", "<i4"), ("accepted", "<i4")])
LOOP_MAX_FRAMES = 4096


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("nlevels", C.c_int32), ("edge_threshold", C.c_int32),
                ("fast_threshold", C.c_int32)]


KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])   # cv::KeyPoint


class WorkStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("hypotheses", "rotations9", "pairs9", "score_evals", "matches", "inliers",
                                              "score_evals_executed", "score_evals_executed_f32", "exact_solves",
                                              "prescreened")] + [("pairs_mode", C.c_int64 * 3),
                                                                 ("score_evals_executed_mfma", C.c_int64),
                                                                 ("score_evals_executed_mfma_finish", C.c_int64),
                                                                 ("max_sweeps9", C.c_int64), ("dense_points", C.c_int64),
                                                                 ("matches_mode1", C.c_int64), ("score_evals_executed_mfma_rest", C.c_int64),
                                                                 ("score_evals_executed_mfma_pilot", C.c_int64)]


class KernelInfo(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("symbol", C.c_char * 160)] + [(n, C.c_int32) for n in (
        "kernel_id", "threads_per_block", "num_regs", "static_lds_bytes", "dynamic_lds_bytes", "scratch_bytes_per_lane",
        "max_threads_per_block", "blocks_per_cu", "waves_per_simd", "reserved")]


EXPORTS = [
    "mvs_abi_version", "mvs_status_str", "mvs_last_error", "mvs_params_default", "mvs_ctx_create",
    "mvs_ctx_create_on_stream", "mvs_ctx_destroy", "mvs_ctx_stream", "mvs_match_hamming", "mvs_two_view",
    "mvs_triangulate", "mvs_recover_pose", "mvs_find_fundamental_matrix", "mvs_ransac_fundamental",
    "mvs_batch_create", "mvs_batch_destroy", "mvs_batch_upload", "mvs_batch_run", "mvs_batch_sync",
    "mvs_batch_time", "mvs_batch_download", "mvs_batch_stats", "mvs_batch_results_device",
    "mvs_batch_copy_results_device", "mvs_pnp_params_default", "mvs_pnp_solve", "mvs_seq_create", "mvs_seq_destroy",
    "mvs_seq_upload", "mvs_seq_run", "mvs_seq_sync", "mvs_seq_time", "mvs_seq_download_pairs", "mvs_seq_download_tracks",
    "mvs_refine_params_default", "mvs_sfm_refine", "mvs_pnp_refine", "mvs_batch_refine", "mvs_batch_download_refined",
    "mvs_orb_params_default", "mvs_extract", "mvs_seq_upload_images", "mvs_seq_refine_pairs", "mvs_seq_download_refined",
    "mvs_ba_refine", "mvs_seq_download_trajectory", "mvs_batch_upload_octaves", "mvs_seq_upload_octaves",
    "mvs_batch_upload_async", "mvs_batch_download_async", "mvs_host_alloc", "mvs_host_free", "mvs_image_pair",
    "mvs_batch_gather_results", "mvs_seq_time_stages", "mvs_batch_time_kernels", "mvs_kernel_info_get",
    "mvs_extract_time", "mvs_ctx_set_half_batches", "mvs_batch_device_state", "mvs_batch_run_points",
    "mvs_ba_refine_window", "mvs_ba_refine_windows", "mvs_ba_refine_sparse", "mvs_seq_refine_windows", "mvs_seq_window_count",
    "mvs_seq_download_windows", "mvs_five_point", "mvs_ransac_essential", "mvs_two_view_essential",
    "mvs_batch_run_points_essential", "mvs_ctx_set_essential_confidence", "mvs_ctx_essential_hypotheses_run",
    "mvs_batch_download_hypotheses_run", "mvs_image_pair_essential", "mvs_batch_run_essential",
    "mvs_batch_download_essential_tables", "mvs_seq_run_essential", "mvs_seq_download_hypotheses_run",
    "mvs_vo_params_default", "mvs_seq_track", "mvs_seq_download_track_frames", "mvs_seq_download_track_map",
    "mvs_seq_download_track_step", "mvs_seq_run_lags", "mvs_seq_download_lag_pairs", "mvs_seq_download_lag_refined",
    "mvs_vo_init_params_default", "mvs_seq_odometry", "mvs_seq_download_odometry_frames",
    "mvs_pose_graph_params_default", "mvs_pose_graph_optimize", "mvs_pose_graph_optimize_batch",
    "mvs_seq_build_pose_graph", "mvs_seq_optimize_pose_graph", "mvs_seq_download_pose_graph",
    "mvs_seq_download_pose_graph_poses", "mvs_seq_loop_scores", "mvs_seq_download_loop_scores", "mvs_seq_select_loops",
    "mvs_seq_verify_loops", "mvs_seq_add_loop_edges", "mvs_seq_download_loop_candidates",
    "mvs_pose_graph_marginals", "mvs_seq_pose_graph_marginals",
    "mvs_ctx_set_pose_graph_solver", "mvs_ctx_pose_graph_direct_info",
    "mvs_ctx_set_pose_graph_loss", "mvs_pose_graph_edge_stats", "mvs_seq_pose_graph_edge_stats",
    "mvs_ctx_set_ba_loss", "mvs_ba_sparse_obs_stats", "mvs_seq_global_obs_stats",
    "mvs_seq_refine_global", "mvs_seq_global_counts", "mvs_seq_download_global", "mvs_seq_download_global_problem",
    "mvs_seq_rescale", "mvs_seq_download_scale_steps",
    "mvs_sim3_graph_params_default", "mvs_sim3_graph_optimize", "mvs_sim3_graph_optimize_batch",
    "mvs_seq_optimize_pose_graph_sim3", "mvs_seq_download_pose_graph_sim3",
]


_dbg = None


def dbg_lib():
    """The diagnostics library, loaded SIDE BY SIDE with the product one (its own handle, its own copy of every symbol): the
    tests let the product binary run the stage and hand its device state to this library's audit (mvs_debug_audit_state)."""
    global _dbg
    if _dbg is None:
        if not os.path.exists(DBG_LIB_PATH):
            raise RuntimeError("libmvslam_hip_dbg.so is missing (%s): make -C mvslam_amd/csrc" % DBG_LIB_PATH)
        _dbg = C.CDLL(DBG_LIB_PATH)
        _dbg.mvs_last_error.restype = C.c_char_p
        _dbg.mvs_last_error.argtypes = [C.c_void_p]
        _dbg.mvs_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        _dbg.mvs_ctx_destroy.argtypes = [C.c_void_p]
        _dbg.mvs_debug_audit_state.restype = C.c_int
        _dbg.mvs_debug_audit_state.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
        _dbg.mvs_debug_seq_global_plan.restype = C.c_int
        _dbg.mvs_debug_seq_global_plan.argtypes = [C.c_void_p] * 12
    return _dbg


class MvsError(RuntimeError):
    def __init__(self, status, what):
        super().__init__("%s: status %d (%s)" % (what, status, status_str(status)))
        self.status = status


_lib = None


def lib():
    """Load the HIP library; raises (loudly) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libmvslam_hip.so is missing (%s): build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C mvslam_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.mvs_status_str.restype = C.c_char_p
        _lib.mvs_last_error.restype = C.c_char_p
        _lib.mvs_last_error.argtypes = [C.c_void_p]
        _lib.mvs_ctx_stream.restype = C.c_void_p
        _lib.mvs_ctx_set_half_batches.restype = C.c_int
        _lib.mvs_ctx_set_half_batches.argtypes = [C.c_void_p, C.c_int]
        _lib.mvs_ctx_stream.argtypes = [C.c_void_p]
        _lib.mvs_ctx_set_essential_confidence.restype = C.c_int
        _lib.mvs_ctx_set_essential_confidence.argtypes = [C.c_void_p, C.c_double]
        _lib.mvs_ctx_essential_hypotheses_run.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        _lib.mvs_ctx_set_pose_graph_solver.restype = C.c_int
        _lib.mvs_ctx_set_pose_graph_solver.argtypes = [C.c_void_p, C.c_int]
        _lib.mvs_ctx_set_pose_graph_loss.restype = C.c_int
        _lib.mvs_ctx_set_pose_graph_loss.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int32]
        _lib.mvs_pose_graph_edge_stats.restype = C.c_int
        _lib.mvs_pose_graph_edge_stats.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                   C.POINTER(C.c_double)]
        _lib.mvs_seq_pose_graph_edge_stats.restype = C.c_int
        _lib.mvs_seq_pose_graph_edge_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib.mvs_ctx_pose_graph_direct_info.restype = C.c_int
        _lib.mvs_ctx_pose_graph_direct_info.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mvs_batch_download_hypotheses_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        _lib.mvs_seq_download_hypotheses_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        _lib.mvs_batch_download_essential_tables.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                                             C.POINTER(C.c_int32)]
        _lib.mvs_ctx_destroy.argtypes = [C.c_void_p]
        _lib.mvs_batch_destroy.argtypes = [C.c_void_p]
        _lib.mvs_seq_destroy.argtypes = [C.c_void_p]
        _lib.mvs_seq_window_count.argtypes = [C.c_void_p, C.c_void_p]
        _lib.mvs_seq_refine_global.argtypes = [C.c_void_p] * 4
        _lib.mvs_seq_global_counts.argtypes = [C.c_void_p] * 3
        _lib.mvs_seq_download_global.argtypes = [C.c_void_p] * 5
        _lib.mvs_seq_download_global_problem.argtypes = [C.c_void_p] * 8
        _lib.mvs_seq_rescale.argtypes = [C.c_void_p] * 2
        _lib.mvs_seq_download_scale_steps.argtypes = [C.c_void_p] * 2
        _lib.mvs_ctx_set_ba_loss.restype = C.c_int
        _lib.mvs_ctx_set_ba_loss.argtypes = [C.c_void_p, C.c_int, C.c_double]
        _lib.mvs_ba_sparse_obs_stats.restype = C.c_int
        _lib.mvs_ba_sparse_obs_stats.argtypes = [C.c_void_p, C.c_void_p] + [C.POINTER(C.c_double)] * 4
        _lib.mvs_seq_global_obs_stats.restype = C.c_int
        _lib.mvs_seq_global_obs_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib.mvs_vo_params_default.restype = None
        _lib.mvs_vo_init_params_default.restype = None
    return _lib


def status_str(status):
    return lib().mvs_status_str(C.c_int(status)).decode()


def default_params(**kw):
    p = Params()
    lib().mvs_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_pnp_params(**kw):
    p = PnpParams()
    lib().mvs_pnp_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_vo_params(**kw):
    p = VoParams()
    lib().mvs_vo_params_default(C.byref(p))
    for k, v in kw.items():
        if k in ("anchor_var", "regulator_var"):
            getattr(p, k)[0], getattr(p, k)[1] = float(v[0]), float(v[1])
        else:
            setattr(p, k, v)
    return p


def default_vo_init_params(**kw):
    p = VoInitParams()
    lib().mvs_vo_init_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_orb_params(**kw):
    p = OrbParams()
    lib().mvs_orb_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_refine_params(**kw):
    p = RefineParams()
    lib().mvs_refine_params_default(C.byref(p))
    for k, v in kw.items():
        if k in ("anchor_sigma", "pose_sigma"):
            getattr(p, k)[0], getattr(p, k)[1] = float(v[0]), float(v[1])
        else:
            setattr(p, k, v)
    return p


def default_pose_graph_params(**kw):
    """mvs_pose_graph_params_default; keywords name a field of the struct or an LM field of its `lm` member"""
    p = PoseGraphParams()
    lib().mvs_pose_graph_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "anchor_sigma":
            p.anchor_sigma[0], p.anchor_sigma[1] = float(v[0]), float(v[1])
        elif k in ("cg_rel_tol", "cg_max_iterations", "cg_chunk_iterations"):
            setattr(p, k, v)
        else:
            setattr(p.lm, k, v)
    return p


def default_sim3_graph_params(**kw):
    """mvs_sim3_graph_params_default; keywords name a field of the struct or an LM field of its `lm` member"""
    p = Sim3GraphParams()
    lib().mvs_sim3_graph_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "anchor_sigma":
            p.anchor_sigma[0], p.anchor_sigma[1], p.anchor_sigma[2] = float(v[0]), float(v[1]), float(v[2])
        elif k in ("cg_rel_tol", "cg_max_iterations", "cg_chunk_iterations"):
            setattr(p, k, v)
        else:
            setattr(p.lm, k, v)
    return p


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def pinned_empty(shape, dtype):
    """numpy array over pinned (page-locked) host memory from mvs_host_alloc: the asynchronous transfers of
    Batch.upload_async / download_async are true DMA copies on such buffers.  Free with pinned_free()."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    p = C.c_void_p()
    st = lib().mvs_host_alloc(C.c_size_t(max(n, 1)), C.byref(p))
    if st != MVS_OK:
        raise MvsError(st, "mvs_host_alloc")
    buf = (C.c_char * max(n, 1)).from_address(p.value)
    a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    _PINNED[a.ctypes.data] = p
    return a


_PINNED = {}


def pinned_free(a):
    p = _PINNED.pop(a.ctypes.data, None)
    if p is not None:
        lib().mvs_host_free(p)


def _ba_sparse_problem(K, frame_pose, frame_prior_var, points, point_prior_cov, obs_off, obs_frame, obs_uv, obs_cov, n_frames):
    """(mvs_ba_sparse, the arrays it points into, n_frames, n_points, n_obs) of ba_refine_sparse's keyword arguments"""
    fp, fv = _f64(frame_pose).reshape(-1, 12), _f64(frame_prior_var).reshape(-1, 6)
    pg, Kc = _f64(points).reshape(-1, 3), _f64(K, (9,))
    off = np.ascontiguousarray(obs_off, dtype=np.int32)
    ofr = np.ascontiguousarray(obs_frame, dtype=np.int32)
    uv = _f64(obs_uv).reshape(-1, 2)
    F, m, n_obs = len(fp) if n_frames is None else n_frames, len(pg), len(ofr)
    pb = BaSparse()
    pb.n_frames, pb.n_points, pb.n_obs = F, m, n_obs
    pb.K, pb.frame_pose, pb.frame_prior_var, pb.points = (_ptr(Kc, C.c_double), _ptr(fp, C.c_double), _ptr(fv, C.c_double),
                                                          _ptr(pg, C.c_double))
    pc = None if point_prior_cov is None else _f64(point_prior_cov, (m, 9))
    oc = None if obs_cov is None else _f64(obs_cov, (n_obs, 4))
    pb.point_prior_cov, pb.obs_cov = _ptr(pc, C.c_double), _ptr(oc, C.c_double)
    pb.obs_off, pb.obs_frame, pb.obs_uv = _ptr(off, C.c_int32), _ptr(ofr, C.c_int32), _ptr(uv, C.c_double)
    return pb, (Kc, fp, fv, pg, pc, oc, off, ofr, uv), F, m, n_obs


class Context:
    """One mvs_ctx: one HIP stream on one GPU."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self._children = weakref.WeakSet()  # batches / sequences must be destroyed before their context
        st = lib().mvs_ctx_create_on_stream(C.c_int(device), C.c_void_p(stream), C.byref(self._h))
        if st != MVS_OK:
            raise MvsError(st, "mvs_ctx_create")

    def close(self):
        if self._h:
            for child in list(self._children):
                child.close()
            lib().mvs_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().mvs_ctx_stream(self._h)

    def set_half_batches(self, enable):
        """Large batches as two halves on two streams (default) or every launch on the one stream."""
        self._check(lib().mvs_ctx_set_half_batches(self._h, C.c_int(1 if enable else 0)), "mvs_ctx_set_half_batches")

    def set_essential_confidence(self, p):
        """Confidence level of the five-point RANSAC: 0 (default) runs every hypothesis, 0 < p < 1 stops each pair at the first
        checkpoint (64, 128, ...) at which its best count reaches that confidence (mvs_ctx_set_essential_confidence)."""
        self._check(lib().mvs_ctx_set_essential_confidence(self._h, C.c_double(p)), "mvs_ctx_set_essential_confidence")

    def set_pose_graph_solver(self, solver):
        """The linear solver of pose graphs of more than 16 nodes: MVS_PG_SOLVER_PCG (default) or MVS_PG_SOLVER_DIRECT, the
        block-scaled skyline Cholesky (mvs_ctx_set_pose_graph_solver).  Anything else raises MvsError (MVS_ERR_INVALID_ARG)."""
        self._check(lib().mvs_ctx_set_pose_graph_solver(self._h, C.c_int(solver)), "mvs_ctx_set_pose_graph_solver")

    def set_pose_graph_loss(self, loss, k=1.0, first_edge=0):
        """The robust loss of the pose graphs' edges (mvs_ctx_set_pose_graph_loss): MVS_PG_LOSS_NONE (default),
        MVS_PG_LOSS_HUBER or MVS_PG_LOSS_CAUCHY with the constant k, on the edges with index >= first_edge inside their graph
        (MVS_PG_LOSS_LOOP_EDGES: the loop edges of a resident graph).  A refused setting raises MvsError
        (MVS_ERR_INVALID_ARG) and leaves the previous one in force."""
        self._check(lib().mvs_ctx_set_pose_graph_loss(self._h, C.c_int(loss), C.c_double(k), C.c_int32(first_edge)),
                    "mvs_ctx_set_pose_graph_loss")

    def set_ba_loss(self, loss, k=1.0):
        """The robust loss of the observation terms of ba_refine_sparse and Sequence.refine_global (mvs_ctx_set_ba_loss):
        MVS_BA_LOSS_NONE (default), MVS_BA_LOSS_HUBER or MVS_BA_LOSS_CAUCHY with the constant k.  Every other bundle adjustment
        ignores it.  A refused setting raises MvsError (MVS_ERR_INVALID_ARG) and leaves the earlier one in place."""
        self._check(lib().mvs_ctx_set_ba_loss(self._h, C.c_int(loss), C.c_double(k)), "mvs_ctx_set_ba_loss")

    def pose_graph_edge_stats(self, graph, poses=None):
        """mvs_pose_graph_edge_stats: (status, chi2 [E], weight [E]) at `poses` (None: the graph's node_pose) -- the squared norm
        of every edge's whitened residual and its weight under the context's loss.  MVS_NO_MODEL is returned (the arrays are
        then zero); argument and capacity errors raise MvsError."""
        npose = _f64(graph["node_pose"]).reshape(-1, 12)
        src = np.ascontiguousarray(graph["edge_src"], dtype=np.int32).reshape(-1)
        dst = np.ascontiguousarray(graph["edge_dst"], dtype=np.int32).reshape(-1)
        ep = _f64(graph["edge_pose"]).reshape(-1, 12)
        ec = _f64(graph["edge_cov"]).reshape(-1, 36)
        if not (len(src) == len(dst) == len(ep) == len(ec)):
            raise ValueError("pose graph: the per-edge arrays differ in length")
        g = PoseGraph(npose.shape[0], len(src), _ptr(npose, C.c_double), _ptr(src, C.c_int32), _ptr(dst, C.c_int32),
                      _ptr(ep, C.c_double), _ptr(ec, C.c_double), int(graph.get("anchor", 0)))
        X = None
        if poses is not None:
            X = _f64(poses).reshape(-1, 12)
            if X.shape[0] != npose.shape[0]:
                raise ValueError("pose graph: `poses` has another node count than the graph")
        chi2, weight = np.zeros(max(len(src), 1)), np.zeros(max(len(src), 1))
        st = lib().mvs_pose_graph_edge_stats(self._h, C.byref(g), _ptr(X, C.c_double), _ptr(chi2, C.c_double),
                                             _ptr(weight, C.c_double))
        self._check(st, "mvs_pose_graph_edge_stats", allow_no_model=True)
        return st, chi2[:len(src)], weight[:len(src)]

    def pose_graph_direct_info(self):
        """what the direct solver met in the last graph that went through it (mvs_ctx_pose_graph_direct_info): a record of
        POSE_GRAPH_DIRECT_INFO_DTYPE"""
        info = np.zeros(1, dtype=POSE_GRAPH_DIRECT_INFO_DTYPE)
        self._check(lib().mvs_ctx_pose_graph_direct_info(self._h, info.ctypes.data_as(C.c_void_p)),
                    "mvs_ctx_pose_graph_direct_info")
        return info[0]

    def essential_hypotheses_run(self):
        """hypotheses that took part in the last single-shot five-point call (mvs_ctx_essential_hypotheses_run)"""
        n = C.c_int32(0)
        self._check(lib().mvs_ctx_essential_hypotheses_run(self._h, C.byref(n)), "mvs_ctx_essential_hypotheses_run")
        return n.value

    def _check(self, st, what, allow_no_model=False):
        if st == MVS_OK or (allow_no_model and st == MVS_NO_MODEL):
            return st
        err = lib().mvs_last_error(self._h)
        raise MvsError(st, what + (" [" + err.decode() + "]" if err else ""))

    def kernel_info(self, max_kp=2000, desc_bytes=32):
        """the kernels of the two-view pipeline as launched for this batch shape: what the RUNTIME reports for the loaded
        code object (registers, LDS, scratch, occupancy), merged with the build's resource-usage digest
        (lib/kernel_resources.json: the VGPR / AGPR split) when that file is present.  {name: {...}}, launch order"""
        import json
        build = {}
        rpath = os.path.join(_PKG, "lib", "kernel_resources.json")
        if os.path.exists(rpath):
            build = json.load(open(rpath))
        out = {}
        i = 0
        while True:
            ki = KernelInfo()
            st = lib().mvs_kernel_info_get(self._h, C.c_int(i), C.c_int(max_kp), C.c_int(desc_bytes), C.byref(ki))
            if st == MVS_ERR_INVALID_ARG:
                break
            self._check(st, "mvs_kernel_info_get")
            d = {n: getattr(ki, n) for n, _ in KernelInfo._fields_[2:] if n != "reserved"}
            d["symbol"] = ki.symbol.decode()
            bres = build.get(d["symbol"])
            if bres:
                d["build"] = bres
            out[ki.name.decode()] = d
            i += 1
        return out

    def _pose_graph_call(self, graphs, params, poses_out, single):
        """one graph through mvs_pose_graph_optimize (`single`) or a list through mvs_pose_graph_optimize_batch"""
        params = params or default_pose_graph_params()
        G = len(graphs)
        arr = (PoseGraph * max(G, 1))()
        keep = []
        nmax = 0
        for i, g in enumerate(graphs):
            npose = _f64(g["node_pose"]).reshape(-1, 12)
            src = np.ascontiguousarray(g["edge_src"], dtype=np.int32).reshape(-1)
            dst = np.ascontiguousarray(g["edge_dst"], dtype=np.int32).reshape(-1)
            ep = _f64(g["edge_pose"]).reshape(-1, 12)
            ec = _f64(g["edge_cov"]).reshape(-1, 36)
            if not (len(src) == len(dst) == len(ep) == len(ec)):
                raise ValueError("pose graph %d: the per-edge arrays differ in length" % i)
            keep.append((npose, src, dst, ep, ec))
            arr[i].n_nodes, arr[i].n_edges = npose.shape[0], len(src)
            arr[i].node_pose = _ptr(npose, C.c_double)
            arr[i].edge_src, arr[i].edge_dst = _ptr(src, C.c_int32), _ptr(dst, C.c_int32)
            arr[i].edge_pose, arr[i].edge_cov = _ptr(ep, C.c_double), _ptr(ec, C.c_double)
            arr[i].anchor_node = int(g.get("anchor", 0))
            nmax = max(nmax, npose.shape[0])
        if poses_out is None:
            poses_out = np.zeros((G, nmax, 12))
        assert poses_out.dtype == np.float64 and poses_out.flags.c_contiguous and poses_out.shape == (G, nmax, 12)
        res = np.zeros(G, dtype=POSE_GRAPH_RESULT_DTYPE)
        if single:
            st = lib().mvs_pose_graph_optimize(self._h, arr, C.byref(params), res.ctypes.data_as(C.c_void_p),
                                               _ptr(poses_out, C.c_double))
        else:
            st = lib().mvs_pose_graph_optimize_batch(self._h, arr, C.c_int(G), C.byref(params),
                                                     res.ctypes.data_as(C.c_void_p), _ptr(poses_out, C.c_double))
        self._check(st, "mvs_pose_graph_optimize", allow_no_model=True)
        return st, res, poses_out

    def pose_graph_optimize_batch(self, graphs, params=None, poses_out=None):
        """mvs_pose_graph_optimize_batch.  graphs: dicts with node_pose (N x 12: R row-major, then t), edge_src, edge_dst,
        edge_pose (E x 12), edge_cov (E x 6 x 6) and anchor (default 0).  Returns
        (status, results[POSE_GRAPH_RESULT_DTYPE], poses n_graphs x Nmax x 12); `poses_out` (that shape, float64,
        contiguous) is written in place when given, rows the library does not write keep their bytes.  Argument and
        capacity errors raise MvsError; MVS_NO_MODEL is returned."""
        return self._pose_graph_call(graphs, params, poses_out, False)

    def pose_graph_optimize(self, graph, params=None, poses_out=None):
        """mvs_pose_graph_optimize: (status, result record, poses N x 12)"""
        if poses_out is not None:
            poses_out = poses_out.reshape(1, -1, 12)
        st, res, poses = self._pose_graph_call([graph], params, poses_out, True)
        return st, res[0], poses[0]

    def _sim3_graph_call(self, graphs, params, nodes_out, single):
        """one graph through mvs_sim3_graph_optimize (`single`) or a list through mvs_sim3_graph_optimize_batch"""
        params = params or default_sim3_graph_params()
        G = len(graphs)
        arr = (Sim3Graph * max(G, 1))()
        keep = []
        nmax = 0
        for i, g in enumerate(graphs):
            node = _f64(g["node_sim3"]).reshape(-1, 13)
            src = np.ascontiguousarray(g["edge_src"], dtype=np.int32).reshape(-1)
            dst = np.ascontiguousarray(g["edge_dst"], dtype=np.int32).reshape(-1)
            ez = _f64(g["edge_sim3"]).reshape(-1, 13)
            ec = _f64(g["edge_cov"]).reshape(-1, 49)
            if not (len(src) == len(dst) == len(ez) == len(ec)):
                raise ValueError("sim3 graph %d: the per-edge arrays differ in length" % i)
            keep.append((node, src, dst, ez, ec))
            arr[i].n_nodes, arr[i].n_edges = int(g.get("n_nodes", node.shape[0])), int(g.get("n_edges", len(src)))
            arr[i].node_sim3 = _ptr(node, C.c_double)
            arr[i].edge_src, arr[i].edge_dst = _ptr(src, C.c_int32), _ptr(dst, C.c_int32)
            arr[i].edge_sim3, arr[i].edge_cov = _ptr(ez, C.c_double), _ptr(ec, C.c_double)
            arr[i].anchor_node = int(g.get("anchor", 0))
            nmax = max(nmax, node.shape[0])
        if nodes_out is None:
            nodes_out = np.zeros((G, nmax, 13))
        assert nodes_out.dtype == np.float64 and nodes_out.flags.c_contiguous and nodes_out.shape == (G, nmax, 13)
        res = np.zeros(G, dtype=POSE_GRAPH_RESULT_DTYPE)
        if single:
            st = lib().mvs_sim3_graph_optimize(self._h, arr, C.byref(params), res.ctypes.data_as(C.c_void_p),
                                               _ptr(nodes_out, C.c_double))
        else:
            st = lib().mvs_sim3_graph_optimize_batch(self._h, arr, C.c_int(G), C.byref(params),
                                                     res.ctypes.data_as(C.c_void_p), _ptr(nodes_out, C.c_double))
        self._check(st, "mvs_sim3_graph_optimize", allow_no_model=True)
        return st, res, nodes_out

    def sim3_graph_optimize_batch(self, graphs, params=None, nodes_out=None):
        """mvs_sim3_graph_optimize_batch.  graphs: dicts with node_sim3 (N x 13: R row-major, t, s), edge_src, edge_dst,
        edge_sim3 (E x 13), edge_cov (E x 7 x 7) and anchor (default 0); n_nodes / n_edges, when present, override the counts
        the arrays imply.  Returns (status, results[POSE_GRAPH_RESULT_DTYPE], nodes n_graphs x Nmax x 13); `nodes_out`
        (that shape, float64, contiguous) is written in place when given, rows the library does not write keep their bytes.
        Argument and capacity errors raise MvsError; MVS_NO_MODEL is returned."""
        return self._sim3_graph_call(graphs, params, nodes_out, False)

    def sim3_graph_optimize(self, graph, params=None, nodes_out=None):
        """mvs_sim3_graph_optimize: (status, result record, nodes N x 13)"""
        if nodes_out is not None:
            nodes_out = nodes_out.reshape(1, -1, 13)
        st, res, nodes = self._sim3_graph_call([graph], params, nodes_out, True)
        return st, res[0], nodes[0]

    def pose_graph_marginals(self, graph, poses=None, queries=None, anchor_sigma=None, cov_out=None):
        """mvs_pose_graph_marginals: blocks of Sigma = H^-1 at `poses` (None: the graph's node_pose).  queries: pairs (i, j),
        None = every diagonal block.  Returns (status, info record, cov [n, 6, 6]); `cov_out` (that shape, float64, contiguous)
        is written in place when given and keeps its bytes on MVS_NO_MODEL.  Argument and capacity errors raise MvsError."""
        npose = _f64(graph["node_pose"]).reshape(-1, 12)
        src = np.ascontiguousarray(graph["edge_src"], dtype=np.int32).reshape(-1)
        dst = np.ascontiguousarray(graph["edge_dst"], dtype=np.int32).reshape(-1)
        ep = _f64(graph["edge_pose"]).reshape(-1, 12)
        ec = _f64(graph["edge_cov"]).reshape(-1, 36)
        if not (len(src) == len(dst) == len(ep) == len(ec)):
            raise ValueError("pose graph: the per-edge arrays differ in length")
        g = PoseGraph(npose.shape[0], len(src), _ptr(npose, C.c_double), _ptr(src, C.c_int32), _ptr(dst, C.c_int32),
                      _ptr(ep, C.c_double), _ptr(ec, C.c_double), int(graph.get("anchor", 0)))
        X = None
        if poses is not None:
            X = _f64(poses).reshape(-1, 12)
            if X.shape[0] != npose.shape[0]:
                raise ValueError("pose graph: `poses` has another node count than the graph")
        sigma, n, qi, qj, cov_out, info = _marginals_args(npose.shape[0], queries, anchor_sigma, cov_out)
        st = lib().mvs_pose_graph_marginals(self._h, C.byref(g), _ptr(X, C.c_double), sigma, C.c_int(n), _ptr(qi, C.c_int32),
                                            _ptr(qj, C.c_int32), _ptr(cov_out, C.c_double), info.ctypes.data_as(C.c_void_p))
        self._check(st, "mvs_pose_graph_marginals", allow_no_model=True)
        return st, info[0], cov_out

    # VisualFeature::match_visual_features(vf1 = train, vf2 = query, max_dist)
    def match_hamming(self, train_desc, query_desc, ratio=0.7, max_dist=-1.0):
        train_desc = np.ascontiguousarray(train_desc, dtype=np.uint8)
        query_desc = np.ascontiguousarray(query_desc, dtype=np.uint8)
        nq = int(query_desc.shape[0])
        out = np.zeros(max(nq, 1), dtype=MATCH_DTYPE)
        n = C.c_int(0)
        st = lib().mvs_match_hamming(
            self._h, _ptr(train_desc, C.c_uint8), C.c_int(int(train_desc.shape[0])), _ptr(query_desc, C.c_uint8),
            C.c_int(nq), C.c_int(int(train_desc.shape[1]) if train_desc.ndim == 2 else 0), C.c_double(ratio),
            C.c_double(max_dist), out.ctypes.data_as(C.c_void_p), C.byref(n))
        self._check(st, "mvs_match_hamming")
        return out[:n.value].copy()

    # ImagePair::ImagePair + reconstruct of one pair in one device pass
    def image_pair(self, base_desc, base_kp, pair_desc, pair_kp, K, params):
        return self._image_pair("mvs_image_pair", base_desc, base_kp, pair_desc, pair_kp, K, params)[0]

    def image_pair_essential(self, base_desc, base_kp, pair_desc, pair_kp, K, params):
        """image_pair() with the five-point essential-matrix RANSAC in place of the 8-point one (mvs_image_pair_essential)"""
        out, res = self._image_pair("mvs_image_pair_essential", base_desc, base_kp, pair_desc, pair_kp, K, params)
        out["raw"] = bytes(res)
        out["hypotheses_run"] = self.essential_hypotheses_run()
        return out

    def _image_pair(self, name, base_desc, base_kp, pair_desc, pair_kp, K, params):
        base_desc = np.ascontiguousarray(base_desc, dtype=np.uint8)
        pair_desc = np.ascontiguousarray(pair_desc, dtype=np.uint8)
        base_kp = np.ascontiguousarray(base_kp, dtype=np.float32).reshape(-1, 2)
        pair_kp = np.ascontiguousarray(pair_kp, dtype=np.float32).reshape(-1, 2)
        n1, n2 = len(base_desc), len(pair_desc)
        res = PairResult()
        mt = np.zeros(max(n2, 1), dtype=MATCH_DTYPE)
        mask = np.zeros(max(n2, 1), dtype=np.uint8)
        pts = np.zeros((max(n2, 1), 3))
        idx = np.zeros(max(n2, 1), dtype=np.int64)
        st = getattr(lib(), name)(self._h, _ptr(base_desc, C.c_uint8), _ptr(base_kp, C.c_float), C.c_int(n1),
                                  _ptr(pair_desc, C.c_uint8), _ptr(pair_kp, C.c_float), C.c_int(n2),
                                  C.c_int(int(base_desc.shape[1])), _ptr(_f64(K, (9,)), C.c_double), C.byref(params),
                                  C.byref(res), mt.ctypes.data_as(C.c_void_p), _ptr(mask, C.c_uint8),
                                  _ptr(pts, C.c_double), _ptr(idx, C.c_int64))
        self._check(st, name, allow_no_model=True)
        r = np.frombuffer(bytes(res), dtype=RESULT_DTYPE)[0]
        out = self._unpack(res, mask, pts, idx, int(r["n_matches"]))
        out["matches"] = mt[:int(r["n_matches"])].copy()
        out["ok"] = st == MVS_OK
        return out, res

    @staticmethod
    def _unpack(res, mask, pts, idx, m):
        r = np.frombuffer(bytes(res), dtype=RESULT_DTYPE)[0]
        out = {k: (r[k].copy() if isinstance(r[k], np.ndarray) else r[k].item()) for k in RESULT_DTYPE.names}
        out["valid"] = bool(out["valid"])
        n = out["n_points"] if out["valid"] else 0
        out["mask"] = None if mask is None else mask[:m].copy()
        out["points"] = pts[:n].copy()
        out["point_idx"] = idx[:n].copy()
        return out

    def _pose_call(self, name, uv1, uv2, K, head=(), mid=(), mask_out=True):
        """the calls that return a pose share one argument shape:
        name(ctx, *head, uv1, uv2, m, K, *mid, R, t, points, point_idx, n_points, [inlier_mask,] result)"""
        uv1, uv2 = _f64(uv1).reshape(-1, 2), _f64(uv2).reshape(-1, 2)
        m = len(uv1)
        R, t = np.zeros(9), np.zeros(3)
        pts = np.zeros((max(m, 1), 3))
        idx = np.zeros(max(m, 1), dtype=np.int64)
        mask = np.zeros(max(m, 1), dtype=np.uint8) if mask_out else None
        n = C.c_int(0)
        res = PairResult()
        tail = (_ptr(mask, C.c_uint8), C.byref(res)) if mask_out else (C.byref(res),)
        st = getattr(lib(), name)(self._h, *head, _ptr(uv1, C.c_double), _ptr(uv2, C.c_double), C.c_int(m),
                                  _ptr(_f64(K, (9,)), C.c_double), *mid, _ptr(R, C.c_double), _ptr(t, C.c_double),
                                  _ptr(pts, C.c_double), _ptr(idx, C.c_int64), C.byref(n), *tail)
        self._check(st, name, allow_no_model=True)
        out = self._unpack(res, mask, pts, idx, m)
        out["ok"] = st == MVS_OK
        return out, res

    # sfm_solve(p1, p2, K, pose2in1, points, point_indexes)
    def two_view(self, uv1, uv2, K, params):
        return self._pose_call("mvs_two_view", uv1, uv2, K, mid=(C.byref(params),))[0]

    # sfm_solve with find_essential_matrix's five-point branch (USE_OPENCV_ESSENTIAL_MATRIX, sfm-solve.cpp:42-63)
    def two_view_essential(self, uv1, uv2, K, params):
        out, res = self._pose_call("mvs_two_view_essential", uv1, uv2, K, mid=(C.byref(params),))
        out["raw"] = bytes(res)
        out["hypotheses_run"] = self.essential_hypotheses_run()
        return out

    def five_point(self, p1, p2):
        """the minimal solver on the device: (n, E[10][3][3]) for 5 x (x, y) ideal-camera points (mvs_five_point)"""
        p1, p2 = _f64(p1, (10,)), _f64(p2, (10,))
        E = np.zeros((10, 3, 3))
        n = C.c_int(0)
        st = lib().mvs_five_point(self._h, _ptr(p1, C.c_double), _ptr(p2, C.c_double), _ptr(E, C.c_double), C.byref(n))
        self._check(st, "mvs_five_point")
        return n.value, E

    def ransac_essential(self, p1, p2, max_error_sq, H, sampler=SAMPLER_PHILOX, seed=0, per_hyp=False):
        p1, p2 = _f64(p1).reshape(-1, 2), _f64(p2).reshape(-1, 2)
        m = len(p1)
        E = np.zeros((3, 3))
        mask = np.zeros(max(m, 1), dtype=np.uint8)
        bh, bt, bc, br = C.c_int(-1), C.c_int(-1), C.c_int(0), C.c_double(0)
        nr = np.zeros(H, dtype=np.int32) if per_hyp else None
        cnt = np.zeros((H, 10), dtype=np.int32) if per_hyp else None
        st = lib().mvs_ransac_essential(
            self._h, _ptr(p1, C.c_double), _ptr(p2, C.c_double), C.c_int(m), C.c_double(max_error_sq), C.c_int(H),
            C.c_int(sampler), C.c_uint64(seed), _ptr(E, C.c_double), _ptr(mask, C.c_uint8), C.byref(bh), C.byref(bt),
            C.byref(bc), C.byref(br), _ptr(nr, C.c_int32), _ptr(cnt, C.c_int32))
        self._check(st, "mvs_ransac_essential", allow_no_model=True)
        out = dict(ok=st == MVS_OK, E=E, mask=mask[:m], best_hyp=bh.value, best_root=bt.value, best_count=bc.value,
                   best_residual=br.value, hypotheses_run=self.essential_hypotheses_run())
        if per_hyp:
            out["n_roots"], out["count"] = nr, cnt
        return out

    # sfm_triangulate with T_1_to_2 composed by the caller
    def triangulate(self, uv1, uv2, K, R1to2, t1to2):
        uv1, uv2 = _f64(uv1).reshape(-1, 2), _f64(uv2).reshape(-1, 2)
        m = len(uv1)
        pts = np.zeros((max(m, 1), 3))
        idx = np.zeros(max(m, 1), dtype=np.int64)
        n = C.c_int(0)
        st = lib().mvs_triangulate(self._h, _ptr(uv1, C.c_double), _ptr(uv2, C.c_double), C.c_int(m),
                                   _ptr(_f64(K, (9,)), C.c_double), _ptr(_f64(R1to2, (9,)), C.c_double),
                                   _ptr(_f64(t1to2, (3,)), C.c_double), _ptr(pts, C.c_double), _ptr(idx, C.c_int64),
                                   C.byref(n))
        self._check(st, "mvs_triangulate")
        return pts[:n.value].copy(), idx[:n.value].copy()

    def recover_pose(self, E, uv1, uv2, K, mask=None):
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        return self._pose_call("mvs_recover_pose", uv1, uv2, K, head=(_ptr(_f64(E, (9,)), C.c_double),),
                               mid=(_ptr(mk, C.c_uint8),), mask_out=False)[0]

    # pnp_solve(world_points, image_points, K, pose, inlier_point_indexes)
    def pnp_solve(self, world_xyz, image_uv, K, params):
        X, uv = _f64(world_xyz).reshape(-1, 3), _f64(image_uv).reshape(-1, 2)
        n = len(X)
        R, t = np.zeros((3, 3)), np.zeros(3)
        idx = np.zeros(max(n, 1), dtype=np.int64)
        ni, bh = C.c_int(0), C.c_int(-1)
        st = lib().mvs_pnp_solve(self._h, _ptr(X, C.c_double), _ptr(uv, C.c_double), C.c_int(n),
                                 _ptr(_f64(K, (9,)), C.c_double), C.byref(params), _ptr(R, C.c_double),
                                 _ptr(t, C.c_double), _ptr(idx, C.c_int64), C.byref(ni), C.byref(bh))
        self._check(st, "mvs_pnp_solve", allow_no_model=True)
        return dict(ok=st == MVS_OK, R=R, t=t, inliers=idx[:ni.value].copy(), best_hyp=bh.value)

    # VisualFeature::extract(image) for a stack of equally sized grayscale images [B, H, W]
    def extract(self, images, params=None, out=None):
        images = np.ascontiguousarray(images, dtype=np.uint8)
        if images.ndim == 2:
            images = images[None]
        B, H, W = images.shape
        params = params or default_orb_params()
        if out is None:
            kp = np.zeros((B, params.nfeatures), dtype=KEYPOINT_DTYPE)
            desc = np.zeros((B, params.nfeatures, 32), dtype=np.uint8)
            n = np.zeros(B, dtype=np.int32)
        else:   # caller-owned outputs (e.g. pinned_empty() arrays: the copies become DMA transfers)
            kp, desc, n = out["kp"], out["desc"], out["n"]
            assert kp.shape == (B, params.nfeatures) and desc.shape == (B, params.nfeatures, 32) and n.shape == (B,)
        st = lib().mvs_extract(self._h, _ptr(images, C.c_uint8), C.c_int(B), C.c_int(W), C.c_int(H), C.byref(params),
                               kp.ctypes.data_as(C.c_void_p), _ptr(desc, C.c_uint8), _ptr(n, C.c_int32))
        self._check(st, "mvs_extract")
        return dict(kp=kp, desc=desc, n=n)

    # sfm_refine(p1_estimates, p2_estimates, K, pose2in1_guess, pointsin1_guess, pose2in1_estimate, pointsin1_estimate, error)
    def extract_time(self, steps=10):
        """kernel ms of ONE replay of the last extraction's launches (HIP events on the ctx stream, no transfers)"""
        ms = C.c_float(0)
        self._check(lib().mvs_extract_time(self._h, C.c_int(steps), C.byref(ms)), "mvs_extract_time")
        return ms.value / steps

    def sfm_refine(self, p1, cov1, p2, cov2, K, R_guess, t_guess, points_guess, params=None, point_cov=True):
        p1, p2, pg = _f64(p1).reshape(-1, 2), _f64(p2).reshape(-1, 2), _f64(points_guess).reshape(-1, 3)
        m = len(p1)
        params = params or default_refine_params()
        c1 = None if cov1 is None else _f64(cov1, (m, 4))
        c2 = None if cov2 is None else _f64(cov2, (m, 4))
        res = np.zeros(1, dtype=REFINE_DTYPE)
        pts = np.zeros((m, 3))
        ptc = np.zeros((m, 3, 3)) if point_cov else None
        st = lib().mvs_sfm_refine(self._h, _ptr(p1, C.c_double), _ptr(c1, C.c_double), _ptr(p2, C.c_double),
                                  _ptr(c2, C.c_double), C.c_int(m), _ptr(_f64(K, (9,)), C.c_double),
                                  _ptr(_f64(R_guess, (9,)), C.c_double), _ptr(_f64(t_guess, (3,)), C.c_double),
                                  _ptr(pg, C.c_double), C.byref(params), res.ctypes.data_as(C.c_void_p),
                                  _ptr(pts, C.c_double), _ptr(ptc, C.c_double))
        self._check(st, "mvs_sfm_refine", allow_no_model=True)
        r = res[0]
        return dict(ok=st == MVS_OK, R=r["R"].copy(), t=r["t"].copy(), pose_cov=r["pose_cov"].copy(), points=pts,
                    point_cov=ptc, error=float(r["error"]), iterations=int(r["iterations"]))

    # pnp_refine(world_point_estimates, image_point_estimates, K, pose_guess, pose_estimate, error)
    def pnp_refine(self, world, world_cov, image, image_cov, K, R_guess, t_guess, params=None):
        X, uv = _f64(world).reshape(-1, 3), _f64(image).reshape(-1, 2)
        m = len(X)
        params = params or default_refine_params()
        wc = _f64(world_cov, (m, 9))
        ic = None if image_cov is None else _f64(image_cov, (m, 4))
        res = np.zeros(1, dtype=REFINE_DTYPE)
        st = lib().mvs_pnp_refine(self._h, _ptr(X, C.c_double), _ptr(wc, C.c_double), _ptr(uv, C.c_double),
                                  _ptr(ic, C.c_double), C.c_int(m), _ptr(_f64(K, (9,)), C.c_double),
                                  _ptr(_f64(R_guess, (9,)), C.c_double), _ptr(_f64(t_guess, (3,)), C.c_double),
                                  C.byref(params), res.ctypes.data_as(C.c_void_p))
        self._check(st, "mvs_pnp_refine", allow_no_model=True)
        r = res[0]
        return dict(ok=st == MVS_OK, R=r["R"].copy(), t=r["t"].copy(), pose_cov=r["pose_cov"].copy(),
                    error=float(r["error"]), iterations=int(r["iterations"]))

    # ba_frame_pose_and_point for one or two frames (sfm_refine, pnp_refine, VisualOdometer::track_refine)
    def ba_refine(self, K, frame_pose, frame_prior_var, points, point_prior_cov, obs, obs_cov, obs_valid, params=None):
        fp, fv, pg = _f64(frame_pose).reshape(-1, 12), _f64(frame_prior_var).reshape(-1, 6), _f64(points).reshape(-1, 3)
        F, m = len(fp), len(pg)
        params = params or default_refine_params()
        keep = [fp, fv, pg, _f64(K, (9,))]
        pb = BaProblem()
        pb.n_frames, pb.n_points = F, m
        pb.K, pb.frame_pose, pb.frame_prior_var, pb.points = (_ptr(keep[3], C.c_double), _ptr(fp, C.c_double),
                                                            _ptr(fv, C.c_double), _ptr(pg, C.c_double))
        if point_prior_cov is not None:
            keep.append(_f64(point_prior_cov, (m, 9)))
            pb.point_prior_cov = _ptr(keep[-1], C.c_double)
        for f in range(F):
            keep.append(_f64(obs[f], (m, 2)))
            pb.obs[f] = _ptr(keep[-1], C.c_double)
            if obs_cov[f] is not None:
                keep.append(_f64(obs_cov[f], (m, 4)))
                pb.obs_cov[f] = _ptr(keep[-1], C.c_double)
            if obs_valid[f] is not None:
                keep.append(np.ascontiguousarray(obs_valid[f], dtype=np.uint8).reshape(m))
                pb.obs_valid[f] = _ptr(keep[-1], C.c_uint8)
        res = np.zeros(F, dtype=REFINE_DTYPE)
        pts, ptc = np.zeros((m, 3)), np.zeros((m, 3, 3))
        st = lib().mvs_ba_refine(self._h, C.byref(pb), C.byref(params), res.ctypes.data_as(C.c_void_p), _ptr(pts, C.c_double),
                                 _ptr(ptc, C.c_double))
        self._check(st, "mvs_ba_refine", allow_no_model=True)
        return dict(ok=st == MVS_OK, R=res["R"].copy(), t=res["t"].copy(), pose_cov=res["pose_cov"].copy(), points=pts,
                    point_cov=ptc, error=float(res["error"][0]), iterations=int(res["iterations"][0]))

    @staticmethod
    def _ba_window(pb, keep):
        """mvs_ba_window of one problem dict (K, frame_pose, frame_prior_var, points, point_prior_cov, obs, obs_cov, obs_valid;
        the last three are lists over the frames, obs_cov / obs_valid may be None or hold None); the arrays it points to
        are appended to `keep`"""
        fp, fv = _f64(pb["frame_pose"]).reshape(-1, 12), _f64(pb["frame_prior_var"]).reshape(-1, 6)
        pg = _f64(pb["points"]).reshape(-1, 3)
        F, m = len(fp), len(pg)
        K = _f64(pb["K"], (9,))
        keep += [fp, fv, pg, K]
        w = BaWindow()
        w.n_frames, w.n_points = F, m
        w.K, w.frame_pose, w.frame_prior_var, w.points = (_ptr(K, C.c_double), _ptr(fp, C.c_double), _ptr(fv, C.c_double),
                                                          _ptr(pg, C.c_double))
        if pb.get("point_prior_cov") is not None:
            keep.append(_f64(pb["point_prior_cov"], (m, 9)))
            w.point_prior_cov = _ptr(keep[-1], C.c_double)
        obs = (C.POINTER(C.c_double) * F)()
        for f in range(F):
            keep.append(_f64(pb["obs"][f], (m, 2)))
            obs[f] = _ptr(keep[-1], C.c_double)
        keep.append(obs)
        w.obs = C.cast(obs, C.POINTER(C.POINTER(C.c_double)))
        if pb.get("obs_cov") is not None:
            cov = (C.POINTER(C.c_double) * F)()
            for f in range(F):
                if pb["obs_cov"][f] is not None:
                    keep.append(_f64(pb["obs_cov"][f], (m, 4)))
                    cov[f] = _ptr(keep[-1], C.c_double)
            keep.append(cov)
            w.obs_cov = C.cast(cov, C.POINTER(C.POINTER(C.c_double)))
        if pb.get("obs_valid") is not None:
            val = (C.POINTER(C.c_uint8) * F)()
            for f in range(F):
                if pb["obs_valid"][f] is not None:
                    keep.append(np.ascontiguousarray(pb["obs_valid"][f], dtype=np.uint8).reshape(m))
                    val[f] = _ptr(keep[-1], C.c_uint8)
            keep.append(val)
            w.obs_valid = C.cast(val, C.POINTER(C.POINTER(C.c_uint8)))
        return w

    # ba_frame_pose_and_point on windows of 1 .. 8 frames, a batch of them in one launch
    def ba_refine_windows(self, problems, params=None, point_cov=True):
        """problems: list of dicts (see _ba_window).  Returns one result dict per window (the layout of ba_refine's);
        `status` in each is the window's own (MVS_OK, or MVS_NO_MODEL where ok = 0)."""
        params = params or default_refine_params()
        keep = []
        n = len(problems)
        arr = (BaWindow * n)(*[self._ba_window(pb, keep) for pb in problems])
        Fmax = max([w.n_frames for w in arr] + [1])
        Mmax = max([w.n_points for w in arr] + [1])
        res = np.zeros((n, Fmax), dtype=REFINE_DTYPE)
        pts = np.zeros((n, Mmax, 3))
        ptc = np.zeros((n, Mmax, 3, 3)) if point_cov else None
        st = lib().mvs_ba_refine_windows(self._h, arr, C.c_int(n), C.byref(params), res.ctypes.data_as(C.c_void_p),
                                         _ptr(pts, C.c_double), _ptr(ptc, C.c_double))
        self._check(st, "mvs_ba_refine_windows", allow_no_model=True)
        out = []
        for p, w in enumerate(arr):
            F, m = w.n_frames, w.n_points
            r = res[p, :F]
            out.append(dict(ok=bool(r["ok"][0]), status=MVS_OK if r["ok"][0] else MVS_NO_MODEL, R=r["R"].copy(), t=r["t"].copy(), pose_cov=r["pose_cov"].copy(),
                            points=pts[p, :m].copy(), point_cov=None if ptc is None else ptc[p, :m].copy(),
                            error=float(r["error"][0]), iterations=int(r["iterations"][0]), raw=r.tobytes()))
        return out

    def ba_refine_window(self, K, frame_pose, frame_prior_var, points, point_prior_cov, obs, obs_cov, obs_valid, params=None):
        """one window through mvs_ba_refine_window; arguments and result as ba_refine"""
        params = params or default_refine_params()
        keep = []
        w = self._ba_window(dict(K=K, frame_pose=frame_pose, frame_prior_var=frame_prior_var, points=points,
                                 point_prior_cov=point_prior_cov, obs=obs, obs_cov=obs_cov, obs_valid=obs_valid), keep)
        F, m = w.n_frames, w.n_points
        res = np.zeros(max(F, 1), dtype=REFINE_DTYPE)
        pts, ptc = np.zeros((max(m, 1), 3)), np.zeros((max(m, 1), 3, 3))
        st = lib().mvs_ba_refine_window(self._h, C.byref(w), C.byref(params), res.ctypes.data_as(C.c_void_p),
                                        _ptr(pts, C.c_double), _ptr(ptc, C.c_double))
        self._check(st, "mvs_ba_refine_window", allow_no_model=True)
        return dict(ok=st == MVS_OK, R=res["R"].copy(), t=res["t"].copy(), pose_cov=res["pose_cov"].copy(), points=pts[:m],
                    point_cov=ptc[:m], error=float(res["error"][0]), iterations=int(res["iterations"][0]), raw=res[:F].tobytes())

    # ba_frame_pose_and_point on 1 .. 4096 frames, fed as a sparse problem
    def ba_refine_sparse(self, K, frame_pose, frame_prior_var, points, point_prior_cov, obs_off, obs_frame, obs_uv, obs_cov=None,
                         params=None, pose_cov=True, point_cov=True, n_frames=None):
        """mvs_ba_refine_sparse.  obs_off [n_points + 1], obs_frame [n_obs] (ascending within a point), obs_uv [n_obs, 2],
        obs_cov [n_obs, 4] or None.  Returns a dict: status (MVS_OK / MVS_NO_MODEL), ok, the result record's fields, R
        [F, 3, 3], t [F, 3], points, pose_cov / point_cov (None when not asked for) and `raw`, the bytes of every output.  On
        MVS_NO_MODEL the output arrays are as they were allocated (zero).  n_frames overrides the count taken from
        frame_pose (the refusal tests)."""
        params = params or default_refine_params()
        pb, _keep, F, m, n_obs = _ba_sparse_problem(K, frame_pose, frame_prior_var, points, point_prior_cov, obs_off, obs_frame,
                                                    obs_uv, obs_cov, n_frames)
        res = BaSparseResult()
        poses, pts = np.zeros((max(F, 1), 12)), np.zeros((max(m, 1), 3))
        pcv = np.zeros((max(F, 1), 6, 6)) if pose_cov else None
        ptc = np.zeros((max(m, 1), 3, 3)) if point_cov else None
        st = lib().mvs_ba_refine_sparse(self._h, C.byref(pb), C.byref(params), C.byref(res), _ptr(poses, C.c_double),
                                        _ptr(pts, C.c_double), _ptr(pcv, C.c_double), _ptr(ptc, C.c_double))
        self._check(st, "mvs_ba_refine_sparse", allow_no_model=True)
        out = {k: getattr(res, k) for k, _ in BaSparseResult._fields_}
        out.update(status=st, ok=bool(res.ok), R=poses[:, :9].reshape(-1, 3, 3).copy(), t=poses[:, 9:].copy(), points=pts,
                   pose_cov=pcv, point_cov=ptc,
                   raw=b"".join(a.tobytes() for a in (poses, pts, pcv, ptc) if a is not None) + bytes(res))
        return out

    def ba_sparse_obs_stats(self, K, frame_pose, frame_prior_var, points, point_prior_cov, obs_off, obs_frame, obs_uv,
                            obs_cov=None, poses=None, points_at=None, n_frames=None, weight=True):
        """mvs_ba_sparse_obs_stats: (status, chi2 [n_obs], weight [n_obs]) of the problem ba_refine_sparse's arguments describe,
        at `poses` [F, 12] and `points_at` [P, 3] (None: the problem's frame_pose / points): s_o = r_o^T W_o r_o and w(s_o)
        under the context's loss (set_ba_loss; 1.0 without one).  weight=False passes NULL and returns None for it.  A refused
        call returns its status with both arrays as they were allocated (zero)."""
        pb, _keep, F, m, n_obs = _ba_sparse_problem(K, frame_pose, frame_prior_var, points, point_prior_cov, obs_off, obs_frame,
                                                    obs_uv, obs_cov, n_frames)
        X = None if poses is None else _f64(poses).reshape(-1, 12)
        Y = None if points_at is None else _f64(points_at).reshape(-1, 3)
        chi2 = np.zeros(max(n_obs, 1))
        wt = np.zeros(max(n_obs, 1)) if weight else None
        st = lib().mvs_ba_sparse_obs_stats(self._h, C.byref(pb), _ptr(X, C.c_double), _ptr(Y, C.c_double), _ptr(chi2, C.c_double),
                                           _ptr(wt, C.c_double))
        if st not in (MVS_OK, MVS_ERR_INVALID_ARG, MVS_ERR_CAPACITY):
            self._check(st, "mvs_ba_sparse_obs_stats")
        return st, chi2[:n_obs], None if wt is None else wt[:n_obs]

    def find_fundamental_matrix(self, p1, p2):
        p1, p2 = _f64(p1, (16,)), _f64(p2, (16,))
        F = np.zeros((3, 3))
        st = lib().mvs_find_fundamental_matrix(self._h, _ptr(p1, C.c_double), _ptr(p2, C.c_double),
                                               _ptr(F, C.c_double))
        self._check(st, "mvs_find_fundamental_matrix", allow_no_model=True)
        return st == MVS_OK, F

    def ransac_fundamental(self, p1, p2, max_error_sq, H, sampler=SAMPLER_PHILOX, seed=0, per_hyp=False):
        p1, p2 = _f64(p1).reshape(-1, 2), _f64(p2).reshape(-1, 2)
        m = len(p1)
        F = np.zeros((3, 3))
        mask = np.zeros(max(m, 1), dtype=np.uint8)
        bh, bc, br = C.c_int(-1), C.c_int(0), C.c_double(0)
        cnt = np.zeros(H, dtype=np.int32) if per_hyp else None
        res = np.zeros(H, dtype=np.float64) if per_hyp else None
        st = lib().mvs_ransac_fundamental(
            self._h, _ptr(p1, C.c_double), _ptr(p2, C.c_double), C.c_int(m), C.c_double(max_error_sq), C.c_int(H),
            C.c_int(sampler), C.c_uint64(seed), _ptr(F, C.c_double), _ptr(mask, C.c_uint8), C.byref(bh),
            C.byref(bc), C.byref(br), _ptr(cnt, C.c_int32), _ptr(res, C.c_double))
        self._check(st, "mvs_ransac_fundamental", allow_no_model=True)
        out = dict(ok=st == MVS_OK, F=F, mask=mask[:m], best_hyp=bh.value, best_count=bc.value,
                   best_residual=br.value)
        if per_hyp:
            out["count"], out["residual"] = cnt, res
        return out


class Batch:
    """Device-resident batch of image pairs (ImagePair ctor + reconstruct per pair)."""

    def __init__(self, ctx, n_pairs, max_kp, desc_bytes=32):
        self.ctx, self.n_pairs, self.max_kp, self.desc_bytes = ctx, n_pairs, max_kp, desc_bytes
        self._h = C.c_void_p()
        st = lib().mvs_batch_create(ctx._h, C.c_int(n_pairs), C.c_int(max_kp), C.c_int(desc_bytes), C.byref(self._h))
        ctx._check(st, "mvs_batch_create")
        ctx._children.add(self)

    def close(self):
        if self._h:
            if self.ctx._h:  # never touch a batch whose context is already gone
                lib().mvs_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, first, base_desc, base_kp, n_base, pair_desc, pair_kp, n_pair, K, global_index=None):
        count = len(n_base)
        N, D = self.max_kp, self.desc_bytes
        base_desc = np.ascontiguousarray(base_desc, dtype=np.uint8).reshape(count, N, D)
        pair_desc = np.ascontiguousarray(pair_desc, dtype=np.uint8).reshape(count, N, D)
        base_kp = np.ascontiguousarray(base_kp, dtype=np.float32).reshape(count, N, 2)
        pair_kp = np.ascontiguousarray(pair_kp, dtype=np.float32).reshape(count, N, 2)
        n_base = np.ascontiguousarray(n_base, dtype=np.int32)
        n_pair = np.ascontiguousarray(n_pair, dtype=np.int32)
        K = _f64(K)
        if K.size == 9:
            K = np.tile(K.reshape(1, 9), (count, 1))
        K = np.ascontiguousarray(K.reshape(count, 9))
        gi = None if global_index is None else np.ascontiguousarray(global_index, dtype=np.int64)
        st = lib().mvs_batch_upload(self._h, C.c_int(first), C.c_int(count), _ptr(base_desc, C.c_uint8),
                                    _ptr(base_kp, C.c_float), _ptr(n_base, C.c_int32), _ptr(pair_desc, C.c_uint8),
                                    _ptr(pair_kp, C.c_float), _ptr(n_pair, C.c_int32), _ptr(K, C.c_double),
                                    _ptr(gi, C.c_int64))
        self.ctx._check(st, "mvs_batch_upload")

    def upload_async(self, first, base_desc, base_kp, n_base, pair_desc, pair_kp, n_pair, K, global_index):
        """enqueue the upload; the arrays (ideally pinned_empty() ones, exactly typed and contiguous: they are NOT
        copied) must stay alive and unchanged until sync()"""
        count = len(n_base)
        for a, t in ((base_desc, np.uint8), (pair_desc, np.uint8), (base_kp, np.float32), (pair_kp, np.float32),
                     (n_base, np.int32), (n_pair, np.int32), (K, np.float64), (global_index, np.int64)):
            assert a.dtype == t and a.flags["C_CONTIGUOUS"]
        assert K.size == 9 * count
        st = lib().mvs_batch_upload_async(self._h, C.c_int(first), C.c_int(count), _ptr(base_desc, C.c_uint8),
                                          _ptr(base_kp, C.c_float), _ptr(n_base, C.c_int32), _ptr(pair_desc, C.c_uint8),
                                          _ptr(pair_kp, C.c_float), _ptr(n_pair, C.c_int32), _ptr(K, C.c_double),
                                          _ptr(global_index, C.c_int64))
        self.ctx._check(st, "mvs_batch_upload_async")

    def download_async(self, first, count, results, matches=None, mask=None, points=None, point_idx32=None):
        """enqueue the download into caller-owned (ideally pinned) arrays; valid after sync()"""
        st = lib().mvs_batch_download_async(
            self._h, C.c_int(first), C.c_int(count), results.ctypes.data_as(C.c_void_p),
            None if matches is None else matches.ctypes.data_as(C.c_void_p), _ptr(mask, C.c_uint8),
            _ptr(points, C.c_double), _ptr(point_idx32, C.c_int32))
        self.ctx._check(st, "mvs_batch_download_async")

    def run(self, params, n_active=None):
        st = lib().mvs_batch_run(self._h, C.byref(params), C.c_int(n_active or self.n_pairs))
        self.ctx._check(st, "mvs_batch_run")

    def upload_intrinsics(self, first, K, global_index=None, count=None):
        """only K (+ the sampler key offsets) of pairs [first, first + count): what run_points() needs resident"""
        K = _f64(K)
        count = count or (K.size // 9 if K.size > 9 else self.n_pairs - first)
        if K.size == 9:
            K = np.tile(K.reshape(1, 9), (count, 1))
        K = np.ascontiguousarray(K.reshape(count, 9))
        gi = None if global_index is None else np.ascontiguousarray(global_index, dtype=np.int64)
        st = lib().mvs_batch_upload(self._h, C.c_int(first), C.c_int(count), None, None, None, None, None, None,
                                    _ptr(K, C.c_double), _ptr(gi, C.c_int64))
        self.ctx._check(st, "mvs_batch_upload")

    def _run_points(self, name, params, uv1, uv2, m):
        m = np.ascontiguousarray(m, dtype=np.int32)
        count, N = len(m), self.max_kp

        def pad(a):
            a = _f64(a)
            out = np.zeros((count, N, 2))
            out[:, :a.shape[1]] = a.reshape(count, -1, 2)
            return out

        u1, u2 = pad(uv1), pad(uv2)
        st = getattr(lib(), name)(self._h, C.byref(params), C.c_int(count), _ptr(u1, C.c_double), _ptr(u2, C.c_double),
                                  _ptr(m, C.c_int32))
        self.ctx._check(st, name)

    def run_points(self, params, uv1, uv2, m):
        """a batch of sfm_solve calls on matched image points: uv1 / uv2 [count][<= max_kp][2], m [count] (mvs_batch_run_points)"""
        self._run_points("mvs_batch_run_points", params, uv1, uv2, m)

    def run_points_essential(self, params, uv1, uv2, m):
        """run_points() with the five-point essential-matrix RANSAC in place of the 8-point one (mvs_batch_run_points_essential)"""
        self._run_points("mvs_batch_run_points_essential", params, uv1, uv2, m)

    def run_essential(self, params, n_active=None):
        """run() with the five-point essential-matrix RANSAC in place of the 8-point one (mvs_batch_run_essential)"""
        st = lib().mvs_batch_run_essential(self._h, C.byref(params), C.c_int(n_active or self.n_pairs))
        self.ctx._check(st, "mvs_batch_run_essential")

    def download_essential_tables(self, num_hypotheses, first=0, count=None):
        """(n_roots [count][H], count [count][H][10]) of the last five-point run of either kind, in ransac_essential()'s
        convention: count -1 past n_roots, nothing from the pair's n_run on (mvs_batch_download_essential_tables)"""
        count = count or (self.n_pairs - first)
        nr = np.zeros((count, num_hypotheses), dtype=np.int32)
        ct = np.zeros((count, num_hypotheses, 10), dtype=np.int32)
        st = lib().mvs_batch_download_essential_tables(self._h, C.c_int(first), C.c_int(count), C.c_int(num_hypotheses),
                                                       _ptr(nr, C.c_int32), _ptr(ct, C.c_int32))
        self.ctx._check(st, "mvs_batch_download_essential_tables")
        return nr, ct

    def hypotheses_run(self):
        """per pair, the hypotheses that took part in the last run_points_essential or run_essential
        (mvs_batch_download_hypotheses_run)"""
        out = np.zeros(self.n_pairs, dtype=np.int32)
        self.ctx._check(lib().mvs_batch_download_hypotheses_run(self._h, C.c_int(0), C.c_int(self.n_pairs), _ptr(out, C.c_int32)),
                        "mvs_batch_download_hypotheses_run")
        return out

    def device_state(self):
        """opaque bytes of the batch's device-resident state (mvs_batch_device_state): for the diagnostics library's audit"""
        n = C.c_size_t(0)
        self.ctx._check(lib().mvs_batch_device_state(self._h, None, C.c_size_t(0), C.byref(n)), "mvs_batch_device_state")
        buf = (C.c_ubyte * n.value)()
        self.ctx._check(lib().mvs_batch_device_state(self._h, buf, n, C.byref(n)), "mvs_batch_device_state")
        return buf

    def sync(self):
        self.ctx._check(lib().mvs_batch_sync(self._h), "mvs_batch_sync")

    def time(self, params, steps, warmup, n_active=None, per_kernel=True):
        total = C.c_float(0)
        kern = (C.c_float * 5)()
        st = lib().mvs_batch_time(self._h, C.byref(params), C.c_int(n_active or self.n_pairs), C.c_int(warmup),
                                  C.c_int(steps), C.byref(total), kern if per_kernel else None)
        self.ctx._check(st, "mvs_batch_time")
        names = ("match", "match_compact", "ransac", "finalize")
        return total.value, {n: kern[i] for i, n in enumerate(names)}

    def time_kernels(self, params, steps, n_active=None):
        """mean ms of every kernel launch of one pipeline pass, in launch order: [(kernel name, ms)] (HIP events in front
        of every launch, on the launches' own stream; an instrumented replay outside any timed region)"""
        cap = 32
        kid = (C.c_int32 * cap)()
        ms = (C.c_float * cap)()
        n = C.c_int(0)
        st = lib().mvs_batch_time_kernels(self._h, C.byref(params), C.c_int(n_active or self.n_pairs), C.c_int(steps),
                                          C.c_int(cap), kid, ms, C.byref(n))
        self.ctx._check(st, "mvs_batch_time_kernels")
        names = {v["kernel_id"]: k for k, v in self.ctx.kernel_info(self.max_kp, self.desc_bytes).items()}
        return [(names.get(kid[k], "kernel_%d" % kid[k]), float(ms[k])) for k in range(n.value)]

    def stats(self, params, n_active=None):
        ws = WorkStats()
        st = lib().mvs_batch_stats(self._h, C.byref(params), C.c_int(n_active or self.n_pairs), C.byref(ws))
        self.ctx._check(st, "mvs_batch_stats")
        d = {n: getattr(ws, n) for n, _ in WorkStats._fields_ if n != "pairs_mode"}
        d["pairs_mode"] = [int(x) for x in ws.pairs_mode]
        return d

    def download(self, first=0, count=None, matches=True, mask=True, points=True):
        count = count or (self.n_pairs - first)
        N = self.max_kp
        res = np.zeros(count, dtype=RESULT_DTYPE)
        mt = np.zeros((count, N), dtype=MATCH_DTYPE) if matches else None
        mk = np.zeros((count, N), dtype=np.uint8) if mask else None
        pts = np.zeros((count, N, 3)) if points else None
        idx = np.zeros((count, N), dtype=np.int64) if points else None
        st = lib().mvs_batch_download(self._h, C.c_int(first), C.c_int(count), res.ctypes.data_as(C.c_void_p),
                                      None if mt is None else mt.ctypes.data_as(C.c_void_p), _ptr(mk, C.c_uint8),
                                      _ptr(pts, C.c_double), _ptr(idx, C.c_int64))
        self.ctx._check(st, "mvs_batch_download")
        return dict(results=res, matches=mt, mask=mk, points=pts, point_idx=idx)

    def upload_octaves(self, first, base_octave=None, pair_octave=None):
        """cv::KeyPoint::octave of the uploaded keypoints, [count][max_kp] uint8 per image (observation covariances
        of refine(): stddev = 2^octave * sigma_px)"""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8) for a in (base_octave, pair_octave)]
        count = next(a for a in arrs if a is not None).shape[0]
        for a in arrs:
            assert a is None or a.shape == (count, self.max_kp)
        st = lib().mvs_batch_upload_octaves(self._h, C.c_int(first), C.c_int(count), _ptr(arrs[0], C.c_uint8),
                                            _ptr(arrs[1], C.c_uint8))
        self.ctx._check(st, "mvs_batch_upload_octaves")

    def refine(self, params=None, sigma_px=0.5):
        """ImagePair::refine of every valid pair, on the device, from the batch's own results (asynchronous)"""
        params = params or default_refine_params()
        self.ctx._check(lib().mvs_batch_refine(self._h, C.byref(params), C.c_double(sigma_px)), "mvs_batch_refine")

    def download_refined(self, points=True, point_cov=False):
        P, N = self.n_pairs, self.max_kp
        res = np.zeros(P, dtype=REFINE_DTYPE)
        pts = np.zeros((P, N, 3)) if points else None
        pc = np.zeros((P, N, 3, 3)) if point_cov else None
        st = lib().mvs_batch_download_refined(self._h, res.ctypes.data_as(C.c_void_p), _ptr(pts, C.c_double),
                                              _ptr(pc, C.c_double))
        self.ctx._check(st, "mvs_batch_download_refined")
        return dict(refined=res, points=pts, point_cov=pc)

    def copy_results_device(self, dst_ptr, first=0, count=None):
        """async D2D copy of the fixed-size result records into caller-owned device memory (e.g. a torch tensor)"""
        st = lib().mvs_batch_copy_results_device(self._h, C.c_int(first), C.c_int(count or self.n_pairs - first),
                                                 C.c_void_p(dst_ptr))
        self.ctx._check(st, "mvs_batch_copy_results_device")

    def results_device(self):
        p = C.c_void_p()
        sz = C.c_size_t(0)
        self.ctx._check(lib().mvs_batch_results_device(self._h, C.byref(p), C.byref(sz)), "mvs_batch_results_device")
        return p.value, sz.value


class Sequence:
    """Device-resident frame sequence (row f2): pair k = frames (k, k+1); track q = pnp_solve of frame q+2 against the
    points pair q triangulated, joined on the device through pair q+1's matches."""

    def __init__(self, ctx, n_frames, max_kp, desc_bytes=32):
        self.ctx, self.n_frames, self.max_kp, self.desc_bytes = ctx, n_frames, max_kp, desc_bytes
        self._h = C.c_void_p()
        ctx._check(lib().mvs_seq_create(ctx._h, C.c_int(n_frames), C.c_int(max_kp), C.c_int(desc_bytes),
                                        C.byref(self._h)), "mvs_seq_create")
        ctx._children.add(self)
        self._windows = None   # SeqWindowParams of the last refine_windows()

    def close(self):
        if self._h:
            if self.ctx._h:
                lib().mvs_seq_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, first, desc, kp, n_kp, K):
        count = len(n_kp)
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(count, self.max_kp, self.desc_bytes)
        kp = np.ascontiguousarray(kp, dtype=np.float32).reshape(count, self.max_kp, 2)
        n_kp = np.ascontiguousarray(n_kp, dtype=np.int32)
        st = lib().mvs_seq_upload(self._h, C.c_int(first), C.c_int(count), _ptr(desc, C.c_uint8), _ptr(kp, C.c_float),
                                  _ptr(n_kp, C.c_int32), _ptr(_f64(K, (9,)), C.c_double))
        self.ctx._check(st, "mvs_seq_upload")

    def run(self, params, pnp_params):
        self.ctx._check(lib().mvs_seq_run(self._h, C.byref(params), C.byref(pnp_params)), "mvs_seq_run")
        self.ctx._check(lib().mvs_seq_sync(self._h), "mvs_seq_sync")

    def run_essential(self, params, pnp_params):
        """run() with the five-point essential-matrix RANSAC for the pairs (mvs_seq_run_essential)"""
        self.ctx._check(lib().mvs_seq_run_essential(self._h, C.byref(params), C.byref(pnp_params)), "mvs_seq_run_essential")
        self.ctx._check(lib().mvs_seq_sync(self._h), "mvs_seq_sync")

    def download_hypotheses_run(self):
        """per pair, the hypotheses that took part in the last run_essential (mvs_seq_download_hypotheses_run)"""
        out = np.zeros(self.n_frames - 1, dtype=np.int32)
        st = lib().mvs_seq_download_hypotheses_run(self._h, C.c_int(0), C.c_int(self.n_frames - 1), _ptr(out, C.c_int32))
        self.ctx._check(st, "mvs_seq_download_hypotheses_run")
        return out

    def time(self, params, pnp_params, steps, warmup):
        ms = C.c_float(0)
        st = lib().mvs_seq_time(self._h, C.byref(params), C.byref(pnp_params), C.c_int(warmup), C.c_int(steps), C.byref(ms))
        self.ctx._check(st, "mvs_seq_time")
        return ms.value

    def time_stages(self, params, pnp_params, steps):
        ms = (C.c_float * 4)()
        st = lib().mvs_seq_time_stages(self._h, C.byref(params), C.byref(pnp_params), C.c_int(steps), ms)
        self.ctx._check(st, "mvs_seq_time_stages")
        return {n: ms[i] / steps for i, n in enumerate(("pairs", "join", "pnp", "chain"))}

    def upload_images(self, first, images, K, params=None):
        """extract keypoints + descriptors of frames [first, first + len(images)) on the device, straight into the
        sequence's resident frame arrays (up to max_kp per frame)"""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        B, H, W = images.shape
        params = params or default_orb_params()
        st = lib().mvs_seq_upload_images(self._h, C.c_int(first), C.c_int(B), _ptr(images, C.c_uint8), C.c_int(W),
                                         C.c_int(H), C.byref(params), None if K is None else _ptr(_f64(K, (9,)), C.c_double))
        self.ctx._check(st, "mvs_seq_upload_images")

    def download_trajectory(self):
        """pose of every frame in frame 0 (pair 0's baseline = 1), pair and track scales (scale propagation, row f2)"""
        F = self.n_frames
        R, t, ps, ts = np.zeros((F, 3, 3)), np.zeros((F, 3)), np.zeros(F - 1), np.zeros(F - 2)
        st = lib().mvs_seq_download_trajectory(self._h, _ptr(R, C.c_double), _ptr(t, C.c_double), _ptr(ps, C.c_double),
                                               _ptr(ts, C.c_double))
        self.ctx._check(st, "mvs_seq_download_trajectory")
        return dict(R=R, t=t, pair_scale=ps, track_scale=ts)

    def rescale(self, rule=SEQ_SCALE_DEPTH_RATIO, min_common=1):
        """the resident trajectory and scales of the last run again, by `rule` (mvs_seq_rescale; asynchronous):
        SEQ_SCALE_DEPTH_RATIO takes every step's scale from the depth ratios of the points two consecutive pairs share (a
        step with fewer than min_common of them keeps the scale), SEQ_SCALE_CHAIN restores what run() left.  Windows, the pose
        graph and the global problem of the old trajectory are retired."""
        sp = SeqScaleParams(int(rule), int(min_common))
        self.ctx._check(lib().mvs_seq_rescale(self._h, C.byref(sp)), "mvs_seq_rescale")

    def download_scale_steps(self):
        """the n_frames - 2 step records of the last rescale() (SCALE_STEP_DTYPE: n_common, n_used, flag, scale)"""
        steps = np.zeros(self.n_frames - 2, dtype=SCALE_STEP_DTYPE)
        st = lib().mvs_seq_download_scale_steps(self._h, steps.ctypes.data_as(C.c_void_p))
        self.ctx._check(st, "mvs_seq_download_scale_steps")
        return steps

    def upload_octaves(self, first, octave):
        octave = np.ascontiguousarray(octave, dtype=np.uint8)
        assert octave.ndim == 2 and octave.shape[1] == self.max_kp
        st = lib().mvs_seq_upload_octaves(self._h, C.c_int(first), C.c_int(octave.shape[0]), _ptr(octave, C.c_uint8))
        self.ctx._check(st, "mvs_seq_upload_octaves")

    def refine_pairs(self, params=None, sigma_px=0.5):
        params = params or default_refine_params()
        self.ctx._check(lib().mvs_seq_refine_pairs(self._h, C.byref(params), C.c_double(sigma_px)), "mvs_seq_refine_pairs")

    def download_refined(self, points=True, point_cov=False):
        P, N = self.n_frames - 1, self.max_kp
        res = np.zeros(P, dtype=REFINE_DTYPE)
        pts = np.zeros((P, N, 3)) if points else None
        pc = np.zeros((P, N, 3, 3)) if point_cov else None
        st = lib().mvs_seq_download_refined(self._h, res.ctypes.data_as(C.c_void_p), _ptr(pts, C.c_double), _ptr(pc, C.c_double))
        self.ctx._check(st, "mvs_seq_download_refined")
        return dict(refined=res, points=pts, point_cov=pc)

    def refine_windows(self, window_frames, stride, max_points=4096, params=None, sigma_px=0.5):
        """bundle-adjust the windows [w * stride, w * stride + window_frames) of a sequence that has been run, assembled on
        the device from the resident matches, points and trajectory (asynchronous; download_windows() fetches the results)"""
        params = params or default_refine_params()
        wp = SeqWindowParams(int(window_frames), int(stride), int(max_points), 0, float(sigma_px))
        self.ctx._check(lib().mvs_seq_refine_windows(self._h, C.byref(wp), C.byref(params)), "mvs_seq_refine_windows")
        self._windows = wp

    def download_windows(self):
        """one dict per window, shaped like Context.ba_refine_windows's, plus first_frame, n_tracks_found, track_kp
        [n_points][F] (keypoint of the point in frame first_frame + f, -1 = not seen) and point_guess [n_points][3]"""
        wp = self._windows
        if wp is None:
            raise MvsError(MVS_ERR_INVALID_ARG, "mvs_seq_download_windows")
        W, F, cap = lib().mvs_seq_window_count(self._h, C.byref(wp)), wp.window_frames, wp.max_points
        info = np.zeros(W, dtype=WINDOW_INFO_DTYPE)
        res = np.zeros((W, F), dtype=REFINE_DTYPE)
        pts, ptc = np.zeros((W, cap, 3)), np.zeros((W, cap, 3, 3))
        tkp = np.zeros((W, cap, F), dtype=np.int32)
        guess = np.zeros((W, cap, 3))
        st = lib().mvs_seq_download_windows(self._h, info.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p),
                                            _ptr(pts, C.c_double), _ptr(ptc, C.c_double), _ptr(tkp, C.c_int32),
                                            _ptr(guess, C.c_double))
        self.ctx._check(st, "mvs_seq_download_windows", allow_no_model=True)
        out = []
        for w in range(W):
            r, m = res[w], int(info[w]["n_points"])
            out.append(dict(ok=bool(r["ok"][0]), status=MVS_OK if r["ok"][0] else MVS_NO_MODEL, R=r["R"].copy(), t=r["t"].copy(),
                            pose_cov=r["pose_cov"].copy(), points=pts[w, :m].copy(), point_cov=ptc[w, :m].copy(),
                            error=float(r["error"][0]), iterations=int(r["iterations"][0]), raw=r.tobytes(),
                            first_frame=int(info[w]["first_frame"]), n_frames=int(info[w]["n_frames"]), n_points=m,
                            n_tracks_found=int(info[w]["n_tracks_found"]), track_kp=tkp[w, :m].copy(),
                            point_guess=guess[w, :m].copy()))
        return out

    def refine_global(self, max_track_frames=0, params=None, sigma_px=0.5):
        """ONE bundle adjustment over every frame of a sequence that has been run, assembled on the device from the resident
        matches, points and trajectory and solved by the sparse solver (mvs_seq_refine_global; synchronous).  Tracks are
        whole (max_track_frames = 0) or cut into pieces of that many frames.  Returns the result record's fields as a dict
        with status (MVS_OK / MVS_NO_MODEL), ok, n_points, n_obs and `raw`, the record's bytes."""
        params = params or default_refine_params()
        gp = SeqGlobalParams(int(max_track_frames), 0, float(sigma_px))
        res = BaSparseResult()
        st = lib().mvs_seq_refine_global(self._h, C.byref(gp), C.byref(params), C.byref(res))
        self.ctx._check(st, "mvs_seq_refine_global", allow_no_model=True)
        out = {k: getattr(res, k) for k, _ in BaSparseResult._fields_}
        n_points, n_obs = self.global_counts()
        out.update(status=st, ok=bool(res.ok), n_points=n_points, n_obs=n_obs, raw=bytes(res))
        return out

    def global_counts(self):
        """(points, observations) of the last refine_global()"""
        n_points, n_obs = C.c_int32(0), C.c_int32(0)
        st = lib().mvs_seq_global_counts(self._h, C.byref(n_points), C.byref(n_obs))
        self.ctx._check(st, "mvs_seq_global_counts")
        return n_points.value, n_obs.value

    def download_global(self, points=True, pose_cov=True, point_cov=True):
        """the estimate of the last refine_global(): status, R [F, 3, 3], t [F, 3], points [P, 3], pose_cov [F, 6, 6] and
        point_cov [P, 3, 3] (None when not asked for; the covariance sweep runs at the first request) and `raw`, the bytes of
        every array.  On MVS_NO_MODEL the arrays are as they were allocated (zero)."""
        F, (P, _) = self.n_frames, self.global_counts()
        poses = np.zeros((F, 12))
        pts = np.zeros((max(P, 1), 3)) if points else None
        pcv = np.zeros((F, 6, 6)) if pose_cov else None
        ptc = np.zeros((max(P, 1), 3, 3)) if point_cov else None
        st = lib().mvs_seq_download_global(self._h, _ptr(poses, C.c_double), _ptr(pts, C.c_double), _ptr(pcv, C.c_double),
                                           _ptr(ptc, C.c_double))
        self.ctx._check(st, "mvs_seq_download_global", allow_no_model=True)
        return dict(status=st, R=poses[:, :9].reshape(-1, 3, 3).copy(), t=poses[:, 9:].copy(), points=pts, pose_cov=pcv,
                    point_cov=ptc, raw=b"".join(a.tobytes() for a in (poses, pts, pcv, ptc) if a is not None))

    def global_obs_stats(self):
        """mvs_seq_global_obs_stats: (chi2 [n_obs], weight [n_obs]) of the resident global problem's observations at the
        estimate of the last refine_global(), under the context's loss (Context.set_ba_loss).  Raises MvsError
        (MVS_ERR_INVALID_ARG) unless that call ended with ok."""
        _, O = self.global_counts()   # refuses (MVS_ERR_INVALID_ARG) where there has been no refine_global()
        chi2, wt = np.zeros(max(O, 1)), np.zeros(max(O, 1))
        st = lib().mvs_seq_global_obs_stats(self._h, _ptr(chi2, C.c_double), _ptr(wt, C.c_double))
        self.ctx._check(st, "mvs_seq_global_obs_stats")
        return chi2[:O], wt[:O]

    def download_global_problem(self):
        """the problem the last refine_global() assembled: obs_off [P + 1], obs_frame / obs_kp [O], head_frame / head_kp [P],
        point_guess [P, 3], obs_uv [O, 2]"""
        P, O = self.global_counts()
        i32 = lambda n: np.zeros(n, dtype=np.int32)
        out = dict(obs_off=i32(P + 1), obs_frame=i32(O), obs_kp=i32(O), head_frame=i32(P), head_kp=i32(P),
                   point_guess=np.zeros((P, 3)), obs_uv=np.zeros((O, 2)))
        st = lib().mvs_seq_download_global_problem(
            self._h, *[out[k].ctypes.data_as(C.c_void_p) for k in ("obs_off", "obs_frame", "obs_kp", "head_frame", "head_kp",
                                                                  "point_guess", "obs_uv")])
        self.ctx._check(st, "mvs_seq_download_global_problem")
        return out

    def track(self, vo_params=None, pnp_params=None, refine_params=None):
        """VisualOdometer::track over the resident sequence (mvs_seq_track): persistent map, PnP, two-frame BA and the
        gates of every frame behind init_pair, on the device (asynchronous; the download_track_* calls fetch the results)"""
        vo_params = vo_params or default_vo_params()
        pnp_params = pnp_params or default_pnp_params()
        refine_params = refine_params or default_refine_params()
        st = lib().mvs_seq_track(self._h, C.byref(vo_params), C.byref(pnp_params), C.byref(refine_params))
        self.ctx._check(st, "mvs_seq_track")

    def download_track_frames(self):
        """one TRACK_FRAME_DTYPE record per frame"""
        fr = np.zeros(self.n_frames, dtype=TRACK_FRAME_DTYPE)
        self.ctx._check(lib().mvs_seq_download_track_frames(self._h, fr.ctypes.data_as(C.c_void_p)),
                        "mvs_seq_download_track_frames")
        return fr

    def download_track_map(self, frame):
        """the map as it stands after `frame`, keyed by the frame's keypoint index: point_id (-1 = none), X"""
        pid, X = np.zeros(self.max_kp, dtype=np.int32), np.zeros((self.max_kp, 3))
        st = lib().mvs_seq_download_track_map(self._h, C.c_int(frame), _ptr(pid, C.c_int32), _ptr(X, C.c_double))
        self.ctx._check(st, "mvs_seq_download_track_map")
        return dict(point_id=pid, X=X)

    def download_track_step(self, frame, record=None):
        """what step `frame` fed its solvers and got back, cut to the counts of the frame's record (download_track_frames()
        [frame] when not given): candidates (cand_base_kp, cand_new_kp, cand_xyz, cand_uv), pnp_inliers, the BA problem
        (point_id, point_kp [m, 2], point_is_new, point_guess, guess_pose [2, 12]), ba_frames [2] and points_refined"""
        N = self.max_kp
        rec = self.download_track_frames()[frame] if record is None else record
        ca, cb, inl, pid = (np.zeros(N, dtype=np.int32) for _ in range(4))
        cX, cuv, pkp, pnew = np.zeros((N, 3)), np.zeros((N, 2)), np.zeros((N, 2), dtype=np.int32), np.zeros(N, dtype=np.uint8)
        guess, pose, pts = np.zeros((N, 3)), np.zeros((2, 12)), np.zeros((N, 3))
        ba = np.zeros(2, dtype=REFINE_DTYPE)
        st = lib().mvs_seq_download_track_step(self._h, C.c_int(frame), _ptr(ca, C.c_int32), _ptr(cb, C.c_int32),
                                               _ptr(cX, C.c_double), _ptr(cuv, C.c_double), _ptr(inl, C.c_int32),
                                               _ptr(pid, C.c_int32), _ptr(pkp, C.c_int32), _ptr(pnew, C.c_uint8),
                                               _ptr(guess, C.c_double), _ptr(pose, C.c_double), ba.ctypes.data_as(C.c_void_p),
                                               _ptr(pts, C.c_double))
        self.ctx._check(st, "mvs_seq_download_track_step")
        nc, ni, m = int(rec["n_cand"]), int(rec["n_pnp_inliers"]), int(rec["n_tracked"]) + int(rec["n_new"])
        full = dict(cand_base_kp=ca, cand_new_kp=cb, cand_xyz=cX, cand_uv=cuv, pnp_inliers=inl, point_id=pid, point_kp=pkp,
                    point_is_new=pnew, point_guess=guess, points_refined=pts)
        cut = dict(cand_base_kp=nc, cand_new_kp=nc, cand_xyz=nc, cand_uv=nc, pnp_inliers=ni)
        out = {k: v[:cut.get(k, m)].copy() for k, v in full.items()}
        out.update(guess_pose=pose, ba_frames=ba, raw=b"".join(v.tobytes() for v in full.values()) + pose.tobytes() + ba.tobytes())
        return out

    def run_lags(self, params, max_lag, essential=False, refine_params=None, sigma_px=0.5):
        """the pairs (k, k + d) of every lag d = 2 .. max_lag through the pipeline of run() (run_essential() if `essential`)
        and ImagePair::refine, and refine_pairs() for lag 1 (mvs_seq_run_lags; asynchronous)"""
        refine_params = refine_params or default_refine_params()
        st = lib().mvs_seq_run_lags(self._h, C.byref(params), C.c_int(max_lag), C.c_int(1 if essential else 0),
                                    C.byref(refine_params), C.c_double(sigma_px))
        self.ctx._check(st, "mvs_seq_run_lags")

    def download_lag_pairs(self, lag):
        """download_pairs() for the n_frames - lag pairs of a resident lag, plus match_ssd"""
        P, N = max(self.n_frames - lag, 1), self.max_kp
        res = np.zeros(P, dtype=RESULT_DTYPE)
        mt = np.zeros((P, N), dtype=MATCH_DTYPE)
        mk = np.zeros((P, N), dtype=np.uint8)
        pts = np.zeros((P, N, 3))
        idx = np.zeros((P, N), dtype=np.int64)
        ssd = np.zeros(P, dtype=np.int32)
        st = lib().mvs_seq_download_lag_pairs(self._h, C.c_int(lag), res.ctypes.data_as(C.c_void_p),
                                              mt.ctypes.data_as(C.c_void_p), _ptr(mk, C.c_uint8), _ptr(pts, C.c_double),
                                              _ptr(idx, C.c_int64), _ptr(ssd, C.c_int32))
        self.ctx._check(st, "mvs_seq_download_lag_pairs")
        return dict(results=res, matches=mt, mask=mk, points=pts, point_idx=idx, match_ssd=ssd)

    def download_lag_refined(self, lag, points=True, point_cov=False):
        """download_refined() for a resident lag"""
        P, N = max(self.n_frames - lag, 1), self.max_kp
        res = np.zeros(P, dtype=REFINE_DTYPE)
        pts = np.zeros((P, N, 3)) if points else None
        pc = np.zeros((P, N, 3, 3)) if point_cov else None
        st = lib().mvs_seq_download_lag_refined(self._h, C.c_int(lag), res.ctypes.data_as(C.c_void_p), _ptr(pts, C.c_double),
                                                _ptr(pc, C.c_double))
        self.ctx._check(st, "mvs_seq_download_lag_refined")
        return dict(refined=res, points=pts, point_cov=pc)

    def odometry(self, vo_params=None, init_params=None, pnp_params=None, refine_params=None):
        """VisualOdometer::add_frame over the resident sequence (mvs_seq_odometry): initialisation from the frame queue with
        re-pairing over the lags of run_lags(), the tracking loop of track(), reset and re-initialisation after a loss, on
        the device (asynchronous; download_odometry_frames() and the download_track_* calls fetch the results)"""
        vo_params = vo_params or default_vo_params()
        init_params = init_params or default_vo_init_params()
        pnp_params = pnp_params or default_pnp_params()
        refine_params = refine_params or default_refine_params()
        st = lib().mvs_seq_odometry(self._h, C.byref(vo_params), C.byref(init_params), C.byref(pnp_params),
                                    C.byref(refine_params))
        self.ctx._check(st, "mvs_seq_odometry")

    def download_odometry_frames(self):
        """one ODO_FRAME_DTYPE record per frame"""
        od = np.zeros(self.n_frames, dtype=ODO_FRAME_DTYPE)
        self.ctx._check(lib().mvs_seq_download_odometry_frames(self._h, od.ctypes.data_as(C.c_void_p)),
                        "mvs_seq_download_odometry_frames")
        return od

    def build_pose_graph(self, max_lag, min_points=0, max_error=1e30, chain_sigma=(0.0, 0.0)):
        """the pose graph of the sequence on the device (mvs_seq_build_pose_graph; asynchronous): nodes = the trajectory,
        edges = the refined pairs of lags 1 .. max_lag from run_lags() that pass the gates, scaled by the trajectory"""
        gp = SeqGraphParams(int(max_lag), int(min_points), float(max_error), (C.c_double * 2)(float(chain_sigma[0]),
                                                                                              float(chain_sigma[1])))
        self.ctx._check(lib().mvs_seq_build_pose_graph(self._h, C.byref(gp)), "mvs_seq_build_pose_graph")
        self._graph_slots = max_lag * self.n_frames - max_lag * (max_lag + 1) // 2
        self._graph_loop_rows = 0

    def optimize_pose_graph(self, params=None):
        """mvs_seq_optimize_pose_graph: (status, result record); download_pose_graph_poses() fetches the nodes"""
        params = params or default_pose_graph_params()
        res = np.zeros(1, dtype=POSE_GRAPH_RESULT_DTYPE)
        st = lib().mvs_seq_optimize_pose_graph(self._h, C.byref(params), res.ctypes.data_as(C.c_void_p))
        self.ctx._check(st, "mvs_seq_optimize_pose_graph", allow_no_model=True)
        return st, res[0]

    def optimize_pose_graph_sim3(self, params=None, scale_sigma=(0.05, 0.05, 0.05)):
        """mvs_seq_optimize_pose_graph_sim3: the resident graph lifted to Sim(3) -- scale_sigma: the log-scale standard deviation
        of a measured, a fallback and a loop edge -- and optimised on the device; (status, result record);
        download_pose_graph_sim3() fetches the nodes"""
        params = params or default_sim3_graph_params()
        sig = (C.c_double * 3)(float(scale_sigma[0]), float(scale_sigma[1]), float(scale_sigma[2]))
        res = np.zeros(1, dtype=POSE_GRAPH_RESULT_DTYPE)
        st = lib().mvs_seq_optimize_pose_graph_sim3(self._h, C.byref(params), sig, res.ctypes.data_as(C.c_void_p))
        self.ctx._check(st, "mvs_seq_optimize_pose_graph_sim3", allow_no_model=True)
        return st, res[0]

    def download_pose_graph_sim3(self):
        """the Sim(3) optimised nodes [n_frames, 13] of the last successful optimize_pose_graph_sim3()"""
        nodes = np.zeros((self.n_frames, 13))
        st = lib().mvs_seq_download_pose_graph_sim3(self._h, _ptr(nodes, C.c_double))
        self.ctx._check(st, "mvs_seq_download_pose_graph_sim3")
        return nodes

    def download_pose_graph(self):
        """the resident graph, cut to its edge count: node_pose [n_frames, 12], edge_src, edge_dst, edge_pose [E, 12],
        edge_cov [E, 36], edge_lag, edge_kind, edge_scale, anchor (0) -- the keys Context.pose_graph_optimize reads, and more"""
        # rows: the build's slots, plus the max_candidates of the selection whose edges add_loop_edges() last added
        S = max(getattr(self, "_graph_slots", 0) + getattr(self, "_graph_loop_rows", 0), 1)
        n = np.zeros(1, dtype=np.int32)
        node = np.zeros((self.n_frames, 12))
        src, dst, lag, kind = (np.zeros(S, dtype=np.int32) for _ in range(4))
        Z, cov, scale = np.zeros((S, 12)), np.zeros((S, 36)), np.zeros(S)
        st = lib().mvs_seq_download_pose_graph(self._h, _ptr(n, C.c_int32), _ptr(node, C.c_double), _ptr(src, C.c_int32),
                                               _ptr(dst, C.c_int32), _ptr(Z, C.c_double), _ptr(cov, C.c_double),
                                               _ptr(lag, C.c_int32), _ptr(kind, C.c_int32), _ptr(scale, C.c_double))
        self.ctx._check(st, "mvs_seq_download_pose_graph")
        E = int(n[0])
        return dict(n_edges=E, node_pose=node, edge_src=src[:E].copy(), edge_dst=dst[:E].copy(), edge_pose=Z[:E].copy(),
                    edge_cov=cov[:E].copy(), edge_lag=lag[:E].copy(), edge_kind=kind[:E].copy(), edge_scale=scale[:E].copy(),
                    anchor=0)

    def download_pose_graph_poses(self):
        """the optimised nodes [n_frames, 12] of the last successful optimize_pose_graph()"""
        poses = np.zeros((self.n_frames, 12))
        st = lib().mvs_seq_download_pose_graph_poses(self._h, _ptr(poses, C.c_double))
        self.ctx._check(st, "mvs_seq_download_pose_graph_poses")
        return poses

    def pose_graph_edge_stats(self):
        """mvs_seq_pose_graph_edge_stats: (status, chi2 [E], weight [E]) of the resident graph's edges at its optimised nodes,
        under the context's loss.  Raises MvsError (MVS_ERR_INVALID_ARG) unless the last optimize_pose_graph() on the current
        graph succeeded."""
        cap = max(getattr(self, "_graph_slots", 0) + getattr(self, "_graph_loop_rows", 0), 1)   # download_pose_graph's rows
        chi2, weight, n = np.zeros(cap), np.zeros(cap), np.zeros(1, dtype=np.int32)
        st = lib().mvs_seq_pose_graph_edge_stats(self._h, _ptr(chi2, C.c_double), _ptr(weight, C.c_double))
        self.ctx._check(st, "mvs_seq_pose_graph_edge_stats", allow_no_model=True)
        self.ctx._check(lib().mvs_seq_download_pose_graph(self._h, _ptr(n, C.c_int32), None, None, None, None, None, None, None,
                                                          None), "mvs_seq_download_pose_graph")
        return st, chi2[:int(n[0])], weight[:int(n[0])]

    def pose_graph_marginals(self, queries=None, anchor_sigma=None, cov_out=None):
        """mvs_seq_pose_graph_marginals: blocks of Sigma = H^-1 of the resident graph at its optimised nodes; as
        Context.pose_graph_marginals.  Raises MvsError (MVS_ERR_INVALID_ARG) unless the last optimize_pose_graph() on the
        current graph succeeded."""
        sigma, n, qi, qj, cov_out, info = _marginals_args(self.n_frames, queries, anchor_sigma, cov_out)
        st = lib().mvs_seq_pose_graph_marginals(self._h, sigma, C.c_int(n), _ptr(qi, C.c_int32), _ptr(qj, C.c_int32),
                                                _ptr(cov_out, C.c_double), info.ctypes.data_as(C.c_void_p))
        self.ctx._check(st, "mvs_seq_pose_graph_marginals", allow_no_model=True)
        return st, info[0], cov_out

    def sync(self):
        """wait for the context's stream (the loop-closure calls are asynchronous)"""
        self.ctx._check(lib().mvs_seq_sync(self._h), "mvs_seq_sync")

    def loop_scores(self, ratio=0.7, max_dist=10.0, min_gap=1):
        """score[i][j], j - i >= min_gap: keypoints of frame j that match into frame i (mvs_seq_loop_scores; asynchronous)"""
        st = lib().mvs_seq_loop_scores(self._h, C.c_double(ratio), C.c_double(max_dist), C.c_int(min_gap))
        self.ctx._check(st, "mvs_seq_loop_scores")

    def download_loop_scores(self):
        """the [n_frames, n_frames] int32 score table, zero outside the eligible triangle"""
        sc = np.zeros((self.n_frames, self.n_frames), dtype=np.int32)
        self.ctx._check(lib().mvs_seq_download_loop_scores(self._h, _ptr(sc, C.c_int32)), "mvs_seq_download_loop_scores")
        return sc

    def select_loops(self, min_score, top_k, max_candidates):
        """per query frame the top_k base frames with score >= min_score, cut at max_candidates (mvs_seq_select_loops)"""
        sp = LoopSelectParams(int(min_score), int(top_k), int(max_candidates), 0)
        self.ctx._check(lib().mvs_seq_select_loops(self._h, C.byref(sp)), "mvs_seq_select_loops")
        self._loop_max_candidates = int(max_candidates)

    def verify_loops(self, params, essential=False, refine_params=None, sigma_px=0.5):
        """the candidates through the two-view pipeline and ImagePair::refine (mvs_seq_verify_loops)"""
        refine_params = refine_params or default_refine_params()
        st = lib().mvs_seq_verify_loops(self._h, C.byref(params), C.c_int(1 if essential else 0), C.byref(refine_params),
                                        C.c_double(sigma_px))
        self.ctx._check(st, "mvs_seq_verify_loops")

    def add_loop_edges(self, min_points=0, max_error=1e30, loop_sigma=(0.0, 0.0)):
        """one edge of kind 2 per accepted candidate behind the built edges of the pose graph (mvs_seq_add_loop_edges)"""
        ep = LoopEdgeParams(int(min_points), 0, float(max_error), (C.c_double * 2)(float(loop_sigma[0]), float(loop_sigma[1])))
        self.ctx._check(lib().mvs_seq_add_loop_edges(self._h, C.byref(ep)), "mvs_seq_add_loop_edges")
        self._graph_loop_rows = getattr(self, "_loop_max_candidates", 0)

    def download_loop_candidates(self, pairs=False):
        """the resident list cut to its kept count: cand (LOOP_CANDIDATE_DTYPE), n_kept, n_found; with pairs=True also what
        Batch.download / download_refined give for the verified candidates (results, matches, mask, points, point_idx, refined)"""
        Cn, N = max(getattr(self, "_loop_max_candidates", 0), 1), self.max_kp
        kept, found = C.c_int32(0), C.c_int32(0)
        cand = np.zeros(Cn, dtype=LOOP_CANDIDATE_DTYPE)
        none = C.c_void_p()
        res = np.zeros(Cn, dtype=RESULT_DTYPE) if pairs else None
        mt = np.zeros((Cn, N), dtype=MATCH_DTYPE) if pairs else None
        mk = np.zeros((Cn, N), dtype=np.uint8) if pairs else None
        pts = np.zeros((Cn, N, 3)) if pairs else None
        idx = np.zeros((Cn, N), dtype=np.int64) if pairs else None
        ref = np.zeros(Cn, dtype=REFINE_DTYPE) if pairs else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else none
        st = lib().mvs_seq_download_loop_candidates(self._h, C.byref(kept), C.byref(found), vp(cand), vp(res), vp(mt), vp(mk),
                                                    vp(pts), vp(idx), vp(ref))
        self.ctx._check(st, "mvs_seq_download_loop_candidates")
        k = kept.value
        out = dict(n_kept=k, n_found=found.value, cand=cand[:k].copy(), cand_all=cand)
        if pairs:
            out.update(results=res[:k], matches=mt[:k], mask=mk[:k], points=pts[:k], point_idx=idx[:k], refined=ref[:k])
        return out

    def download_pairs(self):
        P, N = self.n_frames - 1, self.max_kp
        res = np.zeros(P, dtype=RESULT_DTYPE)
        mt = np.zeros((P, N), dtype=MATCH_DTYPE)
        mk = np.zeros((P, N), dtype=np.uint8)
        pts = np.zeros((P, N, 3))
        idx = np.zeros((P, N), dtype=np.int64)
        st = lib().mvs_seq_download_pairs(self._h, C.c_int(0), C.c_int(P), res.ctypes.data_as(C.c_void_p),
                                          mt.ctypes.data_as(C.c_void_p), _ptr(mk, C.c_uint8), _ptr(pts, C.c_double),
                                          _ptr(idx, C.c_int64))
        self.ctx._check(st, "mvs_seq_download_pairs")
        return dict(results=res, matches=mt, mask=mk, points=pts, point_idx=idx)

    def download_tracks(self):
        T, N = self.n_frames - 2, self.max_kp
        tr = np.zeros(T, dtype=TRACK_DTYPE)
        X = np.zeros((T, N, 3))
        uv = np.zeros((T, N, 2))
        inl = np.zeros((T, N), dtype=np.int64)
        st = lib().mvs_seq_download_tracks(self._h, C.c_int(0), C.c_int(T), tr.ctypes.data_as(C.c_void_p),
                                           _ptr(X, C.c_double), _ptr(uv, C.c_double), _ptr(inl, C.c_int64))
        self.ctx._check(st, "mvs_seq_download_tracks")
        return dict(tracks=tr, corr_xyz=X, corr_uv=uv, inlier_idx=inl)
