/*
 * mvslam_hip.h -- C ABI of libmvslam_hip.so: mvSLAM's front-end two-view geometry
 * hot path (brute-force Hamming match -> 8-point RANSAC -> essential decomposition
 * -> linear triangulation) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (lonelycorn/mvSLAM) has no FFI layer: its boundary for this path is
 * a set of C++ free functions / static methods in namespace mvSLAM.  Every entry
 * point below names the reference interface it stands in for (file:line relative
 * to the reference tree).  The C++ header shim that keeps the reference's own
 * signatures on top of this ABI lives in mvslam_amd/compat/ (see INTEGRATION.md).
 *
 * Conventions
 *   - all pointers are caller-owned HOST memory unless the name says "device";
 *   - matrices are row-major double (reference ScalarType = double, system-config.hpp:6);
 *   - every call returns an mvs_status; nothing here aborts or throws
 *     (the reference asserts on precondition violations, e.g. sfm-solve.cpp:37-41);
 *   - one mvs_ctx per (host thread, GPU); calls on one ctx are serialised by the caller
 *     (the reference path is single-threaded and not re-entrant, visual-feature.cpp:12-25).
 *   - there is NO CPU fallback: without a HIP device mvs_ctx_create fails.
 */
#ifndef MVSLAM_HIP_H
#define MVSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 4): mvs_work_stats grew by FIVE fields (max_sweeps9, dense_points, matches_mode1, score_evals_executed_mfma_rest,
 * score_evals_executed_mfma_pilot; score_evals_executed is the sum of every executed-evaluation counter); every entry point
 * and every other struct is unchanged from version 2 */
/* 4 (round 5): two entry points added -- mvs_batch_device_state (read-only diagnostics view, below) and mvs_batch_run_points
 * (a batch of sfm_solve calls on caller-supplied point pairs); nothing else changed */
/* still 4: mvs_ba_window, mvs_ba_refine_window and mvs_ba_refine_windows are additions (new symbols only); no existing entry
 * point or struct changed */
/* still 4: mvs_seq_window_params, mvs_seq_window_info, mvs_seq_refine_windows, mvs_seq_window_count and
 * mvs_seq_download_windows are additions (new symbols only) */
/* still 4: mvs_five_point, mvs_ransac_essential, mvs_two_view_essential and mvs_batch_run_points_essential are additions (new
 * symbols only): the five-point essential-matrix RANSAC beside the 8-point one */
/* still 4: mvs_ctx_set_essential_confidence, mvs_ctx_essential_hypotheses_run and mvs_batch_download_hypotheses_run are additions
 * (new symbols only): the five-point RANSAC's optional termination rule; off by default, no struct changed */
/* still 4: mvs_image_pair_essential, mvs_batch_run_essential, mvs_seq_run_essential, mvs_seq_download_hypotheses_run and
 * mvs_batch_download_essential_tables are additions (new symbols only): the five-point RANSAC behind the matcher, for one pair,
 * a batch and a sequence; no existing entry point or struct changed */
/* still 4: mvs_seq_run_lags, mvs_seq_download_lag_pairs, mvs_seq_download_lag_refined, mvs_vo_init_params, mvs_odo_frame,
 * mvs_vo_init_params_default, mvs_seq_odometry, mvs_seq_download_odometry_frames and MVS_TRACK_INITIALIZING are additions
 * (new symbols only): VisualOdometer::add_frame on the device */
/* still 4: mvs_vo_params, mvs_track_frame, mvs_vo_params_default, mvs_seq_track, mvs_seq_download_track_frames,
 * mvs_seq_download_track_map and mvs_seq_download_track_step are additions (new symbols only): VisualOdometer::track on a
 * resident sequence */
/* still 4: mvs_seq_loop_scores, mvs_seq_download_loop_scores, mvs_loop_select_params, mvs_loop_candidate, mvs_seq_select_loops,
 * mvs_seq_verify_loops, mvs_loop_edge_params, mvs_seq_add_loop_edges and mvs_seq_download_loop_candidates are additions (new
 * symbols only): loop closures of a resident sequence */
/* still 4: mvs_seq_scale_params, mvs_seq_scale_step, mvs_seq_rescale and mvs_seq_download_scale_steps are additions (new
 * symbols only): the scale of a resident sequence from depth ratios of shared points */
#define MVS_ABI_VERSION 4

typedef enum mvs_status {
    MVS_OK = 0,
    MVS_NO_MODEL = 1,          /* the reference's `return false` (sfm-solve.cpp:319-321,330-334,353-356) */
    MVS_ERR_INVALID_ARG = -1,  /* the reference's assert()s */
    MVS_ERR_NO_DEVICE = -2,
    MVS_ERR_HIP = -3,
    MVS_ERR_CAPACITY = -4,
    MVS_ERR_BAD_INTRINSICS = -5 /* K must be affine: K[6..8] == (0, 0, 1) */
} mvs_status;

/* layout-identical to cv::DMatch (reference MatchResultType, base/image.hpp:37-48) */
typedef struct mvs_match {
    int32_t queryIdx; /* index into vf2 / pair frame */
    int32_t trainIdx; /* index into vf1 / base frame */
    int32_t imgIdx;
    float distance;
} mvs_match;

#define MVS_SAMPLER_IDENTITY 0 /* reference behaviour: the first 8 matches (estimator-RANSAC.cpp:41-48) */
#define MVS_SAMPLER_PHILOX 1   /* Philox4x32-10 keyed (seed, hypothesis id) */

/* Knobs of the path */
typedef struct mvs_params {
    double ratio;           /* Lowe ratio, 0.7 as ScalarType = double (visual-feature.cpp:23) */
    double max_dist;        /* max Hamming distance of a match, < 0 disables (image-pair.cpp:22-23: 10) */
    double max_error_sq;    /* <= 0: 5e-2 / K00 / K11 (sfm-solve.cpp:18-19,311) */
    int32_t num_hypotheses; /* reference: 1 (sfm-solve.cpp:67) */
    int32_t sampler;        /* MVS_SAMPLER_* */
    uint64_t seed;          /* hypothesis sampler key; pair p of a batch uses seed + global_index[p] */
    int32_t min_inliers;    /* 8 (sfm-solve.cpp:20-21,330) */
    int32_t reserved;
} mvs_params;

/* Fixed-size per-pair result (what ImagePair keeps after reconstruct(), image-pair.hpp:56-64) */
typedef struct mvs_pair_result {
    int32_t valid;      /* ImagePair::valid */
    int32_t n_matches;  /* M: matches surviving ratio / max_dist */
    int32_t n_inliers;  /* inliers of the winning hypothesis */
    int32_t n_points;   /* triangulated points that passed cheirality = match_inlier_count */
    int32_t best_hyp;   /* winning hypothesis id (-1: none) */
    int32_t best_count;
    double best_residual;
    double F[9];        /* winning fundamental (= essential on ideal cameras) before projection */
    double E[9];        /* after projection to (s, s, 0) (sfm-solve.cpp:74-84) */
    double R1to2[9];    /* winning candidate of decompose_essential_matrix */
    double t1to2[3];
    double R[9];        /* pose2in1 = SE3(SO3(R1to2), t1to2).inverse() (sfm-solve.cpp:364) = T_pair_to_base */
    double t[3];
} mvs_pair_result;

typedef struct mvs_ctx mvs_ctx;
typedef struct mvs_batch mvs_batch;

/* ---- context ------------------------------------------------------------------ */
int mvs_abi_version(void);
const char *mvs_status_str(mvs_status s);
const char *mvs_last_error(const mvs_ctx *ctx); /* text of the last HIP failure on this ctx */
mvs_status mvs_params_default(mvs_params *p);   /* reference defaults + num_hypotheses = 1, identity sampler */
mvs_status mvs_ctx_create(int device_id, mvs_ctx **out);
mvs_status mvs_ctx_create_on_stream(int device_id, void *hip_stream, mvs_ctx **out); /* borrow a stream */
void mvs_ctx_destroy(mvs_ctx *ctx);
void *mvs_ctx_stream(mvs_ctx *ctx); /* hipStream_t the kernels are launched on */
/* A batch of >= 64 pairs goes down the pipeline as two independent halves, the second on a context-owned side stream that is
 * forked from the context's stream (results are identical: pairs are independent, estimator-RANSAC.cpp:76-84 runs per pair).
 * The side stream is joined back into the context's stream on demand: by the next call on this context that uses the stream
 * for anything but the same run again -- upload, download, copy, refine, stats, timing, sync, destroy, any other entry point
 * -- so back-to-back runs of a resident batch overlap one call's tail with the next call's kernels, and every result a call
 * of this library hands out is complete.  A caller who can enqueue work of their own on the stream sees one stream, as
 * before: if the stream was borrowed (mvs_ctx_create_on_stream) or mvs_ctx_stream() has ever been called on this context, the
 * join happens inside every run, before it returns.  enable = 0 keeps every launch on the one stream.  Default: enabled. */
mvs_status mvs_ctx_set_half_batches(mvs_ctx *ctx, int enable);
/* Confidence level of the five-point essential-matrix RANSAC (the reference's VF_MATCH_CONFIDENCE_LEVEL = 0.99,
 * sfm-solve.cpp:22-23,58), honoured by mvs_ransac_essential, mvs_two_view_essential and mvs_batch_run_points_essential; the
 * 8-point entry points ignore it.  0 (the default): every hypothesis runs.  0 < confidence < 1: each pair stops at the first
 * checkpoint at which the rule stated with those entry points holds.  Anything else (a NaN too): MVS_ERR_INVALID_ARG. */
mvs_status mvs_ctx_set_essential_confidence(mvs_ctx *ctx, double confidence);
/* n_run -- the hypotheses that took part -- of the last single-shot five-point call on this context (0: it had fewer than
 * eight matches).  MVS_ERR_INVALID_ARG before the first such call, and after one that failed before its RANSAC was enqueued
 * (an error status: capacity, intrinsics, allocation): nothing ran, and the call before it is no longer the last.  Without a
 * confidence level the value is known on the host and the call touches no device. */
mvs_status mvs_ctx_essential_hypotheses_run(mvs_ctx *ctx, int32_t *n_run);

/* ---- single-shot entry points (host buffers; the reference's call surface) ------ */

/* VisualFeature::match_visual_features(vf1 = train, vf2 = query, max_dist)
 * (vision/visual-feature.cpp:51-80, decl visual-feature.hpp:23-26).
 * desc: n x desc_bytes row-major CV_8U (desc_bytes multiple of 4, <= 64).
 * out: capacity n_query.  Output order: (distance, queryIdx) ascending.
 * MVS_ERR_INVALID_ARG when n_train < 2 or n_query < 1 (reference: assert / UB). */
mvs_status mvs_match_hamming(mvs_ctx *ctx, const uint8_t *train_desc, int n_train, const uint8_t *query_desc,
                             int n_query, int desc_bytes, double ratio, double max_dist, mvs_match *out,
                             int *n_out);

/* sfm_solve(p1, p2, K, pose2in1, points, point_indexes) (vision/sfm-solve.cpp:285-368, decl sfm.hpp:30-35)
 * with find_essential_matrix's own-RANSAC branch (sfm-solve.cpp:64-90).
 * p1_uv / p2_uv: m x (u, v) image points.  points_xyz: capacity 3*m.  point_idx: capacity m.
 * inlier_mask: capacity m (may be NULL).  result: may be NULL.
 * returns MVS_OK (true) or MVS_NO_MODEL (false). */
mvs_status mvs_two_view(mvs_ctx *ctx, const double *p1_uv, const double *p2_uv, int m, const double K[9],
                        const mvs_params *params, double R[9], double t[3], double *points_xyz,
                        int64_t *point_idx, int *n_points, uint8_t *inlier_mask, mvs_pair_result *result);

/* ImagePair::ImagePair + ImagePair::reconstruct (front-end/image-pair.cpp:30-71,116-174) of ONE pair in a single device
 * pass: match(base = train, pair = query) -> gather + normalise -> sfm_solve, one upload, one synchronisation, one
 * download (the match_visual_features + sfm_solve call pair costs two round trips).  base_kp / pair_kp: n x (x, y)
 * float = cv::KeyPoint::pt.  Outputs (any but `result` may be NULL): matches[<= n_pair] in the canonical order,
 * inlier_mask[n_matches], points_xyz[n_points x 3], point_idx[n_points] (index into matches).  Returns MVS_NO_MODEL when
 * the reference's constructor leaves `valid == false`; result->n_matches etc. are filled either way. */
mvs_status mvs_image_pair(mvs_ctx *ctx, const uint8_t *base_desc, const float *base_kp, int n_base,
                          const uint8_t *pair_desc, const float *pair_kp, int n_pair, int desc_bytes, const double K[9],
                          const mvs_params *params, mvs_pair_result *result, mvs_match *matches, uint8_t *inlier_mask,
                          double *points_xyz, int64_t *point_idx);
/* mvs_image_pair with the five-point branch of find_essential_matrix (sfm-solve.cpp:42-63) in place of the 8-point RANSAC:
 * what mvs_match_hamming, a host gather of kp[trainIdx] / kp[queryIdx] and mvs_two_view_essential return, in one upload, one
 * synchronisation and one download.  Same arguments, outputs and return codes.  Honours mvs_ctx_set_essential_confidence and
 * feeds mvs_ctx_essential_hypotheses_run (0 for a pair with fewer than eight matches). */
mvs_status mvs_image_pair_essential(mvs_ctx *ctx, const uint8_t *base_desc, const float *base_kp, int n_base,
                                    const uint8_t *pair_desc, const float *pair_kp, int n_pair, int desc_bytes,
                                    const double K[9], const mvs_params *params, mvs_pair_result *result, mvs_match *matches,
                                    uint8_t *inlier_mask, double *points_xyz, int64_t *point_idx);

/* sfm_triangulate(p1, p2, K, pose1, pose2, points, point_indexes) (sfm-solve.cpp:370-394, decl sfm.hpp:47-53).
 * R1to2 / t1to2 = (pose2^-1 * pose1), composed by the caller-side shim exactly as the reference does. */
mvs_status mvs_triangulate(mvs_ctx *ctx, const double *p1_uv, const double *p2_uv, int m, const double K[9],
                           const double R1to2[9], const double t1to2[3], double *points_xyz, int64_t *point_idx,
                           int *n_points);

/* recover_pose_and_points(E, ...) + pose inverse (sfm-solve.cpp:232-284,364): the tail of sfm_solve for a
 * caller-supplied essential matrix and inlier mask (mask may be NULL = all ones).  Not public in the
 * reference; exported so the cube fixture (test/test-sfm.cpp:17-90) can pin decomposition + triangulation. */
mvs_status mvs_recover_pose(mvs_ctx *ctx, const double E[9], const double *p1_uv, const double *p2_uv, int m,
                            const double K[9], const uint8_t *inlier_mask, double R[9], double t[3],
                            double *points_xyz, int64_t *point_idx, int *n_points, mvs_pair_result *result);

/* find_fundamental_matrix(p1_sample, p2_sample, F21) (vision/fundamental-matrix.cpp:204-267, hpp:16-19).
 * p1 / p2: 8 x (x, y) ideal-camera points (homogeneous 1).  MVS_NO_MODEL for a degenerate sample. */
mvs_status mvs_find_fundamental_matrix(mvs_ctx *ctx, const double p1_xy[16], const double p2_xy[16], double F[9]);

/* FundamentalMatrixEstimatorRANSAC(max_error_sq, max_iteration).compute(p1, p2, F21, inlier_mask)
 * (vision/estimator-RANSAC.cpp:16-90, hpp:20-24).  p1 / p2: m x (x, y) ideal-camera points.
 * count / residual: optional per-hypothesis tables [num_hypotheses] (count -1 = rejected sample). */
mvs_status mvs_ransac_fundamental(mvs_ctx *ctx, const double *p1_xy, const double *p2_xy, int m,
                                  double max_error_sq, int num_hypotheses, int sampler, uint64_t seed, double F[9],
                                  uint8_t *inlier_mask, int *best_hyp, int *best_count, double *best_residual,
                                  int32_t *count, double *residual);

/* ---- find_essential_matrix under USE_OPENCV_ESSENTIAL_MATRIX (vision/sfm-solve.cpp:42-63; the reference's default build,
 *      SConstruct:81-82): a calibrated five-point RANSAC with a Sampson-distance threshold of sqrt(max_error_sq).  The reference
 *      forwards to cv::findEssentialMat, whose arithmetic is not in its tree; this is the build's own, fully specified estimator
 *      (mvslam_amd/csrc/five_point.hpp, essential5.hip):
 *        sample   the first five indices of the 8-of-M draw of hypothesis h (MVS_SAMPLER_IDENTITY: matches 0 .. 4); m >= 8 as
 *                 sfm-solve.cpp:37 asserts;
 *        solve    Nister's five-point solver: up to ten essential matrices per hypothesis, ordered by ascending root (the ROOT
 *                 INDEX), each with Frobenius norm sqrt(2) and its largest entry positive;
 *        score    match i is an inlier iff its squared Sampson distance num / den satisfies den > 0 and
 *                 num <= max_error_sq * den (binary64, operation order in five_point.hpp);
 *        select   most inliers; then the smaller residual (ONE sequential binary64 sum of num / den over the inliers, i ascending;
 *                 estimator-RANSAC.cpp:76-84); then the smaller hypothesis id; then the smaller root index;
 *        stop     with mvs_ctx_set_essential_confidence at 0 (the default) every hypothesis runs.  With a confidence level
 *                 p (VF_MATCH_CONFIDENCE_LEVEL, sfm-solve.cpp:22-23,58) a pair with M matches is tested at the checkpoints
 *                 T_0 = min(64, H), T_{j+1} = min(2 T_j, H) (H = num_hypotheses): with c the largest count over the
 *                 hypotheses h < T_j it stops at T_j iff T_j = H, or c >= 1 and (1 - (c / M)^5)^(64 2^j) <= 1 - p -- in
 *                 binary64, one rounded operation each: w = c / M, w2 = w w, w5 = (w2 w2) w, q = 1 - w5, then q squared
 *                 6 + j times; no logarithm (e5_confident, five_point.hpp).  The checkpoint T it stops at is the pair's
 *                 n_run, and every output is what the same call returns with num_hypotheses = T: hypotheses >= T take no
 *                 part.  Coarser than cv::findEssentialMat's per-iteration update on purpose: 64 hypotheses cost what one
 *                 costs, and doubling bounds the overrun by a factor of two;
 *        no refit, no projection (:62-63). ---- */

/* The minimal solver alone.  p1_xy / p2_xy: 5 x (x, y) ideal-camera points.  E_out: [10][9] row-major, rows [*n, 10) zero.
 * *n = 0 for a degenerate sample; never a non-finite matrix. */
mvs_status mvs_five_point(mvs_ctx *ctx, const double p1_xy[10], const double p2_xy[10], double E_out[90], int *n);

/* The RANSAC stage alone (the five-point counterpart of mvs_ransac_fundamental).  p1 / p2: m x (x, y) ideal-camera points,
 * 8 <= m <= 4096 (fewer: MVS_NO_MODEL, more: MVS_ERR_CAPACITY).  Outputs (any may be NULL): E of the winner, inlier_mask[m],
 * its hypothesis id, root index, inlier count and residual; n_roots[num_hypotheses] and count[num_hypotheses][10] (-1 past
 * n_roots): the optional per-hypothesis tables; rows from the call's n_run on read n_roots = 0, count = -1. */
mvs_status mvs_ransac_essential(mvs_ctx *ctx, const double *p1_xy, const double *p2_xy, int m, double max_error_sq,
                                int num_hypotheses, int sampler, uint64_t seed, double E[9], uint8_t *inlier_mask, int *best_hyp,
                                int *best_root, int *best_count, double *best_residual, int32_t *n_roots, int32_t *count);

/* sfm_solve (vision/sfm-solve.cpp:285-368) with the five-point branch: arguments and return codes of mvs_two_view.  In the
 * result F and E both hold the winner (returned as is, sfm-solve.cpp:62-63) and best_hyp is its hypothesis id. */
mvs_status mvs_two_view_essential(mvs_ctx *ctx, const double *p1_uv, const double *p2_uv, int m, const double K[9],
                                  const mvs_params *params, double R[9], double t[3], double *points_xyz, int64_t *point_idx,
                                  int *n_points, uint8_t *inlier_mask, mvs_pair_result *result);

/* pnp_solve(world_points, image_points, K, pose, inlier_point_indexes) (vision/pnp-solve.cpp:16-104, decl pnp.hpp:22-26).
 * The reference forwards to cv::solvePnPRansac(SOLVEPNP_P3P, 100, 0.05, 0.95); this is the build's own P3P-RANSAC
 * (Grunert P3P on 3 points + 1 disambiguation point, reprojection-error inlier count over all points, first
 * hypothesis with the most inliers, no refit).  pose = camera in world, i.e.
 * SE3(R_world_to_camera, t).inverse() (pnp-solve.cpp:99-101).  n >= 7 (PNP_MIN_POINT_COUNT, :13) and n <= 4096 (the keypoint capacity).
 * inlier_idx: capacity n, ascending.  returns MVS_OK (true) / MVS_NO_MODEL (false). */
typedef struct mvs_pnp_params {
    int32_t num_hypotheses; /* reference: iterationsCount = 100 (pnp-solve.cpp:47) */
    int32_t sampler;        /* MVS_SAMPLER_* (identity = points 0..3) */
    uint64_t seed;
    double reproj_error;    /* 0.05 (pnp-solve.cpp:48), pixels of the given image points */
    int32_t min_inliers;    /* 4: the model points of the RANSAC kernel */
    int32_t refit;          /* 0 (default): return the best P3P hypothesis.  1: then minimise the reprojection error over
                               ALL inliers (pose only, points fixed), the refit cv::solvePnPRansac ends with
                               (pnp-solve.cpp:53-64); the inlier set stays the RANSAC one.  Honoured by mvs_pnp_solve and,
                               batched over all tracks on the device, by mvs_seq_run */
} mvs_pnp_params;
mvs_status mvs_pnp_params_default(mvs_pnp_params *p);
mvs_status mvs_pnp_solve(mvs_ctx *ctx, const double *world_xyz, const double *image_uv, int n, const double K[9],
                         const mvs_pnp_params *params, double R[9], double t[3], int64_t *inlier_idx, int *n_inliers,
                         int *best_hyp);

/* ---- batched, device-resident pipeline ("one image pair" = ImagePair ctor + reconstruct,
 *      front-end/image-pair.cpp:30-71,116-174, without refine()) ---------------------- */

/* capacity: n_pairs pairs, max_kp keypoints per image (<= 4096), desc_bytes per descriptor. */
mvs_status mvs_batch_create(mvs_ctx *ctx, int n_pairs, int max_kp, int desc_bytes, mvs_batch **out);
void mvs_batch_destroy(mvs_batch *b);

/* Upload pairs [first, first + count).  base = vf1 = train, pair = vf2 = query.
 * desc: count x max_kp x desc_bytes (rows >= n are ignored); kp: count x max_kp x (x, y) float (cv::KeyPoint::pt);
 * n_base / n_pair: count;  K: count x 9;  global_index: count (NULL = first + i), added to params.seed. */
mvs_status mvs_batch_upload(mvs_batch *b, int first, int count, const uint8_t *base_desc, const float *base_kp,
                            const int32_t *n_base, const uint8_t *pair_desc, const float *pair_kp,
                            const int32_t *n_pair, const double *K, const int64_t *global_index);

/* Asynchronous form: enqueues the copies on the ctx stream and returns.  The host buffers must stay valid and unchanged
 * until mvs_batch_sync; with buffers from mvs_host_alloc (pinned) the copies are true DMA transfers that overlap the
 * kernels of another batch / ctx (double buffering: upload batch k+1 while batch k runs).  K^-1 and the default indices
 * are staged in pinned memory owned by the batch. */
mvs_status mvs_batch_upload_async(mvs_batch *b, int first, int count, const uint8_t *base_desc, const float *base_kp,
                                  const int32_t *n_base, const uint8_t *pair_desc, const float *pair_kp,
                                  const int32_t *n_pair, const double *K, const int64_t *global_index);
/* pinned (page-locked) host memory for the asynchronous transfers; any entry point accepts pageable memory too */
mvs_status mvs_host_alloc(size_t bytes, void **out);
void mvs_host_free(void *p);

/* Enqueue the whole pipeline for pairs [0, n_active) on the ctx stream (asynchronous). */
mvs_status mvs_batch_run(mvs_batch *b, const mvs_params *params, int n_active);
mvs_status mvs_batch_sync(mvs_batch *b);

/* A batch of sfm_solve calls (vision/sfm.hpp:30-35; vision/sfm-solve.cpp:285-368) on caller-supplied matched image points:
 * what mvs_batch_run does behind the matcher (normalise -> 8-point RANSAC -> E -> decomposition -> triangulation), for pairs
 * [0, n_active).  uv1 / uv2: HOST memory, [n_active][max_kp][2] doubles, row k of pair p = match k in the base / pair frame;
 * m[p] = matches of pair p (0 .. max_kp; fewer than 8 -> the pair comes back invalid, estimator-RANSAC.cpp:25-29).  Uses
 * the intrinsics and sampler key offsets resident in the batch (mvs_batch_upload accepts null descriptor / keypoint pointers
 * to set only K and global_index).  The host buffers are free again when the call returns; the kernels are asynchronous on
 * the ctx stream.  Afterwards mvs_batch_download returns results / mask / points / point_idx as usual (point_idx indexes the
 * rows of uv1 / uv2) and cleared match rows. */
mvs_status mvs_batch_run_points(mvs_batch *b, const mvs_params *params, int n_active, const double *uv1, const double *uv2,
                                const int32_t *m);

/* mvs_batch_run_points with the five-point branch of find_essential_matrix (mvs_two_view_essential for pairs [0, n_active)):
 * same arguments, same resident intrinsics and sampler key offsets, followed by the usual mvs_batch_download.  One stream, plain
 * launches: no half batches, no captured graph. */
mvs_status mvs_batch_run_points_essential(mvs_batch *b, const mvs_params *params, int n_active, const double *uv1,
                                          const double *uv2, const int32_t *m);
/* mvs_batch_run with the five-point branch: matcher -> five-point RANSAC -> decomposition -> triangulation on the resident
 * descriptors and keypoints of pairs [0, n_active), no host round trip in between.  One stream, plain launches (no half
 * batches, no captured graph); honours mvs_ctx_set_essential_confidence.  Followed by the usual mvs_batch_sync and
 * mvs_batch_download, match list included. */
mvs_status mvs_batch_run_essential(mvs_batch *b, const mvs_params *params, int n_active);
/* n_run[count] of pairs [first, first + count) in the batch's LAST mvs_batch_run_points_essential or mvs_batch_run_essential:
 * num_hypotheses, or the checkpoint the pair stopped at under a confidence level; 0 for a pair with fewer than eight
 * matches and for a pair at or beyond that call's n_active, whatever an earlier call did with it.  The words are the
 * device's: the call waits for the ctx stream.
 * MVS_ERR_INVALID_ARG before the first such call. */
mvs_status mvs_batch_download_hypotheses_run(mvs_batch *b, int first, int count, int32_t *n_run);
/* The per-hypothesis tables of pairs [first, first + count) in the batch's last five-point run of either kind, as
 * mvs_ransac_essential exports them: n_roots [count][num_hypotheses], count_tbl [count][num_hypotheses][10] with -1 past
 * n_roots; from the pair's n_run on (see above; 0 with fewer than eight matches) n_roots = 0 and count = -1.  Either pointer
 * may be NULL.  Waits for the ctx stream.  MVS_ERR_INVALID_ARG before the first such run or when num_hypotheses is not that
 * run's. */
mvs_status mvs_batch_download_essential_tables(mvs_batch *b, int first, int count, int num_hypotheses, int32_t *n_roots,
                                               int32_t *count_tbl);

/* Timed replay: `warmup` untimed + `steps` timed passes over the resident inputs, bracketed by HIP events
 * on the ctx stream.  ms_total: wall ms of the `steps` passes.  ms_kernel[5]: summed ms per kernel over the
 * timed passes, in launch order {match (match_mfma or match_topk), match_compact, ransac, finalize, reserved}; measured with
 * per-kernel events in a SEPARATE instrumented replay of `steps` passes (so ms_total has no event overhead).
 * Either output may be NULL. */
mvs_status mvs_batch_time(mvs_batch *b, const mvs_params *params, int n_active, int warmup, int steps,
                          float *ms_total, float *ms_kernel);

/* Per-launch timing of one pipeline pass: `steps` instrumented passes with a HIP event in front of every kernel launch
 * (on the ctx stream, where the kernels run).  kernel_id[k] / ms[k]: id (index into mvs_kernel_info_get) and mean
 * duration of launch k of a pass, in launch order; *n_launches: launches per pass (<= cap).  Outside any timed region. */
mvs_status mvs_batch_time_kernels(mvs_batch *b, const mvs_params *params, int n_active, int steps, int cap,
                                  int32_t *kernel_id, float *ms, int *n_launches);

/* The kernels of the two-view pipeline as they are launched for a batch of this shape: name (as rocprofv3 prints it) and
 * what the runtime reports for the code object that is actually loaded (hipFuncGetAttributes,
 * hipOccupancyMaxActiveBlocksPerMultiprocessor) -- so a bench line never carries typed-in register counts.
 * index: 0 .. n-1; returns MVS_ERR_INVALID_ARG past the end. */
typedef struct mvs_kernel_info {
    char name[96];
    char symbol[160];              /* mangled name of the code object's kernel (key into lib/kernel_resources.json) */
    int32_t kernel_id;
    int32_t threads_per_block;     /* as launched */
    int32_t num_regs;              /* hipFuncAttributes.numRegs (vector registers per lane, architected + accumulation) */
    int32_t static_lds_bytes;      /* hipFuncAttributes.sharedSizeBytes */
    int32_t dynamic_lds_bytes;     /* as launched for this batch shape */
    int32_t scratch_bytes_per_lane;/* hipFuncAttributes.localSizeBytes */
    int32_t max_threads_per_block;
    int32_t blocks_per_cu;         /* hipOccupancyMaxActiveBlocksPerMultiprocessor at that block size and LDS */
    int32_t waves_per_simd;        /* blocks_per_cu * ceil(threads / 64) / 4 SIMDs, rounded down, at least 1 if resident */
    int32_t reserved;
} mvs_kernel_info;
mvs_status mvs_kernel_info_get(mvs_ctx *ctx, int index, int max_kp, int desc_bytes, mvs_kernel_info *out);

/* Results (host).  Any pointer may be NULL.  results: count;  matches: count x max_kp;  mask: count x max_kp;
 * points: count x max_kp x 3;  point_idx: count x max_kp.  Valid rows of pair p: matches / mask [0, results[p].n_matches),
 * points / point_idx [0, results[p].n_points); every row past them is ZERO (the kernels clear the tails on every run, so
 * the whole-capacity copy is deterministic). */
mvs_status mvs_batch_download(mvs_batch *b, int first, int count, mvs_pair_result *results, mvs_match *matches,
                              uint8_t *inlier_mask, double *points_xyz, int64_t *point_idx);

/* Asynchronous form of mvs_batch_download: enqueues the copies after whatever is already on the ctx stream (no sync is
 * needed between mvs_batch_run and this call) and returns; the data is valid after mvs_batch_sync.  point_idx32 is the
 * device's native int32 index (the synchronous form widens to the reference's size_t on the host).  Row ranges as for
 * mvs_batch_download; rows past them are zero. */
mvs_status mvs_batch_download_async(mvs_batch *b, int first, int count, mvs_pair_result *results, mvs_match *matches,
                                    uint8_t *inlier_mask, double *points_xyz, int32_t *point_idx32);

/* Work statistics of the last run (for the roofline's algorithmic flop count): executed 9x9 Jacobi rotations,
 * visited 9x9 pairs, hypotheses, hypothesis x point evaluations, summed over pairs [0, n_active).
 * Collected by an instrumented replay outside any timed region. */
typedef struct mvs_work_stats {
    int64_t hypotheses;
    int64_t rotations9;
    int64_t pairs9;
    int64_t score_evals;
    int64_t matches; /* sum of M */
    int64_t inliers; /* sum of n_inliers */
    int64_t score_evals_executed; /* (hypothesis, point) evaluations the pruned counting kernels actually executed (incl. the
                                     NaN padding of a pair's last block); 0 when the batch runs on the fused kernel */
    int64_t score_evals_executed_f32; /* the part of them evaluated in single precision (pairs in mode 1) */
    int64_t exact_solves;         /* hypotheses that went through the exact (Jacobi) solve: every hypothesis of a pair in mode
                                     0, + the ones the pre-screen could not certify, + the survivors of the counting */
    int64_t prescreened;          /* hypotheses that only ever got the pre-screen's approximate F (never solved exactly) */
    int64_t pairs_mode[3];        /* pairs per mode: 0 every hypothesis exact, 1 pre-screened + single-precision counting,
                                     2 pre-screened + double-precision counting */
    int64_t score_evals_executed_mfma; /* the part of score_evals_executed done by the dense matrix-core phase (split bf16) */
    int64_t score_evals_executed_mfma_finish; /* ... and by the matrix-core finish (upper and lower bound per evaluation) */
    /* ABI 3 */
    int64_t max_sweeps9;          /* largest number of sweeps any 9x9 Jacobi SVD of the replay took (OpenCV's cap: 30; the
                                     pre-screen's bound assumes the iteration ends by its own test within it) */
    int64_t dense_points;         /* sum over the pairs in mode 1 of n1, the points the dense matrix-core phase covered */
    int64_t matches_mode1;        /* sum of M over the same pairs (dense_points / matches_mode1 = the share of a pair's matches
                                     every hypothesis is counted on before anything can be dropped) */
    int64_t score_evals_executed_mfma_rest; /* evaluations of the finish's second launch (upper counts of the rest of the list);
                                     included in score_evals_executed, not in score_evals_executed_mfma_finish */
    int64_t score_evals_executed_mfma_pilot; /* evaluations of the matrix-core pilot (the first 1024 hypotheses of every pair in
                                     mode 1 on every match, both bounds): included in score_evals_executed */
} mvs_work_stats;
mvs_status mvs_batch_stats(mvs_batch *b, const mvs_params *params, int n_active, mvs_work_stats *out);

/* Diagnostics: a read-only, opaque view of the batch's device-resident state (the library's internal table of device pointers
 * and capacities, prefixed by its size and the ABI version).  Nothing is launched, copied on the device or modified; call
 * mvs_batch_sync first.  Its one consumer is the audit of libmvslam_hip_dbg.so (same sources, same process), which replays
 * every hypothesis exactly and checks the decisions THIS library's kernels left in device memory
 * (tests/audit_gpu_check.py).  dst == NULL: *size receives the number of bytes needed. */
mvs_status mvs_batch_device_state(mvs_batch *b, void *dst, size_t capacity, size_t *size);

/* Device pointer + pitch of the fixed-size result records (mvs_pair_result[n_pairs]) so a caller can hand them
 * to a collective (RCCL all-gather of poses) without a host round trip. */
mvs_status mvs_batch_results_device(mvs_batch *b, void **dev_ptr, size_t *record_bytes);

/* Asynchronous device-to-device copy (on the ctx stream) of the result records of pairs [first, first + count)
 * into caller-owned DEVICE memory, e.g. a torch tensor that is then all-gathered over RCCL. */
mvs_status mvs_batch_copy_results_device(mvs_batch *b, int first, int count, void *dst_device);
/* The one exchange step of the sharded path (pairs are independent: front-end/image-pair.hpp:56-57): one
 * ncclAllGather over RCCL / xGMI of the records of pairs [0, n_active), enqueued on the ctx stream after the batch's
 * kernels.  rccl_comm: the caller's ncclComm_t (one rank per GPU); dst_device: world_size x n_active x
 * sizeof(mvs_pair_result) bytes of device memory, rank-major.  Asynchronous; librccl.so is loaded on first use. */
mvs_status mvs_batch_gather_results(mvs_batch *b, int n_active, void *rccl_comm, void *dst_device);

/* ---- frame sequences, device resident -------------------------------------------------
 * What VisualOdometer::add_frame chains per frame (front-end/visual-odometer.cpp:129-194,384-445,502-615):
 * ImagePair(prev, new) and track_pnp on the 3-D points the previous pair triangulated.  Every frame is uploaded ONCE;
 * pair k = (base = frame k, pair = frame k + 1) is a zero-copy view into the frame arrays (frame k is `pair` of pair
 * k-1 and `base` of pair k).  Track q (q = 0 .. n_frames-3) joins, on the device, the points of pair q (expressed in
 * frame q's camera) to their observations in frame q + 2 through pair q + 1's matches (the vf-index join of
 * visual-odometer.cpp:528-556) and runs pnp_solve on them: pose of frame q + 2 in frame q's camera frame.
 * Of the VO state machine, scale propagation (mvs_seq_download_trajectory), BA (mvs_seq_refine_pairs,
 * mvs_seq_refine_windows) and the tracking loop VisualOdometer::track with its persistent map (mvs_seq_track, below) run on
 * the device behind mvs_seq_run; the initialisation gates (check_image_pair), ImagePair::update and reset() -- the whole of
 * add_frame -- run on the device in mvs_seq_odometry (below), over the lagged pairs of mvs_seq_run_lags. */
typedef struct mvs_seq mvs_seq;
typedef struct mvs_track_result {
    int32_t ok;        /* pnp_solve returned true */
    int32_t n_corr;    /* 3-D / 2-D correspondences found by the join */
    int32_t n_inliers;
    int32_t best_hyp;
    double R[9];       /* pose of frame q + 2 in frame q's camera frame (pnp-solve.cpp:99-101 convention) */
    double t[3];
} mvs_track_result;

mvs_status mvs_seq_create(mvs_ctx *ctx, int n_frames, int max_kp, int desc_bytes, mvs_seq **out);
void mvs_seq_destroy(mvs_seq *s);
/* frames [first, first + count): desc count x max_kp x desc_bytes, kp count x max_kp x 2 float, n_kp count; one camera K */
mvs_status mvs_seq_upload(mvs_seq *s, int first, int count, const uint8_t *desc, const float *kp, const int32_t *n_kp,
                          const double K[9]);
/* all pairs (batched two-view pipeline) + all tracks (join + batched PnP), asynchronous on the ctx stream */
mvs_status mvs_seq_run(mvs_seq *s, const mvs_params *two_view, const mvs_pnp_params *pnp);
/* mvs_seq_run with the five-point RANSAC (mvs_batch_run_essential) for the n_frames - 1 pairs; the join, PnP, optional refit
 * and scale chain are mvs_seq_run's, and every mvs_seq_download_* / mvs_seq_refine_* call works behind it unchanged */
mvs_status mvs_seq_run_essential(mvs_seq *s, const mvs_params *two_view, const mvs_pnp_params *pnp);
/* mvs_batch_download_hypotheses_run for pairs [first, first + count) of the sequence's last mvs_seq_run_essential */
mvs_status mvs_seq_download_hypotheses_run(mvs_seq *s, int first, int count, int32_t *n_run);
mvs_status mvs_seq_sync(mvs_seq *s);
/* `steps` timed passes after `warmup`; ms_total = wall ms of the timed passes (HIP events on the ctx stream) */
mvs_status mvs_seq_time(mvs_seq *s, const mvs_params *two_view, const mvs_pnp_params *pnp, int warmup, int steps,
                        float *ms_total);
/* per-stage HIP-event timing of the sequence step (the kernels' own stream): ms_stage[4] = summed ms over `steps`
 * instrumented passes of {pair pipeline, join, pnp_solve, scale propagation}.  Every pass is an mvs_seq_run with these
 * parameters: afterwards the pairs, tracks and trajectory are the last pass's and the sequence counts as run, and whatever
 * was derived from an earlier run (windows, tracking, refined pairs as a tracking start, lags, odometry, pose graph) is
 * stale, exactly as after mvs_seq_run */
mvs_status mvs_seq_time_stages(mvs_seq *s, const mvs_params *two_view, const mvs_pnp_params *pnp, int steps, float *ms_stage);
/* pairs [first, first + count) of the n_frames - 1 pairs: same layout as mvs_batch_download */
mvs_status mvs_seq_download_pairs(mvs_seq *s, int first, int count, mvs_pair_result *results, mvs_match *matches,
                                  uint8_t *inlier_mask, double *points_xyz, int64_t *point_idx);
/* tracks [first, first + count) of the n_frames - 2 tracks.  corr_xyz / corr_uv: count x max_kp x 3 / 2 (the joined
 * correspondences, may be NULL); inlier_idx: count x max_kp (indices into the correspondences, may be NULL) */
mvs_status mvs_seq_download_tracks(mvs_seq *s, int first, int count, mvs_track_result *tracks, double *corr_xyz,
                                   double *corr_uv, int64_t *inlier_idx);

/* ---------------------------------------------------------------------------------------------------------------
 * Row f4: refinement.  Replaces sfm_refine (vision/sfm.hpp:56-76, sfm-refine.cpp:20-139) and
 * pnp_refine (vision/pnp.hpp:28-46, pnp-refine.cpp:14-108), i.e. the two callers of ba_frame_pose_and_point
 * (vision/ba.cpp:26-156, GTSAM LevenbergMarquardtOptimizer + Marginals).  The library minimises the same cost
 *   1/2 [ pose priors + point priors + reprojection residuals, each in its Mahalanobis norm ]
 * with its own batched Schur-complement Levenberg-Marquardt kernel and returns the minimiser, the marginal covariances
 * of the linearised problem (ba.cpp:127,141,152) and the final error (ba.cpp:155).  Pose tangent order is GTSAM's:
 * (rotation, translation), right perturbation.  DESIGN.md section 4.7. */
typedef struct mvs_refine_params {
    int32_t max_iterations;  /* 100 = gtsam::LevenbergMarquardtParams default */
    int32_t reserved;
    double lambda_initial;   /* 1e-5 */
    double lambda_factor;    /* 10 */
    double lambda_upper;     /* 1e5 */
    double rel_tol;          /* 1e-12: stop when the error decrease is below rel_tol * error ... */
    double abs_tol;          /* 1e-12: ... or below abs_tol (GTSAM's defaults are 1e-5 / 1e-5) */
    double anchor_sigma[2];  /* sfm-refine.cpp:11-14: prior on camera 1, diagonal entries {0-2, 3-5} = {1e-5, 1e-5} */
    double pose_sigma[2];    /* sfm-refine.cpp:15-18, pnp-refine.cpp:9-12: regulator on the moving camera {1e-2, 1e-2} */
    double point_sigma;      /* sfm-refine.cpp:86-94: regulator on every point, 1e-2 */
} mvs_refine_params;
void mvs_refine_params_default(mvs_refine_params *p);

typedef struct mvs_refine_result {
    int32_t ok;          /* 1: converged or stopped by the iteration / lambda limits with a finite error */
    int32_t iterations;  /* linear solves performed */
    double error;        /* 1/2 sum of squared Mahalanobis residuals at the estimate (optimizer.error()) */
    double R[9];         /* the moving camera in the world frame (sfm: pose2in1) */
    double t[3];
    double pose_cov[36]; /* its marginal covariance, row-major 6 x 6, order (rotation, translation) */
} mvs_refine_result;

/* sfm_refine.  p1 / p2: m x 2 image points (host), cov1 / cov2: m x 4 (row-major 2 x 2 covariances) or NULL = identity,
 * K affine, (R_guess, t_guess) = pose2in1 guess, points_guess m x 3 in camera 1.  points_out: m x 3, point_cov_out:
 * m x 9 (may be NULL).  1 <= m <= 4096.  MVS_NO_MODEL if the problem could not be solved. */
mvs_status mvs_sfm_refine(mvs_ctx *ctx, const double *p1, const double *cov1, const double *p2, const double *cov2, int m,
                          const double K[9], const double R_guess[9], const double t_guess[3],
                          const double *points_guess, const mvs_refine_params *params, mvs_refine_result *result,
                          double *points_out, double *point_cov_out);
/* pnp_refine.  world: m x 3 with covariances world_cov m x 9 (the point priors), image points m x 2 with covariances
 * image_cov m x 4 or NULL = identity; (R_guess, t_guess) = camera in world. */
mvs_status mvs_pnp_refine(mvs_ctx *ctx, const double *world, const double *world_cov, const double *image,
                          const double *image_cov, int m, const double K[9], const double R_guess[9],
                          const double t_guess[3], const mvs_refine_params *params, mvs_refine_result *result);
/* ba_frame_pose_and_point (vision/ba.hpp:25-36, ba.cpp:26-156) for the configurations the reference builds -- one or two
 * frames: besides sfm_refine / pnp_refine that is VisualOdometer::track_refine (front-end/visual-odometer.cpp:618-800:
 * last frame anchored at ITS pose, new frame regularised, tracked points with priors, new points without, each frame
 * observing a subset of the points).  All pointers are host memory.  Windows of up to eight frames: mvs_ba_window and
 * mvs_ba_refine_window / mvs_ba_refine_windows below. */
typedef struct mvs_ba_problem {
    int32_t n_frames;               /* 1 or 2 */
    int32_t n_points;               /* 1 .. 4096 */
    const double *K;                /* 9, affine */
    const double *frame_pose;       /* n_frames x 12: R (9 row-major), t (3): camera in world = guess = prior mean */
    const double *frame_prior_var;  /* n_frames x 6: DIAGONAL of the prior covariance in tangent order (rotation,
                                       translation); an entry <= 0 = no prior on that coordinate */
    const double *points;           /* n_points x 3 guesses (= prior means) */
    const double *point_prior_cov;  /* n_points x 9, or NULL = no point has a prior; a point whose covariance has a
                                       first entry <= 0 has no prior (track_refine's new points) */
    const double *obs[2];           /* per frame: n_points x 2 image points */
    const double *obs_cov[2];       /* per frame: n_points x 4 covariances, or NULL = identity */
    const uint8_t *obs_valid[2];    /* per frame: n_points flags (0 = the frame does not observe the point), or NULL = all */
} mvs_ba_problem;
/* frames_out[n_frames]: pose estimate and marginal covariance of every frame (error / iterations repeated in each);
 * points_out n_points x 3, point_cov_out n_points x 9 (may be NULL).  Only the LM fields of params are used. */
mvs_status mvs_ba_refine(mvs_ctx *ctx, const mvs_ba_problem *problem, const mvs_refine_params *params,
                         mvs_refine_result *frames_out, double *points_out, double *point_cov_out);
/* ba_frame_pose_and_point for any frame set of 1 .. 8 frames (the reference takes sets and maps keyed by frame id and loops
 * over whatever it is given, ba.cpp:26-156): a sliding window.  The fields are mvs_ba_problem's; the per-frame arrays are
 * arrays of n_frames pointers, so the frame count is not part of the layout.  ba.cpp:43 demands two priors (the gauge must
 * be fixed: e.g. an anchor on frame 0 and a scale-fixing prior on another frame or on points). */
typedef struct mvs_ba_window {
    int32_t n_frames;                 /* 1 .. 8 */
    int32_t n_points;                 /* 1 .. 4096 */
    const double *K;                  /* 9, affine */
    const double *frame_pose;         /* n_frames x 12 */
    const double *frame_prior_var;    /* n_frames x 6, an entry <= 0 = no prior on that coordinate */
    const double *points;             /* n_points x 3 */
    const double *point_prior_cov;    /* n_points x 9 or NULL; first entry <= 0 = no prior on that point */
    const double *const *obs;         /* n_frames pointers: n_points x 2 image points */
    const double *const *obs_cov;     /* NULL, or n_frames pointers: n_points x 4 covariances or NULL = identity */
    const uint8_t *const *obs_valid;  /* NULL, or n_frames pointers: n_points flags or NULL = the frame sees every point */
} mvs_ba_window;
/* One window.  n_frames 1 or 2 is forwarded to mvs_ba_refine (the same bytes out); 3 .. 8 runs the window kernel (DESIGN.md
 * section 4.7); more than 8 frames or 4096 points: MVS_ERR_CAPACITY; the other argument errors as mvs_ba_refine.  MVS_NO_MODEL
 * (ok = 0 in every frame record) if the problem has no unique minimum to working precision: the reduced camera system or a
 * point's 3 x 3 block is not positive definite -- no prior fixes the gauge, or a point is neither observed nor has a prior.
 * frames_out[n_frames], points_out n_points x 3 (may be NULL), point_cov_out n_points x 9 (may be NULL). */
mvs_status mvs_ba_refine_window(mvs_ctx *ctx, const mvs_ba_window *problem, const mvs_refine_params *params,
                                mvs_refine_result *frames_out, double *points_out, double *point_cov_out);
/* A batch of windows that may differ in frames and points: one upload, ONE launch (one workgroup per window), one
 * synchronisation and one download for all its windows of three and more frames; its windows of one or two frames go through
 * mvs_ba_refine one by one, so that every window returns the bytes the single call returns.  Output strides are the batch's
 * largest frame and point counts (Fmax, Mmax): frames_out[n_problems x Fmax], points_out n_problems x Mmax x 3,
 * point_cov_out n_problems x Mmax x 9 (either may be NULL); rows beyond a window's own counts are not written.  frames_out is
 * zeroed once the frame counts have been checked, also when the call then returns an argument error.  An argument error in any
 * window fails the call before anything runs.  MVS_NO_MODEL if at least one window has
 * ok = 0 (frames_out[p * Fmax].ok tells which). */
mvs_status mvs_ba_refine_windows(mvs_ctx *ctx, const mvs_ba_window *problems, int n_problems, const mvs_refine_params *params,
                                 mvs_refine_result *frames_out, double *points_out, double *point_cov_out);
/* ba_frame_pose_and_point for 1 .. 4096 frames, fed as a SPARSE problem: every point lists the
 * frames that observe it, so an observation a frame lacks is simply absent.  Cost, tangent order (rotation, translation; right
 * perturbation) and LM rule are the window kernel's; the points are eliminated on the device, the reduced camera system is
 * assembled into its block skyline (row i reaches back to the smallest frame that shares a point with frame i) and the LM step
 * is the block-scaled skyline Cholesky of mvs_ctx_set_pose_graph_solver's direct solver; the host drives the lambda schedule
 * with one synchronisation per iteration.  Tracks over consecutive frames give a band whose width is the longest track. */
typedef struct mvs_ba_sparse {        /* all host pointers */
    int32_t n_frames;                 /* 1 .. 4096 */
    int32_t n_points;                 /* 1 .. 1 << 20 */
    int32_t n_obs;                    /* 1 .. 1 << 23 */
    int32_t reserved;
    const double *K;                  /* 9, affine */
    const double *frame_pose;         /* n_frames x 12, as mvs_ba_window */
    const double *frame_prior_var;    /* n_frames x 6, <= 0: no prior on that coordinate */
    const double *points;             /* n_points x 3 */
    const double *point_prior_cov;    /* n_points x 9 or NULL; first entry <= 0: no prior */
    const int32_t *obs_off;           /* n_points + 1: observations of point p are rows obs_off[p] .. obs_off[p+1]-1 */
    const int32_t *obs_frame;         /* n_obs, strictly ascending within a point */
    const double *obs_uv;             /* n_obs x 2 */
    const double *obs_cov;            /* n_obs x 4 or NULL = identity */
} mvs_ba_sparse;
typedef struct mvs_ba_sparse_result {
    int32_t ok, iterations, rejected_steps, failed_solves;
    double error_initial, error;
    int32_t envelope_blocks, widest_row;   /* of the reduced camera system */
    int32_t bad_frame, reserved;           /* first failed pivot's frame, -1 */
} mvs_ba_sparse_result;
/* Every argument error is returned before anything runs.  MVS_ERR_INVALID_ARG: a null pointer (the optional ones apart), a
 * non-finite input, obs_off that is not monotone from 0 to n_obs, obs_frame out of range or not strictly ascending within a
 * point, refine parameters mvs_ba_refine refuses.  MVS_ERR_CAPACITY: the limits above, an envelope of more than 2^21 blocks
 * (the skyline's limit, as for the pose graphs), or more than 2^28 pairs of observations that share a point, counted over all points (sum of t (t - 1) / 2
 * over the tracks' lengths t: the term lists of the assembly).  MVS_NO_MODEL with ok = 0 and every output array untouched: at the estimate (lambda = 0) a point's 3 x 3 block or
 * a pivot of the skyline fails the window kernel's pivot rule -- a gauge no prior fixes, a point with neither observation nor
 * prior; `result` is still filled.  During the iterations such a failure raises lambda (failed_solves counts them).
 * Outputs: poses_out n_frames x 12; points_out n_points x 3, pose_cov_out n_frames x 36 and point_cov_out n_points x 9 may be
 * NULL (the covariance sweep runs only when one of the two is asked for).  Only the LM fields of params are read.  The same
 * input gives the same bytes. */
mvs_status mvs_ba_refine_sparse(mvs_ctx *ctx, const mvs_ba_sparse *problem, const mvs_refine_params *params,
                                mvs_ba_sparse_result *result, double *poses_out /* n_frames x 12 */,
                                double *points_out /* n_points x 3, may be NULL */,
                                double *pose_cov_out /* n_frames x 36, may be NULL */,
                                double *point_cov_out /* n_points x 9, may be NULL */);
/* Robust losses on the reprojection terms of the sparse bundle adjustment, with per-observation statistics (DESIGN.md section
 * 4.7.6; GTSAM: noiseModel::Robust on the projection factors).  New symbols only: mvs_abi_version stays 4.
 * A switch of the context, MVS_BA_LOSS_NONE by default: with it every call launches what it launched before the switch
 * existed and returns the bytes it returned.  mvs_ba_refine_sparse and mvs_seq_refine_global honour it; mvs_ba_refine,
 * mvs_ba_refine_window(s), mvs_seq_refine_windows, mvs_seq_track and every *_refine of pairs IGNORE it.
 *   cost   observation o has the residual r_o (2) and the information matrix W_o; s_o = r_o^T W_o r_o, x = sqrt(s_o).  The
 *          cost becomes 1/2 [pose priors + point priors + sum_o rho2(s_o)], rho2 and the weight w as for the pose graphs:
 *     MVS_BA_LOSS_NONE    rho2 = s                                    w = 1
 *     MVS_BA_LOSS_HUBER   rho2 = s if x <= k, else (2 k) x - k k      w = 1 if x <= k, else k / x
 *     MVS_BA_LOSS_CAUCHY  rho2 = (k k) log1p(s / (k k))               w = (k k) / (k k + s)
 *          The priors are never robustified.  An observation behind its camera keeps its fixed residual (2 fx, 2 fx) and its
 *          zero Jacobians and gets rho2 of that s like any other term.
 *   step   IRLS: observation o enters every sum of the linearisation with the information matrix w(s_o) W_o, nothing else
 *          changes.  s by the cost's own statements (wr0 = fma(W1, r1, W0 r0), wr1 = fma(W2, r1, W1 r0), s = fma(r1, wr1,
 *          r0 wr0)), one sqrt for x, one division for w (the Cauchy cost: log1p of one quotient), three products w W0, w W1,
 *          w W2.  Binary64, no atomics, the same input gives the same bytes; Huber with k = 1e30 has w = 1 and rho2 = s
 *          exactly and returns the bytes of MVS_BA_LOSS_NONE.
 *   LM     the rule, the exits, error, error_initial, rejected_steps and failed_solves are those of mvs_ba_refine_sparse, on
 *          the robust cost: a candidate is accepted when its robust cost is not above the current one.
 *   covariances  pose_cov_out and point_cov_out continue from the lambda = 0 factorisation the solver ends with, which under a
 *          loss is the REWEIGHTED system: they are the covariances of the reweighted linearisation (what GTSAM's Marginals
 *          gives over robust factors).  The pose graphs' marginals, in contrast, stay Gaussian under their loss: that sweep has
 *          an edge evaluation of its own, this one reuses the solver's factor.
 * MVS_ERR_INVALID_ARG, the setting stays: a loss that is none of the three; with a loss other than NONE, a k that is not finite
 * and > 0. */
#define MVS_BA_LOSS_NONE 0
#define MVS_BA_LOSS_HUBER 1
#define MVS_BA_LOSS_CAUCHY 2
mvs_status mvs_ctx_set_ba_loss(mvs_ctx *ctx, int loss, double k);
/* s_o = r_o^T W_o r_o of every observation of `problem` at the given poses and points, and its weight w(s_o) under the
 * context's loss (1.0 under MVS_BA_LOSS_NONE).  The argument checks and status codes are mvs_ba_refine_sparse's (the limits of
 * the plan apart: no plan and no envelope are built, only the observation arrays, the poses and the points are uploaded);
 * non-finite poses or points are MVS_ERR_INVALID_ARG.  Nothing is written on an error.  Waits for the ctx stream. */
mvs_status mvs_ba_sparse_obs_stats(mvs_ctx *ctx, const mvs_ba_sparse *problem,
                                   const double *poses /* n_frames x 12, NULL: frame_pose */,
                                   const double *points /* n_points x 3, NULL: points */,
                                   double *chi2 /* n_obs */, double *weight /* n_obs, may be NULL */);
/* Batched ImagePair::refine (front-end/image-pair.cpp:176-238) on a batch that has been run: every valid pair is refined
 * from its own results on the device.  Observations = the matched keypoints with the covariance
 * VisualFeature::get_point_estimates gives them (vision/visual-feature.cpp:192-207): stddev = (1 << kp.octave) * 0.5 px,
 * i.e. (sigma_px * 2^octave)^2 I with sigma_px = 0.5.  The octave of every keypoint is resident next to its
 * coordinates: written by the device extractor (mvs_seq_upload_images), supplied by the caller for host-uploaded
 * keypoints (mvs_batch_upload_octaves / mvs_seq_upload_octaves), 0 otherwise.
 * Asynchronous on the ctx stream; results stay resident until downloaded. */
mvs_status mvs_batch_refine(mvs_batch *b, const mvs_refine_params *params, double sigma_px);
/* cv::KeyPoint::octave of the keypoints uploaded with mvs_batch_upload: count x max_kp bytes per image (NULL = leave);
 * values above 30 are rejected (MVS_ERR_INVALID_ARG).  Only mvs_batch_refine reads them. */
mvs_status mvs_batch_upload_octaves(mvs_batch *b, int first, int count, const uint8_t *base_octave,
                                    const uint8_t *pair_octave);
/* refined[n_pairs]; points_xyz / point_cov: n_pairs x max_kp x 3 / 9 (NULL to skip), rows [0, results[p].n_points) */
mvs_status mvs_batch_download_refined(mvs_batch *b, mvs_refine_result *refined, double *points_xyz, double *point_cov);
/* the same for the n_frames - 1 consecutive pairs of a sequence that has been run (VisualOdometer::initialize refines its
 * queued pairs, front-end/visual-odometer.cpp:282-286) */
mvs_status mvs_seq_refine_pairs(mvs_seq *s, const mvs_refine_params *params, double sigma_px);
/* octaves of the keypoints of frames [first, first + count) uploaded with mvs_seq_upload: count x max_kp bytes */
mvs_status mvs_seq_upload_octaves(mvs_seq *s, int first, int count, const uint8_t *octave);
mvs_status mvs_seq_download_refined(mvs_seq *s, mvs_refine_result *refined, double *points_xyz, double *point_cov);

/* Bundle adjustment of sliding windows of a sequence that has been run, assembled on the device from what mvs_seq_run left
 * resident (the bookkeeping VisualOdometer::track does per frame with hash maps,
 * front-end/visual-odometer.cpp:417-445,618-800).  Window w covers frames [w * stride, w * stride + window_frames).
 *   links   an inlier match row of a valid pair k joins keypoint trainIdx of frame k to keypoint queryIdx of frame k + 1; of
 *           several rows with one trainIdx the smallest row is kept, so tracks are simple chains;
 *   points  a track that starts in frames a .. a + F - 2 of the window (at frame a it may come from before), cut at frame
 *           a + F - 1, is a point of the window if one of its links inside the window was triangulated; the first such pair k
 *           gives the guess X = traj_R[k] (pair_scale[k] x) + traj_t[k].  Points are numbered by (first frame, keypoint); the
 *           first max_points are kept;
 *   problem poses = the trajectory, frame a carries params->anchor_sigma, the others pose_sigma, every point the prior
 *           point_sigma^2 I at its guess, an observation the covariance (sigma_px * 2^octave)^2 I.
 * One launch of the window kernel of mvs_ba_refine_windows solves all windows. */
typedef struct mvs_seq_window_params {
    int32_t window_frames;  /* F: 3 .. 8 */
    int32_t stride;         /* >= 1 */
    int32_t max_points;     /* 1 .. 4096: point capacity of one window */
    int32_t reserved;
    double sigma_px;        /* as mvs_batch_refine */
} mvs_seq_window_params;
typedef struct mvs_seq_window_info {
    int32_t first_frame, n_frames, n_points, n_tracks_found;   /* n_points = min(n_tracks_found, max_points) */
} mvs_seq_window_info;
/* W = (n_frames - F) / stride + 1; 0 if the sequence is shorter than a window or window_frames, stride or max_points is out
 * of range (sigma_px is not looked at) */
int mvs_seq_window_count(const mvs_seq *s, const mvs_seq_window_params *wp);
/* Asynchronous on the ctx stream, after mvs_seq_run; the results stay resident until downloaded.  MVS_ERR_INVALID_ARG for
 * window_frames outside 3 .. 8, stride < 1, max_points outside 1 .. 4096, sigma_px <= 0, a sequence that has not been run or
 * that is shorter than one window.
 * Memory: the link tables, the windows' problems and their results live in one block owned by the SEQUENCE (the context's
 * window workspace would be overwritten by the next mvs_ba_refine_windows while these results are resident).  The block only
 * grows and is freed by mvs_seq_destroy; every window owns (8 + 18 F + (9 + 5 F) max_points + 18 max_points) doubles and
 * F max_points int32 of it whatever it holds: about 0.5 GB for 249 windows of F = 8 and max_points = 4096.  A caller with
 * many sequences chooses max_points accordingly. */
mvs_status mvs_seq_refine_windows(mvs_seq *s, const mvs_seq_window_params *wp, const mvs_refine_params *params);
/* Any pointer may be NULL.  info[W], frames[W][F], points[W][max_points][3], point_cov[W][max_points][9],
 * track_kp[W][max_points][F] (keypoint of the point in frame first_frame + f, -1 = not seen), point_guess[W][max_points][3];
 * rows [n_points, max_points) of a window are zero (track_kp: -1).  MVS_NO_MODEL if at least one window has ok = 0, which a
 * window without points has (frames[w * F].ok tells which): the convention of mvs_ba_refine_windows. */
mvs_status mvs_seq_download_windows(mvs_seq *s, mvs_seq_window_info *info, mvs_refine_result *frames, double *points,
                                    double *point_cov, int32_t *track_kp, double *point_guess);

/* ONE bundle adjustment over every frame of a sequence that has been run (mvs_seq_run, mvs_seq_run_essential, and whatever
 * ran after them), assembled on the device from what is resident and solved by the sparse solver of mvs_ba_refine_sparse
 * (DESIGN.md section 4.7.5).  New symbols only: mvs_abi_version stays 4.
 *   links   those of mvs_seq_refine_windows: an inlier row of a valid pair k joins keypoint trainIdx of frame k to keypoint
 *           queryIdx of frame k + 1, the smallest row wins per trainIdx, tracks are simple chains;
 *   depth   of a keypoint: the links behind it (0 where no link arrives);
 *   tracks  a head is a keypoint with a link out of it whose depth is 0 (max_track_frames = 0: uncut) or a multiple of
 *           T = max_track_frames; its track is the chain from the head on, to the chain's end or, cut, over T frames at the most.
 *           Every track has at least two frames and its frames are consecutive;
 *   points  a track is a point if one of its OWN links was triangulated; the first such pair k gives the guess
 *           X = traj_R[k] (pair_scale[k] x) + traj_t[k].  Points are numbered by (head frame, head keypoint); the observations
 *           of a point are stored in frame order: obs_frame[obs_off[p] + s] = head_frame[p] + s;
 *   problem the sequence's camera; poses = the trajectory; frame 0 carries params->anchor_sigma, the others pose_sigma
 *           (variances sigma^2, an entry <= 0 would be no prior); every point the prior point_sigma^2 I at its guess; an
 *           observation the covariance (sigma_px * 2^octave)^2 I.  A frame no point reaches is held by its prior alone. */
typedef struct mvs_seq_global_params {
    int32_t max_track_frames;   /* T: 0 = uncut, or 2 .. 4096 */
    int32_t reserved;
    double sigma_px;            /* as mvs_batch_refine */
} mvs_seq_global_params;
/* Synchronous: the host reads the device's counts once (points, observations, blocks of the envelope, pairs), sizes the
 * workspace, and drives lambda with one synchronisation per iteration as mvs_ba_refine_sparse does; `result` is that call's
 * record.  MVS_ERR_INVALID_ARG: a null pointer, a sequence that has not been run, sigma_px <= 0, max_track_frames outside
 * {0, 2 .. 4096}, refine parameters mvs_ba_refine refuses.  MVS_ERR_CAPACITY, before any solve: more than 4096 frames, or
 * counts beyond the limits of mvs_ba_refine_sparse (2^20 points, 2^23 observations, 2^21 blocks, 2^28 pairs).  MVS_NO_MODEL:
 * no point at all (ok = 0), or the solver's own (ok = 0, as mvs_ba_refine_sparse).  The same input gives the same bytes.
 * Memory: the link tables, the problem, the plan and the results live in two blocks owned by the SEQUENCE, which only grow and
 * are freed by mvs_seq_destroy; they stay resident until the next call or the next run. */
mvs_status mvs_seq_refine_global(mvs_seq *s, const mvs_seq_global_params *gp, const mvs_refine_params *params,
                                 mvs_ba_sparse_result *result);
/* points and observations of the last mvs_seq_refine_global (0 and 0 after a call that found no point) */
mvs_status mvs_seq_global_counts(mvs_seq *s, int32_t *n_points, int32_t *n_obs);
/* Any pointer may be NULL.  poses n_frames x 12, points n_points x 3, pose_cov n_frames x 36, point_cov n_points x 9; the
 * covariance sweep runs at the first call that asks for either.  MVS_NO_MODEL with every output untouched when the last
 * mvs_seq_refine_global ended with ok = 0. */
mvs_status mvs_seq_download_global(mvs_seq *s, double *poses, double *points, double *pose_cov, double *point_cov);
/* mvs_ba_sparse_obs_stats on the resident problem at the resident estimate of the last mvs_seq_refine_global, through device
 * pointers, under the context's loss as it is set at this call: chi2 and weight (may be NULL) hold n_obs of
 * mvs_seq_global_counts, and their bytes are those of mvs_ba_sparse_obs_stats on the downloaded problem and estimate.
 * MVS_ERR_INVALID_ARG unless the last mvs_seq_refine_global on the current run ended with ok = 1.  Waits for the ctx stream. */
mvs_status mvs_seq_global_obs_stats(mvs_seq *s, double *chi2, double *weight);
/* The assembled problem, any pointer may be NULL: obs_off[n_points + 1], obs_frame[n_obs], obs_kp[n_obs] (the keypoint of
 * every observation in its frame), head_frame[n_points], head_kp[n_points], point_guess n_points x 3, obs_uv n_obs x 2. */
mvs_status mvs_seq_download_global_problem(mvs_seq *s, int32_t *obs_off, int32_t *obs_frame, int32_t *obs_kp,
                                           int32_t *head_frame, int32_t *head_kp, double *point_guess, double *obs_uv);

/* The tracking loop of a sequence that has been run: VisualOdometer::track (front-end/visual-odometer.cpp:384-500) with
 * track_pnp (:502-615) and track_refine (:618-800), every frame on the device, no host synchronisation between frames
 * (DESIGN.md section 4.7.2).  Unlike the tracks of mvs_seq_run, which only see their own pair's two-view points, the loop
 * keeps a PERSISTENT MAP of points in the init frame's coordinates and carries every refined point forward.
 *
 * Pair k = (frames k, k + 1).  Point j of a valid pair k (ImagePair::matched_points, image-pair.cpp:159-164) has the match
 * row r_j = point_idx[k][j], the base keypoint a_j = trainIdx (frame k), the new keypoint b_j = queryIdx (frame k + 1) and
 * the position x_j in frame k's camera.  Point j is KEPT iff no j' < j has the same a (the rule of the sliding windows'
 * links, in place of the reference's unordered_map order and its assert at :443).
 *   init    (:326-339) frames < init_pair = k0 are not reached (state 0); frame k0 is INIT at the identity, frame k0 + 1 INIT
 *           at pair k0's pose; map[k0 + 1][b_j] = (id = rank of j among the kept points, x_j).  With use_refined_init pose
 *           and points are those of mvs_seq_refine_pairs.  An invalid pair k0 (with use_refined_init also: one whose
 *           refinement has ok = 0) leaves frame k0 + 1 LOST_PNP and nothing else reached.
 *   step f = k0 + 2 .. n_frames - 1, pair k = f - 1, T_last = (R_l, t_l) the pose of frame f - 1, map[f - 1]:
 *     1 candidates  the kept j with map[f - 1][a_j].id >= 0, ascending j: world point = the map's X, image point =
 *                   (double)kp[f][b_j]                                                                    (:519-555)
 *     2 PnP         mvs_pnp_solve on the candidates, refit included, sampler key pnp->seed + f.  False -- also fewer than 7
 *                   candidates or an invalid pair -- is LOST_PNP
 *     3 scale       sqrt((e0 e0 + e1 e1) + e2 e2), e = t_pnp - t_l: the norm of :584-587 (a rotation does not change it)
 *     4 gate        n_pnp_inliers < min_pnp_point_count is LOST_FEW                                     (:409-415)
 *     5 points      tracked = the PnP inliers in candidate order, positions from the map; new = the kept j without a map entry
 *                   at a_j, ascending j, ids continuing one counter for the whole call, position y = scale x_j,
 *                   X_i = ((R_l[i][0] y0 + R_l[i][1] y1) + R_l[i][2] y2) + t_l[i] (:422-445).  PnP outliers leave the map
 *     6 BA          mvs_ba_refine's two-frame problem, points = tracked then new; frame 0 = frame f - 1 at T_last with
 *                   anchor_var, frame 1 = frame f at the PnP pose with regulator_var; tracked points carry the prior
 *                   point_sigma^2 I at their map position, new points none; frame 0 observes only the new points (at
 *                   kp[f - 1][a_j]: last_frame_vf_idx_to_point_id is filled at :438 only), frame 1 all points (at
 *                   kp[f][b_j]); observation covariance (sigma_px 2^octave)^2 I.  ok = 0 is LOST_BA, error > max_error
 *                   LOST_ERROR (:479-483)
 *     7 commit      T_last = the refined pose of frame 1; map[f][b] = (id, refined point) of every point of the problem,
 *                   every other entry empty (:485-498)
 *     8 a LOST frame ends the run: its record says why, later frames keep state 0 and empty maps, and every later kernel reads
 *       one device word and leaves (the solvers see problems of 0 points).
 * Out of scope HERE: ImagePair::update re-pairing (image-pair.cpp:77-114), check_image_pair (:348-382), reset() and the
 * re-initialisation after a loss (the caller picks init_pair and calls again) -- mvs_seq_odometry below has them.  Out of
 * scope altogether: a C++ VisualOdometer shim. */
typedef struct mvs_vo_params {
    int32_t init_pair;           /* k0: the pair the map is initialised from (frames k0, k0 + 1) */
    int32_t use_refined_init;    /* 1: take pose / points of pair k0 from mvs_seq_refine_pairs' resident results */
    int32_t min_pnp_point_count; /* 7  (visual-odometer.cpp:86-87, used at :409) */
    int32_t reserved;
    double max_error;            /* 0.5 (:77-78, used at :479) */
    double anchor_var[2];        /* last frame's prior, DIAGONAL covariance {rotation, translation}: {1e-3, 1e-3}.  The reference
                                    multiplies the identity by the stddev itself (:684-699), so these are the values, unsquared */
    double regulator_var[2];     /* new frame's prior {1e-2, 1e-2} (same lines) */
    double point_sigma;          /* tracked points' prior point_sigma^2 I, 1e-2 (:728-730); new points have none (:719-725) */
    double sigma_px;             /* observation covariance (sigma_px 2^octave)^2 I, 0.5, as mvs_batch_refine */
} mvs_vo_params;
void mvs_vo_params_default(mvs_vo_params *p);
enum {
    MVS_TRACK_NOT_REACHED = 0, MVS_TRACK_INIT = 1, MVS_TRACK_TRACKED = 2, MVS_TRACK_LOST_PNP = 3, MVS_TRACK_LOST_FEW = 4,
    MVS_TRACK_LOST_BA = 5, MVS_TRACK_LOST_ERROR = 6,
    MVS_TRACK_INITIALIZING = 7   /* mvs_seq_odometry only: processed while initialising, and did not initialise */
};
typedef struct mvs_track_frame {
    int32_t state;          /* MVS_TRACK_* */
    int32_t n_cand;         /* candidates of the join with the map */
    int32_t n_pnp_inliers;
    int32_t n_tracked;      /* points of the BA problem with a prior (= n_pnp_inliers when the step got that far) */
    int32_t n_new;          /* points without one; for frame k0 + 1: the points the map starts with */
    int32_t pnp_best_hyp;   /* -1: fewer than 7 candidates */
    int32_t iterations;     /* of the BA */
    int32_t reserved;
    double scale;
    double error;           /* of the BA */
    double R_pnp[9], t_pnp[3];   /* the PnP pose, camera in init frame */
    double R[9], t[3];           /* the accepted pose (INIT and TRACKED frames), camera in init frame; zero otherwise */
} mvs_track_frame;
/* Asynchronous on the ctx stream, after mvs_seq_run or mvs_seq_run_essential; the results stay resident until the next
 * mvs_seq_track or mvs_seq_run.  Of `refine` only the Levenberg-Marquardt fields are used (the whole struct must be valid).
 * Changes nothing mvs_seq_download_pairs / _tracks / _trajectory / _refined / _windows return.
 * MVS_ERR_INVALID_ARG: a sequence that has not been run, init_pair outside [0, n_frames - 2], sigma_px <= 0,
 * point_sigma <= 0, a variance <= 0, use_refined_init without resident refined pairs -- mvs_seq_refine_pairs must have run
 * since the last mvs_seq_run / mvs_seq_run_essential --, PnP parameters mvs_seq_run refuses.
 * Memory: every per-frame buffer lives in one block owned by the SEQUENCE, which only grows and is freed by mvs_seq_destroy.
 * Frame f owns (14 max_kp + 24) doubles, (7 max_kp + 2) int32, max_kp bytes and about 1.5 KB of records of it -- 141 bytes per
 * keypoint slot --, and the block ends with one step's solver scratch of 61 max_kp doubles and the PnP records: 0.29 GB for
 * 1000 frames of 2048 keypoints. */
mvs_status mvs_seq_track(mvs_seq *s, const mvs_vo_params *vo, const mvs_pnp_params *pnp, const mvs_refine_params *refine);
/* frames[n_frames]; waits for the ctx stream.  MVS_ERR_INVALID_ARG before mvs_seq_track (all three downloads) */
mvs_status mvs_seq_download_track_frames(mvs_seq *s, mvs_track_frame *frames);
/* the map as it stands after `frame`, keyed by that frame's keypoint index: point_id[max_kp] (-1 = none), X[max_kp][3] (zero
 * where there is none).  Either pointer may be NULL */
mvs_status mvs_seq_download_track_map(mvs_seq *s, int frame, int32_t *point_id, double *X);
/* What step `frame` fed its solvers and got back, so that a caller can replay them through mvs_pnp_solve / mvs_ba_refine.
 * Any pointer may be NULL; every array has max_kp rows, rows past the count the frame's record gives are zero; a frame that
 * is no step (or that the run did not reach) gives zeros.
 *   candidates [n_cand]: cand_base_kp (a, frame - 1), cand_new_kp (b, frame), cand_xyz [3], cand_uv [2];
 *   pnp_inlier_idx [n_pnp_inliers]: indices into the candidates, ascending;
 *   BA problem [n_tracked + n_new]: point_id, point_kp [2] = (a, b), point_is_new (also: frame 0 observes the point),
 *   point_guess [3], guess_pose [2][12] = R (9), t (3) of frame - 1 and frame; ba_frames [2]: the solver's records of both
 *   frames, points_refined [3]. */
mvs_status mvs_seq_download_track_step(mvs_seq *s, int frame, int32_t *cand_base_kp, int32_t *cand_new_kp, double *cand_xyz,
                                       double *cand_uv, int32_t *pnp_inlier_idx, int32_t *point_id, int32_t *point_kp,
                                       uint8_t *point_is_new, double *point_guess, double *guess_pose,
                                       mvs_refine_result *ba_frames, double *points_refined);

/* ---- lagged pairs of a resident sequence ---------------------------------------------------------
 * Pair k of lag d = (base = frame k, pair = frame k + d), k < n_frames - d: the view of the frame arrays that the sequence's own
 * pairs (lag 1) are, with the second image's pointers moved d frames on.  What VisualOdometer::initialize matches a new frame
 * against (ImagePair::update, image-pair.cpp:77-114), and what keyframe selection or loop-closure candidates would need.
 * Asynchronous on the ctx stream, after mvs_seq_run or mvs_seq_run_essential.  For every lag d = 2 .. max_lag all n_frames - d
 * pairs go through the pipeline of mvs_batch_run (essential = 0) or mvs_batch_run_essential (essential != 0) and then through
 * mvs_batch_refine with the frames' uploaded octaves and sigma_px; lag 1 is the existing run, for which mvs_seq_refine_pairs is
 * (re)run.  Pair k of every lag uses sampler key offset k (the sequence's global indices), as pair k of an uploaded batch with
 * global_index[k] = k does: the results are those of mvs_batch_run on a batch holding the same frame pairs in order k.
 * match_ssd[k] (per pair, int32, 0 for an invalid pair) = the sum over the pair's triangulated points j of the squared
 * integer Hamming distance of match row point_idx[k][j] (ImagePair::match_inlier_ssd, image-pair.cpp:166), for lag 1 too.
 * After the call every lag 1 .. max_lag has resident results and refined results, until the next mvs_seq_run /
 * mvs_seq_run_essential (a later mvs_seq_refine_pairs replaces lag 1's refined results only).
 * MVS_ERR_INVALID_ARG: a sequence that has not been run, max_lag < 1 or >= n_frames, sigma_px <= 0, invalid refine
 * parameters, two-view parameters mvs_seq_run refuses.
 * Memory: ONE BATCH PER LAG, owned by the sequence, created at the first call that needs the lag and freed by
 * mvs_seq_destroy; only the frame arrays, the intrinsics and the key offsets are shared with the sequence.  Per frame and lag
 * that is 187 bytes per keypoint slot of pipeline state (matches, mask, points, point indices and the triangulation scratch)
 * and 272 of refinement state -- 459 max_kp bytes and about 0.7 KB of records -- plus the RANSAC stage's hypothesis tables,
 * 77 bytes x hypotheses for the 8-point path: 0.94 GB + 0.08 GB per 1000 hypotheses for one lag of 1000 frames of 2048 keypoints. */
mvs_status mvs_seq_run_lags(mvs_seq *s, const mvs_params *two_view, int max_lag, int essential,
                            const mvs_refine_params *refine, double sigma_px);
/* The n_frames - lag pairs of a resident lag (1 .. max_lag of the last mvs_seq_run_lags; MVS_ERR_INVALID_ARG otherwise).  The
 * argument lists follow mvs_seq_download_pairs / mvs_seq_download_refined: all pairs of the lag, n_matches is
 * results[k].n_matches, point_idx is int64; match_ssd[n_frames - lag].  Any pointer but `refined` may be NULL.  Lag 1 returns
 * what mvs_seq_download_pairs / mvs_seq_download_refined return. */
mvs_status mvs_seq_download_lag_pairs(mvs_seq *s, int lag, mvs_pair_result *results, mvs_match *matches, uint8_t *inlier_mask,
                                      double *points_xyz, int64_t *point_idx, int32_t *match_ssd);
mvs_status mvs_seq_download_lag_refined(mvs_seq *s, int lag, mvs_refine_result *refined, double *points_xyz, double *point_cov);

/* ---- VisualOdometer::add_frame over a resident sequence (front-end/visual-odometer.cpp:129-382) ----
 * The state machine around the tracking loop above: initialisation from the frame queue with ImagePair::update re-pairing,
 * check_image_pair, and reset() + re-initialisation after a loss, every frame on the device, no host synchronisation between
 * frames.  vo->init_pair and vo->use_refined_init are ignored (initialize() always refines, :282-286); vo->max_error is also
 * the initialisation's error gate (the reference uses one value at :363 and :479).  Q = frame_queue_size.
 *
 * Device state: mode; q0, the oldest frame still queued; held[b] for every queued base frame b = (pair frame, lag, valid,
 * count = n_points, ssd = match_ssd, error, refined).  At the start mode = INITIALIZING, q0 = 0, segment = -1; frame 0 stays
 * NOT_REACHED until a pair with base 0 initialises.
 * Frame f = 1 .. n_frames - 1.  The frame is pushed before it is processed (:138) and the oldest is popped afterwards if the
 * queue then holds more than Q (:181-190): while f is processed the queue holds frames max(q0, f - Q) .. f, so the largest lag
 * is Q, and afterwards q0 = max(q0, f - Q + 1).
 *   TRACKING      steps 1-7 of mvs_seq_track on pair k = f - 1, PnP sampler key seed + f.  A LOST_* verdict does not end the
 *                 run: it is reset() (:203-217): mode = INITIALIZING, q0 = f (the lost frame is kept), the held pairs are
 *                 dropped.  The lost frame's record keeps its LOST_* state and carries no pose.
 *   INITIALIZING  held[f - 1] = (f, lag 1, validity / count / ssd of pair f - 1, error = +inf, not refined); count and ssd of
 *                 an invalid pair are 0.
 *     1 refine    a valid newest pair takes validity and error from its resident refined result (ok = 0: invalid, error +inf)
 *     2 update    every queued b < f - 1, oldest first: ImagePair::update (mvslam_compat.hpp:1034-1051) with the lagged pair
 *                 (b, f).  The candidate must be valid, must not have count < held[b].count nor ssd < held[b].ssd, and
 *                 replaces held[b] only if its refined error is < held[b].error (a failed refinement counts as +inf).  As in
 *                 the shim an INVALID held pair (count 0, ssd 0, error +inf) can be replaced; the reference starts ssd at
 *                 (uint32)-1 and adds a float into it, which is out of range for the conversion back, so its behaviour there
 *                 is undefined and the shim's is kept.
 *     3 choice    the queue is scanned oldest first (:315-345); the first held[b] that passes check_image_pair AND whose pair
 *                 frame is f (the reference asserts that at :327) initialises.  Gates in the order of :353-379: valid;
 *                 count >= min_match_inlier_count; error <= max_error; rot_sq <= max_rotation_magnitude^2 with rot_sq =
 *                 (w0 w0 + w1 w1) + w2 w2, w = SO3::ln of the refined rotation in the shim's operation order
 *                 (mvslam_compat.hpp:176-184); abs_tz = |t[2]| <= max_translation_z.
 *                 Initialising is mvs_seq_track's init with the refined pose and points of that lagged pair: frame b INIT at
 *                 the identity (a base frame that is the lost frame of the segment before keeps its LOST_* record; its pose
 *                 in the new segment is the identity), frame f INIT at the refined pose, map[f][b_j] = (id, refined x_j) over
 *                 the kept points, ids continuing the call's one counter; segment += 1, mode = TRACKING.  Frames between b
 *                 and f keep MVS_TRACK_INITIALIZING.
 *     4 otherwise frame f is MVS_TRACK_INITIALIZING.
 * The per-frame records, maps and steps are mvs_seq_track's: mvs_seq_download_track_frames / _track_map / _track_step serve
 * an odometry run as they serve a tracking run, and the run lives in the same block of the sequence (plus 72 bytes per frame).
 * Asynchronous on the ctx stream.  MVS_ERR_INVALID_ARG: what mvs_seq_track refuses except the init_pair and use_refined_init
 * conditions; frame_queue_size < 2; min_match_inlier_count < 0; a negative (or NaN) gate; lags 1 .. min(Q, n_frames - 1) not
 * all resident from one mvs_seq_run_lags since the last mvs_seq_run / mvs_seq_run_essential. */
typedef struct mvs_vo_init_params {
    int32_t frame_queue_size;        /* 10  (visual-odometer.cpp:71-72)  */
    int32_t min_match_inlier_count;  /* 20  (:74-75, used at :358)       */
    double  max_rotation_magnitude;  /* 0.1 (:80-81, used at :368-369)   */
    double  max_translation_z;       /* 0.1 (:83-84, used at :374-375)   */
} mvs_vo_init_params;                /* max_error is mvs_vo_params.max_error */
void mvs_vo_init_params_default(mvs_vo_init_params *p);
typedef struct mvs_odo_frame {
    int32_t mode_after;     /* 0 INITIALIZING, 1 TRACKING: the state add_frame leaves behind */
    int32_t segment;        /* -1 before the first initialisation; counts initialisations from 0 */
    int32_t init_base;      /* for a frame that initialised: the base frame b of the chosen pair (b, f); -1 otherwise */
    int32_t queue_first;    /* oldest frame in the queue when this frame was processed */
    int32_t n_updated;      /* queue entries this frame's ImagePair::update replaced */
    int32_t gate_fail;      /* for the NEWEST pair (f-1, f) when nothing initialised: 0 passed / not looked at, 1 invalid,
                               2 inliers, 3 error, 4 rotation, 5 translation z  (the order of :353-379) */
    double  rot_sq, abs_tz; /* of the chosen pair, or of the newest pair when none was chosen (0 for an invalid pair and for a
                               frame processed while tracking) */
} mvs_odo_frame;
mvs_status mvs_seq_odometry(mvs_seq *s, const mvs_vo_params *vo, const mvs_vo_init_params *init,
                            const mvs_pnp_params *pnp, const mvs_refine_params *refine);
/* odo[n_frames]; waits for the ctx stream.  MVS_ERR_INVALID_ARG unless the sequence's last tracking call was mvs_seq_odometry */
mvs_status mvs_seq_download_odometry_frames(mvs_seq *s, mvs_odo_frame *odo);

/* ---------------------------------------------------------------------------------------------------------------
 * Row f3: keypoint + descriptor extraction.  Replaces VisualFeature::extract
 * (vision/visual-feature.cpp:40-49, decl visual-feature.hpp:16-20) = cv::ORB::create(500)->detect + compute
 * (visual-feature.cpp:12-17).  cv::ORB is OpenCV-internal and its learned sampling pattern is not in the reference
 * tree: this is ORB's published pipeline with the reference's parameters and the library's own fully specified
 * resize / blur / ranking / pattern -- keypoints and descriptors are NOT bit-identical to
 * OpenCV's, they are bit-identical to the CPU oracle's. */
typedef struct mvs_orb_params {
    int32_t nfeatures;       /* 500 = MAX_FEATURE_COUNT (visual-feature.cpp:9) */
    int32_t nlevels;         /* 8, scale factor 1.2 (cv::ORB::create defaults) */
    int32_t edge_threshold;  /* 31 */
    int32_t fast_threshold;  /* 20 */
} mvs_orb_params;
typedef struct mvs_keypoint { /* layout of cv::KeyPoint (base/image.hpp:37-48 DetectorResultType element) */
    float x, y, size, angle, response;
    int32_t octave, class_id;
} mvs_keypoint;
void mvs_orb_params_default(mvs_orb_params *p);
/* images: n_images x height x width grayscale (CV_8UC1, continuous), host.  keypoints: n_images x nfeatures,
 * descriptors: n_images x nfeatures x 32, n_keypoints: n_images (rows [0, n_keypoints[i]) are valid; ordered by
 * pyramid level, then response descending).  MVS_ERR_CAPACITY if the image is larger than 65535 in a dimension, or -- only
 * when a level's quota exceeds 8192 features (the selection holds 2 n_l <= 16384 keys in LDS) -- if that level has more than
 * 16384 corners; otherwise a level's candidate list holds every corner the non-maximum suppression can leave (round 5). */
mvs_status mvs_extract(mvs_ctx *ctx, const uint8_t *images, int n_images, int width, int height,
                       const mvs_orb_params *params, mvs_keypoint *keypoints, uint8_t *descriptors,
                       int32_t *n_keypoints);
/* Kernel time of the extraction: replays the launches of the LAST mvs_extract / mvs_seq_upload_images on this context
 * (its captured graph; the workspace still holds that call's images) `steps` times between HIP events on the ctx stream.
 * No transfers are inside the measurement.  MVS_ERR_INVALID_ARG before the first extraction. */
mvs_status mvs_extract_time(mvs_ctx *ctx, int steps, float *ms_total);
/* Extraction straight into a sequence's resident frame arrays (no host round trip of descriptors): frames
 * [first, first + count) of `s` get up to max_kp keypoints each (params->nfeatures is overridden by max_kp). */
mvs_status mvs_seq_upload_images(mvs_seq *s, int first, int count, const uint8_t *images, int width, int height,
                                 const mvs_orb_params *params, const double K[9]);

/* Scale propagation and trajectory of a sequence that has been run (the last stage of mvs_seq_run; row f2,
 * front-end/visual-odometer.cpp:422-445,577-588).  Pair k has a unit baseline; track q is in pair q's scale;
 *   track_scale[q] = |(pair_q^-1 o track_q).t| = baseline(pair q+1) / baseline(pair q)      (n_frames - 2 entries)
 *   pair_scale[k]  = prod_{j<k} track_scale[j] = pair k's baseline in units of pair 0's      (n_frames - 1 entries)
 *   R / t          = pose of frame k in frame 0: G_0 = I, G_1 = pair 0, G_{q+2} = G_q o (R_track_q, pair_scale[q] t_track_q)
 * (a failed track keeps the scale and falls back to the two-view pose of pair q+1).  Any pointer may be NULL. */
mvs_status mvs_seq_download_trajectory(mvs_seq *s, double *R, double *t, double *pair_scale, double *track_scale);

/* The scale of a sequence that has been run, again, by another rule.  mvs_seq_run keeps the rule
 * above; mvs_seq_rescale overwrites the resident R / t / pair_scale / track_scale, which mvs_seq_download_trajectory then
 * returns, and retires what was derived from the old trajectory as a new run does: window results, the pose graph and its
 * optimised nodes, the global problem.  Pairs, tracks, refined pairs, lags, tracking and odometry stay valid.
 *   MVS_SEQ_SCALE_CHAIN        the fold of mvs_seq_run again: the bytes it left; the step records are zero.
 *   MVS_SEQ_SCALE_DEPTH_RATIO  step q = 0 .. n_frames - 3, from pairs q and q + 1.  Point j of a valid pair k: match row
 *     point_idx[k][j], base keypoint a = trainIdx, new keypoint b = queryIdx, position x in frame k's camera (a row or a
 *     keypoint outside the frame arrays: no point).  Keypoint c of frame q + 1 is SHARED when a point j of pair q has b = c
 *     and a point j' of pair q + 1 has a = c; of several j' with a = c the smallest counts.  Shared points in ascending j';
 *     with (R, t) of pair q and d = x_j - t:   z_a = (R[0][2] d0 + R[1][2] d1) + R[2][2] d2,   z_b = x_j'[2];
 *     the point is USED when both are finite and > 0, and then rho = z_a / z_b.  n_common / n_used count the shared / used
 *     points; scale = the lower median of the used rho (element (n_used - 1) / 2 in ascending order).  flag 1: pair q or
 *     q + 1 is invalid (no points: both counts 0); flag 2: n_used < min_common; both: scale = 1.  flag 0 otherwise.
 *     track_scale[q] = scale_q;  pair_scale[0] = 1, pair_scale[q+1] = pair_scale[q] * scale_q, in this order;
 *     G_0 = I, G_{k+1} = G_k o (R_k, pair_scale[k] t_k) from the pairs alone (an invalid pair: the identity; the PnP tracks
 *     are not read), composed as above: s = pair_scale[k] t_k first, then (A0 c0 + A1 c1) + A2 c2 (+ A.t).
 * Binary64, + - * / with one rounding each, no atomics on values: the same pairs give the same bytes.
 * Asynchronous on the ctx stream.  MVS_ERR_INVALID_ARG, nothing touched: a null pointer, a sequence that has not been run, a
 * rule that is neither of the two, min_common < 1. */
#define MVS_SEQ_SCALE_CHAIN 0
#define MVS_SEQ_SCALE_DEPTH_RATIO 1
typedef struct mvs_seq_scale_params {
    int32_t rule;        /* MVS_SEQ_SCALE_CHAIN, MVS_SEQ_SCALE_DEPTH_RATIO */
    int32_t min_common;  /* >= 1; below it a step keeps the scale */
} mvs_seq_scale_params;
typedef struct mvs_seq_scale_step {
    int32_t n_common, n_used, flag, reserved;
    double scale;
} mvs_seq_scale_step;
mvs_status mvs_seq_rescale(mvs_seq *s, const mvs_seq_scale_params *p);
/* steps[n_frames - 2] of the last mvs_seq_rescale on the current run; waits for the ctx stream.  MVS_ERR_INVALID_ARG before it. */
mvs_status mvs_seq_download_scale_steps(mvs_seq *s, mvs_seq_scale_step *steps);

/* ---------------------------------------------------------------------------------------------------------------
 * The back end: pose graphs.  Replaces Graph / GraphOptimizer of back-end/graph.{hpp,cpp}, i.e. GTSAM's
 * LevenbergMarquardtOptimizer over Pose3 values, BetweenFactor<Pose3> edges with full 6 x 6 covariances and one prior that
 * anchors a node at its initial value.  The library minimises
 *   1/2 [ |e_anchor|^2_Sa + sum_k |e_k|^2_Sk ],   Sa = diag(sigma_rot^2 I3, sigma_trans^2 I3),
 *   e_k = ( Log(Rz^T Rs^T Rd),  Rz^T (Rs^T (td - ts) - tz) )     for edge k = (s, d, Z = (Rz, tz)): Z measures Xs^-1 Xd,
 * tangent order (rotation, translation), right perturbation R <- R Exp(dw), t <- t + R dv, with the Levenberg-Marquardt
 * rule of the refinement (the LM fields of mvs_refine_params).  Graphs of up to 16 nodes are solved by one workgroup with
 * a dense Cholesky in LDS (a batch of them is one launch); up to 4096 nodes and 65536 edges by a block-Jacobi
 * preconditioned conjugate gradient, one host synchronisation per LM iteration (more with cg_chunk_iterations).  Binary64, fixed reduction orders: the
 * same input gives the same bytes.  DESIGN.md section 4.10. */
typedef struct mvs_pose_graph {            /* all host pointers */
    int32_t n_nodes, n_edges;
    const double *node_pose;               /* n_nodes x 12: initial values, R row-major (9) then t (3) */
    const int32_t *edge_src, *edge_dst;    /* n_edges */
    const double *edge_pose;               /* n_edges x 12: Z */
    const double *edge_cov;                /* n_edges x 36: row-major 6 x 6, order (rotation, translation) */
    int32_t anchor_node;                   /* the reference: the origin */
} mvs_pose_graph;
typedef struct mvs_pose_graph_params {
    mvs_refine_params lm;                  /* only the LM fields: max_iterations, lambda_*, rel_tol, abs_tol */
    double anchor_sigma[2];                /* rotation, translation: 1e-4, 1e-4 (graph.cpp GRAPH_ANCHOR_STDDEV) */
    double cg_rel_tol;                     /* 1e-10: the linear solve of the large path stops at |r| <= cg_rel_tol |g| ... */
    int32_t cg_max_iterations;             /* ... or after this many iterations; 0 = 6 n_nodes */
    int32_t cg_chunk_iterations;           /* large path: 0 (the default; anything <= 0) enqueues the whole CG budget of an LM
                                              iteration at once; c > 0 enqueues c iterations, reads the 64-byte status and goes
                                              on only while the solve is neither converged nor broken.  The same kernels with
                                              the same arguments: every output byte and result field equals those at 0.
                                              Recommended: 64 (1000 nodes, 2030 edges: 1.08 s instead of 2.34 s; 16 and 256
                                              are within 3 % of it; profiles/seq_pose_graph_latency.json) */
} mvs_pose_graph_params;
typedef struct mvs_pose_graph_result {
    int32_t ok;              /* 1: converged or stopped by the iteration / lambda limits with a finite error */
    int32_t iterations;      /* linear solves attempted (LM iterations) */
    int32_t cg_iterations;   /* conjugate-gradient iterations over all of them (0 on the dense path) */
    int32_t rejected_steps;  /* LM iterations whose candidate was not accepted */
    double error_initial;    /* 1/2 sum of squared Mahalanobis residuals at the initial values ... */
    double error;            /* ... and at the estimate */
} mvs_pose_graph_result;
void mvs_pose_graph_params_default(mvs_pose_graph_params *p);
/* poses_out: n_nodes x 12.  MVS_ERR_INVALID_ARG (null pointers, indices out of range, src == dst, non-finite input) and
 * MVS_ERR_CAPACITY (more than 4096 nodes or 65536 edges) are returned before anything runs.  MVS_NO_MODEL with ok = 0 and
 * poses_out untouched: a covariance that is not positive definite, a node no path of edges joins to the anchor, or finite
 * input whose cost at the initial values is not finite; every other field of the result is then zero. */
mvs_status mvs_pose_graph_optimize(mvs_ctx *ctx, const mvs_pose_graph *graph, const mvs_pose_graph_params *params,
                                   mvs_pose_graph_result *result, double *poses_out);
/* n_graphs graphs; graph i's poses at poses_out + i * 12 * (largest n_nodes of the batch), rows beyond its own node count
 * are not written.  Graphs of up to 16 nodes share one launch, larger ones run one after another; every graph gets the
 * bytes the single call returns for it.  MVS_NO_MODEL if some graph failed (results[i].ok tells which). */
mvs_status mvs_pose_graph_optimize_batch(mvs_ctx *ctx, const mvs_pose_graph *graphs, int n_graphs,
                                         const mvs_pose_graph_params *params, mvs_pose_graph_result *results,
                                         double *poses_out);

/* ---- The linear solver of the large path -------------------------------------------------------
 * A switch of the context, MVS_PG_SOLVER_PCG by default: with it every call returns the bytes it returned before the switch
 * existed.  Any other value than the two below: MVS_ERR_INVALID_ARG, the setting stays.  With MVS_PG_SOLVER_DIRECT graphs of
 * more than 16 nodes in mvs_pose_graph_optimize, mvs_pose_graph_optimize_batch and mvs_seq_optimize_pose_graph solve every
 * LM step exactly; graphs of up to 16 nodes take the dense path and return the same bytes under either setting.  One step at
 * the current poses X and damping lambda, with the optimiser's own residuals, Jacobians, whitening and anchor term:
 *   1. A = H + lambda I as a block lower triangle inside its envelope (row i holds the blocks first[i] .. i, first[i] the
 *      smallest of i and its neighbours, nodes in their natural order) and the gradient g; every block's terms are summed in
 *      edge order, the anchor's last.
 *   2. A_ii = C_i C_i^T (a 6 x 6 Cholesky);  A~_ij = C_i^-1 A_ij C_j^-T off the diagonal, A~_ii = I exactly, b~_i = -C_i^-1 g_i.
 *   3. A~ = L L^T in the skyline; fill stays inside a row's envelope.
 *   4. L y = b~, then L^T z = y with the rows in descending order: row i finishes z_i, then subtracts L(i, c)^T z_i from y_c
 *      for every c of its envelope.
 *   5. delta_i = C_i^-T z_i; retraction and candidate cost as under PCG.
 * A pivot that is not finite and positive, in step 2 or 3, is a failed solve: the step is rejected, lambda is multiplied by
 * lambda_factor and no stall test is made; the rest of the LM rule is unchanged.  The block scaling is what the PCG's
 * block-Jacobi preconditioner does implicitly; without it H of a long monocular sequence is not positive definite in binary64.
 * Binary64, explicit FMAs, fixed summation orders, no floating-point atomics: the same input gives the same bytes.  One host
 * synchronisation and a constant number of launches per LM iteration.
 * cg_rel_tol, cg_max_iterations and cg_chunk_iterations are ignored and cg_iterations is 0.  Argument, topology and covariance
 * errors are those of the PCG path, with the same status codes and the same "poses_out untouched, result zero".  One more
 * refusal: an envelope of more than 2^21 blocks (the limit of mvs_pose_graph_marginals) is MVS_ERR_CAPACITY, reported for a
 * graph of more than 16 nodes before anything is launched.  There is no fill-reducing ordering: a 4096-node hub (8.4 million
 * blocks) optimises under PCG and is refused under DIRECT. */
#define MVS_PG_SOLVER_PCG 0
#define MVS_PG_SOLVER_DIRECT 1
mvs_status mvs_ctx_set_pose_graph_solver(mvs_ctx *ctx, int solver);
/* What the direct solver met in the context's last graph that went through it (MVS_ERR_INVALID_ARG before there is one). */
typedef struct mvs_pose_graph_direct_info {
    int32_t envelope_blocks;   /* sum_i (i - first[i] + 1) */
    int32_t widest_row;        /* max_i (i - first[i] + 1) */
    int32_t failed_solves;     /* LM iterations whose solve failed on a pivot */
    int32_t bad_node;          /* the node of the first such pivot, -1 if there was none */
    double min_pivot;          /* the smallest diagonal entry of L over the call's completed factorisations of the scaled
                                  matrix (1 = a node nothing couples), 0 if none completed */
    double failed_pivot;       /* the first failed pivot of the skyline, before its square root (<= 0 or not finite); 0 if
                                  there was none or a diagonal block of H + lambda I failed */
} mvs_pose_graph_direct_info;
mvs_status mvs_ctx_pose_graph_direct_info(mvs_ctx *ctx, mvs_pose_graph_direct_info *info);

/* ---- The pose graph of a resident sequence: what feeds the back end ---------------------------
 * Built on the device from what the sequence calls left resident, optimised there, no pose or covariance on the host in
 * between.
 *   Nodes       node k = frame k, k = 0 .. n_frames - 1, initial value G_k = (R_k, t_k) of mvs_seq_download_trajectory.  The
 *               anchor is node 0.
 *   Candidates  one per lag d = 1 .. max_lag and base k < n_frames - d: source k, destination k + d, measured by r =
 *               refined[d][k] of mvs_seq_run_lags (pose2in1 of frame k + d in frame k = Xs^-1 Xd of an edge).
 *   Acceptance  the pair is valid and r.ok; n_points >= min_points; r.error <= max_error; the scale s is finite and > 0; the
 *               scaled covariance is positive definite by the solver's own 6 x 6 Cholesky test (on its lower triangle).  A
 *               candidate that fails is dropped; it does not fail the graph.
 *   Scale       a monocular pair has no metric scale, the trajectory supplies it.  D = t_{k+d} - t_k,
 *               q_i = (R_k[0][i] D0 + R_k[1][i] D1) + R_k[2][i] D2,  s = sqrt((q0 q0 + q1 q1) + q2 q2) / sqrt((u0 u0 + u1 u1) +
 *               u2 u2) with u = r.t;  Z = (r.R, (s u0, s u1, s u2)).
 *   Covariance  S' = D S D, D = diag(1, 1, 1, s, s, s), every entry (f_i S_ij) f_j: under the right perturbation t + R dv a
 *               translation scaled by s scales dv by s.
 *   Fallback    where slot (1, k) yields no edge and both chain_sigma > 0: the edge (k, k + 1) with
 *               Z = G_k^-1 G_{k+1} = (R_k^T R_{k+1}, q) -- R_Z[i][j] = (R_k[0][i] R_{k+1}[0][j] + R_k[1][i] R_{k+1}[1][j]) +
 *               R_k[2][i] R_{k+1}[2][j], q as above at d = 1 -- and S = diag(chain_sigma[0]^2 I, chain_sigma[1]^2 I); kind 1,
 *               scale 1.  Without it a node no path joins to node 0 makes the optimisation MVS_NO_MODEL.
 *   Order       ascending (d, k); a fallback sits in slot (1, k).  Part of the contract: the solver sums in edge order.
 * Plain binary64 multiplies and adds in exactly the order written, no fused operation: tests/seq_graph_model.py reproduces
 * every byte. */
typedef struct mvs_seq_graph_params {
    int32_t max_lag;        /* 1 .. the lags resident from the last mvs_seq_run_lags */
    int32_t min_points;     /* 0 = no gate */
    double  max_error;      /* gate on the refined error; 1e30 = open */
    double  chain_sigma[2]; /* rotation, translation of the fallback edge; <= 0: none */
} mvs_seq_graph_params;
/* Asynchronous on the ctx stream.  MVS_ERR_INVALID_ARG: max_lag < 1 or >= n_frames, min_points < 0, a negative or NaN
 * max_error, a NaN chain_sigma; a sequence not run, or lags 1 .. max_lag not all resident from one mvs_seq_run_lags since the
 * last run.  MVS_ERR_CAPACITY (a matter of n_frames and max_lag alone, reported before the sequence's state is looked at):
 * more than 4096 frames or more than 65536 candidate slots.  The graph lives in a block of the sequence that only grows and
 * stays until the next mvs_seq_run / _run_essential / _run_lags. */
mvs_status mvs_seq_build_pose_graph(mvs_seq *s, const mvs_seq_graph_params *p);
/* mvs_pose_graph_optimize on the resident graph: up to 16 frames through the dense path, more through the large path; result
 * and optimised nodes are, byte for byte, those of mvs_pose_graph_optimize on the downloaded graph with anchor_node 0.  Only
 * the edges' endpoints and their count come to the host (connectivity, the incidence list).  Waits for the ctx stream.
 * MVS_NO_MODEL as there (the result is then zero and the resident optimised nodes are not written);
 * MVS_ERR_INVALID_ARG before mvs_seq_build_pose_graph or for parameters mvs_pose_graph_optimize refuses. */
mvs_status mvs_seq_optimize_pose_graph(mvs_seq *s, const mvs_pose_graph_params *p, mvs_pose_graph_result *result);
/* The resident graph: *n_edges = E, node_pose n_frames x 12, and the first E rows of edge_src / edge_dst / edge_lag /
 * edge_kind (0 measured, 1 fallback, 2 loop closure) / edge_scale (E), edge_pose (E x 12), edge_cov (E x 36).  Every array
 * must hold the candidate slot count max_lag n_frames - max_lag (max_lag + 1) / 2 of the build -- after a successful
 * mvs_seq_add_loop_edges that slot count PLUS the max_candidates of the selection whose edges that call added (a later
 * mvs_seq_select_loops does not change the graph, nor what its download needs) --; any pointer but n_edges may be NULL.
 * MVS_ERR_INVALID_ARG before mvs_seq_build_pose_graph. */
mvs_status mvs_seq_download_pose_graph(mvs_seq *s, int32_t *n_edges, double *node_pose, int32_t *edge_src, int32_t *edge_dst,
                                       double *edge_pose, double *edge_cov, int32_t *edge_lag, int32_t *edge_kind, double *edge_scale);
/* poses: n_frames x 12, the optimised nodes.  MVS_ERR_INVALID_ARG unless the last mvs_seq_optimize_pose_graph on the current
 * graph succeeded. */
mvs_status mvs_seq_download_pose_graph_poses(mvs_seq *s, double *poses);

/* ---- Marginal covariances of a pose graph ---------------------------------------------------------
 * Inputs: a graph g as above, poses X (n_nodes x 12, the linearisation point; NULL: g.node_pose) and anchor_sigma.
 *   H = J_a^T W_a J_a + sum_k J_k^T W_k J_k,  no lambda.
 * Residuals, Jacobians, tangent order (rotation, translation), right perturbation and whitening are exactly those of the
 * optimiser.  The anchor's mean is g.node_pose[anchor_node], as there; J_a is evaluated at X[anchor_node].  Sigma = H^-1.
 * The call returns the 6 x 6 blocks Sigma_ij, row-major, of a list of queries (i, j): i = j is the marginal covariance of node
 * i, i != j the cross-covariance.
 *   - A diagonal block is returned exactly symmetric.
 *   - The bytes of Sigma_ji are the transpose of the bytes of Sigma_ij.
 *   - A block's bytes do not depend on which other queries are in the call or on their order.
 *   - The same input gives the same bytes: binary64, explicit FMAs, fixed summation orders, no floating-point atomics.
 * How: H is assembled as a block lower triangle inside its envelope (nodes in their natural order; row i stores the blocks
 * first[i] .. i, first[i] = the smallest of i and its neighbours), factorised there (H = L L^T, one workgroup, fill never leaves
 * a row's envelope) and Sigma_ij = (L^-1 E_i)^T (L^-1 E_j) comes from forward solves alone, one workgroup per query.
 * envelope_blocks = sum_i (i - first[i] + 1); more than 2^21 blocks (604 MB) is MVS_ERR_CAPACITY, reported before anything is
 * launched.  One path for 1 .. 4096 nodes. */
typedef struct mvs_pose_graph_marginals_info {
    int32_t ok;               /* 1: factorised, every block written */
    int32_t envelope_blocks;  /* 6 x 6 blocks stored for L */
    int32_t bad_node;         /* node whose pivot failed, -1 otherwise */
    int32_t reserved;
    double  min_pivot;        /* smallest diagonal entry of L */
} mvs_pose_graph_marginals_info;
/* cov_out: n_query x 36.  n_query = 0 with both lists NULL: every diagonal block, cov_out n_nodes x 36.  Argument, capacity and
 * topology errors are those of mvs_pose_graph_optimize with the same status codes; a query index out of range, a list that is
 * missing, non-finite poses or an anchor_sigma that is not positive are MVS_ERR_INVALID_ARG.  MVS_NO_MODEL with ok = 0 and cov_out
 * untouched: an edge covariance that is not positive definite, a node no path of edges joins to the anchor, or a pivot of the
 * factorisation that is not finite and positive (bad_node tells where).  Waits for the ctx stream. */
mvs_status mvs_pose_graph_marginals(mvs_ctx *ctx, const mvs_pose_graph *graph, const double *poses /* NULL: node_pose */,
                                    const double anchor_sigma[2], int n_query, const int32_t *query_i,
                                    const int32_t *query_j, double *cov_out /* n x 36 */,
                                    mvs_pose_graph_marginals_info *info);
/* The same on the resident graph of a sequence (loop edges included) at its resident OPTIMISED nodes, read through device
 * pointers: only the edges' endpoints go to the host and only the blocks come back.  The bytes are those of
 * mvs_pose_graph_marginals on mvs_seq_download_pose_graph plus mvs_seq_download_pose_graph_poses with anchor_node 0.
 * MVS_ERR_INVALID_ARG unless the last mvs_seq_optimize_pose_graph on the current graph succeeded. */
mvs_status mvs_seq_pose_graph_marginals(mvs_seq *s, const double anchor_sigma[2], int n_query, const int32_t *query_i,
                                        const int32_t *query_j, double *cov_out, mvs_pose_graph_marginals_info *info);

/* ---- Robust edge losses and per-edge residuals --------------------------------------------------
 * A switch of the context, MVS_PG_LOSS_NONE by default: with it every call returns the bytes it returned before the switch
 * existed.  With s_k = |r_k|^2, the squared norm of edge k's whitened residual, the optimiser's cost becomes
 *   1/2 [ |e_anchor|^2 + sum_{k < first_edge} s_k + sum_{k >= first_edge} rho2(s_k) ],   x = sqrt(s):
 *     MVS_PG_LOSS_NONE    rho2 = s                                    w = 1
 *     MVS_PG_LOSS_HUBER   rho2 = s if x <= k, else (2 k) x - k k      w = 1 if x <= k, else k / x
 *     MVS_PG_LOSS_CAUCHY  rho2 = (k k) log1p(s / (k k))               w = (k k) / (k k + s)
 * (GTSAM's mEstimator::Huber and mEstimator::Cauchy, in this library's "twice the cost" convention).  The linearisation is
 * iteratively reweighted least squares, as GTSAM's: a robustified edge enters H and g as sqrt(w) r, sqrt(w) A_src and
 * sqrt(w) A_dst, nothing else changes.  The anchor is never robustified.  The LM rule, its exits, error and error_initial are
 * those of mvs_pose_graph_optimize on the cost above: a candidate is accepted when its ROBUST cost is not above the current one.
 * Order of operations, part of the contract: s by the optimiser's fused sum of squares; x = sqrt(s); one division for w (Cauchy's
 * cost: log1p of one quotient); sqrt(w); each of the 78 doubles of the linearised edge multiplied once by sqrt(w).  Binary64, no
 * further fused operation, no atomics: the same input gives the same bytes.
 * first_edge: the edges with index >= first_edge inside their graph (of a batch: inside each graph) get the loss; 0 = all.
 * MVS_PG_LOSS_LOOP_EDGES stands, in mvs_seq_optimize_pose_graph and mvs_seq_pose_graph_edge_stats, for the number of edges the
 * resident graph had before mvs_seq_add_loop_edges: exactly its edges of kind 2 get the loss (none added: no edge does, and the
 * bytes are those of MVS_PG_LOSS_NONE).  The calls on a host graph refuse it with MVS_ERR_INVALID_ARG before anything runs.
 * MVS_ERR_INVALID_ARG, the setting stays: a loss that is none of the three; with a loss other than NONE a k that is not finite
 * and > 0; first_edge < -1.  The setting holds for mvs_pose_graph_optimize, mvs_pose_graph_optimize_batch and
 * mvs_seq_optimize_pose_graph on every path (dense, PCG, direct).  mvs_pose_graph_marginals and mvs_seq_pose_graph_marginals
 * IGNORE it: their H is the Gaussian one, whatever loss the poses were optimised under. */
#define MVS_PG_LOSS_NONE 0
#define MVS_PG_LOSS_HUBER 1
#define MVS_PG_LOSS_CAUCHY 2
#define MVS_PG_LOSS_LOOP_EDGES (-1)
mvs_status mvs_ctx_set_pose_graph_loss(mvs_ctx *ctx, int loss, double k, int32_t first_edge);
/* chi2[k] = s_k at `poses` (n_nodes x 12; NULL: graph->node_pose) for every edge, and, with weight != NULL, weight[k] = w(s_k)
 * under the context's current loss, 1 for the edges below first_edge: what tells a caller which edge the loss turned down.  Both
 * arrays hold n_edges doubles.  Argument, capacity, topology and covariance errors are those of mvs_pose_graph_optimize with its
 * status codes (MVS_NO_MODEL: a node no path joins to the anchor, a covariance that is not positive definite; nothing is
 * written then); non-finite poses and MVS_PG_LOSS_LOOP_EDGES are MVS_ERR_INVALID_ARG.  Waits for the ctx stream. */
mvs_status mvs_pose_graph_edge_stats(mvs_ctx *ctx, const mvs_pose_graph *graph, const double *poses /* NULL: node_pose */,
                                     double *chi2 /* n_edges: s_k */, double *weight /* n_edges, may be NULL */);
/* The same on the resident graph of a sequence at its resident OPTIMISED nodes, through device pointers; the arrays hold what
 * mvs_seq_download_pose_graph's hold.  The bytes are those of mvs_pose_graph_edge_stats on the downloaded graph and poses (with
 * first_edge resolved as above).  MVS_ERR_INVALID_ARG unless the last mvs_seq_optimize_pose_graph on the current graph
 * succeeded. */
mvs_status mvs_seq_pose_graph_edge_stats(mvs_seq *s, double *chi2, double *weight);

/* ---- Pose graphs over Sim(3) -----------------------------------------------------------------------
 * The same graph with one more degree of freedom per node: every node carries a scale.  A monocular sequence fixes every edge's
 * length from its (drifted) trajectory, so an SE(3) graph can bend a trajectory and cannot change the scale drift along it; with
 * a scale per node, sequential edges say "my neighbour has my scale, to within sigma" and a loop's position constraint
 * redistributes scale around the loop (Strasdat et al. 2010).  The reference has no counterpart; the contract is the library's
 * own and tests/sim3graph_model.py restates it in numpy.
 *   Node      X = (R, t, s), 13 doubles: R row-major (9), t (3), s > 0.  It maps local to world by x_w = s R x + t.
 *   Relative  Xs^-1 Xd = (Rs^T Rd,  Rs^T (td - ts) / ss,  sd / ss).
 *   Edge      k = (src, dst, Z = (Rz, tz, sz), S_k 7 x 7 row-major), tangent order (rotation, translation, log-scale).  With
 *             q = Rs^T (td - ts) / ss:   e = ( Log(Rz^T Rs^T Rd),  Rz^T (q - tz),  log sd - log ss - log sz ).
 *   Update    the right perturbation of Sim(3): R <- R Exp(dw), t <- t + s R dv, s <- s exp(ds).
 *   Jacobians with E = Rz^T Rs^T Rd and Jr^-1 the inverse right Jacobian of SO(3) at e_w:
 *               d e_w / d dw:  dst Jr^-1,        src -Jr^-1 (Rs^T Rd)^T
 *               d e_t / d dv:  dst (sd / ss) E,  src -Rz^T
 *               d e_t / d dw:  dst 0,            src Rz^T [q]x
 *               d e_t / d ds:  dst 0,            src -Rz^T q
 *               d e_s / d ds:  dst +1,           src -1
 *             and zero everywhere else.  With every s = 1 and ds = 0 this is the SE(3) edge above, computed by the same
 *             operations on the same operands in the same order.
 *   Cost      1/2 [ |e_a|^2_Sa + sum_k |e_k|^2_Sk ].  The anchor is a 7-dimensional prior at the anchor node's initial value
 *             X0: e_a = ( Log(R0^T R), R0^T (t - t0), log s - log s0 ), Sa = diag(sigma_rot^2 I3, sigma_trans^2 I3,
 *             sigma_scale^2); its Jacobians are Jr^-1, s R0^T R and 1.
 *   LM        the rule of mvs_pose_graph_optimize unchanged: lambda ADDED to the diagonal, the same acceptance and termination,
 *             the LM fields of mvs_refine_params.
 * Graphs of up to 16 nodes are solved by one workgroup with a dense Cholesky in LDS: 7 * 16 = 112 unknowns, a packed triangle
 * of 112 * 113 / 2 = 6328 doubles = 50624 B, plus 4 * 112 doubles of solve vectors, 2 * 16 * 13 of node tables, 26 of the
 * anchor's record and 4 reduction cells: 57776 B, 58032 B as compiled with its padding, of the 65536 B of static LDS and no
 * scratch, so the boundary between the paths is the SE(3) solver's.  A linearised edge is 7 + 2 * 49 = 105 doubles in global memory; every entry of H is summed by one thread in edge
 * order.  Graphs of 17 .. 4096 nodes and up to 65536 edges: linearise per edge, gather per node in edge order, a block-Jacobi
 * (7 x 7) preconditioned conjugate gradient whose budget is enqueued behind a status word; cg_max_iterations = 0 means
 * 7 n_nodes and cg_chunk_iterations has the meaning, and the "every byte equals chunk 0" property, it has above.  Binary64,
 * explicit FMAs where the SE(3) solver has them, fixed summation orders, no floating-point atomics: the same input gives the
 * same bytes, and a graph in a batch gets the bytes of the single call.
 * mvs_ctx_set_pose_graph_solver and mvs_ctx_set_pose_graph_loss do NOT apply to the calls of this section: they always run the
 * conjugate gradient with no loss.  (A direct solver, marginals and robust losses for 7-DoF graphs do not exist yet.) */
typedef struct mvs_sim3_graph {            /* all host pointers */
    int32_t n_nodes, n_edges;
    const double *node_sim3;               /* n_nodes x 13: initial values, R row-major (9), t (3), s */
    const int32_t *edge_src, *edge_dst;    /* n_edges */
    const double *edge_sim3;               /* n_edges x 13: Z */
    const double *edge_cov;                /* n_edges x 49: row-major 7 x 7, order (rotation, translation, log-scale) */
    int32_t anchor_node;
} mvs_sim3_graph;
typedef struct mvs_sim3_graph_params {
    mvs_refine_params lm;                  /* only the LM fields */
    double anchor_sigma[3];                /* rotation, translation, log-scale: 1e-4 each */
    double cg_rel_tol;                     /* 1e-10 */
    int32_t cg_max_iterations;             /* 0 = 7 n_nodes */
    int32_t cg_chunk_iterations;           /* as in mvs_pose_graph_params */
} mvs_sim3_graph_params;
void mvs_sim3_graph_params_default(mvs_sim3_graph_params *p);
/* nodes_out: n_nodes x 13.  The refusals are those of mvs_pose_graph_optimize, code for code: MVS_ERR_INVALID_ARG (null
 * pointers, indices out of range, src == dst, non-finite input, a node or edge scale <= 0) and MVS_ERR_CAPACITY (more than
 * 4096 nodes or 65536 edges) before anything runs; MVS_NO_MODEL with ok = 0, every other field of the result zero and nodes_out
 * untouched for a covariance that fails the solver's 7 x 7 Cholesky test on its lower triangle (nothing is repaired), a node no
 * path of edges joins to the anchor, or finite input whose cost at the initial values is not finite. */
mvs_status mvs_sim3_graph_optimize(mvs_ctx *ctx, const mvs_sim3_graph *graph, const mvs_sim3_graph_params *params,
                                   mvs_pose_graph_result *result, double *nodes_out);
/* n_graphs graphs; graph i's nodes at nodes_out + i * 13 * (largest n_nodes of the batch), rows beyond its own node count are
 * not written.  Graphs of up to 16 nodes share one launch, larger ones run one after another; every graph gets the bytes the
 * single call returns for it.  MVS_NO_MODEL if some graph failed (results[i].ok tells which). */
mvs_status mvs_sim3_graph_optimize_batch(mvs_ctx *ctx, const mvs_sim3_graph *graphs, int n_graphs,
                                         const mvs_sim3_graph_params *params, mvs_pose_graph_result *results,
                                         double *nodes_out);
/* The resident graph of a sequence (mvs_seq_build_pose_graph, with the loop edges of mvs_seq_add_loop_edges when present)
 * lifted to Sim(3) on the device and optimised there through device pointers: node k becomes (G_k, 1), edge e becomes
 * Z = (Rz, tz, 1) with S7 = blockdiag(S'_6, scale_sigma[kind_e] * scale_sigma[kind_e]) and zero cross terms, kind 0 measured,
 * 1 fallback, 2 loop.  The lift is copies and that one multiply: result and nodes are, byte for byte, those of
 * mvs_sim3_graph_optimize on the lifted downloaded graph with anchor_node 0.  The SE(3) optimised nodes and everything else of
 * the graph stay as they are.  Waits for the ctx stream.  MVS_ERR_INVALID_ARG before mvs_seq_build_pose_graph, for parameters
 * mvs_sim3_graph_optimize refuses, or for a scale_sigma that is not finite and > 0; MVS_NO_MODEL as there. */
mvs_status mvs_seq_optimize_pose_graph_sim3(mvs_seq *s, const mvs_sim3_graph_params *p, const double scale_sigma[3],
                                            mvs_pose_graph_result *result);
/* nodes13: n_frames x 13, the Sim(3) optimised nodes.  MVS_ERR_INVALID_ARG unless the last mvs_seq_optimize_pose_graph_sim3 on
 * the current graph succeeded; whatever retires or changes the graph (a run, a rebuild, added loop edges) retires them. */
mvs_status mvs_seq_download_pose_graph_sim3(mvs_seq *s, double *nodes13);

/* ---- Loop closures of a resident sequence -------------------------------------------------------
 * Every edge of the graph above joins frames at most max_lag apart: it smooths a trajectory and cannot remove its drift.  These
 * calls find frames that see the same place again, verify the pairs with the two-view pipeline and the refinement, and append
 * them to the resident graph.  The reference has no loop closure; this is the library's own, specified here and restated in
 * numpy by tests/seq_loop_model.py.  Asynchronous on the ctx stream unless stated otherwise.
 *
 * 1 Scores.  For frames i < j with j - i >= min_gap, score[i][j] = the number of keypoints of frame j (queries) that pass the
 *   matcher's test against frame i (trains): n_i >= 2, (double)(float)D0 < ratio (double)(float)D1, and max_dist < 0 or
 *   (double)(float)D0 <= max_dist, with D0 <= D1 the two smallest Hamming distances counted with multiplicity (two trains at
 *   one distance: D1 = D0).  It is the n_matches the pair pipeline reports for base i, pair j.  Every other entry of the
 *   n_frames x n_frames table (row i, column j) is zero.  Needs the frames uploaded, not a run.  A later mvs_seq_upload or
 *   mvs_seq_upload_images discards the table, the list and the verification (their calls and downloads return
 *   MVS_ERR_INVALID_ARG until mvs_seq_loop_scores runs again); mvs_seq_upload_octaves discards the verification.  Edges
 *   already in the graph stay.
 *   MVS_ERR_INVALID_ARG: min_gap < 1 or >= n_frames, a NaN ratio or max_dist.  MVS_ERR_CAPACITY: more than 4096 frames
 *   (reported first).  The table (4 n_frames^2 bytes) is owned by the sequence. */
mvs_status mvs_seq_loop_scores(mvs_seq *s, double ratio, double max_dist, int min_gap);
/* scores: n_frames x n_frames int32.  Waits for the ctx stream.  MVS_ERR_INVALID_ARG before mvs_seq_loop_scores. */
mvs_status mvs_seq_download_loop_scores(mvs_seq *s, int32_t *scores);

/* 2 Selection.  (i, j) is eligible iff score[i][j] >= min_score.  Every j keeps its top_k eligible i by score, the smaller i
 *   on a tie.  The list is ordered by ascending j, then descending score, then ascending i, and cut after max_candidates
 *   entries; both the kept and the uncut count are recorded.  On the device; the list stays resident.
 *   MVS_ERR_INVALID_ARG: before mvs_seq_loop_scores, min_score < 1, top_k < 1, max_candidates < 1. */
typedef struct mvs_loop_select_params {
    int32_t min_score;       /* >= 1 */
    int32_t top_k;           /* >= 1 */
    int32_t max_candidates;  /* >= 1 */
    int32_t reserved;
} mvs_loop_select_params;
typedef struct mvs_loop_candidate {
    int32_t i, j;            /* base (train) and query frame, i < j */
    int32_t score;
    int32_t accepted;        /* 1: mvs_seq_add_loop_edges made it an edge; 0 before that call */
} mvs_loop_candidate;
mvs_status mvs_seq_select_loops(mvs_seq *s, const mvs_loop_select_params *p);

/* 3 Verification.  Candidate c = (i, j) becomes pair c of one batch owned by the sequence (max_candidates pairs that own their
 *   images, created at the first call): a device gather of descriptors, keypoints, octaves and counts of frames i and j, the
 *   intrinsics of the sequence's pair i, sampler key offset c.  Then mvs_batch_run (essential = 0) or mvs_batch_run_essential
 *   on the kept candidates, then mvs_batch_refine.  Results and refined results are, byte for byte, those of these calls on an
 *   uploaded batch holding the same frame pairs in candidate order with global_index[c] = c.  The call reads the kept count
 *   on the host once (it waits for the ctx stream there).
 *   MVS_ERR_INVALID_ARG: before mvs_seq_select_loops, sigma_px <= 0, parameters mvs_batch_run / mvs_batch_refine refuse.
 *   Memory: what mvs_seq_run_lags states per lag, for max_candidates pairs, plus their own two images each. */
mvs_status mvs_seq_verify_loops(mvs_seq *s, const mvs_params *two_view, int essential, const mvs_refine_params *refine,
                                double sigma_px);

/* 4 Edges.  After mvs_seq_build_pose_graph and mvs_seq_verify_loops: one edge per accepted candidate is appended behind the
 *   built edges, in candidate order: source i, destination j, edge_lag = j - i, edge_kind = 2.  Acceptance, the scale s and
 *   S' = D S D are the rules of mvs_seq_build_pose_graph with (k, k + d) = (i, j) and r = the candidate's refined result.
 *   Then loop_sigma[0]^2 is added to the three rotation diagonal entries of S' and loop_sigma[1]^2 to the three translation
 *   ones (each only where its loop_sigma > 0): the scale of a loop edge comes from a drifted trajectory, and at a true revisit
 *   s is small, so S' alone would be far too tight.  The positive-definite test runs on the final matrix.  Plain binary64 in
 *   the order written, no fused operation.  A second call first cuts the graph back to its built edges; the call clears what
 *   mvs_seq_optimize_pose_graph left.  mvs_seq_optimize_pose_graph works on the longer list unchanged.
 *   MVS_ERR_CAPACITY (reported first, nothing changes): the build's candidate slots plus max_candidates exceed 65536.
 *   MVS_ERR_INVALID_ARG: min_points < 0, a negative or NaN max_error, a NaN loop_sigma, no graph built, candidates not
 *   verified since the last selection. */
typedef struct mvs_loop_edge_params {
    int32_t min_points;     /* 0 = no gate */
    int32_t reserved;
    double  max_error;      /* gate on the refined error; 1e30 = open */
    double  loop_sigma[2];  /* rotation, translation; <= 0 adds nothing */
} mvs_loop_edge_params;
mvs_status mvs_seq_add_loop_edges(mvs_seq *s, const mvs_loop_edge_params *p);

/* The resident list.  *n_kept entries of cand[max_candidates] are candidates (the rest zero), *n_found is the count before the
 * cut.  results / matches / inlier_mask / points_xyz / point_idx: rows [0, n_kept) as mvs_batch_download lays them out, and
 * refined[n_kept]: valid after mvs_seq_verify_loops (MVS_ERR_INVALID_ARG if one of them is asked for before).  Any pointer may
 * be NULL.  Waits for the ctx stream.  MVS_ERR_INVALID_ARG before mvs_seq_select_loops. */
mvs_status mvs_seq_download_loop_candidates(mvs_seq *s, int32_t *n_kept, int32_t *n_found, mvs_loop_candidate *cand,
                                            mvs_pair_result *results, mvs_match *matches, uint8_t *inlier_mask,
                                            double *points_xyz, int64_t *point_idx, mvs_refine_result *refined);

#ifdef __cplusplus
}
#endif
#endif /* MVSLAM_HIP_H */
