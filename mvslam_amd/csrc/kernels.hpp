// kernels.hpp -- device data layout + kernel launch interface (host side sees only PODs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mvslam_hip.h"

namespace mvs {

constexpr int kBoxRec = 12;          // doubles per pair in BatchDev::box
constexpr int kMaxKp = 4096;          // capacity limit of one image (LDS lists in finalize/compact)
constexpr int kSortBins = kMaxKp + 1;  // counts 0 .. kMaxKp (ransac_list_sort_kernel)
constexpr int kHypPerBlock = 256;     // hypotheses per RANSAC workgroup (one per lane, 4 waves)
constexpr int kMaxDescWords = 16;     // descriptor <= 64 bytes
constexpr int kHypRec = 10;           // doubles per hypothesis record: F[9], counting threshold (thr + band)
constexpr int kHypRec32 = 12;         // floats per single-precision record (mode 1): F~[9], tu, tl, spare

// Best hypothesis of one RANSAC workgroup.  count < 0: no valid hypothesis in the group.
struct WgBest {
    int32_t count;
    uint32_t hyp;
    double residual;
    double F[9];
};
static_assert(sizeof(WgBest) == 88, "WgBest layout");

// What finalize_model hands to triangulate / finalize_select for one pair.
struct FinModel {
    double R[2][9];   // Ra, Rb (raw)
    double Rr[2][9];  // rectified (SO3 ctor) -> P2
    double T[3];
    int32_t n_inl;
    int32_t ncand;
    int32_t proceed;
    int32_t npre;        // inliers [0, npre) are triangulated under EVERY candidate by finalize_model (the prefix)
    int32_t pre_cnt[4];  // points of the prefix in front of both cameras, per candidate
    int32_t best_c;      // candidate with the largest prefix count (lowest index on ties): the one triangulate completes
    int32_t pad[3];
};

// Resident state of a batch (all device pointers).  P pairs, capacity N keypoints per image.
struct BatchDev {
    int n_pairs;
    int max_kp;       // N
    int desc_words;   // descriptor bytes / 4
    int max_groups;   // capacity of wgbest per pair
    int cu_count;     // compute units of the batch's device (hipDeviceAttributeMultiprocessorCount): launch-shape decisions

    // inputs
    const uint32_t *desc1;  // [P][N][desc_words]   base / train (vf1)
    const uint32_t *desc2;  // [P][N][desc_words]   pair / query (vf2)
    const float *kp1;       // [P][N][2]
    const float *kp2;       // [P][N][2]
    const uint8_t *oct1;    // [P][N] pyramid octave of every keypoint (cv::KeyPoint::octave), 0 where unknown
    const uint8_t *oct2;    // [P][N]
    const int32_t *n1;      // [P]
    const int32_t *n2;      // [P]
    const double *Kinv;     // [P][9]  host-computed cofactor inverse (camera.cpp:16)
    const double *K;        // [P][9]
    const int64_t *gidx;    // [P] global pair index (sampler key offset)

    // intermediates
    int32_t *knn_train;  // [P][N] best train index per query, -1 = rejected
    int32_t *knn_dist;   // [P][N]
    int32_t *M;          // [P] number of matches
    mvs_match *matches;  // [P][N]
    double *pts;         // [P][N][4]  (x1, y1, x2, y2) ideal-camera coordinates of match m
    WgBest *wgbest;      // [P][max_groups]
    double *hyp_F;       // [P][max_groups * 256][kHypRec]: F (9) of every hypothesis + its counting threshold thr + band
                         // (solve / pre-screen -> scoring hand-over), may be null
    float *hyp_r32;      // [P][max_groups * 256][kHypRec32]: the SINGLE-PRECISION pre-screen records of the pairs in mode 1 (48
                         // bytes: F~ as 9 floats, upper and lower counting threshold, one spare): written by the pre-screen, read
                         // by the pilot / dense / finish counting kernels.  Exact F (survivors, uncertified) stays in hyp_F
    uint8_t *hyp_okf;    // [P][max_groups * 256] state of the record: 0 rejected sample, 1 approximate F (pre-screen), 2 waits
                         // for the exact solve, 3 exact F
    int32_t *hyp_cnt;    // [P][max_groups * 256] full (upper-bound) inlier count of a hypothesis that can still win, -1 otherwise
    int32_t *bound;      // [P] largest full (lower-bound) count seen so far: the pruning bound of the counting kernel
    double *box;         // [P][kBoxRec] bounding box of the pair's matches (x1lo, x1hi, y1lo, y1hi, x2lo, x2hi, y2lo, y2hi) and
                         // its absolute maxima max(|lo|, |hi|) per coordinate (x1, y1, x2, y2): what the pre-screen's bounds
                         // need of the box alone, once per pair instead of once per hypothesis
    int32_t *mode;       // [P] 0: every hypothesis is solved exactly; 1: pre-screened, counted in single precision; 2: pre-
                         // screened, counted in double precision
    uint32_t *clist;     // [P][max_groups * 256] hypotheses of the pair the dense counting phase left alive (for the finish)
    uint32_t *clist2;    // [P][max_groups * 256] the same list sorted by partial count (ransac_list_sort_kernel)
    int32_t *cpos;       // [P][kSortBins] cpos[c] = entries of the sorted list with a partial count >= c (the sort's own
                         // offsets): the finish reads how long the list's live prefix is instead of walking the dead rest
    int32_t *ccount;     // [P] their number
    int32_t *pcount;     // [P] entries of the pair's candidate list for the selection (ransac_survivors_kernel -> ransac_select_kernel;
                         // the list itself reuses the first half of clist, which is dead after the list sort)
    int32_t *m0list;     // [1 + P] number of pairs in mode 0, then those pairs (mode0_list_kernel -> ransac_solve_list_kernel)
    int32_t *dense_n1;   // [P] points the dense (matrix-core) counting phase covered for the pair
    uint32_t *xlist;     // [P * max_groups * 256] work list of the list-driven exact solve: flat indices pair * Hp + h
    uint32_t *xcount;    // [2] {entries of the list: flagged by the pre-screen + survivors of the count, unused}
    double *cand_pts;    // [P][4][N][3] triangulation scratch
    FinModel *fin;       // [P]
    uint16_t *inl;       // [P][N] ordered inlier list
    uint8_t *okf;        // [P][4][N] cheirality flags per candidate

    // outputs
    mvs_pair_result *results;  // [P]
    uint8_t *mask;             // [P][N]
    double *points;            // [P][N][3]
    int32_t *point_idx;        // [P][N]

    // optional per-hypothesis tables (single-shot diagnostics), may be null
    int32_t *hyp_count;     // [P][H]
    double *hyp_residual;   // [P][H]

    // work statistics (instrumented replay only), may be null: {rotations9, pairs9}
    unsigned long long *stats;
};

enum FinalizeMode : int {
    kFinalizeFull = 0,      // reduce wgbest -> F -> mask -> E -> decompose -> triangulate -> pose
    kFinalizeFromE = 1,     // results[p].E and mask are given
    kFinalizeTriangulate = 2, // results[p].R1to2 / t1to2 given, mask given; one candidate
    kFinalizeEssential = 3    // as kFinalizeFromE, behind the five-point RANSAC (essential5.hip): its selection has also written
                              // best_hyp / best_count / best_residual / F, which are kept, and sfm_solve's inlier gate applies
};

struct RunParams {
    double ratio;
    double max_dist;
    double max_error_sq;  // <= 0: 5e-2 / K00 / K11 per pair
    int num_hypotheses;
    int sampler;
    uint64_t seed;
    int min_inliers;
};

// ---- pnp_solve (row f1) ----------------------------------------------------------------------------
constexpr int kPnpMaxPoints = kMaxKp;  // = the keypoint capacity (round 5: the point stream is chunked through LDS; 2048 before)

struct PnpRec {  // best hypothesis of one RANSAC workgroup
    int32_t count;
    uint32_t hyp;
    double R[9];
    double t[3];
};

struct PnpOut {
    int32_t ok;
    int32_t n_inliers;
    int32_t best_hyp;
    int32_t pad;
    double R[9];     // camera in world = SE3(SO3(Rw2c), tw2c).inverse()
    double t[3];
    double Rw2c[9];
    double tw2c[3];
};

struct PnpDev {       // a batch of PnP problems; problem q owns slice [q * stride, q * stride + n[q])
    int n_problems;
    int stride;       // capacity (points) of one problem, <= kPnpMaxPoints
    int num_hypotheses;
    int sampler;
    int min_inliers;
    int max_groups;   // records per problem
    uint64_t seed;    // problem q uses seed + gidx[q]
    double thr2;      // reproj_error^2
    const int32_t *n;       // [Q] points of each problem (< 7: no model)
    const int64_t *gidx;    // [Q] sampler key offsets (may be null = 0)
    const double *K;        // [Q][9]
    const double *Kinv;     // [Q][9]
    const double *X;        // [Q][stride][3] world points
    const double *uv;       // [Q][stride][2] image points
    double *xy;             // [Q][stride][2] ideal-camera coordinates
    double *fb;             // [Q][stride][3] unit bearings
    PnpRec *rec;            // [Q][max_groups]
    int32_t *inliers;       // [Q][stride]
    PnpOut *out;            // [Q]
};

void launch_pnp(const PnpDev &p, hipStream_t stream);

// ---- frame sequences (row f2): join of pair q's points with their observations in frame q + 2 ------------------
struct SeqJoinDev {
    int n_tracks;      // n_frames - 2
    int max_kp;
    int stride;        // capacity of one PnP problem = min(max_kp, kPnpMaxPoints)
    const mvs_pair_result *results;  // [n_frames - 1]
    const mvs_match *matches;        // [n_frames - 1][max_kp]
    const int32_t *M;                // [n_frames - 1]
    const double *points;            // [n_frames - 1][max_kp][3]
    const int32_t *point_idx;        // [n_frames - 1][max_kp]
    const float *kp;                 // [n_frames][max_kp][2]
    double *X;                       // [n_tracks][stride][3]
    double *uv;                      // [n_tracks][stride][2]
    int32_t *n_corr;                 // [n_tracks]
};
void launch_seq_join(const SeqJoinDev &j, hipStream_t stream);

// scale propagation + trajectory of a sequence (sequential fold over the frames, pnp.hip)
struct SeqChainDev {
    int n_frames;
    const mvs_pair_result *results;  // [n_frames - 1]
    const PnpOut *tracks;            // [n_frames - 2]
    const int32_t *n_corr;           // [n_frames - 2]
    double *traj_R;                  // [n_frames][9] pose of frame k in frame 0 (pair 0's baseline = 1)
    double *traj_t;                  // [n_frames][3]
    double *traj_sigma;              // [n_frames - 1] sigma_k = pair k's unit baseline in units of pair 0's
    double *track_scale;             // [n_frames - 2]
};
void launch_seq_chain(const SeqChainDev &c, hipStream_t stream);

// mvs_seq_rescale, MVS_SEQ_SCALE_DEPTH_RATIO: the scale steps from depth ratios of the points consecutive pairs share, then
// sigma and the trajectory from the pairs alone, over SeqChainDev's outputs (pnp.hip)
struct SeqScaleDev {
    int n_frames;
    int max_kp;
    int min_common;                  // fewer used points: the step keeps the scale
    const mvs_pair_result *results;  // [n_frames - 1]
    const mvs_match *matches;        // [n_frames - 1][max_kp]
    const int32_t *point_idx;        // [n_frames - 1][max_kp]
    const double *points;            // [n_frames - 1][max_kp][3]
    mvs_seq_scale_step *steps;       // [n_frames - 2]
    double *traj_R, *traj_t, *traj_sigma, *track_scale;   // SeqChainDev's
};
void launch_seq_rescale(const SeqScaleDev &d, hipStream_t stream);

// ---- sfm_refine / pnp_refine (row f4): batched Schur-complement Levenberg-Marquardt ---------------------------
struct RefineCfg {
    int max_iterations;
    double lambda_initial, lambda_factor, lambda_upper, rel_tol, abs_tol;
    double w[2][6];   // 1 / sigma^2 of the pose priors, frame 0 and 1
};

struct RefineDev {     // G problems; problem g owns slice [g * stride, g * stride + m[g])
    int n_problems;
    int stride;        // point capacity of one problem
    int n_frames;      // 2: frame 0 = camera 1 anchored at the identity, frame 1 = camera 2.  1: the moving camera
    RefineCfg cfg;
    const int32_t *m;        // [G] points (< 1: not solved)
    const double *K;         // [G][9]
    const double *pose0;     // [G][12] guess of the moving camera: R (9), t (3), camera in world
    const double *pose0_all; // optional [G][n_frames][12]: every frame's guess (general two-frame problem), else null
    const double *obs[2];    // [G][stride][2] image points seen by frame f
    const double *oinfo[2];  // [G][stride][3] their information matrices (xx xy yy)
    const double *pts0;      // [G][stride][3] point guesses = prior means
    const double *pinfo;     // [G][stride][6] point prior information (xx xy xz yy yz zz)
    double *pts;             // [G][stride][3] refined points (out)
    double *pts_tmp;         // [G][stride][3] candidate buffer
    double *point_cov;       // [G][stride][9] marginal covariances (out), may be null
    mvs_refine_result *out;  // [G] the moving camera (frame n_frames - 1)
    mvs_refine_result *out_all;  // optional [G][n_frames]: every frame, else null
};
// covariance -> information on the device.  cov2_[f]: [G][stride][4] or null (identity); cov3: [G][stride][9] or null
// (isotropic weight iso3).  Writes d.oinfo / d.pinfo (cast away const by the caller's own buffers).
void launch_refine_prep(const RefineDev &d, const double *cov2_0, const double *cov2_1, const double *cov3, double iso3,
                        double *oinfo0, double *oinfo1, double *pinfo, const uint8_t *valid0, const uint8_t *valid1,
                        hipStream_t stream);
void launch_refine(const RefineDev &d, hipStream_t stream);
// pnp_solve's refit over the inliers for a batch of PnP problems (the tracks of a sequence): gather -> refine_kernel<1>
// -> poses written back into p.out.  d: a one-frame RefineDev over the same problems with its own buffers.
void launch_pnp_refit(const PnpDev &p, const RefineDev &d, double point_sigma, hipStream_t stream);
// batch glue: build the two-view refinement problems of every pair from the batch's own results
void launch_refine_gather(const BatchDev &b, int n_active, double sigma_px, double point_sigma, int stride, int32_t *m,
                          double *pose0, double *obs0, double *obs1, double *oinfo0, double *oinfo1, double *pts0,
                          double *pinfo, hipStream_t stream);

// ---- ba_frame_pose_and_point on windows of 3 .. 8 frames (refine_window_kernel) ---------------------------------
constexpr int kWinMaxFrames = 8;
struct WinProblem {      // one window of a batch; windows differ in frames and points, so every array is ragged
    int32_t n_frames;    // F
    int32_t n_points;    // m
    int64_t in_off;      // first double of the window's inputs in WinDev::in: camera fx sk cx fy cy (5, padded to 8), poses
                         // F x 12 (guess = prior mean), pose prior weights F x 6, point guesses m x 3, point prior information
                         // m x 6 (xx xy xz yy yz zz), observations F x m x 2, their information F x m x 3 (0 0 0 = not seen)
    int64_t pt_off;      // first point of the window in pts / pts_tmp / point_cov
    int64_t fr_off;      // first frame of the window in out
};
static_assert(sizeof(WinProblem) == 32, "WinProblem layout");
struct WinDev {
    int n_problems;
    RefineCfg cfg;       // the Levenberg-Marquardt fields; the prior weights travel with each window
    const WinProblem *prob;
    const double *in;
    double *pts;         // [sum m][3] refined points (out)
    double *pts_tmp;     // [sum m][3] candidate buffer
    double *point_cov;   // [sum m][9] marginal covariances (out), may be null
    mvs_refine_result *out;   // [sum F]
};
void launch_refine_window(const WinDev &d, hipStream_t stream);

// ---- pose graphs: the back end (posegraph.hip) ---------------------------------------------
constexpr int kPgDenseMaxNodes = 16;     // up to here one workgroup solves the dense 6N x 6N system in LDS
constexpr int kPgMaxNodes = 4096, kPgMaxEdges = 65536;
constexpr int kPgLin = 78;               // doubles of one linearised edge: whitened residual 6, A_src 36, A_dst 36 (row-major)
struct PgCfg {
    int max_iterations;
    double lambda_initial, lambda_factor, lambda_upper, rel_tol, abs_tol;
    double w_anchor[2];                  // 1 / sigma^2 of the anchor prior: rotation, translation
    double cg_rel_tol;
    int cg_max_iterations;
    // robust loss of the edges with index >= loss_first inside their graph (mvs_ctx_set_pose_graph_loss; DESIGN.md section
    // 4.10.5): 0 none, 1 Huber, 2 Cauchy, with the constant loss_k.  0 runs the statements the kernels ran before there was one.
    int loss, loss_first;
    double loss_k;
};
struct PgProblem {       // one graph of a dense-path batch
    int32_t n_nodes, n_edges, anchor, reserved;
    int64_t node_off;    // first node of the graph in node_pose / poses_out
    int64_t edge_off;    // first edge of the graph in every per-edge array
};
static_assert(sizeof(PgProblem) == 32, "PgProblem layout");
struct PgDenseDev {
    int n_problems;
    PgCfg cfg;
    const PgProblem *prob;
    const double *node_pose;     // [sum N][12] initial values; the anchor's is its prior mean
    const int32_t *edge_src, *edge_dst;
    const double *edge_pose;     // [sum E][12] Z
    const double *edge_cov;      // [sum E][36]
    double *W;                   // [sum E][21] whitening factor L^-1 of every edge (packed lower)
    double *lin;                 // [sum E][kPgLin]
    double *poses_out;           // [sum N][12]
    mvs_pose_graph_result *out;  // [G]
};
void launch_pg_dense(const PgDenseDev &d, hipStream_t stream);

struct PgState {         // what the host reads once per LM iteration of the large path
    double cost0, cand;  // sum of squared whitened residuals at the initial / candidate values
    double rz, gnorm2, rr;
    int32_t done;        // CG status word: 0 running, 1 converged, 2 broke down (p.Hp <= 0 or a block not positive definite)
    int32_t cg_iters;
    int32_t bad_cov;     // some edge covariance is not positive definite
    int32_t reserved;
};
struct PgLargeDev {
    int n_nodes, n_edges, anchor;
    PgCfg cfg;
    const int32_t *edge_src, *edge_dst;
    const double *edge_pose, *edge_cov;
    const int32_t *csr_off;      // [N + 1]
    const int32_t *csr_inc;      // [2 E] incident edges of every node in edge order: 2 * edge + (0: node is src, 1: dst)
    const double *pose0;         // [N][12] initial values
    double *pose[2];             // [N][12] current / candidate (which is which: the host's)
    double *W, *lin, *u, *ecost; // [E][21], [E][kPgLin], [E][6], [E]
    double *D, *Mf;              // [N][21] diagonal blocks of H; Cholesky factors of the damped blocks
    double *g, *x, *r, *z, *p, *q;   // [N][6]
    double *pq;                  // [N]
    double *Ha;                  // [36] the anchor prior's block of H
    PgState *state;
};
void launch_pg_prep(const PgLargeDev &d, hipStream_t stream);
// one LM iteration at pose[cur] with damping lam, in three parts the host enqueues in this order:
//   begin  linearise, gather, PCG start.  `first`: the cost at pose[cur] -> state->cost0 before it.
//   cg     n PCG iterations; the status word makes the ones behind convergence leave at once.  The whole budget in one call
//          or in chunks with a status read between them (mvs_pose_graph_params.cg_chunk_iterations): the same kernels with
//          the same arguments either way.
//   end    candidate = pose[cur ^ 1], its cost -> state->cand.
void launch_pg_begin(const PgLargeDev &d, int cur, double lam, bool first, hipStream_t stream);
void launch_pg_cg(const PgLargeDev &d, double lam, int n, hipStream_t stream);
void launch_pg_end(const PgLargeDev &d, int cur, hipStream_t stream);
// begin without the PCG start: what the direct step (below) has in front of it
void launch_pg_linearise(const PgLargeDev &d, int cur, bool first, hipStream_t stream);

// per-edge residuals of one graph at the poses X (mvs_pose_graph_edge_stats): chi2[k] = |r_k|^2 of the whitened residual and,
// with `weight`, w(chi2[k]) under cfg's loss (1 below cfg.loss_first).  Every pointer is device memory; W is scratch.
struct PgStatsDev {
    int n_edges;
    PgCfg cfg;                   // loss, loss_first and loss_k are read
    const int32_t *edge_src, *edge_dst;
    const double *edge_pose, *edge_cov;
    const double *X;             // [N][12]
    double *W;                   // [E][21]
    double *chi2, *weight;       // [E]; weight may be null
    int32_t *bad_cov;            // set to 1 when an edge covariance is not positive definite (zeroed by the launch's caller)
};
void launch_pg_edge_stats(const PgStatsDev &d, hipStream_t stream);

// ---- pose graphs over Sim(3) (sim3graph.hip) ------------------------------------------------------
// The same two paths with 7 degrees of freedom per node: a node is (R, t, s) in 13 doubles, an edge's covariance 7 x 7, its
// whitening factor 28 doubles.  PgProblem and PgState are the SE(3) solver's.
constexpr int kS3DenseMaxNodes = 16;     // 7 * 16 = 112 unknowns: a packed triangle of 6328 doubles = 50624 B of LDS
constexpr int kS3Node = 13, kS3Cov = 49, kS3W = 28;
constexpr int kS3Lin = 105;              // whitened residual 7, A_src 49, A_dst 49 (row-major)
struct S3Cfg {
    int max_iterations;
    double lambda_initial, lambda_factor, lambda_upper, rel_tol, abs_tol;
    double w_anchor[3];                  // 1 / sigma^2 of the anchor prior: rotation, translation, log-scale
    double cg_rel_tol;
    int cg_max_iterations;
};
struct S3DenseDev {
    int n_problems;
    S3Cfg cfg;
    const PgProblem *prob;
    const double *node;          // [sum N][13] initial values; the anchor's is its prior mean
    const int32_t *edge_src, *edge_dst;
    const double *edge_z;        // [sum E][13]
    const double *edge_cov;      // [sum E][49]
    double *W;                   // [sum E][28]
    double *lin;                 // [sum E][kS3Lin]
    double *nodes_out;           // [sum N][13]
    mvs_pose_graph_result *out;  // [G]
};
void launch_s3_dense(const S3DenseDev &d, hipStream_t stream);
struct S3LargeDev {
    int n_nodes, n_edges, anchor;
    S3Cfg cfg;
    const int32_t *edge_src, *edge_dst;
    const double *edge_z, *edge_cov;
    const int32_t *csr_off, *csr_inc;   // PgLargeDev's
    const double *node0;         // [N][13] initial values
    double *node[2];             // [N][13] current / candidate
    double *W, *lin, *u, *ecost; // [E][28], [E][kS3Lin], [E][7], [E]
    double *D, *Mf;              // [N][28]
    double *g, *x, *r, *z, *p, *q;   // [N][7]
    double *pq;                  // [N]
    double *Ha;                  // [49] the anchor prior's block of H
    PgState *state;
};
// the parts of one LM iteration, as launch_pg_prep / _begin / _cg / _end
void launch_s3_prep(const S3LargeDev &d, hipStream_t stream);
void launch_s3_begin(const S3LargeDev &d, int cur, double lam, bool first, hipStream_t stream);
void launch_s3_cg(const S3LargeDev &d, double lam, int n, hipStream_t stream);
void launch_s3_end(const S3LargeDev &d, int cur, hipStream_t stream);
// an SE(3) graph lifted to Sim(3) (mvs_seq_optimize_pose_graph_sim3): node k -> (pose, 1), edge e -> (Z, 1) and
// blockdiag(cov, scale_sigma[kind_e] * scale_sigma[kind_e]); copies and one multiply
struct S3LiftDev {
    int n_nodes, n_edges;
    double scale_sigma[3];
    const double *node_pose, *edge_pose, *edge_cov;   // [N][12], [E][12], [E][36]
    const int32_t *edge_kind;                         // [E]
    double *node, *edge_z, *cov;                      // [N][13], [E][13], [E][49]
};
void launch_s3_lift(const S3LiftDev &d, hipStream_t stream);

// ---- the direct LM step of the large path (pg_direct.hip) ------------------------------------
// (H + lambda I) x = -g by a block-scaled skyline Cholesky.  The diagonal blocks D and the gradient g are pg_gather_kernel's;
// C_i C_i^T = D_i + lambda I, the scaled matrix C_i^-1 A_ij C_j^-T (unit diagonal blocks) is assembled into the envelope of
// pg_envelope.hpp, factorised in place and solved; x_i = C_i^-T z_i.
struct PgdState {
    int32_t status;      // 0 solved; 2 a diagonal block of H + lambda I failed its Cholesky; 3 a pivot of the skyline failed
    int32_t bad_code;    // n_nodes - (the first node at which that happened); 0: none
    double min_d;        // the smallest pivot of the scaled factorisation before its square root (status 0 or 3)
};
struct PgdDev {
    int n_nodes, n_blocks;
    const int32_t *first;        // [N]
    const int32_t *row_off;      // [N + 1]
    const int32_t *blk_row;      // [n_blocks] the row of every block of the envelope
    const int32_t *blk_slot;     // [n_blocks] its slot in the term lists, -1: no term touches it (fill only)
    const int32_t *slot_off;     // [n_slots + 1]
    const int32_t *codes;        // pg_envelope.hpp block_lists
    const double *lin;           // [E][kPgLin]
    const double *D, *g;         // [N][21], [N][6]: pg_gather_kernel's
    double *Cinv;                // [N][21] C_i^-1, packed lower
    double *sky;                 // [n_blocks][36]; a diagonal block of the factor holds L_ii^-1
    double *y;                   // [N][6] right-hand side, then y, then z
    double *x;                   // [N][6] the step
    PgdState *state;
    // the second source (ba_sparse.hip), zero for the pose graphs: `pre` holds the off-diagonal blocks
    // of the envelope already summed, unscaled ([n_blocks][36]; it may be `sky` itself) and the term lists are not read; D and g
    // are then the caller's own.  A pivot of the skyline must exceed pivot_tol (the scaled matrix has a unit diagonal).
    const double *pre;
    double pivot_tol;
};
// scale, assemble, factorise (the forward substitution rides along), back-substitute and unscale: four launches
void launch_pgd_step(const PgdDev &d, double lam, hipStream_t stream);

// ---- sparse bundle adjustment of up to 4096 frames (ba_sparse.hip) ----------------------------
// The points are eliminated per point, the reduced camera system goes into the skyline of ba_envelope.hpp and the step is
// launch_pgd_step's with PgdDev::pre = sky, D and g the arrays below.  The host drives the LM loop.
constexpr int kBasLin = 20;      // doubles of one linearised observation: Jc 12 (2 x 6), Jp 6 (2 x 3), r 2
constexpr int kBasRedChunk = 4096;   // terms one workgroup of the cost's first reduction stage sums
// the pivot rule of the bundle adjustments (refine_window_kernel, the point blocks, PgdDev::pivot_tol of the sparse path): a
// pivot must exceed this times the entry before elimination.  2.3e-13 ~ 16 x 48 x 2^-52
constexpr double kBaPivotTol = 1.0 / (double)(1ll << 42);
struct BasState {        // what the host reads once per LM iteration
    double cost;         // sum of the squared Mahalanobis norms at the values of the last cost launch (no 1/2)
    int32_t bad_point;   // some point's V failed the pivot rule in the last build
    int32_t reserved;
};
struct BasDev {
    int n_frames, n_points, n_obs, n_blocks;
    double cam[5];               // fx sk cx fy cy
    const double *pose0, *w;     // [F][12] guess = prior mean; [F][6] prior weights (0: none)
    const double *pts0, *pinfo;  // [P][3] guess = prior mean; [P][6] prior information (xx xy xz yy yz zz)
    const int32_t *obs_off, *obs_frame, *obs_point;   // [P + 1], [O], [O]
    const double *obs_uv, *oinfo;                     // [O][2], [O][3] (xx xy yy)
    const int32_t *fr_off, *fr_obs;                   // [F + 1], [O]
    const int32_t *first, *row_off, *blk_row, *last;  // the envelope: [F], [F + 1], [n_blocks], [F]
    const int32_t *pair_off, *pair_a, *pair_c;        // [n_blocks + 1], [pairs], [pairs]
    double *pose[2], *pts[2];    // [F][12], [P][3]: current / candidate (which is which: the host's)
    double *lin;                 // [O][kBasLin]; the covariance pass keeps Y_o (18) in it
    double *Li, *gh;             // [P][6] L^-1 of V = L L^T (l00 l10 l11 l20 l21 l22), [P][3] L^-1 g_p
    double *Z, *zd;              // [O][18] Z_o = Hcp_o L^-T (6 x 3), [O][3] Z_o^T delta_f
    double *prior;               // [F][27] the pose priors' share of Hcc_f (21, packed lower) and g_f (6)
    double *D, *g;               // [F][21], [F][6]: diagonal blocks and gradient of the reduced system (lambda not in it)
    double *sky;                 // [n_blocks][36]
    const double *Cinv, *x;      // [F][21], [F][6]: the step's scaling and the step (PgdDev's)
    double *terms, *partial;     // [O + P + F] cost terms, [ceil(that / kBasRedChunk)]
    double *inv, *colm;          // [n_blocks][36] blocks of the scaled S^-1, [F][36] (covariance pass)
    double *pose_cov, *point_cov;   // [F][36], [P][9]; either may be null
    BasState *state;
    // robust loss of the observation terms (mvs_ctx_set_ba_loss): 0 none, 1 Huber, 2 Cauchy, with the
    // constant loss_k.  0 issues the launches there were before there was one and reads oinfo alone.  With a loss, oinfo is
    // the array the robust linearisation writes, w(s_o) W_o, which is all the build kernels see of it; the cost and the
    // statistics read the caller's W_o through oinfo0.
    int loss;
    double loss_k;
    const double *oinfo0;        // [O][3]
    double *oinfo_w;             // [O][3]: what oinfo points at under a loss
};
// s_o and w(s_o) of every observation at the given poses and points (device pointers; weight may be null): reads n_obs, cam,
// obs_frame, obs_point, obs_uv, oinfo0, loss and loss_k of d
void launch_bas_obs_stats(const BasDev &d, const double *poses, const double *points, double *chi2, double *weight,
                          hipStream_t stream);
// cost at pose[which], pts[which] -> state->cost
void launch_bas_cost(const BasDev &d, int which, hipStream_t stream);
// linearise at [cur] with damping lam: Li, gh, Z, D, g and the off-diagonal blocks of sky; clears state->bad_point first
void launch_bas_build(const BasDev &d, int cur, double lam, hipStream_t stream);
// candidate = [cur ^ 1] from the step x
void launch_bas_update(const BasDev &d, int cur, hipStream_t stream);
// behind a build and a step at lambda = 0: blocks of S^-1 inside the envelope, pose_cov, point_cov
void launch_bas_cov(const BasDev &d, hipStream_t stream);

// ---- marginal covariances of a pose graph (pg_marginals.hip) ---------------------------------
// H = J_a^T W_a J_a + sum_k J_k^T W_k J_k at the poses X, no lambda, as the block lower triangle inside its envelope (row i
// holds the blocks first[i] .. i, 36 doubles each, row-major); factorised in place, H = L L^T.
struct PgmState {
    int32_t status;      // 0 running / done, 1 an edge covariance is not positive definite, 2 a pivot failed
    int32_t bad_node;    // the node of that pivot, -1 otherwise
    double min_d;        // the smallest pivot before its square root (the smallest diagonal entry of L, squared)
};
struct PgmDev {
    int n_nodes, n_edges, anchor, n_slots;
    double w_anchor[2];
    const int32_t *edge_src, *edge_dst;
    const double *edge_pose, *edge_cov;
    const double *pose0;         // [N][12] the anchor's mean is pose0[anchor]
    const double *X;             // [N][12] the linearisation point
    const int32_t *first;        // [N]
    const int32_t *row_off;      // [N + 1] first block of every row in sky
    const int32_t *slot_blk;     // [n_slots] block of H that slot s owns
    const int32_t *slot_off;     // [n_slots + 1]
    const int32_t *codes;        // terms of every slot in edge order (pg_envelope.hpp block_lists)
    double *lin;                 // [E][kPgLin]
    double *Ha;                  // [36] the anchor prior's block
    double *sky;                 // [envelope blocks][36]
    PgmState *state;
    // the solves: query q = (qi[q], qj[q]) owns y[q] and writes out[q]
    const int32_t *qi, *qj;
    double *y;                   // [chunk][N][6][12]
    double *out;                 // [chunk][36]
};
void launch_pgm_assemble(const PgmDev &d, hipStream_t stream);
void launch_pgm_factor(const PgmDev &d, hipStream_t stream);
void launch_pgm_solve(const PgmDev &d, int n_query, hipStream_t stream);

// ---- sliding windows of a resident sequence (mvs_seq_refine_windows) -------------------------
// seq_link_kernel chains the inlier matches of consecutive pairs into tracks (every keypoint gets at most one successor and
// one predecessor); seq_window_assemble_kernel turns the tracks of window w = frames [w * stride, w * stride + F) into the
// inputs refine_window_kernel reads.  Every window owns in_stride doubles of `in` and max_points points, whatever it holds.
constexpr int kSeqWinMaxOctave = 30;   // mvs_seq_upload_octaves admits no more
struct SeqWinDev {
    int n_frames, max_kp;              // the sequence: frames, keypoint capacity N of a frame
    int F, stride, max_points, n_windows;
    // resident state of the sequence (mvs_seq_run)
    const mvs_pair_result *results;    // [n_frames - 1]
    const mvs_match *matches;          // [n_frames - 1][N]
    const uint8_t *mask;               // [n_frames - 1][N]
    const double *points;              // [n_frames - 1][N][3]
    const int32_t *point_idx;          // [n_frames - 1][N]
    const float *kp;                   // [n_frames][N][2]
    const uint8_t *oct;                // [n_frames][N]
    const double *K;                   // [9] the sequence's camera
    const double *traj_R, *traj_t, *traj_sigma;   // SeqChainDev's outputs
    // links (seq_link_kernel): pair k joins keypoint i of frame k to keypoint matches[k][succ[k][i]].queryIdx of frame k + 1
    int32_t *succ;                     // [n_frames - 1][N] match row of the link out of keypoint i, -1 = none
    int32_t *pred;                     // [n_frames][N] keypoint of the previous frame linked to keypoint i, -1 = none
    int32_t *row_to_point;             // [n_frames - 1][N] inverse of point_idx: triangulated point of a match row, -1 = none
    // what every window shares: prior weights of frame a and of the other frames, the points' prior information (xx xy xz yy
    // yz zz) and the observations' information (xx xy yy) per octave, all worked out on the host
    double w_anchor[6], w_pose[6], pinfo[6], oinfo[kSeqWinMaxOctave + 1][3];
    // outputs
    WinProblem *prob;                  // [n_windows]
    double *in;                        // [n_windows][in_stride]
    int64_t in_stride;
    mvs_seq_window_info *info;         // [n_windows]
    int32_t *track_kp;                 // [n_windows][max_points][F] keypoint of the track in frame a + f, -1 = not seen
    double *point_guess;               // [n_windows][max_points][3]
};
void launch_seq_windows(const SeqWinDev &d, hipStream_t stream);
// seq_link_kernel alone: succ, pred and row_to_point of d (n_frames, max_kp and the resident state are read)
void launch_seq_link(const SeqWinDev &d, hipStream_t stream);

// ---- the global problem of a resident sequence (mvs_seq_refine_global; seq_global.hip) ----------
// The tracks of seq_link_kernel's tables, whole (T = 0) or cut into pieces of T frames, become the points of ONE sparse
// problem in the layout BasDev reads, and every list of mvs_bas::plan (ba_envelope.hpp) is built on the device.  Two stages
// with one host read of SeqGlobState between them: the first is sized by the sequence alone, the second by the counts.
struct SeqGlobState {
    int32_t n_points, n_obs;
    int64_t pairs;               // sum of t (t - 1) / 2 over the tracks' lengths
    int64_t blocks;              // of the envelope
    int32_t widest, reserved;
};
struct SeqGlobDev {
    SeqWinDev w;                 // the sequence's resident state, the link tables, w_anchor, w_pose, pinfo, oinfo
    int T;                       // max_track_frames: 0 = uncut
    // stage 1
    int32_t *depth;              // [n_frames][N] links behind keypoint i
    int32_t *rank;               // [n_frames][N] in-frame rank of the point whose head keypoint i is, -1: none
    int32_t *oofs;               // [n_frames][N] in-frame offset of that point's observations
    int32_t *fr_points, *fr_nobs, *fr_reach;   // [n_frames] points and observations that start in a frame, the last frame they reach
    int64_t *fr_pairs;           // [n_frames]
    int32_t *pt_base, *ob_base;  // [n_frames] exclusive scans of fr_points / fr_nobs
    int32_t *first, *row_off, *last;   // [n_frames], [n_frames + 1], [n_frames]: the envelope
    SeqGlobState *state;
    // stage 2
    int n_points, n_obs, n_blocks;
    int64_t n_pairs;
    int32_t *kp_obs;             // [n_frames][N] the observation keypoint i makes, -1: none; then every frame's sorted list
    int32_t *obs_off, *head_frame, *head_kp;   // [P + 1], [P], [P]
    int32_t *obs_frame, *obs_point, *obs_kp;   // [O]
    double *obs_uv, *oinfo;      // [O][2], [O][3]
    double *pts0, *pinfo;        // [P][3], [P][6]
    double *pose0, *wts;         // [n_frames][12], [n_frames][6]
    int32_t *fr_cnt, *fr_off, *fr_obs;         // [n_frames], [n_frames + 1], [O]
    int32_t *blk_row, *pair_rel; // [n_blocks]: the row of a block, the offset of its pairs inside the row
    int32_t *row_pairs, *row_base;   // [n_frames], [n_frames + 1]: pairs of a row, their exclusive scan
    int32_t *pair_off, *pair_a, *pair_c;       // [n_blocks + 1], [pairs], [pairs]
};
// links, depths, counts, scans and the envelope: everything SeqGlobState holds
void launch_seq_glob_count(const SeqGlobDev &d, hipStream_t stream);
// the problem (emit) and the plan's lists; kp_obs has been set to -1 by the caller
void launch_seq_glob_build(const SeqGlobDev &d, hipStream_t stream);

// ---- the tracking loop of a resident sequence (mvs_seq_track) -------------------------------------
// Glue between the solvers of one step f (pair k = f - 1), one workgroup each: vo_join_kernel joins pair k's kept points with
// map[f - 1] into frame f's slice of a PnpDev; vo_assemble_kernel reads the PnP result, applies the gates and writes the
// two-frame problem refine_prep_kernel + refine_kernel<2> read; vo_commit_kernel reads the BA result, applies the error gate
// and writes T_last and map[f].  state[0] = 0 once a frame is lost: every later kernel leaves at once.
struct VoDev {
    int n_frames, max_kp;              // the sequence: frames, keypoint capacity N of a frame
    int k0, use_refined, min_pnp_points;
    double max_error, sigma_px, point_var;   // point_var = point_sigma^2
    // resident state of the sequence (mvs_seq_run, mvs_seq_refine_pairs)
    const mvs_pair_result *results;    // [n_frames - 1]
    const mvs_match *matches;          // [n_frames - 1][N]
    const double *points;              // [n_frames - 1][N][3]
    const int32_t *point_idx;          // [n_frames - 1][N]
    const float *kp;                   // [n_frames][N][2]
    const uint8_t *oct;                // [n_frames][N]
    const mvs_refine_result *refined;  // [n_frames - 1], use_refined only
    const double *refined_pts;         // [n_frames - 1][N][3], use_refined only
    // the loop's state
    int32_t *state;                    // {1 while the run goes on, next point id}
    double *T_last;                    // R (9), t (3)
    int64_t *gidx;                     // [n_frames] = f: the sampler key offset of step f's PnP
    // per frame
    mvs_track_frame *frames;           // [n_frames]
    int32_t *map_id;                   // [n_frames][N] -1 = none
    double *map_X;                     // [n_frames][N][3]
    int32_t *n_cand;                   // [n_frames]
    int32_t *cand_a, *cand_b;          // [n_frames][N] keypoints of the candidates in frame f - 1 / f
    double *cand_X, *cand_uv;          // [n_frames][N][3 / 2]: the step's PnP problem
    const PnpOut *pnp_out;             // [n_frames]
    const int32_t *inliers;            // [n_frames][N]
    int32_t *m;                        // [n_frames] points of the step's BA problem
    int32_t *pt_id, *pt_kp;            // [n_frames][N], [n_frames][N][2] = (a, b)
    uint8_t *pt_new;                   // [n_frames][N]: the point has no prior and frame 0 observes it
    double *guess;                     // [n_frames][N][3]
    double *pose0;                     // [n_frames][2][12]
    const mvs_refine_result *ba_out;   // [n_frames][2]
    const double *pts;                 // [n_frames][N][3] refined points
    // one step's inputs of refine_prep_kernel
    double *obs0, *obs1;               // [N][2]
    double *cov0, *cov1;               // [N][4]
    double *cov3;                      // [N][9]
};
void launch_vo_init(const VoDev &d, hipStream_t stream);
void launch_vo_join(const VoDev &d, int f, hipStream_t stream);
void launch_vo_assemble(const VoDev &d, int f, hipStream_t stream);
void launch_vo_commit(const VoDev &d, int f, hipStream_t stream);

// ---- lagged pairs and VisualOdometer::add_frame on a resident sequence (mvs_seq_run_lags, mvs_seq_odometry; DESIGN.md
// section 4.7.3) ------------------------------------------------------------------------------------------------------------
// ssd[k] = sum over the triangulated points j of pair k of the squared Hamming distance of match row point_idx[k][j]
// (image-pair.cpp:166), 0 for an invalid pair.  Grid n_pairs, one workgroup per pair.
void launch_pair_ssd(const mvs_pair_result *results, const mvs_match *matches, const int32_t *point_idx, int n_pairs, int max_kp,
                     int32_t *ssd, hipStream_t stream);
// what the state machine reads of lag d: pair k = (frame k, frame k + d), n_frames - d pairs
struct LagDev {
    const mvs_pair_result *results;    // [n_frames - d]
    const mvs_match *matches;          // [n_frames - d][N]
    const int32_t *point_idx;          // [n_frames - d][N]
    const int32_t *ssd;                // [n_frames - d]
    const mvs_refine_result *refined;  // [n_frames - d]
    const double *refined_pts;         // [n_frames - d][N][3]
};
// the image pair the queue holds for base frame b (ImagePair of m_image_pair_queue)
struct OdoHeld {
    int32_t pair, lag, valid, count, ssd, refined;
    double error;
};
// q = {q0: the oldest frame still queued, segment, lag / base of the pair that initialises this frame, 1: it does}
constexpr int kOdoWords = 8;
struct OdoDev {
    int queue_size, min_inliers;             // Q, min_match_inlier_count
    double max_error, max_rot_sq, max_tz;    // max_rot_sq = max_rotation_magnitude^2
    const LagDev *lags;                      // [Q + 1] device table, entry 0 unused
    int32_t *q;                              // [kOdoWords]
    OdoHeld *held;                           // [n_frames]
    mvs_odo_frame *odo;                      // [n_frames]
};
// The loop of mvs_seq_odometry enqueues, per frame f: the step's kernels of mvs_seq_track (they run while VoDev::state[0] = 1 =
// TRACKING and leave at once otherwise), then vo_queue_kernel (reset() after a lost step, or -- INITIALIZING -- the new pair,
// the update scan, the gates and the choice), then vo_map_init_kernel (the map of the chosen pair; sets state[0] = 1).
// table[lag] = entry, by one thread: the device table of mvs_seq_run_lags is written entry by entry from kernel arguments
void launch_lag_table_set(LagDev *table, int lag, const LagDev &entry, hipStream_t stream);
void launch_vo_odo_begin(const VoDev &d, const OdoDev &o, hipStream_t stream);
void launch_vo_queue(const VoDev &d, const OdoDev &o, int f, hipStream_t stream);
void launch_vo_map_init(const VoDev &d, const OdoDev &o, int f, hipStream_t stream);

// ---- the pose graph of a resident sequence (seq_graph.hip) -------------------------------------
// Candidate slot (d, k), d = 1 .. max_lag, k < n_frames - d, sits at seq_graph_slot_off(n_frames, d) + k: ascending (d, k).
__host__ __device__ constexpr int seq_graph_slot_off(int n_frames, int d) { return (d - 1) * n_frames - d * (d - 1) / 2; }
struct SeqGraphDev {
    int n_frames, max_lag, n_slots;
    int min_points;
    double max_error;
    int chain_on;                      // both chain sigmas > 0
    double chain_var[2];               // sigma^2: rotation, translation
    // resident state of the sequence
    const LagDev *lags;                // [max_lag + 1] device table of mvs_seq_run_lags, entry 0 unused
    const double *traj_R, *traj_t;     // SeqChainDev's outputs
    // per slot (seq_graph_edges_kernel); pose and cov are written for kept slots only
    int32_t *slot_keep, *slot_kind;    // [n_slots]
    double *slot_scale;                // [n_slots]
    double *slot_pose;                 // [n_slots][12]
    double *slot_cov;                  // [n_slots][36]
    // the graph (seq_graph_compact_kernel): E = *n_edges dense entries in slot order
    int32_t *n_edges;                  // [1]
    int32_t *edge_src, *edge_dst, *edge_lag, *edge_kind;   // [n_slots]
    double *edge_scale;                // [n_slots]
    double *edge_pose;                 // [n_slots][12]
    double *edge_cov;                  // [n_slots][36]
    double *node_pose;                 // [n_frames][12]
};
void launch_seq_graph(const SeqGraphDev &g, hipStream_t stream);

// ---- loop closures of a resident sequence (loop.hip, seq_graph.hip) ---------------------------
constexpr int kLoopMaxFrames = 4096;
struct LoopDev {
    int n_frames, max_kp, desc_words;
    // the sequence's frame arrays
    const uint32_t *desc;              // [n_frames][N][desc_words]
    const float *kp;                   // [n_frames][N][2]
    const uint8_t *oct;                // [n_frames][N]
    const int32_t *n_kp;               // [n_frames]
    const double *K, *Kinv;            // [n_frames - 1][9] intrinsics of the sequence's pairs
    int32_t *score;                    // [n_frames][n_frames], row i (base / train), column j (query); zero unless j - i >= min_gap
    // selection (loop_select_rows_kernel, loop_select_compact_kernel)
    int min_score, top_k, max_candidates;
    int32_t *row_n;                    // [n_frames] candidates of query frame j (<= top_k)
    int32_t *row_key;                  // [n_frames][top_k] score << 12 | (4095 - i), descending
    mvs_loop_candidate *cand;          // [max_candidates], rows past the kept count zero
    int32_t *counts;                   // {kept, found}: entries of the list, and of the list before the cut
};
// score[i][j] for every i <= j - min_gap, on a table cleared first (the status is that clear's: nothing is launched if it
// fails).  desc_words 8: the FP4 matrix-core kernel; 4 and 16: popcount
hipError_t launch_loop_scores(const LoopDev &d, double ratio, double max_dist, int min_gap, hipStream_t stream);
void launch_loop_select(const LoopDev &d, hipStream_t stream);
// pair c of `b` (a batch whose pairs own both images) = (frame cand[c].i, frame cand[c].j) for c < counts[0]: descriptors,
// keypoints, octaves, counts, the intrinsics of the sequence's pair i and the sampler key offset c
void launch_loop_gather(const LoopDev &d, const BatchDev &b, hipStream_t stream);
// Appends one edge per accepted candidate behind the *n_built edges of the graph (seq_graph.hip): the rule of
// seq_graph_edges_kernel with (k, k + d) = (i, j), plus var[0] / var[1] on the diagonal where add[0] / add[1]
struct LoopEdgeDev {
    mvs_loop_candidate *cand;          // the list; `accepted` is written
    const int32_t *counts;             // {kept, found}
    const mvs_pair_result *results;    // [max_candidates] of the verification batch
    const mvs_refine_result *refined;  // [max_candidates]
    const int32_t *n_built;            // [1] edges of the built graph
    int max_candidates, min_points;
    double max_error;
    int add[2];
    double var[2];
};
void launch_loop_edges(const SeqGraphDev &g, const LoopEdgeDev &e, hipStream_t stream);

// ---- VisualFeature::extract (row f3): ORB-style extraction for a batch of equally sized images ----------------
constexpr int kOrbMaxLevels = 16;
constexpr int kOrbSelCap = 16384;    // keys of one (image, level) the selection can hold in LDS (128 KB): 2 n_l <= this, or the
                                     // level's candidate list is capped at it (then, and only then, a level can overflow)

struct OrbLevel {
    int w, h;
    int n_keep;        // n_l: keypoints kept at this level
    float scale;       // 1.2^l
    size_t offset;     // pixels of one image's pyramid before this level
    size_t tab_offset; // first entry of this level's resize table (w column entries, then h row entries)
    int cand_cap;      // capacity of the level's candidate list: the non-maximum suppression's own bound (one survivor per 2x2
                       // block of the detection area: the list cannot overflow; round 5 -- 16384 before, MVS_ERR_CAPACITY beyond)
    size_t cand_off;   // first key of the level inside one image's candidate block
};
struct OrbSel {        // a selected keypoint of one level
    int32_t x, y;
    float harris;
};
struct OrbDev {
    int n_images, n_levels, nfeatures, edge, fast_threshold;
    size_t cand_stride;    // keys of one image's candidate block (sum of the levels' cand_cap)
    int flat_order;        // 0: XCD-aware block order of describe_kernel (the product); 1: (level, image, split) as in rounds 2-4 --
                           // only the diagnostics build can set it (MVS_ORB_FLAT_ORDER, tools/profile_extract.sh: the A/B of DESIGN 4.8)
    OrbLevel level[kOrbMaxLevels];
    uint8_t *pyr;          // [level][image][h_l][w_l]; level 0 = the input images
    uint8_t *blur;         // same layout: blurred levels
    const int2 *resize_tab;  // per level >= 1: {source index, 11-bit weight} per destination column and row
    uint64_t *cand_keys;   // [image][cand_stride]: level l at cand_off, cand_cap keys
    int32_t *cand_count;   // [image][level]
    OrbSel *sel;           // [image][level][nfeatures]
    int32_t *sel_count;    // [image][level]
    int32_t *overflow;     // [1] set when a level had more than cand_cap corners (possible only for capped lists, see kOrbSelCap)
    const int8_t *pattern; // [256][4]
    mvs_keypoint *kp;      // [image][nfeatures]
    uint8_t *desc;         // [image][nfeatures][32]
    int32_t *n_kp;         // [image]
    float *kp_xy;          // optional [image][nfeatures][2] (the layout the matcher reads), may be null
    uint8_t *kp_oct;       // optional [image][nfeatures] octave of every keypoint (refinement weights), may be null
};
hipError_t orb_prepare();
void launch_orb(const OrbDev &d, hipStream_t stream);

// ---- single-shot glue: pair 0's scalars as kernel arguments, pair 0's outputs gathered for one device-to-host copy --------
struct SingleParams {
    int32_t n1, n2;
    int64_t gidx;
    double K[9], Kinv[9];
    uint32_t part_bytes[4];   // desc1, desc2, kp1, kp2 of the packed input block (when one is given)
};
struct SingleLayout {
    size_t mask, points, idx, matches, total;
};
// flags: 1 mask, 2 points, 4 point indices, 8 matches
__host__ __device__ inline SingleLayout single_layout(int rows, int flags)
{
    auto up = [](size_t x) { return (x + 15) & ~size_t(15); };
    SingleLayout L;
    size_t o = 512;   // the 368-byte result record
    L.mask = o;
    o += (flags & 1) ? up((size_t)rows) : 0;
    L.points = o;
    o += (flags & 2) ? up((size_t)rows * 24) : 0;
    L.idx = o;
    o += (flags & 4) ? up((size_t)rows * 4) : 0;
    L.matches = o;
    o += (flags & 8) ? up((size_t)rows * 16) : 0;
    L.total = o;
    return L;
}
void launch_single_params(const BatchDev &b, const SingleParams &sp, const void *packed_in, hipStream_t stream);
void launch_single_gather(const BatchDev &b, int rows, int flags, unsigned char *out, hipStream_t stream);

// ---- kernel table (mvs_kernel_info_get) and per-launch timing (mvs_batch_time_kernels) ---------------------------
// One id per kernel of the two-view pipeline.  launch_* record an event in front of every launch when given a
// LaunchTimer, so the per-kernel times of the bench line are measured on the launches' own stream, launch by launch.
enum KernelId : int {
    kKMatchTopk = 0,
    kKMatchCompact,
    kKRansacFused,     // solve + hypothesis-per-lane scoring in one launch (short launches, per-hypothesis tables)
    kKRansacSolve,
    kKRansacSelect,
    kKPairPrepare,     // bounding box of the pair's matches + probe: is this pair pre-screened?
    kKRansacPrescreen, // approximate F + certified band per hypothesis
    kKRansacExactList, // exact solve of the listed hypotheses (flagged by the pre-screen / survivors of the count)
    kKRansacCount2,    // pruned counting with per-hypothesis thresholds (upper / lower bounds of the exact count)
    kKRansacCountPilot,  // ransac_finish_mfma_kernel<., true>: the first kPilotMfmaHyp hypotheses in full -> the pair's first bound
    kKRansacCountMfma,   // dense counting of the points that must be seen before anything can be dropped: split bf16 on the
                         // matrix cores, no exit tests
    kKRansacCountFinish, // the first batch of every pair's list (largest partial counts): upper and lower count bounds, matrix cores
    kKRansacCountFinishRest, // the rest of the list: upper counts completed behind the dense phase's points
    kKRansacSurvivors, // hypotheses whose upper bound reaches the pair's best lower bound -> work list
    kKFinModel,
    kKTriangulate,
    kKFinSelect,
    kKMatchTopkVec,    // match_topk_kernel<8>: the vector 2-NN kernel when a 256-bit launch is too small for the matrix-core one
    kKernelCountProduct,   // the product library's table ends here
    // exists in the diagnostics build (-DMVS_DEBUG_HOOKS) only
    kKRansacCount32 = kKernelCountProduct,   // vector single-precision counting, everything in one launch (mvs_debug_set_count_dense(0))
    kKernelCount
};
struct LaunchTimer {
    hipStream_t stream;
    hipEvent_t *ev;   // cap + 1 events
    int32_t *kid;     // kernel id of launch k
    int cap;
    int n;
    void mark(int id)
    {
        if (n < cap) {
            (void)hipEventRecord(ev[n], stream);
            kid[n] = id;
            ++n;
        }
    }
    void end() { (void)hipEventRecord(ev[n], stream); }
};
struct KernelDesc {
    const char *name;     // as rocprofv3 prints it
    const void *fn;       // host-side handle of the __global__ function
    int threads;          // threads per workgroup as launched
    size_t dynamic_lds;   // bytes of dynamic LDS as launched for `max_kp`
};
// entry `id` of the table for a batch with `max_kp` keypoints per image; false past the end
bool kernel_desc(int id, int max_kp, int desc_words, KernelDesc *out);

// launch wrappers (all asynchronous on `stream`); lt: optional per-launch timer
void launch_match_topk(const BatchDev &b, const RunParams &rp, int n_active, hipStream_t stream, LaunchTimer *lt = nullptr);
void launch_match_compact(const BatchDev &b, const RunParams &rp, int n_active, hipStream_t stream, LaunchTimer *lt = nullptr);
void launch_prep_points(const BatchDev &b, const double *uv1, const double *uv2, int n_active, hipStream_t stream);
// after_dense: recorded on `stream` behind the dense count of the pre-screened stage (the end of its throughput-bound part)
void launch_ransac(const BatchDev &b, const RunParams &rp, int n_active, bool stats, hipStream_t stream, LaunchTimer *lt = nullptr,
                   hipEvent_t after_dense = nullptr);
void launch_finalize(const BatchDev &b, const RunParams &rp, int n_active, int mode, hipStream_t stream, LaunchTimer *lt = nullptr);
// opt-in to > 64 KB of dynamic LDS for the kernels that need it, once per device; hipSuccess or the first error
hipError_t prepare_kernels();
#ifdef MVS_DEBUG_HOOKS
// diagnostics build only (libmvslam_hip_dbg.so): process-global switches, the reference counting kernel, probes, the audit.
// (The experiment ladder of rounds 1-3 and its variant switch are gone from the tree; their code is in git history at 77282af.)
// pair_prepare + ransac_prescreen only, every pair forced into the pre-screened mode
void launch_prescreen_only(const BatchDev &b, const RunParams &rp, int n_active, int mode, hipStream_t stream);
void launch_mfma_probe(const uint16_t *A, const uint16_t *B, float *out, hipStream_t stream);
void set_count_dense(int v);      // 1 = single-precision counting as pilot + dense MFMA phase + finish (the product), 0 = one
                                  // ransac_count32 launch, 2 = ransac_count32 as the finish; 1000 + margin, 100000 + pilot size
void set_match_mfma(int v);       // 1 (default) 256-bit descriptors on the matrix cores by batch size, 0 the VALU kernel
void set_prescreen_force(int m);   // -1 probe decides (default), 0 every pair exact, 1 every pair pre-screened
hipError_t prescreen_fallback_waves(unsigned int *out, bool reset);   // wavefronts that took the guarded normalisation
void set_split_min_pairs(int v);  // launches with fewer pairs stay on the fused hypothesis-per-lane kernel (default 3)
void launch_fastmath_check(const double *x, const double *y, int n, unsigned long long *out, hipStream_t stream);
void launch_pairstep_check(const double *rows, int n, unsigned long long *out, hipStream_t stream);
// full-population audit of the pre-screened stage (kernels.hip: audit_kernel); out: 16 counters, maxc: [n_active]
void launch_count_only(const BatchDev &b, const RunParams &rp, int n_active, int pmode, int dense, const int32_t *keep,
                       hipStream_t stream);
void launch_indicator_probe(const float *a, const float *tu, const float *tl, const float *T, int n, float *ind_u, float *ind_l,
                            float *scale, hipStream_t stream);
void launch_rounding_probe(const double *in, int n, double *out, hipStream_t stream);
hipError_t launch_audit(const BatchDev &b, const RunParams &rp, int n_active, int phase, unsigned long long *out, int32_t *maxc,
                        hipStream_t stream);
#endif
void launch_fundamental(const double *p1, const double *p2, double *F, int *ok, hipStream_t stream);

// ---- five-point essential-matrix RANSAC (essential5.hip) ----------------------------------------
constexpr int kE5MaxRoots = 10;      // models of one hypothesis (five_point.hpp)
constexpr int kE5HypPerBlock = 64;   // hypotheses per workgroup of the solve + count kernel: one per lane of a wavefront
// opt-in to the kernels' LDS workspaces (> 64 KB), once per device
hipError_t essential5_prepare();
// pairs [0, n_active): every hypothesis solved and counted on the pair's resident normalised points, then the selection, which
// writes results[p].{best_hyp, best_count, best_residual, F, E} and the mask (rows past M cleared); launch_finalize with
// kFinalizeEssential completes the record.  n_roots: [P][h_stride], count: [P][h_stride][10] (-1 past n_roots);
// best_root: [P] root index of the winner (-1: none).  confidence: 0 = every hypothesis runs; in (0, 1) = the termination rule of
// five_point.hpp, applied per pair at the checkpoints 64, 128, ... by one round of launches each (no host synchronisation).
// n_run: [P], always written: the hypotheses each pair ran -- the checkpoint it stopped at, or with confidence 0 all of them
// (0: fewer than eight matches); rows >= n_run of the tables are not defined.  c_max: [P] scratch of the rounds, untouched with
// confidence 0, when the stage is two launches: solve + count (four wavefronts count each workgroup's 64 hypotheses) and the
// selection
void launch_essential5(const BatchDev &b, const RunParams &rp, int n_active, int32_t *n_roots, int32_t *count, int h_stride,
                       int32_t *best_root, int32_t *n_run, int32_t *c_max, double confidence, hipStream_t stream);
// the minimal solver alone: p1 / p2 5 x (x, y), E [10][9], n
void launch_five_point(const double *p1, const double *p2, double *E, int *n, hipStream_t stream);

}  // namespace mvs
