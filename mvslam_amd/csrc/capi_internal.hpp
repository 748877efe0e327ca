// capi_internal.hpp -- what the host files of libmvslam_hip.so (capi.hip, capi_orb.hip, capi_graph.hip, capi_ba.hip, capi_debug.hip) share:
// the owners of device memory, the three opaque objects of include/mvslam_hip.h, HIP_TRY and the helpers that cross a file
// boundary.  A helper that one file uses is static in that file and is not declared here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "kernels.hpp"

using namespace mvs;   // every host file speaks of the kernels' records (BatchDev, PnpDev, ...) unqualified

// ---- device memory: every block has one owner, whose destructor frees it ---------------------------------------------
struct HipFree {
    void operator()(void *p) const { (void)hipFree(p); }
};
using DevPtr = std::unique_ptr<void, HipFree>;
// the blocks of a batch, a sequence or a probe's temporaries, allocated group by group (DevGroup)
using DevBlocks = std::vector<DevPtr>;
// one grow-only workspace of a context (ws_grow)
struct DevWorkspace {
    DevPtr p;
    size_t bytes = 0;
    template <typename T = char>
    T *ptr() const { return static_cast<T *>(p.get()); }
};

struct mvs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // second queue of a large batch: its pairs go down the pipeline as two independent halves, one per lane (`stream` and
    // `side`), so that the latency-bound kernels of one half (list sort, exact solve of the few survivors, selection, ...) run
    // under the throughput-bound kernels of the other -- and, while nothing else uses the context, under those of the NEXT
    // call: a halves run leaves the side lane open (enqueue_pipeline) and whatever uses the context's stream next joins it
    // (ctx_stream).  Nothing but ctx_stream, enqueue_pipeline, close_lane and create / destroy reads `stream` or `side`.
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_dense[2]{};   // recorded behind a lane's dense count: the other lane's next throughput section waits for it
    bool lane_open = false;                 // work of a halves run is on `side` that `stream` has not joined yet
    const mvs_batch *lane_batch = nullptr;  // the open lane's batch and pairs: only the same run again leaves it open
    int lane_pairs = 0;
    // the caller can enqueue work of their own on the stream (it is theirs, or mvs_ctx_stream has handed it out): every halves
    // run joins before it returns, "the caller sees one stream"
    bool caller_sees_stream = false;
    bool half_batches = true;
    double e5_confidence = 0.0;   // mvs_ctx_set_essential_confidence: 0 = every hypothesis of the five-point RANSAC runs
    int pg_solver = MVS_PG_SOLVER_PCG;   // mvs_ctx_set_pose_graph_solver: the linear solver of the pose graphs' large path
    // mvs_ctx_set_pose_graph_loss: the robust loss of the pose graphs' edges from pg_loss_first on (-1: the loop edges of a
    // resident graph), its constant
    int pg_loss = MVS_PG_LOSS_NONE;
    double pg_loss_k = 1.0;
    int32_t pg_loss_first = 0;
    // mvs_ctx_set_ba_loss: the robust loss of the observation terms of mvs_ba_refine_sparse and mvs_seq_refine_global, its constant
    int ba_loss = MVS_BA_LOSS_NONE;
    double ba_loss_k = 1.0;
    bool pgd_ran = false;               // a graph has gone through the direct solver: pgd_info is that of the last one
    mvs_pose_graph_direct_info pgd_info{};
    // n_run of the last single-shot five-point call: none yet, or that call failed before its RANSAC was enqueued (-1); in
    // e5_single_run (0: the host returned before the RANSAC -- fewer than eight matches, so 0 -- or the word was saved from a
    // scratch batch that has been replaced since); in scratch->e5_nrun[0] (1: the call enqueued its RANSAC)
    int e5_single = -1;
    int32_t e5_single_run = 0;
    int cu_count = 256;   // hipDeviceAttributeMultiprocessorCount of `device` (mvs_ctx_create); MI355X: 256
    std::string err;
    mvs_batch *scratch = nullptr;  // batch of one pair backing the single-shot entry points
    // workspaces, freed by their destructors
    DevWorkspace uv;          // image points of a single-shot call: [max_kp][2] of camera 1, then the same of camera 2
    DevWorkspace small;       // 128 doubles of staging (fundamental_kernel, five_point_kernel)
    DevWorkspace single;      // gathered outputs of a single-shot call (one device-to-host copy)
    DevWorkspace single_in;   // packed inputs of mvs_image_pair (one host-to-device copy)
    DevWorkspace pnp;         // pnp_solve workspace
    DevWorkspace ref;         // sfm_refine / pnp_refine workspace
    DevWorkspace win;         // mvs_ba_refine_windows workspace
    DevWorkspace pg;          // mvs_pose_graph_optimize workspace
    DevWorkspace pgm;         // mvs_pose_graph_marginals workspace: uploads, lists, the skyline, the solves' y
    DevWorkspace bas;         // mvs_ba_refine_sparse workspace: uploads, lists, linearisation, the skyline (capi_ba.hip)
    DevWorkspace orb;         // extraction workspace: orb_graph points into it
    int32_t *h_orb_ovf = nullptr;   // pinned: the extraction's overflow flag travels with the outputs (one stream wait per call)
    bool orb_ready = false;
    // the ~50 launches of one extraction, captured once per (batch shape, parameters, buffers) and replayed
    hipGraphExec_t orb_graph = nullptr;
    OrbDev orb_graph_key{};
    bool orb_graph_valid = false;
    // pinned staging arena of the single-shot entry points: small parameters and results travel through it with
    // hipMemcpyAsync on the ctx stream (no synchronous pageable copies, no sync "so that a stack temporary may die")
    char *h_pin = nullptr;
    size_t h_pin_cap = 0, h_pin_off = 0;
    bool pin_in_flight = false;   // an asynchronous copy may still be reading / writing the arena (set by pin_get, cleared
                                  // by whoever synchronises the stream at the end of the call)
};

struct mvs_seq;

struct mvs_batch {
    mvs_ctx *ctx = nullptr;
    BatchDev d{};
    DevBlocks blocks;
    double *uv1 = nullptr, *uv2 = nullptr;   // [n_pairs][max_kp][2] staging of mvs_batch_run_points (first use)
    // the optional per-hypothesis tables of mvs_ransac_fundamental (d.hyp_count / d.hyp_residual during that call only)
    int hyp_table_cap = 0;
    int32_t *hyp_table_count = nullptr;
    double *hyp_table_residual = nullptr;
    // tables of the five-point RANSAC (essential5.hip), sized for the largest hypothesis count seen so far (first use)
    int e5_cap = 0;
    int32_t *e5_nroots = nullptr;   // [n_pairs][e5_cap]
    int32_t *e5_count = nullptr;    // [n_pairs][e5_cap][10]
    int32_t *e5_root = nullptr;     // [n_pairs] root index of the winner
    int32_t *e5_nrun = nullptr;     // [n_pairs] hypotheses each pair ran: the checkpoint it stopped at, or all / none of them
    int32_t *e5_cmax = nullptr;     // [n_pairs] largest count so far, between the rounds of a call with a confidence level
    // the last five-point call on this batch (mvs_batch_download_hypotheses_run): its pairs and hypotheses
    bool e5_ran = false;
    int e5_last_n = 0, e5_last_H = 0;
    hipEvent_t ev[8]{};
    RefineDev refine{};     // allocated by the first mvs_batch_refine
    bool refine_ran = false;
    // pinned staging of the per-pair parameters derived on the host (K^-1, default indices): two slot sets used in turn,
    // each guarded by an event recorded behind its copies, so an asynchronous upload waits for the copies of the upload
    // before last at most -- never for the kernels or downloads queued on the stream in between
    char *h_pin = nullptr;
    hipEvent_t pin_ev[2]{};
    bool pin_ev_live[2] = {false, false};
    int pin_turn = 0;
};

struct mvs_seq {
    mvs_ctx *ctx = nullptr;
    mvs_batch *batch = nullptr;  // n_frames - 1 pairs viewing the frame arrays
    int n_frames = 0, n_tracks = 0, stride = 0;
    SeqJoinDev join{};
    PnpDev pnp{};
    SeqChainDev chain{};
    RefineDev refit{};          // pnp_solve's refit over the inliers of every track (mvs_pnp_params.refit), allocated on demand
    bool refit_on = false;
    DevBlocks blocks;
    bool ran = false;           // mvs_seq_run has filled the pairs, the tracks and the trajectory
    // mvs_seq_rescale: the step records [n_tracks], resident until the next run
    mvs_seq_scale_step *scale_steps = nullptr;
    bool rescaled = false;      // the records are those of a rescale of the last run
    // mvs_seq_refine_windows: link tables, the windows' problems and their results, resident until the next call
    DevWorkspace win;
    SeqWinDev wd{};             // n_windows = 0 until the first call
    WinDev ws{};
    // mvs_seq_track: every per-frame buffer of the tracking loop and one step's solver scratch, resident until the next call
    DevWorkspace trk;
    VoDev vo{};
    bool track_ran = false;
    bool refined_ran = false;   // mvs_seq_refine_pairs has refined the pairs of the LAST run (use_refined_init reads them)
    // mvs_seq_run_lags: one batch per lag d >= 2 viewing the frame arrays (lag_batch[d], entries 0 and 1 stay null), the
    // device table of what the state machine reads of every lag and the per-pair descriptor SSDs, resident until the next run
    std::vector<mvs_batch *> lag_batch;
    DevWorkspace lagws;         // LagDev[lag_cap + 1], then int32 ssd[lag_cap + 1][n_frames]
    int lag_cap = 0;
    std::vector<LagDev> lag_host;   // the table's host copy (the downloads read the ssd pointers from it)
    int lags_ran = 0;           // lags 1 .. lags_ran are resident from one mvs_seq_run_lags since the last run
    bool odo_ran = false;       // the resident tracking results are mvs_seq_odometry's
    OdoDev odo{};
    // mvs_seq_build_pose_graph: the candidate slots, the graph and the optimised nodes, resident until the next run
    DevWorkspace graph;
    SeqGraphDev gd{};
    double *graph_opt_pose = nullptr;   // [n_frames][12] in `graph`
    bool graph_built = false;   // the graph is that of the last run and its lags
    bool graph_opt = false;     // mvs_seq_optimize_pose_graph has succeeded on it
    // mvs_seq_optimize_pose_graph_sim3: the Sim(3) optimised nodes [n_frames][13]; graph_sim3 only while graph_built
    DevWorkspace graph_s3;
    bool graph_sim3 = false;    // it has succeeded on the current graph (a build or added loop edges clear it)
    int graph_edge_cap = 0;     // rows of the graph's edge arrays: the build's slots, plus room for loop edges
    int32_t *graph_n_built = nullptr;   // [1] in `graph`: edges of the built graph, behind which the loop edges go
    // loop closures (mvs_seq_loop_scores .. mvs_seq_add_loop_edges): the score table, the selection's block (counts,
    // per-frame rows, the list) and the batch that verifies the candidates, created at the first
    // verification and replaced when max_candidates changes
    DevWorkspace loop_score, loop_sel;
    LoopDev ld{};
    mvs_batch *loop_batch = nullptr;
    int loop_kept = 0;                 // candidates the last verification ran on
    bool loop_scored = false, loop_selected = false;
    bool loop_verified = false;        // the batch holds the results of the current list
    bool loop_edges_added = false;     // the graph's edges past *graph_n_built are loop edges
    // mvs_seq_refine_global (capi_ba.hip): the link tables and counts (glob_tab, sized by the sequence alone), then the problem,
    // the plan and the solver's arrays (glob, sized by the counts), resident until the next call or run
    DevWorkspace glob_tab, glob;
    SeqGlobDev gl{};
    BasDev glob_bas{};                 // the solver's view of `glob`
    int glob_cur = 0;                  // which of glob_bas.pose / pts holds the estimate
    bool glob_counted = false;         // gl holds the counts of the last call
    bool glob_built = false;           // ... and the problem and the plan have been built from them
    bool glob_solved = false;          // ... and the solver has run on them: glob_res is its record
    bool glob_cov = false;             // the covariance sweep has run at the estimate
    mvs_ba_sparse_result glob_res{};
};

#define HIP_TRY(ctx_, expr)                                                                    \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            if (ctx_)                                                                          \
                (ctx_)->err = std::string(#expr) + ": " + hipGetErrorString(e_);               \
            return MVS_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

// One all-or-nothing group of device blocks for an owner.  add() allocates max(count, 1) elements for a destination
// pointer (nothing more after a failure); commit() then either reports the failure -- the partial blocks are freed, no
// pointer has changed -- or points every destination at its new block, hands the blocks to the owner and only then frees
// the owner's blocks they supersede (the stream must be idle for that).
class DevGroup {
public:
    DevGroup(mvs_ctx *ctx, DevBlocks &owner) : ctx_(ctx), owner_(owner) {}
    template <typename T>
    DevGroup &add(T *&dst, size_t count)
    {
        void *p = nullptr;
        if (e_ == hipSuccess && (e_ = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T))) == hipSuccess)
            parts_.emplace_back(DevPtr(p), [&dst](void *q) -> const void * {
                const void *old = dst;
                dst = static_cast<T *>(q);
                return old;
            });
        return *this;
    }
    mvs_status commit()
    {
        if (e_ != hipSuccess) {
            ctx_->err = std::string("hipMalloc: ") + hipGetErrorString(e_);
            return MVS_ERR_HIP;
        }
        std::vector<const void *> old;
        for (auto &part : parts_) {
            old.push_back(part.second(part.first.get()));
            owner_.push_back(std::move(part.first));
        }
        for (const void *o : old)
            for (auto it = owner_.begin(); o && it != owner_.end(); ++it)
                if (it->get() == o) {
                    owner_.erase(it);
                    break;
                }
        return MVS_OK;
    }

private:
    mvs_ctx *ctx_;
    DevBlocks &owner_;
    hipError_t e_ = hipSuccess;
    std::vector<std::pair<DevPtr, std::function<const void *(void *)>>> parts_;
};

// Layout of a workspace as consecutive parts: take() returns the offset of the next part, rounded up to `align` (a power of
// two); end is where the last part ends, total() the same rounded up.
struct Carve {
    size_t align, end = 0;
    size_t up(size_t x) const { return (x + align - 1) & ~(align - 1); }
    size_t take(size_t bytes)
    {
        const size_t o = up(end);
        end = o + bytes;
        return o;
    }
    size_t total() const { return up(end); }
};

// ---- helpers that cross a file boundary ---------------------------------------------------------------------------------
// Hidden: none of them enters the dynamic symbol table of the library (tests/test_abi.py looks).  Each is defined, with its
// comment, in the file named above it as mvs_host::name.
namespace mvs_host __attribute__((visibility("hidden"))) {

// PinholeCamera caches K.inverse() (vision/camera.cpp:16): fixed-size 3x3 cofactor inverse,
// inv(r, c) = cofactor(c, r) * (1 / det), det expanded along the first column.
inline void mat3_inverse(const double *K, double *inv)
{
    auto m = [&](int r, int c) { return K[(r % 3) * 3 + (c % 3)]; };
    auto cof = [&](int i, int j) { return m(i + 1, j + 1) * m(i + 2, j + 2) - m(i + 1, j + 2) * m(i + 2, j + 1); };
    const double c00 = cof(0, 0), c10 = cof(1, 0), c20 = cof(2, 0);
    const double det = (c00 * K[0] + c10 * K[3]) + c20 * K[6];
    const double invdet = 1.0 / det;
    inv[0] = c00 * invdet;       inv[1] = c10 * invdet;       inv[2] = c20 * invdet;
    inv[3] = cof(0, 1) * invdet; inv[4] = cof(1, 1) * invdet; inv[5] = cof(2, 1) * invdet;
    inv[6] = cof(0, 2) * invdet; inv[7] = cof(1, 2) * invdet; inv[8] = cof(2, 2) * invdet;
}

inline bool affine_K(const double *K) { return K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && K[0] != 0.0 && K[4] != 0.0; }

// capi.hip
hipError_t close_lane(mvs_ctx *ctx);
// The context's stream, for every use but the halves path of enqueue_pipeline: an open side lane is joined into it first, so
// that whatever the caller enqueues, records or waits for on the returned stream is behind both halves.
inline hipStream_t ctx_stream(mvs_ctx *ctx)
{
    if (ctx->lane_open)
        (void)close_lane(ctx);   // without an event edge it has waited for the lane on the host: joined either way
    return ctx->stream;
}
hipError_t sync_stream(mvs_ctx *ctx);
mvs_status ws_grow(mvs_ctx *ctx, DevWorkspace &w, size_t bytes, size_t floor = 0);
void drop_orb_graph(mvs_ctx *ctx);
RunParams to_run(const mvs_params &p);
mvs_status ensure_groups(mvs_batch *b, int num_hypotheses);
enum class Estimator { kEightPoint, kFivePoint };   // the model stage of a pair pipeline: kernels.hip or essential5.hip
mvs_status ensure_tables(mvs_batch *b, Estimator est, int num_hypotheses);
mvs_status batch_create_impl(mvs_ctx *ctx, int n_pairs, int max_kp, int desc_bytes, int n_frames, mvs_batch **out,
                             const BatchDev *frames_of = nullptr, int lag = 1);
mvs_status check_params(const mvs_params *p);
mvs_status run_pairs(mvs_batch *b, Estimator est, const RunParams &rp, int n);
bool refine_params_ok(const mvs_refine_params *p);
void obs_cov_to_info(const double *cv, double *o);
void point_cov_to_info(const double *C, double *L);

// capi_orb.hip
mvs_status orb_run(mvs_ctx *ctx, const uint8_t *images, int n, int w, int h, const mvs_orb_params &prm, uint8_t *d_desc_ext,
                   float *d_kp_xy_ext, int32_t *d_n_ext, OrbDev &d, uint8_t *d_kp_oct_ext = nullptr, bool wait = true);

}  // namespace mvs_host

