// capi.hip -- host side of libmvslam_hip.so: contexts, resident batches, the C ABI of include/mvslam_hip.h.  Extraction is
// in capi_orb.hip, the back end (pose graphs, marginals, loop closures) in capi_graph.hip, the mvs_debug_* hooks of the
// diagnostics library in capi_debug.hip; capi_internal.hpp holds what they share.
// No CPU fallback exists anywhere in these files: every entry point ends in a HIP kernel launch.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "capi_internal.hpp"

using namespace mvs_host;

// Joins the open side lane of a halves run into the context's stream (enqueue_pipeline leaves it open; ctx_stream is the one
// caller outside it).  Whatever fails, nothing is left running unjoined: without an event edge the lane is waited for on the
// host -- a later download or a release of the groups must never race with the second half.
hipError_t mvs_host::close_lane(mvs_ctx *ctx)
{
    if (!ctx->lane_open)
        return hipSuccess;
    ctx->lane_open = false;
    ctx->lane_batch = nullptr;
    hipError_t e = hipEventRecord(ctx->ev_join, ctx->side);
    if (e == hipSuccess)
        e = hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
    if (e != hipSuccess)
        (void)hipStreamSynchronize(ctx->side);
    return e;
}

// every wait for the ctx stream goes through here (an open side lane is joined first: ctx_stream): once it has drained nothing
// reads or writes the arena any more
hipError_t mvs_host::sync_stream(mvs_ctx *ctx)
{
    const hipError_t e = hipStreamSynchronize(ctx_stream(ctx));
    if (e == hipSuccess)
        ctx->pin_in_flight = false;
    return e;
}
// ---- pinned staging arena -------------------------------------------------------------------------------------------
// pin_begin() opens a call: the arena is made large enough for everything the call will stage (growing it waits for
// the stream first, nothing of an earlier call may still be in flight) and the cursor rewinds.  pin_put() copies a host
// block in and returns its pinned address, pin_get() reserves room for a device -> host copy.
static mvs_status pin_begin(mvs_ctx *ctx, size_t bytes)
{
    bytes += 4096;
    if (ctx->h_pin_cap < bytes) {
        HIP_TRY(ctx, sync_stream(ctx));
        if (ctx->h_pin)
            (void)hipHostFree(ctx->h_pin);
        ctx->h_pin = nullptr;
        ctx->h_pin_cap = 0;
        const size_t cap = std::max<size_t>(bytes * 2, size_t(1) << 20);
        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_pin, cap, hipHostMallocDefault));
        ctx->h_pin_cap = cap;
    }
    if (ctx->pin_in_flight) {
        // the previous call left through an error path after it had enqueued copies from / into the arena: wait for
        // them before the cursor rewinds and their source bytes are overwritten
        HIP_TRY(ctx, sync_stream(ctx));
        ctx->pin_in_flight = false;
    }
    ctx->h_pin_off = 0;
    return MVS_OK;
}
static void *pin_get(mvs_ctx *ctx, size_t bytes)
{
    const size_t off = (ctx->h_pin_off + 63) & ~size_t(63);
    if (off + bytes > ctx->h_pin_cap)
        return nullptr;   // pin_begin() was given too small a figure: a bug, reported as MVS_ERR_HIP by the callers
    ctx->h_pin_off = off + bytes;
    ctx->pin_in_flight = true;
    return ctx->h_pin + off;
}
static void *pin_put(mvs_ctx *ctx, const void *src, size_t bytes)
{
    void *p = pin_get(ctx, bytes);
    if (p && bytes)
        std::memcpy(p, src, bytes);
    return p;
}
#define PIN_TRY(ctx_, ptr_)                                   \
    do {                                                      \
        if (!(ptr_)) {                                        \
            (ctx_)->err = "pinned staging arena exhausted";   \
            return MVS_ERR_HIP;                               \
        }                                                     \
    } while (0)
// host block -> pinned arena -> device, asynchronous
static mvs_status up_async(mvs_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    void *p = pin_put(ctx, src, bytes);
    PIN_TRY(ctx, p);
    HIP_TRY(ctx, hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, ctx_stream(ctx)));
    return MVS_OK;
}

// pnp_solve's refit (pnp-solve.cpp:53-64) as a refinement problem: points fixed (sigma 1e-9), no prior on the pose
constexpr double kRefitPointSigma = 1e-9, kRefitPoseSigma = 1e6;
static RefineCfg to_cfg(const mvs_refine_params &p, int n_frames);

// the refit's parameters: the defaults with no prior on the pose; its configuration as a one-frame problem
static mvs_refine_params refit_params()
{
    mvs_refine_params rp;
    mvs_refine_params_default(&rp);
    rp.pose_sigma[0] = rp.pose_sigma[1] = kRefitPoseSigma;
    return rp;
}
static RefineCfg refit_cfg() { return to_cfg(refit_params(), 1); }

static bool pnp_params_ok(const mvs_pnp_params *p)
{
    return p && p->num_hypotheses >= 1 && p->reproj_error > 0.0 &&   // pnp-solve.cpp:13,22-23 (assert)
           (p->sampler == MVS_SAMPLER_IDENTITY || p->sampler == MVS_SAMPLER_PHILOX);
}

// record groups of a PnP RANSAC: one per 256 hypotheses (pnp.hip)
static int pnp_groups(const mvs_pnp_params &p) { return (p.num_hypotheses + 255) / 256; }

// the parameters' share of a PnP problem; max_groups is the size of the caller's records and is set where they are laid out
static void set_pnp_params(PnpDev &d, const mvs_pnp_params &p)
{
    d.num_hypotheses = p.num_hypotheses;
    d.sampler = p.sampler;
    d.min_inliers = p.min_inliers;
    d.seed = p.seed;
    d.thr2 = p.reproj_error * p.reproj_error;
}

RunParams mvs_host::to_run(const mvs_params &p)
{
    RunParams r;
    r.ratio = p.ratio;
    r.max_dist = p.max_dist;
    r.max_error_sq = p.max_error_sq;
    r.num_hypotheses = p.num_hypotheses;
    r.sampler = p.sampler;
    r.seed = p.seed;
    r.min_inliers = p.min_inliers;
    return r;
}

// Grows a context workspace to at least `bytes` (first size: max(bytes, floor)).  Growing waits for the ctx stream, frees
// the old block and marks the workspace empty before it allocates: a failed growth leaves no block behind.
mvs_status mvs_host::ws_grow(mvs_ctx *ctx, DevWorkspace &w, size_t bytes, size_t floor)
{
    if (w.bytes >= bytes)
        return MVS_OK;
    HIP_TRY(ctx, sync_stream(ctx));
    w.p.reset();
    w.bytes = 0;
    void *p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, std::max(bytes, floor)));
    w.p.reset(p);
    w.bytes = std::max(bytes, floor);
    return MVS_OK;
}

// the captured extraction graph points into the extraction workspace: dropped before that block is freed or replaced
void mvs_host::drop_orb_graph(mvs_ctx *ctx)
{
    if (ctx->orb_graph)
        (void)hipGraphExecDestroy(ctx->orb_graph);
    ctx->orb_graph = nullptr;
    ctx->orb_graph_valid = false;
}

// per-hypothesis buffers of the RANSAC stage, sized for the largest hypothesis count seen so far: one group, so a failed
// allocation leaves the batch as it was; the superseded blocks are freed at once: 77 B x hypotheses x pairs is 2 GB at the
// bench size.
mvs_status mvs_host::ensure_groups(mvs_batch *b, int num_hypotheses)
{
    const int G = (num_hypotheses + kHypPerBlock - 1) / kHypPerBlock;
    if (G <= b->d.max_groups)
        return MVS_OK;
    HIP_TRY(b->ctx, sync_stream(b->ctx));
    const size_t P = (size_t)b->d.n_pairs, Hp = (size_t)G * kHypPerBlock;
    if (P * Hp >= (size_t(1) << 32))
        return MVS_ERR_CAPACITY;   // the exact solve's work list holds flat 32-bit record indices
    BatchDev &d = b->d;
    DevGroup g(b->ctx, b->blocks);
    g.add(d.wgbest, P * G);
    g.add(d.hyp_F, P * kHypRec * Hp);       // record of every hypothesis (F + counting threshold): 80 B x hypotheses x pairs
    g.add(d.hyp_r32, P * kHypRec32 * Hp);   // single-precision pre-screen records (mode 1): 48 B x hypotheses x pairs
    g.add(d.hyp_okf, P * Hp);
    g.add(d.hyp_cnt, P * Hp);
    g.add(d.xlist, P * Hp);
    g.add(d.clist, 2 * P * Hp);   // the list + its sorted copy
    if (!d.bound) g.add(d.bound, P);
    if (!d.box) g.add(d.box, P * kBoxRec);
    if (!d.mode) g.add(d.mode, P);
    if (!d.dense_n1) g.add(d.dense_n1, P);
    if (!d.ccount) g.add(d.ccount, P);
    if (!d.pcount) g.add(d.pcount, P);
    if (!d.cpos) g.add(d.cpos, P * kSortBins);
    if (!d.m0list) g.add(d.m0list, 2 * (P + 1));   // one list per half (batch_view)
    if (!d.xcount) g.add(d.xcount, 4);
    const mvs_status st = g.commit();
    if (st != MVS_OK)
        return st;
    d.clist2 = d.clist + P * Hp;
    d.max_groups = G;
    return MVS_OK;
}

// the tables of the five-point stage: one group, so a failed allocation leaves the batch as it was
static mvs_status ensure_e5(mvs_batch *b, int num_hypotheses)
{
    if (num_hypotheses <= b->e5_cap)
        return MVS_OK;
    HIP_TRY(b->ctx, sync_stream(b->ctx));
    const size_t P = (size_t)b->d.n_pairs, H = (size_t)num_hypotheses;
    DevGroup g(b->ctx, b->blocks);
    g.add(b->e5_nroots, P * H);
    g.add(b->e5_count, P * H * kE5MaxRoots);
    const bool first = !b->e5_root;
    if (first)
        g.add(b->e5_root, P).add(b->e5_nrun, P).add(b->e5_cmax, P);
    const mvs_status st = g.commit();
    if (st != MVS_OK)
        return st;
    b->e5_cap = num_hypotheses;
    return MVS_OK;
}

// The model stage in front of the shared tail (decomposition, triangulation): the 8-point RANSAC of kernels.hip or the
// five-point one of essential5.hip (Estimator: capi_internal.hpp).  Everything the two differ in on the host is in the two
// functions below and in run_pairs.
mvs_status mvs_host::ensure_tables(mvs_batch *b, Estimator est, int num_hypotheses)
{
    switch (est) {
    case Estimator::kEightPoint: return ensure_groups(b, num_hypotheses);
    case Estimator::kFivePoint: return ensure_e5(b, num_hypotheses);
    }
    return MVS_ERR_INVALID_ARG;
}

// model stage + its finalize mode for pairs [0, n) on the ctx stream, plain launches (the tables are grown: ensure_tables)
static void enqueue_model(mvs_batch *b, Estimator est, const RunParams &rp, int n)
{
    hipStream_t s = ctx_stream(b->ctx);
    switch (est) {
    case Estimator::kEightPoint:
        launch_ransac(b->d, rp, n, false, s);
        launch_finalize(b->d, rp, n, kFinalizeFull, s);
        break;
    case Estimator::kFivePoint:
        launch_essential5(b->d, rp, n, b->e5_nroots, b->e5_count, b->e5_cap, b->e5_root, b->e5_nrun, b->e5_cmax,
                          b->ctx->e5_confidence, s);
        b->e5_ran = true;
        b->e5_last_n = n;
        b->e5_last_H = rp.num_hypotheses;
        if (b == b->ctx->scratch)
            b->ctx->e5_single = 1;
        launch_finalize(b->d, rp, n, kFinalizeEssential, s);
        break;
    }
}

// the device arrays of `problems` refinement problems of `stride` points seen by `frames` frames (two: the batch's
// problems, with marginal covariances; one: a sequence's refit), allocated as one group; K is the caller's
static mvs_status alloc_refine(mvs_ctx *ctx, DevBlocks &owner, RefineDev &d, int problems, int stride, int frames,
                               const double *K)
{
    const size_t T = problems, S = stride;
    RefineDev r{};
    r.n_problems = problems;
    r.stride = stride;
    r.n_frames = frames;
    r.K = K;
    DevGroup g(ctx, owner);
    for (int f = 0; f < frames; ++f) {
        g.add(r.obs[f], T * S * 2);
        g.add(r.oinfo[f], T * S * 3);
    }
    g.add(r.pts0, T * S * 3);
    g.add(r.pinfo, T * S * 6);
    g.add(r.pts, T * S * 3);
    g.add(r.pts_tmp, T * S * 3);
    if (frames == 2)
        g.add(r.point_cov, T * S * 9);
    g.add(r.pose0, T * 12);
    g.add(r.m, T);
    g.add(r.out, T);
    const mvs_status st = g.commit();
    if (st != MVS_OK)
        return st;
    // rows [m, stride) of a problem are never written: zero, so that a download is the same bytes wherever the block came from
    HIP_TRY(ctx, hipMemsetAsync(r.pts, 0, T * S * 3 * sizeof(double), ctx_stream(ctx)));
    if (r.point_cov)
        HIP_TRY(ctx, hipMemsetAsync(r.point_cov, 0, T * S * 9 * sizeof(double), ctx_stream(ctx)));
    d = r;
    return MVS_OK;
}

extern "C" {

int mvs_abi_version(void) { return MVS_ABI_VERSION; }

const char *mvs_status_str(mvs_status s)
{
    switch (s) {
    case MVS_OK: return "ok";
    case MVS_NO_MODEL: return "no model (reference: return false)";
    case MVS_ERR_INVALID_ARG: return "invalid argument (reference: assert)";
    case MVS_ERR_NO_DEVICE: return "no HIP device";
    case MVS_ERR_HIP: return "HIP runtime error";
    case MVS_ERR_CAPACITY: return "capacity exceeded";
    case MVS_ERR_BAD_INTRINSICS: return "camera intrinsics must be affine (last row 0 0 1)";
    }
    return "unknown";
}

const char *mvs_last_error(const mvs_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

mvs_status mvs_params_default(mvs_params *p)
{
    if (!p)
        return MVS_ERR_INVALID_ARG;
    p->ratio = 0.7;          // visual-feature.cpp:23
    p->max_dist = 10.0;      // image-pair.cpp:22-23
    p->max_error_sq = 0.0;   // derive from K (sfm-solve.cpp:311)
    p->num_hypotheses = 1;   // sfm-solve.cpp:67
    p->sampler = MVS_SAMPLER_IDENTITY;
    p->seed = 0;
    p->min_inliers = 8;      // sfm-solve.cpp:20-21
    p->reserved = 0;
    return MVS_OK;
}

mvs_status mvs_ctx_create_on_stream(int device_id, void *hip_stream, mvs_ctx **out)
{
    if (!out)
        return MVS_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return MVS_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *c = new mvs_ctx();
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) {
        delete c;
        return MVS_ERR_NO_DEVICE;
    }
    if (hip_stream) {
        c->stream = static_cast<hipStream_t>(hip_stream);
        c->caller_sees_stream = true;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return MVS_ERR_HIP;
        }
        c->own_stream = true;
    }
    {
        // the scoring, refinement and extraction kernels are laid out for the 160 KB of LDS a gfx950 compute unit has
        int lds = 0, cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0)
            c->cu_count = cus;
        const hipError_t e1 = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id);
        hipError_t e2 = e1 == hipSuccess && lds >= 160 * 1024 ? prepare_kernels() : hipErrorInvalidDevice;
        if (e2 == hipSuccess)
            e2 = essential5_prepare();
        if (e2 != hipSuccess) {
            std::fprintf(stderr, "mvs_ctx_create: device %d offers %d bytes of LDS per workgroup (%s); this library is built "
                                 "for gfx950 (160 KB)\n", device_id, lds, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
            if (c->own_stream)
                (void)hipStreamDestroy(c->stream);
            delete c;
            return MVS_ERR_NO_DEVICE;
        }
    }
    if (ws_grow(c, c->small, 128 * sizeof(double)) != MVS_OK ||
        hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_dense[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_dense[1], hipEventDisableTiming) != hipSuccess) {
        mvs_ctx_destroy(c);
        return MVS_ERR_HIP;
    }
    *out = c;
    return MVS_OK;
}

mvs_status mvs_ctx_create(int device_id, mvs_ctx **out) { return mvs_ctx_create_on_stream(device_id, nullptr, out); }

void mvs_ctx_destroy(mvs_ctx *ctx)
{
    if (!ctx)
        return;
    (void)hipSetDevice(ctx->device);
    (void)sync_stream(ctx);
    if (ctx->scratch)
        mvs_batch_destroy(ctx->scratch);
    drop_orb_graph(ctx);
    if (ctx->h_orb_ovf) (void)hipHostFree(ctx->h_orb_ovf);
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
    if (ctx->side) {
        (void)hipStreamSynchronize(ctx->side);
        (void)hipStreamDestroy(ctx->side);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    for (hipEvent_t e : ctx->ev_dense)
        if (e) (void)hipEventDestroy(e);
    if (ctx->own_stream)
        (void)hipStreamDestroy(ctx->stream);
    delete ctx;   // the workspaces' destructors free them
}

void *mvs_ctx_stream(mvs_ctx *ctx)
{
    if (!ctx)
        return nullptr;
    ctx->caller_sees_stream = true;   // from now on every halves run joins before it returns
    return (void *)ctx_stream(ctx);
}

mvs_status mvs_ctx_set_half_batches(mvs_ctx *ctx, int enable)
{
    if (!ctx)
        return MVS_ERR_INVALID_ARG;
    ctx->half_batches = enable != 0;
    return MVS_OK;
}

mvs_status mvs_ctx_set_essential_confidence(mvs_ctx *ctx, double confidence)
{
    if (!ctx || !(confidence == 0.0 || (confidence > 0.0 && confidence < 1.0)))   // (a NaN fails both)
        return MVS_ERR_INVALID_ARG;
    ctx->e5_confidence = confidence == 0.0 ? 0.0 : confidence;   // (-0.0 is 0)
    return MVS_OK;
}

mvs_status mvs_ctx_essential_hypotheses_run(mvs_ctx *ctx, int32_t *n_run)
{
    if (!ctx || !n_run || ctx->e5_single < 0)
        return MVS_ERR_INVALID_ARG;
    *n_run = ctx->e5_single_run;
    if (ctx->e5_single == 0)
        return MVS_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(n_run, ctx->scratch->e5_nrun, sizeof(int32_t), hipMemcpyDeviceToHost, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

// ---------------------------------------------------------------------------------------------
// batches
// ---------------------------------------------------------------------------------------------
// n_frames == 0: every pair owns its two images.  n_frames == n_pairs + 1: the images are the frames of a sequence,
// stored once; pair k = (frame k, frame k + 1) is a view into the frame arrays (row f2).
mvs_status mvs_batch_create(mvs_ctx *ctx, int n_pairs, int max_kp, int desc_bytes, mvs_batch **out)
{
    return batch_create_impl(ctx, n_pairs, max_kp, desc_bytes, 0, out);
}

// n_frames != 0: the batch of a sequence, pair k = (frame k, frame k + lag) viewing ONE set of frame arrays -- its own, or
// with frames_of those (and the intrinsics and key offsets) of the sequence's lag-1 batch.  (extern "C++": a member of
// mvs_host defined inside the extern "C" block keeps the linkage of its declaration.)
extern "C++" mvs_status mvs_host::batch_create_impl(mvs_ctx *ctx, int n_pairs, int max_kp, int desc_bytes, int n_frames,
                                                    mvs_batch **out, const BatchDev *frames_of, int lag)
{
    if (!ctx || !out || n_pairs < 1 || max_kp < 1)
        return MVS_ERR_INVALID_ARG;
    if (max_kp > kMaxKp)
        return MVS_ERR_CAPACITY;
    if (!(desc_bytes == 16 || desc_bytes == 32 || desc_bytes == 64))
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mvs_batch *b = new mvs_batch();
    b->ctx = ctx;
    BatchDev &d = b->d;
    d.n_pairs = n_pairs;
    d.max_kp = max_kp;
    d.desc_words = desc_bytes / 4;
    d.max_groups = 0;
    d.cu_count = ctx->cu_count;
    const size_t P = n_pairs, N = max_kp;
    uint32_t *desc1 = nullptr, *desc2 = nullptr;
    float *kp1 = nullptr, *kp2 = nullptr;
    uint8_t *oct1 = nullptr, *oct2 = nullptr;
    int32_t *n1 = nullptr, *n2 = nullptr;
    double *Kinv = nullptr, *K = nullptr;
    int64_t *gidx = nullptr;
    const size_t NI = n_frames ? (size_t)n_frames : P;  // images held by desc1 / kp1 / n1
    DevGroup g(ctx, b->blocks);
    if (!frames_of) {
        g.add(desc1, NI * N * d.desc_words);
        g.add(kp1, NI * N * 2);
        g.add(oct1, NI * N);
        g.add(n1, NI);
    }
    if (!n_frames) {
        g.add(desc2, P * N * d.desc_words);
        g.add(kp2, P * N * 2);
        g.add(oct2, P * N);
        g.add(n2, P);
    }
    if (!frames_of) {
        g.add(Kinv, P * 9);
        g.add(K, P * 9);
        g.add(gidx, P);
    }
    g.add(d.knn_train, P * N);
    g.add(d.knn_dist, P * N);
    g.add(d.M, P);
    g.add(d.matches, P * N);
    g.add(d.pts, P * N * 4);
    g.add(d.cand_pts, P * 4 * N * 3);
    g.add(d.fin, P);
    g.add(d.inl, P * N);
    g.add(d.okf, P * 4 * N);
    g.add(d.results, P);
    g.add(d.mask, P * N);
    g.add(d.points, P * N * 3);
    g.add(d.point_idx, P * N);
    g.add(d.stats, 16);
    const mvs_status st = g.commit();
    if (st != MVS_OK) {
        mvs_batch_destroy(b);
        return st;
    }
    if (frames_of) {   // shared, never written through this batch; pair k of the view is pair k of the owner
        desc1 = const_cast<uint32_t *>(frames_of->desc1);
        kp1 = const_cast<float *>(frames_of->kp1);
        oct1 = const_cast<uint8_t *>(frames_of->oct1);
        n1 = const_cast<int32_t *>(frames_of->n1);
        Kinv = const_cast<double *>(frames_of->Kinv);
        K = const_cast<double *>(frames_of->K);
        gidx = const_cast<int64_t *>(frames_of->gidx);
    }
    if (n_frames) {  // pair k's second image is frame k + lag
        const size_t L = (size_t)lag;
        desc2 = desc1 + L * N * d.desc_words;
        kp2 = kp1 + L * N * 2;
        oct2 = oct1 + L * N;
        n2 = n1 + L;
    }
    d.desc1 = desc1; d.desc2 = desc2; d.kp1 = kp1; d.kp2 = kp2; d.n1 = n1; d.n2 = n2;
    d.oct1 = oct1; d.oct2 = oct2;
    d.Kinv = Kinv; d.K = K; d.gidx = gidx;   // the RANSAC stage's blocks stay null until ensure_groups
    hipStream_t s = ctx_stream(ctx);
    // deterministic contents for rows the caller never uploads
    if (!frames_of) {
        (void)hipMemsetAsync(desc1, 0, NI * N * d.desc_words * 4, s);
        (void)hipMemsetAsync(kp1, 0, NI * N * 2 * sizeof(float), s);
        (void)hipMemsetAsync(n1, 0, NI * sizeof(int32_t), s);
        (void)hipMemsetAsync(oct1, 0, NI * N, s);   // octave 0 (stddev = sigma_px) unless the extractor / caller says otherwise
    }
    if (!n_frames) {
        (void)hipMemsetAsync(oct2, 0, P * N, s);
        (void)hipMemsetAsync(desc2, 0, P * N * d.desc_words * 4, s);
        (void)hipMemsetAsync(kp2, 0, P * N * 2 * sizeof(float), s);
        (void)hipMemsetAsync(n2, 0, P * sizeof(int32_t), s);
    }
    if (!frames_of)
        (void)hipMemsetAsync(gidx, 0, P * sizeof(int64_t), s);
    (void)hipMemsetAsync(d.M, 0, P * sizeof(int32_t), s);
    (void)hipMemsetAsync(d.results, 0, P * sizeof(mvs_pair_result), s);
    (void)hipMemsetAsync(d.mask, 0, P * N, s);
    for (auto &e : b->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            mvs_batch_destroy(b);
            return MVS_ERR_HIP;
        }
    if (sync_stream(ctx) != hipSuccess) {
        ctx->err = "mvs_batch_create: hipStreamSynchronize failed";
        mvs_batch_destroy(b);
        return MVS_ERR_HIP;
    }
    *out = b;
    return MVS_OK;
}

void mvs_batch_destroy(mvs_batch *b)
{
    if (!b)
        return;
    (void)hipSetDevice(b->ctx->device);
    (void)sync_stream(b->ctx);
    for (auto &e : b->ev)
        if (e)
            (void)hipEventDestroy(e);
    if (b->h_pin)
        (void)hipHostFree(b->h_pin);
    for (auto &e : b->pin_ev)
        if (e)
            (void)hipEventDestroy(e);
    delete b;
}

static mvs_status batch_upload_impl(mvs_batch *b, int first, int count, const uint8_t *base_desc, const float *base_kp,
                                    const int32_t *n_base, const uint8_t *pair_desc, const float *pair_kp,
                                    const int32_t *n_pair, const double *K, const int64_t *global_index, bool sync)
{
    if (!b || first < 0 || count < 1 || first + count > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const BatchDev &d = b->d;
    hipStream_t s = ctx_stream(ctx);
    const size_t N = d.max_kp, DW = d.desc_words;
    if (n_base)
        for (int i = 0; i < count; ++i)
            if (n_base[i] < 0 || n_base[i] > (int)N)
                return MVS_ERR_CAPACITY;
    if (n_pair)
        for (int i = 0; i < count; ++i)
            if (n_pair[i] < 0 || n_pair[i] > (int)N)
                return MVS_ERR_CAPACITY;
    // host-derived per-pair parameters live in pinned memory owned by the batch (slot = pair index), so that the
    // asynchronous form needs no temporaries that outlive the call
    const size_t set_bytes = (size_t)d.n_pairs * (9 * sizeof(double) + sizeof(int64_t));
    if (!b->h_pin) {
        HIP_TRY(ctx, hipHostMalloc((void **)&b->h_pin, 2 * set_bytes, hipHostMallocDefault));
        for (auto &e : b->pin_ev)
            HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (K)
        for (int i = 0; i < count; ++i)
            if (!affine_K(K + 9 * i))
                return MVS_ERR_BAD_INTRINSICS;
    const bool staged = K || !global_index;
    const int set = b->pin_turn;
    char *base = b->h_pin + (size_t)set * set_bytes;
    double *kinv = reinterpret_cast<double *>(base) + (size_t)first * 9;
    int64_t *gi = reinterpret_cast<int64_t *>(base + (size_t)d.n_pairs * 9 * sizeof(double)) + first;
    if (staged && b->pin_ev_live[set])
        HIP_TRY(ctx, hipEventSynchronize(b->pin_ev[set]));   // only the copies that last read this slot set
    if (K)
        for (int i = 0; i < count; ++i)
            mat3_inverse(K + 9 * i, kinv + 9 * i);
    if (!global_index) {
        for (int i = 0; i < count; ++i)
            gi[i] = first + i;
        global_index = gi;
    }
    const size_t off = first;
#define UP(dst, src, bytes_per_pair)                                                                                   \
    if (src)                                                                                                           \
    HIP_TRY(ctx, hipMemcpyAsync((char *)(dst) + off * (bytes_per_pair), (src), (size_t)count * (bytes_per_pair),       \
                                hipMemcpyHostToDevice, s))
    UP(const_cast<uint32_t *>(d.desc1), base_desc, N * DW * 4);
    UP(const_cast<uint32_t *>(d.desc2), pair_desc, N * DW * 4);
    UP(const_cast<float *>(d.kp1), base_kp, N * 2 * sizeof(float));
    UP(const_cast<float *>(d.kp2), pair_kp, N * 2 * sizeof(float));
    UP(const_cast<int32_t *>(d.n1), n_base, sizeof(int32_t));
    UP(const_cast<int32_t *>(d.n2), n_pair, sizeof(int32_t));
    UP(const_cast<double *>(d.K), K, 9 * sizeof(double));
    const double *kinv_p = K ? kinv : nullptr;
    UP(const_cast<double *>(d.Kinv), kinv_p, 9 * sizeof(double));
    UP(const_cast<int64_t *>(d.gidx), global_index, sizeof(int64_t));
#undef UP
    if (staged) {
        HIP_TRY(ctx, hipEventRecord(b->pin_ev[set], s));
        b->pin_ev_live[set] = true;
        b->pin_turn = set ^ 1;
    }
    if (sync)
        HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_batch_upload(mvs_batch *b, int first, int count, const uint8_t *base_desc, const float *base_kp,
                            const int32_t *n_base, const uint8_t *pair_desc, const float *pair_kp,
                            const int32_t *n_pair, const double *K, const int64_t *global_index)
{
    return batch_upload_impl(b, first, count, base_desc, base_kp, n_base, pair_desc, pair_kp, n_pair, K, global_index, true);
}

mvs_status mvs_batch_upload_async(mvs_batch *b, int first, int count, const uint8_t *base_desc, const float *base_kp,
                                  const int32_t *n_base, const uint8_t *pair_desc, const float *pair_kp,
                                  const int32_t *n_pair, const double *K, const int64_t *global_index)
{
    return batch_upload_impl(b, first, count, base_desc, base_kp, n_base, pair_desc, pair_kp, n_pair, K, global_index, false);
}

mvs_status mvs_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0)
        return MVS_ERR_INVALID_ARG;
    *out = nullptr;
    return hipHostMalloc(out, bytes, hipHostMallocPortable) == hipSuccess ? MVS_OK : MVS_ERR_HIP;
}

void mvs_host_free(void *p)
{
    if (p)
        (void)hipHostFree(p);
}

extern "C++" mvs_status mvs_host::check_params(const mvs_params *p)
{
    if (!p || p->num_hypotheses < 1 || (p->sampler != MVS_SAMPLER_IDENTITY && p->sampler != MVS_SAMPLER_PHILOX))
        return MVS_ERR_INVALID_ARG;  // estimator-RANSAC.cpp:13 assert(max_iteration > 0)
    return MVS_OK;
}

// Pairs [first, first + count) of a batch as a batch of their own: every per-pair array advanced to its first pair, the two
// per-launch scalars (work-list length, mode-0 pair list) given a slot per half.  The kernels index by the pair's position
// in the launch, so they need no change; flat record indices (xlist) are relative to the view's hyp_F.
static BatchDev batch_view(const BatchDev &b, int first, int count, int half)
{
    BatchDev v = b;
    const size_t f = (size_t)first, N = (size_t)b.max_kp, Hp = (size_t)b.max_groups * kHypPerBlock;
    v.n_pairs = count;
    v.desc1 += f * N * b.desc_words; v.desc2 += f * N * b.desc_words;
    v.kp1 += f * N * 2; v.kp2 += f * N * 2;
    v.oct1 += f * N; v.oct2 += f * N;
    v.n1 += f; v.n2 += f;
    v.Kinv += f * 9; v.K += f * 9; v.gidx += f;
    v.knn_train += f * N; v.knn_dist += f * N;
    v.M += f; v.matches += f * N; v.pts += f * N * 4;
    v.wgbest += f * b.max_groups;
    v.hyp_F += f * Hp * kHypRec; v.hyp_r32 += f * Hp * kHypRec32;
    v.hyp_okf += f * Hp; v.hyp_cnt += f * Hp;
    v.bound += f; v.box += f * kBoxRec; v.mode += f;
    v.clist += f * Hp; v.clist2 += f * Hp; v.cpos += f * kSortBins;
    v.ccount += f; v.pcount += f; v.dense_n1 += f;
    v.m0list += (size_t)half * ((size_t)b.n_pairs + 1);
    v.xlist += f * Hp;
    v.xcount += 2 * half;
    v.cand_pts += f * 4 * N * 3; v.fin += f; v.inl += f * N; v.okf += f * 4 * N;
    v.results += f; v.mask += f * N; v.points += f * N * 3; v.point_idx += f * N;
    return v;
}

constexpr int kHalvesMinPairs = 64;   // a batch of at least this many pairs runs as two halves on two streams

static void enqueue_stages(const BatchDev &d, const RunParams &rp, int n_active, bool stats, hipStream_t s, hipEvent_t *ev,
                           LaunchTimer *lt, bool with_match = true, hipEvent_t wait_for = nullptr, hipEvent_t after_dense = nullptr)
{
    if (wait_for) (void)hipStreamWaitEvent(s, wait_for, 0);
    if (ev) (void)hipEventRecord(ev[0], s);
    if (with_match)
        launch_match_topk(d, rp, n_active, s, lt);
    if (ev) (void)hipEventRecord(ev[1], s);
    if (with_match)
        launch_match_compact(d, rp, n_active, s, lt);
    if (ev) (void)hipEventRecord(ev[2], s);
    launch_ransac(d, rp, n_active, stats, s, lt, after_dense);
    if (ev) (void)hipEventRecord(ev[3], s);
    launch_finalize(d, rp, n_active, kFinalizeFull, s, lt);
    if (ev) (void)hipEventRecord(ev[4], s);
}

static mvs_status enqueue_pipeline(mvs_batch *b, const RunParams &rp, int n_active, bool stats, hipEvent_t *ev,
                                   LaunchTimer *lt = nullptr, bool with_match = true)
{
    mvs_ctx *ctx = b->ctx;
    const bool halves = n_active >= kHalvesMinPairs && !stats && !ev && !lt && !b->d.hyp_count && ctx->half_batches;
    if (!halves) {
        enqueue_stages(b->d, rp, n_active, stats, ctx_stream(ctx), ev, lt, with_match);
    } else {
        // Two independent halves, one per lane: the first on the context's stream, the second on the side stream.  This is the
        // one place that reads the two streams directly.  The side lane is NOT joined back here: it stays open, and whatever
        // uses the context's stream next joins it first (ctx_stream) -- unless that is this very run again (same batch, same
        // pairs, nothing in between), whose halves touch exactly what the same lane's previous half touched (batch_view: every
        // per-pair array and both per-launch scalars belong to one half) and so need their own lane's order only.
        // The lanes alternate: a half's throughput section (match ... dense count) waits for the event the other lane records
        // behind its latest dense count, so the heavy sections run one after the other at full chip width and the latency-bound
        // tail of a half (list sort ... selection ... triangulation, ~0.8 ms whatever its size) runs under the other lane's
        // heavy section -- the last one under the NEXT call's.  Only a run that continues an open lane is chained (below).  Measured on the bench batch (ms per step, three runs each,
        // parent and change alternating): joined inside every call 4.378-4.402, free-running open lanes 4.220-4.238 (they fall
        // into lock-step, both tails coincide again), alternating open lanes 4.121-4.176 (kept).  A caller who sees the stream
        // gets the parent's arrangement unchanged: two free halves, joined before the call returns.
        // Inside one call (measured earlier): 2 parts +2.2 % pairs/s, +10 % frames/s on the sequence; 3 and 4 parts, a 40:60
        // split and a lower or higher priority of the side stream are all within noise of or below two halves.
        if (ctx->lane_open && (ctx->lane_batch != b || ctx->lane_pairs != n_active))
            (void)close_lane(ctx);   // another batch shares the workspaces, another count moves the split
        hipStream_t s = ctx->stream;
        const int na = (n_active + 1) / 2;
        const bool repeat = ctx->lane_open;
        if (!repeat) {
            // the second half waits for whatever is on the main stream (uploads, ...); nothing of this call is on the side
            // stream yet: a plain return is safe
            HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
        }
        // The chain of dense-count events exists between calls only: the first run behind a join is two free halves, as it
        // has always been -- that is the whole of a run that something joins at once (a sequence's pairs, a lag, an upload /
        // run / download loop) -- and records the events the next run's halves wait for.
        const bool chain = repeat && !ctx->caller_sees_stream;
        const bool record = !ctx->caller_sees_stream;
        enqueue_stages(batch_view(b->d, 0, na, 0), rp, na, false, s, nullptr, nullptr, with_match,
                       chain ? ctx->ev_dense[1] : nullptr, record ? ctx->ev_dense[0] : nullptr);
        const hipError_t e_first = hipGetLastError();            // a launch failure of the first half, attributed to it
        // from here on work may be queued on the side stream: the lane is open, and whatever fails it is joined before this
        // call returns
        ctx->lane_open = true;
        ctx->lane_batch = b;
        ctx->lane_pairs = n_active;
        enqueue_stages(batch_view(b->d, na, n_active - na, 1), rp, n_active - na, false, ctx->side, nullptr, nullptr, with_match,
                       chain ? ctx->ev_dense[0] : nullptr, record ? ctx->ev_dense[1] : nullptr);
        const hipError_t e_second = hipGetLastError();
        hipError_t e_join = hipSuccess;
        if (ctx->caller_sees_stream || e_first != hipSuccess || e_second != hipSuccess)
            e_join = close_lane(ctx);
        HIP_TRY(ctx, e_first);
        HIP_TRY(ctx, e_second);
        HIP_TRY(ctx, e_join);
    }
    if (lt) lt->end();
    HIP_TRY(ctx, hipGetLastError());
    return MVS_OK;
}

mvs_status mvs_batch_run(mvs_batch *b, const mvs_params *params, int n_active)
{
    if (!b || n_active < 1 || n_active > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(params);
    if (st != MVS_OK)
        return st;
    HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
    st = ensure_groups(b, params->num_hypotheses);
    if (st != MVS_OK)
        return st;
    return enqueue_pipeline(b, to_run(*params), n_active, false, nullptr);
}

// What the two mvs_batch_run_points* share: the checks, the estimator's tables, the caller's image points and match counts
// on the device, normalised points in d.pts.  `matches` rows of the batch are cleared (there is no match list: point k IS
// match k).
static mvs_status stage_batch_points(mvs_batch *b, Estimator est, const mvs_params *params, int n_active, const double *uv1,
                                     const double *uv2, const int32_t *m)
{
    if (!b || !uv1 || !uv2 || !m || n_active < 1 || n_active > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(params);
    if (st != MVS_OK)
        return st;
    const size_t N = (size_t)b->d.max_kp;
    for (int p = 0; p < n_active; ++p)
        if (m[p] < 0 || m[p] > (int)N)
            return MVS_ERR_CAPACITY;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((st = ensure_tables(b, est, params->num_hypotheses)) != MVS_OK)
        return st;
    if (!b->uv1) {   // staging for the image points, allocated on first use and owned by the batch
        const size_t count = (size_t)b->d.n_pairs * N * 2;
        if ((st = DevGroup(ctx, b->blocks).add(b->uv1, count).add(b->uv2, count).commit()) != MVS_OK)
            return st;
    }
    hipStream_t s = ctx_stream(ctx);
    const size_t pb = (size_t)n_active * N * 2 * sizeof(double);
    HIP_TRY(ctx, hipMemcpyAsync(b->uv1, uv1, pb, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(b->uv2, uv2, pb, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(b->d.M, m, (size_t)n_active * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(b->d.matches, 0, (size_t)n_active * N * sizeof(mvs_match), s));
    // the host buffers are the caller's: they may change as soon as this call returns (pageable copies are staged by the
    // runtime before hipMemcpyAsync returns; pinned ones are not) -- wait for the three copies, not for the kernels
    HIP_TRY(ctx, sync_stream(ctx));
    launch_prep_points(b->d, b->uv1, b->uv2, n_active, s);
    return MVS_OK;
}

// A batch of sfm_solve calls (vision/sfm.hpp:30-35, sfm-solve.cpp:285-368) on caller-supplied point pairs: the matcher is
// skipped, everything behind it is mvs_batch_run's (normalise -> RANSAC stage -> decomposition -> triangulation, half batches
// on two streams included).  uv1 / uv2: HOST, [n_active][max_kp][2] doubles (image points of the base / pair frame, row k of
// pair p = match k); m[p]: matches of pair p (0 .. max_kp).  The intrinsics and the sampler's key offsets are the resident
// ones (mvs_batch_upload with null descriptor / keypoint pointers sets just K and global_index).  results / mask / points /
// point_idx as after mvs_batch_run.
mvs_status mvs_batch_run_points(mvs_batch *b, const mvs_params *params, int n_active, const double *uv1, const double *uv2,
                                const int32_t *m)
{
    const mvs_status st = stage_batch_points(b, Estimator::kEightPoint, params, n_active, uv1, uv2, m);
    if (st != MVS_OK)
        return st;
    return enqueue_pipeline(b, to_run(*params), n_active, false, nullptr, nullptr, false);
}

// mvs_batch_run_points with find_essential_matrix's five-point branch (sfm-solve.cpp:42-63) in place of the 8-point RANSAC:
// normalise -> five-point RANSAC (essential5.hip) -> decomposition -> triangulation, plain launches on the one stream (no half
// batches, no captured graph).
mvs_status mvs_batch_run_points_essential(mvs_batch *b, const mvs_params *params, int n_active, const double *uv1,
                                          const double *uv2, const int32_t *m)
{
    const mvs_status st = stage_batch_points(b, Estimator::kFivePoint, params, n_active, uv1, uv2, m);
    if (st != MVS_OK)
        return st;
    enqueue_model(b, Estimator::kFivePoint, to_run(*params), n_active);
    HIP_TRY(b->ctx, hipGetLastError());
    return MVS_OK;
}

// The descriptor-fed five-point pipeline for pairs [0, n): matcher -> match_compact (which leaves the normalised points of the
// match list in d.pts, where the stage reads them) -> five-point RANSAC -> decomposition and triangulation.  One stream, plain
// launches.
static mvs_status enqueue_essential(mvs_batch *b, const RunParams &rp, int n)
{
    hipStream_t s = ctx_stream(b->ctx);
    launch_match_topk(b->d, rp, n, s);
    launch_match_compact(b->d, rp, n, s);
    enqueue_model(b, Estimator::kFivePoint, rp, n);
    HIP_TRY(b->ctx, hipGetLastError());
    return MVS_OK;
}

// the descriptor-fed pipeline of either estimator for pairs [0, n) (the tables are grown: ensure_tables)
extern "C++" mvs_status mvs_host::run_pairs(mvs_batch *b, Estimator est, const RunParams &rp, int n)
{
    return est == Estimator::kEightPoint ? enqueue_pipeline(b, rp, n, false, nullptr) : enqueue_essential(b, rp, n);
}

// mvs_batch_run with find_essential_matrix's five-point branch (sfm-solve.cpp:42-63) in place of the 8-point RANSAC
mvs_status mvs_batch_run_essential(mvs_batch *b, const mvs_params *params, int n_active)
{
    if (!b || n_active < 1 || n_active > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(params);
    if (st != MVS_OK)
        return st;
    HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
    if ((st = ensure_tables(b, Estimator::kFivePoint, params->num_hypotheses)) != MVS_OK)
        return st;
    return enqueue_essential(b, to_run(*params), n_active);
}

mvs_status mvs_batch_download_hypotheses_run(mvs_batch *b, int first, int count, int32_t *n_run)
{
    if (!b || !n_run || first < 0 || count < 1 || first + count > b->d.n_pairs || !b->e5_ran)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // pairs the last call did not reach: 0.  The others: the word its selection left on the device
    std::fill(n_run, n_run + count, 0);
    const int reached = std::min(count, b->e5_last_n - first);
    if (reached < 1)
        return MVS_OK;
    HIP_TRY(ctx, hipMemcpyAsync(n_run, b->e5_nrun + first, (size_t)reached * sizeof(int32_t), hipMemcpyDeviceToHost,
                                ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

// The per-hypothesis tables of the batch's last five-point run, in mvs_ransac_essential's convention: rows below the pair's
// n_run as counted, the rows from there on (not defined on the device) n_roots = 0, count = -1.
mvs_status mvs_batch_download_essential_tables(mvs_batch *b, int first, int count, int num_hypotheses, int32_t *n_roots,
                                               int32_t *count_tbl)
{
    if (!b || first < 0 || count < 1 || first + count > b->d.n_pairs || !b->e5_ran || num_hypotheses != b->e5_last_H)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    std::vector<int32_t> run(count);
    const mvs_status st = mvs_batch_download_hypotheses_run(b, first, count, run.data());
    if (st != MVS_OK)
        return st;
    const size_t H = (size_t)num_hypotheses, cap = (size_t)b->e5_cap;
    for (int p = 0; p < count; ++p) {
        const size_t T = std::min(H, (size_t)std::max(run[p], 0)), row = (size_t)(first + p) * cap;
        if (n_roots) {
            int32_t *dst = n_roots + (size_t)p * H;
            if (T)
                HIP_TRY(ctx, hipMemcpyAsync(dst, b->e5_nroots + row, T * sizeof(int32_t), hipMemcpyDeviceToHost, ctx_stream(ctx)));
            std::fill(dst + T, dst + H, 0);
        }
        if (count_tbl) {
            int32_t *dst = count_tbl + (size_t)p * H * kE5MaxRoots;
            if (T)
                HIP_TRY(ctx, hipMemcpyAsync(dst, b->e5_count + row * kE5MaxRoots, T * kE5MaxRoots * sizeof(int32_t),
                                            hipMemcpyDeviceToHost, ctx_stream(ctx)));
            std::fill(dst + T * kE5MaxRoots, dst + H * kE5MaxRoots, -1);
        }
    }
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_batch_sync(mvs_batch *b)
{
    if (!b)
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(b->ctx, sync_stream(b->ctx));
    return MVS_OK;
}

mvs_status mvs_batch_time(mvs_batch *b, const mvs_params *params, int n_active, int warmup, int steps,
                          float *ms_total, float *ms_kernel)
{
    if (!b || n_active < 1 || n_active > b->d.n_pairs || steps < 1 || warmup < 0)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(params);
    if (st != MVS_OK)
        return st;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = ensure_groups(b, params->num_hypotheses);
    if (st != MVS_OK)
        return st;
    const RunParams rp = to_run(*params);
    for (int i = 0; i < warmup; ++i)
        if ((st = enqueue_pipeline(b, rp, n_active, false, nullptr)) != MVS_OK)
            return st;
    HIP_TRY(ctx, sync_stream(ctx));
    // the two events bracket both lanes: the first run forks behind ev[5], ctx_stream joins the open lane in front of ev[6]
    HIP_TRY(ctx, hipEventRecord(b->ev[5], ctx_stream(ctx)));
    for (int i = 0; i < steps; ++i)
        if ((st = enqueue_pipeline(b, rp, n_active, false, nullptr)) != MVS_OK)
            return st;
    HIP_TRY(ctx, hipEventRecord(b->ev[6], ctx_stream(ctx)));
    HIP_TRY(ctx, hipEventSynchronize(b->ev[6]));
    if (ms_total)
        HIP_TRY(ctx, hipEventElapsedTime(ms_total, b->ev[5], b->ev[6]));
    if (ms_kernel) {
        for (int k = 0; k < 5; ++k)
            ms_kernel[k] = 0.f;
        for (int i = 0; i < steps; ++i) {
            if ((st = enqueue_pipeline(b, rp, n_active, false, b->ev)) != MVS_OK)
                return st;
            HIP_TRY(ctx, hipEventSynchronize(b->ev[4]));
            for (int k = 0; k < 4; ++k) {
                float ms = 0.f;
                HIP_TRY(ctx, hipEventElapsedTime(&ms, b->ev[k], b->ev[k + 1]));
                ms_kernel[k] += ms;
            }
        }
    }
    return MVS_OK;
}

mvs_status mvs_batch_time_kernels(mvs_batch *b, const mvs_params *params, int n_active, int steps, int cap,
                                  int32_t *kernel_id, float *ms, int *n_launches)
{
    if (!b || !kernel_id || !ms || !n_launches || n_active < 1 || n_active > b->d.n_pairs || steps < 1 || cap < 1)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(params);
    if (st != MVS_OK)
        return st;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = ensure_groups(b, params->num_hypotheses);
    if (st != MVS_OK)
        return st;
    const RunParams rp = to_run(*params);
    constexpr int kMaxLaunches = 32;
    cap = std::min(cap, kMaxLaunches);
    hipEvent_t ev[kMaxLaunches + 1] = {};
    int32_t kid[kMaxLaunches];
    for (int k = 0; k <= cap; ++k)
        if (hipEventCreate(&ev[k]) != hipSuccess) {
            for (int j = 0; j < k; ++j)
                (void)hipEventDestroy(ev[j]);
            ctx->err = "mvs_batch_time_kernels: hipEventCreate failed";
            return MVS_ERR_HIP;
        }
    int n = 0;
    st = MVS_OK;
    for (int k = 0; k < cap; ++k)
        ms[k] = 0.f;
    for (int i = 0; i < steps && st == MVS_OK; ++i) {
        LaunchTimer lt{ctx_stream(ctx), ev, kid, cap, 0};
        st = enqueue_pipeline(b, rp, n_active, false, nullptr, &lt);
        if (st != MVS_OK)
            break;
        if (hipEventSynchronize(ev[lt.n]) != hipSuccess) {
            ctx->err = "mvs_batch_time_kernels: hipEventSynchronize failed";
            st = MVS_ERR_HIP;
            break;
        }
        n = lt.n;
        for (int k = 0; k < n; ++k) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, ev[k], ev[k + 1]) != hipSuccess) {
                ctx->err = "mvs_batch_time_kernels: hipEventElapsedTime failed";
                st = MVS_ERR_HIP;
                break;
            }
            ms[k] += t;
            kernel_id[k] = kid[k];
        }
    }
    for (int k = 0; k <= cap; ++k)
        (void)hipEventDestroy(ev[k]);
    if (st != MVS_OK)
        return st;
    for (int k = 0; k < n; ++k)
        ms[k] /= (float)steps;
    *n_launches = n;
    return MVS_OK;
}

mvs_status mvs_kernel_info_get(mvs_ctx *ctx, int index, int max_kp, int desc_bytes, mvs_kernel_info *out)
{
    if (!ctx || !out || index < 0 || max_kp < 1 || max_kp > kMaxKp)
        return MVS_ERR_INVALID_ARG;
    KernelDesc kd;
    if (!kernel_desc(index, max_kp, desc_bytes / 4, &kd))
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->name, sizeof(out->name), "%s", kd.name);
    const char *sym = hipKernelNameRefByPtr(kd.fn, ctx_stream(ctx));
    std::snprintf(out->symbol, sizeof(out->symbol), "%s", sym ? sym : "");
    hipFuncAttributes fa;
    HIP_TRY(ctx, hipFuncGetAttributes(&fa, kd.fn));
    out->kernel_id = index;
    out->threads_per_block = kd.threads;
    out->num_regs = fa.numRegs;
    out->static_lds_bytes = (int32_t)fa.sharedSizeBytes;
    out->dynamic_lds_bytes = (int32_t)kd.dynamic_lds;
    out->scratch_bytes_per_lane = (int32_t)fa.localSizeBytes;
    out->max_threads_per_block = fa.maxThreadsPerBlock;
    int nb = 0;
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kd.fn, kd.threads, kd.dynamic_lds));
    out->blocks_per_cu = nb;
    const int waves = nb * ((kd.threads + 63) / 64);
    out->waves_per_simd = waves ? std::max(1, waves / 4) : 0;
    return MVS_OK;
}

// enqueue the device -> host copies of a batch's outputs on the ctx stream (after whatever has been enqueued: a
// preceding mvs_batch_run needs no synchronisation in between)
static mvs_status batch_download_enqueue(mvs_batch *b, int first, int count, mvs_pair_result *results, mvs_match *matches,
                                         uint8_t *inlier_mask, double *points_xyz, int32_t *point_idx32)
{
    mvs_ctx *ctx = b->ctx;
    hipStream_t s = ctx_stream(ctx);
    const BatchDev &d = b->d;
    const size_t N = d.max_kp, off = first, cnt = count;
    if (results)
        HIP_TRY(ctx, hipMemcpyAsync(results, d.results + off, cnt * sizeof(mvs_pair_result), hipMemcpyDeviceToHost, s));
    if (matches)
        HIP_TRY(ctx, hipMemcpyAsync(matches, d.matches + off * N, cnt * N * sizeof(mvs_match), hipMemcpyDeviceToHost, s));
    if (inlier_mask)
        HIP_TRY(ctx, hipMemcpyAsync(inlier_mask, d.mask + off * N, cnt * N, hipMemcpyDeviceToHost, s));
    if (points_xyz)
        HIP_TRY(ctx, hipMemcpyAsync(points_xyz, d.points + off * N * 3, cnt * N * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (point_idx32)
        HIP_TRY(ctx, hipMemcpyAsync(point_idx32, d.point_idx + off * N, cnt * N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return MVS_OK;
}

mvs_status mvs_batch_download(mvs_batch *b, int first, int count, mvs_pair_result *results, mvs_match *matches,
                              uint8_t *inlier_mask, double *points_xyz, int64_t *point_idx)
{
    if (!b || first < 0 || count < 1 || first + count > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t N = b->d.max_kp, cnt = count;
    std::vector<int32_t> tmp(point_idx ? cnt * N : 0);
    mvs_status st = batch_download_enqueue(b, first, count, results, matches, inlier_mask, points_xyz,
                                           point_idx ? tmp.data() : nullptr);
    if (st != MVS_OK)
        return st;
    HIP_TRY(ctx, sync_stream(ctx));
    for (size_t i = 0; i < tmp.size(); ++i)
        point_idx[i] = tmp[i];  // reference type: size_t (sfm.hpp:35)
    return MVS_OK;
}

mvs_status mvs_batch_download_async(mvs_batch *b, int first, int count, mvs_pair_result *results, mvs_match *matches,
                                    uint8_t *inlier_mask, double *points_xyz, int32_t *point_idx32)
{
    if (!b || first < 0 || count < 1 || first + count > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
    return batch_download_enqueue(b, first, count, results, matches, inlier_mask, points_xyz, point_idx32);
}

// The one exchange step of the path: all-gather of the fixed-size result records over RCCL, callable from
// host C++.  librccl is resolved at the first call (dlopen), so the library itself carries no link-time dependency on it
// and single-GPU callers never load it.  `rccl_comm` is the caller's ncclComm_t (one rank per GPU, created by the caller:
// ncclCommInitRank with an id it distributes however it likes); the collective is enqueued on the ctx stream, i.e. after
// the kernels of a preceding mvs_batch_run, and the call returns without waiting.
mvs_status mvs_batch_gather_results(mvs_batch *b, int n_active, void *rccl_comm, void *dst_device)
{
    if (!b || !rccl_comm || !dst_device || n_active < 1 || n_active > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    typedef int (*allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
    typedef const char *(*errstr_fn)(int);
    static allgather_fn fn = nullptr;
    static errstr_fn es = nullptr;
    if (!fn) {
        void *h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h)
            h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            ctx->err = std::string("dlopen(librccl.so): ") + dlerror();
            return MVS_ERR_HIP;
        }
        fn = reinterpret_cast<allgather_fn>(dlsym(h, "ncclAllGather"));
        es = reinterpret_cast<errstr_fn>(dlsym(h, "ncclGetErrorString"));
        if (!fn) {
            ctx->err = "librccl.so has no ncclAllGather";
            return MVS_ERR_HIP;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = fn(b->d.results, dst_device, (size_t)n_active * sizeof(mvs_pair_result), /* ncclUint8 */ 1, rccl_comm,
                      ctx_stream(ctx));
    if (rc != 0) {
        ctx->err = std::string("ncclAllGather: ") + (es ? es(rc) : "error");
        return MVS_ERR_HIP;
    }
    return MVS_OK;
}

mvs_status mvs_batch_stats(mvs_batch *b, const mvs_params *params, int n_active, mvs_work_stats *out)
{
    if (!b || !out || n_active < 1 || n_active > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(params);
    if (st != MVS_OK)
        return st;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = ensure_groups(b, params->num_hypotheses);
    if (st != MVS_OK)
        return st;
    hipStream_t s = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemsetAsync(b->d.stats, 0, 16 * sizeof(unsigned long long), s));
    st = enqueue_pipeline(b, to_run(*params), n_active, true, nullptr);
    if (st != MVS_OK)
        return st;
    HIP_TRY(ctx, sync_stream(ctx));
    unsigned long long h[16];
    HIP_TRY(ctx, hipMemcpy(h, b->d.stats, sizeof(h), hipMemcpyDeviceToHost));
    std::vector<mvs_pair_result> res(n_active);
    HIP_TRY(ctx, hipMemcpy(res.data(), b->d.results, n_active * sizeof(mvs_pair_result), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof(*out));
    out->rotations9 = (int64_t)h[0];
    out->pairs9 = (int64_t)h[1];
    out->score_evals_executed = (int64_t)(h[2] + h[3] + h[4] + h[5] + h[7] + h[8]);   // double-, single-precision and matrix-core counting
    out->score_evals_executed_mfma_pilot = (int64_t)h[8];
    out->score_evals_executed_mfma_rest = (int64_t)h[7];
    out->score_evals_executed_f32 = (int64_t)h[3];
    out->score_evals_executed_mfma = (int64_t)h[4];
    out->score_evals_executed_mfma_finish = (int64_t)h[5];
    out->max_sweeps9 = (int64_t)h[6];
    if (b->d.mode && b->d.xcount && h[2] + h[3] + h[4] + h[5] + h[8] > 0) {   // the pre-screened stage ran: its bookkeeping
        std::vector<int32_t> mode(n_active);
        uint32_t xc[2] = {0, 0};
        HIP_TRY(ctx, hipMemcpy(mode.data(), b->d.mode, n_active * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(xc, b->d.xcount, sizeof(xc), hipMemcpyDeviceToHost));
        std::vector<int32_t> n1(n_active);
        HIP_TRY(ctx, hipMemcpy(n1.data(), b->d.dense_n1, n_active * sizeof(int32_t), hipMemcpyDeviceToHost));
        int64_t legacy = 0, screened = 0;
        for (int i = 0; i < n_active; ++i) {
            if (res[i].n_matches < 8)
                continue;
            const int m = mode[i] < 0 || mode[i] > 2 ? 0 : mode[i];
            out->pairs_mode[m] += 1;
            (m == 0 ? legacy : screened) += params->num_hypotheses;
            if (m == 1) {
                out->dense_points += n1[i];
                out->matches_mode1 += res[i].n_matches;
            }
        }
        out->exact_solves = legacy + (int64_t)xc[0];
        out->prescreened = screened - (int64_t)xc[0];
    }
    for (const auto &r : res) {
        out->matches += r.n_matches;
        out->inliers += r.n_inliers;
        if (r.n_matches >= 8) {
            out->hypotheses += params->num_hypotheses;
            out->score_evals += (int64_t)params->num_hypotheses * r.n_matches;
        }
    }
    return MVS_OK;
}


// Read-only view of the batch's device-resident state for diagnostics (round 5): the bytes of the internal
// BatchDev (device pointers + capacities, mvslam_amd/csrc/kernels.hpp), so that the audit in libmvslam_hip_dbg.so -- built from
// the same sources -- can check what THIS library's kernels wrote, in place, in the same process.  Nothing is launched,
// copied on the device or changed; the caller synchronises the batch first.  The layout is private: the blob starts with
// its own size and the ABI version, which the consumer compares with its own.
mvs_status mvs_batch_device_state(mvs_batch *b, void *dst, size_t capacity, size_t *size)
{
    struct Blob {
        uint64_t bytes, abi;
        BatchDev d;
    };
    static_assert(std::is_trivially_copyable<BatchDev>::value, "BatchDev is a POD of device pointers and sizes");
    if (!b || !size)
        return MVS_ERR_INVALID_ARG;
    *size = sizeof(Blob);
    if (!dst)
        return MVS_OK;   // size query
    if (capacity < sizeof(Blob))
        return MVS_ERR_CAPACITY;
    Blob blob{sizeof(Blob), (uint64_t)MVS_ABI_VERSION, b->d};
    blob.d.hyp_count = nullptr;      // the optional per-hypothesis tables belong to the table entry points
    blob.d.hyp_residual = nullptr;
    std::memcpy(dst, &blob, sizeof(Blob));
    return MVS_OK;
}

mvs_status mvs_batch_results_device(mvs_batch *b, void **dev_ptr, size_t *record_bytes)
{
    if (!b || !dev_ptr)
        return MVS_ERR_INVALID_ARG;
    *dev_ptr = b->d.results;
    if (record_bytes)
        *record_bytes = sizeof(mvs_pair_result);
    return MVS_OK;
}

mvs_status mvs_batch_copy_results_device(mvs_batch *b, int first, int count, void *dst_device)
{
    if (!b || !dst_device || first < 0 || count < 1 || first + count > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
    HIP_TRY(b->ctx, hipMemcpyAsync(dst_device, b->d.results + first, (size_t)count * sizeof(mvs_pair_result),
                                   hipMemcpyDeviceToDevice, ctx_stream(b->ctx)));
    return MVS_OK;
}

// ---------------------------------------------------------------------------------------------
// single-shot entry points: a resident batch of one pair owned by the context
// ---------------------------------------------------------------------------------------------
static mvs_status ensure_scratch(mvs_ctx *ctx, int max_kp, int desc_bytes)
{
    if (max_kp > kMaxKp)
        return MVS_ERR_CAPACITY;
    if (ctx->scratch && ctx->scratch->d.max_kp >= max_kp && ctx->scratch->d.desc_words * 4 == desc_bytes)
        return MVS_OK;
    if (ctx->scratch) {
        max_kp = std::max(max_kp, ctx->scratch->d.max_kp);
        if (ctx->e5_single == 1) {   // mvs_ctx_essential_hypotheses_run outlives the batch it would read
            HIP_TRY(ctx, hipMemcpyAsync(&ctx->e5_single_run, ctx->scratch->e5_nrun, sizeof(int32_t), hipMemcpyDeviceToHost,
                                        ctx_stream(ctx)));
            HIP_TRY(ctx, sync_stream(ctx));
            ctx->e5_single = 0;
        }
        mvs_batch_destroy(ctx->scratch);
        ctx->scratch = nullptr;
    }
    max_kp = std::max(max_kp, 64);
    return mvs_batch_create(ctx, 1, max_kp, desc_bytes, &ctx->scratch);
}

// What fetch_single may reserve in the pinned arena for a scratch batch of `max_kp` rows (every output wanted, pin_get's
// alignment and some slack on top): a call adds this to what it stages upward when it opens the arena (pin_begin).
static size_t fetch_single_bound(int max_kp) { return single_layout(max_kp, 15).total + 512; }

// stage image points + camera of a single-shot call; leaves normalised points in batch->pts
static mvs_status stage_points(mvs_ctx *ctx, const double *p1_uv, const double *p2_uv, int m, const double K[9])
{
    if (!affine_K(K))
        return MVS_ERR_BAD_INTRINSICS;
    const int desc_bytes = ctx->scratch ? ctx->scratch->d.desc_words * 4 : 32;
    mvs_status st = ensure_scratch(ctx, std::max(m, 8), desc_bytes);
    if (st != MVS_OK)
        return st;
    mvs_batch *b = ctx->scratch;
    const size_t half = (size_t)b->d.max_kp * 2;   // doubles of one camera's points
    if ((st = ws_grow(ctx, ctx->uv, 2 * half * sizeof(double))) != MVS_OK)
        return st;
    double *d_uv1 = ctx->uv.ptr<double>(), *d_uv2 = d_uv1 + half;
    hipStream_t s = ctx_stream(ctx);
    double kinv[9];
    mat3_inverse(K, kinv);
    const int64_t zero = 0;
    const int32_t M = m;
    const size_t pb = (size_t)m * 2 * sizeof(double);
    // results come back through the same arena (fetch_single): size it for both directions now
    if ((st = pin_begin(ctx, 2 * pb + 1024 + fetch_single_bound(b->d.max_kp))) != MVS_OK)
        return st;
    if ((st = up_async(ctx, d_uv1, p1_uv, pb)) != MVS_OK) return st;
    if ((st = up_async(ctx, d_uv2, p2_uv, pb)) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<double *>(b->d.K), K, 9 * sizeof(double))) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<double *>(b->d.Kinv), kinv, 9 * sizeof(double))) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<int64_t *>(b->d.gidx), &zero, sizeof(zero))) != MVS_OK) return st;
    if ((st = up_async(ctx, b->d.M, &M, sizeof(M))) != MVS_OK) return st;
    launch_prep_points(b->d, d_uv1, d_uv2, 1, s);
    return MVS_OK;
}

// results of a single-shot call: asynchronous copies into the pinned arena (opened by the staging half of the call),
// ONE synchronisation, then plain memcpy into the caller's buffers.  The row counts are only known after the copy, so
// the m-row capacity is fetched (m <= 4096: at most 180 KB).
static mvs_status fetch_single(mvs_ctx *ctx, int m, mvs_pair_result *res, double *points_xyz, int64_t *point_idx,
                               uint8_t *mask, mvs_match *matches = nullptr)
{
    mvs_batch *b = ctx->scratch;
    hipStream_t s = ctx_stream(ctx);
    const size_t rows = (size_t)std::max(m, 0);
    // pair 0's outputs gathered on the device into one block, ONE copy to the pinned arena
    const int flags = ((mask && rows) ? 1 : 0) | ((points_xyz && rows) ? 2 : 0) | ((point_idx && rows) ? 4 : 0) |
                      ((matches && rows) ? 8 : 0);
    const SingleLayout L = single_layout((int)rows, flags);
    mvs_status st = ws_grow(ctx, ctx->single, L.total, single_layout(b->d.max_kp, 15).total);
    if (st != MVS_OK)
        return st;
    unsigned char *d_single = ctx->single.ptr<unsigned char>();
    unsigned char *h_all = static_cast<unsigned char *>(pin_get(ctx, L.total));
    PIN_TRY(ctx, h_all);
    launch_single_gather(b->d, (int)rows, flags, d_single, s);
    HIP_TRY(ctx, hipMemcpyAsync(h_all, d_single, L.total, hipMemcpyDeviceToHost, s));
    const mvs_pair_result *h_res = reinterpret_cast<const mvs_pair_result *>(h_all);
    const uint8_t *h_mask = (flags & 1) ? h_all + L.mask : nullptr;
    const double *h_pts = (flags & 2) ? reinterpret_cast<const double *>(h_all + L.points) : nullptr;
    const int32_t *h_idx = (flags & 4) ? reinterpret_cast<const int32_t *>(h_all + L.idx) : nullptr;
    const mvs_match *h_mt = (flags & 8) ? reinterpret_cast<const mvs_match *>(h_all + L.matches) : nullptr;
    HIP_TRY(ctx, sync_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    *res = *h_res;
    const size_t M = (size_t)std::min<int>(std::max(res->n_matches, 0), (int)rows);
    if (h_mask)
        std::memcpy(mask, h_mask, matches ? M : rows);
    const int n = res->valid ? res->n_points : 0;
    if (n > 0 && h_pts)
        std::memcpy(points_xyz, h_pts, (size_t)n * 3 * sizeof(double));
    if (n > 0 && h_idx)
        for (int i = 0; i < n; ++i)
            point_idx[i] = h_idx[i];   // reference type: size_t (sfm.hpp:35)
    if (h_mt && M)
        std::memcpy(matches, h_mt, M * sizeof(mvs_match));
    return MVS_OK;
}

mvs_status mvs_match_hamming(mvs_ctx *ctx, const uint8_t *train_desc, int n_train, const uint8_t *query_desc,
                             int n_query, int desc_bytes, double ratio, double max_dist, mvs_match *out, int *n_out)
{
    if (!ctx || !train_desc || !query_desc || !out || !n_out)
        return MVS_ERR_INVALID_ARG;
    *n_out = 0;
    if (n_train < 2 || n_query < 1)  // visual-feature.cpp:56 assert(valid), :67 needs two neighbours
        return MVS_ERR_INVALID_ARG;
    if (!(desc_bytes == 16 || desc_bytes == 32 || desc_bytes == 64))
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mvs_status st = ensure_scratch(ctx, std::max(n_train, n_query), desc_bytes);
    if (st != MVS_OK)
        return st;
    mvs_batch *b = ctx->scratch;
    hipStream_t s = ctx_stream(ctx);
    const int32_t n1 = n_train, n2 = n_query;
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const size_t cap = (size_t)std::min(n_train, n_query);   // a query matches at most once
    (void)cap;
    const size_t tb = (size_t)n_train * desc_bytes, qb = (size_t)n_query * desc_bytes;
    if ((st = pin_begin(ctx, tb + qb + 1024 + sizeof(int32_t) + ((size_t)n_query) * sizeof(mvs_match))) != MVS_OK)
        return st;
    // descriptors (<= 4096 x 64 B per image) and the small parameters all go through the pinned arena: every device copy
    // is an asynchronous DMA, whatever memory the caller's cv::Mat lives in
    if ((st = up_async(ctx, const_cast<uint32_t *>(b->d.desc1), train_desc, tb)) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<uint32_t *>(b->d.desc2), query_desc, qb)) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<int32_t *>(b->d.n1), &n1, sizeof(n1))) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<int32_t *>(b->d.n2), &n2, sizeof(n2))) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<double *>(b->d.Kinv), eye, sizeof(eye))) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<double *>(b->d.K), eye, sizeof(eye))) != MVS_OK) return st;
    RunParams rp{};
    rp.ratio = ratio;
    rp.max_dist = max_dist;
    launch_match_topk(b->d, rp, 1, s);
    launch_match_compact(b->d, rp, 1, s);
    int32_t *h_M = static_cast<int32_t *>(pin_get(ctx, sizeof(int32_t)));
    mvs_match *h_mt = static_cast<mvs_match *>(pin_get(ctx, (size_t)n_query * sizeof(mvs_match)));
    PIN_TRY(ctx, h_M);
    PIN_TRY(ctx, h_mt);
    HIP_TRY(ctx, hipMemcpyAsync(h_M, b->d.M, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(h_mt, b->d.matches, (size_t)n_query * sizeof(mvs_match), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    const int32_t M = *h_M;
    if (M > 0)
        std::memcpy(out, h_mt, (size_t)M * sizeof(mvs_match));
    *n_out = M;
    return MVS_OK;
}

// the end of every call that returns a pose: the record, then R / t / point count of a valid one
static mvs_status return_pose(const mvs_pair_result &res, mvs_pair_result *result, double R[9], double t[3], int *n_points)
{
    if (result)
        *result = res;
    if (!res.valid)
        return MVS_NO_MODEL;
    if (R) std::memcpy(R, res.R, sizeof(res.R));
    if (t) std::memcpy(t, res.t, sizeof(res.t));
    if (n_points) *n_points = res.n_points;
    return MVS_OK;
}

// sfm_solve (sfm-solve.cpp:285-368) of one pair with either estimator in front of the same tail
static mvs_status two_view_impl(mvs_ctx *ctx, Estimator est, const double *p1_uv, const double *p2_uv, int m, const double K[9],
                                const mvs_params *params, double R[9], double t[3], double *points_xyz, int64_t *point_idx,
                                int *n_points, uint8_t *inlier_mask, mvs_pair_result *result)
{
    if (!ctx || !p1_uv || !p2_uv || !K || m < 0)
        return MVS_ERR_INVALID_ARG;
    if (est == Estimator::kFivePoint)
        ctx->e5_single = -1;   // a call that fails before its RANSAC is enqueued leaves no n_run behind
    mvs_status st = check_params(params);
    if (st != MVS_OK)
        return st;
    if (n_points)
        *n_points = 0;
    mvs_pair_result res;
    std::memset(&res, 0, sizeof(res));
    res.best_hyp = -1;
    res.n_matches = m;
    if (m < 8) {  // sfm-solve.cpp:37 asserts; estimator-RANSAC.cpp:25-29 returns false
        if (result)
            *result = res;
        if (est == Estimator::kFivePoint && m >= 1) {
            ctx->e5_single = 0;
            ctx->e5_single_run = 0;
        }
        return m < 1 ? MVS_ERR_INVALID_ARG : MVS_NO_MODEL;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = stage_points(ctx, p1_uv, p2_uv, m, K);
    if (st != MVS_OK)
        return st;
    if ((st = ensure_tables(ctx->scratch, est, params->num_hypotheses)) != MVS_OK)
        return st;
    enqueue_model(ctx->scratch, est, to_run(*params), 1);
    st = fetch_single(ctx, m, &res, points_xyz, point_idx, inlier_mask);
    if (st != MVS_OK)
        return st;
    return return_pose(res, result, R, t, n_points);
}

mvs_status mvs_two_view(mvs_ctx *ctx, const double *p1_uv, const double *p2_uv, int m, const double K[9],
                        const mvs_params *params, double R[9], double t[3], double *points_xyz,
                        int64_t *point_idx, int *n_points, uint8_t *inlier_mask, mvs_pair_result *result)
{
    return two_view_impl(ctx, Estimator::kEightPoint, p1_uv, p2_uv, m, K, params, R, t, points_xyz, point_idx, n_points,
                         inlier_mask, result);
}

// sfm_solve with find_essential_matrix's five-point branch (sfm-solve.cpp:42-63,285-368): mvs_two_view with the five-point
// RANSAC of essential5.hip in front of the same tail.  No refit and no projection: F and E of the result both hold the winner.
mvs_status mvs_two_view_essential(mvs_ctx *ctx, const double *p1_uv, const double *p2_uv, int m, const double K[9],
                                  const mvs_params *params, double R[9], double t[3], double *points_xyz, int64_t *point_idx,
                                  int *n_points, uint8_t *inlier_mask, mvs_pair_result *result)
{
    return two_view_impl(ctx, Estimator::kFivePoint, p1_uv, p2_uv, m, K, params, R, t, points_xyz, point_idx, n_points,
                         inlier_mask, result);
}

// ImagePair::ImagePair + reconstruct (front-end/image-pair.cpp:30-71,116-174) of ONE pair in one device pass: the
// descriptors and keypoints go up once, the four stages run back to back on the stream, everything comes back through the
// pinned arena after a single synchronisation (match -> host gather -> sfm_solve as separate calls costs two round trips).
static mvs_status image_pair_impl(mvs_ctx *ctx, Estimator est, const uint8_t *base_desc, const float *base_kp, int n_base,
                                  const uint8_t *pair_desc, const float *pair_kp, int n_pair, int desc_bytes, const double K[9],
                                  const mvs_params *params, mvs_pair_result *result, mvs_match *matches, uint8_t *inlier_mask,
                                  double *points_xyz, int64_t *point_idx)
{
    if (!ctx || !base_desc || !base_kp || !pair_desc || !pair_kp || !K || !result)
        return MVS_ERR_INVALID_ARG;
    if (est == Estimator::kFivePoint)
        ctx->e5_single = -1;   // a call that fails before its RANSAC is enqueued leaves no n_run behind
    mvs_status st = check_params(params);
    if (st != MVS_OK)
        return st;
    if (n_base < 2 || n_pair < 1)   // visual-feature.cpp:56,67
        return MVS_ERR_INVALID_ARG;
    if (!(desc_bytes == 16 || desc_bytes == 32 || desc_bytes == 64))
        return MVS_ERR_INVALID_ARG;
    if (!affine_K(K))
        return MVS_ERR_BAD_INTRINSICS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((st = ensure_scratch(ctx, std::max(n_base, n_pair), desc_bytes)) != MVS_OK)
        return st;
    mvs_batch *b = ctx->scratch;
    if ((st = ensure_tables(b, est, params->num_hypotheses)) != MVS_OK)
        return st;
    const size_t db1 = (size_t)n_base * desc_bytes, db2 = (size_t)n_pair * desc_bytes;
    const size_t kb1 = (size_t)n_base * 2 * sizeof(float), kb2 = (size_t)n_pair * 2 * sizeof(float);
    if ((st = pin_begin(ctx, db1 + db2 + kb1 + kb2 + 2048 + fetch_single_bound(b->d.max_kp))) != MVS_OK)
        return st;
    double kinv[9];
    mat3_inverse(K, kinv);
    const int32_t n1 = n_base, n2 = n_pair;
    const int64_t zero = 0;
    // <= 4096 x 64 B per image: through the pinned arena (a memcpy of ~160 KB), so that the device copy is true asynchronous
    // DMA whatever memory the caller's cv::Mat / std::vector lives in -- as ONE block [desc1 | desc2 | kp1 | kp2] and one copy
    // command; the kernel that receives the pair's scalars as arguments also puts the parts in place
    {
        Carve L{16};
        const size_t o_desc1 = L.take(db1), o_desc2 = L.take(db2), o_kp1 = L.take(kb1), o_kp2 = L.take(kb2);
        const size_t total = L.total();
        if ((st = ws_grow(ctx, ctx->single_in, total, (size_t)b->d.max_kp * (2 * 64 + 2 * 8) + 64)) != MVS_OK)
            return st;
        unsigned char *h_in = static_cast<unsigned char *>(pin_get(ctx, total));
        PIN_TRY(ctx, h_in);
        std::memcpy(h_in + o_desc1, base_desc, db1);
        std::memcpy(h_in + o_desc2, pair_desc, db2);
        std::memcpy(h_in + o_kp1, base_kp, kb1);
        std::memcpy(h_in + o_kp2, pair_kp, kb2);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->single_in.ptr(), h_in, total, hipMemcpyHostToDevice, ctx_stream(ctx)));
        SingleParams sp;
        sp.n1 = n1;
        sp.n2 = n2;
        sp.gidx = zero;
        for (int k = 0; k < 9; ++k) {
            sp.K[k] = K[k];
            sp.Kinv[k] = kinv[k];
        }
        sp.part_bytes[0] = (uint32_t)db1; sp.part_bytes[1] = (uint32_t)db2;
        sp.part_bytes[2] = (uint32_t)kb1; sp.part_bytes[3] = (uint32_t)kb2;
        launch_single_params(b->d, sp, ctx->single_in.ptr(), ctx_stream(ctx));
    }
    if ((st = run_pairs(b, est, to_run(*params), 1)) != MVS_OK)
        return st;
    if ((st = fetch_single(ctx, n_pair, result, points_xyz, point_idx, inlier_mask, matches)) != MVS_OK)
        return st;
    return result->valid ? MVS_OK : MVS_NO_MODEL;
}

mvs_status mvs_image_pair(mvs_ctx *ctx, const uint8_t *base_desc, const float *base_kp, int n_base,
                          const uint8_t *pair_desc, const float *pair_kp, int n_pair, int desc_bytes, const double K[9],
                          const mvs_params *params, mvs_pair_result *result, mvs_match *matches, uint8_t *inlier_mask,
                          double *points_xyz, int64_t *point_idx)
{
    return image_pair_impl(ctx, Estimator::kEightPoint, base_desc, base_kp, n_base, pair_desc, pair_kp, n_pair, desc_bytes, K,
                           params, result, matches, inlier_mask, points_xyz, point_idx);
}

// mvs_image_pair with find_essential_matrix's five-point branch (sfm-solve.cpp:42-63): what mvs_match_hamming, a host gather
// and mvs_two_view_essential compute in two round trips, in one pass.
mvs_status mvs_image_pair_essential(mvs_ctx *ctx, const uint8_t *base_desc, const float *base_kp, int n_base,
                                    const uint8_t *pair_desc, const float *pair_kp, int n_pair, int desc_bytes,
                                    const double K[9], const mvs_params *params, mvs_pair_result *result, mvs_match *matches,
                                    uint8_t *inlier_mask, double *points_xyz, int64_t *point_idx)
{
    return image_pair_impl(ctx, Estimator::kFivePoint, base_desc, base_kp, n_base, pair_desc, pair_kp, n_pair, desc_bytes, K,
                           params, result, matches, inlier_mask, points_xyz, point_idx);
}

static mvs_status upload_mask(mvs_ctx *ctx, const uint8_t *mask, int m)
{
    mvs_batch *b = ctx->scratch;
    if (mask) {   // the caller's buffer outlives the call: every entry point synchronises before it returns
        HIP_TRY(ctx, hipMemcpyAsync(b->d.mask, mask, (size_t)m, hipMemcpyHostToDevice, ctx_stream(ctx)));
    } else {
        HIP_TRY(ctx, hipMemsetAsync(b->d.mask, 1, (size_t)m, ctx_stream(ctx)));
    }
    return MVS_OK;
}

mvs_status mvs_triangulate(mvs_ctx *ctx, const double *p1_uv, const double *p2_uv, int m, const double K[9],
                           const double R1to2[9], const double t1to2[3], double *points_xyz, int64_t *point_idx,
                           int *n_points)
{
    if (!ctx || !p1_uv || !p2_uv || !K || !R1to2 || !t1to2 || !n_points || m < 1)  // sfm-solve.cpp:143-144
        return MVS_ERR_INVALID_ARG;
    *n_points = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mvs_status st = stage_points(ctx, p1_uv, p2_uv, m, K);
    if (st != MVS_OK)
        return st;
    mvs_batch *b = ctx->scratch;
    mvs_pair_result res;
    std::memset(&res, 0, sizeof(res));
    std::memcpy(res.R1to2, R1to2, sizeof(res.R1to2));
    std::memcpy(res.t1to2, t1to2, sizeof(res.t1to2));
    if ((st = up_async(ctx, b->d.results, &res, sizeof(res))) != MVS_OK)
        return st;
    if ((st = upload_mask(ctx, nullptr, m)) != MVS_OK)
        return st;
    RunParams rp{};
    rp.num_hypotheses = 1;
    launch_finalize(b->d, rp, 1, kFinalizeTriangulate, ctx_stream(ctx));
    st = fetch_single(ctx, m, &res, points_xyz, point_idx, nullptr);
    if (st != MVS_OK)
        return st;
    *n_points = res.valid ? res.n_points : 0;
    return MVS_OK;
}

mvs_status mvs_recover_pose(mvs_ctx *ctx, const double E[9], const double *p1_uv, const double *p2_uv, int m,
                            const double K[9], const uint8_t *inlier_mask, double R[9], double t[3],
                            double *points_xyz, int64_t *point_idx, int *n_points, mvs_pair_result *result)
{
    if (!ctx || !E || !p1_uv || !p2_uv || !K || m < 1)
        return MVS_ERR_INVALID_ARG;
    if (n_points)
        *n_points = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mvs_status st = stage_points(ctx, p1_uv, p2_uv, m, K);
    if (st != MVS_OK)
        return st;
    mvs_batch *b = ctx->scratch;
    mvs_pair_result res;
    std::memset(&res, 0, sizeof(res));
    std::memcpy(res.E, E, sizeof(res.E));
    if ((st = up_async(ctx, b->d.results, &res, sizeof(res))) != MVS_OK)
        return st;
    if ((st = upload_mask(ctx, inlier_mask, m)) != MVS_OK)
        return st;
    RunParams rp{};
    rp.num_hypotheses = 1;
    launch_finalize(b->d, rp, 1, kFinalizeFromE, ctx_stream(ctx));
    st = fetch_single(ctx, m, &res, points_xyz, point_idx, nullptr);
    if (st != MVS_OK)
        return st;
    return return_pose(res, result, R, t, n_points);
}

mvs_status mvs_find_fundamental_matrix(mvs_ctx *ctx, const double p1_xy[16], const double p2_xy[16], double F[9])
{
    if (!ctx || !p1_xy || !p2_xy || !F)
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    double *d = ctx->small.ptr<double>();  // [0,16) p1, [16,32) p2, [32,41) F, [48] ok flag (as int)
    HIP_TRY(ctx, hipMemcpyAsync(d, p1_xy, 16 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d + 16, p2_xy, 16 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, sync_stream(ctx));
    launch_fundamental(d, d + 16, d + 32, reinterpret_cast<int *>(d + 48), s);
    HIP_TRY(ctx, sync_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    int ok = 0;
    HIP_TRY(ctx, hipMemcpy(F, d + 32, 9 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(&ok, d + 48, sizeof(int), hipMemcpyDeviceToHost));
    return ok ? MVS_OK : MVS_NO_MODEL;
}

// What the two mvs_ransac_* share behind their own argument checks: the scratch batch with the estimator's tables, the
// ideal-camera points packed four to a row into its pts (they are already normalised: pure packing), identity intrinsics,
// and the parameters of a RANSAC stage that stops after the mask.
static mvs_status stage_ideal(mvs_ctx *ctx, Estimator est, const double *p1_xy, const double *p2_xy, int m, double max_error_sq,
                              int num_hypotheses, int sampler, uint64_t seed, RunParams *rp)
{
    if (m > kMaxKp)
        return MVS_ERR_CAPACITY;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int desc_bytes = ctx->scratch ? ctx->scratch->d.desc_words * 4 : 32;
    mvs_status st = ensure_scratch(ctx, m, desc_bytes);
    if (st != MVS_OK)
        return st;
    mvs_batch *b = ctx->scratch;
    if ((st = ensure_tables(b, est, num_hypotheses)) != MVS_OK)
        return st;
    std::vector<double> packed((size_t)m * 4);
    for (int i = 0; i < m; ++i) {
        packed[4 * i] = p1_xy[2 * i];
        packed[4 * i + 1] = p1_xy[2 * i + 1];
        packed[4 * i + 2] = p2_xy[2 * i];
        packed[4 * i + 3] = p2_xy[2 * i + 1];
    }
    const int32_t M = m;
    const int64_t zero = 0;
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if ((st = pin_begin(ctx, packed.size() * sizeof(double) + 2048 + fetch_single_bound(b->d.max_kp))) != MVS_OK)
        return st;
    if ((st = up_async(ctx, b->d.pts, packed.data(), packed.size() * sizeof(double))) != MVS_OK) return st;
    if ((st = up_async(ctx, b->d.M, &M, sizeof(M))) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<int64_t *>(b->d.gidx), &zero, sizeof(zero))) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<double *>(b->d.K), eye, sizeof(eye))) != MVS_OK) return st;
    if ((st = up_async(ctx, const_cast<double *>(b->d.Kinv), eye, sizeof(eye))) != MVS_OK) return st;
    *rp = RunParams{};
    rp->max_error_sq = max_error_sq;
    rp->num_hypotheses = num_hypotheses;
    rp->sampler = sampler;
    rp->seed = seed;
    rp->min_inliers = 0x7fffffff;  // stop after the mask: no decomposition / triangulation wanted here
    return MVS_OK;
}

// `sampler` is not validated here: any non-zero value samples as Philox.
mvs_status mvs_ransac_fundamental(mvs_ctx *ctx, const double *p1_xy, const double *p2_xy, int m, double max_error_sq,
                                  int num_hypotheses, int sampler, uint64_t seed, double F[9], uint8_t *inlier_mask,
                                  int *best_hyp, int *best_count, double *best_residual, int32_t *count,
                                  double *residual)
{
    if (!ctx || !p1_xy || !p2_xy || m < 0 || num_hypotheses < 1)
        return MVS_ERR_INVALID_ARG;
    if (!(max_error_sq > 2.220446049250313e-16))  // estimator-RANSAC.cpp:12
        return MVS_ERR_INVALID_ARG;
    if (best_hyp) *best_hyp = -1;
    if (best_count) *best_count = 0;
    if (best_residual) *best_residual = 0.0;
    if (m < 8)
        return MVS_NO_MODEL;  // estimator-RANSAC.cpp:25-29
    RunParams rp;
    mvs_status st = stage_ideal(ctx, Estimator::kEightPoint, p1_xy, p2_xy, m, max_error_sq, num_hypotheses, sampler, seed, &rp);
    if (st != MVS_OK)
        return st;
    mvs_batch *b = ctx->scratch;
    // The only place a BatchDev's per-hypothesis tables are ever hooked up: whichever way this call ends they are unhooked
    // again, so everywhere else d.hyp_count / d.hyp_residual are null.
    struct Unhook {
        BatchDev &d;
        ~Unhook() { d.hyp_count = nullptr; d.hyp_residual = nullptr; }
    } unhook{b->d};
    if (count || residual) {
        if (b->hyp_table_cap < num_hypotheses) {
            HIP_TRY(ctx, sync_stream(ctx));   // the tables it replaces are freed
            const size_t H = num_hypotheses;
            if ((st = DevGroup(ctx, b->blocks).add(b->hyp_table_count, H).add(b->hyp_table_residual, H).commit()) != MVS_OK)
                return st;
            b->hyp_table_cap = num_hypotheses;
        }
        b->d.hyp_count = b->hyp_table_count;
        b->d.hyp_residual = b->hyp_table_residual;
    }
    enqueue_model(b, Estimator::kEightPoint, rp, 1);
    mvs_pair_result res;
    if ((st = fetch_single(ctx, m, &res, nullptr, nullptr, inlier_mask)) != MVS_OK)
        return st;
    if (count)
        HIP_TRY(ctx, hipMemcpy(count, b->d.hyp_count, (size_t)num_hypotheses * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (residual)
        HIP_TRY(ctx, hipMemcpy(residual, b->d.hyp_residual, (size_t)num_hypotheses * sizeof(double),
                               hipMemcpyDeviceToHost));
    if (F) std::memcpy(F, res.F, sizeof(res.F));
    if (best_hyp) *best_hyp = res.best_hyp;
    if (best_count) *best_count = res.best_count;
    if (best_residual) *best_residual = res.best_residual;
    return res.best_count > 0 ? MVS_OK : MVS_NO_MODEL;  // estimator-RANSAC.cpp:89
}

// The minimal solver on the device (five_point.hpp): what cv::findEssentialMat runs per sample.
mvs_status mvs_five_point(mvs_ctx *ctx, const double p1_xy[10], const double p2_xy[10], double E_out[90], int *n)
{
    if (!ctx || !p1_xy || !p2_xy || !E_out || !n)
        return MVS_ERR_INVALID_ARG;
    *n = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    double *d = ctx->small.ptr<double>();  // [0,10) p1, [10,20) p2, [20,110) E, [110] n (as int)
    HIP_TRY(ctx, hipMemcpyAsync(d, p1_xy, 10 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d + 10, p2_xy, 10 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, sync_stream(ctx));
    launch_five_point(d, d + 10, d + 20, reinterpret_cast<int *>(d + 110), s);
    HIP_TRY(ctx, sync_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpy(E_out, d + 20, 90 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(n, d + 110, sizeof(int), hipMemcpyDeviceToHost));
    return MVS_OK;
}

// The RANSAC stage alone on ideal-camera points (the five-point counterpart of mvs_ransac_fundamental).
mvs_status mvs_ransac_essential(mvs_ctx *ctx, const double *p1_xy, const double *p2_xy, int m, double max_error_sq,
                                int num_hypotheses, int sampler, uint64_t seed, double E[9], uint8_t *inlier_mask, int *best_hyp,
                                int *best_root, int *best_count, double *best_residual, int32_t *n_roots, int32_t *count)
{
    if (!ctx || !p1_xy || !p2_xy || m < 0 || num_hypotheses < 1 ||
        (sampler != MVS_SAMPLER_IDENTITY && sampler != MVS_SAMPLER_PHILOX))
        return MVS_ERR_INVALID_ARG;
    if (!(max_error_sq > 2.220446049250313e-16))  // estimator-RANSAC.cpp:12
        return MVS_ERR_INVALID_ARG;
    ctx->e5_single = -1;   // a call that fails before its RANSAC is enqueued leaves no n_run behind
    if (best_hyp) *best_hyp = -1;
    if (best_root) *best_root = -1;
    if (best_count) *best_count = 0;
    if (best_residual) *best_residual = 0.0;
    if (m < 8) {
        ctx->e5_single = 0;
        ctx->e5_single_run = 0;
        return MVS_NO_MODEL;  // sfm-solve.cpp:37
    }
    RunParams rp;
    mvs_status st = stage_ideal(ctx, Estimator::kFivePoint, p1_xy, p2_xy, m, max_error_sq, num_hypotheses, sampler, seed, &rp);
    if (st != MVS_OK)
        return st;
    mvs_batch *b = ctx->scratch;
    enqueue_model(b, Estimator::kFivePoint, rp, 1);
    mvs_pair_result res;
    if ((st = fetch_single(ctx, m, &res, nullptr, nullptr, inlier_mask)) != MVS_OK)
        return st;
    // the tables: rows below the pair's n_run as counted, the rows from there on (not defined on the device) cleared
    const size_t H = (size_t)num_hypotheses;
    size_t T = H;
    if ((n_roots || count) && ctx->e5_confidence > 0.0) {
        int32_t n_run = 0;
        HIP_TRY(ctx, hipMemcpy(&n_run, b->e5_nrun, sizeof(int32_t), hipMemcpyDeviceToHost));
        T = std::min(H, (size_t)std::max(n_run, 0));
    }
    if (n_roots) {
        HIP_TRY(ctx, hipMemcpy(n_roots, b->e5_nroots, T * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::fill(n_roots + T, n_roots + H, 0);
    }
    if (count) {
        HIP_TRY(ctx, hipMemcpy(count, b->e5_count, T * kE5MaxRoots * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::fill(count + T * kE5MaxRoots, count + H * kE5MaxRoots, -1);
    }
    if (best_root)
        HIP_TRY(ctx, hipMemcpy(best_root, b->e5_root, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (E) std::memcpy(E, res.E, sizeof(res.E));
    if (best_hyp) *best_hyp = res.best_hyp;
    if (best_count) *best_count = res.best_count;
    if (best_residual) *best_residual = res.best_residual;
    return res.best_count > 0 ? MVS_OK : MVS_NO_MODEL;  // estimator-RANSAC.cpp:89
}

// ---------------------------------------------------------------------------------------------
// frame sequences (row f2)
// ---------------------------------------------------------------------------------------------
mvs_status mvs_seq_create(mvs_ctx *ctx, int n_frames, int max_kp, int desc_bytes, mvs_seq **out)
{
    if (!ctx || !out || n_frames < 3)
        return MVS_ERR_INVALID_ARG;
    *out = nullptr;
    mvs_seq *q = new mvs_seq();
    q->ctx = ctx;
    q->n_frames = n_frames;
    q->n_tracks = n_frames - 2;
    mvs_status st = batch_create_impl(ctx, n_frames - 1, max_kp, desc_bytes, n_frames, &q->batch);
    if (st != MVS_OK) {
        delete q;
        return st;
    }
    q->stride = std::min(max_kp, kPnpMaxPoints);
    const size_t T = q->n_tracks, S = q->stride;
    double *X = nullptr, *uv = nullptr, *xy = nullptr, *fb = nullptr, *K = nullptr, *Kinv = nullptr;
    int32_t *n_corr = nullptr, *inl = nullptr;
    int64_t *gidx = nullptr;
    PnpOut *po = nullptr;
    double *traj_R = nullptr, *traj_t = nullptr, *traj_s = nullptr, *trk_s = nullptr;   // scale-propagation fold outputs
    mvs_seq_scale_step *steps = nullptr;
    DevGroup grp(ctx, q->blocks);
    grp.add(X, T * S * 3);
    grp.add(uv, T * S * 2);
    grp.add(xy, T * S * 2);
    grp.add(fb, T * S * 3);
    grp.add(K, T * 9);
    grp.add(Kinv, T * 9);
    grp.add(n_corr, T);
    grp.add(inl, T * S);
    grp.add(gidx, T);
    grp.add(po, T);
    grp.add(traj_R, (size_t)n_frames * 9);
    grp.add(traj_t, (size_t)n_frames * 3);
    grp.add(traj_s, (size_t)n_frames);
    grp.add(trk_s, (size_t)n_frames);
    grp.add(steps, T);
    if ((st = grp.commit()) != MVS_OK) {
        mvs_seq_destroy(q);
        return st;
    }
    std::vector<int64_t> g(T);
    for (size_t i = 0; i < T; ++i)
        g[i] = (int64_t)i;
    {   // on the ctx stream (it is non-blocking: NULL-stream copies would not be ordered against the kernels that write
        // these buffers later), and with the partly built object released on failure
        hipError_t e = hipMemcpyAsync(gidx, g.data(), T * sizeof(int64_t), hipMemcpyHostToDevice, ctx_stream(ctx));
        if (e == hipSuccess) e = hipMemsetAsync(n_corr, 0, T * sizeof(int32_t), ctx_stream(ctx));
        if (e == hipSuccess) e = hipMemsetAsync(po, 0, T * sizeof(PnpOut), ctx_stream(ctx));
        if (e == hipSuccess) e = sync_stream(ctx);   // `g` lives on this frame
        if (e != hipSuccess) {
            ctx->err = std::string("mvs_seq_create: ") + hipGetErrorString(e);
            mvs_seq_destroy(q);
            return MVS_ERR_HIP;
        }
    }
    const BatchDev &d = q->batch->d;
    q->join.n_tracks = q->n_tracks;
    q->join.max_kp = d.max_kp;
    q->join.stride = q->stride;
    q->join.results = d.results;
    q->join.matches = d.matches;
    q->join.M = d.M;
    q->join.points = d.points;
    q->join.point_idx = d.point_idx;
    q->join.kp = d.kp1;
    q->join.X = X;
    q->join.uv = uv;
    q->join.n_corr = n_corr;
    q->pnp.n_problems = q->n_tracks;
    q->pnp.stride = q->stride;
    q->pnp.n = n_corr;
    q->pnp.gidx = gidx;
    q->pnp.K = K;
    q->pnp.Kinv = Kinv;
    q->pnp.X = X;
    q->pnp.uv = uv;
    q->pnp.xy = xy;
    q->pnp.fb = fb;
    q->pnp.inliers = inl;
    q->pnp.out = po;
    q->chain.n_frames = n_frames;
    q->chain.results = d.results;
    q->chain.tracks = po;
    q->chain.traj_R = traj_R;
    q->chain.traj_t = traj_t;
    q->chain.traj_sigma = traj_s;
    q->chain.track_scale = trk_s;
    q->scale_steps = steps;
    q->pnp.rec = nullptr;
    q->pnp.max_groups = 0;
    *out = q;
    return MVS_OK;
}

void mvs_seq_destroy(mvs_seq *q)
{
    if (!q)
        return;
    (void)hipSetDevice(q->ctx->device);
    (void)sync_stream(q->ctx);
    for (mvs_batch *lb : q->lag_batch)
        if (lb)
            mvs_batch_destroy(lb);
    if (q->loop_batch)
        mvs_batch_destroy(q->loop_batch);
    if (q->batch)
        mvs_batch_destroy(q->batch);
    delete q;
}

mvs_status mvs_seq_upload(mvs_seq *q, int first, int count, const uint8_t *desc, const float *kp, const int32_t *n_kp,
                          const double K[9])
{
    if (!q || first < 0 || count < 1 || first + count > q->n_frames)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    q->loop_scored = q->loop_selected = q->loop_verified = false;   // the table, the list and the batch describe other frames
    const BatchDev &d = q->batch->d;
    hipStream_t s = ctx_stream(ctx);
    const size_t N = d.max_kp, DW = d.desc_words, off = first;
    if (n_kp)
        for (int i = 0; i < count; ++i)
            if (n_kp[i] < 0 || n_kp[i] > (int)N)
                return MVS_ERR_CAPACITY;
    if (desc)
        HIP_TRY(ctx, hipMemcpyAsync((char *)d.desc1 + off * N * DW * 4, desc, (size_t)count * N * DW * 4, hipMemcpyHostToDevice, s));
    if (kp)
        HIP_TRY(ctx, hipMemcpyAsync((char *)d.kp1 + off * N * 2 * sizeof(float), kp, (size_t)count * N * 2 * sizeof(float),
                                    hipMemcpyHostToDevice, s));
    if (n_kp)
        HIP_TRY(ctx, hipMemcpyAsync((char *)d.n1 + off * sizeof(int32_t), n_kp, (size_t)count * sizeof(int32_t),
                                    hipMemcpyHostToDevice, s));
    std::vector<double> kk, ki;
    std::vector<int64_t> gi;
    if (K) {
        if (!affine_K(K))
            return MVS_ERR_BAD_INTRINSICS;
        double inv[9];
        mat3_inverse(K, inv);
        const size_t P = d.n_pairs;
        kk.resize(P * 9);
        ki.resize(P * 9);
        gi.resize(P);
        for (size_t i = 0; i < P; ++i) {
            std::memcpy(&kk[9 * i], K, 9 * sizeof(double));
            std::memcpy(&ki[9 * i], inv, 9 * sizeof(double));
            gi[i] = (int64_t)i;
        }
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<double *>(d.K), kk.data(), P * 9 * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<double *>(d.Kinv), ki.data(), P * 9 * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<int64_t *>(d.gidx), gi.data(), P * sizeof(int64_t), hipMemcpyHostToDevice, s));
        const size_t T = q->n_tracks;
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<double *>(q->pnp.K), kk.data(), T * 9 * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<double *>(q->pnp.Kinv), ki.data(), T * 9 * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

static mvs_status seq_prepare(mvs_seq *q, Estimator est, const mvs_params *tv, const mvs_pnp_params *pp)
{
    if (!q || !pnp_params_ok(pp))
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(tv);
    if (st != MVS_OK)
        return st;
    HIP_TRY(q->ctx, hipSetDevice(q->ctx->device));
    if ((st = ensure_tables(q->batch, est, tv->num_hypotheses)) != MVS_OK)
        return st;
    const int G = pnp_groups(*pp);
    if (G > q->pnp.max_groups) {
        HIP_TRY(q->ctx, sync_stream(q->ctx));   // the records it replaces are freed
        if ((st = DevGroup(q->ctx, q->blocks).add(q->pnp.rec, (size_t)q->n_tracks * G).commit()) != MVS_OK)
            return st;
        q->pnp.max_groups = G;
    }
    set_pnp_params(q->pnp, *pp);
    q->refit_on = pp->refit != 0;
    if (q->refit_on && !q->refit.out &&
        (st = alloc_refine(q->ctx, q->blocks, q->refit, q->n_tracks, q->stride, 1, q->pnp.K)) != MVS_OK)
        return st;
    if (q->refit_on)
        q->refit.cfg = refit_cfg();
    return MVS_OK;
}

// One step of a prepared sequence: pair pipeline, join, PnP (and its optional refit), chain.  ev (mvs_seq_time_stages): five
// events recorded around those four stages; the pair pipeline itself is not instrumented (it keeps its two halves).
static mvs_status seq_enqueue(mvs_seq *q, Estimator est, const RunParams &rp, hipEvent_t *ev = nullptr)
{
    if (ev) HIP_TRY(q->ctx, hipEventRecord(ev[0], ctx_stream(q->ctx)));
    mvs_status st = run_pairs(q->batch, est, rp, q->n_frames - 1);
    if (st != MVS_OK)
        return st;
    hipStream_t s = ctx_stream(q->ctx);   // behind both halves of the pairs: the join reads every pair
    if (ev) HIP_TRY(q->ctx, hipEventRecord(ev[1], s));
    launch_seq_join(q->join, s);
    if (ev) HIP_TRY(q->ctx, hipEventRecord(ev[2], s));
    launch_pnp(q->pnp, s);
    if (q->refit_on)
        launch_pnp_refit(q->pnp, q->refit, kRefitPointSigma, s);
    if (ev) HIP_TRY(q->ctx, hipEventRecord(ev[3], s));
    q->chain.n_corr = q->pnp.n;
    launch_seq_chain(q->chain, s);
    if (ev) HIP_TRY(q->ctx, hipEventRecord(ev[4], s));
    HIP_TRY(q->ctx, hipGetLastError());
    q->ran = true;
    q->wd.n_windows = 0;   // windows of an earlier run are not this run's
    q->track_ran = false;  // nor is its tracking loop
    q->refined_ran = false;  // nor are refined pairs (the batch keeps them downloadable; mvs_seq_track does not start from them)
    q->lags_ran = 0;         // nor are lagged pairs
    q->odo_ran = false;
    q->graph_built = q->graph_opt = false;   // nor is a pose graph
    q->glob_counted = q->glob_built = q->glob_solved = q->glob_cov = false;   // nor is a global problem
    q->rescaled = false;     // nor are the step records of a rescale
    return MVS_OK;
}

mvs_status mvs_seq_run(mvs_seq *q, const mvs_params *two_view, const mvs_pnp_params *pnp)
{
    mvs_status st = seq_prepare(q, Estimator::kEightPoint, two_view, pnp);
    if (st != MVS_OK)
        return st;
    return seq_enqueue(q, Estimator::kEightPoint, to_run(*two_view));
}

// mvs_seq_run with the five-point RANSAC for the n_frames - 1 pairs; the join, PnP, optional refit and chain read the pairs'
// results, masks and points, which do not depend on the estimator
mvs_status mvs_seq_run_essential(mvs_seq *q, const mvs_params *two_view, const mvs_pnp_params *pnp)
{
    mvs_status st = seq_prepare(q, Estimator::kFivePoint, two_view, pnp);
    if (st != MVS_OK)
        return st;
    return seq_enqueue(q, Estimator::kFivePoint, to_run(*two_view));
}

mvs_status mvs_seq_download_hypotheses_run(mvs_seq *q, int first, int count, int32_t *n_run)
{
    if (!q)
        return MVS_ERR_INVALID_ARG;
    return mvs_batch_download_hypotheses_run(q->batch, first, count, n_run);
}

mvs_status mvs_seq_sync(mvs_seq *q)
{
    if (!q)
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(q->ctx, sync_stream(q->ctx));
    return MVS_OK;
}

mvs_status mvs_seq_time(mvs_seq *q, const mvs_params *two_view, const mvs_pnp_params *pnp, int warmup, int steps,
                        float *ms_total)
{
    if (steps < 1 || warmup < 0 || !ms_total)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = seq_prepare(q, Estimator::kEightPoint, two_view, pnp);
    if (st != MVS_OK)
        return st;
    const RunParams rp = to_run(*two_view);
    for (int i = 0; i < warmup; ++i)
        if ((st = seq_enqueue(q, Estimator::kEightPoint, rp)) != MVS_OK)
            return st;
    HIP_TRY(q->ctx, sync_stream(q->ctx));
    HIP_TRY(q->ctx, hipEventRecord(q->batch->ev[5], ctx_stream(q->ctx)));
    for (int i = 0; i < steps; ++i)
        if ((st = seq_enqueue(q, Estimator::kEightPoint, rp)) != MVS_OK)
            return st;
    HIP_TRY(q->ctx, hipEventRecord(q->batch->ev[6], ctx_stream(q->ctx)));   // (the stream is fetched behind every pipeline)
    HIP_TRY(q->ctx, hipEventSynchronize(q->batch->ev[6]));
    HIP_TRY(q->ctx, hipEventElapsedTime(ms_total, q->batch->ev[5], q->batch->ev[6]));
    return MVS_OK;
}

// per-stage HIP-event timing of the sequence step on the kernels' own stream: ms_stage[4] = summed ms over `steps`
// instrumented passes of {pair pipeline, join, pnp_solve (prep + ransac + finalize), chain}.  Every pass is a run
// (seq_enqueue): it leaves the sequence as mvs_seq_run does, what was derived from an earlier run stale
mvs_status mvs_seq_time_stages(mvs_seq *q, const mvs_params *two_view, const mvs_pnp_params *pnp, int steps, float *ms_stage)
{
    if (steps < 1 || !ms_stage)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = seq_prepare(q, Estimator::kEightPoint, two_view, pnp);
    if (st != MVS_OK)
        return st;
    const RunParams rp = to_run(*two_view);
    hipEvent_t *ev = q->batch->ev;
    for (int k = 0; k < 4; ++k)
        ms_stage[k] = 0.f;
    for (int i = 0; i < steps; ++i) {
        if ((st = seq_enqueue(q, Estimator::kEightPoint, rp, ev)) != MVS_OK)
            return st;
        HIP_TRY(q->ctx, hipEventSynchronize(ev[4]));
        for (int k = 0; k < 4; ++k) {
            float ms = 0.f;
            HIP_TRY(q->ctx, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            ms_stage[k] += ms;
        }
    }
    return MVS_OK;
}

mvs_status mvs_seq_download_pairs(mvs_seq *q, int first, int count, mvs_pair_result *results, mvs_match *matches,
                                  uint8_t *inlier_mask, double *points_xyz, int64_t *point_idx)
{
    if (!q)
        return MVS_ERR_INVALID_ARG;
    return mvs_batch_download(q->batch, first, count, results, matches, inlier_mask, points_xyz, point_idx);
}

mvs_status mvs_seq_download_tracks(mvs_seq *q, int first, int count, mvs_track_result *tracks, double *corr_xyz,
                                   double *corr_uv, int64_t *inlier_idx)
{
    if (!q || first < 0 || count < 1 || first + count > q->n_tracks)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sync_stream(ctx));
    const size_t S = q->stride, N = q->batch->d.max_kp, off = first, cnt = count;
    if (tracks) {
        std::vector<PnpOut> po(cnt);
        std::vector<int32_t> nc(cnt);
        HIP_TRY(ctx, hipMemcpy(po.data(), q->pnp.out + off, cnt * sizeof(PnpOut), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(nc.data(), q->pnp.n + off, cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; ++i) {
            mvs_track_result &t = tracks[i];
            t.ok = nc[i] >= 7 ? po[i].ok : 0;
            t.n_corr = nc[i];
            t.n_inliers = t.ok ? po[i].n_inliers : 0;
            t.best_hyp = nc[i] >= 7 ? po[i].best_hyp : -1;
            std::memcpy(t.R, po[i].R, sizeof(t.R));
            std::memcpy(t.t, po[i].t, sizeof(t.t));
        }
    }
    // device layout has `stride` slots per track, the host layout max_kp
    auto fetch = [&](const void *dev, size_t elem_bytes, size_t per, void *host) -> mvs_status {
        std::vector<char> tmp(cnt * S * per * elem_bytes);
        HIP_TRY(ctx, hipMemcpy(tmp.data(), (const char *)dev + off * S * per * elem_bytes, tmp.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; ++i)
            std::memcpy((char *)host + i * N * per * elem_bytes, tmp.data() + i * S * per * elem_bytes, S * per * elem_bytes);
        return MVS_OK;
    };
    mvs_status st = MVS_OK;
    if (corr_xyz && (st = fetch(q->pnp.X, sizeof(double), 3, corr_xyz)) != MVS_OK)
        return st;
    if (corr_uv && (st = fetch(q->pnp.uv, sizeof(double), 2, corr_uv)) != MVS_OK)
        return st;
    if (inlier_idx) {
        std::vector<int32_t> tmp(cnt * S);
        HIP_TRY(ctx, hipMemcpy(tmp.data(), q->pnp.inliers + off * S, tmp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; ++i)
            for (size_t k = 0; k < S; ++k)
                inlier_idx[i * N + k] = tmp[i * S + k];
    }
    return MVS_OK;
}

mvs_status mvs_pnp_params_default(mvs_pnp_params *p)
{
    if (!p)
        return MVS_ERR_INVALID_ARG;
    p->num_hypotheses = 100;  // pnp-solve.cpp:47
    p->sampler = MVS_SAMPLER_PHILOX;
    p->seed = 0;
    p->reproj_error = 0.05;   // pnp-solve.cpp:48
    p->min_inliers = 4;
    p->refit = 0;
    return MVS_OK;
}

mvs_status mvs_pnp_solve(mvs_ctx *ctx, const double *world_xyz, const double *image_uv, int n, const double K[9],
                         const mvs_pnp_params *params, double R[9], double t[3], int64_t *inlier_idx, int *n_inliers,
                         int *best_hyp)
{
    if (!ctx || !world_xyz || !image_uv || !K || !params || !n_inliers)
        return MVS_ERR_INVALID_ARG;
    *n_inliers = 0;
    if (best_hyp)
        *best_hyp = -1;
    if (n < 7 || !pnp_params_ok(params))
        return MVS_ERR_INVALID_ARG;
    if (n > kPnpMaxPoints)
        return MVS_ERR_CAPACITY;
    if (!affine_K(K))
        return MVS_ERR_BAD_INTRINSICS;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int G = pnp_groups(*params);
    // workspace layout: X[3n] uv[2n] xy[2n] fb[3n] | K[9] Kinv[9] | rec[G] | out | inliers[n] n
    Carve L{64};
    const size_t off_x = L.take((size_t)n * 10 * sizeof(double));
    const size_t off_k = L.take(18 * sizeof(double));
    const size_t off_rec = L.take((size_t)G * sizeof(PnpRec));
    const size_t off_out = L.take(sizeof(PnpOut));
    const size_t off_inl = L.take(((size_t)n + 1) * sizeof(int32_t));
    const mvs_status st = ws_grow(ctx, ctx->pnp, L.end);
    if (st != MVS_OK)
        return st;
    char *base = ctx->pnp.ptr();
    double *dX = reinterpret_cast<double *>(base + off_x), *duv = dX + 3 * (size_t)n, *dxy = duv + 2 * (size_t)n, *dfb = dxy + 2 * (size_t)n;
    double *dK = reinterpret_cast<double *>(base + off_k);
    int32_t *dinl = reinterpret_cast<int32_t *>(base + off_inl);
    hipStream_t s = ctx_stream(ctx);
    double kk[18];
    std::memcpy(kk, K, 9 * sizeof(double));
    mat3_inverse(K, kk + 9);
    const int32_t n32 = n;
    HIP_TRY(ctx, hipMemcpyAsync(dX, world_xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(duv, image_uv, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(dK, kk, sizeof(kk), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(dinl + n, &n32, sizeof(n32), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, sync_stream(ctx));
    PnpDev p{};
    p.n_problems = 1;
    p.stride = n;
    set_pnp_params(p, *params);
    p.max_groups = G;
    p.n = dinl + n;
    p.gidx = nullptr;
    p.K = dK;
    p.Kinv = dK + 9;
    p.X = dX;
    p.uv = duv;
    p.xy = dxy;
    p.fb = dfb;
    p.rec = reinterpret_cast<PnpRec *>(base + off_rec);
    p.out = reinterpret_cast<PnpOut *>(base + off_out);
    p.inliers = dinl;
    launch_pnp(p, s);
    HIP_TRY(ctx, sync_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    PnpOut out;
    HIP_TRY(ctx, hipMemcpy(&out, p.out, sizeof(out), hipMemcpyDeviceToHost));
    if (best_hyp)
        *best_hyp = out.best_hyp;
    if (!out.ok)
        return MVS_NO_MODEL;
    *n_inliers = out.n_inliers;
    std::vector<int32_t> tmp;
    if ((inlier_idx || params->refit) && out.n_inliers > 0) {
        tmp.resize(out.n_inliers);
        HIP_TRY(ctx, hipMemcpy(tmp.data(), p.inliers, (size_t)out.n_inliers * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (inlier_idx)
            for (int i = 0; i < out.n_inliers; ++i)
                inlier_idx[i] = tmp[i];
    }
    if (params->refit && out.n_inliers >= 4) {
        // cv::solvePnPRansac ends with a refit over the inliers (pnp-solve.cpp:53-64).  Here: the refinement kernel as
        // a motion-only problem -- the inliers' world points held by a prior of sigma 1e-9 (fixed), identity image
        // covariances (unweighted pixels), no prior on the pose.  A failed refit keeps the RANSAC pose.
        const size_t m = out.n_inliers;
        std::vector<double> X(3 * m), XC(9 * m, 0.0), uv(2 * m);
        for (size_t i = 0; i < m; ++i) {
            std::memcpy(&X[3 * i], world_xyz + 3 * (size_t)tmp[i], 3 * sizeof(double));
            std::memcpy(&uv[2 * i], image_uv + 2 * (size_t)tmp[i], 2 * sizeof(double));
            XC[9 * i] = XC[9 * i + 4] = XC[9 * i + 8] = kRefitPointSigma * kRefitPointSigma;
        }
        const mvs_refine_params rp = refit_params();
        mvs_refine_result rr;
        if (mvs_pnp_refine(ctx, X.data(), XC.data(), uv.data(), nullptr, (int)m, K, out.R, out.t, &rp, &rr) == MVS_OK && rr.ok) {
            std::memcpy(out.R, rr.R, sizeof(out.R));
            std::memcpy(out.t, rr.t, sizeof(out.t));
        }
    }
    if (R) std::memcpy(R, out.R, sizeof(out.R));
    if (t) std::memcpy(t, out.t, sizeof(out.t));
    return MVS_OK;
}

// ---------------------------------------------------------------------------------------------
// refinement (row f4)
void mvs_refine_params_default(mvs_refine_params *p)
{
    if (!p)
        return;
    p->max_iterations = 100;
    p->reserved = 0;
    p->lambda_initial = 1e-5;
    p->lambda_factor = 10.0;
    p->lambda_upper = 1e5;
    p->rel_tol = 1e-12;
    p->abs_tol = 1e-12;
    p->anchor_sigma[0] = p->anchor_sigma[1] = 1e-5;
    p->pose_sigma[0] = p->pose_sigma[1] = 1e-2;
    p->point_sigma = 1e-2;
}

extern "C++" bool mvs_host::refine_params_ok(const mvs_refine_params *p)
{
    return p && p->max_iterations >= 0 && p->lambda_initial >= 0.0 && p->lambda_factor > 1.0 &&
           p->lambda_upper > 0.0 && p->anchor_sigma[0] > 0.0 && p->anchor_sigma[1] > 0.0 && p->pose_sigma[0] > 0.0 &&
           p->pose_sigma[1] > 0.0 && p->point_sigma > 0.0;
}

static RefineCfg to_cfg(const mvs_refine_params &p, int n_frames)
{
    RefineCfg c{};
    c.max_iterations = p.max_iterations;
    c.lambda_initial = p.lambda_initial;
    c.lambda_factor = p.lambda_factor;
    c.lambda_upper = p.lambda_upper;
    c.rel_tol = p.rel_tol;
    c.abs_tol = p.abs_tol;
    // the reference fills diagonal entries 0-2 with its "position" and 3-5 with its "orientation" sigma
    // (sfm-refine.cpp:62-66); GTSAM reads the first three as rotation.  Kept as is: entry k gets sigma[k / 3].
    for (int k = 0; k < 6; ++k) {
        const double a = p.anchor_sigma[k / 3], m = p.pose_sigma[k / 3];
        if (n_frames == 2) {
            c.w[0][k] = 1.0 / (a * a);
            c.w[1][k] = 1.0 / (m * m);
        } else {
            c.w[0][k] = 1.0 / (m * m);
            c.w[1][k] = 0.0;
        }
    }
    return c;
}

// extras of the general two-frame problem (mvs_ba_refine); all null for sfm_refine / pnp_refine
struct RefineExtra {
    const double *poses_all = nullptr;    // frames x 12: every frame's guess
    const uint8_t *valid[2] = {nullptr, nullptr};
    const RefineCfg *cfg = nullptr;       // explicit prior weights
    mvs_refine_result *results_all = nullptr;  // frames records out
};

// one problem through the ctx workspace.  frames: 2 = sfm_refine (obs_a = camera 1, obs_b = camera 2), 1 = pnp_refine
static mvs_status refine_single(mvs_ctx *ctx, int frames, const double *obs_a, const double *cov_a, const double *obs_b,
                                const double *cov_b, const double *pts0, const double *cov3, int m, const double K[9],
                                const double R_guess[9], const double t_guess[3], const mvs_refine_params *params,
                                mvs_refine_result *result, double *points_out, double *point_cov_out,
                                const RefineExtra &ex = RefineExtra())
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t M = (size_t)m;
    // doubles: obs0 2 obs1 2 oinfo0 3 oinfo1 3 pts0 3 pinfo 6 pts 3 tmp 3 pcov 9 cov2a 4 cov2b 4 cov3 9 = 51 per point
    Carve L{64};
    const size_t off_w = L.take((M * 51 + 9 + 12 + 24) * sizeof(double));
    const size_t off_out = L.take(sizeof(mvs_refine_result));
    const size_t off_all = L.take(2 * sizeof(mvs_refine_result));
    const size_t off_m = L.take(64);
    const size_t off_valid0 = L.take(M), off_valid1 = L.take(M);
    const mvs_status st = ws_grow(ctx, ctx->ref, L.total());
    if (st != MVS_OK)
        return st;
    char *base = ctx->ref.ptr();
    double *w = reinterpret_cast<double *>(base + off_w);
    double *obs0 = w, *obs1 = obs0 + 2 * M, *oinfo0 = obs1 + 2 * M, *oinfo1 = oinfo0 + 3 * M, *dp0 = oinfo1 + 3 * M;
    double *pinfo = dp0 + 3 * M, *dpts = pinfo + 6 * M, *dtmp = dpts + 3 * M, *dpcov = dtmp + 3 * M;
    double *c2a = dpcov + 9 * M, *c2b = c2a + 4 * M, *c3 = c2b + 4 * M, *dK = c3 + 9 * M, *dpose = dK + 9, *dpose_all = dpose + 12;
    int32_t *dm = reinterpret_cast<int32_t *>(base + off_m);
    uint8_t *dv0 = reinterpret_cast<uint8_t *>(base + off_valid0), *dv1 = reinterpret_cast<uint8_t *>(base + off_valid1);
    hipStream_t s = ctx_stream(ctx);
    const int32_t m32 = m;
    double pose[12];
    std::memcpy(pose, R_guess, 9 * sizeof(double));
    std::memcpy(pose + 9, t_guess, 3 * sizeof(double));
    HIP_TRY(ctx, hipMemcpyAsync(obs0, obs_a, M * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    if (frames == 2)
        HIP_TRY(ctx, hipMemcpyAsync(obs1, obs_b, M * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    if (cov_a)
        HIP_TRY(ctx, hipMemcpyAsync(c2a, cov_a, M * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    if (frames == 2 && cov_b)
        HIP_TRY(ctx, hipMemcpyAsync(c2b, cov_b, M * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    if (cov3)
        HIP_TRY(ctx, hipMemcpyAsync(c3, cov3, M * 9 * sizeof(double), hipMemcpyHostToDevice, s));
    if (ex.poses_all)
        HIP_TRY(ctx, hipMemcpyAsync(dpose_all, ex.poses_all, (size_t)frames * 12 * sizeof(double), hipMemcpyHostToDevice, s));
    if (ex.valid[0])
        HIP_TRY(ctx, hipMemcpyAsync(dv0, ex.valid[0], M, hipMemcpyHostToDevice, s));
    if (frames == 2 && ex.valid[1])
        HIP_TRY(ctx, hipMemcpyAsync(dv1, ex.valid[1], M, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(dp0, pts0, M * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(dK, K, 9 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(dpose, pose, sizeof(pose), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(dm, &m32, sizeof(m32), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, sync_stream(ctx));  // the staging buffers above live on this frame
    RefineDev d{};
    d.n_problems = 1;
    d.stride = m;
    d.n_frames = frames;
    d.cfg = ex.cfg ? *ex.cfg : to_cfg(*params, frames);
    d.m = dm;
    d.K = dK;
    d.pose0 = dpose;
    d.pose0_all = ex.poses_all ? dpose_all : nullptr;
    d.obs[0] = obs0;
    d.obs[1] = obs1;
    d.oinfo[0] = oinfo0;
    d.oinfo[1] = oinfo1;
    d.pts0 = dp0;
    d.pinfo = pinfo;
    d.pts = dpts;
    d.pts_tmp = dtmp;
    d.point_cov = point_cov_out ? dpcov : nullptr;
    d.out = reinterpret_cast<mvs_refine_result *>(base + off_out);
    d.out_all = ex.results_all ? reinterpret_cast<mvs_refine_result *>(base + off_all) : nullptr;
    launch_refine_prep(d, cov_a ? c2a : nullptr, (frames == 2 && cov_b) ? c2b : nullptr, cov3 ? c3 : nullptr,
                       1.0 / (params->point_sigma * params->point_sigma), oinfo0, oinfo1, pinfo,
                       ex.valid[0] ? dv0 : nullptr, (frames == 2 && ex.valid[1]) ? dv1 : nullptr, s);
    launch_refine(d, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(result, d.out, sizeof(*result), hipMemcpyDeviceToHost, s));
    if (ex.results_all)
        HIP_TRY(ctx, hipMemcpyAsync(ex.results_all, d.out_all, (size_t)frames * sizeof(mvs_refine_result), hipMemcpyDeviceToHost, s));
    if (points_out)
        HIP_TRY(ctx, hipMemcpyAsync(points_out, dpts, M * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (point_cov_out)
        HIP_TRY(ctx, hipMemcpyAsync(point_cov_out, dpcov, M * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return result->ok ? MVS_OK : MVS_NO_MODEL;
}

mvs_status mvs_sfm_refine(mvs_ctx *ctx, const double *p1, const double *cov1, const double *p2, const double *cov2, int m,
                          const double K[9], const double R_guess[9], const double t_guess[3],
                          const double *points_guess, const mvs_refine_params *params, mvs_refine_result *result,
                          double *points_out, double *point_cov_out)
{
    if (!ctx || !p1 || !p2 || !K || !R_guess || !t_guess || !points_guess || !result || !refine_params_ok(params))
        return MVS_ERR_INVALID_ARG;
    std::memset(result, 0, sizeof(*result));
    if (m < 1)
        return MVS_ERR_INVALID_ARG;
    if (m > kMaxKp)
        return MVS_ERR_CAPACITY;
    if (!affine_K(K))
        return MVS_ERR_BAD_INTRINSICS;
    return refine_single(ctx, 2, p1, cov1, p2, cov2, points_guess, nullptr, m, K, R_guess, t_guess, params, result,
                         points_out, point_cov_out);
}

mvs_status mvs_pnp_refine(mvs_ctx *ctx, const double *world, const double *world_cov, const double *image,
                          const double *image_cov, int m, const double K[9], const double R_guess[9],
                          const double t_guess[3], const mvs_refine_params *params, mvs_refine_result *result)
{
    if (!ctx || !world || !world_cov || !image || !K || !R_guess || !t_guess || !result || !refine_params_ok(params))
        return MVS_ERR_INVALID_ARG;
    std::memset(result, 0, sizeof(*result));
    if (m < 1)
        return MVS_ERR_INVALID_ARG;
    if (m > kMaxKp)
        return MVS_ERR_CAPACITY;
    if (!affine_K(K))
        return MVS_ERR_BAD_INTRINSICS;
    return refine_single(ctx, 1, image, image_cov, nullptr, nullptr, world, world_cov, m, K, R_guess, t_guess, params,
                         result, nullptr, nullptr);
}

mvs_status mvs_ba_refine(mvs_ctx *ctx, const mvs_ba_problem *pb, const mvs_refine_params *params, mvs_refine_result *frames_out,
                         double *points_out, double *point_cov_out)
{
    if (!ctx || !pb || !frames_out || !refine_params_ok(params) || !pb->K || !pb->frame_pose || !pb->frame_prior_var ||
        !pb->points || !pb->obs[0] || (pb->n_frames != 1 && pb->n_frames != 2) || (pb->n_frames == 2 && !pb->obs[1]))
        return MVS_ERR_INVALID_ARG;
    std::memset(frames_out, 0, (size_t)pb->n_frames * sizeof(mvs_refine_result));
    if (pb->n_points < 1)
        return MVS_ERR_INVALID_ARG;
    if (pb->n_points > kMaxKp)
        return MVS_ERR_CAPACITY;
    if (!affine_K(pb->K))
        return MVS_ERR_BAD_INTRINSICS;
    RefineCfg cfg = to_cfg(*params, pb->n_frames);
    for (int f = 0; f < pb->n_frames; ++f)
        for (int k = 0; k < 6; ++k) {
            const double v = pb->frame_prior_var[6 * f + k];
            cfg.w[f][k] = v > 0.0 ? 1.0 / v : 0.0;   // <= 0: no prior on this coordinate
        }
    RefineExtra ex;
    ex.poses_all = pb->frame_pose;
    ex.valid[0] = pb->obs_valid[0];
    ex.valid[1] = pb->obs_valid[1];
    ex.cfg = &cfg;
    ex.results_all = frames_out;
    // a NULL point_prior_cov means "no prior on any point": hand the kernel an all-zero covariance table
    std::vector<double> none;
    const double *pc = pb->point_prior_cov;
    if (!pc) {
        none.assign((size_t)pb->n_points * 9, 0.0);
        pc = none.data();
    }
    mvs_refine_result last;
    const double *pose_last = pb->frame_pose + 12 * (pb->n_frames - 1);
    return refine_single(ctx, pb->n_frames, pb->obs[0], pb->obs_cov[0], pb->obs[1], pb->obs_cov[1], pb->points, pc,
                         pb->n_points, pb->K, pose_last, pose_last + 9, params, &last, points_out, point_cov_out, ex);
}

// ---- windows of up to eight frames --------------------------------------------------------------------------------------
// argument errors of one window, in mvs_ba_refine's order (the frame count has been checked by the caller)
static mvs_status window_check(const mvs_ba_window *w)
{
    if (!w->K || !w->frame_pose || !w->frame_prior_var || !w->points || !w->obs)
        return MVS_ERR_INVALID_ARG;
    for (int f = 0; f < w->n_frames; ++f)
        if (!w->obs[f])
            return MVS_ERR_INVALID_ARG;
    if (w->n_points < 1)
        return MVS_ERR_INVALID_ARG;
    if (w->n_points > kMaxKp)
        return MVS_ERR_CAPACITY;
    if (!affine_K(w->K))
        return MVS_ERR_BAD_INTRINSICS;
    return MVS_OK;
}

// covariance -> information with refine_prep_kernel's formulas: a 2 x 2 observation covariance (row-major) to (xx xy yy), a
// 3 x 3 point prior covariance to (xx xy xz yy yz zz)
extern "C++" void mvs_host::obs_cov_to_info(const double *cv, double *o)
{
    const double a = cv[0], b = 0.5 * (cv[1] + cv[2]), dd = cv[3];
    const double id = 1.0 / (a * dd - b * b);
    o[0] = dd * id, o[1] = -(b * id), o[2] = a * id;
}
extern "C++" void mvs_host::point_cov_to_info(const double *C, double *L)
{
    const double a[6] = {C[0], 0.5 * (C[1] + C[3]), 0.5 * (C[2] + C[6]), C[4], 0.5 * (C[5] + C[7]), C[8]};
    const double c00 = a[3] * a[5] - a[4] * a[4], c01 = a[2] * a[4] - a[1] * a[5], c02 = a[1] * a[4] - a[2] * a[3];
    const double id = 1.0 / ((a[0] * c00 + a[1] * c01) + a[2] * c02);
    L[0] = c00 * id, L[1] = c01 * id, L[2] = c02 * id;
    L[3] = (a[0] * a[5] - a[2] * a[2]) * id, L[4] = (a[1] * a[2] - a[0] * a[4]) * id, L[5] = (a[0] * a[3] - a[1] * a[1]) * id;
}

// the inputs of one window in the layout refine_window_kernel reads (WinProblem::in_off); covariances become information
// matrices here
static void window_pack(const mvs_ba_window *w, std::vector<double> &in)
{
    const size_t F = (size_t)w->n_frames, m = (size_t)w->n_points;
    const size_t o_cam = in.size();
    in.resize(o_cam + 8 + 18 * F + 9 * m + 5 * F * m, 0.0);
    double *cam = in.data() + o_cam, *pose = cam + 8, *wt = pose + 12 * F, *p0 = wt + 6 * F, *pinfo = p0 + 3 * m;
    double *obs = pinfo + 6 * m, *oinfo = obs + 2 * F * m;
    cam[0] = w->K[0], cam[1] = w->K[1], cam[2] = w->K[2], cam[3] = w->K[4], cam[4] = w->K[5];
    std::memcpy(pose, w->frame_pose, 12 * F * sizeof(double));
    for (size_t k = 0; k < 6 * F; ++k)
        wt[k] = w->frame_prior_var[k] > 0.0 ? 1.0 / w->frame_prior_var[k] : 0.0;   // <= 0: no prior on this coordinate
    std::memcpy(p0, w->points, 3 * m * sizeof(double));
    for (size_t i = 0; i < m && w->point_prior_cov; ++i) {
        const double *C = w->point_prior_cov + 9 * i;
        if (!(C[0] > 0.0))
            continue;   // no prior on this point
        point_cov_to_info(C, pinfo + 6 * i);
    }
    for (size_t f = 0; f < F; ++f) {
        std::memcpy(obs + 2 * m * f, w->obs[f], 2 * m * sizeof(double));
        const double *cv = w->obs_cov ? w->obs_cov[f] : nullptr;
        const uint8_t *vd = w->obs_valid ? w->obs_valid[f] : nullptr;
        double *o = oinfo + 3 * m * f;
        for (size_t i = 0; i < m; ++i, o += 3) {
            if (vd && !vd[i])
                continue;   // not seen: zero information
            if (!cv)
                o[0] = 1.0, o[2] = 1.0;
            else
                obs_cov_to_info(cv + 4 * i, o);
        }
    }
}

mvs_status mvs_ba_refine_windows(mvs_ctx *ctx, const mvs_ba_window *problems, int n_problems, const mvs_refine_params *params,
                                 mvs_refine_result *frames_out, double *points_out, double *point_cov_out)
{
    if (!ctx || !problems || n_problems < 1 || !frames_out || !refine_params_ok(params))
        return MVS_ERR_INVALID_ARG;
    int Fmax = 0, Mmax = 0;
    for (int p = 0; p < n_problems; ++p) {
        if (problems[p].n_frames < 1)
            return MVS_ERR_INVALID_ARG;
        if (problems[p].n_frames > kWinMaxFrames)
            return MVS_ERR_CAPACITY;
        Fmax = std::max(Fmax, problems[p].n_frames);
    }
    std::memset(frames_out, 0, (size_t)n_problems * Fmax * sizeof(mvs_refine_result));
    for (int p = 0; p < n_problems; ++p) {
        const mvs_status st = window_check(&problems[p]);
        if (st != MVS_OK)
            return st;
        Mmax = std::max(Mmax, problems[p].n_points);
    }
    bool all_ok = true;
    // the batch's windows of three and more frames: one upload, one launch, one download
    std::vector<WinProblem> desc;
    std::vector<int> which;
    std::vector<double> in;
    size_t n_pts = 0, n_fr = 0;
    for (int p = 0; p < n_problems; ++p) {
        const mvs_ba_window &w = problems[p];
        if (w.n_frames <= 2)
            continue;
        WinProblem d{};
        d.n_frames = w.n_frames;
        d.n_points = w.n_points;
        d.in_off = (int64_t)in.size();
        d.pt_off = (int64_t)n_pts;
        d.fr_off = (int64_t)n_fr;
        window_pack(&w, in);
        n_pts += (size_t)w.n_points;
        n_fr += (size_t)w.n_frames;
        desc.push_back(d);
        which.push_back(p);
    }
    if (!desc.empty()) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t G = desc.size(), head = (G * sizeof(WinProblem) + 63) & ~size_t(63);
        // outputs first and contiguous (frames, points, covariances: the download is their prefix), then the candidate
        // points and the uploaded block (descriptors, then inputs)
        Carve L{64};
        const size_t off_out = L.take(n_fr * sizeof(mvs_refine_result));
        const size_t off_pts = L.take(n_pts * 3 * sizeof(double));
        const size_t off_cov = L.take(n_pts * 9 * sizeof(double));
        const size_t off_tmp = L.take(n_pts * 3 * sizeof(double));
        const size_t off_up = L.take(head + in.size() * sizeof(double));
        const mvs_status st = ws_grow(ctx, ctx->win, L.total());
        if (st != MVS_OK)
            return st;
        char *base = ctx->win.ptr();
        std::vector<char> up(head + in.size() * sizeof(double));
        std::memcpy(up.data(), desc.data(), G * sizeof(WinProblem));
        std::memcpy(up.data() + head, in.data(), in.size() * sizeof(double));
        hipStream_t s = ctx_stream(ctx);
        HIP_TRY(ctx, hipMemcpyAsync(base + off_up, up.data(), up.size(), hipMemcpyHostToDevice, s));
        WinDev d{};
        d.n_problems = (int)G;
        d.cfg = to_cfg(*params, 1);
        d.prob = reinterpret_cast<const WinProblem *>(base + off_up);
        d.in = reinterpret_cast<const double *>(base + off_up + head);
        d.pts = reinterpret_cast<double *>(base + off_pts);
        d.pts_tmp = reinterpret_cast<double *>(base + off_tmp);
        d.point_cov = point_cov_out ? reinterpret_cast<double *>(base + off_cov) : nullptr;
        d.out = reinterpret_cast<mvs_refine_result *>(base + off_out);
        launch_refine_window(d, s);
        HIP_TRY(ctx, hipGetLastError());
        const size_t down = point_cov_out ? off_cov + n_pts * 9 * sizeof(double) : points_out ? off_cov : off_pts;
        std::vector<char> host(down);
        HIP_TRY(ctx, hipMemcpyAsync(host.data(), base, down, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, sync_stream(ctx));
        for (size_t g = 0; g < G; ++g) {
            const int p = which[g];
            const size_t F = (size_t)desc[g].n_frames, m = (size_t)desc[g].n_points;
            mvs_refine_result *fo = frames_out + (size_t)p * Fmax;
            std::memcpy(fo, host.data() + off_out + (size_t)desc[g].fr_off * sizeof(mvs_refine_result), F * sizeof(mvs_refine_result));
            all_ok = all_ok && fo[0].ok;
            if (points_out)
                std::memcpy(points_out + (size_t)p * Mmax * 3, host.data() + off_pts + (size_t)desc[g].pt_off * 3 * sizeof(double),
                            m * 3 * sizeof(double));
            if (point_cov_out)
                std::memcpy(point_cov_out + (size_t)p * Mmax * 9, host.data() + off_cov + (size_t)desc[g].pt_off * 9 * sizeof(double),
                            m * 9 * sizeof(double));
        }
    }
    // windows of one or two frames go through mvs_ba_refine, one call each: the bytes mvs_ba_refine returns
    for (int p = 0; p < n_problems; ++p) {
        const mvs_ba_window &w = problems[p];
        if (w.n_frames > 2)
            continue;
        mvs_ba_problem pb{};
        pb.n_frames = w.n_frames;
        pb.n_points = w.n_points;
        pb.K = w.K;
        pb.frame_pose = w.frame_pose;
        pb.frame_prior_var = w.frame_prior_var;
        pb.points = w.points;
        pb.point_prior_cov = w.point_prior_cov;
        for (int f = 0; f < w.n_frames; ++f) {
            pb.obs[f] = w.obs[f];
            pb.obs_cov[f] = w.obs_cov ? w.obs_cov[f] : nullptr;
            pb.obs_valid[f] = w.obs_valid ? w.obs_valid[f] : nullptr;
        }
        const mvs_status st = mvs_ba_refine(ctx, &pb, params, frames_out + (size_t)p * Fmax,
                                            points_out ? points_out + (size_t)p * Mmax * 3 : nullptr,
                                            point_cov_out ? point_cov_out + (size_t)p * Mmax * 9 : nullptr);
        if (st != MVS_OK && st != MVS_NO_MODEL)
            return st;
        all_ok = all_ok && st == MVS_OK;
    }
    return all_ok ? MVS_OK : MVS_NO_MODEL;
}

mvs_status mvs_ba_refine_window(mvs_ctx *ctx, const mvs_ba_window *problem, const mvs_refine_params *params,
                                mvs_refine_result *frames_out, double *points_out, double *point_cov_out)
{
    return mvs_ba_refine_windows(ctx, problem, 1, params, frames_out, points_out, point_cov_out);
}

mvs_status mvs_batch_refine(mvs_batch *b, const mvs_refine_params *params, double sigma_px)
{
    if (!b || !refine_params_ok(params) || !(sigma_px > 0.0))
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const BatchDev &bd = b->d;
    const size_t P = bd.n_pairs, N = bd.max_kp;
    RefineDev &d = b->refine;
    if (!d.out) {
        mvs_status st = alloc_refine(ctx, b->blocks, d, (int)P, (int)N, 2, bd.K);
        if (st != MVS_OK)
            return st;
    }
    d.cfg = to_cfg(*params, 2);
    hipStream_t s = ctx_stream(ctx);
    launch_refine_gather(bd, (int)P, sigma_px, params->point_sigma, d.stride, const_cast<int32_t *>(d.m),
                         const_cast<double *>(d.pose0), const_cast<double *>(d.obs[0]), const_cast<double *>(d.obs[1]),
                         const_cast<double *>(d.oinfo[0]), const_cast<double *>(d.oinfo[1]),
                         const_cast<double *>(d.pts0), const_cast<double *>(d.pinfo), s);
    launch_refine(d, s);
    HIP_TRY(ctx, hipGetLastError());
    b->refine_ran = true;
    return MVS_OK;
}

mvs_status mvs_batch_download_refined(mvs_batch *b, mvs_refine_result *refined, double *points_xyz, double *point_cov)
{
    if (!b || !refined || !b->refine_ran)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const RefineDev &d = b->refine;
    const size_t P = d.n_problems, N = d.stride;
    hipStream_t s = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(refined, d.out, P * sizeof(mvs_refine_result), hipMemcpyDeviceToHost, s));
    if (points_xyz)
        HIP_TRY(ctx, hipMemcpyAsync(points_xyz, d.pts, P * N * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (point_cov)
        HIP_TRY(ctx, hipMemcpyAsync(point_cov, d.point_cov, P * N * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_download_trajectory(mvs_seq *q, double *R, double *t, double *pair_scale, double *track_scale)
{
    if (!q)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    const size_t F = q->n_frames;
    if (R)
        HIP_TRY(ctx, hipMemcpyAsync(R, q->chain.traj_R, F * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (t)
        HIP_TRY(ctx, hipMemcpyAsync(t, q->chain.traj_t, F * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (pair_scale)
        HIP_TRY(ctx, hipMemcpyAsync(pair_scale, q->chain.traj_sigma, (F - 1) * sizeof(double), hipMemcpyDeviceToHost, s));
    if (track_scale)
        HIP_TRY(ctx, hipMemcpyAsync(track_scale, q->chain.track_scale, (F - 2) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

// The trajectory of the last run by another rule, over the chain's outputs.  What read the old trajectory is retired as
// seq_enqueue retires it; what does not read it (pairs, tracks, refined pairs, lags, tracking, odometry) stays.
mvs_status mvs_seq_rescale(mvs_seq *q, const mvs_seq_scale_params *p)
{
    if (!q || !p || !q->ran || (p->rule != MVS_SEQ_SCALE_CHAIN && p->rule != MVS_SEQ_SCALE_DEPTH_RATIO) || p->min_common < 1)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    if (p->rule == MVS_SEQ_SCALE_CHAIN) {
        HIP_TRY(ctx, hipMemsetAsync(q->scale_steps, 0, (size_t)q->n_tracks * sizeof(mvs_seq_scale_step), s));
        launch_seq_chain(q->chain, s);
    } else {
        const BatchDev &bd = q->batch->d;
        SeqScaleDev d{};
        d.n_frames = q->n_frames;
        d.max_kp = bd.max_kp;
        d.min_common = p->min_common;
        d.results = bd.results;
        d.matches = bd.matches;
        d.point_idx = bd.point_idx;
        d.points = bd.points;
        d.steps = q->scale_steps;
        d.traj_R = q->chain.traj_R;
        d.traj_t = q->chain.traj_t;
        d.traj_sigma = q->chain.traj_sigma;
        d.track_scale = q->chain.track_scale;
        launch_seq_rescale(d, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    q->rescaled = true;
    q->wd.n_windows = 0;                                                       // windows of the old trajectory
    q->graph_built = q->graph_opt = false;                                     // its pose graph
    q->glob_counted = q->glob_built = q->glob_solved = q->glob_cov = false;    // its global problem
    return MVS_OK;
}

mvs_status mvs_seq_download_scale_steps(mvs_seq *q, mvs_seq_scale_step *steps)
{
    if (!q || !steps || !q->rescaled)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(steps, q->scale_steps, (size_t)q->n_tracks * sizeof(mvs_seq_scale_step), hipMemcpyDeviceToHost,
                                ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_refine_pairs(mvs_seq *q, const mvs_refine_params *params, double sigma_px)
{
    if (!q)
        return MVS_ERR_INVALID_ARG;
    const mvs_status st = mvs_batch_refine(q->batch, params, sigma_px);
    if (st == MVS_OK)
        q->refined_ran = q->ran;
    return st;
}

// ---- sliding windows of a sequence that has been run ------------------------------------------------------------------
// the fields that shape the windows (sigma_px only weighs the observations: mvs_seq_refine_windows checks it)
static bool seq_window_shape_ok(const mvs_seq_window_params *wp)
{
    return wp && wp->window_frames >= 3 && wp->window_frames <= kWinMaxFrames && wp->stride >= 1 && wp->max_points >= 1 &&
           wp->max_points <= kMaxKp;
}

int mvs_seq_window_count(const mvs_seq *q, const mvs_seq_window_params *wp)
{
    if (!q || !seq_window_shape_ok(wp) || q->n_frames < wp->window_frames)
        return 0;
    return (q->n_frames - wp->window_frames) / wp->stride + 1;
}

mvs_status mvs_seq_refine_windows(mvs_seq *q, const mvs_seq_window_params *wp, const mvs_refine_params *params)
{
    if (!q || !seq_window_shape_ok(wp) || !(wp->sigma_px > 0.0) || !refine_params_ok(params) || !q->ran ||
        q->n_frames < wp->window_frames)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const BatchDev &bd = q->batch->d;
    const size_t W = (size_t)mvs_seq_window_count(q, wp), F = (size_t)wp->window_frames, cap = (size_t)wp->max_points;
    const size_t NF = (size_t)q->n_frames, N = (size_t)bd.max_kp;
    const size_t in_stride = 8 + 18 * F + 9 * cap + 5 * F * cap;
    // every window owns a fixed share of each array, so the offsets are known before the device has counted a point.
    // Outputs first (what the download reads), then the candidate points, the problems and the link tables
    Carve L{64};
    const size_t off_info = L.take(W * sizeof(mvs_seq_window_info));
    const size_t off_out = L.take(W * F * sizeof(mvs_refine_result));
    const size_t off_pts = L.take(W * cap * 3 * sizeof(double));
    const size_t off_cov = L.take(W * cap * 9 * sizeof(double));
    const size_t off_tkp = L.take(W * cap * F * sizeof(int32_t));
    const size_t off_guess = L.take(W * cap * 3 * sizeof(double));
    const size_t off_zero_end = off_tkp;   // records, points and covariances are cleared before every solve
    const size_t off_tmp = L.take(W * cap * 3 * sizeof(double));
    const size_t off_prob = L.take(W * sizeof(WinProblem));
    const size_t off_in = L.take(W * in_stride * sizeof(double));
    const size_t off_succ = L.take((NF - 1) * N * sizeof(int32_t));
    const size_t off_pred = L.take(NF * N * sizeof(int32_t));
    const size_t off_rtp = L.take((NF - 1) * N * sizeof(int32_t));
    q->wd.n_windows = 0;   // growing frees the block an earlier call's results live in
    const mvs_status st = ws_grow(ctx, q->win, L.total());
    if (st != MVS_OK)
        return st;
    char *base = q->win.ptr();
    SeqWinDev d{};
    d.n_frames = q->n_frames;
    d.max_kp = bd.max_kp;
    d.F = wp->window_frames;
    d.stride = wp->stride;
    d.max_points = wp->max_points;
    d.n_windows = (int)W;
    d.results = bd.results;
    d.matches = bd.matches;
    d.mask = bd.mask;
    d.points = bd.points;
    d.point_idx = bd.point_idx;
    d.kp = bd.kp1;
    d.oct = bd.oct1;
    d.K = bd.K;
    d.traj_R = q->chain.traj_R;
    d.traj_t = q->chain.traj_t;
    d.traj_sigma = q->chain.traj_sigma;
    d.succ = reinterpret_cast<int32_t *>(base + off_succ);
    d.pred = reinterpret_cast<int32_t *>(base + off_pred);
    d.row_to_point = reinterpret_cast<int32_t *>(base + off_rtp);
    // the prior weights as mvs_seq_refine_pairs applies them (to_cfg), the information matrices as window_pack derives them
    // from the covariances sigma^2 I
    const RefineCfg two = to_cfg(*params, 2);
    for (int k = 0; k < 6; ++k) {
        d.w_anchor[k] = two.w[0][k];
        d.w_pose[k] = two.w[1][k];
    }
    const double pv = params->point_sigma * params->point_sigma;
    const double pc[9] = {pv, 0.0, 0.0, 0.0, pv, 0.0, 0.0, 0.0, pv};
    point_cov_to_info(pc, d.pinfo);
    for (int oc = 0; oc <= kSeqWinMaxOctave; ++oc) {
        const double sd = std::ldexp(wp->sigma_px, oc);   // VisualFeature::get_point_estimates: stddev = 2^octave * sigma_px
        const double cv[4] = {sd * sd, 0.0, 0.0, sd * sd};
        obs_cov_to_info(cv, d.oinfo[oc]);
    }
    d.prob = reinterpret_cast<WinProblem *>(base + off_prob);
    d.in = reinterpret_cast<double *>(base + off_in);
    d.in_stride = (int64_t)in_stride;
    d.info = reinterpret_cast<mvs_seq_window_info *>(base + off_info);
    d.track_kp = reinterpret_cast<int32_t *>(base + off_tkp);
    d.point_guess = reinterpret_cast<double *>(base + off_guess);
    WinDev s{};
    s.n_problems = (int)W;
    s.cfg = to_cfg(*params, 1);
    s.prob = d.prob;
    s.in = d.in;
    s.pts = reinterpret_cast<double *>(base + off_pts);
    s.pts_tmp = reinterpret_cast<double *>(base + off_tmp);
    s.point_cov = reinterpret_cast<double *>(base + off_cov);
    s.out = reinterpret_cast<mvs_refine_result *>(base + off_out);
    hipStream_t stream = ctx_stream(ctx);
    // a window without points is left alone by the window kernel: its records read ok = 0
    HIP_TRY(ctx, hipMemsetAsync(base + off_out, 0, off_zero_end - off_out, stream));
    launch_seq_windows(d, stream);
    launch_refine_window(s, stream);
    HIP_TRY(ctx, hipGetLastError());
    q->wd = d;
    q->ws = s;
    return MVS_OK;
}

mvs_status mvs_seq_download_windows(mvs_seq *q, mvs_seq_window_info *info, mvs_refine_result *frames, double *points,
                                    double *point_cov, int32_t *track_kp, double *point_guess)
{
    if (!q || q->wd.n_windows < 1)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SeqWinDev &d = q->wd;
    const size_t W = (size_t)d.n_windows, F = (size_t)d.F, cap = (size_t)d.max_points;
    hipStream_t s = ctx_stream(ctx);
    std::vector<mvs_refine_result> own;
    if (!frames) {   // the status needs the records
        own.resize(W * F);
        frames = own.data();
    }
    HIP_TRY(ctx, hipMemcpyAsync(frames, q->ws.out, W * F * sizeof(mvs_refine_result), hipMemcpyDeviceToHost, s));
    if (info)
        HIP_TRY(ctx, hipMemcpyAsync(info, d.info, W * sizeof(mvs_seq_window_info), hipMemcpyDeviceToHost, s));
    if (points)
        HIP_TRY(ctx, hipMemcpyAsync(points, q->ws.pts, W * cap * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (point_cov)
        HIP_TRY(ctx, hipMemcpyAsync(point_cov, q->ws.point_cov, W * cap * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (track_kp)
        HIP_TRY(ctx, hipMemcpyAsync(track_kp, d.track_kp, W * cap * F * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (point_guess)
        HIP_TRY(ctx, hipMemcpyAsync(point_guess, d.point_guess, W * cap * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    for (size_t w = 0; w < W; ++w)
        if (!frames[w * F].ok)
            return MVS_NO_MODEL;
    return MVS_OK;
}

// ---- the tracking loop of a sequence that has been run ---------------------------------------
void mvs_vo_params_default(mvs_vo_params *p)
{
    if (!p)
        return;
    p->init_pair = 0;
    p->use_refined_init = 0;
    p->min_pnp_point_count = 7;   // visual-odometer.cpp:86-87
    p->reserved = 0;
    p->max_error = 0.5;           // :77-78
    p->anchor_var[0] = p->anchor_var[1] = 1e-3;         // :684-699: the identity times the stddev itself
    p->regulator_var[0] = p->regulator_var[1] = 1e-2;
    p->point_sigma = 1e-2;        // :728-730
    p->sigma_px = 0.5;            // visual-feature.cpp:203
}

// what mvs_seq_track and mvs_seq_odometry both refuse: everything but the choice of the initial pair
static bool track_args_ok(const mvs_seq *q, const mvs_vo_params *vp, const mvs_pnp_params *pp, const mvs_refine_params *rp)
{
    return q && vp && pnp_params_ok(pp) && refine_params_ok(rp) && q->ran && vp->sigma_px > 0.0 && vp->point_sigma > 0.0 &&
           vp->anchor_var[0] > 0.0 && vp->anchor_var[1] > 0.0 && vp->regulator_var[0] > 0.0 && vp->regulator_var[1] > 0.0;
}

// The block's layout and the launches of a run whose arguments have been checked.  mvs_seq_track: ip = nullptr, the map
// starts from pair k0 (vo_init_kernel).  mvs_seq_odometry: ip = the queue's parameters, k0 = 0, and the queue's two kernels
// follow every step.
static mvs_status seq_track_enqueue(mvs_seq *q, const mvs_vo_params *vp, int k0, bool use_refined, const mvs_vo_init_params *ip,
                                    const mvs_pnp_params *pp, const mvs_refine_params *rp)
{
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const BatchDev &bd = q->batch->d;
    const size_t F = (size_t)q->n_frames, N = (size_t)bd.max_kp, G = (size_t)pnp_groups(*pp);
    const size_t D = sizeof(double), I = sizeof(int32_t);
    // what the downloads read first (cleared before every run), then the maps' ids (set to -1), then one step's scratch
    Carve L{64};
    const size_t off_frames = L.take(F * sizeof(mvs_track_frame));
    const size_t off_ncand = L.take(F * I), off_m = L.take(F * I);
    const size_t off_pnp = L.take(F * sizeof(PnpOut));
    const size_t off_ba = L.take(F * 2 * sizeof(mvs_refine_result));
    const size_t off_pose = L.take(F * 24 * D);
    const size_t off_ca = L.take(F * N * I), off_cb = L.take(F * N * I), off_inl = L.take(F * N * I);
    const size_t off_pid = L.take(F * N * I), off_pkp = L.take(F * N * 2 * I), off_pnew = L.take(F * N);
    const size_t off_cX = L.take(F * N * 3 * D), off_cuv = L.take(F * N * 2 * D), off_guess = L.take(F * N * 3 * D);
    const size_t off_pts = L.take(F * N * 3 * D), off_mX = L.take(F * N * 3 * D);
    const size_t off_state = L.take(2 * I), off_T = L.take(12 * D), off_gidx = L.take(F * sizeof(int64_t));
    const size_t off_mid = L.take(F * N * I);
    const size_t off_scratch = L.take(0);
    const size_t off_xy = L.take(N * 2 * D), off_fb = L.take(N * 3 * D), off_rec = L.take(G * sizeof(PnpRec));
    const size_t off_obs0 = L.take(N * 2 * D), off_obs1 = L.take(N * 2 * D), off_cov0 = L.take(N * 4 * D);
    const size_t off_cov1 = L.take(N * 4 * D), off_cov3 = L.take(N * 9 * D), off_oi0 = L.take(N * 3 * D);
    const size_t off_oi1 = L.take(N * 3 * D), off_pinfo = L.take(N * 6 * D), off_tmp = L.take(N * 3 * D);
    // pnp_solve's refit: a one-frame problem over the step's inliers
    const size_t off_robs = L.take(N * 2 * D), off_roi = L.take(N * 3 * D), off_rp0 = L.take(N * 3 * D);
    const size_t off_rpinfo = L.take(N * 6 * D), off_rpts = L.take(N * 3 * D), off_rtmp = L.take(N * 3 * D);
    const size_t off_rpose = L.take(12 * D), off_rm = L.take(I), off_rout = L.take(sizeof(mvs_refine_result));
    // the queue of mvs_seq_odometry, behind everything mvs_seq_track lays out
    const size_t off_odo = L.take(ip ? F * sizeof(mvs_odo_frame) : 0), off_held = L.take(ip ? F * sizeof(OdoHeld) : 0);
    const size_t off_q = L.take(ip ? kOdoWords * I : 0), off_odo_end = L.take(0);
    q->track_ran = false;   // growing frees the block an earlier call's results live in
    q->odo_ran = false;
    const mvs_status st = ws_grow(ctx, q->trk, L.total());
    if (st != MVS_OK)
        return st;
    char *base = q->trk.ptr();
    auto dbl = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    auto i32 = [&](size_t off) { return reinterpret_cast<int32_t *>(base + off); };
    VoDev d{};
    d.n_frames = q->n_frames;
    d.max_kp = bd.max_kp;
    d.k0 = k0;
    d.use_refined = use_refined;
    d.min_pnp_points = vp->min_pnp_point_count;
    d.max_error = vp->max_error;
    d.sigma_px = vp->sigma_px;
    d.point_var = vp->point_sigma * vp->point_sigma;
    d.results = bd.results;
    d.matches = bd.matches;
    d.points = bd.points;
    d.point_idx = bd.point_idx;
    d.kp = bd.kp1;
    d.oct = bd.oct1;
    d.refined = d.use_refined ? q->batch->refine.out : nullptr;
    d.refined_pts = d.use_refined ? q->batch->refine.pts : nullptr;
    d.state = i32(off_state);
    d.T_last = dbl(off_T);
    d.gidx = reinterpret_cast<int64_t *>(base + off_gidx);
    d.frames = reinterpret_cast<mvs_track_frame *>(base + off_frames);
    d.map_id = i32(off_mid);
    d.map_X = dbl(off_mX);
    d.n_cand = i32(off_ncand);
    d.cand_a = i32(off_ca);
    d.cand_b = i32(off_cb);
    d.cand_X = dbl(off_cX);
    d.cand_uv = dbl(off_cuv);
    d.pnp_out = reinterpret_cast<PnpOut *>(base + off_pnp);
    d.inliers = i32(off_inl);
    d.m = i32(off_m);
    d.pt_id = i32(off_pid);
    d.pt_kp = i32(off_pkp);
    d.pt_new = reinterpret_cast<uint8_t *>(base + off_pnew);
    d.guess = dbl(off_guess);
    d.pose0 = dbl(off_pose);
    d.ba_out = reinterpret_cast<mvs_refine_result *>(base + off_ba);
    d.pts = dbl(off_pts);
    d.obs0 = dbl(off_obs0);
    d.obs1 = dbl(off_obs1);
    d.cov0 = dbl(off_cov0);
    d.cov1 = dbl(off_cov1);
    d.cov3 = dbl(off_cov3);
    // the step's PnP: mvs_pnp_solve's problem, one slice per frame
    PnpDev p{};
    p.n_problems = 1;
    p.stride = (int)N;
    set_pnp_params(p, *pp);
    p.max_groups = (int)G;
    p.K = q->pnp.K;
    p.Kinv = q->pnp.Kinv;
    p.xy = dbl(off_xy);
    p.fb = dbl(off_fb);
    p.rec = reinterpret_cast<PnpRec *>(base + off_rec);
    RefineDev rf{};   // its refit, as seq_prepare sets it up for the tracks
    rf.n_problems = 1;
    rf.stride = (int)N;
    rf.n_frames = 1;
    rf.cfg = refit_cfg();
    rf.m = i32(off_rm);
    rf.K = q->pnp.K;
    rf.pose0 = dbl(off_rpose);
    rf.obs[0] = dbl(off_robs);
    rf.oinfo[0] = dbl(off_roi);
    rf.pts0 = dbl(off_rp0);
    rf.pinfo = dbl(off_rpinfo);
    rf.pts = dbl(off_rpts);
    rf.pts_tmp = dbl(off_rtmp);
    rf.out = reinterpret_cast<mvs_refine_result *>(base + off_rout);
    // the step's BA: mvs_ba_refine's problem (refine_single with RefineExtra), prior weights from the variances
    RefineDev ba{};
    ba.n_problems = 1;
    ba.stride = (int)N;
    ba.n_frames = 2;
    ba.cfg = to_cfg(*rp, 2);
    for (int k = 0; k < 6; ++k) {
        ba.cfg.w[0][k] = 1.0 / vp->anchor_var[k / 3];
        ba.cfg.w[1][k] = 1.0 / vp->regulator_var[k / 3];
    }
    ba.K = bd.K;
    ba.obs[0] = d.obs0;
    ba.obs[1] = d.obs1;
    ba.oinfo[0] = dbl(off_oi0);
    ba.oinfo[1] = dbl(off_oi1);
    ba.pinfo = dbl(off_pinfo);
    ba.pts_tmp = dbl(off_tmp);
    hipStream_t s = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemsetAsync(base, 0, off_mid, s));
    HIP_TRY(ctx, hipMemsetAsync(base + off_mid, 0xff, off_scratch - off_mid, s));
    OdoDev o{};
    if (ip) {
        o.queue_size = ip->frame_queue_size;
        o.min_inliers = ip->min_match_inlier_count;
        o.max_error = vp->max_error;
        o.max_rot_sq = ip->max_rotation_magnitude * ip->max_rotation_magnitude;
        o.max_tz = ip->max_translation_z;
        o.lags = q->lagws.ptr<LagDev>();
        o.odo = reinterpret_cast<mvs_odo_frame *>(base + off_odo);
        o.held = reinterpret_cast<OdoHeld *>(base + off_held);
        o.q = i32(off_q);
        HIP_TRY(ctx, hipMemsetAsync(base + off_odo, 0, off_odo_end - off_odo, s));
        launch_vo_odo_begin(d, o, s);
        launch_vo_queue(d, o, 1, s);   // frame 1 cannot be a tracking step: its step's kernels are not enqueued
        launch_vo_map_init(d, o, 1, s);
    } else {
        launch_vo_init(d, s);
    }
    for (int f = d.k0 + 2; f < q->n_frames; ++f) {
        const size_t of = (size_t)f * N;
        launch_vo_join(d, f, s);
        p.n = d.n_cand + f;
        p.gidx = d.gidx + f;
        p.X = d.cand_X + 3 * of;
        p.uv = d.cand_uv + 2 * of;
        p.inliers = const_cast<int32_t *>(d.inliers) + of;
        p.out = const_cast<PnpOut *>(d.pnp_out) + f;
        launch_pnp(p, s);
        if (pp->refit)
            launch_pnp_refit(p, rf, kRefitPointSigma, s);
        launch_vo_assemble(d, f, s);
        ba.m = d.m + f;
        ba.pose0_all = d.pose0 + 24 * (size_t)f;
        ba.pose0 = ba.pose0_all + 12;
        ba.pts0 = d.guess + 3 * of;
        ba.pts = const_cast<double *>(d.pts) + 3 * of;
        ba.out_all = const_cast<mvs_refine_result *>(d.ba_out) + 2 * (size_t)f;
        ba.out = ba.out_all + 1;
        launch_refine_prep(ba, d.cov0, d.cov1, d.cov3, 1.0 / d.point_var, const_cast<double *>(ba.oinfo[0]),
                           const_cast<double *>(ba.oinfo[1]), const_cast<double *>(ba.pinfo), d.pt_new + of, nullptr, s);
        launch_refine(ba, s);
        launch_vo_commit(d, f, s);
        if (ip) {
            launch_vo_queue(d, o, f, s);
            launch_vo_map_init(d, o, f, s);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    q->vo = d;
    q->track_ran = true;
    if (ip) {
        q->odo = o;
        q->odo_ran = true;
    }
    return MVS_OK;
}

mvs_status mvs_seq_track(mvs_seq *q, const mvs_vo_params *vp, const mvs_pnp_params *pp, const mvs_refine_params *rp)
{
    if (!track_args_ok(q, vp, pp, rp) || vp->init_pair < 0 || vp->init_pair > q->n_frames - 2 ||
        (vp->use_refined_init && !q->refined_ran))
        return MVS_ERR_INVALID_ARG;
    return seq_track_enqueue(q, vp, vp->init_pair, vp->use_refined_init != 0, nullptr, pp, rp);
}

// ---- lagged pairs and VisualOdometer::add_frame over them ------------------------------------------
mvs_status mvs_seq_run_lags(mvs_seq *q, const mvs_params *two_view, int max_lag, int essential, const mvs_refine_params *rp,
                            double sigma_px)
{
    if (!q || !q->ran || max_lag < 1 || max_lag >= q->n_frames || !refine_params_ok(rp) || !(sigma_px > 0.0))
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(two_view);
    if (st != MVS_OK)
        return st;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    q->lags_ran = 0;
    q->graph_built = q->graph_opt = false;   // a graph of the lags this call overwrites
    const BatchDev &bd = q->batch->d;
    const size_t F = (size_t)q->n_frames;
    const Estimator est = essential ? Estimator::kFivePoint : Estimator::kEightPoint;
    if ((int)q->lag_batch.size() < max_lag + 1)
        q->lag_batch.resize((size_t)max_lag + 1, nullptr);
    for (int lag = 2; lag <= max_lag; ++lag) {
        if (!q->lag_batch[lag] && (st = batch_create_impl(ctx, q->n_frames - lag, bd.max_kp, bd.desc_words * 4, q->n_frames,
                                                          &q->lag_batch[lag], &bd, lag)) != MVS_OK)
            return st;
        if ((st = ensure_tables(q->lag_batch[lag], est, two_view->num_hypotheses)) != MVS_OK)
            return st;
    }
    if (max_lag > q->lag_cap) {
        Carve L{64};
        L.take(((size_t)max_lag + 1) * sizeof(LagDev));
        L.take(((size_t)max_lag + 1) * F * sizeof(int32_t));
        if ((st = ws_grow(ctx, q->lagws, L.total())) != MVS_OK)
            return st;
        q->lag_cap = max_lag;
    }
    const size_t off_ssd = Carve{64}.up(((size_t)q->lag_cap + 1) * sizeof(LagDev));
    int32_t *ssd = reinterpret_cast<int32_t *>(q->lagws.ptr() + off_ssd);
    const RunParams run = to_run(*two_view);
    // a failure on the way leaves lags_ran = 0: nothing reads a half-run set of lags
    for (int lag = 1; lag <= max_lag; ++lag) {
        mvs_batch *b = lag == 1 ? q->batch : q->lag_batch[lag];
        const int n = q->n_frames - lag;
        if (lag > 1 && (st = run_pairs(b, est, run, n)) != MVS_OK)
            return st;
        if ((st = mvs_batch_refine(b, rp, sigma_px)) != MVS_OK)
            return st;
        // the stream is fetched behind the pipeline: it may have left the side lane open, and this reads every pair
        launch_pair_ssd(b->d.results, b->d.matches, b->d.point_idx, n, bd.max_kp, ssd + (size_t)lag * F, ctx_stream(ctx));
    }
    HIP_TRY(ctx, hipGetLastError());
    hipStream_t s = ctx_stream(ctx);
    q->lag_host.assign((size_t)q->lag_cap + 1, LagDev{});
    for (int lag = 1; lag <= max_lag; ++lag) {
        const mvs_batch *b = lag == 1 ? q->batch : q->lag_batch[lag];
        q->lag_host[lag] = LagDev{b->d.results, b->d.matches, b->d.point_idx, ssd + (size_t)lag * F, b->refine.out, b->refine.pts};
    }
    for (int lag = 1; lag <= max_lag; ++lag)   // the entry travels as a kernel argument: no host buffer has to outlive the call
        launch_lag_table_set(q->lagws.ptr<LagDev>(), lag, q->lag_host[lag], s);
    HIP_TRY(ctx, hipGetLastError());
    q->refined_ran = true;   // lag 1's refinement is mvs_seq_refine_pairs
    q->lags_ran = max_lag;
    return MVS_OK;
}

mvs_status mvs_seq_download_lag_pairs(mvs_seq *q, int lag, mvs_pair_result *results, mvs_match *matches, uint8_t *inlier_mask,
                                      double *points_xyz, int64_t *point_idx, int32_t *match_ssd)
{
    if (!q || lag < 1 || lag > q->lags_ran)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    const int n = q->n_frames - lag;
    if (match_ssd) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipMemcpyAsync(match_ssd, q->lag_host[lag].ssd, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx_stream(ctx)));
    }
    return mvs_batch_download(lag == 1 ? q->batch : q->lag_batch[lag], 0, n, results, matches, inlier_mask, points_xyz, point_idx);
}

mvs_status mvs_seq_download_lag_refined(mvs_seq *q, int lag, mvs_refine_result *refined, double *points_xyz, double *point_cov)
{
    if (!q || lag < 1 || lag > q->lags_ran)
        return MVS_ERR_INVALID_ARG;
    return mvs_batch_download_refined(lag == 1 ? q->batch : q->lag_batch[lag], refined, points_xyz, point_cov);
}

void mvs_vo_init_params_default(mvs_vo_init_params *p)
{
    if (!p)
        return;
    p->frame_queue_size = 10;          // visual-odometer.cpp:71-72
    p->min_match_inlier_count = 20;    // :74-75
    p->max_rotation_magnitude = 0.1;   // :80-81
    p->max_translation_z = 0.1;        // :83-84
}

mvs_status mvs_seq_odometry(mvs_seq *q, const mvs_vo_params *vp, const mvs_vo_init_params *ip, const mvs_pnp_params *pp,
                            const mvs_refine_params *rp)
{
    // init_pair and use_refined_init are not looked at: the queue chooses the pair, and it is always a refined one
    if (!track_args_ok(q, vp, pp, rp) || !ip || ip->frame_queue_size < 2 || ip->min_match_inlier_count < 0 ||
        !(ip->max_rotation_magnitude >= 0.0) || !(ip->max_translation_z >= 0.0) || !(vp->max_error >= 0.0) ||
        q->lags_ran < std::min(ip->frame_queue_size, q->n_frames - 1))
        return MVS_ERR_INVALID_ARG;
    return seq_track_enqueue(q, vp, 0, false, ip, pp, rp);
}

mvs_status mvs_seq_download_odometry_frames(mvs_seq *q, mvs_odo_frame *odo)
{
    if (!q || !odo || !q->track_ran || !q->odo_ran)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(odo, q->odo.odo, (size_t)q->n_frames * sizeof(mvs_odo_frame), hipMemcpyDeviceToHost, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_download_track_frames(mvs_seq *q, mvs_track_frame *frames)
{
    if (!q || !frames || !q->track_ran)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(frames, q->vo.frames, (size_t)q->n_frames * sizeof(mvs_track_frame), hipMemcpyDeviceToHost,
                                ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_download_track_map(mvs_seq *q, int frame, int32_t *point_id, double *X)
{
    if (!q || !q->track_ran || frame < 0 || frame >= q->n_frames)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)q->vo.max_kp, of = (size_t)frame * N;
    hipStream_t s = ctx_stream(ctx);
    if (point_id)
        HIP_TRY(ctx, hipMemcpyAsync(point_id, q->vo.map_id + of, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (X)
        HIP_TRY(ctx, hipMemcpyAsync(X, q->vo.map_X + 3 * of, N * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_download_track_step(mvs_seq *q, int frame, int32_t *cand_base_kp, int32_t *cand_new_kp, double *cand_xyz,
                                       double *cand_uv, int32_t *pnp_inlier_idx, int32_t *point_id, int32_t *point_kp,
                                       uint8_t *point_is_new, double *point_guess, double *guess_pose,
                                       mvs_refine_result *ba_frames, double *points_refined)
{
    if (!q || !q->track_ran || frame < 0 || frame >= q->n_frames)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const VoDev &d = q->vo;
    const size_t N = (size_t)d.max_kp, of = (size_t)frame * N;
    hipStream_t s = ctx_stream(ctx);
    const struct {
        void *dst;
        const void *src;
        size_t bytes;
    } parts[] = {{cand_base_kp, d.cand_a + of, N * sizeof(int32_t)},
                 {cand_new_kp, d.cand_b + of, N * sizeof(int32_t)},
                 {cand_xyz, d.cand_X + 3 * of, N * 3 * sizeof(double)},
                 {cand_uv, d.cand_uv + 2 * of, N * 2 * sizeof(double)},
                 {pnp_inlier_idx, d.inliers + of, N * sizeof(int32_t)},
                 {point_id, d.pt_id + of, N * sizeof(int32_t)},
                 {point_kp, d.pt_kp + 2 * of, N * 2 * sizeof(int32_t)},
                 {point_is_new, d.pt_new + of, N},
                 {point_guess, d.guess + 3 * of, N * 3 * sizeof(double)},
                 {guess_pose, d.pose0 + 24 * (size_t)frame, 24 * sizeof(double)},
                 {ba_frames, d.ba_out + 2 * (size_t)frame, 2 * sizeof(mvs_refine_result)},
                 {points_refined, d.pts + 3 * of, N * 3 * sizeof(double)}};
    for (const auto &pt : parts)
        if (pt.dst)
            HIP_TRY(ctx, hipMemcpyAsync(pt.dst, pt.src, pt.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_batch_upload_octaves(mvs_batch *b, int first, int count, const uint8_t *base_octave,
                                    const uint8_t *pair_octave)
{
    if (!b || first < 0 || count < 1 || first + count > b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t N = b->d.max_kp, off = (size_t)first * N, bytes = (size_t)count * N;
    for (const uint8_t *o : {base_octave, pair_octave})
        if (o)
            for (size_t i = 0; i < bytes; ++i)
                if (o[i] > 30)
                    return MVS_ERR_INVALID_ARG;   // stddev = (1 << octave) * 0.5 (visual-feature.cpp:203)
    if (base_octave)
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint8_t *>(b->d.oct1) + off, base_octave, bytes, hipMemcpyHostToDevice,
                                    ctx_stream(ctx)));
    if (pair_octave)
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint8_t *>(b->d.oct2) + off, pair_octave, bytes, hipMemcpyHostToDevice,
                                    ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_upload_octaves(mvs_seq *q, int first, int count, const uint8_t *octave)
{
    if (!q || !octave || first < 0 || count < 1 || first + count > q->n_frames)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t N = q->batch->d.max_kp, bytes = (size_t)count * N;
    for (size_t i = 0; i < bytes; ++i)
        if (octave[i] > 30)
            return MVS_ERR_INVALID_ARG;
    q->loop_verified = false;   // the verification's refinement weighed the observations by the octaves before
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint8_t *>(q->batch->d.oct1) + (size_t)first * N, octave, bytes,
                                hipMemcpyHostToDevice, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_download_refined(mvs_seq *q, mvs_refine_result *refined, double *points_xyz, double *point_cov)
{
    return q ? mvs_batch_download_refined(q->batch, refined, points_xyz, point_cov) : MVS_ERR_INVALID_ARG;
}

mvs_status mvs_seq_upload_images(mvs_seq *q, int first, int count, const uint8_t *images, int width, int height,
                                 const mvs_orb_params *params, const double K[9])
{
    if (!q || !images || !params || first < 0 || count < 1 || first + count > q->n_frames)
        return MVS_ERR_INVALID_ARG;
    const BatchDev &bd = q->batch->d;
    if (bd.desc_words != 8)
        return MVS_ERR_INVALID_ARG;   // the extractor writes 256-bit descriptors
    mvs_orb_params prm = *params;
    prm.nfeatures = bd.max_kp;
    const size_t N = bd.max_kp, off = first;
    q->loop_scored = q->loop_selected = q->loop_verified = false;   // as mvs_seq_upload
    OrbDev d;
    mvs_status st = orb_run(q->ctx, images, count, width, height, prm,
                            reinterpret_cast<uint8_t *>(const_cast<uint32_t *>(bd.desc1)) + off * N * 32,
                            const_cast<float *>(bd.kp1) + off * N * 2, const_cast<int32_t *>(bd.n1) + off, d,
                            const_cast<uint8_t *>(bd.oct1) + off * N);
    if (st != MVS_OK)
        return st;
    return K ? mvs_seq_upload(q, first, count, nullptr, nullptr, nullptr, K) : MVS_OK;
}
}  // extern "C"
