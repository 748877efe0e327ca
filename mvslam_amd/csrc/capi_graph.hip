// capi_graph.hip -- host side of libmvslam_hip.so: the back end.  Pose graphs (posegraph.hip; the direct
// LM step of pg_direct.hip, section 4.10.4; the Sim(3) graphs of sim3graph.hip, section 4.10.6), the
// graph of a resident sequence (seq_graph.hip), marginal covariances (pg_marginals.hip) and loop closures (loop.hip).  What it
// decides about a graph without the device is in pg_host.hpp and pg_envelope.hpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "pg_envelope.hpp"
#include "pg_host.hpp"

using namespace mvs_host;
using namespace mvs_pg;

extern "C" {

void mvs_pose_graph_params_default(mvs_pose_graph_params *p)
{
    if (!p)
        return;
    mvs_refine_params_default(&p->lm);
    p->anchor_sigma[0] = p->anchor_sigma[1] = 1e-4;   // graph.cpp GRAPH_ANCHOR_STDDEV
    p->cg_rel_tol = 1e-10;
    p->cg_max_iterations = 0;                         // 6 n_nodes
    p->cg_chunk_iterations = 0;                       // the whole budget at once
}

mvs_status mvs_ctx_set_pose_graph_solver(mvs_ctx *ctx, int solver)
{
    if (!ctx || (solver != MVS_PG_SOLVER_PCG && solver != MVS_PG_SOLVER_DIRECT))
        return MVS_ERR_INVALID_ARG;
    ctx->pg_solver = solver;
    return MVS_OK;
}

mvs_status mvs_ctx_set_pose_graph_loss(mvs_ctx *ctx, int loss, double k, int32_t first_edge)
{
    if (!ctx || !loss_args_ok(loss, k, first_edge))
        return MVS_ERR_INVALID_ARG;
    ctx->pg_loss = loss;
    ctx->pg_loss_k = k;
    ctx->pg_loss_first = first_edge;
    return MVS_OK;
}

mvs_status mvs_ctx_set_ba_loss(mvs_ctx *ctx, int loss, double k)
{
    if (!ctx || !ba_loss_args_ok(loss, k))
        return MVS_ERR_INVALID_ARG;
    ctx->ba_loss = loss;
    ctx->ba_loss_k = k;
    return MVS_OK;
}

mvs_status mvs_ctx_pose_graph_direct_info(mvs_ctx *ctx, mvs_pose_graph_direct_info *info)
{
    if (!ctx || !info || !ctx->pgd_ran)
        return MVS_ERR_INVALID_ARG;
    *info = ctx->pgd_info;
    return MVS_OK;
}

// weights of the anchor's prior (rotation, translation) from its standard deviations
static void anchor_weights(const double sigma[2], double w[2])
{
    w[0] = 1.0 / (sigma[0] * sigma[0]);
    w[1] = 1.0 / (sigma[1] * sigma[1]);
}

// the robust loss of one call's edges: the context's setting with first_edge resolved
struct PgLoss {
    int loss = MVS_PG_LOSS_NONE;
    double k = 0.0;
    int32_t first = 0;
};
// the context's setting for a host graph, where first_edge stands for itself (the callers have refused
// MVS_PG_LOSS_LOOP_EDGES)
static PgLoss ctx_loss(const mvs_ctx *ctx)
{
    PgLoss l;
    if (ctx->pg_loss != MVS_PG_LOSS_NONE)
        l.loss = ctx->pg_loss, l.k = ctx->pg_loss_k, l.first = ctx->pg_loss_first;
    return l;
}

static PgCfg to_pg_cfg(const mvs_pose_graph_params &p, const PgLoss &loss)
{
    PgCfg c{};
    c.loss = loss.loss, c.loss_first = loss.first, c.loss_k = loss.k;
    c.max_iterations = p.lm.max_iterations;
    c.lambda_initial = p.lm.lambda_initial;
    c.lambda_factor = p.lm.lambda_factor;
    c.lambda_upper = p.lm.lambda_upper;
    c.rel_tol = p.lm.rel_tol;
    c.abs_tol = p.lm.abs_tol;
    anchor_weights(p.anchor_sigma, c.w_anchor);
    c.cg_rel_tol = p.cg_rel_tol;
    c.cg_max_iterations = p.cg_max_iterations;
    return c;
}

// arguments of one graph: MVS_ERR_INVALID_ARG / MVS_ERR_CAPACITY before anything runs
static mvs_status pose_graph_check(const mvs_pose_graph &g)
{
    if (g.n_nodes < 1 || g.n_edges < 0 || !g.node_pose)
        return MVS_ERR_INVALID_ARG;
    if (g.n_edges > 0 && (!g.edge_src || !g.edge_dst || !g.edge_pose || !g.edge_cov))
        return MVS_ERR_INVALID_ARG;
    if (g.n_nodes > kPgMaxNodes || g.n_edges > kPgMaxEdges)
        return MVS_ERR_CAPACITY;
    if (g.anchor_node < 0 || g.anchor_node >= g.n_nodes)
        return MVS_ERR_INVALID_ARG;
    if (!edges_in_range(g.n_nodes, g.n_edges, g.edge_src, g.edge_dst))
        return MVS_ERR_INVALID_ARG;
    if (!all_finite(g.node_pose, 12 * (size_t)g.n_nodes) || !all_finite(g.edge_pose, 12 * (size_t)g.n_edges) ||
        !all_finite(g.edge_cov, 36 * (size_t)g.n_edges))
        return MVS_ERR_INVALID_ARG;
    return MVS_OK;
}

// ---- the solver's entries over device-resident graphs ------------------------------------------------------------------
// The host-pointer calls upload and come here; mvs_seq_optimize_pose_graph comes here with the graph of its sequence.  Only
// edge_src / edge_dst are also needed on the host (connectivity, the CSR list).

// scratch of the large path for N nodes and E edges, as offsets from one base in ctx->pg
struct PgLargeLayout {
    size_t o_state, o_off, o_inc, o_pa, o_pb, o_W, o_lin, o_u, o_ec, o_D, o_Mf, o_vec[6], o_pq, o_Ha, total;
    PgLargeLayout(size_t N, size_t E)
    {
        Carve L{64};
        o_state = L.take(sizeof(PgState));
        o_off = L.take((N + 1) * 4), o_inc = L.take(2 * E * 4);
        o_pa = L.take(N * 12 * 8), o_pb = L.take(N * 12 * 8);
        o_W = L.take(E * 21 * 8), o_lin = L.take(E * kPgLin * 8), o_u = L.take(E * 6 * 8), o_ec = L.take(E * 8);
        o_D = L.take(N * 21 * 8), o_Mf = L.take(N * 21 * 8);
        for (size_t &o : o_vec)
            o = L.take(N * 6 * 8);
        o_pq = L.take(N * 8), o_Ha = L.take(36 * 8);
        total = L.total();
    }
};

// what the direct solver (pg_direct.hip) has the host decide before anything is launched: the
// envelope, the per-block term lists and the blocks' rows and slots
struct PgdPlan {
    std::vector<int32_t> first, row_off;
    mvs_pgm::BlockLists lists;
    mvs_pgm::DirectPlan blk;
    int64_t blocks = 0;
};
static mvs_status pgd_plan(int N, int E, int anchor, const int32_t *src, const int32_t *dst, PgdPlan &P)
{
    P.blocks = mvs_pgm::envelope(N, E, src, dst, P.first, P.row_off);
    if (P.blocks > mvs_pgm::kMaxEnvelopeBlocks)
        return MVS_ERR_CAPACITY;
    P.lists = mvs_pgm::block_lists(E, anchor, src, dst, P.first, P.row_off);
    P.blk = mvs_pgm::direct_plan(N, P.first, P.row_off, P.lists);
    return MVS_OK;
}
// the direct solver's scratch behind the large path's, as offsets from the end of PgLargeLayout
struct PgdLayout {
    size_t o_state, o_first, o_row, o_brow, o_bslot, o_soff, o_codes, o_sky, total;
    PgdLayout(size_t N, const PgdPlan &P)
    {
        Carve L{64};
        o_state = L.take(sizeof(PgdState));
        o_first = L.take(N * 4), o_row = L.take((N + 1) * 4);
        o_brow = L.take((size_t)P.blocks * 4), o_bslot = L.take((size_t)P.blocks * 4);
        o_soff = L.take(P.lists.slot_off.size() * 4), o_codes = L.take(P.lists.codes.size() * 4);
        o_sky = L.take((size_t)P.blocks * 36 * 8);
        total = L.total();
    }
};
// scratch of one large-path graph: PCG's, and with a plan the direct solver's behind it
static size_t pg_large_scratch(size_t N, size_t E, const PgdPlan *plan)
{
    return PgLargeLayout(N, E).total + (plan ? PgdLayout(N, *plan).total : 0);
}

// one graph of 17 .. 4096 nodes: LM on the host, one synchronisation per iteration (and, with cg_chunk_iterations > 0, one
// per chunk of CG iterations that did not converge).  `plan`: null for the PCG, the direct solver's plan otherwise (then the
// scratch is pg_large_scratch's).  h_src / h_dst: the edges on the host; every d_* pointer is device
// memory that stays valid through the call; `base` is scratch of PgLargeLayout(N, E).total bytes.  The optimised nodes go
// to poses_out with a copy of kind `out_kind` (device to host, or device to device), only when the result is ok.
static mvs_status pose_graph_large_dev(mvs_ctx *ctx, char *base, int n_nodes, int n_edges, int anchor, const int32_t *h_src,
                                       const int32_t *h_dst, const int32_t *d_src, const int32_t *d_dst, const double *d_node,
                                       const double *d_z, const double *d_cov, const mvs_pose_graph_params &params,
                                       const PgLoss &loss, mvs_pose_graph_result *res, double *poses_out,
                                       hipMemcpyKind out_kind, const PgdPlan *plan = nullptr)
{
    const size_t N = (size_t)n_nodes, E = (size_t)n_edges;
    std::vector<int32_t> off, inc;
    incidence_csr(n_nodes, n_edges, h_src, h_dst, off, inc);
    const PgLargeLayout L(N, E);
    hipStream_t s = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemsetAsync(base + L.o_state, 0, sizeof(PgState), s));
    HIP_TRY(ctx, hipMemcpyAsync(base + L.o_off, off.data(), (N + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(base + L.o_inc, inc.data(), 2 * E * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(base + L.o_pa, d_node, N * 12 * 8, hipMemcpyDeviceToDevice, s));
    auto dp = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<const int32_t *>(base + o); };
    PgLargeDev d{};
    d.n_nodes = n_nodes, d.n_edges = n_edges, d.anchor = anchor;
    d.cfg = to_pg_cfg(params, loss);
    d.edge_src = d_src, d.edge_dst = d_dst, d.csr_off = ip(L.o_off), d.csr_inc = ip(L.o_inc);
    d.edge_pose = d_z, d.edge_cov = d_cov, d.pose0 = d_node;
    d.pose[0] = dp(L.o_pa), d.pose[1] = dp(L.o_pb);
    d.W = dp(L.o_W), d.lin = dp(L.o_lin), d.u = dp(L.o_u), d.ecost = dp(L.o_ec), d.D = dp(L.o_D), d.Mf = dp(L.o_Mf);
    d.g = dp(L.o_vec[0]), d.x = dp(L.o_vec[1]), d.r = dp(L.o_vec[2]), d.z = dp(L.o_vec[3]), d.p = dp(L.o_vec[4]), d.q = dp(L.o_vec[5]);
    d.pq = dp(L.o_pq), d.Ha = dp(L.o_Ha);
    d.state = reinterpret_cast<PgState *>(base + L.o_state);
    // the direct solver reads D and g of the gather, keeps C_i^-1 where the PCG keeps its block factors, the right-hand side in
    // r, and leaves the step in x
    PgdDev pd{};
    PgdState hd{};
    if (plan) {
        const PgdLayout Ld(N, *plan);
        char *db = base + L.total;
        auto up = [&](size_t o, const std::vector<int32_t> &v) {
            return v.empty() ? hipSuccess : hipMemcpyAsync(db + o, v.data(), v.size() * 4, hipMemcpyHostToDevice, s);
        };
        HIP_TRY(ctx, up(Ld.o_first, plan->first));
        HIP_TRY(ctx, up(Ld.o_row, plan->row_off));
        HIP_TRY(ctx, up(Ld.o_brow, plan->blk.blk_row));
        HIP_TRY(ctx, up(Ld.o_bslot, plan->blk.blk_slot));
        HIP_TRY(ctx, up(Ld.o_soff, plan->lists.slot_off));
        HIP_TRY(ctx, up(Ld.o_codes, plan->lists.codes));
        auto dip = [&](size_t o) { return reinterpret_cast<const int32_t *>(db + o); };
        pd.n_nodes = n_nodes, pd.n_blocks = (int)plan->blocks;
        pd.first = dip(Ld.o_first), pd.row_off = dip(Ld.o_row), pd.blk_row = dip(Ld.o_brow), pd.blk_slot = dip(Ld.o_bslot);
        pd.slot_off = dip(Ld.o_soff), pd.codes = dip(Ld.o_codes);
        pd.lin = d.lin, pd.D = d.D, pd.g = d.g, pd.Cinv = d.Mf, pd.y = d.r, pd.x = d.x;
        pd.sky = reinterpret_cast<double *>(db + Ld.o_sky);
        pd.state = reinterpret_cast<PgdState *>(db + Ld.o_state);
        ctx->pgd_ran = true;
        ctx->pgd_info = mvs_pose_graph_direct_info{(int32_t)plan->blocks, plan->blk.widest, 0, -1, 0.0, 0.0};
    }
    const int cg_max = params.cg_max_iterations > 0 ? params.cg_max_iterations : 6 * n_nodes;
    const int chunk = params.cg_chunk_iterations;
    PgState h{};
    mvs_status st;
    // the status word behind what has been launched so far: the one place this function waits for the device
    auto read_state = [&]() -> mvs_status {
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&h, d.state, sizeof(h), hipMemcpyDeviceToHost, s));
        if (plan)
            HIP_TRY(ctx, hipMemcpyAsync(&hd, pd.state, sizeof(hd), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, sync_stream(ctx));
        return MVS_OK;
    };
    launch_pg_prep(d, s);
    // a covariance that is not positive definite ends the call here, before anything is linearised on its whitening factor
    if ((st = read_state()) != MVS_OK)   // `off`, `inc` and the plan's lists have been read by here, too
        return st;
    if (h.bad_cov) {
        *res = mvs_pose_graph_result{};
        return MVS_OK;
    }

    // the LM rule of refine_kernel, on the host: the device computes, the host decides
    const PgCfg &cfg = d.cfg;
    int cb = 0, it = 0, rejected = 0, cg_total = 0;
    double cur = 0.0, cost0 = 0.0, lam = cfg.lambda_initial;
    bool ok0 = true, have0 = false;
    // one iteration on the device and its status; the first one also gives the cost at the initial values
    auto iterate = [&](bool with_cg) -> mvs_status {
        if (plan) {
            // a constant number of launches whatever the graph: linearise, gather, the four of the solve, update and cost
            // (max_iterations = 0: the cost at the initial values alone)
            launch_pg_linearise(d, cb, !have0, s);
            if (with_cg) {
                HIP_TRY(ctx, hipMemsetAsync(pd.state, 0, sizeof(PgdState), s));
                launch_pgd_step(pd, lam, s);
                launch_pg_end(d, cb, s);
            }
            if ((st = read_state()) != MVS_OK)
                return st;
            if (!have0) {
                have0 = true;
                cost0 = cur = h.cost0;
                ok0 = std::isfinite(cur);
            }
            return MVS_OK;
        }
        launch_pg_begin(d, cb, lam, !have0, s);
        if (with_cg && chunk <= 0) {
            launch_pg_cg(d, lam, cg_max, s);
        } else if (with_cg) {
            // chunk by chunk: the iterations not enqueued are the ones the status word would have sent away at once
            for (int left = cg_max; left > 0;) {
                const int n = std::min(chunk, left);
                launch_pg_cg(d, lam, n, s);
                left -= n;
                if (left > 0) {
                    if ((st = read_state()) != MVS_OK)
                        return st;
                    if (h.done)
                        break;
                }
            }
        }
        launch_pg_end(d, cb, s);
        if ((st = read_state()) != MVS_OK)
            return st;
        if (!have0) {
            have0 = true;
            cost0 = cur = h.cost0;
            ok0 = std::isfinite(cur);
        }
        return MVS_OK;
    };
    while (ok0 && it < cfg.max_iterations) {
        if ((st = iterate(true)) != MVS_OK)
            return st;
        if (!ok0)
            break;
        cg_total += h.cg_iters;
        if (plan) {
            mvs_pose_graph_direct_info &info = ctx->pgd_info;
            if (hd.status != 0 && info.failed_solves++ == 0) {
                info.bad_node = n_nodes - hd.bad_code;
                info.failed_pivot = hd.status == 3 ? hd.min_d : 0.0;
            }
            if (hd.status == 0) {   // a factorisation that completed
                const double piv = std::sqrt(hd.min_d);
                info.min_pivot = info.min_pivot > 0.0 ? std::min(info.min_pivot, piv) : piv;
            }
        }
        // the linear solve counts as done when the CG converged, or ran out of iterations with a smaller residual; the direct
        // solve when no pivot failed
        const bool solved = plan ? hd.status == 0 : (h.done == 1 || (h.done == 0 && h.rr < h.gnorm2));
        const double cand = h.cand;
        const bool accepted = solved && cand <= cur;
        ++it;
        if (accepted) {
            cb ^= 1;
            const double dec = 0.5 * (cur - cand);
            const bool done = dec <= cfg.abs_tol || dec <= cfg.rel_tol * (0.5 * cur);
            cur = cand;
            lam = lam / cfg.lambda_factor;
            if (done)
                break;
        } else {
            ++rejected;
            const double inc_e = 0.5 * (cand - cur);
            if (solved && (inc_e <= cfg.abs_tol || inc_e <= cfg.rel_tol * (0.5 * cur)))
                break;
            lam = lam * cfg.lambda_factor;
            if (lam > cfg.lambda_upper)
                break;
        }
    }
    // max_iterations = 0: the cost at the initial values alone (an iteration with no CG steps leaves x = 0)
    if (!have0 && (st = iterate(false)) != MVS_OK)
        return st;
    res->ok = ok0 ? 1 : 0;
    res->iterations = it;
    res->cg_iterations = cg_total;
    res->rejected_steps = rejected;
    res->error_initial = ok0 ? 0.5 * cost0 : 0.0;
    res->error = ok0 ? 0.5 * cur : 0.0;
    if (ok0) {
        HIP_TRY(ctx, hipMemcpyAsync(poses_out, d.pose[cb], N * 12 * 8, out_kind, s));
        HIP_TRY(ctx, sync_stream(ctx));
    }
    return MVS_OK;
}

// one host-pointer graph on the device, in front of `scratch_bytes` of its solver's scratch in the workspace `ws`
struct PgUploaded {
    const int32_t *src, *dst;
    const double *z, *cov, *node, *x;   // x: the second pose array, with one
    char *scratch;
};
static mvs_status pose_graph_upload(mvs_ctx *ctx, DevWorkspace &ws, const mvs_pose_graph &g, const double *x, size_t scratch_bytes,
                                    PgUploaded &u)
{
    const size_t N = (size_t)g.n_nodes, E = (size_t)g.n_edges;
    const struct {
        const void *host;
        size_t bytes;
    } parts[] = {{g.edge_src, E * 4}, {g.edge_dst, E * 4}, {g.edge_pose, E * 96}, {g.edge_cov, E * 288}, {g.node_pose, N * 96},
                 {x, x ? N * 96 : 0}};
    Carve U{64};
    size_t o[6];
    for (int i = 0; i < 6; ++i)
        o[i] = U.take(parts[i].bytes);
    const mvs_status st = ws_grow(ctx, ws, U.total() + scratch_bytes);
    if (st != MVS_OK)
        return st;
    char *base = ws.ptr();
    for (int i = 0; i < 6; ++i)
        if (parts[i].bytes)
            HIP_TRY(ctx, hipMemcpyAsync(base + o[i], parts[i].host, parts[i].bytes, hipMemcpyHostToDevice, ctx_stream(ctx)));
    auto dp = [&](int i) { return reinterpret_cast<const double *>(base + o[i]); };
    auto ip = [&](int i) { return reinterpret_cast<const int32_t *>(base + o[i]); };
    u = PgUploaded{ip(0), ip(1), dp(2), dp(3), dp(4), dp(5), base + U.total()};
    return MVS_OK;
}

// the host-pointer entry of the large path: upload, then the entry above
static mvs_status pose_graph_large(mvs_ctx *ctx, const mvs_pose_graph &g, const mvs_pose_graph_params &params,
                                   mvs_pose_graph_result *res, double *poses_out, const PgdPlan *plan)
{
    PgUploaded u;
    const mvs_status st = pose_graph_upload(ctx, ctx->pg, g, nullptr, pg_large_scratch((size_t)g.n_nodes, (size_t)g.n_edges, plan), u);
    if (st != MVS_OK)
        return st;
    return pose_graph_large_dev(ctx, u.scratch, g.n_nodes, g.n_edges, g.anchor_node, g.edge_src, g.edge_dst, u.src, u.dst, u.node,
                                u.z, u.cov, params, ctx_loss(ctx), res, poses_out, hipMemcpyDeviceToHost, plan);
}

// scratch of a dense-path batch of G graphs with sumN nodes and sumE edges.  Outputs first and contiguous (results,
// poses): a download is their prefix.
struct PgDenseLayout {
    size_t o_out, o_po, down, o_W, o_lin, total;
    PgDenseLayout(size_t G, size_t sumN, size_t sumE)
    {
        Carve L{64};
        o_out = L.take(G * sizeof(mvs_pose_graph_result)), o_po = L.take(sumN * 12 * 8);
        down = L.total();
        o_W = L.take(sumE * 21 * 8), o_lin = L.take(sumE * kPgLin * 8);
        total = L.total();
    }
};

// graphs of up to 16 nodes over device-resident inputs: one launch.  `base`: scratch of PgDenseLayout::total bytes.
static mvs_status pose_graph_dense_dev(mvs_ctx *ctx, char *base, const PgDenseLayout &L, int n_graphs,
                                       const mvs_pose_graph_params &params, const PgLoss &loss, const PgProblem *d_prob,
                                       const double *d_node, const int32_t *d_src, const int32_t *d_dst, const double *d_z,
                                       const double *d_cov)
{
    PgDenseDev d{};
    d.n_problems = n_graphs;
    d.cfg = to_pg_cfg(params, loss);
    d.prob = d_prob;
    d.node_pose = d_node;
    d.edge_pose = d_z;
    d.edge_cov = d_cov;
    d.edge_src = d_src;
    d.edge_dst = d_dst;
    d.W = reinterpret_cast<double *>(base + L.o_W);
    d.lin = reinterpret_cast<double *>(base + L.o_lin);
    d.poses_out = reinterpret_cast<double *>(base + L.o_po);
    d.out = reinterpret_cast<mvs_pose_graph_result *>(base + L.o_out);
    launch_pg_dense(d, ctx_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    return MVS_OK;
}

static bool pose_graph_params_ok(const mvs_pose_graph_params *params)
{
    return params && params->lm.max_iterations >= 0 && params->lm.lambda_initial >= 0.0 && params->lm.lambda_factor > 1.0 &&
           params->lm.lambda_upper > 0.0 && params->anchor_sigma[0] > 0.0 && params->anchor_sigma[1] > 0.0 &&
           params->cg_rel_tol >= 0.0 && params->cg_max_iterations >= 0;
}

mvs_status mvs_pose_graph_optimize_batch(mvs_ctx *ctx, const mvs_pose_graph *graphs, int n_graphs,
                                         const mvs_pose_graph_params *params, mvs_pose_graph_result *results,
                                         double *poses_out)
{
    if (!ctx || !graphs || n_graphs < 1 || !params || !results || !poses_out)
        return MVS_ERR_INVALID_ARG;
    if (!pose_graph_params_ok(params) || !loss_fits_host_graph(ctx->pg_loss, ctx->pg_loss_first))
        return MVS_ERR_INVALID_ARG;
    int Nmax = 0;
    for (int i = 0; i < n_graphs; ++i) {
        const mvs_status st = pose_graph_check(graphs[i]);
        if (st != MVS_OK)
            return st;
        Nmax = std::max(Nmax, graphs[i].n_nodes);
    }
    // the direct solver's plans, and its one refusal, before anything is launched
    std::vector<PgdPlan> plans(ctx->pg_solver == MVS_PG_SOLVER_DIRECT ? (size_t)n_graphs : 0);
    for (size_t i = 0; i < plans.size(); ++i) {
        const mvs_pose_graph &g = graphs[i];
        if (g.n_nodes <= kPgDenseMaxNodes)
            continue;
        const mvs_status st = pgd_plan(g.n_nodes, g.n_edges, g.anchor_node, g.edge_src, g.edge_dst, plans[i]);
        if (st != MVS_OK)
            return st;
    }
    std::memset(results, 0, (size_t)n_graphs * sizeof(mvs_pose_graph_result));
    std::vector<char> joined((size_t)n_graphs);
    for (int i = 0; i < n_graphs; ++i) {
        const mvs_pose_graph &g = graphs[i];
        joined[(size_t)i] = pose_graph_connected(g.n_nodes, g.n_edges, g.edge_src, g.edge_dst, g.anchor_node) ? 1 : 0;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the batch's graphs of up to 16 nodes: one upload, one launch, one download
    std::vector<PgProblem> desc;
    std::vector<int> which;
    size_t sumN = 0, sumE = 0;
    for (int i = 0; i < n_graphs; ++i) {
        const mvs_pose_graph &g = graphs[i];
        if (!joined[(size_t)i] || g.n_nodes > kPgDenseMaxNodes)
            continue;
        PgProblem p{};
        p.n_nodes = g.n_nodes, p.n_edges = g.n_edges, p.anchor = g.anchor_node;
        p.node_off = (int64_t)sumN, p.edge_off = (int64_t)sumE;
        sumN += (size_t)g.n_nodes;
        sumE += (size_t)g.n_edges;
        desc.push_back(p);
        which.push_back(i);
    }
    if (!desc.empty()) {
        const size_t G = desc.size();
        const PgDenseLayout L(G, sumN, sumE);
        const size_t o_up = L.total;   // the uploaded block: descriptors, node poses, edge poses, covariances, src, dst
        Carve U{64};
        const size_t u_desc = U.take(G * sizeof(PgProblem)), u_np = U.take(sumN * 12 * 8), u_z = U.take(sumE * 12 * 8);
        const size_t u_cov = U.take(sumE * 36 * 8), u_src = U.take(sumE * 4), u_dst = U.take(sumE * 4);
        mvs_status st = ws_grow(ctx, ctx->pg, o_up + U.total());
        if (st != MVS_OK)
            return st;
        std::vector<char> up(U.total());
        std::memcpy(up.data() + u_desc, desc.data(), G * sizeof(PgProblem));
        for (size_t k = 0; k < G; ++k) {
            const mvs_pose_graph &g = graphs[which[k]];
            const size_t n = (size_t)g.n_nodes, e = (size_t)g.n_edges, no = (size_t)desc[k].node_off, eo = (size_t)desc[k].edge_off;
            std::memcpy(up.data() + u_np + no * 96, g.node_pose, n * 96);
            if (e) {
                std::memcpy(up.data() + u_z + eo * 96, g.edge_pose, e * 96);
                std::memcpy(up.data() + u_cov + eo * 288, g.edge_cov, e * 288);
                std::memcpy(up.data() + u_src + eo * 4, g.edge_src, e * 4);
                std::memcpy(up.data() + u_dst + eo * 4, g.edge_dst, e * 4);
            }
        }
        char *base = ctx->pg.ptr();
        hipStream_t s = ctx_stream(ctx);
        HIP_TRY(ctx, hipMemcpyAsync(base + o_up, up.data(), up.size(), hipMemcpyHostToDevice, s));
        auto dp = [&](size_t o) { return reinterpret_cast<const double *>(base + o_up + o); };
        auto ip = [&](size_t o) { return reinterpret_cast<const int32_t *>(base + o_up + o); };
        st = pose_graph_dense_dev(ctx, base, L, (int)G, *params, ctx_loss(ctx),
                                  reinterpret_cast<const PgProblem *>(base + o_up + u_desc), dp(u_np), ip(u_src), ip(u_dst), dp(u_z),
                                  dp(u_cov));
        if (st != MVS_OK)
            return st;
        std::vector<char> host(L.down);
        HIP_TRY(ctx, hipMemcpyAsync(host.data(), base, L.down, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, sync_stream(ctx));
        for (size_t k = 0; k < G; ++k) {
            const int i = which[k];
            std::memcpy(&results[i], host.data() + L.o_out + k * sizeof(mvs_pose_graph_result), sizeof(mvs_pose_graph_result));
            if (results[i].ok)
                std::memcpy(poses_out + (size_t)i * Nmax * 12, host.data() + L.o_po + (size_t)desc[k].node_off * 96,
                            (size_t)graphs[i].n_nodes * 96);
        }
    }
    // larger graphs, one after another
    for (int i = 0; i < n_graphs; ++i) {
        if (!joined[(size_t)i] || graphs[i].n_nodes <= kPgDenseMaxNodes)
            continue;
        const mvs_status st = pose_graph_large(ctx, graphs[i], *params, &results[i], poses_out + (size_t)i * Nmax * 12,
                                               plans.empty() ? nullptr : &plans[(size_t)i]);
        if (st != MVS_OK)
            return st;
    }
    bool all_ok = true;
    for (int i = 0; i < n_graphs; ++i)
        all_ok = all_ok && results[i].ok;
    return all_ok ? MVS_OK : MVS_NO_MODEL;
}

mvs_status mvs_pose_graph_optimize(mvs_ctx *ctx, const mvs_pose_graph *graph, const mvs_pose_graph_params *params,
                                   mvs_pose_graph_result *result, double *poses_out)
{
    return mvs_pose_graph_optimize_batch(ctx, graph, 1, params, result, poses_out);
}

// ---- the pose graph of a resident sequence (seq_graph.hip) -------------------------------------
// The graph's block: S candidate slots, room for `cap` >= S edges (the loop edges of mvs_seq_add_loop_edges sit behind the
// built ones), F nodes.  The count, src and dst first and in this order: seq_graph_head downloads that prefix.
struct SeqGraphLayout {
    // the block's arrays in their order, and what each has a row for: the block (one row), an edge, a node or a slot.  The
    // one list of them: point(), the download and the regrow of mvs_seq_add_loop_edges go by it.
    enum Part { kCount, kSrc, kDst, kLag, kKind, kScale, kPose, kCov, kNode, kOpt, kSlotKeep, kSlotKind, kSlotScale, kSlotPose, kSlotCov,
                kBuilt, kParts };   // kBuilt: edges of the built graph, behind which the loop edges go (mvs_seq_add_loop_edges)
    enum Per { kBlock, kEdge, kNodeRow, kSlot };
    struct Spec {
        size_t elem;
        Per per;
    };
    static constexpr Spec kSpec[kParts] ={{4, kBlock}, {4, kEdge}, {4, kEdge}, {4, kEdge}, {4, kEdge}, {8, kEdge}, {96, kEdge}, {288, kEdge},
                       {96, kNodeRow}, {96, kNodeRow}, {4, kSlot}, {4, kSlot}, {8, kSlot}, {96, kSlot}, {288, kSlot}, {4, kBlock}};
    size_t S, cap, F, off[kParts], total;
    SeqGraphLayout(size_t S_, size_t cap_, size_t F_) : S(S_), cap(cap_), F(F_)
    {
        Carve L{64};
        for (int p = 0; p < kParts; ++p)
            off[p] = L.take(bytes(p, cap));
        total = L.total();
    }
    // bytes of array p when the graph has `edges` edges
    size_t bytes(int p, size_t edges) const
    {
        const size_t rows[] = {1, edges, F, S};
        return kSpec[p].elem * rows[kSpec[p].per];
    }
    // points g's arrays into the block at `base`
    void point(SeqGraphDev &g, char *base) const
    {
        auto dp = [&](Part p) { return reinterpret_cast<double *>(base + off[p]); };
        auto ip = [&](Part p) { return reinterpret_cast<int32_t *>(base + off[p]); };
        g.slot_keep = ip(kSlotKeep), g.slot_kind = ip(kSlotKind), g.slot_scale = dp(kSlotScale), g.slot_pose = dp(kSlotPose);
        g.slot_cov = dp(kSlotCov), g.n_edges = ip(kCount), g.edge_src = ip(kSrc), g.edge_dst = ip(kDst), g.edge_lag = ip(kLag);
        g.edge_kind = ip(kKind), g.edge_scale = dp(kScale), g.edge_pose = dp(kPose), g.edge_cov = dp(kCov), g.node_pose = dp(kNode);
    }
};

// the layout of q's resident graph block, and q's own pointers into it
static SeqGraphLayout seq_graph_layout(const mvs_seq *q)
{
    return SeqGraphLayout((size_t)q->gd.n_slots, (size_t)q->graph_edge_cap, (size_t)q->n_frames);
}
static void seq_graph_adopt(mvs_seq *q, const SeqGraphLayout &L)
{
    q->graph_opt_pose = reinterpret_cast<double *>(q->graph.ptr() + L.off[SeqGraphLayout::kOpt]);
    q->graph_n_built = reinterpret_cast<int32_t *>(q->graph.ptr() + L.off[SeqGraphLayout::kBuilt]);
    q->graph_edge_cap = (int)L.cap;
}

// The count and the endpoints of the resident graph's edges, checked: all the host needs of the graph.  A count outside the
// block or an endpoint outside [0, n_frames) is not a graph the library built: MVS_ERR_HIP, under the caller's name.
struct SeqGraphHead {
    std::vector<char> buf;
    int32_t n_edges = 0;
    const int32_t *src = nullptr, *dst = nullptr;
};
static mvs_status seq_graph_head(mvs_seq *q, const char *caller, SeqGraphHead &h)
{
    mvs_ctx *ctx = q->ctx;
    const SeqGraphLayout L = seq_graph_layout(q);
    h.buf.resize(L.off[L.kDst] + L.bytes(L.kDst, L.cap));
    HIP_TRY(ctx, hipMemcpyAsync(h.buf.data(), q->graph.ptr(), h.buf.size(), hipMemcpyDeviceToHost, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    std::memcpy(&h.n_edges, h.buf.data() + L.off[L.kCount], 4);
    h.src = reinterpret_cast<const int32_t *>(h.buf.data() + L.off[L.kSrc]);
    h.dst = reinterpret_cast<const int32_t *>(h.buf.data() + L.off[L.kDst]);
    if (h.n_edges < 0 || h.n_edges > q->graph_edge_cap || !edges_in_range(q->n_frames, h.n_edges, h.src, h.dst)) {
        ctx->err = std::string(caller) + ": the resident graph's edges are out of range";
        return MVS_ERR_HIP;
    }
    return MVS_OK;
}

// The context's loss for q's resident graph of E edges: MVS_PG_LOSS_LOOP_EDGES becomes the number of edges the graph had
// before mvs_seq_add_loop_edges, the word the block keeps for that call (none added: E, so that no edge has the loss).
static mvs_status seq_graph_loss(mvs_seq *q, const char *caller, int32_t E, PgLoss &loss)
{
    mvs_ctx *ctx = q->ctx;
    loss = ctx_loss(ctx);
    if (loss.loss == MVS_PG_LOSS_NONE || loss.first != MVS_PG_LOSS_LOOP_EDGES)
        return MVS_OK;
    loss.first = E;
    if (!q->loop_edges_added)
        return MVS_OK;
    HIP_TRY(ctx, hipMemcpyAsync(&loss.first, q->graph_n_built, sizeof(int32_t), hipMemcpyDeviceToHost, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    if (loss.first < 0 || loss.first > E) {
        ctx->err = std::string(caller) + ": the resident graph's count of built edges is out of range";
        return MVS_ERR_HIP;
    }
    return MVS_OK;
}

mvs_status mvs_seq_build_pose_graph(mvs_seq *q, const mvs_seq_graph_params *p)
{
    if (!q || !p || p->max_lag < 1 || p->max_lag >= q->n_frames || p->min_points < 0 || !(p->max_error >= 0.0) ||
        p->chain_sigma[0] != p->chain_sigma[0] || p->chain_sigma[1] != p->chain_sigma[1])
        return MVS_ERR_INVALID_ARG;
    const int64_t slots64 = (int64_t)p->max_lag * q->n_frames - (int64_t)p->max_lag * (p->max_lag + 1) / 2;
    if (q->n_frames > kPgMaxNodes || slots64 > kPgMaxEdges)
        return MVS_ERR_CAPACITY;
    if (!q->ran || p->max_lag > q->lags_ran)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    q->graph_built = q->graph_opt = q->graph_sim3 = false;
    const size_t S = (size_t)slots64;
    // room behind the slots for the loop edges of the current selection (mvs_seq_add_loop_edges grows the block otherwise)
    const size_t want = S + (q->loop_selected ? (size_t)q->ld.max_candidates : 0);
    const SeqGraphLayout L(S, want > (size_t)kPgMaxEdges ? S : want, (size_t)q->n_frames);
    const mvs_status st = ws_grow(ctx, q->graph, L.total);
    if (st != MVS_OK)
        return st;
    SeqGraphDev g{};
    g.n_frames = q->n_frames, g.max_lag = p->max_lag, g.n_slots = (int)S;
    g.min_points = p->min_points;
    g.max_error = p->max_error;
    g.chain_on = p->chain_sigma[0] > 0.0 && p->chain_sigma[1] > 0.0;
    g.chain_var[0] = p->chain_sigma[0] * p->chain_sigma[0];
    g.chain_var[1] = p->chain_sigma[1] * p->chain_sigma[1];
    g.lags = q->lagws.ptr<LagDev>();
    g.traj_R = q->chain.traj_R, g.traj_t = q->chain.traj_t;
    L.point(g, q->graph.ptr());
    seq_graph_adopt(q, L);
    q->loop_edges_added = false;
    launch_seq_graph(g, ctx_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    q->gd = g;
    q->graph_built = true;
    return MVS_OK;
}

mvs_status mvs_seq_optimize_pose_graph(mvs_seq *q, const mvs_pose_graph_params *params, mvs_pose_graph_result *result)
{
    if (!q || !q->graph_built || !result || !pose_graph_params_ok(params))
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SeqGraphDev &g = q->gd;
    hipStream_t s = ctx_stream(ctx);
    q->graph_opt = false;
    *result = mvs_pose_graph_result{};
    SeqGraphHead head;
    mvs_status st = seq_graph_head(q, "mvs_seq_optimize_pose_graph", head);
    if (st != MVS_OK)
        return st;
    const int N = g.n_frames, E = head.n_edges;
    PgLoss loss;
    if ((st = seq_graph_loss(q, "mvs_seq_optimize_pose_graph", E, loss)) != MVS_OK)
        return st;
    PgdPlan plan;
    const bool direct = ctx->pg_solver == MVS_PG_SOLVER_DIRECT && N > kPgDenseMaxNodes;
    if (direct && (st = pgd_plan(N, E, 0, head.src, head.dst, plan)) != MVS_OK)
        return st;
    if (!pose_graph_connected(N, E, head.src, head.dst, 0))
        return MVS_NO_MODEL;
    if (N <= kPgDenseMaxNodes) {
        PgProblem pr{};
        pr.n_nodes = N, pr.n_edges = E, pr.anchor = 0;
        const PgDenseLayout L(1, (size_t)N, (size_t)E);
        const size_t o_desc = L.total;
        if ((st = ws_grow(ctx, ctx->pg, o_desc + sizeof(PgProblem))) != MVS_OK)
            return st;
        char *base = ctx->pg.ptr();
        HIP_TRY(ctx, hipMemcpyAsync(base + o_desc, &pr, sizeof(pr), hipMemcpyHostToDevice, s));
        st = pose_graph_dense_dev(ctx, base, L, 1, *params, loss, reinterpret_cast<const PgProblem *>(base + o_desc), g.node_pose,
                                  g.edge_src, g.edge_dst, g.edge_pose, g.edge_cov);
        if (st != MVS_OK)
            return st;
        HIP_TRY(ctx, hipMemcpyAsync(result, base + L.o_out, sizeof(*result), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, sync_stream(ctx));   // `pr` lives on this frame
        if (result->ok)
            HIP_TRY(ctx, hipMemcpyAsync(q->graph_opt_pose, base + L.o_po, (size_t)N * 96, hipMemcpyDeviceToDevice, s));
    } else {
        if ((st = ws_grow(ctx, ctx->pg, pg_large_scratch((size_t)N, (size_t)E, direct ? &plan : nullptr))) != MVS_OK)
            return st;
        st = pose_graph_large_dev(ctx, ctx->pg.ptr(), N, E, 0, head.src, head.dst, g.edge_src, g.edge_dst, g.node_pose, g.edge_pose,
                                  g.edge_cov, *params, loss, result, q->graph_opt_pose, hipMemcpyDeviceToDevice,
                                  direct ? &plan : nullptr);
        if (st != MVS_OK)
            return st;
    }
    q->graph_opt = result->ok != 0;
    return result->ok ? MVS_OK : MVS_NO_MODEL;
}

mvs_status mvs_seq_download_pose_graph(mvs_seq *q, int32_t *n_edges, double *node_pose, int32_t *edge_src, int32_t *edge_dst,
                                       double *edge_pose, double *edge_cov, int32_t *edge_lag, int32_t *edge_kind,
                                       double *edge_scale)
{
    if (!q || !q->graph_built || !n_edges)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(n_edges, q->gd.n_edges, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    const size_t E = (size_t)std::min(std::max(*n_edges, 0), q->graph_edge_cap);
    const SeqGraphLayout L = seq_graph_layout(q);
    const struct {
        void *dst;
        SeqGraphLayout::Part part;
    } parts[] = {{node_pose, L.kNode}, {edge_src, L.kSrc}, {edge_dst, L.kDst}, {edge_pose, L.kPose},
                 {edge_cov, L.kCov}, {edge_lag, L.kLag}, {edge_kind, L.kKind}, {edge_scale, L.kScale}};
    for (const auto &pt : parts)
        if (pt.dst && L.bytes(pt.part, E))
            HIP_TRY(ctx, hipMemcpyAsync(pt.dst, q->graph.ptr() + L.off[pt.part], L.bytes(pt.part, E), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_download_pose_graph_poses(mvs_seq *q, double *poses)
{
    if (!q || !poses || !q->graph_built || !q->graph_opt)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(poses, q->graph_opt_pose, (size_t)q->n_frames * 96, hipMemcpyDeviceToHost, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

// ---- pose graphs over Sim(3) (sim3graph.hip) -----------------------------------------------------
// The SE(3) entries' host side with 13-double records and 49-double covariances; always the conjugate gradient with no loss.
// The connectivity check and the CSR list are the SE(3) ones.

void mvs_sim3_graph_params_default(mvs_sim3_graph_params *p)
{
    if (!p)
        return;
    mvs_refine_params_default(&p->lm);
    p->anchor_sigma[0] = p->anchor_sigma[1] = p->anchor_sigma[2] = 1e-4;
    p->cg_rel_tol = 1e-10;
    p->cg_max_iterations = 0;                         // 7 n_nodes
    p->cg_chunk_iterations = 0;                       // the whole budget at once
}

static S3Cfg to_s3_cfg(const mvs_sim3_graph_params &p)
{
    S3Cfg c{};
    c.max_iterations = p.lm.max_iterations;
    c.lambda_initial = p.lm.lambda_initial;
    c.lambda_factor = p.lm.lambda_factor;
    c.lambda_upper = p.lm.lambda_upper;
    c.rel_tol = p.lm.rel_tol;
    c.abs_tol = p.lm.abs_tol;
    for (int k = 0; k < 3; ++k)
        c.w_anchor[k] = 1.0 / (p.anchor_sigma[k] * p.anchor_sigma[k]);
    c.cg_rel_tol = p.cg_rel_tol;
    c.cg_max_iterations = p.cg_max_iterations;
    return c;
}

static bool sim3_graph_params_ok(const mvs_sim3_graph_params *params)
{
    return params && params->lm.max_iterations >= 0 && params->lm.lambda_initial >= 0.0 && params->lm.lambda_factor > 1.0 &&
           params->lm.lambda_upper > 0.0 && params->anchor_sigma[0] > 0.0 && params->anchor_sigma[1] > 0.0 &&
           params->anchor_sigma[2] > 0.0 && params->cg_rel_tol >= 0.0 && params->cg_max_iterations >= 0;
}

// arguments of one graph: MVS_ERR_INVALID_ARG / MVS_ERR_CAPACITY before anything runs, in pose_graph_check's order
static mvs_status sim3_graph_check(const mvs_sim3_graph &g)
{
    if (g.n_nodes < 1 || g.n_edges < 0 || !g.node_sim3)
        return MVS_ERR_INVALID_ARG;
    if (g.n_edges > 0 && (!g.edge_src || !g.edge_dst || !g.edge_sim3 || !g.edge_cov))
        return MVS_ERR_INVALID_ARG;
    if (g.n_nodes > kPgMaxNodes || g.n_edges > kPgMaxEdges)
        return MVS_ERR_CAPACITY;
    if (g.anchor_node < 0 || g.anchor_node >= g.n_nodes)
        return MVS_ERR_INVALID_ARG;
    if (!edges_in_range(g.n_nodes, g.n_edges, g.edge_src, g.edge_dst))
        return MVS_ERR_INVALID_ARG;
    if (!all_finite(g.node_sim3, kS3Node * (size_t)g.n_nodes) || !all_finite(g.edge_sim3, kS3Node * (size_t)g.n_edges) ||
        !all_finite(g.edge_cov, kS3Cov * (size_t)g.n_edges))
        return MVS_ERR_INVALID_ARG;
    if (!sim3_scales_positive(g.node_sim3, (size_t)g.n_nodes) || !sim3_scales_positive(g.edge_sim3, (size_t)g.n_edges))
        return MVS_ERR_INVALID_ARG;
    return MVS_OK;
}

// scratch of the large path for N nodes and E edges, as offsets from one base
struct S3LargeLayout {
    size_t o_state, o_off, o_inc, o_pa, o_pb, o_W, o_lin, o_u, o_ec, o_D, o_Mf, o_vec[6], o_pq, o_Ha, total;
    S3LargeLayout(size_t N, size_t E)
    {
        Carve L{64};
        o_state = L.take(sizeof(PgState));
        o_off = L.take((N + 1) * 4), o_inc = L.take(2 * E * 4);
        o_pa = L.take(N * kS3Node * 8), o_pb = L.take(N * kS3Node * 8);
        o_W = L.take(E * kS3W * 8), o_lin = L.take(E * kS3Lin * 8), o_u = L.take(E * 7 * 8), o_ec = L.take(E * 8);
        o_D = L.take(N * kS3W * 8), o_Mf = L.take(N * kS3W * 8);
        for (size_t &o : o_vec)
            o = L.take(N * 7 * 8);
        o_pq = L.take(N * 8), o_Ha = L.take(kS3Cov * 8);
        total = L.total();
    }
};

// one graph of 17 .. 4096 nodes: pose_graph_large_dev's LM loop on the host over the s3_* kernels.  h_src / h_dst: the edges
// on the host; every d_* pointer is device memory that stays valid through the call; `base` is scratch of
// S3LargeLayout(N, E).total bytes.  The optimised nodes go to nodes_out with a copy of kind `out_kind`, only when ok.
static mvs_status sim3_graph_large_dev(mvs_ctx *ctx, char *base, int n_nodes, int n_edges, int anchor, const int32_t *h_src,
                                       const int32_t *h_dst, const int32_t *d_src, const int32_t *d_dst, const double *d_node,
                                       const double *d_z, const double *d_cov, const mvs_sim3_graph_params &params,
                                       mvs_pose_graph_result *res, double *nodes_out, hipMemcpyKind out_kind)
{
    const size_t N = (size_t)n_nodes, E = (size_t)n_edges;
    std::vector<int32_t> off, inc;
    incidence_csr(n_nodes, n_edges, h_src, h_dst, off, inc);
    const S3LargeLayout L(N, E);
    hipStream_t s = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemsetAsync(base + L.o_state, 0, sizeof(PgState), s));
    HIP_TRY(ctx, hipMemcpyAsync(base + L.o_off, off.data(), (N + 1) * 4, hipMemcpyHostToDevice, s));
    if (E)
        HIP_TRY(ctx, hipMemcpyAsync(base + L.o_inc, inc.data(), 2 * E * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(base + L.o_pa, d_node, N * kS3Node * 8, hipMemcpyDeviceToDevice, s));
    auto dp = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<const int32_t *>(base + o); };
    S3LargeDev d{};
    d.n_nodes = n_nodes, d.n_edges = n_edges, d.anchor = anchor;
    d.cfg = to_s3_cfg(params);
    d.edge_src = d_src, d.edge_dst = d_dst, d.csr_off = ip(L.o_off), d.csr_inc = ip(L.o_inc);
    d.edge_z = d_z, d.edge_cov = d_cov, d.node0 = d_node;
    d.node[0] = dp(L.o_pa), d.node[1] = dp(L.o_pb);
    d.W = dp(L.o_W), d.lin = dp(L.o_lin), d.u = dp(L.o_u), d.ecost = dp(L.o_ec), d.D = dp(L.o_D), d.Mf = dp(L.o_Mf);
    d.g = dp(L.o_vec[0]), d.x = dp(L.o_vec[1]), d.r = dp(L.o_vec[2]), d.z = dp(L.o_vec[3]), d.p = dp(L.o_vec[4]), d.q = dp(L.o_vec[5]);
    d.pq = dp(L.o_pq), d.Ha = dp(L.o_Ha);
    d.state = reinterpret_cast<PgState *>(base + L.o_state);
    const int cg_max = params.cg_max_iterations > 0 ? params.cg_max_iterations : 7 * n_nodes;
    const int chunk = params.cg_chunk_iterations;
    PgState h{};
    mvs_status st;
    // the status word behind what has been launched so far: the one place this function waits for the device
    auto read_state = [&]() -> mvs_status {
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&h, d.state, sizeof(h), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, sync_stream(ctx));
        return MVS_OK;
    };
    launch_s3_prep(d, s);
    if ((st = read_state()) != MVS_OK)   // `off` and `inc` have been read by here, too
        return st;
    if (h.bad_cov) {
        *res = mvs_pose_graph_result{};
        return MVS_OK;
    }
    const S3Cfg &cfg = d.cfg;
    int cb = 0, it = 0, rejected = 0, cg_total = 0;
    double cur = 0.0, cost0 = 0.0, lam = cfg.lambda_initial;
    bool ok0 = true, have0 = false;
    // one iteration on the device and its status; the first one also gives the cost at the initial values
    auto iterate = [&](bool with_cg) -> mvs_status {
        launch_s3_begin(d, cb, lam, !have0, s);
        if (with_cg && chunk <= 0) {
            launch_s3_cg(d, lam, cg_max, s);
        } else if (with_cg) {
            // chunk by chunk: the iterations not enqueued are the ones the status word would have sent away at once
            for (int left = cg_max; left > 0;) {
                const int n = std::min(chunk, left);
                launch_s3_cg(d, lam, n, s);
                left -= n;
                if (left > 0) {
                    if ((st = read_state()) != MVS_OK)
                        return st;
                    if (h.done)
                        break;
                }
            }
        }
        launch_s3_end(d, cb, s);
        if ((st = read_state()) != MVS_OK)
            return st;
        if (!have0) {
            have0 = true;
            cost0 = cur = h.cost0;
            ok0 = std::isfinite(cur);
        }
        return MVS_OK;
    };
    while (ok0 && it < cfg.max_iterations) {
        if ((st = iterate(true)) != MVS_OK)
            return st;
        if (!ok0)
            break;
        cg_total += h.cg_iters;
        // the linear solve counts as done when the CG converged, or ran out of iterations with a smaller residual
        const bool solved = h.done == 1 || (h.done == 0 && h.rr < h.gnorm2);
        const double cand = h.cand;
        const bool accepted = solved && cand <= cur;
        ++it;
        if (accepted) {
            cb ^= 1;
            const double dec = 0.5 * (cur - cand);
            const bool done = dec <= cfg.abs_tol || dec <= cfg.rel_tol * (0.5 * cur);
            cur = cand;
            lam = lam / cfg.lambda_factor;
            if (done)
                break;
        } else {
            ++rejected;
            const double inc_e = 0.5 * (cand - cur);
            if (solved && (inc_e <= cfg.abs_tol || inc_e <= cfg.rel_tol * (0.5 * cur)))
                break;
            lam = lam * cfg.lambda_factor;
            if (lam > cfg.lambda_upper)
                break;
        }
    }
    // max_iterations = 0: the cost at the initial values alone (an iteration with no CG steps leaves x = 0)
    if (!have0 && (st = iterate(false)) != MVS_OK)
        return st;
    res->ok = ok0 ? 1 : 0;
    res->iterations = it;
    res->cg_iterations = cg_total;
    res->rejected_steps = rejected;
    res->error_initial = ok0 ? 0.5 * cost0 : 0.0;
    res->error = ok0 ? 0.5 * cur : 0.0;
    if (ok0) {
        HIP_TRY(ctx, hipMemcpyAsync(nodes_out, d.node[cb], N * kS3Node * 8, out_kind, s));
        HIP_TRY(ctx, sync_stream(ctx));
    }
    return MVS_OK;
}

// scratch of a dense-path batch of G graphs with sumN nodes and sumE edges.  Outputs first and contiguous (results, nodes): a
// download is their prefix.
struct S3DenseLayout {
    size_t o_out, o_po, down, o_W, o_lin, total;
    S3DenseLayout(size_t G, size_t sumN, size_t sumE)
    {
        Carve L{64};
        o_out = L.take(G * sizeof(mvs_pose_graph_result)), o_po = L.take(sumN * kS3Node * 8);
        down = L.total();
        o_W = L.take(sumE * kS3W * 8), o_lin = L.take(sumE * kS3Lin * 8);
        total = L.total();
    }
};

// graphs of up to 16 nodes over device-resident inputs: one launch.  `base`: scratch of S3DenseLayout::total bytes.
static mvs_status sim3_graph_dense_dev(mvs_ctx *ctx, char *base, const S3DenseLayout &L, int n_graphs,
                                       const mvs_sim3_graph_params &params, const PgProblem *d_prob, const double *d_node,
                                       const int32_t *d_src, const int32_t *d_dst, const double *d_z, const double *d_cov)
{
    S3DenseDev d{};
    d.n_problems = n_graphs;
    d.cfg = to_s3_cfg(params);
    d.prob = d_prob;
    d.node = d_node;
    d.edge_z = d_z;
    d.edge_cov = d_cov;
    d.edge_src = d_src;
    d.edge_dst = d_dst;
    d.W = reinterpret_cast<double *>(base + L.o_W);
    d.lin = reinterpret_cast<double *>(base + L.o_lin);
    d.nodes_out = reinterpret_cast<double *>(base + L.o_po);
    d.out = reinterpret_cast<mvs_pose_graph_result *>(base + L.o_out);
    launch_s3_dense(d, ctx_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    return MVS_OK;
}

mvs_status mvs_sim3_graph_optimize_batch(mvs_ctx *ctx, const mvs_sim3_graph *graphs, int n_graphs,
                                         const mvs_sim3_graph_params *params, mvs_pose_graph_result *results, double *nodes_out)
{
    if (!ctx || !graphs || n_graphs < 1 || !params || !results || !nodes_out)
        return MVS_ERR_INVALID_ARG;
    if (!sim3_graph_params_ok(params))
        return MVS_ERR_INVALID_ARG;
    int Nmax = 0;
    for (int i = 0; i < n_graphs; ++i) {
        const mvs_status st = sim3_graph_check(graphs[i]);
        if (st != MVS_OK)
            return st;
        Nmax = std::max(Nmax, graphs[i].n_nodes);
    }
    std::memset(results, 0, (size_t)n_graphs * sizeof(mvs_pose_graph_result));
    std::vector<char> joined((size_t)n_graphs);
    for (int i = 0; i < n_graphs; ++i) {
        const mvs_sim3_graph &g = graphs[i];
        joined[(size_t)i] = pose_graph_connected(g.n_nodes, g.n_edges, g.edge_src, g.edge_dst, g.anchor_node) ? 1 : 0;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    // the batch's graphs of up to 16 nodes: one upload, one launch, one download
    std::vector<PgProblem> desc;
    std::vector<int> which;
    size_t sumN = 0, sumE = 0;
    for (int i = 0; i < n_graphs; ++i) {
        const mvs_sim3_graph &g = graphs[i];
        if (!joined[(size_t)i] || g.n_nodes > kS3DenseMaxNodes)
            continue;
        PgProblem p{};
        p.n_nodes = g.n_nodes, p.n_edges = g.n_edges, p.anchor = g.anchor_node;
        p.node_off = (int64_t)sumN, p.edge_off = (int64_t)sumE;
        sumN += (size_t)g.n_nodes;
        sumE += (size_t)g.n_edges;
        desc.push_back(p);
        which.push_back(i);
    }
    if (!desc.empty()) {
        const size_t G = desc.size();
        const S3DenseLayout L(G, sumN, sumE);
        const size_t o_up = L.total;   // the uploaded block: descriptors, nodes, edge measurements, covariances, src, dst
        Carve U{64};
        const size_t u_desc = U.take(G * sizeof(PgProblem)), u_np = U.take(sumN * kS3Node * 8), u_z = U.take(sumE * kS3Node * 8);
        const size_t u_cov = U.take(sumE * kS3Cov * 8), u_src = U.take(sumE * 4), u_dst = U.take(sumE * 4);
        mvs_status st = ws_grow(ctx, ctx->pg, o_up + U.total());
        if (st != MVS_OK)
            return st;
        std::vector<char> up(U.total());
        std::memcpy(up.data() + u_desc, desc.data(), G * sizeof(PgProblem));
        for (size_t k = 0; k < G; ++k) {
            const mvs_sim3_graph &g = graphs[which[k]];
            const size_t n = (size_t)g.n_nodes, e = (size_t)g.n_edges, no = (size_t)desc[k].node_off, eo = (size_t)desc[k].edge_off;
            std::memcpy(up.data() + u_np + no * kS3Node * 8, g.node_sim3, n * kS3Node * 8);
            if (e) {
                std::memcpy(up.data() + u_z + eo * kS3Node * 8, g.edge_sim3, e * kS3Node * 8);
                std::memcpy(up.data() + u_cov + eo * kS3Cov * 8, g.edge_cov, e * kS3Cov * 8);
                std::memcpy(up.data() + u_src + eo * 4, g.edge_src, e * 4);
                std::memcpy(up.data() + u_dst + eo * 4, g.edge_dst, e * 4);
            }
        }
        char *base = ctx->pg.ptr();
        HIP_TRY(ctx, hipMemcpyAsync(base + o_up, up.data(), up.size(), hipMemcpyHostToDevice, s));
        auto dp = [&](size_t o) { return reinterpret_cast<const double *>(base + o_up + o); };
        auto ip = [&](size_t o) { return reinterpret_cast<const int32_t *>(base + o_up + o); };
        st = sim3_graph_dense_dev(ctx, base, L, (int)G, *params, reinterpret_cast<const PgProblem *>(base + o_up + u_desc), dp(u_np),
                                  ip(u_src), ip(u_dst), dp(u_z), dp(u_cov));
        if (st != MVS_OK)
            return st;
        std::vector<char> host(L.down);
        HIP_TRY(ctx, hipMemcpyAsync(host.data(), base, L.down, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, sync_stream(ctx));
        for (size_t k = 0; k < G; ++k) {
            const int i = which[k];
            std::memcpy(&results[i], host.data() + L.o_out + k * sizeof(mvs_pose_graph_result), sizeof(mvs_pose_graph_result));
            if (results[i].ok)
                std::memcpy(nodes_out + (size_t)i * Nmax * kS3Node, host.data() + L.o_po + (size_t)desc[k].node_off * kS3Node * 8,
                            (size_t)graphs[i].n_nodes * kS3Node * 8);
        }
    }
    // larger graphs, one after another: upload in front of the solver's scratch
    for (int i = 0; i < n_graphs; ++i) {
        const mvs_sim3_graph &g = graphs[i];
        if (!joined[(size_t)i] || g.n_nodes <= kS3DenseMaxNodes)
            continue;
        const size_t N = (size_t)g.n_nodes, E = (size_t)g.n_edges;
        const struct {
            const void *host;
            size_t bytes;
        } parts[] = {{g.edge_src, E * 4}, {g.edge_dst, E * 4}, {g.edge_sim3, E * kS3Node * 8}, {g.edge_cov, E * kS3Cov * 8},
                     {g.node_sim3, N * kS3Node * 8}};
        Carve U{64};
        size_t o[5];
        for (int k = 0; k < 5; ++k)
            o[k] = U.take(parts[k].bytes);
        mvs_status st = ws_grow(ctx, ctx->pg, U.total() + S3LargeLayout(N, E).total);
        if (st != MVS_OK)
            return st;
        char *base = ctx->pg.ptr();
        for (int k = 0; k < 5; ++k)
            if (parts[k].bytes)
                HIP_TRY(ctx, hipMemcpyAsync(base + o[k], parts[k].host, parts[k].bytes, hipMemcpyHostToDevice, s));
        auto dp = [&](int k) { return reinterpret_cast<const double *>(base + o[k]); };
        auto ip = [&](int k) { return reinterpret_cast<const int32_t *>(base + o[k]); };
        st = sim3_graph_large_dev(ctx, base + U.total(), g.n_nodes, g.n_edges, g.anchor_node, g.edge_src, g.edge_dst, ip(0), ip(1), dp(4),
                                  dp(2), dp(3), *params, &results[i], nodes_out + (size_t)i * Nmax * kS3Node, hipMemcpyDeviceToHost);
        if (st != MVS_OK)
            return st;
    }
    bool all_ok = true;
    for (int i = 0; i < n_graphs; ++i)
        all_ok = all_ok && results[i].ok;
    return all_ok ? MVS_OK : MVS_NO_MODEL;
}

mvs_status mvs_sim3_graph_optimize(mvs_ctx *ctx, const mvs_sim3_graph *graph, const mvs_sim3_graph_params *params,
                                   mvs_pose_graph_result *result, double *nodes_out)
{
    return mvs_sim3_graph_optimize_batch(ctx, graph, 1, params, result, nodes_out);
}

mvs_status mvs_seq_optimize_pose_graph_sim3(mvs_seq *q, const mvs_sim3_graph_params *params, const double scale_sigma[3],
                                            mvs_pose_graph_result *result)
{
    if (!q || !q->graph_built || !result || !scale_sigma || !sim3_graph_params_ok(params) || !scale_sigmas_ok(scale_sigma))
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SeqGraphDev &g = q->gd;
    hipStream_t s = ctx_stream(ctx);
    q->graph_sim3 = false;
    *result = mvs_pose_graph_result{};
    SeqGraphHead head;
    mvs_status st = seq_graph_head(q, "mvs_seq_optimize_pose_graph_sim3", head);
    if (st != MVS_OK)
        return st;
    const int N = g.n_frames, E = head.n_edges;
    if (!pose_graph_connected(N, E, head.src, head.dst, 0))
        return MVS_NO_MODEL;
    const size_t Nz = (size_t)N, Ez = (size_t)E;
    const bool dense = N <= kS3DenseMaxNodes;
    const S3DenseLayout Ld(1, Nz, Ez);
    // the lifted graph in front of the solver's scratch, the dense path's descriptor behind it
    Carve U{64};
    const size_t o_node = U.take(Nz * kS3Node * 8), o_z = U.take(Ez * kS3Node * 8), o_cov = U.take(Ez * kS3Cov * 8);
    const size_t o_scratch = U.total(), scratch = dense ? Ld.total + sizeof(PgProblem) : S3LargeLayout(Nz, Ez).total;
    if ((st = ws_grow(ctx, ctx->pg, o_scratch + scratch)) != MVS_OK)
        return st;
    if ((st = ws_grow(ctx, q->graph_s3, Nz * kS3Node * 8)) != MVS_OK)
        return st;
    char *base = ctx->pg.ptr();
    S3LiftDev lf{};
    lf.n_nodes = N, lf.n_edges = E;
    for (int k = 0; k < 3; ++k)
        lf.scale_sigma[k] = scale_sigma[k];
    lf.node_pose = g.node_pose, lf.edge_pose = g.edge_pose, lf.edge_cov = g.edge_cov, lf.edge_kind = g.edge_kind;
    lf.node = reinterpret_cast<double *>(base + o_node), lf.edge_z = reinterpret_cast<double *>(base + o_z);
    lf.cov = reinterpret_cast<double *>(base + o_cov);
    launch_s3_lift(lf, s);
    HIP_TRY(ctx, hipGetLastError());
    double *nodes = q->graph_s3.ptr<double>();
    if (dense) {
        PgProblem pr{};
        pr.n_nodes = N, pr.n_edges = E, pr.anchor = 0;
        char *sb = base + o_scratch;
        HIP_TRY(ctx, hipMemcpyAsync(sb + Ld.total, &pr, sizeof(pr), hipMemcpyHostToDevice, s));
        st = sim3_graph_dense_dev(ctx, sb, Ld, 1, *params, reinterpret_cast<const PgProblem *>(sb + Ld.total), lf.node, g.edge_src,
                                  g.edge_dst, lf.edge_z, lf.cov);
        if (st != MVS_OK)
            return st;
        HIP_TRY(ctx, hipMemcpyAsync(result, sb + Ld.o_out, sizeof(*result), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, sync_stream(ctx));   // `pr` lives on this frame
        if (result->ok)
            HIP_TRY(ctx, hipMemcpyAsync(nodes, sb + Ld.o_po, Nz * kS3Node * 8, hipMemcpyDeviceToDevice, s));
    } else {
        st = sim3_graph_large_dev(ctx, base + o_scratch, N, E, 0, head.src, head.dst, g.edge_src, g.edge_dst, lf.node, lf.edge_z, lf.cov,
                                  *params, result, nodes, hipMemcpyDeviceToDevice);
        if (st != MVS_OK)
            return st;
    }
    q->graph_sim3 = result->ok != 0;
    return result->ok ? MVS_OK : MVS_NO_MODEL;
}

mvs_status mvs_seq_download_pose_graph_sim3(mvs_seq *q, double *nodes13)
{
    if (!q || !nodes13 || !q->graph_built || !q->graph_sim3)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(nodes13, q->graph_s3.ptr(), (size_t)q->n_frames * kS3Node * 8, hipMemcpyDeviceToHost, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

// ---- marginal covariances of a pose graph (pg_marginals.hip, pg_envelope.hpp) -------------------
// what the host decides before anything is launched: the query list, the envelope, the per-block term lists, the chunk
struct PgmPlan {
    std::vector<int32_t> first, row_off, qi, qj;
    mvs_pgm::BlockLists lists;
    int64_t blocks = 0;
    int chunk = 1;
};

static mvs_status pgm_plan(int N, int E, int anchor, const int32_t *src, const int32_t *dst, int n_query, const int32_t *qi,
                           const int32_t *qj, PgmPlan &P)
{
    if (!mvs_pgm::expand_queries(N, n_query, qi, qj, P.qi, P.qj))
        return MVS_ERR_INVALID_ARG;
    P.blocks = mvs_pgm::envelope(N, E, src, dst, P.first, P.row_off);
    if (P.blocks > mvs_pgm::kMaxEnvelopeBlocks)
        return MVS_ERR_CAPACITY;
    P.lists = mvs_pgm::block_lists(E, anchor, src, dst, P.first, P.row_off);
    P.chunk = std::min(mvs_pgm::query_chunk(N), (int)P.qi.size());
    return MVS_OK;
}

// the solver's scratch, as offsets from one base in ctx->pgm
struct PgmLayout {
    size_t o_state, o_first, o_row, o_sblk, o_soff, o_codes, o_qi, o_qj, o_Ha, o_out, o_lin, o_sky, o_y, total;
    PgmLayout(size_t N, size_t E, const PgmPlan &P)
    {
        Carve L{64};
        o_state = L.take(sizeof(PgmState));
        o_first = L.take(N * 4), o_row = L.take((N + 1) * 4);
        o_sblk = L.take(P.lists.slot_blk.size() * 4), o_soff = L.take(P.lists.slot_off.size() * 4);
        o_codes = L.take(P.lists.codes.size() * 4);
        o_qi = L.take(P.qi.size() * 4), o_qj = L.take(P.qj.size() * 4);
        o_Ha = L.take(36 * 8), o_out = L.take((size_t)P.chunk * 36 * 8);
        o_lin = L.take(E * kPgLin * 8), o_sky = L.take((size_t)P.blocks * 36 * 8);
        o_y = L.take((size_t)P.chunk * N * 6 * mvs_pgm::kYCols * 8);
        total = L.total();
    }
};

// assembly, factorisation and the solves over a device-resident graph; `base`: scratch of PgmLayout::total bytes.  d_node
// holds the anchor's mean, d_X the linearisation point.  cov_out is written only behind a factorisation that succeeded.
static mvs_status pgm_run(mvs_ctx *ctx, char *base, const PgmLayout &L, const PgmPlan &P, int N, int E, int anchor,
                          const int32_t *d_src, const int32_t *d_dst, const double *d_node, const double *d_X, const double *d_z,
                          const double *d_cov, const double anchor_sigma[2], double *cov_out, mvs_pose_graph_marginals_info *info)
{
    hipStream_t s = ctx_stream(ctx);
    const PgmState st0{0, -1, HUGE_VAL};
    auto up = [&](size_t o, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIP_TRY(ctx, up(L.o_state, &st0, sizeof(st0)));
    HIP_TRY(ctx, up(L.o_first, P.first.data(), P.first.size() * 4));
    HIP_TRY(ctx, up(L.o_row, P.row_off.data(), P.row_off.size() * 4));
    HIP_TRY(ctx, up(L.o_sblk, P.lists.slot_blk.data(), P.lists.slot_blk.size() * 4));
    HIP_TRY(ctx, up(L.o_soff, P.lists.slot_off.data(), P.lists.slot_off.size() * 4));
    HIP_TRY(ctx, up(L.o_codes, P.lists.codes.data(), P.lists.codes.size() * 4));
    HIP_TRY(ctx, up(L.o_qi, P.qi.data(), P.qi.size() * 4));
    HIP_TRY(ctx, up(L.o_qj, P.qj.data(), P.qj.size() * 4));
    HIP_TRY(ctx, hipMemsetAsync(base + L.o_sky, 0, (size_t)P.blocks * 36 * 8, s));
    auto dp = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<const int32_t *>(base + o); };
    PgmDev d{};
    d.n_nodes = N, d.n_edges = E, d.anchor = anchor, d.n_slots = (int)P.lists.slot_blk.size();
    anchor_weights(anchor_sigma, d.w_anchor);
    d.edge_src = d_src, d.edge_dst = d_dst, d.edge_pose = d_z, d.edge_cov = d_cov, d.pose0 = d_node, d.X = d_X;
    d.first = ip(L.o_first), d.row_off = ip(L.o_row), d.slot_blk = ip(L.o_sblk), d.slot_off = ip(L.o_soff), d.codes = ip(L.o_codes);
    d.lin = dp(L.o_lin), d.Ha = dp(L.o_Ha), d.sky = dp(L.o_sky), d.y = dp(L.o_y), d.out = dp(L.o_out);
    d.state = reinterpret_cast<PgmState *>(base + L.o_state);
    launch_pgm_assemble(d, s);
    launch_pgm_factor(d, s);
    HIP_TRY(ctx, hipGetLastError());
    PgmState h{};
    HIP_TRY(ctx, hipMemcpyAsync(&h, d.state, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));   // the plan's vectors and st0 have been read by here, too
    info->bad_node = h.bad_node;
    info->min_pivot = h.status == 1 ? 0.0 : std::sqrt(h.min_d);
    if (h.status)
        return MVS_NO_MODEL;
    const int nq = (int)P.qi.size();
    for (int off = 0; off < nq; off += P.chunk) {
        const int n = std::min(P.chunk, nq - off);
        d.qi = ip(L.o_qi) + off, d.qj = ip(L.o_qj) + off;
        launch_pgm_solve(d, n, s);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(cov_out + (size_t)off * 36, d.out, (size_t)n * 36 * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, sync_stream(ctx));
    info->ok = 1;
    return MVS_OK;
}

// what info reads until a factorisation has run: not ok, no failed pivot
static const mvs_pose_graph_marginals_info kPgmNoInfo{0, 0, -1, 0, 0.0};

static bool pgm_args_ok(const double anchor_sigma[2], int n_query, const double *cov_out, const mvs_pose_graph_marginals_info *info)
{
    return anchor_sigma && anchor_sigma[0] > 0.0 && anchor_sigma[1] > 0.0 && n_query >= 0 && cov_out && info;
}

mvs_status mvs_pose_graph_marginals(mvs_ctx *ctx, const mvs_pose_graph *graph, const double *poses, const double anchor_sigma[2],
                                    int n_query, const int32_t *query_i, const int32_t *query_j, double *cov_out,
                                    mvs_pose_graph_marginals_info *info)
{
    if (!ctx || !graph || !pgm_args_ok(anchor_sigma, n_query, cov_out, info))
        return MVS_ERR_INVALID_ARG;
    const mvs_pose_graph &g = *graph;
    mvs_status st = pose_graph_check(g);
    if (st != MVS_OK)
        return st;
    const size_t N = (size_t)g.n_nodes, E = (size_t)g.n_edges;
    if (poses && !all_finite(poses, 12 * N))
        return MVS_ERR_INVALID_ARG;
    *info = kPgmNoInfo;
    PgmPlan P;
    st = pgm_plan(g.n_nodes, g.n_edges, g.anchor_node, g.edge_src, g.edge_dst, n_query, query_i, query_j, P);
    if (st != MVS_OK)
        return st;
    info->envelope_blocks = (int32_t)P.blocks;
    if (!pose_graph_connected(g.n_nodes, g.n_edges, g.edge_src, g.edge_dst, g.anchor_node))
        return MVS_NO_MODEL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const PgmLayout L(N, E, P);
    PgUploaded u;
    if ((st = pose_graph_upload(ctx, ctx->pgm, g, poses ? poses : g.node_pose, L.total, u)) != MVS_OK)
        return st;
    return pgm_run(ctx, u.scratch, L, P, g.n_nodes, g.n_edges, g.anchor_node, u.src, u.dst, u.node, u.x, u.z, u.cov, anchor_sigma,
                   cov_out, info);
}

mvs_status mvs_seq_pose_graph_marginals(mvs_seq *q, const double anchor_sigma[2], int n_query, const int32_t *query_i,
                                        const int32_t *query_j, double *cov_out, mvs_pose_graph_marginals_info *info)
{
    if (!q || !q->graph_built || !q->graph_opt || !pgm_args_ok(anchor_sigma, n_query, cov_out, info))
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SeqGraphDev &g = q->gd;
    SeqGraphHead head;
    mvs_status st = seq_graph_head(q, "mvs_seq_pose_graph_marginals", head);
    if (st != MVS_OK)
        return st;
    const int N = g.n_frames, E = head.n_edges;
    *info = kPgmNoInfo;
    PgmPlan P;
    if ((st = pgm_plan(N, E, 0, head.src, head.dst, n_query, query_i, query_j, P)) != MVS_OK)
        return st;
    info->envelope_blocks = (int32_t)P.blocks;
    if (!pose_graph_connected(N, E, head.src, head.dst, 0))
        return MVS_NO_MODEL;
    const PgmLayout L((size_t)N, (size_t)E, P);
    st = ws_grow(ctx, ctx->pgm, L.total);
    if (st != MVS_OK)
        return st;
    return pgm_run(ctx, ctx->pgm.ptr(), L, P, N, E, 0, g.edge_src, g.edge_dst, g.node_pose, q->graph_opt_pose, g.edge_pose,
                   g.edge_cov, anchor_sigma, cov_out, info);
}

// ---- per-edge residuals and weights (pg_edge_stats_kernel) ----------------------------------------
// scratch of the stats launch for E edges, as offsets from one base: the outputs first and contiguous
struct PgStatsLayout {
    size_t o_chi2, o_weight, o_bad, o_W, total;
    explicit PgStatsLayout(size_t E)
    {
        Carve L{64};
        o_chi2 = L.take(E * 8), o_weight = L.take(E * 8), o_bad = L.take(4), o_W = L.take(E * 21 * 8);
        total = L.total();
    }
};

// the launch over a device-resident graph and poses d_X, and the download; `base`: scratch of PgStatsLayout(E).total bytes.
// MVS_NO_MODEL, nothing written: an edge covariance that is not positive definite.
static mvs_status pg_stats_run(mvs_ctx *ctx, char *base, int E, const PgLoss &loss, const int32_t *d_src, const int32_t *d_dst,
                               const double *d_z, const double *d_cov, const double *d_X, double *chi2, double *weight)
{
    if (E == 0)
        return MVS_OK;
    const PgStatsLayout L((size_t)E);
    hipStream_t s = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemsetAsync(base + L.o_bad, 0, 4, s));
    PgStatsDev d{};
    d.n_edges = E;
    d.cfg.loss = loss.loss, d.cfg.loss_first = loss.first, d.cfg.loss_k = loss.k;
    d.edge_src = d_src, d.edge_dst = d_dst, d.edge_pose = d_z, d.edge_cov = d_cov, d.X = d_X;
    d.W = reinterpret_cast<double *>(base + L.o_W);
    d.chi2 = reinterpret_cast<double *>(base + L.o_chi2);
    d.weight = weight ? reinterpret_cast<double *>(base + L.o_weight) : nullptr;
    d.bad_cov = reinterpret_cast<int32_t *>(base + L.o_bad);
    launch_pg_edge_stats(d, s);
    HIP_TRY(ctx, hipGetLastError());
    int32_t bad = 0;
    std::vector<double> host(2 * (size_t)E);
    HIP_TRY(ctx, hipMemcpyAsync(&bad, d.bad_cov, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), d.chi2, (size_t)E * 8, hipMemcpyDeviceToHost, s));
    if (weight)
        HIP_TRY(ctx, hipMemcpyAsync(host.data() + E, d.weight, (size_t)E * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    if (bad)
        return MVS_NO_MODEL;
    std::memcpy(chi2, host.data(), (size_t)E * 8);
    if (weight)
        std::memcpy(weight, host.data() + E, (size_t)E * 8);
    return MVS_OK;
}

mvs_status mvs_pose_graph_edge_stats(mvs_ctx *ctx, const mvs_pose_graph *graph, const double *poses, double *chi2, double *weight)
{
    if (!ctx || !graph || !chi2 || !loss_fits_host_graph(ctx->pg_loss, ctx->pg_loss_first))
        return MVS_ERR_INVALID_ARG;
    const mvs_pose_graph &g = *graph;
    mvs_status st = pose_graph_check(g);
    if (st != MVS_OK)
        return st;
    if (poses && !all_finite(poses, 12 * (size_t)g.n_nodes))
        return MVS_ERR_INVALID_ARG;
    if (!pose_graph_connected(g.n_nodes, g.n_edges, g.edge_src, g.edge_dst, g.anchor_node))
        return MVS_NO_MODEL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PgUploaded u;
    if ((st = pose_graph_upload(ctx, ctx->pg, g, poses ? poses : g.node_pose, PgStatsLayout((size_t)g.n_edges).total, u)) != MVS_OK)
        return st;
    return pg_stats_run(ctx, u.scratch, g.n_edges, ctx_loss(ctx), u.src, u.dst, u.z, u.cov, u.x, chi2, weight);
}

mvs_status mvs_seq_pose_graph_edge_stats(mvs_seq *q, double *chi2, double *weight)
{
    if (!q || !q->graph_built || !q->graph_opt || !chi2)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SeqGraphDev &g = q->gd;
    SeqGraphHead head;
    mvs_status st = seq_graph_head(q, "mvs_seq_pose_graph_edge_stats", head);
    if (st != MVS_OK)
        return st;
    const int N = g.n_frames, E = head.n_edges;
    PgLoss loss;
    if ((st = seq_graph_loss(q, "mvs_seq_pose_graph_edge_stats", E, loss)) != MVS_OK)
        return st;
    if (!pose_graph_connected(N, E, head.src, head.dst, 0))
        return MVS_NO_MODEL;
    if ((st = ws_grow(ctx, ctx->pg, PgStatsLayout((size_t)E).total)) != MVS_OK)
        return st;
    return pg_stats_run(ctx, ctx->pg.ptr(), E, loss, g.edge_src, g.edge_dst, g.edge_pose, g.edge_cov, q->graph_opt_pose, chi2, weight);
}

// ---- loop closures of a resident sequence (loop.hip, seq_graph.hip) -----------------------------
mvs_status mvs_seq_loop_scores(mvs_seq *q, double ratio, double max_dist, int min_gap)
{
    if (!q)
        return MVS_ERR_INVALID_ARG;
    if (q->n_frames > kLoopMaxFrames)
        return MVS_ERR_CAPACITY;
    if (min_gap < 1 || min_gap >= q->n_frames || ratio != ratio || max_dist != max_dist)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    q->loop_scored = q->loop_selected = q->loop_verified = false;
    const size_t F = (size_t)q->n_frames;
    const mvs_status st = ws_grow(ctx, q->loop_score, F * F * sizeof(int32_t));
    if (st != MVS_OK)
        return st;
    const BatchDev &d = q->batch->d;
    LoopDev &l = q->ld;
    l.n_frames = q->n_frames, l.max_kp = d.max_kp, l.desc_words = d.desc_words;
    l.desc = d.desc1, l.kp = d.kp1, l.oct = d.oct1, l.n_kp = d.n1, l.K = d.K, l.Kinv = d.Kinv;
    l.score = q->loop_score.ptr<int32_t>();
    HIP_TRY(ctx, launch_loop_scores(l, ratio, max_dist, min_gap, ctx_stream(ctx)));
    HIP_TRY(ctx, hipGetLastError());
    q->loop_scored = true;
    return MVS_OK;
}

mvs_status mvs_seq_download_loop_scores(mvs_seq *q, int32_t *scores)
{
    if (!q || !scores || !q->loop_scored)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t F = (size_t)q->n_frames;
    HIP_TRY(ctx, hipMemcpyAsync(scores, q->ld.score, F * F * sizeof(int32_t), hipMemcpyDeviceToHost, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_select_loops(mvs_seq *q, const mvs_loop_select_params *p)
{
    if (!q || !p || !q->loop_scored || p->min_score < 1 || p->top_k < 1 || p->max_candidates < 1)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    q->loop_selected = q->loop_verified = false;
    const size_t F = (size_t)q->n_frames, C = (size_t)p->max_candidates;
    const size_t top_k = (size_t)std::min(p->top_k, q->n_frames);   // a frame has fewer than n_frames base frames
    Carve L{64};
    const size_t o_counts = L.take(2 * 4), o_rown = L.take(F * 4), o_rowkey = L.take(F * top_k * 4);
    const size_t o_cand = L.take(C * sizeof(mvs_loop_candidate));
    const mvs_status st = ws_grow(ctx, q->loop_sel, L.total());
    if (st != MVS_OK)
        return st;
    char *base = q->loop_sel.ptr();
    LoopDev &l = q->ld;
    l.min_score = p->min_score, l.top_k = (int)top_k, l.max_candidates = p->max_candidates;
    l.counts = reinterpret_cast<int32_t *>(base + o_counts);
    l.row_n = reinterpret_cast<int32_t *>(base + o_rown);
    l.row_key = reinterpret_cast<int32_t *>(base + o_rowkey);
    l.cand = reinterpret_cast<mvs_loop_candidate *>(base + o_cand);
    launch_loop_select(l, ctx_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    q->loop_selected = true;
    return MVS_OK;
}

// enqueues the read-back of the selection's counts (candidates kept, candidates found); the caller waits for the stream
static hipError_t loop_counts_async(const mvs_seq *q, int32_t counts[2])
{
    return hipMemcpyAsync(counts, q->ld.counts, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx_stream(q->ctx));
}

mvs_status mvs_seq_verify_loops(mvs_seq *q, const mvs_params *two_view, int essential, const mvs_refine_params *rp,
                                double sigma_px)
{
    if (!q || !q->loop_selected || !refine_params_ok(rp) || !(sigma_px > 0.0))
        return MVS_ERR_INVALID_ARG;
    mvs_status st = check_params(two_view);
    if (st != MVS_OK)
        return st;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    q->loop_verified = false;
    const LoopDev &l = q->ld;
    if (q->loop_batch && q->loop_batch->d.n_pairs != l.max_candidates) {
        mvs_batch_destroy(q->loop_batch);
        q->loop_batch = nullptr;
    }
    if (!q->loop_batch &&
        (st = batch_create_impl(ctx, l.max_candidates, l.max_kp, l.desc_words * 4, 0, &q->loop_batch)) != MVS_OK)
        return st;
    mvs_batch *b = q->loop_batch;
    const Estimator est = essential ? Estimator::kFivePoint : Estimator::kEightPoint;
    if ((st = ensure_tables(b, est, two_view->num_hypotheses)) != MVS_OK)
        return st;
    hipStream_t s = ctx_stream(ctx);
    // the one host read between selection and verification: how many pairs the pipeline runs on
    int32_t counts[2] = {0, 0};
    HIP_TRY(ctx, loop_counts_async(q, counts));
    HIP_TRY(ctx, sync_stream(ctx));
    const int kept = counts[0];
    if (kept < 0 || kept > l.max_candidates) {
        ctx->err = "mvs_seq_verify_loops: candidate count out of range";
        return MVS_ERR_HIP;
    }
    // pairs past the kept ones are no candidates: their records read "invalid", so the refinement skips them
    HIP_TRY(ctx, hipMemsetAsync(b->d.results + kept, 0, (size_t)(l.max_candidates - kept) * sizeof(mvs_pair_result), s));
    if (kept > 0) {
        launch_loop_gather(l, b->d, s);
        HIP_TRY(ctx, hipGetLastError());
        if ((st = run_pairs(b, est, to_run(*two_view), kept)) != MVS_OK)
            return st;
    }
    if ((st = mvs_batch_refine(b, rp, sigma_px)) != MVS_OK)
        return st;
    q->loop_kept = kept;
    q->loop_verified = true;
    return MVS_OK;
}

mvs_status mvs_seq_add_loop_edges(mvs_seq *q, const mvs_loop_edge_params *p)
{
    if (!q || !p)
        return MVS_ERR_INVALID_ARG;
    if (q->graph_built && q->loop_selected && (int64_t)q->gd.n_slots + q->ld.max_candidates > kPgMaxEdges)
        return MVS_ERR_CAPACITY;
    if (p->min_points < 0 || !(p->max_error >= 0.0) || p->loop_sigma[0] != p->loop_sigma[0] || p->loop_sigma[1] != p->loop_sigma[1] ||
        !q->graph_built || !q->loop_verified)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    const int need = q->gd.n_slots + q->ld.max_candidates;
    if (q->graph_edge_cap < need) {
        // the block was carved before this selection: a larger one, every array of the graph copied over at its old capacity
        // (the slots are scratch)
        const SeqGraphLayout Lo = seq_graph_layout(q), Ln(Lo.S, (size_t)need, Lo.F);
        void *np = nullptr;
        HIP_TRY(ctx, hipMalloc(&np, Ln.total));
        DevPtr fresh(np);
        for (int p = 0; p < Lo.kParts; ++p)
            if (Lo.kSpec[p].per != Lo.kSlot)
                HIP_TRY(ctx, hipMemcpyAsync(static_cast<char *>(np) + Ln.off[p], q->graph.ptr() + Lo.off[p], Lo.bytes(p, Lo.cap),
                                            hipMemcpyDeviceToDevice, s));
        HIP_TRY(ctx, sync_stream(ctx));   // the old block is freed
        q->graph.p = std::move(fresh);
        q->graph.bytes = Ln.total;
        Ln.point(q->gd, q->graph.ptr());
        seq_graph_adopt(q, Ln);
    }
    if (!q->loop_edges_added)   // the first call behind a build: remember where the built edges end
        HIP_TRY(ctx, hipMemcpyAsync(q->graph_n_built, q->gd.n_edges, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    LoopEdgeDev e{};
    e.cand = q->ld.cand, e.counts = q->ld.counts;
    e.results = q->loop_batch->d.results, e.refined = q->loop_batch->refine.out;
    e.n_built = q->graph_n_built;
    e.max_candidates = q->ld.max_candidates, e.min_points = p->min_points;
    e.max_error = p->max_error;
    for (int k = 0; k < 2; ++k) {
        e.add[k] = p->loop_sigma[k] > 0.0;
        e.var[k] = p->loop_sigma[k] * p->loop_sigma[k];
    }
    launch_loop_edges(q->gd, e, s);
    HIP_TRY(ctx, hipGetLastError());
    q->loop_edges_added = true;
    q->graph_opt = q->graph_sim3 = false;
    return MVS_OK;
}

mvs_status mvs_seq_download_loop_candidates(mvs_seq *q, int32_t *n_kept, int32_t *n_found, mvs_loop_candidate *cand,
                                            mvs_pair_result *results, mvs_match *matches, uint8_t *inlier_mask,
                                            double *points_xyz, int64_t *point_idx, mvs_refine_result *refined)
{
    if (!q || !q->loop_selected)
        return MVS_ERR_INVALID_ARG;
    const bool pairs = results || matches || inlier_mask || points_xyz || point_idx;
    if ((pairs || refined) && !q->loop_verified)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx_stream(ctx);
    int32_t counts[2] = {0, 0};
    HIP_TRY(ctx, loop_counts_async(q, counts));
    if (cand)
        HIP_TRY(ctx, hipMemcpyAsync(cand, q->ld.cand, (size_t)q->ld.max_candidates * sizeof(mvs_loop_candidate), hipMemcpyDeviceToHost, s));
    if (refined && q->loop_kept > 0)
        HIP_TRY(ctx, hipMemcpyAsync(refined, q->loop_batch->refine.out, (size_t)q->loop_kept * sizeof(mvs_refine_result),
                                    hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    if (n_kept)
        *n_kept = counts[0];
    if (n_found)
        *n_found = counts[1];
    if (pairs && q->loop_kept > 0)
        return mvs_batch_download(q->loop_batch, 0, q->loop_kept, results, matches, inlier_mask, points_xyz, point_idx);
    return MVS_OK;
}
}  // extern "C"
