// capi_ba.hip -- the host side of the sparse bundle adjustment (include/mvslam_hip.h; DESIGN.md sections 4.7.4 and 4.7.5).
// One solver, bas_solve: the LM loop of refine_window_kernel driven from here over a problem and a plan that lie in device
// memory -- the device computes (ba_sparse.hip, pg_direct.hip), the host decides, one synchronisation per iteration.  Two
// entries feed it: mvs_ba_refine_sparse (argument checks, the plan of ba_envelope.hpp, packing and upload into a workspace of
// the context) and mvs_seq_refine_global (the problem and the plan built on the device from a resident sequence by
// seq_global.hip, in two workspaces of the sequence).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ba_envelope.hpp"
#include "capi_internal.hpp"
#include "pg_host.hpp"
#include "seq_global_host.hpp"

using namespace mvs_host;

namespace {

bool all_finite(const double *v, size_t n)
{
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(v[k]))
            return false;
    return true;
}

// a prior variance as the weight the kernels read: none where the variance is not positive
double prior_weight(double var) { return var > 0.0 ? 1.0 / var : 0.0; }

// the solver's own arrays as offsets into a workspace, laid out behind whatever the entry has laid out for its inputs and lists
struct BasWork {
    size_t pose[2], pts[2], lin, oinfo_w, Li, gh, Z, zd, prior, D, g, sky, Cinv, y, x, terms, part, pst, bst, inv, colm, pcov, ptcov;
    bool want_cov, pose_cov, point_cov;
};
BasWork carve_work(Carve &L, size_t F, size_t P, size_t O, size_t B, bool pose_cov, bool point_cov)
{
    BasWork k{};
    const bool want_cov = pose_cov || point_cov;
    const int64_t n_terms = (int64_t)O + (int64_t)P + (int64_t)F;
    const size_t chunks = (size_t)((n_terms + kBasRedChunk - 1) / kBasRedChunk);
    k.pose[0] = L.take(12 * F * 8), k.pose[1] = L.take(12 * F * 8);
    k.pts[0] = L.take(3 * P * 8), k.pts[1] = L.take(3 * P * 8);
    k.lin = L.take((size_t)kBasLin * O * 8), k.Li = L.take(6 * P * 8), k.gh = L.take(3 * P * 8);
    k.oinfo_w = L.take(3 * O * 8);   // w(s_o) W_o of a robust loss; not touched without one
    k.Z = L.take(18 * O * 8), k.zd = L.take(3 * O * 8);
    k.prior = L.take(27 * F * 8);
    k.D = L.take(21 * F * 8), k.g = L.take(6 * F * 8), k.sky = L.take(36 * B * 8);
    k.Cinv = L.take(21 * F * 8), k.y = L.take(6 * F * 8), k.x = L.take(6 * F * 8);
    k.terms = L.take((size_t)n_terms * 8), k.part = L.take(chunks * 8);
    k.pst = L.take(sizeof(PgdState)), k.bst = L.take(sizeof(BasState));
    k.inv = L.take(want_cov ? 36 * B * 8 : 0), k.colm = L.take(want_cov ? 36 * F * 8 : 0);
    k.pcov = L.take(pose_cov ? 36 * F * 8 : 0), k.ptcov = L.take(point_cov ? 9 * P * 8 : 0);
    k.want_cov = want_cov, k.pose_cov = pose_cov, k.point_cov = point_cov;
    return k;
}
// d's counts, inputs and lists are set: this adds the solver's arrays, and pd, the step (pg_direct.hip's kernels on their
// second source), and the context's robust loss: with one, the build kernels read the reweighted information matrices
void bind_work(const mvs_ctx *ctx, char *base, const BasWork &k, BasDev &d, PgdDev &pd)
{
    auto dp = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    d.loss = ctx->ba_loss, d.loss_k = ctx->ba_loss_k;
    d.oinfo0 = d.oinfo, d.oinfo_w = dp(k.oinfo_w);
    if (d.loss != MVS_BA_LOSS_NONE)
        d.oinfo = d.oinfo_w;
    d.pose[0] = dp(k.pose[0]), d.pose[1] = dp(k.pose[1]), d.pts[0] = dp(k.pts[0]), d.pts[1] = dp(k.pts[1]);
    d.lin = dp(k.lin), d.Li = dp(k.Li), d.gh = dp(k.gh), d.Z = dp(k.Z), d.zd = dp(k.zd), d.D = dp(k.D), d.g = dp(k.g);
    d.prior = dp(k.prior);
    d.sky = dp(k.sky), d.Cinv = dp(k.Cinv), d.x = dp(k.x), d.terms = dp(k.terms), d.partial = dp(k.part);
    d.inv = k.want_cov ? dp(k.inv) : nullptr, d.colm = k.want_cov ? dp(k.colm) : nullptr;
    d.pose_cov = k.pose_cov ? dp(k.pcov) : nullptr, d.point_cov = k.point_cov ? dp(k.ptcov) : nullptr;
    d.state = reinterpret_cast<BasState *>(base + k.bst);
    pd = PgdDev{};
    pd.n_nodes = d.n_frames, pd.n_blocks = d.n_blocks;
    pd.first = d.first, pd.row_off = d.row_off, pd.blk_row = d.blk_row;
    pd.D = d.D, pd.g = d.g, pd.Cinv = dp(k.Cinv), pd.sky = d.sky, pd.y = dp(k.y), pd.x = dp(k.x);
    pd.state = reinterpret_cast<PgdState *>(base + k.pst);
    pd.pre = d.sky, pd.pivot_tol = kBaPivotTol;
}

// The solver over a problem whose inputs and lists lie in device memory (or are on their way there on the context's stream):
// the LM loop from the guesses pose0 / pts0, then the factorisation at the estimate with lambda = 0, which decides ok and is
// what launch_bas_cov continues from.  Under a robust loss (d.loss) the cost is the robust one and every build the reweighted
// one (IRLS), so that factorisation is the reweighted system's; the rule and the exits below do not know.  *result is filled
// whenever MVS_OK or MVS_NO_MODEL is returned; the estimate is then d.pose[*cur_out] / d.pts[*cur_out].
mvs_status bas_solve(mvs_ctx *ctx, const BasDev &d, const PgdDev &pd, const mvs_refine_params *params, int widest,
                     mvs_ba_sparse_result *result, int *cur_out)
{
    const int F = d.n_frames;
    hipStream_t s = ctx_stream(ctx);
    mvs_status st = MVS_OK;
    HIP_TRY(ctx, hipMemcpyAsync(d.pose[0], d.pose0, 12 * (size_t)F * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.pts[0], d.pts0, 3 * (size_t)d.n_points * 8, hipMemcpyDeviceToDevice, s));

    BasState hb{};
    PgdState hd{};
    auto read_state = [&]() -> mvs_status {
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&hb, d.state, sizeof(hb), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(&hd, pd.state, sizeof(hd), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, sync_stream(ctx));
        return MVS_OK;
    };
    mvs_ba_sparse_result res{};
    res.envelope_blocks = (int32_t)d.n_blocks, res.widest_row = widest, res.bad_frame = -1;
    bool have_bad = false;
    auto note_failure = [&]() {
        if (!have_bad && hd.status != 0) {
            have_bad = true;
            res.bad_frame = F - hd.bad_code;
        }
    };
    HIP_TRY(ctx, hipMemsetAsync(pd.state, 0, sizeof(PgdState), s));
    HIP_TRY(ctx, hipMemsetAsync(d.state, 0, sizeof(BasState), s));
    launch_bas_cost(d, 0, s);
    if ((st = read_state()) != MVS_OK)   // whatever the caller has enqueued in front (uploads, the assembly) is done by here, too
        return st;

    // the LM rule of refine_window_kernel
    double cur = hb.cost, lam = params->lambda_initial;
    const double cost0 = cur;
    const bool ok0 = std::isfinite(cur);
    int cb = 0, it = 0;
    while (ok0 && it < params->max_iterations) {
        launch_bas_build(d, cb, lam, s);
        HIP_TRY(ctx, hipMemsetAsync(pd.state, 0, sizeof(PgdState), s));
        launch_pgd_step(pd, lam, s);
        launch_bas_update(d, cb, s);
        launch_bas_cost(d, cb ^ 1, s);
        if ((st = read_state()) != MVS_OK)
            return st;
        const bool solved = hb.bad_point == 0 && hd.status == 0;
        const double cand = solved ? hb.cost : 0.0;
        const bool accepted = solved && cand <= cur;
        ++it;
        if (!solved) {
            ++res.failed_solves;
            note_failure();
        }
        if (accepted) {
            cb ^= 1;
            const double dec = 0.5 * (cur - cand);
            const bool done = dec <= params->abs_tol || dec <= params->rel_tol * (0.5 * cur);
            cur = cand;
            lam = lam / params->lambda_factor;
            if (done)
                break;
        } else {
            if (solved)
                ++res.rejected_steps;
            // a trial within the tolerances ABOVE the current error: at the minimum to rounding, stop
            const double inc = 0.5 * (cand - cur);
            if (solved && (inc <= params->abs_tol || inc <= params->rel_tol * (0.5 * cur)))
                break;
            lam = lam * params->lambda_factor;
            if (lam > params->lambda_upper)
                break;
        }
    }

    // at the estimate, lambda = 0: the factorisation decides ok, the covariances come from it
    bool ok = ok0;
    if (ok) {
        launch_bas_build(d, cb, 0.0, s);
        HIP_TRY(ctx, hipMemsetAsync(pd.state, 0, sizeof(PgdState), s));
        launch_pgd_step(pd, 0.0, s);
        if ((st = read_state()) != MVS_OK)
            return st;
        ok = hb.bad_point == 0 && hd.status == 0;
        if (!ok)
            note_failure();
    }
    res.ok = ok ? 1 : 0;
    res.iterations = it;
    res.error_initial = 0.5 * cost0;
    res.error = 0.5 * cur;
    *result = res;
    *cur_out = cb;
    return ok ? MVS_OK : MVS_NO_MODEL;
}

// the checks mvs_ba_refine_sparse and mvs_ba_sparse_obs_stats make of a problem before anything runs (the plan's limits apart)
mvs_status sparse_problem_status(const mvs_ba_sparse *pb)
{
    if (pb->n_frames < 1 || pb->n_points < 1 || pb->n_obs < 1)
        return MVS_ERR_INVALID_ARG;
    if (pb->n_frames > mvs_bas::kMaxFrames || pb->n_points > mvs_bas::kMaxPoints || pb->n_obs > mvs_bas::kMaxObs)
        return MVS_ERR_CAPACITY;
    if (!pb->K || !pb->frame_pose || !pb->frame_prior_var || !pb->points || !pb->obs_off || !pb->obs_frame || !pb->obs_uv)
        return MVS_ERR_INVALID_ARG;
    const int F = pb->n_frames, P = pb->n_points, O = pb->n_obs;
    if (!all_finite(pb->K, 9) || !affine_K(pb->K) || !all_finite(pb->frame_pose, 12 * (size_t)F) ||
        !all_finite(pb->frame_prior_var, 6 * (size_t)F) || !all_finite(pb->points, 3 * (size_t)P) ||
        (pb->point_prior_cov && !all_finite(pb->point_prior_cov, 9 * (size_t)P)) || !all_finite(pb->obs_uv, 2 * (size_t)O) ||
        (pb->obs_cov && !all_finite(pb->obs_cov, 4 * (size_t)O)))
        return MVS_ERR_INVALID_ARG;
    if (mvs_bas::check_csr(F, P, O, pb->obs_off, pb->obs_frame) != 0)
        return MVS_ERR_INVALID_ARG;
    return MVS_OK;
}
// the information matrices the kernels read of the observations: identity without covariances
void pack_obs_info(const mvs_ba_sparse *pb, std::vector<double> &oinfo)
{
    const size_t O = (size_t)pb->n_obs;
    oinfo.assign(3 * O, 0.0);
    for (size_t o = 0; o < O; ++o) {
        if (!pb->obs_cov)
            oinfo[3 * o] = 1.0, oinfo[3 * o + 2] = 1.0;
        else
            obs_cov_to_info(pb->obs_cov + 4 * o, oinfo.data() + 3 * o);
    }
}

}  // namespace

extern "C" {

mvs_status mvs_ba_refine_sparse(mvs_ctx *ctx, const mvs_ba_sparse *pb, const mvs_refine_params *params,
                                mvs_ba_sparse_result *result, double *poses_out, double *points_out, double *pose_cov_out,
                                double *point_cov_out)
{
    if (!ctx || !pb || !result || !poses_out || !refine_params_ok(params))
        return MVS_ERR_INVALID_ARG;
    mvs_status st = sparse_problem_status(pb);
    if (st != MVS_OK)
        return st;
    const int F = pb->n_frames, P = pb->n_points, O = pb->n_obs;
    const mvs_bas::Plan plan = mvs_bas::plan(F, P, O, pb->obs_off, pb->obs_frame);
    if (!plan.fits())
        return MVS_ERR_CAPACITY;
    const size_t B = (size_t)plan.blocks, NP = (size_t)plan.pairs;
    const bool want_cov = pose_cov_out || point_cov_out;

    // the uploaded doubles: weights and information matrices are derived here
    std::vector<double> w(6 * (size_t)F), pinfo(6 * (size_t)P, 0.0), oinfo;
    for (size_t k = 0; k < w.size(); ++k)
        w[k] = prior_weight(pb->frame_prior_var[k]);
    for (size_t i = 0; i < (size_t)P && pb->point_prior_cov; ++i)
        if (pb->point_prior_cov[9 * i] > 0.0)
            point_cov_to_info(pb->point_prior_cov + 9 * i, pinfo.data() + 6 * i);
    pack_obs_info(pb, oinfo);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Carve L{64};
    const size_t o_pose0 = L.take(12 * (size_t)F * 8), o_w = L.take(6 * (size_t)F * 8), o_pts0 = L.take(3 * (size_t)P * 8);
    const size_t o_pinfo = L.take(6 * (size_t)P * 8), o_uv = L.take(2 * (size_t)O * 8), o_oinfo = L.take(3 * (size_t)O * 8);
    const size_t o_ooff = L.take(((size_t)P + 1) * 4), o_ofr = L.take((size_t)O * 4), o_opt = L.take((size_t)O * 4);
    const size_t o_froff = L.take(((size_t)F + 1) * 4), o_frobs = L.take((size_t)O * 4);
    const size_t o_first = L.take((size_t)F * 4), o_row = L.take(((size_t)F + 1) * 4), o_brow = L.take(B * 4);
    const size_t o_last = L.take((size_t)F * 4), o_poff = L.take((B + 1) * 4), o_pa = L.take(NP * 4), o_pc = L.take(NP * 4);
    const BasWork wk = carve_work(L, (size_t)F, (size_t)P, (size_t)O, B, pose_cov_out != nullptr, point_cov_out != nullptr);
    if ((st = ws_grow(ctx, ctx->bas, L.total())) != MVS_OK)
        return st;
    char *base = ctx->bas.ptr();
    hipStream_t s = ctx_stream(ctx);
    auto dp = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
    auto up = [&](size_t o, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIP_TRY(ctx, up(o_pose0, pb->frame_pose, 12 * (size_t)F * 8));
    HIP_TRY(ctx, up(o_w, w.data(), w.size() * 8));
    HIP_TRY(ctx, up(o_pts0, pb->points, 3 * (size_t)P * 8));
    HIP_TRY(ctx, up(o_pinfo, pinfo.data(), pinfo.size() * 8));
    HIP_TRY(ctx, up(o_uv, pb->obs_uv, 2 * (size_t)O * 8));
    HIP_TRY(ctx, up(o_oinfo, oinfo.data(), oinfo.size() * 8));
    HIP_TRY(ctx, up(o_ooff, pb->obs_off, ((size_t)P + 1) * 4));
    HIP_TRY(ctx, up(o_ofr, pb->obs_frame, (size_t)O * 4));
    HIP_TRY(ctx, up(o_opt, plan.obs_point.data(), (size_t)O * 4));
    HIP_TRY(ctx, up(o_froff, plan.fr_off.data(), ((size_t)F + 1) * 4));
    HIP_TRY(ctx, up(o_frobs, plan.fr_obs.data(), (size_t)O * 4));
    HIP_TRY(ctx, up(o_first, plan.first.data(), (size_t)F * 4));
    HIP_TRY(ctx, up(o_row, plan.row_off.data(), ((size_t)F + 1) * 4));
    HIP_TRY(ctx, up(o_brow, plan.blk_row.data(), B * 4));
    HIP_TRY(ctx, up(o_last, plan.last.data(), (size_t)F * 4));
    HIP_TRY(ctx, up(o_poff, plan.pair_off.data(), (B + 1) * 4));
    HIP_TRY(ctx, up(o_pa, plan.pair_a.data(), NP * 4));
    HIP_TRY(ctx, up(o_pc, plan.pair_c.data(), NP * 4));

    BasDev d{};
    d.n_frames = F, d.n_points = P, d.n_obs = O, d.n_blocks = (int)B;
    d.cam[0] = pb->K[0], d.cam[1] = pb->K[1], d.cam[2] = pb->K[2], d.cam[3] = pb->K[4], d.cam[4] = pb->K[5];
    d.pose0 = dp(o_pose0), d.w = dp(o_w), d.pts0 = dp(o_pts0), d.pinfo = dp(o_pinfo);
    d.obs_off = ip(o_ooff), d.obs_frame = ip(o_ofr), d.obs_point = ip(o_opt), d.obs_uv = dp(o_uv), d.oinfo = dp(o_oinfo);
    d.fr_off = ip(o_froff), d.fr_obs = ip(o_frobs);
    d.first = ip(o_first), d.row_off = ip(o_row), d.blk_row = ip(o_brow), d.last = ip(o_last);
    d.pair_off = ip(o_poff), d.pair_a = ip(o_pa), d.pair_c = ip(o_pc);
    PgdDev pd{};
    bind_work(ctx, base, wk, d, pd);
    int cb = 0;
    // the plan's lists and the packed inputs have been read once the solver has read its first cost
    if ((st = bas_solve(ctx, d, pd, params, plan.widest, result, &cb)) != MVS_OK)
        return st;
    if (want_cov)
        launch_bas_cov(d, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(poses_out, d.pose[cb], 12 * (size_t)F * 8, hipMemcpyDeviceToHost, s));
    if (points_out)
        HIP_TRY(ctx, hipMemcpyAsync(points_out, d.pts[cb], 3 * (size_t)P * 8, hipMemcpyDeviceToHost, s));
    if (pose_cov_out)
        HIP_TRY(ctx, hipMemcpyAsync(pose_cov_out, d.pose_cov, 36 * (size_t)F * 8, hipMemcpyDeviceToHost, s));
    if (point_cov_out)
        HIP_TRY(ctx, hipMemcpyAsync(point_cov_out, d.point_cov, 9 * (size_t)P * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

// ---- per-observation statistics ------------------------------------------------------------------
mvs_status mvs_ba_sparse_obs_stats(mvs_ctx *ctx, const mvs_ba_sparse *pb, const double *poses, const double *points, double *chi2,
                                   double *weight)
{
    if (!ctx || !pb || !chi2)
        return MVS_ERR_INVALID_ARG;
    mvs_status st = sparse_problem_status(pb);
    if (st != MVS_OK)
        return st;
    const size_t F = (size_t)pb->n_frames, P = (size_t)pb->n_points, O = (size_t)pb->n_obs;
    if ((poses && !all_finite(poses, 12 * F)) || (points && !all_finite(points, 3 * P)))
        return MVS_ERR_INVALID_ARG;
    std::vector<double> oinfo;
    pack_obs_info(pb, oinfo);
    std::vector<int32_t> obs_point(O);
    for (size_t i = 0; i < P; ++i)
        for (int32_t o = pb->obs_off[i]; o < pb->obs_off[i + 1]; ++o)
            obs_point[(size_t)o] = (int32_t)i;

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Carve L{64};
    const size_t o_pose = L.take(12 * F * 8), o_pts = L.take(3 * P * 8), o_uv = L.take(2 * O * 8), o_oinfo = L.take(3 * O * 8);
    const size_t o_ofr = L.take(O * 4), o_opt = L.take(O * 4), o_chi2 = L.take(O * 8), o_wt = L.take(O * 8);
    if ((st = ws_grow(ctx, ctx->bas, L.total())) != MVS_OK)
        return st;
    char *base = ctx->bas.ptr();
    hipStream_t s = ctx_stream(ctx);
    auto dp = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
    auto up = [&](size_t o, const void *src, size_t bytes) { return hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, s); };
    HIP_TRY(ctx, up(o_pose, poses ? poses : pb->frame_pose, 12 * F * 8));
    HIP_TRY(ctx, up(o_pts, points ? points : pb->points, 3 * P * 8));
    HIP_TRY(ctx, up(o_uv, pb->obs_uv, 2 * O * 8));
    HIP_TRY(ctx, up(o_oinfo, oinfo.data(), 3 * O * 8));
    HIP_TRY(ctx, up(o_ofr, pb->obs_frame, O * 4));
    HIP_TRY(ctx, up(o_opt, obs_point.data(), O * 4));
    BasDev d{};
    d.n_frames = (int)F, d.n_points = (int)P, d.n_obs = (int)O;
    d.cam[0] = pb->K[0], d.cam[1] = pb->K[1], d.cam[2] = pb->K[2], d.cam[3] = pb->K[4], d.cam[4] = pb->K[5];
    d.obs_frame = ip(o_ofr), d.obs_point = ip(o_opt), d.obs_uv = dp(o_uv), d.oinfo = d.oinfo0 = dp(o_oinfo);
    d.loss = ctx->ba_loss, d.loss_k = ctx->ba_loss_k;
    launch_bas_obs_stats(d, dp(o_pose), dp(o_pts), dp(o_chi2), weight ? dp(o_wt) : nullptr, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(chi2, dp(o_chi2), O * 8, hipMemcpyDeviceToHost, s));
    if (weight)
        HIP_TRY(ctx, hipMemcpyAsync(weight, dp(o_wt), O * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

// ---- the global problem of a sequence that has been run -----------------------------------------
mvs_status mvs_seq_refine_global(mvs_seq *q, const mvs_seq_global_params *gp, const mvs_refine_params *params,
                                 mvs_ba_sparse_result *result)
{
    if (!q || !gp || !result || !refine_params_ok(params) || !q->ran || q->n_frames < 2 || !(gp->sigma_px > 0.0) ||
        !mvs_seqg::track_frames_ok(gp->max_track_frames))
        return MVS_ERR_INVALID_ARG;
    if (q->n_frames > mvs_bas::kMaxFrames)
        return MVS_ERR_CAPACITY;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const BatchDev &bd = q->batch->d;
    const size_t F = (size_t)q->n_frames, N = (size_t)bd.max_kp, I = sizeof(int32_t);
    q->glob_counted = q->glob_built = q->glob_solved = q->glob_cov = false;   // growing frees what an earlier call left

    // stage 1, sized by the sequence alone: the link tables, one word per keypoint for the depth, the rank, the observation
    // offset and the observation itself, and the per-frame counts and scans
    Carve A{64};
    const size_t a_succ = A.take((F - 1) * N * I), a_pred = A.take(F * N * I), a_rtp = A.take((F - 1) * N * I);
    const size_t a_depth = A.take(F * N * I), a_rank = A.take(F * N * I), a_oofs = A.take(F * N * I), a_kpo = A.take(F * N * I);
    const size_t a_frp = A.take(F * I), a_fro = A.take(F * I), a_reach = A.take(F * I), a_frq = A.take(F * 8);
    const size_t a_ptb = A.take(F * I), a_obb = A.take(F * I);
    const size_t a_first = A.take(F * I), a_row = A.take((F + 1) * I), a_last = A.take(F * I);
    const size_t a_cnt = A.take(F * I), a_froff = A.take((F + 1) * I), a_rowp = A.take(F * I), a_rowb = A.take((F + 1) * I);
    const size_t a_state = A.take(sizeof(SeqGlobState));
    mvs_status st = ws_grow(ctx, q->glob_tab, A.total());
    if (st != MVS_OK)
        return st;
    char *tab = q->glob_tab.ptr();
    auto ti = [&](size_t o) { return reinterpret_cast<int32_t *>(tab + o); };
    SeqGlobDev g{};
    g.w.n_frames = q->n_frames;
    g.w.max_kp = bd.max_kp;
    g.w.results = bd.results;
    g.w.matches = bd.matches;
    g.w.mask = bd.mask;
    g.w.points = bd.points;
    g.w.point_idx = bd.point_idx;
    g.w.kp = bd.kp1;
    g.w.oct = bd.oct1;
    g.w.K = bd.K;
    g.w.traj_R = q->chain.traj_R;
    g.w.traj_t = q->chain.traj_t;
    g.w.traj_sigma = q->chain.traj_sigma;
    g.w.succ = ti(a_succ), g.w.pred = ti(a_pred), g.w.row_to_point = ti(a_rtp);
    // frame 0 carries anchor_sigma, the others pose_sigma: variances sigma * sigma, weights as the sparse entry derives them;
    // every point the prior point_sigma^2 I, an observation the covariance (sigma_px * 2^octave)^2 I
    for (int k = 0; k < 6; ++k) {
        const double a = params->anchor_sigma[k / 3], m = params->pose_sigma[k / 3];
        g.w.w_anchor[k] = prior_weight(a * a);
        g.w.w_pose[k] = prior_weight(m * m);
    }
    const double pv = params->point_sigma * params->point_sigma;
    const double pc[9] = {pv, 0.0, 0.0, 0.0, pv, 0.0, 0.0, 0.0, pv};
    point_cov_to_info(pc, g.w.pinfo);
    for (int oc = 0; oc <= kSeqWinMaxOctave; ++oc) {
        const double sd = std::ldexp(gp->sigma_px, oc);
        const double cv[4] = {sd * sd, 0.0, 0.0, sd * sd};
        obs_cov_to_info(cv, g.w.oinfo[oc]);
    }
    g.T = gp->max_track_frames;
    g.depth = ti(a_depth), g.rank = ti(a_rank), g.oofs = ti(a_oofs), g.kp_obs = ti(a_kpo);
    g.fr_points = ti(a_frp), g.fr_nobs = ti(a_fro), g.fr_reach = ti(a_reach);
    g.fr_pairs = reinterpret_cast<int64_t *>(tab + a_frq);
    g.pt_base = ti(a_ptb), g.ob_base = ti(a_obb);
    g.first = ti(a_first), g.row_off = ti(a_row), g.last = ti(a_last);
    g.fr_cnt = ti(a_cnt), g.fr_off = ti(a_froff), g.row_pairs = ti(a_rowp), g.row_base = ti(a_rowb);
    g.state = reinterpret_cast<SeqGlobState *>(tab + a_state);
    hipStream_t s = ctx_stream(ctx);
    launch_seq_glob_count(g, s);
    HIP_TRY(ctx, hipGetLastError());
    // the one read before the LM loop: the counts, and the camera the solver takes by value
    SeqGlobState hs{};
    double K[9];
    HIP_TRY(ctx, hipMemcpyAsync(&hs, g.state, sizeof(hs), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(K, bd.K, sizeof(K), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    const mvs_seqg::Counts fit = mvs_seqg::counts_status((int64_t)F, hs.n_points, hs.n_obs, hs.blocks, hs.pairs);
    if (fit == mvs_seqg::kTooLarge)
        return MVS_ERR_CAPACITY;
    g.n_points = hs.n_points, g.n_obs = hs.n_obs, g.n_blocks = (int)hs.blocks, g.n_pairs = hs.pairs;
    q->gl = g;
    q->glob_counted = true;
    if (fit == mvs_seqg::kNoPoints) {
        mvs_ba_sparse_result none{};
        none.envelope_blocks = (int32_t)hs.blocks, none.widest_row = hs.widest, none.bad_frame = -1;
        *result = none;
        q->glob_res = none;
        return MVS_NO_MODEL;
    }

    // stage 2, sized by the counts: the problem, the plan's lists, the solver's arrays (covariances included: the sweep runs
    // when a download asks for them)
    const size_t P = (size_t)hs.n_points, O = (size_t)hs.n_obs, B = (size_t)hs.blocks, NP = (size_t)hs.pairs;
    Carve L{64};
    const size_t o_pose0 = L.take(12 * F * 8), o_w = L.take(6 * F * 8), o_pts0 = L.take(3 * P * 8), o_pinfo = L.take(6 * P * 8);
    const size_t o_uv = L.take(2 * O * 8), o_oinfo = L.take(3 * O * 8);
    const size_t o_ooff = L.take((P + 1) * I), o_hf = L.take(P * I), o_hk = L.take(P * I);
    const size_t o_ofr = L.take(O * I), o_opt = L.take(O * I), o_okp = L.take(O * I), o_frobs = L.take(O * I);
    const size_t o_brow = L.take(B * I), o_prel = L.take(B * I), o_poff = L.take((B + 1) * I);
    const size_t o_pa = L.take(NP * I), o_pc = L.take(NP * I);
    const BasWork wk = carve_work(L, F, P, O, B, true, true);
    if ((st = ws_grow(ctx, q->glob, L.total())) != MVS_OK)
        return st;
    char *base = q->glob.ptr();
    auto dp = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
    g.pose0 = dp(o_pose0), g.wts = dp(o_w), g.pts0 = dp(o_pts0), g.pinfo = dp(o_pinfo);
    g.obs_uv = dp(o_uv), g.oinfo = dp(o_oinfo);
    g.obs_off = ip(o_ooff), g.head_frame = ip(o_hf), g.head_kp = ip(o_hk);
    g.obs_frame = ip(o_ofr), g.obs_point = ip(o_opt), g.obs_kp = ip(o_okp), g.fr_obs = ip(o_frobs);
    g.blk_row = ip(o_brow), g.pair_rel = ip(o_prel), g.pair_off = ip(o_poff), g.pair_a = ip(o_pa), g.pair_c = ip(o_pc);
    HIP_TRY(ctx, hipMemsetAsync(g.kp_obs, 0xff, F * N * I, s));
    launch_seq_glob_build(g, s);
    HIP_TRY(ctx, hipGetLastError());
    q->gl = g;
    q->glob_built = true;

    BasDev d{};
    d.n_frames = (int)F, d.n_points = (int)P, d.n_obs = (int)O, d.n_blocks = (int)B;
    d.cam[0] = K[0], d.cam[1] = K[1], d.cam[2] = K[2], d.cam[3] = K[4], d.cam[4] = K[5];
    d.pose0 = g.pose0, d.w = g.wts, d.pts0 = g.pts0, d.pinfo = g.pinfo;
    d.obs_off = g.obs_off, d.obs_frame = g.obs_frame, d.obs_point = g.obs_point, d.obs_uv = g.obs_uv, d.oinfo = g.oinfo;
    d.fr_off = g.fr_off, d.fr_obs = g.fr_obs;
    d.first = g.first, d.row_off = g.row_off, d.blk_row = g.blk_row, d.last = g.last;
    d.pair_off = g.pair_off, d.pair_a = g.pair_a, d.pair_c = g.pair_c;
    PgdDev pd{};
    bind_work(ctx, base, wk, d, pd);
    int cb = 0;
    st = bas_solve(ctx, d, pd, params, hs.widest, result, &cb);
    if (st != MVS_OK && st != MVS_NO_MODEL)
        return st;
    q->glob_bas = d;
    q->glob_cur = cb;
    q->glob_res = *result;
    q->glob_solved = true;
    return st;
}

mvs_status mvs_seq_global_counts(mvs_seq *q, int32_t *n_points, int32_t *n_obs)
{
    if (!q || !q->glob_counted)
        return MVS_ERR_INVALID_ARG;
    if (n_points)
        *n_points = q->gl.n_points;
    if (n_obs)
        *n_obs = q->gl.n_obs;
    return MVS_OK;
}

mvs_status mvs_seq_download_global(mvs_seq *q, double *poses, double *points, double *pose_cov, double *point_cov)
{
    if (!q || !q->glob_counted)
        return MVS_ERR_INVALID_ARG;
    if (!q->glob_solved || !q->glob_res.ok)
        return MVS_NO_MODEL;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const BasDev &d = q->glob_bas;
    const size_t F = (size_t)d.n_frames, P = (size_t)d.n_points;
    hipStream_t s = ctx_stream(ctx);
    if ((pose_cov || point_cov) && !q->glob_cov) {   // the sweep continues from the factorisation the solver ended on
        launch_bas_cov(d, s);
        HIP_TRY(ctx, hipGetLastError());
        q->glob_cov = true;
    }
    if (poses)
        HIP_TRY(ctx, hipMemcpyAsync(poses, d.pose[q->glob_cur], 12 * F * 8, hipMemcpyDeviceToHost, s));
    if (points)
        HIP_TRY(ctx, hipMemcpyAsync(points, d.pts[q->glob_cur], 3 * P * 8, hipMemcpyDeviceToHost, s));
    if (pose_cov)
        HIP_TRY(ctx, hipMemcpyAsync(pose_cov, d.pose_cov, 36 * F * 8, hipMemcpyDeviceToHost, s));
    if (point_cov)
        HIP_TRY(ctx, hipMemcpyAsync(point_cov, d.point_cov, 9 * P * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_global_obs_stats(mvs_seq *q, double *chi2, double *weight)
{
    if (!q || !chi2 || !q->glob_solved || !q->glob_res.ok)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the resident problem at the resident estimate under the context's loss as it is NOW; zd, which nothing reads behind the
    // solver's last update, takes the two result arrays
    BasDev d = q->glob_bas;
    d.loss = ctx->ba_loss, d.loss_k = ctx->ba_loss_k;
    const size_t O = (size_t)d.n_obs;
    hipStream_t s = ctx_stream(ctx);
    double *d_chi2 = d.zd, *d_wt = d.zd + O;
    launch_bas_obs_stats(d, d.pose[q->glob_cur], d.pts[q->glob_cur], d_chi2, weight ? d_wt : nullptr, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(chi2, d_chi2, O * 8, hipMemcpyDeviceToHost, s));
    if (weight)
        HIP_TRY(ctx, hipMemcpyAsync(weight, d_wt, O * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

mvs_status mvs_seq_download_global_problem(mvs_seq *q, int32_t *obs_off, int32_t *obs_frame, int32_t *obs_kp, int32_t *head_frame,
                                           int32_t *head_kp, double *point_guess, double *obs_uv)
{
    if (!q || !q->glob_built)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SeqGlobDev &g = q->gl;
    const size_t P = (size_t)g.n_points, O = (size_t)g.n_obs, I = sizeof(int32_t);
    hipStream_t s = ctx_stream(ctx);
    auto get = [&](void *dst, const void *src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    HIP_TRY(ctx, get(obs_off, g.obs_off, (P + 1) * I));
    HIP_TRY(ctx, get(obs_frame, g.obs_frame, O * I));
    HIP_TRY(ctx, get(obs_kp, g.obs_kp, O * I));
    HIP_TRY(ctx, get(head_frame, g.head_frame, P * I));
    HIP_TRY(ctx, get(head_kp, g.head_kp, P * I));
    HIP_TRY(ctx, get(point_guess, g.pts0, 3 * P * 8));
    HIP_TRY(ctx, get(obs_uv, g.obs_uv, 2 * O * 8));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

}  // extern "C"
