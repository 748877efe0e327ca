// capi_ba.hip -- the host side of mvs_ba_refine_sparse (include/mvslam_hip.h): argument checks, the
// plan of ba_envelope.hpp, one workspace of the context, and the LM loop of refine_window_kernel driven from here -- the device
// computes (ba_sparse.hip, pg_direct.hip), the host decides, one synchronisation per iteration.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ba_envelope.hpp"
#include "capi_internal.hpp"

using namespace mvs_host;

namespace {

constexpr double kPivotTol = 1.0 / (double)(1ll << 42);   // refine.hip's kWinPivotTol

bool all_finite(const double *v, size_t n)
{
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(v[k]))
            return false;
    return true;
}

// capi.hip's obs_cov_to_info / point_cov_to_info (same statements)
void obs_info(const double *cv, double *o)
{
    const double a = cv[0], b = 0.5 * (cv[1] + cv[2]), dd = cv[3];
    const double id = 1.0 / (a * dd - b * b);
    o[0] = dd * id, o[1] = -(b * id), o[2] = a * id;
}
void point_info(const double *C, double *L)
{
    const double a[6] = {C[0], 0.5 * (C[1] + C[3]), 0.5 * (C[2] + C[6]), C[4], 0.5 * (C[5] + C[7]), C[8]};
    const double c00 = a[3] * a[5] - a[4] * a[4], c01 = a[2] * a[4] - a[1] * a[5], c02 = a[1] * a[4] - a[2] * a[3];
    const double id = 1.0 / ((a[0] * c00 + a[1] * c01) + a[2] * c02);
    L[0] = c00 * id, L[1] = c01 * id, L[2] = c02 * id;
    L[3] = (a[0] * a[5] - a[2] * a[2]) * id, L[4] = (a[1] * a[2] - a[0] * a[4]) * id, L[5] = (a[0] * a[3] - a[1] * a[1]) * id;
}

}  // namespace

extern "C" {

mvs_status mvs_ba_refine_sparse(mvs_ctx *ctx, const mvs_ba_sparse *pb, const mvs_refine_params *params,
                                mvs_ba_sparse_result *result, double *poses_out, double *points_out, double *pose_cov_out,
                                double *point_cov_out)
{
    if (!ctx || !pb || !result || !poses_out || !refine_params_ok(params))
        return MVS_ERR_INVALID_ARG;
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
    const mvs_bas::Plan plan = mvs_bas::plan(F, P, O, pb->obs_off, pb->obs_frame);
    if (!plan.fits())
        return MVS_ERR_CAPACITY;
    const size_t B = (size_t)plan.blocks, NP = (size_t)plan.pairs;
    const bool want_cov = pose_cov_out || point_cov_out;

    // the uploaded doubles: weights and information matrices are derived here
    std::vector<double> w(6 * (size_t)F), pinfo(6 * (size_t)P, 0.0), oinfo(3 * (size_t)O, 0.0);
    for (size_t k = 0; k < w.size(); ++k)
        w[k] = pb->frame_prior_var[k] > 0.0 ? 1.0 / pb->frame_prior_var[k] : 0.0;
    for (size_t i = 0; i < (size_t)P && pb->point_prior_cov; ++i)
        if (pb->point_prior_cov[9 * i] > 0.0)
            point_info(pb->point_prior_cov + 9 * i, pinfo.data() + 6 * i);
    for (size_t o = 0; o < (size_t)O; ++o) {
        if (!pb->obs_cov)
            oinfo[3 * o] = 1.0, oinfo[3 * o + 2] = 1.0;
        else
            obs_info(pb->obs_cov + 4 * o, oinfo.data() + 3 * o);
    }

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n_terms = (int64_t)O + P + F;
    const size_t chunks = (size_t)((n_terms + kBasRedChunk - 1) / kBasRedChunk);
    Carve L{64};
    const size_t o_pose0 = L.take(12 * (size_t)F * 8), o_w = L.take(6 * (size_t)F * 8), o_pts0 = L.take(3 * (size_t)P * 8);
    const size_t o_pinfo = L.take(6 * (size_t)P * 8), o_uv = L.take(2 * (size_t)O * 8), o_oinfo = L.take(3 * (size_t)O * 8);
    const size_t o_ooff = L.take(((size_t)P + 1) * 4), o_ofr = L.take((size_t)O * 4), o_opt = L.take((size_t)O * 4);
    const size_t o_froff = L.take(((size_t)F + 1) * 4), o_frobs = L.take((size_t)O * 4);
    const size_t o_first = L.take((size_t)F * 4), o_row = L.take(((size_t)F + 1) * 4), o_brow = L.take(B * 4);
    const size_t o_last = L.take((size_t)F * 4), o_poff = L.take((B + 1) * 4), o_pa = L.take(NP * 4), o_pc = L.take(NP * 4);
    const size_t o_pose[2] = {L.take(12 * (size_t)F * 8), L.take(12 * (size_t)F * 8)};
    const size_t o_pts[2] = {L.take(3 * (size_t)P * 8), L.take(3 * (size_t)P * 8)};
    const size_t o_lin = L.take((size_t)kBasLin * O * 8), o_Li = L.take(6 * (size_t)P * 8), o_gh = L.take(3 * (size_t)P * 8);
    const size_t o_Z = L.take(18 * (size_t)O * 8), o_zd = L.take(3 * (size_t)O * 8);
    const size_t o_prior = L.take(27 * (size_t)F * 8);
    const size_t o_D = L.take(21 * (size_t)F * 8), o_g = L.take(6 * (size_t)F * 8), o_sky = L.take(36 * B * 8);
    const size_t o_Cinv = L.take(21 * (size_t)F * 8), o_y = L.take(6 * (size_t)F * 8), o_x = L.take(6 * (size_t)F * 8);
    const size_t o_terms = L.take((size_t)n_terms * 8), o_part = L.take(chunks * 8);
    const size_t o_pst = L.take(sizeof(PgdState)), o_bst = L.take(sizeof(BasState));
    const size_t o_inv = L.take(want_cov ? 36 * B * 8 : 0), o_colm = L.take(want_cov ? 36 * (size_t)F * 8 : 0);
    const size_t o_pcov = L.take(pose_cov_out ? 36 * (size_t)F * 8 : 0), o_ptcov = L.take(point_cov_out ? 9 * (size_t)P * 8 : 0);
    mvs_status st = ws_grow(ctx, ctx->bas, L.total());
    if (st != MVS_OK)
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
    HIP_TRY(ctx, hipMemcpyAsync(base + o_pose[0], base + o_pose0, 12 * (size_t)F * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_pts[0], base + o_pts0, 3 * (size_t)P * 8, hipMemcpyDeviceToDevice, s));

    BasDev d{};
    d.n_frames = F, d.n_points = P, d.n_obs = O, d.n_blocks = (int)B;
    d.cam[0] = pb->K[0], d.cam[1] = pb->K[1], d.cam[2] = pb->K[2], d.cam[3] = pb->K[4], d.cam[4] = pb->K[5];
    d.pose0 = dp(o_pose0), d.w = dp(o_w), d.pts0 = dp(o_pts0), d.pinfo = dp(o_pinfo);
    d.obs_off = ip(o_ooff), d.obs_frame = ip(o_ofr), d.obs_point = ip(o_opt), d.obs_uv = dp(o_uv), d.oinfo = dp(o_oinfo);
    d.fr_off = ip(o_froff), d.fr_obs = ip(o_frobs);
    d.first = ip(o_first), d.row_off = ip(o_row), d.blk_row = ip(o_brow), d.last = ip(o_last);
    d.pair_off = ip(o_poff), d.pair_a = ip(o_pa), d.pair_c = ip(o_pc);
    d.pose[0] = dp(o_pose[0]), d.pose[1] = dp(o_pose[1]), d.pts[0] = dp(o_pts[0]), d.pts[1] = dp(o_pts[1]);
    d.lin = dp(o_lin), d.Li = dp(o_Li), d.gh = dp(o_gh), d.Z = dp(o_Z), d.zd = dp(o_zd), d.D = dp(o_D), d.g = dp(o_g);
    d.prior = dp(o_prior);
    d.sky = dp(o_sky), d.Cinv = dp(o_Cinv), d.x = dp(o_x), d.terms = dp(o_terms), d.partial = dp(o_part);
    d.inv = want_cov ? dp(o_inv) : nullptr, d.colm = want_cov ? dp(o_colm) : nullptr;
    d.pose_cov = pose_cov_out ? dp(o_pcov) : nullptr, d.point_cov = point_cov_out ? dp(o_ptcov) : nullptr;
    d.state = reinterpret_cast<BasState *>(base + o_bst);
    // the step: pg_direct.hip's kernels on their second source
    PgdDev pd{};
    pd.n_nodes = F, pd.n_blocks = (int)B;
    pd.first = d.first, pd.row_off = d.row_off, pd.blk_row = d.blk_row;
    pd.D = d.D, pd.g = d.g, pd.Cinv = dp(o_Cinv), pd.sky = d.sky, pd.y = dp(o_y), pd.x = dp(o_x);
    pd.state = reinterpret_cast<PgdState *>(base + o_pst);
    pd.pre = d.sky, pd.pivot_tol = kPivotTol;

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
    res.envelope_blocks = (int32_t)plan.blocks, res.widest_row = plan.widest, res.bad_frame = -1;
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
    if ((st = read_state()) != MVS_OK)   // the plan's lists and the packed inputs have been read by here, too
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
    if (!ok)
        return MVS_NO_MODEL;
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

}  // extern "C"
