// ba_sparse.hip -- bundle adjustment of up to 4096 frames fed as a sparse problem (mvs_ba_refine_sparse; DESIGN.md section
// 4.7.4).  The cost, the tangent order and the pivot rule are refine_window_kernel's (refine.hip); the work is laid out for
// problems that no workgroup holds:
//   bas_lin_kernel       one thread per observation: residual and Jacobians (Jc 2 x 6, Jp 2 x 3) at the current values.
//   bas_point_kernel     one thread per point: V = prior + sum Jp^T W Jp (+ lambda) and g_p over its observations in ascending
//                        order -- nine values per observation is all a long track serialises --, V = L L^T with the pivot
//                        rule, L^-1 and L^-1 g_p.
//   bas_z_kernel         one thread per observation: Z_o = Jc^T W Jp L^-T (6 x 3).
//   bas_prior_kernel     one thread per frame: the pose prior's share of Hcc_f and g_f.
//   bas_frame_kernel     one thread per entry of {Hcc_f (21), g_f (6)}: sum over the frame's observations in ascending index
//                        (the host's CSR by frame), the prior, minus the frame's own Schur terms Z_o Z_o^T / Z_o L^-1 g_p.
//   bas_schur_kernel     one thread per entry of every off-diagonal block of the envelope: -sum Z_a Z_c^T over the host's
//                        pair list of the block, in point order.
//   (pg_direct.hip's four kernels: scaling, assembly from `pre`, factorisation, back substitution -- launch_pgd_step)
//   bas_zd_kernel        one thread per observation: Z_o^T delta_f.
//   bas_update_kernel    one thread per point (delta_p = -L^-T (L^-1 g_p + sum Z_o^T delta_f), ascending) or per frame (the
//                        retraction).
//   bas_terms_kernel     one thread per cost term (observations, point priors, pose priors), then bas_reduce_kernel twice:
//                        chunks of 4096 terms in a fixed order, then the chunks' sums in a fixed order.
//   covariances at the estimate: bas_selinv_kernel (ONE workgroup: the blocks of the scaled S^-1 inside the envelope by the
//   selected-inversion recurrence, columns in descending order), bas_pose_cov_kernel, bas_zs_kernel, bas_y_kernel,
//   bas_point_cov_kernel.
//   robust losses (mvs_ctx_set_ba_loss) enter through three kernels of their own and nothing else:
//   bas_robust_lin_kernel (bas_lin_kernel's statements, plus w(s_o) W_o into the array BasDev::oinfo then points at),
//   bas_robust_terms_kernel (bas_terms_kernel's, with rho2(s_o) for an observation's term) and bas_obs_stats_kernel (s_o and
//   w(s_o) at given values).  Every other kernel reads what those left; without a loss the launches are the ones they were.
// One owner per entry everywhere, no floating-point atomics, binary64 with explicit FMAs: the same input gives the same bytes.
//
// The projection, the pose prior, the 3 x 3 Cholesky of bas_point_kernel and the loss functions are lm_math.hpp's, shared with refine.hip.
#include "lm_math.hpp"

namespace mvs {

namespace {

constexpr int kBasThreads = 256;
constexpr int kBasPerWg = 7;   // blocks of the envelope one workgroup of bas_schur_kernel owns: 7 * 36 = 252 threads

__device__ __forceinline__ Cam cam_of(const BasDev &d)
{
    Cam cam;
    cam.fx = d.cam[0], cam.sk = d.cam[1], cam.cx = d.cam[2], cam.fy = d.cam[3], cam.cy = d.cam[4];
    return cam;
}

__device__ __forceinline__ void load_pose(const double *pose, int f, double (&R)[9], double (&t)[3])
{
    const double *q = pose + 12 * (int64_t)f;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        R[k] = q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        t[k] = q[9 + k];
}

// row r of the symmetric 6 x 6 block e = lidx(a, b): the pair (a, b), a >= b
__device__ __forceinline__ void unpack21(int e, int &a, int &b)
{
    a = 0;
    while ((a + 1) * (a + 2) / 2 <= e)
        ++a;
    b = e - a * (a + 1) / 2;
}

// ---- linearisation ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBasThreads) void bas_lin_kernel(BasDev d, int cur)
{
    const int o = blockIdx.x * kBasThreads + threadIdx.x;
    if (o >= d.n_obs)
        return;
    if (o == 0)
        d.state->bad_point = 0;   // bas_point_kernel, the next launch, sets it
    const Cam cam = cam_of(d);
    double R[9], t[3], p[3], r[2], Jc[12], Jp[6];
    load_pose(d.pose[cur], d.obs_frame[o], R, t);
    const double *pp = d.pts[cur] + 3 * (int64_t)d.obs_point[o];
    p[0] = pp[0], p[1] = pp[1], p[2] = pp[2];
    project_lin<true>(cam, R, t, p, d.obs_uv[2 * (int64_t)o], d.obs_uv[2 * (int64_t)o + 1], r, Jc, Jp);
    double *L = d.lin + (int64_t)kBasLin * o;
#pragma unroll
    for (int k = 0; k < 12; ++k)
        L[k] = Jc[k];
#pragma unroll
    for (int k = 0; k < 6; ++k)
        L[12 + k] = Jp[k];
    L[18] = r[0];
    L[19] = r[1];
}

__global__ __launch_bounds__(kBasThreads) void bas_point_kernel(BasDev d, int cur, double lam)
{
    const int i = blockIdx.x * kBasThreads + threadIdx.x;
    if (i >= d.n_points)
        return;
    double Hpp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gp[3] = {0.0, 0.0, 0.0};
    for (int o = d.obs_off[i]; o < d.obs_off[i + 1]; ++o) {
        const double *L = d.lin + (int64_t)kBasLin * o, *Jp = L + 12;
        const double W0 = d.oinfo[3 * (int64_t)o], W1 = d.oinfo[3 * (int64_t)o + 1], W2 = d.oinfo[3 * (int64_t)o + 2];
        const double r0 = L[18], r1 = L[19];
        const double wr0 = fd2(W0, r0, W1, r1), wr1 = fd2(W1, r0, W2, r1);
        double WJp[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            WJp[k] = fd2(W0, Jp[k], W1, Jp[3 + k]);
            WJp[3 + k] = fd2(W1, Jp[k], W2, Jp[3 + k]);
        }
        Hpp[0] = Hpp[0] + fd2(Jp[0], WJp[0], Jp[3], WJp[3]);
        Hpp[1] = Hpp[1] + fd2(Jp[0], WJp[1], Jp[3], WJp[4]);
        Hpp[2] = Hpp[2] + fd2(Jp[0], WJp[2], Jp[3], WJp[5]);
        Hpp[3] = Hpp[3] + fd2(Jp[1], WJp[1], Jp[4], WJp[4]);
        Hpp[4] = Hpp[4] + fd2(Jp[1], WJp[2], Jp[4], WJp[5]);
        Hpp[5] = Hpp[5] + fd2(Jp[2], WJp[2], Jp[5], WJp[5]);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            gp[k] = gp[k] + fd2(Jp[k], wr0, Jp[3 + k], wr1);
    }
    const double *p = d.pts[cur] + 3 * (int64_t)i, *p0 = d.pts0 + 3 * (int64_t)i, *L = d.pinfo + 6 * (int64_t)i;
    const double d0 = p[0] - p0[0], d1 = p[1] - p0[1], d2 = p[2] - p0[2];
    double V[6];
#pragma unroll
    for (int k = 0; k < 6; ++k)
        V[k] = L[k] + Hpp[k];
    const double g0 = fd3(L[0], d0, L[1], d1, L[2], d2) + gp[0];
    const double g1 = fd3(L[1], d0, L[3], d1, L[4], d2) + gp[1];
    const double g2 = fd3(L[2], d0, L[4], d1, L[5], d2) + gp[2];
    const double v0 = V[0] + lam, v3 = V[3] + lam, v5 = V[5] + lam;
    // V = L L^T, then L^-1
    double Li[6];
    const bool ok = chol3_pivot(V, v0, v3, v5, Li);
    double gh[3];
    gh[0] = Li[0] * g0;
    gh[1] = fd2(Li[1], g0, Li[2], g1);
    gh[2] = fd3(Li[3], g0, Li[4], g1, Li[5], g2);
    if (!ok) {
        gh[0] = gh[1] = gh[2] = 0.0;
        d.state->bad_point = 1;   // every writer stores the same word
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        d.Li[6 * (int64_t)i + k] = Li[k];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        d.gh[3 * (int64_t)i + k] = gh[k];
}

__global__ __launch_bounds__(kBasThreads) void bas_z_kernel(BasDev d)
{
    const int o = blockIdx.x * kBasThreads + threadIdx.x;
    if (o >= d.n_obs)
        return;
    const double *L = d.lin + (int64_t)kBasLin * o, *Jp = L + 12, *Li = d.Li + 6 * (int64_t)d.obs_point[o];
    const double W0 = d.oinfo[3 * (int64_t)o], W1 = d.oinfo[3 * (int64_t)o + 1], W2 = d.oinfo[3 * (int64_t)o + 2];
    double WJp[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        WJp[k] = fd2(W0, Jp[k], W1, Jp[3 + k]);
        WJp[3 + k] = fd2(W1, Jp[k], W2, Jp[3 + k]);
    }
    double *Z = d.Z + 18 * (int64_t)o;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const double h0 = fd2(L[a], WJp[0], L[6 + a], WJp[3]), h1 = fd2(L[a], WJp[1], L[6 + a], WJp[4]),
                     h2 = fd2(L[a], WJp[2], L[6 + a], WJp[5]);
        Z[3 * a] = h0 * Li[0];
        Z[3 * a + 1] = fd2(h0, Li[1], h1, Li[2]);
        Z[3 * a + 2] = fd3(h0, Li[3], h1, Li[4], h2, Li[5]);
    }
}

// ---- the reduced camera system ----------------------------------------------------------------------------------------------
// the prior's share of {Hcc_f (21, packed lower), g_f (6)}: one thread per frame, refine_window_kernel's statements
__global__ __launch_bounds__(64) void bas_prior_kernel(BasDev d, int cur)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= d.n_frames)
        return;
    double R0[9], t0[3], R[9], t[3], e[6], Jw[9], Jv[9], w[6];
    load_pose(d.pose0, f, R0, t0);
    load_pose(d.pose[cur], f, R, t);
#pragma unroll
    for (int k = 0; k < 6; ++k)
        w[k] = d.w[6 * (int64_t)f + k];
    pose_prior<true>(R0, t0, R, t, e, Jw, Jv);
    double *out = d.prior + 27 * (int64_t)f;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const int half = a / 3, a3 = a % 3;
        const double *J = half ? Jv : Jw;
        const double w0 = w[3 * half], w1 = w[3 * half + 1], w2 = w[3 * half + 2];
#pragma unroll
        for (int c = 0; c <= a; ++c) {
            double h = 0.0;
            if (c / 3 == half) {
                const int c3 = c % 3;
                h = (J[a3] * w0 * J[c3] + J[3 + a3] * w1 * J[3 + c3]) + J[6 + a3] * w2 * J[6 + c3];
            }
            out[lidx(a, c)] = h;
        }
        out[21 + a] = (J[a3] * w0 * e[3 * half] + J[3 + a3] * w1 * e[3 * half + 1]) + J[6 + a3] * w2 * e[3 * half + 2];
    }
}

__global__ __launch_bounds__(kBasThreads) void bas_frame_kernel(BasDev d, int cur)
{
    const int gid = blockIdx.x * kBasThreads + threadIdx.x;
    const int f = gid / 27, e = gid - 27 * f;
    if (f >= d.n_frames)
        return;
    int a, b;
    if (e < 21)
        unpack21(e, a, b);
    else
        a = e - 21, b = 0;
    double accH = 0.0, accZ = 0.0;
    for (int k = d.fr_off[f]; k < d.fr_off[f + 1]; ++k) {
        const int o = d.fr_obs[k];
        const double *Jc = d.lin + (int64_t)kBasLin * o, *Z = d.Z + 18 * (int64_t)o;
        const double W0 = d.oinfo[3 * (int64_t)o], W1 = d.oinfo[3 * (int64_t)o + 1], W2 = d.oinfo[3 * (int64_t)o + 2];
        if (e < 21) {
            const double w0 = fd2(W0, Jc[b], W1, Jc[6 + b]), w1 = fd2(W1, Jc[b], W2, Jc[6 + b]);
            accH = accH + fd2(Jc[a], w0, Jc[6 + a], w1);
            accZ = fma(Z[3 * a + 2], Z[3 * b + 2], fma(Z[3 * a + 1], Z[3 * b + 1], fma(Z[3 * a], Z[3 * b], accZ)));
        } else {
            const double r0 = Jc[18], r1 = Jc[19];
            const double wr0 = fd2(W0, r0, W1, r1), wr1 = fd2(W1, r0, W2, r1);
            accH = accH + fd2(Jc[a], wr0, Jc[6 + a], wr1);
            const double *gh = d.gh + 3 * (int64_t)d.obs_point[o];
            accZ = fma(Z[3 * a + 2], gh[2], fma(Z[3 * a + 1], gh[1], fma(Z[3 * a], gh[0], accZ)));
        }
    }
    // the frame's prior (bas_prior_kernel)
    const double pr = d.prior[27 * (int64_t)f + e];
    if (e < 21)
        d.D[21 * (int64_t)f + e] = (accH + pr) - accZ;
    else
        d.g[6 * (int64_t)f + a] = (accH + pr) - accZ;
}

__global__ __launch_bounds__(kBasThreads) void bas_schur_kernel(BasDev d)
{
    const int tid = threadIdx.x, lb = tid / 36, e = tid - 36 * lb, a = e / 6, c = e - 6 * a;
    const int64_t b = (int64_t)blockIdx.x * kBasPerWg + lb;
    if (lb >= kBasPerWg || b >= d.n_blocks)
        return;
    double acc = 0.0;
    for (int t = d.pair_off[b]; t < d.pair_off[b + 1]; ++t) {
        const double *Za = d.Z + 18 * (int64_t)d.pair_a[t] + 3 * a, *Zc = d.Z + 18 * (int64_t)d.pair_c[t] + 3 * c;
        acc = fma(Za[2], Zc[2], fma(Za[1], Zc[1], fma(Za[0], Zc[0], acc)));
    }
    d.sky[36 * b + e] = 0.0 - acc;   // a diagonal block (no pairs) is written by the step's assembly
}

// ---- update and cost ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBasThreads) void bas_zd_kernel(BasDev d)
{
    const int o = blockIdx.x * kBasThreads + threadIdx.x;
    if (o >= d.n_obs)
        return;
    const double *Z = d.Z + 18 * (int64_t)o, *dc = d.x + 6 * (int64_t)d.obs_frame[o];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double x = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
            x = fma(Z[3 * a + k], dc[a], x);
        d.zd[3 * (int64_t)o + k] = x;
    }
}

__global__ __launch_bounds__(kBasThreads) void bas_update_kernel(BasDev d, int cur)
{
    const int gid = blockIdx.x * kBasThreads + threadIdx.x;
    if (gid < d.n_points) {
        const int i = gid;
        const double *gh = d.gh + 3 * (int64_t)i, *Li = d.Li + 6 * (int64_t)i, *p = d.pts[cur] + 3 * (int64_t)i;
        double s[3] = {0.0, 0.0, 0.0};
        for (int o = d.obs_off[i]; o < d.obs_off[i + 1]; ++o)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                s[k] = s[k] + d.zd[3 * (int64_t)o + k];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            s[k] = gh[k] + s[k];
        const double dp[3] = {fd3(Li[0], s[0], Li[1], s[1], Li[3], s[2]), fd2(Li[2], s[1], Li[4], s[2]), Li[5] * s[2]};
        double *q = d.pts[cur ^ 1] + 3 * (int64_t)i;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = p[k] - dp[k];
        return;
    }
    const int f = gid - d.n_points;
    if (f >= d.n_frames)
        return;
    const double *dl = d.x + 6 * (int64_t)f, *Rc = d.pose[cur] + 12 * (int64_t)f;
    double *out = d.pose[cur ^ 1] + 12 * (int64_t)f;
    const double dw[3] = {dl[0], dl[1], dl[2]};
    double E[9];
    so3_exp(dw, E);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[3 * r + c] = (Rc[3 * r] * E[c] + Rc[3 * r + 1] * E[3 + c]) + Rc[3 * r + 2] * E[6 + c];
        out[9 + r] = Rc[9 + r] + ((Rc[3 * r] * dl[3] + Rc[3 * r + 1] * dl[4]) + Rc[3 * r + 2] * dl[5]);
    }
}

__global__ __launch_bounds__(kBasThreads) void bas_terms_kernel(BasDev d, int which)
{
    const int64_t gid = (int64_t)blockIdx.x * kBasThreads + threadIdx.x;
    const int64_t n = (int64_t)d.n_obs + d.n_points + d.n_frames;
    if (gid >= n)
        return;
    double c = 0.0;
    if (gid < d.n_obs) {
        const int o = (int)gid;
        const Cam cam = cam_of(d);
        double R[9], t[3], p[3], r[2], Jc[12], Jp[6];
        load_pose(d.pose[which], d.obs_frame[o], R, t);
        const double *pp = d.pts[which] + 3 * (int64_t)d.obs_point[o];
        p[0] = pp[0], p[1] = pp[1], p[2] = pp[2];
        project_lin<false>(cam, R, t, p, d.obs_uv[2 * (int64_t)o], d.obs_uv[2 * (int64_t)o + 1], r, Jc, Jp);
        const double W0 = d.oinfo[3 * (int64_t)o], W1 = d.oinfo[3 * (int64_t)o + 1], W2 = d.oinfo[3 * (int64_t)o + 2];
        const double wr0 = fd2(W0, r[0], W1, r[1]), wr1 = fd2(W1, r[0], W2, r[1]);
        c = fma(r[1], wr1, r[0] * wr0);
    } else if (gid < (int64_t)d.n_obs + d.n_points) {
        const int64_t i = gid - d.n_obs;
        const double *p = d.pts[which] + 3 * i, *p0 = d.pts0 + 3 * i, *L = d.pinfo + 6 * i;
        const double d0 = p[0] - p0[0], d1 = p[1] - p0[1], d2 = p[2] - p0[2];
        c = fd3(d0, fd3(L[0], d0, L[1], d1, L[2], d2), d1, fd3(L[1], d0, L[3], d1, L[4], d2), d2,
                fd3(L[2], d0, L[4], d1, L[5], d2));
    } else {
        const int f = (int)(gid - d.n_obs - d.n_points);
        double R0[9], t0[3], R[9], t[3], e[6], Jw[9], Jv[9];
        load_pose(d.pose0, f, R0, t0);
        load_pose(d.pose[which], f, R, t);
        pose_prior<false>(R0, t0, R, t, e, Jw, Jv);
#pragma unroll
        for (int k = 0; k < 6; ++k)
            c = c + (e[k] * e[k]) * d.w[6 * (int64_t)f + k];
    }
    d.terms[gid] = c;
}

// ---- robust losses (mvs_ctx_set_ba_loss) -----------------------------------------------------------
// s = r^T W r of one observation: bas_terms_kernel's statements
__device__ __forceinline__ double obs_chi2(const double (&r)[2], double W0, double W1, double W2)
{
    const double wr0 = fd2(W0, r[0], W1, r[1]), wr1 = fd2(W1, r[0], W2, r[1]);
    return fma(r[1], wr1, r[0] * wr0);
}

// bas_lin_kernel under a loss: the same 20 doubles of lin, and w(s_o) W_o for the build kernels
__global__ __launch_bounds__(kBasThreads) void bas_robust_lin_kernel(BasDev d, int cur)
{
    const int o = blockIdx.x * kBasThreads + threadIdx.x;
    if (o >= d.n_obs)
        return;
    if (o == 0)
        d.state->bad_point = 0;   // bas_point_kernel, the next launch, sets it
    const Cam cam = cam_of(d);
    double R[9], t[3], p[3], r[2], Jc[12], Jp[6];
    load_pose(d.pose[cur], d.obs_frame[o], R, t);
    const double *pp = d.pts[cur] + 3 * (int64_t)d.obs_point[o];
    p[0] = pp[0], p[1] = pp[1], p[2] = pp[2];
    project_lin<true>(cam, R, t, p, d.obs_uv[2 * (int64_t)o], d.obs_uv[2 * (int64_t)o + 1], r, Jc, Jp);
    double *L = d.lin + (int64_t)kBasLin * o;
#pragma unroll
    for (int k = 0; k < 12; ++k)
        L[k] = Jc[k];
#pragma unroll
    for (int k = 0; k < 6; ++k)
        L[12 + k] = Jp[k];
    L[18] = r[0];
    L[19] = r[1];
    const double W0 = d.oinfo0[3 * (int64_t)o], W1 = d.oinfo0[3 * (int64_t)o + 1], W2 = d.oinfo0[3 * (int64_t)o + 2];
    const double s = obs_chi2(r, W0, W1, W2);
    const double w = loss_weight(d.loss, d.loss_k, s, sqrt(s));
    double *Ww = d.oinfo_w + 3 * (int64_t)o;
    Ww[0] = w * W0;
    Ww[1] = w * W1;
    Ww[2] = w * W2;
}

// bas_terms_kernel under a loss: rho2(s_o) for an observation, the priors as they are
__global__ __launch_bounds__(kBasThreads) void bas_robust_terms_kernel(BasDev d, int which)
{
    const int64_t gid = (int64_t)blockIdx.x * kBasThreads + threadIdx.x;
    const int64_t n = (int64_t)d.n_obs + d.n_points + d.n_frames;
    if (gid >= n)
        return;
    double c = 0.0;
    if (gid < d.n_obs) {
        const int o = (int)gid;
        const Cam cam = cam_of(d);
        double R[9], t[3], p[3], r[2], Jc[12], Jp[6];
        load_pose(d.pose[which], d.obs_frame[o], R, t);
        const double *pp = d.pts[which] + 3 * (int64_t)d.obs_point[o];
        p[0] = pp[0], p[1] = pp[1], p[2] = pp[2];
        project_lin<false>(cam, R, t, p, d.obs_uv[2 * (int64_t)o], d.obs_uv[2 * (int64_t)o + 1], r, Jc, Jp);
        const double W0 = d.oinfo0[3 * (int64_t)o], W1 = d.oinfo0[3 * (int64_t)o + 1], W2 = d.oinfo0[3 * (int64_t)o + 2];
        const double s = obs_chi2(r, W0, W1, W2);
        c = ba_loss_rho2(d.loss, d.loss_k, s, sqrt(s));
    } else if (gid < (int64_t)d.n_obs + d.n_points) {
        const int64_t i = gid - d.n_obs;
        const double *p = d.pts[which] + 3 * i, *p0 = d.pts0 + 3 * i, *L = d.pinfo + 6 * i;
        const double d0 = p[0] - p0[0], d1 = p[1] - p0[1], d2 = p[2] - p0[2];
        c = fd3(d0, fd3(L[0], d0, L[1], d1, L[2], d2), d1, fd3(L[1], d0, L[3], d1, L[4], d2), d2,
                fd3(L[2], d0, L[4], d1, L[5], d2));
    } else {
        const int f = (int)(gid - d.n_obs - d.n_points);
        double R0[9], t0[3], R[9], t[3], e[6], Jw[9], Jv[9];
        load_pose(d.pose0, f, R0, t0);
        load_pose(d.pose[which], f, R, t);
        pose_prior<false>(R0, t0, R, t, e, Jw, Jv);
#pragma unroll
        for (int k = 0; k < 6; ++k)
            c = c + (e[k] * e[k]) * d.w[6 * (int64_t)f + k];
    }
    d.terms[gid] = c;
}

// s_o and w(s_o) of every observation at the given poses and points; w = 1 without a loss
__global__ __launch_bounds__(kBasThreads) void bas_obs_stats_kernel(BasDev d, const double *poses, const double *points,
                                                                    double *chi2, double *weight)
{
    const int o = blockIdx.x * kBasThreads + threadIdx.x;
    if (o >= d.n_obs)
        return;
    const Cam cam = cam_of(d);
    double R[9], t[3], p[3], r[2], Jc[12], Jp[6];
    load_pose(poses, d.obs_frame[o], R, t);
    const double *pp = points + 3 * (int64_t)d.obs_point[o];
    p[0] = pp[0], p[1] = pp[1], p[2] = pp[2];
    project_lin<false>(cam, R, t, p, d.obs_uv[2 * (int64_t)o], d.obs_uv[2 * (int64_t)o + 1], r, Jc, Jp);
    const double W0 = d.oinfo0[3 * (int64_t)o], W1 = d.oinfo0[3 * (int64_t)o + 1], W2 = d.oinfo0[3 * (int64_t)o + 2];
    const double s = obs_chi2(r, W0, W1, W2);
    chi2[o] = s;
    if (weight)
        weight[o] = d.loss != 0 ? loss_weight(d.loss, d.loss_k, s, sqrt(s)) : 1.0;
}

// out[blockIdx.x] = the sum of in[blockIdx.x * chunk .. + chunk) (clipped to n): thread t takes t, t + 256, ... in order, then
// a fixed tree over the 256 partial sums.  The second stage is one workgroup with chunk >= n.
__global__ __launch_bounds__(kBasThreads) void bas_reduce_kernel(const double *in, int64_t n, int64_t chunk, double *out)
{
    __shared__ double red[kBasThreads];
    const int tid = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    for (int64_t k = lo + tid; k < hi; k += kBasThreads)
        s = s + in[k];
    red[tid] = s;
    __syncthreads();
    for (int w = kBasThreads / 2; w > 0; w >>= 1) {
        if (tid < w)
            red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    if (tid == 0)
        out[blockIdx.x] = red[0];
}

// ---- covariances ----------------------------------------------------------------------------------------------------------------
// The blocks of X = (L L^T)^-1 inside the envelope of the factor the step left in sky (a diagonal block holds L_jj^-1), from
// X L = L^-T: for column j in descending order, with the rows k > j whose envelope reaches j (first[k] <= j, k <= last[j]),
//   M_k  = L_kj L_jj^-1
//   X_ij = -sum_k X_ik M_k                          for every such row i (X_ik is block (i, k) or the transpose of (k, i):
//                                                    both lie inside the envelope, which is closed under the recurrence)
//   X_jj = L_jj^-T L_jj^-1 - sum_k X_kj^T M_k       (its lower triangle, mirrored)
// every sum over k ascending; one owner per entry, three barriers per column.
__global__ __launch_bounds__(kBasThreads) void bas_selinv_kernel(BasDev d)
{
    const int tid = threadIdx.x, N = d.n_frames;
    auto blk = [&](int r, int c) { return (int64_t)d.row_off[r] + (c - d.first[r]); };
    for (int j = N - 1; j >= 0; --j) {
        const int last = d.last[j], rows = last - j;
        const double *Lj = d.sky + 36 * blk(j, j);   // L_jj^-1, lower
        for (int it = tid; it < rows * 36; it += kBasThreads) {
            const int k = j + 1 + it / 36, e = it % 36, q = e / 6, c = e - 6 * q;
            if (d.first[k] > j)
                continue;
            const double *B = d.sky + 36 * blk(k, j);
            double v = B[6 * q + c] * Lj[6 * c + c];
            for (int p = c + 1; p < 6; ++p)
                v = fma(B[6 * q + p], Lj[6 * p + c], v);
            d.colm[36 * (int64_t)k + e] = v;
        }
        __syncthreads();
        for (int it = tid; it < rows * 36; it += kBasThreads) {
            const int i = j + 1 + it / 36, e = it % 36, r = e / 6, c = e - 6 * r;
            if (d.first[i] > j)
                continue;
            double acc = 0.0;
            for (int k = j + 1; k <= last; ++k) {
                if (d.first[k] > j)
                    continue;
                const double *M = d.colm + 36 * (int64_t)k;
                if (k <= i) {
                    const double *X = d.inv + 36 * blk(i, k);
#pragma unroll
                    for (int q = 0; q < 6; ++q)
                        acc = fma(X[6 * r + q], M[6 * q + c], acc);
                } else {
                    const double *X = d.inv + 36 * blk(k, i);
#pragma unroll
                    for (int q = 0; q < 6; ++q)
                        acc = fma(X[6 * q + r], M[6 * q + c], acc);
                }
            }
            d.inv[36 * blk(i, j) + e] = 0.0 - acc;
        }
        __syncthreads();
        if (tid < 36) {
            const int r0 = tid / 6, c0 = tid - 6 * r0, r = r0 >= c0 ? r0 : c0, c = r0 >= c0 ? c0 : r0;
            double v = Lj[6 * r + r] * Lj[6 * r + c];
            for (int p = r + 1; p < 6; ++p)
                v = fma(Lj[6 * p + r], Lj[6 * p + c], v);
            double acc = 0.0;
            for (int k = j + 1; k <= last; ++k) {
                if (d.first[k] > j)
                    continue;
                const double *M = d.colm + 36 * (int64_t)k, *X = d.inv + 36 * blk(k, j);
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    acc = fma(X[6 * q + r], M[6 * q + c], acc);
            }
            d.inv[36 * blk(j, j) + tid] = v - acc;
        }
        __syncthreads();
    }
}

// pose_cov_f = C_f^-T X_ff C_f^-1
__global__ __launch_bounds__(kBasThreads) void bas_pose_cov_kernel(BasDev d)
{
    const int gid = blockIdx.x * kBasThreads + threadIdx.x;
    const int f = gid / 36, e = gid - 36 * f, r = e / 6, c = e - 6 * r;
    if (f >= d.n_frames)
        return;
    const double *Cf = d.Cinv + 21 * (int64_t)f;
    const double *X = d.inv + 36 * ((int64_t)d.row_off[f] + (f - d.first[f]));
    double v = 0.0;
    for (int p = r; p < 6; ++p) {
        double s = 0.0;
        for (int q = c; q < 6; ++q)
            s = fma(X[6 * p + q], Cf[lidx(q, c)], s);
        v = fma(Cf[lidx(p, r)], s, v);
    }
    d.pose_cov[36 * (int64_t)f + e] = v;
}

// Z_o <- C_f^-1 Z_o: the scaled system's Z
__global__ __launch_bounds__(kBasThreads) void bas_zs_kernel(BasDev d)
{
    const int o = blockIdx.x * kBasThreads + threadIdx.x;
    if (o >= d.n_obs)
        return;
    const double *Cf = d.Cinv + 21 * (int64_t)d.obs_frame[o];
    double *Z = d.Z + 18 * (int64_t)o;
    double z[18];
#pragma unroll
    for (int k = 0; k < 18; ++k)
        z[k] = Z[k];
#pragma unroll
    for (int a = 5; a >= 0; --a)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double s = Cf[lidx(a, 0)] * z[k];
#pragma unroll
            for (int p = 1; p <= a; ++p)
                s = fma(Cf[lidx(a, p)], z[3 * p + k], s);
            Z[3 * a + k] = s;
        }
}

// Y_o = sum over the observations c of o's point of X(f_o, f_c) Z_c (6 x 3), ascending
__global__ __launch_bounds__(kBasThreads) void bas_y_kernel(BasDev d)
{
    const int o = blockIdx.x * kBasThreads + threadIdx.x;
    if (o >= d.n_obs)
        return;
    const int i = d.obs_point[o], fo = d.obs_frame[o];
    double Y[18];
#pragma unroll
    for (int k = 0; k < 18; ++k)
        Y[k] = 0.0;
    for (int c = d.obs_off[i]; c < d.obs_off[i + 1]; ++c) {
        const int fc = d.obs_frame[c];
        const double *Zc = d.Z + 18 * (int64_t)c;
        const bool lower = fo >= fc;
        const double *X = d.inv + 36 * (lower ? (int64_t)d.row_off[fo] + (fc - d.first[fo]) : (int64_t)d.row_off[fc] + (fo - d.first[fc]));
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const double x = lower ? X[6 * a + q] : X[6 * q + a];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    Y[3 * a + k] = fma(x, Zc[3 * q + k], Y[3 * a + k]);
            }
    }
    double *out = d.lin + (int64_t)kBasLin * o;
#pragma unroll
    for (int k = 0; k < 18; ++k)
        out[k] = Y[k];
}

// point_cov = L^-T (I + sum_o Z_o^T Y_o) L^-1: refine_window_kernel's statements
__global__ __launch_bounds__(kBasThreads) void bas_point_cov_kernel(BasDev d)
{
    const int i = blockIdx.x * kBasThreads + threadIdx.x;
    if (i >= d.n_points)
        return;
    double M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
        M[k] = 0.0;
    for (int o = d.obs_off[i]; o < d.obs_off[i + 1]; ++o) {
        const double *Z = d.Z + 18 * (int64_t)o, *Y = d.lin + (int64_t)kBasLin * o;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double z = Z[3 * a + r];
                M[3 * r] = fma(z, Y[3 * a], M[3 * r]);
                M[3 * r + 1] = fma(z, Y[3 * a + 1], M[3 * r + 1]);
                M[3 * r + 2] = fma(z, Y[3 * a + 2], M[3 * r + 2]);
            }
    }
    const double *Li = d.Li + 6 * (int64_t)i;
    const double b00 = 1.0 + M[0], b01 = 0.5 * (M[1] + M[3]), b02 = 0.5 * (M[2] + M[6]), b11 = 1.0 + M[4],
                 b12 = 0.5 * (M[5] + M[7]), b22 = 1.0 + M[8];
    const double T00 = fd3(b00, Li[0], b01, Li[1], b02, Li[3]), T01 = fd2(b01, Li[2], b02, Li[4]), T02 = b02 * Li[5];
    const double T10 = fd3(b01, Li[0], b11, Li[1], b12, Li[3]), T11 = fd2(b11, Li[2], b12, Li[4]), T12 = b12 * Li[5];
    const double T20 = fd3(b02, Li[0], b12, Li[1], b22, Li[3]), T21 = fd2(b12, Li[2], b22, Li[4]), T22 = b22 * Li[5];
    const double C00 = fd3(Li[0], T00, Li[1], T10, Li[3], T20);
    const double C01 = fd3(Li[0], T01, Li[1], T11, Li[3], T21);
    const double C02 = fd3(Li[0], T02, Li[1], T12, Li[3], T22);
    const double C11 = fd2(Li[2], T11, Li[4], T21);
    const double C12 = fd2(Li[2], T12, Li[4], T22);
    const double C22 = Li[5] * T22;
    double *o = d.point_cov + 9 * (int64_t)i;
    o[0] = C00, o[1] = C01, o[2] = C02, o[3] = C01, o[4] = C11, o[5] = C12, o[6] = C02, o[7] = C12, o[8] = C22;
}

inline int grid_of(int64_t n) { return (int)((n + kBasThreads - 1) / kBasThreads); }

}  // namespace

void launch_bas_cost(const BasDev &d, int which, hipStream_t stream)
{
    const int64_t n = (int64_t)d.n_obs + d.n_points + d.n_frames;
    const int chunks = (int)((n + kBasRedChunk - 1) / kBasRedChunk);
    if (d.loss != 0)
        hipLaunchKernelGGL(bas_robust_terms_kernel, dim3(grid_of(n)), dim3(kBasThreads), 0, stream, d, which);
    else
        hipLaunchKernelGGL(bas_terms_kernel, dim3(grid_of(n)), dim3(kBasThreads), 0, stream, d, which);
    hipLaunchKernelGGL(bas_reduce_kernel, dim3(chunks), dim3(kBasThreads), 0, stream, d.terms, n, (int64_t)kBasRedChunk, d.partial);
    hipLaunchKernelGGL(bas_reduce_kernel, dim3(1), dim3(kBasThreads), 0, stream, d.partial, (int64_t)chunks, (int64_t)chunks,
                       &d.state->cost);
}

void launch_bas_build(const BasDev &d, int cur, double lam, hipStream_t stream)
{
    if (d.loss != 0)
        hipLaunchKernelGGL(bas_robust_lin_kernel, dim3(grid_of(d.n_obs)), dim3(kBasThreads), 0, stream, d, cur);
    else
        hipLaunchKernelGGL(bas_lin_kernel, dim3(grid_of(d.n_obs)), dim3(kBasThreads), 0, stream, d, cur);
    hipLaunchKernelGGL(bas_point_kernel, dim3(grid_of(d.n_points)), dim3(kBasThreads), 0, stream, d, cur, lam);
    hipLaunchKernelGGL(bas_z_kernel, dim3(grid_of(d.n_obs)), dim3(kBasThreads), 0, stream, d);
    hipLaunchKernelGGL(bas_prior_kernel, dim3((d.n_frames + 63) / 64), dim3(64), 0, stream, d, cur);
    hipLaunchKernelGGL(bas_frame_kernel, dim3(grid_of(27 * (int64_t)d.n_frames)), dim3(kBasThreads), 0, stream, d, cur);
    hipLaunchKernelGGL(bas_schur_kernel, dim3((d.n_blocks + kBasPerWg - 1) / kBasPerWg), dim3(kBasThreads), 0, stream, d);
}

void launch_bas_update(const BasDev &d, int cur, hipStream_t stream)
{
    hipLaunchKernelGGL(bas_zd_kernel, dim3(grid_of(d.n_obs)), dim3(kBasThreads), 0, stream, d);
    hipLaunchKernelGGL(bas_update_kernel, dim3(grid_of((int64_t)d.n_points + d.n_frames)), dim3(kBasThreads), 0, stream, d, cur);
}

void launch_bas_obs_stats(const BasDev &d, const double *poses, const double *points, double *chi2, double *weight,
                          hipStream_t stream)
{
    hipLaunchKernelGGL(bas_obs_stats_kernel, dim3(grid_of(d.n_obs)), dim3(kBasThreads), 0, stream, d, poses, points, chi2, weight);
}

void launch_bas_cov(const BasDev &d, hipStream_t stream)
{
    hipLaunchKernelGGL(bas_selinv_kernel, dim3(1), dim3(kBasThreads), 0, stream, d);
    if (d.pose_cov)
        hipLaunchKernelGGL(bas_pose_cov_kernel, dim3(grid_of(36 * (int64_t)d.n_frames)), dim3(kBasThreads), 0, stream, d);
    if (d.point_cov) {
        hipLaunchKernelGGL(bas_zs_kernel, dim3(grid_of(d.n_obs)), dim3(kBasThreads), 0, stream, d);
        hipLaunchKernelGGL(bas_y_kernel, dim3(grid_of(d.n_obs)), dim3(kBasThreads), 0, stream, d);
        hipLaunchKernelGGL(bas_point_cov_kernel, dim3(grid_of(d.n_points)), dim3(kBasThreads), 0, stream, d);
    }
}

}  // namespace mvs
