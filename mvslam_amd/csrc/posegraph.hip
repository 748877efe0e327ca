// posegraph.hip -- the back end: Graph / GraphOptimizer of back-end/graph.{hpp,cpp}, i.e. GTSAM's
// Levenberg-Marquardt over Pose3 values, BetweenFactor<Pose3> edges with full 6 x 6 covariances and one anchoring prior.
// DESIGN.md section 4.10 states the contract; in short
//   cost = 1/2 [ |e_anchor|^2 + sum_k |e_k|^2 ],  e_k = ( Log(Rz^T Rs^T Rd),  Rz^T (Rs^T (td - ts) - tz) ),
// every residual whitened by L^-1 of its covariance S = L L^T, right perturbation R <- R Exp(dw), t <- t + R dv.
//
// Two paths, one arithmetic:
//   N <= 16 nodes (pg_dense_kernel): one workgroup per graph, the whole LM loop in one launch (the shape of
//   refine_window_kernel).  Edges are strided over the threads, which park every linearised edge in global memory; then
//   every entry of the dense lower triangle of H in LDS (at most 96 * 97 / 2 doubles = 37 KB) is summed by ONE thread over
//   the edges in edge order -- no atomics, no partial-sum tree whose shape depends on the launch.  Cholesky and the two
//   triangular solves run on that triangle in LDS.
//   17 <= N <= 4096 (the pg_* kernels behind launch_pg_begin / _cg / _end): LM driven from the host, one synchronisation per LM
//   iteration; H is never formed.  One thread per edge linearises, one thread per node gathers its incident edges (a CSR
//   list in edge order) into the diagonal block and the gradient, and a block-Jacobi preconditioned conjugate gradient
//   solves (H + lambda I) x = -g with H p = edge kernel + the same gather.  The CG iterations of the budget are enqueued
//   up front (all of them, or chunk by chunk with a status read in between: launch_pg_begin / _cg / _end); a status word on
//   the device makes the ones behind convergence leave at once (DESIGN.md 4.7.3's pattern).
// The LM rule is refine_kernel's, restated: lambda is ADDED to the diagonal, a candidate is accepted when its cost is not
// above the current one, lambda /= factor on acceptance and *= factor on rejection, stop when the decrease (or, for a
// rejected candidate that did solve, the increase) of the error is within abs_tol or rel_tol * error, or lambda passes
// lambda_upper, or after max_iterations linear solves.
//
// Robust edge losses (mvs_ctx_set_pose_graph_loss) enter through pg_loss alone: an edge's term of
// the cost becomes rho2(|r|^2) and its linearisation is multiplied by sqrt(w), in pg_dense_kernel and pg_edge_kernel; every
// other kernel, pg_direct.hip's included, reads what those two left.  Without a loss the kernels are the ones they were.
//
// The SO(3), prior, Cholesky and loss functions are lm_math.hpp's and the edge functions pg_edge.hpp's, shared with the other solvers.
#include "pg_edge.hpp"

namespace mvs {

namespace {

constexpr int kPgThreads = 256;
constexpr int kPgDim = 6 * kPgDenseMaxNodes;   // 96

__device__ __forceinline__ double sq6(const double (&r)[6])
{
    return fma(r[5], r[5], fma(r[4], r[4], fma(r[3], r[3], fma(r[2], r[2], fma(r[1], r[1], r[0] * r[0])))));
}

// ---- robust losses (mvs_ctx_set_pose_graph_loss) ----------------------------------------------
// edge k_index with s = |r|^2: rho2(s), its term of twice the cost, and sqrt(w(s)), the factor of its residual and Jacobians.
// Below cfg.loss_first: s and 1.  The order is the contract's: one sqrt, one division (the Cauchy cost: log1p of one
// quotient), one sqrt.
__device__ __forceinline__ void pg_loss(const PgCfg &cfg, int k_index, double s, double &rho2, double &sqrt_w)
{
    rho2 = s;
    sqrt_w = 1.0;
    if (k_index < cfg.loss_first)
        return;
    const double k = cfg.loss_k, x = sqrt(s);
    rho2 = pg_loss_rho2(cfg.loss, k, s, x);
    sqrt_w = sqrt(loss_weight(cfg.loss, k, s, x));
}
// the linearised edge {r, A_src, A_dst} times sqrt(w): what makes the normal equations those of the reweighted problem
__device__ __forceinline__ void pg_scale_lin(double *lin, double sqrt_w)
{
    for (int i = 0; i < kPgLin; ++i)
        lin[i] = lin[i] * sqrt_w;
}

// anchor prior at pose P with mean P0: cost, and when JAC the error and the two Jacobians into anc = {e[6], Jw[9], Jv[9]}
template <bool JAC>
__device__ __forceinline__ double anchor_eval(const PgCfg &cfg, const double *P0, const double *P, double *anc)
{
    double R0[9], t0[3], R[9], t[3], e[6], Jw[9], Jv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        R0[k] = P0[k];
        R[k] = P[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t0[k] = P0[9 + k];
        t[k] = P[9 + k];
    }
    pose_prior<JAC>(R0, t0, R, t, e, Jw, Jv);
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            anc[k] = e[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            anc[6 + k] = Jw[k];
            anc[15 + k] = Jv[k];
        }
    }
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        c = c + (e[k] * e[k]) * cfg.w_anchor[k / 3];
    return c;
}
// entry (i, j) of the prior's block of H and entry i of its gradient, from anc
__device__ __forceinline__ double anchor_h(const PgCfg &cfg, const double *anc, int i, int j)
{
    if ((i < 3) != (j < 3))
        return 0.0;
    const double *J = anc + (i < 3 ? 6 : 15);
    const double w = i < 3 ? cfg.w_anchor[0] : cfg.w_anchor[1];
    const int a = i % 3, c = j % 3;
    return (J[a] * w * J[c] + J[3 + a] * w * J[3 + c]) + J[6 + a] * w * J[6 + c];
}
__device__ __forceinline__ double anchor_g(const PgCfg &cfg, const double *anc, int i)
{
    const double *J = anc + (i < 3 ? 6 : 15), *e = anc + (i < 3 ? 0 : 3);
    const double w = i < 3 ? cfg.w_anchor[0] : cfg.w_anchor[1];
    const int a = i % 3;
    return (J[a] * w * e[0] + J[3 + a] * w * e[1]) + J[6 + a] * w * e[2];
}

// R <- R Exp(dw), t <- t + R dv
__device__ __forceinline__ void retract(const double *P, const double *dx, double *Pn)
{
    const double dw[3] = {dx[0], dx[1], dx[2]};
    double E[9];
    so3_exp(dw, E);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            Pn[3 * r + c] = (P[3 * r] * E[c] + P[3 * r + 1] * E[3 + c]) + P[3 * r + 2] * E[6 + c];
        Pn[9 + r] = P[9 + r] + ((P[3 * r] * dx[3] + P[3 * r + 1] * dx[4]) + P[3 * r + 2] * dx[5]);
    }
}

// fixed-order sum over the workgroup (4 wavefronts): xor butterfly inside each wavefront, then (w0 + w1) + (w2 + w3).
// Every thread returns the same bits.
__device__ __forceinline__ double block_sum(double x, double *red)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1)
        x = x + __shfl_xor(x, s);
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = x;
    __syncthreads();
    const double t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}

// ---- dense path -------------------------------------------------------------------------------------------------------
// LOSS: the context has a robust loss.  Without it the kernel holds the statements it held before there were losses.
template <bool LOSS>
__global__ __launch_bounds__(kPgThreads) void pg_dense_kernel(PgDenseDev d)
{
    __shared__ double H[kPgDim * (kPgDim + 1) / 2];
    __shared__ double gv[kPgDim], yv[kPgDim], dg[kPgDim], inv[kPgDim];
    __shared__ double pose[2][kPgDenseMaxNodes * 12];
    __shared__ double anc[24];
    __shared__ double red[4];
    const PgProblem P = d.prob[blockIdx.x];
    const PgCfg &cfg = d.cfg;
    const int N = P.n_nodes, E = P.n_edges, n = 6 * N, tid = threadIdx.x;
    mvs_pose_graph_result *out = d.out + blockIdx.x;
    if (N < 1 || N > kPgDenseMaxNodes || E < 0 || P.anchor < 0 || P.anchor >= N) {   // the host never sends such a graph
        if (tid == 0) {
            out->ok = 0, out->iterations = 0, out->cg_iterations = 0, out->rejected_steps = 0;
            out->error_initial = 0.0, out->error = 0.0;
        }
        return;
    }
    const int32_t *src = d.edge_src + P.edge_off, *dst = d.edge_dst + P.edge_off;
    const double *Z = d.edge_pose + 12 * P.edge_off, *cov = d.edge_cov + 36 * P.edge_off;
    const double *pose0 = d.node_pose + 12 * P.node_off;
    double *W = d.W + 21 * P.edge_off, *lin = d.lin + (int64_t)kPgLin * P.edge_off;

    for (int i = tid; i < 12 * N; i += kPgThreads)
        pose[0][i] = pose0[i];
    int bad = 0;
    for (int k = tid; k < E; k += kPgThreads) {
        const int s = src[k], t = dst[k];
        if (s < 0 || s >= N || t < 0 || t >= N || s == t || !edge_prep(cov + 36 * (int64_t)k, W + 21 * (int64_t)k))
            bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) {
            out->ok = 0, out->iterations = 0, out->cg_iterations = 0, out->rejected_steps = 0;
            out->error_initial = 0.0, out->error = 0.0;
        }
        return;
    }

    // sum of the squared whitened residuals (under a loss: of rho2 of each) at ps (an LDS pose table), the same bits in
    // every thread
    auto cost_at = [&](const double *ps) -> double {
        double c = 0.0;
        for (int k = tid; k < E; k += kPgThreads) {
            double r[6];
            edge_eval<false>(Z + 12 * (int64_t)k, W + 21 * (int64_t)k, ps + 12 * src[k], ps + 12 * dst[k], r, nullptr);
            if (LOSS) {
                double rho2, sw;
                pg_loss(cfg, k, sq6(r), rho2, sw);
                c = c + rho2;
            } else {
                c = c + sq6(r);
            }
        }
        return block_sum(c, red) + anchor_eval<false>(cfg, pose0 + 12 * P.anchor, ps + 12 * P.anchor, nullptr);
    };

    int cb = 0;
    double cur = cost_at(pose[0]);
    const double cost0 = cur;
    double lam = cfg.lambda_initial;
    int it = 0, rejected = 0;
    const bool ok0 = cur < __builtin_inf() && cur == cur;
    while (ok0 && it < cfg.max_iterations) {
        const double *ps = pose[cb];
        double *pn = pose[cb ^ 1];
        // linearise: every edge's whitened residual and Jacobians, parked in global memory
        for (int k = tid; k < E; k += kPgThreads) {
            double r[6];
            edge_eval<true>(Z + 12 * (int64_t)k, W + 21 * (int64_t)k, ps + 12 * src[k], ps + 12 * dst[k], r,
                            lin + (int64_t)kPgLin * k);
            if (LOSS) {
                double rho2, sw;
                pg_loss(cfg, k, sq6(r), rho2, sw);
                pg_scale_lin(lin + (int64_t)kPgLin * k, sw);
            }
        }
        if (tid == 0)
            anchor_eval<true>(cfg, pose0 + 12 * P.anchor, ps + 12 * P.anchor, anc);
        __syncthreads();
        // H (lower triangle) and the right-hand side -g: one thread per entry, edges in edge order
        for (int idx = tid; idx < n * n; idx += kPgThreads) {
            const int row = idx / n, col = idx - row * n;
            if (col > row)
                continue;
            const int a = row / 6, i = row - 6 * a, b = col / 6, j = col - 6 * b;
            double acc = 0.0;
            for (int k = 0; k < E; ++k) {
                const int s = src[k], t = dst[k];
                const double *As = lin + (int64_t)kPgLin * k + 6, *Ad = As + 36;
                if (a == b) {
                    if (s == a)
                        acc = acc + coldot(As, i, As, j);
                    else if (t == a)
                        acc = acc + coldot(Ad, i, Ad, j);
                } else if (s == a && t == b) {
                    acc = acc + coldot(As, i, Ad, j);
                } else if (s == b && t == a) {
                    acc = acc + coldot(Ad, i, As, j);
                }
            }
            if (a == b && a == P.anchor)
                acc = acc + anchor_h(cfg, anc, i, j);
            if (row == col)
                acc = acc + lam;
            H[lidx(row, col)] = acc;
        }
        for (int row = tid; row < n; row += kPgThreads) {
            const int a = row / 6, i = row - 6 * a;
            double acc = 0.0;
            for (int k = 0; k < E; ++k) {
                const double *L = lin + (int64_t)kPgLin * k;
                if (src[k] == a)
                    acc = acc + colvec(L + 6, i, L);
                else if (dst[k] == a)
                    acc = acc + colvec(L + 42, i, L);
            }
            if (a == P.anchor)
                acc = acc + anchor_g(cfg, anc, i);
            gv[row] = -acc;
        }
        __syncthreads();
        // Cholesky in LDS, column by column: thread t owns row j + t of column j; inv[j] = 1 / l_jj
        bool solved = true;
        for (int j = 0; j < n; ++j) {
            const int i = j + tid;
            double v = 0.0;
            if (i < n) {
                v = H[lidx(i, j)];
                for (int k = 0; k < j; ++k)
                    v = fma(-H[lidx(i, k)], H[lidx(j, k)], v);
                if (tid == 0)
                    dg[j] = v;
            }
            __syncthreads();
            const double dd = dg[j];
            solved = solved && (dd > 0.0) && (dd < __builtin_inf());
            const double iv = 1.0 / sqrt(dd);
            if (i < n) {
                if (tid == 0)
                    inv[j] = iv;
                else
                    H[lidx(i, j)] = v * iv;
            }
            __syncthreads();
        }
        bool accepted = false;
        double cand = 0.0;
        if (solved) {   // uniform: every thread read the same pivots
            for (int k = 0; k < n; ++k) {          // L y = -g
                const double yk = gv[k] * inv[k];
                const int i = k + 1 + tid;
                if (i < n)
                    gv[i] = fma(-H[lidx(i, k)], yk, gv[i]);
                if (tid == 0)
                    yv[k] = yk;
                __syncthreads();
            }
            for (int k = n - 1; k >= 0; --k) {     // L^T x = y, x into gv
                const double xk = yv[k] * inv[k];
                if (tid < k)
                    yv[tid] = fma(-H[lidx(k, tid)], xk, yv[tid]);
                if (tid == 0)
                    gv[k] = xk;
                __syncthreads();
            }
            if (tid < N)
                retract(ps + 12 * tid, gv + 6 * tid, pn + 12 * tid);
            __syncthreads();
            cand = cost_at(pn);
            accepted = cand <= cur;
        }
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
            // a trial within the tolerances ABOVE the current error: at the minimum to rounding, stop
            const double inc = 0.5 * (cand - cur);
            if (solved && (inc <= cfg.abs_tol || inc <= cfg.rel_tol * (0.5 * cur)))
                break;
            lam = lam * cfg.lambda_factor;
            if (lam > cfg.lambda_upper)
                break;
        }
        __syncthreads();   // the next linearisation overwrites anc / H / gv
    }
    __syncthreads();
    if (ok0) {
        double *po = d.poses_out + 12 * P.node_off;
        for (int i = tid; i < 12 * N; i += kPgThreads)
            po[i] = pose[cb][i];
    }
    if (tid == 0) {
        out->ok = ok0 ? 1 : 0;
        out->iterations = it;
        out->cg_iterations = 0;
        out->rejected_steps = rejected;
        out->error_initial = ok0 ? 0.5 * cost0 : 0.0;   // a cost that is not finite: the zero record of every other failure
        out->error = ok0 ? 0.5 * cur : 0.0;
    }
}

// ---- large path -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgThreads) void pg_prep_kernel(PgLargeDev d)
{
    const int k = blockIdx.x * kPgThreads + threadIdx.x;
    if (k == 0) {
        d.state->done = 0;
        d.state->cg_iters = 0;
    }
    if (k >= d.n_edges)
        return;
    if (!edge_prep(d.edge_cov + 36 * (int64_t)k, d.W + 21 * (int64_t)k))
        d.state->bad_cov = 1;   // every writer stores the same word (the host zeroes it before the launch)
}

// LOSS: as in pg_dense_kernel.  The PCG and the direct step read `lin` and `ecost` and nothing else of an edge, so the loss
// reaches both through this kernel alone.
template <bool JAC, bool LOSS>
__global__ __launch_bounds__(kPgThreads) void pg_edge_kernel(PgLargeDev d, const double *ps)
{
    const int k = blockIdx.x * kPgThreads + threadIdx.x;
    if (k >= d.n_edges)
        return;
    double r[6];
    edge_eval<JAC>(d.edge_pose + 12 * (int64_t)k, d.W + 21 * (int64_t)k, ps + 12 * (int64_t)d.edge_src[k],
                   ps + 12 * (int64_t)d.edge_dst[k], r, JAC ? d.lin + (int64_t)kPgLin * k : nullptr);
    if (LOSS) {
        double rho2, sw;
        pg_loss(d.cfg, k, sq6(r), rho2, sw);
        if (JAC)
            pg_scale_lin(d.lin + (int64_t)kPgLin * k, sw);
        else
            d.ecost[k] = rho2;
    } else if (!JAC) {
        d.ecost[k] = sq6(r);
    }
}

// edge k at the poses d.X: chi2 = |r|^2 of its whitened residual and its weight under d.cfg's loss
__global__ __launch_bounds__(kPgThreads) void pg_edge_stats_kernel(PgStatsDev d)
{
    const int k = blockIdx.x * kPgThreads + threadIdx.x;
    if (k >= d.n_edges)
        return;
    double *W = d.W + 21 * (int64_t)k;
    if (!edge_prep(d.edge_cov + 36 * (int64_t)k, W))
        *d.bad_cov = 1;   // every writer stores the same word
    double r[6];
    edge_eval<false>(d.edge_pose + 12 * (int64_t)k, W, d.X + 12 * (int64_t)d.edge_src[k], d.X + 12 * (int64_t)d.edge_dst[k], r,
                     nullptr);
    const double s = sq6(r);
    d.chi2[k] = s;
    if (d.weight)
        d.weight[k] = d.cfg.loss != 0 && k >= d.cfg.loss_first ? loss_weight(d.cfg.loss, d.cfg.loss_k, s, sqrt(s)) : 1.0;
}

// sum of the edges' costs (thread t: edges t, t + 256, ... in order; then the workgroup tree) + the anchor -> *dst
__global__ __launch_bounds__(kPgThreads) void pg_cost_reduce_kernel(PgLargeDev d, const double *ps, double *dst)
{
    __shared__ double red[4];
    double c = 0.0;
    for (int k = threadIdx.x; k < d.n_edges; k += kPgThreads)
        c = c + d.ecost[k];
    const double tot = block_sum(c, red) +
                       anchor_eval<false>(d.cfg, d.pose0 + 12 * (int64_t)d.anchor, ps + 12 * (int64_t)d.anchor, nullptr);
    if (threadIdx.x == 0)
        *dst = tot;
}

// node i: diagonal block D_i = sum A^T A and gradient g_i = sum A^T r over its incident edges, in edge order
__global__ __launch_bounds__(64) void pg_gather_kernel(PgLargeDev d, const double *ps)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= d.n_nodes)
        return;
    double D[21], g[6];
#pragma unroll
    for (int k = 0; k < 21; ++k)
        D[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        g[k] = 0.0;
    for (int c = d.csr_off[i]; c < d.csr_off[i + 1]; ++c) {
        const int code = d.csr_inc[c];
        const double *L = d.lin + (int64_t)kPgLin * (code >> 1), *A = L + 6 + 36 * (code & 1);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b)
                D[lidx(a, b)] = D[lidx(a, b)] + coldot(A, a, A, b);
            g[a] = g[a] + colvec(A, a, L);
        }
    }
    if (i == d.anchor) {
        double anc[24];
        anchor_eval<true>(d.cfg, d.pose0 + 12 * (int64_t)i, ps + 12 * (int64_t)i, anc);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const double h = anchor_h(d.cfg, anc, a, b);
                d.Ha[6 * a + b] = h;
                if (b <= a)
                    D[lidx(a, b)] = D[lidx(a, b)] + h;
            }
            g[a] = g[a] + anchor_g(d.cfg, anc, a);
        }
    }
#pragma unroll
    for (int k = 0; k < 21; ++k)
        d.D[21 * (int64_t)i + k] = D[k];
#pragma unroll
    for (int k = 0; k < 6; ++k)
        d.g[6 * (int64_t)i + k] = g[k];
}

// PCG start (one workgroup): M_i = (D_i + lambda I)^-1 as Cholesky factors, x = 0, r = -g, z = M r, p = z
__global__ __launch_bounds__(kPgThreads) void pg_cg_init_kernel(PgLargeDev d, double lam)
{
    __shared__ double red[4];
    double rz = 0.0, rr = 0.0;
    int bad = 0;
    for (int i = threadIdx.x; i < d.n_nodes; i += kPgThreads) {
        double M[21], r[6], z[6];
#pragma unroll
        for (int k = 0; k < 21; ++k)
            M[k] = d.D[21 * (int64_t)i + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            M[lidx(k, k)] = M[lidx(k, k)] + lam;
            r[k] = -d.g[6 * (int64_t)i + k];
            z[k] = r[k];
        }
        if (!chol_packed<6>(M))
            bad = 1;
        chol_solve<6>(M, z);
#pragma unroll
        for (int k = 0; k < 21; ++k)
            d.Mf[21 * (int64_t)i + k] = M[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            d.x[6 * (int64_t)i + k] = 0.0;
            d.r[6 * (int64_t)i + k] = r[k];
            d.z[6 * (int64_t)i + k] = z[k];
            d.p[6 * (int64_t)i + k] = z[k];
            rz = fma(r[k], z[k], rz);
            rr = fma(r[k], r[k], rr);
        }
    }
    bad = __syncthreads_or(bad);
    rz = block_sum(rz, red);
    rr = block_sum(rr, red);
    if (threadIdx.x == 0) {
        d.state->rz = rz;
        d.state->gnorm2 = rr;
        d.state->rr = rr;
        d.state->cg_iters = 0;
        d.state->done = bad || !(rr == rr) || !(rr < __builtin_inf()) ? 2 : (rr == 0.0 ? 1 : 0);
    }
}

// u_k = A_src p_src + A_dst p_dst
__global__ __launch_bounds__(kPgThreads) void pg_edge_mv_kernel(PgLargeDev d)
{
    if (d.state->done)
        return;
    const int k = blockIdx.x * kPgThreads + threadIdx.x;
    if (k >= d.n_edges)
        return;
    const double *As = d.lin + (int64_t)kPgLin * k + 6, *Ad = As + 36;
    const double *ps = d.p + 6 * (int64_t)d.edge_src[k], *pd = d.p + 6 * (int64_t)d.edge_dst[k];
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        double s = As[6 * m] * ps[0];
#pragma unroll
        for (int i = 1; i < 6; ++i)
            s = fma(As[6 * m + i], ps[i], s);
#pragma unroll
        for (int i = 0; i < 6; ++i)
            s = fma(Ad[6 * m + i], pd[i], s);
        d.u[6 * (int64_t)k + m] = s;
    }
}

// q_i = sum A^T u over the incident edges (edge order) + prior block + lambda p_i;  pq_i = p_i . q_i
__global__ __launch_bounds__(64) void pg_node_mv_kernel(PgLargeDev d, double lam)
{
    if (d.state->done)
        return;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= d.n_nodes)
        return;
    double q[6], p[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        q[k] = 0.0;
        p[k] = d.p[6 * (int64_t)i + k];
    }
    for (int c = d.csr_off[i]; c < d.csr_off[i + 1]; ++c) {
        const int code = d.csr_inc[c];
        const double *A = d.lin + (int64_t)kPgLin * (code >> 1) + 6 + 36 * (code & 1), *u = d.u + 6 * (int64_t)(code >> 1);
#pragma unroll
        for (int a = 0; a < 6; ++a)
            q[a] = q[a] + colvec(A, a, u);
    }
    if (i == d.anchor) {
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double s = d.Ha[6 * a] * p[0];
#pragma unroll
            for (int b = 1; b < 6; ++b)
                s = fma(d.Ha[6 * a + b], p[b], s);
            q[a] = q[a] + s;
        }
    }
    double pq = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        q[k] = fma(lam, p[k], q[k]);
        d.q[6 * (int64_t)i + k] = q[k];
        pq = fma(p[k], q[k], pq);
    }
    d.pq[i] = pq;
}

// the rest of one PCG iteration (one workgroup): alpha, x, r, z, the stopping rule, beta, p
__global__ __launch_bounds__(kPgThreads) void pg_cg_step_kernel(PgLargeDev d)
{
    __shared__ double red[4];
    PgState *st = d.state;
    if (st->done)
        return;
    double s = 0.0;
    for (int i = threadIdx.x; i < d.n_nodes; i += kPgThreads)
        s = s + d.pq[i];
    const double pq = block_sum(s, red);
    const double rz = st->rz, gn2 = st->gnorm2;
    const int iters = st->cg_iters;
    __syncthreads();   // every thread has read the state before thread 0 rewrites it
    if (!(pq > 0.0) || !(pq < __builtin_inf())) {
        if (threadIdx.x == 0)
            st->done = 2;
        return;
    }
    const double alpha = rz / pq;
    double rzn = 0.0, rr = 0.0;
    for (int i = threadIdx.x; i < d.n_nodes; i += kPgThreads) {
        double M[21], r[6], z[6];
#pragma unroll
        for (int k = 0; k < 21; ++k)
            M[k] = d.Mf[21 * (int64_t)i + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int64_t o = 6 * (int64_t)i + k;
            d.x[o] = fma(alpha, d.p[o], d.x[o]);
            r[k] = fma(-alpha, d.q[o], d.r[o]);
            d.r[o] = r[k];
            z[k] = r[k];
        }
        chol_solve<6>(M, z);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            d.z[6 * (int64_t)i + k] = z[k];
            rzn = fma(r[k], z[k], rzn);
            rr = fma(r[k], r[k], rr);
        }
    }
    rzn = block_sum(rzn, red);
    rr = block_sum(rr, red);
    const bool conv = sqrt(rr) <= d.cfg.cg_rel_tol * sqrt(gn2);
    const bool broke = !(rr == rr) || !(rzn > 0.0);   // rzn = r^T M r = 0 only at r = 0, which conv has caught
    if (!conv && !broke) {
        const double beta = rzn / rz;
        for (int i = threadIdx.x; i < d.n_nodes; i += kPgThreads) {
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int64_t o = 6 * (int64_t)i + k;
                d.p[o] = fma(beta, d.p[o], d.z[o]);
            }
        }
    }
    if (threadIdx.x == 0) {
        st->rz = rzn;
        st->rr = rr;
        st->cg_iters = iters + 1;
        st->done = conv ? 1 : (broke ? 2 : 0);
    }
}

__global__ __launch_bounds__(64) void pg_update_kernel(PgLargeDev d, const double *ps, double *pn)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= d.n_nodes)
        return;
    retract(ps + 12 * (int64_t)i, d.x + 6 * (int64_t)i, pn + 12 * (int64_t)i);
}

}  // namespace

void launch_pg_dense(const PgDenseDev &d, hipStream_t stream)
{
    if (d.n_problems <= 0)
        return;
    if (d.cfg.loss != 0)
        hipLaunchKernelGGL(pg_dense_kernel<true>, dim3(d.n_problems), dim3(kPgThreads), 0, stream, d);
    else
        hipLaunchKernelGGL(pg_dense_kernel<false>, dim3(d.n_problems), dim3(kPgThreads), 0, stream, d);
}

void launch_pg_prep(const PgLargeDev &d, hipStream_t stream)
{
    const int eb = (d.n_edges + kPgThreads - 1) / kPgThreads;
    hipLaunchKernelGGL(pg_prep_kernel, dim3(eb > 0 ? eb : 1), dim3(kPgThreads), 0, stream, d);
}

namespace {
dim3 pg_edge_blocks(const PgLargeDev &d)
{
    const int eb = (d.n_edges + kPgThreads - 1) / kPgThreads;
    return dim3(eb > 0 ? eb : 1);
}
// pg_edge_kernel<JAC> at the poses ps, with or without the context's loss
template <bool JAC>
void launch_pg_edges(const PgLargeDev &d, const double *ps, hipStream_t stream)
{
    if (d.cfg.loss != 0)
        hipLaunchKernelGGL((pg_edge_kernel<JAC, true>), pg_edge_blocks(d), dim3(kPgThreads), 0, stream, d, ps);
    else
        hipLaunchKernelGGL((pg_edge_kernel<JAC, false>), pg_edge_blocks(d), dim3(kPgThreads), 0, stream, d, ps);
}
}  // namespace

void launch_pg_linearise(const PgLargeDev &d, int cur, bool first, hipStream_t stream)
{
    const dim3 nb((d.n_nodes + 63) / 64);
    const double *ps = d.pose[cur];
    if (first) {
        launch_pg_edges<false>(d, ps, stream);
        hipLaunchKernelGGL(pg_cost_reduce_kernel, dim3(1), dim3(kPgThreads), 0, stream, d, ps, &d.state->cost0);
    }
    launch_pg_edges<true>(d, ps, stream);
    hipLaunchKernelGGL(pg_gather_kernel, nb, dim3(64), 0, stream, d, ps);
}

void launch_pg_begin(const PgLargeDev &d, int cur, double lam, bool first, hipStream_t stream)
{
    launch_pg_linearise(d, cur, first, stream);
    hipLaunchKernelGGL(pg_cg_init_kernel, dim3(1), dim3(kPgThreads), 0, stream, d, lam);
}

void launch_pg_cg(const PgLargeDev &d, double lam, int n, hipStream_t stream)
{
    const dim3 eb = pg_edge_blocks(d);
    const dim3 nb((d.n_nodes + 63) / 64);
    for (int c = 0; c < n; ++c) {
        hipLaunchKernelGGL(pg_edge_mv_kernel, eb, dim3(kPgThreads), 0, stream, d);
        hipLaunchKernelGGL(pg_node_mv_kernel, nb, dim3(64), 0, stream, d, lam);
        hipLaunchKernelGGL(pg_cg_step_kernel, dim3(1), dim3(kPgThreads), 0, stream, d);
    }
}

void launch_pg_end(const PgLargeDev &d, int cur, hipStream_t stream)
{
    const dim3 nb((d.n_nodes + 63) / 64);
    const double *ps = d.pose[cur];
    double *pn = d.pose[cur ^ 1];
    hipLaunchKernelGGL(pg_update_kernel, nb, dim3(64), 0, stream, d, ps, pn);
    launch_pg_edges<false>(d, pn, stream);
    hipLaunchKernelGGL(pg_cost_reduce_kernel, dim3(1), dim3(kPgThreads), 0, stream, d, pn, &d.state->cand);
}

void launch_pg_edge_stats(const PgStatsDev &d, hipStream_t stream)
{
    if (d.n_edges <= 0)
        return;
    hipLaunchKernelGGL(pg_edge_stats_kernel, dim3((d.n_edges + kPgThreads - 1) / kPgThreads), dim3(kPgThreads), 0, stream, d);
}

}  // namespace mvs
