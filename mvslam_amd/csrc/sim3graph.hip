// sim3graph.hip -- pose graphs over Sim(3): posegraph.hip's two paths with one more degree of freedom per node (DESIGN.md
// section 4.10.6).  A node is X = (R, t, s), x_w = s R x + t; an edge measures Xs^-1 Xd = (Rs^T Rd, Rs^T (td - ts) / ss, sd / ss),
//   cost = 1/2 [ |e_anchor|^2 + sum_k |e_k|^2 ],  e_k = ( Log(Rz^T Rs^T Rd),  Rz^T (q - tz),  log sd - log ss - log sz ),
// every residual whitened by L^-1 of its 7 x 7 covariance, right perturbation R <- R Exp(dw), t <- t + s R dv, s <- s exp(ds).
//
//   N <= 16 nodes (s3_dense_kernel): one workgroup per graph, the whole LM loop in one launch.  The dense lower triangle of H
//   in LDS is 112 * 113 / 2 doubles = 50624 B; with the solve vectors (4 * 112 doubles), the two node tables (2 * 16 * 13), the
//   anchor record and the reduction cells the kernel holds 57776 B (58032 B as compiled) of static LDS.  Every entry of H is summed by ONE thread
//   over the edges in edge order.
//   17 <= N <= 4096 (the s3_* kernels behind launch_s3_begin / _cg / _end): linearise per edge, gather per node over the CSR
//   list in edge order, block-Jacobi (7 x 7) preconditioned conjugate gradient whose budget is enqueued behind a status word.
// The LM rule, the stopping rules and the reduction shapes are posegraph.hip's, restated.  No robust loss and no direct solver
// here: the context's switches do not reach these kernels.
#include "sim3_edge.hpp"

namespace mvs {

namespace {

constexpr int kS3Threads = 256;
constexpr int kS3Dim = 7 * kS3DenseMaxNodes;   // 112

__device__ __forceinline__ double sq7(const double (&r)[7])
{
    return fma(r[6], r[6], fma(r[5], r[5], fma(r[4], r[4], fma(r[3], r[3], fma(r[2], r[2], fma(r[1], r[1], r[0] * r[0]))))));
}

// anchor prior at node P with mean P0: pose_prior plus log s - log s0.  Cost, and when JAC the error and the Jacobians into
// anc = {e[7], Jw[9], Jv[9]}: Jv = s R0^T R under t + s R dv; the scale's own Jacobian is 1 and nothing else couples to it.
template <bool JAC>
__device__ __forceinline__ double s3_anchor_eval(const S3Cfg &cfg, const double *P0, const double *P, double *anc)
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
    const double es = log(P[12]) - log(P0[12]);
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            anc[k] = e[k];
        anc[6] = es;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            anc[7 + k] = Jw[k];
            anc[16 + k] = P[12] * Jv[k];
        }
    }
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        c = c + (e[k] * e[k]) * cfg.w_anchor[k / 3];
    return c + (es * es) * cfg.w_anchor[2];
}
// entry (i, j) of the prior's block of H and entry i of its gradient, from anc
__device__ __forceinline__ double s3_anchor_h(const S3Cfg &cfg, const double *anc, int i, int j)
{
    if (i == 6 || j == 6)
        return i == j ? cfg.w_anchor[2] : 0.0;
    if ((i < 3) != (j < 3))
        return 0.0;
    const double *J = anc + (i < 3 ? 7 : 16);
    const double w = i < 3 ? cfg.w_anchor[0] : cfg.w_anchor[1];
    const int a = i % 3, c = j % 3;
    return (J[a] * w * J[c] + J[3 + a] * w * J[3 + c]) + J[6 + a] * w * J[6 + c];
}
__device__ __forceinline__ double s3_anchor_g(const S3Cfg &cfg, const double *anc, int i)
{
    if (i == 6)
        return cfg.w_anchor[2] * anc[6];
    const double *J = anc + (i < 3 ? 7 : 16), *e = anc + (i < 3 ? 0 : 3);
    const double w = i < 3 ? cfg.w_anchor[0] : cfg.w_anchor[1];
    const int a = i % 3;
    return (J[a] * w * e[0] + J[3 + a] * w * e[1]) + J[6 + a] * w * e[2];
}

// R <- R Exp(dw), t <- t + s R dv, s <- s exp(ds)
__device__ __forceinline__ void s3_retract(const double *P, const double *dx, double *Pn)
{
    const double dw[3] = {dx[0], dx[1], dx[2]};
    const double s = P[12];
    double E[9];
    so3_exp(dw, E);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            Pn[3 * r + c] = (P[3 * r] * E[c] + P[3 * r + 1] * E[3 + c]) + P[3 * r + 2] * E[6 + c];
        Pn[9 + r] = P[9 + r] + s * ((P[3 * r] * dx[3] + P[3 * r + 1] * dx[4]) + P[3 * r + 2] * dx[5]);
    }
    Pn[12] = s * exp(dx[6]);
}

// fixed-order sum over the workgroup (4 wavefronts): xor butterfly inside each wavefront, then (w0 + w1) + (w2 + w3).
// Every thread returns the same bits.
__device__ __forceinline__ double s3_block_sum(double x, double *red)
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

__device__ __forceinline__ void s3_zero_result(mvs_pose_graph_result *out)
{
    out->ok = 0, out->iterations = 0, out->cg_iterations = 0, out->rejected_steps = 0;
    out->error_initial = 0.0, out->error = 0.0;
}

// ---- dense path -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kS3Threads) void s3_dense_kernel(S3DenseDev d)
{
    __shared__ double H[kS3Dim * (kS3Dim + 1) / 2];
    __shared__ double gv[kS3Dim], yv[kS3Dim], dg[kS3Dim], inv[kS3Dim];
    __shared__ double node[2][kS3DenseMaxNodes * kS3Node];
    __shared__ double anc[26];
    __shared__ double red[4];
    const PgProblem P = d.prob[blockIdx.x];
    const S3Cfg &cfg = d.cfg;
    const int N = P.n_nodes, E = P.n_edges, n = 7 * N, tid = threadIdx.x;
    mvs_pose_graph_result *out = d.out + blockIdx.x;
    if (N < 1 || N > kS3DenseMaxNodes || E < 0 || P.anchor < 0 || P.anchor >= N) {   // the host never sends such a graph
        if (tid == 0)
            s3_zero_result(out);
        return;
    }
    const int32_t *src = d.edge_src + P.edge_off, *dst = d.edge_dst + P.edge_off;
    const double *Z = d.edge_z + kS3Node * P.edge_off, *cov = d.edge_cov + kS3Cov * P.edge_off;
    const double *node0 = d.node + kS3Node * P.node_off;
    double *W = d.W + kS3W * P.edge_off, *lin = d.lin + (int64_t)kS3Lin * P.edge_off;

    for (int i = tid; i < kS3Node * N; i += kS3Threads)
        node[0][i] = node0[i];
    int bad = 0;
    for (int k = tid; k < E; k += kS3Threads) {
        const int s = src[k], t = dst[k];
        if (s < 0 || s >= N || t < 0 || t >= N || s == t || !s3_edge_prep(cov + kS3Cov * (int64_t)k, W + kS3W * (int64_t)k))
            bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0)
            s3_zero_result(out);
        return;
    }

    // sum of the squared whitened residuals at ps (an LDS node table), the same bits in every thread
    auto cost_at = [&](const double *ps) -> double {
        double c = 0.0;
        for (int k = tid; k < E; k += kS3Threads) {
            double r[7];
            s3_edge_eval<false>(Z + kS3Node * (int64_t)k, W + kS3W * (int64_t)k, ps + kS3Node * src[k], ps + kS3Node * dst[k], r,
                                nullptr);
            c = c + sq7(r);
        }
        return s3_block_sum(c, red) +
               s3_anchor_eval<false>(cfg, node0 + kS3Node * P.anchor, ps + kS3Node * P.anchor, nullptr);
    };

    int cb = 0;
    double cur = cost_at(node[0]);
    const double cost0 = cur;
    double lam = cfg.lambda_initial;
    int it = 0, rejected = 0;
    const bool ok0 = cur < __builtin_inf() && cur == cur;
    while (ok0 && it < cfg.max_iterations) {
        const double *ps = node[cb];
        double *pn = node[cb ^ 1];
        // linearise: every edge's whitened residual and Jacobians, parked in global memory
        for (int k = tid; k < E; k += kS3Threads) {
            double r[7];
            s3_edge_eval<true>(Z + kS3Node * (int64_t)k, W + kS3W * (int64_t)k, ps + kS3Node * src[k], ps + kS3Node * dst[k], r,
                               lin + (int64_t)kS3Lin * k);
        }
        if (tid == 0)
            s3_anchor_eval<true>(cfg, node0 + kS3Node * P.anchor, ps + kS3Node * P.anchor, anc);
        __syncthreads();
        // H (lower triangle) and the right-hand side -g: one thread per entry, edges in edge order
        for (int idx = tid; idx < n * n; idx += kS3Threads) {
            const int row = idx / n, col = idx - row * n;
            if (col > row)
                continue;
            const int a = row / 7, i = row - 7 * a, b = col / 7, j = col - 7 * b;
            double acc = 0.0;
            for (int k = 0; k < E; ++k) {
                const int s = src[k], t = dst[k];
                const double *As = lin + (int64_t)kS3Lin * k + 7, *Ad = As + 49;
                if (a == b) {
                    if (s == a)
                        acc = acc + s3_coldot(As, i, As, j);
                    else if (t == a)
                        acc = acc + s3_coldot(Ad, i, Ad, j);
                } else if (s == a && t == b) {
                    acc = acc + s3_coldot(As, i, Ad, j);
                } else if (s == b && t == a) {
                    acc = acc + s3_coldot(Ad, i, As, j);
                }
            }
            if (a == b && a == P.anchor)
                acc = acc + s3_anchor_h(cfg, anc, i, j);
            if (row == col)
                acc = acc + lam;
            H[lidx(row, col)] = acc;
        }
        for (int row = tid; row < n; row += kS3Threads) {
            const int a = row / 7, i = row - 7 * a;
            double acc = 0.0;
            for (int k = 0; k < E; ++k) {
                const double *L = lin + (int64_t)kS3Lin * k;
                if (src[k] == a)
                    acc = acc + s3_colvec(L + 7, i, L);
                else if (dst[k] == a)
                    acc = acc + s3_colvec(L + 56, i, L);
            }
            if (a == P.anchor)
                acc = acc + s3_anchor_g(cfg, anc, i);
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
                s3_retract(ps + kS3Node * tid, gv + 7 * tid, pn + kS3Node * tid);
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
        double *po = d.nodes_out + kS3Node * P.node_off;
        for (int i = tid; i < kS3Node * N; i += kS3Threads)
            po[i] = node[cb][i];
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
__global__ __launch_bounds__(kS3Threads) void s3_prep_kernel(S3LargeDev d)
{
    const int k = blockIdx.x * kS3Threads + threadIdx.x;
    if (k == 0) {
        d.state->done = 0;
        d.state->cg_iters = 0;
    }
    if (k >= d.n_edges)
        return;
    if (!s3_edge_prep(d.edge_cov + kS3Cov * (int64_t)k, d.W + kS3W * (int64_t)k))
        d.state->bad_cov = 1;   // every writer stores the same word (the host zeroes it before the launch)
}

template <bool JAC>
__global__ __launch_bounds__(kS3Threads) void s3_edge_kernel(S3LargeDev d, const double *ps)
{
    const int k = blockIdx.x * kS3Threads + threadIdx.x;
    if (k >= d.n_edges)
        return;
    double r[7];
    s3_edge_eval<JAC>(d.edge_z + kS3Node * (int64_t)k, d.W + kS3W * (int64_t)k, ps + kS3Node * (int64_t)d.edge_src[k],
                      ps + kS3Node * (int64_t)d.edge_dst[k], r, JAC ? d.lin + (int64_t)kS3Lin * k : nullptr);
    if (!JAC)
        d.ecost[k] = sq7(r);
}

// sum of the edges' costs (thread t: edges t, t + 256, ... in order; then the workgroup tree) + the anchor -> *dst
__global__ __launch_bounds__(kS3Threads) void s3_cost_reduce_kernel(S3LargeDev d, const double *ps, double *dst)
{
    __shared__ double red[4];
    double c = 0.0;
    for (int k = threadIdx.x; k < d.n_edges; k += kS3Threads)
        c = c + d.ecost[k];
    const double tot = s3_block_sum(c, red) + s3_anchor_eval<false>(d.cfg, d.node0 + kS3Node * (int64_t)d.anchor,
                                                                    ps + kS3Node * (int64_t)d.anchor, nullptr);
    if (threadIdx.x == 0)
        *dst = tot;
}

// node i: diagonal block D_i = sum A^T A and gradient g_i = sum A^T r over its incident edges, in edge order
__global__ __launch_bounds__(64) void s3_gather_kernel(S3LargeDev d, const double *ps)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= d.n_nodes)
        return;
    double D[28], g[7];
#pragma unroll
    for (int k = 0; k < 28; ++k)
        D[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k)
        g[k] = 0.0;
    for (int c = d.csr_off[i]; c < d.csr_off[i + 1]; ++c) {
        const int code = d.csr_inc[c];
        const double *L = d.lin + (int64_t)kS3Lin * (code >> 1), *A = L + 7 + 49 * (code & 1);
#pragma unroll
        for (int a = 0; a < 7; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b)
                D[lidx(a, b)] = D[lidx(a, b)] + s3_coldot(A, a, A, b);
            g[a] = g[a] + s3_colvec(A, a, L);
        }
    }
    if (i == d.anchor) {
        double anc[26];
        s3_anchor_eval<true>(d.cfg, d.node0 + kS3Node * (int64_t)i, ps + kS3Node * (int64_t)i, anc);
#pragma unroll
        for (int a = 0; a < 7; ++a) {
#pragma unroll
            for (int b = 0; b < 7; ++b) {
                const double h = s3_anchor_h(d.cfg, anc, a, b);
                d.Ha[7 * a + b] = h;
                if (b <= a)
                    D[lidx(a, b)] = D[lidx(a, b)] + h;
            }
            g[a] = g[a] + s3_anchor_g(d.cfg, anc, a);
        }
    }
#pragma unroll
    for (int k = 0; k < 28; ++k)
        d.D[28 * (int64_t)i + k] = D[k];
#pragma unroll
    for (int k = 0; k < 7; ++k)
        d.g[7 * (int64_t)i + k] = g[k];
}

// PCG start (one workgroup): M_i = (D_i + lambda I)^-1 as Cholesky factors, x = 0, r = -g, z = M r, p = z
__global__ __launch_bounds__(kS3Threads) void s3_cg_init_kernel(S3LargeDev d, double lam)
{
    __shared__ double red[4];
    double rz = 0.0, rr = 0.0;
    int bad = 0;
    for (int i = threadIdx.x; i < d.n_nodes; i += kS3Threads) {
        double M[28], r[7], z[7];
#pragma unroll
        for (int k = 0; k < 28; ++k)
            M[k] = d.D[28 * (int64_t)i + k];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            M[lidx(k, k)] = M[lidx(k, k)] + lam;
            r[k] = -d.g[7 * (int64_t)i + k];
            z[k] = r[k];
        }
        if (!chol_packed<7>(M))
            bad = 1;
        chol_solve<7>(M, z);
#pragma unroll
        for (int k = 0; k < 28; ++k)
            d.Mf[28 * (int64_t)i + k] = M[k];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            d.x[7 * (int64_t)i + k] = 0.0;
            d.r[7 * (int64_t)i + k] = r[k];
            d.z[7 * (int64_t)i + k] = z[k];
            d.p[7 * (int64_t)i + k] = z[k];
            rz = fma(r[k], z[k], rz);
            rr = fma(r[k], r[k], rr);
        }
    }
    bad = __syncthreads_or(bad);
    rz = s3_block_sum(rz, red);
    rr = s3_block_sum(rr, red);
    if (threadIdx.x == 0) {
        d.state->rz = rz;
        d.state->gnorm2 = rr;
        d.state->rr = rr;
        d.state->cg_iters = 0;
        d.state->done = bad || !(rr == rr) || !(rr < __builtin_inf()) ? 2 : (rr == 0.0 ? 1 : 0);
    }
}

// u_k = A_src p_src + A_dst p_dst
__global__ __launch_bounds__(kS3Threads) void s3_edge_mv_kernel(S3LargeDev d)
{
    if (d.state->done)
        return;
    const int k = blockIdx.x * kS3Threads + threadIdx.x;
    if (k >= d.n_edges)
        return;
    const double *As = d.lin + (int64_t)kS3Lin * k + 7, *Ad = As + 49;
    const double *ps = d.p + 7 * (int64_t)d.edge_src[k], *pd = d.p + 7 * (int64_t)d.edge_dst[k];
#pragma unroll
    for (int m = 0; m < 7; ++m) {
        double s = As[7 * m] * ps[0];
#pragma unroll
        for (int i = 1; i < 7; ++i)
            s = fma(As[7 * m + i], ps[i], s);
#pragma unroll
        for (int i = 0; i < 7; ++i)
            s = fma(Ad[7 * m + i], pd[i], s);
        d.u[7 * (int64_t)k + m] = s;
    }
}

// q_i = sum A^T u over the incident edges (edge order) + prior block + lambda p_i;  pq_i = p_i . q_i
__global__ __launch_bounds__(64) void s3_node_mv_kernel(S3LargeDev d, double lam)
{
    if (d.state->done)
        return;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= d.n_nodes)
        return;
    double q[7], p[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        q[k] = 0.0;
        p[k] = d.p[7 * (int64_t)i + k];
    }
    for (int c = d.csr_off[i]; c < d.csr_off[i + 1]; ++c) {
        const int code = d.csr_inc[c];
        const double *A = d.lin + (int64_t)kS3Lin * (code >> 1) + 7 + 49 * (code & 1), *u = d.u + 7 * (int64_t)(code >> 1);
#pragma unroll
        for (int a = 0; a < 7; ++a)
            q[a] = q[a] + s3_colvec(A, a, u);
    }
    if (i == d.anchor) {
#pragma unroll
        for (int a = 0; a < 7; ++a) {
            double s = d.Ha[7 * a] * p[0];
#pragma unroll
            for (int b = 1; b < 7; ++b)
                s = fma(d.Ha[7 * a + b], p[b], s);
            q[a] = q[a] + s;
        }
    }
    double pq = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        q[k] = fma(lam, p[k], q[k]);
        d.q[7 * (int64_t)i + k] = q[k];
        pq = fma(p[k], q[k], pq);
    }
    d.pq[i] = pq;
}

// the rest of one PCG iteration (one workgroup): alpha, x, r, z, the stopping rule, beta, p
__global__ __launch_bounds__(kS3Threads) void s3_cg_step_kernel(S3LargeDev d)
{
    __shared__ double red[4];
    PgState *st = d.state;
    if (st->done)
        return;
    double s = 0.0;
    for (int i = threadIdx.x; i < d.n_nodes; i += kS3Threads)
        s = s + d.pq[i];
    const double pq = s3_block_sum(s, red);
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
    for (int i = threadIdx.x; i < d.n_nodes; i += kS3Threads) {
        double M[28], r[7], z[7];
#pragma unroll
        for (int k = 0; k < 28; ++k)
            M[k] = d.Mf[28 * (int64_t)i + k];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int64_t o = 7 * (int64_t)i + k;
            d.x[o] = fma(alpha, d.p[o], d.x[o]);
            r[k] = fma(-alpha, d.q[o], d.r[o]);
            d.r[o] = r[k];
            z[k] = r[k];
        }
        chol_solve<7>(M, z);
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            d.z[7 * (int64_t)i + k] = z[k];
            rzn = fma(r[k], z[k], rzn);
            rr = fma(r[k], r[k], rr);
        }
    }
    rzn = s3_block_sum(rzn, red);
    rr = s3_block_sum(rr, red);
    const bool conv = sqrt(rr) <= d.cfg.cg_rel_tol * sqrt(gn2);
    const bool broke = !(rr == rr) || !(rzn > 0.0);   // rzn = r^T M r = 0 only at r = 0, which conv has caught
    if (!conv && !broke) {
        const double beta = rzn / rz;
        for (int i = threadIdx.x; i < d.n_nodes; i += kS3Threads) {
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const int64_t o = 7 * (int64_t)i + k;
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

__global__ __launch_bounds__(64) void s3_update_kernel(S3LargeDev d, const double *ps, double *pn)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= d.n_nodes)
        return;
    s3_retract(ps + kS3Node * (int64_t)i, d.x + 7 * (int64_t)i, pn + kS3Node * (int64_t)i);
}

// thread k: node k (k < N) and edge k (k < E) of the lifted graph.  A kind outside 0 .. 2 is not one the library wrote: its
// scale variance becomes NaN, which no Cholesky accepts.
__global__ __launch_bounds__(kS3Threads) void s3_lift_kernel(S3LiftDev d)
{
    const int k = blockIdx.x * kS3Threads + threadIdx.x;
    if (k < d.n_nodes) {
        for (int i = 0; i < 12; ++i)
            d.node[kS3Node * (int64_t)k + i] = d.node_pose[12 * (int64_t)k + i];
        d.node[kS3Node * (int64_t)k + 12] = 1.0;
    }
    if (k < d.n_edges) {
        for (int i = 0; i < 12; ++i)
            d.edge_z[kS3Node * (int64_t)k + i] = d.edge_pose[12 * (int64_t)k + i];
        d.edge_z[kS3Node * (int64_t)k + 12] = 1.0;
        const int kind = d.edge_kind[k];
        const double sg = kind == 0 ? d.scale_sigma[0] : kind == 1 ? d.scale_sigma[1] : kind == 2 ? d.scale_sigma[2] : __builtin_nan("");
        double *C = d.cov + kS3Cov * (int64_t)k;
        for (int r = 0; r < 6; ++r) {
            for (int c = 0; c < 6; ++c)
                C[7 * r + c] = d.edge_cov[36 * (int64_t)k + 6 * r + c];
            C[7 * r + 6] = 0.0;
            C[42 + r] = 0.0;
        }
        C[48] = sg * sg;
    }
}

dim3 s3_edge_blocks(const S3LargeDev &d)
{
    const int eb = (d.n_edges + kS3Threads - 1) / kS3Threads;
    return dim3(eb > 0 ? eb : 1);
}

}  // namespace

void launch_s3_dense(const S3DenseDev &d, hipStream_t stream)
{
    if (d.n_problems <= 0)
        return;
    hipLaunchKernelGGL(s3_dense_kernel, dim3(d.n_problems), dim3(kS3Threads), 0, stream, d);
}

void launch_s3_prep(const S3LargeDev &d, hipStream_t stream)
{
    hipLaunchKernelGGL(s3_prep_kernel, s3_edge_blocks(d), dim3(kS3Threads), 0, stream, d);
}

void launch_s3_begin(const S3LargeDev &d, int cur, double lam, bool first, hipStream_t stream)
{
    const dim3 eb = s3_edge_blocks(d), nb((d.n_nodes + 63) / 64);
    const double *ps = d.node[cur];
    if (first) {
        hipLaunchKernelGGL(s3_edge_kernel<false>, eb, dim3(kS3Threads), 0, stream, d, ps);
        hipLaunchKernelGGL(s3_cost_reduce_kernel, dim3(1), dim3(kS3Threads), 0, stream, d, ps, &d.state->cost0);
    }
    hipLaunchKernelGGL(s3_edge_kernel<true>, eb, dim3(kS3Threads), 0, stream, d, ps);
    hipLaunchKernelGGL(s3_gather_kernel, nb, dim3(64), 0, stream, d, ps);
    hipLaunchKernelGGL(s3_cg_init_kernel, dim3(1), dim3(kS3Threads), 0, stream, d, lam);
}

void launch_s3_cg(const S3LargeDev &d, double lam, int n, hipStream_t stream)
{
    const dim3 eb = s3_edge_blocks(d), nb((d.n_nodes + 63) / 64);
    for (int c = 0; c < n; ++c) {
        hipLaunchKernelGGL(s3_edge_mv_kernel, eb, dim3(kS3Threads), 0, stream, d);
        hipLaunchKernelGGL(s3_node_mv_kernel, nb, dim3(64), 0, stream, d, lam);
        hipLaunchKernelGGL(s3_cg_step_kernel, dim3(1), dim3(kS3Threads), 0, stream, d);
    }
}

void launch_s3_end(const S3LargeDev &d, int cur, hipStream_t stream)
{
    const dim3 nb((d.n_nodes + 63) / 64);
    const double *ps = d.node[cur];
    double *pn = d.node[cur ^ 1];
    hipLaunchKernelGGL(s3_update_kernel, nb, dim3(64), 0, stream, d, ps, pn);
    hipLaunchKernelGGL(s3_edge_kernel<false>, s3_edge_blocks(d), dim3(kS3Threads), 0, stream, d, pn);
    hipLaunchKernelGGL(s3_cost_reduce_kernel, dim3(1), dim3(kS3Threads), 0, stream, d, pn, &d.state->cand);
}

void launch_s3_lift(const S3LiftDev &d, hipStream_t stream)
{
    const int n = d.n_nodes > d.n_edges ? d.n_nodes : d.n_edges;
    if (n <= 0)
        return;
    hipLaunchKernelGGL(s3_lift_kernel, dim3((n + kS3Threads - 1) / kS3Threads), dim3(kS3Threads), 0, stream, d);
}

}  // namespace mvs
