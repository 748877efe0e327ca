// pg_marginals.hip -- marginal covariances of a pose graph: Sigma = H^-1 at given poses, from a block-skyline Cholesky of H
// on the device (include/mvslam_hip.h mvs_pose_graph_marginals states the contract).
//   H = J_a^T W_a J_a + sum_k J_k^T W_k J_k,  no lambda; residuals, Jacobians, tangent order, right perturbation and
//   whitening are posegraph.hip's.
// Four kernels, in stream order:
//   pgm_lin_kernel     one thread per edge: whitening factor of its covariance and the whitened Jacobians at X; one more
//                      thread for the anchor prior's block.
//   pgm_gather_kernel  one thread per entry of every block of H some term touches: the block's terms summed in edge order
//                      (the host's per-block lists), the anchor's last.  One owner per entry, no atomics.
//   pgm_factor_kernel  ONE workgroup: block rows in order.  Row i is solved column block by column block: Y_c <- Y_c L_cc^-T
//                      (six threads, one per row of the block), then every later block of the row takes its update
//                      Y_c' -= Y_c L(c', c)^T in parallel -- each entry sums over c ascending, a fixed order with no partial
//                      sums to combine -- and the diagonal block is factorised by chol_packed's statements.  Fill stays
//                      inside the row's envelope.  A pivot that is not finite and positive writes the status word and leaves.
//   pgm_solve_kernel   one workgroup per query (i, j): L y = E for the 6 (i = j) or 12 columns from row min(i, j) down, y
//                      kept in the workspace, the 36 sums over rows >= max(i, j) accumulated in row order.  No back
//                      substitution.  A column's bits depend on its node alone, so a block's bytes do not depend on the
//                      other queries, and Sigma_ji is the byte transpose of Sigma_ij.
// Every kernel leaves at once when the status word is set.
//
// The prior and Cholesky functions are lm_math.hpp's and the edge functions pg_edge.hpp's, shared with the other solvers.
#include "pg_edge.hpp"

namespace mvs {

namespace {

constexpr int kPgmThreads = 256;
constexpr int kPgmY = 72;   // doubles of one block row of y: 6 rows x 12 columns

// the anchor prior's block of H at pose P with mean P0: entry (i, j) as posegraph.hip's anchor_h
__device__ __forceinline__ void anchor_block(const double (&w)[2], const double *P0, const double *P, double *Ha)
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
    pose_prior<true>(R0, t0, R, t, e, Jw, Jv);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double h = 0.0;
            if ((i < 3) == (j < 3)) {
                const double *J = i < 3 ? Jw : Jv;
                const double wt = i < 3 ? w[0] : w[1];
                const int a = i % 3, c = j % 3;
                h = (J[a] * wt * J[c] + J[3 + a] * wt * J[3 + c]) + J[6 + a] * wt * J[6 + c];
            }
            Ha[6 * i + j] = h;
        }
}

// ---- assembly -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgmThreads) void pgm_lin_kernel(PgmDev d)
{
    const int k = blockIdx.x * kPgmThreads + threadIdx.x;
    if (k == d.n_edges) {
        const double w[2] = {d.w_anchor[0], d.w_anchor[1]};
        anchor_block(w, d.pose0 + 12 * (int64_t)d.anchor, d.X + 12 * (int64_t)d.anchor, d.Ha);
    }
    if (k >= d.n_edges)
        return;
    double W[21], r[6];
    if (!edge_prep(d.edge_cov + 36 * (int64_t)k, W))
        d.state->status = 1;   // every writer stores the same word (the host clears it before the launch)
    edge_eval<true>(d.edge_pose + 12 * (int64_t)k, W, d.X + 12 * (int64_t)d.edge_src[k], d.X + 12 * (int64_t)d.edge_dst[k], r,
                    d.lin + (int64_t)kPgLin * k);
}

__global__ __launch_bounds__(kPgmThreads) void pgm_gather_kernel(PgmDev d)
{
    if (d.state->status)
        return;
    const int gid = blockIdx.x * kPgmThreads + threadIdx.x;
    const int slot = gid / 36, e = gid - 36 * slot;
    if (slot >= d.n_slots)
        return;
    const int a = e / 6, b = e - 6 * a;
    double acc = 0.0;
    for (int c = d.slot_off[slot]; c < d.slot_off[slot + 1]; ++c) {
        const int code = d.codes[c];
        if (code < 0) {
            acc = acc + d.Ha[e];
            continue;
        }
        const double *As = d.lin + (int64_t)kPgLin * (code >> 2) + 6, *Ad = As + 36;
        const int kind = code & 3;
        const double *Ar = (kind == 0 || kind == 2) ? As : Ad;   // the row's Jacobian
        const double *Ac = (kind == 0 || kind == 3) ? As : Ad;   // the column's
        acc = acc + coldot(Ar, a, Ac, b);
    }
    d.sky[36 * (int64_t)d.slot_blk[slot] + e] = acc;
}

// ---- factorisation --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgmThreads) void pgm_factor_kernel(PgmDev d)
{
    __shared__ int fail;
    PgmState *st = d.state;
    if (st->status)
        return;
    const int tid = threadIdx.x, N = d.n_nodes;
    if (tid == 0)
        fail = 0;
    double min_d = __builtin_inf();   // thread 0's
    __syncthreads();
    for (int i = 0; i < N; ++i) {
        const int f = d.first[i];
        double *row = d.sky + 36 * (int64_t)d.row_off[i];   // block (i, c) at row + 36 (c - f)
        for (int c = f; c < i; ++c) {
            double *Yc = row + 36 * (c - f);
            // Y_c <- Y_c L_cc^-T: thread m owns row m of the block
            if (tid < 6) {
                const double *Lcc = d.sky + 36 * ((int64_t)d.row_off[c] + (c - d.first[c]));
                double x[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    double v = Yc[6 * tid + q];
#pragma unroll
                    for (int p = 0; p < q; ++p)
                        v = fma(-x[p], Lcc[6 * q + p], v);
                    x[q] = v * Lcc[7 * q];
                }
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    Yc[6 * tid + q] = x[q];
            }
            __syncthreads();
            // every later block c' of the row whose own row reaches back to c: Y_c' -= Y_c L(c', c)^T; the diagonal block
            // (c' = i) takes Y_c Y_c^T
            const int items = (i - c) * 36;
            for (int it = tid; it < items; it += kPgmThreads) {
                const int cp = c + 1 + it / 36, e = it % 36, m = e / 6, q = e - 6 * m;
                const int fc = d.first[cp];
                if (fc > c)
                    continue;
                const double *M = cp < i ? d.sky + 36 * ((int64_t)d.row_off[cp] + (c - fc)) : Yc;
                double *T = row + 36 * (cp - f) + e;
                double v = *T;
#pragma unroll
                for (int t = 0; t < 6; ++t)
                    v = fma(-Yc[6 * m + t], M[6 * q + t], v);
                *T = v;
            }
            __syncthreads();
        }
        if (tid == 0) {
            double *D = row + 36 * (i - f);
            double S[21];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c)
                    S[lidx(r, c)] = D[6 * r + c];
            const bool ok = chol_packed<6>(S, min_d);
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    D[6 * r + c] = c <= r ? S[lidx(r, c)] : 0.0;
            if (!ok) {
                fail = 1;
                st->status = 2;
                st->bad_node = i;
            }
        }
        __syncthreads();
        if (fail)   // uniform
            break;
    }
    if (tid == 0)
        st->min_d = min_d;
}

// ---- solves -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgmThreads) void pgm_solve_kernel(PgmDev d)
{
    __shared__ double part[3][kPgmY];
    __shared__ double ycur[kPgmY];
    if (d.state->status)
        return;
    const int qn = blockIdx.x, tid = threadIdx.x, N = d.n_nodes;
    const int qi = d.qi[qn], qj = d.qj[qn];
    const int lo = qi < qj ? qi : qj, hi = qi < qj ? qj : qi;
    double *y = d.y + (int64_t)qn * N * kPgmY;   // block row r at y + 72 r: [6][12], columns 0-5 node lo, 6-11 node hi
    // dot products: thread (p, m, col) sums the blocks k = k0 + p, k0 + p + 3, ... of entry (m, col)
    const int p = tid / kPgmY, e = tid - kPgmY * p, m = e / 12, col = e - 12 * m;
    const int node = col < 6 ? lo : hi;
    const bool col_on = col < 6 || hi != lo;
    // sums: thread (a, b) < 36 owns entry (a, b) of the block
    const int a = tid / 6, b = tid - 6 * a;
    const int ca = (qi == lo ? 0 : 6) + a, cb = (qj == lo ? 0 : 6) + b;
    double acc = 0.0;
    for (int r = lo; r < N; ++r) {
        const int f = d.first[r];
        const double *Lrow = d.sky + 36 * (int64_t)d.row_off[r];   // block (r, k) at Lrow + 36 (k - f)
        if (tid < 3 * kPgmY) {
            double s = 0.0;
            if (col_on && r > node) {
                const int k0 = f > node ? f : node;
                for (int k = k0 + p; k < r; k += 3) {
                    const double *Lb = Lrow + 36 * (k - f) + 6 * m;
                    const double *yk = y + (int64_t)kPgmY * k + col;
#pragma unroll
                    for (int t = 0; t < 6; ++t)
                        s = fma(Lb[t], yk[12 * t], s);
                }
            }
            part[p][e] = s;
        }
        __syncthreads();
        if (tid < 12) {   // column tid of the block row: the 6 x 6 forward substitution with L_rr
            const int nd = tid < 6 ? lo : hi;
            const bool on = (tid < 6 || hi != lo) && r >= nd;
            const double *Lrr = Lrow + 36 * (r - f);
            double yv[6];
#pragma unroll
            for (int mm = 0; mm < 6; ++mm) {
                double v = (r == nd && mm == tid % 6) ? 1.0 : 0.0;
                v = v - ((part[0][12 * mm + tid] + part[1][12 * mm + tid]) + part[2][12 * mm + tid]);
#pragma unroll
                for (int t = 0; t < mm; ++t)
                    v = fma(-Lrr[6 * mm + t], yv[t], v);
                yv[mm] = on ? v * Lrr[7 * mm] : 0.0;
            }
#pragma unroll
            for (int mm = 0; mm < 6; ++mm) {
                ycur[12 * mm + tid] = yv[mm];
                y[(int64_t)kPgmY * r + 12 * mm + tid] = yv[mm];
            }
        }
        __syncthreads();
        if (tid < 36 && r >= hi) {
#pragma unroll
            for (int mm = 0; mm < 6; ++mm)
                acc = fma(ycur[12 * mm + ca], ycur[12 * mm + cb], acc);
        }
    }
    if (tid < 36)
        d.out[36 * (int64_t)qn + tid] = acc;
}

}  // namespace

void launch_pgm_assemble(const PgmDev &d, hipStream_t stream)
{
    const int eb = (d.n_edges + 1 + kPgmThreads - 1) / kPgmThreads;
    hipLaunchKernelGGL(pgm_lin_kernel, dim3(eb), dim3(kPgmThreads), 0, stream, d);
    const int gb = (int)(((int64_t)d.n_slots * 36 + kPgmThreads - 1) / kPgmThreads);
    hipLaunchKernelGGL(pgm_gather_kernel, dim3(gb), dim3(kPgmThreads), 0, stream, d);
}

void launch_pgm_factor(const PgmDev &d, hipStream_t stream)
{
    hipLaunchKernelGGL(pgm_factor_kernel, dim3(1), dim3(kPgmThreads), 0, stream, d);
}

void launch_pgm_solve(const PgmDev &d, int n_query, hipStream_t stream)
{
    if (n_query <= 0)
        return;
    hipLaunchKernelGGL(pgm_solve_kernel, dim3(n_query), dim3(kPgmThreads), 0, stream, d);
}

}  // namespace mvs
