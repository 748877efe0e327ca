// pg_direct.hip -- the direct linear solve of the large path's LM step: (H + lambda I) x = -g by a block-scaled skyline
// Cholesky on the device (include/mvslam_hip.h mvs_ctx_set_pose_graph_solver states the contract).
// Linearisation, the gather of the diagonal blocks D_i and the gradient g_i, the update and the cost are posegraph.hip's
// kernels as they are.  Four kernels here, in stream order:
//   pgd_scale_kernel     one thread per node: A_ii = D_i + lambda I = C_i C_i^T (chol_packed's statements), C_i^-1 by forward
//                        substitution of the unit vectors, right-hand side b_i = -C_i^-1 g_i.
//   pgd_assemble_kernel  one thread per entry of every block of the envelope: an off-diagonal block's terms summed in edge order
//                        (pg_envelope.hpp's lists, one owner per entry, no atomics), then C_i^-1 A_ij C_j^-T through LDS; a
//                        block no term touches is zero, a diagonal block the identity.
//   pgd_factor_kernel    ONE workgroup, block rows in order, right-looking inside the row as pgm_factor_kernel, with two
//                        changes: a diagonal block of the factor is stored as its explicit inverse, so Y_c = B_c L_cc^-T is 36
//                        independent dot products instead of six threads' substitutions, and Y_c is handed to the updates
//                        through LDS.  The right-hand side is one more column of the row: t_i -= L_ic y_c rides along with
//                        the updates of step c and y_i = L_ii^-1 t_i with the diagonal block, so the forward substitution adds
//                        no barrier.  A pivot that is not finite and positive writes the status word and leaves.
//   pgd_solve_kernel     ONE workgroup: rows in descending order, z_i = L_ii^-T y_i, then y_c -= L(i, c)^T z_i for every c of
//                        the row's envelope (one owner per entry, one row at a time); at the end x_i = C_i^-T z_i.
// Every kernel leaves at once when the status word is set.  Binary64, explicit FMAs, every sum in a fixed order.
// The sparse bundle adjustment (ba_sparse.hip; section 4.7.4) runs the same four kernels on a second source: PgdDev::pre holds
// the off-diagonal blocks already summed, D and g are its own, PgdDev::pivot_tol its pivot rule.  Both are zero for the pose
// graphs, whose statements and bytes are what they were.
//
// chol_packed is lm_math.hpp's and coldot pg_edge.hpp's, shared with the other solvers.
#include "pg_edge.hpp"

namespace mvs {

namespace {

constexpr int kPgdThreads = 256;
constexpr int kPgdPerWg = 7;   // blocks of the envelope one workgroup of pgd_assemble_kernel owns: 7 * 36 = 252 threads

// W = L^-1 (packed lower) of the factor chol_packed left in S: column c by forward substitution of the unit vector e_c
__device__ __forceinline__ void tri_inverse(const double (&S)[21], double (&W)[21])
{
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double b[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < i; ++k)
                v = fma(-S[lidx(i, k)], b[k], v);
            b[i] = v * S[lidx(i, i)];
            if (i >= c)
                W[lidx(i, c)] = b[i];
        }
    }
}

// ---- scaling of the diagonal ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pgd_scale_kernel(PgdDev d, double lam)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= d.n_nodes)
        return;
    double S[21], W[21], g[6];
#pragma unroll
    for (int k = 0; k < 21; ++k)
        S[k] = d.D[21 * (int64_t)i + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        S[lidx(k, k)] = S[lidx(k, k)] + lam;
        g[k] = d.g[6 * (int64_t)i + k];
    }
    if (!chol_packed<6>(S)) {
        d.state->status = 2;   // every writer stores the same word (the host clears it before the launch)
        atomicMax(&d.state->bad_code, d.n_nodes - i);
    }
    tri_inverse(S, W);
#pragma unroll
    for (int k = 0; k < 21; ++k)
        d.Cinv[21 * (int64_t)i + k] = W[k];
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        double s = W[lidx(m, 0)] * g[0];
#pragma unroll
        for (int c = 1; c <= m; ++c)
            s = fma(W[lidx(m, c)], g[c], s);
        d.y[6 * (int64_t)i + m] = -s;
    }
}

// ---- assembly of the scaled matrix ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgdThreads) void pgd_assemble_kernel(PgdDev d)
{
    __shared__ double A[kPgdPerWg][36], T[kPgdPerWg][36];
    if (d.state->status)   // uniform
        return;
    const int tid = threadIdx.x, lb = tid / 36, e = tid - 36 * lb, a = e / 6, c = e - 6 * a;
    const int64_t b = (int64_t)blockIdx.x * kPgdPerWg + lb;
    const bool on = lb < kPgdPerWg && b < d.n_blocks;
    int i = 0, j = 0;
    bool off = false;   // an off-diagonal block some term touches
    if (on) {
        i = d.blk_row[b];
        j = d.first[i] + (int)(b - d.row_off[i]);
        const int slot = d.pre ? -1 : d.blk_slot[b];
        off = i != j && (d.pre || slot >= 0);
        if (off && d.pre) {   // the second source: the block has been summed already
            A[lb][e] = d.pre[36 * b + e];
        } else if (off) {
            double acc = 0.0;
            for (int t = d.slot_off[slot]; t < d.slot_off[slot + 1]; ++t) {
                const int code = d.codes[t];
                if (code < 0)   // the anchor's term: a diagonal block's, never here
                    continue;
                const double *As = d.lin + (int64_t)kPgLin * (code >> 2) + 6, *Ad = As + 36;
                const int kind = code & 3;
                const double *Ar = (kind == 0 || kind == 2) ? As : Ad;   // the row's Jacobian
                const double *Ac = (kind == 0 || kind == 3) ? As : Ad;   // the column's
                acc = acc + coldot(Ar, a, Ac, c);
            }
            A[lb][e] = acc;
        }
    }
    __syncthreads();
    if (off) {   // T = C_i^-1 A
        const double *Ci = d.Cinv + 21 * (int64_t)i;
        double t = Ci[lidx(a, 0)] * A[lb][c];
        for (int p = 1; p <= a; ++p)
            t = fma(Ci[lidx(a, p)], A[lb][6 * p + c], t);
        T[lb][e] = t;
    }
    __syncthreads();
    if (!on)
        return;
    double v = (i == j && a == c) ? 1.0 : 0.0;
    if (off) {   // T C_j^-T
        const double *Cj = d.Cinv + 21 * (int64_t)j;
        v = T[lb][6 * a] * Cj[lidx(c, 0)];
        for (int q = 1; q <= c; ++q)
            v = fma(T[lb][6 * a + q], Cj[lidx(c, q)], v);
    }
    d.sky[36 * b + e] = v;
}

// ---- factorisation, with the forward substitution ---------------------------------------------------------------------------
__global__ __launch_bounds__(kPgdThreads) void pgd_factor_kernel(PgdDev d)
{
    __shared__ double Yc[36];
    __shared__ int fail;
    PgdState *st = d.state;
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
        double *ti = d.y + 6 * (int64_t)i;
        for (int c = f; c < i; ++c) {
            double *B = row + 36 * (c - f);
            // Y_c = B L_cc^-T: entry (m, q) = sum over p <= q of B[m][p] L_cc^-1[q][p]
            if (tid < 36) {
                const double *Li = d.sky + 36 * ((int64_t)d.row_off[c] + (c - d.first[c]));
                const int m = tid / 6, q = tid - 6 * m;
                double v = B[6 * m] * Li[6 * q];
                for (int p = 1; p <= q; ++p)
                    v = fma(B[6 * m + p], Li[6 * q + p], v);
                Yc[tid] = v;
            }
            __syncthreads();
            if (tid < 36)
                B[tid] = Yc[tid];
            // every later block c' of the row whose own row reaches back to c: Y_c' -= Y_c L(c', c)^T; the diagonal block
            // (c' = i) takes Y_c Y_c^T; the right-hand side takes Y_c y_c
            const int blk_items = (i - c) * 36, items = blk_items + 6;
            for (int it = tid; it < items; it += kPgdThreads) {
                if (it >= blk_items) {
                    const int m = it - blk_items;
                    const double *yc = d.y + 6 * (int64_t)c;
                    double v = ti[m];
#pragma unroll
                    for (int t = 0; t < 6; ++t)
                        v = fma(-Yc[6 * m + t], yc[t], v);
                    ti[m] = v;
                    continue;
                }
                const int cp = c + 1 + it / 36, e = it % 36, m = e / 6, q = e - 6 * m;
                const int fc = d.first[cp];
                if (fc > c)
                    continue;
                const double *M = cp < i ? d.sky + 36 * ((int64_t)d.row_off[cp] + (c - fc)) : Yc;
                double *Tp = row + 36 * (cp - f) + e;
                double v = *Tp;
#pragma unroll
                for (int t = 0; t < 6; ++t)
                    v = fma(-Yc[6 * m + t], M[6 * q + t], v);
                *Tp = v;
            }
            __syncthreads();
        }
        if (tid == 0) {
            double *Dg = row + 36 * (i - f);
            double S[21], W[21];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c)
                    S[lidx(r, c)] = Dg[6 * r + c];
            const bool ok = chol_packed<6>(S, min_d) && min_d > d.pivot_tol;   // 0 for the pose graphs: chol_packed's own rule
            tri_inverse(S, W);
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    Dg[6 * r + c] = c <= r ? W[lidx(r, c)] : 0.0;
            double yv[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) {   // y_i = L_ii^-1 t_i
                double s = W[lidx(m, 0)] * ti[0];
#pragma unroll
                for (int c = 1; c <= m; ++c)
                    s = fma(W[lidx(m, c)], ti[c], s);
                yv[m] = s;
            }
#pragma unroll
            for (int m = 0; m < 6; ++m)
                ti[m] = yv[m];
            if (!ok) {
                fail = 1;
                st->status = 3;
                st->bad_code = N - i;
            }
        }
        __syncthreads();
        if (fail)   // uniform
            break;
    }
    if (tid == 0)
        st->min_d = min_d;
}

// ---- back substitution and unscaling ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgdThreads) void pgd_solve_kernel(PgdDev d)
{
    __shared__ double zc[6];
    if (d.state->status)
        return;
    const int tid = threadIdx.x, N = d.n_nodes;
    for (int i = N - 1; i >= 0; --i) {
        const int f = d.first[i];
        const double *row = d.sky + 36 * (int64_t)d.row_off[i];
        double *yi = d.y + 6 * (int64_t)i;
        if (tid < 6) {   // z_i = L_ii^-T y_i: entry m sums over p >= m
            const double *Li = row + 36 * (i - f);
            double s = Li[6 * tid + tid] * yi[tid];
            for (int p = tid + 1; p < 6; ++p)
                s = fma(Li[6 * p + tid], yi[p], s);
            zc[tid] = s;
        }
        __syncthreads();
        if (tid < 6)
            yi[tid] = zc[tid];
        const int items = (i - f) * 6;
        for (int it = tid; it < items; it += kPgdThreads) {   // y_c -= L(i, c)^T z_i
            const int c = it / 6, m = it - 6 * c;
            const double *Lb = row + 36 * c;
            double *yc = d.y + 6 * (int64_t)(f + c);
            double v = yc[m];
#pragma unroll
            for (int t = 0; t < 6; ++t)
                v = fma(-Lb[6 * t + m], zc[t], v);
            yc[m] = v;
        }
        __syncthreads();
    }
    for (int it = tid; it < 6 * N; it += kPgdThreads) {   // x_n = C_n^-T z_n
        const int n = it / 6, m = it - 6 * n;
        const double *Cn = d.Cinv + 21 * (int64_t)n, *z = d.y + 6 * (int64_t)n;
        double s = Cn[lidx(m, m)] * z[m];
        for (int p = m + 1; p < 6; ++p)
            s = fma(Cn[lidx(p, m)], z[p], s);
        d.x[it] = s;
    }
}

}  // namespace

void launch_pgd_step(const PgdDev &d, double lam, hipStream_t stream)
{
    hipLaunchKernelGGL(pgd_scale_kernel, dim3((d.n_nodes + 63) / 64), dim3(64), 0, stream, d, lam);
    const int ab = (d.n_blocks + kPgdPerWg - 1) / kPgdPerWg;
    hipLaunchKernelGGL(pgd_assemble_kernel, dim3(ab), dim3(kPgdThreads), 0, stream, d);
    hipLaunchKernelGGL(pgd_factor_kernel, dim3(1), dim3(kPgdThreads), 0, stream, d);
    hipLaunchKernelGGL(pgd_solve_kernel, dim3(1), dim3(kPgdThreads), 0, stream, d);
}

}  // namespace mvs
