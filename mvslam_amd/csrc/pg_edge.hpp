// pg_edge.hpp -- one edge of a pose graph on the device: the whitening factor of its covariance, its whitened residual and
// Jacobians, and the column products the normal equations are gathered from.  posegraph.hip, pg_marginals.hip and
// pg_direct.hip include it, and nothing else does; device only, forced inline into an anonymous namespace like lm_math.hpp.
#pragma once
#include "lm_math.hpp"

namespace mvs {

namespace {

// whitening factor of one edge: S = L L^T, W = L^-1 (packed lower).  False if S (its lower triangle) is not positive
// definite; nothing is repaired.
__device__ __forceinline__ bool edge_prep(const double *cov, double *Wout)
{
    double S[21];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c)
            S[lidx(r, c)] = cov[6 * r + c];
    const bool ok = chol_packed<6>(S);
#pragma unroll
    for (int c = 0; c < 6; ++c) {   // column c of L^-1: forward substitution of the unit vector e_c
        double b[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < i; ++k)
                v = fma(-S[lidx(i, k)], b[k], v);
            b[i] = v * S[lidx(i, i)];
            if (i >= c)
                Wout[lidx(i, c)] = b[i];
        }
    }
    return ok;
}

// out = W v, W packed lower 6 x 6
__device__ __forceinline__ void whiten(const double (&W)[21], const double (&v)[6], double *out, int stride)
{
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        double s = W[lidx(m, 0)] * v[0];
#pragma unroll
        for (int c = 1; c <= m; ++c)
            s = fma(W[lidx(m, c)], v[c], s);
        out[m * stride] = s;
    }
}

// whitened residual of edge (Z, W) between (Rs, ts) and (Rd, td); when JAC, its whitened Jacobians too, written column by
// column so that no 6 x 6 block ever lives in registers: lin = {r[6], A_src[6][6], A_dst[6][6]} (row-major)
//   d e / d dst = [ Jr^-1(e_w)          0 ]      d e / d src = [ -Jr^-1(e_w) (Rs^T Rd)^T      0    ]
//                 [ 0                   E ]                    [  Rz^T [q]x                  -Rz^T ]
// with E = Rz^T Rs^T Rd and q = Rs^T (td - ts).
template <bool JAC>
__device__ __forceinline__ void edge_eval(const double *Zp, const double *Wp, const double *ps, const double *pd,
                                          double (&r)[6], double *lin)
{
    double Rz[9], W[21], Rsd[9], E[9], e[6];
#pragma unroll
    for (int k = 0; k < 9; ++k)
        Rz[k] = Zp[k];
#pragma unroll
    for (int k = 0; k < 21; ++k)
        W[k] = Wp[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Rsd[3 * i + j] = (ps[i] * pd[j] + ps[3 + i] * pd[3 + j]) + ps[6 + i] * pd[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            E[3 * i + j] = (Rz[i] * Rsd[j] + Rz[3 + i] * Rsd[3 + j]) + Rz[6 + i] * Rsd[6 + j];
    so3_log(E, e);
    const double d0 = pd[9] - ps[9], d1 = pd[10] - ps[10], d2 = pd[11] - ps[11];
    double q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        q[i] = (ps[i] * d0 + ps[3 + i] * d1) + ps[6 + i] * d2;
    const double m0 = q[0] - Zp[9], m1 = q[1] - Zp[10], m2 = q[2] - Zp[11];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        e[3 + i] = (Rz[i] * m0 + Rz[3 + i] * m1) + Rz[6 + i] * m2;
    whiten(W, e, r, 1);
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            lin[k] = r[k];
        double Jri[9];
        so3_jrinv(e, Jri);
        // [q]x by columns
        const double qx[3][3] = {{0.0, q[2], -q[1]}, {-q[2], 0.0, q[0]}, {q[1], -q[0], 0.0}};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double cs[6], cd[6];   // column i of d e / d src and d e / d dst
            if (i < 3) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    cs[c] = -((Jri[3 * c] * Rsd[3 * i] + Jri[3 * c + 1] * Rsd[3 * i + 1]) + Jri[3 * c + 2] * Rsd[3 * i + 2]);
                    cs[3 + c] = (Rz[c] * qx[i][0] + Rz[3 + c] * qx[i][1]) + Rz[6 + c] * qx[i][2];
                    cd[c] = Jri[3 * c + i];
                    cd[3 + c] = 0.0;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    cs[c] = 0.0;
                    cs[3 + c] = -Rz[3 * (i - 3) + c];
                    cd[c] = 0.0;
                    cd[3 + c] = E[3 * c + (i - 3)];
                }
            }
            whiten(W, cs, lin + 6 + i, 6);
            whiten(W, cd, lin + 42 + i, 6);
        }
    }
}

// column i of A . column j of B (A, B row-major 6 x 6)
__device__ __forceinline__ double coldot(const double *A, int i, const double *B, int j)
{
    double s = A[i] * B[j];
#pragma unroll
    for (int m = 1; m < 6; ++m)
        s = fma(A[6 * m + i], B[6 * m + j], s);
    return s;
}
// column i of A . r
__device__ __forceinline__ double colvec(const double *A, int i, const double *r)
{
    double s = A[i] * r[0];
#pragma unroll
    for (int m = 1; m < 6; ++m)
        s = fma(A[6 * m + i], r[m], s);
    return s;
}

}  // namespace

}  // namespace mvs
