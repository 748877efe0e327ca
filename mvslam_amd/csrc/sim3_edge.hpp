// sim3_edge.hpp -- one edge of a pose graph over Sim(3) on the device: the whitening factor of its
// 7 x 7 covariance, its whitened residual and Jacobians, and the column products the normal equations are gathered from.
// sim3graph.hip includes it, and nothing else does; device only, forced inline into an anonymous namespace like pg_edge.hpp,
// whose 6 x 6 statements these are with the scale's row and column added: with every scale 1 the shared terms are the same
// operations on the same operands in the same order.
#pragma once
#include "lm_math.hpp"

namespace mvs {

namespace {

// whitening factor of one edge: S = L L^T, W = L^-1 (packed lower, 28).  False if S (its lower triangle) is not positive
// definite; nothing is repaired.
__device__ __forceinline__ bool s3_edge_prep(const double *cov, double *Wout)
{
    double S[28];
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c)
            S[lidx(r, c)] = cov[7 * r + c];
    const bool ok = chol_packed<7>(S);
#pragma unroll
    for (int c = 0; c < 7; ++c) {   // column c of L^-1: forward substitution of the unit vector e_c
        double b[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
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

// out = W v, W packed lower 7 x 7
__device__ __forceinline__ void s3_whiten(const double (&W)[28], const double (&v)[7], double *out, int stride)
{
#pragma unroll
    for (int m = 0; m < 7; ++m) {
        double s = W[lidx(m, 0)] * v[0];
#pragma unroll
        for (int c = 1; c <= m; ++c)
            s = fma(W[lidx(m, c)], v[c], s);
        out[m * stride] = s;
    }
}

// whitened residual of edge (Z = (Rz, tz, sz), W) between the nodes ps = (Rs, ts, ss) and pd = (Rd, td, sd); when JAC, its
// whitened Jacobians too, written column by column so that no 7 x 7 block ever lives in registers:
// lin = {r[7], A_src[7][7], A_dst[7][7]} (row-major).  With E = Rz^T Rs^T Rd and q = Rs^T (td - ts) / ss,
//   e = ( Log(E),  Rz^T (q - tz),  log sd - log ss - log sz )
//   d e / d dst = [ Jr^-1(e_w)   0            0 ]      d e / d src = [ -Jr^-1(e_w) (Rs^T Rd)^T    0      0      ]
//                 [ 0            (sd / ss) E  0 ]                    [  Rz^T [q]x                -Rz^T  -Rz^T q ]
//                 [ 0            0            1 ]                    [  0                         0     -1      ]
// columns in the tangent order (rotation, translation, log-scale) of the update R Exp(dw), t + s R dv, s exp(ds).
template <bool JAC>
__device__ __forceinline__ void s3_edge_eval(const double *Zp, const double *Wp, const double *ps, const double *pd,
                                             double (&r)[7], double *lin)
{
    double Rz[9], W[28], Rsd[9], E[9], e6[6], e[7];
#pragma unroll
    for (int k = 0; k < 9; ++k)
        Rz[k] = Zp[k];
#pragma unroll
    for (int k = 0; k < 28; ++k)
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
    so3_log(E, e6);
    const double ss = ps[12], sd = pd[12];
    const double d0 = pd[9] - ps[9], d1 = pd[10] - ps[10], d2 = pd[11] - ps[11];
    double q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        q[i] = ((ps[i] * d0 + ps[3 + i] * d1) + ps[6 + i] * d2) / ss;
    const double m0 = q[0] - Zp[9], m1 = q[1] - Zp[10], m2 = q[2] - Zp[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        e[i] = e6[i];
        e[3 + i] = (Rz[i] * m0 + Rz[3 + i] * m1) + Rz[6 + i] * m2;
    }
    e[6] = (log(sd) - log(ss)) - log(Zp[12]);
    s3_whiten(W, e, r, 1);
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
            lin[k] = r[k];
        double Jri[9];
        so3_jrinv(e6, Jri);
        const double ratio = sd / ss;
        // [q]x by columns
        const double qx[3][3] = {{0.0, q[2], -q[1]}, {-q[2], 0.0, q[0]}, {q[1], -q[0], 0.0}};
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            double cs[7], cd[7];   // column i of d e / d src and d e / d dst
            if (i < 3) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    cs[c] = -((Jri[3 * c] * Rsd[3 * i] + Jri[3 * c + 1] * Rsd[3 * i + 1]) + Jri[3 * c + 2] * Rsd[3 * i + 2]);
                    cs[3 + c] = (Rz[c] * qx[i][0] + Rz[3 + c] * qx[i][1]) + Rz[6 + c] * qx[i][2];
                    cd[c] = Jri[3 * c + i];
                    cd[3 + c] = 0.0;
                }
                cs[6] = 0.0;
                cd[6] = 0.0;
            } else if (i < 6) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    cs[c] = 0.0;
                    cs[3 + c] = -Rz[3 * (i - 3) + c];
                    cd[c] = 0.0;
                    cd[3 + c] = ratio * E[3 * c + (i - 3)];
                }
                cs[6] = 0.0;
                cd[6] = 0.0;
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    cs[c] = 0.0;
                    cs[3 + c] = -((Rz[c] * q[0] + Rz[3 + c] * q[1]) + Rz[6 + c] * q[2]);
                    cd[c] = 0.0;
                    cd[3 + c] = 0.0;
                }
                cs[6] = -1.0;
                cd[6] = 1.0;
            }
            s3_whiten(W, cs, lin + 7 + i, 7);
            s3_whiten(W, cd, lin + 56 + i, 7);
        }
    }
}

// column i of A . column j of B (A, B row-major 7 x 7)
__device__ __forceinline__ double s3_coldot(const double *A, int i, const double *B, int j)
{
    double s = A[i] * B[j];
#pragma unroll
    for (int m = 1; m < 7; ++m)
        s = fma(A[7 * m + i], B[7 * m + j], s);
    return s;
}
// column i of A . r
__device__ __forceinline__ double s3_colvec(const double *A, int i, const double *r)
{
    double s = A[i] * r[0];
#pragma unroll
    for (int m = 1; m < 7; ++m)
        s = fma(A[7 * m + i], r[m], s);
    return s;
}

}  // namespace

}  // namespace mvs
