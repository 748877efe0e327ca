// lm_math.hpp -- the small-matrix device math the Levenberg-Marquardt solvers share: refine.hip, posegraph.hip,
// sim3graph.hip, pg_marginals.hip, pg_direct.hip, ba_sparse.hip and seq_graph.hip include it, and nothing else does.  SO(3) maps, the pose
// prior, the pinhole projection with its Jacobians, packed Cholesky factorisation and solves, the point block's 3 x 3
// Cholesky under the pivot rule, the robust-loss weight and rho2.  Device only; everything is forced inline into an anonymous
// namespace, so a file's kernels are compiled from these statements in this order exactly as if they stood in the file.
// The one definition is what makes "the same input gives the same bytes on every path" hold between the solvers.
#pragma once
#include "kernels.hpp"

namespace mvs {

namespace {

__host__ __device__ constexpr int lidx(int r, int c) { return r * (r + 1) / 2 + c; }  // r >= c

struct Cam {
    double fx, fy, sk, cx, cy;
};

// fused building blocks (one v_fma_f64 each); the oracle uses the same ones in the same places
__device__ __forceinline__ double fd2(double a0, double b0, double a1, double b1) { return fma(a1, b1, a0 * b0); }
__device__ __forceinline__ double fd3(double a0, double b0, double a1, double b1, double a2, double b2)
{
    return fma(a2, b2, fma(a1, b1, a0 * b0));
}
__device__ __forceinline__ double fx2(double a, double b, double c, double d) { return fma(a, b, -(c * d)); }  // a b - c d

__device__ __forceinline__ void so3_exp(const double (&w)[3], double (&R)[9])
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(th2);
    double A, B;
    if (th < 1e-4) {
        A = 1.0 - th2 / 6.0;
        B = 0.5 - th2 / 24.0;
    } else {
        A = sin(th) / th;
        B = (1.0 - cos(th)) / th2;
    }
    const double x = w[0], y = w[1], z = w[2];
    R[0] = 1.0 - B * (y * y + z * z);
    R[1] = B * (x * y) - A * z;
    R[2] = B * (x * z) + A * y;
    R[3] = B * (x * y) + A * z;
    R[4] = 1.0 - B * (x * x + z * z);
    R[5] = B * (y * z) - A * x;
    R[6] = B * (x * z) - A * y;
    R[7] = B * (y * z) + A * x;
    R[8] = 1.0 - B * (x * x + y * y);
}

__device__ __forceinline__ void so3_log(const double (&R)[9], double (&w)[6])
{
    const double vx = 0.5 * (R[7] - R[5]), vy = 0.5 * (R[2] - R[6]), vz = 0.5 * (R[3] - R[1]);
    const double s = sqrt((vx * vx + vy * vy) + vz * vz);
    const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double th = atan2(s, c);
    double k;
    if (s < 1e-4 && c > 0.0)
        k = 1.0 + (s * s) / 6.0;
    else
        k = th / s;
    w[0] = k * vx;
    w[1] = k * vy;
    w[2] = k * vz;
}

__device__ __forceinline__ void so3_jrinv(const double (&w)[6], double (&J)[9])
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(th2);
    double g;
    if (th < 1e-4)
        g = 1.0 / 12.0 + th2 / 720.0;
    else
        g = 1.0 / th2 - (1.0 + cos(th)) / ((2.0 * th) * sin(th));
    const double x = w[0], y = w[1], z = w[2];
    J[0] = 1.0 + g * (x * x - th2);
    J[1] = g * (x * y) - 0.5 * z;
    J[2] = g * (x * z) + 0.5 * y;
    J[3] = g * (x * y) + 0.5 * z;
    J[4] = 1.0 + g * (y * y - th2);
    J[5] = g * (y * z) - 0.5 * x;
    J[6] = g * (x * z) - 0.5 * y;
    J[7] = g * (y * z) + 0.5 * x;
    J[8] = 1.0 + g * (z * z - th2);
}

// pose prior of one frame (or node): error e = (Log(R0^T R), R0^T (t - t0)); Jw = Jr^-1(e_w), Jv = R0^T R
template <bool JAC>
__device__ __forceinline__ void pose_prior(const double (&R0)[9], const double (&t0)[3], const double (&R)[9],
                                           const double (&t)[3], double (&e)[6], double (&Jw)[9], double (&Jv)[9])
{
    double Re[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Re[3 * i + j] = (R0[i] * R[j] + R0[3 + i] * R[3 + j]) + R0[6 + i] * R[6 + j];
    so3_log(Re, e);
    const double d0 = t[0] - t0[0], d1 = t[1] - t0[1], d2 = t[2] - t0[2];
    e[3] = (R0[0] * d0 + R0[3] * d1) + R0[6] * d2;
    e[4] = (R0[1] * d0 + R0[4] * d1) + R0[7] * d2;
    e[5] = (R0[2] * d0 + R0[5] * d1) + R0[8] * d2;
    if (JAC) {
        so3_jrinv(e, Jw);
#pragma unroll
        for (int k = 0; k < 9; ++k)
            Jv[k] = Re[k];
    }
}

// residual of one observation (and its Jacobians): GenericProjectionFactor with throwCheirality = false
template <bool JAC>
__device__ __forceinline__ void project_lin(const Cam &cam, const double (&R)[9], const double (&t)[3],
                                            const double (&p)[3], double u, double v, double (&r)[2], double (&Jc)[12],
                                            double (&Jp)[6])
{
    const double d0 = p[0] - t[0], d1 = p[1] - t[1], d2 = p[2] - t[2];
    const double q0 = fd3(R[0], d0, R[3], d1, R[6], d2);
    const double q1 = fd3(R[1], d0, R[4], d1, R[7], d2);
    const double q2 = fd3(R[2], d0, R[5], d1, R[8], d2);
    if (!(q2 > 0.0)) {
        r[0] = 2.0 * cam.fx;
        r[1] = 2.0 * cam.fx;
        if (JAC) {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                Jc[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                Jp[k] = 0.0;
        }
        return;
    }
    const double iz = 1.0 / q2, xn = q0 * iz, yn = q1 * iz;
    const double un = fd2(cam.fx, xn, cam.sk, yn), vn = cam.fy * yn;
    r[0] = (un + cam.cx) - u;
    r[1] = (vn + cam.cy) - v;
    if (JAC) {
        const double A[6] = {cam.fx * iz, cam.sk * iz, -(un * iz), 0.0, cam.fy * iz, -(vn * iz)};
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double a0 = A[3 * a], a1 = A[3 * a + 1], a2 = A[3 * a + 2];
            Jc[6 * a + 0] = fx2(a1, q2, a2, q1);
            Jc[6 * a + 1] = fx2(a2, q0, a0, q2);
            Jc[6 * a + 2] = fx2(a0, q1, a1, q0);
            Jc[6 * a + 3] = -a0;
            Jc[6 * a + 4] = -a1;
            Jc[6 * a + 5] = -a2;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                Jp[3 * a + k] = fd3(a0, R[3 * k], a1, R[3 * k + 1], a2, R[3 * k + 2]);
        }
    }
}

// in-place Cholesky of the packed lower triangle; false if not positive definite.  The diagonal holds 1 / l_jj (one
// division per column; the other 78 divisions of a factorisation + solve are multiplications by it, as in the oracle).
// Two forms, one statement apart, and they stay two: with the first forwarding to the second (directly, or through a common
// body with a compile-time flag) refine_kernel<2> comes out with the operands of two multiplications exchanged -- the same
// values from other machine code than the build before the functions were shared.
template <int N>
__device__ __forceinline__ bool chol_packed(double (&S)[N * (N + 1) / 2])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = S[lidx(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k)
            d = fma(-S[lidx(j, k)], S[lidx(j, k)], d);
        ok = ok && (d > 0.0) && (d < __builtin_inf());
        const double inv = 1.0 / sqrt(d);
        S[lidx(j, j)] = inv;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = S[lidx(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k)
                v = fma(-S[lidx(i, k)], S[lidx(j, k)], v);
            S[lidx(i, j)] = v * inv;
        }
    }
    return ok;
}
// the same, and `min_d` follows the smallest pivot (l_jj squared)
template <int N>
__device__ __forceinline__ bool chol_packed(double (&S)[N * (N + 1) / 2], double &min_d)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = S[lidx(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k)
            d = fma(-S[lidx(j, k)], S[lidx(j, k)], d);
        ok = ok && (d > 0.0) && (d < __builtin_inf());
        min_d = d < min_d ? d : min_d;
        const double inv = 1.0 / sqrt(d);
        S[lidx(j, j)] = inv;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = S[lidx(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k)
                v = fma(-S[lidx(i, k)], S[lidx(j, k)], v);
            S[lidx(i, j)] = v * inv;
        }
    }
    return ok;
}

template <int N>
__device__ __forceinline__ void chol_solve(const double (&Lc)[N * (N + 1) / 2], double (&b)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k)
            v = fma(-Lc[lidx(i, k)], b[k], v);
        b[i] = v * Lc[lidx(i, i)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = b[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k)
            v = fma(-Lc[lidx(k, i)], b[k], v);
        b[i] = v * Lc[lidx(i, i)];
    }
}

// the point block V (packed xx xy xz yy yz zz; v0, v3, v5: its diagonal with lambda added) = L L^T under the pivot rule: a
// pivot must exceed kBaPivotTol times the entry before elimination.  Li = L^-1 (l00 l10 l11 l20 l21 l22), zero if V fails.
__device__ __forceinline__ bool chol3_pivot(const double (&V)[6], double v0, double v3, double v5, double (&Li)[6])
{
    const double inf = __builtin_inf();
    bool ok = v0 > 0.0 && v0 < inf;
    const double i0 = 1.0 / sqrt(v0);
    const double l10 = V[1] * i0, l20 = V[2] * i0;
    const double e1 = fma(-l10, l10, v3);
    ok = ok && e1 > kBaPivotTol * v3 && e1 < inf;
    const double i1 = 1.0 / sqrt(e1);
    const double l21 = fma(-l20, l10, V[4]) * i1;
    const double e2 = fma(-l21, l21, fma(-l20, l20, v5));
    ok = ok && e2 > kBaPivotTol * v5 && e2 < inf;
    const double i2 = 1.0 / sqrt(e2);
    const double m10 = -(l10 * i0) * i1, m21 = -(l21 * i1) * i2, m20 = -fd2(l20, i0, l21, m10) * i2;
    Li[0] = ok ? i0 : 0.0;
    Li[1] = ok ? m10 : 0.0;
    Li[2] = ok ? i1 : 0.0;
    Li[3] = ok ? m20 : 0.0;
    Li[4] = ok ? m21 : 0.0;
    Li[5] = ok ? i2 : 0.0;
    return ok;
}

// ---- robust losses (DESIGN.md sections 4.7.6 and 4.10.5): loss 1 Huber, otherwise Cauchy, constant k ------------------------
// weight w(s) of a robustified term from s = |r|^2 and x = sqrt(s): Huber 1 or k / x, Cauchy k^2 / (k^2 + s)
__device__ __forceinline__ double loss_weight(int loss, double k, double s, double x)
{
    if (loss == 1)
        return x <= k ? 1.0 : k / x;
    const double k2 = k * k;
    return k2 / (k2 + s);
}
// rho2(s), the term's share of twice the cost (the Cauchy cost: log1p of one quotient).  The same values from two forms, the
// bundle adjustment's and the pose graph's, and they stay two: either file's kernels compiled from the other's form come out
// as other machine code than the build before the functions were shared.
__device__ __forceinline__ double ba_loss_rho2(int loss, double k, double s, double x)
{
    if (loss == 1)
        return x <= k ? s : (2.0 * k) * x - k * k;
    const double k2 = k * k;
    return k2 * log1p(s / k2);
}
__device__ __forceinline__ double pg_loss_rho2(int loss, double k, double s, double x)
{
    double rho2 = s;
    if (loss == 1) {
        if (!(x <= k))
            rho2 = (2.0 * k) * x - k * k;
    } else {
        const double k2 = k * k;
        rho2 = k2 * log1p(s / k2);
    }
    return rho2;
}

}  // namespace

}  // namespace mvs
