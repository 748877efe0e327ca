// five_point.hpp -- the minimal five-point essential-matrix solver (Nister, "An efficient solution to the five-point relative
// pose problem", PAMI 2004) and the Sampson inlier rule of the five-point RANSAC (essential5.hip).  Stands in for the
// cv::findEssentialMat call of the reference's default build (vision/sfm-solve.cpp:42-63 under USE_OPENCV_ESSENTIAL_MATRIX,
// SConstruct:81-82).  OpenCV's arithmetic is not in the reference tree: everything below is this build's own, fully stated rule.
//
// Plain C++ written against MVS_DEV like sampler.hpp: a host translation unit that defines MVS_DEV before including this file
// gets the same functions, and the same BITS -- the only operations are + - * / sqrt and explicit fma (no libm call, no
// contraction: every build passes -ffp-contract=off), all correctly rounded on both sides (tests/cpp/five_point_host.cpp).
//
// Every array the solver works on lives in a caller-supplied workspace of kE5Ws doubles addressed with a stride: the host passes
// a plain array (stride 1), a kernel passes its lane's column of an LDS block (stride = lanes), so indices computed at run time
// (pivot rows, root slots) never force a register array into scratch memory.
//
// Definition.  Five correspondences x1_i <-> x2_i in ideal-camera coordinates, x2_i^T E x1_i = 0.
//   1. Null space.  Row i of the 5 x 9 design matrix is (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1) (E row-major).  Its
//      transpose (9 x 5) is reduced by five Householder reflections in column order, no pivoting; the last four columns of
//      Q = H0 H1 H2 H3 H4 are the orthonormal basis X, Y, Z, W.  Householder rather than the one-sided Jacobi code of
//      device_math.hpp: a fixed operation count (no sweeps, no convergence test), an orthonormal basis to working precision, and
//      the rank test comes for free -- |R_kk|^2 <= kE5RankTol2 x (largest squared row norm of the design matrix) for any k means
//      the null space has more than four dimensions (repeated points, collinear points): n = 0.
//   2. E = x X + y Y + z Z + W.  det E = 0 and 2 E E^T E - tr(E E^T) E = 0 (halved: (E E^T - tr/2 I) E) are ten cubics in
//      (x, y, z): a 10 x 20 matrix over the monomials, in Nister's order
//        x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.
//   3. Elimination.  Gauss-Jordan on the left 10 x 10 block with PARTIAL (row) pivoting: step k takes the row r >= k with the
//      largest |a_rk|, the lowest r on ties, scales it by the reciprocal of the pivot and subtracts it from the rows below; a
//      pivot with |a_rk| <= kE5PivotTol x (largest |entry| of the matrix as built) or a non-finite one: n = 0.  The back
//      substitution only runs on rows 4 .. 9 (the ones with leading monomials x^2z x^2 y^2z y^2 xyz xy), right half only.
//   4. B(z) (x, y, 1)^T = 0 with rows (e - z f), (g - z h), (i - z j): det B(z) is the tenth-degree polynomial, built from the
//      2 x 2 minors p1, p2, p3 of the first two rows; x = p1(z) / p3(z), y = p2(z) / p3(z).
//   5. Real roots by critical points: the roots of a polynomial lie one each between consecutive roots of its derivative.  From
//      the ninth derivative (linear) up to the polynomial itself, level k keeps k sorted slots; the k intervals between the
//      slots of level k - 1 (and -R, R; R = 1 + max |c_i / c_10|, Cauchy's bound) are tested for a sign change (v < 0 against
//      v >= 0) at their ends, evaluated by Horner's rule with fma.  An interval without one hands its upper end on as an empty
//      slot.  Otherwise bisection, at most kE5BisectMax halvings, until the width is at most 2^-26 of the larger end or no
//      double lies strictly between the ends; then kE5Newton Newton steps, each kept only if it stays inside the bracket.
//   6. Every real root z, ascending (that order is the ROOT INDEX), gives E, scaled to Frobenius norm sqrt(2), sign such that
//      the entry of largest magnitude is positive (lowest index on ties).  A root whose E has a non-finite entry is dropped.
// n = 0 as well when the polynomial has no usable root bound (R > 1e150 or not a number: leading coefficient zero or tiny).  Never aborts, never
// returns a non-finite E.
#pragma once
#include <stdint.h>
#ifndef MVS_DEV
#include <hip/hip_runtime.h>
#define MVS_DEV __device__ __forceinline__
#endif
#ifdef __HIPCC__
#define MVS_E5_MEMBER __device__ __forceinline__
#else
#define MVS_E5_MEMBER inline   // (MVS_DEV is `static inline` in a host build: not for a member function)
#endif

namespace mvs {

constexpr int kE5Ws = 276;                 // doubles of workspace per solve
constexpr int kE5Models = 10;              // models are left in workspace [0, 90): model r at [9 r, 9 r + 9)
constexpr double kE5RankTol2 = 1e-24;      // step 1
constexpr double kE5PivotTol = 1e-14;      // step 3
constexpr int kE5BisectMax = 128;          // step 5
constexpr int kE5Newton = 4;
constexpr double kE5Huge = 1.7e308;

struct E5Ws {
    double *p;
    int s;
    MVS_E5_MEMBER double &operator()(int k) const { return p[(size_t)k * (size_t)s]; }
};

// index of the product of linear monomials i, j (x y z 1) among the quadratic ones x^2 xy xz x y^2 yz y z^2 z 1
MVS_DEV int e5_qidx(int i, int j) { return (int)((0x9863875265413210ull >> (4 * (i * 4 + j))) & 15u); }
// column (Nister's order) of quadratic monomial q times linear monomial l
MVS_DEV int e5_cidx(int q, int l)
{
    const int g = q / 3;
    const uint64_t wd = g == 0 ? 0x5a9044a06229040ull : g == 1 ? 0x734c83982362d25ull : g == 2 ? 0x945cb8c1aa7b8e9ull : 0x9c9ecull;
    return (int)((wd >> (20 * (q - 3 * g) + 5 * l)) & 31u);
}

// workspace layout
constexpr int kE5Mat = 0;      // [200] the 10 x 20 matrix, row-major; before it is built: the 9 x 5 Householder matrix + 5 betas
constexpr int kE5Bas = 200;    // [36] basis: entry e (0 .. 8) of X, Y, Z, W at 200 + 4 e + {0, 1, 2, 3}
constexpr int kE5Tr = 236;     // [10] tr(E E^T) as a quadratic; later p1 [8]
constexpr int kE5Lam = 246;    // [30] one row of E E^T - tr/2 I; later p2 [8], p3 [7], c [11] from 244
constexpr int kE5P1 = 236, kE5P2 = 244, kE5P3 = 252, kE5C = 259;
constexpr int kE5B = 0;        // [39] B(z): row i at 13 i: x part [4], y part [4], constant part [5], ascending powers
constexpr int kE5Lev = 90;     // [65] level polynomials: degree 10 first, degree 1 last
constexpr int kE5Slot = 155;   // [2][10] root slots of the previous and the current level

MVS_DEV int e5_lev_off(int k)   // level k has k + 1 coefficients
{
    // 90 + sum_{j = k + 1 .. 10} (j + 1)
    return kE5Lev + (66 - ((k + 1) * (k + 2)) / 2);
}

MVS_DEV double e5_horner(const E5Ws &w, int off, int deg, double z)
{
    double v = w(off + deg);
    for (int i = deg - 1; i >= 0; --i)
        v = __builtin_fma(v, z, w(off + i));
    return v;
}

// dst (quadratic, 10) += sgn * a * b, a and b linear (4)
MVS_DEV void e5_quad_acc(const E5Ws &w, int dst, int a, int b, double sgn)
{
    for (int i = 0; i < 4; ++i) {
        const double ai = sgn * w(a + i);
        for (int j = 0; j < 4; ++j)
            w(dst + e5_qidx(i, j)) += ai * w(b + j);
    }
}
// row (cubic, 20) += q * l, q quadratic (10), l linear (4)
MVS_DEV void e5_cubic_acc(const E5Ws &w, int row, int q, int l)
{
    for (int i = 0; i < 10; ++i) {
        const double qi = w(q + i);
        for (int j = 0; j < 4; ++j)
            w(row + e5_cidx(i, j)) += qi * w(l + j);
    }
}
// dst += sgn * a * b, polynomials in z with na and nb coefficients
MVS_DEV void e5_conv_acc(const E5Ws &w, int dst, int a, int na, int b, int nb, double sgn)
{
    for (int i = 0; i < na; ++i) {
        const double ai = sgn * w(a + i);
        for (int j = 0; j < nb; ++j)
            w(dst + i + j) += ai * w(b + j);
    }
}
MVS_DEV void e5_zero(const E5Ws &w, int off, int n)
{
    for (int i = 0; i < n; ++i)
        w(off + i) = 0.0;
}

// p1 / p2: the five points of the two views, (x, y) each.  Returns n; model r is left in w(9 r .. 9 r + 8).
MVS_DEV int five_point(const double *p1, const double *p2, const E5Ws &w)
{
    // ---- 1. null space ----
    double amax = 0.0;
    for (int c = 0; c < 5; ++c) {
        const double x1 = p1[2 * c], y1 = p1[2 * c + 1], x2 = p2[2 * c], y2 = p2[2 * c + 1];
        w(0 * 5 + c) = x2 * x1; w(1 * 5 + c) = x2 * y1; w(2 * 5 + c) = x2;
        w(3 * 5 + c) = y2 * x1; w(4 * 5 + c) = y2 * y1; w(5 * 5 + c) = y2;
        w(6 * 5 + c) = x1;      w(7 * 5 + c) = y1;      w(8 * 5 + c) = 1.0;
        double nn = 0.0;
        for (int r = 0; r < 9; ++r)
            nn += w(r * 5 + c) * w(r * 5 + c);
        amax = nn > amax ? nn : amax;
    }
    if (!(amax <= kE5Huge))
        return 0;
    for (int k = 0; k < 5; ++k) {
        double sigma = 0.0;
        for (int r = k; r < 9; ++r)
            sigma += w(r * 5 + k) * w(r * 5 + k);
        if (!(sigma > kE5RankTol2 * amax))
            return 0;
        const double nrm = __builtin_sqrt(sigma);
        const double akk = w(k * 5 + k);
        const double vk = akk >= 0.0 ? akk + nrm : akk - nrm;
        w(k * 5 + k) = vk;
        double vtv = vk * vk;
        for (int r = k + 1; r < 9; ++r)
            vtv += w(r * 5 + k) * w(r * 5 + k);
        const double beta = 2.0 / vtv;
        w(45 + k) = beta;
        for (int c = k + 1; c < 5; ++c) {
            double s = 0.0;
            for (int r = k; r < 9; ++r)
                s += w(r * 5 + k) * w(r * 5 + c);
            s *= beta;
            for (int r = k; r < 9; ++r)
                w(r * 5 + c) -= s * w(r * 5 + k);
        }
    }
    for (int j = 0; j < 4; ++j) {
        for (int e = 0; e < 9; ++e)
            w(kE5Bas + 4 * e + j) = e == 5 + j ? 1.0 : 0.0;
        for (int k = 4; k >= 0; --k) {
            double s = 0.0;
            for (int r = k; r < 9; ++r)
                s += w(r * 5 + k) * w(kE5Bas + 4 * r + j);
            s *= w(45 + k);
            for (int r = k; r < 9; ++r)
                w(kE5Bas + 4 * r + j) -= s * w(r * 5 + k);
        }
    }

    // ---- 2. the ten cubic constraints ----
    e5_zero(w, kE5Mat, 200);
    {
        // det E: the three cofactors of the first row as quadratics, then row 0 = sum_j cofactor_j e_0j
        const int L = kE5Lam;
        e5_zero(w, L, 30);
        auto ent = [](int e) { return kE5Bas + 4 * e; };
        e5_quad_acc(w, L, ent(4), ent(8), 1.0);
        e5_quad_acc(w, L, ent(5), ent(7), -1.0);
        e5_quad_acc(w, L + 10, ent(5), ent(6), 1.0);
        e5_quad_acc(w, L + 10, ent(3), ent(8), -1.0);
        e5_quad_acc(w, L + 20, ent(3), ent(7), 1.0);
        e5_quad_acc(w, L + 20, ent(4), ent(6), -1.0);
        for (int j = 0; j < 3; ++j)
            e5_cubic_acc(w, kE5Mat, L + 10 * j, ent(j));
        // tr(E E^T)
        e5_zero(w, kE5Tr, 10);
        for (int e = 0; e < 9; ++e)
            e5_quad_acc(w, kE5Tr, ent(e), ent(e), 1.0);
        // rows 1 + 3 i + j: sum_k (E E^T - tr/2 I)_ik e_kj
        for (int i = 0; i < 3; ++i) {
            e5_zero(w, L, 30);
            for (int k = 0; k < 3; ++k) {
                for (int m = 0; m < 3; ++m)
                    e5_quad_acc(w, L + 10 * k, ent(3 * i + m), ent(3 * k + m), 1.0);
                if (k == i)
                    for (int q = 0; q < 10; ++q)
                        w(L + 10 * k + q) -= 0.5 * w(kE5Tr + q);
            }
            for (int j = 0; j < 3; ++j)
                for (int k = 0; k < 3; ++k)
                    e5_cubic_acc(w, kE5Mat + 20 * (1 + 3 * i + j), L + 10 * k, ent(3 * k + j));
        }
    }

    // ---- 3. elimination ----
    {
        double mmax = 0.0;
        for (int i = 0; i < 200; ++i) {
            const double a = __builtin_fabs(w(kE5Mat + i));
            mmax = a > mmax ? a : mmax;
        }
        if (!(mmax <= kE5Huge))
            return 0;
        const double ptol = kE5PivotTol * mmax;
        for (int k = 0; k < 10; ++k) {
            int pr = k;
            double pa = __builtin_fabs(w(kE5Mat + 20 * k + k));
            for (int r = k + 1; r < 10; ++r) {
                const double a = __builtin_fabs(w(kE5Mat + 20 * r + k));
                if (a > pa) {
                    pa = a;
                    pr = r;
                }
            }
            if (!(pa > ptol) || !(pa <= kE5Huge))
                return 0;
            if (pr != k)
                for (int c = k; c < 20; ++c) {
                    const double t = w(kE5Mat + 20 * k + c);
                    w(kE5Mat + 20 * k + c) = w(kE5Mat + 20 * pr + c);
                    w(kE5Mat + 20 * pr + c) = t;
                }
            const double inv = 1.0 / w(kE5Mat + 20 * k + k);
            for (int c = k; c < 20; ++c)
                w(kE5Mat + 20 * k + c) *= inv;
            for (int r = k + 1; r < 10; ++r) {
                const double f = w(kE5Mat + 20 * r + k);
                for (int c = k; c < 20; ++c)
                    w(kE5Mat + 20 * r + c) -= f * w(kE5Mat + 20 * k + c);
            }
        }
        for (int k = 9; k >= 5; --k)
            for (int r = 4; r < k; ++r) {
                const double f = w(kE5Mat + 20 * r + k);
                for (int c = 10; c < 20; ++c)
                    w(kE5Mat + 20 * r + c) -= f * w(kE5Mat + 20 * k + c);
            }
    }

    // ---- 4. B(z), its minors, the tenth-degree polynomial ----
    for (int i = 0; i < 3; ++i) {
        const int a = kE5Mat + 20 * (4 + 2 * i) + 10, b = a + 20, B = kE5B + 13 * i;
        // (rows 0 and 1 of the matrix, which B overwrites, are dead; a and b are rows 4 .. 9)
        w(B + 0) = w(a + 2); w(B + 1) = w(a + 1) - w(b + 2); w(B + 2) = w(a + 0) - w(b + 1); w(B + 3) = -w(b + 0);
        w(B + 4) = w(a + 5); w(B + 5) = w(a + 4) - w(b + 5); w(B + 6) = w(a + 3) - w(b + 4); w(B + 7) = -w(b + 3);
        w(B + 8) = w(a + 9); w(B + 9) = w(a + 8) - w(b + 9); w(B + 10) = w(a + 7) - w(b + 8);
        w(B + 11) = w(a + 6) - w(b + 7); w(B + 12) = -w(b + 6);
    }
    {
        const int B0 = kE5B, B1 = kE5B + 13, B2 = kE5B + 26;
        e5_zero(w, kE5P1, 34);   // p1, p2, p3, c are consecutive
        e5_conv_acc(w, kE5P1, B0 + 4, 4, B1 + 8, 5, 1.0);    // p1 = B01 B12 - B02 B11
        e5_conv_acc(w, kE5P1, B0 + 8, 5, B1 + 4, 4, -1.0);
        e5_conv_acc(w, kE5P2, B0 + 8, 5, B1 + 0, 4, 1.0);    // p2 = B02 B10 - B00 B12
        e5_conv_acc(w, kE5P2, B0 + 0, 4, B1 + 8, 5, -1.0);
        e5_conv_acc(w, kE5P3, B0 + 0, 4, B1 + 4, 4, 1.0);    // p3 = B00 B11 - B01 B10
        e5_conv_acc(w, kE5P3, B0 + 4, 4, B1 + 0, 4, -1.0);
        e5_conv_acc(w, kE5C, kE5P1, 8, B2 + 0, 4, 1.0);
        e5_conv_acc(w, kE5C, kE5P2, 8, B2 + 4, 4, 1.0);
        e5_conv_acc(w, kE5C, kE5P3, 7, B2 + 8, 5, 1.0);
    }

    // ---- 5. real roots ----
    double R;
    {
        const double lead = __builtin_fabs(w(kE5C + 10));
        double cm = 0.0;
        for (int i = 0; i < 10; ++i) {
            const double a = __builtin_fabs(w(kE5C + i));
            cm = a > cm ? a : cm;
        }
        R = 1.0 + cm / lead;
        if (!(R <= 1e150))   // (also a NaN: lead == 0 with cm == 0) -- no usable root bound
            return 0;
    }
    for (int i = 0; i <= 10; ++i)
        w(e5_lev_off(10) + i) = w(kE5C + i);
    for (int k = 10; k >= 2; --k)
        for (int i = 0; i < k; ++i)
            w(e5_lev_off(k - 1) + i) = w(e5_lev_off(k) + i + 1) * (double)(i + 1);
    int prev = kE5Slot, cur = kE5Slot + 10;
    {
        const int o = e5_lev_off(1);
        double t = -w(o) / w(o + 1);
        t = t >= -R ? t : -R;   // (a NaN ends at -R)
        t = t <= R ? t : R;
        w(prev) = t;
    }
    unsigned valid = 0;
    for (int k = 2; k <= 10; ++k) {
        const int o = e5_lev_off(k), od = e5_lev_off(k - 1);
        valid = 0;
        for (int j = 0; j < k; ++j) {
            double a = j == 0 ? -R : w(prev + j - 1);
            double b = j == k - 1 ? R : w(prev + j);
            const bool sa = e5_horner(w, o, k, a) < 0.0, sb = e5_horner(w, o, k, b) < 0.0;
            double z = b;
            if (sa != sb) {
                for (int it = 0; it < kE5BisectMax; ++it) {
                    const double aa = __builtin_fabs(a), ab = __builtin_fabs(b);
                    if (b - a <= 0x1p-26 * (aa > ab ? aa : ab))
                        break;
                    const double m = 0.5 * a + 0.5 * b;
                    if (!(m > a && m < b))
                        break;
                    if ((e5_horner(w, o, k, m) < 0.0) == sa)
                        a = m;
                    else
                        b = m;
                }
                z = 0.5 * a + 0.5 * b;
                for (int it = 0; it < kE5Newton; ++it) {
                    const double zn = z - e5_horner(w, o, k, z) / e5_horner(w, od, k - 1, z);
                    if (!(zn >= a && zn <= b))
                        break;
                    z = zn;
                }
                valid |= 1u << j;
            }
            w(cur + j) = z;
        }
        const int t = prev;
        prev = cur;
        cur = t;
    }

    // ---- 6. the models (prev: the slots of level 10) ----
    int n = 0;
    for (int j = 0; j < 10; ++j) {
        if (!((valid >> j) & 1u))
            continue;
        const double z = w(prev + j);
        const double d3 = e5_horner(w, kE5P3, 6, z);
        const double x = e5_horner(w, kE5P1, 7, z) / d3, y = e5_horner(w, kE5P2, 7, z) / d3;
        double E[9], f2 = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const int o = kE5Bas + 4 * e;
            E[e] = ((w(o) * x + w(o + 1) * y) + w(o + 2) * z) + w(o + 3);
            f2 += E[e] * E[e];
        }
        const double s = 1.4142135623730951 / __builtin_sqrt(f2);
        double big = -1.0, sg = 1.0;
        bool fin = s > 0.0 && s <= kE5Huge;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            E[e] *= s;
            const double a = __builtin_fabs(E[e]);
            fin = fin && a <= kE5Huge;
            if (a > big) {
                big = a;
                sg = E[e] < 0.0 ? -1.0 : 1.0;
            }
        }
        if (!fin)
            continue;
#pragma unroll
        for (int e = 0; e < 9; ++e)
            w(9 * n + e) = sg * E[e];
        ++n;
    }
    return n;
}

// ---- the inlier rule of the five-point RANSAC -------------------------------------------------------------------------------
// Squared Sampson distance of match (x1, y1) <-> (x2, y2) under E, as numerator and denominator (binary64, this order):
//   a = E x1:    a_r = (E_r0 x1 + E_r1 y1) + E_r2
//   b = E^T x2:  b_c = (E_0c x2 + E_1c y2) + E_2c        (c = 0, 1)
//   r = (x2 a_0 + y2 a_1) + a_2,   num = r r,   den = ((a_0 a_0 + a_1 a_1) + b_0 b_0) + b_1 b_1
// inlier iff den > 0 and num <= max_error_sq den (the reference's threshold sqrt(max_error_sq) on the distance,
// sfm-solve.cpp:55-57, squared; no division); its residual term is num / den.
MVS_DEV void e5_sampson(const double (&E)[9], double x1, double y1, double x2, double y2, double &num, double &den)
{
    const double a0 = (E[0] * x1 + E[1] * y1) + E[2];
    const double a1 = (E[3] * x1 + E[4] * y1) + E[5];
    const double a2 = (E[6] * x1 + E[7] * y1) + E[8];
    const double b0 = (E[0] * x2 + E[3] * y2) + E[6];
    const double b1 = (E[1] * x2 + E[4] * y2) + E[7];
    const double r = (x2 * a0 + y2 * a1) + a2;
    num = r * r;
    den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
}
MVS_DEV bool e5_inlier(double num, double den, double thr) { return den > 0.0 && num <= thr * den; }
// a residual sum that is not finite (overflowing terms) counts as the worst possible one, so that the selection order is total
MVS_DEV double e5_residual_key(double sum) { return sum <= kE5Huge ? sum : __builtin_inf(); }

// ---- the termination rule of the five-point RANSAC (essential5.hip) -----------------------------------
// With a confidence level p in (0, 1) a pair's hypotheses are counted up to a CHECKPOINT and no further once the best count
// seen so far makes another all-inlier sample unnecessary with probability p.  Checkpoints: T_0 = min(kE5Checkpoint0, H),
// T_{j+1} = min(2 T_j, H) (H = num_hypotheses; kE5Checkpoint0 = one workgroup of the solve + count kernel).  At T_j < H, with
// c the largest count over (h < T_j, root) and M the pair's matches, the pair stops iff c >= 1 and
//   (1 - (c / M)^5)^(64 2^j) <= 1 - p,   evaluated as  w = c / M, w2 = w w, w5 = (w2 w2) w, q = 1 - w5, q squared 6 + j times;
// at T_j = H it stops whatever c is.  Every operation is one rounded binary64 operation (no libm: a log or a pow that differs
// in its last place between host and device would move the answer by a whole block of hypotheses; no contraction: 1 - w5 is a
// subtraction, never the tail of an fma).  p = 0 switches the rule off: no checkpoints, every hypothesis runs.
constexpr int kE5Checkpoint0 = 64;
// (constexpr: the launch sequence on the host and a kernel share them)
constexpr int e5_checkpoint_first(int H) { return H < kE5Checkpoint0 ? H : kE5Checkpoint0; }
constexpr int e5_checkpoint_next(int T, int H) { return T >= H - T ? H : 2 * T; }   // min(2 T, H) without overflow
MVS_DEV bool e5_confident(int c, int M, int j, double p)
{
    if (c < 1)
        return false;
    const double w = (double)c / (double)M;
    const double w2 = w * w;
    const double w5 = (w2 * w2) * w;
    double x = 1.0 - w5;
    for (int i = 0; i < 6 + j; ++i)
        x = x * x;
    return x <= 1.0 - p;
}

}  // namespace mvs
