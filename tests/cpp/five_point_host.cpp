// Host build of the five-point solver and of the Sampson rule (mvslam_amd/csrc/five_point.hpp) and, on top of them and of the
// device's sampler (sampler.hpp), the host model of the five-point RANSAC stage (essential5.hip): sample -> solve -> count ->
// select with the four-level tie order.  Built by tests/test_five_point_host.py
//   - as a stand-alone program (main below: random and degenerate samples, every returned matrix finite and normalised, the
//     model run on a small scene), once plain and once under -fsanitize=address,undefined;
//   - as a shared object the tests load with ctypes (the extern "C" functions).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define MVS_DEV static inline
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }
#include "../../mvslam_amd/csrc/sampler.hpp"
#include "../../mvslam_amd/csrc/five_point.hpp"

extern "C" {

// p1 / p2: 5 x (x, y).  E: [10][9], rows past n zeroed.  Returns n.
int e5_five_point(const double *p1, const double *p2, double *E)
{
    double ws[mvs::kE5Ws];
    const mvs::E5Ws w{ws, 1};
    const int n = mvs::five_point(p1, p2, w);
    for (int k = 0; k < 90; ++k)
        E[k] = k < 9 * n ? ws[k] : 0.0;
    return n;
}

void e5_sampson_terms(const double *E, double x1, double y1, double x2, double y2, double *num, double *den)
{
    double e[9];
    for (int k = 0; k < 9; ++k)
        e[k] = E[k];
    mvs::e5_sampson(e, x1, y1, x2, y2, *num, *den);
}

void e5_sample5(uint64_t seed, uint32_t hyp, int M, int sampler, int *idx5)
{
    int idx[8];
    mvs::sample8(seed, hyp, M, sampler, idx);
    for (int k = 0; k < 5; ++k)
        idx5[k] = idx[k];
}

// The selection over supplied models (models [H][10][9], n_roots [H], count [H][10]): among the models with the largest count
// the smaller residual, then the smaller hypothesis, then the smaller root.  Returns the largest count (-1: no model).
int e5_select(const double *models, const int32_t *n_roots, const int32_t *count, int H, const double *P, int m, double thr,
              int *best_hyp, int *best_root, double *best_residual)
{
    int best = -1;
    for (int h = 0; h < H; ++h)
        for (int r = 0; r < n_roots[h] && r < 10; ++r)
            best = count[h * 10 + r] > best ? count[h * 10 + r] : best;
    *best_hyp = -1; *best_root = -1; *best_residual = 0.0;
    if (best < 0)
        return best;
    bool have = false;
    for (int h = 0; h < H; ++h)
        for (int r = 0; r < n_roots[h] && r < 10; ++r) {
            if (count[h * 10 + r] != best)
                continue;
            double e[9];
            for (int k = 0; k < 9; ++k)
                e[k] = models[(size_t)h * 90 + 9 * r + k];
            double sum = 0.0;
            for (int i = 0; i < m; ++i) {
                double num, den;
                mvs::e5_sampson(e, P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], num, den);
                if (mvs::e5_inlier(num, den, thr))
                    sum += num / den;
            }
            sum = mvs::e5_residual_key(sum);
            if (!have || sum < *best_residual) {   // ascending (hypothesis, root): a tie keeps the earlier one
                have = true;
                *best_residual = sum; *best_hyp = h; *best_root = r;
            }
        }
    return best;
}

// count of one supplied model (the inlier rule of the header)
int e5_count(const double *E, const double *P, int m, double thr)
{
    double e[9];
    for (int k = 0; k < 9; ++k)
        e[k] = E[k];
    int c = 0;
    for (int i = 0; i < m; ++i) {
        double num, den;
        mvs::e5_sampson(e, P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], num, den);
        c += mvs::e5_inlier(num, den, thr) ? 1 : 0;
    }
    return c;
}

// The RANSAC stage on m matches P = (x1, y1, x2, y2) per match.  n_roots [H], count [H][10] (-1 past n_roots).
// Returns 1 if a model was selected (best_count may still be 0), else 0 with best_hyp = best_root = -1.
int e5_ransac(const double *P, int m, double thr, int H, int sampler, uint64_t seed, double *E, uint8_t *mask, int *best_hyp,
              int *best_root, int *best_count, double *best_residual, int32_t *n_roots, int32_t *count)
{
    for (int k = 0; k < 9; ++k)
        E[k] = 0.0;
    for (int i = 0; i < m; ++i)
        mask[i] = 0;
    *best_hyp = -1; *best_root = -1; *best_count = 0; *best_residual = 0.0;
    if (m < 8)
        return 0;
    std::vector<double> models((size_t)H * 90);
    int best = -1;
    for (int h = 0; h < H; ++h) {
        int idx[8];
        mvs::sample8(seed, (uint32_t)h, m, sampler, idx);
        double p1[10], p2[10];
        for (int k = 0; k < 5; ++k) {
            p1[2 * k] = P[4 * idx[k]]; p1[2 * k + 1] = P[4 * idx[k] + 1];
            p2[2 * k] = P[4 * idx[k] + 2]; p2[2 * k + 1] = P[4 * idx[k] + 3];
        }
        const int n = e5_five_point(p1, p2, &models[(size_t)h * 90]);
        n_roots[h] = n;
        for (int r = 0; r < 10; ++r) {
            int c = -1;
            if (r < n) {
                double e[9];
                for (int k = 0; k < 9; ++k)
                    e[k] = models[(size_t)h * 90 + 9 * r + k];
                c = 0;
                for (int i = 0; i < m; ++i) {
                    double num, den;
                    mvs::e5_sampson(e, P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], num, den);
                    c += mvs::e5_inlier(num, den, thr) ? 1 : 0;
                }
            }
            count[h * 10 + r] = c;
            best = c > best ? c : best;
        }
    }
    if (best < 0)
        return 0;
    double bres = 0.0;
    int bh = -1, br = -1;
    e5_select(models.data(), n_roots, count, H, P, m, thr, &bh, &br, &bres);
    double e[9];
    for (int k = 0; k < 9; ++k)
        E[k] = e[k] = models[(size_t)bh * 90 + 9 * br + k];
    for (int i = 0; i < m; ++i) {
        double num, den;
        mvs::e5_sampson(e, P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], num, den);
        mask[i] = mvs::e5_inlier(num, den, thr) ? 1 : 0;
    }
    *best_hyp = bh; *best_root = br; *best_count = best; *best_residual = bres;
    return 1;
}

}  // extern "C"

// ---- stand-alone self-check ---------------------------------------------------------------------------------------------------
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double urand()   // xorshift64*, [0, 1)
{
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

static long check_models(const double *E, int n, const double *p1, const double *p2, long &bad)
{
    for (int r = 0; r < n; ++r) {
        double f2 = 0.0, worst = 0.0;
        for (int k = 0; k < 9; ++k) {
            if (!isfinite(E[9 * r + k]))
                ++bad;
            f2 += E[9 * r + k] * E[9 * r + k];
        }
        if (!(fabs(f2 - 2.0) < 1e-9))
            ++bad;
        if (p1)
            for (int c = 0; c < 5; ++c) {
                double num, den;
                e5_sampson_terms(E + 9 * r, p1[2 * c], p1[2 * c + 1], p2[2 * c], p2[2 * c + 1], &num, &den);
                worst = fmax(worst, sqrt(num));
            }
        if (!(worst < 1e-6))
            ++bad;
    }
    return n;
}

int main()
{
    long bad = 0, models = 0, samples = 0;
    double E[90];
    // generic samples: a rotation about a random axis (|omega| <= 0.3), unit baseline, depths in [2, 10]
    for (int s = 0; s < 3000; ++s) {
        double om[3], t[3], nt = 0.0, no = 0.0;
        for (int k = 0; k < 3; ++k) { om[k] = urand() - 0.5; t[k] = urand() - 0.5; no += om[k] * om[k]; nt += t[k] * t[k]; }
        const double ang = 0.3 * urand();
        no = sqrt(no); nt = sqrt(nt);
        for (int k = 0; k < 3; ++k) { om[k] /= no; t[k] /= nt; }
        const double c = cos(ang), sn = sin(ang);
        double R[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                R[3 * i + j] = (i == j ? c : 0.0) + (1.0 - c) * om[i] * om[j];
        R[1] -= sn * om[2]; R[2] += sn * om[1]; R[3] += sn * om[2]; R[5] -= sn * om[0]; R[6] -= sn * om[1]; R[7] += sn * om[0];
        double p1[10], p2[10];
        for (int k = 0; k < 5; ++k) {
            const double z = 2.0 + 8.0 * urand(), x = (urand() - 0.5) * z, y = (urand() - 0.5) * z;
            p1[2 * k] = x / z; p1[2 * k + 1] = y / z;
            const double X2 = R[0] * x + R[1] * y + R[2] * z + t[0], Y2 = R[3] * x + R[4] * y + R[5] * z + t[1],
                         Z2 = R[6] * x + R[7] * y + R[8] * z + t[2];
            p2[2 * k] = X2 / Z2; p2[2 * k + 1] = Y2 / Z2;
        }
        const int n = e5_five_point(p1, p2, E);
        if (n < 0 || n > 10)
            ++bad;
        models += check_models(E, n, p1, p2, bad);
        ++samples;
    }
    // degenerate inputs: finite matrices or none
    {
        double p1[10], p2[10];
        for (int k = 0; k < 5; ++k) { p1[2 * k] = 0.25; p1[2 * k + 1] = -0.5; p2[2 * k] = 0.3; p2[2 * k + 1] = 0.1; }
        models += check_models(E, e5_five_point(p1, p2, E), nullptr, nullptr, bad);      // five equal points
        for (int k = 0; k < 5; ++k) { p1[2 * k] = 0.1 * k; p1[2 * k + 1] = 0.2 * k - 0.3; p2[2 * k] = 0.1 * k + 0.05; p2[2 * k + 1] = 0.2 * k - 0.25; }
        models += check_models(E, e5_five_point(p1, p2, E), nullptr, nullptr, bad);      // five collinear points
        for (int k = 0; k < 5; ++k) { p1[2 * k] = urand() - 0.5; p1[2 * k + 1] = urand() - 0.5; p2[2 * k] = p1[2 * k]; p2[2 * k + 1] = p1[2 * k + 1]; }
        models += check_models(E, e5_five_point(p1, p2, E), nullptr, nullptr, bad);      // identical views
        for (int k = 0; k < 10; ++k) { p1[k] = 0.0; p2[k] = 0.0; }
        models += check_models(E, e5_five_point(p1, p2, E), nullptr, nullptr, bad);
        for (int k = 0; k < 10; ++k) { p1[k] = 1e200 * (k + 1); p2[k] = -1e180 * (k + 2); }
        models += check_models(E, e5_five_point(p1, p2, E), nullptr, nullptr, bad);      // overflowing intermediates
        p1[3] = NAN;
        models += check_models(E, e5_five_point(p1, p2, E), nullptr, nullptr, bad);
        samples += 6;
    }
    // the RANSAC model on a small scene with wrong matches: tables consistent with the winner
    {
        const int m = 37, H = 70;
        std::vector<double> P(4 * m);
        for (int i = 0; i < m; ++i) {
            const double z = 2.0 + 8.0 * urand(), x = (urand() - 0.5) * z, y = (urand() - 0.5) * z;
            P[4 * i] = x / z; P[4 * i + 1] = y / z;
            P[4 * i + 2] = (x + 1.0) / z; P[4 * i + 3] = y / z;
            if (i % 3 == 0) { P[4 * i + 2] = urand() - 0.5; P[4 * i + 3] = urand() - 0.5; }
        }
        std::vector<uint8_t> mask(m);
        std::vector<int32_t> nr(H), cnt(H * 10);
        double Eb[9], res;
        int bh, br, bc;
        for (int sampler = 0; sampler < 2; ++sampler) {
            const int got = e5_ransac(P.data(), m, 1e-6, H, sampler, 12345, Eb, mask.data(), &bh, &br, &bc, &res, nr.data(), cnt.data());
            int sum = 0;
            for (int i = 0; i < m; ++i)
                sum += mask[i];
            if (!got || bh < 0 || br < 0 || br >= nr[bh] || cnt[bh * 10 + br] != bc || sum != bc || !(res >= 0.0))
                ++bad;
            for (int h = 0; h < H; ++h)
                for (int r = 0; r < 10; ++r)
                    if ((r < nr[h]) != (cnt[h * 10 + r] >= 0) || cnt[h * 10 + r] > bc)
                        ++bad;
        }
        if (bc < 20)   // 25 of the 37 matches are right
            ++bad;
    }
    printf("five_point samples=%ld models=%ld bad=%ld\n", samples, models, bad);
    return bad == 0 ? 0 : 1;
}
