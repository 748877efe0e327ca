// pnp.hip -- pnp_solve (vision/pnp-solve.cpp:16-104) as a batched P3P-RANSAC.
//
// The reference forwards to cv::solvePnPRansac(SOLVEPNP_P3P, 100 iterations, reprojection error 0.05, confidence
// 0.95) and inverts the pose.  OpenCV's RANSAC kernel, RNG and final EPnP refit are third-party and differ between
// the 3.x versions the reference admits, so this is the build's own algorithm, written with
// + - * / sqrt only so that it matches the CPU oracle bit for bit:
//   pnp_prep      K^-1 (u, v, 1) and unit bearings                                   thread per point
//   pnp_ransac    one hypothesis per LANE: sample 4 -> Grunert P3P on 3 (quartic by Ferrari, resolvent cubic by
//                 64 bisections) -> pick among <= 4 solutions with the 4th point -> division-free reprojection
//                 test on all n points (point stream staged in LDS, broadcast reads) -> workgroup arg-best
//   pnp_finalize  arg-best over workgroups (most inliers, then first hypothesis: cv::RANSACPointSetRegistrator's
//                 rule), ordered inlier list, pose = SE3(SO3(R), t).inverse()          (pnp-solve.cpp:99-101)
#include "kernels.hpp"

#include "device_math.hpp"

namespace mvs {

// 4 distinct indices in [0, n): Philox block 2 (blocks 0 / 1 belong to the 8-of-M sampler), same draw rule
__device__ __forceinline__ void sample4(uint64_t seed, uint32_t hyp, int n, int sampler, int (&idx)[4])
{
    if (sampler == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            idx[k] = k;
        return;
    }
    uint32_t w[4];
    philox4x32_10(hyp, 2u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    int sorted[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        sorted[k] = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t r = __umulhi(w[k], (uint32_t)(n - k));
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < k && r >= (uint32_t)sorted[t])
                ++r;
        idx[k] = (int)r;
        int carry = (int)r;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t <= k) {
                const int cur = sorted[t];
                const bool sw = carry < cur;
                sorted[t] = sw ? carry : cur;
                carry = sw ? cur : carry;
            }
        }
    }
}

// real roots of x^4 + b x^3 + c x^2 + d x + e in fixed slots (valid flags), order: factor sg=+1 (larger, smaller),
// then sg=-1 (larger, smaller); biquadratic case: +-sqrt(y2a), +-sqrt(y2b)
__device__ __forceinline__ void quartic_real_roots(double b, double c, double d, double e, double (&roots)[4],
                                                   bool (&valid)[4])
{
    const double p = c - 3.0 * b * b / 8.0;
    const double q = d - b * c / 2.0 + b * b * b / 8.0;
    const double r = e - b * d / 4.0 + b * b * c / 16.0 - 3.0 * b * b * b * b / 256.0;
    const double sh = b / 4.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        roots[k] = 0.0;
        valid[k] = false;
    }
    if (q == 0.0) {
        const double disc = p * p - 4.0 * r;
        if (disc >= 0.0) {
            const double sd = dsqrt(disc);
            const double y2a = (-p + sd) / 2.0, y2b = (-p - sd) / 2.0;
            if (y2a >= 0.0) {
                const double y = dsqrt(y2a);
                roots[0] = y - sh;
                roots[1] = -y - sh;
                valid[0] = valid[1] = true;
            }
            if (y2b >= 0.0) {
                const double y = dsqrt(y2b);
                roots[2] = y - sh;
                roots[3] = -y - sh;
                valid[2] = valid[3] = true;
            }
        }
        return;
    }
    const double c1 = 2.0 * p * p - 8.0 * r, c0 = q * q;
    double hi = dabs(p);
    const double h1 = dabs(c1 / 8.0), h2 = dabs(c0 / 8.0);
    if (h1 > hi) hi = h1;
    if (h2 > hi) hi = h2;
    hi = hi + 1.0;
    double lo = 0.0;
    for (int it = 0; it < 64; ++it) {
        const double mid = 0.5 * (lo + hi);
        const double fm = ((8.0 * mid + 8.0 * p) * mid + c1) * mid - c0;
        const bool pos = fm > 0.0;
        hi = pos ? mid : hi;
        lo = pos ? lo : mid;
    }
    const double m = 0.5 * (lo + hi);
    const double s = dsqrt(2.0 * m);
    const double t = q / (2.0 * s);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double sg = k == 0 ? 1.0 : -1.0;
        const double cc = p / 2.0 + m + sg * t;
        const double disc = s * s - 4.0 * cc;
        if (disc >= 0.0) {
            const double sd = dsqrt(disc);
            roots[2 * k] = (sg * s + sd) / 2.0 - sh;
            roots[2 * k + 1] = (sg * s - sd) / 2.0 - sh;
            valid[2 * k] = valid[2 * k + 1] = true;
        }
    }
}

__device__ __forceinline__ double dot3r(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// orthonormal frame of a triangle P (3 points, row-major), columns e1, e2, e3
__device__ __forceinline__ void tri_frame(const double (&P)[9], double (&Fm)[9])
{
    double e1[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]};
    const double n1 = dsqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]);
    e1[0] = e1[0] / n1; e1[1] = e1[1] / n1; e1[2] = e1[2] / n1;
    const double d[3] = {P[6] - P[0], P[7] - P[1], P[8] - P[2]};
    double e3[3] = {e1[1] * d[2] - e1[2] * d[1], e1[2] * d[0] - e1[0] * d[2], e1[0] * d[1] - e1[1] * d[0]};
    const double n3 = dsqrt((e3[0] * e3[0] + e3[1] * e3[1]) + e3[2] * e3[2]);
    e3[0] = e3[0] / n3; e3[1] = e3[1] / n3; e3[2] = e3[2] / n3;
    const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Fm[k * 3 + 0] = e1[k];
        Fm[k * 3 + 1] = e2[k];
        Fm[k * 3 + 2] = e3[k];
    }
}

// division-free reprojection test (squared pixel error times zc^2 against err^2 zc^2, and zc > 0)
__device__ __forceinline__ bool pnp_inlier(const double (&R)[9], const double (&t)[3], double X0, double X1, double X2,
                                           double xi, double yi, double fx2, double fy2, double thr2, double &lhs,
                                           double &rhs)
{
    const double xc = dfma(R[0], X0, dfma(R[1], X1, dfma(R[2], X2, t[0])));
    const double yc = dfma(R[3], X0, dfma(R[4], X1, dfma(R[5], X2, t[1])));
    const double zc = dfma(R[6], X0, dfma(R[7], X1, dfma(R[8], X2, t[2])));
    const double dx = dfma(-xi, zc, xc), dy = dfma(-yi, zc, yc);
    lhs = dfma(fy2, dy * dy, fx2 * (dx * dx));
    rhs = thr2 * (zc * zc);
    return (zc > 0.0) && (lhs <= rhs);
}

// Grunert's P3P on 3 bearings / world points + disambiguation by a 4th correspondence.  returns false if no solution.
__device__ __forceinline__ bool p3p_select(const double (&f)[9], const double (&X)[9], const double (&X4)[3], double x4,
                                           double y4, double fx2, double fy2, double thr2, double (&Rb)[9],
                                           double (&tb)[3])
{
    const double d12[3] = {X[0] - X[3], X[1] - X[4], X[2] - X[5]};
    const double d13[3] = {X[0] - X[6], X[1] - X[7], X[2] - X[8]};
    const double d23[3] = {X[3] - X[6], X[4] - X[7], X[5] - X[8]};
    const double a2 = dot3r(d23, d23), b2 = dot3r(d13, d13), c2 = dot3r(d12, d12);
    const double ca = dot3r(&f[3], &f[6]), cb = dot3r(&f[0], &f[6]), cg = dot3r(&f[0], &f[3]);
    const double k1 = (a2 - c2) / b2, k2 = (a2 + c2) / b2, k3 = (b2 - c2) / b2, k4 = (b2 - a2) / b2;
    const double A4 = (k1 - 1.0) * (k1 - 1.0) - 4.0 * c2 / b2 * ca * ca;
    const double A3 = 4.0 * (k1 * (1.0 - k1) * cb - (1.0 - k2) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb);
    const double A2 = 2.0 * (k1 * k1 - 1.0 + 2.0 * k1 * k1 * cb * cb + 2.0 * k3 * ca * ca - 4.0 * k2 * ca * cb * cg +
                             2.0 * k4 * cg * cg);
    const double A1 = 4.0 * (-k1 * (1.0 + k1) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - k2) * ca * cg);
    const double A0 = (1.0 + k1) * (1.0 + k1) - 4.0 * a2 / b2 * cg * cg;
    double roots[4];
    bool valid[4];
    quartic_real_roots(A3 / A4, A2 / A4, A1 / A4, A0 / A4, roots, valid);
    double Fw[9];
    tri_frame(X, Fw);
    bool have = false;
    double sel_lhs = 0.0, sel_rhs = 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double v = roots[k];
        bool ok = valid[k] && (v > 0.0);
        const double u = ((-1.0 + k1) * v * v - 2.0 * k1 * cb * v + 1.0 + k1) / (2.0 * (cg - v * ca));
        ok = ok && (u > 0.0);
        if (ok) {  // divergent, but each branch is ~150 instructions and runs for most lanes of at most 2-4 slots
            const double s1 = dsqrt(c2 / (1.0 + u * u - 2.0 * u * cg));
            const double s2 = u * s1, s3 = v * s1;
            const double Pc[9] = {s1 * f[0], s1 * f[1], s1 * f[2], s2 * f[3], s2 * f[4], s2 * f[5],
                                  s3 * f[6], s3 * f[7], s3 * f[8]};
            double Fc[9], Rk[9], tk[3];
            tri_frame(Pc, Fc);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    Rk[i * 3 + j] = (Fc[i * 3 + 0] * Fw[j * 3 + 0] + Fc[i * 3 + 1] * Fw[j * 3 + 1]) + Fc[i * 3 + 2] * Fw[j * 3 + 2];
#pragma unroll
            for (int i = 0; i < 3; ++i)
                tk[i] = Pc[i] - dot3r(&Rk[3 * i], &X[0]);
            double lhs, rhs;
            pnp_inlier(Rk, tk, X4[0], X4[1], X4[2], x4, y4, fx2, fy2, thr2, lhs, rhs);
            // smallest squared pixel error on the 4th point, compared without dividing (rhs = err^2 zc^2 > 0)
            if ((rhs > 0.0) && (!have || lhs * sel_rhs < sel_lhs * rhs)) {
                have = true;
                sel_lhs = lhs;
                sel_rhs = rhs;
#pragma unroll
                for (int i = 0; i < 9; ++i)
                    Rb[i] = Rk[i];
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    tb[i] = tk[i];
            }
        }
    }
    return have;
}

// grid (ceil(stride/256), Q): ideal-camera coordinates and unit bearings
__global__ __launch_bounds__(256) void pnp_prep_kernel(PnpDev p)
{
    const int q = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n[q])
        return;
    const size_t o = (size_t)q * p.stride + i;
    const double *Ki = p.Kinv + (size_t)q * 9;
    const double u = p.uv[2 * o], v = p.uv[2 * o + 1];
    const double x = (Ki[0] * u + Ki[1] * v) + Ki[2];
    const double y = (Ki[3] * u + Ki[4] * v) + Ki[5];
    const double nn = dsqrt((x * x + y * y) + 1.0);
    p.xy[2 * o] = x;
    p.xy[2 * o + 1] = y;
    p.fb[3 * o] = x / nn;
    p.fb[3 * o + 1] = y / nn;
    p.fb[3 * o + 2] = 1.0 / nn;
}

constexpr int kPnpChunk = 768;
// grid (ceil(H/256), Q), block 256.
// Round 5: (1) the point stream goes through LDS in chunks of 768 points (36 KB: four workgroups per CU) -- the 2048-point
// array of rounds 2-4 (96 KB) left ONE workgroup per CU, four rounds of workgroups for the sequence's 998 tracks of ~570
// points; (2) a block with fewer than 129 live
// hypotheses -- the reference's iterationsCount is 100 -- has idle wavefronts: they take the same hypotheses and a share of the
// POINTS (wavefront w: hypothesis group w mod groups, points part, part + split, ...), and the integer counts are added up
// in LDS.  Every hypothesis is still solved and scored by the same operations on the same numbers: same counts, same winner.
__global__ __launch_bounds__(256) void pnp_ransac_kernel(PnpDev p)
{
    __shared__ __attribute__((aligned(16))) double s_pts[kPnpChunk * 6];  // a chunk of the point stream: X0 X1 X2 x y pad
    __shared__ int s_part[4][64];
    __shared__ int s_cnt[4];
    __shared__ uint32_t s_hyp[4];
    __shared__ uint32_t s_win;
    const int tid = threadIdx.x, q = blockIdx.y, n = p.n[q];
    PnpRec *rec = p.rec + (size_t)q * p.max_groups + blockIdx.x;
    if (n < 7) {  // pnp-solve.cpp:13,22 (the reference asserts)
        if (tid == 0) {
            rec->count = -1;
            rec->hyp = 0xffffffffu;
        }
        return;
    }
    const size_t o = (size_t)q * p.stride;
    const double *X = p.X + 3 * o, *xy = p.xy + 2 * o, *fb = p.fb + 3 * o;
    const double *K = p.K + (size_t)q * 9;
    const double fx2 = K[0] * K[0], fy2 = K[4] * K[4], thr2 = p.thr2;
    // hypotheses of this block: groups of 64 (one per lane); 4 / groups wavefronts share a group's points
    const int lane = tid & 63, wave = tid >> 6;
    const int in_block = min(p.num_hypotheses - (int)blockIdx.x * 256, 256);
    const int groups = (in_block + 63) >> 6, split = 4 / groups;          // 1, 2, 3, 4 groups -> 4, 2, 1, 1 parts
    const int grp = wave % groups, part = wave / groups;                   // (3 groups: wavefront 3 has part 1 >= split: idle)
    const uint32_t h = blockIdx.x * 256 + grp * 64 + lane;
    const bool live = h < (uint32_t)p.num_hypotheses && part < split;
    const uint32_t hh = h < (uint32_t)p.num_hypotheses ? h : (uint32_t)(p.num_hypotheses - 1);
    const uint64_t seed = p.seed + (p.gidx ? (uint64_t)p.gidx[q] : 0ull);
    int idx[4];
    sample4(seed, hh, n, p.sampler, idx);
    double f3[9], X3[9], X4[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f3[3 * k + c] = fb[3 * idx[k] + c];
            X3[3 * k + c] = X[3 * idx[k] + c];
        }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        X4[c] = X[3 * idx[3] + c];
    double R[9], t[3];
    const bool have = p3p_select(f3, X3, X4, xy[2 * idx[3]], xy[2 * idx[3] + 1], fx2, fy2, thr2, R, t);
    int cnt = 0;
    const bool score = part < split && __any(have);
    for (int c0 = 0; c0 < n; c0 += kPnpChunk) {   // the point stream in LDS chunks (n is the same for the whole block)
        const int cn = min(n - c0, kPnpChunk);
        __syncthreads();
        for (int i = tid; i < cn; i += 256) {
            s_pts[6 * i + 0] = X[3 * (c0 + i)];
            s_pts[6 * i + 1] = X[3 * (c0 + i) + 1];
            s_pts[6 * i + 2] = X[3 * (c0 + i) + 2];
            s_pts[6 * i + 3] = xy[2 * (c0 + i)];
            s_pts[6 * i + 4] = xy[2 * (c0 + i) + 1];
            s_pts[6 * i + 5] = 0.0;
        }
        __syncthreads();
        if (score) {
#pragma unroll 4
            for (int i = part; i < cn; i += split) {
                const double *pt = &s_pts[6 * i];  // wave-uniform address: LDS broadcast
                double lhs, rhs;
                cnt += pnp_inlier(R, t, pt[0], pt[1], pt[2], pt[3], pt[4], fx2, fy2, thr2, lhs, rhs) ? 1 : 0;
            }
        }
    }
    s_part[wave][lane] = cnt;
    __syncthreads();
    if (part == 0) {
        cnt = 0;
        for (int k = 0; k < split; ++k)
            cnt += s_part[grp + k * groups][lane];
    }
    if (!have || !live || part != 0)
        cnt = -1;
    // workgroup arg-best: most inliers, then the smaller hypothesis id (first maximum of the sequential loop)
    int bc = cnt;
    uint32_t bh = h;
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) {
        const int oc = __shfl_xor(bc, o2);
        const uint32_t oh = __shfl_xor(bh, o2);
        if (oc > bc || (oc == bc && oh < bh)) {
            bc = oc;
            bh = oh;
        }
    }
    if (lane == 0) {
        s_cnt[wave] = bc;
        s_hyp[wave] = bh;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (s_cnt[w] > bc || (s_cnt[w] == bc && s_hyp[w] < bh)) {
                bc = s_cnt[w];
                bh = s_hyp[w];
            }
        s_win = bh;
        rec->count = bc;
        rec->hyp = bh;
    }
    __syncthreads();
    if (h == s_win && part == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i)
            rec->R[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            rec->t[i] = t[i];
    }
}

// grid Q, block 256
__global__ __launch_bounds__(256) void pnp_finalize_kernel(PnpDev p)
{
    __shared__ int s_tot[4];
    __shared__ double s_R[9], s_t[3];
    __shared__ int s_ok;
    const int tid = threadIdx.x, q = blockIdx.x, n = p.n[q];
    const int G = (p.num_hypotheses + 255) / 256;
    const PnpRec *rec = p.rec + (size_t)q * p.max_groups;
    PnpOut *out = p.out + q;
    if (tid == 0) {
        int bc = -1, bg = -1;
        uint32_t bh = 0xffffffffu;
        if (n >= 7) {
            for (int g = 0; g < G; ++g) {
                const int c = rec[g].count;
                const uint32_t h = rec[g].hyp;
                if (c >= 0 && (c > bc || (c == bc && h < bh))) {
                    bc = c;
                    bh = h;
                    bg = g;
                }
            }
        }
        const bool ok = bg >= 0 && bc >= p.min_inliers;
        s_ok = ok ? 1 : 0;
        out->ok = ok ? 1 : 0;
        out->best_hyp = bg >= 0 ? (int)bh : -1;
        out->n_inliers = 0;
        if (ok) {
#pragma unroll
            for (int i = 0; i < 9; ++i)
                s_R[i] = rec[bg].R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i)
                s_t[i] = rec[bg].t[i];
        }
    }
    __syncthreads();
    if (!s_ok) {
        // rows of the inlier list behind n_inliers are cleared on every run (a download of the whole capacity is deterministic)
        int32_t *z = p.inliers + (size_t)q * p.stride;
        for (int i = tid; i < p.stride; i += 256)
            z[i] = 0;
        return;
    }
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i)
        R[i] = s_R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        t[i] = s_t[i];
    const size_t o = (size_t)q * p.stride;
    const double *X = p.X + 3 * o, *xy = p.xy + 2 * o;
    const double *K = p.K + (size_t)q * 9;
    const double fx2 = K[0] * K[0], fy2 = K[4] * K[4];
    int32_t *inl = p.inliers + o;
    // ordered inlier list
    const int lane = tid & 63, w = tid >> 6;
    int basepos = 0;
    for (int start = 0; start < n; start += 256) {
        const int i = start + tid;
        bool flag = false;
        if (i < n) {
            double lhs, rhs;
            flag = pnp_inlier(R, t, X[3 * i], X[3 * i + 1], X[3 * i + 2], xy[2 * i], xy[2 * i + 1], fx2, fy2, p.thr2, lhs, rhs);
        }
        const unsigned long long bal = __ballot(flag);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0)
            s_tot[w] = __popcll(bal);
        __syncthreads();
        int off = basepos, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = s_tot[k];
            off += (k < w) ? v : 0;
            tot += v;
        }
        if (flag)
            inl[off + pre] = i;
        basepos += tot;
        __syncthreads();
    }
    for (int i = basepos + tid; i < p.stride; i += 256)
        inl[i] = 0;
    if (tid == 0) {
        out->n_inliers = basepos;
        // pose = SE3(SO3(R), t).inverse() (pnp-solve.cpp:99-101; lie-group.hpp:31-36,212-216)
        double Rr[3][3], RT[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                Rr[i][j] = R[i * 3 + j];
                out->Rw2c[i * 3 + j] = R[i * 3 + j];
            }
        rectify3(Rr);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                RT[i][j] = Rr[j][i];
        rectify3(RT);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            out->tw2c[i] = t[i];
            out->t[i] = -((RT[i][0] * t[0] + RT[i][1] * t[1]) + RT[i][2] * t[2]);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                out->R[i * 3 + j] = RT[i][j];
        }
    }
}

// grid n_tracks, block 256.  Track q: pair a = q (frames q, q+1), pair b = q + 1 (frames q+1, q+2).
// point j of pair a belongs to match m = point_idx[a][j], whose queryIdx is a keypoint index of frame q+1; every
// match m' of pair b whose trainIdx is that keypoint observes the same point in frame q+2 (queryIdx of m').
// Correspondences are emitted in the order of pair b's match list (visual-odometer.cpp:528-556 restated as a join).
__global__ __launch_bounds__(256) void seq_join_kernel(SeqJoinDev j)
{
    __shared__ int16_t s_tbl[kMaxKp];
    __shared__ int s_tot[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int a = q, b = q + 1;
    const size_t N = j.max_kp;
    const bool valid = j.results[a].valid != 0;
    const int npts = valid ? j.results[a].n_points : 0;
    const int Mb = min(j.M[b], j.max_kp);
    for (int i = tid; i < j.max_kp; i += 256)
        s_tbl[i] = -1;
    __syncthreads();
    for (int p = tid; p < npts; p += 256) {
        const int m = j.point_idx[a * N + p];
        s_tbl[j.matches[a * N + m].queryIdx] = (int16_t)p;  // queryIdx values are unique within one match list
    }
    __syncthreads();
    const float *kp2 = j.kp + (size_t)(q + 2) * N * 2;
    double *X = j.X + (size_t)q * j.stride * 3, *uv = j.uv + (size_t)q * j.stride * 2;
    int basepos = 0;
    for (int start = 0; start < Mb; start += 256) {
        const int m = start + tid;
        int p = -1, qi = 0;
        if (m < Mb) {
            const mvs_match mt = j.matches[b * N + m];
            p = s_tbl[mt.trainIdx];
            qi = mt.queryIdx;
        }
        const bool flag = p >= 0;
        const unsigned long long bal = __ballot(flag);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0)
            s_tot[w] = __popcll(bal);
        __syncthreads();
        int off = basepos, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = s_tot[k];
            off += (k < w) ? v : 0;
            tot += v;
        }
        const int pos = off + pre;
        if (flag && pos < j.stride) {
            const double *src = j.points + ((size_t)a * N + p) * 3;
            X[3 * pos] = src[0];
            X[3 * pos + 1] = src[1];
            X[3 * pos + 2] = src[2];
            uv[2 * pos] = (double)kp2[2 * qi];       // visual-feature.cpp:179-190 float -> double
            uv[2 * pos + 1] = (double)kp2[2 * qi + 1];
        }
        basepos += tot;
        __syncthreads();
    }
    if (tid == 0)
        j.n_corr[q] = min(basepos, j.stride);
}

void launch_seq_join(const SeqJoinDev &j, hipStream_t stream)
{
    hipLaunchKernelGGL(seq_join_kernel, dim3(j.n_tracks), dim3(256), 0, stream, j);
}

// ---- the tracking loop of a resident sequence (mvs_seq_track) -------------------------------------
// Glue kernels of one step, one workgroup of 256 each.  The arithmetic they do themselves (scale, a new point's position) is
// written in the order the header states, + * sqrt only, no fma.
namespace {

// point j of pair k: base keypoint a (frame k), new keypoint b (frame k + 1); false for indices outside the frame arrays
__device__ __forceinline__ bool vo_point(const VoDev &d, int k, int j, int &a, int &b)
{
    const int N = d.max_kp;
    const size_t o = (size_t)k * N;
    const int r = d.point_idx[o + j];
    if ((unsigned)r >= (unsigned)N)
        return false;
    const mvs_match mt = d.matches[o + r];
    a = mt.trainIdx;
    b = mt.queryIdx;
    return (unsigned)a < (unsigned)N && (unsigned)b < (unsigned)N;
}

// s_first[a] = the smallest point j of pair k with base keypoint a (INT_MAX: none): point j is kept iff s_first[a_j] == j.
// A minimum does not depend on the order the points arrive in.  Returns the pair's point count; ends with a barrier.
__device__ __forceinline__ int vo_first_table(const VoDev &d, int k, bool valid, int *s_first)
{
    const int N = d.max_kp, tid = threadIdx.x;
    const int npts = valid ? min(max(d.results[k].n_points, 0), N) : 0;
    for (int i = tid; i < N; i += 256)
        s_first[i] = INT_MAX;
    __syncthreads();
    for (int j = tid; j < npts; j += 256) {
        int a, b;
        if (vo_point(d, k, j, a, b))
            atomicMin(&s_first[a], j);
    }
    __syncthreads();
    return npts;
}

// position of a flagged thread among the flagged threads of the workgroup, in thread order, behind `basepos` (which moves on
// by their number): the ballot compaction of seq_join_kernel.  Every thread of the workgroup calls it.
__device__ __forceinline__ int vo_compact(bool flag, int *s_tot, int &basepos)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0)
        s_tot[w] = __popcll(bal);
    __syncthreads();
    int off = basepos, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int v = s_tot[k];
        off += (k < w) ? v : 0;
        tot += v;
    }
    basepos += tot;
    __syncthreads();
    return off + pre;
}

// grid 1.  Frames k0 and k0 + 1, the map the run starts with, the loop's state words.
__global__ __launch_bounds__(256) void vo_init_kernel(VoDev d)
{
    __shared__ int s_first[kMaxKp];
    __shared__ int s_tot[4];
    const int tid = threadIdx.x, N = d.max_kp, k = d.k0;
    const mvs_pair_result &res = d.results[k];
    const bool valid = res.valid != 0 && (!d.use_refined || d.refined[k].ok != 0);
    const int npts = vo_first_table(d, k, valid, s_first);
    for (int f = tid; f < d.n_frames; f += 256)
        d.gidx[f] = f;
    int32_t *mid = d.map_id + (size_t)(k + 1) * N;
    double *mX = d.map_X + (size_t)(k + 1) * N * 3;
    const double *x = (d.use_refined ? d.refined_pts : d.points) + (size_t)k * N * 3;
    int basepos = 0;
    for (int start = 0; start < npts; start += 256) {
        const int j = start + tid;
        int a = 0, b = 0;
        const bool flag = j < npts && vo_point(d, k, j, a, b) && s_first[a] == j;
        const int pos = vo_compact(flag, s_tot, basepos);
        if (flag) {   // queryIdx values are unique within one match list
            mid[b] = pos;
            mX[3 * b] = x[3 * j];
            mX[3 * b + 1] = x[3 * j + 1];
            mX[3 * b + 2] = x[3 * j + 2];
        }
    }
    if (tid == 0) {
        const double *R = d.use_refined ? d.refined[k].R : res.R, *t = d.use_refined ? d.refined[k].t : res.t;
        mvs_track_frame a{}, b{};
        a.state = MVS_TRACK_INIT;
        a.pnp_best_hyp = b.pnp_best_hyp = -1;
        a.R[0] = a.R[4] = a.R[8] = 1.0;
        b.state = valid ? MVS_TRACK_INIT : MVS_TRACK_LOST_PNP;
        if (valid) {
            b.n_new = basepos;
            for (int i = 0; i < 9; ++i)
                b.R[i] = d.T_last[i] = R[i];
            for (int i = 0; i < 3; ++i)
                b.t[i] = d.T_last[9 + i] = t[i];
        }
        d.frames[k] = a;
        d.frames[k + 1] = b;
        d.state[0] = valid ? 1 : 0;
        d.state[1] = basepos;
    }
}

// grid 1.  Step f, pair k = f - 1: the kept points whose base keypoint has a map entry, in point order, become frame f's PnP
// problem (visual-odometer.cpp:519-555).
__global__ __launch_bounds__(256) void vo_join_kernel(VoDev d, int f)
{
    __shared__ int s_first[kMaxKp];
    __shared__ int s_tot[4];
    const int tid = threadIdx.x, N = d.max_kp, k = f - 1;
    if (d.state[0] == 0) {   // written by earlier kernels only: uniform
        if (tid == 0)
            d.n_cand[f] = 0;
        return;
    }
    const int npts = vo_first_table(d, k, d.results[k].valid != 0, s_first);
    const size_t of = (size_t)f * N, ol = (size_t)(f - 1) * N;
    const int32_t *mid = d.map_id + ol;
    const double *mX = d.map_X + 3 * ol;
    const float *kpf = d.kp + 2 * of;
    int32_t *ca = d.cand_a + of, *cb = d.cand_b + of;
    double *X = d.cand_X + 3 * of, *uv = d.cand_uv + 2 * of;
    int basepos = 0;
    for (int start = 0; start < npts; start += 256) {
        const int j = start + tid;
        int a = 0, b = 0;
        const bool flag = j < npts && vo_point(d, k, j, a, b) && s_first[a] == j && mid[a] >= 0;
        const int pos = vo_compact(flag, s_tot, basepos);
        if (flag) {   // pos < npts <= N
            ca[pos] = a;
            cb[pos] = b;
            X[3 * pos] = mX[3 * a];
            X[3 * pos + 1] = mX[3 * a + 1];
            X[3 * pos + 2] = mX[3 * a + 2];
            uv[2 * pos] = (double)kpf[2 * b];       // visual-feature.cpp:179-190 float -> double
            uv[2 * pos + 1] = (double)kpf[2 * b + 1];
        }
    }
    if (tid == 0)
        d.n_cand[f] = basepos;
}

// grid 1.  Step f behind its PnP: the gates, the scale, and the two-frame problem of visual-odometer.cpp:618-800 as
// mvs_ba_refine takes it -- covariances and flags for refine_prep_kernel, so that the informations are that entry's.
__global__ __launch_bounds__(256) void vo_assemble_kernel(VoDev d, int f)
{
    __shared__ int s_first[kMaxKp];
    __shared__ int s_tot[4];
    const int tid = threadIdx.x, N = d.max_kp, k = f - 1;
    const int alive = d.state[0], id0 = d.state[1];
    double Tl[12];
#pragma unroll
    for (int i = 0; i < 12; ++i)
        Tl[i] = d.T_last[i];
    __syncthreads();   // thread 0 writes the state words below
    if (alive == 0) {
        if (tid == 0)
            d.m[f] = 0;
        return;
    }
    const PnpOut &po = d.pnp_out[f];
    const int nc = d.n_cand[f];
    const bool pnp_ok = nc >= 7 && po.ok != 0;   // pnp-solve.cpp:13,22
    const int n_inl = pnp_ok ? min(max(po.n_inliers, 0), nc) : 0;
    double scale = 0.0;
    if (pnp_ok) {
        const double e0 = po.t[0] - Tl[9], e1 = po.t[1] - Tl[10], e2 = po.t[2] - Tl[11];
        scale = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    }
    mvs_track_frame fr{};
    fr.n_cand = nc;
    fr.n_pnp_inliers = n_inl;
    fr.pnp_best_hyp = nc >= 7 ? po.best_hyp : -1;
    fr.scale = scale;
    if (pnp_ok) {
        for (int i = 0; i < 9; ++i)
            fr.R_pnp[i] = po.R[i];
        for (int i = 0; i < 3; ++i)
            fr.t_pnp[i] = po.t[i];
    }
    if (!pnp_ok || n_inl < d.min_pnp_points) {
        if (tid == 0) {
            fr.state = pnp_ok ? MVS_TRACK_LOST_FEW : MVS_TRACK_LOST_PNP;
            d.frames[f] = fr;
            d.m[f] = 0;
            d.state[0] = 0;
        }
        return;
    }
    const size_t of = (size_t)f * N, ol = (size_t)(f - 1) * N;
    const int32_t *mid = d.map_id + ol, *ca = d.cand_a + of, *cb = d.cand_b + of, *inl = d.inliers + of;
    const double *cX = d.cand_X + 3 * of;
    const float *kpl = d.kp + 2 * ol, *kpf = d.kp + 2 * of;
    const uint8_t *ocl = d.oct + ol, *ocf = d.oct + of;
    int32_t *pid = d.pt_id + of, *pkp = d.pt_kp + 2 * of;
    uint8_t *pnew = d.pt_new + of;
    double *guess = d.guess + 3 * of;
    auto put = [&](int p, int id, int a, int b, bool is_new, double X0, double X1, double X2) {
        pid[p] = id;
        pkp[2 * p] = a;
        pkp[2 * p + 1] = b;
        pnew[p] = is_new ? 1 : 0;
        guess[3 * p] = X0, guess[3 * p + 1] = X1, guess[3 * p + 2] = X2;
        d.obs0[2 * p] = (double)kpl[2 * a], d.obs0[2 * p + 1] = (double)kpl[2 * a + 1];
        d.obs1[2 * p] = (double)kpf[2 * b], d.obs1[2 * p + 1] = (double)kpf[2 * b + 1];
        // VisualFeature::get_point_estimates: stddev = 2^octave * sigma_px (a power of two scales exactly)
        const double s0 = ldexp(d.sigma_px, min((int)ocl[a], kSeqWinMaxOctave));
        const double s1 = ldexp(d.sigma_px, min((int)ocf[b], kSeqWinMaxOctave));
        const double v0 = s0 * s0, v1 = s1 * s1, pv = is_new ? 0.0 : d.point_var;   // no prior on a new point
        d.cov0[4 * p] = v0, d.cov0[4 * p + 1] = 0.0, d.cov0[4 * p + 2] = 0.0, d.cov0[4 * p + 3] = v0;
        d.cov1[4 * p] = v1, d.cov1[4 * p + 1] = 0.0, d.cov1[4 * p + 2] = 0.0, d.cov1[4 * p + 3] = v1;
#pragma unroll
        for (int e = 0; e < 9; ++e)
            d.cov3[9 * p + e] = (e % 4 == 0) ? pv : 0.0;
    };
    // tracked points: the PnP inliers in candidate order, where the map has them
    for (int i = tid; i < n_inl; i += 256) {
        const int c = min(max(inl[i], 0), nc - 1);
        const int a = ca[c], b = cb[c];
        put(i, mid[a], a, b, false, cX[3 * c], cX[3 * c + 1], cX[3 * c + 2]);
    }
    // new points: the kept points of the pair whose base keypoint the map does not hold, scaled and moved into the init frame
    const int npts = vo_first_table(d, k, d.results[k].valid != 0, s_first);
    const double *x = d.points + 3 * ol;   // pair k's points: [k][N][3]
    int basepos = 0;
    for (int start = 0; start < npts; start += 256) {
        const int j = start + tid;
        int a = 0, b = 0;
        const bool flag = j < npts && vo_point(d, k, j, a, b) && s_first[a] == j && mid[a] < 0;
        const int pos = vo_compact(flag, s_tot, basepos);
        if (flag && n_inl + pos < N) {   // tracked + new <= kept points <= N: the bound never cuts
            const double y0 = scale * x[3 * j], y1 = scale * x[3 * j + 1], y2 = scale * x[3 * j + 2];
            put(n_inl + pos, id0 + pos, a, b, true, ((Tl[0] * y0 + Tl[1] * y1) + Tl[2] * y2) + Tl[9],
                ((Tl[3] * y0 + Tl[4] * y1) + Tl[5] * y2) + Tl[10], ((Tl[6] * y0 + Tl[7] * y1) + Tl[8] * y2) + Tl[11]);
        }
    }
    if (tid == 0) {
        const int n_new = min(basepos, N - n_inl);
        double *pose = d.pose0 + 24 * (size_t)f;
        for (int i = 0; i < 12; ++i)
            pose[i] = Tl[i];
        for (int i = 0; i < 9; ++i)
            pose[12 + i] = po.R[i];
        for (int i = 0; i < 3; ++i)
            pose[21 + i] = po.t[i];
        fr.n_tracked = n_inl;
        fr.n_new = n_new;
        d.frames[f] = fr;   // the state stays 0 until vo_commit_kernel has seen the BA
        d.m[f] = n_inl + n_new;
        d.state[1] = id0 + n_new;
    }
}

// grid 1.  Step f behind its BA: the error gate (visual-odometer.cpp:479-483), T_last and map[f] (:485-498).
__global__ __launch_bounds__(256) void vo_commit_kernel(VoDev d, int f)
{
    const int tid = threadIdx.x, N = d.max_kp;
    const int alive = d.state[0];
    __syncthreads();   // thread 0 may clear the word below
    if (alive == 0)
        return;
    const mvs_refine_result &r = d.ba_out[2 * (size_t)f + 1];   // the new frame
    const int m = min(max(d.m[f], 0), N);
    const int st = r.ok == 0 ? MVS_TRACK_LOST_BA : (r.error > d.max_error ? MVS_TRACK_LOST_ERROR : MVS_TRACK_TRACKED);
    if (tid == 0) {
        mvs_track_frame &fr = d.frames[f];
        fr.state = st;
        fr.iterations = r.iterations;
        fr.error = r.error;
        if (st == MVS_TRACK_TRACKED) {
            for (int i = 0; i < 9; ++i)
                fr.R[i] = d.T_last[i] = r.R[i];
            for (int i = 0; i < 3; ++i)
                fr.t[i] = d.T_last[9 + i] = r.t[i];
        } else {
            d.state[0] = 0;
        }
    }
    if (st != MVS_TRACK_TRACKED)
        return;
    const size_t of = (size_t)f * N;
    const int32_t *pid = d.pt_id + of, *pkp = d.pt_kp + 2 * of;
    const double *P = d.pts + 3 * of;
    int32_t *mid = d.map_id + of;
    double *mX = d.map_X + 3 * of;
    for (int p = tid; p < m; p += 256) {
        const int b = pkp[2 * p + 1];   // < N (vo_point); unique within the problem
        mid[b] = pid[p];
        mX[3 * b] = P[3 * p];
        mX[3 * b + 1] = P[3 * p + 1];
        mX[3 * b + 2] = P[3 * p + 2];
    }
}

// ---- lagged pairs and VisualOdometer::add_frame (mvs_seq_run_lags, mvs_seq_odometry) ---------------
// grid n_pairs, block 256.  Integer sum: the order of the additions does not matter.
__global__ __launch_bounds__(256) void pair_ssd_kernel(const mvs_pair_result *results, const mvs_match *matches,
                                                       const int32_t *point_idx, int N, int32_t *ssd)
{
    __shared__ int s_sum[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const mvs_pair_result &res = results[k];
    const int npts = res.valid != 0 ? min(max(res.n_points, 0), N) : 0;
    const size_t o = (size_t)k * N;
    int sum = 0;
    for (int j = tid; j < npts; j += 256) {
        const int r = point_idx[o + j];
        if ((unsigned)r < (unsigned)N) {
            const int dist = (int)matches[o + r].distance;   // an integer Hamming distance held in a float
            sum += dist * dist;
        }
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
            s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    if (tid == 0)
        ssd[k] = s_sum[0];
}

// grid 1, block 1.
__global__ void lag_table_set_kernel(LagDev *table, int lag, LagDev entry)
{
    table[lag] = entry;
}

// grid 1, block 64.  The words a run starts from: INITIALIZING (state[0] = 0 by the host's memset), an empty queue that starts
// at frame 0, no segment yet, the PnP's sampler key offsets.
__global__ __launch_bounds__(64) void vo_odo_begin_kernel(VoDev d, OdoDev o)
{
    const int tid = threadIdx.x;
    for (int f = tid; f < d.n_frames; f += 64)
        d.gidx[f] = f;
    if (tid == 0) {
        o.q[0] = 0;
        o.q[1] = -1;
        o.q[2] = o.q[3] = o.q[4] = 0;
        mvs_odo_frame r{};
        r.segment = -1;
        r.init_base = -1;
        o.odo[0] = r;
    }
}

// check_image_pair (visual-odometer.cpp:353-379) of a held pair with base frame b: 0 passed, else the first gate that fails in
// the reference's order.  rot_sq / abs_tz are those of the refined pose whenever the pair is valid (a valid held pair has
// been refined), 0 otherwise.  SO3::ln in the operation order of the shim (mvslam_compat.hpp:176-184).
__device__ __forceinline__ int vo_check_pair(const OdoDev &o, const OdoHeld &h, int b, double &rot_sq, double &abs_tz)
{
    rot_sq = 0.0;
    abs_tz = 0.0;
    if (!h.valid)
        return 1;
    const mvs_refine_result &r = o.lags[h.lag].refined[b];
    double c = 0.5 * (((r.R[0] + r.R[4]) + r.R[8]) - 1.0);
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double theta = acos(c);
    const double v0 = r.R[7] - r.R[5], v1 = r.R[2] - r.R[6], v2 = r.R[3] - r.R[1];
    const double A = theta < 1e-5 ? (1.0 + theta * theta / 6.0) * 0.5 : 0.5 * theta / sin(theta);
    const double w0 = v0 * A, w1 = v1 * A, w2 = v2 * A;
    rot_sq = (w0 * w0 + w1 * w1) + w2 * w2;
    abs_tz = fabs(r.t[2]);
    if (h.count < o.min_inliers)
        return 2;
    if (h.error > o.max_error)
        return 3;
    if (rot_sq > o.max_rot_sq)
        return 4;
    if (abs_tz > o.max_tz)
        return 5;
    return 0;
}

// grid 1, block 64.  Frame f behind its step's kernels: what add_frame does around track() / initialize().
//   queue   the frame is pushed before it is processed (visual-odometer.cpp:138) and the oldest frame is popped afterwards
//           if the queue then holds more than Q frames (:181-190), so the queue holds at most Q after every frame and at most
//           Q + 1 while frame f is processed: frames max(q0, f - Q) .. f, largest lag Q; afterwards q0 = max(q0, f - Q + 1).
//           reset() (:203-217) keeps the last frame only: q0 = f, and no pop follows.
//   TRACKING at entry: the step's kernels have written frames[f].state (2 .. 6).  A LOST_* state is reset(): state[0] is 0
//           already (vo_assemble_kernel / vo_commit_kernel), q0 = f; the held pairs before f are never read again.
//   INITIALIZING at entry (frames[f].state is still 0): held[f - 1] = the new adjacent pair, refined when valid (:283-286);
//           ImagePair::update of every older queued base frame against the lagged pair (b, f) (:288-296), one lane per base
//           frame; then the scan, oldest first (:315-345), by thread 0.
__global__ __launch_bounds__(64) void vo_queue_kernel(VoDev d, OdoDev o, int f)
{
    __shared__ int s_upd;
    const int tid = threadIdx.x, Q = o.queue_size;
    const int st_f = d.frames[f].state, q0 = o.q[0], seg = o.q[1];
    const int qf = max(q0, f - Q);
    if (tid == 0)
        s_upd = 0;
    __syncthreads();   // thread 0 writes the words read above
    mvs_odo_frame rec{};
    rec.segment = seg;
    rec.init_base = -1;
    rec.queue_first = qf;
    if (st_f != MVS_TRACK_NOT_REACHED) {
        if (tid == 0) {
            const bool tracked = st_f == MVS_TRACK_TRACKED;
            rec.mode_after = tracked ? 1 : 0;
            o.odo[f] = rec;
            o.q[0] = tracked ? max(q0, f - Q + 1) : f;
            o.q[4] = 0;
        }
        return;
    }
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    if (tid == 0) {
        const LagDev &L = o.lags[1];
        const mvs_pair_result &res = L.results[f - 1];
        OdoHeld h{};
        h.pair = f;
        h.lag = 1;
        h.valid = res.valid != 0;
        h.count = h.valid ? res.n_points : 0;
        h.ssd = h.valid ? L.ssd[f - 1] : 0;
        h.error = inf;
        if (h.valid) {
            const mvs_refine_result &rr = L.refined[f - 1];
            h.valid = h.refined = rr.ok != 0;
            if (rr.ok != 0)
                h.error = rr.error;
        }
        o.held[f - 1] = h;
    }
    for (int b = qf + tid; b < f - 1; b += 64) {   // lag f - b <= Q: b >= f - Q
        const int lag = f - b;
        const LagDev &L = o.lags[lag];
        const mvs_pair_result &res = L.results[b];
        const OdoHeld h = o.held[b];
        if (res.valid == 0)
            continue;
        const int cnt = res.n_points, ssd = L.ssd[b];
        if (cnt < h.count || ssd < h.ssd)
            continue;
        const mvs_refine_result &rr = L.refined[b];
        const double err = rr.ok != 0 ? rr.error : inf;
        if (err < h.error) {   // so the refinement succeeded
            OdoHeld n{};
            n.pair = f;
            n.lag = lag;
            n.valid = n.refined = 1;
            n.count = cnt;
            n.ssd = ssd;
            n.error = err;
            o.held[b] = n;
            atomicAdd(&s_upd, 1);
        }
    }
    __threadfence_block();
    __syncthreads();
    if (tid != 0)
        return;
    int chosen = -1;
    double rot = 0.0, tz = 0.0;
    for (int b = qf; b < f; ++b) {
        const OdoHeld h = o.held[b];
        double r2, az;
        const int code = vo_check_pair(o, h, b, r2, az);
        if (b == f - 1) {
            rec.gate_fail = code;
            rot = r2;
            tz = az;
        }
        if (code == 0 && h.pair == f) {   // the reference asserts the latter (:327)
            chosen = b;
            rot = r2;
            tz = az;
            break;
        }
    }
    rec.n_updated = s_upd;
    rec.rot_sq = rot;
    rec.abs_tz = tz;
    if (chosen >= 0) {
        rec.mode_after = 1;
        rec.segment = seg + 1;
        rec.init_base = chosen;
        rec.gate_fail = 0;
        o.q[1] = seg + 1;
        o.q[2] = o.held[chosen].lag;
        o.q[3] = chosen;
    } else {
        mvs_track_frame fr{};
        fr.state = MVS_TRACK_INITIALIZING;
        d.frames[f] = fr;
    }
    o.q[4] = chosen >= 0 ? 1 : 0;
    o.q[0] = max(q0, f - Q + 1);
    o.odo[f] = rec;
}

// grid 1.  vo_init_kernel for the pair vo_queue_kernel chose: base frame b, lag f - b, refined pose and points; ids go on from
// the call's counter.  A base frame that is the lost frame of the segment before keeps its LOST_* record.
__global__ __launch_bounds__(256) void vo_map_init_kernel(VoDev d, OdoDev o, int f)
{
    __shared__ int s_first[kMaxKp];
    __shared__ int s_tot[4];
    const int tid = threadIdx.x, N = d.max_kp;
    if (o.q[4] == 0)   // written by vo_queue_kernel only: uniform
        return;
    const int lag = o.q[2], k = o.q[3], id0 = d.state[1];
    const LagDev L = o.lags[lag];
    VoDev e = d;   // vo_point / vo_first_table on the lag's tables
    e.results = L.results;
    e.matches = L.matches;
    e.point_idx = L.point_idx;
    const int npts = vo_first_table(e, k, true, s_first);
    int32_t *mid = d.map_id + (size_t)f * N;
    double *mX = d.map_X + (size_t)f * N * 3;
    const double *x = L.refined_pts + (size_t)k * N * 3;
    int basepos = 0;
    for (int start = 0; start < npts; start += 256) {
        const int j = start + tid;
        int a = 0, b = 0;
        const bool flag = j < npts && vo_point(e, k, j, a, b) && s_first[a] == j;
        const int pos = vo_compact(flag, s_tot, basepos);
        if (flag) {
            mid[b] = id0 + pos;
            mX[3 * b] = x[3 * j];
            mX[3 * b + 1] = x[3 * j + 1];
            mX[3 * b + 2] = x[3 * j + 2];
        }
    }
    if (tid == 0) {
        const mvs_refine_result &r = L.refined[k];
        mvs_track_frame a{}, b{};
        a.state = b.state = MVS_TRACK_INIT;
        a.pnp_best_hyp = b.pnp_best_hyp = -1;
        a.R[0] = a.R[4] = a.R[8] = 1.0;
        b.n_new = basepos;
        for (int i = 0; i < 9; ++i)
            b.R[i] = d.T_last[i] = r.R[i];
        for (int i = 0; i < 3; ++i)
            b.t[i] = d.T_last[9 + i] = r.t[i];
        const int sk = d.frames[k].state;
        if (sk < MVS_TRACK_LOST_PNP || sk > MVS_TRACK_LOST_ERROR)
            d.frames[k] = a;
        d.frames[f] = b;
        d.state[0] = 1;
        d.state[1] = id0 + basepos;
    }
}

}  // namespace

void launch_pair_ssd(const mvs_pair_result *results, const mvs_match *matches, const int32_t *point_idx, int n_pairs, int max_kp,
                     int32_t *ssd, hipStream_t stream)
{
    hipLaunchKernelGGL(pair_ssd_kernel, dim3(n_pairs), dim3(256), 0, stream, results, matches, point_idx, max_kp, ssd);
}
void launch_lag_table_set(LagDev *table, int lag, const LagDev &entry, hipStream_t stream)
{
    hipLaunchKernelGGL(lag_table_set_kernel, dim3(1), dim3(1), 0, stream, table, lag, entry);
}
void launch_vo_odo_begin(const VoDev &d, const OdoDev &o, hipStream_t stream)
{
    hipLaunchKernelGGL(vo_odo_begin_kernel, dim3(1), dim3(64), 0, stream, d, o);
}
void launch_vo_queue(const VoDev &d, const OdoDev &o, int f, hipStream_t stream)
{
    hipLaunchKernelGGL(vo_queue_kernel, dim3(1), dim3(64), 0, stream, d, o, f);
}
void launch_vo_map_init(const VoDev &d, const OdoDev &o, int f, hipStream_t stream)
{
    hipLaunchKernelGGL(vo_map_init_kernel, dim3(1), dim3(256), 0, stream, d, o, f);
}

void launch_vo_init(const VoDev &d, hipStream_t stream)
{
    hipLaunchKernelGGL(vo_init_kernel, dim3(1), dim3(256), 0, stream, d);
}
void launch_vo_join(const VoDev &d, int f, hipStream_t stream)
{
    hipLaunchKernelGGL(vo_join_kernel, dim3(1), dim3(256), 0, stream, d, f);
}
void launch_vo_assemble(const VoDev &d, int f, hipStream_t stream)
{
    hipLaunchKernelGGL(vo_assemble_kernel, dim3(1), dim3(256), 0, stream, d, f);
}
void launch_vo_commit(const VoDev &d, int f, hipStream_t stream)
{
    hipLaunchKernelGGL(vo_commit_kernel, dim3(1), dim3(256), 0, stream, d, f);
}

// ---- sliding windows of a sequence: links between consecutive frames, then the windows' problems 
// grid n_frames - 1, block 256.  Pair k: a link is an inlier row r < n_matches of a valid pair; it joins keypoint trainIdx of
// frame k to keypoint queryIdx of frame k + 1.  Rows that share a trainIdx: the smallest row wins (a minimum does not depend
// on the order the rows arrive in), the others are dropped; queryIdx values are unique within one match list.  So every
// keypoint has at most one successor and one predecessor.  Also inverts point_idx: row_to_point[k][r].
__global__ __launch_bounds__(256) void seq_link_kernel(SeqWinDev d)
{
    __shared__ int s_row[kMaxKp];
    const int k = blockIdx.x, tid = threadIdx.x, N = d.max_kp;
    const size_t o = (size_t)k * N;
    const mvs_pair_result &res = d.results[k];
    const bool valid = res.valid != 0;
    const int M = valid ? min(max(res.n_matches, 0), N) : 0, npts = valid ? min(max(res.n_points, 0), N) : 0;
    int32_t *pred = d.pred + o + N;   // of frame k + 1
    for (int i = tid; i < N; i += 256) {
        s_row[i] = INT_MAX;
        pred[i] = -1;
        d.row_to_point[o + i] = -1;
        if (k == 0)
            d.pred[i] = -1;           // frame 0 has no predecessors
    }
    __syncthreads();
    auto link = [&](int r, mvs_match &mt) {
        mt = d.matches[o + r];
        return d.mask[o + r] == 1 && (unsigned)mt.trainIdx < (unsigned)N && (unsigned)mt.queryIdx < (unsigned)N;
    };
    for (int r = tid; r < M; r += 256) {
        mvs_match mt;
        if (link(r, mt))
            atomicMin(&s_row[mt.trainIdx], r);
    }
    for (int j = tid; j < npts; j += 256) {
        const int r = d.point_idx[o + j];
        if ((unsigned)r < (unsigned)M)
            d.row_to_point[o + r] = j;   // point_idx holds every row once
    }
    __syncthreads();
    for (int r = tid; r < M; r += 256) {
        mvs_match mt;
        if (link(r, mt) && s_row[mt.trainIdx] == r)
            pred[mt.queryIdx] = mt.trainIdx;
    }
    for (int i = tid; i < N; i += 256)
        d.succ[o + i] = s_row[i] == INT_MAX ? -1 : s_row[i];
}

// grid n_windows, block 256.  Window w = frames a .. a + F - 1, a = w * stride.  Pass 1 flags the heads -- (frame j <= a + F - 2,
// keypoint i) with a link out of pair j and, for j > a, none into it -- whose chain, cut at frame a + F - 1, holds a
// triangulated link, and numbers them by a workgroup prefix sum in the order (j, i): no atomic decides an index, two runs give
// the same bytes.  Pass 2: every kept head walks its chain (at most F - 1 steps) and writes its rows straight into the layout
// refine_window_kernel reads, for m = min(heads, max_points) points.
__global__ __launch_bounds__(256) void seq_window_assemble_kernel(SeqWinDev d)
{
    __shared__ uint16_t s_head[kMaxKp];   // kept heads: (j - a) << 12 | i
    __shared__ int s_tot[4];
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = d.max_kp, F = d.F, a = w * d.stride, cap = d.max_points;
    int basepos = 0;
    for (int g = 0; g < F - 1; ++g) {
        const size_t o = (size_t)(a + g) * N;
        for (int start = 0; start < N; start += 256) {
            const int i = start + tid;
            bool flag = false;
            if (i < N) {
                int r = d.succ[o + i];
                if (r >= 0 && (g == 0 || d.pred[o + i] < 0)) {
                    size_t of = o;
                    for (int f = g;;) {
                        if (d.row_to_point[of + r] >= 0) {
                            flag = true;
                            break;
                        }
                        if (++f > F - 2)
                            break;
                        const int cur = d.matches[of + r].queryIdx;
                        of += N;
                        r = d.succ[of + cur];
                        if (r < 0)
                            break;
                    }
                }
            }
            const unsigned long long bal = __ballot(flag);
            const int pre = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0)
                s_tot[wave] = __popcll(bal);
            __syncthreads();
            int off = basepos, tot = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int v = s_tot[k];
                off += (k < wave) ? v : 0;
                tot += v;
            }
            const int pos = off + pre;
            if (flag && pos < cap)
                s_head[pos] = (uint16_t)((g << 12) | i);
            basepos += tot;
            __syncthreads();
        }
    }
    const int m = min(basepos, cap);
    // the window's inputs: camera (5, padded to 8), poses F x 12, prior weights F x 6, guesses m x 3, point information m x 6,
    // observations F x m x 2, their information F x m x 3
    double *in = d.in + (size_t)w * d.in_stride;
    double *pose = in + 8, *wt = pose + 12 * (size_t)F, *p0 = wt + 6 * (size_t)F, *pinfo = p0 + 3 * (size_t)m;
    double *obs = pinfo + 6 * (size_t)m, *oinfo = obs + 2 * (size_t)F * m;
    if (tid < 8)
        in[tid] = tid < 5 ? d.K[tid < 3 ? tid : tid + 1] : 0.0;   // fx sk cx fy cy = K[0 1 2 4 5]
    for (int k = tid; k < 12 * F; k += 256) {
        const int f = k / 12, e = k - 12 * f;
        pose[k] = e < 9 ? d.traj_R[9 * (size_t)(a + f) + e] : d.traj_t[3 * (size_t)(a + f) + (e - 9)];
    }
    if (tid < 6 * F)
        wt[tid] = tid < 6 ? d.w_anchor[tid] : d.w_pose[tid % 6];
    if (tid == 0) {
        WinProblem pb;
        pb.n_frames = F;
        pb.n_points = m;
        pb.in_off = (int64_t)w * d.in_stride;
        pb.pt_off = (int64_t)w * cap;
        pb.fr_off = (int64_t)w * F;
        d.prob[w] = pb;
        mvs_seq_window_info wi;
        wi.first_frame = a;
        wi.n_frames = F;
        wi.n_points = m;
        wi.n_tracks_found = basepos;
        d.info[w] = wi;
    }
    int32_t *tkp = d.track_kp + (size_t)w * cap * F;
    double *guess = d.point_guess + (size_t)w * cap * 3;
    for (int p = tid; p < cap; p += 256) {
        if (p >= m) {   // rows past the window's points: the download is the whole capacity
            for (int f = 0; f < F; ++f)
                tkp[(size_t)p * F + f] = -1;
            guess[3 * p] = guess[3 * p + 1] = guess[3 * p + 2] = 0.0;
            continue;
        }
        const int g0 = s_head[p] >> 12, i0 = s_head[p] & 4095;
        int cur = -1, tri_k = -1, tri_j = 0;
        int kpi[kWinMaxFrames];
#pragma unroll
        for (int g = 0; g < kWinMaxFrames; ++g) {
            if (g == g0)
                cur = i0;
            kpi[g] = g < F ? cur : -1;
            if (cur >= 0 && g < F - 1) {
                const size_t of = (size_t)(a + g) * N;
                const int r = d.succ[of + cur];
                if (r >= 0) {
                    const int j = d.row_to_point[of + r];
                    if (tri_k < 0 && j >= 0) {
                        tri_k = a + g;
                        tri_j = j;
                    }
                    cur = d.matches[of + r].queryIdx;
                } else {
                    cur = -1;
                }
            }
        }
        // the first triangulated link gives the guess: pair tri_k's point, scaled and moved into the trajectory's frame
        tri_k = max(tri_k, a);   // pass 1 kept the head for its triangulated link: tri_k is one of the window's pairs
        const double *x = d.points + 3 * ((size_t)tri_k * N + tri_j), *R = d.traj_R + 9 * (size_t)tri_k;
        const double *t = d.traj_t + 3 * (size_t)tri_k, sg = d.traj_sigma[tri_k];
        const double s0 = sg * x[0], s1 = sg * x[1], s2 = sg * x[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double X = ((R[3 * i] * s0 + R[3 * i + 1] * s1) + R[3 * i + 2] * s2) + t[i];
            p0[3 * (size_t)p + i] = X;
            guess[3 * p + i] = X;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
            pinfo[6 * (size_t)p + k] = d.pinfo[k];
#pragma unroll
        for (int g = 0; g < kWinMaxFrames; ++g) {
            if (g >= F)
                continue;
            const int i = kpi[g];
            tkp[(size_t)p * F + g] = i;
            double u = 0.0, v = 0.0, W0 = 0.0, W1 = 0.0, W2 = 0.0;   // not seen: zero information
            if (i >= 0) {
                const size_t s = (size_t)(a + g) * N + i;
                u = (double)d.kp[2 * s];
                v = (double)d.kp[2 * s + 1];
                const int oc = min((int)d.oct[s], kSeqWinMaxOctave);
                W0 = d.oinfo[oc][0], W1 = d.oinfo[oc][1], W2 = d.oinfo[oc][2];
            }
            double *ob = obs + 2 * ((size_t)m * g + p), *oi = oinfo + 3 * ((size_t)m * g + p);
            ob[0] = u, ob[1] = v;
            oi[0] = W0, oi[1] = W1, oi[2] = W2;
        }
    }
}

void launch_seq_windows(const SeqWinDev &d, hipStream_t stream)
{
    if (d.n_windows <= 0)
        return;
    hipLaunchKernelGGL(seq_link_kernel, dim3(d.n_frames - 1), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_window_assemble_kernel, dim3(d.n_windows), dim3(256), 0, stream, d);
}

void launch_seq_link(const SeqWinDev &d, hipStream_t stream)
{
    if (d.n_frames < 2)
        return;
    hipLaunchKernelGGL(seq_link_kernel, dim3(d.n_frames - 1), dim3(256), 0, stream, d);
}

void launch_pnp(const PnpDev &p, hipStream_t stream)
{
    const int Q = p.n_problems;
    hipLaunchKernelGGL(pnp_prep_kernel, dim3((p.stride + 255) / 256, Q), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(pnp_ransac_kernel, dim3((p.num_hypotheses + 255) / 256, Q), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(pnp_finalize_kernel, dim3(Q), dim3(256), 0, stream, p);
}

// ---- scale propagation and trajectory of a sequence (row f2; front-end/visual-odometer.cpp:422-445,577-588) ------------
// Pair k gives the pose of frame k+1 in frame k with a UNIT baseline; track q gives the pose of frame q+2 in frame q in pair
// q's scale.  rel_q = pair_q^-1 o track_q is the pose of frame q+2 in frame q+1 in pair q's scale, so
//   scale_q = |rel_q.t| = baseline(pair q+1) / baseline(pair q)      (visual-odometer.cpp:583-587)
//   sigma_0 = 1, sigma_{q+1} = sigma_q * scale_q                    (everything in pair 0's baseline)
//   G_0 = I, G_1 = pair_0, G_{q+2} = G_q o (R_track_q, sigma_q t_track_q)           (the PnP pose is the frame pose)
// A failed track keeps the scale (scale_q = 1) and falls back to the two-view pose: G_{q+2} = G_{q+1} o (R, sigma t) of
// pair q+1; an invalid pair contributes the identity.  A sequential fold: the order of operations WITHIN an output element is
// part of the specification (the CPU oracle repeats it) -- but the twelve elements of one composition are independent of each
// other, so (round 5) the fold runs on sixteen lanes of one wavefront instead of one: quad i holds row i of the running
// rotation in its lanes 0..2 and t_i in lane 3, the three factors A_i0, A_i1, A_i2 every element of row i needs are quad
// broadcasts (DPP quad_perm, a register move: no LDS, no scalar round trip), and each lane evaluates its own element with
// exactly the operations of the one-lane loop: (a0 c0 + a1 c1) + a2 c2 (+ a3 for the translation lanes).  The dependent
// chain per frame is ~9 instructions instead of ~100: 0.46 -> 0.05 ms per 1000 frames, every trajectory byte unchanged.
template <int M>
__device__ __forceinline__ double quad_bcast(double v)
{
    constexpr int ctrl = M | (M << 2) | (M << 4) | (M << 6);   // quad_perm:[M,M,M,M]
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), ctrl, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), ctrl, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(256) void seq_chain_kernel(SeqChainDev c)
{
    // Only the fold itself is sequential.  Per chunk of kChunk steps the workgroup first prepares, in parallel, everything
    // that does not depend on the running state -- which operand a step composes with (track pose on G_q, or the next
    // pair's pose on G_{q+1}) and its scale ratio (the sqrt) -- into LDS; sixteen lanes then fold the chunk out of LDS with
    // the next step's operands prefetched, and the workgroup writes the chunk's results back.  (Reading HBM inside the
    // dependent loop cost 2 us per frame.)
    constexpr int kChunk = 128;
    __shared__ double s_op[kChunk * 12];    // R (9), t (3) of the step's operand, unscaled
    __shared__ double s_scale[kChunk];
    __shared__ int s_sel[kChunk];           // 0: compose on G_q, 1: on G_{q+1}
    __shared__ double s_out[kChunk * 14];   // G_{q+2} (12), track_scale, sigma_{q+1}
    __shared__ double s_g[24];              // G_0, G_1 (R 9, t 3 each)
    const int F = c.n_frames, tid = threadIdx.x;
    auto compose = [](const double *A, const double *R, const double *t, double sig, double *out) {
        // out = A o (R, sig * t):  R_out = A.R R,  t_out = A.R (sig t) + A.t
        const double s0 = sig * t[0], s1 = sig * t[1], s2 = sig * t[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                out[3 * i + j] = (A[3 * i] * R[j] + A[3 * i + 1] * R[3 + j]) + A[3 * i + 2] * R[6 + j];
            out[9 + i] = ((A[3 * i] * s0 + A[3 * i + 1] * s1) + A[3 * i + 2] * s2) + A[9 + i];
        }
    };
    if (tid == 0) {
        const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z3[3] = {0, 0, 0};
        double Ga[12], Gb[12];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            Ga[k] = (k < 9 && k % 4 == 0) ? 1.0 : 0.0;
        const mvs_pair_result &p0 = c.results[0];
        compose(Ga, p0.valid ? p0.R : I3, p0.valid ? p0.t : Z3, 1.0, Gb);
        for (int k = 0; k < 9; ++k) {
            c.traj_R[k] = Ga[k];
            c.traj_R[9 + k] = Gb[k];
        }
        for (int k = 0; k < 3; ++k) {
            c.traj_t[k] = Ga[9 + k];
            c.traj_t[3 + k] = Gb[9 + k];
        }
        c.traj_sigma[0] = 1.0;
        for (int k = 0; k < 12; ++k) {
            s_g[k] = Ga[k];
            s_g[12 + k] = Gb[k];
        }
    }
    __syncthreads();
    // fold lanes: tid = 4 i + j; j < 3: element (i, j) of the rotation, j = 3: t_i; quad 3 idles (its results are not stored)
    const int fi = min(tid >> 2, 2), fj = tid & 3;
    const bool fold_lane = tid < 12, is_t = fj == 3;
    const int elem = is_t ? 9 + fi : 3 * fi + fj;                     // this lane's element of a pose (R 9, t 3)
    const int o0 = is_t ? 9 : fj, o1 = is_t ? 10 : 3 + fj, o2 = is_t ? 11 : 6 + fj;   // its operand column
    double ga = s_g[elem], gb = s_g[12 + elem];   // this lane's element of G_q and G_{q+1}
    double sigma = 1.0;
    const int T = F - 2;
    for (int q0 = 0; q0 < T; q0 += kChunk) {
        const int n = min(kChunk, T - q0);
        __syncthreads();
        for (int j = tid; j < n; j += 256) {   // state-independent part of step q = q0 + j
            const int q = q0 + j;
            const mvs_pair_result &pq = c.results[q], &pn = c.results[q + 1];
            const PnpOut &tr = c.tracks[q];
            const bool ok = c.n_corr[q] >= 7 && tr.ok && pq.valid;
            double scale = 1.0;
            double *op = s_op + 12 * j;
            if (ok) {
                // rel.t = R_pair^T (t_track - t_pair)
                const double d0 = tr.t[0] - pq.t[0], d1 = tr.t[1] - pq.t[1], d2 = tr.t[2] - pq.t[2];
                const double r0 = (pq.R[0] * d0 + pq.R[3] * d1) + pq.R[6] * d2;
                const double r1 = (pq.R[1] * d0 + pq.R[4] * d1) + pq.R[7] * d2;
                const double r2 = (pq.R[2] * d0 + pq.R[5] * d1) + pq.R[8] * d2;
                scale = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
                for (int k = 0; k < 9; ++k) op[k] = tr.R[k];
                for (int k = 0; k < 3; ++k) op[9 + k] = tr.t[k];
            } else if (pn.valid) {
                for (int k = 0; k < 9; ++k) op[k] = pn.R[k];
                for (int k = 0; k < 3; ++k) op[9 + k] = pn.t[k];
            } else {
                for (int k = 0; k < 12; ++k) op[k] = (k < 9 && k % 4 == 0) ? 1.0 : 0.0;
            }
            s_scale[j] = scale;
            s_sel[j] = ok ? 0 : 1;
        }
        __syncthreads();
        if (tid < 64) {   // the whole first wavefront walks the loop (the DPP moves need their source lanes active)
            double c0 = s_op[o0], c1 = s_op[o1], c2 = s_op[o2], scale = s_scale[0];
            int sel = s_sel[0];
            for (int j = 0; j < n; ++j) {
                const int jn = min(j + 1, n - 1);
                // prefetch the next step's operands while this step's products are in flight
                const double n0 = s_op[12 * jn + o0], n1 = s_op[12 * jn + o1], n2 = s_op[12 * jn + o2], nscale = s_scale[jn];
                const int nsel = s_sel[jn];
                const double a = sel == 0 ? ga : gb;                   // this lane's element of the left factor
                const double a0 = quad_bcast<0>(a), a1 = quad_bcast<1>(a), a2 = quad_bcast<2>(a);
                const double f = is_t ? sigma : 1.0;                    // translation lanes: the operand is sigma * t (x * 1.0 == x)
                const double r = (a0 * (f * c0) + a1 * (f * c1)) + a2 * (f * c2);
                const double gn = is_t ? r + a : r;                     // ... + A.t_i on the translation lanes
                sigma = sigma * scale;
                if (fold_lane)
                    s_out[14 * j + elem] = gn;
                if (tid == 0) {
                    s_out[14 * j + 12] = scale;
                    s_out[14 * j + 13] = sigma;
                }
                ga = gb;
                gb = gn;
                c0 = n0; c1 = n1; c2 = n2; scale = nscale; sel = nsel;
            }
        }
        __syncthreads();
        for (int i = tid; i < n * 14; i += 256) {
            const int j = i / 14, k = i - j * 14, q = q0 + j;
            const double v = s_out[i];
            if (k < 9) c.traj_R[9 * (size_t)(q + 2) + k] = v;
            else if (k < 12) c.traj_t[3 * (size_t)(q + 2) + (k - 9)] = v;
            else if (k == 12) c.track_scale[q] = v;
            else c.traj_sigma[q + 1] = v;
        }
    }
}

void launch_seq_chain(const SeqChainDev &c, hipStream_t stream)
{
    hipLaunchKernelGGL(seq_chain_kernel, dim3(1), dim3(256), 0, stream, c);
}

// ---- the scale of a sequence from depth ratios of shared points (mvs_seq_rescale) ---------------
// Step q, pairs q and q + 1.  Keypoint c of frame q + 1 is shared when it is the new keypoint of a point j of pair q and the
// base keypoint of a point j' of pair q + 1 (the smallest j' per keypoint: seq_link_kernel's rule).  Both pairs know the depth
// of that point in frame q + 1, each in its own unit baseline, so
//   rho = z_a / z_b = baseline(pair q+1) / baseline(pair q),   z_a = (R_q^T (x_j - t_q))[2],   z_b = x_j'[2]
// and scale_q = the lower median of rho over the shared points with two finite positive depths.  The operations and their
// order are the header's (tests/seq_rescale_model.py restates them): + - * /, one rounding each.
//
// grid n_frames - 2, block 256.  Pass 1: s_at[c] = point of pair q at keypoint c (b is unique per match row: plain stores of
// distinct addresses).  Pass 2: s_first[c] = smallest point of pair q + 1 with base keypoint c (an integer minimum does not
// depend on the order of arrival).  Pass 3 walks pair q + 1's points in ascending order in chunks of 256 and compacts the
// ratios of the used points into LDS by ballot (seq_join_kernel's scan); a bitonic sort of the list padded with +inf to a
// power of two (seq_glob_sort_kernel's network) puts the lower median at (n_used - 1) / 2.  Equal ratios are equal bit
// patterns, so the result does not depend on how the network orders them.  Every index read from a table is range-checked.
__global__ __launch_bounds__(256) void seq_ratio_kernel(SeqScaleDev d)
{
    __shared__ double s_rho[kMaxKp];
    __shared__ int s_first[kMaxKp];
    __shared__ int16_t s_at[kMaxKp];
    __shared__ int s_tot[4], s_tot2[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, N = d.max_kp;
    const mvs_pair_result &pq = d.results[q], &pn = d.results[q + 1];
    const bool valid = pq.valid != 0 && pn.valid != 0;
    const int nq = valid ? min(max(pq.n_points, 0), N) : 0, nn = valid ? min(max(pn.n_points, 0), N) : 0;
    const size_t oq = (size_t)q * N, on = oq + N;
    // point j of the pair at offset o: base keypoint a, new keypoint b
    auto point = [&](size_t o, int j, int &a, int &b) {
        const int r = d.point_idx[o + j];
        if ((unsigned)r >= (unsigned)N)
            return false;
        const mvs_match mt = d.matches[o + r];
        a = mt.trainIdx;
        b = mt.queryIdx;
        return (unsigned)a < (unsigned)N && (unsigned)b < (unsigned)N;
    };
    for (int i = tid; i < N; i += 256) {
        s_at[i] = -1;
        s_first[i] = INT_MAX;
    }
    __syncthreads();
    for (int j = tid; j < nq; j += 256) {
        int a, b;
        if (point(oq, j, a, b))
            s_at[b] = (int16_t)j;
    }
    for (int j = tid; j < nn; j += 256) {
        int a, b;
        if (point(on, j, a, b))
            atomicMin(&s_first[a], j);
    }
    __syncthreads();
    const double R02 = pq.R[2], R12 = pq.R[5], R22 = pq.R[8], t0 = pq.t[0], t1 = pq.t[1], t2 = pq.t[2];
    int n_common = 0, n_used = 0;
    for (int start = 0; start < nn; start += 256) {
        const int jn = start + tid;
        bool shared = false, used = false;
        double rho = 0.0;
        if (jn < nn) {
            int a, b;
            if (point(on, jn, a, b) && s_first[a] == jn && s_at[a] >= 0) {
                shared = true;
                const double *x = d.points + 3 * (oq + (size_t)s_at[a]);
                const double d0 = x[0] - t0, d1 = x[1] - t1, d2 = x[2] - t2;
                const double za = (R02 * d0 + R12 * d1) + R22 * d2;
                const double zb = d.points[3 * (on + (size_t)jn) + 2];
                used = za > 0.0 && za < HUGE_VAL && zb > 0.0 && zb < HUGE_VAL;   // finite and positive (a NaN fails both)
                if (used)
                    rho = za / zb;
            }
        }
        const unsigned long long bs = __ballot(shared), bu = __ballot(used);
        const int pre = __popcll(bu & ((1ull << lane) - 1ull));
        if (lane == 0) {
            s_tot[w] = __popcll(bu);
            s_tot2[w] = __popcll(bs);
        }
        __syncthreads();
        int off = n_used;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = s_tot[k];
            off += (k < w) ? v : 0;
            n_used += v;
            n_common += s_tot2[k];
        }
        if (used)
            s_rho[off + pre] = rho;   // off + pre < nn <= N: one slot per point of pair q + 1 at the most
        __syncthreads();
    }
    int n2 = 2;
    while (n2 < n_used)
        n2 <<= 1;
    for (int k = n_used + tid; k < n2; k += 256)
        s_rho[k] = HUGE_VAL;
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int k = tid; k < (n2 >> 1); k += 256) {
                const int lo = 2 * k - (k & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const double a = s_rho[lo], b = s_rho[hi];
                if ((a > b) == up) {
                    s_rho[lo] = b;
                    s_rho[hi] = a;
                }
            }
        }
    __syncthreads();
    if (tid == 0) {
        const int flag = !valid ? 1 : (n_used < d.min_common ? 2 : 0);
        const double scale = flag == 0 ? s_rho[(n_used - 1) >> 1] : 1.0;
        mvs_seq_scale_step st;
        st.n_common = n_common;
        st.n_used = n_used;
        st.flag = flag;
        st.reserved = 0;
        st.scale = scale;
        d.steps[q] = st;
        d.track_scale[q] = scale;
    }
}

// grid 1, block 256.  sigma_0 = 1, sigma_{q+1} = sigma_q * scale_q: a sequential product (its order is the contract), by one
// thread per chunk.  G_0 = I, G_{k+1} = G_k o (R_k, sigma_k t_k) from the pairs alone (an invalid pair is the identity), in
// seq_chain_kernel's compose order.  Per chunk of kChunk steps the workgroup loads the operands into LDS, thread 0 extends the
// product, the workgroup scales the translations, and the sixteen fold lanes of seq_chain_kernel (quad i = row i of the running
// rotation and t_i; the factors are quad broadcasts) walk the chunk; the running pose stays in their registers across chunks.
__global__ __launch_bounds__(256) void seq_sigma_fold_kernel(SeqScaleDev d)
{
    constexpr int kChunk = 128;
    __shared__ double s_op[kChunk * 12];    // R_k (9), sigma_k t_k (3)
    __shared__ double s_sig[kChunk];        // in: scale_{k-1}; out: sigma_k
    __shared__ double s_out[kChunk * 12];   // G_{k+1}
    const int F = d.n_frames, tid = threadIdx.x, P = F - 1;
    if (tid < 12) {
        const double v = (tid < 9 && tid % 4 == 0) ? 1.0 : 0.0;   // G_0 = I
        if (tid < 9)
            d.traj_R[tid] = v;
        else
            d.traj_t[tid - 9] = v;
    }
    // fold lanes: tid = 4 i + j; j < 3: element (i, j) of the rotation, j = 3: t_i; quad 3 idles (its results are not stored)
    const int fi = min(tid >> 2, 2), fj = tid & 3;
    const bool fold_lane = tid < 12, is_t = fj == 3;
    const int elem = is_t ? 9 + fi : 3 * fi + fj;
    const int o0 = is_t ? 9 : fj, o1 = is_t ? 10 : 3 + fj, o2 = is_t ? 11 : 6 + fj;
    double g = (!is_t && fi == fj) ? 1.0 : 0.0;   // this lane's element of G_k
    double sigma = 1.0;                           // thread 0: sigma_k
    for (int k0 = 0; k0 < P; k0 += kChunk) {
        const int n = min(kChunk, P - k0);
        __syncthreads();
        for (int i = tid; i < n * 12; i += 256) {
            const int j = i / 12, e = i - 12 * j;
            const mvs_pair_result &p = d.results[k0 + j];
            s_op[i] = p.valid ? (e < 9 ? p.R[e] : p.t[e - 9]) : ((e < 9 && e % 4 == 0) ? 1.0 : 0.0);
        }
        for (int j = tid; j < n; j += 256)
            s_sig[j] = k0 + j > 0 ? d.track_scale[k0 + j - 1] : 1.0;
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < n; ++j) {
                if (k0 + j > 0)
                    sigma = sigma * s_sig[j];
                s_sig[j] = sigma;
            }
        __syncthreads();
        for (int i = tid; i < n * 3; i += 256) {
            const int j = i / 3, e = i - 3 * j;
            s_op[12 * j + 9 + e] = s_sig[j] * s_op[12 * j + 9 + e];
        }
        __syncthreads();
        if (tid < 64) {   // the whole first wavefront walks the loop (the DPP moves need their source lanes active)
            double c0 = s_op[o0], c1 = s_op[o1], c2 = s_op[o2];
            for (int j = 0; j < n; ++j) {
                const int jn = min(j + 1, n - 1);
                const double n0 = s_op[12 * jn + o0], n1 = s_op[12 * jn + o1], n2 = s_op[12 * jn + o2];
                const double a0 = quad_bcast<0>(g), a1 = quad_bcast<1>(g), a2 = quad_bcast<2>(g);
                const double r = (a0 * c0 + a1 * c1) + a2 * c2;
                g = is_t ? r + g : r;   // ... + A.t_i on the translation lanes
                if (fold_lane)
                    s_out[12 * j + elem] = g;
                c0 = n0; c1 = n1; c2 = n2;
            }
        }
        __syncthreads();
        for (int i = tid; i < n * 12; i += 256) {
            const int j = i / 12, e = i - 12 * j, k = k0 + j;
            if (e < 9)
                d.traj_R[9 * (size_t)(k + 1) + e] = s_out[i];
            else
                d.traj_t[3 * (size_t)(k + 1) + (e - 9)] = s_out[i];
        }
        for (int j = tid; j < n; j += 256)
            d.traj_sigma[k0 + j] = s_sig[j];
    }
}

void launch_seq_rescale(const SeqScaleDev &d, hipStream_t stream)
{
    if (d.n_frames > 2)
        hipLaunchKernelGGL(seq_ratio_kernel, dim3(d.n_frames - 2), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_sigma_fold_kernel, dim3(1), dim3(256), 0, stream, d);
}

}  // namespace mvs
