// essential5.hip -- the five-point essential-matrix RANSAC: find_essential_matrix under USE_OPENCV_ESSENTIAL_MATRIX
// (vision/sfm-solve.cpp:42-63; the reference's default build, SConstruct:81-82), beside the 8-point stage of kernels.hip.
//
//   sample   the first five indices of sample8(seed + global index, hypothesis, M, sampler) -- the sample stream is untouched;
//   solve    five_point() (five_point.hpp): up to ten models per hypothesis;
//   score    match i is an inlier of model E iff e5_inlier(e5_sampson(E, match i), max_error_sq) (five_point.hpp);
//   select   the larger count; among equal counts the smaller residual = ONE sequential binary64 sum of num / den over the
//            inliers, i ascending (a sum that is not finite counts as +infinity), worked out only for the models tied at the
//            largest count (estimator-RANSAC.cpp:76-84); then
//            the smaller hypothesis id; then the smaller root index;
//   no early exit (every hypothesis runs; VF_MATCH_CONFIDENCE_LEVEL is unused), no refit, no projection (sfm-solve.cpp:62-63).
//
// Layout.  essential5_solve_count_kernel: grid (hypothesis blocks, pairs), one wavefront per workgroup,
// one hypothesis per lane.  The solver's arrays (10 x 20 elimination matrix, basis, polynomials: kE5Ws = 276 doubles) are the
// lane's column of a 138 KB LDS block -- run-time indices (pivot rows, root slots) stay out of scratch memory -- and the
// hypothesis' models stay in that block: the points of the pair are read once per model at a wavefront-uniform address and only
// n_roots and ten int32 counts per hypothesis go to device memory.  essential5_select_kernel: one wavefront per pair reduces the
// count table, RE-SOLVES the hypotheses tied at the largest count with the same device function (the same bits) for their
// residuals, re-solves the winner once more for E and writes the mask.
#include "kernels.hpp"
#include "sampler.hpp"
#include "five_point.hpp"

namespace mvs {

constexpr int kE5Lanes = kE5HypPerBlock;
constexpr size_t kE5LdsBytes = (size_t)kE5Ws * kE5Lanes * sizeof(double);   // 141 312

__device__ __forceinline__ double e5_max_error_sq(const BatchDev &b, const RunParams &rp, int pair)
{
    if (rp.max_error_sq > 0.0)
        return rp.max_error_sq;
    const double *K = b.K + (size_t)pair * 9;
    return 5e-2 / K[0] / K[4];  // sfm-solve.cpp:311
}

// hypothesis h of the pair whose normalised points are P (x1, y1, x2, y2 per match): models into w, returns their number
__device__ __forceinline__ int e5_solve_hyp(const double *P, int M, uint64_t seed, uint32_t h, int sampler, const E5Ws &w)
{
    int idx[8];
    sample8(seed, h, M, sampler, idx);
    double p1[10], p2[10];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double4 q = *reinterpret_cast<const double4 *>(P + (size_t)idx[k] * 4);
        p1[2 * k] = q.x; p1[2 * k + 1] = q.y;
        p2[2 * k] = q.z; p2[2 * k + 1] = q.w;
    }
    return five_point(p1, p2, w);
}

__global__ __launch_bounds__(kE5Lanes) void essential5_solve_count_kernel(BatchDev b, RunParams rp, int32_t *n_roots, int32_t *count,
                                                                          int h_stride)
{
    extern __shared__ double s_w[];
    const int pair = blockIdx.y, lane = threadIdx.x;
    const int M = min(b.M[pair], b.max_kp);
    if (M < 8)   // sfm-solve.cpp:37; the selection reports "no model" without reading the tables
        return;
    const int H = rp.num_hypotheses;
    const int h = blockIdx.x * kE5Lanes + lane;
    const bool live = h < H;
    const double *P = b.pts + (size_t)pair * b.max_kp * 4;
    const E5Ws w{s_w + lane, kE5Lanes};
    const double thr = e5_max_error_sq(b, rp, pair);
    int n = 0;
    if (live)
        n = e5_solve_hyp(P, M, rp.seed + (uint64_t)b.gidx[pair], (uint32_t)h, rp.sampler, w);
    int32_t *cout = count + ((size_t)pair * h_stride + (live ? h : 0)) * kE5MaxRoots;
    for (int r = 0; r < kE5MaxRoots; ++r) {
        int cnt = -1;
        if (r < n) {
            double E[9];
#pragma unroll
            for (int e = 0; e < 9; ++e)
                E[e] = w(9 * r + e);
            cnt = 0;
            for (int i = 0; i < M; ++i) {
                const double4 q = *reinterpret_cast<const double4 *>(P + (size_t)i * 4);
                double num, den;
                e5_sampson(E, q.x, q.y, q.z, q.w, num, den);
                cnt += e5_inlier(num, den, thr) ? 1 : 0;
            }
        }
        if (live)
            cout[r] = cnt;
    }
    if (live)
        n_roots[(size_t)pair * h_stride + h] = n;
}

struct E5Best {
    double res;
    int hyp, root;   // hyp < 0: none
};
__device__ __forceinline__ bool e5_better(const E5Best &a, const E5Best &b)   // a before b in the selection order
{
    if (a.hyp < 0) return false;
    if (b.hyp < 0) return true;
    if (a.res != b.res) return a.res < b.res;
    if (a.hyp != b.hyp) return a.hyp < b.hyp;
    return a.root < b.root;
}

__global__ __launch_bounds__(kE5Lanes) void essential5_select_kernel(BatchDev b, RunParams rp, const int32_t *n_roots,
                                                                     const int32_t *count, int h_stride, int32_t *best_root)
{
    extern __shared__ double s_w[];
    __shared__ double s_E[9];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int M = min(b.M[pair], b.max_kp);
    const int H = rp.num_hypotheses;
    mvs_pair_result *res = b.results + pair;
    uint8_t *mask = b.mask + (size_t)pair * b.max_kp;
    const double *P = b.pts + (size_t)pair * b.max_kp * 4;
    const int32_t *C = count + (size_t)pair * h_stride * kE5MaxRoots;
    const E5Ws w{s_w + lane, kE5Lanes};

    for (int i = M + lane; i < b.max_kp; i += kE5Lanes)   // rows past the match list: cleared (deterministic downloads)
        mask[i] = 0;
    if (lane < 9) {   // the pose of a pair that ends without one is zero, whatever ran on the batch before
        res->R1to2[lane] = 0.0;
        res->R[lane] = 0.0;
        if (lane < 3) {
            res->t1to2[lane] = 0.0;
            res->t[lane] = 0.0;
        }
    }
    int best = -1;
    if (M >= 8)
        for (int k = lane; k < H * kE5MaxRoots; k += kE5Lanes)
            best = max(best, C[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        best = max(best, __shfl_xor(best, o));
    if (best < 0) {
        for (int i = lane; i < M; i += kE5Lanes)
            mask[i] = 0;
        if (lane < 9) {
            res->F[lane] = 0.0;
            res->E[lane] = 0.0;
        }
        if (lane == 0) {
            res->best_hyp = -1;
            res->best_count = 0;
            res->best_residual = 0.0;
            best_root[pair] = -1;
        }
        return;
    }
    const double thr = e5_max_error_sq(b, rp, pair);
    const uint64_t seed = rp.seed + (uint64_t)b.gidx[pair];
    // ---- residuals of the models tied at the largest count (lane l visits hypotheses l, l + 64, ... ascending) ----
    E5Best me{0.0, -1, 0};
    for (int h = lane; h < H; h += kE5Lanes) {
        unsigned tied = 0;
        for (int r = 0; r < kE5MaxRoots; ++r)
            tied |= C[(size_t)h * kE5MaxRoots + r] == best ? 1u << r : 0u;
        if (!tied)
            continue;
        const int n = e5_solve_hyp(P, M, seed, (uint32_t)h, rp.sampler, w);
        for (int r = 0; r < n; ++r) {
            if (!((tied >> r) & 1u))
                continue;
            double E[9];
#pragma unroll
            for (int e = 0; e < 9; ++e)
                E[e] = w(9 * r + e);
            double sum = 0.0;
            for (int i = 0; i < M; ++i) {
                const double4 q = *reinterpret_cast<const double4 *>(P + (size_t)i * 4);
                double num, den;
                e5_sampson(E, q.x, q.y, q.z, q.w, num, den);
                if (e5_inlier(num, den, thr))
                    sum += num / den;
            }
            const E5Best c{e5_residual_key(sum), h, r};
            if (e5_better(c, me))
                me = c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        E5Best other;
        other.res = __shfl_xor(me.res, o);
        other.hyp = __shfl_xor(me.hyp, o);
        other.root = __shfl_xor(me.root, o);
        if (e5_better(other, me))
            me = other;
    }
    // ---- the winner's E (solved once more: the same function, the same bits) and its mask ----
    if (lane == 0) {
        int n = 0;
        if (me.hyp >= 0)
            n = e5_solve_hyp(P, M, seed, (uint32_t)me.hyp, rp.sampler, w);
        const bool ok = me.hyp >= 0 && me.root < n;
        for (int e = 0; e < 9; ++e) {
            const double v = ok ? w(9 * me.root + e) : 0.0;
            s_E[e] = v;
            res->F[e] = v;
            res->E[e] = v;
        }
        res->best_hyp = ok ? me.hyp : -1;
        res->best_count = ok ? best : 0;
        res->best_residual = ok ? me.res : 0.0;
        best_root[pair] = ok ? me.root : -1;
    }
    __syncthreads();
    double E[9];
#pragma unroll
    for (int e = 0; e < 9; ++e)
        E[e] = s_E[e];
    for (int i = lane; i < M; i += kE5Lanes) {
        const double4 q = *reinterpret_cast<const double4 *>(P + (size_t)i * 4);
        double num, den;
        e5_sampson(E, q.x, q.y, q.z, q.w, num, den);
        mask[i] = e5_inlier(num, den, thr) ? 1 : 0;
    }
}

// mvs_five_point: one solve by lane 0 (workspace stride 1)
__global__ __launch_bounds__(64) void five_point_kernel(const double *p1, const double *p2, double *Eout, int *nout)
{
    __shared__ double s_one[kE5Ws];
    if (threadIdx.x != 0)
        return;
    double a[10], c[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        a[k] = p1[k];
        c[k] = p2[k];
    }
    const E5Ws w{s_one, 1};
    const int n = five_point(a, c, w);
    for (int k = 0; k < 9 * kE5Models; ++k)
        Eout[k] = k < 9 * n ? w(k) : 0.0;
    *nout = n;
}

hipError_t essential5_prepare()
{
    hipError_t e = hipFuncSetAttribute((const void *)essential5_solve_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kE5LdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)essential5_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kE5LdsBytes);
    return e;
}

void launch_essential5(const BatchDev &b, const RunParams &rp, int n_active, int32_t *n_roots, int32_t *count, int h_stride,
                       int32_t *best_root, hipStream_t stream)
{
    const int G = (rp.num_hypotheses + kE5Lanes - 1) / kE5Lanes;
    hipLaunchKernelGGL(essential5_solve_count_kernel, dim3(G, n_active), dim3(kE5Lanes), kE5LdsBytes, stream, b, rp, n_roots, count,
                       h_stride);
    hipLaunchKernelGGL(essential5_select_kernel, dim3(n_active), dim3(kE5Lanes), kE5LdsBytes, stream, b, rp, n_roots, count, h_stride,
                       best_root);
}

void launch_five_point(const double *p1, const double *p2, double *E, int *n, hipStream_t stream)
{
    hipLaunchKernelGGL(five_point_kernel, dim3(1), dim3(64), 0, stream, p1, p2, E, n);
}

}  // namespace mvs
