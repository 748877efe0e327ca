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
//   stop     confidence = 0 (the default): every hypothesis runs.  0 < confidence < 1 (VF_MATCH_CONFIDENCE_LEVEL,
//            sfm-solve.cpp:22-23,58): per pair, at the checkpoints T_0 = min(64, H), T_{j+1} = min(2 T_j, H), the rule
//            e5_confident() of five_point.hpp on the largest count so far; a pair that stops at T (its n_run) gives exactly what
//            the same call gives with num_hypotheses = T -- hypotheses >= T take no part, counted or not;
//   no refit, no projection (sfm-solve.cpp:62-63).
//
// Layout.  essential5_solve_count_kernel: grid (hypothesis blocks, pairs), four wavefronts per
// workgroup, one hypothesis per lane.  Wavefront 0 solves: the solver's arrays (10 x 20 elimination matrix, basis, polynomials:
// kE5Ws = 276 doubles) are the lane's column of a 138 KB LDS block -- run-time indices (pivot rows, root slots) stay out of
// scratch memory -- and the hypothesis' models stay in that block.  All four wavefronts count -- wavefront v takes matches
// v, v + 4, ..., each read once per model at a wavefront-uniform address -- and wavefront 0 adds the four integer partial counts,
// so only n_roots and ten int32 counts per hypothesis go to device memory.  essential5_select_kernel: one wavefront per pair
// reduces the count table, RE-SOLVES the hypotheses tied at the largest count with the same device function (the same bits) for
// their residuals, re-solves the winner once more for E, writes the mask and leaves the pair's n_run on the device.
//
// Without a confidence level these two launches are the stage.  With one the stage is a fixed sequence of rounds, one per
// checkpoint (their number depends on H alone), plain launches on the one stream and no host synchronisation: round j is
// essential5_solve_count_kernel over [T_{j-1}, T_j) (round 0: the first 64 hypotheses, n_run null), in which a workgroup of a
// pair that has stopped returns after reading the pair's n_run word: block-uniform, before any work; each round ends with
// essential5_horizon_kernel, one wavefront per pair, which folds the new counts into the pair's running maximum, applies the
// rule and writes n_run = T_j for a pair that stops (-1: still running).  The selection then takes its hypothesis bound from
// n_run.  No atomics, no flag is waited for: the order of the launches on the stream is the only synchronisation.  Every entry
// point, point-fed or descriptor-fed, runs this one sequence.
#include "kernels.hpp"
#include "sampler.hpp"
#include "five_point.hpp"

namespace mvs {

constexpr int kE5Lanes = kE5HypPerBlock;
constexpr size_t kE5LdsBytes = (size_t)kE5Ws * kE5Lanes * sizeof(double);   // 141 312
constexpr int kE5Waves = 4;   // wavefronts of essential5_solve_count_kernel: one per SIMD of the CU its LDS block fills
constexpr int kE5CountThreads = kE5Lanes * kE5Waves;
// the workspace + [wavefront][root][lane] int32 partial counts: 151 552 of the CU's 163 840 bytes
constexpr size_t kE5CountLdsBytes = kE5LdsBytes + (size_t)kE5Waves * kE5MaxRoots * kE5Lanes * sizeof(int32_t);

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

// Checkpoint j = [h_first, h_last) just counted.  One wavefront per pair: the largest count of the range joins the pair's running
// maximum c_max, and the pair stops here -- n_run = h_last -- if this is the last checkpoint or e5_confident() says so; a pair
// that goes on keeps n_run = -1.  The first checkpoint (h_first = 0) reads neither word: it initialises both, and gives the
// pairs with fewer than eight matches n_run = 0.
__global__ __launch_bounds__(kE5Lanes) void essential5_horizon_kernel(BatchDev b, const int32_t *count, int h_stride,
                                                                      int h_first, int h_last, int is_last, int j,
                                                                      double confidence, int32_t *n_run, int32_t *c_max)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int M = min(b.M[pair], b.max_kp);
    int state = -1, c = -1;
    if (M < 8)
        state = 0;
    else if (h_first > 0) {
        state = n_run[pair];
        c = c_max[pair];
    }
    if (state < 0) {   // (uniform over the wavefront: a running pair)
        const int32_t *C = count + (size_t)pair * h_stride * kE5MaxRoots;
        for (int k = h_first * kE5MaxRoots + lane; k < h_last * kE5MaxRoots; k += kE5Lanes)
            c = max(c, C[k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            c = max(c, __shfl_xor(c, o));
        if (is_last || e5_confident(c, M, j, confidence))
            state = h_last;
    }
    if (lane == 0) {
        n_run[pair] = state;
        c_max[pair] = c;
    }
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

// The solve + count kernel: grid (hypothesis blocks of [h_first, ...), pairs), four wavefronts.  Wavefront 0 solves hypothesis
// h_first + 64 blockIdx.x + lane into the lane's LDS column; then thread (wavefront v, lane l) scores the models of hypothesis
// l against matches v, v + 4, ... (each match read at a wavefront-uniform address; every wavefront reads its own lanes'
// columns, so the stride-64 layout stays free of bank conflicts) and wavefront 0 adds the four integer partial counts per
// (lane, root) and writes the tables: count -1 past the hypothesis' n_roots.  n_run: null (a plain run, or round 0) or the pairs' checkpoints, a pair with n_run >= 0 having stopped.  Both
// early returns are block-uniform and in front of the first barrier.
__global__ __launch_bounds__(kE5CountThreads) void essential5_solve_count_kernel(BatchDev b, RunParams rp, int32_t *n_roots,
                                                                                 int32_t *count, int h_stride, int h_first,
                                                                                 const int32_t *n_run)
{
    extern __shared__ double s_w[];
    __shared__ int s_n[kE5Lanes];
    int32_t *s_part = reinterpret_cast<int32_t *>(s_w + (size_t)kE5Ws * kE5Lanes);
    const int pair = blockIdx.y, lane = threadIdx.x % kE5Lanes;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kE5Lanes);
    const int M = min(b.M[pair], b.max_kp);
    if (M < 8)   // sfm-solve.cpp:37; the selection reports "no model" without reading the tables
        return;
    if (n_run && n_run[pair] >= 0)   // the pair has stopped at an earlier checkpoint
        return;
    const int h = h_first + blockIdx.x * kE5Lanes + lane;
    const bool live = h < rp.num_hypotheses;
    const double *P = b.pts + (size_t)pair * b.max_kp * 4;
    const E5Ws w{s_w + lane, kE5Lanes};
    const double thr = e5_max_error_sq(b, rp, pair);
    if (wave == 0) {
        int n = 0;
        if (live)
            n = e5_solve_hyp(P, M, rp.seed + (uint64_t)b.gidx[pair], (uint32_t)h, rp.sampler, w);
        s_n[lane] = n;
    }
    __syncthreads();
    const int n = s_n[lane];
    for (int r = 0; r < kE5MaxRoots; ++r) {
        int cnt = 0;
        if (r < n) {
            double E[9];
#pragma unroll
            for (int e = 0; e < 9; ++e)
                E[e] = w(9 * r + e);
            for (int i = wave; i < M; i += kE5Waves) {
                const double4 q = *reinterpret_cast<const double4 *>(P + (size_t)i * 4);
                double num, den;
                e5_sampson(E, q.x, q.y, q.z, q.w, num, den);
                cnt += e5_inlier(num, den, thr) ? 1 : 0;
            }
        }
        s_part[(wave * kE5MaxRoots + r) * kE5Lanes + lane] = cnt;
    }
    __syncthreads();
    if (wave != 0 || !live)
        return;
    int32_t *cout = count + ((size_t)pair * h_stride + h) * kE5MaxRoots;
    for (int r = 0; r < kE5MaxRoots; ++r) {
        int cnt = -1;
        if (r < n) {
            cnt = 0;
#pragma unroll
            for (int v = 0; v < kE5Waves; ++v)
                cnt += s_part[(v * kE5MaxRoots + r) * kE5Lanes + lane];
        }
        cout[r] = cnt;
    }
    n_roots[(size_t)pair * h_stride + h] = n;
}

// The selection, one wavefront per pair.  confident: the pair's hypothesis bound is the n_run its rounds left; otherwise every
// hypothesis ran (none for a pair with fewer than eight matches, sfm-solve.cpp:37) and the kernel writes that n_run itself, so
// the host reads one array whatever the call was.
__global__ __launch_bounds__(kE5Lanes) void essential5_select_kernel(BatchDev b, RunParams rp, const int32_t *n_roots,
                                                                     const int32_t *count, int h_stride, int32_t *best_root,
                                                                     int32_t *n_run, int confident)
{
    extern __shared__ double s_w[];
    __shared__ double s_E[9];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int M = min(b.M[pair], b.max_kp);
    const int H = confident ? n_run[pair] : (M >= 8 ? rp.num_hypotheses : 0);
    if (!confident && lane == 0)
        n_run[pair] = H;
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
    const hipError_t e = hipFuncSetAttribute((const void *)essential5_solve_count_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kE5CountLdsBytes);
    if (e != hipSuccess)
        return e;
    return hipFuncSetAttribute((const void *)essential5_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kE5LdsBytes);
}

static_assert(kE5Checkpoint0 == kE5HypPerBlock, "the first checkpoint is one workgroup of the solve + count kernel");

void launch_essential5(const BatchDev &b, const RunParams &rp, int n_active, int32_t *n_roots, int32_t *count, int h_stride,
                       int32_t *best_root, int32_t *n_run, int32_t *c_max, double confidence, hipStream_t stream)
{
    const int H = rp.num_hypotheses;
    const bool confident = confidence > 0.0;
    // round j counts [first, last) and tests at last; without a confidence level the one round is every hypothesis, untested
    int first = 0, last = confident ? e5_checkpoint_first(H) : H;
    for (int j = 0;; ++j) {
        const int G = (last - first + kE5Lanes - 1) / kE5Lanes;
        hipLaunchKernelGGL(essential5_solve_count_kernel, dim3(G, n_active), dim3(kE5CountThreads), kE5CountLdsBytes, stream, b,
                           rp, n_roots, count, h_stride, first, j == 0 ? (const int32_t *)nullptr : n_run);
        if (!confident)
            break;
        hipLaunchKernelGGL(essential5_horizon_kernel, dim3(n_active), dim3(kE5Lanes), 0, stream, b, count, h_stride, first, last,
                           last == H ? 1 : 0, j, confidence, n_run, c_max);
        if (last == H)
            break;
        first = last;
        last = e5_checkpoint_next(last, H);
    }
    hipLaunchKernelGGL(essential5_select_kernel, dim3(n_active), dim3(kE5Lanes), kE5LdsBytes, stream, b, rp, n_roots, count,
                       h_stride, best_root, n_run, confident ? 1 : 0);
}

void launch_five_point(const double *p1, const double *p2, double *E, int *n, hipStream_t stream)
{
    hipLaunchKernelGGL(five_point_kernel, dim3(1), dim3(64), 0, stream, p1, p2, E, n);
}

}  // namespace mvs
