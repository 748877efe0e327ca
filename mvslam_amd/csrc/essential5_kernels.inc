// essential5_kernels.inc -- the solve + count kernel and the selection kernel of the five-point RANSAC, included TWICE by
// essential5.hip (which documents them):
//   E5_ROUNDS 0  essential5_solve_count_kernel / essential5_select_kernel: every hypothesis of [0, rp.num_hypotheses).  These are,
//                token for token, the kernels there were before the termination rule: a call without a confidence level runs the
//                code it ran, not a specialisation the compiler is trusted to fold back into it;
//   E5_ROUNDS 1  e5_solve_count_rounds_kernel / e5_select_rounds_kernel: a later round of a call with a confidence level, and its
//                selection -- the hypothesis range starts at h_first, a pair that has stopped (n_run >= 0) is skipped, the
//                selection's bound is the pair's n_run.
// One text rather than a template <bool> body inlined into two kernels: that was tried, and the structs handed through the
// inlined call changed the register allocation of the plain kernels (254 -> 242 VGPRs, 68 -> 86 SGPRs).
#if E5_ROUNDS
#define E5_SOLVE_COUNT_KERNEL e5_solve_count_rounds_kernel
#define E5_SELECT_KERNEL e5_select_rounds_kernel
#else
#define E5_SOLVE_COUNT_KERNEL essential5_solve_count_kernel
#define E5_SELECT_KERNEL essential5_select_kernel
#endif

#if E5_ROUNDS
__global__ __launch_bounds__(kE5Lanes) void E5_SOLVE_COUNT_KERNEL(BatchDev b, RunParams rp, int32_t *n_roots, int32_t *count,
                                                                  int h_stride, int h_first, const int32_t *n_run)
#else
__global__ __launch_bounds__(kE5Lanes) void E5_SOLVE_COUNT_KERNEL(BatchDev b, RunParams rp, int32_t *n_roots, int32_t *count,
                                                                  int h_stride)
#endif
{
    extern __shared__ double s_w[];
    const int pair = blockIdx.y, lane = threadIdx.x;
    const int M = min(b.M[pair], b.max_kp);
    if (M < 8)   // sfm-solve.cpp:37; the selection reports "no model" without reading the tables
        return;
#if E5_ROUNDS
    if (n_run[pair] >= 0)   // the pair has stopped at an earlier checkpoint (block-uniform, before any work)
        return;
#endif
    const int H = rp.num_hypotheses;
#if E5_ROUNDS
    const int h = h_first + blockIdx.x * kE5Lanes + lane;
#else
    const int h = blockIdx.x * kE5Lanes + lane;
#endif
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

#if E5_ROUNDS
__global__ __launch_bounds__(kE5Lanes) void E5_SELECT_KERNEL(BatchDev b, RunParams rp, const int32_t *n_roots, const int32_t *count,
                                                             int h_stride, int32_t *best_root, const int32_t *n_run)
#else
__global__ __launch_bounds__(kE5Lanes) void E5_SELECT_KERNEL(BatchDev b, RunParams rp, const int32_t *n_roots, const int32_t *count,
                                                             int h_stride, int32_t *best_root)
#endif
{
    extern __shared__ double s_w[];
    __shared__ double s_E[9];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int M = min(b.M[pair], b.max_kp);
#if E5_ROUNDS
    const int H = n_run[pair];   // (0 where M < 8)
#else
    const int H = rp.num_hypotheses;
#endif
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

#undef E5_SOLVE_COUNT_KERNEL
#undef E5_SELECT_KERNEL
