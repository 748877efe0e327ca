// kernels_experiments.hip -- reference kernels and device-side probes of the diagnostics build.  NOT a translation unit of its
// own: included by kernels.hip under -DMVS_DEBUG_HOOKS only (libmvslam_hip_dbg.so), after every device function of the product
// path and in front of the launch wrappers.  Nothing here is reachable from libmvslam_hip.so.  What is here:
//   ransac_count32_kernel   the vector form of the single-precision counting, which the matrix-core kernels replaced in the
//                           product.  tests/prescreen_gpu_check.py and tests/constants_gpu_check.py compare
//                           the product's counting with it: everything in one launch (mvs_debug_set_count_dense(0)) and as
//                           the finish behind the dense phase (2); byte-identical results are asserted.
//   mfma_probe_kernel, fastmath_check_kernel   probes of the matrix-core tile and of the unscaled sqrt / div sequences
//                           (pairstep_check_kernel, the third probe, sits with the audit in kernels_audit.hip).
// The experiment ladder of rounds 1-3 (ransac_solve / ransac_score / ransac_solve_av / ransac_count behind a variant switch) is
// gone from the tree; what each kernel was, and why it lost, is in docs/DESIGN_rounds_1_2.md and DESIGN.md 4.3.
#ifndef MVS_DEBUG_HOOKS
#error "kernels_experiments.hip belongs to the diagnostics build"
#endif

// Single-precision form of ransac_count2_kernel for pairs in mode 1: the record holds F~ as 9 floats and the two counting
// thresholds, already widened by the pre-screen's band AND by the bound on the binary32 evaluation error (prescreen.hpp),
// the points are rounded to binary32 in LDS (16 bytes per point: one ds_read_b128).  v_fma_f32 issues at twice the rate of
// v_fma_f64, the residual is the same nine instructions.  Exact records do not occur in these pairs before the selection
// (hypotheses without a certificate wait for the exact solve with an "infinite" count).
// Packed single precision.  A plain v_fma_f32 issues at the rate of v_fma_f64 on this part (16 lanes per clock and SIMD);
// the fp32 vector peak is v_pk_fma_f32's: two FMAs per lane and instruction.  Each lane therefore carries TWO points per
// packed register pair -- the LDS block is laid out so that (x2 of point l, x2 of point l + 64) arrive adjacent -- and F comes
// straight out of the scalar registers the record was loaded into: op_sel picks the low or the high float of an aligned SGPR
// pair for both halves, so nothing is duplicated or moved.  Written as inline asm: left to itself hipcc's SLP vectoriser does
// emit v_pk_fma_f32, but with F splatted into vector register pairs first (200 v_mov per 192 packed FMAs; this file is built
// with -fno-slp-vectorize).
typedef __attribute__((address_space(4))) unsigned long long CU64;

// d = a * s.lo + c  /  d = a * s.hi + c  (both halves of a, c; s = an aligned scalar register pair holding two floats)
__device__ __forceinline__ f32x2 pk_fma_slo(f32x2 a, unsigned long long s, f32x2 c)
{
    f32x2 d;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "s"(s), "v"(c));
    return d;
}
__device__ __forceinline__ f32x2 pk_fma_shi(f32x2 a, unsigned long long s, f32x2 c)
{
    f32x2 d;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(d) : "v"(a), "s"(s), "v"(c));
    return d;
}
__device__ __forceinline__ f32x2 pk_fma_vv(f32x2 a, f32x2 b, f32x2 c)
{
    f32x2 d;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

struct Rec32 {                 // one single-precision record as it sits in scalar registers
    unsigned long long q01, q23, q45;   // (F0, F1), (F2, F3), (F4, F5)
    f32x2 f6, f7, f8;                   // (F6, F6), (F7, F7), (F8, F8): the inner addends, in vector registers
    float tu, tl;
};

// inliers among the 128 points a wavefront's lanes hold as two packed planes: A = (x1a, x1b, y1a, y1b), B = (x2a, x2b, y2a, y2b)
__device__ __forceinline__ int count_pair32(const Rec32 &r, const float4 &A, const float4 &B, float thr)
{
    const f32x2 X1 = {A.x, A.y}, Y1 = {A.z, A.w}, X2 = {B.x, B.y}, Y2 = {B.z, B.w};
    const f32x2 u0 = pk_fma_slo(X2, r.q01, pk_fma_shi(Y2, r.q23, r.f6));   // x2 F0 + (y2 F3 + F6)
    const f32x2 u1 = pk_fma_shi(X2, r.q01, pk_fma_slo(Y2, r.q45, r.f7));   // x2 F1 + (y2 F4 + F7)
    const f32x2 u2 = pk_fma_slo(X2, r.q23, pk_fma_shi(Y2, r.q45, r.f8));   // x2 F2 + (y2 F5 + F8)
    const f32x2 e = pk_fma_vv(u0, X1, pk_fma_vv(u1, Y1, u2));
    // NaN (padding lanes) compares false
    return __popcll(__ballot(__builtin_fabsf(e.x) < thr)) + __popcll(__ballot(__builtin_fabsf(e.y) < thr));
}

// phase: 1 = everything in one go (no pilot, no dense phase); 2 = the FINISH (every hypothesis resumes behind the points
// [0, n1) the dense matrix-core phase has already counted: hyp_cnt holds that partial upper-bound count)
template <int CNT_THREADS, int PPL, int SLOTS, int phase, bool STATS = false>
__global__ __launch_bounds__(CNT_THREADS) void ransac_count32_kernel(BatchDev b, RunParams rp, int wg_per_pair)
{
    static_assert(SLOTS == 4 && PPL % 2 == 0, "four records per group; points come in packed pairs");
    static_assert(phase == 1 || phase == 2, "one launch over everything, or the finish behind the dense phase");
    extern __shared__ __attribute__((aligned(16))) double s_cpts[];
    __shared__ int s_bound;
    const int pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int M = min(b.M[pair], b.max_kp);
    if (M < 8 || b.mode[pair] != 1)
        return;
    const int H = rp.num_hypotheses;
    const size_t Hp = (size_t)b.max_groups * kHypPerBlock;
    constexpr int BW = 64 * PPL;                  // points per block
    constexpr int NP = PPL / 2;                   // packed pairs per lane and block
    const int nblk = (M + BW - 1) / BW;
    // points [0, n1) were counted by the dense phase (n1 = dense_points(M, the pilot's bound), a multiple of 32): the finish
    // starts in the block that holds point n1 and blanks the points before it
    const int n1 = phase == 2 ? b.dense_n1[pair] : 0;
    const int blk0 = n1 / BW;
    // phase 2 works through the pair's list of hypotheses the dense phase left alive, four list entries per group
    const uint32_t *clist = b.clist + (size_t)pair * Hp;
    const int n_list = phase == 2 ? b.ccount[pair] : 0;
    // LDS: [block][pair u][plane A / B][lane] float4; point i = blk * BW + u * 128 + half * 64 + lane sits in half `half`
    float *s_f = reinterpret_cast<float *>(s_cpts);
    {
        const double4 *src = reinterpret_cast<const double4 *>(b.pts + (size_t)pair * b.max_kp * 4);
        const float qnan = __builtin_nanf("");
        for (int i = tid; i < nblk * BW; i += CNT_THREADS) {
            float x1 = qnan, y1 = qnan, x2 = qnan, y2 = qnan;
            if (i < M) {
                const double4 p = src[i];
                x1 = (float)p.x; y1 = (float)p.y; x2 = (float)p.z; y2 = (float)p.w;
            }
            const int blk = i / BW, w = i - blk * BW, u = w >> 7, half = (w >> 6) & 1, l = w & 63;
            float *A = s_f + ((((size_t)blk * NP + u) * 2 + 0) * 64 + l) * 4;
            float *Bp = s_f + ((((size_t)blk * NP + u) * 2 + 1) * 64 + l) * 4;
            A[half] = x1; A[2 + half] = y1;
            Bp[half] = x2; Bp[2 + half] = y2;
        }
    }
    int *gbound = b.bound + pair;
    if (tid == 0)
        s_bound = __hip_atomic_load(gbound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const float *Fp = b.hyp_r32 + (size_t)pair * Hp * kHypRec32;   // 48-byte single-precision records
    const uint32_t *okp = reinterpret_cast<const uint32_t *>(b.hyp_okf + (size_t)pair * Hp);
    int32_t *cntp = b.hyp_cnt + (size_t)pair * Hp;
    const float4 *L = reinterpret_cast<const float4 *>(s_f) + lane;   // plane stride 64, pair stride 128, block stride 128 NP
    const int n_groups = phase == 2 ? (n_list + SLOTS - 1) / SLOTS : (H + SLOTS - 1) / SLOTS;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_waves = wg_per_pair * (CNT_THREADS / 64);
    int B = 0;
    unsigned long long visits = 0;
    for (int g = blockIdx.x * (CNT_THREADS / 64) + wave; g < n_groups; g += n_waves) {
        const int h0 = g * SLOTS;
        const int gb = __hip_atomic_load(gbound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        B = __builtin_amdgcn_readfirstlane(max(B, *(volatile int *)&s_bound));
        // the four hypotheses of the group: consecutive ones, or (finish) four entries of the list
        int hq[SLOTS];
        if (phase == 2) {
            const uint32_t mine = lane < SLOTS && h0 + lane < n_list ? clist[h0 + lane] : 0u;
#pragma unroll
            for (int q = 0; q < SLOTS; ++q)
                hq[q] = __builtin_amdgcn_readlane((int)mine, q);
        } else {
#pragma unroll
            for (int q = 0; q < SLOTS; ++q)
                hq[q] = h0 + q;
        }
        Rec32 R[SLOTS];
#pragma unroll
        for (int q = 0; q < SLOTS; ++q) {
            // (one base + constant offsets when the four records are neighbours: the loads coalesce)
            const CU64 *f = phase == 2 ? (const CU64 *)(uintptr_t)(Fp + (size_t)hq[q] * kHypRec32)
                                       : (const CU64 *)(uintptr_t)(Fp + (size_t)h0 * kHypRec32) + q * (kHypRec32 / 2);
            R[q].q01 = f[0];
            R[q].q23 = f[1];
            R[q].q45 = f[2];
            const unsigned long long q67 = f[3], q8u = f[4], ql = f[5];
            const float f6 = __uint_as_float((unsigned)q67), f7 = __uint_as_float((unsigned)(q67 >> 32));
            const float f8 = __uint_as_float((unsigned)q8u);
            R[q].f6 = f32x2{f6, f6};
            R[q].f7 = f32x2{f7, f7};
            R[q].f8 = f32x2{f8, f8};
            R[q].tu = __uint_as_float((unsigned)(q8u >> 32));
            R[q].tl = __uint_as_float((unsigned)ql);
        }
        unsigned alive = 0, wait = 0;
        int c[SLOTS];
#pragma unroll
        for (int q = 0; q < SLOTS; ++q)
            c[q] = 0;
        if (phase == 2) {
            // resume: every listed hypothesis is an approximate record; the dense phase left its upper-bound count over
            // points [0, n1) in hyp_cnt.  A slot that cannot reach the bound (it may have risen since the list was
            // written) even if every remaining point were an inlier is dead on arrival
            const int have = lane < SLOTS && h0 + lane < n_list ? cntp[clist[h0 + lane]] : 0;
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) {
                c[q] = __builtin_amdgcn_readlane(have, q);
                if (h0 + q < n_list && !(c[q] + (M - n1) < B))
                    alive |= 1u << q;
            }
        } else {
            const uint32_t ok4 = __builtin_amdgcn_readfirstlane(okp[g]);
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) {
                const unsigned st = (ok4 >> (8 * k)) & 0xffu;
                alive |= (st == kPsApprox && h0 + k < H) ? (1u << k) : 0u;
                wait |= (st == kPsNeedExact && h0 + k < H) ? (1u << k) : 0u;
            }
        }
        float4 pa[PPL], pb[PPL];   // [2 u] = plane A, [2 u + 1] = plane B of packed pair u
        auto load = [&](float4 (&p)[PPL], int blk) {
            const int nb = min(blk, nblk - 1) * (128 * NP);
#pragma unroll
            for (int u = 0; u < PPL; ++u)
                p[u] = L[nb + u * 64];
            if (blk == blk0 && n1 > blk0 * BW) {
                // the dense phase has already counted the points of this block below n1: blank them (NaN is no inlier).
                // p[2 u] / p[2 u + 1] hold points blk BW + 128 u + lane (x, z components) and + 64 (y, w components)
                const float qnan = __builtin_nanf("");
#pragma unroll
                for (int u = 0; u < NP; ++u) {
                    const int i0 = blk * BW + u * 128 + lane;
                    if (i0 < n1) { p[2 * u].x = qnan; p[2 * u + 1].x = qnan; }
                    if (i0 + 64 < n1) { p[2 * u].y = qnan; p[2 * u + 1].y = qnan; }
                }
            }
        };
        auto process = [&](const float4 (&p)[PPL], int blk) {
            const int need = B - max(M - (blk + 1) * BW, 0);   // a slot whose count stays below this cannot reach B
            if (STATS)
                visits += (unsigned)__builtin_popcount(alive);
            if (alive == (1u << SLOTS) - 1u) {
                // all four alive (the usual state until they die together): one straight-line stretch, so that the
                // scheduler interleaves the slots' independent FMA chains -- slot by slot behind uniform branches a
                // wavefront has two short dependent chains in flight and the SIMD waits on latencies
                int add[SLOTS];
#pragma unroll
                for (int q = 0; q < SLOTS; ++q) {
                    add[q] = 0;
#pragma unroll
                    for (int u = 0; u < NP; ++u)
                        add[q] += count_pair32(R[q], p[2 * u], p[2 * u + 1], R[q].tu);
                }
#pragma unroll
                for (int q = 0; q < SLOTS; ++q) {
                    c[q] += add[q];
                    alive &= (c[q] < need) ? ~(1u << q) : ~0u;
                }
            } else {
#pragma unroll
                for (int q = 0; q < SLOTS; ++q) {
                    if (alive & (1u << q)) {
#pragma unroll
                        for (int u = 0; u < NP; ++u)
                            c[q] += count_pair32(R[q], p[2 * u], p[2 * u + 1], R[q].tu);
                        if (c[q] < need) alive &= ~(1u << q);
                    }
                }
            }
        };
        if (alive)
            load(pa, blk0);
        for (int blk = blk0; blk < nblk && alive; blk += 2) {
            load(pb, blk + 1);
            process(pa, blk);
            if (!(blk + 1 < nblk && alive))
                break;
            load(pa, blk + 2);
            process(pb, blk + 1);
        }
        // lower bounds of the slots that saw every point: one more pass against the lower threshold
        int v[SLOTS], lo[SLOTS];
        int cm = -1;
#pragma unroll
        for (int q = 0; q < SLOTS; ++q) {
            const bool al = (alive >> q) & 1u;
            v[q] = al ? c[q] : ((wait >> q) & 1u) ? 0x7fffffff : -1;
            lo[q] = -1;
            if (al) {
                int cl = 0;
                for (int blk = 0; blk < nblk; ++blk) {
#pragma unroll
                    for (int u = 0; u < NP; ++u)
                        cl += count_pair32(R[q], L[blk * (128 * NP) + (2 * u) * 64], L[blk * (128 * NP) + (2 * u + 1) * 64], R[q].tl);
                }
                if (STATS)
                    visits += (unsigned)nblk;
                lo[q] = cl;
            }
            cm = max(cm, lo[q]);
        }
        if (lane < SLOTS && (phase != 2 || h0 + lane < n_list)) {
            int mine = v[0], where = hq[0];
#pragma unroll
            for (int q = 1; q < SLOTS; ++q) {
                mine = lane == q ? v[q] : mine;
                where = lane == q ? hq[q] : where;
            }
            cntp[where] = mine;
        }
        cm = __builtin_amdgcn_readfirstlane(cm);
        if (cm > B) {
            B = cm;
            if (lane == 0) {
                atomicMax(&s_bound, cm);
                __hip_atomic_fetch_max(gbound, cm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        B = max(B, __builtin_amdgcn_readfirstlane(gb));
    }
    if (STATS && lane == 0 && b.stats)
        atomicAdd(&b.stats[3], visits * (unsigned long long)BW);   // executed single-precision evaluations
}

constexpr int kCnt32Threads = 768;
constexpr int kCnt32Slots = 4;     // hypotheses a wavefront carries at a time
constexpr int kCnt32Ppl = 4;       // single-precision counting: four points per lane and block (scalar work per evaluation halves)
static size_t count32_lds_bytes(int max_kp)
{
    const int bw = 64 * kCnt32Ppl;
    return (size_t)((max_kp + bw - 1) / bw) * bw * 4 * sizeof(float);
}
template <int phase>
static void launch_count32(const BatchDev &b, const RunParams &rp, int wg, int n_active, bool stats, hipStream_t stream)
{
    const dim3 grid(wg, n_active), block(kCnt32Threads);
    const size_t lds = count32_lds_bytes(b.max_kp);
    if (stats)
        hipLaunchKernelGGL((ransac_count32_kernel<kCnt32Threads, kCnt32Ppl, kCnt32Slots, phase, true>), grid, block, lds, stream, b,
                           rp, wg);
    else
        hipLaunchKernelGGL((ransac_count32_kernel<kCnt32Threads, kCnt32Ppl, kCnt32Slots, phase>), grid, block, lds, stream, b, rp,
                           wg);
}


// diagnostics: one 32 x 32 x 32 tile through the two MFMAs exactly as the counting kernels issue them.  A, B: [32][32] bf16
// bit patterns (row = point / hypothesis, column = K slot); out[point][hypothesis] (binary32).  Pins the K slot mapping, the
// accumulator layout and the accumulation error the bound assumes (tests/test_prescreen.py).
__global__ __launch_bounds__(64) void mfma_probe_kernel(const uint16_t *A, const uint16_t *B, float *out)
{
    const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
    v8bf a[2], bb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint32_t wa[4], wb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s0 = j * 16 + half * 8 + 2 * e;
            wa[e] = (uint32_t)A[col * 32 + s0] | ((uint32_t)A[col * 32 + s0 + 1] << 16);
            wb[e] = (uint32_t)B[col * 32 + s0] | ((uint32_t)B[col * 32 + s0 + 1] << 16);
        }
        a[j] = __builtin_bit_cast(v8bf, make_uint4(wa[0], wa[1], wa[2], wa[3]));
        bb[j] = __builtin_bit_cast(v8bf, make_uint4(wb[0], wb[1], wb[2], wb[3]));
    }
    v16f acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], bb[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], bb[1], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;   // the point
        out[row * 32 + col] = acc[r];
    }
}
void launch_mfma_probe(const uint16_t *A, const uint16_t *B, float *out, hipStream_t stream)
{
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, stream, A, B, out);
}


// diagnostics: compare the unscaled sqrt / div sequences with the compiler's IEEE ones on caller-supplied operands.
// out[0] = sqrt mismatches among operands that pass sqrt_fast_ok, out[1] = div mismatches among operand pairs
// inside the guarded range, out[2] / out[3] = number of operands / pairs that were inside the guards.
__global__ __launch_bounds__(256) void fastmath_check_kernel(const double *x, const double *y, int n, unsigned long long *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const double a = x[i], b = y[i];
    if (sqrt_fast_ok(a)) {
        const double f = sqrt_fast(a), g = dsqrt(a);
        atomicAdd(&out[2], 1ull);
        if (__double_as_longlong(f) != __double_as_longlong(g) && !(f != f && g != g))
            atomicAdd(&out[0], 1ull);
    }
    const double aa = dabs(a), ab = dabs(b);
    if (ab >= 0x1p-200 && ab <= 0x1p200 && ((aa >= 0x1p-200 && aa <= 0x1p200) || a == 0.0)) {
        const double f = div_fast(a, b), g = a / b;
        atomicAdd(&out[3], 1ull);
        if (__double_as_longlong(f) != __double_as_longlong(g))
            atomicAdd(&out[1], 1ull);
    }
}
