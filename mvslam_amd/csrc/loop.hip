// loop.hip -- loop-closure candidates of a resident sequence (include/mvslam_hip.h,
// mvs_seq_loop_scores / mvs_seq_select_loops / mvs_seq_verify_loops).
//
//   loop_scores_mfma_kernel   score[i][j] = queries of frame j that pass the matcher's test against the trains of frame i, for
//                             256-bit descriptors on the FP4 matrix cores: match_mfma_kernel's tile, with the query block's B
//                             operand kept in registers over a RUN of base frames and nothing written per query.
//   loop_scores_popc_kernel   the same definition by xor + popcount, for 128- and 512-bit descriptors (correct, not fast).
//   loop_select_rows_kernel   per query frame j the top_k eligible base frames; loop_select_compact_kernel the list.
//   loop_gather_kernel        the candidates' frames copied into a batch whose pairs own their images.
//
// Every score is an integer sum of ballot counts: no output byte depends on how the workgroups are scheduled.
#include <algorithm>

#include "match_fp4.hpp"

namespace mvs {

namespace {

// The matcher's test on the two smallest distances (the end of match_mfma_kernel; visual-feature.cpp:67-68); n_i >= 2 is
// the caller's.
__device__ __forceinline__ bool loop_pass(int D0, int D1, double ratio, double max_dist)
{
    const float f0 = (float)D0, f1 = (float)D1;
    const bool check1 = (double)f0 < ratio * (double)f1;
    const bool check2 = (max_dist < 0.0) || ((double)f0 <= max_dist);
    return check1 && check2;
}

// grid (ceil(N / 256), j, run): the workgroup owns queries [256 x, 256 x + 256) of frame j and the base frames
// [run * run_len, min((run + 1) * run_len, j - min_gap + 1)).  Layouts, operand forms and the exactness argument are
// match_mfma_kernel's; the key carries no train index (its low 12 bits are zero), so equal distances give equal keys and the
// min / max insertion counts them with multiplicity: two trains at the smallest distance leave D1 = D0.  CAPPED as there: only
// keys below the cap can change a verdict, and the verdict is all that is kept.
template <bool CAPPED>
__global__ __launch_bounds__(kMmThreads) __attribute__((amdgpu_waves_per_eu(3, 8))) void loop_scores_mfma_kernel(
    LoopDev d, double ratio, double max_dist, int cap_dist, int min_gap, int run_len)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[2][32 * kMmRowBytes];   // unpacked train tiles (double buffer)
    __shared__ __attribute__((aligned(16))) float s_key[2][32];                           // (|t| + 257) << 12
    const int j = blockIdx.y, F = d.n_frames;
    const int n2 = min(d.n_kp[j], d.max_kp);
    const int q0 = blockIdx.x * kMmQueries;
    const int i_begin = blockIdx.z * run_len, i_end = min(i_begin + run_len, j - min_gap + 1);
    if (q0 >= n2 || i_begin >= i_end)
        return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 31, half = lane >> 5;
    // B operands, once per run: this lane's 32-bit slices of its queries, one per k-step (query form: 0b1010 = -1.0)
    v8i Bf[kMmBlocks][4];
    int qn[kMmBlocks];
    uint32_t capk[kMmBlocks];
#pragma unroll
    for (int c = 0; c < kMmBlocks; ++c) {
        const int q = q0 + w * 32 * kMmBlocks + c * 32 + col;
        const uint32_t *qd = d.desc + ((size_t)j * d.max_kp + (q < n2 ? q : q0)) * 8;
        const uint4 lo = *reinterpret_cast<const uint4 *>(qd), hi = *reinterpret_cast<const uint4 *>(qd + 4);
        const uint32_t dq[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        qn[c] = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s)
            qn[c] += __popc(dq[s]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const v4i t = unpack32_fp4((uint32_t)((((uint64_t)dq[2 * s + 1] << 32) | dq[2 * s]) >> (32 * half)));
            const v4i m = t | (t << 2);
            Bf[c][s] = __builtin_shufflevector(m, m, 0, 1, 2, 3, -1, -1, -1, -1);
        }
        // relevant keys of this lane's query: distance = (key >> 12) - 257 + |q| < cap_dist (a negative bound has the sign bit
        // set, above every key: every key is relevant)
        capk[c] = __float_as_uint((float)((cap_dist + kMmKeyBias - qn[c]) * (1 << kMmKeyShift)));
    }
    for (int i = i_begin; i < i_end; ++i) {
        const int n1 = min(d.n_kp[i], d.max_kp);
        if (n1 < 2)   // wave-uniform: no query passes against fewer than two trains, the entry stays zero
            continue;
        const uint32_t *tr = d.desc + (size_t)i * d.max_kp * 8;
        // stage tile `t` (trains [32 t, 32 t + 32)) into buffer `buf`: work item = (row, dword): 32 bits -> 32 nibbles
        auto stage = [&](int t, int buf) {
#pragma unroll
            for (int it0 = 0; it0 < 256 / kMmThreads; ++it0) {
                const int it = tid + it0 * kMmThreads, row = it >> 3, dw = it & 7;
                const int tr_i = t * 32 + row;
                const uint32_t bits = tr_i < n1 ? tr[(size_t)tr_i * 8 + dw] : 0u;
                *reinterpret_cast<v4i *>(&s_tile[buf][row * kMmRowBytes + dw * 16]) = unpack32_fp4(bits);
                int tn = __popc(bits);
                tn += __shfl_xor(tn, 1);
                tn += __shfl_xor(tn, 2);
                tn += __shfl_xor(tn, 4);
                if (dw == 0)
                    s_key[buf][row] = tr_i < n1 ? (float)((tn + kMmKeyBias) << kMmKeyShift) : __uint_as_float(kMmKeyNone);
            }
        };
        const int n_tiles = (n1 + 31) / 32;
        uint32_t k0[kMmBlocks], k1[kMmBlocks];
#pragma unroll
        for (int c = 0; c < kMmBlocks; ++c)
            k0[c] = k1[c] = kMmKeyNone;
        stage(0, 0);   // the last tile of the frame before ended with a barrier: both buffers are free
        __syncthreads();
        for (int t = 0; t < n_tiles; ++t) {
            const int buf = t & 1;
            if (t + 1 < n_tiles)
                stage(t + 1, buf ^ 1);
            // accumulator: column = lane & 31 (the query), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (the train)
            v16f kb;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float4 kb4 = *reinterpret_cast<const float4 *>(&s_key[buf][8 * g4 + 4 * half]);
                kb[4 * g4] = kb4.x;
                kb[4 * g4 + 1] = kb4.y;
                kb[4 * g4 + 2] = kb4.z;
                kb[4 * g4 + 3] = kb4.w;
            }
            v16f acc[kMmBlocks];
            const unsigned char *arow = &s_tile[buf][col * kMmRowBytes + half * 16];   // A: row = lane & 31, dword 2 s + half
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const v4i a4 = *reinterpret_cast<const v4i *>(arow + s * 32);
                const v8i Af = __builtin_shufflevector(a4, a4, 0, 1, 2, 3, -1, -1, -1, -1);
#pragma unroll
                for (int c = 0; c < kMmBlocks; ++c)
                    acc[c] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(Af, Bf[c][s], s == 0 ? kb : acc[c], 4, 4, 0,
                                                                             kMmScaleTrain, 0, kMmScaleQuery);
            }
            // no inline assembly on the accumulators (the note above key_insert_mm): compiler-visible min / max only
            if (!CAPPED) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
#pragma unroll
                    for (int c = 0; c < kMmBlocks; ++c)
                        key_insert_mm(k0[c], k1[c], __float_as_uint(acc[c][r]));
            } else {
#pragma unroll
                for (int c = 0; c < kMmBlocks; ++c) {
                    uint32_t g[4];
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4)
                        g[q4] = min(umin3(__float_as_uint(acc[c][4 * q4]), __float_as_uint(acc[c][4 * q4 + 1]),
                                          __float_as_uint(acc[c][4 * q4 + 2])),
                                    __float_as_uint(acc[c][4 * q4 + 3]));
                    const uint32_t tm = min(umin3(g[0], g[1], g[2]), g[3]);
                    if (__any(tm < capk[c])) {   // wave-uniform: some lane has a relevant key in this tile
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4)
                            if (__any(g[q4] < capk[c])) {
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    key_insert_mm(k0[c], k1[c], __float_as_uint(acc[c][4 * q4 + e]));
                            }
                    }
                }
            }
            __syncthreads();
        }
        // lanes l and l + 32 saw the same query over different rows: merge, test, count
        int passed = 0;
#pragma unroll
        for (int c = 0; c < kMmBlocks; ++c) {
            uint32_t m0 = k0[c], m1 = k1[c];
            const uint32_t o0 = (uint32_t)__shfl_xor((int)k0[c], 32), o1 = (uint32_t)__shfl_xor((int)k1[c], 32);
            key_insert_mm(m0, m1, o0);
            key_insert_mm(m0, m1, o1);
            const int q = q0 + w * 32 * kMmBlocks + c * 32 + col;
            // the integer keys (exact: below 2^22); distance = (key >> 12) - 257 + |q|
            const uint32_t i0 = (uint32_t)__uint_as_float(m0), i1 = (uint32_t)__uint_as_float(m1);
            const int D0 = m0 == kMmKeyNone ? 0x7fffffff : (int)(i0 >> kMmKeyShift) - kMmKeyBias + qn[c];
            const int D1 = m1 == kMmKeyNone ? 0x7fffffff : (int)(i1 >> kMmKeyShift) - kMmKeyBias + qn[c];
            const bool pass = half == 0 && q < n2 && loop_pass(D0, D1, ratio, max_dist);
            passed += __popcll(__ballot(pass));
        }
        if (lane == 0 && passed)
            atomicAdd(&d.score[(size_t)i * F + j], passed);
    }
}

// grid (ceil(N / 256), j, i): one query per thread, every train of frame i read in turn (wave-uniform addresses).
template <int DW>
__global__ __launch_bounds__(256) void loop_scores_popc_kernel(LoopDev d, double ratio, double max_dist, int min_gap)
{
    const int j = blockIdx.y, i = blockIdx.z, F = d.n_frames;
    if (i > j - min_gap)
        return;
    const int n1 = min(d.n_kp[i], d.max_kp), n2 = min(d.n_kp[j], d.max_kp);
    const int q0 = blockIdx.x * 256;
    if (q0 >= n2 || n1 < 2)
        return;
    const int q = q0 + threadIdx.x;
    const bool live = q < n2;
    uint32_t qv[DW];
    const uint32_t *qd = d.desc + ((size_t)j * d.max_kp + (live ? q : q0)) * DW;
#pragma unroll
    for (int k = 0; k < DW; ++k)
        qv[k] = qd[k];
    const uint32_t *tr = d.desc + (size_t)i * d.max_kp * DW;
    int D0 = 0x7fffffff, D1 = 0x7fffffff;   // the two smallest distances, with multiplicity
    for (int r = 0; r < n1; ++r) {
        int dist = 0;
#pragma unroll
        for (int k = 0; k < DW; ++k)
            dist += __popc(qv[k] ^ tr[(size_t)r * DW + k]);
        if (dist < D0) {
            D1 = D0;
            D0 = dist;
        } else if (dist < D1)
            D1 = dist;
    }
    const int passed = __popcll(__ballot(live && loop_pass(D0, D1, ratio, max_dist)));
    if ((threadIdx.x & 63) == 0 && passed)
        atomicAdd(&d.score[(size_t)i * F + j], passed);
}

// ---- selection ---------------------------------------------------------------------------------------------------------
constexpr int kLoopSelThreads = 256;
constexpr int kLoopSelPerThread = kLoopMaxFrames / kLoopSelThreads;
static_assert(kMaxKp < (1 << 13) && kLoopMaxFrames <= (1 << 12), "score and base frame share a 32-bit selection key");

// grid j: the top_k eligible base frames of query frame j.  key = score << 12 | (4095 - i): unique per i, larger = better
// score, then smaller i.  Round k takes the largest key below round k - 1's.
__global__ __launch_bounds__(kLoopSelThreads) void loop_select_rows_kernel(LoopDev d)
{
    __shared__ uint32_t s_red[kLoopSelThreads / 64];
    const int j = blockIdx.x, F = d.n_frames, tid = threadIdx.x;
    uint32_t key[kLoopSelPerThread];
#pragma unroll
    for (int u = 0; u < kLoopSelPerThread; ++u) {
        const int i = tid + u * kLoopSelThreads;
        const int sc = i < j ? d.score[(size_t)i * F + j] : 0;
        key[u] = sc >= d.min_score ? ((uint32_t)sc << 12) | (uint32_t)(4095 - i) : 0u;
    }
    uint32_t prev = 0xffffffffu;
    int n = 0;
    for (; n < d.top_k; ++n) {
        uint32_t best = 0u;
#pragma unroll
        for (int u = 0; u < kLoopSelPerThread; ++u)
            best = max(best, key[u] < prev ? key[u] : 0u);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            best = max(best, (uint32_t)__shfl_xor((int)best, o));
        if ((tid & 63) == 0)
            s_red[tid >> 6] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kLoopSelThreads / 64; ++w)
            best = max(best, s_red[w]);
        __syncthreads();   // s_red is rewritten by the next round
        if (best == 0u)
            break;
        if (tid == 0)
            d.row_key[(size_t)j * d.top_k + n] = best;
        prev = best;
    }
    if (tid == 0)
        d.row_n[j] = n;
}

// one workgroup: exclusive prefix sum of the rows' counts (integer scan, ascending j) and the list, cut at max_candidates
__global__ __launch_bounds__(kLoopSelThreads) void loop_select_compact_kernel(LoopDev d)
{
    __shared__ int s_wave[kLoopSelThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = d.n_frames;
    int running = 0;
    for (int base = 0; base < F; base += kLoopSelThreads) {
        const int j = base + tid;
        const int n = j < F ? d.row_n[j] : 0;
        int incl = n;   // inclusive scan inside the wavefront
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            incl += lane >= o ? v : 0;
        }
        if (lane == 63)
            s_wave[wave] = incl;
        __syncthreads();
        int pos = running + incl - n, total = 0;
#pragma unroll
        for (int w = 0; w < kLoopSelThreads / 64; ++w) {
            pos += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        for (int k = 0; k < n && pos + k < d.max_candidates; ++k) {
            const uint32_t key = (uint32_t)d.row_key[(size_t)j * d.top_k + k];
            mvs_loop_candidate c;
            c.i = 4095 - (int)(key & 0xfffu);
            c.j = j;
            c.score = (int)(key >> 12);
            c.accepted = 0;
            d.cand[pos + k] = c;
        }
        running += total;
        __syncthreads();   // s_wave is rewritten by the next tile
    }
    const int kept = min(running, d.max_candidates);
    for (int c = kept + tid; c < d.max_candidates; c += kLoopSelThreads)
        d.cand[c] = mvs_loop_candidate{0, 0, 0, 0};
    if (tid == 0) {
        d.counts[0] = kept;
        d.counts[1] = running;
    }
}

// grid (max_candidates, chunks): pair c of the batch = (frame i, frame j) of candidate c
__global__ __launch_bounds__(256) void loop_gather_kernel(LoopDev d, BatchDev b)
{
    const int c = blockIdx.x;
    if (c >= d.counts[0])
        return;
    const mvs_loop_candidate cd = d.cand[c];
    const size_t N = (size_t)d.max_kp, DW = (size_t)d.desc_words;
    const size_t fi = (size_t)cd.i * N, fj = (size_t)cd.j * N, pc = (size_t)c * N;
    const int first = blockIdx.y * 256 + threadIdx.x, step = gridDim.y * 256;
    uint32_t *desc1 = const_cast<uint32_t *>(b.desc1), *desc2 = const_cast<uint32_t *>(b.desc2);
    float *kp1 = const_cast<float *>(b.kp1), *kp2 = const_cast<float *>(b.kp2);
    uint8_t *oct1 = const_cast<uint8_t *>(b.oct1), *oct2 = const_cast<uint8_t *>(b.oct2);
    for (size_t e = first; e < N * DW; e += step) {
        desc1[pc * DW + e] = d.desc[fi * DW + e];
        desc2[pc * DW + e] = d.desc[fj * DW + e];
    }
    for (size_t e = first; e < N * 2; e += step) {
        kp1[pc * 2 + e] = d.kp[fi * 2 + e];
        kp2[pc * 2 + e] = d.kp[fj * 2 + e];
    }
    for (size_t e = first; e < N; e += step) {
        oct1[pc + e] = d.oct[fi + e];
        oct2[pc + e] = d.oct[fj + e];
    }
    if (blockIdx.y == 0) {
        if (threadIdx.x < 9) {
            const_cast<double *>(b.K)[9 * (size_t)c + threadIdx.x] = d.K[9 * (size_t)cd.i + threadIdx.x];
            const_cast<double *>(b.Kinv)[9 * (size_t)c + threadIdx.x] = d.Kinv[9 * (size_t)cd.i + threadIdx.x];
        }
        if (threadIdx.x == 0) {
            const_cast<int32_t *>(b.n1)[c] = d.n_kp[cd.i];
            const_cast<int32_t *>(b.n2)[c] = d.n_kp[cd.j];
            const_cast<int64_t *>(b.gidx)[c] = (int64_t)c;
        }
    }
}

}  // namespace

// Base frames per workgroup of the matrix-core kernel: long runs amortise the query unpack, short ones keep a short
// sequence's few workgroups apart.
static int loop_run_len(int n_frames, int min_gap) { return n_frames - min_gap > 64 ? 16 : 4; }

hipError_t launch_loop_scores(const LoopDev &d, double ratio, double max_dist, int min_gap, hipStream_t stream)
{
    const int F = d.n_frames;
    // the kernels ADD to the table: without the clear they would add to the scores of the call before
    const hipError_t e = hipMemsetAsync(d.score, 0, (size_t)F * F * sizeof(int32_t), stream);
    if (e != hipSuccess)
        return e;
    if (d.desc_words == 8) {
        const int run = loop_run_len(F, min_gap);
        const dim3 grid((d.max_kp + kMmQueries - 1) / kMmQueries, F, (F - min_gap + run - 1) / run);
        const int cap = match_cap_distance(ratio, max_dist);
        if (cap >= 0)
            hipLaunchKernelGGL(loop_scores_mfma_kernel<true>, grid, dim3(kMmThreads), 0, stream, d, ratio, max_dist, cap, min_gap, run);
        else
            hipLaunchKernelGGL(loop_scores_mfma_kernel<false>, grid, dim3(kMmThreads), 0, stream, d, ratio, max_dist, 0, min_gap, run);
    } else {
        const dim3 grid((d.max_kp + 255) / 256, F, F - min_gap);
        if (d.desc_words == 4)
            hipLaunchKernelGGL(loop_scores_popc_kernel<4>, grid, dim3(256), 0, stream, d, ratio, max_dist, min_gap);
        else
            hipLaunchKernelGGL(loop_scores_popc_kernel<16>, grid, dim3(256), 0, stream, d, ratio, max_dist, min_gap);
    }
    return hipSuccess;
}

void launch_loop_select(const LoopDev &d, hipStream_t stream)
{
    hipLaunchKernelGGL(loop_select_rows_kernel, dim3(d.n_frames), dim3(kLoopSelThreads), 0, stream, d);
    hipLaunchKernelGGL(loop_select_compact_kernel, dim3(1), dim3(kLoopSelThreads), 0, stream, d);
}

void launch_loop_gather(const LoopDev &d, const BatchDev &b, hipStream_t stream)
{
    const int chunks = std::min(64, (d.max_kp * d.desc_words + 255) / 256);
    hipLaunchKernelGGL(loop_gather_kernel, dim3(d.max_candidates, chunks), dim3(256), 0, stream, d, b);
}

}  // namespace mvs
