// seq_graph.hip -- the pose graph of a resident sequence: nodes = the trajectory of
// seq_chain_kernel, edges = the refined lagged pairs of mvs_seq_run_lags with their 6 x 6 marginal covariances, assembled on
// the device for the solver of posegraph.hip.  include/mvslam_hip.h (mvs_seq_build_pose_graph) states the definition and
// tests/seq_graph_model.py restates it in numpy; the two agree byte for byte because every value here is a chain of single
// binary64 operations in a fixed order (the file is compiled with -ffp-contract=off like the rest; the only fused operations
// are the explicit ones of the Cholesky test, which decides and whose values are not stored).
//
//   seq_graph_edges_kernel    one thread per candidate slot (d, k): gates, scale, Z, S' -> the slot.  Thread i < n_frames
//                             also writes node i = (R_i, t_i).
//   seq_graph_compact_kernel  one workgroup: exclusive prefix sum of the keep flags, tile of 256 slots by tile, and the
//                             scatter of every kept slot to its place.  Integer scan, no atomics: the output order is the
//                             slot order, ascending (d, k).
//   loop_edges_kernel         one workgroup: the verified loop-closure candidates (loop.hip) through the same rule, appended
//                             behind the built edges in candidate order.
// The positive-definiteness test of an edge covariance is lm_math.hpp's chol_packed<6>, the one the solver's pg_prep_kernel runs.
#include "lm_math.hpp"

namespace mvs {

namespace {

constexpr int kSgThreads = 256;

__global__ __launch_bounds__(kSgThreads) void seq_graph_edges_kernel(SeqGraphDev g)
{
    const int idx = blockIdx.x * kSgThreads + threadIdx.x;
    const int F = g.n_frames;
    if (idx < F) {
        double *np = g.node_pose + 12 * (int64_t)idx;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            np[k] = g.traj_R[9 * (int64_t)idx + k];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            np[9 + k] = g.traj_t[3 * (int64_t)idx + k];
    }
    if (idx >= g.n_slots)
        return;
    int d = 1;
    while (d < g.max_lag && idx >= seq_graph_slot_off(F, d + 1))
        ++d;
    const int k = idx - seq_graph_slot_off(F, d);   // 0 <= k < F - d
    const LagDev L = g.lags[d];
    const mvs_pair_result &pr = L.results[k];
    const mvs_refine_result &rr = L.refined[k];
    const double *Rk = g.traj_R + 9 * (int64_t)k, *tk = g.traj_t + 3 * (int64_t)k, *tn = g.traj_t + 3 * (int64_t)(k + d);
    // q = R_k^T (t_{k+d} - t_k): the step of the trajectory in frame k
    const double d0 = tn[0] - tk[0], d1 = tn[1] - tk[1], d2 = tn[2] - tk[2];
    double q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        q[i] = (Rk[i] * d0 + Rk[3 + i] * d1) + Rk[6 + i] * d2;
    double *Zo = g.slot_pose + 12 * (int64_t)idx, *Co = g.slot_cov + 36 * (int64_t)idx;
    int keep = 0, kind = 0;
    double scale = 0.0;
    if (pr.valid && rr.ok && pr.n_points >= g.min_points && rr.error <= g.max_error) {
        const double t0 = rr.t[0], t1 = rr.t[1], t2 = rr.t[2];
        const double s = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) / sqrt((t0 * t0 + t1 * t1) + t2 * t2);
        if (s > 0.0 && s < __builtin_inf()) {
            double S[21];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c)
                    S[lidx(r, c)] = ((r < 3 ? 1.0 : s) * rr.pose_cov[6 * r + c]) * (c < 3 ? 1.0 : s);
            if (chol_packed<6>(S)) {   // pg_prep_kernel's test: is the packed lower triangle positive definite?
                keep = 1;
                scale = s;
#pragma unroll
                for (int i = 0; i < 9; ++i)
                    Zo[i] = rr.R[i];
                Zo[9] = s * t0;
                Zo[10] = s * t1;
                Zo[11] = s * t2;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c < 6; ++c)
                        Co[6 * r + c] = ((r < 3 ? 1.0 : s) * rr.pose_cov[6 * r + c]) * (c < 3 ? 1.0 : s);
            }
        }
    }
    if (!keep && d == 1 && g.chain_on) {   // the chain fallback: Z = G_k^-1 G_{k+1}, R_k^T in front
        const double *Rn = g.traj_R + 9 * (int64_t)(k + 1);
        keep = 1;
        kind = 1;
        scale = 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                Zo[3 * i + j] = (Rk[i] * Rn[j] + Rk[3 + i] * Rn[3 + j]) + Rk[6 + i] * Rn[6 + j];
            Zo[9 + i] = q[i];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c)
                Co[6 * r + c] = r == c ? g.chain_var[r / 3] : 0.0;
    }
    g.slot_keep[idx] = keep;
    g.slot_kind[idx] = kind;
    g.slot_scale[idx] = scale;
}

__global__ __launch_bounds__(kSgThreads) void seq_graph_compact_kernel(SeqGraphDev g)
{
    __shared__ int s_wave[kSgThreads / 64];
    __shared__ int s_pos[kSgThreads];   // place of the tile's slot among the edges, -1 = dropped
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = g.n_frames;
    int running = 0;   // kept slots before this tile (the same in every thread)
    for (int base = 0; base < g.n_slots; base += kSgThreads) {
        const int slot = base + tid;
        const int keep = slot < g.n_slots ? g.slot_keep[slot] : 0;
        const unsigned long long bal = __ballot(keep != 0);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0)
            s_wave[wave] = __popcll(bal);
        __syncthreads();
        int pos = running + before, total = 0;
#pragma unroll
        for (int w = 0; w < kSgThreads / 64; ++w) {
            pos += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        s_pos[tid] = keep ? pos : -1;
        if (keep) {
            int d = 1;
            while (d < g.max_lag && slot >= seq_graph_slot_off(F, d + 1))
                ++d;
            const int k = slot - seq_graph_slot_off(F, d);
            g.edge_src[pos] = k;
            g.edge_dst[pos] = k + d;
            g.edge_lag[pos] = d;
            g.edge_kind[pos] = g.slot_kind[slot];
            g.edge_scale[pos] = g.slot_scale[slot];
        }
        __syncthreads();
        // the tile's 12 + 36 doubles per kept slot, the workgroup together (consecutive threads, consecutive doubles)
        const int n_tile = min(kSgThreads, g.n_slots - base);
        for (int i = tid; i < n_tile * 48; i += kSgThreads) {
            const int sl = i / 48, e = i - 48 * sl, p = s_pos[sl];
            if (p < 0)
                continue;
            if (e < 12)
                g.edge_pose[12 * (int64_t)p + e] = g.slot_pose[12 * (int64_t)(base + sl) + e];
            else
                g.edge_cov[36 * (int64_t)p + (e - 12)] = g.slot_cov[36 * (int64_t)(base + sl) + (e - 12)];
        }
        running += total;
        __syncthreads();   // s_wave / s_pos are rewritten by the next tile
    }
    if (tid == 0)
        *g.n_edges = running;
}

// Loop-closure edges, one workgroup: candidate c = (i, j) of the verified list, tile of 256 by
// tile.  The gates, the scale and S' = D S D are seq_graph_edges_kernel's with (k, k + d) = (i, j); then the loop variances go
// on the diagonal and the Cholesky test runs on that final matrix.  The accepted candidates are appended behind the *n_built
// edges of the graph in candidate order (the integer scan of seq_graph_compact_kernel) and *n_edges = *n_built + accepted.
__global__ __launch_bounds__(kSgThreads) void loop_edges_kernel(SeqGraphDev g, LoopEdgeDev e)
{
    __shared__ int s_wave[kSgThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_cand = min(e.counts[0], e.max_candidates);
    int running = *e.n_built;
    for (int base = 0; base < n_cand; base += kSgThreads) {
        const int c = base + tid;
        int keep = 0, ci = 0, cj = 0;
        double s = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
        if (c < n_cand) {
            ci = e.cand[c].i, cj = e.cand[c].j;
            const mvs_pair_result &pr = e.results[c];
            const mvs_refine_result &rr = e.refined[c];
            if (pr.valid && rr.ok && pr.n_points >= e.min_points && rr.error <= e.max_error) {
                const double *Ri = g.traj_R + 9 * (int64_t)ci, *ti = g.traj_t + 3 * (int64_t)ci, *tj = g.traj_t + 3 * (int64_t)cj;
                const double d0 = tj[0] - ti[0], d1 = tj[1] - ti[1], d2 = tj[2] - ti[2];
                double q[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    q[k] = (Ri[k] * d0 + Ri[3 + k] * d1) + Ri[6 + k] * d2;
                t0 = rr.t[0], t1 = rr.t[1], t2 = rr.t[2];
                s = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) / sqrt((t0 * t0 + t1 * t1) + t2 * t2);
                if (s > 0.0 && s < __builtin_inf()) {
                    double S[21];
#pragma unroll
                    for (int r = 0; r < 6; ++r)
#pragma unroll
                        for (int cc = 0; cc <= r; ++cc) {
                            double v = ((r < 3 ? 1.0 : s) * rr.pose_cov[6 * r + cc]) * (cc < 3 ? 1.0 : s);
                            if (r == cc && e.add[r / 3])
                                v = v + e.var[r / 3];
                            S[lidx(r, cc)] = v;
                        }
                    keep = chol_packed<6>(S) ? 1 : 0;
                }
            }
        }
        const unsigned long long bal = __ballot(keep != 0);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0)
            s_wave[wave] = __popcll(bal);
        __syncthreads();
        int pos = running + before, total = 0;
#pragma unroll
        for (int w = 0; w < kSgThreads / 64; ++w) {
            pos += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (c < n_cand)
            e.cand[c].accepted = keep;
        if (keep) {
            const mvs_refine_result &rr = e.refined[c];
            g.edge_src[pos] = ci;
            g.edge_dst[pos] = cj;
            g.edge_lag[pos] = cj - ci;
            g.edge_kind[pos] = 2;
            g.edge_scale[pos] = s;
            double *Zo = g.edge_pose + 12 * (int64_t)pos, *Co = g.edge_cov + 36 * (int64_t)pos;
#pragma unroll
            for (int k = 0; k < 9; ++k)
                Zo[k] = rr.R[k];
            Zo[9] = s * t0;
            Zo[10] = s * t1;
            Zo[11] = s * t2;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int cc = 0; cc < 6; ++cc) {
                    double v = ((r < 3 ? 1.0 : s) * rr.pose_cov[6 * r + cc]) * (cc < 3 ? 1.0 : s);
                    if (r == cc && e.add[r / 3])
                        v = v + e.var[r / 3];
                    Co[6 * r + cc] = v;
                }
        }
        running += total;
        __syncthreads();   // s_wave is rewritten by the next tile
    }
    if (tid == 0)
        *g.n_edges = running;
}

}  // namespace

void launch_loop_edges(const SeqGraphDev &g, const LoopEdgeDev &e, hipStream_t stream)
{
    hipLaunchKernelGGL(loop_edges_kernel, dim3(1), dim3(kSgThreads), 0, stream, g, e);
}

void launch_seq_graph(const SeqGraphDev &g, hipStream_t stream)
{
    const int n = g.n_slots > g.n_frames ? g.n_slots : g.n_frames;
    hipLaunchKernelGGL(seq_graph_edges_kernel, dim3((n + kSgThreads - 1) / kSgThreads), dim3(kSgThreads), 0, stream, g);
    hipLaunchKernelGGL(seq_graph_compact_kernel, dim3(1), dim3(kSgThreads), 0, stream, g);
}

}  // namespace mvs
