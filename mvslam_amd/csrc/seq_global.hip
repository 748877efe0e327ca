// seq_global.hip -- the global bundle adjustment of a resident sequence, assembled on the device (mvs_seq_refine_global;
// DESIGN.md section 4.7.5).  seq_link_kernel's tables (pnp.hip) are the tracks; here they become one sparse problem in the
// layout ba_sparse.hip reads, and every list of mvs_bas::plan (ba_envelope.hpp) is built from it:
//   seq_glob_depth_kernel     one lane per keypoint: the links behind it (a back-walk of at most n_frames steps).
//   seq_glob_count_kernel     one workgroup per frame: flags the heads that are points, gives them in-frame ranks and in-frame
//                             observation offsets by workgroup prefix sums with a running base over the chunks of 256
//                             keypoints; the frame's points, observations, sum of t (t - 1) / 2 and the last frame it reaches.
//   seq_glob_scan_kernel      ONE workgroup: exclusive scans of both counts over the frames, the 64-bit pair total.
//   seq_glob_envelope_kernel  ONE workgroup: first / last / row_off of the skyline from the frames' reach, blocks, widest row.
//   (the host reads SeqGlobState here, once)
//   seq_glob_emit_kernel      one lane per head: walks its track once and writes the point and its observations.
//   seq_glob_frames_kernel    poses and prior weights of the frames.
//   seq_glob_sort_kernel      one workgroup per frame: the frame's observations in ascending index (bitonic sort in LDS).
//   seq_glob_offsets_kernel   ONE workgroup: an exclusive scan of n_frames counts (fr_off; the rows' pair bases).
//   seq_glob_gather_kernel    fr_obs from the sorted lists.
//   seq_glob_rows_kernel      one workgroup per row of the envelope: blk_row and the pair count of every block, scanned in the row.
//   seq_glob_pairs_kernel     one workgroup per row: pair_off, pair_a, pair_c.
// Tracks have no gaps, which is what makes this cheap: frame i's list, being in point order, is in head-frame order, so the
// pairs of block (i, j) are a PREFIX of it -- the observations whose point starts at or before frame j.
// No floating-point atomics; the only atomics are a minimum and a maximum on integers in LDS (the envelope), which do not
// depend on the order of arrival.  No atomic decides an index: the same input gives the same bytes.
#include <climits>

#include "kernels.hpp"

namespace mvs {

namespace {

constexpr int kGlobMaxFrames = 4096;   // mvs_bas::kMaxFrames

// inclusive prefix sum over a wavefront
__device__ __forceinline__ int wave_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int n = __shfl_up(v, d);
        if (lane >= d)
            v += n;
    }
    return v;
}

// exclusive prefix sum of v over the 256 threads of a workgroup, `tot` their sum; s_w: 4 ints of LDS.  Every thread calls it.
__device__ __forceinline__ int block_scan(int v, int *s_w, int &tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_scan(v, lane);
    if (lane == 63)
        s_w[wave] = inc;
    __syncthreads();
    int off = 0;
    tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = s_w[k];
        off += (k < wave) ? x : 0;
        tot += x;
    }
    __syncthreads();
    return off + inc - v;
}

// out[k] = in[0] + .. + in[k - 1] for k < n, by one workgroup in chunks of 256 with a running base; returns the total
__device__ __forceinline__ int scan_array(const int32_t *in, int32_t *out, int n, int *s_w)
{
    int base = 0;
    for (int start = 0; start < n; start += 256) {
        const int k = start + (int)threadIdx.x;
        const int v = k < n ? in[k] : 0;
        int tot;
        const int ex = block_scan(v, s_w, tot);
        if (k < n)
            out[k] = base + ex;
        base += tot;
    }
    return base;
}

// What a head (frame j, keypoint i) finds along its track: the frames it covers and its first triangulated link.  visit(s, kp)
// is called for every frame j + s of the track with the track's keypoint there.  The walk takes at most max_frames - 1 links
// and never leaves the sequence; every index read from a table is range-checked as seq_link_kernel checks the match rows.
struct Track {
    int len;           // frames
    int tri_k, tri_j;  // the first triangulated link: pair, point of the pair; tri_k = -1: none
};
template <typename Visit>
__device__ __forceinline__ Track walk_track(const SeqWinDev &w, int j, int i, int max_frames, Visit visit)
{
    const int N = w.max_kp;
    Track t{1, -1, 0};
    int cur = i;
    visit(0, cur);
    for (int f = j; t.len < max_frames && f < w.n_frames - 1; ++f) {
        const size_t of = (size_t)f * N;
        const int r = w.succ[of + cur];
        if ((unsigned)r >= (unsigned)N)
            break;
        const int q = w.matches[of + r].queryIdx;
        if ((unsigned)q >= (unsigned)N)
            break;
        const int pt = w.row_to_point[of + r];
        if (t.tri_k < 0 && (unsigned)pt < (unsigned)N) {
            t.tri_k = f;
            t.tri_j = pt;
        }
        cur = q;
        visit(t.len, cur);
        ++t.len;
    }
    return t;
}

__device__ __forceinline__ int track_cap(const SeqGlobDev &d) { return d.T > 0 ? d.T : d.w.n_frames; }

// grid (ceil(N / 256), n_frames), block 256
__global__ __launch_bounds__(256) void seq_glob_depth_kernel(SeqGlobDev d)
{
    const int N = d.w.max_kp, f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N)
        return;
    int depth = 0, cur = i;
    for (int g = f; g > 0 && depth < d.w.n_frames; --g) {
        const int p = d.w.pred[(size_t)g * N + cur];
        if ((unsigned)p >= (unsigned)N)
            break;
        cur = p;
        ++depth;
    }
    d.depth[(size_t)f * N + i] = depth;
}

// grid n_frames, block 256
__global__ __launch_bounds__(256) void seq_glob_count_kernel(SeqGlobDev d)
{
    __shared__ int s_w[4];
    __shared__ long long s_pairs[256];
    __shared__ int s_reach[256];
    const int N = d.w.max_kp, j = blockIdx.x, tid = threadIdx.x;
    const size_t o = (size_t)j * N;
    const int cap = track_cap(d);
    int base_p = 0, base_o = 0, reach = j;
    long long pairs = 0;
    for (int start = 0; start < N; start += 256) {
        const int i = start + tid;
        int len = 0;
        if (i < N && j < d.w.n_frames - 1 && d.w.succ[o + i] >= 0) {
            const int dep = d.depth[o + i];
            if (d.T > 0 ? dep % d.T == 0 : dep == 0) {
                const Track t = walk_track(d.w, j, i, cap, [](int, int) {});
                if (t.tri_k >= 0 && t.len >= 2)
                    len = t.len;
            }
        }
        int tot_p, tot_o;
        const int rk = block_scan(len > 0 ? 1 : 0, s_w, tot_p);
        const int oo = block_scan(len, s_w, tot_o);
        if (i < N) {
            d.rank[o + i] = len > 0 ? base_p + rk : -1;
            d.oofs[o + i] = base_o + oo;
        }
        base_p += tot_p;
        base_o += tot_o;
        pairs += (long long)len * (len - 1) / 2;
        reach = max(reach, j + len - 1);
    }
    s_pairs[tid] = pairs;
    s_reach[tid] = reach;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            s_pairs[tid] += s_pairs[tid + h];
            s_reach[tid] = max(s_reach[tid], s_reach[tid + h]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        d.fr_points[j] = base_p;
        d.fr_nobs[j] = base_o;
        d.fr_pairs[j] = s_pairs[0];
        d.fr_reach[j] = s_reach[0];
    }
}

// grid 1, block 256
__global__ __launch_bounds__(256) void seq_glob_scan_kernel(SeqGlobDev d)
{
    __shared__ int s_w[4];
    __shared__ long long s_pairs[256];
    const int F = d.w.n_frames, tid = threadIdx.x;
    const int P = scan_array(d.fr_points, d.pt_base, F, s_w);
    const int O = scan_array(d.fr_nobs, d.ob_base, F, s_w);
    long long pairs = 0;
    for (int f = tid; f < F; f += 256)
        pairs += d.fr_pairs[f];
    s_pairs[tid] = pairs;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
            s_pairs[tid] += s_pairs[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        d.state->n_points = P;
        d.state->n_obs = O;
        d.state->pairs = s_pairs[0];
    }
}

// grid 1, block 256; n_frames <= kGlobMaxFrames.  A point that starts in frame j reaches fr_reach[j] at the most and tracks have
// no gaps, so first[i] = the smallest j < i with fr_reach[j] >= i (i itself if there is none); last[c] = the largest row whose
// envelope holds column c.
__global__ __launch_bounds__(256) void seq_glob_envelope_kernel(SeqGlobDev d)
{
    __shared__ int s_first[kGlobMaxFrames], s_last[kGlobMaxFrames], s_w[4], s_max[256];
    const int F = min(d.w.n_frames, kGlobMaxFrames), tid = threadIdx.x;
    for (int i = tid; i < F; i += 256)
        s_first[i] = s_last[i] = i;
    __syncthreads();
    for (int j = tid; j < F; j += 256) {
        const int reach = min(d.fr_reach[j], F - 1);
        for (int f = j + 1; f <= reach; ++f)
            atomicMin(&s_first[f], j);
    }
    __syncthreads();
    for (int i = tid; i < F; i += 256)
        for (int c = s_first[i]; c < i; ++c)
            atomicMax(&s_last[c], i);
    __syncthreads();
    int base = 0, widest = 0;
    for (int start = 0; start < F; start += 256) {
        const int i = start + tid;
        const int w = i < F ? i - s_first[i] + 1 : 0;
        int tot;
        const int ex = block_scan(w, s_w, tot);
        if (i < F) {
            d.first[i] = s_first[i];
            d.last[i] = s_last[i];
            d.row_off[i] = base + ex;
        }
        base += tot;
        widest = max(widest, w);
    }
    s_max[tid] = widest;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
            s_max[tid] = max(s_max[tid], s_max[tid + h]);
        __syncthreads();
    }
    if (tid == 0) {
        d.row_off[F] = base;
        d.state->blocks = base;
        d.state->widest = s_max[0];
        d.state->reserved = 0;
    }
}

// grid (ceil(N / 256), n_frames - 1), block 256.  The lane of a head that is a point walks the track once more and writes the
// point p = pt_base[j] + rank and its observations from ob_base[j] + oofs on.
__global__ __launch_bounds__(256) void seq_glob_emit_kernel(SeqGlobDev d)
{
    const int N = d.w.max_kp, j = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N)
        return;
    const size_t o = (size_t)j * N;
    const int rk = d.rank[o + i];
    if (rk < 0)
        return;
    const int p = d.pt_base[j] + rk, o0 = d.ob_base[j] + d.oofs[o + i];
    if (p >= d.n_points)
        return;
    const SeqWinDev &w = d.w;
    const Track t = walk_track(w, j, i, track_cap(d), [&](int s, int kp) {
        const int ob = o0 + s;
        if (ob >= d.n_obs)
            return;
        const size_t at = (size_t)(j + s) * N + kp;
        d.obs_frame[ob] = j + s;
        d.obs_point[ob] = p;
        d.obs_kp[ob] = kp;
        d.kp_obs[at] = ob;
        d.obs_uv[2 * (size_t)ob] = (double)w.kp[2 * at];
        d.obs_uv[2 * (size_t)ob + 1] = (double)w.kp[2 * at + 1];
        const int oc = min((int)w.oct[at], kSeqWinMaxOctave);
        d.oinfo[3 * (size_t)ob] = w.oinfo[oc][0];
        d.oinfo[3 * (size_t)ob + 1] = w.oinfo[oc][1];
        d.oinfo[3 * (size_t)ob + 2] = w.oinfo[oc][2];
    });
    d.obs_off[p] = o0;
    if (p == d.n_points - 1)
        d.obs_off[d.n_points] = o0 + t.len;
    d.head_frame[p] = j;
    d.head_kp[p] = i;
    // the first triangulated link gives the guess (seq_window_assemble_kernel's statements)
    const int tk = max(t.tri_k, 0);
    const double *x = w.points + 3 * ((size_t)tk * N + t.tri_j), *R = w.traj_R + 9 * (size_t)tk;
    const double *tt = w.traj_t + 3 * (size_t)tk, sg = w.traj_sigma[tk];
    const double s0 = sg * x[0], s1 = sg * x[1], s2 = sg * x[2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        d.pts0[3 * (size_t)p + k] = ((R[3 * k] * s0 + R[3 * k + 1] * s1) + R[3 * k + 2] * s2) + tt[k];
#pragma unroll
    for (int k = 0; k < 6; ++k)
        d.pinfo[6 * (size_t)p + k] = w.pinfo[k];
}

// grid ceil(18 n_frames / 256), block 256
__global__ __launch_bounds__(256) void seq_glob_frames_kernel(SeqGlobDev d)
{
    const int k = blockIdx.x * 256 + threadIdx.x, F = d.w.n_frames;
    if (k >= 18 * F)
        return;
    const int f = k / 18, e = k - 18 * f;
    if (e < 9)
        d.pose0[12 * (size_t)f + e] = d.w.traj_R[9 * (size_t)f + e];
    else if (e < 12)
        d.pose0[12 * (size_t)f + e] = d.w.traj_t[3 * (size_t)f + (e - 9)];
    else
        d.wts[6 * (size_t)f + (e - 12)] = f == 0 ? d.w.w_anchor[e - 12] : d.w.w_pose[e - 12];
}

// grid n_frames, block 256.  Frame i's observations (one per keypoint at the most) sorted ascending in LDS and written back
// over the frame's row of kp_obs; fr_cnt[i] = how many.
__global__ __launch_bounds__(256) void seq_glob_sort_kernel(SeqGlobDev d)
{
    __shared__ int s_v[kMaxKp], s_w[4];
    const int N = d.w.max_kp, i = blockIdx.x, tid = threadIdx.x;
    int32_t *row = d.kp_obs + (size_t)i * N;
    int n2 = 256;
    while (n2 < N)
        n2 <<= 1;
    int mine = 0;
    for (int k = tid; k < n2; k += 256) {
        const int v = k < N ? row[k] : -1;
        s_v[k] = v >= 0 ? v : INT_MAX;
        mine += v >= 0 ? 1 : 0;
    }
    int cnt;
    (void)block_scan(mine, s_w, cnt);
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int k = tid; k < (n2 >> 1); k += 256) {
                const int lo = 2 * k - (k & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const int a = s_v[lo], b = s_v[hi];
                if ((a > b) == up) {
                    s_v[lo] = b;
                    s_v[hi] = a;
                }
            }
        }
    __syncthreads();
    for (int k = tid; k < N; k += 256)
        row[k] = k < cnt ? s_v[k] : -1;
    if (tid == 0)
        d.fr_cnt[i] = cnt;
}

// grid 1, block 256: out[0 .. n] = the exclusive scan of in[0 .. n) and the total
__global__ __launch_bounds__(256) void seq_glob_offsets_kernel(const int32_t *in, int32_t *out, int n)
{
    __shared__ int s_w[4];
    const int tot = scan_array(in, out, n, s_w);
    if (threadIdx.x == 0)
        out[n] = tot;
}

// grid (ceil(N / 256), n_frames), block 256
__global__ __launch_bounds__(256) void seq_glob_gather_kernel(SeqGlobDev d)
{
    const int N = d.w.max_kp, i = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N || r >= d.fr_cnt[i])
        return;
    const int at = d.fr_off[i] + r;
    if (at < d.n_obs)
        d.fr_obs[at] = d.kp_obs[(size_t)i * N + r];
}

// grid n_frames, block 256.  Row i: block (i, j), first[i] <= j < i, sums over the observations of frame i whose point starts
// at or before frame j: a prefix of the frame's list, found by bisection on the head frames.  pair_rel = the exclusive scan of
// those counts inside the row (the diagonal block, which has no pairs, holds the row's total).
__global__ __launch_bounds__(256) void seq_glob_rows_kernel(SeqGlobDev d)
{
    __shared__ int s_w[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int f0 = d.first[i], r0 = d.row_off[i], width = i - f0 + 1;
    const int32_t *list = d.fr_obs + d.fr_off[i];
    const int n = d.fr_cnt[i];
    int base = 0;
    for (int start = 0; start < width; start += 256) {
        const int idx = start + tid;
        int c = 0;
        if (idx < width - 1) {
            const int j = f0 + idx;
            int lo = 0, hi = n;   // the first entry whose point starts behind frame j
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (d.head_frame[d.obs_point[list[mid]]] <= j)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            c = lo;
        }
        int tot;
        const int ex = block_scan(c, s_w, tot);
        if (idx < width && r0 + idx < d.n_blocks) {
            d.pair_rel[r0 + idx] = base + ex;
            d.blk_row[r0 + idx] = i;
        }
        base += tot;
    }
    if (tid == 0)
        d.row_pairs[i] = base;
}

// grid n_frames, block 256.  Row i: pair_off of its blocks and their pairs (a, c): a = the observation of frame i, c = the
// observation of frame j of the same point, which lies j - head_frame behind the point's first.
__global__ __launch_bounds__(256) void seq_glob_pairs_kernel(SeqGlobDev d)
{
    const int i = blockIdx.x, tid = threadIdx.x;
    const int f0 = d.first[i], r0 = d.row_off[i], width = i - f0 + 1, rb = d.row_base[i];
    const int32_t *list = d.fr_obs + d.fr_off[i];
    for (int idx = tid; idx < width; idx += 256)
        if (r0 + idx < d.n_blocks)
            d.pair_off[r0 + idx] = rb + d.pair_rel[r0 + idx];
    if (i == d.w.n_frames - 1 && tid == 0)
        d.pair_off[d.n_blocks] = rb + d.row_pairs[i];
    for (int idx = 0; idx < width - 1; ++idx) {
        const int b = r0 + idx;
        if (b + 1 >= d.n_blocks)
            break;
        const int rel = d.pair_rel[b], cnt = d.pair_rel[b + 1] - rel, j = f0 + idx;
        const int64_t off = (int64_t)rb + rel;
        for (int r = tid; r < cnt; r += 256) {
            if (off + r >= d.n_pairs)
                break;
            const int a = list[r], p = d.obs_point[a];
            d.pair_a[off + r] = a;
            d.pair_c[off + r] = d.obs_off[p] + (j - d.head_frame[p]);
        }
    }
}

}  // namespace

void launch_seq_glob_count(const SeqGlobDev &d, hipStream_t stream)
{
    const int F = d.w.n_frames, gx = (d.w.max_kp + 255) / 256;
    launch_seq_link(d.w, stream);
    hipLaunchKernelGGL(seq_glob_depth_kernel, dim3(gx, F), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_glob_count_kernel, dim3(F), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_glob_scan_kernel, dim3(1), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_glob_envelope_kernel, dim3(1), dim3(256), 0, stream, d);
}

void launch_seq_glob_build(const SeqGlobDev &d, hipStream_t stream)
{
    const int F = d.w.n_frames, gx = (d.w.max_kp + 255) / 256;
    hipLaunchKernelGGL(seq_glob_emit_kernel, dim3(gx, F - 1), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_glob_frames_kernel, dim3((18 * F + 255) / 256), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_glob_sort_kernel, dim3(F), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_glob_offsets_kernel, dim3(1), dim3(256), 0, stream, d.fr_cnt, d.fr_off, F);
    hipLaunchKernelGGL(seq_glob_gather_kernel, dim3(gx, F), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_glob_rows_kernel, dim3(F), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(seq_glob_offsets_kernel, dim3(1), dim3(256), 0, stream, d.row_pairs, d.row_base, F);
    hipLaunchKernelGGL(seq_glob_pairs_kernel, dim3(F), dim3(256), 0, stream, d);
}

}  // namespace mvs
