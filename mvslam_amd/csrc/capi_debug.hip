// capi_debug.hip -- the mvs_debug_* hooks.  Compiled with -DMVS_DEBUG_HOOKS into libmvslam_hip_dbg.so only.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.hpp"

using namespace mvs_host;

// generic "n inputs -> m outputs" staging for the two probes below
template <typename Launch>
static int probe_io(mvs_ctx *ctx, const void *const *in, const size_t *in_bytes, int n_in, void *const *outp, const size_t *out_bytes,
                    int n_out, Launch launch)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned char *d[8] = {};
    DevBlocks tmp;
    DevGroup g(ctx, tmp);
    for (int k = 0; k < n_in + n_out; ++k)
        g.add(d[k], k < n_in ? in_bytes[k] : out_bytes[k - n_in]);
    const mvs_status st = g.commit();
    if (st != MVS_OK)
        return st;
    hipError_t e = hipSuccess;
    for (int k = 0; k < n_in && e == hipSuccess; ++k)
        e = hipMemcpy(d[k], in[k], in_bytes[k], hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch(d);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = sync_stream(ctx);
    for (int k = 0; k < n_out && e == hipSuccess; ++k)
        e = hipMemcpy(outp[k], d[n_in + k], out_bytes[k], hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        ctx->err = std::string("probe: ") + hipGetErrorString(e);
        return MVS_ERR_HIP;
    }
    return MVS_OK;
}

extern "C" {

// Diagnostics, compiled ONLY into libmvslam_hip_dbg.so (make dbg; tests/ and tools/ load that library explicitly).  The
// product library has neither symbol: a process-global kernel-variant switch is not something a caller of the
// reference's interface should be able to reach.
// diagnostics only (not in the public header): bitwise comparison of the unscaled sqrt / div device sequences with
// the compiler's IEEE ones on host-supplied operands.  counts[4] = {sqrt mismatches, div mismatches, sqrt checked,
// div checked}
int mvs_debug_fastmath_check(mvs_ctx *ctx, const double *x, const double *y, int n, unsigned long long counts[4])
{
    if (!ctx || n < 1)
        return MVS_ERR_INVALID_ARG;
    double *dx = nullptr, *dy = nullptr;
    unsigned long long *dc = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBlocks tmp;
    const mvs_status st = DevGroup(ctx, tmp).add(dx, n).add(dy, n).add(dc, 4).commit();
    if (st != MVS_OK)
        return st;
    HIP_TRY(ctx, hipMemcpyAsync(dx, x, (size_t)n * 8, hipMemcpyHostToDevice, ctx_stream(ctx)));
    HIP_TRY(ctx, hipMemcpyAsync(dy, y, (size_t)n * 8, hipMemcpyHostToDevice, ctx_stream(ctx)));
    HIP_TRY(ctx, hipMemsetAsync(dc, 0, 32, ctx_stream(ctx)));
    launch_fastmath_check(dx, dy, n, dc, ctx_stream(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(counts, dc, 32, hipMemcpyDeviceToHost, ctx_stream(ctx)));
    HIP_TRY(ctx, sync_stream(ctx));
    return MVS_OK;
}

// diagnostics only: one guarded Jacobi pair step per row pair against the IEEE one (pairstep_check_kernel).
// rows: n x 6 doubles.  counts[4] = {steps that differ, steps compared, decisions that differ, bits of the largest
// |1 - gamma * 2 h| seen (accuracy of the reciprocal estimate the seeded divisions start from)}
int mvs_debug_pairstep_check(mvs_ctx *ctx, const double *rows, int n, unsigned long long counts[4])
{
    if (!ctx || n < 1)
        return MVS_ERR_INVALID_ARG;
    double *dr = nullptr;
    unsigned long long *dc = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBlocks tmp;
    const mvs_status st = DevGroup(ctx, tmp).add(dr, (size_t)n * 6).add(dc, 4).commit();
    if (st != MVS_OK)
        return st;
    hipError_t e = hipMemcpyAsync(dr, rows, (size_t)n * 48, hipMemcpyHostToDevice, ctx_stream(ctx));
    if (e == hipSuccess)
        e = hipMemsetAsync(dc, 0, 32, ctx_stream(ctx));
    if (e == hipSuccess) {
        launch_pairstep_check(dr, n, dc, ctx_stream(ctx));
        e = hipMemcpyAsync(counts, dc, 32, hipMemcpyDeviceToHost, ctx_stream(ctx));
    }
    if (e == hipSuccess)
        e = sync_stream(ctx);
    return e == hipSuccess ? MVS_OK : MVS_ERR_HIP;
}

// diagnostics only (not in the public header): the counting variant of the pre-screened stage (kernels.hpp: set_count_dense)
int mvs_debug_set_count_dense(int v)
{
    set_count_dense(v);
    return MVS_OK;
}

// one 32 x 32 x 32 bf16 tile through the counting kernels' two MFMAs: a, b = [32][32] bf16 bit patterns on the host,
// out = [32][32] binary32 (point x hypothesis)
int mvs_debug_mfma_probe(mvs_ctx *ctx, const uint16_t *a, const uint16_t *b, float *out)
{
    if (!ctx || !a || !b || !out)
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint16_t *da = nullptr, *db = nullptr;
    float *dout = nullptr;
    DevBlocks tmp;
    const mvs_status st = DevGroup(ctx, tmp).add(da, 1024).add(db, 1024).add(dout, 1024).commit();
    if (st != MVS_OK)
        return st;
    HIP_TRY(ctx, hipMemcpy(da, a, 1024 * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(db, b, 1024 * sizeof(uint16_t), hipMemcpyHostToDevice));
    launch_mfma_probe(da, db, dout, ctx_stream(ctx));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, sync_stream(ctx));
    HIP_TRY(ctx, hipMemcpy(out, dout, 1024 * sizeof(float), hipMemcpyDeviceToHost));
    return MVS_OK;
}

int mvs_debug_set_split_min_pairs(int v)
{
    set_split_min_pairs(v);
    return MVS_OK;
}

int mvs_debug_set_match_mfma(int v)
{
    set_match_mfma(v);
    return MVS_OK;
}

int mvs_debug_set_prescreen_force(int m)
{
    set_prescreen_force(m);
    return MVS_OK;
}

// wavefronts of pair_prepare / ransac_prescreen that left the relaxed normalisation for the guarded one (its range test
// fired) since the last reset; the caller has synchronised the launches it asks about.  reset != 0: zero afterwards
int mvs_debug_prescreen_fallback_waves(mvs_ctx *ctx, int reset, unsigned int *out)
{
    if (!ctx || !out)
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, prescreen_fallback_waves(out, reset != 0));
    return MVS_OK;
}

// records of the RANSAC stage as the last run left them: rec_out n_hyp x 10 (F, counting threshold), state bytes, counts;
// info[0..3] = {mode of the pair, bound of the pair, work-list entries 0, work-list entries 1}
int mvs_debug_read_hyp_rec(mvs_batch *b, int pair, int n_hyp, double *rec_out, unsigned char *state_out, int32_t *cnt_out,
                           int32_t *info)
{
    if (!b || !b->d.hyp_F || pair < 0 || pair >= b->d.n_pairs || n_hyp < 1 || n_hyp > b->d.max_groups * kHypPerBlock)
        return MVS_ERR_INVALID_ARG;
    const size_t Hp = (size_t)b->d.max_groups * kHypPerBlock;
    HIP_TRY(b->ctx, sync_stream(b->ctx));
    std::vector<unsigned char> stv(n_hyp);
    HIP_TRY(b->ctx, hipMemcpy(stv.data(), b->d.hyp_okf + (size_t)pair * Hp, (size_t)n_hyp, hipMemcpyDeviceToHost));
    if (rec_out) {
        HIP_TRY(b->ctx, hipMemcpy(rec_out, b->d.hyp_F + (size_t)pair * Hp * kHypRec, (size_t)n_hyp * kHypRec * sizeof(double),
                                  hipMemcpyDeviceToHost));
        // a pair in mode 1 keeps its APPROXIMATE records in the 48-byte single-precision array: they are returned in the
        // first 48 bytes of the hypothesis' 80-byte slot (the layout the records had when they shared one array)
        int32_t pmode = 0;
        HIP_TRY(b->ctx, hipMemcpy(&pmode, b->d.mode + pair, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (pmode == 1) {
            std::vector<float> r32((size_t)n_hyp * kHypRec32);
            HIP_TRY(b->ctx, hipMemcpy(r32.data(), b->d.hyp_r32 + (size_t)pair * Hp * kHypRec32, r32.size() * sizeof(float),
                                      hipMemcpyDeviceToHost));
            for (int h = 0; h < n_hyp; ++h)
                if (stv[h] == 1)
                    std::memcpy(rec_out + (size_t)h * kHypRec, r32.data() + (size_t)h * kHypRec32, kHypRec32 * sizeof(float));
        }
    }
    if (state_out)
        std::memcpy(state_out, stv.data(), (size_t)n_hyp);
    if (cnt_out)
        HIP_TRY(b->ctx, hipMemcpy(cnt_out, b->d.hyp_cnt + (size_t)pair * Hp, (size_t)n_hyp * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (info) {
        uint32_t xc[2] = {0, 0};
        HIP_TRY(b->ctx, hipMemcpy(&info[0], b->d.mode + pair, sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(b->ctx, hipMemcpy(&info[1], b->d.bound + pair, sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(b->ctx, hipMemcpy(xc, b->d.xcount, sizeof(xc), hipMemcpyDeviceToHost));
        info[2] = (int32_t)xc[0];
        info[3] = (int32_t)xc[1];
    }
    return MVS_OK;
}

// the pre-screen alone over pairs [0, n_active) of a batch that has been run (matches and points resident): pair_prepare +
// ransac_prescreen, every pair forced into pre-screened mode `mode` (1: single-precision records, 2: double precision),
// nothing solved exactly afterwards -- the records then hold F~ and the widened thresholds (state 1), or wait for the exact
// solve (state 2): tests compare them with the oracle's exact F
int mvs_debug_prescreen_only(mvs_batch *b, const mvs_params *params, int n_active, int mode)
{
    if (!b || !params || n_active < 1 || n_active > b->d.n_pairs || (mode != 1 && mode != 2))
        return MVS_ERR_INVALID_ARG;
    mvs_status st = ensure_groups(b, params->num_hypotheses);
    if (st != MVS_OK)
        return st;
    launch_prescreen_only(b->d, to_run(*params), n_active, mode, ctx_stream(b->ctx));
    HIP_TRY(b->ctx, hipGetLastError());
    HIP_TRY(b->ctx, sync_stream(b->ctx));
    return MVS_OK;
}

// full-population audit (kernels.hip: audit_kernel).  phase 0: pair_prepare + ransac_prescreen run here (the probe decides every
// pair's mode), then every record is checked against the exact solve of its sample; phase 1: the caller has just run the
// batch with the same parameters, the stage's decisions are checked.  counters[16] as documented at audit_kernel; maxc /
// bound / mode: [n_active] (largest exact count, the stage's bound, the pair's mode), each may be null.
int mvs_debug_audit(mvs_batch *b, const mvs_params *params, int n_active, int phase, unsigned long long counters[16],
                    int32_t *maxc, int32_t *bound, int32_t *mode)
{
    if (!b || !params || !counters || n_active < 1 || n_active > b->d.n_pairs || (phase != 0 && phase != 1))
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mvs_status st = ensure_groups(b, params->num_hypotheses);
    if (st != MVS_OK)
        return st;
    const RunParams rp = to_run(*params);
    unsigned long long *dc = nullptr;
    int32_t *dm = nullptr;
    DevBlocks tmp;
    if ((st = DevGroup(ctx, tmp).add(dc, 16).add(dm, n_active).commit()) != MVS_OK)
        return st;
    hipError_t e = hipMemsetAsync(dc, 0, 16 * sizeof(unsigned long long), ctx_stream(ctx));
    if (e == hipSuccess)
        e = hipMemsetAsync(dm, 0xff, (size_t)n_active * sizeof(int32_t), ctx_stream(ctx));
    if (e == hipSuccess && phase == 0)
        launch_prescreen_only(b->d, rp, n_active, -1, ctx_stream(ctx));
    if (e == hipSuccess)
        e = launch_audit(b->d, rp, n_active, phase, dc, dm, ctx_stream(ctx));
    if (e == hipSuccess)
        e = sync_stream(ctx);
    if (e == hipSuccess)
        e = hipMemcpy(counters, dc, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess && maxc)
        e = hipMemcpy(maxc, dm, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && bound)
        e = hipMemcpy(bound, b->d.bound, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mode)
        e = hipMemcpy(mode, b->d.mode, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        ctx->err = std::string("mvs_debug_audit: ") + hipGetErrorString(e);
        return MVS_ERR_HIP;
    }
    return MVS_OK;
}

// The same audit over the device state of ANOTHER library instance's batch (mvs_batch_device_state of libmvslam_hip.so, loaded
// in the same process): the product binary ran the stage, this library only replays every hypothesis exactly and compares.
// phase 1: the stage's decisions; phase 2: the records as the product's pre-screen wrote them and the stage left them (every
// record still in state kPsApprox: (B) on every match, U >= c_J >= L) -- phase 0's checks WITHOUT re-running the pre-screen.
int mvs_debug_audit_state(mvs_ctx *ctx, const void *state, size_t state_bytes, const mvs_params *params, int n_active, int phase,
                          unsigned long long counters[16], int32_t *maxc, int32_t *bound, int32_t *mode)
{
    struct Blob {
        uint64_t bytes, abi;
        BatchDev d;
    };
    if (!ctx || !state || !params || !counters || (phase != 1 && phase != 2))
        return MVS_ERR_INVALID_ARG;
    Blob blob;
    if (state_bytes != sizeof(Blob))
        return MVS_ERR_INVALID_ARG;
    std::memcpy(&blob, state, sizeof(Blob));
    if (blob.bytes != sizeof(Blob) || blob.abi != (uint64_t)MVS_ABI_VERSION)
        return MVS_ERR_INVALID_ARG;   // not the same build
    const BatchDev &d = blob.d;
    if (n_active < 1 || n_active > d.n_pairs || (params->num_hypotheses + kHypPerBlock - 1) / kHypPerBlock > d.max_groups)
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const RunParams rp = to_run(*params);
    unsigned long long *dc = nullptr;
    int32_t *dm = nullptr;
    DevBlocks tmp;
    const mvs_status st = DevGroup(ctx, tmp).add(dc, 16).add(dm, n_active).commit();
    if (st != MVS_OK)
        return st;
    hipError_t e = hipMemsetAsync(dc, 0, 16 * sizeof(unsigned long long), ctx_stream(ctx));
    if (e == hipSuccess)
        e = hipMemsetAsync(dm, 0xff, (size_t)n_active * sizeof(int32_t), ctx_stream(ctx));
    if (e == hipSuccess)
        e = launch_audit(d, rp, n_active, phase == 2 ? 0 : 1, dc, dm, ctx_stream(ctx));
    if (e == hipSuccess)
        e = sync_stream(ctx);
    if (e == hipSuccess)
        e = hipMemcpy(counters, dc, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess && maxc)
        e = hipMemcpy(maxc, dm, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && bound)
        e = hipMemcpy(bound, d.bound, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mode)
        e = hipMemcpy(mode, d.mode, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        ctx->err = std::string("mvs_debug_audit_state: ") + hipGetErrorString(e);
        return MVS_ERR_HIP;
    }
    return MVS_OK;
}

// overwrite the ideal-camera points of one pair: pts4 = m x (x1, y1, x2, y2) doubles (the matcher's output is bypassed)
int mvs_debug_set_points(mvs_batch *b, int pair, int m, const double *pts4)
{
    if (!b || !pts4 || pair < 0 || pair >= b->d.n_pairs || m < 0 || m > b->d.max_kp)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sync_stream(ctx));
    HIP_TRY(ctx, hipMemcpy(b->d.pts + (size_t)pair * b->d.max_kp * 4, pts4, (size_t)m * 4 * sizeof(double), hipMemcpyHostToDevice));
    const int32_t mm = m;
    HIP_TRY(ctx, hipMemcpy(b->d.M + pair, &mm, sizeof(mm), hipMemcpyHostToDevice));
    return MVS_OK;
}

// read the ideal-camera points of one pair as the kernels see them: pts4 = capacity x 4 doubles, *m = the pair's match count
int mvs_debug_get_points(mvs_batch *b, int pair, int *m, double *pts4)
{
    if (!b || !pts4 || !m || pair < 0 || pair >= b->d.n_pairs)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sync_stream(ctx));
    int32_t mm = 0;
    HIP_TRY(ctx, hipMemcpy(&mm, b->d.M + pair, sizeof(mm), hipMemcpyDeviceToHost));
    mm = std::min(mm, b->d.max_kp);
    HIP_TRY(ctx, hipMemcpy(pts4, b->d.pts + (size_t)pair * b->d.max_kp * 4, (size_t)mm * 4 * sizeof(double), hipMemcpyDeviceToHost));
    *m = mm;
    return MVS_OK;
}

// pre-screen (every pair forced into mode pmode: 1 single-, 2 double-precision records) + the counting launches alone, with
// only hypothesis keep[p] of pair p left valid (keep may be null).  dense: 0 = ransac_count32 in one launch, 1 = the product's
// pilot + matrix-core dense phase + finish.  Out, each [n_active] and optional: the kept hypothesis' recorded count (U), the
// pair's bound (best lower bound), the points the dense phase covered.
int mvs_debug_count_only(mvs_batch *b, const mvs_params *params, int n_active, int pmode, int dense, const int32_t *keep,
                         int32_t *cnt_out, int32_t *bound_out, int32_t *n1_out)
{
    if (!b || !params || n_active < 1 || n_active > b->d.n_pairs || (pmode != 1 && pmode != 2) || dense < 0 || dense > 2)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mvs_status st = ensure_groups(b, params->num_hypotheses);
    if (st != MVS_OK)
        return st;
    const size_t Hp = (size_t)b->d.max_groups * kHypPerBlock;
    int32_t *dk = nullptr;
    DevBlocks tmp;
    if (keep) {
        for (int p = 0; p < n_active; ++p)
            if (keep[p] >= (int32_t)Hp)
                return MVS_ERR_INVALID_ARG;
        if ((st = DevGroup(ctx, tmp).add(dk, n_active).commit()) != MVS_OK)
            return st;
        HIP_TRY(ctx, hipMemcpy(dk, keep, (size_t)n_active * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx, hipMemsetAsync(b->d.dense_n1, 0, (size_t)n_active * sizeof(int32_t), ctx_stream(ctx)));
    launch_count_only(b->d, to_run(*params), n_active, pmode, dense, dk, ctx_stream(ctx));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = sync_stream(ctx);
    for (int p = 0; p < n_active && e == hipSuccess; ++p) {
        if (cnt_out && keep && keep[p] >= 0)
            e = hipMemcpy(cnt_out + p, b->d.hyp_cnt + (size_t)p * Hp + keep[p], sizeof(int32_t), hipMemcpyDeviceToHost);
    }
    if (e == hipSuccess && bound_out)
        e = hipMemcpy(bound_out, b->d.bound, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && n1_out)
        e = hipMemcpy(n1_out, b->d.dense_n1, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        ctx->err = std::string("mvs_debug_count_only: ") + hipGetErrorString(e);
        return MVS_ERR_HIP;
    }
    return MVS_OK;
}

// the matrix-core counting's compare-free indicator on caller-supplied accumulator values (kernels.hip: indicator_probe_kernel)
int mvs_debug_indicator_probe(mvs_ctx *ctx, const float *a, const float *tu, const float *tl, const float *T, int n, float *ind_u,
                              float *ind_l, float *scale)
{
    if (!ctx || !a || !tu || !tl || !T || !ind_u || !ind_l || !scale || n < 1)
        return MVS_ERR_INVALID_ARG;
    const size_t nb = (size_t)n * sizeof(float);
    const void *in[4] = {a, tu, tl, T};
    const size_t ib[4] = {nb, nb, nb, nb};
    void *out[3] = {ind_u, ind_l, scale};
    const size_t ob[3] = {nb, nb, nb};
    return probe_io(ctx, in, ib, 4, out, ob, 3, [&](unsigned char **d) {
        launch_indicator_probe((const float *)d[0], (const float *)d[1], (const float *)d[2], (const float *)d[3], n, (float *)d[4],
                               (float *)d[5], (float *)d[6], ctx_stream(ctx));
    });
}

// de-normalisation + fused residual of both paths on caller-supplied (Fn, transforms, point) tuples: in n x 19, out n x 2
int mvs_debug_rounding_probe(mvs_ctx *ctx, const double *in19, int n, double *out2)
{
    if (!ctx || !in19 || !out2 || n < 1)
        return MVS_ERR_INVALID_ARG;
    const void *in[1] = {in19};
    const size_t ib[1] = {(size_t)n * 19 * sizeof(double)};
    void *out[1] = {out2};
    const size_t ob[1] = {(size_t)n * 2 * sizeof(double)};
    return probe_io(ctx, in, ib, 1, out, ob, 1,
                    [&](unsigned char **d) { launch_rounding_probe((const double *)d[0], n, (double *)d[1], ctx_stream(ctx)); });
}

// the plan lists the device built for the last mvs_seq_refine_global (seq_global.hip), to be compared with mvs_bas::plan on the
// downloaded CSR.  counts[6] = {frames, points, observations, blocks, pairs, widest row}; every list may be NULL: first[F],
// row_off[F + 1], blk_row[blocks], last[F], obs_point[O], fr_off[F + 1], fr_obs[O], pair_off[blocks + 1], pair_a / pair_c[pairs]
int mvs_debug_seq_global_plan(mvs_seq *q, int64_t *counts, int32_t *first, int32_t *row_off, int32_t *blk_row, int32_t *last,
                              int32_t *obs_point, int32_t *fr_off, int32_t *fr_obs, int32_t *pair_off, int32_t *pair_a,
                              int32_t *pair_c)
{
    if (!q || !q->glob_built)
        return MVS_ERR_INVALID_ARG;
    mvs_ctx *ctx = q->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sync_stream(ctx));
    const SeqGlobDev &g = q->gl;
    const size_t F = (size_t)g.w.n_frames, O = (size_t)g.n_obs, B = (size_t)g.n_blocks, NP = (size_t)g.n_pairs, I = sizeof(int32_t);
    if (counts) {
        SeqGlobState hs{};
        HIP_TRY(ctx, hipMemcpy(&hs, g.state, sizeof(hs), hipMemcpyDeviceToHost));
        counts[0] = (int64_t)F, counts[1] = hs.n_points, counts[2] = hs.n_obs, counts[3] = hs.blocks, counts[4] = hs.pairs;
        counts[5] = hs.widest;
    }
    auto get = [&](void *dst, const void *src, size_t bytes) {
        return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIP_TRY(ctx, get(first, g.first, F * I));
    HIP_TRY(ctx, get(row_off, g.row_off, (F + 1) * I));
    HIP_TRY(ctx, get(blk_row, g.blk_row, B * I));
    HIP_TRY(ctx, get(last, g.last, F * I));
    HIP_TRY(ctx, get(obs_point, g.obs_point, O * I));
    HIP_TRY(ctx, get(fr_off, g.fr_off, (F + 1) * I));
    HIP_TRY(ctx, get(fr_obs, g.fr_obs, O * I));
    HIP_TRY(ctx, get(pair_off, g.pair_off, (B + 1) * I));
    HIP_TRY(ctx, get(pair_a, g.pair_a, NP * I));
    HIP_TRY(ctx, get(pair_c, g.pair_c, NP * I));
    return MVS_OK;
}
}  // extern "C"
