// capi_orb.hip -- host side of libmvslam_hip.so: ORB extraction (pattern, pyramid layout, the captured launch graph).
// The one capi file with an #ifdef MVS_DEBUG_HOOKS (two getenv A/B switches): the diagnostics library recompiles it.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "capi_internal.hpp"

using namespace mvs_host;

static void philox_host(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t out[4])
{   // Philox4x32-10 (Random123), counter (c0, c1, 0, 0)
    uint32_t c[4] = {c0, c1, 0, 0};
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1,
                       n3 = (uint32_t)p0;
        c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    std::memcpy(out, c, sizeof(c));
}

// the 256 point pairs of the steered-BRIEF tests
static void orb_pattern_host(int8_t P[1024])
{
    for (int i = 0; i < 256; ++i) {
        uint32_t w[8];
        philox_host((uint32_t)i, 0, 0x0B5EED00u, 0x31u, w);
        philox_host((uint32_t)i, 1, 0x0B5EED00u, 0x31u, w + 4);
        int c[4];
        for (int k = 0; k < 4; ++k) {
            const uint32_t a = w[2 * k], b = w[2 * k + 1];
            const int u = (int)((a & 0xffffu) + (a >> 16) + (b & 0xffffu) + (b >> 16)) - 131072;
            c[k] = std::max(-13, std::min(13, (u * 11) / 65536));
        }
        if (c[0] == c[2] && c[1] == c[3])
            c[2] = c[0] + (c[0] < 0 ? 3 : -3);
        for (int k = 0; k < 4; ++k)
            P[4 * i + k] = (int8_t)c[k];
    }
}

// pyramid layout and per-level quotas (cv::ORB: n_l proportional to 1.2^-l, the last level takes the remainder)
static bool orb_layout_host(int w, int h, const mvs_orb_params &p, OrbDev &d, size_t &pixels)
{
    if (p.nlevels < 1 || p.nlevels > kOrbMaxLevels || p.nfeatures < 1)
        return false;
    double s = 1.0;
    pixels = 0;
    for (int l = 0; l < p.nlevels; ++l) {
        OrbLevel &L = d.level[l];
        L.w = (int)std::lrint((double)w / s);
        L.h = (int)std::lrint((double)h / s);
        L.scale = (float)s;
        L.offset = pixels;
        pixels += (size_t)std::max(L.w, 0) * std::max(L.h, 0);
        s = s * 1.2;
    }
    const double factor = 1.0 / 1.2;
    double fn = 1.0;
    for (int l = 0; l < p.nlevels; ++l)
        fn = fn * factor;
    double nd = (double)p.nfeatures * (1.0 - factor) / (1.0 - fn);
    int sum = 0;
    for (int l = 0; l < p.nlevels - 1; ++l) {
        // the rounded shares can add up to more than nfeatures when nfeatures is small (cv::ORB then returns more
        // keypoints than asked for); the outputs have room for nfeatures: a level takes at most what is left
        d.level[l].n_keep = std::min((int)std::lrint(nd), p.nfeatures - sum);
        sum += d.level[l].n_keep;
        nd = nd * factor;
    }
    d.level[p.nlevels - 1].n_keep = std::max(p.nfeatures - sum, 0);
    return true;
}

// runs the extraction of n images (host pointer) through the ctx workspace; outputs go to the given DEVICE arrays
// (desc / kp_xy / n_kp may belong to a sequence) and, when kp_rec_out is non-null, records are also left in the workspace
// wait = false: the overflow flag's copy is queued but not waited for -- the caller queues its own downloads behind it, waits
// once and then reads *ctx->h_orb_ovf
mvs_status mvs_host::orb_run(mvs_ctx *ctx, const uint8_t *images, int n, int w, int h, const mvs_orb_params &prm,
                             uint8_t *d_desc_ext, float *d_kp_xy_ext, int32_t *d_n_ext, OrbDev &d, uint8_t *d_kp_oct_ext,
                             bool wait)
{
    if (w < 1 || h < 1 || w > 65535 || h > 65535)
        return MVS_ERR_CAPACITY;
    if (prm.fast_threshold < 1 || prm.fast_threshold > 254 || prm.edge_threshold < 19)
        return MVS_ERR_INVALID_ARG;
    d = OrbDev{};
    size_t T = 0;
    if (!orb_layout_host(w, h, prm, d, T))
        return MVS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->orb_ready) {
        HIP_TRY(ctx, orb_prepare());
        ctx->orb_ready = true;
    }
    const size_t B = (size_t)n, NL = (size_t)prm.nlevels, NF = (size_t)prm.nfeatures;
    Carve L{256};
    const size_t o_pyr = L.take(T * B);
    const size_t o_blur = L.take(T * B);
    // resize tables: for every level >= 1, {source index, 11-bit weight} per destination column, then per row.  Their layout
    // is part of the key, their contents are built only when the key is new (below)
    size_t tab_entries = 0;
    for (int l = 1; l < prm.nlevels; ++l) {
        d.level[l].tab_offset = tab_entries;
        tab_entries += (size_t)std::max(d.level[l].w, 0) + (size_t)std::max(d.level[l].h, 0);
    }
    auto build_tab = [&](std::vector<int2> &tab) {
        tab.reserve(tab_entries);
        for (int l = 1; l < prm.nlevels; ++l) {
            const OrbLevel &Lv = d.level[l], &Pv = d.level[l - 1];
            for (int pass = 0; pass < 2; ++pass) {
                const long long sn = pass ? Pv.h : Pv.w, dn = pass ? Lv.h : Lv.w;
                for (long long dd = 0; dd < dn; ++dd) {
                    const long long num = (2 * dd + 1) * sn - dn, den = 2 * dn;   // source coordinate = num / den (>= 0 here)
                    long long si = num >= 0 ? num / den : -1;
                    const long long fr = num - si * den;
                    int wgt = (int)((fr * 4096 + den) / (2 * den));               // round(frac * 2048)
                    if (si < 0) si = 0, wgt = 0;
                    if (si >= sn - 1) si = sn - 1;
                    tab.push_back(make_int2((int)si, wgt));
                }
            }
        }
    };
    const size_t o_tab = L.take(std::max<size_t>(tab_entries, 1) * sizeof(int2));
    // candidate lists: a level's list holds the non-maximum suppression's own bound -- strict 3x3 maxima of the detection
    // area, at most one per 2x2 block -- so it cannot overflow; only when 2 n_l exceeds what the selection holds in LDS the
    // list is capped there (and a fuller level is reported as MVS_ERR_CAPACITY, as every level was in rounds 2-4)
    int max_keep = 0;
    for (int l = 0; l < prm.nlevels; ++l)
        max_keep = std::max(max_keep, d.level[l].n_keep);
    size_t cand_total = 0;
    for (int l = 0; l < prm.nlevels; ++l) {
        OrbLevel &Lv = d.level[l];
        const long long dw = (long long)Lv.w - 2 * prm.edge_threshold, dh = (long long)Lv.h - 2 * prm.edge_threshold;
        long long cap = dw > 0 && dh > 0 ? ((dw + 1) / 2) * ((dh + 1) / 2) + 64 : 64;
        if (2LL * max_keep > kOrbSelCap)
            cap = std::min<long long>(cap, kOrbSelCap);
        if (cap > 0x7fffffff)
            return MVS_ERR_CAPACITY;
        Lv.cand_cap = (int)cap;
        Lv.cand_off = cand_total;
        cand_total += (size_t)cap;
    }
    d.cand_stride = cand_total;
    const size_t o_keys = L.take(B * cand_total * 8);
    const size_t o_cc = L.take(B * NL * 4);
    const size_t o_sel = L.take(B * NL * NF * sizeof(OrbSel));
    const size_t o_sc = L.take(B * NL * 4);
    const size_t o_ovf = L.take(4);
    const size_t o_pat = L.take(1024);
    const size_t o_kp = L.take(B * NF * sizeof(mvs_keypoint));
    const size_t o_desc = L.take(B * NF * 32);
    const size_t o_n = L.take(B * 4);
    if (ctx->orb.bytes < L.total())
        drop_orb_graph(ctx);   // before its workspace is freed: a failed growth must not leave it behind
    const mvs_status st = ws_grow(ctx, ctx->orb, L.total());
    if (st != MVS_OK)
        return st;
    char *base = ctx->orb.ptr();
    d.n_images = n;
    d.n_levels = prm.nlevels;
    d.nfeatures = prm.nfeatures;
    d.edge = prm.edge_threshold;
    d.fast_threshold = prm.fast_threshold;
#ifdef MVS_DEBUG_HOOKS
    d.flat_order = std::getenv("MVS_ORB_FLAT_ORDER") != nullptr;   // A/B of the describe kernel's block order (tools/profile_extract.sh)
#endif
    d.pyr = reinterpret_cast<uint8_t *>(base + o_pyr);
    d.blur = reinterpret_cast<uint8_t *>(base + o_blur);
    d.resize_tab = reinterpret_cast<const int2 *>(base + o_tab);
    d.cand_keys = reinterpret_cast<uint64_t *>(base + o_keys);
    d.cand_count = reinterpret_cast<int32_t *>(base + o_cc);
    d.sel = reinterpret_cast<OrbSel *>(base + o_sel);
    d.sel_count = reinterpret_cast<int32_t *>(base + o_sc);
    d.overflow = reinterpret_cast<int32_t *>(base + o_ovf);
    d.pattern = reinterpret_cast<int8_t *>(base + o_pat);
    d.kp = reinterpret_cast<mvs_keypoint *>(base + o_kp);
    d.desc = d_desc_ext ? d_desc_ext : reinterpret_cast<uint8_t *>(base + o_desc);
    d.n_kp = d_n_ext ? d_n_ext : reinterpret_cast<int32_t *>(base + o_n);
    d.kp_xy = d_kp_xy_ext;
    d.kp_oct = d_kp_oct_ext;
    hipStream_t s = ctx_stream(ctx);
    // the test pattern and the resize tables depend on (size, parameters, workspace) only: a call with the key of the captured
    // graph finds them in the workspace (round 5: they were uploaded, and the stream synchronised for them, on every call)
    const bool same_key = ctx->orb_graph_valid && std::memcmp(&ctx->orb_graph_key, &d, sizeof(d)) == 0;
    int8_t pat[1024];
    std::vector<int2> tab;
    if (!same_key) {
        orb_pattern_host(pat);
        build_tab(tab);
        HIP_TRY(ctx, hipMemcpyAsync(base + o_pat, pat, sizeof(pat), hipMemcpyHostToDevice, s));
        if (!tab.empty())
            HIP_TRY(ctx, hipMemcpyAsync(base + o_tab, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d.pyr, images, (size_t)w * h * B, hipMemcpyHostToDevice, s));  // level 0 = the input
    if (!same_key)
        HIP_TRY(ctx, sync_stream(ctx));   // `pat` and `tab` live on this frame
#ifdef MVS_DEBUG_HOOKS
    static const bool no_graph = std::getenv("MVS_NO_GRAPH") != nullptr;   // A/B switch for tools/extract_bench.py (diagnostics build only)
#else
    constexpr bool no_graph = false;
#endif
    if (no_graph) {
        launch_orb(d, s);
    } else {
        if (!same_key) {
            drop_orb_graph(ctx);
            hipGraph_t graph = nullptr;
            HIP_TRY(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            launch_orb(d, s);
            HIP_TRY(ctx, hipStreamEndCapture(s, &graph));
            const hipError_t ie = hipGraphInstantiate(&ctx->orb_graph, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            HIP_TRY(ctx, ie);
            std::memcpy(&ctx->orb_graph_key, &d, sizeof(d));
            ctx->orb_graph_valid = true;
        }
        HIP_TRY(ctx, hipGraphLaunch(ctx->orb_graph, s));
    }
    HIP_TRY(ctx, hipGetLastError());
    if (!ctx->h_orb_ovf)
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_orb_ovf), 64, hipHostMallocDefault));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_orb_ovf, d.overflow, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (!wait)
        return MVS_OK;
    HIP_TRY(ctx, sync_stream(ctx));
    return *ctx->h_orb_ovf ? MVS_ERR_CAPACITY : MVS_OK;
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// extraction (row f3)
void mvs_orb_params_default(mvs_orb_params *p)
{
    if (!p)
        return;
    p->nfeatures = 500;
    p->nlevels = 8;
    p->edge_threshold = 31;
    p->fast_threshold = 20;
}

mvs_status mvs_extract_time(mvs_ctx *ctx, int steps, float *ms_total)
{
    if (!ctx || !ms_total || steps < 1)
        return MVS_ERR_INVALID_ARG;
    if (!ctx->orb_graph_valid || !ctx->orb_graph)
        return MVS_ERR_INVALID_ARG;   // nothing has been extracted on this context yet
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        ctx->err = "mvs_extract_time: hipEventCreate failed";
        return MVS_ERR_HIP;
    }
    hipStream_t s = ctx_stream(ctx);
    hipError_t e = hipEventRecord(e0, s);
    for (int i = 0; i < steps && e == hipSuccess; ++i)
        e = hipGraphLaunch(ctx->orb_graph, s);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(ms_total, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIP_TRY(ctx, e);
    return MVS_OK;
}

mvs_status mvs_extract(mvs_ctx *ctx, const uint8_t *images, int n_images, int width, int height,
                       const mvs_orb_params *params, mvs_keypoint *keypoints, uint8_t *descriptors, int32_t *n_keypoints)
{
    if (!ctx || !images || !params || !keypoints || !descriptors || !n_keypoints || n_images < 1)
        return MVS_ERR_INVALID_ARG;
    OrbDev d;
    // one wait per call: the outputs are queued behind the launches and the overflow flag (round 5: the flag had its own wait)
    const mvs_status st = orb_run(ctx, images, n_images, width, height, *params, nullptr, nullptr, nullptr, d, nullptr, false);
    if (st != MVS_OK)
        return st;
    const size_t B = n_images, NF = params->nfeatures;
    hipStream_t s = ctx_stream(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(keypoints, d.kp, B * NF * sizeof(mvs_keypoint), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(descriptors, d.desc, B * NF * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(n_keypoints, d.n_kp, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, sync_stream(ctx));
    return *ctx->h_orb_ovf ? MVS_ERR_CAPACITY : MVS_OK;
}
}  // extern "C"
