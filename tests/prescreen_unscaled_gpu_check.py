#!/usr/bin/env python3
"""GPU checks of the pre-screen with relaxed roots and quotients (run by tests/test_prescreen_unscaled.py in a process of its
own with MVS_USE_DEBUG_LIB=1: the mode switch and the record reader exist in the diagnostics library only).

  winners:<thr>  4 pairs x 256 matches x 512 hypotheses on the pre-screened stage, the probe deciding (-1) and every pair forced
                 to mode 0 (exact), 1 (matrix cores) and 2 (double-precision counting): winner, count, residual sum and mask are
                 the oracle's in every mode; after the pre-screen alone every certified record keeps the oracle's residuals
                 within its band.
  flags          the front-end check's crafted pair (tests/prescreen_frontend_gpu_check.py, imported: its rules are the
                 parent's -- state 0 <=> the oracle rejects the sample and no q is tiny, tiny => state 2, certified records
                 within their band, winners = oracle in every mode) with 256 hypotheses and four spreads of the image-1
                 coordinates: 1e-201 (every q = 0), 1e-130 (0 < q < 2^-767), 1e-20 (2^-767 <= q < 2^-100: the range the
                 relaxed normalisation hands to the guarded one as well) and 1e30 (means of roots above 2^60, the upper guard; still
                 inside binary32's range, which mode 1's points need).  That the fall-back is TAKEN is observed, not inferred:
                 per spread, the diagnostics library's count of wavefronts that took the guarded normalisation in one
                 pre-screen pass over the three pairs equals the count the range test gives in numpy -- every wavefront of the
                 crafted pair and its probe, none of the two general pairs'.
Prints one JSON line; exit code 0 = all checks passed."""
import contextlib
import ctypes as C
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MVS_USE_DEBUG_LIB"] = "1"
import oracle_lib as o  # noqa: E402
import prescreen_frontend_gpu_check as fe  # noqa: E402
import prescreen_model as pm  # noqa: E402
import prescreen_unscaled_model as pu  # noqa: E402
from mvslam_amd import capi  # noqa: E402

P, N, H, SEED = 4, 256, 512, 0x5EED1000


def winners(thr):
    uv1, uv2, K = np.zeros((P, N, 2)), np.zeros((P, N, 2)), np.zeros((P, 3, 3))
    for p in range(P):
        a, c = fe.scene(70 + p, N, outliers=0.25 + 0.1 * p)
        K[p] = fe.KCAM
        uv1[p] = a * 525 + np.array([320, 240.0])
        uv2[p] = c * 525 + np.array([320, 240.0])
    sizes = [N] * P
    gidx = np.arange(P, dtype=np.int64) + 2
    ctx = capi.Context(0)
    lib = capi.lib()
    b = capi.Batch(ctx, P, N, 32)
    b.upload_intrinsics(0, K.reshape(P, 9), gidx, count=P)
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=SEED, max_error_sq=thr)
    refs = [o.sfm_solve(uv1[p], uv2[p], K[p], o.make_params(H, o.SAMPLER_PHILOX, SEED + int(gidx[p]), thr)) for p in range(P)]
    stats = dict(thr=thr, pairs=P, modes_run=[], mismatch=0, certified=0, viol=0, probe_modes=[], worst_ratio=0.0)
    for mode in (-1, 0, 1, 2):
        lib.mvs_debug_set_prescreen_force(C.c_int(mode))
        b.run_points(prm, uv1, uv2, sizes)
        b.sync()
        out = b.download()
        stats["modes_run"].append(mode)
        for p in range(P):
            r, ref = out["results"][p], refs[p]
            good = bool(r["valid"]) == bool(ref["ok"])
            if good and ref["ok"]:
                good = (r["best_hyp"] == ref["best_hyp"] and r["best_count"] == ref["best_count"]
                        and r["best_residual"] == ref["best_residual"] and np.array_equal(out["mask"][p][:N], ref["mask"][:N]))
            stats["mismatch"] += not good
            if mode == -1:
                info = (C.c_int32 * 4)()
                state = np.zeros(H, dtype=np.uint8)
                st = lib.mvs_debug_read_hyp_rec(b._h, C.c_int(p), C.c_int(H), None, state.ctypes.data_as(C.POINTER(C.c_ubyte)), None, info)
                assert st == 0, st
                stats["probe_modes"].append(int(info[0]))
    lib.mvs_debug_set_prescreen_force(C.c_int(-1))
    # the pre-screen alone, double-precision records: every certified band covers the oracle's residuals
    st = lib.mvs_debug_prescreen_only(b._h, C.byref(prm), C.c_int(P), C.c_int(2))
    assert st == 0, st
    for p in range(P):
        p1, p2 = o.normalize_points(K[p], uv1[p]), o.normalize_points(K[p], uv2[p])
        rec = np.zeros((H, 10))
        state = np.zeros(H, dtype=np.uint8)
        info = (C.c_int32 * 4)()
        st = lib.mvs_debug_read_hyp_rec(b._h, C.c_int(p), C.c_int(H), rec.ctypes.data_as(C.POINTER(C.c_double)),
                                        state.ctypes.data_as(C.POINTER(C.c_ubyte)), None, info)
        assert st == 0, st
        for h in np.nonzero(state == 1)[0]:
            ok, FJ = o.find_fundamental_matrix(p1[o.sample8(SEED + int(gidx[p]), int(h), N)], p2[o.sample8(SEED + int(gidx[p]), int(h), N)])
            assert ok
            band = rec[h, 9] - thr
            d = float(np.abs(pm.residuals(FJ, p1, p2) - pm.residuals(rec[h, :9].reshape(3, 3), p1, p2)).max())
            stats["certified"] += 1
            stats["viol"] += not (0 < band and d <= band)
            stats["worst_ratio"] = max(stats["worst_ratio"], d / band)
    b.close()
    ctx.close()
    return stats


def front_end(spread, hyps):
    """tests/prescreen_frontend_gpu_check.py's main() for one spread and `hyps` hypotheses.  It takes both from its module
    (H, sys.argv[1]); they are set for the call and put back.  It asserts states, bands and winners itself (an AssertionError
    ends this process with a non-zero exit code) and prints one JSON line, which is returned."""
    old_h, old_argv = fe.H, sys.argv
    buf = io.StringIO()
    try:
        fe.H, sys.argv = hyps, [old_argv[0], repr(spread)]
        with contextlib.redirect_stdout(buf):
            fe.main()
    finally:
        fe.H, sys.argv = old_h, old_argv
    return json.loads([ln for ln in buf.getvalue().splitlines() if ln.startswith("{")][-1])


def fallback_waves(spread, hyps):
    """(counted, expected, of) wavefronts of one pair_prepare + ransac_prescreen pass over the front-end check's three pairs
    that took the guarded normalisation: the diagnostics library's counter against the range test evaluated in numpy on
    the radicands in the device's order of operations (a wavefront falls back as soon as one of its 64 samples has a
    radicand below Q_MIN or means of roots adding up to SC_MAX or more; the probe is one more wavefront per pair, on the
    pair's first 64 hypotheses)"""
    uv1, uv2, K = fe.inputs(spread)
    gidx = np.array([3, 4, 5], dtype=np.int64)
    expected = waves = 0
    for p, m in enumerate(fe.SIZES):
        p1, p2 = o.normalize_points(K[p], uv1[p, :m]), o.normalize_points(K[p], uv2[p, :m])
        redo = np.zeros(hyps, dtype=bool)
        for h in range(hyps):
            q = fe.sample_q(p1, p2, o.sample8(fe.SEED + int(gidx[p]), h, m))
            with np.errstate(over="ignore", invalid="ignore"):
                sc = np.sqrt(q[:8]).mean() + np.sqrt(q[8:]).mean()
            redo[h] = not (q.min() >= pu.Q_MIN) or not (sc < pu.SC_MAX)
        per_wave = redo.reshape(-1, 64).any(axis=1)
        expected += int(per_wave.sum()) + int(per_wave[0])
        waves += len(per_wave) + 1
    ctx = capi.Context(0)
    lib = capi.lib()
    b = capi.Batch(ctx, fe.P, fe.N, 32)
    b.upload_intrinsics(0, K.reshape(fe.P, 9), gidx, count=fe.P)
    prm = capi.default_params(num_hypotheses=hyps, sampler=capi.SAMPLER_PHILOX, seed=fe.SEED, max_error_sq=fe.THR)
    b.run_points(prm, uv1, uv2, fe.SIZES)   # (the points reach the device with a run)
    b.sync()
    n = C.c_uint(0)
    st = lib.mvs_debug_prescreen_fallback_waves(ctx._h, C.c_int(1), C.byref(n))
    assert st == 0, st
    st = lib.mvs_debug_prescreen_only(b._h, C.byref(prm), C.c_int(fe.P), C.c_int(2))
    assert st == 0, st
    st = lib.mvs_debug_prescreen_fallback_waves(ctx._h, C.c_int(1), C.byref(n))
    assert st == 0, st
    b.close()
    ctx.close()
    return int(n.value), expected, waves


def flags():
    hyps = 256
    assert hyps % 64 == 0
    tot = dict(viol=0, zero_q=0, tiny=0, certified=0, fallback={})
    for spread in (1e-201, 1e-130, 1e-20, 1e30):
        st = front_end(spread, hyps)
        tot["viol"] += st["viol"] + st["count_viol"]
        tot["zero_q"] += st["zero_q"]
        tot["tiny"] += st["tiny"]
        tot["certified"] += st["certified"]
        tot["fallback"][repr(spread)] = fallback_waves(spread, hyps)
    return tot


if __name__ == "__main__":
    what = sys.argv[1]
    res = winners(float(what.split(":")[1])) if what.startswith("winners:") else flags()
    print(json.dumps(res))
    sys.exit(0 if res.get("mismatch", 0) == 0 and res["viol"] == 0 else 1)
