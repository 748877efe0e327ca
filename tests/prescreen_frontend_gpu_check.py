#!/usr/bin/env python3
"""GPU check of the pre-screen's front end -- the sampler, the gathers and the two Hartley normalisations -- on samples
that take its guarded path (run by tests/test_prescreen_frontend.py in its own process with MVS_USE_DEBUG_LIB=1: the record
reader and the mode switch exist in the diagnostics library only).

The normalisation takes its sixteen square roots without their zero / infinity / range fix-ups and tests the smallest
radicand q once; a wavefront with any q outside [2^-767, inf) recomputes with the guarded sequences.  Three pairs, 512
hypotheses (the pre-screened stage), M = 33 / 9 / 8:
  pair 0  general matches (fast path in nearly every wavefront);
  pair 1  two matches equal in image 1 (dependent rows in 7 of 9 samples: no certificate, exact solve);
  pair 2  all image-1 coordinates `spread` apart, K = identity, M = 8: every sample is a permutation of all matches.
          spread 1e-201: every q underflows to 0 -- the samples are rejected; spread 1e-130: 0 < q < 2^-767, the `tiny`
          decision -- no certificate, the exact solve rejects them.
Expected values come from the oracle (its sampler, its find_fundamental_matrix of every sample, its sfm_solve of every
pair) and from the q of each sample evaluated in numpy:
  * after the pre-screen alone: state 0  <=>  the oracle rejects the sample and no q is tiny; tiny => state 2; a certified
    record (state 1) satisfies |r_i(F_J) - r_i(F~)| <= band on every match, hence U >= count_J >= L;
  * after the whole stage (every pair exact / pre-screened single / double precision / the probe decides): state 0 <=> the
    oracle rejects the sample, and winner, count, residual sum and mask are the oracle's, byte for byte in every mode.
Prints one JSON line; exit code 0 = all checks passed."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MVS_USE_DEBUG_LIB"] = "1"
import oracle_lib as o  # noqa: E402
import prescreen_model as pm  # noqa: E402
from mvslam_amd import capi  # noqa: E402

P, N, H, THR, SEED = 3, 64, 512, 1e-2, 0x5EED0000
SIZES = [33, 9, 8]
KCAM = np.array([[525.0, 0, 320], [0, 525, 240], [0, 0, 1]])


def scene(seed, m, noise=3e-4, outliers=0.3):
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    R = o.rodrigues(w * (0.08 / np.linalg.norm(w)))
    X = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(3, 9, m)], axis=1)
    X2 = (R @ X.T).T + np.array([0.3, 0.02, 0.01])
    p1 = X[:, :2] / X[:, 2:3] + rng.normal(scale=noise, size=(m, 2))
    p2 = X2[:, :2] / X2[:, 2:3] + rng.normal(scale=noise, size=(m, 2))
    bad = rng.random(m) < outliers
    p2[bad] = rng.uniform(-0.5, 0.5, size=(int(bad.sum()), 2))
    return p1, p2


def inputs(spread):
    uv1, uv2, K = np.zeros((P, N, 2)), np.zeros((P, N, 2)), np.zeros((P, 3, 3))
    for p, m in enumerate(SIZES):
        a, c = scene(50 + p, m, outliers=0.3 if p == 0 else 0.0)
        if p < 2:
            K[p] = KCAM
            uv1[p, :m] = a * 525 + np.array([320, 240.0])
            uv2[p, :m] = c * 525 + np.array([320, 240.0])
        else:
            K[p] = np.eye(3)      # ideal coordinates pass through bit for bit
            k = np.arange(m, dtype=np.float64)
            uv1[p, :m] = np.stack([k * spread, ((k * k) % 5) * spread], 1)
            uv2[p, :m] = c
    uv1[1, 1] = uv1[1, 0]         # two matches equal in image 1
    return uv1, uv2, K


def sample_q(p1, p2, idx):
    """the sixteen radicands of the sample's two Hartley normalisations, in the device's order of operations"""
    qs = []
    for pts in (p1[idx], p2[idx]):
        mx = my = 0.0
        for i in range(8):
            mx += pts[i, 0]
            my += pts[i, 1]
        mx *= 0.125
        my *= 0.125
        dx, dy = pts[:, 0] - mx, pts[:, 1] - my
        qs.append(dx * dx + dy * dy)
    return np.concatenate(qs)


def main():
    spread = float(sys.argv[1])
    uv1, uv2, K = inputs(spread)
    gidx = np.array([3, 4, 5], dtype=np.int64)
    ctx = capi.Context(0)
    lib = capi.lib()
    b = capi.Batch(ctx, P, N, 32)
    b.upload_intrinsics(0, K.reshape(P, 9), gidx, count=P)
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=SEED, max_error_sq=THR)
    stats = dict(spread=spread, hyp=0, invalid=0, tiny=0, zero_q=0, certified=0, need_exact=0, viol=0, count_viol=0, worst_ratio=0.0)
    # the oracle's view of every sample, once
    truth = []
    for p, m in enumerate(SIZES):
        p1, p2 = o.normalize_points(K[p], uv1[p, :m]), o.normalize_points(K[p], uv2[p, :m])
        rows = []
        for h in range(H):
            idx = o.sample8(SEED + int(gidx[p]), h, m)
            ok, FJ = o.find_fundamental_matrix(p1[idx], p2[idx])
            q = sample_q(p1, p2, idx)
            rows.append((bool(ok), FJ, bool(((q > 0) & (q < 2.0 ** -767)).any()), bool((q == 0).any())))
        truth.append((p1, p2, rows))
    # the whole stage in every mode, and the states it leaves behind when every pair is pre-screened
    outs = []
    for mode in (0, 1, 2, -1):
        lib.mvs_debug_set_prescreen_force(C.c_int(mode))
        b.run_points(prm, uv1, uv2, SIZES)
        b.sync()
        outs.append(b.download())
        if mode == 1:
            for p in range(P):
                state = np.zeros(H, dtype=np.uint8)
                info = (C.c_int32 * 4)()
                st = lib.mvs_debug_read_hyp_rec(b._h, C.c_int(p), C.c_int(H), None, state.ctypes.data_as(C.POINTER(C.c_ubyte)), None, info)
                assert st == 0 and info[0] == 1, (st, p, info[0])
                for h, (ok, _, _, _) in enumerate(truth[p][2]):
                    assert (state[h] == 0) == (not ok), ("state after the stage", p, h, int(state[h]), ok)
                    assert state[h] in (0, 1, 3), (p, h, int(state[h]))
    lib.mvs_debug_set_prescreen_force(C.c_int(-1))
    for k in ("results", "mask", "points", "point_idx"):
        assert all(outs[0][k].tobytes() == o_[k].tobytes() for o_ in outs[1:]), ("modes differ", k)
    for p, m in enumerate(SIZES):
        ref = o.sfm_solve(uv1[p, :m], uv2[p, :m], K[p], o.make_params(H, o.SAMPLER_PHILOX, SEED + int(gidx[p]), THR))
        r = outs[1]["results"][p]
        assert r["n_matches"] == m and bool(r["valid"]) == bool(ref["ok"]), (p, bool(r["valid"]), ref["ok"])
        if not ref["ok"]:     # (no sample of the pair survives: there is no winner to compare)
            continue
        assert r["best_hyp"] == ref["best_hyp"] and r["best_count"] == ref["best_count"], (p, int(r["best_hyp"]), ref["best_hyp"])
        assert r["best_residual"] == ref["best_residual"], (p, float(r["best_residual"]), ref["best_residual"])
        assert np.array_equal(outs[1]["mask"][p][:m], ref["mask"][:m]), p
    stats["valid"] = [int(v) for v in outs[1]["results"]["valid"]]
    # the pre-screen alone: per-hypothesis records and state bytes
    for pmode in (2, 1):
        st = lib.mvs_debug_prescreen_only(b._h, C.byref(prm), C.c_int(P), C.c_int(pmode))
        assert st == 0, st
        for p, m in enumerate(SIZES):
            p1, p2, rows = truth[p]
            rec = np.zeros((H, 10))
            state = np.zeros(H, dtype=np.uint8)
            info = (C.c_int32 * 4)()
            st = lib.mvs_debug_read_hyp_rec(b._h, C.c_int(p), C.c_int(H), rec.ctypes.data_as(C.POINTER(C.c_double)),
                                            state.ctypes.data_as(C.POINTER(C.c_ubyte)), None, info)
            assert st == 0 and info[0] == pmode
            rec32 = rec.view(np.float32).reshape(H, 20)
            q1, q2 = p1.astype(np.float32).astype(np.float64), p2.astype(np.float32).astype(np.float64)
            a1, a2 = np.c_[np.abs(q1), np.ones(m)], np.c_[np.abs(q2), np.ones(m)]
            for h, (ok, FJ, tiny, zero) in enumerate(rows):
                stats["hyp"] += 1
                stats["tiny"] += tiny
                stats["zero_q"] += zero
                assert (state[h] == 0) == (not ok and not tiny), ("state", pmode, p, h, int(state[h]), ok, tiny)
                if tiny:
                    assert state[h] == 2, ("tiny", pmode, p, h, int(state[h]))
                if state[h] == 0:
                    stats["invalid"] += 1
                    continue
                if state[h] == 2:
                    stats["need_exact"] += 1
                    continue
                assert state[h] == 1 and ok
                stats["certified"] += 1
                rj = pm.residuals(FJ, p1, p2)
                cj = int((rj < THR).sum())
                if pmode == 2:
                    band = rec[h, 9] - THR
                    assert 0 < band <= pm.BAND_FRAC * THR * (1 + 1e-12), (p, h, band)
                    ra = pm.residuals(rec[h, :9].reshape(3, 3), p1, p2)
                    d = float(np.abs(rj - ra).max())
                    cu, cl = int((ra < THR + band).sum()), int((ra < THR - band).sum())
                else:
                    F32 = rec32[h, :9].astype(np.float64).reshape(3, 3)
                    tu, tl = float(rec32[h, 9]), float(rec32[h, 10])
                    band = tu - THR if tl <= 0.0 else min(tu - THR, THR - tl)
                    assert 0 < band <= pm.BAND_FRAC * THR * (1 + 1e-5), (p, h, band)
                    ra = pm.residuals(F32, q1, q2)
                    slack = 11.01 * 2.0 ** -24 * np.einsum("ij,jk,ik->i", a2, np.abs(F32), a1)
                    d = float((np.abs(rj - ra) + slack).max())
                    cu, cl = int((ra - slack < tu).sum()), int((ra + slack < tl).sum())
                stats["worst_ratio"] = max(stats["worst_ratio"], d / band)
                stats["viol"] += d > band
                stats["count_viol"] += not (cu >= cj >= cl)
    b.close()
    ctx.close()
    print(json.dumps({k: (int(v) if isinstance(v, (bool, np.integer)) else v) for k, v in stats.items()}))
    assert stats["viol"] == 0 and stats["count_viol"] == 0


if __name__ == "__main__":
    main()
