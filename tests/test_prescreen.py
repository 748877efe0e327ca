"""The RANSAC pre-screen (mvslam_amd/csrc/prescreen.hpp): an approximate fundamental matrix per
hypothesis with a certified bound on every match's residual against the exact (one-sided Jacobi) result, so that
hypotheses which provably cannot win are never solved exactly -- and the winner is still the reference's, bit for bit.

CPU part: tests/prescreen_model.py (the same arithmetic and the same constants in numpy) against the oracle's
find_fundamental_matrix on random and adversarial samples: wherever the model certifies a band, the oracle's residuals lie
within it.  GPU part: the device code itself, hypothesis by hypothesis, and the whole stage in every mode
(tests/prescreen_gpu_check.py, its own process: the record reader lives in the diagnostics library)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as o
import prescreen_model as pm
from mvslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bbox(p1, p2):
    return (p1[:, 0].min(), p1[:, 0].max(), p1[:, 1].min(), p1[:, 1].max(),
            p2[:, 0].min(), p2[:, 0].max(), p2[:, 1].min(), p2[:, 1].max())


def _check(p1, p2, idx, bbox, stats, v3=None):
    r = pm.prescreen(p1[idx, 0], p1[idx, 1], p2[idx, 0], p2[idx, 1], bbox, v3)
    ok, FJ = o.find_fundamental_matrix(p1[idx], p2[idx])
    assert ok == r["ok"]
    stats["n"] += 1
    if not r["screenable"]:
        return
    stats["cert"] += 1
    rj, ra = pm.residuals(FJ, p1, p2), pm.residuals(r["F"], p1, p2)
    d = float(np.abs(rj - ra).max())
    assert d <= r["band"], (d, r["band"])
    stats["worst"] = max(stats["worst"], d / r["band"])
    sv = np.linalg.svd(r["A"], compute_uv=False)
    assert r["sig8_lb"] <= sv[7] * (1 + 1e-12)                      # a LOWER bound of sigma_8(A)
    # the single-precision leg: residuals of the binary32-rounded F~ and points stay within band + e32 (the arithmetic
    # roundings of the device's binary32 evaluation are the rest of e32's sixteen)
    F32 = r["F"].astype(np.float32).astype(np.float64)
    q1, q2 = p1.astype(np.float32).astype(np.float64), p2.astype(np.float32).astype(np.float64)
    d32 = float(np.abs(rj - pm.residuals(F32, q1, q2)).max())
    assert d32 <= r["band"] + 0.25 * r["e32"], (d32, r["band"], r["e32"])


def test_model_band_covers_the_oracle_on_synthetic_pairs():
    stats = dict(n=0, cert=0, worst=0.0)
    for pi in range(2):
        d = synth.make_pair(pi, n_kp=1000)
        mt = o.match_visual_features(d["desc1"], d["desc2"], 0.7, 10.0)
        p1 = o.normalize_points(d["K"], d["kp1"][mt["trainIdx"]].astype(np.float64))
        p2 = o.normalize_points(d["K"], d["kp2"][mt["queryIdx"]].astype(np.float64))
        bbox = _bbox(p1, p2)
        for h in range(400):
            _check(p1, p2, o.sample8(synth.SEED_BASE + pi, h, len(mt)), bbox, stats)
    assert stats["cert"] > 0.9 * stats["n"]          # well-conditioned samples get a certificate ...
    assert stats["worst"] < 1e-3                     # ... and the bound is conservative by orders of magnitude


def test_model_band_on_adversarial_samples():
    """near-degenerate samples: the model must either refuse a certificate or still cover the oracle"""
    rng = np.random.default_rng(5)
    stats = dict(n=0, cert=0, worst=0.0)
    R = np.array([[0.9998, -0.01, 0.015], [0.0102, 0.9999, -0.004], [-0.0149, 0.0042, 0.9999]])
    t = np.array([0.3, 0.02, 0.01])
    for trial in range(300):
        kind = trial % 6
        n = 40
        X = np.c_[rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2, 10, n)]
        if kind == 1:      # the sample almost collinear in image 1
            X[:8, 1] = 0.3 * X[:8, 0] + 10.0 ** rng.uniform(-9, -2) * rng.normal(size=8)
            X[:8, 2] = 4.0
        if kind == 2:      # two sample points (nearly) identical
            X[1] = X[0] + 10.0 ** rng.uniform(-12, -3) * rng.normal(size=3)
        if kind == 3:      # the sample in a tiny cluster, the other points far away
            X[:8] = X[0] + 10.0 ** rng.uniform(-6, -2) * rng.normal(size=(8, 3))
        if kind == 4:      # coplanar scene (a degenerate configuration for F)
            X[:, 2] = 5.0 + 10.0 ** rng.uniform(-8, -1) * rng.normal(size=n)
        p1 = X[:, :2] / X[:, 2:3]
        X2 = (R @ X.T).T + t
        p2 = X2[:, :2] / X2[:, 2:3]
        if kind == 5:      # pure outliers
            p2 = rng.uniform(-0.5, 0.5, size=(n, 2))
        p1 = p1 + rng.normal(scale=1e-3, size=p1.shape)
        p2 = p2 + rng.normal(scale=1e-3, size=p2.shape)
        _check(p1, p2, np.arange(8), _bbox(p1, p2), stats)
    assert stats["n"] == 300 and stats["cert"] > 100


def test_rank2_step_is_a_posteriori():
    """the rank-2 step takes ANY approximation of the smallest right singular vector: a vector that is off by 1e-9 ... 1e-2
    must widen the band (or lose the certificate), never break the bound; noise-free samples (sigma_3 ~ 1e-16, where the
    left vector is rounding noise) take the second branch of the step and keep a small band"""
    rng = np.random.default_rng(11)
    d = synth.make_pair(0, n_kp=1000)
    mt = o.match_visual_features(d["desc1"], d["desc2"], 0.7, 10.0)
    p1 = o.normalize_points(d["K"], d["kp1"][mt["trainIdx"]].astype(np.float64))
    p2 = o.normalize_points(d["K"], d["kp2"][mt["queryIdx"]].astype(np.float64))
    bbox = _bbox(p1, p2)
    base = dict(n=0, cert=0, worst=0.0)
    for mag in (1e-9, 1e-6, 1e-4, 1e-2):
        stats = dict(n=0, cert=0, worst=0.0)
        for h in range(60):
            idx = o.sample8(synth.SEED_BASE, h, len(mt))
            r0 = pm.prescreen(p1[idx, 0], p1[idx, 1], p2[idx, 0], p2[idx, 1], bbox)
            if not r0["ok"] or "n" not in r0:
                continue
            G = r0["n"].reshape(3, 3)
            v = np.linalg.eigh(G.T @ G)[1][:, 0] + mag * rng.normal(size=3)
            _check(p1, p2, idx, bbox, stats, v3=v)
            r1 = pm.prescreen(p1[idx, 0], p1[idx, 1], p2[idx, 0], p2[idx, 1], bbox, v)
            if r0["screenable"] and r1["screenable"]:
                assert r1["band"] >= r0["band"] * (1 - 1e-9)
        assert stats["n"] > 50
        base[mag] = stats["cert"]
    assert base[1e-9] > 50 and base[1e-2] <= base[1e-9]
    # noise-free two-view geometry: exact epipolar constraint up to rounding
    R = np.array([[0.9998, -0.01, 0.015], [0.0102, 0.9999, -0.004], [-0.0149, 0.0042, 0.9999]])
    t = np.array([0.3, 0.02, 0.01])
    stats = dict(n=0, cert=0, worst=0.0)
    for trial in range(40):
        X = np.c_[rng.uniform(-1.5, 1.5, 40), rng.uniform(-1.0, 1.0, 40), rng.uniform(2, 10, 40)]
        q1 = X[:, :2] / X[:, 2:3]
        X2 = (R @ X.T).T + t
        q2 = X2[:, :2] / X2[:, 2:3]
        _check(q1, q2, np.arange(8), _bbox(q1, q2), stats)
    assert stats["cert"] > 30


def test_mixed_precision_study_numerics():
    """tools/mixed_precision_study.py (the CPU model that came BEFORE any device code): a binary32 Householder
    null vector is ~1e6 x worse than the binary64 one, one binary64 refinement step through the binary32 factors brings its
    residual back below the a-priori bound the band already carries -- the band is then the binary64 pre-screen's within a
    per cent.  (The study's verdict is about COST: profiles/r05_mixed_precision_study.json)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mps", os.path.join(ROOT, "tools", "mixed_precision_study.py"))
    mps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mps)
    d = synth.make_pair(0, n_kp=1000)
    mt = o.match_visual_features(d["desc1"], d["desc2"], 0.7, 10.0)
    p1 = o.normalize_points(d["K"], d["kp1"][mt["trainIdx"]].astype(np.float64))
    p2 = o.normalize_points(d["K"], d["kp2"][mt["queryIdx"]].astype(np.float64))
    rows = []
    mps.study_pair(p1, p2, synth.SEED_BASE, 60, rows)
    assert len(rows) > 50
    rho0 = np.median([r["rho0"] for r in rows])
    rho1 = np.median([r["rho1_meas"] for r in rows])
    assert 1e-8 < rho0 < 1e-5 and rho1 < 1e-5 * rho0
    ratio = np.array([r["band_mixed_1"] / r["band64"] for r in rows])
    assert np.isfinite(ratio).all() and np.median(ratio) < 1.05 and np.median([r["band_mixed_0"] / r["band64"] for r in rows]) > 50


def _bf16_bits(x):
    """round-to-nearest-even bf16 of finite binary32 values, as uint16 bit patterns (bf16_bits of kernels.hip)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def _bf16_value(b):
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def test_bf16_split_error_bound():
    """x = hi + lo + d with |d| <= 2^-16 |x| for the round-to-nearest-even bf16 split the counting kernels
    use, x - hi exact in binary32, and the three kept products of two split operands within 3 x 2^-16 of the full product --
    on random operands, on operands just below a rounding boundary (the worst case), and on powers of two."""
    rng = np.random.default_rng(3)
    x = (rng.normal(size=200000) * 10.0 ** rng.uniform(-6, 6, size=200000)).astype(np.float32)
    # the worst case of round-to-nearest: just below the midpoint between two bf16 numbers, at both levels
    worst = np.float32(1.0) + np.float32(2.0 ** -8) - np.float32(2.0 ** -23) + np.float32(2.0 ** -16) - np.float32(2.0 ** -22)
    x = np.concatenate([x, worst * np.float32(2.0) ** rng.integers(-20, 20, size=1000).astype(np.float32),
                        np.float32(2.0) ** np.arange(-30, 30, dtype=np.float32)]).astype(np.float32)
    hi = _bf16_value(_bf16_bits(x))
    r = (x - hi.astype(np.float32))
    assert np.all(r.astype(np.float64) == x.astype(np.float64) - hi)          # the difference is exact in binary32
    lo = _bf16_value(_bf16_bits(r))
    xd = x.astype(np.float64)
    assert np.all(np.abs(xd - hi) <= 2.0 ** -8 * np.abs(xd))
    d = np.abs(xd - hi - lo)
    assert np.all(d <= 2.0 ** -16 * np.abs(xd))
    y = rng.permutation(x)
    yh = _bf16_value(_bf16_bits(y))
    yl = _bf16_value(_bf16_bits(y - yh.astype(np.float32)))
    yd = y.astype(np.float64)
    kept = hi * yh + hi * yl + lo * yh
    err = np.abs(xd * yd - kept)
    assert np.all(err <= 3 * 2.0 ** -16 * np.abs(xd * yd) * (1 + 1e-9))
    print("worst split error %.3f x 2^-16, worst three-product error %.3f x 2^-16"
          % (float((d / np.abs(xd)).max() * 2 ** 16), float((err / np.abs(xd * yd)).max() * 2 ** 16)))


@pytest.mark.gpu
def test_matrix_core_tile_layout_and_accumulation_error():
    """the counting kernels sum 27 (+5 zero) products of bf16 numbers per evaluation with two
    v_mfma_f32_32x32x16_bf16; the bound assumes (A2) that every addition of the accumulation is off by at most 2^-23 of the sum
    of magnitudes.  One 32 x 32 x 32 tile through the same two instructions (diagnostics hook): out[point][hypothesis] must be
    the dot product of row `point` of A and row `hypothesis` of B -- which pins the K slot mapping and the accumulator layout
    -- to within 32 * 2^-23 * sum |terms| on operands of mixed magnitude and sign (heavy cancellation included); the worst
    ratio seen is printed."""
    import ctypes as C
    from mvslam_amd import capi

    dbg = C.CDLL(capi.DBG_LIB_PATH)
    h = C.c_void_p()
    assert dbg.mvs_ctx_create(C.c_int(0), C.byref(h)) == 0
    dbg.mvs_ctx_destroy.argtypes = [C.c_void_p]
    dbg.mvs_debug_mfma_probe.argtypes = [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_float)]
    rng = np.random.default_rng(7)
    worst = 0.0
    try:
        for trial in range(64):
            kind = trial % 4
            a = rng.normal(size=(32, 32)) * 10.0 ** rng.uniform(-3, 3, size=(32, 32) if kind != 1 else (32, 1))
            b = rng.normal(size=(32, 32)) * 10.0 ** rng.uniform(-3, 3, size=(32, 32) if kind != 1 else (32, 1))
            if kind == 2:      # cancellation: second half of the slots repeats the first with the opposite sign (nearly)
                a[:, 16:] = a[:, :16]
                b[:, 16:] = -b[:, :16] * (1 + 2.0 ** -7 * rng.normal(size=(32, 16)))
            if kind == 3:      # the kernels' own shape: hi / lo parts, five zero slots
                x, y = rng.normal(size=(32, 9)).astype(np.float32), rng.normal(size=(32, 9)).astype(np.float32)
                xh, yh = _bf16_value(_bf16_bits(x)), _bf16_value(_bf16_bits(y))
                xl, yl = (x - xh.astype(np.float32)), (y - yh.astype(np.float32))
                a = np.concatenate([xh, xh, xl, np.zeros((32, 5))], axis=1)
                b = np.concatenate([yh, yl, yh, np.zeros((32, 5))], axis=1)
            A, B = _bf16_bits(a.astype(np.float32)), _bf16_bits(b.astype(np.float32))
            out = np.zeros((32, 32), dtype=np.float32)
            st = dbg.mvs_debug_mfma_probe(h, A.ctypes.data_as(C.POINTER(C.c_uint16)), B.ctypes.data_as(C.POINTER(C.c_uint16)),
                                          out.ctypes.data_as(C.POINTER(C.c_float)))
            assert st == 0
            av, bv = _bf16_value(A), _bf16_value(B)
            exact = av @ bv.T                              # [point][hypothesis], binary64: products of bf16 are exact
            mag = np.abs(av) @ np.abs(bv).T
            err = np.abs(out.astype(np.float64) - exact)
            assert np.all(err <= 32 * 2.0 ** -23 * mag + 1e-300), (trial, float((err / mag).max()))
            worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
    finally:
        dbg.mvs_ctx_destroy(h)
    print("worst accumulation error / sum of magnitudes: %.3g = %.2f * 2^-24" % (worst, worst * 2.0 ** 24))
    assert worst <= 32 * 2.0 ** -23


@pytest.mark.gpu
def test_device_prescreen_against_the_oracle_hypothesis_by_hypothesis():
    env = dict(os.environ, MVS_USE_DEBUG_LIB="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prescreen_gpu_check.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    st = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert st["viol"] == 0 and st["count_viol"] == 0 and st["certified"] > 0.5 * st["hyp"]
    assert st["mode0_list"] == [0, 0]                 # forced exact: nothing on the work list
    assert st["mode1_list"][0] > 0 and st["auto_list"][0] > 0
    assert st["mfma_checked"] > 20       # upper bounds of the matrix-core counting checked against exact counts


@pytest.mark.gpu
def test_full_population_device_audit():
    """VERDICT r3 #1b: every one of the 25.6 M hypotheses of BASELINE configs[2] (and of a 64-pair slice at the reference
    threshold, and of the first 128 sequence pairs) is solved exactly once more on the device and the stage's decision about
    it is checked there (tests/audit_gpu_check.py; estimator-RANSAC.cpp:76-84,100-129).  Round 5: the stage
    under audit is the PRODUCT binary's -- libmvslam_hip.so runs it, the diagnostics library only reads what it left in
    device memory (mvs_batch_device_state) and replays."""
    env = {k: v for k, v in os.environ.items() if k != "MVS_USE_DEBUG_LIB"}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "audit_gpu_check.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    st = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(st))
    assert st["ok"] and len(st["cases"]) == 4
    assert st["stage_binary"] == "libmvslam_hip.so" and st["audit_binary"] == "libmvslam_hip_dbg.so"
    assert st["negative_control"]["count_viol"] > 0          # the checker trips when it should
    c3 = st["cases"][0]
    assert c3["hypotheses"] == 512 * 50000 and c3["pairs_mode"][1] == 512       # all of configs[2] is pre-screened at 1e-2
    assert c3["phase2"]["checked"] > 0.9 * c3["hypotheses"]                     # ... and nearly all of it certified
    assert c3["phase2"]["matches_checked"] > 2.5e10                             # (B) on every match of every certified record
    assert c3["phase2"]["worst_ratio"] < 1.0
    assert st["cases"][1]["pairs_mode"][0] == 64                                # the reference threshold: every pair exact
    for c in st["cases"]:
        assert c["phase1"]["count_viol"] == 0 and c["phase1"]["max_sweeps9"] <= 30
    mixed = st["cases"][3]                                                        # a K per pair, five camera families
    assert mixed["pairs"] == 20 and mixed["hypotheses"] == 20 * 50000
    for ph in ("phase1", "phase2"):
        c = mixed[ph]
        assert c["count_viol"] == 0 and c["band_viol"] == 0 and c["upper_viol"] == 0, (ph, c)
        assert c["worst_ratio"] < 1.0 and c["checked"] > 0, (ph, c)
