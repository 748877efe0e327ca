"""The pre-screen with relaxed roots and quotients on the way to F~ (prescreen.hpp sqrt_relaxed_h / rcp_relaxed, DESIGN.md
section 4.3e (viii)).

CPU: tests/prescreen_unscaled_model.py (the relaxed sequences in the device's operation order, exact fma, hardware seeds
modelled as the true value (1 + e), |e| <= 2^-26) against the error bounds the derivation states, against the old model
(certificates lost) and against the oracle (the band).  GPU: the device code against the oracle, winners / counts / masks at
three thresholds in every counting mode, and the range test's fall-back on crafted samples
(tests/prescreen_unscaled_gpu_check.py, a process of its own: the mode switch and the record reader live in the diagnostics
library).  Build only: the resource digest."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as o
import prescreen_model as pm
import prescreen_unscaled_model as pu
from mvslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = pm.U


def _rel_err_sqrt(g, x):
    """| g / sqrt(x) - 1 | in units of u, from exact rationals: g^2 / x - 1 = 2 e + e^2"""
    t = Fraction(g) * Fraction(g) / Fraction(x) - 1
    return abs(float(t)) / 2.0 / U


def test_relaxed_sequences_meet_their_stated_error_bounds():
    """sqrt_relaxed_h <= 1.01 u, rcp_relaxed <= 3.01 u, the reciprocal from the root's by-product <= 3.1 u -- for seeds at
    both ends of +-2^-26 and random ones, radicands over the guarded range"""
    rng = np.random.default_rng(3)
    xs = np.concatenate([2.0 ** rng.uniform(-100, 100, 300), rng.uniform(1.0, 4.0, 300), 2.0 ** rng.uniform(-760, 760, 100)])
    worst = dict(sqrt=0.0, rcp=0.0, rcph=0.0)
    for mode in ("plus", "minus", "rand"):
        seeds = pu.Seeds(mode, 7)
        for x in xs:
            x = float(x)
            g, h = pu.sqrt_relaxed_h(x, seeds)
            worst["sqrt"] = max(worst["sqrt"], _rel_err_sqrt(g, x))
            if 2.0 ** -500 < x < 2.0 ** 500:
                r = pu.rcp_relaxed(x, seeds)
                worst["rcp"] = max(worst["rcp"], abs(float(Fraction(r) * Fraction(x) - 1)) / U)
                iv = pu.rcp_from_h(g, h)
                worst["rcph"] = max(worst["rcph"], abs(float(Fraction(iv) * Fraction(g) - 1)) / U)
    print(json.dumps(worst))
    assert worst["sqrt"] <= 1.01 and worst["rcp"] <= 3.01 and worst["rcph"] <= 3.1, worst


def test_header_constants_cover_the_derivation():
    """the model's constants ARE prescreen.hpp's (parsed from it); they cover what DESIGN.md 4.3e (viii) derives"""
    assert pu.RHO_C == pu.header_constant("kPsRhoC") and pu.TRIP_E == pu.header_constant("kPsTrip")
    assert pu.RHO_C >= (1548 + 4.1 + 50.2) * U                     # rho: QR + relaxed column norms + A - A~
    assert pu.TRIP_E >= 1e-12 + 2.01 * pu.SCALE_U * U * 1.01        # kappa: + de-normalising with the relaxed scales
    assert pu.SCALE_U >= (1.01 + 7 + 3.01 + 1) + (1 + 7 + 1)        # | s~ / s - 1 | in u: relaxed path + exact path
    assert pu.Q_MIN == 2.0 ** -100 and pu.SC_MAX == 2.0 ** 60       # the range test the fall-back tests are built for


def _pairs():
    """two bench-like pairs and two small-baseline sequence pairs (the kinds DESIGN.md 4.3i (1) studied)"""
    work = []
    for pi in range(2):
        d = synth.make_pair(pi, n_kp=1000)
        mt = o.match_visual_features(d["desc1"], d["desc2"], 0.7, 10.0)
        work.append(("bench %d" % pi, o.normalize_points(d["K"], d["kp1"][mt["trainIdx"]].astype(np.float64)),
                     o.normalize_points(d["K"], d["kp2"][mt["queryIdx"]].astype(np.float64)), synth.SEED_BASE + pi))
    seq = synth.make_sequence(5, n_kp=1000)
    K = np.asarray(seq["K"]).reshape(3, 3)
    for k in (0, 3):
        mt = o.match_visual_features(seq["desc"][k][:seq["n_kp"][k]], seq["desc"][k + 1][:seq["n_kp"][k + 1]], 0.7, 10.0)
        work.append(("sequence %d" % k, o.normalize_points(K, seq["kp"][k][mt["trainIdx"]].astype(np.float64)),
                     o.normalize_points(K, seq["kp"][k + 1][mt["queryIdx"]].astype(np.float64)), synth.SEED_BASE + k))
    return work


def test_constants_hold_and_few_certificates_are_lost():
    """4 pairs x 800 hypotheses, each through the relaxed model three times: random hardware seeds, every seed at +2^-26,
    every seed at -2^-26.  The constants are the device's, read from prescreen.hpp by the model.  Per hypothesis: the relaxed scales are within SCALE_U u of the exact path's and the design
    matrix within 50.1 u ||A||_F; ||A n~|| for the EXACT path's A is within the new rho; sigma8's bound is a lower bound of
    sigma_8 of the exact path's A; and for every certified hypothesis |r_i(F_J) - r_i(F~)| <= band on every match.  Certified =
    the model certifies and band <= 4 thr (thr = 1e-2).  The share of hypotheses certified by the old model and not by the
    new one is printed and stays below 1 %."""
    thr, hyps = 1e-2, 800
    modes = ("rand", "plus", "minus")
    tot = {m: dict(n=0, cert_old=0, cert_new=0, lost=0, worst=0.0, worst_scale_u=0.0, worst_dA_u=0.0, worst_rho=0.0) for m in modes}
    for name, p1, p2, seed in _pairs():
        bbox = (p1[:, 0].min(), p1[:, 0].max(), p1[:, 1].min(), p1[:, 1].max(),
                p2[:, 0].min(), p2[:, 0].max(), p2[:, 1].min(), p2[:, 1].max())
        seeds = {m: pu.Seeds(m, seed & 0xFFFF) for m in modes}
        st = {m: dict(n=0, cert_old=0, cert_new=0, lost=0) for m in modes}
        r_j = pm.residuals   # (shorthand)
        for h in range(hyps):
            idx = o.sample8(seed, h, len(p1))
            # once per hypothesis: the old model, the oracle's F_J and residuals, the exact path's normalisation and design matrix
            r0 = pm.prescreen(p1[idx, 0], p1[idx, 1], p2[idx, 0], p2[idx, 1], bbox)
            ok, FJ = o.find_fundamental_matrix(p1[idx], p2[idx])
            res_j = r_j(FJ, p1, p2) if ok else None
            c0 = bool(r0["screenable"] and r0["band"] <= pm.BAND_FRAC * thr)
            a1, b1, s1, _, _, _ = pm.hartley(p1[idx, 0], p1[idx, 1])
            a2, b2, s2, _, _, _ = pm.hartley(p2[idx, 0], p2[idx, 1])
            A = pm.design(a1, b1, a2, b2)
            nA = float(np.sqrt((A * A).sum()))
            sig8 = np.linalg.svd(A, compute_uv=False)[7]
            # the relaxed model with random seeds and with every seed at either end of +-2^-26, where the 22 u / 50.1 u /
            # rho bounds are tightest
            for m in modes:
                t, s = tot[m], st[m]
                r1 = pu.prescreen(p1[idx, 0], p1[idx, 1], p2[idx, 0], p2[idx, 1], bbox, seeds[m])
                assert ok == r1["ok"] == r0["ok"] and not r1["fallback"]
                c1 = bool(r1["screenable"] and r1["band"] <= pm.BAND_FRAC * thr)
                s["n"] += 1
                s["cert_old"] += c0
                s["cert_new"] += c1
                s["lost"] += c0 and not c1
                t["worst_scale_u"] = max(t["worst_scale_u"], abs(r1["s"][0] / s1 - 1) / U, abs(r1["s"][1] / s2 - 1) / U)
                t["worst_dA_u"] = max(t["worst_dA_u"], float(np.sqrt(((A - r1["A"]) ** 2).sum())) / nA / U)
                res = float(np.sqrt(((A @ r1["n"]) ** 2).sum()))
                assert res <= r1["rho"], (name, m, h, res, r1["rho"])
                t["worst_rho"] = max(t["worst_rho"], res / r1["rho"])
                if "sig8_lb" in r1:
                    assert r1["sig8_lb"] <= sig8 * (1 + 1e-12), (name, m, h)
                if not r1["screenable"]:
                    continue
                d = float(np.abs(res_j - r_j(r1["F"], p1, p2)).max())
                assert d <= r1["band"], (name, m, h, d, r1["band"])     # soundness: the one thing the band has to do
                t["worst"] = max(t["worst"], d / r1["band"])            # (printed: how far inside)
        for m in modes:
            print(name, m, json.dumps(st[m]))
            assert st[m]["lost"] < 0.01 * st[m]["n"], (name, m, st[m])
            for k in st[m]:
                tot[m][k] += st[m][k]
    print(json.dumps(tot))
    assert pu.RHO_C >= 1.8e-13 and pu.TRIP_E >= pm.TRIP_E          # the constants only grow (the data-dependent eps2 of a
                                                                    # hypothesis follows F~'s last bits either way)
    for m in modes:
        t = tot[m]
        assert t["n"] == 4 * hyps and t["cert_new"] > 0.5 * t["n"], (m, t)
        assert t["lost"] < 0.01 * t["n"], (m, t)
        assert t["worst_scale_u"] <= pu.SCALE_U and t["worst_dA_u"] <= 50.1, (m, t)


def test_model_takes_the_old_path_outside_the_range_test():
    """a radicand below 2^-100 (two coincident sample points: q of neither is small, but a point ON the mean is) sends the
    sample through the old model, unchanged"""
    rng = np.random.default_rng(2)
    x1, y1, x2, y2 = rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8)
    x1[7] = x1[:7].sum() / 7.0
    y1[7] = y1[:7].sum() / 7.0          # point 7 on the mean of the sample up to rounding: q ~ 1e-32
    bbox = (-1, 1, -1, 1, -1, 1, -1, 1)
    r = pu.prescreen(x1, y1, x2, y2, bbox)
    assert r["fallback"]
    r0 = pm.prescreen(x1, y1, x2, y2, bbox)
    assert r["ok"] == r0["ok"] and r["band"] == r0["band"]


def _run(what):
    env = dict(os.environ, MVS_USE_DEBUG_LIB="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prescreen_unscaled_gpu_check.py"), what], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    st = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(st))
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [1e-2, 1e-3, 1e-4])
def test_winners_counts_and_masks_are_the_oracles(thr):
    """4 pairs x 256 keypoints x 512 hypotheses on the pre-screened stage: winner, best count, residual sum and mask equal the
    oracle's with the probe deciding and with every pair forced to mode 0, 1 and 2"""
    st = _run("winners:%r" % thr)
    assert st["pairs"] == 4 and st["modes_run"] == [-1, 0, 1, 2] and st["mismatch"] == 0
    assert st["certified"] > 0 and st["viol"] == 0


@pytest.mark.gpu
def test_range_test_falls_back_with_the_parents_flags():
    """one crafted pair, 64 keypoints x 256 hypotheses (+ two filler pairs so that the stage is taken): coincident points
    (q = 0), 0 < q < 2^-767, 2^-767 <= q < 2^-100 and coordinates near the upper guard.  States follow the rule the parent
    implements (0 <=> the oracle rejects and no q is tiny; tiny => 2), certified records keep their band, winner = oracle:
    the front-end check asserts these itself, and the process ends with a non-zero exit code (caught in _run) if one fails.
    That the fall-back path is taken is read from the diagnostics library's counter: per spread, the wavefronts of one
    pre-screen pass that took the guarded normalisation are exactly those the range test selects in numpy -- all of the
    crafted pair's (256 / 64 + its probe = 5), none of the two general pairs' (the other 10 of 15)"""
    st = _run("flags")
    assert st["viol"] == 0 and st["zero_q"] > 0 and st["tiny"] > 0
    assert sorted(st["fallback"]) == sorted(repr(s) for s in (1e-201, 1e-130, 1e-20, 1e30))
    for spread, (counted, expected, waves) in st["fallback"].items():
        assert counted == expected, (spread, counted, expected)
        assert waves == 15 and 5 <= expected < waves, (spread, expected, waves)


def test_prescreen_keeps_three_wavefronts_and_no_scratch():
    path = os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")
    if not os.path.exists(path):
        pytest.fail("kernel_resources.json is missing: build first")
    res = json.load(open(path))
    key = [k for k in res if "ransac_prescreen_kernel" in k]
    assert len(key) == 1
    r = res[key[0]]
    assert r["occupancy_waves_per_simd"] >= 3 and r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
