"""CPU tests of the pose graphs' robust edge losses: the numpy model of their contract
(tests/pg_robust_model.py) against closed forms and central differences, the claim the feature rests on, the decision margins
of the fixtures the GPU tests share, the recorded exact-against-PCG gaps behind the GPU tolerance of the large path
(tests/golden/pg_robust_pcg_vs_exact.json) and the argument rules of mvs_ctx_set_pose_graph_loss."""
import json
import os
import subprocess

import numpy as np
import pytest

import pg_robust_model as rm
import posegraph_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pg_robust_pcg_vs_exact.json")

_RUNS = {}


def run(name, solver="exact"):
    """the model's answer for a fixture of pg_robust_model.FIXTURES, computed once per process and never modified"""
    if (name, solver) not in _RUNS:
        make, kw = rm.FIXTURES[name]
        g = make()
        _RUNS[(name, solver)] = (g, rm.optimize(g, solver=solver, **kw))
    return _RUNS[(name, solver)]


def clean_optimum(g):
    return m.optimize(rm.without_outliers(g))["poses"]


def test_loss_against_closed_forms():
    for s in (0.0, 1e-12, 0.5, 1.0, 1.8, 1.809025, 4.0, 1e4, 1e12):
        x = np.sqrt(s)
        assert rm.loss(s, rm.NONE, 1.0) == (1.0, s)
        for k in (0.3, 1.0, 1.345, 3.0):
            w, rho = rm.loss(s, rm.HUBER, k)
            if x <= k:
                assert (w, rho) == (1.0, s)
            else:
                assert abs(w - k / x) <= 1e-15 * w and abs(rho - (2 * k * x - k * k)) <= 1e-12 * max(rho, 1.0)
                assert rho < s and 0.0 < w < 1.0
            w, rho = rm.loss(s, rm.CAUCHY, k)
            assert abs(w - 1.0 / (1.0 + s / (k * k))) <= 4e-16 and abs(rho - k * k * np.log(1.0 + s / (k * k))) <= 1e-12 * max(rho, 1e-3)
            assert rho <= s and 0.0 < w <= 1.0
    # GTSAM's conventions: Huber's weight at twice the threshold is one half, Cauchy's at s = k^2 too
    assert rm.loss(4.0 * 1.345 ** 2, rm.HUBER, 1.345)[0] == pytest.approx(0.5, abs=1e-15)
    assert rm.loss(9.0, rm.CAUCHY, 3.0)[0] == 0.5
    # a Huber constant nothing reaches: the plain cost, exactly
    for s in (0.0, 3.7, 1e40):
        assert rm.loss(s, rm.HUBER, 1e30) == (1.0, s)


def test_weight_is_the_derivative_of_the_cost():
    """d(rho2 / 2) / d(s / 2) = w: central differences with h = 1e-6 s leave a relative truncation error of about h^2 and a
    rounding error of about eps / h, both below 1e-8"""
    for kind, k in ((rm.HUBER, 1.345), (rm.HUBER, 0.3), (rm.CAUCHY, 1.0), (rm.CAUCHY, 3.0)):
        for s in (0.01, 0.5, 2.5, 40.0, 1e4, 1e8):
            if kind == rm.HUBER and abs(np.sqrt(s) - k) < 1e-3:
                continue
            h = 1e-6 * s
            fd = (rm.loss(s + h, kind, k)[1] - rm.loss(s - h, kind, k)[1]) / (2 * h)
            w = rm.loss(s, kind, k)[0]
            assert abs(fd - w) <= 1e-8 * max(w, 1e-3) + 1e-9, (kind, k, s, fd, w)


def test_huber_is_continuous_at_its_threshold():
    for k in (0.3, 1.0, 1.345, 3.0):
        s = k * k
        lo, hi = rm.loss(s * (1 - 1e-12), rm.HUBER, k), rm.loss(s * (1 + 1e-12), rm.HUBER, k)
        assert lo[0] == 1.0 and abs(hi[0] - 1.0) <= 1e-11 and abs(hi[1] - lo[1]) <= 1e-11 * s


def test_gradient_of_the_robust_cost_matches_central_differences():
    """on the n = 12 fixture at its initial values, under both losses: h = 1e-6 on every tangent coordinate; the cost is of
    size 1e4 with third derivatives of size 1e8 (weights of 1e4 on residuals of size 1), so the bound is 1e-6 relative to
    the gradient's largest entry"""
    for name in ("n12_cauchy", "n12_huber", "n12_full_cauchy", "n12_cauchy3_all"):
        make, kw = rm.FIXTURES[name]
        g = make()
        kind, k, first = kw["loss"], kw["k"], kw["first_edge"]
        P = g["node_pose"]
        grad = rm.gradient(g, P, kind, k, first)
        h, fd = 1e-6, np.zeros(6 * 12)
        for i in range(12):
            for j in range(6):
                dx = np.zeros(6)
                dx[j] = h
                a, b = P.copy(), P.copy()
                a[i], b[i] = m.retract(P[i], dx), m.retract(P[i], -dx)
                fd[6 * i + j] = 0.5 * (rm.cost(g, a, kind, k, first) - rm.cost(g, b, kind, k, first)) / (2 * h)
        worst = float(np.abs(fd - grad).max() / np.abs(grad).max())
        print("%s: gradient against central differences, relative %.3e" % (name, worst))
        assert worst <= 1e-6, (name, worst)


def test_optimize_without_a_loss_is_the_plain_model():
    for g in (m.triangle(3)[0], m.ring(17), rm.outlier_ring(12)):
        # against posegraph_model: the cost is summed edge by edge here and over all residuals there, so to rounding
        a, b = m.optimize(g), rm.optimize(g)
        rot, trans = m.pose_distance(a["poses"], b["poses"])
        assert rot <= 1e-12 and trans <= 1e-12 and abs(a["error"] - b["error"]) <= 1e-12 * a["error"]
        # w = 1 and rho2 = s exactly: the same bytes
        c = rm.optimize(g, loss=rm.HUBER, k=1e30)
        assert b["poses"].tobytes() == c["poses"].tobytes() and b["error"] == c["error"] and b["iterations"] == c["iterations"]
        d = rm.optimize(g, loss=rm.CAUCHY, k=1.0, first_edge=len(g["edge_src"]))
        assert b["poses"].tobytes() == d["poses"].tobytes() and b["error"] == d["error"] and b["iterations"] == d["iterations"]


def test_fixture_shapes():
    for n in (12, 17, 20):
        g = rm.outlier_ring(n)
        assert g["node_pose"].shape[0] == n and len(g["edge_src"]) == 2 * n + 2
        assert list(zip(g["edge_src"][-2:].tolist(), g["edge_dst"][-2:].tolist())) == [(1, n // 2), (3, n - 2)]
        plain = m.ring(n, chords=(2,), full=False, extra_edges=[(1, n // 2), (3, n - 2)])
        assert g["edge_pose"][:2 * n].tobytes() == plain["edge_pose"][:2 * n].tobytes()
        assert m.pose_distance(g["edge_pose"][-2:], plain["edge_pose"][-2:])[0] > 0.8
        c = rm.without_outliers(g)
        assert len(c["edge_src"]) == 2 * n and c["node_pose"].tobytes() == g["node_pose"].tobytes()
    full = rm.outlier_ring(12, full=True)
    assert any(abs(c.reshape(6, 6)[0, 4]) > 1e-6 for c in full["edge_cov"])
    for name, (make, kw) in rm.FIXTURES.items():
        E = len(make()["edge_src"])
        assert kw["first_edge"] in (0, E - 2), name


def test_cauchy_on_the_added_edges_recovers_the_clean_optimum():
    """the claim the feature rests on: on both fixtures the optimum under Cauchy from first_edge is at least 100 x closer to
    the optimum of the clean graph than the unweighted one, in rotation and in translation"""
    for name in ("n12_cauchy", "n20_cauchy", "n12_full_cauchy"):
        g, r = run(name)
        clean = clean_optimum(g)
        plain = m.optimize(g)
        d_plain, d_rob = m.pose_distance(plain["poses"], clean), m.pose_distance(r["poses"], clean)
        s, w = rm.edge_stats(g, r["poses"], rm.CAUCHY, rm.CAUCHY_K, rm.FIXTURES[name][1]["first_edge"])
        print("%s: unweighted %.3e / %.3e, Cauchy %.3e / %.3e, iterations %d rejected %d, weights of the added edges %s" % (
            name, d_plain[0], d_plain[1], d_rob[0], d_rob[1], r["iterations"], r["rejected_steps"], w[-2:]))
        assert r["ok"] and r["exit"] == "converged"
        assert d_plain[0] >= 100.0 * d_rob[0] and d_plain[1] >= 100.0 * d_rob[1], name
        assert (w[:-2] == 1.0).all() and w[-2:].max() < 1e-3 and sorted(np.argsort(w)[:2]) == [len(w) - 2, len(w) - 1]
    for name in ("n12_huber", "n20_huber", "n12_cauchy3_all", "n20_cauchy3_all"):
        g, r = run(name)
        clean = clean_optimum(g)
        d_plain, d_rob = m.pose_distance(m.optimize(g)["poses"], clean), m.pose_distance(r["poses"], clean)
        print("%s: unweighted %.3e / %.3e, robust %.3e / %.3e, iterations %d" % (name, *d_plain, *d_rob, r["iterations"]))
        assert r["ok"] and d_plain[0] >= 10.0 * d_rob[0] and d_plain[1] >= 10.0 * d_rob[1], name


def counts_are_asserted(name, solver):
    """does the GPU test assert iterations / rejected_steps of this fixture?  Only where every decision of the model's run
    lies at least MARGIN units of eps * cost from the rounding of the cost."""
    return m.decision_margin(run(name, solver)[1]) >= rm.MARGIN


def test_decision_margins_decide_which_counts_are_asserted():
    """IRLS converges linearly: its last accepted step lowers the cost by a few units of eps * cost, so on most fixtures the
    accept / reject decision of that step is the rounding's, and the GPU test asserts no integer there"""
    for name in rm.FIXTURES:
        for solver in ("exact", "pcg"):
            r = run(name, solver)[1]
            margin = m.decision_margin(r)
            print("%s (%s): iterations %d rejected %d exit %s margin %.3g -> counts %s" % (
                name, solver, r["iterations"], r["rejected_steps"], r["exit"], margin,
                "asserted" if margin >= rm.MARGIN else "not asserted"))
            assert r["ok"] and r["iterations"] < m.LM_DEFAULT["max_iterations"]
            assert counts_are_asserted(name, solver) == (margin >= rm.MARGIN)


def measure_gaps():
    """the model with exact solves against the model with the block-Jacobi PCG on the large-path fixtures: the way
    profiles/pose_graph_pcg_vs_exact.json was measured"""
    rows = {}
    for name in rm.FIXTURES:
        if rm.dense(name):
            continue
        g, a = run(name, "exact")
        _, b = run(name, "pcg")
        dr, dt = m.pose_distance(a["poses"], b["poses"])
        rows[name] = dict(nodes=int(g["node_pose"].shape[0]), edges=int(len(g["edge_src"])), lm_iterations_exact=a["iterations"],
                          lm_iterations_pcg=b["iterations"], cg_iterations=b["cg_iterations"], rotation=dr, translation=dt,
                          error_exact=a["error"], error_pcg=b["error"])
    return rows


def large_tol(name):
    """the GPU bound of a large-path fixture under the PCG: 10 x its recorded gap and not below the converged bound of the
    large path, tests/test_pose_graph.py's rule"""
    rec = json.load(open(GOLDEN))["fixtures"][name]
    base = json.load(open(os.path.join(ROOT, "profiles", "pose_graph_pcg_vs_exact.json")))
    return max(10.0 * rec["rotation"], 10.0 * base["rotation"]), max(10.0 * rec["translation"], 10.0 * base["translation"])


def test_recorded_gaps_name_their_fixtures_and_hold():
    rec = json.load(open(GOLDEN))
    rows = measure_gaps()
    assert set(rec["fixtures"]) == set(rows)
    for name, row in rows.items():
        tr, tt = large_tol(name)
        print("%s: exact against PCG, rotation %.3e (recorded %.3e) translation %.3e (recorded %.3e)" % (
            name, row["rotation"], rec["fixtures"][name]["rotation"], row["translation"], rec["fixtures"][name]["translation"]))
        assert row["rotation"] <= tr and row["translation"] <= tt, name
        assert row["lm_iterations_exact"] == row["lm_iterations_pcg"] == rec["fixtures"][name]["lm_iterations_pcg"]


def test_loss_argument_rules_under_the_sanitizers(tmp_path):
    """tests/cpp/pg_loss_args_check.cpp over mvslam_amd/csrc/pg_host.hpp with -fsanitize=address,undefined.  A program of
    its own: nothing of it is loaded into python."""
    exe = str(tmp_path / "pg_loss_args_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mvslam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pg_loss_args_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip() == "ok"


def test_setter_and_stats_refuse_without_a_device():
    """a null context is refused before anything else is looked at, and the names are exported"""
    import ctypes as C

    from mvslam_amd import capi

    lib = capi.lib()
    assert lib.mvs_ctx_set_pose_graph_loss(None, capi.MVS_PG_LOSS_CAUCHY, 1.0, 0) == capi.MVS_ERR_INVALID_ARG
    chi2 = np.zeros(4)
    assert lib.mvs_pose_graph_edge_stats(None, None, None, chi2.ctypes.data_as(C.POINTER(C.c_double)), None) == capi.MVS_ERR_INVALID_ARG
    assert lib.mvs_seq_pose_graph_edge_stats(None, chi2.ctypes.data_as(C.POINTER(C.c_double)), None) == capi.MVS_ERR_INVALID_ARG
    for name in ("mvs_ctx_set_pose_graph_loss", "mvs_pose_graph_edge_stats", "mvs_seq_pose_graph_edge_stats"):
        assert name in capi.EXPORTS
    assert (capi.MVS_PG_LOSS_NONE, capi.MVS_PG_LOSS_HUBER, capi.MVS_PG_LOSS_CAUCHY, capi.MVS_PG_LOSS_LOOP_EDGES) == (0, 1, 2, -1)
    assert (rm.NONE, rm.HUBER, rm.CAUCHY) == (capi.MVS_PG_LOSS_NONE, capi.MVS_PG_LOSS_HUBER, capi.MVS_PG_LOSS_CAUCHY)
    assert capi.lib().mvs_abi_version() == 4
