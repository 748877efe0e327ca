"""CPU tests of the Sim(3) pose graphs: the layout of the public structs, the numpy model of the contract
(tests/sim3graph_model.py) against central differences, against the SE(3) model it must reduce to and against a fixture whose
optimum is known exactly, the lift rule of mvs_seq_optimize_pose_graph_sim3, and the measurement the GPU tolerance of the large
path rests on (profiles/sim3_graph_pcg_vs_exact.json)."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np

import posegraph_model as pm
import sim3graph_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "sim3_graph_pcg_vs_exact.json")


def test_struct_layouts_match_header():
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu\n", sizeof(mvs_sim3_graph), sizeof(mvs_sim3_graph_params));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(mvs_sim3_graph, n_edges), offsetof(mvs_sim3_graph, node_sim3),
         offsetof(mvs_sim3_graph, edge_src), offsetof(mvs_sim3_graph, edge_dst), offsetof(mvs_sim3_graph, edge_sim3),
         offsetof(mvs_sim3_graph, edge_cov), offsetof(mvs_sim3_graph, anchor_node));
  printf("%zu %zu %zu %zu\n", offsetof(mvs_sim3_graph_params, anchor_sigma), offsetof(mvs_sim3_graph_params, cg_rel_tol),
         offsetof(mvs_sim3_graph_params, cg_max_iterations), offsetof(mvs_sim3_graph_params, cg_chunk_iterations));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    G, P = capi.Sim3Graph, capi.Sim3GraphParams
    assert v[:2] == [C.sizeof(G), C.sizeof(P)]
    assert v[2:9] == [G.n_edges.offset, G.node_sim3.offset, G.edge_src.offset, G.edge_dst.offset, G.edge_sim3.offset,
                      G.edge_cov.offset, G.anchor_node.offset]
    assert v[9:13] == [P.anchor_sigma.offset, P.cg_rel_tol.offset, P.cg_max_iterations.offset, P.cg_chunk_iterations.offset]


def test_exports_and_default_params():
    from mvslam_amd import capi

    lib = capi.lib()
    for name in ("mvs_sim3_graph_params_default", "mvs_sim3_graph_optimize", "mvs_sim3_graph_optimize_batch",
                 "mvs_seq_optimize_pose_graph_sim3", "mvs_seq_download_pose_graph_sim3"):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
    p, q = capi.default_sim3_graph_params(), capi.default_pose_graph_params()
    assert tuple(p.anchor_sigma) == m.ANCHOR_SIGMA == (1e-4, 1e-4, 1e-4)
    assert (p.cg_rel_tol, p.cg_max_iterations, p.cg_chunk_iterations) == (q.cg_rel_tol, 0, 0) and p.cg_rel_tol == m.CG_REL_TOL
    for f in ("max_iterations", "lambda_initial", "lambda_factor", "lambda_upper", "rel_tol", "abs_tol"):
        assert getattr(p.lm, f) == getattr(q.lm, f) == m.LM_DEFAULT[f], f
    p = capi.default_sim3_graph_params(anchor_sigma=(0.1, 0.2, 0.3), cg_chunk_iterations=16, max_iterations=7)
    assert tuple(p.anchor_sigma) == (0.1, 0.2, 0.3) and p.cg_chunk_iterations == 16 and p.lm.max_iterations == 7


def _random_nodes(rng):
    """an edge and its two nodes, scales in [0.3, 3], the rotation of the error up to 2 rad"""
    Z = m.sim3(rng.normal(size=3), rng.normal(size=3), rng.uniform(0.3, 3.0))
    Ps = m.sim3(rng.normal(size=3) * 1.1, rng.normal(size=3), rng.uniform(0.3, 3.0))
    w = rng.normal(size=3)
    w *= rng.uniform(0.0, 2.0) / np.linalg.norm(w)
    Pd = m.compose(m.compose(Ps, Z), m.sim3(w, rng.normal(size=3) * 0.3, rng.uniform(0.3, 3.0) / (Ps[12] * Z[12])))
    return Z, Ps, Pd, w


def test_model_jacobians_match_central_differences():
    """the bound and the step of tests/test_pose_graph_host.py for the SE(3) edge: central differences with h = 1e-6 have a
    truncation error of about h^2 times the third derivative and a rounding error of about eps / h; 1e-8"""
    rng = np.random.default_rng(0)
    h, worst, smin, smax = 1e-6, 0.0, np.inf, 0.0
    for _ in range(40):
        Z, Ps, Pd, w = _random_nodes(rng)
        assert 0.3 <= Ps[12] <= 3.0 and 0.3 <= Pd[12] <= 3.0 and 0.3 <= Z[12] <= 3.0
        smin, smax = min(smin, Ps[12], Pd[12]), max(smax, Ps[12], Pd[12])
        e, Js, Jd = m.edge_error(Z, Ps, Pd, True)
        assert abs(np.linalg.norm(e[:3]) - np.linalg.norm(w)) < 1e-9
        for which, J in ((0, Js), (1, Jd)):
            for i in range(7):
                dx = np.zeros(7)
                dx[i] = h
                a, b = [Ps, Pd], [Ps, Pd]
                a[which], b[which] = m.retract(a[which], dx), m.retract(b[which], -dx)
                fd = (m.edge_error(Z, *a) - m.edge_error(Z, *b)) / (2 * h)
                worst = max(worst, float(np.abs(fd - J[:, i]).max()))
        # the prior between two nodes whose rotations differ by the same w (up to 2 rad, as the edge's error)
        Pp = m.compose(Ps, m.sim3(w, rng.normal(size=3) * 0.3, Pd[12] / Ps[12]))
        e, Ja = m.prior_error(Ps, Pp, True)
        assert abs(np.linalg.norm(e[:3]) - np.linalg.norm(w)) < 1e-9
        for i in range(7):
            dx = np.zeros(7)
            dx[i] = h
            fd = (m.prior_error(Ps, m.retract(Pp, dx)) - m.prior_error(Ps, m.retract(Pp, -dx))) / (2 * h)
            worst = max(worst, float(np.abs(fd - Ja[:, i]).max()))
    print("largest |central difference - Jacobian| %.3e, scales %.2f .. %.2f" % (worst, smin, smax))
    assert smin < 0.5 and smax > 2.0            # away from 1
    assert worst < 1e-8, worst


def test_model_reduces_to_the_se3_edge_exactly():
    rng = np.random.default_rng(1)
    for _ in range(40):
        Z, Ps, Pd, _ = _random_nodes(rng)
        Z[12] = Ps[12] = Pd[12] = 1.0
        e, Js, Jd = m.edge_error(Z, Ps, Pd, True)
        e6, Js6, Jd6 = pm.edge_error(Z[:12], Ps[:12], Pd[:12], True)
        assert e[6] == 0.0 and np.array_equal(e[:6], e6)
        assert np.array_equal(Js[:6, :6], Js6) and np.array_equal(Jd[:6, :6], Jd6)
        assert not Js[6, :6].any() and not Jd[6, :6].any() and not Jd[:6, 6].any() and not Js[:3, 6].any()
        p, J = m.prior_error(Ps, Pd, True)
        p6, J6 = pm.prior_error(Ps[:12], Pd[:12], True)
        assert np.array_equal(p[:6], p6) and np.array_equal(J[:6, :6], J6) and p[6] == 0.0
        dx = rng.normal(size=7) * 0.1
        dx[6] = 0.0
        assert np.array_equal(m.retract(Ps, dx)[:12], pm.retract(Ps[:12], dx[:6])) and m.retract(Ps, dx)[12] == 1.0


_RUNS = {}


def _run(name, solver):
    """the model's answer for a fixture, computed once per process and never modified"""
    if (name, solver) not in _RUNS:
        make = dict(m.DENSE_FIXTURES, **m.PCG_FIXTURES)[name]
        _RUNS[(name, solver)] = m.optimize(make(), solver=solver)
    return _RUNS[(name, solver)]


def test_exact_recovery_on_the_drift_ring_and_what_se3_leaves():
    g, truth, g6 = m.drift_ring()
    n = m.DRIFT_N
    assert truth.shape == (40, 13) and 1.9 < truth[-1, 12] / truth[0, 12] < 2.0
    assert list(zip(g["edge_src"].tolist(), g["edge_dst"].tolist())) == [(i, i + 1) for i in range(n - 1)] + [(n - 1, 0)]
    for k in range(n):                               # measurements are exactly Xs^-1 Xd of the truth
        assert np.abs(m.edge_error(g["edge_sim3"][k], truth[g["edge_src"][k]], truth[g["edge_dst"][k]])).max() < 1e-14
    assert np.array_equal(g["node_sim3"][0], truth[0])
    rot0, trans0, scale0 = m.pose_distance(g["node_sim3"], truth)
    assert trans0 > 0.05 and scale0 > 0.02            # the chain drifted, in position and in scale
    rec = {}
    for solver in ("exact", "pcg"):
        r = _run("drift_ring40", solver)
        rot, trans, scale = m.pose_distance(r["nodes"], truth)
        print("Sim(3) %s: error %.3e -> %.3e, to the truth: rotation %.3e translation %.3e log-scale %.3e" % (
            solver, r["error_initial"], r["error"], rot, trans, scale))
        assert r["ok"] and r["exit"] == "converged" and r["error"] <= 1e-16 * r["error_initial"]
        assert max(rot, trans, scale) <= 1e-8
        rec["sim3_" + solver] = dict(rotation=rot, translation=trans, log_scale=scale, error_initial=r["error_initial"],
                                     error=r["error"], iterations=r["iterations"])
    # the same rotations and translations as an SE(3) graph: it cannot repair the scale of the chain
    assert np.array_equal(g6["node_pose"], g["node_sim3"][:, :12]) and np.array_equal(g6["edge_pose"][:, :9], g["edge_sim3"][:, :9])
    r6 = pm.optimize(g6)
    rot6, trans6 = pm.pose_distance(r6["poses"], truth[:, :12])
    print("SE(3): error %.3e -> %.3e, to the truth: rotation %.3e translation %.3e" % (r6["error_initial"], r6["error"], rot6, trans6))
    assert r6["ok"] and r6["error"] > 0.0
    assert trans6 > rec["sim3_exact"]["translation"]
    rec["se3"] = dict(rotation=rot6, translation=trans6, error_initial=r6["error_initial"], error=r6["error"],
                      iterations=r6["iterations"])
    rec["initial"] = dict(rotation=rot0, translation=trans0, log_scale=scale0)
    _RUNS["drift_record"] = rec


def test_pcg_against_exact_solves_and_record_the_gap():
    """The number the GPU tolerance of the large path rests on, measured as tests/test_pose_graph_host.py measures the SE(3)
    one: the model with exact solves against the model with the block-Jacobi PCG at cg_rel_tol = 1e-10 on the large-path
    fixtures; the largest rotation angle, |t1 - t2| and |log s1 - log s2| go to profiles/sim3_graph_pcg_vs_exact.json, with the
    drift ring's gaps to its truth under Sim(3) and under SE(3)."""
    if "drift_record" not in _RUNS:
        test_exact_recovery_on_the_drift_ring_and_what_se3_leaves()
    rows, worst = {}, [0.0, 0.0, 0.0]
    for name, make in m.PCG_FIXTURES.items():
        g = make()
        a, b = _run(name, "exact"), _run(name, "pcg")
        assert a["ok"] and b["ok"] and b["cg_iterations"] > 0
        gap = m.pose_distance(a["nodes"], b["nodes"])
        rows[name] = dict(nodes=int(g["node_sim3"].shape[0]), edges=int(len(g["edge_src"])), lm_iterations_exact=a["iterations"],
                          lm_iterations_pcg=b["iterations"], cg_iterations=b["cg_iterations"], rotation=gap[0],
                          translation=gap[1], log_scale=gap[2], error_exact=a["error"], error_pcg=b["error"])
        worst = [max(w, x) for w, x in zip(worst, gap)]
    # a relative residual of 1e-10 in each linear solve cannot move a minimiser of nodes of size 1 .. 3 by more than 1e-6
    assert max(worst) < 1e-6, rows
    out = dict(what="numpy model of the Sim(3) graphs, exact solves against block-Jacobi (7 x 7) PCG at cg_rel_tol 1e-10: "
                    "largest node difference", cg_rel_tol=m.CG_REL_TOL, rotation=worst[0], translation=worst[1],
               log_scale=worst[2], fixtures=rows, drift_ring=_RUNS["drift_record"])
    with open(PROFILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def test_recorded_gaps_name_their_fixtures():
    rec = json.load(open(PROFILE))
    assert set(rec["fixtures"]) == set(m.PCG_FIXTURES)
    for w in ("rotation", "translation", "log_scale"):
        assert rec[w] == max(v[w] for v in rec["fixtures"].values()) > 0.0
    assert rec["fixtures"]["star70"]["nodes"] == 71 and rec["fixtures"]["ring17"]["nodes"] == 17
    assert rec["drift_ring"]["se3"]["translation"] > rec["drift_ring"]["sim3_exact"]["translation"]


def test_no_lm_decision_of_a_compared_fixture_is_marginal():
    """a run whose accept / reject or stop decision is a toss-up to rounding ends one Newton step earlier or later on the
    device, and the comparison at 1e-9 then says nothing (posegraph_model.DENSE_SIZE_SEED's comment)"""
    margins = {"triangle%d" % s: m.decision_margin(m.optimize(m.triangle(s))) for s in m.TRIANGLE_SEEDS}
    for name in m.DENSE_FIXTURES:
        margins[name] = m.decision_margin(_run(name, "exact"))
    for n in (2, 16):
        margins["ring%d" % n] = m.decision_margin(m.optimize(m.dense_ring(n)))
    for name in m.PCG_FIXTURES:
        margins[name + " (pcg)"] = m.decision_margin(_run(name, "pcg"))
    print({k: float("%.3g" % v) for k, v in margins.items()})
    assert len(set(m.TRIANGLE_SEEDS)) == 8
    assert min(margins.values()) >= m.DENSE_MARGIN, margins


def test_dense_fixtures_are_what_they_say():
    g = m.parallel16()
    pairs = list(zip(g["edge_src"].tolist(), g["edge_dst"].tolist()))
    assert len(pairs) == 272 > 256 and g["node_sim3"].shape[0] == 16 and pairs.count((3, 4)) == 2 and pairs.count((3, 5)) == 2
    assert len({tuple(z) for z in g["edge_sim3"]}) == 272                      # fresh noise: no measurement repeats
    g = m.all_pairs16()
    pairs = list(zip(g["edge_src"].tolist(), g["edge_dst"].tolist()))
    assert sorted(pairs) == sorted((s, d) for s in range(16) for d in range(16) if s != d)
    g = m.full_cov_graph()
    assert len(g["edge_src"]) == 9 and max(np.linalg.cond(c.reshape(7, 7)) for c in g["edge_cov"]) <= 1e6
    assert any(abs(c.reshape(7, 7)[6, 2]) > 1e-6 for c in g["edge_cov"])      # really full, the scale's row too
    g = m.anchor5()
    assert g["anchor"] == 5 and np.array_equal(g["node_sim3"][m.ANCHOR5_PERM], m.dense_ring(8)["node_sim3"])
    a, b = _run("anchor5", "exact"), m.optimize(m.dense_ring(8))
    assert max(m.pose_distance(a["nodes"][m.ANCHOR5_PERM], b["nodes"])) <= 1e-9
    s = m.star()
    assert s["node_sim3"].shape[0] == 71 and min(s["node_sim3"][:, 12]) < 0.6 and max(s["node_sim3"][:, 12]) > 1.8
    for seed in m.TRIANGLE_SEEDS:
        t = m.triangle(seed)
        loop = np.prod(t["edge_sim3"][:3, 12])                                   # the three steps ask for 1.331, the loop for 1
        r = m.optimize(t)
        assert abs(loop - 1.331) < 0.1 and t["edge_sim3"][3, 12] == 1.0 and r["ok"] and r["error"] > 1.0


def test_model_failures():
    assert m.optimize(m.disconnected())["ok"] == 0 and not m.connected(m.disconnected())
    assert m.optimize(m.indefinite(m.triangle(2), 1))["ok"] == 0
    assert m.optimize(m.indefinite(m.dense_ring(17), 3), solver="pcg")["ok"] == 0


def test_lift_rule():
    """lift(graph6, scale_sigma): copies and one multiply, and a covariance the 7 x 7 Cholesky test accepts"""
    g6 = pm.ring(9)
    E = len(g6["edge_src"])
    g6["edge_kind"] = np.array([k % 3 for k in range(E)], dtype=np.int32)
    sig = (0.03, 0.2, 0.007)
    g = m.lift(g6, sig)
    assert g["node_sim3"].shape == (9, 13) and g["edge_sim3"].shape == (E, 13) and g["edge_cov"].shape == (E, 49)
    assert np.array_equal(g["node_sim3"][:, :12], g6["node_pose"]) and np.all(g["node_sim3"][:, 12] == 1.0)
    assert np.array_equal(g["edge_sim3"][:, :12], g6["edge_pose"]) and np.all(g["edge_sim3"][:, 12] == 1.0)
    for k in range(E):
        c = g["edge_cov"][k].reshape(7, 7)
        assert np.array_equal(c[:6, :6], g6["edge_cov"][k].reshape(6, 6))
        assert not c[6, :6].any() and not c[:6, 6].any() and c[6, 6] == sig[k % 3] * sig[k % 3]
        assert m.chol7_ok(c)
    assert np.array_equal(g["edge_src"], g6["edge_src"]) and g["anchor"] == 0
    assert not m.chol7_ok(m.indefinite(g, 0)["edge_cov"][0])
    # with the scales tied down the lifted graph is the SE(3) graph: the same minimiser
    tight = m.lift(g6, (1e-6, 1e-6, 1e-6))
    a, b = m.optimize(tight), pm.optimize(g6)
    rot, trans = pm.pose_distance(a["nodes"][:, :12], b["poses"])
    assert a["ok"] and rot < 1e-6 and trans < 1e-6 and np.abs(np.log(a["nodes"][:, 12])).max() < 1e-6


def test_new_kernels_in_the_resource_digest():
    res = json.load(open(os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "S3DenseDev" in k or "S3LargeDev" in k or "S3LiftDev" in k}
    assert len(mine) >= 12 and sum("s3_dense_kernel" in k for k in mine) == 1
    for k, v in mine.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0, (k, v)
        assert v["static_lds_bytes"] <= 64 * 1024, (k, v)
    dense = [v for k, v in mine.items() if "s3_dense_kernel" in k][0]
    assert 50624 < dense["static_lds_bytes"] <= 65536
    assert any("pg_dense_kernel" in k for k in res) and any("pg_gather_kernel" in k for k in res)   # the old entries stay
