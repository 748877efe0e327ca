"""CPU tests of the pose-graph back end: the layout of its public structs, the numpy model of its contract
(tests/posegraph_model.py) against itself and against the two scenarios of the reference's test/test-graph.cpp, the argument
errors the library returns before it touches a device, and the measurement the GPU tolerance of the large path rests on
(profiles/pose_graph_pcg_vs_exact.json)."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import posegraph_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_match_header():
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(mvs_pose_graph), sizeof(mvs_pose_graph_params), sizeof(mvs_pose_graph_result));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(mvs_pose_graph, n_edges), offsetof(mvs_pose_graph, node_pose),
         offsetof(mvs_pose_graph, edge_src), offsetof(mvs_pose_graph, edge_dst), offsetof(mvs_pose_graph, edge_pose),
         offsetof(mvs_pose_graph, edge_cov), offsetof(mvs_pose_graph, anchor_node));
  printf("%zu %zu %zu\n", offsetof(mvs_pose_graph_params, anchor_sigma), offsetof(mvs_pose_graph_params, cg_rel_tol),
         offsetof(mvs_pose_graph_params, cg_max_iterations));
  printf("%zu %zu %zu %zu %zu\n", offsetof(mvs_pose_graph_result, iterations), offsetof(mvs_pose_graph_result, cg_iterations),
         offsetof(mvs_pose_graph_result, rejected_steps), offsetof(mvs_pose_graph_result, error_initial),
         offsetof(mvs_pose_graph_result, error));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    G, P, R = capi.PoseGraph, capi.PoseGraphParams, capi.PoseGraphResult
    assert v[:3] == [C.sizeof(G), C.sizeof(P), C.sizeof(R)]
    assert v[2] == capi.POSE_GRAPH_RESULT_DTYPE.itemsize == 32
    assert v[3:10] == [G.n_edges.offset, G.node_pose.offset, G.edge_src.offset, G.edge_dst.offset, G.edge_pose.offset,
                       G.edge_cov.offset, G.anchor_node.offset]
    assert v[10:13] == [P.anchor_sigma.offset, P.cg_rel_tol.offset, P.cg_max_iterations.offset]
    assert v[13:18] == [R.iterations.offset, R.cg_iterations.offset, R.rejected_steps.offset, R.error_initial.offset,
                        R.error.offset]
    assert [capi.POSE_GRAPH_RESULT_DTYPE.fields[k][1] for k in ("iterations", "cg_iterations", "rejected_steps",
                                                                "error_initial", "error")] == v[13:18]


def test_default_params():
    from mvslam_amd import capi

    p = capi.default_pose_graph_params()
    r = capi.default_refine_params()
    assert (p.lm.max_iterations, p.lm.lambda_initial, p.lm.lambda_factor, p.lm.lambda_upper, p.lm.rel_tol, p.lm.abs_tol) == \
           (r.max_iterations, r.lambda_initial, r.lambda_factor, r.lambda_upper, r.rel_tol, r.abs_tol)
    assert tuple(p.anchor_sigma) == (1e-4, 1e-4) and p.cg_rel_tol == 1e-10 and p.cg_max_iterations == 0
    assert (p.lm.max_iterations, p.lm.lambda_initial, p.lm.rel_tol) == \
           (m.LM_DEFAULT["max_iterations"], m.LM_DEFAULT["lambda_initial"], m.LM_DEFAULT["rel_tol"])


def test_model_jacobians_match_central_differences():
    """random edges, rotations of the error up to 2 rad; central differences with h = 1e-6 have a truncation error of about
    h^2 times the third derivative and a rounding error of about eps / h: 1e-8 leaves a factor of 30 over what they give"""
    rng = np.random.default_rng(0)
    h, worst = 1e-6, 0.0
    for _ in range(40):
        Z = m.se3(rng.normal(size=3), rng.normal(size=3))
        Ps = m.se3(rng.normal(size=3) * 1.1, rng.normal(size=3))
        w = rng.normal(size=3)
        w *= rng.uniform(0.0, 2.0) / np.linalg.norm(w)
        Pd = m.compose(m.compose(Ps, Z), m.se3(w, rng.normal(size=3) * 0.3))
        e, Js, Jd = m.edge_error(Z, Ps, Pd, True)
        assert abs(np.linalg.norm(e[:3]) - np.linalg.norm(w)) < 1e-9
        for which, J in ((0, Js), (1, Jd)):
            for i in range(6):
                dx = np.zeros(6)
                dx[i] = h
                a, b = [Ps, Pd], [Ps, Pd]
                a[which], b[which] = m.retract(a[which], dx), m.retract(b[which], -dx)
                fd = (m.edge_error(Z, *a) - m.edge_error(Z, *b)) / (2 * h)
                worst = max(worst, float(np.abs(fd - J[:, i]).max()))
        e, Ja = m.prior_error(Ps, Pd, True)
        for i in range(6):
            dx = np.zeros(6)
            dx[i] = h
            fd = (m.prior_error(Ps, m.retract(Pd, dx)) - m.prior_error(Ps, m.retract(Pd, -dx))) / (2 * h)
            worst = max(worst, float(np.abs(fd - Ja[:, i]).max()))
    assert worst < 1e-8, worst


def test_model_reproduces_the_reference_trivial_scenario():
    g, truth = m.trivial()
    r = m.optimize(g)
    rot, trans = m.pose_distance(r["poses"], truth)
    assert r["ok"] and rot < 0.01 and trans < 0.01, (rot, trans)          # test-graph.cpp `trivial`: TOLERANCE 0.01
    assert m.pose_distance(g["node_pose"], truth)[1] > 0.1                 # the guess was off


@pytest.mark.parametrize("seed", range(8))
def test_model_reproduces_the_reference_triangle_scenario(seed):
    g, truth = m.triangle(seed)
    r = m.optimize(g)
    rot, trans = m.pose_distance(r["poses"], truth)
    assert r["ok"] and rot < 0.03 and trans < 0.03, (rot, trans)          # `planar_triangle`: TOLERANCE 0.03
    assert r["error"] < r["error_initial"]


def test_model_rejects_steps_on_the_far_off_fixtures():
    for n in m.FAR_OFF:
        r = m.optimize(m.far_off(n))
        assert r["ok"] and r["rejected_steps"] >= 1 and r["iterations"] < m.LM_DEFAULT["max_iterations"], (n, r)


def test_model_failures():
    assert m.optimize(m.disconnected())["ok"] == 0
    g, _ = m.triangle(0)
    g["edge_cov"][1] = np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]).reshape(36)
    assert m.optimize(g)["ok"] == 0


def test_full_covariances_are_well_conditioned():
    g = m.full_cov_graph()
    assert len(g["edge_src"]) == 9 and g["node_pose"].shape[0] == 6
    assert max(np.linalg.cond(c.reshape(6, 6)) for c in g["edge_cov"]) <= 1e6
    assert any(abs(c.reshape(6, 6)[0, 4]) > 1e-6 for c in g["edge_cov"])    # really full


def test_pcg_against_exact_solves_and_record_the_gap():
    """The number the GPU tolerance of the large path rests on: the model with exact solves against the model with the
    block-Jacobi PCG at cg_rel_tol = 1e-10 on the large-path fixtures; the largest rotation angle of R1^T R2 and the largest
    |t1 - t2| go to profiles/pose_graph_pcg_vs_exact.json.  Here: the two agree where the tolerance of the linear solve says
    they must -- a relative residual of 1e-10 in each step cannot move a minimiser of poses of size 1..3 by more than 1e-6."""
    rows, rot, trans = {}, 0.0, 0.0
    for name, make in m.PCG_FIXTURES.items():
        g = make()
        a, b = m.optimize(g), m.optimize(g, solver="pcg", cg_rel_tol=m.CG_REL_TOL)
        assert a["ok"] and b["ok"]
        dr, dt = m.pose_distance(a["poses"], b["poses"])
        rows[name] = dict(nodes=int(g["node_pose"].shape[0]), edges=int(len(g["edge_src"])), lm_iterations_exact=a["iterations"],
                          lm_iterations_pcg=b["iterations"], cg_iterations=b["cg_iterations"], rotation=dr, translation=dt,
                          error_exact=a["error"], error_pcg=b["error"])
        rot, trans = max(rot, dr), max(trans, dt)
    assert rot < 1e-6 and trans < 1e-6, rows
    # runs away from the default parameters: the same measurement, each under its own name
    runs = {}
    for name, (make, kw) in m.PARAM_RUNS.items():
        g = make()
        a, b = m.optimize(g, **kw), m.optimize(g, solver="pcg", **kw)
        assert a["ok"] and b["ok"] and a["exit"] == b["exit"], name
        dr, dt = m.pose_distance(a["poses"], b["poses"])
        runs[name] = dict(parameters=_plain(kw), nodes=int(g["node_pose"].shape[0]), lm_iterations_pcg=b["iterations"],
                          rejected_pcg=b["rejected_steps"], cg_iterations=b["cg_iterations"], exit=b["exit"], rotation=dr,
                          translation=dt)
        assert dr < 1e-6 and dt < 1e-6, runs
    # a truncated CG: the exact solve says nothing about it.  The same recursion with H applied as the dense product and as
    # the device applies it (edge-wise A^T (A p) + prior block + lambda p): how far two legal summation orders drift apart.
    g = m.ring(17)
    a, b = m.optimize(g, solver="pcg", **m.TRUNCATED), m.optimize(g, solver="pcg", h_apply="edges", **m.TRUNCATED)
    dr, dt = m.pose_distance(a["poses"], b["poses"])
    assert a["trace"][0]["cg_status"] == b["trace"][0]["cg_status"] == 0 and dr < 1e-12 and dt < 1e-12
    truncated = dict(fixture="ring17", parameters=_plain(m.TRUNCATED), rotation=dr, translation=dt,
                     what="PCG with H p as a dense product against H p edge-wise, both stopped after 3 CG iterations")
    # first-order optimality: |J^T r| at the model's own answer over |J^T r| at the initial values
    grad = {}
    for name, (make, solver) in m.GRADIENT_FIXTURES.items():
        g = make()
        r = m.optimize(g, solver=solver)
        ratio = float(np.linalg.norm(m.gradient(g, r["poses"])) / np.linalg.norm(m.gradient(g, g["node_pose"])))
        assert ratio < 1e-8, (name, ratio)        # the answer is a stationary point to what rel_tol = 1e-12 leaves
        grad[name] = dict(solver=solver, ratio=ratio)
    out = dict(what="numpy model, exact solves against block-Jacobi PCG at cg_rel_tol 1e-10: largest pose difference",
               cg_rel_tol=m.CG_REL_TOL, rotation=rot, translation=trans, fixtures=rows, parameter_runs=runs,
               truncated_cg=truncated, gradient_ratio=grad)
    with open(os.path.join(ROOT, "profiles", "pose_graph_pcg_vs_exact.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def _plain(kw):
    return {k: (dict(v) if isinstance(v, dict) else list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}


def _recorded():
    return json.load(open(os.path.join(ROOT, "profiles", "pose_graph_pcg_vs_exact.json")))


DENSE_TOL = 1e-9           # tests/test_pose_graph.py: the bound of the dense path


def _pcg_tol():
    rec = _recorded()
    return 10.0 * rec["rotation"], 10.0 * rec["translation"]


def _run_tol(*names):
    """10 x the recorded exact-against-PCG gap of the named parameter runs, and not below the converged bound"""
    rec = _recorded()["parameter_runs"]
    return tuple(max(10.0 * max(rec[k][w] for k in names), t) for w, t in zip(("rotation", "translation"), _pcg_tol()))


def _within(A, B, tol):
    rot, trans = m.pose_distance(A, B)
    return rot <= tol[0] and trans <= tol[1]


def test_recorded_gaps_name_their_fixtures():
    rec = _recorded()
    assert set(rec["fixtures"]) == set(m.PCG_FIXTURES) and set(rec["parameter_runs"]) == set(m.PARAM_RUNS)
    assert rec["fixtures"]["ring257"]["nodes"] == 257                      # the large path's strided loops: a second trip
    assert rec["rotation"] == max(v["rotation"] for v in rec["fixtures"].values())
    assert rec["translation"] == max(v["translation"] for v in rec["fixtures"].values())
    assert set(rec["gradient_ratio"]) == set(m.GRADIENT_FIXTURES) and rec["truncated_cg"]["fixture"] == "ring17"


def test_case1_relabelled_rings_and_the_orphan():
    for name, (n, perm) in m.PERMUTATIONS.items():
        g, p = m.ring(n), m.permuted_ring(name)
        assert p["anchor"] == perm[0] == int(name.split("_a")[1]) and p["anchor"] != 0 and m.connected(p)
        assert np.array_equal(p["node_pose"][perm], g["node_pose"])
        assert np.array_equal(np.asarray(perm)[g["edge_src"]], p["edge_src"])
        solver, tol = ("exact", (DENSE_TOL, DENSE_TOL)) if n <= 16 else ("pcg", _pcg_tol())
        a, b = m.optimize(g, solver=solver), m.optimize(p, solver=solver)
        assert a["ok"] and b["ok"] and _within(b["poses"][perm], a["poses"], tol), name
    o = m.orphan_node0()
    assert o["anchor"] == 1 and 0 not in set(o["edge_src"]) | set(o["edge_dst"])
    assert m.connected(dict(o, node_pose=o["node_pose"][1:], edge_src=o["edge_src"] - 1, edge_dst=o["edge_dst"] - 1, anchor=0))
    assert not m.connected(o) and m.optimize(o)["ok"] == 0


def test_case2_model_is_invariant_under_a_rigid_motion():
    R, t = m.split(m.RIGID_T)
    assert abs(np.linalg.norm(m.so3_log(R)) - 2.0) < 1e-12 and 10.0 < np.linalg.norm(t) < 20.0
    assert np.abs(m.so3_log(R) / 2.0).min() > 0.4                         # a skew axis: no component is small
    for g, solver, tol in ((m.full_cov_graph(), "exact", (DENSE_TOL, DENSE_TOL)), (m.ring(17), "pcg", _run_tol("ring17_moved"))):
        a, b = m.optimize(g, solver=solver), m.optimize(m.moved(g), solver=solver)
        assert abs(a["error_initial"] - b["error_initial"]) <= 1e-9 * a["error_initial"]
        rot, trans = m.pose_distance(b["poses"], m.moved_poses(a["poses"]))
        print("model, rigid motion (%s): rotation %.3e translation %.3e" % (solver, rot, trans))
        assert rot <= tol[0] and trans <= tol[1]


def test_case4_loose_anchor_moves_and_the_two_sigmas_differ():
    for n, solver in ((8, "exact"), (17, "pcg")):
        g = m.loose_anchor(n)
        a = m.optimize(g, lm=m.LOOSE_LM, anchor_sigma=m.LOOSE_SIGMA, solver=solver)
        b = m.optimize(g, lm=m.LOOSE_LM, anchor_sigma=m.LOOSE_SIGMA[::-1], solver=solver)
        rot, trans = m.pose_distance(a["poses"][0], g["node_pose"][0])
        assert rot > 1e-3 and trans > 1e-3, (n, rot, trans)                # the anchor moved
        tol = (DENSE_TOL, DENSE_TOL) if n == 8 else _run_tol("loose_anchor17", "loose_anchor17_swapped")
        rot, trans = m.pose_distance(a["poses"], b["poses"])
        assert rot > 1e3 * tol[0] and trans > 1e3 * tol[1], (n, rot, trans, tol)   # w_anchor[k / 3] is observable


def test_case5_exits_of_the_model():
    for g, solver in ((m.ring(8), "exact"), (m.ring(17), "pcg")):
        r = m.optimize(g, lm=dict(max_iterations=0), solver=solver)
        assert r["ok"] == 1 and r["iterations"] == 0 and r["error"] == r["error_initial"] and r["exit"] == "max_iterations"
        assert r["poses"].tobytes() == g["node_pose"].tobytes()
    g = m.far_off(8)
    r = m.optimize(g, lm=dict(max_iterations=2))
    assert r["exit"] == "max_iterations" and r["iterations"] == 2 and m.decision_margin(r) >= 1e3
    r = m.optimize(g, lm=m.LAMBDA_UPPER8)
    assert r["exit"] == "lambda_upper" and r["rejected_steps"] >= 1 and r["iterations"] > r["rejected_steps"]
    assert m.decision_margin(r, m.LAMBDA_UPPER8) >= 1e3
    make, kw = m.PARAM_RUNS["lambda_upper20"]
    r = m.optimize(make(), solver="pcg", **kw)
    assert r["exit"] == "lambda_upper" and r["rejected_steps"] >= 1 and r["iterations"] > r["rejected_steps"]
    r = m.optimize(m.ring(17), solver="pcg", h_apply="edges", **m.TRUNCATED)
    t = r["trace"][0]
    assert (t["cg"], t["cg_status"], t["solved"], t["accepted"], r["iterations"]) == (3, 0, True, True, 1)
    a, b = m.optimize(m.ring(17), solver="pcg"), m.optimize(m.ring(17), solver="pcg", cg_rel_tol=1e-4)
    assert b["ok"] and b["exit"] == "converged" and b["cg_iterations"] < a["cg_iterations"]


def test_case6_dense_stride_and_parallel_edges():
    g = m.all_pairs16()
    pairs = list(zip(g["edge_src"].tolist(), g["edge_dst"].tolist()))
    assert len(pairs) == 272 > 256 and g["node_pose"].shape[0] == 16
    for a in range(16):
        for b in range(a + 1, 16):
            assert pairs.count((a, b)) >= 1 and pairs.count((b, a)) >= 1 and pairs.count((a, b)) + pairs.count((b, a)) >= 2
    assert pairs.count((3, 4)) == 2 and pairs.count((3, 5)) == 2            # ring and chord: measured twice one way
    assert len({tuple(z) for z in g["edge_pose"]}) == 272                   # fresh noise: no measurement repeats
    p = m.parallel3()
    assert p["node_pose"].shape[0] == 3 and len(p["edge_src"]) == 5
    for x in (g, p):
        r = m.optimize(x)
        assert r["ok"] and r["exit"] == "converged" and r["error"] < r["error_initial"]
    assert m.decision_margin(m.optimize(g)) >= m.DENSE_MARGIN


def test_case7_every_dense_size():
    for n in range(1, 17):
        g = m.dense_size(n)
        assert g["node_pose"].shape[0] == n and m.connected(g)
        assert len(g["edge_src"]) == (0 if n == 1 else n if n < 4 else 2 * n)
        r = m.optimize(g)
        assert r["ok"] and r["exit"] == "converged" and (n == 1 or m.decision_margin(r) >= m.DENSE_MARGIN), n
    r = m.optimize(m.dense_size(1))
    assert r["iterations"] == 1 and r["error"] == 0.0 and r["poses"].tobytes() == m.dense_size(1)["node_pose"].tobytes()


def test_case9_the_partly_failing_batch():
    good = [m.ring(40), m.ring(17), m.trivial()[0]]
    bad = [m.indefinite(m.triangle(0)[0], 1), m.disconnected(), m.indefinite(m.ring(17), 3)]
    assert all(m.optimize(g)["ok"] == 1 for g in good) and all(m.optimize(g)["ok"] == 0 for g in bad)
    assert m.connected(bad[0]) and m.connected(bad[2]) and not m.connected(bad[1])


def test_case10_near_pi_the_model_reaches_the_truth():
    g, truth = m.near_pi_pair()
    e = m.edge_error(g["edge_pose"][0], g["node_pose"][0], g["node_pose"][1])
    assert 3.0 < np.linalg.norm(e[:3]) < np.pi                              # c < 0 in so3_log, sin(th) small in so3_jrinv
    r = m.optimize(g)
    rot, trans = m.pose_distance(r["poses"], truth)
    assert r["ok"] and rot < 1e-6 and trans < 1e-6 and m.decision_margin(r) >= 1e3, (rot, trans)
    g, truth = m.near_pi_ring()
    e = m.prior_error(truth[6], g["node_pose"][6])
    assert abs(np.linalg.norm(e[:3]) - m.NEAR_PI) < 1e-9
    for solver in ("exact", "pcg"):
        r = m.optimize(g, solver=solver)
        rot, trans = m.pose_distance(r["poses"], truth)
        assert r["ok"] and r["rejected_steps"] >= 1 and rot < 1e-6 and trans < 1e-6, (solver, rot, trans)


def test_case11_finite_input_whose_cost_overflows():
    for g in (m.overflowing(m.triangle(0)[0]), m.overflowing(m.ring(17))):
        assert np.all(np.isfinite(g["node_pose"])) and m.connected(g)
        assert m.optimize(g)["ok"] == 0


def test_host_logic_under_the_sanitizers(tmp_path):
    """tests/cpp/pg_host_check.cpp over mvslam_amd/csrc/pg_host.hpp: N = 1 with no edges, a chain, two components, duplicate
    edges in both orientations, the 4096-node hub, endpoints out of range, the CSR list against a brute-force one and
    all_finite, with -fsanitize=address,undefined.  A program of its own: nothing of it is loaded into python."""
    exe = str(tmp_path / "pg_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mvslam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pg_host_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip() == "ok"


REF = "/root/reference/source"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not present on this machine")
def test_replacement_graph_unit_parses_against_the_reference_headers():
    """integration/source/back-end/graph.cpp through the check tests/test_integration_syntax.py runs on its siblings in
    vision/: g++ -fsyntax-only against the reference's own headers, so a member the reference's classes do not declare or a
    signature that differs is a hard error.  The file must leave BackEndTypes::generate_*_id to back-end/data-type.cpp,
    which stays on the reference's link line: defining them here would be a duplicate definition there."""
    tu = os.path.join(ROOT, "integration", "source", "back-end", "graph.cpp")
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + REF, "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration", "source", "vision"), tu],
                       capture_output=True, text=True, cwd=os.path.dirname(tu), timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    text = open(tu).read()
    assert not re.search(r"BackEndTypes::generate_\w+\(\)\s*\{", text)       # used, never defined
    # every member of the two classes the reference declares (print included) is defined, with the reference's signature
    for member in ("Graph::Graph(", "Graph::~Graph(", "Graph::add_pose_node(", "Graph::add_transformation_edge(",
                   "Graph::has_node(", "Graph::has_edge(", "Graph::get_pose_node_value(", "Graph::get_all_pose_node_value(",
                   "Graph::reconcile_with(", "Graph::get_id(", "Graph::get_origin_node_id(", "Graph::print(",
                   "GraphOptimizer::GraphOptimizer(", "GraphOptimizer::~GraphOptimizer(", "GraphOptimizer::optimize(",
                   "GraphOptimizer::update_graph("):
        assert member in text, member


def _call(graph_fields, params=None, ctx=C.c_void_p(None), result=True, poses=True):
    """mvs_pose_graph_optimize with a null context by default: the argument checks come first"""
    from mvslam_amd import capi

    g = capi.PoseGraph(**graph_fields)
    p = params or capi.default_pose_graph_params()
    res = capi.PoseGraphResult()
    out = np.zeros((max(int(g.n_nodes), 1), 12))
    return capi.lib().mvs_pose_graph_optimize(ctx, C.byref(g), C.byref(p), C.byref(res) if result else None,
                                              out.ctypes.data_as(C.POINTER(C.c_double)) if poses else None)


def test_null_arguments_are_refused_without_a_device():
    from mvslam_amd import capi

    g, _ = m.trivial()
    keep = [g["node_pose"], g["edge_src"], g["edge_dst"], g["edge_pose"], g["edge_cov"]]
    f = dict(n_nodes=2, n_edges=1, node_pose=capi._ptr(keep[0], C.c_double), edge_src=capi._ptr(keep[1], C.c_int32),
             edge_dst=capi._ptr(keep[2], C.c_int32), edge_pose=capi._ptr(keep[3], C.c_double),
             edge_cov=capi._ptr(keep[4], C.c_double), anchor_node=0)
    assert _call(f) == capi.MVS_ERR_INVALID_ARG          # no context
