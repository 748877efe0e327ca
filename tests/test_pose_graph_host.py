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
    out = dict(what="numpy model, exact solves against block-Jacobi PCG at cg_rel_tol 1e-10: largest pose difference",
               cg_rel_tol=m.CG_REL_TOL, rotation=rot, translation=trans, fixtures=rows)
    with open(os.path.join(ROOT, "profiles", "pose_graph_pcg_vs_exact.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


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
