"""CPU tests of the direct LM step of the pose graphs' large path: the numpy model of the
block-scaled skyline solve (tests/pg_direct_model.py) against the model with numpy's dense Cholesky, the recorded gap the GPU
tolerance of tests/test_pg_direct.py rests on (profiles/pose_graph_direct_vs_exact.json, written by
tools/pose_graph_direct_accuracy.py), the host planning under the sanitizers, and what the switch refuses without a device."""
import ctypes as C
import importlib.util
import json
import os
import subprocess

import numpy as np

import pg_direct_model as dm
import pg_marginals_model as pgm
import posegraph_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_TOL = 1e-9           # tests/test_pose_graph.py: the bound of the dense path


def _tool():
    spec = importlib.util.spec_from_file_location("pose_graph_direct_accuracy",
                                                  os.path.join(ROOT, "tools", "pose_graph_direct_accuracy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _recorded():
    return json.load(open(os.path.join(ROOT, "profiles", "pose_graph_direct_vs_exact.json")))


def test_one_scaled_solve_against_numpy():
    """(H + lambda I) x = -g at the initial values: the scaled skyline solve against numpy.linalg.solve.  Both are backward
    stable, so they differ by about cond * eps relative to |x|; the scaled matrix of these fixtures has a condition number
    below 1e7 (asserted), which leaves 1e-8 a factor of ten."""
    for make in (lambda: pm.ring(17), pgm.chain40, pgm.FIXTURES["ring24_relabelled"], pm.star):
        g = make()
        A, b = dm.system(g)
        first, _, _ = pgm.graph_envelope(g)
        As, _, _ = dm.scaled_system(A, b, first)
        assert np.linalg.cond(As) < 1e7
        info = {}
        x, ref = dm.solve(A, b, first, info), np.linalg.solve(A, b)
        assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
        assert 0.0 < info["min_pivot"] <= 1.0           # unit diagonal blocks: no pivot of the scaled matrix exceeds 1
        for i in range(len(first)):                      # A~_ii = I exactly
            assert np.array_equal(As[6 * i:6 * i + 6, 6 * i:6 * i + 6], np.eye(6))


def test_direct_against_exact_and_the_recorded_gap():
    """every fixture of the direct path: the two models take the same decisions and end within the recorded gap, and a fresh
    measurement does not exceed what is committed (the figures are deterministic on one machine; 4 x leaves room for another
    BLAS's summation order, far below the 1e-9 the GPU tests use)"""
    rec, fresh = _recorded(), _tool().measure()
    assert set(rec["fixtures"]) == set(fresh["fixtures"])
    for name, row in fresh["fixtures"].items():
        print(name, row["rotation"], row["translation"], row["iterations_direct"], row["rejected_direct"])
        assert (row["iterations_direct"], row["rejected_direct"], row["exit_direct"]) == \
               (row["iterations_exact"], row["rejected_exact"], row["exit_exact"]), name
        # relatively, as the GPU tests compare it; an error of rounding size (star70 fits its measurements exactly) absolutely
        assert abs(row["error_direct"] - row["error_exact"]) <= 1e-9 * (row["error_exact"] if row["error_exact"] > 1e-20 else 1.0), name
    assert rec["rotation"] == max(v["rotation"] for v in rec["fixtures"].values())
    assert rec["translation"] == max(v["translation"] for v in rec["fixtures"].values())
    assert fresh["rotation"] <= max(4.0 * rec["rotation"], 1e-13) and fresh["translation"] <= max(4.0 * rec["translation"], 1e-13)
    assert 10.0 * rec["rotation"] < DENSE_TOL and 10.0 * rec["translation"] < DENSE_TOL   # the GPU bound is the dense path's
    assert fresh["fixtures"]["far_off20"]["rejected_direct"] >= 1
    assert fresh["fixtures"]["lambda_upper20"]["exit_direct"] == "lambda_upper"


def test_a_failed_pivot_is_a_rejected_step():
    """lambda = 0 on a graph without an anchor term worth the name is singular to rounding: the solve raises, the step counts
    as rejected, lambda grows and no stall test is made -- as under solver="exact" """
    g = pm.ring(17)
    kw = dict(lm=dict(lambda_initial=0.0, max_iterations=3), anchor_sigma=(1e160, 1e160))
    a, b = pm.optimize(g, **kw), dm.optimize_direct(g, **kw)
    assert [t["solved"] for t in a["trace"]] == [t["solved"] for t in b["trace"]]
    assert not b["trace"][0]["solved"] and b["rejected_steps"] == 3 and b["exit"] == "max_iterations"
    assert b["poses"].tobytes() == g["node_pose"].tobytes()


def test_model_failures_and_limits():
    assert dm.optimize_direct(pm.disconnected())["ok"] == 0
    assert dm.optimize_direct(pm.indefinite(pm.ring(17), 3))["ok"] == 0
    assert dm.optimize_direct(pm.overflowing(pm.ring(17)))["ok"] == 0
    r = dm.optimize_direct(pm.ring(17), lm=dict(max_iterations=0))
    assert r["ok"] == 1 and r["iterations"] == 0 and r["error"] == r["error_initial"]


def test_host_planning_under_the_sanitizers(tmp_path):
    """tests/cpp/pg_direct_plan_check.cpp over mvslam_amd/csrc/pg_envelope.hpp's direct_plan with -fsanitize=address,undefined.
    A program of its own: nothing of it is loaded into python."""
    exe = str(tmp_path / "pg_direct_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mvslam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pg_direct_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip() == "ok"


def test_switch_refuses_a_null_context():
    from mvslam_amd import capi

    assert (capi.MVS_PG_SOLVER_PCG, capi.MVS_PG_SOLVER_DIRECT) == (0, 1)
    assert capi.lib().mvs_ctx_set_pose_graph_solver(C.c_void_p(None), 1) == capi.MVS_ERR_INVALID_ARG
    info = np.zeros(1, dtype=capi.POSE_GRAPH_DIRECT_INFO_DTYPE)
    assert capi.lib().mvs_ctx_pose_graph_direct_info(C.c_void_p(None), info.ctypes.data_as(C.c_void_p)) == capi.MVS_ERR_INVALID_ARG
    assert capi.POSE_GRAPH_DIRECT_INFO_DTYPE.itemsize == 32
    header = open(os.path.join(ROOT, "include", "mvslam_hip.h")).read()
    assert "#define MVS_PG_SOLVER_PCG 0" in header and "#define MVS_PG_SOLVER_DIRECT 1" in header
