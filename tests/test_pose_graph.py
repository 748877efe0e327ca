"""GPU tests of the pose-graph back end (mvs_pose_graph_optimize, posegraph.hip) against the numpy model of its contract
(tests/posegraph_model.py).

Tolerances, device against model.  Dense path (N <= 16): both sides solve exactly and differ in libm and summation order;
the bound is the project's bound for GPU <-> oracle refinement parity, 1e-9 on the pose (README.md).  Large path: 10 x the
model's own PCG-against-exact gap, measured on the CPU by tests/test_pose_graph_host.py and committed in
profiles/pose_graph_pcg_vs_exact.json.  The final error is compared relatively with the same bounds.  Nothing here is derived
from what the device returns."""
import json
import os

import numpy as np
import pytest

import posegraph_model as m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_TOL = 1e-9
SENTINEL = -12345.678


def _pcg_tol():
    rec = json.load(open(os.path.join(ROOT, "profiles", "pose_graph_pcg_vs_exact.json")))
    return 10.0 * rec["rotation"], 10.0 * rec["translation"]


@pytest.fixture(scope="module")
def ctx():
    from mvslam_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


_MODEL = {}


def model(name, make, **kw):
    """the model's answer for a fixture, computed once per process and never modified"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _MODEL:
        g = make()
        _MODEL[key] = (g, m.optimize(g, **kw))
    return _MODEL[key]


def check(res, poses, ref, tol_rot, tol_trans, what=""):
    rot, trans = m.pose_distance(poses, ref["poses"])
    rel = abs(res["error"] - ref["error"]) / max(abs(ref["error"]), 1e-300) if ref["error"] > 1e-20 else abs(res["error"])
    print("%s: rotation %.3e translation %.3e error %.17g (model %.17g) iterations %d/%d cg %d rejected %d/%d" % (
        what, rot, trans, res["error"], ref["error"], res["iterations"], ref["iterations"], res["cg_iterations"],
        res["rejected_steps"], ref["rejected_steps"]))
    assert res["ok"] == 1 and ref["ok"] == 1
    assert rot <= tol_rot and trans <= tol_trans, (what, rot, trans)
    assert rel <= max(tol_rot, tol_trans), (what, res["error"], ref["error"])
    assert abs(res["error_initial"] - ref["error_initial"]) <= 1e-9 * max(1.0, ref["error_initial"])


def test_trivial_two_nodes(ctx):
    from mvslam_amd import capi

    g, ref = model("trivial", lambda: m.trivial()[0])
    before = {k: np.array(v, copy=True) for k, v in g.items() if isinstance(v, np.ndarray)}
    st, res, poses = ctx.pose_graph_optimize(g)
    assert st == capi.MVS_OK and res["cg_iterations"] == 0
    check(res, poses, ref, DENSE_TOL, DENSE_TOL, "trivial")
    assert m.pose_distance(poses, m.trivial()[1])[1] < 0.01
    for k, v in before.items():
        assert np.array_equal(g[k], v), k


def test_triangle_single_and_batch(ctx):
    from mvslam_amd import capi

    graphs, single = [], []
    for seed in range(8):
        g, ref = model("triangle%d" % seed, lambda: m.triangle(seed)[0])
        st, res, poses = ctx.pose_graph_optimize(g)
        assert st == capi.MVS_OK
        check(res, poses, ref, DENSE_TOL, DENSE_TOL, "triangle %d" % seed)
        rot, trans = m.pose_distance(poses, m.triangle(seed)[1])
        assert rot < 0.03 and trans < 0.03
        graphs.append(g)
        single.append((res.tobytes(), poses.tobytes()))
    st, res, poses = ctx.pose_graph_optimize_batch(graphs)
    assert st == capi.MVS_OK
    for i in range(8):
        assert res[i].tobytes() == single[i][0] and poses[i].tobytes() == single[i][1], i


def test_full_covariances(ctx):
    g, ref = model("full_cov", m.full_cov_graph)
    assert max(np.linalg.cond(c.reshape(6, 6)) for c in g["edge_cov"]) <= 1e6
    st, res, poses = ctx.pose_graph_optimize(g)
    check(res, poses, ref, DENSE_TOL, DENSE_TOL, "full covariances")


def test_boundary_between_the_paths(ctx):
    g16, ref16 = model("ring16", lambda: m.ring(16))
    _, ref16p = model("ring16", lambda: m.ring(16), solver="pcg")
    rot, trans = m.pose_distance(ref16["poses"], ref16p["poses"])
    print("model, N = 16, exact against PCG: rotation %.3e translation %.3e" % (rot, trans))
    tr, tt = _pcg_tol()
    assert rot <= tr and trans <= tt
    st, res, poses = ctx.pose_graph_optimize(g16)
    assert res["cg_iterations"] == 0                        # the dense path
    check(res, poses, ref16, DENSE_TOL, DENSE_TOL, "ring 16 (dense)")
    g17, ref17 = model("ring17", m.PCG_FIXTURES["ring17"], solver="pcg")
    st, res, poses = ctx.pose_graph_optimize(g17)
    assert res["cg_iterations"] > 0                         # the PCG path
    check(res, poses, ref17, tr, tt, "ring 17 (PCG)")


def test_star_and_long_ring(ctx):
    tr, tt = _pcg_tol()
    for name in ("star70", "ring200"):
        g, ref = model(name, m.PCG_FIXTURES[name], solver="pcg")
        st, res, poses = ctx.pose_graph_optimize(g)
        assert res["cg_iterations"] > 0
        check(res, poses, ref, tr, tt, name)


def test_rejected_steps(ctx):
    g, ref = model("far_off8", lambda: m.far_off(8))
    assert ref["rejected_steps"] >= 1                       # the model first, on the CPU
    st, res, poses = ctx.pose_graph_optimize(g)
    check(res, poses, ref, DENSE_TOL, DENSE_TOL, "far off 8 (dense)")
    assert (res["iterations"], res["rejected_steps"]) == (ref["iterations"], ref["rejected_steps"])
    g, ref = model("far_off20", m.PCG_FIXTURES["far_off20"], solver="pcg")
    assert ref["rejected_steps"] >= 1
    st, res, poses = ctx.pose_graph_optimize(g)
    tr, tt = _pcg_tol()
    check(res, poses, ref, tr, tt, "far off 20 (PCG)")
    assert res["rejected_steps"] >= 1


def test_mixed_batch(ctx):
    from mvslam_amd import capi

    graphs = [m.trivial()[0], m.ring(16), m.ring(17), m.ring(40)]
    single = [ctx.pose_graph_optimize(g) for g in graphs]
    out = np.full((4, 40, 12), SENTINEL)
    st, res, poses = ctx.pose_graph_optimize_batch(graphs, poses_out=out)
    assert st == capi.MVS_OK and poses is out
    for i, g in enumerate(graphs):
        n = g["node_pose"].shape[0]
        assert res[i].tobytes() == single[i][1].tobytes(), i
        assert out[i, :n].tobytes() == single[i][2].tobytes(), i
        assert np.all(out[i, n:] == SENTINEL), i


def test_failures_leave_the_context_usable(ctx):
    from mvslam_amd import capi

    out = np.full((4, 12), SENTINEL)
    st, res, _ = ctx.pose_graph_optimize(m.disconnected(), poses_out=out)
    assert st == capi.MVS_NO_MODEL and res["ok"] == 0 and np.all(out == SENTINEL)
    g, _ = m.triangle(0)
    g["edge_cov"] = g["edge_cov"].copy()
    g["edge_cov"][1] = np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]).reshape(36)
    st, res, _ = ctx.pose_graph_optimize(g, poses_out=out)
    assert st == capi.MVS_NO_MODEL and res["ok"] == 0 and np.all(out == SENTINEL)
    big = m.ring(17)
    big["edge_cov"] = big["edge_cov"].copy()
    big["edge_cov"][3] = np.diag([1.0, -1.0, 1.0, 1.0, 1.0, 1.0]).reshape(36)
    out17 = np.full((17, 12), SENTINEL)
    st, res, _ = ctx.pose_graph_optimize(big, poses_out=out17)
    assert st == capi.MVS_NO_MODEL and res["ok"] == 0 and np.all(out17 == SENTINEL)
    n = capi.POSE_GRAPH_MAX_NODES + 1
    eye = m.se3([0, 0, 0], [0, 0, 0])
    over = m.graph(np.tile(eye, (n, 1)), [(0, 1)], [eye], m.iso_cov(1.0, 1))
    with pytest.raises(capi.MvsError) as e:
        ctx.pose_graph_optimize(over)
    assert e.value.status == capi.MVS_ERR_CAPACITY
    loop, _ = m.trivial()
    loop["edge_dst"] = loop["edge_src"].copy()
    with pytest.raises(capi.MvsError) as e:
        ctx.pose_graph_optimize(loop)
    assert e.value.status == capi.MVS_ERR_INVALID_ARG
    nan, _ = m.trivial()
    nan["edge_pose"] = nan["edge_pose"].copy()
    nan["edge_pose"][0, 3] = np.nan
    with pytest.raises(capi.MvsError) as e:
        ctx.pose_graph_optimize(nan)
    assert e.value.status == capi.MVS_ERR_INVALID_ARG
    g, ref = model("trivial", lambda: m.trivial()[0])
    st, res, poses = ctx.pose_graph_optimize(g)
    assert st == capi.MVS_OK
    check(res, poses, ref, DENSE_TOL, DENSE_TOL, "trivial after the failures")


def test_determinism(ctx):
    for g in (m.triangle(3)[0], m.ring(200, chords=(5,))):
        a, b = ctx.pose_graph_optimize(g), ctx.pose_graph_optimize(g)
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_kernel_resources():
    res = json.load(open(os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "PgDenseDev" in k or "PgLargeDev" in k}
    assert len(mine) >= 11 and any("pg_dense_kernel" in k for k in mine)
    for k, v in mine.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0, (k, v)
        assert v["static_lds_bytes"] <= 64 * 1024, (k, v)
