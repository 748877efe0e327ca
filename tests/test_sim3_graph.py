"""GPU tests of the Sim(3) pose graphs (mvs_sim3_graph_optimize, sim3graph.hip) against the numpy model of their contract
(tests/sim3graph_model.py).

Tolerances, device against model.  Dense path (N <= 16): both sides solve exactly and differ in libm and summation order; the
bound is the project's bound for refinement parity, 1e-9 on rotation, translation and log-scale and relatively on the error
(DENSE_TOL of tests/test_pose_graph.py).  Large path: 10 x the model's own PCG-against-exact gap, measured on the CPU by
tests/test_sim3_graph_host.py and committed in profiles/sim3_graph_pcg_vs_exact.json.  Nothing here is derived from what the
device returns."""
import json
import os

import numpy as np
import pytest

import sim3graph_model as m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_TOL = (1e-9, 1e-9, 1e-9)
SENTINEL = -12345.678


def _pcg_tol():
    rec = json.load(open(os.path.join(ROOT, "profiles", "sim3_graph_pcg_vs_exact.json")))
    return 10.0 * rec["rotation"], 10.0 * rec["translation"], 10.0 * rec["log_scale"]


@pytest.fixture(scope="module")
def ctx():
    from mvslam_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


_MODEL = {}


def model(name, make, **kw):
    """the model's answer for a fixture, computed once per process and never modified"""
    key = (name, repr(sorted(kw.items())))
    if key not in _MODEL:
        g = make()
        _MODEL[key] = (g, m.optimize(g, **kw))
    return _MODEL[key]


def check(res, nodes, ref, tol, what=""):
    rot, trans, scale = m.pose_distance(nodes, ref["nodes"])
    rel = abs(res["error"] - ref["error"]) / max(abs(ref["error"]), 1e-300) if ref["error"] > 1e-20 else abs(res["error"])
    print("%s: rotation %.3e translation %.3e log-scale %.3e error %.17g (model %.17g) iterations %d/%d cg %d rejected %d/%d" % (
        what, rot, trans, scale, res["error"], ref["error"], res["iterations"], ref["iterations"], res["cg_iterations"],
        res["rejected_steps"], ref["rejected_steps"]))
    assert res["ok"] == 1 and ref["ok"] == 1
    assert rot <= tol[0] and trans <= tol[1] and scale <= tol[2], (what, rot, trans, scale, tol)
    assert rel <= max(tol), (what, res["error"], ref["error"])
    assert abs(res["error_initial"] - ref["error_initial"]) <= 1e-9 * max(1.0, ref["error_initial"])


def test_two_nodes(ctx):
    from mvslam_amd import capi

    g, ref = model("pair", m.DENSE_FIXTURES["pair"])
    before = {k: np.array(v, copy=True) for k, v in g.items() if isinstance(v, np.ndarray)}
    st, res, nodes = ctx.sim3_graph_optimize(g)
    assert st == capi.MVS_OK and res["cg_iterations"] == 0
    check(res, nodes, ref, DENSE_TOL, "pair")
    assert max(m.pose_distance(nodes, m.pair()[1])) < 1e-9           # the edge is exact: the truth, scale 1.7 included
    for k, v in before.items():
        assert np.array_equal(g[k], v), k


def test_triangles_with_inconsistent_scales_single_and_batch(ctx):
    from mvslam_amd import capi

    graphs, single = [], []
    for seed in m.TRIANGLE_SEEDS:
        g, ref = model("triangle%d" % seed, lambda: m.triangle(seed))
        st, res, nodes = ctx.sim3_graph_optimize(g)
        assert st == capi.MVS_OK
        check(res, nodes, ref, DENSE_TOL, "triangle %d" % seed)
        graphs.append(g)
        single.append((res.tobytes(), nodes.tobytes()))
    st, res, nodes = ctx.sim3_graph_optimize_batch(graphs)
    assert st == capi.MVS_OK
    for i in range(8):
        assert res[i].tobytes() == single[i][0] and nodes[i].tobytes() == single[i][1], i


@pytest.mark.parametrize("name", ["full_cov", "all_pairs16", "parallel16", "anchor5"])
def test_dense_fixtures(ctx, name):
    g, ref = model(name, m.DENSE_FIXTURES[name])
    if name == "full_cov":
        assert max(np.linalg.cond(c.reshape(7, 7)) for c in g["edge_cov"]) <= 1e6
    if name == "parallel16":
        assert len(g["edge_src"]) > 256 and g["node_sim3"].shape[0] == 16
    if name == "anchor5":
        assert g["anchor"] == 5
    st, res, nodes = ctx.sim3_graph_optimize(g)
    assert res["cg_iterations"] == 0
    check(res, nodes, ref, DENSE_TOL, name)


def test_mixed_batch_equals_the_single_calls(ctx):
    from mvslam_amd import capi

    graphs = [m.pair()[0], m.dense_ring(5), m.dense_ring(16), m.dense_ring(17)]
    single = [ctx.sim3_graph_optimize(g) for g in graphs]
    out = np.full((4, 17, 13), SENTINEL)
    st, res, nodes = ctx.sim3_graph_optimize_batch(graphs, nodes_out=out)
    assert st == capi.MVS_OK and nodes is out
    for i, g in enumerate(graphs):
        n = g["node_sim3"].shape[0]
        assert single[i][0] == capi.MVS_OK and res[i].tobytes() == single[i][1].tobytes(), i
        assert out[i, :n].tobytes() == single[i][2].tobytes(), i
        assert np.all(out[i, n:] == SENTINEL), i
    _, ref = model("ring5", m.DENSE_FIXTURES["ring5"])
    check(res[1], out[1, :5], ref, DENSE_TOL, "ring 5 in the batch")


def test_boundary_between_the_paths(ctx):
    g16, ref16 = model("ring16", m.DENSE_FIXTURES["ring16"])
    st, res, nodes = ctx.sim3_graph_optimize(g16)
    assert res["cg_iterations"] == 0                        # the dense path
    check(res, nodes, ref16, DENSE_TOL, "ring 16 (dense)")
    g17, ref17 = model("ring17", m.PCG_FIXTURES["ring17"], solver="pcg")
    st, res, nodes = ctx.sim3_graph_optimize(g17)
    assert res["cg_iterations"] > 0                         # the PCG path
    check(res, nodes, ref17, _pcg_tol(), "ring 17 (PCG)")


@pytest.mark.parametrize("name", ["star70", "ring257"])
def test_large_path(ctx, name):
    g, ref = model(name, m.PCG_FIXTURES[name], solver="pcg")
    st, res, nodes = ctx.sim3_graph_optimize(g)
    assert res["cg_iterations"] > 0
    check(res, nodes, ref, _pcg_tol(), name)


def test_drift_ring_reaches_the_truth(ctx):
    g, truth, _ = m.drift_ring()
    _, ref = model("drift_ring40", m.PCG_FIXTURES["drift_ring40"], solver="pcg")
    st, res, nodes = ctx.sim3_graph_optimize(g)
    tol = _pcg_tol()
    rot, trans, scale = m.pose_distance(nodes, truth)
    print("drift ring against the truth: rotation %.3e translation %.3e log-scale %.3e (bounds %s), error %.3e -> %.3e" % (
        rot, trans, scale, tol, res["error_initial"], res["error"]))
    assert res["ok"] == 1 and res["cg_iterations"] > 0
    assert rot <= tol[0] and trans <= tol[1] and scale <= tol[2]
    check(res, nodes, ref, tol, "drift ring 40 (PCG)")


def test_cg_chunks_and_determinism(ctx):
    from mvslam_amd import capi

    for g in (m.dense_ring(17), m.star()):
        st, res0, nodes0 = ctx.sim3_graph_optimize(g)
        assert st == capi.MVS_OK and res0["cg_iterations"] > 0
        for chunk in (1, 16, 64):
            st, res, nodes = ctx.sim3_graph_optimize(g, params=capi.default_sim3_graph_params(cg_chunk_iterations=chunk))
            assert res.tobytes() == res0.tobytes() and nodes.tobytes() == nodes0.tobytes(), chunk
        st, res, nodes = ctx.sim3_graph_optimize(g)
        assert res.tobytes() == res0.tobytes() and nodes.tobytes() == nodes0.tobytes()
    g = m.triangle(m.TRIANGLE_SEEDS[0])
    a, b = ctx.sim3_graph_optimize(g), ctx.sim3_graph_optimize(g)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def _refused(ctx, g, status, n_out=None):
    """the call is refused with `status` and leaves a sentinel-filled output untouched"""
    from mvslam_amd import capi

    out = np.full((n_out or g["node_sim3"].shape[0], 13), SENTINEL)
    if status == capi.MVS_NO_MODEL:
        st, res, _ = ctx.sim3_graph_optimize(g, nodes_out=out)
        assert st == capi.MVS_NO_MODEL and res["ok"] == 0 and res["error"] == 0.0 and res["iterations"] == 0
    else:
        with pytest.raises(capi.MvsError) as e:
            ctx.sim3_graph_optimize(g, nodes_out=out)
        assert e.value.status == status
    assert np.all(out == SENTINEL)


def _with(g, key, index, value):
    g = dict(g, **{key: g[key].copy()})
    g[key][index] = value
    return g


def test_refusals(ctx):
    from mvslam_amd import capi

    tri, big = m.triangle(m.TRIANGLE_SEEDS[0]), m.dense_ring(17)
    for g in (tri, big):
        for value in (0.0, -1.0, np.nan, np.inf):
            _refused(ctx, _with(g, "node_sim3", (1, 12), value), capi.MVS_ERR_INVALID_ARG)
            _refused(ctx, _with(g, "edge_sim3", (1, 12), value), capi.MVS_ERR_INVALID_ARG)
        _refused(ctx, _with(g, "node_sim3", (2, 10), np.nan), capi.MVS_ERR_INVALID_ARG)
        _refused(ctx, _with(g, "edge_cov", (0, 5), np.inf), capi.MVS_ERR_INVALID_ARG)
        _refused(ctx, _with(g, "edge_dst", 1, int(g["edge_src"][1])), capi.MVS_ERR_INVALID_ARG)       # src == dst
        _refused(ctx, _with(g, "edge_dst", 1, g["node_sim3"].shape[0]), capi.MVS_ERR_INVALID_ARG)    # out of range
        _refused(ctx, _with(g, "edge_src", 0, -1), capi.MVS_ERR_INVALID_ARG)
        _refused(ctx, dict(g, anchor=g["node_sim3"].shape[0]), capi.MVS_ERR_INVALID_ARG)
        _refused(ctx, m.indefinite(g, 1), capi.MVS_NO_MODEL)
    _refused(ctx, m.disconnected(), capi.MVS_NO_MODEL)
    keep = [k for k in range(len(big["edge_src"])) if 1 not in (int(big["edge_src"][k]), int(big["edge_dst"][k]))]
    far = dict(big, edge_src=big["edge_src"][keep].copy(), edge_dst=big["edge_dst"][keep].copy(),
               edge_sim3=big["edge_sim3"][keep].copy(), edge_cov=big["edge_cov"][keep].copy())     # node 1 hangs on nothing
    _refused(ctx, far, capi.MVS_NO_MODEL)
    # capacity: the count alone decides, the arrays are the triangle's
    _refused(ctx, dict(tri, n_nodes=capi.POSE_GRAPH_MAX_NODES + 1), capi.MVS_ERR_CAPACITY)
    _refused(ctx, dict(tri, n_edges=capi.POSE_GRAPH_MAX_EDGES + 1), capi.MVS_ERR_CAPACITY)
    for kw in (dict(lambda_factor=1.0), dict(anchor_sigma=(1e-4, 1e-4, 0.0)), dict(anchor_sigma=(0.0, 1e-4, 1e-4)),
               dict(cg_max_iterations=-1), dict(max_iterations=-1), dict(cg_rel_tol=-1e-10)):
        with pytest.raises(capi.MvsError) as e:
            ctx.sim3_graph_optimize(tri, params=capi.default_sim3_graph_params(**kw))
        assert e.value.status == capi.MVS_ERR_INVALID_ARG, kw
    # a batch that fails in part: the good graphs get the bytes of their single calls, the bad ones keep the sentinel
    graphs = [tri, m.indefinite(big, 3), m.disconnected(), big]
    single = {i: ctx.sim3_graph_optimize(graphs[i]) for i in (0, 3)}
    out = np.full((4, 17, 13), SENTINEL)
    st, res, _ = ctx.sim3_graph_optimize_batch(graphs, nodes_out=out)
    assert st == capi.MVS_NO_MODEL and res[1]["ok"] == 0 and res[2]["ok"] == 0 and np.all(out[1:3] == SENTINEL)
    for i in (0, 3):
        n = graphs[i]["node_sim3"].shape[0]
        assert res[i].tobytes() == single[i][1].tobytes() and out[i, :n].tobytes() == single[i][2].tobytes()
    g, ref = model("pair", m.DENSE_FIXTURES["pair"])
    st, res, nodes = ctx.sim3_graph_optimize(g)
    check(res, nodes, ref, DENSE_TOL, "pair after the refusals")


def test_the_context_switches_do_not_reach_the_sim3_calls(ctx):
    from mvslam_amd import capi

    g = m.dense_ring(17)
    _, res0, nodes0 = ctx.sim3_graph_optimize(g)
    try:
        ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_DIRECT)
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_HUBER, 0.5, 0)
        _, res, nodes = ctx.sim3_graph_optimize(g)
    finally:
        ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_PCG)
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_NONE)
    assert res.tobytes() == res0.tobytes() and nodes.tobytes() == nodes0.tobytes() and res["cg_iterations"] > 0


def test_max_iterations_zero(ctx):
    from mvslam_amd import capi

    for g in (m.dense_ring(8), m.dense_ring(17)):
        st, res, nodes = ctx.sim3_graph_optimize(g, params=capi.default_sim3_graph_params(max_iterations=0))
        assert st == capi.MVS_OK and res["ok"] == 1 and res["iterations"] == 0 and res["cg_iterations"] == 0
        assert res["error"] == res["error_initial"] > 0.0 and nodes.tobytes() == g["node_sim3"].tobytes()
        ref = m.optimize(g, lm=dict(max_iterations=0))
        assert abs(res["error"] - ref["error"]) <= 1e-9 * ref["error"]
