"""GPU tests of the pose-graph back end (mvs_pose_graph_optimize, posegraph.hip) against the numpy model of its contract
(tests/posegraph_model.py).

Tolerances, device against model.  Dense path (N <= 16): both sides solve exactly and differ in libm and summation order;
the bound is the project's bound for GPU <-> oracle refinement parity, 1e-9 on the pose (README.md).  Large path: 10 x the
model's own PCG-against-exact gap, measured on the CPU by tests/test_pose_graph_host.py and committed in
profiles/pose_graph_pcg_vs_exact.json.  The final error is compared relatively with the same bounds.  A large-path run away
from the default parameters (posegraph_model.PARAM_RUNS) has its own recorded gap there and is held to 10 x that, never
below the converged bound; the one run whose CG is cut short is held to 10 x the recorded drift between two summation orders
of the same recursion (`truncated_cg`), with the same floor.  Nothing here is derived from what the device returns."""
import json
import os

import numpy as np
import pytest

import posegraph_model as m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_TOL = 1e-9
SENTINEL = -12345.678


def _recorded():
    return json.load(open(os.path.join(ROOT, "profiles", "pose_graph_pcg_vs_exact.json")))


def _pcg_tol():
    rec = _recorded()
    return 10.0 * rec["rotation"], 10.0 * rec["translation"]


def _floor_tol(rec):
    """10 x a recorded gap, and not below the converged bound of the large path"""
    return tuple(max(10.0 * rec[w], t) for w, t in zip(("rotation", "translation"), _pcg_tol()))


def _run_tol(name):
    """the bound of a large-path run away from the default parameters (posegraph_model.PARAM_RUNS)"""
    return _floor_tol(_recorded()["parameter_runs"][name])


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


def run(ctx, g, poses_out=None, **kw):
    """one graph on the device with the model's keywords (lm = dict of LM fields, anchor_sigma, cg_rel_tol, cg_max_iterations)"""
    from mvslam_amd import capi

    flat = dict(kw.pop("lm", None) or {}, **kw)
    return ctx.pose_graph_optimize(g, params=capi.default_pose_graph_params(**flat) if flat else None, poses_out=poses_out)


def gap(what, A, B, tol):
    rot, trans = m.pose_distance(A, B)
    print("%s: rotation %.3e (bound %.3e) translation %.3e (bound %.3e)" % (what, rot, tol[0], trans, tol[1]))
    assert rot <= tol[0] and trans <= tol[1], (what, rot, trans, tol)


def counts(res):
    return int(res["iterations"]), int(res["rejected_steps"])


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


def test_anchor_in_the_middle_and_at_the_end(ctx):
    from mvslam_amd import capi

    for name, (n, perm) in m.PERMUTATIONS.items():
        dense = n <= m_dense()
        tol = (DENSE_TOL, DENSE_TOL) if dense else _pcg_tol()
        g, ref = model(name, lambda: m.permuted_ring(name), solver="exact" if dense else "pcg")
        assert g["anchor"] == perm[0] != 0
        st, res, poses = ctx.pose_graph_optimize(g)
        assert st == capi.MVS_OK and (res["cg_iterations"] == 0) == dense
        check(res, poses, ref, tol[0], tol[1], name)
        st, _, plain = ctx.pose_graph_optimize(m.ring(n))                   # independent of the model's solve
        gap(name + ", mapped back, against the device's own ring(%d)" % n, poses[perm], plain, tol)
    out = np.full((4, 12), SENTINEL)
    st, res, _ = ctx.pose_graph_optimize(m.orphan_node0(), poses_out=out)
    assert st == capi.MVS_NO_MODEL and res["ok"] == 0 and np.all(out == SENTINEL)


def m_dense():
    from mvslam_amd import capi

    return capi.POSE_GRAPH_DENSE_MAX_NODES


def test_rigid_motion_invariance(ctx):
    for name, make, tol in (("full_cov", m.full_cov_graph, (DENSE_TOL, DENSE_TOL)),
                            ("ring17", m.PCG_FIXTURES["ring17"], _run_tol("ring17_moved"))):
        g = make()
        _, a, pa = ctx.pose_graph_optimize(g)
        _, b, pb = ctx.pose_graph_optimize(m.moved(g))
        assert a["ok"] == 1 and b["ok"] == 1
        gap("optimize(T g) against T optimize(g), " + name, pb, m.moved_poses(pa), tol)
        assert abs(a["error"] - b["error"]) <= max(tol) * a["error"]


def test_first_order_optimality_at_the_device_answer(ctx):
    rec = _recorded()["gradient_ratio"]
    for name, (make, solver) in m.GRADIENT_FIXTURES.items():
        g = make()
        st, res, poses = ctx.pose_graph_optimize(g)
        assert res["ok"] == 1 and (res["cg_iterations"] > 0) == (solver == "pcg")
        ratio = np.linalg.norm(m.gradient(g, poses)) / np.linalg.norm(m.gradient(g, g["node_pose"]))
        print("%s: |J^T r| at the device's answer / at the initial values %.3e (model %.3e, bound %.3e)" % (
            name, ratio, rec[name]["ratio"], 10.0 * rec[name]["ratio"]))
        assert ratio <= 10.0 * rec[name]["ratio"]


def test_anchor_sigmas(ctx):
    for n, sigma, tol in ((8, m.LOOSE_SIGMA, (DENSE_TOL, DENSE_TOL)), (8, m.LOOSE_SIGMA[::-1], (DENSE_TOL, DENSE_TOL)),
                          (17, m.LOOSE_SIGMA, _run_tol("loose_anchor17")),
                          (17, m.LOOSE_SIGMA[::-1], _run_tol("loose_anchor17_swapped"))):
        kw = dict(lm=m.LOOSE_LM, anchor_sigma=sigma)
        g, ref = model("loose_anchor%d" % n, lambda: m.loose_anchor(n), solver="exact" if n == 8 else "pcg", **kw)
        st, res, poses = run(ctx, g, **kw)
        assert (res["cg_iterations"] > 0) == (n == 17)
        check(res, poses, ref, tol[0], tol[1], "loose anchor %d, sigma %s" % (n, sigma))
        assert counts(res) == counts(ref)                                    # two solves, the cap is the exit


def test_max_iterations_zero_and_two(ctx):
    from mvslam_amd import capi

    for g in (m.ring(8), m.ring(17)):
        st, res, poses = run(ctx, g, lm=dict(max_iterations=0))
        assert st == capi.MVS_OK and res["ok"] == 1 and res["iterations"] == 0 and res["cg_iterations"] == 0
        assert res["rejected_steps"] == 0 and res["error"] == res["error_initial"] > 0.0
        assert poses.tobytes() == g["node_pose"].tobytes()
        ref = m.optimize(g, lm=dict(max_iterations=0))
        assert abs(res["error"] - ref["error"]) <= 1e-9 * ref["error"]
    kw = dict(lm=dict(max_iterations=2))
    g, ref = model("far_off8", lambda: m.far_off(8), **kw)
    assert ref["exit"] == "max_iterations"
    st, res, poses = run(ctx, g, **kw)
    check(res, poses, ref, DENSE_TOL, DENSE_TOL, "far off 8, two iterations")
    assert counts(res) == counts(ref) == (2, 0)


def test_lambda_upper_exit(ctx):
    kw = dict(lm=m.LAMBDA_UPPER8)
    g, ref = model("far_off8", lambda: m.far_off(8), **kw)
    assert ref["exit"] == "lambda_upper" and ref["rejected_steps"] >= 1
    st, res, poses = run(ctx, g, **kw)
    check(res, poses, ref, DENSE_TOL, DENSE_TOL, "far off 8, lambda_upper (dense)")
    assert counts(res) == counts(ref)
    make, kw = m.PARAM_RUNS["lambda_upper20"]
    g, ref = model("far_off20", make, solver="pcg", **kw)
    assert ref["exit"] == "lambda_upper" and ref["rejected_steps"] >= 1
    st, res, poses = run(ctx, g, **kw)
    tol = _run_tol("lambda_upper20")
    check(res, poses, ref, tol[0], tol[1], "far off 20, lambda_upper (PCG)")
    assert res["rejected_steps"] >= 1 and res["iterations"] < 100


def test_cg_limits(ctx):
    g, ref = model("ring17", m.PCG_FIXTURES["ring17"], solver="pcg", h_apply="edges", **m.TRUNCATED)
    assert ref["trace"][0]["cg_status"] == 0 and ref["trace"][0]["accepted"]   # out of iterations, smaller residual, accepted
    st, res, poses = run(ctx, g, **m.TRUNCATED)
    tol = _floor_tol(_recorded()["truncated_cg"])
    check(res, poses, ref, tol[0], tol[1], "ring 17, three CG iterations")
    assert (res["cg_iterations"], res["iterations"], res["rejected_steps"]) == (3, 1, 0)
    _, default, _ = ctx.pose_graph_optimize(g)
    kw = m.PARAM_RUNS["cg_rel_tol_1e-4"][1]
    g, ref = model("ring17", m.PCG_FIXTURES["ring17"], solver="pcg", **kw)
    _, full = model("ring17", m.PCG_FIXTURES["ring17"], solver="pcg")
    assert ref["cg_iterations"] < full["cg_iterations"]
    st, res, poses = run(ctx, g, **kw)
    tol = _run_tol("cg_rel_tol_1e-4")
    check(res, poses, ref, tol[0], tol[1], "ring 17, cg_rel_tol 1e-4")
    print("CG iterations at 1e-4: %d, at the default: %d" % (res["cg_iterations"], default["cg_iterations"]))
    assert 0 < res["cg_iterations"] < default["cg_iterations"]


def test_refused_parameters(ctx):
    from mvslam_amd import capi

    g, ref = model("trivial", lambda: m.trivial()[0])
    for kw in (dict(lambda_factor=1.0), dict(anchor_sigma=(0.0, 1e-4)), dict(anchor_sigma=(1e-4, 0.0)),
               dict(cg_max_iterations=-1), dict(max_iterations=-1), dict(cg_rel_tol=-1e-10)):
        for call in (lambda p: ctx.pose_graph_optimize_batch([g, m.ring(17)], params=p),
                     lambda p: ctx.pose_graph_optimize(g, params=p)):
            with pytest.raises(capi.MvsError) as e:
                call(capi.default_pose_graph_params(**kw))
            assert e.value.status == capi.MVS_ERR_INVALID_ARG, kw
    st, res, poses = ctx.pose_graph_optimize(g)
    assert st == capi.MVS_OK
    check(res, poses, ref, DENSE_TOL, DENSE_TOL, "trivial after the refused parameters")


def test_dense_stride_and_parallel_edges(ctx):
    for name, make in (("all_pairs16 (272 edges)", m.all_pairs16), ("parallel3", m.parallel3)):
        g, ref = model(name, make)
        st, res, poses = ctx.pose_graph_optimize(g)
        assert res["cg_iterations"] == 0
        check(res, poses, ref, DENSE_TOL, DENSE_TOL, name)


def test_every_dense_size_in_one_batch(ctx):
    from mvslam_amd import capi

    graphs = [m.dense_size(n) for n in range(1, 17)]
    single = [ctx.pose_graph_optimize(g) for g in graphs]
    out = np.full((16, 16, 12), SENTINEL)
    st, res, poses = ctx.pose_graph_optimize_batch(graphs, poses_out=out)
    assert st == capi.MVS_OK
    worst = [0.0, 0.0]
    for i, g in enumerate(graphs):
        n = i + 1
        assert single[i][0] == capi.MVS_OK and res[i]["ok"] == 1 and res[i]["cg_iterations"] == 0
        assert res[i].tobytes() == single[i][1].tobytes(), n
        assert out[i, :n].tobytes() == single[i][2].tobytes(), n
        assert np.all(out[i, n:] == SENTINEL), n
        _, ref = model("dense_size%d" % n, lambda: m.dense_size(n))
        rot, trans = m.pose_distance(out[i, :n], ref["poses"])
        worst = [max(worst[0], rot), max(worst[1], trans)]
        assert rot <= DENSE_TOL and trans <= DENSE_TOL, (n, rot, trans)
        assert abs(res[i]["error"] - ref["error"]) <= DENSE_TOL * max(ref["error"], 1.0), n
    print("N = 1 .. 16 in one batch: rotation %.3e translation %.3e (bound %.1e)" % (worst[0], worst[1], DENSE_TOL))
    assert out[0, 0].tobytes() == graphs[0]["node_pose"].tobytes() and res[0]["error"] == 0.0   # N = 1: nothing to move


def test_more_than_256_nodes(ctx):
    tr, tt = _pcg_tol()
    g, ref = model("ring257", m.PCG_FIXTURES["ring257"], solver="pcg")
    st, res, poses = ctx.pose_graph_optimize(g)
    assert res["cg_iterations"] > 0
    check(res, poses, ref, tr, tt, "ring257")


def test_batch_that_fails_in_part_and_shrinks(ctx):
    from mvslam_amd import capi

    graphs = [m.ring(40), m.ring(17), m.indefinite(m.triangle(0)[0], 1), m.disconnected(), m.indefinite(m.ring(17), 3),
              m.trivial()[0]]
    good, bad = (0, 1, 5), (2, 3, 4)
    single = {i: ctx.pose_graph_optimize(graphs[i]) for i in good}
    out = np.full((6, 40, 12), SENTINEL)
    st, res, poses = ctx.pose_graph_optimize_batch(graphs, poses_out=out)
    assert st == capi.MVS_NO_MODEL and poses is out
    for i in bad:
        assert res[i]["ok"] == 0 and np.all(out[i] == SENTINEL), i
    for i in good:
        n = graphs[i]["node_pose"].shape[0]
        assert single[i][0] == capi.MVS_OK and res[i]["ok"] == 1
        assert res[i].tobytes() == single[i][1].tobytes(), i
        assert out[i, :n].tobytes() == single[i][2].tobytes(), i
        assert np.all(out[i, n:] == SENTINEL), i


def test_rotation_near_pi(ctx):
    g, ref = model("near_pi_pair", lambda: m.near_pi_pair()[0])
    st, res, poses = ctx.pose_graph_optimize(g)
    check(res, poses, ref, DENSE_TOL, DENSE_TOL, "two nodes, %.1f rad off" % m.NEAR_PI)
    assert counts(res) == counts(ref)
    gap("two nodes against the truth", poses, m.near_pi_pair()[1], (1e-6, 1e-6))
    tr, tt = _pcg_tol()
    g, ref = model("near_pi_ring", m.PCG_FIXTURES["near_pi_ring"], solver="pcg")
    st, res, poses = ctx.pose_graph_optimize(g)
    assert res["cg_iterations"] > 0
    check(res, poses, ref, tr, tt, "ring 17, one node %.1f rad off" % m.NEAR_PI)
    gap("ring 17 against the truth", poses, m.near_pi_ring()[1], (1e-6, 1e-6))


def test_overflowing_cost(ctx):
    from mvslam_amd import capi

    for g in (m.overflowing(m.triangle(0)[0]), m.overflowing(m.ring(17))):
        out = np.full((g["node_pose"].shape[0], 12), SENTINEL)
        st, res, _ = ctx.pose_graph_optimize(g, poses_out=out)
        assert st == capi.MVS_NO_MODEL and res["ok"] == 0 and np.all(out == SENTINEL)
        assert res["error"] == 0.0 and res["error_initial"] == 0.0
    g, ref = model("ring17", m.PCG_FIXTURES["ring17"], solver="pcg")
    st, res, poses = ctx.pose_graph_optimize(g)
    tr, tt = _pcg_tol()
    check(res, poses, ref, tr, tt, "ring 17 after the overflowing costs")


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
