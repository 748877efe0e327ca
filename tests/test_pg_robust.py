"""GPU tests of the pose graphs' robust edge losses (mvs_ctx_set_pose_graph_loss, mvs_pose_graph_edge_stats; posegraph.hip,
DESIGN.md section 4.10.5) against the numpy model of their contract (tests/pg_robust_model.py).

Tolerances, device against model: those of tests/test_pose_graph.py and tests/test_pg_direct.py.  Dense path: DENSE_TOL.
Large path under the PCG: 10 x the model's own exact-against-PCG gap of the fixture, recorded in
tests/golden/pg_robust_pcg_vs_exact.json by tests/test_pg_robust_host.py's measurement, and not below the converged bound of
the large path (10 x profiles/pose_graph_pcg_vs_exact.json).  Large path under the direct solver: tests/test_pg_direct.py's
bound, the larger of DENSE_TOL and 10 x profiles/pose_graph_direct_vs_exact.json, against the model with exact solves.
iterations and rejected_steps are asserted where the model's decision margin is at least 1e3
(tests/test_pg_robust_host.py prints which fixtures those are).  Nothing here is derived from what the device returns."""
import json
import os
from contextlib import contextmanager

import numpy as np
import pytest

import pg_robust_model as rm
import posegraph_model as m
import test_pg_robust_host as host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_TOL = 1e-9
NEUTRAL = {"triangle3": lambda: m.triangle(3)[0], "ring17": lambda: m.ring(17), "ring200": lambda: m.ring(200, chords=(5,))}


def direct_tol():
    rec = json.load(open(os.path.join(ROOT, "profiles", "pose_graph_direct_vs_exact.json")))
    return max(DENSE_TOL, 10.0 * rec["rotation"]), max(DENSE_TOL, 10.0 * rec["translation"])


def tol_of(name, direct):
    if rm.dense(name):
        return DENSE_TOL, DENSE_TOL
    return direct_tol() if direct else host.large_tol(name)


@pytest.fixture(scope="module")
def ctx():
    from mvslam_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@contextmanager
def setting(ctx, loss=rm.NONE, k=1.0, first_edge=0, direct=False):
    """the context under a loss (and the direct solver) for the length of a block"""
    from mvslam_amd import capi

    ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_DIRECT if direct else capi.MVS_PG_SOLVER_PCG)
    ctx.set_pose_graph_loss(loss, k, first_edge)
    try:
        yield ctx
    finally:
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_NONE)
        ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_PCG)


def same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def check(res, poses, ref, tol, what, counts):
    rot, trans = m.pose_distance(poses, ref["poses"])
    rel = abs(res["error"] - ref["error"]) / ref["error"]
    print("%s: rotation %.3e (bound %.3e) translation %.3e (bound %.3e) error %.17g (model %.17g) iterations %d/%d cg %d "
          "rejected %d/%d, counts %s" % (what, rot, tol[0], trans, tol[1], res["error"], ref["error"], res["iterations"],
                                         ref["iterations"], res["cg_iterations"], res["rejected_steps"], ref["rejected_steps"],
                                         "asserted" if counts else "not asserted"))
    assert res["ok"] == 1 and ref["ok"] == 1
    assert rot <= tol[0] and trans <= tol[1], (what, rot, trans)
    assert rel <= max(tol), (what, res["error"], ref["error"])
    assert abs(res["error_initial"] - ref["error_initial"]) <= 1e-9 * max(1.0, ref["error_initial"])
    if counts:
        assert (res["iterations"], res["rejected_steps"]) == (ref["iterations"], ref["rejected_steps"]), what


CASES = [(name, False) for name in rm.FIXTURES] + [(name, True) for name in ("n20_cauchy", "n20_huber", "n17_cauchy", "n17_huber")]


@pytest.mark.parametrize("name,direct", CASES, ids=["%s-%s" % (n, "direct" if d else "default") for n, d in CASES])
def test_device_against_model(ctx, name, direct):
    from mvslam_amd import capi

    solver = rm.model_solver(name, direct)
    g, ref = host.run(name, solver)
    kw = rm.FIXTURES[name][1]
    with setting(ctx, kw["loss"], kw["k"], kw["first_edge"], direct):
        single = ctx.pose_graph_optimize(g)
        batch = ctx.pose_graph_optimize_batch([m.triangle(0)[0], g])
    st, res, poses = single
    assert st == capi.MVS_OK and (res["cg_iterations"] > 0) == (not rm.dense(name) and not direct)
    check(res, poses, ref, tol_of(name, direct), "%s%s" % (name, " (direct)" if direct else ""), host.counts_are_asserted(name, solver))
    n = g["node_pose"].shape[0]
    assert batch[0] == capi.MVS_OK and batch[1][1].tobytes() == res.tobytes() and batch[2][1, :n].tobytes() == poses.tobytes()


@pytest.mark.parametrize("name", ["n12_cauchy", "n20_cauchy", "n12_full_cauchy"])
def test_cauchy_lands_at_the_clean_optimum_and_the_plain_cost_does_not(ctx, name):
    g, ref = host.run(name, rm.model_solver(name))
    clean = host.clean_optimum(g)
    want = m.pose_distance(ref["poses"], clean)            # how close the model's robust optimum is
    tol = tol_of(name, False)
    kw = rm.FIXTURES[name][1]
    with setting(ctx, kw["loss"], kw["k"], kw["first_edge"]):
        _, res, poses = ctx.pose_graph_optimize(g)
    _, res0, poses0 = ctx.pose_graph_optimize(g)
    got, got0 = m.pose_distance(poses, clean), m.pose_distance(poses0, clean)
    print("%s: to the clean optimum, Cauchy %.3e / %.3e (model %.3e / %.3e), no loss %.3e / %.3e" % (name, *got, *want, *got0))
    assert res["ok"] == 1 and res0["ok"] == 1
    assert got[0] <= want[0] + tol[0] and got[1] <= want[1] + tol[1]
    assert got0[0] > 100.0 * (want[0] + tol[0]) and got0[1] > 100.0 * (want[1] + tol[1])


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
@pytest.mark.parametrize("name", list(NEUTRAL))
def test_neutrality(ctx, name, direct):
    """a loss set and taken back, Huber with a constant nothing reaches (w = 1 and rho2 = s exactly) and a first_edge behind
    the last edge all return the bytes of a context that never had a loss"""
    from mvslam_amd import capi

    g = NEUTRAL[name]()
    fresh = capi.Context(0)
    try:
        if direct:
            fresh.set_pose_graph_solver(capi.MVS_PG_SOLVER_DIRECT)
        want = fresh.pose_graph_optimize(g)
    finally:
        fresh.close()
    assert want[0] == capi.MVS_OK
    with setting(ctx, rm.HUBER, 1.0, 0, direct):
        robust = ctx.pose_graph_optimize(g)
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_NONE)
        assert same(ctx.pose_graph_optimize(g), want)                       # (a) set, then NONE
    assert not same(robust, want)                                           # the loss did something in between
    with setting(ctx, rm.HUBER, 1e30, 0, direct):
        assert same(ctx.pose_graph_optimize(g), want)                       # (b) the plumbing and the summation order
    with setting(ctx, rm.CAUCHY, 1.0, len(g["edge_src"]), direct):
        assert same(ctx.pose_graph_optimize(g), want)                       # first_edge = n_edges
    with setting(ctx, rm.NONE, float("nan"), capi.MVS_PG_LOSS_LOOP_EDGES, direct):
        assert same(ctx.pose_graph_optimize(g), want)                       # under NONE neither k nor first_edge is looked at


def test_first_edge_counts_inside_each_graph_of_a_batch(ctx):
    from mvslam_amd import capi

    graphs = [rm.outlier_ring(12), rm.outlier_ring(20), m.triangle(1)[0]]
    with setting(ctx, rm.CAUCHY, rm.CAUCHY_K, 24):
        single = [ctx.pose_graph_optimize(g) for g in graphs]
        st, res, poses = ctx.pose_graph_optimize_batch(graphs)
    assert st == capi.MVS_OK
    for i, g in enumerate(graphs):
        n = g["node_pose"].shape[0]
        assert res[i].tobytes() == single[i][1].tobytes() and poses[i, :n].tobytes() == single[i][2].tobytes(), i
    plain = ctx.pose_graph_optimize(graphs[2])
    assert same(single[2], plain)                                           # 4 edges: none at or behind 24
    # first_edge = 24 in the 42-edge graph covers 16 clean edges too: another answer than first_edge = 40
    with setting(ctx, rm.CAUCHY, rm.CAUCHY_K, 40):
        assert not same(ctx.pose_graph_optimize(graphs[1]), single[1])
    ref = rm.optimize(graphs[1], loss=rm.CAUCHY, k=rm.CAUCHY_K, first_edge=24, solver="pcg")
    rot, trans = m.pose_distance(single[1][2], ref["poses"])
    tol = host.large_tol("n20_cauchy")
    print("n = 20, Cauchy from edge 24: rotation %.3e translation %.3e" % (rot, trans))
    assert rot <= max(tol[0], DENSE_TOL) and trans <= max(tol[1], DENSE_TOL)


@pytest.mark.parametrize("name", ["n12_cauchy", "n12_huber", "n12_full_cauchy", "n20_cauchy", "n20_huber", "n20_cauchy3_all"])
def test_edge_stats(ctx, name):
    from mvslam_amd import capi

    g = rm.FIXTURES[name][0]()
    kw = rm.FIXTURES[name][1]
    E = len(g["edge_src"])
    with setting(ctx, kw["loss"], kw["k"], kw["first_edge"]):
        _, res, poses = ctx.pose_graph_optimize(g)
        st, chi2, weight = ctx.pose_graph_edge_stats(g, poses)
        st0, chi2_0, weight_0 = ctx.pose_graph_edge_stats(g)                # poses = NULL: at node_pose
        st1, chi2_1, weight_1 = ctx.pose_graph_edge_stats(g, g["node_pose"])
    assert st == st0 == st1 == capi.MVS_OK and chi2.shape == weight.shape == (E,)
    s, w = rm.edge_stats(g, poses, kw["loss"], kw["k"], kw["first_edge"])   # the model at the DEVICE's optimum
    print("%s: chi2 relative %.3e, weight relative %.3e, weights of the added edges %s" % (
        name, np.abs(chi2 / s - 1).max(), np.abs(weight / w - 1).max(), weight[-2:]))
    assert (np.abs(chi2 - s) <= 1e-9 * s).all()
    assert (np.abs(weight - w) <= 1e-9 * w).all()
    assert chi2_0.tobytes() == chi2_1.tobytes() and weight_0.tobytes() == weight_1.tobytes()
    s0, _ = rm.edge_stats(g, None)
    assert (np.abs(chi2_0 - s0) <= 1e-9 * s0).all() and chi2_0.tobytes() != chi2.tobytes()
    if kw["first_edge"] > 0:
        assert (weight[:kw["first_edge"]] == 1.0).all()
        assert sorted(np.argsort(weight)[:2].tolist()) == [E - 2, E - 1] and weight[-2:].max() < 0.05
    # without a loss every weight is 1 and chi2 is the same
    st, chi2_n, weight_n = ctx.pose_graph_edge_stats(g, poses)
    assert chi2_n.tobytes() == chi2.tobytes() and (weight_n == 1.0).all()
    # the sum of rho2 over the edges is the error the optimiser reported, to the anchor's share (zero at an optimum up to 1e-9)
    rho = np.array([rm.loss(x, kw["loss"], kw["k"])[1] if e >= kw["first_edge"] else x for e, x in enumerate(chi2)])
    assert abs(0.5 * rho.sum() - res["error"]) <= 1e-6 * res["error"]


def test_edge_stats_failures(ctx):
    from mvslam_amd import capi

    st, chi2, weight = ctx.pose_graph_edge_stats(m.disconnected())
    assert st == capi.MVS_NO_MODEL and (chi2 == 0.0).all()
    st, chi2, weight = ctx.pose_graph_edge_stats(m.indefinite(m.ring(17), 3))
    assert st == capi.MVS_NO_MODEL and (chi2 == 0.0).all()
    bad = m.ring(17)
    poses = bad["node_pose"].copy()
    poses[2, 4] = np.nan
    with pytest.raises(capi.MvsError) as e:
        ctx.pose_graph_edge_stats(bad, poses)
    assert e.value.status == capi.MVS_ERR_INVALID_ARG
    st, chi2, _ = ctx.pose_graph_edge_stats(m.dense_size(1))                # one node, no edge
    assert st == capi.MVS_OK and chi2.shape == (0,)
    st, chi2, _ = ctx.pose_graph_edge_stats(m.ring(17))
    assert st == capi.MVS_OK and (chi2 > 0.0).all()


def test_refusals_leave_the_setting_and_the_context(ctx):
    from mvslam_amd import capi

    g = m.ring(17)
    plain = ctx.pose_graph_optimize(g)
    with setting(ctx, rm.CAUCHY, 2.0, 3):
        robust = ctx.pose_graph_optimize(g)
        assert not same(robust, plain)
        for args in ((3, 1.0, 0), (-1, 1.0, 0), (capi.MVS_PG_LOSS_HUBER, 0.0, 0), (capi.MVS_PG_LOSS_HUBER, -1.0, 0),
                     (capi.MVS_PG_LOSS_CAUCHY, float("nan"), 0), (capi.MVS_PG_LOSS_CAUCHY, float("inf"), 0),
                     (capi.MVS_PG_LOSS_CAUCHY, 1.0, -2)):
            with pytest.raises(capi.MvsError) as e:
                ctx.set_pose_graph_loss(*args)
            assert e.value.status == capi.MVS_ERR_INVALID_ARG, args
            assert same(ctx.pose_graph_optimize(g), robust), args          # the previous setting is still in force
        # the loop edges of a host graph: accepted by the setter, refused by every host-graph call before anything runs
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_CAUCHY, 2.0, capi.MVS_PG_LOSS_LOOP_EDGES)
        for call in (lambda: ctx.pose_graph_optimize(g), lambda: ctx.pose_graph_optimize_batch([g, m.triangle(0)[0]]),
                     lambda: ctx.pose_graph_edge_stats(g)):
            with pytest.raises(capi.MvsError) as e:
                call()
            assert e.value.status == capi.MVS_ERR_INVALID_ARG
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_CAUCHY, 2.0, 3)
        assert same(ctx.pose_graph_optimize(g), robust)
    assert same(ctx.pose_graph_optimize(g), plain)                          # its usual bytes


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
def test_determinism(ctx, direct):
    for kind, k in ((rm.HUBER, rm.HUBER_K), (rm.CAUCHY, rm.CAUCHY_K)):
        for g, first in ((rm.outlier_ring(12), 24), (rm.outlier_ring(20), 40), (m.ring(200, chords=(5,)), 390)):
            with setting(ctx, kind, k, first, direct):
                a, b = ctx.pose_graph_optimize(g), ctx.pose_graph_optimize(g)
                sa, sb = ctx.pose_graph_edge_stats(g, a[2]), ctx.pose_graph_edge_stats(g, a[2])
            assert a[1]["ok"] == 1 and same(a, b) and same(sa, sb)


def test_kernel_resources_of_the_new_kernels():
    res = json.load(open(os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")))
    new = {k: v for k, v in res.items() if "pg_edge_stats_kernel" in k or "pg_dense_kernelILb1E" in k
           or "pg_edge_kernelILb0ELb1E" in k or "pg_edge_kernelILb1ELb1E" in k}
    assert len(new) == 4, sorted(new)
    for k, v in new.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0, (k, v)
        assert v["static_lds_bytes"] <= 64 * 1024, (k, v)
