"""GPU tests of the direct LM step of the pose graphs' large path (mvs_ctx_set_pose_graph_solver, pg_direct.hip; DESIGN.md
section 4.10.4) against the numpy model of its contract (tests/pg_direct_model.py).

Tolerance, device against model.  Both sides solve every step exactly and differ in summation order and libm; the bound is
the larger of the dense path's 1e-9 (DENSE_TOL of tests/test_pose_graph.py) and 10 x the gap between the model's scaled
skyline solve and numpy's dense Cholesky, measured on the CPU and committed in profiles/pose_graph_direct_vs_exact.json.  The
final error is compared relatively with the same bound.  Nothing here is derived from what the device returns."""
import json
import os

import numpy as np
import pytest

import pg_direct_model as dm
import pg_marginals_model as pgm
import posegraph_model as m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_TOL = 1e-9
SENTINEL = -12345.678


def _tol():
    rec = json.load(open(os.path.join(ROOT, "profiles", "pose_graph_direct_vs_exact.json")))
    return max(DENSE_TOL, 10.0 * rec["rotation"]), max(DENSE_TOL, 10.0 * rec["translation"])


def _pcg_tol():
    rec = json.load(open(os.path.join(ROOT, "profiles", "pose_graph_pcg_vs_exact.json")))
    return 10.0 * rec["rotation"], 10.0 * rec["translation"]


@pytest.fixture(scope="module")
def ctx():
    from mvslam_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture()
def direct(ctx):
    """the module's context with the direct solver selected for the length of a test"""
    from mvslam_amd import capi

    ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_DIRECT)
    yield ctx
    ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_PCG)


_MODEL = {}


def model(name, make, **kw):
    """optimize_direct's answer for a fixture, computed once per process and never modified"""
    key = (name, repr(sorted(kw.items())))
    if key not in _MODEL:
        g = make()
        _MODEL[key] = (g, dm.optimize_direct(g, **kw))
    return _MODEL[key]


def run(ctx, g, poses_out=None, **kw):
    from mvslam_amd import capi

    flat = dict(kw.pop("lm", None) or {}, **kw)
    return ctx.pose_graph_optimize(g, params=capi.default_pose_graph_params(**flat) if flat else None, poses_out=poses_out)


def check(res, poses, ref, what, counts=None):
    tr, tt = _tol()
    rot, trans = m.pose_distance(poses, ref["poses"])
    rel = abs(res["error"] - ref["error"]) / max(abs(ref["error"]), 1e-300) if ref["error"] > 1e-20 else abs(res["error"])
    print("%s: rotation %.3e translation %.3e error %.17g (model %.17g) iterations %d/%d rejected %d/%d" % (
        what, rot, trans, res["error"], ref["error"], res["iterations"], ref["iterations"], res["rejected_steps"],
        ref["rejected_steps"]))
    assert res["ok"] == 1 and ref["ok"] == 1 and res["cg_iterations"] == 0
    assert rot <= tr and trans <= tt, (what, rot, trans)
    assert rel <= max(tr, tt), (what, res["error"], ref["error"])
    assert abs(res["error_initial"] - ref["error_initial"]) <= 1e-9 * max(1.0, ref["error_initial"])
    if counts is None:
        counts = m.decision_margin(ref) >= 1e3
    if counts:
        assert (res["iterations"], res["rejected_steps"]) == (ref["iterations"], ref["rejected_steps"]), what


def test_switch(ctx):
    from mvslam_amd import capi

    g = m.ring(17)
    st, a, pa = ctx.pose_graph_optimize(g)
    assert st == capi.MVS_OK and a["cg_iterations"] > 0
    with pytest.raises(capi.MvsError):
        ctx.pose_graph_direct_info()                                        # nothing has gone through the direct solver yet
    ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_DIRECT)
    try:
        st, b, pb = ctx.pose_graph_optimize(g)
        assert st == capi.MVS_OK and b["ok"] == 1 and b["cg_iterations"] == 0
        for bad in (2, -1, 7):
            with pytest.raises(capi.MvsError) as e:
                ctx.set_pose_graph_solver(bad)
            assert e.value.status == capi.MVS_ERR_INVALID_ARG
        st, b2, _ = ctx.pose_graph_optimize(g)
        assert b2["cg_iterations"] == 0 and b2.tobytes() == b.tobytes()     # the setting was left alone
        info = ctx.pose_graph_direct_info()
        first, _, blocks = pgm.graph_envelope(g)
        assert info["envelope_blocks"] == blocks == 75 and info["widest_row"] == 17
        assert info["failed_solves"] == 0 and info["bad_node"] == -1 and 0.0 < info["min_pivot"] <= 1.0
    finally:
        ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_PCG)
    st, c, pc = ctx.pose_graph_optimize(g)
    assert c.tobytes() == a.tobytes() and pc.tobytes() == pa.tobytes()


def test_dense_graphs_are_untouched(ctx):
    from mvslam_amd import capi

    for g in (m.ring(16), m.trivial()[0]):
        _, a, pa = ctx.pose_graph_optimize(g)
        ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_DIRECT)
        try:
            _, b, pb = ctx.pose_graph_optimize(g)
        finally:
            ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_PCG)
        assert a["ok"] == 1 and a.tobytes() == b.tobytes() and pa.tobytes() == pb.tobytes()


PARITY = {"ring17": lambda: m.ring(17), "star70": m.star, "ring200": lambda: m.ring(200, chords=(5,)),
          "ring257": lambda: m.ring(257, chords=(7, 40)), "ring24_relabelled": pgm.FIXTURES["ring24_relabelled"],
          "chain40": pgm.chain40, "near_pi_ring": lambda: m.near_pi_ring()[0], "ring40": lambda: m.ring(40),
          "ring17_a16": lambda: m.permuted_ring("ring17_a16"), "ring17_a9": lambda: m.permuted_ring("ring17_a9")}


@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_with_the_model(direct, name):
    from mvslam_amd import capi

    g, ref = model(name, PARITY[name])
    if name == "ring40":                                                    # full covariances on more than 16 nodes
        assert all(abs(c.reshape(6, 6)[0, 4]) > 1e-7 for c in g["edge_cov"][:8])
    if name == "ring24_relabelled":
        assert pgm.graph_envelope(g)[2] == 246
    if name.startswith("ring17_a"):
        assert g["anchor"] in (9, 16)
    st, res, poses = direct.pose_graph_optimize(g)
    assert st == capi.MVS_OK
    check(res, poses, ref, name)
    info = direct.pose_graph_direct_info()
    assert info["envelope_blocks"] == pgm.graph_envelope(g)[2] and info["failed_solves"] == 0
    if name == "near_pi_ring":
        rot, trans = m.pose_distance(poses, m.near_pi_ring()[1])
        assert rot <= 1e-6 and trans <= 1e-6


def test_loose_anchor(direct):
    for name in ("loose_anchor17", "loose_anchor17_swapped"):
        make, kw = m.PARAM_RUNS[name]
        g, ref = model(name, make, **kw)
        st, res, poses = run(direct, g, **kw)
        check(res, poses, ref, name, counts=True)                           # two solves, the cap is the exit
        rot, trans = m.pose_distance(poses[0], g["node_pose"][0])
        assert rot > 1e-3 and trans > 1e-3                                  # the anchor moved


def test_lm_decisions(direct):
    g, ref = model("far_off20", lambda: m.far_off(20))
    assert ref["rejected_steps"] >= 1                                       # the model first, on the CPU
    st, res, poses = direct.pose_graph_optimize(g)
    check(res, poses, ref, "far off 20")
    assert res["rejected_steps"] >= 1
    for g in (m.ring(17),):
        st, res, poses = run(direct, g, lm=dict(max_iterations=0))
        assert res["ok"] == 1 and res["iterations"] == 0 and res["rejected_steps"] == 0 and res["cg_iterations"] == 0
        assert res["error"] == res["error_initial"] > 0.0 and poses.tobytes() == g["node_pose"].tobytes()
        ref = dm.optimize_direct(g, lm=dict(max_iterations=0))
        assert abs(res["error"] - ref["error"]) <= 1e-9 * ref["error"]
    kw = dict(lm=dict(max_iterations=2))
    g, ref = model("far_off20", lambda: m.far_off(20), **kw)
    assert ref["exit"] == "max_iterations"
    st, res, poses = run(direct, g, **kw)
    check(res, poses, ref, "far off 20, two iterations", counts=True)
    make, kw = m.PARAM_RUNS["lambda_upper20"]
    g, ref = model("lambda_upper20", make, **kw)
    assert ref["exit"] == "lambda_upper" and ref["rejected_steps"] >= 1
    st, res, poses = run(direct, g, **kw)
    check(res, poses, ref, "far off 20, lambda_upper")
    assert res["rejected_steps"] >= 1 and res["iterations"] < 100


def test_first_order_optimality_at_the_device_answer(direct):
    rec = json.load(open(os.path.join(ROOT, "profiles", "pose_graph_pcg_vs_exact.json")))["gradient_ratio"]["ring17"]
    g = m.ring(17)
    st, res, poses = direct.pose_graph_optimize(g)
    ratio = np.linalg.norm(m.gradient(g, poses)) / np.linalg.norm(m.gradient(g, g["node_pose"]))
    print("|J^T r| at the device's answer / at the initial values %.3e (bound %.3e)" % (ratio, 10.0 * rec["ratio"]))
    assert res["ok"] == 1 and ratio <= 10.0 * rec["ratio"]


def test_failures_leave_the_context_usable(direct):
    from mvslam_amd import capi

    good, ref = model("ring17", PARITY["ring17"])

    def still_works(what):
        st, res, poses = direct.pose_graph_optimize(good)
        assert st == capi.MVS_OK
        check(res, poses, ref, "ring 17 after " + what)

    out = np.full((4, 12), SENTINEL)
    st, res, _ = direct.pose_graph_optimize(m.disconnected(), poses_out=out)
    assert st == capi.MVS_NO_MODEL and res.tobytes() == bytes(32) and np.all(out == SENTINEL)
    r20 = m.ring(20, chords=())
    keep = [k for k in range(20) if 5 not in (int(r20["edge_src"][k]), int(r20["edge_dst"][k]))]
    cut = m.graph(r20["node_pose"], np.stack([r20["edge_src"], r20["edge_dst"]], axis=1)[keep], r20["edge_pose"][keep],
                  r20["edge_cov"][keep])                                    # 20 nodes, node 5 hangs on nothing
    assert not m.connected(cut)
    for g in (cut, m.indefinite(m.ring(17), 3), m.overflowing(m.ring(17))):
        n = g["node_pose"].shape[0]
        out = np.full((n, 12), SENTINEL)
        st, res, _ = direct.pose_graph_optimize(g, poses_out=out)
        assert st == capi.MVS_NO_MODEL and res.tobytes() == bytes(32) and np.all(out == SENTINEL)
        still_works("a failure")
    n = capi.POSE_GRAPH_MAX_NODES
    eye = m.se3([0, 0, 0], [0, 0, 0])
    hub = m.graph(np.tile(eye, (n, 1)), [(0, i) for i in range(1, n)], np.tile(eye, (n - 1, 1)), m.iso_cov(1.0, n - 1))
    assert pgm.graph_envelope(hub)[2] > pgm.MAX_ENVELOPE_BLOCKS
    with pytest.raises(capi.MvsError) as e:
        direct.pose_graph_optimize(hub)
    assert e.value.status == capi.MVS_ERR_CAPACITY
    with pytest.raises(capi.MvsError) as e:
        direct.pose_graph_optimize_batch([good, hub])
    assert e.value.status == capi.MVS_ERR_CAPACITY
    still_works("the refused hub")


def test_batch(direct):
    from mvslam_amd import capi

    graphs = [m.trivial()[0], m.ring(16), m.ring(17), m.ring(40)]
    single = [direct.pose_graph_optimize(g) for g in graphs]
    out = np.full((4, 40, 12), SENTINEL)
    st, res, poses = direct.pose_graph_optimize_batch(graphs, poses_out=out)
    assert st == capi.MVS_OK and poses is out
    for i, g in enumerate(graphs):
        n = g["node_pose"].shape[0]
        assert res[i]["ok"] == 1 and res[i]["cg_iterations"] == 0
        assert res[i].tobytes() == single[i][1].tobytes(), i
        assert out[i, :n].tobytes() == single[i][2].tobytes(), i
        assert np.all(out[i, n:] == SENTINEL), i


def test_determinism(direct):
    from mvslam_amd import capi

    g = m.ring(200, chords=(5,))
    a, b = direct.pose_graph_optimize(g), direct.pose_graph_optimize(g)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    other = capi.Context(0)
    try:
        other.set_pose_graph_solver(capi.MVS_PG_SOLVER_DIRECT)
        c = other.pose_graph_optimize(g)
    finally:
        other.close()
    assert a[1].tobytes() == c[1].tobytes() and a[2].tobytes() == c[2].tobytes()


def test_resident_sequence(ctx):
    from mvslam_amd import capi, synth

    import test_seq_loops as tl

    data = synth.make_loop_sequence(tl.LOOP_FRAMES, **tl.LOOP_ARGS)
    s = capi.Sequence(ctx, tl.LOOP_FRAMES, tl.N_KP, 32)
    try:
        s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
        s.upload_octaves(0, tl.st._octaves(tl.LOOP_FRAMES))
        s.run(tl._two_view(), tl.so._pnp())
        s.run_lags(tl._two_view(), 2)
        s.build_pose_graph(2)
        s.loop_scores(tl.MATCH["ratio"], tl.MATCH["max_dist"], tl.LOOP_GAP)
        s.select_loops(tl.LOOP_MIN_SCORE, tl.LOOP_TOP_K, tl.LOOP_CAP)
        s.verify_loops(tl._two_view())
        s.add_loop_edges()
        g = s.download_pose_graph()
        assert g["node_pose"].shape[0] == tl.LOOP_FRAMES > 16 and (g["edge_kind"] == 2).sum() >= 1
        st, pcg = s.optimize_pose_graph()
        assert st == capi.MVS_OK and pcg["cg_iterations"] > 0
        pcg_poses = s.download_pose_graph_poses()
        ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_DIRECT)
        try:
            st, res = s.optimize_pose_graph()
            poses = s.download_pose_graph_poses()
            st2, res2, poses2 = ctx.pose_graph_optimize(g)
        finally:
            ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_PCG)
        assert st == st2 == capi.MVS_OK and res["ok"] == 1 and res["cg_iterations"] == 0
        assert res.tobytes() == res2.tobytes() and poses.tobytes() == poses2.tobytes()
        rot, trans = m.pose_distance(poses, pcg_poses)
        tr, tt = _pcg_tol()
        print("resident graph, direct against PCG: rotation %.3e (bound %.3e) translation %.3e (bound %.3e)" % (rot, tr, trans, tt))
        assert rot <= tr and trans <= tt
        assert s.download_pose_graph_poses().tobytes() == poses.tobytes()
        st, info, cov = s.pose_graph_marginals()                            # accepted: the graph counts as optimised
        assert st in (capi.MVS_OK, capi.MVS_NO_MODEL) and info["envelope_blocks"] > 0
    finally:
        s.close()


def test_kernel_resources():
    res = json.load(open(os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if "PgdDev" in k}
    assert len(mine) == 4 and all(any(n in k for k in mine) for n in ("pgd_scale_kernel", "pgd_assemble_kernel",
                                                                       "pgd_factor_kernel", "pgd_solve_kernel"))
    for k, v in mine.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0, (k, v)
        assert v["static_lds_bytes"] <= 64 * 1024, (k, v)
