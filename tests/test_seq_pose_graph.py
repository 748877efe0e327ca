"""The pose graph of a resident sequence on the device: mvs_seq_build_pose_graph / _optimize_pose_graph (seq_graph.hip,
DESIGN.md section 4.10.1) against the numpy definition tests/seq_graph_model.py and against mvs_pose_graph_optimize on the
downloaded graph, and the chunked CG enqueue of the large path (mvs_pose_graph_params.cg_chunk_iterations).

Shapes: test_seq_windows.SEQ_ARGS with the generator seed of test_seq_track.py, 300 keypoints, 600 two-view hypotheses, 100
PnP hypotheses, lags up to 3; 8 frames (dense path) and 20 frames of the same generator (N = 20 > 16: the large path).  The
two sequences are run once per module and only read afterwards; every test builds its own graph on them."""
import numpy as np
import pytest

import posegraph_model as pm
import seq_graph_model as gm
import test_seq_odometry as so
import test_seq_track as st
import test_seq_windows as sw

N_KP, MAX_LAG, OPEN = 300, 3, 1e30
RESULT_FIELDS = ("ok", "iterations", "cg_iterations", "rejected_steps", "error_initial", "error")


def _open(ctx, n_frames, n_kp=None, max_lag=MAX_LAG):
    from mvslam_amd import capi, synth

    seq = synth.make_sequence(n_frames, seed=st.SEED, **sw.SEQ_ARGS)
    s = capi.Sequence(ctx, n_frames, N_KP, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"] if n_kp is None else n_kp(seq["n_kp"].copy()), seq["K"])
    s.upload_octaves(0, st._octaves(n_frames))
    s.run(so._params(), so._pnp())
    if max_lag:
        s.run_lags(so._params(), max_lag)
    return s


def _tables(s, max_lag=MAX_LAG):
    pairs = {d: s.download_lag_pairs(d) for d in range(1, max_lag + 1)}
    refined = {d: s.download_lag_refined(d, points=False) for d in range(1, max_lag + 1)}
    return gm.tables_from_downloads(pairs, refined)


@pytest.fixture(scope="module")
def seq8(ctx):
    s = _open(ctx, 8)
    yield s, s.download_trajectory(), _tables(s)
    s.close()


@pytest.fixture(scope="module")
def seq20(ctx):
    s = _open(ctx, 20)
    yield s, s.download_trajectory(), _tables(s)
    s.close()


def _build_and_compare(s, traj, tables, max_lag, **kw):
    """build on the device, download, compare every array with the model's; returns (device graph, model graph)"""
    s.build_pose_graph(max_lag, **kw)
    got = s.download_pose_graph()
    want = gm.build(traj["R"], traj["t"], tables, max_lag, **kw)
    print("max_lag", max_lag, kw, "edges", got["n_edges"], "of", gm.n_slots(s.n_frames, max_lag), "slots; per lag",
          np.bincount(got["edge_lag"], minlength=max_lag + 1)[1:].tolist(), "kinds", np.bincount(got["edge_kind"], minlength=2).tolist())
    assert gm.same_bytes(got, want) == []
    return got, want


# ---------------------------------------------------------------------------------------------------------------------
# 1 assembly

@pytest.mark.gpu
@pytest.mark.parametrize("which", ["seq8", "seq20"])
@pytest.mark.parametrize("max_lag", [1, 3])
def test_gpu_assembly_bytes(request, which, max_lag):
    s, traj, tables = request.getfixturevalue(which)
    got, _ = _build_and_compare(s, traj, tables, max_lag)
    per_lag = np.bincount(got["edge_lag"], minlength=max_lag + 1)[1:]
    assert np.all(per_lag >= 1), "a lag contributes no edge: %s" % per_lag.tolist()
    assert not got["edge_kind"].any() and np.all(got["edge_scale"] > 0.0)
    assert got["node_pose"].tobytes() == np.concatenate([traj["R"].reshape(-1, 9), traj["t"]], axis=1).tobytes()
    if max_lag == 3:
        assert got["n_edges"] > s.n_frames - 1, "the graph of max_lag 3 is no more than a chain"


# ---------------------------------------------------------------------------------------------------------------------
# 2 gates

@pytest.mark.gpu
def test_gpu_gates_from_the_tables(seq8):
    s, traj, tables = seq8
    full, _ = _build_and_compare(s, traj, tables, 3)
    err = np.array([tables[d][k]["error"] for d, k in zip(full["edge_lag"], full["edge_src"])])
    order = np.argsort(err)
    hi, nxt = err[order[-1]], err[order[-2]]
    gate = 0.5 * (hi + nxt)
    every = [e["error"] for d in tables for e in tables[d] if e["valid"] and e["ok"]]
    assert all(so._far(v, gate) for v in every), "the error gate sits within 1e-6 of a gated value"
    got, _ = _build_and_compare(s, traj, tables, 3, max_error=gate)
    lost = (int(full["edge_lag"][order[-1]]), int(full["edge_src"][order[-1]]))
    assert got["n_edges"] == full["n_edges"] - 1
    assert lost not in list(zip(got["edge_lag"].tolist(), got["edge_src"].tolist()))
    # a whole lag: more points than any pair of that lag has.  The lag is the one whose best pair is the poorest.
    pts = {d: max(tables[d][k]["n_points"] for dd, k in zip(full["edge_lag"], full["edge_src"]) if dd == d) for d in (1, 2, 3)}
    d_lost = min(pts, key=pts.get)
    got, _ = _build_and_compare(s, traj, tables, 3, min_points=pts[d_lost] + 1)
    per_lag = np.bincount(got["edge_lag"], minlength=4)[1:]
    assert per_lag[d_lost - 1] == 0 and got["n_edges"] > 0, per_lag.tolist()
    assert sorted(pts.values())[1] > pts[d_lost], "two lags share the largest point count: the gate drops both"
    # both gates at once, and the open gate spelled out
    _build_and_compare(s, traj, tables, 3, max_error=gate, min_points=pts[d_lost] + 1)
    again, _ = _build_and_compare(s, traj, tables, 3, max_error=OPEN, min_points=0)
    assert gm.same_bytes(again, full) == []


# ---------------------------------------------------------------------------------------------------------------------
# 3 fallback and connectivity: fixture (b) of test_seq_odometry.py

@pytest.mark.gpu
def test_gpu_fallback_and_connectivity(ctx):
    from mvslam_amd import capi

    def five_at_4(n_kp):
        n_kp[4] = 5
        return n_kp

    s = _open(ctx, 8, n_kp=five_at_4)
    try:
        traj, tables = s.download_trajectory(), _tables(s)
        assert not tables[1][3]["valid"] and not tables[1][4]["valid"], "fixture (b): pairs (3, 4) and (4, 5) are invalid"
        # lag 1 alone, no fallback: frame 4 hangs on nothing
        g1, _ = _build_and_compare(s, traj, tables, 1)
        assert 3 not in g1["edge_src"].tolist() and 4 not in g1["edge_src"].tolist() and not pm.connected(g1)
        status, res = s.optimize_pose_graph()
        assert status == capi.MVS_NO_MODEL and res["ok"] == 0 and res.tobytes() == bytes(res.nbytes)
        with pytest.raises(capi.MvsError) as e:
            s.download_pose_graph_poses()
        assert e.value.status == capi.MVS_ERR_INVALID_ARG
        # with the fallback: the two chain edges in slots (1, 3) and (1, 4)
        sig = (0.05, 0.5)
        g2, _ = _build_and_compare(s, traj, tables, 1, chain_sigma=sig)
        assert g2["n_edges"] == 7 and g2["edge_src"].tolist() == list(range(7))      # with the fallback every slot of lag 1 holds an edge
        assert g2["edge_kind"][3] == g2["edge_kind"][4] == 1 and g2["edge_scale"][3] == g2["edge_scale"][4] == 1.0
        assert g2["edge_kind"][:3].tolist() == [0, 0, 0]                             # the pairs in front of the gap are measured
        assert g2["edge_cov"][3].tobytes() == np.diag([sig[0] * sig[0]] * 3 + [sig[1] * sig[1]] * 3).reshape(36).tobytes()
        status, res = s.optimize_pose_graph()
        assert status == capi.MVS_OK and res["ok"] == 1 and res["error"] <= res["error_initial"]
        poses = s.download_pose_graph_poses()
        st2, res2, poses2 = ctx.pose_graph_optimize(g2)
        assert st2 == capi.MVS_OK and res2.tobytes() == res.tobytes() and poses2.tobytes() == poses.tobytes()
        # lags up to 3 and no fallback: whatever the tables say about the lagged pairs over the gap
        g3, want3 = _build_and_compare(s, traj, tables, 3)
        edges = set(zip(g3["edge_src"].tolist(), g3["edge_dst"].tolist()))
        usable = lambda d, k: tables[d][k]["valid"] and tables[d][k]["ok"]
        for d, k in ((2, 2), (2, 3), (3, 1), (3, 2), (3, 3), (2, 4), (3, 4)):   # every lagged pair that touches or spans frame 4
            # a usable pair over a trajectory step of length zero has scale 0 and is no edge: the definition decides
            print("pair", (k, k + d), "usable" if usable(d, k) else "not usable", "edge" if (k, k + d) in edges else "no edge")
            assert ((k, k + d) in edges) == ((d, k) in want3["slots"]) and ((k, k + d) not in edges or usable(d, k))
        bridged = pm.connected(want3)
        status, res = s.optimize_pose_graph()
        print("lagged edges bridge the gap:", bridged, "status", status)
        assert (status == capi.MVS_OK and res["ok"] == 1) if bridged else (status == capi.MVS_NO_MODEL and res["ok"] == 0)
        if not bridged:
            with pytest.raises(capi.MvsError):
                s.download_pose_graph_poses()
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4 solver parity

LM_OTHER = dict(lambda_initial=1e-2, lambda_factor=4.0, max_iterations=7)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["seq8", "seq20"])
@pytest.mark.parametrize("lm", [{}, LM_OTHER], ids=["default", "other_lm"])
def test_gpu_solver_parity_with_the_host_pointer_call(ctx, request, which, lm):
    from mvslam_amd import capi

    s, traj, tables = request.getfixturevalue(which)
    s.build_pose_graph(3)
    g = s.download_pose_graph()
    prm = capi.default_pose_graph_params(**lm)
    status, res = s.optimize_pose_graph(prm)
    poses = s.download_pose_graph_poses()
    st2, res2, poses2 = ctx.pose_graph_optimize(g, capi.default_pose_graph_params(**lm))
    print(which, lm, {k: res[k] for k in RESULT_FIELDS})
    assert status == st2 == capi.MVS_OK
    assert res.tobytes() == res2.tobytes() and poses.tobytes() == poses2.tobytes()
    assert res["ok"] == 1 and res["error"] <= res["error_initial"] and res["iterations"] >= 1
    if s.n_frames <= capi.POSE_GRAPH_DENSE_MAX_NODES:
        assert res["cg_iterations"] == 0
    else:
        assert res["cg_iterations"] > 0
    assert s.download_pose_graph_poses().tobytes() == poses.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5 chunked CG enqueue

def _same_result(a, b):
    return all(a[0][k] == b[0][k] for k in RESULT_FIELDS) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [0, 5], ids=["full_budget", "budget_cut_to_5"])
def test_gpu_chunked_cg_gives_the_unchunked_bytes(ctx, seq20, cut):
    """chunks of 1, 7 and 64 CG iterations against the whole budget at once, on the 20-frame sequence graph through the
    sequence call and on posegraph_model's ring through mvs_pose_graph_optimize.  cut = 5: cg_max_iterations = 5, so a chunk of
    7 or 64 holds the whole budget, a chunk of 1 ends on it, and the budget runs out inside the chunk of 7"""
    from mvslam_amd import capi

    s, _, _ = seq20
    s.build_pose_graph(3)
    ring = pm.ring(17)
    # the cut run is one LM iteration, so that its CG count says whether the budget was what ended the solve
    prm = lambda chunk: capi.default_pose_graph_params(cg_chunk_iterations=chunk, cg_max_iterations=cut,
                                                       **(dict(max_iterations=1) if cut else {}))

    def run_seq(chunk):
        status, res = s.optimize_pose_graph(prm(chunk))
        assert status == capi.MVS_OK
        return res, s.download_pose_graph_poses()

    def run_ring(chunk):
        status, res, poses = ctx.pose_graph_optimize(ring, prm(chunk))
        assert status == capi.MVS_OK
        return res, poses

    for run in (run_seq, run_ring):
        base = run(0)
        print(run.__name__, "cut", cut, {k: base[0][k] for k in RESULT_FIELDS})
        assert base[0]["ok"] == 1 and base[0]["cg_iterations"] > 0
        if cut:
            assert base[0]["iterations"] == 1 and base[0]["cg_iterations"] == cut, "the cut budget does not bind"
        for chunk in (1, 7, 64):
            assert _same_result(run(chunk), base), (run.__name__, chunk)
        assert _same_result(run(-3), base)            # anything <= 0 is the whole budget


# ---------------------------------------------------------------------------------------------------------------------
# 6 refusals and side effects

def _status_of(fn, *a, **kw):
    from mvslam_amd import capi

    with pytest.raises(capi.MvsError) as e:
        fn(*a, **kw)
    return e.value.status


@pytest.mark.gpu
def test_gpu_refusals_and_side_effects(ctx, seq8):
    from mvslam_amd import capi

    s, _, _ = seq8
    I, CAP = capi.MVS_ERR_INVALID_ARG, capi.MVS_ERR_CAPACITY
    s.track(so._vo(), so._pnp(), capi.default_refine_params())

    def snapshot():
        out = [s.download_pairs(), s.download_tracks(), s.download_trajectory(), s.download_refined(point_cov=True)]
        for d in range(1, MAX_LAG + 1):
            out += [s.download_lag_pairs(d), s.download_lag_refined(d, point_cov=True)]
        snap = st._snapshot(s)
        return b"".join(x[k].tobytes() for x in out for k in sorted(x) if x[k] is not None) + \
            b"".join(st._frame_bytes(snap, f) for f in range(s.n_frames))

    before = snapshot()
    s.build_pose_graph(3, chain_sigma=(0.05, 0.5))
    g = s.download_pose_graph()
    status, res = s.optimize_pose_graph()
    assert status == capi.MVS_OK
    poses = s.download_pose_graph_poses()
    assert snapshot() == before
    # determinism: the same build and solve again
    s.build_pose_graph(3, chain_sigma=(0.05, 0.5))
    assert _status_of(s.download_pose_graph_poses) == I                    # a new graph: not optimised yet
    assert gm.same_bytes(s.download_pose_graph(), g) == []
    status, res2 = s.optimize_pose_graph()
    assert res2.tobytes() == res.tobytes() and s.download_pose_graph_poses().tobytes() == poses.tobytes()
    # arguments
    for kw in (dict(max_lag=0), dict(max_lag=-1), dict(max_lag=MAX_LAG + 1), dict(max_lag=s.n_frames), dict(min_points=-1),
               dict(max_error=-1.0), dict(max_error=float("nan")), dict(chain_sigma=(float("nan"), 1.0))):
        assert _status_of(s.build_pose_graph, **dict(dict(max_lag=2), **kw)) == I, kw
    s.build_pose_graph(2)                                                     # a refused build left nothing half done
    for kw in (dict(lambda_factor=1.0), dict(max_iterations=-1), dict(anchor_sigma=(0.0, 1.0)), dict(cg_max_iterations=-1),
               dict(cg_rel_tol=float("nan"))):
        assert _status_of(s.optimize_pose_graph, capi.default_pose_graph_params(**kw)) == I, kw
    fresh = capi.Sequence(ctx, 8, N_KP, 32)
    try:
        assert _status_of(fresh.build_pose_graph, 1) == I                     # not run
        assert _status_of(fresh.optimize_pose_graph) == I and _status_of(fresh.download_pose_graph) == I
        assert _status_of(fresh.download_pose_graph_poses) == I
    finally:
        fresh.close()
    # capacity is a matter of n_frames and max_lag alone: reported before the state of the sequence is looked at
    for frames, lag, want in ((4097, 1, CAP), (4096, 17, CAP), (4096, 16, I)):  # 4096 * 17 - 153 = 69 479 > 65 536 >= 65 400
        big = capi.Sequence(ctx, frames, 16, 32)
        try:
            assert _status_of(big.build_pose_graph, lag) == want, (frames, lag)
        finally:
            big.close()


@pytest.mark.gpu
def test_gpu_build_after_a_new_run_refuses(ctx):
    from mvslam_amd import capi

    s = _open(ctx, 8, max_lag=2)
    try:
        s.build_pose_graph(2)
        assert s.optimize_pose_graph()[0] == capi.MVS_OK
        s.run(so._params(), so._pnp())                                        # the lags belonged to the run before
        I = capi.MVS_ERR_INVALID_ARG
        assert _status_of(s.build_pose_graph, 1) == I and _status_of(s.optimize_pose_graph) == I
        assert _status_of(s.download_pose_graph) == I and _status_of(s.download_pose_graph_poses) == I
        s.run_lags(so._params(), 1)
        assert _status_of(s.build_pose_graph, 2) == I                         # lag 2 is not resident now
        s.build_pose_graph(1)
        assert s.download_pose_graph()["n_edges"] >= 1
    finally:
        s.close()
