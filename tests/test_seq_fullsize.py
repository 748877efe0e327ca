"""Every consumer of a resident sequence at full-size frames: FULL, 4 frames of 4096 keypoints (the
capacity), and WORK, 5 frames of 2000 keypoints (the benchmark's frame size), from tests/seq_fullsize.py.

Nothing here defines a comparison or a bound: each test calls the comparison of the consumer's own small test, on these
sequences -- test_seq_rescale._rescale_and_compare, test_seq_windows._check_assembly / _check_solve, test_seq_pose_graph.
_build_and_compare and its solver parity, test_seq_global._check_assembly / _check_plan / _check_solve, test_seq_track._replay,
test_seq_odometry._replay, and test_seq_loops' three checks on a loop sequence of 2000 keypoints.
tests/test_seq_fullsize_host.py shows on the CPU oracle alone which paths these sequences reach.

A sequence is uploaded, run and given its lagged pairs once per module.  No consumer retires the run or the lags; a rescale
retires what read the trajectory, so every test reads the trajectory afresh and builds its own windows, graph or problem.
mvs_seq_refine_windows admits 3 .. 8 frames, so the second window shape is F = 3 at stride 2 (test_seq_windows' own).
"""
import numpy as np
import pytest

import seq_fullsize as fs
import seq_global_model as ggm
import seq_graph_model as gm
import seq_loop_model as lm
import seq_rescale_model as rm
import test_ba_window as tw
import test_seq_global as sg
import test_seq_loops as tl
import test_seq_odometry as so
import test_seq_pose_graph as spg
import test_seq_rescale as sr
import test_seq_track as st
import test_seq_windows as sw

TRACKED = st.TRACKED


def _open(ctx, name):
    """upload, run (test_seq_windows' parameters), lags up to 2; dict(s, dev, seq, octave)"""
    seq = fs.make(name)
    F, N = seq["kp"].shape[:2]
    s, dev = st._run(ctx, seq, octave=fs.octaves(F, N))
    s.run_lags(so._params(), fs.MAX_LAG)
    return dict(s=s, dev=dev, seq=seq, name=name)


@pytest.fixture(scope="module")
def full(ctx):
    h = _open(ctx, "FULL")
    yield h
    h["s"].close()


@pytest.fixture(scope="module")
def work(ctx):
    h = _open(ctx, "WORK")
    yield h
    h["s"].close()


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return ggm.compile_planner(tmp_path_factory.mktemp("seq_fullsize_plan"), sanitize=False)


def _dev(h):
    """the builder's inputs with the trajectory the sequence holds now"""
    return dict(h["dev"], traj=h["s"].download_trajectory())


def _pick(request, which):
    return request.getfixturevalue(which.lower())


# ---------------------------------------------------------------------------------------------------------------------
# rescale

@pytest.mark.gpu
@pytest.mark.parametrize("which", ["FULL", "WORK"])
def test_gpu_fullsize_rescale_bitwise(request, which):
    from mvslam_amd import capi

    h = _pick(request, which)
    s = h["s"]
    N = s.max_kp
    pairs = rm.pairs_of_download(s.download_pairs())
    try:
        got, _ = sr._rescale_and_compare(s, pairs, 1)
        print("%s: n_common %s, n_used %s, scale %s" % (which, got["n_common"].tolist(), got["n_used"].tolist(),
                                                        got["scale"].tolist()))
        assert np.all(got["flag"] == 0) and all(p["valid"] for p in pairs)
        if which == "FULL":        # the device's own pairs reach what test_seq_fullsize_host.py shows on the oracle's
            j = np.concatenate([rm.shared_points(pairs[q], pairs[q + 1], N)[0] for q in range(len(pairs) - 1)])
            assert got["n_used"].max() > 1024 and (j >= 3072).any()
        else:
            assert all(len(p["point_idx"]) % 256 for p in pairs)
        low = int(got["n_used"].min())
        at, _ = sr._rescale_and_compare(s, pairs, low)
        assert np.all(at["flag"] == 0)
        above, _ = sr._rescale_and_compare(s, pairs, low + 1)
        assert np.array_equal(above["flag"] == 2, got["n_used"] == low) and np.all(above["scale"][above["flag"] == 2] == 1.0)
    finally:
        s.rescale(capi.SEQ_SCALE_CHAIN)     # the run's trajectory again


# ---------------------------------------------------------------------------------------------------------------------
# windows

@pytest.mark.gpu
@pytest.mark.parametrize("F,stride", [(4, 1), (3, 2)])
@pytest.mark.parametrize("which", ["FULL", "WORK"])
def test_gpu_fullsize_windows_assembly_and_solve(ctx, request, which, F, stride):
    from mvslam_amd import capi

    h = _pick(request, which)
    s, dev = h["s"], _dev(h)
    params = capi.default_refine_params()
    s.refine_windows(F, stride, 4096, params, fs.SIGMA_PX)
    got = s.download_windows()
    sw._check_assembly(got, dev, F, stride, 4096)
    sw._check_solve(ctx, got, dev, params, fs.SIGMA_PX)
    print("%s F = %d stride %d: points %s, ok %s" % (which, F, stride, [g["n_points"] for g in got], [g["ok"] for g in got]))
    assert max(g["n_points"] for g in got) > 1024


# ---------------------------------------------------------------------------------------------------------------------
# pose graph

@pytest.mark.gpu
@pytest.mark.parametrize("which", ["FULL", "WORK"])
def test_gpu_fullsize_pose_graph_bytes_and_solver_parity(ctx, request, which):
    from mvslam_amd import capi

    h = _pick(request, which)
    s = h["s"]
    traj, tables = s.download_trajectory(), spg._tables(s, fs.MAX_LAG)
    for max_lag in (1, 2):
        got, _ = spg._build_and_compare(s, traj, tables, max_lag)
        assert got["n_edges"] == gm.n_slots(s.n_frames, max_lag) and not got["edge_kind"].any()     # every edge is valid
    status, res = s.optimize_pose_graph()
    poses = s.download_pose_graph_poses()
    st2, res2, poses2 = ctx.pose_graph_optimize(got)
    print(which, {k: res[k] for k in spg.RESULT_FIELDS})
    assert status == st2 == capi.MVS_OK
    assert res.tobytes() == res2.tobytes() and poses.tobytes() == poses2.tobytes()
    assert res["ok"] == 1 and res["error"] <= res["error_initial"] and res["iterations"] >= 1


# ---------------------------------------------------------------------------------------------------------------------
# global bundle adjustment

@pytest.mark.gpu
@pytest.mark.parametrize("T", [0, 3])
@pytest.mark.parametrize("which", ["FULL", "WORK"])
def test_gpu_fullsize_global_assembly_plan_and_solve(ctx, request, planner, which, T):
    from mvslam_amd import capi

    h = _pick(request, which)
    s, dev = h["s"], _dev(h)
    params = capi.default_refine_params()
    res = s.refine_global(T, params, fs.SIGMA_PX)
    got, want = sg._check_assembly(s, dev, T)
    plan = sg._check_plan(s, planner, got)
    sg._check_solve(ctx, s, dev, got, res, params, fs.SIGMA_PX)
    rows = np.diff(plan["fr_off"])
    print("%s T = %d: plan rows %s" % (which, T, rows.tolist()))
    assert res["widest_row"] == plan["widest"][0] == int(np.diff(want["obs_off"]).max()) == (T or s.n_frames)
    assert res["envelope_blocks"] == plan["blocks"][0] and (T or rows.max() > 1024)


# ---------------------------------------------------------------------------------------------------------------------
# tracking and odometry

@pytest.mark.gpu
def test_gpu_fullsize_track_replay(ctx, work):
    from mvslam_amd import capi

    s, dev = work["s"], work["dev"]
    vo, rp = capi.default_vo_params(max_error=1e30), capi.default_refine_params()
    s.track(vo, st._pnp_params(), rp)
    snap = st._snapshot(s)
    fr = snap["frames"]
    print("states", fr["state"].tolist(), "candidates", fr["n_cand"].tolist(), "tracked", fr["n_tracked"].tolist(),
          "new", fr["n_new"].tolist())
    st._replay(ctx, snap, dev, vo, st._pnp_params(), rp)
    assert fr["state"][2] == TRACKED, "the fixture loses track at its first step: the test shows nothing"
    assert fr["n_cand"][2] > 256 and fr["n_new"][2] > 0             # the join and the map cross the 256-wide chunks


@pytest.mark.gpu
def test_gpu_fullsize_odometry_replay(ctx, work):
    from mvslam_amd import capi

    s, seq = work["s"], work["seq"]
    F, N = seq["kp"].shape[:2]
    vo, ip, rp = so._vo(), so._init(2), capi.default_refine_params()
    s.odometry(vo, ip, so._pnp(), rp)
    snap, odo = so._replay(ctx, s, seq, vo, ip, so._pnp(), rp, n_frames=F, octaves=fs.octaves(F, N))
    # On WORK the refined initialisation's first step ends LOST_BA (a prior-less new point runs off: test_seq_track.py's
    # docstring on its seed; mvs_ba_refine on the downloaded problem says the same, which the replay asserts), the queue
    # restarts and frame 4 tracks in a second segment: the replay covers a loss, a re-initialisation and a tracked step.
    fr = snap["frames"]
    tracked = fr["state"] == TRACKED
    assert odo["init_base"][1] == 0 and fr["state"][:2].tolist() == [so.INIT, so.INIT]
    assert tracked.any(), "the fixture tracks no frame: the test shows nothing"
    assert (fr["n_cand"][tracked] > 256).all() and (fr["n_cand"][2:] > 256).any()


# ---------------------------------------------------------------------------------------------------------------------
# loops: 10 frames of 2000 keypoints

@pytest.fixture(scope="module")
def loop2000(ctx):
    from mvslam_amd import capi

    data = fs.make_loop()
    F, N = data["kp"].shape[:2]
    s = capi.Sequence(ctx, F, N, 32)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    s.upload_octaves(0, st._octaves(F, N))
    s.loop_scores(tl.MATCH["ratio"], tl.MATCH["max_dist"], tl.LOOP_GAP)
    s.select_loops(tl.LOOP_MIN_SCORE, tl.LOOP_TOP_K, tl.LOOP_CAP)
    s.run(tl._two_view(), so._pnp())
    s.run_lags(tl._two_view(), 2)
    yield s, data
    s.close()


@pytest.mark.gpu
def test_gpu_fullsize_loop_selection_equals_the_model(loop2000):
    s, data = loop2000
    table = s.download_loop_scores()
    assert np.array_equal(table, lm.scores(data["desc"], data["n_kp"], tl.MATCH["ratio"], tl.MATCH["max_dist"], tl.LOOP_GAP))
    try:
        # everything, one a column, a cut list, a minimum between the scores, a minimum above them
        cut = int(np.sort(table[table > 0])[-2])
        tl.check_selection_equals_the_model(s, table, ((1, 3, 1000), (1, 1, 1000), (1, 3, 2), (cut, 2, 8), (100000, 2, 4)))
        want, found = lm.select(table, tl.LOOP_MIN_SCORE, tl.LOOP_TOP_K, tl.LOOP_CAP)
        assert (0, fs.LOOP_FRAMES - 1) in [(i, j) for i, j, _ in want] and found == 3 > 2
    finally:
        s.select_loops(tl.LOOP_MIN_SCORE, tl.LOOP_TOP_K, tl.LOOP_CAP)    # the module's list again


@pytest.mark.gpu
def test_gpu_fullsize_loop_verification_equals_an_uploaded_batch(ctx, loop2000):
    s, data = loop2000
    tl.check_verification_equals_an_uploaded_batch(ctx, s, data, False, n_kp=data["kp"].shape[1])


@pytest.mark.gpu
def test_gpu_fullsize_loop_edges_equal_the_model_and_optimise(ctx, loop2000):
    s, _ = loop2000
    tl.check_loop_edges_equal_the_model_and_optimise(ctx, s, n_frames=fs.LOOP_FRAMES)


# ---------------------------------------------------------------------------------------------------------------------
# determinism: every consumer twice on FULL

def _raw(d):
    return b"".join(np.ascontiguousarray(d[k]).tobytes() for k in sorted(d) if isinstance(d[k], np.ndarray))


@pytest.mark.gpu
def test_gpu_fullsize_every_consumer_twice_gives_the_same_bytes(ctx, full):
    from mvslam_amd import capi

    s = full["s"]
    rp = capi.default_refine_params()

    def rescale():
        s.rescale(capi.SEQ_SCALE_DEPTH_RATIO, 1)
        out = s.download_scale_steps().tobytes() + sr._traj_bytes(s.download_trajectory())
        s.rescale(capi.SEQ_SCALE_CHAIN)
        return out

    def windows():
        s.refine_windows(4, 1, 4096, rp, fs.SIGMA_PX)
        return b"".join(tw._bytes(g) + g["track_kp"].tobytes() + g["point_guess"].tobytes() for g in s.download_windows())

    def pose_graph():
        s.build_pose_graph(fs.MAX_LAG)
        g = s.download_pose_graph()
        status, res = s.optimize_pose_graph()
        assert status == capi.MVS_OK
        return b"".join(np.ascontiguousarray(g[k]).tobytes() for k in gm.GRAPH_KEYS) + res.tobytes() + \
            s.download_pose_graph_poses().tobytes()

    def global_ba():
        res = s.refine_global(0, rp, fs.SIGMA_PX)
        prob = s.download_global_problem()
        return res["raw"] + s.download_global()["raw"] + b"".join(prob[k].tobytes() for k in sorted(prob)) + \
            b"".join(np.array(v, np.int64).tobytes() for _, v in sorted(sg._device_plan(s).items()))

    def track():
        s.track(capi.default_vo_params(max_error=1e30), st._pnp_params(), rp)
        snap = st._snapshot(s)
        return b"".join(st._frame_bytes(snap, f) for f in range(s.n_frames))

    def odometry():
        s.odometry(so._vo(), so._init(2), so._pnp(), rp)
        snap = st._snapshot(s)
        return b"".join(st._frame_bytes(snap, f) for f in range(s.n_frames)) + s.download_odometry_frames().tobytes()

    def loops():
        s.loop_scores(tl.MATCH["ratio"], tl.MATCH["max_dist"], 2)
        s.select_loops(1, 2, 8)
        s.verify_loops(tl._two_view())
        s.build_pose_graph(fs.MAX_LAG)
        s.add_loop_edges(loop_sigma=(0.02, 0.2))
        cd = s.download_loop_candidates(pairs=True)
        assert cd["n_kept"] == 3
        g = s.download_pose_graph()
        return s.download_loop_scores().tobytes() + _raw(cd) + b"".join(np.ascontiguousarray(g[k]).tobytes() for k in gm.GRAPH_KEYS)

    for consumer in (rescale, windows, pose_graph, global_ba, track, odometry, loops):
        first, second = consumer(), consumer()
        assert len(first) > 0 and first == second, consumer.__name__
