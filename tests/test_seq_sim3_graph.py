"""GPU tests of the resident graph of a sequence through the Sim(3) solver (mvs_seq_optimize_pose_graph_sim3): the loop
fixture of tests/test_seq_loops.py, lifted on the device, against mvs_sim3_graph_optimize on sim3graph_model.lift of the
downloaded graph, byte for byte; what the call leaves alone; what retires its result; its refusals."""
import numpy as np
import pytest

import sim3graph_model as m
import test_seq_loops as sl
import test_seq_odometry as so
import test_seq_track as st

pytestmark = pytest.mark.gpu
SCALE_SIGMA = (0.05, 0.2, 0.02)     # measured, fallback, loop: three different values, so that a kind read wrongly shows


@pytest.fixture(scope="module")
def loop_seq(ctx):
    """the loop fixture of tests/test_seq_loops.py: its frames, its selection, run and lags"""
    from mvslam_amd import capi, synth

    data = synth.make_loop_sequence(sl.LOOP_FRAMES, **sl.LOOP_ARGS)
    s = capi.Sequence(ctx, sl.LOOP_FRAMES, sl.N_KP, 32)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    s.upload_octaves(0, st._octaves(sl.LOOP_FRAMES))
    s.loop_scores(sl.MATCH["ratio"], sl.MATCH["max_dist"], sl.LOOP_GAP)
    s.select_loops(sl.LOOP_MIN_SCORE, sl.LOOP_TOP_K, sl.LOOP_CAP)
    s.run(sl._two_view(), so._pnp())
    s.run_lags(sl._two_view(), 2)
    yield s, data
    s.close()


def _raises(status, fn, *a, **kw):
    from mvslam_amd import capi

    with pytest.raises(capi.MvsError) as e:
        fn(*a, **kw)
    assert e.value.status == status


def _truth_gap(data, nodes):
    """largest distance between the camera centres of the generator and the nodes' positions, both in the frame of camera 0,
    after the one scale that fits them best"""
    R0, t0 = data["poses"][0]
    gt = np.array([R0 @ (-(R.T @ t)) + t0 for R, t in data["poses"]])
    est = np.asarray(nodes)[:, 9:12]
    s = float((est * gt).sum() / max((est * est).sum(), 1e-300))
    return float(np.linalg.norm(s * est - gt, axis=1).max())


def _against_the_host_call(ctx, s, g6, sigma=SCALE_SIGMA, params=None):
    from mvslam_amd import capi

    status, res = s.optimize_pose_graph_sim3(params=params, scale_sigma=sigma)
    nodes = s.download_pose_graph_sim3()
    g7 = m.lift(g6, sigma)
    assert all(m.chol7_ok(c) for c in g7["edge_cov"])
    st2, res2, nodes2 = ctx.sim3_graph_optimize(g7, params=params)
    print("sim3 on the resident graph: edges %d, error %.6e -> %.6e, iterations %d, cg %d, scales %.4f .. %.4f" % (
        g6["n_edges"], res["error_initial"], res["error"], res["iterations"], res["cg_iterations"], nodes[:, 12].min(),
        nodes[:, 12].max()))
    assert status == st2 == capi.MVS_OK and res["ok"] == 1 and res["error"] <= res["error_initial"]
    assert res.tobytes() == res2.tobytes() and nodes.tobytes() == nodes2.tobytes()
    return res, nodes


def test_gpu_resident_graph_with_loop_edges_through_sim3(ctx, loop_seq):
    from mvslam_amd import capi

    s, data = loop_seq
    s.verify_loops(sl._two_view())
    sl._built(s)
    _raises(capi.MVS_ERR_INVALID_ARG, s.download_pose_graph_sim3)           # before the call
    s.add_loop_edges(loop_sigma=(0.02, 0.2))
    g6 = s.download_pose_graph()
    assert (g6["edge_kind"] == 2).sum() >= 1 and g6["node_pose"].shape[0] == sl.LOOP_FRAMES > 16
    _raises(capi.MVS_ERR_INVALID_ARG, s.download_pose_graph_sim3)
    status, res6 = s.optimize_pose_graph()
    assert status == capi.MVS_OK
    se3_before = s.download_pose_graph_poses()
    res, nodes = _against_the_host_call(ctx, s, g6)
    assert res["cg_iterations"] > 0                                         # 24 frames: the large path
    # the call leaves the SE(3) optimised nodes and the graph as they were
    assert s.download_pose_graph_poses().tobytes() == se3_before.tobytes()
    after = s.download_pose_graph()
    for k, v in g6.items():
        assert np.array_equal(after[k], v), k
    # chunked conjugate gradient: the same bytes
    res_c, nodes_c = _against_the_host_call(ctx, s, g6, params=capi.default_sim3_graph_params(cg_chunk_iterations=16))
    assert res_c.tobytes() == res.tobytes() and nodes_c.tobytes() == nodes.tobytes()
    print("gap to the generator's trajectory: before %.4f, after SE(3) %.4f, after Sim(3) %.4f" % (
        _truth_gap(data, g6["node_pose"]), _truth_gap(data, se3_before), _truth_gap(data, nodes)))
    # refused scale sigmas leave the result of the last call in place
    for bad in ((0.0, 0.2, 0.02), (0.05, -0.2, 0.02), (0.05, 0.2, float("nan")), (float("inf"), 0.2, 0.02)):
        _raises(capi.MVS_ERR_INVALID_ARG, s.optimize_pose_graph_sim3, scale_sigma=bad)
    _raises(capi.MVS_ERR_INVALID_ARG, s.optimize_pose_graph_sim3, params=capi.default_sim3_graph_params(anchor_sigma=(1e-4, 1e-4, 0.0)))
    assert s.download_pose_graph_sim3().tobytes() == nodes.tobytes()
    # added loop edges and a rebuild retire the Sim(3) nodes
    s.add_loop_edges(loop_sigma=(0.02, 0.2))
    _raises(capi.MVS_ERR_INVALID_ARG, s.download_pose_graph_sim3)
    s.optimize_pose_graph_sim3(scale_sigma=SCALE_SIGMA)
    s.download_pose_graph_sim3()
    sl._built(s)
    _raises(capi.MVS_ERR_INVALID_ARG, s.download_pose_graph_sim3)


SHORT_FRAMES = 12


def test_gpu_short_sequence_without_loop_edges_takes_the_dense_path(ctx):
    from mvslam_amd import capi, synth

    data = synth.make_loop_sequence(SHORT_FRAMES, **sl.LOOP_ARGS)
    s = capi.Sequence(ctx, SHORT_FRAMES, sl.N_KP, 32)
    try:
        s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
        s.upload_octaves(0, st._octaves(SHORT_FRAMES))
        s.run(sl._two_view(), so._pnp())
        s.run_lags(sl._two_view(), 2)
        _raises(capi.MVS_ERR_INVALID_ARG, s.optimize_pose_graph_sim3)       # before the build
        g6 = sl._built(s, SHORT_FRAMES)
        assert g6["node_pose"].shape[0] == SHORT_FRAMES <= capi.POSE_GRAPH_DENSE_MAX_NODES and not (g6["edge_kind"] == 2).any()
        res, nodes = _against_the_host_call(ctx, s, g6)
        assert res["cg_iterations"] == 0                                    # the dense path
        _raises(capi.MVS_ERR_INVALID_ARG, s.download_pose_graph_poses)      # no SE(3) optimisation has run, and none was faked
    finally:
        s.close()
