"""The scale of a resident sequence from depth ratios of shared points on the device: mvs_seq_rescale and
mvs_seq_download_scale_steps against the numpy model of tests/seq_rescale_model.py.

The model is fed the device's own downloaded pairs and must give every step record (integers equal, scale bitwise),
track_scale, pair_scale and the trajectory byte for byte: the definition fixes every operation and its order.
tests/test_seq_rescale_host.py shows on the CPU that the sequences exercise what is compared here.
"""
import ctypes as C

import numpy as np
import pytest

import seq_rescale_model as rm
import test_seq_pose_graph as spg
import test_seq_windows as sw
from mvslam_amd import synth
from test_seq_global_host import LONG_ARGS, LONG_FRAMES, LONG_T
from test_seq_rescale_host import WIDE_ARGS, shared_twice, twin_sequence

TRAJ_KEYS = ("R", "t", "pair_scale", "track_scale")


def _params():
    from mvslam_amd import capi

    return (capi.default_params(num_hypotheses=sw.PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=sw.PRM["seed"],
                                max_error_sq=sw.PRM["thr"]),
            capi.default_pnp_params(num_hypotheses=sw.PPRM["H"], seed=sw.PPRM["seed"], reproj_error=sw.PPRM["err"]))


def _open(ctx, seq, n_kp=None, essential=False):
    """upload and run; returns the open Sequence, the model's pairs from its download, and the run's trajectory"""
    from mvslam_amd import capi

    F, N = seq["kp"].shape[0], seq["kp"].shape[1]
    s = capi.Sequence(ctx, F, N, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"] if n_kp is None else n_kp, seq["K"])
    (s.run_essential if essential else s.run)(*_params())
    return s, rm.pairs_of_download(s.download_pairs()), s.download_trajectory()


def _traj_bytes(traj):
    return b"".join(traj[k].tobytes() for k in TRAJ_KEYS)


def _status_of(fn, *a, **kw):
    from mvslam_amd import capi

    with pytest.raises(capi.MvsError) as e:
        fn(*a, **kw)
    return e.value.status


def _rescale_and_compare(s, pairs, min_common=1):
    """DEPTH_RATIO on the device against the model on the device's pairs; returns (records, trajectory)"""
    from mvslam_amd import capi

    s.rescale(capi.SEQ_SCALE_DEPTH_RATIO, min_common)
    got, traj = s.download_scale_steps(), s.download_trajectory()
    want, wtraj = rm.rescale(pairs, s.max_kp, min_common)
    for k in ("n_common", "n_used", "flag", "reserved"):
        assert np.array_equal(got[k], want[k]), k
    assert got["scale"].tobytes() == want["scale"].tobytes()
    for k in TRAJ_KEYS:
        assert traj[k].tobytes() == wtraj[k].tobytes(), k
    assert traj["track_scale"].tobytes() == got["scale"].tobytes()
    return got, traj


@pytest.fixture(scope="module")
def six(ctx):
    """test_seq_global's sequence (6 frames of 300 keypoints), run once; rescaled by the tests, never run again"""
    seq = sw.make_seq()
    s, pairs, traj0 = _open(ctx, seq)
    yield s, pairs, traj0, seq
    s.close()


@pytest.fixture(scope="module")
def long_seq(ctx):
    """test_seq_global's 260 frames of 96 keypoints, run once"""
    s, pairs, traj0 = _open(ctx, synth.make_sequence(LONG_FRAMES, **LONG_ARGS))
    yield s, pairs, traj0
    s.close()


@pytest.mark.gpu
def test_gpu_rescale_six_frames_bitwise(ctx, six):
    s, pairs, _, _ = six
    got, traj = _rescale_and_compare(s, pairs)
    print("six frames: n_common %s, n_used %s, scale %s; %d keypoints shared twice"
          % (got["n_common"].tolist(), got["n_used"].tolist(), got["scale"].tolist(), shared_twice(pairs, 300)))
    assert np.all(got["flag"] == 0) and got["n_used"].min() >= 50 and all(p["valid"] for p in pairs)
    # min_common at and above the smallest n_used: the step with it keeps its ratio, then keeps the scale
    low = int(got["n_used"].min())
    at, _ = _rescale_and_compare(s, pairs, low)
    assert np.all(at["flag"] == 0)
    above, _ = _rescale_and_compare(s, pairs, low + 1)
    assert np.array_equal(above["flag"] == 2, got["n_used"] == low) and np.all(above["scale"][above["flag"] == 2] == 1.0)


@pytest.mark.gpu
def test_gpu_rescale_after_the_essential_run(ctx, six):
    _, _, _, seq = six
    s, pairs, _ = _open(ctx, seq, essential=True)
    try:
        got, _ = _rescale_and_compare(s, pairs)
        assert np.all(got["flag"] == 0) and got["n_used"].min() >= 50
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_rescale_twin_keypoint(ctx, six):
    """no keypoint of the six frames (nor of the 260) is shared twice, so frame 3 gets a copy of a keypoint whose point of pair
    2 sits on a keypoint pairs 1 and 2 share: that keypoint of frame 2 is then the base keypoint of two points of pair 2, and
    the smaller point is the one step 1 uses"""
    _, pairs0, _, seq0 = six
    s, pairs, _ = _open(ctx, twin_sequence(seq0, pairs0))
    try:
        twice = shared_twice(pairs, 300)
        print("%d keypoints shared twice" % twice)
        assert twice >= 1 and shared_twice(pairs[1:3], 300) >= 1
        got, _ = _rescale_and_compare(s, pairs)
        _, _, okn = rm.point_keypoints(pairs[2], 300)
        an = rm.point_keypoints(pairs[2], 300)[0][okn]
        bq = rm.point_keypoints(pairs[1], 300)[1]
        assert got["n_common"][1] == len(np.intersect1d(an, bq)) < int(np.isin(an, bq).sum())   # counted once
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_rescale_long_sequence_crosses_the_fold_chunks(ctx, long_seq):
    """260 frames: 259 poses are folded in chunks of 128, the running pose and sigma cross two chunk edges"""
    s, pairs, _ = long_seq
    got, traj = _rescale_and_compare(s, pairs)
    print("260 frames: n_used %d .. %d, sigma_last %.3e, %d keypoints shared twice"
          % (got["n_used"].min(), got["n_used"].max(), traj["pair_scale"][-1], shared_twice(pairs, LONG_ARGS["n_kp"])))
    assert np.all(got["flag"] == 0) and len(got) > 2 * 128


@pytest.mark.gpu
def test_gpu_rescale_wide_frames_cross_the_keypoint_chunks(ctx):
    """3 frames of 600 keypoints: the keypoint tables and the compaction cross 256 (and the tables 512)"""
    s, pairs, _ = _open(ctx, synth.make_sequence(3, **WIDE_ARGS))
    try:
        got, _ = _rescale_and_compare(s, pairs)
        j, jn = rm.shared_points(pairs[0], pairs[1], 600)
        c = rm.point_keypoints(pairs[1], 600)[0][jn]
        assert got["flag"][0] == 0 and (c >= 512).any() and (c < 256).any() and (jn >= 256).any() and (jn < 256).any()
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_rescale_with_a_blind_frame(ctx, six):
    """frame 3 cut to five keypoints (test_seq_odometry's device): pairs 2 and 3 are invalid, the three steps that touch them
    carry flag 1 and keep the scale, and the trajectory stands still across both pairs"""
    _, _, _, seq = six
    n_kp = seq["n_kp"].copy()
    n_kp[3] = 5
    s, pairs, _ = _open(ctx, seq, n_kp=n_kp)
    try:
        assert [p["valid"] for p in pairs] == [True, True, False, False, True]
        got, traj = _rescale_and_compare(s, pairs)
        assert got["flag"].tolist() == [0, 1, 1, 1] and got["scale"][1:].tolist() == [1.0, 1.0, 1.0]
        assert not np.any(got["n_common"][1:]) and not np.any(got["n_used"][1:])
        for k in (3, 4):
            assert traj["R"][k].tobytes() == traj["R"][2].tobytes() and traj["t"][k].tobytes() == traj["t"][2].tobytes()
        assert np.any(traj["t"][5] != traj["t"][4])
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_rescale_chain_restores_the_run_and_is_deterministic(ctx, six):
    from mvslam_amd import capi

    s, pairs, traj0, _ = six
    s.rescale(capi.SEQ_SCALE_DEPTH_RATIO, 1)
    a = s.download_scale_steps().tobytes() + _traj_bytes(s.download_trajectory())
    assert _traj_bytes(s.download_trajectory()) != _traj_bytes(traj0)
    s.rescale(capi.SEQ_SCALE_CHAIN, 1)
    assert _traj_bytes(s.download_trajectory()) == _traj_bytes(traj0)
    assert not np.any(s.download_scale_steps().view(np.uint8))               # the chain has no step records: zero
    s.rescale(capi.SEQ_SCALE_DEPTH_RATIO, 1)
    assert s.download_scale_steps().tobytes() + _traj_bytes(s.download_trajectory()) == a
    s.rescale(capi.SEQ_SCALE_CHAIN, 7)
    assert _traj_bytes(s.download_trajectory()) == _traj_bytes(traj0)


@pytest.mark.gpu
def test_gpu_rescale_argument_errors_touch_nothing(ctx, six):
    from mvslam_amd import capi

    s, _, _, seq = six
    s.rescale(capi.SEQ_SCALE_DEPTH_RATIO, 1)
    before = s.download_scale_steps().tobytes() + _traj_bytes(s.download_trajectory())
    I = capi.MVS_ERR_INVALID_ARG
    for rule, mc in ((2, 1), (-1, 1), (capi.SEQ_SCALE_DEPTH_RATIO, 0), (capi.SEQ_SCALE_DEPTH_RATIO, -3), (capi.SEQ_SCALE_CHAIN, 0)):
        assert _status_of(s.rescale, rule, mc) == I, (rule, mc)
    lib = capi.lib()
    sp = capi.SeqScaleParams(capi.SEQ_SCALE_DEPTH_RATIO, 1)
    assert lib.mvs_seq_rescale(s._h, None) == I and lib.mvs_seq_rescale(None, C.byref(sp)) == I
    assert lib.mvs_seq_download_scale_steps(s._h, None) == I
    assert s.download_scale_steps().tobytes() + _traj_bytes(s.download_trajectory()) == before
    fresh = capi.Sequence(ctx, 6, 300, 32)                                   # uploaded, never run
    try:
        fresh.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
        assert _status_of(fresh.rescale) == I and _status_of(fresh.download_scale_steps) == I
        fresh.run(*_params())
        assert _status_of(fresh.download_scale_steps) == I                   # run, not rescaled
        fresh.rescale()
        assert len(fresh.download_scale_steps()) == 4
        fresh.run(*_params())                                                # a new run retires the records
        assert _status_of(fresh.download_scale_steps) == I
    finally:
        fresh.close()


@pytest.mark.gpu
def test_gpu_rescale_retires_what_read_the_trajectory(ctx):
    """windows, the pose graph with its optimised nodes and the global problem refuse after a rescale as after a new run;
    pairs, tracks and lagged pairs keep their bytes, and the consumers build again on the new trajectory"""
    from mvslam_amd import capi

    def raw(d):
        return b"".join(np.ascontiguousarray(d[k]).tobytes() for k in sorted(d))

    s = spg._open(ctx, 8, max_lag=2)
    try:
        s.build_pose_graph(2)
        assert s.optimize_pose_graph()[0] == capi.MVS_OK
        s.download_pose_graph_poses()
        assert s.refine_global(3)["n_points"] >= 30
        s.download_global()
        s.refine_windows(4, 1)
        s.download_windows()
        kept = [raw(s.download_pairs()), raw(s.download_tracks()), raw(s.download_lag_pairs(1)), raw(s.download_lag_pairs(2))]
        s.rescale()
        I = capi.MVS_ERR_INVALID_ARG
        assert _status_of(s.download_pose_graph_poses) == I and _status_of(s.download_pose_graph) == I
        assert _status_of(s.optimize_pose_graph) == I
        assert _status_of(s.download_global) == I and _status_of(s.global_counts) == I
        assert _status_of(s.download_windows) == I
        assert kept == [raw(s.download_pairs()), raw(s.download_tracks()), raw(s.download_lag_pairs(1)), raw(s.download_lag_pairs(2))]
        traj = s.download_trajectory()
        s.build_pose_graph(2)                                                # the lags are still the run's
        node = s.download_pose_graph()["node_pose"]
        assert node[:, :9].tobytes() == traj["R"].tobytes() and node[:, 9:].tobytes() == traj["t"].tobytes()
        assert s.refine_global(3)["status"] in (capi.MVS_OK, capi.MVS_NO_MODEL)
        s.rescale(capi.SEQ_SCALE_CHAIN)                                      # the chain's rule retires them as well
        assert _status_of(s.download_pose_graph) == I and _status_of(s.global_counts) == I
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_rescale_lowers_the_global_problems_initial_error(ctx, long_seq):
    """260 frames at T = 8, test_seq_global's long case: mvs_seq_refine_global under the chain's trajectory and under the
    depth ratios'.  Both records are finite and the depth ratios start lower.  Measured: error_initial 1.532907e15 under the
    chain (11 failed solves, ok 0) and 3.368157e5 under the depth ratios (no failed solve, 11 rejected steps, ok 1); the
    figures of both runs are printed (DESIGN.md section 4.6.1 records them); ok is reported, not asserted."""
    from mvslam_amd import capi

    s, pairs, traj0 = long_seq
    params = capi.default_refine_params()
    s.rescale(capi.SEQ_SCALE_CHAIN)
    assert _traj_bytes(s.download_trajectory()) == _traj_bytes(traj0)
    chain = s.refine_global(LONG_T, params, 0.5)
    s.rescale(capi.SEQ_SCALE_DEPTH_RATIO, 1)
    ratio = s.refine_global(LONG_T, params, 0.5)
    for name, r in (("chain", chain), ("depth ratio", ratio)):
        print("%s: error_initial %.6e, error %.6e, iterations %d, rejected %d, failed_solves %d, ok %d, %d points, %d observations"
              % (name, r["error_initial"], r["error"], r["iterations"], r["rejected_steps"], r["failed_solves"], r["ok"],
                 r["n_points"], r["n_obs"]))
        assert np.isfinite(r["error_initial"]) and np.isfinite(r["error"])
    assert ratio["error_initial"] < chain["error_initial"]
    assert (ratio["n_points"], ratio["n_obs"]) == (chain["n_points"], chain["n_obs"])
