"""The full-size sequences of tests/seq_fullsize.py reach the paths that small frames never reach: shown on the CPU oracle's
pairs and the numpy models alone.  These are conditions, not measurements: nothing under test
decides them, and tests/test_seq_fullsize.py is about these paths only because they hold.

FULL (4 frames of 4096 keypoints): a depth-ratio step with more than 512 and more than 1024 used ratios (the bitonic sort's
second and further trips, n2 >= 2048), shared points of pair q with point index >= 2048 and >= 3072 (the int16 table of
point indices), a shared keypoint >= 3840, pair q + 1's shared points in 8 or more chunks of 256.  WORK (5 frames of 2000
keypoints): every pair's point list ends in a partial chunk of 256 that holds a shared point.  Both: a window of more than
1024 points, a frame row of the global plan with more than 1024 observations, a track seen in every frame, every edge of
lags 1 and 2 in the pose graph.  The loop sequence: a revisit under min_gap at the smallest frame count that has one.

Measured with the committed generator arguments (printed by the tests):
  FULL  points per pair 3177 / 3214 / 3168; n_used 3117, 3111; largest j 3213, largest c 4095; 13 chunks; window of 4 frames
        3331 points; plan rows 3207 / 3274 / 3271 / 3222 observations; 3098 tracks seen in all 4 frames
  WORK  points per pair 901 / 897 / 856 / 836 (partial chunks of 133 / 129 / 88 / 68); n_used 626, 604, 553; windows of 4
        frames 1421 and 1429 points; plan rows 922 .. 1174; 279 tracks seen in all 5 frames
"""
import numpy as np
import pytest

import seq_fullsize as fs
import seq_global_model as ggm
import seq_graph_model as gm
import seq_loop_model as lm
import seq_rescale_model as rm
import test_seq_loops as tl
import test_seq_windows as sw
import test_sequence as ts


@pytest.fixture(scope="module")
def host():
    """per sequence: the oracle's pairs and tracks, computed once"""
    out = {}
    for name in fs.SEQS:
        seq = fs.make(name)
        pairs, tracks = ts.oracle_sequence(seq, sw.PRM, sw.PPRM, threads=16)
        out[name] = dict(seq=seq, pairs=[dict(p, valid=p["ok"]) for p in pairs], tracks=tracks)
    return out


def _eye(F):
    return dict(R=np.tile(np.eye(3), (F, 1, 1)), t=np.zeros((F, 3)), pair_scale=np.ones(F - 1))


def _shared(pairs, N):
    """per step q: (j, j', c) of the shared points: point of pair q, point of pair q + 1, keypoint of frame q + 1"""
    out = []
    for q in range(len(pairs) - 1):
        j, jn = rm.shared_points(pairs[q], pairs[q + 1], N)
        out.append((j, jn, rm.point_keypoints(pairs[q + 1], N)[0][jn]))
    return out


def test_full_reaches_the_sort_trips_the_wide_indices_and_many_chunks(host):
    h = host["FULL"]
    N, pairs = h["seq"]["kp"].shape[1], h["pairs"]
    assert h["seq"]["kp"].shape[:2] == (fs.FULL_FRAMES, 4096) and all(p["valid"] for p in pairs)
    steps = rm.scale_steps(pairs, N, 1)
    sh = _shared(pairs, N)
    chunks = [len(np.unique(jn // 256)) for _, jn, _ in sh]
    print("FULL: points per pair %s, n_common %s, n_used %d .. %d, largest j %d, largest c %d, chunks of pair q + 1 %s"
          % ([len(p["point_idx"]) for p in pairs], steps["n_common"].tolist(), steps["n_used"].min(), steps["n_used"].max(),
             max(j.max() for j, _, _ in sh), max(c.max() for _, _, c in sh), chunks))
    assert np.all(steps["flag"] == 0)
    assert (steps["n_used"] > 512).any() and (steps["n_used"] > 1024).any()
    assert any((j >= 2048).any() for j, _, _ in sh) and any((j >= 3072).any() for j, _, _ in sh)
    assert any((c >= 3840).any() for _, _, c in sh)
    assert max(chunks) >= 8


def test_work_ends_every_point_list_in_a_partial_chunk_that_is_shared(host):
    h = host["WORK"]
    N, pairs = h["seq"]["kp"].shape[1], h["pairs"]
    assert h["seq"]["kp"].shape[:2] == (fs.WORK_FRAMES, 2000) and N % 256 != 0 and all(p["valid"] for p in pairs)
    steps = rm.scale_steps(pairs, N, 1)
    n_pts = [len(p["point_idx"]) for p in pairs]
    sh = _shared(pairs, N)
    in_last = [int((jn // 256 == (n_pts[q + 1] - 1) // 256).sum()) for q, (_, jn, _) in enumerate(sh)]
    print("WORK: points per pair %s (partial chunks %s), n_used %d .. %d, shared points in pair q + 1's last chunk %s"
          % (n_pts, [n % 256 for n in n_pts], steps["n_used"].min(), steps["n_used"].max(), in_last))
    assert np.all(steps["flag"] == 0)
    assert all(n % 256 != 0 for n in n_pts)
    assert all(k >= 1 for k in in_last)


@pytest.mark.parametrize("name", ["FULL", "WORK"])
def test_windows_and_the_global_plan_exceed_1024(host, name):
    h = host[name]
    F, N = h["seq"]["kp"].shape[:2]
    pairs = h["pairs"]
    sizes = {}
    for Fw, stride in ((4, 1), (3, 2)):
        wins = sw.build_windows(pairs, _eye(F), h["seq"]["kp"], None, Fw, stride, 4096)
        sizes[(Fw, stride)] = [w["n_points"] for w in wins]
        assert all(w["n_points"] == w["n_tracks_found"] for w in wins)       # nothing is cut at max_points = 4096
    g = ggm.build_global(pairs, _eye(F), N, 0)
    plan = ggm.plan_gap_free(F, g["obs_off"], g["obs_frame"], g["head_frame"])
    rows = np.diff(plan["fr_off"])
    whole = int((np.diff(g["obs_off"]) == F).sum())
    print("%s: windows (F, stride) -> points %s; global: %d points, %d observations, plan rows %s, %d tracks in all %d frames"
          % (name, sizes, len(g["head_frame"]), len(g["obs_frame"]), rows.tolist(), whole, F))
    assert max(sizes[(4, 1)]) > 1024
    assert rows.max() > 1024 and whole >= 1 and g["longest_chain"] == F


@pytest.mark.parametrize("name", ["FULL", "WORK"])
def test_the_pose_graph_holds_every_edge_of_lags_1_and_2(host, name):
    h = host[name]
    seq, pairs = h["seq"], h["pairs"]
    F = seq["kp"].shape[0]
    tables = fs.oracle_tables(seq, {1: pairs, 2: fs.oracle_lagged(seq, 2)})
    traj = fs.oracle_trajectory(pairs, h["tracks"])
    g = gm.build(traj["R"], traj["t"], tables, fs.MAX_LAG)
    print("%s: %d of %d slots hold an edge; points per pair %s" % (name, g["n_edges"], gm.n_slots(F, fs.MAX_LAG),
                                                                 [e["n_points"] for d in tables for e in tables[d]]))
    assert g["slots"] == [(d, k) for d in (1, 2) for k in range(F - d)] and not g["edge_kind"].any()


def test_loop_sequence_has_a_revisit_under_min_gap_at_the_smallest_frame_count():
    from mvslam_amd import synth

    gap = tl.LOOP_GAP
    few = synth.make_loop_sequence(fs.LOOP_FRAMES - 1, **dict(fs.LOOP_ARGS, n_kp=8, n_map=64))["revisit"]
    assert not any(g >= 0 and f - g >= gap for f, g in enumerate(few)), "a shorter sequence has a revisit under min_gap"
    data = fs.make_loop()
    rv = data["revisit"]
    far = [(int(g), f) for f, g in enumerate(rv) if g >= 0 and f - g >= gap]
    assert far == [(0, fs.LOOP_FRAMES - 1)] and data["kp"].shape[1] == 2000
    table = lm.scores(data["desc"], data["n_kp"], tl.MATCH["ratio"], tl.MATCH["max_dist"], gap)
    want, found = lm.select(table, tl.LOOP_MIN_SCORE, tl.LOOP_TOP_K, tl.LOOP_CAP)
    print("loop sequence: candidates %s" % want)
    assert (0, fs.LOOP_FRAMES - 1) in [(i, j) for i, j, _ in want] and found == len(want) >= 2
    assert all(abs(int(rv[j]) - i) <= 1 for i, j, _ in want)                  # the revisit and its neighbours
