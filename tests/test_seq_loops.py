"""Loop closures of a resident sequence on the device (loop.hip, seq_graph.hip):
mvs_seq_loop_scores against tests/seq_loop_model.py and against mvs_match_hamming pair by pair, mvs_seq_select_loops against
the model, mvs_seq_verify_loops against an uploaded batch of the same frame pairs, mvs_seq_add_loop_edges against the model
and mvs_seq_optimize_pose_graph on the longer edge list against mvs_pose_graph_optimize on the downloaded graph.

Shapes.  Scores: 7 frames of up to 300 keypoints with the counts [300, 257, 256, 33, 1, 0, 290] (a partial 32-row train
tile, both sides of the 256-query block edge, a frame with fewer than two trains, an empty frame); 7 frames at min_gap 1 give
the last query frame two runs of base frames.  Loop sequence: synth.make_loop_sequence, 24 frames, 300 keypoints, 256
two-view hypotheses; it is scored, selected and run once per module and only read afterwards."""
import numpy as np
import pytest

import seq_graph_model as gm
import seq_loop_model as lm
import test_seq_odometry as so
import test_seq_track as st
import test_seq_windows as sw

# the (ratio, max_dist) settings of tests/test_gpu_parity.py
SETTINGS = ((0.7, -1.0), (0.7, 10.0), (0.95, 200.0), (0.7, 64.0), (0.9, 3.0), (0.7, 0.0))
COUNTS = np.array([300, 257, 256, 33, 1, 0, 290], dtype=np.int32)
N_KP = 300


def _flip(row, n_bits, rng):
    """`row` (uint8 descriptor) with exactly n_bits bits flipped"""
    bits = np.unpackbits(row, bitorder="little")
    bits[rng.choice(bits.size, size=n_bits, replace=False)] ^= 1
    return np.packbits(bits, bitorder="little")


def score_frames(desc_bytes=32, counts=COUNTS, max_kp=N_KP, seed=11):
    """frames whose keypoints are partly views of one pool: true partners at small distances, exact duplicates inside a
    frame (D1 = D0), and partners planted at exactly 0, 3, 4, 10, 11, 64 and 65 bits from a pool row"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, size=(max_kp, desc_bytes), dtype=np.uint8)
    desc = rng.integers(0, 256, size=(len(counts), max_kp, desc_bytes), dtype=np.uint8)
    planted = (0, 3, 4, 10, 11, 64, 65)
    for f, n in enumerate(counts):
        m = min(int(n), 200)
        for r in range(0, m, 2):                       # every second row is a view of pool row r
            d = planted[(r // 2) % len(planted)] if r < 60 else int(rng.integers(0, 9))
            desc[f, r] = _flip(pool[r], min(d, desc_bytes * 8 - 1), rng)
        if n >= 8:                                     # duplicates: rows 1 and 3 repeat rows 0 and 2
            desc[f, 1], desc[f, 3] = desc[f, 0], desc[f, 2]
    return desc


def _seq_with(ctx, desc, counts, max_kp, desc_bytes=32):
    from mvslam_amd import capi, synth

    s = capi.Sequence(ctx, len(counts), max_kp, desc_bytes)
    kp = np.zeros((len(counts), max_kp, 2), dtype=np.float32)
    s.upload(0, desc, kp, counts, synth.K_DEFAULT)
    return s


@pytest.fixture(scope="module")
def score_seq(ctx):
    desc = score_frames()
    s = _seq_with(ctx, desc, COUNTS, N_KP)
    yield s, desc
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1 scores

@pytest.mark.gpu
@pytest.mark.parametrize("ratio,max_dist", SETTINGS)
def test_gpu_scores_equal_the_model_and_the_matcher(ctx, score_seq, ratio, max_dist):
    s, desc = score_seq
    s.loop_scores(ratio, max_dist, 1)
    got = s.download_loop_scores()
    want = lm.scores(desc, COUNTS, ratio, max_dist, 1)
    print("ratio", ratio, "max_dist", max_dist, "scores\n", got)
    assert np.array_equal(got, want)
    assert not np.tril(got).any()
    for j in range(len(COUNTS)):
        for i in range(j):
            if COUNTS[i] >= 2 and COUNTS[j] >= 1:
                m = len(ctx.match_hamming(desc[i][:COUNTS[i]], desc[j][:COUNTS[j]], ratio, max_dist))
            else:
                m = 0     # mvs_match_hamming refuses these; the pipeline reports no match
            assert got[i, j] == m, (i, j, got[i, j], m)
    assert got[0, 1] > 0 and got[0, 6] > 0, "the planted partners give no matches: the fixture tests nothing"
    s.loop_scores(ratio, max_dist, 1)
    assert s.download_loop_scores().tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.gpu
def test_gpu_scores_min_gap_leaves_a_zero_band(score_seq):
    s, desc = score_seq
    s.loop_scores(0.7, 64.0, 3)
    got = s.download_loop_scores()
    assert np.array_equal(got, lm.scores(desc, COUNTS, 0.7, 64.0, 3))
    F = len(COUNTS)
    assert all(got[i, j] == 0 for i in range(F) for j in range(F) if j - i < 3) and got[0, 3] > 0 and got[0, 6] > 0


@pytest.mark.gpu
def test_gpu_scores_two_frames_of_4096_keypoints(ctx):
    counts = np.array([4096, 4096, 0], dtype=np.int32)
    rng = np.random.default_rng(5)
    desc = rng.integers(0, 256, size=(3, 4096, 32), dtype=np.uint8)
    for r in range(0, 4096, 3):
        desc[1, (r * 7) % 4096] = _flip(desc[0, r], int(rng.integers(0, 14)), rng)
    s = _seq_with(ctx, desc, counts, 4096)
    try:
        for ratio, max_dist in ((0.7, 10.0), (0.7, -1.0)):
            s.loop_scores(ratio, max_dist, 1)
            got = s.download_loop_scores()
            want = lm.scores(desc, counts, ratio, max_dist, 1)
            print(ratio, max_dist, "score", got[0, 1], "model", want[0, 1])
            assert np.array_equal(got, want) and got[0, 1] > 300
            assert got[0, 1] == len(ctx.match_hamming(desc[0], desc[1], ratio, max_dist))
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("desc_bytes", [16, 64])
def test_gpu_scores_other_descriptor_sizes(ctx, desc_bytes):
    counts = np.array([100, 70, 65, 3], dtype=np.int32)
    desc = score_frames(desc_bytes, counts, 100, seed=3)
    s = _seq_with(ctx, desc, counts, 100, desc_bytes)
    try:
        for ratio, max_dist in ((0.7, -1.0), (0.7, 10.0), (0.9, 3.0)):
            s.loop_scores(ratio, max_dist, 1)
            got = s.download_loop_scores()
            assert np.array_equal(got, lm.scores(desc, counts, ratio, max_dist, 1)), (ratio, max_dist)
            for j in range(4):
                for i in range(j):
                    assert got[i, j] == len(ctx.match_hamming(desc[i][:counts[i]], desc[j][:counts[j]], ratio, max_dist))
            assert got[0, 1] > 0
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2 selection

@pytest.mark.gpu
def test_gpu_selection_equals_the_model(ctx):
    """10 frames of 64 keypoints; frames 1 and 2 are the same image, so their scores tie in every column"""
    rng = np.random.default_rng(21)
    F, N = 10, 64
    pool = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    desc = rng.integers(0, 256, size=(F, N, 32), dtype=np.uint8)
    for f in range(F):
        shared = 12 + 4 * (f % 5)
        for r in range(shared):
            desc[f, r] = _flip(pool[r], int(rng.integers(0, 6)), rng)
    desc[2] = desc[1]
    counts = np.full(F, N, dtype=np.int32)
    s = _seq_with(ctx, desc, counts, N)
    try:
        s.loop_scores(0.7, 64.0, 1)
        table = s.download_loop_scores()
        assert np.array_equal(table, lm.scores(desc, counts, 0.7, 64.0, 1))
        assert all(table[1, j] == table[2, j] for j in range(3, F)) and table[1, 5] > 0, "no ties in the table"
        check_selection_equals_the_model(s, table, ((1, 3, 1000), (14, 2, 1000), (1, 3, 11), (20, 20, 5), (1000, 2, 4)))
        _, found = lm.select(table, 1, 3, 11)
        assert found > 11, "the cut case cuts nothing"
        rows = lm.select(table, 14, 2, 1000)[0]
        per_j = np.bincount([j for _, j, _ in rows], minlength=F)
        assert (per_j < 2).any() and (per_j == 2).any(), "no row with fewer than top_k eligible entries"
        assert any(c[0] == 1 for c in lm.select(table, 1, 3, 1000)[0]), "the tie is never selected"
    finally:
        s.close()


def check_selection_equals_the_model(s, table, settings):
    """mvs_seq_select_loops on the scored sequence `s` against the model on its downloaded table, for every
    (min_score, top_k, max_candidates) of `settings`; the rows behind the kept candidates are zero"""
    for min_score, top_k, cap in settings:
        s.select_loops(min_score, top_k, cap)
        got = s.download_loop_candidates()
        want, found = lm.select(table, min_score, top_k, cap)
        print((min_score, top_k, cap), "kept", got["n_kept"], "found", got["n_found"])
        assert got["n_found"] == found and got["n_kept"] == len(want)
        assert [(int(c["i"]), int(c["j"]), int(c["score"])) for c in got["cand"]] == want
        assert not got["cand"]["accepted"].any()
        assert got["cand_all"][got["n_kept"]:].tobytes() == bytes(16 * (cap - got["n_kept"]))


# ---------------------------------------------------------------------------------------------------------------------
# 3 verification, 4 edges: one loop sequence per module

# 0.5 m and 0.08 rad per frame: frames eight apart share few enough map points that a revisit outscores them.  With these
# values the 16 candidates are the revisits and their neighbours, and the CPU oracle's two-view + refine accepts every one of
# them (valid, refined ok, positive definite covariance; checked before the seed was fixed).
LOOP_FRAMES, LOOP_GAP, LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP = 24, 8, 200, 2, 16
LOOP_ARGS = dict(shift=0.1, seed=st.SEED, n_kp=300, n_map=1500, noise_px=0.3, step=0.5, yaw_step=0.08)
MATCH = dict(ratio=0.7, max_dist=64.0)


def _two_view(**kw):
    from mvslam_amd import capi

    return capi.default_params(num_hypotheses=256, sampler=capi.SAMPLER_PHILOX, seed=sw.PRM["seed"], max_error_sq=sw.PRM["thr"],
                               **MATCH, **kw)


@pytest.fixture(scope="module")
def loop_seq(ctx):
    from mvslam_amd import capi, synth

    data = synth.make_loop_sequence(LOOP_FRAMES, **LOOP_ARGS)
    s = capi.Sequence(ctx, LOOP_FRAMES, N_KP, 32)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    s.upload_octaves(0, st._octaves(LOOP_FRAMES))
    s.loop_scores(MATCH["ratio"], MATCH["max_dist"], LOOP_GAP)
    s.select_loops(LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP)
    s.run(_two_view(), so._pnp())
    s.run_lags(_two_view(), 2)
    yield s, data
    s.close()


@pytest.mark.gpu
def test_gpu_loop_sequence_selects_its_revisits(loop_seq):
    s, data = loop_seq
    got = s.download_loop_candidates()
    table = s.download_loop_scores()
    want, found = lm.select(table, LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP)
    assert [(int(c["i"]), int(c["j"]), int(c["score"])) for c in got["cand"]] == want and got["n_found"] == found
    hits = sum(1 for i, j, _ in want if abs(int(data["revisit"][j]) - i) <= 1)
    print("candidates", want, "revisit hits", hits)
    assert got["n_kept"] >= 4 and hits >= 4, "the selection does not find the revisits"


@pytest.mark.gpu
@pytest.mark.parametrize("essential", [False, True], ids=["eight_point", "five_point"])
def test_gpu_verification_equals_an_uploaded_batch(ctx, loop_seq, essential):
    s, data = loop_seq
    check_verification_equals_an_uploaded_batch(ctx, s, data, essential)


def check_verification_equals_an_uploaded_batch(ctx, s, data, essential, desc_bytes=32, n_kp=N_KP):
    """the verification of the selected candidates of `s` (which holds `data` and st._octaves at `n_kp` keypoints a frame)
    against a batch of the same (i, j) frames uploaded from the host: every byte of the pair results and of the refinement
    records"""
    from mvslam_amd import capi

    prm = _two_view()
    s.verify_loops(prm, essential=essential)
    got = s.download_loop_candidates(pairs=True)
    k = got["n_kept"]
    ci, cj = got["cand"]["i"], got["cand"]["j"]
    b = capi.Batch(ctx, k, n_kp, desc_bytes)
    try:
        oct_ = st._octaves(s.n_frames, n_kp)
        b.upload(0, data["desc"][ci], data["kp"][ci], data["n_kp"][ci], data["desc"][cj], data["kp"][cj], data["n_kp"][cj],
                 np.tile(data["K"].reshape(1, 9), (k, 1)), np.arange(k, dtype=np.int64))
        b.upload_octaves(0, oct_[ci], oct_[cj])
        (b.run_essential if essential else b.run)(prm)
        b.refine(sigma_px=0.5)
        b.sync()
        want = b.download()
        wref = b.download_refined(points=False)
    finally:
        b.close()
    print("valid", got["results"]["valid"].tolist(), "refined ok", got["refined"]["ok"].tolist())
    for key in ("results", "matches", "mask", "points", "point_idx"):
        assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(want[key]).tobytes(), key
    assert got["refined"].tobytes() == wref["refined"].tobytes()
    assert got["results"]["valid"].sum() >= 2 and got["refined"]["ok"].sum() >= 2
    assert np.array_equal(got["results"]["n_matches"], got["cand"]["score"]), "score != n_matches of the pair pipeline"


def _built(s, n_frames=LOOP_FRAMES):
    s.build_pose_graph(2)
    g = s.download_pose_graph()
    assert g["n_edges"] > n_frames - 1 and not (g["edge_kind"] == 2).any()
    return g


@pytest.mark.gpu
def test_gpu_loop_edges_equal_the_model_and_optimise(ctx, loop_seq):
    s, _ = loop_seq
    check_loop_edges_equal_the_model_and_optimise(ctx, s)


def check_loop_edges_equal_the_model_and_optimise(ctx, s, n_frames=LOOP_FRAMES):
    """`s`: a sequence of n_frames frames that is scored, selected, run and holds lags up to 2"""
    from mvslam_amd import capi

    s.verify_loops(_two_view())
    cd = s.download_loop_candidates(pairs=True)
    cand = [(int(c["i"]), int(c["j"]), int(c["score"])) for c in cd["cand"]]
    recs = lm.records(cd["results"], cd["refined"])
    traj = s.download_trajectory()
    built = _built(s, n_frames)
    last = None
    for kw in (dict(), dict(loop_sigma=(0.02, 0.2)), dict(loop_sigma=(0.0, 0.3), min_points=30), dict(loop_sigma=(0.02, 0.2))):
        s.add_loop_edges(**kw)      # every call after the first replaces the edges of the call before
        got = s.download_pose_graph()
        want, acc = lm.add_loop_edges(built, traj["R"], traj["t"], cand, recs, **kw)
        n_loop = int((got["edge_kind"] == 2).sum())
        print(kw, "edges", got["n_edges"], "loop edges", n_loop, "scales", got["edge_scale"][got["edge_kind"] == 2])
        assert gm.same_bytes(got, want) == []
        assert n_loop == acc.sum() and n_loop >= 1, "no loop edge was accepted: the test shows nothing"
        assert np.array_equal(s.download_loop_candidates()["cand"]["accepted"], acc)
        loops = got["edge_kind"] == 2
        assert np.array_equal(got["edge_lag"][loops], got["edge_dst"][loops] - got["edge_src"][loops])
        assert (got["edge_lag"][loops] >= LOOP_GAP).all() and not loops[:built["n_edges"]].any()
        last = got
    # the optimiser on the longer list: the resident call against the host call on the downloaded graph
    status, res = s.optimize_pose_graph()
    poses = s.download_pose_graph_poses()
    st2, res2, poses2 = ctx.pose_graph_optimize(last)
    assert status == st2 == capi.MVS_OK and res["ok"] == 1 and res["error"] <= res["error_initial"]
    assert res.tobytes() == res2.tobytes() and poses.tobytes() == poses2.tobytes()
    # adding edges again clears the optimised state
    s.add_loop_edges()
    with pytest.raises(capi.MvsError) as e:
        s.download_pose_graph_poses()
    assert e.value.status == capi.MVS_ERR_INVALID_ARG


@pytest.mark.gpu
def test_gpu_loop_edges_after_a_larger_selection(loop_seq):
    """build, select few, verify, add; then a selection with a larger top_k and max_candidates (the selection's block and the
    verification batch are replaced, the graph's block grows), verify, add: the second call's edges replace the first's behind
    the same built edges.  A smaller selection afterwards changes neither the graph nor its download."""
    s, _ = loop_seq
    traj = s.download_trajectory()
    try:
        s.select_loops(LOOP_MIN_SCORE, 1, 5)
        built = _built(s)
        graphs = []
        for top_k, cap in ((1, 5), (3, 40)):
            s.select_loops(LOOP_MIN_SCORE, top_k, cap)
            s.verify_loops(_two_view())
            s.add_loop_edges(loop_sigma=(0.02, 0.2))
            cd = s.download_loop_candidates(pairs=True)
            cand = [(int(c["i"]), int(c["j"]), int(c["score"])) for c in cd["cand"]]
            got = s.download_pose_graph()
            want, acc = lm.add_loop_edges(built, traj["R"], traj["t"], cand, lm.records(cd["results"], cd["refined"]),
                                          loop_sigma=(0.02, 0.2))
            print("top_k", top_k, "cap", cap, "kept", cd["n_kept"], "edges", got["n_edges"], "loop edges", int(acc.sum()))
            assert gm.same_bytes(got, want) == [] and acc.sum() >= 1
            assert np.array_equal(cd["cand"]["accepted"], acc)
            graphs.append(got)
        assert graphs[1]["n_edges"] > graphs[0]["n_edges"] > built["n_edges"], "the second list is no longer than the first"
        s.select_loops(LOOP_MIN_SCORE, 1, 2)
        assert gm.same_bytes(s.download_pose_graph(), graphs[1]) == []
    finally:
        s.select_loops(LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP)    # the module's list again


@pytest.mark.gpu
def test_gpu_loop_state_is_dropped_by_an_upload(ctx):
    from mvslam_amd import capi, synth

    desc = score_frames(counts=COUNTS[:4])
    s = _seq_with(ctx, desc, COUNTS[:4], N_KP)
    try:
        s.loop_scores(0.7, 10.0, 1)
        s.select_loops(1, 1, 4)
        s.verify_loops(_two_view())
        s.download_loop_candidates(pairs=True)
        s.upload_octaves(0, np.zeros((4, N_KP), dtype=np.uint8))       # the verification weighed other octaves
        _raises(capi.MVS_ERR_INVALID_ARG, s.download_loop_candidates, pairs=True)
        s.download_loop_candidates()
        s.upload(1, desc[:1], np.zeros((1, N_KP, 2), dtype=np.float32), COUNTS[:1], synth.K_DEFAULT)   # another frame 1
        _raises(capi.MVS_ERR_INVALID_ARG, s.download_loop_scores)
        _raises(capi.MVS_ERR_INVALID_ARG, s.download_loop_candidates)
        _raises(capi.MVS_ERR_INVALID_ARG, s.select_loops, 1, 1, 4)
        s.loop_scores(0.7, 10.0, 1)
        assert np.array_equal(s.download_loop_scores(), lm.scores(np.concatenate([desc[:1], desc[:1], desc[2:]]),
                                                                  np.array([300, 300, 256, 33]), 0.7, 10.0, 1))
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_loop_edges_over_capacity_changes_nothing(loop_seq):
    from mvslam_amd import capi

    s, _ = loop_seq
    s.verify_loops(_two_view())
    _built(s)
    s.add_loop_edges(loop_sigma=(0.02, 0.2))
    before = s.download_pose_graph()
    try:
        s.select_loops(LOOP_MIN_SCORE, LOOP_TOP_K, capi.POSE_GRAPH_MAX_EDGES)     # slots + candidates > 65536
        with pytest.raises(capi.MvsError) as e:
            s.add_loop_edges(loop_sigma=(0.02, 0.2))
        assert e.value.status == capi.MVS_ERR_CAPACITY
        assert gm.same_bytes(s.download_pose_graph(), before) == []
    finally:
        s.select_loops(LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP)    # the module's list again


# ---------------------------------------------------------------------------------------------------------------------
# 5 argument errors, one test per error the header lists

def _raises(status, fn, *a, **kw):
    from mvslam_amd import capi

    with pytest.raises(capi.MvsError) as e:
        fn(*a, **kw)
    assert e.value.status == status


@pytest.fixture()
def fresh(ctx):
    s = _seq_with(ctx, score_frames(counts=COUNTS[:4]), COUNTS[:4], N_KP)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(0.7, 10.0, 0), (0.7, 10.0, 4), (float("nan"), 10.0, 1), (0.7, float("nan"), 1)])
def test_gpu_scores_argument_errors(fresh, args):
    from mvslam_amd import capi

    _raises(capi.MVS_ERR_INVALID_ARG, fresh.loop_scores, *args)


@pytest.mark.gpu
def test_gpu_scores_download_before_scores(fresh):
    from mvslam_amd import capi

    _raises(capi.MVS_ERR_INVALID_ARG, fresh.download_loop_scores)


@pytest.mark.gpu
def test_gpu_scores_capacity(ctx):
    from mvslam_amd import capi

    s = capi.Sequence(ctx, capi.LOOP_MAX_FRAMES + 1, 4, 32)
    try:
        _raises(capi.MVS_ERR_CAPACITY, s.loop_scores, 0.7, 10.0, 1)
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_select_before_scores(fresh):
    from mvslam_amd import capi

    _raises(capi.MVS_ERR_INVALID_ARG, fresh.select_loops, 1, 1, 1)
    _raises(capi.MVS_ERR_INVALID_ARG, fresh.download_loop_candidates)


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(0, 1, 1), (1, 0, 1), (1, 1, 0)])
def test_gpu_select_argument_errors(fresh, args):
    from mvslam_amd import capi

    fresh.loop_scores(0.7, 10.0, 1)
    _raises(capi.MVS_ERR_INVALID_ARG, fresh.select_loops, *args)


@pytest.mark.gpu
def test_gpu_verify_argument_errors(fresh):
    from mvslam_amd import capi

    _raises(capi.MVS_ERR_INVALID_ARG, fresh.verify_loops, _two_view())            # before the selection
    fresh.loop_scores(0.7, 10.0, 1)
    fresh.select_loops(1, 1, 4)
    _raises(capi.MVS_ERR_INVALID_ARG, fresh.download_loop_candidates, pairs=True)  # pair results before the verification
    _raises(capi.MVS_ERR_INVALID_ARG, fresh.verify_loops, _two_view(), sigma_px=0.0)
    _raises(capi.MVS_ERR_INVALID_ARG, fresh.verify_loops, capi.default_params(num_hypotheses=0))
    _raises(capi.MVS_ERR_INVALID_ARG, fresh.verify_loops, _two_view(), refine_params=capi.default_refine_params(lambda_factor=1.0))


@pytest.mark.gpu
def test_gpu_add_edges_without_a_graph(fresh):
    from mvslam_amd import capi

    fresh.loop_scores(0.7, 10.0, 1)
    fresh.select_loops(1, 1, 4)
    fresh.verify_loops(_two_view())                                                # verified candidates, but no graph
    _raises(capi.MVS_ERR_INVALID_ARG, fresh.add_loop_edges)


@pytest.mark.gpu
def test_gpu_add_edges_without_a_verification(loop_seq):
    from mvslam_amd import capi

    s, _ = loop_seq
    _built(s)
    s.select_loops(LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP)                           # a graph, but a list that is not verified
    _raises(capi.MVS_ERR_INVALID_ARG, s.add_loop_edges)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(min_points=-1), dict(max_error=-1.0), dict(max_error=float("nan")),
                                dict(loop_sigma=(float("nan"), 0.0)), dict(loop_sigma=(0.0, float("nan")))],
                         ids=["min_points", "max_error_negative", "max_error_nan", "sigma_rot_nan", "sigma_trans_nan"])
def test_gpu_add_edges_argument_errors(loop_seq, kw):
    from mvslam_amd import capi

    s, _ = loop_seq
    s.verify_loops(_two_view())
    _built(s)
    _raises(capi.MVS_ERR_INVALID_ARG, s.add_loop_edges, **kw)
    s.add_loop_edges()                                                             # the same state accepts valid arguments
