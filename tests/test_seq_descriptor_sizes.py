"""Resident sequences with 128- and 512-bit descriptors: every other Sequence of the suite holds 256-bit ones.

A sequence keeps its frames in one allocation (the pair frame of pair k is the base frame of pair k + 1, desc2 = desc1 +
max_kp * desc_words) and offsets frames, lag batches and the loop batch's gather by max_kp * desc_words; a stride written for
8 words would pass everywhere else.  Here the consecutive-pair run (8-point and five-point), the lag batches, the loop
verification through its gather and the refusal of mvs_seq_upload_images run at 4 and 16 words, against an uploaded batch of
the same frames (every byte), the oracle (match lists, models, the join and the PnP) and mvs_match_hamming frame by frame.
Last, the point-fed single-shot calls, which inherit the descriptor size the context's scratch batch happens to have, are
shown not to depend on it.

Shapes.  Pairs: synth.make_sequence, 6 frames of up to 300 keypoints with the counts [300, 257, 290, 263, 300, 199] (none a
multiple of 32 or 64; the rows beyond are zeroed), 256 two-view hypotheses, Philox sampler, test_seq_loops' matcher setting
(ratio 0.7, max_dist 64: at 512 bits and the generator's 2 % bit flips a partner is about 20 bits away, so the suite's other
setting, max_dist 10, leaves no matches, while this one gives at least 150 per pair at both sizes with flip_p unchanged).
Loops: synth.make_loop_sequence with test_seq_loops' arguments, 12 frames with ragged counts, min_gap 4, min_score 180,
top_k 2: the model selects the eight revisits and neighbours.  The tests without the gpu mark show both on the CPU."""
import functools

import numpy as np
import pytest

import helpers
import oracle_lib as o
import seq_loop_model as lm
import test_seq_loops as sl
import test_seq_odometry as so
import test_seq_track as st
import test_sequence as ts
from mvslam_amd import synth

SIZES = (16, 64)
N_KP = sl.N_KP
COUNTS = np.array([300, 257, 290, 263, 300, 199], dtype=np.int32)
LOOP_COUNTS = np.array([300, 297, 290, 263, 300, 281, 299, 257, 300, 295, 271, 289], dtype=np.int32)
LOOP_GAP, LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP = 4, 180, 2, 16
PRM = dict(H=256, seed=so.PRM["seed"], thr=so.PRM["thr"])      # what test_seq_loops._two_view() asks for
PPRM = dict(H=100, seed=99, err=2.0)
MATCH = sl.MATCH


def _ragged(data, counts):
    data["n_kp"] = counts.copy()
    for f, n in enumerate(counts):
        data["desc"][f, n:] = 0
        data["kp"][f, n:] = 0
    return data


@functools.lru_cache(maxsize=None)
def pair_data(db):
    return _ragged(synth.make_sequence(len(COUNTS), n_kp=N_KP, desc_bytes=db), COUNTS)


@functools.lru_cache(maxsize=None)
def loop_data(db):
    return _ragged(synth.make_loop_sequence(len(LOOP_COUNTS), **dict(sl.LOOP_ARGS, desc_bytes=db)), LOOP_COUNTS)


@functools.lru_cache(maxsize=None)
def oracle_run(db):
    """the oracle's pairs and tracks of pair_data(db)"""
    return ts.oracle_sequence(pair_data(db), PRM, PPRM, threads=4, **MATCH)


def _pnp():
    from mvslam_amd import capi

    return capi.default_pnp_params(num_hypotheses=PPRM["H"], seed=PPRM["seed"], reproj_error=PPRM["err"])


# ---------------------------------------------------------------------------------------------------------------------
# the fixtures, on the CPU

@pytest.mark.parametrize("db", SIZES)
def test_pair_fixture_is_valid(db):
    data = pair_data(db)
    assert data["desc"].shape == (len(COUNTS), N_KP, db) and not any(n % 32 == 0 for n in COUNTS)
    pairs, tracks = oracle_run(db)
    print([(p["ok"], p["n_matches"], p["n_points"]) for p in pairs], [(t["ok"], len(t["X"])) for t in tracks])
    assert all(p["ok"] and p["valid"] and p["n_matches"] >= 100 for p in pairs)
    assert all(t["ok"] for t in tracks)


@pytest.mark.parametrize("db", SIZES)
def test_loop_fixture_selects_its_revisits(db):
    data = loop_data(db)
    table = lm.scores(data["desc"], LOOP_COUNTS, MATCH["ratio"], MATCH["max_dist"], LOOP_GAP)
    want, found = lm.select(table, LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP)
    hits = sum(1 for i, j, _ in want if abs(int(data["revisit"][j]) - i) <= 1)
    print(want)
    assert found == len(want) >= 3 and hits >= 3
    assert any(LOOP_COUNTS[i] % 32 and LOOP_COUNTS[j] % 32 and LOOP_COUNTS[i] < N_KP and LOOP_COUNTS[j] < N_KP for i, j, _ in want)


# ---------------------------------------------------------------------------------------------------------------------
# the device

def _open(ctx, db):
    from mvslam_amd import capi

    data = pair_data(db)
    s = capi.Sequence(ctx, len(COUNTS), N_KP, db)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    s.upload_octaves(0, st._octaves(len(COUNTS)))
    return s, data, db


@pytest.fixture(scope="module", params=SIZES)
def seq(ctx, request):
    """(Sequence, data, descriptor bytes): uploaded once; every test runs it itself"""
    opened = _open(ctx, request.param)
    yield opened
    opened[0].close()


def _run(s, essential=False):
    (s.run_essential if essential else s.run)(sl._two_view(), _pnp())
    return s.download_pairs(), s.download_tracks()


def _bytes(*downloads):
    return b"".join(np.ascontiguousarray(d[k]).tobytes() for d in downloads for k in sorted(d))


def _as_oracle_pairs(gp):
    """download_pairs() as the records oracle_sequence joins"""
    out = []
    for k, r in enumerate(gp["results"]):
        M, n = int(r["n_matches"]), int(r["n_points"]) if r["valid"] else 0
        out.append(dict(ok=bool(r["valid"]), matches=gp["matches"][k][:M], point_idx=gp["point_idx"][k][:n],
                        points=gp["points"][k][:n]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("essential", [False, True], ids=["eight_point", "five_point"])
def test_gpu_run_equals_an_uploaded_batch_and_the_oracle(ctx, seq, essential):
    from mvslam_amd import capi

    s, data, db = seq
    gp, gt = _run(s, essential)
    P = len(COUNTS) - 1
    b = capi.Batch(ctx, P, N_KP, db)
    try:
        b.upload(0, data["desc"][:P], data["kp"][:P], data["n_kp"][:P], data["desc"][1:], data["kp"][1:], data["n_kp"][1:],
                 data["K"], np.arange(P))
        (b.run_essential if essential else b.run)(sl._two_view())
        b.sync()
        want = b.download()
    finally:
        b.close()
    print("valid", gp["results"]["valid"].tolist(), "matches", gp["results"]["n_matches"].tolist(), "tracks",
          gt["tracks"]["ok"].tolist())
    for key in ("results", "matches", "mask", "points", "point_idx"):
        assert gp[key].tobytes() == want[key].tobytes(), key
    assert np.all(gp["results"]["valid"] == 1) and np.all(gp["results"]["n_matches"] >= 100)
    if essential:      # the oracle has no five-point path: its join and its PnP on the device's own pairs
        _, tracks = ts.oracle_sequence(data, PRM, PPRM, pairs=_as_oracle_pairs(gp), **MATCH)
        for k in range(P):
            m = o.match_visual_features(data["desc"][k][:COUNTS[k]], data["desc"][k + 1][:COUNTS[k + 1]], **MATCH)
            assert gp["matches"][k][:len(m)].tobytes() == m.tobytes() and gp["results"]["n_matches"][k] == len(m)
    else:
        pairs, tracks = oracle_run(db)
        ts.check_pairs_against_oracle(gp, pairs)
        for k, ref in enumerate(pairs):
            r = gp["results"][k]
            assert r["n_points"] == ref["n_points"] and r["best_hyp"] == ref["best_hyp"] and r["best_count"] == ref["best_count"]
    assert ts.check_tracks_against_oracle(gt, tracks) >= len(COUNTS) - 3


@pytest.mark.gpu
@pytest.mark.parametrize("essential", [False, True], ids=["eight_point", "five_point"])
@pytest.mark.parametrize("db", SIZES)
def test_gpu_lags_equal_an_uploaded_batch(ctx, db, essential):
    """a sequence of its own, as in test_seq_odometry: the comparison is of every byte, and the refined rows past a pair's
    n_points, which the header leaves open, are zero only where nothing was refined before"""
    s, data, _ = _open(ctx, db)
    try:
        _run(s, essential)
        s.run_lags(sl._two_view(), 3, essential=essential)
        raw = {d: (s.download_lag_pairs(d), s.download_lag_refined(d, point_cov=True)) for d in (1, 2, 3)}
        one = s.download_pairs()
        for key in ("results", "matches", "mask", "points", "point_idx"):
            assert raw[1][0][key].tobytes() == one[key].tobytes(), key
        assert all(raw[d][0]["results"]["valid"].any() and len(raw[d][0]["results"]) == len(COUNTS) - d for d in raw)
        so.check_lags_equal_a_batch(ctx, raw, one, data, st._octaves(len(COUNTS)), sl._two_view(), essential, desc_bytes=db)
    finally:
        s.close()


@pytest.fixture(scope="module", params=SIZES)
def loop_seq(ctx, request):
    from mvslam_amd import capi

    db = request.param
    data = loop_data(db)
    s = capi.Sequence(ctx, len(LOOP_COUNTS), N_KP, db)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    s.upload_octaves(0, st._octaves(len(LOOP_COUNTS)))
    s.loop_scores(MATCH["ratio"], MATCH["max_dist"], LOOP_GAP)
    s.select_loops(LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP)
    yield s, data, db
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("essential", [False, True], ids=["eight_point", "five_point"])
def test_gpu_loops_are_selected_and_verified_through_the_gather(ctx, loop_seq, essential):
    s, data, db = loop_seq
    table = s.download_loop_scores()
    assert np.array_equal(table, lm.scores(data["desc"], LOOP_COUNTS, MATCH["ratio"], MATCH["max_dist"], LOOP_GAP))
    got = s.download_loop_candidates()
    want, found = lm.select(table, LOOP_MIN_SCORE, LOOP_TOP_K, LOOP_CAP)
    print("candidates", want)
    assert [(int(c["i"]), int(c["j"]), int(c["score"])) for c in got["cand"]] == want and got["n_found"] == found
    assert got["n_kept"] >= 3
    sl.check_verification_equals_an_uploaded_batch(ctx, s, data, essential, desc_bytes=db)


@pytest.mark.gpu
def test_gpu_frames_match_their_own_neighbour_only(ctx, seq):
    """no call downloads a resident frame, so: two runs give the same bytes, and pair f's match list is what
    mvs_match_hamming and the oracle give for frames f and f + 1 fed on their own.  A wrong frame stride would match a frame
    against rows of another."""
    s, data, db = seq
    first = _bytes(*_run(s))
    gp, gt = _run(s)
    assert _bytes(gp, gt) == first
    for f in range(len(COUNTS) - 1):
        a, b = data["desc"][f][:COUNTS[f]], data["desc"][f + 1][:COUNTS[f + 1]]
        m = ctx.match_hamming(a, b, **MATCH)
        assert m.tobytes() == o.match_visual_features(a, b, **MATCH).tobytes()
        assert gp["results"]["n_matches"][f] == len(m) >= 100 and gp["matches"][f][:len(m)].tobytes() == m.tobytes(), f
        assert m["trainIdx"].max() < COUNTS[f] and m["queryIdx"].max() < COUNTS[f + 1]


@pytest.mark.gpu
def test_gpu_upload_images_is_refused_and_changes_nothing(seq):
    from mvslam_amd import capi

    s, data, db = seq
    before = _bytes(*_run(s))
    images = np.random.default_rng(db).integers(0, 256, size=(2, 96, 128), dtype=np.uint8)
    for first in (0, len(COUNTS) - 2):
        with pytest.raises(capi.MvsError) as e:
            s.upload_images(first, images, data["K"], capi.default_orb_params(nfeatures=N_KP, nlevels=2))
        assert e.value.status == capi.MVS_ERR_INVALID_ARG
    assert _bytes(*_run(s)) == before


# ---------------------------------------------------------------------------------------------------------------------
# the scratch batch's history

@pytest.mark.gpu
def test_gpu_point_calls_do_not_depend_on_the_scratch_batch(ctx):
    """mvs_match_hamming and mvs_image_pair re-create the context's scratch batch at their descriptor size; mvs_two_view*,
    mvs_triangulate and mvs_recover_pose take whatever size it has.  One fresh context: the four point-fed calls first (a
    32-byte scratch batch is made), after a 16-byte match, after a 64-byte image pair and after a 32-byte match again."""
    from mvslam_amd import capi

    pair, K = synth.make_pair(5, n_kp=150, noise_px=0.3), synth.K_DEFAULT
    m = o.match_visual_features(pair["desc1"], pair["desc2"], 0.7, 64.0)
    assert len(m) >= 60
    uv1, uv2 = pair["kp1"][m["trainIdx"]].astype(np.float64), pair["kp2"][m["queryIdx"]].astype(np.float64)
    prm = capi.default_params(num_hypotheses=128, sampler=capi.SAMPLER_PHILOX, seed=31, max_error_sq=1e-2)
    rig = helpers.two_camera_rig("cube")
    c = capi.Context(0)
    try:
        def point_calls():
            a = c.two_view(uv1, uv2, K, prm)
            e = c.two_view_essential(uv1, uv2, K, prm)
            assert a["ok"] and e["ok"] and a["n_points"] >= 20 and e["n_points"] >= 20
            X, idx = c.triangulate(rig["uv1"], rig["uv2"], rig["K"], *rig["T1to2"])
            assert len(idx) == 8
            r = c.recover_pose(a["E"], uv1, uv2, K, a["mask"])
            assert r["ok"] and r["n_points"] >= 20
            recs = [a, {k: v for k, v in e.items() if k != "hypotheses_run"}, dict(X=X, idx=idx), r]
            return b"".join(v.tobytes() if isinstance(v, np.ndarray) else repr(v).encode() for d in recs
                            for _, v in sorted(d.items()) if v is not None)

        def match(db):
            d = synth.make_pair(7, n_kp=130, desc_bytes=db, flip_p=0.01)
            got = c.match_hamming(d["desc1"], d["desc2"][:97], 0.7, 10.0)
            assert len(got) >= 30 and got.tobytes() == o.match_visual_features(d["desc1"], d["desc2"][:97], 0.7, 10.0).tobytes()

        def image_pair(db):
            d = synth.make_pair(9, n_kp=200, desc_bytes=db, flip_p=0.01)
            p = capi.default_params(num_hypotheses=128, sampler=capi.SAMPLER_PHILOX, seed=5, max_error_sq=1e-2)
            got = c.image_pair(d["desc1"], d["kp1"], d["desc2"][:171], d["kp2"][:171], d["K"], p)
            ref = o.image_pair(d["desc1"], d["kp1"], d["desc2"][:171], d["kp2"][:171], d["K"],
                               o.make_params(128, o.SAMPLER_PHILOX, 5, 1e-2), 0.7, 10.0)
            M, n = ref["n_matches"], ref["n_points"]
            assert ref["ok"] and got["ok"] and M >= 50 and got["n_matches"] == M and got["matches"].tobytes() == ref["matches"].tobytes()
            assert got["best_hyp"] == ref["best_hyp"] and got["best_count"] == ref["best_count"] and got["n_points"] == n
            assert np.array_equal(got["mask"], ref["mask"]) and np.array_equal(got["point_idx"], ref["point_idx"])

        first = point_calls()
        for step, db in ((match, 16), (image_pair, 64), (match, 32)):
            step(db)
            assert point_calls() == first, (step.__name__, db)
    finally:
        c.close()
