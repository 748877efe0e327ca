"""VisualOdometer::add_frame over a resident sequence on the device: mvs_seq_run_lags and mvs_seq_odometry (DESIGN.md section
4.7.3).  The definition is tests/test_seq_odometry_host.py's; this file runs it against the device.

Shapes: 8 frames of 300 keypoints (test_seq_windows.SEQ_ARGS, the generator seed of test_seq_track.py), octaves 0 .. 2, 600
two-view hypotheses, 100 PnP hypotheses, lags up to 3, Q <= 3.

Fixtures (the gates stand open unless said otherwise: no inlier minimum, error / rotation / translation gates at 1e30):
  (a) Q = 2.  Pair (0, 1) initialises at frame 1 and the frames behind it track as they do in test_seq_track.py.
  (b) Q = 2, frame 4 uploaded with 5 keypoints.  Pairs (3, 4) and (4, 5) are invalid, so step 4 finds no candidates: LOST_PNP,
      reset, the queue restarts at frame 4.  Frame 5 cannot initialise (its only queued base is frame 4), frame 6 initialises
      from pair (5, 6) -- frame 5 becomes the INIT base of segment 1 -- and frame 7 tracks in its coordinates.
  (c) Q = 3, frame 1 uploaded with 5 keypoints.  Pairs (0, 1) and (1, 2) are invalid and (0, 2) is the only candidate at
      frame 2: ImagePair::update replaces the invalid held pair of base 0, which then initialises at lag 2; frame 3 tracks on a
      map keyed by frame 2's keypoints.
It is a condition of the tests that (a) has at least three TRACKED frames, (b) one in each segment, (c) one behind the lagged
initialisation; they assert it.  Finite gates: on (a)'s sequence at Q = 3, gates that no pair passes (each alone, and several
at once for the order) and, per gated quantity, a gate that exactly one pair of all lags passes; the values come from the
downloaded tables and sit 1e-6 (relative) away from every gated value, which _replay asserts.  On this sequence the update
scan of the closed-gate runs meets 11 (held, candidate) pairs: 7 refused for count, 2 for an error that is not smaller, 2
replaced, none refused for ssd -- a lagged pair with no fewer points and a smaller descriptor SSD does not occur in it; that
branch is the model's own test in test_seq_odometry_host.py only.  Whether a step's BA reports ok hangs on its prior-less points (test_seq_track.py's docstring
on its seed); the seed was not searched again for this file.
"""
import numpy as np
import pytest

import test_seq_odometry_host as om
import test_seq_track as st
import test_seq_windows as sw

N_FRAMES, N_KP, MAX_LAG = 8, 300, 3
PRM = sw.PRM
NOT_REACHED, INIT, TRACKED, LOST_PNP, LOST_FEW, LOST_BA, LOST_ERROR, INITIALIZING = range(8)
OPEN = 1e30


def make_seq():
    from mvslam_amd import synth

    return synth.make_sequence(N_FRAMES, seed=st.SEED, **sw.SEQ_ARGS)


def _octaves():
    return st._octaves(N_FRAMES)


def _params():
    from mvslam_amd import capi

    return capi.default_params(num_hypotheses=PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=PRM["seed"], max_error_sq=PRM["thr"])


def _pnp(seed=None):
    from mvslam_amd import capi

    return capi.default_pnp_params(num_hypotheses=100, seed=sw.PPRM["seed"] if seed is None else seed,
                                   reproj_error=sw.PPRM["err"])


def _vo(**kw):
    from mvslam_amd import capi

    return capi.default_vo_params(**dict(dict(max_error=OPEN), **kw))


def _init(Q, **kw):
    from mvslam_amd import capi

    return capi.default_vo_init_params(**dict(dict(frame_queue_size=Q, min_match_inlier_count=0, max_rotation_magnitude=OPEN,
                                                   max_translation_z=OPEN), **kw))


def _open(ctx, seq, n_kp=None, essential=False, max_lag=MAX_LAG):
    """upload, run, run_lags: the open Sequence"""
    from mvslam_amd import capi

    s = capi.Sequence(ctx, N_FRAMES, N_KP, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"] if n_kp is None else n_kp, seq["K"])
    s.upload_octaves(0, _octaves())
    (s.run_essential if essential else s.run)(_params(), _pnp())
    if max_lag:
        s.run_lags(_params(), max_lag, essential=essential)
    return s


def _lags(s, max_lag=MAX_LAG):
    """the downloads of every lag: raw[d] = (pairs, refined); tables for the model; pairs[d][b] as test_seq_track takes them"""
    raw, tables, pairs = {}, {}, {}
    for d in range(1, max_lag + 1):
        gp, gr = s.download_lag_pairs(d), s.download_lag_refined(d, point_cov=True)
        raw[d] = (gp, gr)
        tables[d], pairs[d] = [], []
        for b, r in enumerate(gp["results"]):
            v = bool(r["valid"])
            M, n = int(r["n_matches"]), int(r["n_points"]) if v else 0
            q = gr["refined"][b]
            tables[d].append(dict(valid=v, count=int(r["n_points"]), ssd=int(gp["match_ssd"][b]), ok=bool(q["ok"]),
                                  error=float(q["error"]), R=q["R"], t=q["t"]))
            pairs[d].append(dict(valid=v, matches=gp["matches"][b][:M], point_idx=gp["point_idx"][b][:n],
                                 points=gp["points"][b][:n], refined_points=gr["points"][b][:n], R=r["R"], t=r["t"]))
    return raw, tables, pairs


def _ssd(gp):
    out = []
    for b, r in enumerate(gp["results"]):
        n = int(r["n_points"]) if r["valid"] else 0
        dist = gp["matches"][b]["distance"][gp["point_idx"][b][:n]].astype(np.int64)
        out.append(int((dist * dist).sum()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1 lagged pairs

@pytest.mark.gpu
@pytest.mark.parametrize("essential", [False, True])
def test_gpu_lagged_pairs_equal_the_batch_path(ctx, essential):
    seq = make_seq()
    s = _open(ctx, seq, essential=essential)
    try:
        raw, _, _ = _lags(s)
        one, oner = s.download_pairs(), s.download_refined(point_cov=True)
        for k in ("results", "matches", "mask", "points", "point_idx"):
            assert raw[1][0][k].tobytes() == one[k].tobytes(), k
        for k in ("refined", "points", "point_cov"):
            assert raw[1][1][k].tobytes() == oner[k].tobytes(), k
        for d in range(1, MAX_LAG + 1):
            gp = raw[d][0]
            assert gp["match_ssd"].tolist() == _ssd(gp), d
            assert gp["results"]["valid"].any() and gp["match_ssd"].min() >= 0 and len(gp["results"]) == N_FRAMES - d
        assert any(raw[d][0]["match_ssd"].max() > 0 for d in raw)
        check_lags_equal_a_batch(ctx, raw, one, seq, _octaves(), _params(), essential)
    finally:
        s.close()


def check_lags_equal_a_batch(ctx, raw, one, seq, octaves, prm, essential, lags=(2, 3), desc_bytes=32):
    """raw[d] = (download_lag_pairs(d), download_lag_refined(d, point_cov=True)) of a sequence holding `seq` and `octaves`,
    run with `prm`: every byte equals an uploaded batch of the pairs (i, i + d); one = the sequence's download_pairs()"""
    from mvslam_amd import capi

    n_frames, n_kp = seq["desc"].shape[:2]
    for d in lags:
        P = n_frames - d
        b = capi.Batch(ctx, P, n_kp, desc_bytes)
        try:
            b.upload(0, seq["desc"][:P], seq["kp"][:P], seq["n_kp"][:P], seq["desc"][d:], seq["kp"][d:], seq["n_kp"][d:],
                     seq["K"], np.arange(P))
            b.upload_octaves(0, octaves[:P], octaves[d:])
            (b.run_essential if essential else b.run)(prm)
            b.refine(sigma_px=0.5)
            want, wantr = b.download(), b.download_refined(point_cov=True)
        finally:
            b.close()
        for k in ("results", "matches", "mask", "points", "point_idx"):
            assert raw[d][0][k].tobytes() == want[k].tobytes(), (d, k)
        for k in ("refined", "points", "point_cov"):   # every byte: rows past n_points are zero on both sides
            assert raw[d][1][k].tobytes() == wantr[k].tobytes(), (d, k)
        assert raw[d][0]["results"].tobytes() != one["results"][:P].tobytes()       # not the adjacent pairs again


# ---------------------------------------------------------------------------------------------------------------------
# 2 the replay

def _far(value, gate):
    return not np.isfinite(gate) or abs(value - gate) >= 1e-6 * max(abs(value), abs(gate))


def _replay(ctx, s, seq, vo, ip, pnp, refine, n_frames=N_FRAMES, octaves=None):
    """the device's run against the definition: the integer side exact from the downloaded lag tables and the device's own
    step verdicts; every initialisation and every tracking step from the device's own previous state.  Returns
    (snapshot, odo records).  n_frames, octaves: of the sequence `s` holds (default: this file's, _octaves())."""
    Q = ip.frame_queue_size
    _, tables, pairs = _lags(s, min(Q, n_frames - 1))
    snap, odo = st._snapshot(s), s.download_odometry_frames()
    fr, K, kp, octv = snap["frames"], seq["K"], seq["kp"], _octaves() if octaves is None else octaves
    gates = dict(min_inliers=ip.min_match_inlier_count, max_error=vo.max_error, max_rot=ip.max_rotation_magnitude,
                 max_tz=ip.max_translation_z)
    # no gate decides a case in the last place
    for d in tables:
        for e in tables[d]:
            if e["valid"] and e["ok"]:
                assert _far(e["error"], gates["max_error"]) and _far(om.so3_ln_sq(e["R"]), gates["max_rot"] ** 2)
                assert _far(abs(e["t"][2]), gates["max_tz"])
    assert all(_far(float(r["error"]), vo.max_error) for r in fr if r["state"] in (TRACKED, LOST_ERROR))
    inits = []
    states, recs, _ = om.odo_run(tables, n_frames, Q, gates, lambda f: int(fr[f]["state"]), lambda f, b, lag: inits.append((f, b, lag)))
    print("states", fr["state"].tolist(), "segments", odo["segment"].tolist(), "inits", inits)
    assert fr["state"].tolist() == states
    for f, r in enumerate(recs):
        for k in ("mode_after", "segment", "init_base", "queue_first", "n_updated", "gate_fail"):
            assert odo[f][k] == r[k], (f, k, odo[f], r)
        for k in ("rot_sq", "abs_tz"):
            assert abs(odo[f][k] - r[k]) <= 1e-12 * max(1.0, abs(r[k])), (f, k)
    empty = lambda f: np.all(snap["maps"][f]["point_id"] == -1) and not np.any(snap["maps"][f]["X"])
    zero_step = lambda f: snap["steps"][f]["raw"] == bytes(len(snap["steps"][f]["raw"]))
    init_of = {f: (b, lag) for f, b, lag in inits}
    next_id = 0
    for f in range(n_frames):
        rec, stp = fr[f], snap["steps"][f]
        if rec["state"] in (NOT_REACHED, INITIALIZING):
            want = np.zeros(1, fr.dtype)
            want["state"] = rec["state"]
            assert rec.tobytes() == want.tobytes() and empty(f) and zero_step(f)
            continue
        if rec["state"] == INIT and f not in init_of:       # the base frame of an initialisation
            assert np.array_equal(rec["R"], np.eye(3)) and not np.any(rec["t"]) and empty(f) and zero_step(f)
            continue
        if f in init_of:
            b, lag = init_of[f]
            p = pairs[lag][b]
            e = tables[lag][b]
            assert rec["state"] == INIT and rec["R"].tobytes() == e["R"].tobytes() and rec["t"].tobytes() == e["t"].tobytes()
            assert zero_step(f) and rec["pnp_best_hyp"] == -1
            kept = st.kept_points(p)
            assert rec["n_new"] == len(kept) > 0
            got = st._map_of(snap["maps"][f])
            assert sorted(got) == sorted(bq for _, _, bq in kept)
            for i, (j, a, bq) in enumerate(kept):
                assert got[bq][0] == next_id + i and got[bq][1].tobytes() == p["refined_points"][j].tobytes()
            next_id += len(kept)
            if fr[b]["state"] != INIT:                        # the lost frame of the segment before keeps its record
                assert fr[b]["state"] in om.LOST
            continue
        # a tracking step, as test_seq_track._replay checks it
        pair, map_prev = pairs[1][f - 1], st._map_of(snap["maps"][f - 1])
        R_l, t_l = fr[f - 1]["R"], fr[f - 1]["t"]
        assert fr[f - 1]["state"] in (INIT, TRACKED)
        cands = st.vo_join(pair, map_prev)
        assert rec["n_cand"] == len(cands)
        assert stp["cand_base_kp"].tolist() == [c[0] for c in cands] and stp["cand_new_kp"].tolist() == [c[1] for c in cands]
        assert stp["cand_xyz"].tobytes() == np.array([c[2] for c in cands]).reshape(-1, 3).tobytes()
        assert stp["cand_uv"].tobytes() == kp[f][stp["cand_new_kp"]].astype(np.float64).tobytes()
        one = ctx.pnp_solve(stp["cand_xyz"], stp["cand_uv"], K, _pnp(pnp.seed + f)) if len(cands) >= 7 else dict(ok=False, best_hyp=-1)
        assert rec["pnp_best_hyp"] == one["best_hyp"]
        if not one["ok"]:
            assert rec["state"] == LOST_PNP and empty(f) and rec["n_pnp_inliers"] == 0 and rec["n_tracked"] == rec["n_new"] == 0
            assert not np.any(rec["R"]) and not np.any(rec["t"])
            continue
        assert rec["R_pnp"].tobytes() == one["R"].tobytes() and rec["t_pnp"].tobytes() == one["t"].tobytes()
        assert rec["n_pnp_inliers"] == len(one["inliers"]) and np.array_equal(stp["pnp_inliers"], one["inliers"])
        scale = st.vo_scale(rec["t_pnp"], t_l)
        assert abs(rec["scale"] - scale) <= 1e-12 * max(1.0, abs(scale))
        if len(one["inliers"]) < vo.min_pnp_point_count:
            assert rec["state"] == LOST_FEW and empty(f) and rec["n_tracked"] == rec["n_new"] == 0
            continue
        pts = st.vo_assemble(pair, map_prev, cands, [int(c) for c in one["inliers"]], R_l, t_l, scale, next_id)
        n_new = sum(p[3] for p in pts)
        next_id += n_new
        nt = len(pts) - n_new
        assert (rec["n_tracked"], rec["n_new"]) == (nt, n_new)
        assert stp["point_id"].tolist() == [p[0] for p in pts] and stp["point_kp"].tolist() == [[p[1], p[2]] for p in pts]
        assert stp["point_is_new"].tolist() == [p[3] for p in pts]
        want = np.array([p[4] for p in pts]).reshape(-1, 3)
        assert stp["point_guess"][:nt].tobytes() == want[:nt].tobytes()
        assert np.all(np.abs(stp["point_guess"][nt:] - want[nt:]) <= 1e-12 * np.maximum(1.0, np.abs(want[nt:])))
        assert stp["guess_pose"][0].tobytes() == R_l.tobytes() + t_l.tobytes()
        assert stp["guess_pose"][1].tobytes() == rec["R_pnp"].tobytes() + rec["t_pnp"].tobytes()
        a, b = stp["point_kp"][:, 0], stp["point_kp"][:, 1]
        cov = []
        for frame, idx in ((f - 1, a), (f, b)):
            sd = np.ldexp(float(vo.sigma_px), octv[frame][idx].astype(np.int32))
            cov.append(np.stack([sd * sd, np.zeros(len(pts)), np.zeros(len(pts)), sd * sd], 1))
        pv = vo.point_sigma * vo.point_sigma
        prior = np.where(stp["point_is_new"][:, None] == 1, 0.0, np.tile((np.eye(3) * pv).reshape(9), (len(pts), 1)))
        var = [[vo.anchor_var[0]] * 3 + [vo.anchor_var[1]] * 3, [vo.regulator_var[0]] * 3 + [vo.regulator_var[1]] * 3]
        ref = ctx.ba_refine(K, stp["guess_pose"], var, stp["point_guess"], prior,
                            [kp[f - 1][a].astype(np.float64), kp[f][b].astype(np.float64)], cov, [stp["point_is_new"], None], refine)
        ba = stp["ba_frames"]
        assert bool(ba["ok"][1]) == ref["ok"] and ba["R"].tobytes() == ref["R"].tobytes() and ba["t"].tobytes() == ref["t"].tobytes()
        assert stp["points_refined"].tobytes() == ref["points"].tobytes()
        assert (rec["error"], rec["iterations"]) == (ref["error"], ref["iterations"]) == (ba["error"][1], ba["iterations"][1])
        print("frame %d: %d candidates, %d inliers, %d new, BA error %.4e" % (f, len(cands), nt, n_new, rec["error"]))
        if not ref["ok"] or rec["error"] > vo.max_error:
            assert rec["state"] == (LOST_ERROR if ref["ok"] else LOST_BA) and empty(f) and not np.any(rec["R"])
            continue
        assert rec["state"] == TRACKED and rec["R"].tobytes() == ref["R"][1].tobytes() and rec["t"].tobytes() == ref["t"][1].tobytes()
        got = st._map_of(snap["maps"][f])
        assert sorted(got) == sorted(int(x) for x in b)
        for i, p in enumerate(pts):
            assert got[p[2]][0] == p[0] and got[p[2]][1].tobytes() == ref["points"][i].tobytes()
        assert not np.any(snap["maps"][f]["X"][snap["maps"][f]["point_id"] < 0])
    return snap, odo


@pytest.fixture(scope="module")
def fixture_a(ctx):
    seq = make_seq()
    s = _open(ctx, seq)
    yield s, seq
    s.close()


@pytest.mark.gpu
def test_gpu_odometry_first_pair_initialises_and_tracks(ctx, fixture_a):
    """fixture (a)"""
    from mvslam_amd import capi

    s, seq = fixture_a
    vo, ip, rp = _vo(), _init(2), capi.default_refine_params()
    s.odometry(vo, ip, _pnp(), rp)
    snap, odo = _replay(ctx, s, seq, vo, ip, _pnp(), rp)
    assert odo["init_base"][1] == 0 and odo["segment"][1] == 0 and snap["frames"]["state"][:2].tolist() == [INIT, INIT]
    assert int((snap["frames"]["state"] == TRACKED).sum()) >= 3, "fixture (a) tracks fewer than three frames"


@pytest.mark.gpu
def test_gpu_odometry_loss_and_new_segment(ctx):
    """fixture (b)"""
    from mvslam_amd import capi

    seq = make_seq()
    n_kp = seq["n_kp"].copy()
    n_kp[4] = 5
    s = _open(ctx, seq, n_kp=n_kp)
    try:
        vo, ip, rp = _vo(), _init(2), capi.default_refine_params()
        s.odometry(vo, ip, _pnp(), rp)
        snap, odo = _replay(ctx, s, seq, vo, ip, _pnp(), rp)
    finally:
        s.close()
    states = snap["frames"]["state"].tolist()
    assert states[:2] == [INIT, INIT] and states[4] == LOST_PNP and states[5:7] == [INIT, INIT]   # 5: the new segment's base
    assert odo["mode_after"].tolist()[3:] == [1, 0, 0, 1, 1] and odo["gate_fail"][5] == 1
    assert odo["segment"].tolist()[4:] == [0, 0, 1, 1] and odo["init_base"][6] == 5 and odo["queue_first"][5] == 4
    assert TRACKED in states[2:4] and states[7] == TRACKED, "fixture (b) needs a TRACKED frame in each segment"
    assert np.any(snap["frames"][7]["t"]) and not np.any(snap["frames"][4]["R"])        # a pose in the new segment; none where lost
    ids6, ids3 = snap["maps"][6]["point_id"], snap["maps"][3]["point_id"]
    assert ids6[ids6 >= 0].min() > ids3.max()                                         # ids continue the call's one counter


@pytest.mark.gpu
def test_gpu_odometry_lagged_initialisation(ctx):
    """fixture (c)"""
    from mvslam_amd import capi

    seq = make_seq()
    n_kp = seq["n_kp"].copy()
    n_kp[1] = 5
    s = _open(ctx, seq, n_kp=n_kp)
    try:
        gp1, gp2 = s.download_lag_pairs(1), s.download_lag_pairs(2)
        assert not gp1["results"]["valid"][0] and not gp1["results"]["valid"][1] and gp2["results"]["valid"][0]
        vo, ip, rp = _vo(), _init(3), capi.default_refine_params()
        s.odometry(vo, ip, _pnp(), rp)
        snap, odo = _replay(ctx, s, seq, vo, ip, _pnp(), rp)
    finally:
        s.close()
    states = snap["frames"]["state"].tolist()
    assert states[:3] == [INIT, INITIALIZING, INIT]
    assert odo["init_base"][2] == 0 and odo["n_updated"][2] == 1 and odo["gate_fail"][1] == 1 and odo["segment"][2] == 0
    assert states[3] == TRACKED, "fixture (c) needs a TRACKED frame behind the lagged initialisation"
    assert snap["frames"][3]["n_cand"] >= 7                                           # joined through frame 2's keypoints


# ---------------------------------------------------------------------------------------------------------------------
# 3b finite gates, chosen from the downloaded tables (fixture (a)'s sequence, Q = 3, every pair of every lag valid)

def _quantities(tables):
    """per quantity, (value, lag, base) of every pair whose refinement is ok"""
    out = dict(count=[], error=[], rot=[], tz=[])
    for d in tables:
        for b, e in enumerate(tables[d]):
            if e["valid"] and e["ok"]:
                out["count"].append((e["count"], d, b))
                out["error"].append((e["error"], d, b))
                out["rot"].append((om.so3_ln_sq(e["R"]), d, b))
                out["tz"].append((abs(float(e["t"][2])), d, b))
    return out


def _gates_for(q, **which):
    """vo / init parameters: every gate open except those named, which close on every pair (a value no pair reaches)"""
    vo, ip = {}, {}
    if which.get("count"):
        ip["min_match_inlier_count"] = max(v for v, _, _ in q["count"]) + 1
    if which.get("error"):
        vo["max_error"] = 0.5 * min(v for v, _, _ in q["error"])
    if which.get("rot"):
        ip["max_rotation_magnitude"] = float(np.sqrt(0.25 * min(v for v, _, _ in q["rot"])))
    if which.get("tz"):
        ip["max_translation_z"] = 0.5 * min(v for v, _, _ in q["tz"])
    return _vo(**vo), _init(3, **ip)


@pytest.mark.gpu
@pytest.mark.parametrize("closed,code", [(("count",), 2), (("error",), 3), (("rot",), 4), (("tz",), 5),
                                         (("count", "error", "rot", "tz"), 2), (("error", "rot", "tz"), 3), (("rot", "tz"), 4)])
def test_gpu_odometry_closed_gates_keep_initializing(ctx, fixture_a, closed, code):
    """A gate that no pair passes: the run stays INITIALIZING over all seven frames, every frame reports that gate -- with
    several closed, the first in the reference's order -- and the held pairs of three queued frames meet their lagged
    candidates frame after frame: n_updated and the held table's effects equal the model's."""
    from mvslam_amd import capi

    s, seq = fixture_a
    _, tables, _ = _lags(s)
    assert all(e["valid"] and e["ok"] for d in tables for e in tables[d]), "fixture (a) has an invalid pair"
    q = _quantities(tables)
    vo, ip = _gates_for(q, **{k: True for k in closed})
    rp = capi.default_refine_params()
    s.odometry(vo, ip, _pnp(), rp)
    snap, odo = _replay(ctx, s, seq, vo, ip, _pnp(), rp)
    assert snap["frames"]["state"].tolist() == [NOT_REACHED] + [INITIALIZING] * (N_FRAMES - 1)
    assert odo["gate_fail"].tolist() == [0] + [code] * (N_FRAMES - 1) and odo["queue_first"].tolist() == [0, 0, 0, 0, 1, 2, 3, 4]
    assert np.all(odo["rot_sq"][1:] > 0.0) and np.all(odo["abs_tz"][1:] > 0.0) and np.all(odo["segment"] == -1)
    # what the update scan met, from the model's held table (the device's n_updated equals the model's, frame by frame)
    gates = dict(min_inliers=ip.min_match_inlier_count, max_error=vo.max_error, max_rot=ip.max_rotation_magnitude,
                 max_tz=ip.max_translation_z)
    _, recs, held = om.odo_run(tables, N_FRAMES, 3, gates, None)
    kinds = dict(count=0, ssd=0, error=0, replaced=0)
    for f in range(2, N_FRAMES):
        for b in range(recs[f]["queue_first"], f - 1):
            h, e = held[f - 1][b], tables[f - b][b]
            assert h["valid"]
            kind = ("count" if e["count"] < h["count"] else "ssd" if e["ssd"] < h["ssd"] else
                    "replaced" if e["error"] < h["error"] else "error")
            kinds[kind] += 1
    print("update scan:", kinds, "n_updated", odo["n_updated"].tolist())
    assert sum(kinds.values()) == 11 and kinds["replaced"] == int(odo["n_updated"].sum())


@pytest.mark.gpu
def test_gpu_odometry_one_pair_passes_a_finite_gate(ctx, fixture_a):
    """Per quantity, a gate between its best and its second best value over all pairs of all lags, so that exactly one pair
    (b, b + d) can pass it.  The run must stay INITIALIZING, reporting that gate, until frame b + d at the earliest, and
    everything it does equals the model.  The test needs one quantity at least whose best pair ends at frame 3 or later."""
    from mvslam_amd import capi

    s, seq = fixture_a
    _, tables, _ = _lags(s)
    q = _quantities(tables)
    rp = capi.default_refine_params()
    late = 0
    for name, code in (("count", 2), ("error", 3), ("rot", 4), ("tz", 5)):
        vals = sorted(q[name], reverse=name == "count")
        (v0, d, b), v1 = vals[0], vals[1][0]
        vo_kw, ip_kw = {}, {}
        if name == "count":
            if v0 == v1:
                continue
            ip_kw["min_match_inlier_count"] = int(v0)
        elif name == "error":
            vo_kw["max_error"] = 0.5 * (v0 + v1)
        elif name == "rot":
            ip_kw["max_rotation_magnitude"] = float(np.sqrt(0.5 * (v0 + v1)))
        else:
            ip_kw["max_translation_z"] = 0.5 * (v0 + v1)
        vo, ip = _vo(**vo_kw), _init(3, **ip_kw)
        s.odometry(vo, ip, _pnp(), rp)
        snap, odo = _replay(ctx, s, seq, vo, ip, _pnp(), rp)
        first = next((f for f in range(N_FRAMES) if odo["init_base"][f] >= 0), N_FRAMES)
        print(name, "best pair", (b, b + d), "value", v0, "next", v1, "first initialisation at", first,
              "gate_fail", odo["gate_fail"].tolist(), "n_updated", odo["n_updated"].tolist())
        assert first >= b + d and odo["gate_fail"][1:min(first, N_FRAMES)].tolist() == [code] * (min(first, N_FRAMES) - 1)
        if first < N_FRAMES:
            assert (int(odo["init_base"][first]), first) == (b, b + d)
        late += int(b + d >= 3)
    assert late >= 1, "no quantity's best pair ends at frame 3 or later: the fixture shows nothing"


@pytest.mark.gpu
def test_gpu_odometry_finite_gate_decides_a_late_initialisation(ctx, fixture_a):
    """A gate between two observed values under which the model, fed with the downloaded tables, initialises for the first time
    at frame 3 or later: the thresholds tried are the midpoints of adjacent sorted values of the refinement error, rot_sq and
    |t_z| over all pairs of all lags, the first that gives a late initialisation is taken (one per quantity that has one; at
    least one must).  The device must stay INITIALIZING, reporting that gate, up to the same frame, choose the same pair and
    track on from it."""
    from mvslam_amd import capi

    s, seq = fixture_a
    _, tables, _ = _lags(s)
    q = _quantities(tables)
    rp = capi.default_refine_params()
    found = 0
    for name, code in (("error", 3), ("rot", 4), ("tz", 5)):
        vals = sorted(set(v for v, _, _ in q[name]))
        pick = None
        for lo, hi in zip(vals, vals[1:]):
            mid = 0.5 * (lo + hi)
            if not (_far(lo, mid) and _far(hi, mid)):
                continue
            g = dict(min_inliers=0, max_error=OPEN, max_rot=OPEN, max_tz=OPEN)
            g.update({"error": dict(max_error=mid), "rot": dict(max_rot=float(np.sqrt(mid))), "tz": dict(max_tz=mid)}[name])
            _, recs, _ = om.odo_run(tables, N_FRAMES, 3, g, lambda f: TRACKED)
            first = next((f for f in range(N_FRAMES) if recs[f]["init_base"] >= 0), N_FRAMES)
            if 3 <= first < N_FRAMES:
                pick = (g, first, recs[first]["init_base"])
                break
        if pick is None:
            continue
        g, first, base = pick
        found += 1
        vo, ip = _vo(max_error=g["max_error"]), _init(3, max_rotation_magnitude=g["max_rot"], max_translation_z=g["max_tz"])
        s.odometry(vo, ip, _pnp(), rp)
        snap, odo = _replay(ctx, s, seq, vo, ip, _pnp(), rp)
        print(name, "gate", g, "initialises at", first, "from base", base, "gate_fail", odo["gate_fail"].tolist(),
              "n_updated", odo["n_updated"].tolist(), "states", snap["frames"]["state"].tolist())
        assert (int(odo["init_base"][first]), int(odo["segment"][first])) == (base, 0) and np.all(odo["init_base"][:first] == -1)
        assert odo["gate_fail"][1:first].tolist() == [code] * (first - 1)
        assert snap["frames"]["state"][first] == INIT
    assert found >= 1, "no threshold gives a first initialisation at frame 3 or later: the fixture shows nothing"


# ---------------------------------------------------------------------------------------------------------------------
# 4 the existing loop

@pytest.mark.gpu
def test_gpu_odometry_equals_the_tracking_loop(ctx, fixture_a):
    """gates open, Q = 2: the records, maps and steps of mvs_seq_track(init_pair 0, refined initialisation), byte for byte, for
    every frame of the sequence (the tracking loop loses none on this fixture, which the test asserts)"""
    from mvslam_amd import capi

    s, _ = fixture_a
    rp = capi.default_refine_params()
    s.odometry(_vo(), _init(2), _pnp(), rp)
    got = st._snapshot(s)
    s.track(_vo(init_pair=0, use_refined_init=1), _pnp(), rp)
    want = st._snapshot(s)
    states = want["frames"]["state"].tolist()
    print("tracking loop states", states)
    assert states == [INIT, INIT] + [TRACKED] * (N_FRAMES - 2), "the tracking loop loses a frame: the comparison would stop there"
    for f in range(N_FRAMES):
        assert st._frame_bytes(got, f) == st._frame_bytes(want, f), f


# ---------------------------------------------------------------------------------------------------------------------
# 5 refusals and side effects

@pytest.mark.gpu
def test_gpu_odometry_refusals_determinism_and_no_side_effects(ctx, fixture_a):
    from mvslam_amd import capi

    s, seq = fixture_a
    rp = capi.default_refine_params()

    def status_of(fn, *a, **kw):
        with pytest.raises(capi.MvsError) as e:
            fn(*a, **kw)
        return e.value.status

    s.track(_vo(), _pnp(), rp)
    track_before = st._snapshot(s)
    assert status_of(s.download_odometry_frames) == capi.MVS_ERR_INVALID_ARG         # the resident results are mvs_seq_track's
    before = (s.download_pairs(), s.download_tracks(), s.download_trajectory(), s.download_refined(point_cov=True))
    runs = []
    for _ in range(2):
        s.odometry(_vo(), _init(3), _pnp(), rp)
        snap = st._snapshot(s)
        runs.append(b"".join(st._frame_bytes(snap, f) for f in range(N_FRAMES)) + s.download_odometry_frames().tobytes())
    assert runs[0] == runs[1]
    after = (s.download_pairs(), s.download_tracks(), s.download_trajectory(), s.download_refined(point_cov=True))
    for x, y in zip(before, after):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k
    s.refine_windows(3, 1, max_points=512)
    win = s.download_windows()
    s.odometry(_vo(), _init(3), _pnp(), rp)
    assert [w["raw"] for w in s.download_windows()] == [w["raw"] for w in win]
    s.track(_vo(), _pnp(), rp)
    again = st._snapshot(s)
    for f in range(N_FRAMES):
        assert st._frame_bytes(again, f) == st._frame_bytes(track_before, f), f
    I = capi.MVS_ERR_INVALID_ARG
    for kw in (dict(sigma_px=0.0), dict(point_sigma=0.0), dict(anchor_var=(0.0, 1e-3)), dict(regulator_var=(1e-2, -1.0)),
               dict(max_error=-1.0)):
        assert status_of(s.odometry, _vo(**kw), _init(2), _pnp(), rp) == I, kw
    s.odometry(_vo(init_pair=-5, use_refined_init=7), _init(2), _pnp(), rp)           # ignored, not refused
    for kw in (dict(frame_queue_size=1), dict(min_match_inlier_count=-1), dict(max_rotation_magnitude=-0.1),
               dict(max_translation_z=-0.1), dict(frame_queue_size=MAX_LAG + 1)):          # lag 4 is not resident
        assert status_of(s.odometry, _vo(), _init(2, **kw), _pnp(), rp) == I, kw
    assert status_of(s.odometry, _vo(), _init(2), capi.default_pnp_params(num_hypotheses=0), rp) == I
    for lag in (0, MAX_LAG + 1):
        assert status_of(s.download_lag_pairs, lag) == I and status_of(s.download_lag_refined, lag) == I
    for kw in (dict(max_lag=0), dict(max_lag=N_FRAMES), dict(sigma_px=0.0), dict(sigma_px=-1.0)):
        args = dict(dict(max_lag=2, sigma_px=0.5), **kw)
        assert status_of(s.run_lags, _params(), args["max_lag"], sigma_px=args["sigma_px"]) == I, kw
    assert status_of(s.run_lags, capi.default_params(num_hypotheses=0), 2) == I
    fresh = capi.Sequence(ctx, N_FRAMES, N_KP, 32)
    try:
        fresh.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
        assert status_of(fresh.run_lags, _params(), 2) == I                              # not run
        assert status_of(fresh.odometry, _vo(), _init(2), _pnp(), rp) == I
        fresh.run(_params(), _pnp())
        assert status_of(fresh.odometry, _vo(), _init(2), _pnp(), rp) == I              # run, but no lags
        fresh.run_lags(_params(), 2)
        fresh.odometry(_vo(), _init(2), _pnp(), rp)
        assert status_of(fresh.odometry, _vo(), _init(3), _pnp(), rp) == I              # lag 3 is not resident
        fresh.run(_params(), _pnp())
        assert status_of(fresh.odometry, _vo(), _init(2), _pnp(), rp) == I              # the lags belonged to the run before
        assert status_of(fresh.download_lag_pairs, 1) == I
    finally:
        fresh.close()
