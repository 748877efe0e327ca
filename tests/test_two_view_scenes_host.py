"""The two-view scene families (tests/two_view_scenes.py) on the CPU oracle alone: what makes tests/test_two_view_scenes.py
non-vacuous, and the oracle itself against the scenes' ground truth.

  * ground truth: on noise-free matches of the well-posed families the oracle's sfm_solve returns the true rotation, the true
    direction of the baseline and the true points;
  * branch conditions: on the noisy scenes the families reach what the sideways scene never does -- the triangulation drops
    points, the points split between several of the four (R, t) candidates, more than one candidate outlives the 64-inlier
    prefix, the epipole lies inside the image, three of the four candidates win somewhere;
  * the tie regime's recorded `ok` flags."""
import numpy as np
import pytest

import oracle_lib as o
import two_view_scenes as tv

K = tv.synth.K_DEFAULT


# ----------------------------------------------------------------------------- ground truth
@pytest.mark.parametrize("family", tv.WELL_POSED)
def test_oracle_recovers_the_true_motion_and_points(family):
    """noise = 0, outliers = 0, 64 matches, 256 Philox hypotheses: R, t / |t| and baseline * points to 1e-6 (the values reached
    are printed: 1e-15 .. 1e-13 for the pose, up to 2e-9 for `far`, whose parallax is 1e-3 of a sideways scene's).  planar,
    near_planar, pure_rotation and tiny_baseline are degenerate for eight points: no accuracy claim."""
    for seed in (1, 2, 3):
        sc = tv.scene(seed, 64, family, 0.0, 0.0)
        ref = o.sfm_solve(sc["uv1"], sc["uv2"], K, o.make_params(256, o.SAMPLER_PHILOX, 5, 2e-3))
        assert ref["ok"] and ref["n_inliers"] == 64
        base = np.linalg.norm(sc["t"])
        err_R = np.abs(ref["R1to2"] - sc["R"]).max()
        err_t = np.abs(ref["t1to2"] - sc["t"] / base).max()
        Xt = sc["X"][ref["point_idx"]]
        err_X = (np.linalg.norm(ref["points"] * base - Xt, axis=1) / np.linalg.norm(Xt, axis=1)).max()
        print("%s seed %d: R %.2e  t %.2e  points %.2e (%d kept)" % (family, seed, err_R, err_t, err_X, ref["n_points"]))
        assert ref["n_points"] == 64
        assert err_R <= 1e-6 and err_t <= 1e-6 and err_X <= 1e-6


# ----------------------------------------------------------------------------- branch conditions
_SOLVED = {}


def solved(family, thr, seed=tv.SCENE_SEED):
    """(scene, oracle sfm_solve, normalised points, per-candidate surviving counts, winning candidate), computed once"""
    key = (family, thr, seed)
    if key not in _SOLVED:
        sc = tv.scene(seed, tv.M, family)
        ref = o.sfm_solve(sc["uv1"], sc["uv2"], K, o.make_params(tv.H, o.SAMPLER_PHILOX, tv.SAMPLER_SEED, thr))
        p1, p2 = o.normalize_points(K, sc["uv1"]), o.normalize_points(K, sc["uv2"])
        kept, win = None, None
        if ref["ok"]:
            cands = tv.candidates(ref["E"])
            kept = [len(o.triangulate_points(R, t, p1, p2, ref["mask"])[1]) for R, t in cands]
            ok, R, t, pts, idx = o.recover_pose_and_points(ref["E"], p1, p2, ref["mask"])
            assert ok and R.tobytes() == ref["R1to2"].tobytes() and t.tobytes() == ref["t1to2"].tobytes()
            hits = [c for c, (Rc, tc) in enumerate(cands) if Rc.tobytes() == R.tobytes() and tc.tobytes() == t.tobytes()]
            assert len(hits) == 1 and len(idx) == kept[hits[0]] == ref["n_points"]
            win = hits[0]
        _SOLVED[key] = (sc, ref, p1, p2, kept, win)
    return _SOLVED[key]


@pytest.mark.parametrize("thr", tv.THRESHOLDS)
@pytest.mark.parametrize("family", tv.FAMILIES)
def test_oracle_returns_a_model_for_every_family(family, thr):
    sc, ref, _, _, kept, win = solved(family, thr)
    print("%s thr %g: inliers %d points %d, per candidate %s, winner %d" % (family, thr, ref["n_inliers"], ref["n_points"], kept, win))
    assert ref["ok"] and ref["n_inliers"] >= 8 and ref["n_points"] >= 1
    if family == "side":
        assert ref["n_points"] == ref["n_inliers"]          # the control: nothing dropped, one candidate takes everything


@pytest.mark.parametrize("family", ["planar", "pure_rotation", "tiny_baseline", "mixed_far"])
def test_triangulation_drops_a_fifth_of_the_inliers(family):
    _, ref, _, _, kept, _ = solved(family, 1e-2)
    assert ref["n_points"] <= 0.8 * ref["n_inliers"], (ref["n_points"], ref["n_inliers"], kept)


@pytest.mark.parametrize("family", ["planar", "pure_rotation"])
def test_two_candidates_outlive_the_prefix(family):
    """finalize_select_kernel triangulates each candidate on a 64-inlier prefix and completes a loser only while it could still
    win: with two candidates beyond 64 points a loser has to be completed"""
    _, _, _, _, kept, _ = solved(family, 1e-2)
    assert sum(k > 64 for k in kept) >= 2, kept


@pytest.mark.parametrize("family", ["forward", "backward"])
def test_epipoles_lie_inside_the_image(family):
    """of the true motion and of the oracle's estimate, in both images (640 x 480)"""
    sc, ref, _, _, _, _ = solved(family, 1e-2)
    for R, t in ((sc["R"], sc["t"]), (ref["R1to2"], ref["t1to2"])):
        for e in (K @ t, K @ (-R.T @ t)):            # image 2: the projection of camera 1's centre; image 1: of camera 2's
            u, v = e[0] / e[2], e[1] / e[2]
            assert 0 <= u <= 640 and 0 <= v <= 480, (family, u, v)


# scene seeds of the winner census: the shared one suffices (all four candidates win on some family and threshold)
WINNER_SEEDS = (tv.SCENE_SEED,)


def test_three_of_the_four_candidates_win_somewhere():
    winners = set()
    for seed in WINNER_SEEDS:
        for family in tv.FAMILIES:
            for thr in tv.THRESHOLDS:
                winners.add(solved(family, thr, seed)[5])
    print("winning candidates:", sorted(winners))
    assert len(winners) >= 3


# ----------------------------------------------------------------------------- the tie regime
def test_tie_regime_flags_are_the_recorded_ones():
    """noise = 0, 30 % outliers, max_error_sq = 0 (the reference threshold): whether the oracle returns a model, per family --
    tv.TIE_OK is what tests/test_two_view_scenes.py asserts of the device"""
    got = {}
    for family in tv.FAMILIES:
        sc = tv.tie_scene(family)
        ref = o.sfm_solve(sc["uv1"], sc["uv2"], K, o.make_params(tv.H, o.SAMPLER_PHILOX, tv.SAMPLER_SEED, 0.0))
        got[family] = ref["ok"]
        print("%s: ok %d winner %d count %d residual %.17g points %d" % (family, ref["ok"], ref["best_hyp"], ref["best_count"],
                                                                         ref["best_residual"], ref["n_points"]))
    assert got == tv.TIE_OK
