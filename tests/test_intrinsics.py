"""Every path that reads the camera matrix, at general per-pair intrinsics (helpers.CAMERAS: fx != fy, skew, principal points
off centre and in a corner, a short and a long lens, and a different K for every pair of a batch).

CPU part: the oracle against references that share none of its code -- exact rational arithmetic for K^-1, numpy for the
epipolar residuals and the inlier rule, the generator's ground truth, the inlier rule of pnp_solve at a skewed K.
GPU part: the device against the oracle, with the checks and tolerances of the single-camera tests.
"""
from fractions import Fraction

import numpy as np
import pytest

import helpers
import oracle_lib as o
from mvslam_amd import capi, synth

FAMILIES = helpers.FAMILIES


# ----------------------------------------------------------------------------- K^-1 and normalisation
def _exact_inverse(K):
    a = [[Fraction(float(K[i, j])) for j in range(3)] for i in range(3)]
    det = sum(a[0][j] * (a[1][(j + 1) % 3] * a[2][(j + 2) % 3] - a[1][(j + 2) % 3] * a[2][(j + 1) % 3]) for j in range(3))
    return [[(a[(j + 1) % 3][(i + 1) % 3] * a[(j + 2) % 3][(i + 2) % 3] - a[(j + 1) % 3][(i + 2) % 3] * a[(j + 2) % 3][(i + 1) % 3])
             / det for j in range(3)] for i in range(3)]


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_inverse_and_normalisation_are_exact_at_every_camera(family):
    """K^-1 entry by entry and K^-1 (u, v, 1) against exact rational arithmetic, rounded once: within 1e-15 of the entry,
    and of the magnitude of the terms that make up the coordinate (a coordinate near the principal point is a cancellation)."""
    K, w, h = helpers.CAMERAS[family]
    Ke = _exact_inverse(K)
    assert np.allclose(np.array(Ke, dtype=float), np.linalg.inv(K), rtol=1e-14, atol=0)
    Ki = o.mat3_inverse(K)
    for i in range(3):
        for j in range(3):
            assert abs(Ki[i, j] - float(Ke[i][j])) <= 1e-15 * abs(float(Ke[i][j])), (i, j)
    rng = np.random.default_rng(11)
    uv = np.concatenate([np.stack([rng.uniform(0, w, 400), rng.uniform(0, h, 400)], 1),
                         [[0, 0], [w, h], [0, h], [w, 0], [K[0, 2], K[1, 2]]]]).astype(np.float32).astype(np.float64)
    got = o.normalize_points(K, uv)
    for (u, v), g in zip(uv, got):
        for r in range(2):
            terms = (Ke[r][0] * Fraction(u), Ke[r][1] * Fraction(v), Ke[r][2])
            assert abs(g[r] - float(sum(terms))) <= 1e-15 * float(sum(abs(t) for t in terms)), (u, v, r)


# ----------------------------------------------------------------------------- image_pair, checked in numpy
def _epipolar(K, kp1, kp2, mt, F):
    Kinv = np.linalg.inv(K)
    x1 = (Kinv @ np.c_[kp1[mt["trainIdx"]].astype(float), np.ones(len(mt))].T).T
    x2 = (Kinv @ np.c_[kp2[mt["queryIdx"]].astype(float), np.ones(len(mt))].T).T
    return np.abs(np.einsum("ij,jk,ik->i", x2, F, x1))


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_image_pair_at_every_camera(family):
    """The winner's inlier mask is the threshold rule on epipolar residuals built from numpy's K^-1 (1e-9 relative margin),
    at 1e-3 and at the per-pair reference threshold 5e-2 / fx / fy; noise-free pairs give back the generator's motion."""
    K = helpers.CAMERAS[family][0]
    noisy = helpers.make_family_pair(31, family, n_kp=1000)
    exact = helpers.make_family_pair(31, family, n_kp=1000, noise_px=0.0)
    for p, thr in ((noisy, 1e-3), (noisy, 0.0), (exact, 1e-3), (exact, 0.0)):
        ref = o.image_pair(p["desc1"], p["kp1"], p["desc2"], p["kp2"], K, o.make_params(1000, o.SAMPLER_PHILOX, 5, thr))
        assert ref["n_matches"] > 700
        if thr > 0:
            assert ref["ok"]
        if not ref["ok"]:      # the reference threshold on noisy points: fewer than eight inliers, no model
            continue
        t = thr if thr > 0 else 5e-2 / K[0, 0] / K[1, 1]
        res = _epipolar(K, p["kp1"], p["kp2"], ref["matches"], ref["F"])
        inl = ref["mask"].astype(bool)
        assert inl.sum() == ref["best_count"] == ref["n_inliers"]
        assert (res[inl] < t * (1 + 1e-9)).all() and (res[~inl] > t * (1 - 1e-9)).all()
        if p is exact:
            assert np.abs(ref["R1to2"] - p["R_1to2"]).max() < 1e-4
            d = ref["t1to2"] / np.linalg.norm(ref["t1to2"])
            assert np.abs(d - p["t_1to2"] / np.linalg.norm(p["t_1to2"])).max() < 2e-3    # tele: a narrow baseline angle


# ----------------------------------------------------------------------------- pnp_solve's inlier rule at a skewed K
PNP_THR = 0.05


def _pnp_probe_scene():
    """60 exact correspondences at aniso_skew (the first four: the one identity-sampler hypothesis, so the pose is exact)
    plus probes displaced by (a, b) = (fx dx, fy dy) in K^-1-normalised
    coordinates, chosen so that three rules disagree about them:
      rule   a^2 + b^2 <= thr^2                              (what pnp_solve applies: fx dx, fy dy)
      pixel  (a + skew / fy * b)^2 + b^2 <= thr^2            (the true pixel distance at this K)
      swap   (fy / fx * a)^2 + (fx / fy * b)^2 <= thr^2      (fx and fy exchanged)"""
    K = helpers.CAMERAS["aniso_skew"][0]
    fx, sk, fy = K[0, 0], K[0, 1], K[1, 1]
    rng = np.random.default_rng(77)
    R, t = o.rodrigues(np.array([0.03, -0.05, 0.02])), np.array([0.1, -0.05, 0.2])
    n_clean = 60
    shifts = [(0.98 / np.sqrt(2), 0.98 / np.sqrt(2))] * 2 + [(1.02 / np.sqrt(2), -1.02 / np.sqrt(2))] * 2 + \
             [(1.3, 0.0)] * 4 + [(0.0, 0.8)] * 1
    m = n_clean + len(shifts)
    X = np.stack([rng.uniform(-1.5, 1.5, m), rng.uniform(-1, 1, m), rng.uniform(4, 8, m)], 1)
    Xc = X @ R.T + t
    xn = Xc[:, :2] / Xc[:, 2:3]
    ab = np.zeros((m, 2))
    ab[n_clean:] = np.array(shifts) * PNP_THR
    xi = xn + ab / [fx, fy]
    uv = np.stack([fx * xi[:, 0] + sk * xi[:, 1] + K[0, 2], fy * xi[:, 1] + K[1, 2]], 1)
    a, b = ab[:, 0], ab[:, 1]
    rules = dict(rule=a * a + b * b <= PNP_THR ** 2, pixel=(a + sk / fy * b) ** 2 + b * b <= PNP_THR ** 2,
                 swap=(fy / fx * a) ** 2 + (fx / fy * b) ** 2 <= PNP_THR ** 2)
    return K, X, uv, rules


def test_pnp_probe_scene_separates_the_rules():
    _, _, _, rules = _pnp_probe_scene()
    assert (rules["rule"] != rules["pixel"]).sum() == 4 and (rules["rule"] != rules["swap"]).sum() >= 4
    assert rules["rule"].sum() != rules["swap"].sum()      # a swapped rule also changes the hypothesis' count


def test_oracle_pnp_inlier_rule_is_fx_dx_fy_dy_on_normalised_points():
    """the reprojection test is fx^2 dx^2 + fy^2 dy^2 <= err^2 on K^-1-normalised points -- not the pixel
    distance (which would add skew * dy to the first component), and not with fx and fy exchanged."""
    K, X, uv, rules = _pnp_probe_scene()
    r = o.pnp_solve(X, uv, K, o.make_pnp_params(1, o.SAMPLER_IDENTITY, 0, PNP_THR))
    assert r["ok"]
    assert r["inliers"].tolist() == np.nonzero(rules["rule"])[0].tolist()


@pytest.mark.gpu
def test_gpu_pnp_inlier_rule_is_the_oracle_rule(ctx):
    K, X, uv, rules = _pnp_probe_scene()
    got = ctx.pnp_solve(X, uv, K, capi.default_pnp_params(num_hypotheses=1, sampler=capi.SAMPLER_IDENTITY,
                                                          reproj_error=PNP_THR))
    ref = o.pnp_solve(X, uv, K, o.make_pnp_params(1, o.SAMPLER_IDENTITY, 0, PNP_THR))
    assert got["ok"] and got["best_hyp"] == ref["best_hyp"]
    assert got["inliers"].tolist() == ref["inliers"].tolist() == np.nonzero(rules["rule"])[0].tolist()
    assert got["R"].tobytes() == ref["R"].tobytes() and got["t"].tobytes() == ref["t"].tobytes()


# ----------------------------------------------------------------------------- GPU: batches with a K per pair
_MIXED = {}


def _mixed10():
    if "d" not in _MIXED:
        _MIXED["d"] = helpers.mixed_batch(0, 10, n_kp=2000)
    return _MIXED["d"]


def _same_outputs(a, b, i, j):
    """pair i of download a and pair j of download b: every output byte"""
    ra, rb = a["results"][i], b["results"][j]
    assert ra.tobytes() == rb.tobytes(), (i, j)
    M, n = int(ra["n_matches"]), int(ra["n_points"])
    assert a["matches"][i][:M].tobytes() == b["matches"][j][:M].tobytes(), (i, j)
    assert a["mask"][i][:M].tobytes() == b["mask"][j][:M].tobytes(), (i, j)
    assert a["point_idx"][i][:n].tobytes() == b["point_idx"][j][:n].tobytes(), (i, j)
    assert a["points"][i][:n].tobytes() == b["points"][j][:n].tobytes(), (i, j)


@pytest.mark.gpu
def test_gpu_mixed_batch_parity_through_the_prescreened_stage(ctx):
    """10 pairs (two per camera family) x 2000 keypoints x 50 000 hypotheses at 1e-2, 1e-3 and the per-pair reference
    threshold: every pair against the oracle (winner, count, residual sum bitwise, mask, point indices, points bitwise);
    the stage's mode per family from each family's pairs alone, which must add up to the mixed batch's own bookkeeping."""
    P, N, H = 10, 2000, 50000
    data = _mixed10()
    seen, mode1_families = set(), set()
    for thr in (1e-2, 1e-3, 0.0):
        prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=synth.SEED_BASE, max_error_sq=thr)
        _, out = helpers.run_batch(ctx, 0, P, N, prm, data=data)
        refs = helpers.check_batch_against_oracle(data, out, prm, n_threads=16)
        for i, ref in enumerate(refs):
            r = out["results"][i]
            assert r["best_residual"] == ref["best_residual"], (thr, i)
            if ref["ok"]:
                assert out["points"][i][:ref["n_points"]].tobytes() == ref["points"].tobytes(), (thr, i)
        live = int((out["results"]["n_matches"] >= 8).sum())
        b = capi.Batch(ctx, P, N, 32)
        b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"],
                 data["global_index"])
        whole = b.stats(prm)["pairs_mode"]
        b.close()
        per = {}
        for fam in FAMILIES:
            sub = helpers.take(data, np.nonzero(data["family"] == fam)[0])
            b = capi.Batch(ctx, len(sub["n1"]), N, 32)
            b.upload(0, sub["desc1"], sub["kp1"], sub["n1"], sub["desc2"], sub["kp2"], sub["n2"], sub["K"], sub["global_index"])
            per[fam] = b.stats(prm)["pairs_mode"]
            b.close()
        print("max_error_sq=%g pairs_mode %s per family %s" % (thr, whole, per))
        assert sum(whole) == live == P, (thr, whole)
        assert [sum(per[f][m] for f in FAMILIES) for m in range(3)] == whole, (thr, whole, per)
        seen |= {m for m in range(3) if whole[m]}
        mode1_families |= {f for f in FAMILIES if per[f][1]}
    assert {0, 1} <= seen
    assert mode1_families - {"default"}


def _pinned_copy(a):
    p = capi.pinned_empty(a.shape, a.dtype)
    p[...] = a
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [1e-2, 0.0])
def test_gpu_K_travels_with_its_pair(ctx, thr):
    """One mixed batch four ways -- one upload; three synchronous slices at first = 0, 3, 7; two asynchronous slices from
    pinned buffers; the pairs in reverse order with their global indices kept -- gives byte-identical outputs per pair,
    which are the oracle's."""
    P, N, H = 10, 800, 4096
    data = helpers.mixed_batch(40, P, n_kp=N)
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=23, max_error_sq=thr)
    keys = ("desc1", "kp1", "n1", "desc2", "kp2", "n2", "K", "global_index")
    _, one = helpers.run_batch(ctx, 0, P, N, prm, data=data)
    helpers.check_batch_against_oracle(data, one, prm, n_threads=16)
    b = capi.Batch(ctx, P, N, 32)
    for a, e in ((0, 3), (3, 7), (7, 10)):
        b.upload(a, *[data[k][a:e] for k in keys])
    b.run(prm)
    b.sync()
    sliced = b.download()
    pinned = []
    for a, e in ((0, 5), (5, 10)):
        arrs = [_pinned_copy(np.ascontiguousarray(data[k][a:e])) for k in keys]
        pinned += arrs
        b.upload_async(a, *arrs)
    b.run(prm)
    b.sync()
    asynced = b.download()
    b.close()
    for a in pinned:
        capi.pinned_free(a)
    rev = helpers.take(data, np.arange(P)[::-1])
    _, reverse = helpers.run_batch(ctx, 0, P, N, prm, data=rev)
    for i in range(P):
        _same_outputs(one, sliced, i, i)
        _same_outputs(one, asynced, i, i)
        _same_outputs(one, reverse, i, P - 1 - i)


@pytest.mark.gpu
def test_gpu_half_batches_keep_each_pairs_K(ctx):
    """65 mixed pairs (at least 64 run as two halves on two streams; the split at pair 33 falls inside the family cycle) at
    the per-pair reference threshold: halves on and off give the same bytes, and pairs either side of the split and at both
    ends are the oracle's."""
    P, N, H = 65, 400, 2048
    data = helpers.mixed_batch(300, P, n_kp=N)
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=91, max_error_sq=0.0)
    outs = []
    for halves in (True, False):
        ctx.set_half_batches(halves)
        try:
            outs.append(helpers.run_batch(ctx, 0, P, N, prm, data=data)[1])
        finally:
            ctx.set_half_batches(True)
    for i in range(P):
        _same_outputs(outs[0], outs[1], i, i)
    keep = [0, 1, 32, 33, 34, 35, 36, 37, 63, 64]
    helpers.check_batch_against_oracle(helpers.take(data, keep), {k: v[keep] for k, v in outs[0].items()}, prm, n_threads=16)


# ----------------------------------------------------------------------------- GPU: refinement with a K per problem
def _close(a, b, rel, what):
    scale = max(np.abs(b).max(), 1e-300)
    err = np.abs(np.asarray(a) - np.asarray(b)).max() / scale
    assert err <= rel, "%s: relative error %.3e > %.1e" % (what, err, rel)


@pytest.mark.gpu
def test_gpu_batch_refine_reads_each_pairs_K(ctx):
    """ImagePair::refine of a mixed batch with random octaves, pair by pair against the oracle's sfm_refine with that
    pair's K (tolerances of test_gpu_batch_refine_matches_oracle_and_improves_reprojection)."""
    P, N = 10, 600
    data = helpers.mixed_batch(0, P, n_kp=N)
    rng = np.random.default_rng(5)
    oct1 = rng.integers(0, 4, size=(P, N)).astype(np.uint8)
    oct2 = rng.integers(0, 4, size=(P, N)).astype(np.uint8)
    b = capi.Batch(ctx, P, N)
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"],
             data["global_index"])
    b.upload_octaves(0, oct1, oct2)
    prm = capi.default_params(num_hypotheses=2048, sampler=capi.SAMPLER_PHILOX, seed=11, max_error_sq=1e-2)
    b.run(prm)
    b.refine(sigma_px=0.5)
    b.sync()
    out = b.download()
    ref = b.download_refined(points=True, point_cov=True)
    b.close()
    n_checked = 0
    for p in range(P):
        r = out["results"][p]
        if not r["valid"]:
            assert ref["refined"][p]["ok"] == 0
            continue
        n = int(r["n_points"])
        mt = out["matches"][p][out["point_idx"][p][:n]]
        p1 = data["kp1"][p][mt["trainIdx"]].astype(np.float64)
        p2 = data["kp2"][p][mt["queryIdx"]].astype(np.float64)
        s1 = 0.5 * 2.0 ** oct1[p][mt["trainIdx"]].astype(np.float64)
        s2 = 0.5 * 2.0 ** oct2[p][mt["queryIdx"]].astype(np.float64)
        cov1 = (s1 * s1)[:, None] * np.eye(2).reshape(1, 4)
        cov2 = (s2 * s2)[:, None] * np.eye(2).reshape(1, 4)
        want = o.sfm_refine(p1, cov1, p2, cov2, data["K"][p].reshape(3, 3), r["R"], r["t"], out["points"][p][:n])
        got = ref["refined"][p]
        assert got["ok"] == 1 and want["ok"], p
        assert abs(got["error"] - want["error"]) <= 1e-9 * want["error"], p
        assert np.abs(got["R"] - want["R"]).max() < 1e-9 and np.abs(got["t"] - want["t"]).max() < 1e-9, p
        assert np.abs(ref["points"][p][:n] - want["points"]).max() < 1e-8, p
        _close(got["pose_cov"], want["pose_cov"], 1e-6, "pose_cov")
        _close(ref["point_cov"][p][:n], want["point_cov"], 1e-6, "point_cov")
        n_checked += 1
    assert n_checked >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(helpers.K_REFINE))
def test_gpu_refine_entry_points_at_general_K(ctx, name):
    """sfm_refine, pnp_refine and ba_refine at a skewed / anisotropic and at a short off-centre K, against the oracle at
    the tolerances of tests/test_refine.py (the skew column of the projection Jacobian is non-zero here)."""
    import test_refine as tr

    K = helpers.K_REFINE[name]
    pb = tr.two_view_problem(2, 300, K=K, sig=0.5, baseline=0.3, depth=(2.0, 10.0))
    ref = o.sfm_refine(pb["p1"], pb["cov"], pb["p2"], pb["cov"], K, pb["Rg"], pb["tg"], pb["Xg"])
    got = ctx.sfm_refine(pb["p1"], pb["cov"], pb["p2"], pb["cov"], K, pb["Rg"], pb["tg"], pb["Xg"])
    assert got["ok"] == ref["ok"] is True and got["iterations"] == ref["iterations"]
    assert abs(got["error"] - ref["error"]) <= 1e-10 * ref["error"]
    assert np.abs(got["R"] - ref["R"]).max() < 1e-10 and np.abs(got["t"] - ref["t"]).max() < 1e-10
    assert np.abs(got["points"] - ref["points"]).max() < 1e-9
    _close(got["pose_cov"], ref["pose_cov"], 1e-7, "pose_cov")
    _close(got["point_cov"], ref["point_cov"], 1e-7, "point_cov")
    pb = tr.pnp_problem(6, 200, K=K)
    ref = o.pnp_refine(pb["X"], pb["wcov"], pb["uv"], pb["icov"], K, pb["Rg"], pb["tg"])
    got = ctx.pnp_refine(pb["X"], pb["wcov"], pb["uv"], pb["icov"], K, pb["Rg"], pb["tg"])
    assert got["ok"] and ref["ok"] and got["iterations"] == ref["iterations"]
    assert abs(got["error"] - ref["error"]) <= 1e-10 * max(ref["error"], 1.0)
    assert np.abs(got["R"] - ref["R"]).max() < 1e-10 and np.abs(got["t"] - ref["t"]).max() < 1e-10
    _close(got["pose_cov"], ref["pose_cov"], 1e-7, "pose_cov")
    pb = tr.track_refine_problem(4, 400, 60, K=K)
    want = o.ba_refine(K, pb["poses"], pb["var"], pb["Xg"], pb["pcov"], pb["obs"], pb["cov"], pb["valid"])
    got = ctx.ba_refine(K, pb["poses"], pb["var"], pb["Xg"], pb["pcov"], pb["obs"], pb["cov"], pb["valid"])
    assert got["ok"] and want["ok"] and got["iterations"] == want["iterations"]
    assert abs(got["error"] - want["error"]) <= 1e-10 * want["error"]
    assert np.abs(got["R"] - want["R"]).max() < 1e-9 and np.abs(got["t"] - want["t"]).max() < 1e-9
    assert np.abs(got["points"] - want["points"]).max() < 1e-8
    for f in range(2):
        _close(got["pose_cov"][f], want["pose_cov"][f], 1e-6, "pose_cov[%d]" % f)
    _close(got["point_cov"], want["point_cov"], 1e-6, "point_cov")


# ----------------------------------------------------------------------------- GPU: single-shot pnp_solve near the threshold
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_gpu_pnp_solve_at_every_camera(ctx, family):
    """image noise of about the reprojection threshold (0.05 px): inlier decisions, and so the winner, depend on fx and fy
    separately; winner, inliers and pose bitwise against the oracle."""
    K = helpers.CAMERAS[family][0]
    rng = np.random.default_rng(FAMILIES.index(family) + 90)
    n, H = 300, 500
    R, t = o.rodrigues(rng.normal(size=3) * 0.08), np.array([0.2, -0.1, 0.3])
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 9, n)], axis=1)
    uv = o.project_points(K, R, t, X) + rng.normal(scale=0.05, size=(n, 2))
    got = ctx.pnp_solve(X, uv, K, capi.default_pnp_params(num_hypotheses=H, seed=7, reproj_error=PNP_THR))
    ref = o.pnp_solve(X, uv, K, o.make_pnp_params(H, o.SAMPLER_PHILOX, 7, PNP_THR))
    assert ref["ok"] and got["ok"] and got["best_hyp"] == ref["best_hyp"]
    assert np.array_equal(got["inliers"], ref["inliers"])
    assert got["R"].tobytes() == ref["R"].tobytes() and got["t"].tobytes() == ref["t"].tobytes()


# ----------------------------------------------------------------------------- pre-screen model band on every box
@pytest.mark.parametrize("family", FAMILIES)
def test_model_band_covers_the_oracle_at_every_camera(family):
    """test_model_band_covers_the_oracle_on_synthetic_pairs once per camera: the ideal-coordinate boxes here are about
    +-0.61 x +-0.46 (default), one-sided (offcentre), +-5.3 x +-4.0 (wide) and +-0.08 (tele)"""
    import test_prescreen as tp

    stats = dict(n=0, cert=0, worst=0.0)
    for pi in range(2):
        d = helpers.make_family_pair(pi, family, n_kp=1000)
        mt = o.match_visual_features(d["desc1"], d["desc2"], 0.7, 10.0)
        p1 = o.normalize_points(d["K"], d["kp1"][mt["trainIdx"]].astype(np.float64))
        p2 = o.normalize_points(d["K"], d["kp2"][mt["queryIdx"]].astype(np.float64))
        bbox = tp._bbox(p1, p2)
        for hh in range(400):
            tp._check(p1, p2, o.sample8(synth.SEED_BASE + pi, hh, len(mt)), bbox, stats)
    assert stats["cert"] > 0.9 * stats["n"]
    assert stats["worst"] < 1e-3


# ----------------------------------------------------------------------------- pnp_solve: the count follows the rule too
def _pnp_count_scene():
    """Two rigid groups of 30 exact correspondences at aniso_skew, seen under two different poses A and B, each with two
    probes: A's displaced by b = 0.8 thr (an inlier under the rule, an outlier with fx and fy exchanged), B's by a = 1.3 thr
    (the other way round).  Under the rule a hypothesis solved from A counts 32 and one from B 30, so an A hypothesis wins;
    with fx and fy exchanged in the counting it is 30 against 32 and a B hypothesis wins."""
    K = helpers.CAMERAS["aniso_skew"][0]
    fx, sk, fy = K[0, 0], K[0, 1], K[1, 1]
    rng = np.random.default_rng(5)
    poses = [(o.rodrigues(np.array([0.03, -0.05, 0.02])), np.array([0.1, -0.05, 0.2])),
             (o.rodrigues(np.array([-0.04, 0.06, -0.01])), np.array([-0.2, 0.1, 0.1]))]
    probes = [(0.0, 0.8), (1.3, 0.0)]
    Xs, uvs, kind = [], [], []
    for g, (R, t) in enumerate(poses):
        X = np.stack([rng.uniform(-1.5, 1.5, 32), rng.uniform(-1, 1, 32), rng.uniform(4, 8, 32)], 1)
        Xc = X @ R.T + t
        ab = np.zeros((32, 2))
        ab[30:] = np.array(probes[g]) * PNP_THR
        xi = Xc[:, :2] / Xc[:, 2:3] + ab / [fx, fy]
        Xs.append(X)
        uvs.append(np.stack([fx * xi[:, 0] + sk * xi[:, 1] + K[0, 2], fy * xi[:, 1] + K[1, 2]], 1))
        kind += ["%s clean" % "AB"[g]] * 30 + ["%s probe" % "AB"[g]] * 2
    return K, np.concatenate(Xs), np.concatenate(uvs), np.array(kind)


def _pnp_count_check(r, kind, H, seed):
    n = len(kind)
    samples = [set(kind[o.sample4(seed, h, n)]) for h in range(H)]
    assert {"B clean"} in samples                                  # a B hypothesis is there to win under a swapped rule
    assert r["ok"] and samples[r["best_hyp"]] == {"A clean"}
    assert r["inliers"].tolist() == np.nonzero(np.char.startswith(kind, "A"))[0].tolist()


def test_oracle_pnp_count_follows_the_rule():
    K, X, uv, kind = _pnp_count_scene()
    _pnp_count_check(o.pnp_solve(X, uv, K, o.make_pnp_params(200, o.SAMPLER_PHILOX, 1, PNP_THR)), kind, 200, 1)


@pytest.mark.gpu
def test_gpu_pnp_count_follows_the_rule(ctx):
    """the counting kernel's rule (the winner) and the inlier list's rule, on the device, against the oracle"""
    K, X, uv, kind = _pnp_count_scene()
    got = ctx.pnp_solve(X, uv, K, capi.default_pnp_params(num_hypotheses=200, sampler=capi.SAMPLER_PHILOX, seed=1,
                                                          reproj_error=PNP_THR))
    ref = o.pnp_solve(X, uv, K, o.make_pnp_params(200, o.SAMPLER_PHILOX, 1, PNP_THR))
    _pnp_count_check(got, kind, 200, 1)
    assert got["best_hyp"] == ref["best_hyp"] and np.array_equal(got["inliers"], ref["inliers"])
    assert got["R"].tobytes() == ref["R"].tobytes() and got["t"].tobytes() == ref["t"].tobytes()


# ----------------------------------------------------------------------------- GPU: single-shot two-view entry points
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_gpu_single_shot_two_view_entry_points_at_every_camera(ctx, family):
    """image_pair, two_view (at 2e-3 and at 5e-2 / fx / fy), triangulate and recover_pose on one pair of each camera,
    against the oracle with the checks of tests/test_gpu_parity.py"""
    from test_gpu_parity import _check_two_view

    K = helpers.CAMERAS[family][0]
    p = helpers.make_family_pair(50 + FAMILIES.index(family), family, n_kp=1000)
    H, thr = 2048, 2e-3
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=17, max_error_sq=thr)
    got = ctx.image_pair(p["desc1"], p["kp1"], p["desc2"], p["kp2"], K, prm)
    ref = o.image_pair(p["desc1"], p["kp1"], p["desc2"], p["kp2"], K, o.make_params(H, o.SAMPLER_PHILOX, 17, thr),
                       prm.ratio, prm.max_dist)
    M = ref["n_matches"]
    assert ref["ok"] and got["n_matches"] == M and got["matches"].tobytes() == ref["matches"].tobytes()
    _check_two_view(got, ref, M)
    mt = ref["matches"]
    uv1, uv2 = p["kp1"][mt["trainIdx"]].astype(np.float64), p["kp2"][mt["queryIdx"]].astype(np.float64)
    for t in (thr, 0.0):
        g = ctx.two_view(uv1, uv2, K, capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=17,
                                                          max_error_sq=t))
        _check_two_view(g, o.sfm_solve(uv1, uv2, K, o.make_params(H, o.SAMPLER_PHILOX, 17, t)), M)
    R12, t12 = ref["R1to2"], ref["t1to2"]
    pts, idx = ctx.triangulate(uv1, uv2, K, R12, t12)
    # the oracle's triangulation on the same T_1to2 (sfm_triangulate would take it as the inverse of pose 2 and compose it
    # back: a rounding of the input that the far, narrow-baseline points of the short and long lenses amplify past 1e-12)
    rpts, ridx = o.triangulate_points(R12, t12, o.normalize_points(K, uv1), o.normalize_points(K, uv2))
    assert len(ridx) > 8 and idx.tolist() == ridx.tolist()
    assert helpers.rel_err(pts, rpts) <= helpers.TIGHT
    g = ctx.recover_pose(ref["E"], uv1, uv2, K, ref["mask"])
    ok, R, t, rpts, ridx = o.recover_pose_and_points(ref["E"], o.normalize_points(K, uv1), o.normalize_points(K, uv2),
                                                     ref["mask"])
    assert ok and g["ok"] and g["point_idx"].tolist() == ridx.tolist()
    assert helpers.rel_err(g["R1to2"], R) <= helpers.TIGHT and helpers.rel_err(g["t1to2"], t) <= helpers.TIGHT
    assert helpers.rel_err(g["points"], rpts) <= helpers.TIGHT


# ----------------------------------------------------------------------------- GPU: a sequence at a skewed camera
@pytest.mark.gpu
def test_gpu_sequence_at_a_skewed_off_centre_camera(ctx):
    """20 frames at fx 640, fy 450, skew 25, principal point (250, 300): pairs, the join, every track's PnP and the
    trajectory fold against the oracle, as test_gpu_sequence_matches_oracle and the trajectory test do at K_DEFAULT"""
    import test_sequence as ts

    K = helpers.camera(640.0, 450.0, 25.0, 250.0, 300.0)
    F, N = 20, 600
    seq = synth.make_sequence(F, n_kp=N, n_map=8000, noise_px=0.3, K=K)
    prm = dict(H=600, seed=4242, thr=1e-2)
    pprm = dict(H=300, seed=99, err=2.0)
    s = capi.Sequence(ctx, F, N, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
    s.run(capi.default_params(num_hypotheses=prm["H"], sampler=capi.SAMPLER_PHILOX, seed=prm["seed"], max_error_sq=prm["thr"]),
          capi.default_pnp_params(num_hypotheses=pprm["H"], seed=pprm["seed"], reproj_error=pprm["err"]))
    gp, gt, tr = s.download_pairs(), s.download_tracks(), s.download_trajectory()
    s.close()
    pairs, tracks = ts.oracle_sequence(seq, prm, pprm, threads=16)
    for k, ref in enumerate(pairs):
        r = gp["results"][k]
        M = ref["n_matches"]
        assert r["n_matches"] == M and gp["matches"][k][:M].tobytes() == ref["matches"].tobytes(), k
        assert bool(r["valid"]) == ref["ok"] and np.array_equal(gp["mask"][k][:M], ref["mask"]), k
        if ref["ok"]:
            n = ref["n_points"]
            assert np.array_equal(gp["point_idx"][k][:n], ref["point_idx"]), k
            assert gp["points"][k][:n].tobytes() == ref["points"].tobytes(), k
    n_ok = 0
    for q, ref in enumerate(tracks):
        t = gt["tracks"][q]
        nc = len(ref["X"])
        assert t["n_corr"] == nc and gt["corr_xyz"][q][:nc].tobytes() == ref["X"].tobytes(), q
        assert gt["corr_uv"][q][:nc].tobytes() == ref["uv"].tobytes(), q
        assert bool(t["ok"]) == ref["ok"] and t["best_hyp"] == ref["best_hyp"], q
        if ref["ok"]:
            n_ok += 1
            ni = len(ref["inliers"])
            assert t["n_inliers"] == ni and np.array_equal(gt["inlier_idx"][q][:ni], ref["inliers"]), q
            assert t["R"].tobytes() == ref["R"].tobytes() and t["t"].tobytes() == ref["t"].tobytes(), q
    assert n_ok >= F - 3
    res, trk = gp["results"], gt["tracks"]
    want = o.seq_chain(res["R"], res["t"], res["valid"], trk["R"], trk["t"], trk["ok"])
    for k in ("R", "t", "pair_scale", "track_scale"):
        assert tr[k].tobytes() == want[k].tobytes(), k
