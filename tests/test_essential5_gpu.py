"""The five-point essential-matrix RANSAC on the GPU (essential5.hip) against the host build of the same header and the host
model of the stage (tests/cpp/five_point_host.cpp through tests/e5_model.py): byte for byte.  The kernels read the pair's points
from device memory at a wavefront-uniform address (no point chunks through LDS), so the point counts are the edges of the
sampler and of the capacity; the hypothesis counts are the edges of the 64-lane block and of a partial last block."""
import numpy as np
import pytest

import e5_model as em
import helpers
import oracle_lib as o
from mvslam_amd import capi

pytestmark = pytest.mark.gpu

REL_TOL, TIGHT = helpers.REL_TOL, helpers.TIGHT


def _scene(seed, m, outliers=0.0, planar=False, noise=0.0):
    """ideal-camera matches of a random pose (|omega| <= 0.3, unit baseline, depths in [2, 10]); the wrong matches come first
    and last alternately so that the identity sampler meets some"""
    rng = np.random.default_rng(seed)
    om = rng.normal(size=3)
    om *= rng.uniform(0.05, 0.3) / np.linalg.norm(om)
    R = o.se3_exp(np.concatenate([np.zeros(3), om]))[0]
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    z = rng.uniform(2, 10, size=m)
    X = np.stack([rng.uniform(-0.5, 0.5, m) * z, rng.uniform(-0.5, 0.5, m) * z, z], axis=1)
    if planar:
        X[:, 2] = 4.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    X2 = X @ R.T + t
    p1, p2 = X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]
    if noise:
        p1 = p1 + rng.normal(scale=noise, size=p1.shape)
        p2 = p2 + rng.normal(scale=noise, size=p2.shape)
    bad = rng.random(m) < outliers
    if outliers < 0.4:
        bad[:5] = False
    p2[bad] = rng.uniform(-0.5, 0.5, size=(int(bad.sum()), 2))
    return p1, p2, R, t, ~bad


def test_five_point_matches_the_host_build_byte_for_byte(ctx):
    rng = np.random.default_rng(5)
    cases = [em.random_sample(rng)[:2] for _ in range(506)]
    eq = (np.tile([0.25, -0.5], (5, 1)), np.tile([0.3, 0.1], (5, 1)))
    k = np.arange(5.0)[:, None]
    col = (np.hstack([0.1 * k, 0.2 * k - 0.3]), np.hstack([0.1 * k + 0.05, 0.2 * k - 0.25]))
    same = rng.uniform(-0.5, 0.5, size=(5, 2))
    cases += [eq, col, (same, same.copy()), (np.zeros((5, 2)), np.zeros((5, 2))),
              (1e200 * np.arange(1.0, 11).reshape(5, 2), -1e180 * np.arange(2.0, 12).reshape(5, 2)),
              (np.array([[0.1, 0.2], [0.3, np.nan], [0.5, 0.6], [0.7, 0.8], [0.9, 1.0]]), same)]
    assert len(cases) == 512
    total = 0
    for i, (p1, p2) in enumerate(cases):
        n, E = ctx.five_point(p1, p2)
        hn, hE = em.host_five_point(p1, p2)
        assert n == hn, i
        assert E.tobytes() == hE.tobytes(), i
        assert np.isfinite(E).all(), i
        total += n
    assert total > 1500


_SCENES = {}


def _get_scene(key):
    if key not in _SCENES:
        kind, m = key
        if kind == "outliers":
            _SCENES[key] = _scene(100 + m, m, outliers=0.5, noise=1e-4)
        elif kind == "planar":
            _SCENES[key] = _scene(200 + m, m, planar=True, noise=1e-4)
        else:
            _SCENES[key] = _scene(300 + m, m, outliers=0.2, noise=1e-4)
    return _SCENES[key]


def _check_ransac(ctx, p1, p2, thr, H, sampler, seed):
    got = ctx.ransac_essential(p1, p2, thr, H, sampler, seed, per_hyp=True)
    ref = em.host_ransac(p1, p2, thr, H, sampler, seed)
    assert np.array_equal(got["n_roots"], ref["n_roots"])
    assert np.array_equal(got["count"], ref["count"])
    assert (got["best_hyp"], got["best_root"], got["best_count"]) == (ref["best_hyp"], ref["best_root"], ref["best_count"])
    assert np.float64(got["best_residual"]).tobytes() == np.float64(ref["best_residual"]).tobytes()
    assert got["E"].tobytes() == ref["E"].tobytes()
    assert np.array_equal(got["mask"], ref["mask"])
    assert got["ok"] == (ref["found"] and ref["best_count"] > 0)
    return got


@pytest.mark.parametrize("m", [8, 9, 10, 11, 63, 64, 65, 4096])
def test_ransac_essential_point_counts(ctx, m):
    p1, p2 = _get_scene(("mixed", m))[:2]
    for sampler, thr in ((capi.SAMPLER_PHILOX, 1e-6), (capi.SAMPLER_IDENTITY, 1e-3)):
        _check_ransac(ctx, p1, p2, thr, 70, sampler, 11)


@pytest.mark.parametrize("H", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_ransac_essential_hypothesis_counts(ctx, H):
    p1, p2 = _get_scene(("mixed", 150))[:2]
    got = _check_ransac(ctx, p1, p2, 1e-6, H, capi.SAMPLER_PHILOX, 3)
    if H >= 63:
        assert got["best_count"] >= 100
    _check_ransac(ctx, p1, p2, 1e-3, H, capi.SAMPLER_IDENTITY, 3)


@pytest.mark.parametrize("kind", ["outliers", "planar"])
def test_ransac_essential_scenes(ctx, kind):
    p1, p2, R, t, good = _get_scene((kind, 300))
    for thr in (1e-6, 1e-4):
        got = _check_ransac(ctx, p1, p2, thr, 500, capi.SAMPLER_PHILOX, 9)
        assert got["best_count"] >= 0.8 * good.sum()


def test_ransac_essential_return_codes(ctx):
    p1, p2 = _get_scene(("mixed", 64))[:2]
    assert not ctx.ransac_essential(p1[:7], p2[:7], 1e-4, 8)["ok"]          # m < 8: MVS_NO_MODEL
    big = np.zeros((4097, 2))
    with pytest.raises(capi.MvsError) as e:
        ctx.ransac_essential(big, big, 1e-4, 8)
    assert e.value.status == capi.MVS_ERR_CAPACITY
    same = np.tile([0.1, 0.2], (20, 1))
    got = _check_ransac(ctx, same, same, 1e-4, 10, capi.SAMPLER_PHILOX, 0)   # every sample degenerate
    assert got["best_hyp"] == -1 and (got["n_roots"] == 0).all() and (got["count"] == -1).all() and not got["mask"].any()


def _pose_ok(got, R21, t21, tol=1e-3):
    return got["ok"] and np.abs(got["R"].reshape(3, 3) - R21).max() < tol and np.abs(got["t"] - t21).max() < tol


def test_two_view_essential_cube(ctx):
    """the reference's headline test (test/test-sfm.cpp:17-90): K = I, default threshold; a critical configuration for the 8-point
    solver (tests/test_oracle_kat.py::test_sfm_solve_cube_is_degenerate_for_8_point)"""
    rig = helpers.two_camera_rig("cube")
    prm = capi.default_params(num_hypotheses=64, sampler=capi.SAMPLER_PHILOX, seed=0)
    got = ctx.two_view_essential(rig["uv1"], rig["uv2"], rig["K"], prm)
    assert got["ok"] and got["n_points"] == 8 and got["best_count"] == 8
    assert np.abs(o.se3_ln(got["R"].reshape(3, 3), got["t"]) - np.array([1, 0, 0, 0, 0, 0.0])).max() < 1e-3
    assert got["point_idx"].tolist() == list(range(8))
    assert np.abs(got["points"] - rig["X"]).max() < 1e-3
    assert np.array_equal(got["F"], got["E"])


def _planar_scene():
    p1, p2, R, t, good = _scene(4242, 200, outliers=0.3, planar=True)
    K = helpers.camera(525.0, 525.0, 0.0, 320.0, 240.0)
    h = lambda p: np.hstack([p, np.ones((len(p), 1))]) @ K.T   # noqa: E731
    return p1, p2, h(p1)[:, :2], h(p2)[:, :2], K, R, t, good


def test_two_view_essential_planar_scene_and_the_gap_it_closes(ctx):
    p1, p2, uv1, uv2, K, R, t, good = _planar_scene()
    R21, t21 = o.se3_inverse(R, t)
    prm = capi.default_params(num_hypotheses=500, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-8)
    got = ctx.two_view_essential(uv1, uv2, K, prm)
    assert _pose_ok(got, R21, t21)
    # mask = the host model's on the normalised points the device sees (K^-1 by the cofactor inverse, as the oracle does)
    n1, n2 = o.normalize_points(K, uv1), o.normalize_points(K, uv2)
    ref = em.host_ransac(n1, n2, 1e-8, 500, capi.SAMPLER_PHILOX, 1)
    assert np.array_equal(got["mask"], ref["mask"]) and got["best_hyp"] == ref["best_hyp"]
    assert got["E"].tobytes() == ref["E"].tobytes()
    ok, Ro, to, pts, idx = o.recover_pose_and_points(ref["E"], n1, n2, ref["mask"])
    assert ok and got["point_idx"].tolist() == idx.tolist()
    assert helpers.rel_err(got["R1to2"], Ro) <= TIGHT and helpers.rel_err(got["points"], pts) <= TIGHT
    assert helpers.rel_err(got["t1to2"], to) <= TIGHT
    # the 8-point path on the same scene does not recover the pose: all points on one plane
    eight = ctx.two_view(uv1, uv2, K, prm)
    assert not _pose_ok(eight, R21, t21)


def test_batch_run_points_essential_equals_the_single_calls(ctx):
    P, N, H = 64, 96, 40
    rng = np.random.default_rng(77)
    fams = list(helpers.CAMERAS)
    Ks = np.stack([helpers.CAMERAS[fams[p % len(fams)]][0] for p in range(P)])   # per pair, skew on the aniso_skew pairs
    m = rng.integers(8, N + 1, size=P).astype(np.int32)
    m[3], m[10], m[11] = 5, N, 8
    uv1, uv2 = np.zeros((P, N, 2)), np.zeros((P, N, 2))
    for p in range(P):
        a, b2 = _scene(1000 + p, N, outliers=1.0 if p == 7 else 0.25, noise=1e-4)[:2]
        h = lambda q: np.hstack([q, np.ones((N, 1))]) @ Ks[p].T   # noqa: E731
        uv1[p], uv2[p] = h(a)[:, :2], h(b2)[:, :2]
        uv1[p, m[p]:], uv2[p, m[p]:] = 0.0, 0.0
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=500)
    b = capi.Batch(ctx, P, N, 32)
    b.upload_intrinsics(0, Ks, global_index=np.arange(P) * 3)
    outs = []
    for _ in range(2):
        b.run_points_essential(prm, uv1, uv2, m)
        b.sync()
        outs.append(b.download())
    b.close()
    for k in ("results", "mask", "points", "point_idx"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    out = outs[0]
    assert not out["results"][3]["valid"] and out["results"][3]["n_matches"] == 5
    n_valid = 0
    for p in range(P):
        prm1 = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=500 + 3 * p)
        one = ctx.two_view_essential(uv1[p, :m[p]], uv2[p, :m[p]], Ks[p], prm1)
        assert out["results"][p].tobytes() == one["raw"], p
        assert np.array_equal(out["mask"][p][:m[p]], one["mask"]), p
        n = int(out["results"][p]["n_points"]) if out["results"][p]["valid"] else 0
        assert out["points"][p][:n].tobytes() == one["points"].tobytes(), p
        assert np.array_equal(out["point_idx"][p][:n], one["point_idx"]), p
        assert not out["mask"][p][m[p]:].any() and not out["points"][p][n:].any()
        n_valid += bool(out["results"][p]["valid"])
    assert n_valid >= P // 2


_DOWNLOAD_KEYS = ("results", "matches", "mask", "points", "point_idx")


@pytest.mark.parametrize("P", [4, 64])
def test_batch_run_points_of_both_estimators_alternate_on_one_batch(ctx, P):
    """mvs_batch_run_points and mvs_batch_run_points_essential stage their points the same way and grow their own tables on
    the same batch: alternated on one batch, each gives the bytes it gives as the first call on a fresh batch -- below the
    half-batch threshold and at it (64 pairs: the 8-point call runs as two halves on two streams) -- also after a call
    refused for a match count beyond the capacity.  Every byte of a download is compared but the pose (R, t, R1to2, t1to2) in
    the record of a pair WITHOUT a model: the 8-point stage does not write it, what is there is the previous call's."""
    N, H = 96, 40
    rng = np.random.default_rng(78)
    fams = list(helpers.CAMERAS)
    Ks = np.stack([helpers.CAMERAS[fams[p % len(fams)]][0] for p in range(P)])
    m = rng.integers(8, N + 1, size=P).astype(np.int32)
    m[0], m[1], m[2] = 5, N, 8
    uv1, uv2 = np.zeros((P, N, 2)), np.zeros((P, N, 2))
    for p in range(P):
        a, b2 = _scene(2000 + p, N, outliers=0.25, noise=1e-4)[:2]
        h = lambda q: np.hstack([q, np.ones((N, 1))]) @ Ks[p].T   # noqa: E731
        uv1[p], uv2[p] = h(a)[:, :2], h(b2)[:, :2]
        uv1[p, m[p]:], uv2[p, m[p]:] = 0.0, 0.0
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=500, max_error_sq=2e-3)

    def new_batch():
        b = capi.Batch(ctx, P, N, 32)
        b.upload_intrinsics(0, Ks, global_index=np.arange(P) * 3)
        return b

    def run(b, name):
        getattr(b, name)(prm, uv1, uv2, m)
        b.sync()
        out = b.download()
        for k in ("R", "t", "R1to2", "t1to2"):
            out["results"][k][out["results"]["valid"] == 0] = 0.0
        return {k: out[k].tobytes() for k in _DOWNLOAD_KEYS}

    fresh = {}
    for name in ("run_points", "run_points_essential"):
        b = new_batch()
        fresh[name] = run(b, name)
        b.close()
    for name in fresh:   # most pairs have a model under either estimator (pair 0 has five matches: none), not the same one
        valid = np.frombuffer(fresh[name]["results"], dtype=capi.RESULT_DTYPE)["valid"]
        assert not valid[0] and valid.sum() >= P // 2, name
    assert fresh["run_points"]["results"] != fresh["run_points_essential"]["results"]
    b = new_batch()
    for name in ("run_points", "run_points_essential", "run_points", "run_points_essential"):
        assert run(b, name) == fresh[name], name
    for name in ("run_points", "run_points_essential"):
        for bad in (N + 1, -1):
            m_bad = m.copy()
            m_bad[P - 1] = bad
            with pytest.raises(capi.MvsError) as e:
                getattr(b, name)(prm, uv1, uv2, m_bad)
            assert e.value.status == capi.MVS_ERR_CAPACITY, (name, bad)
        assert run(b, name) == fresh[name], name
    b.close()
