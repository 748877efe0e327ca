"""The five-point RANSAC behind the matcher on the GPU: mvs_image_pair_essential, mvs_batch_run_essential and
mvs_seq_run_essential against the point-fed calls they replace (mvs_match_hamming + mvs_two_view_essential,
mvs_batch_run_points_essential) and the host model (tests/e5_model.py), byte for byte.

Match counts are crafted: independent random 256-bit descriptors are at least ~85 bits apart, so copying k descriptors of the
base frame into the pair frame gives exactly k matches under max_dist = 10."""
import os
import subprocess

import numpy as np
import pytest

import e5_model as em
import helpers
import oracle_lib as o
from mvslam_amd import capi, synth
from test_essential_paths_host import SRC, build_one_pass, one_pass_exe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DATA_KEYS = ("results", "mask", "points", "point_idx")


def _correspondences(p):
    """(i, j): keypoint i of the base frame is keypoint j of the pair frame -- a pair made with outlier_frac = 0, flip_p = 0"""
    where = {bytes(d): j for j, d in enumerate(p["desc2"])}
    return [(i, where[bytes(p["desc1"][i])]) for i in range(p["n_common"])]


def crafted_pair(index, n_kp, M, wrong=0.0, **kw):
    """keypoints of synth.make_pair, descriptors with exactly M matches; a fraction `wrong` of them joins two different points"""
    p = synth.make_pair(index, n_kp=n_kp, outlier_frac=0.0, flip_p=0.0, common_frac=1.0 if M > 0.85 * n_kp else 0.9, **kw)
    corr = _correspondences(p)
    assert len(corr) >= M, (len(corr), M)
    rng = np.random.default_rng(77000 + index)
    d1 = rng.integers(0, 256, size=(n_kp, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, size=(n_kp, 32), dtype=np.uint8)
    pick = [corr[k] for k in rng.permutation(len(corr))[:M]]
    n_wrong = int(wrong * M)
    js = [j for _, j in pick]
    js[:n_wrong] = js[1:n_wrong] + js[:1] if n_wrong > 1 else js[:n_wrong]
    for (i, _), j in zip(pick, js):
        d2[j] = d1[i]
    return dict(p, desc1=d1, desc2=d2)


def _expected_n_run(count, M, H, p):
    """the termination rule of five_point.hpp on a host count table ([H][10], -1 past n_roots): the operations of e5_confident"""
    if M < 8:
        return 0
    T, j = min(64, H), 0
    while T < H:
        c = int(count[:T].max())
        if c >= 1:
            w = float(c) / float(M)
            w2 = w * w
            x = 1.0 - (w2 * w2) * w
            for _ in range(6 + j):
                x = x * x
            if x <= 1.0 - p:
                return T
        T, j = (H if T >= H - T else 2 * T), j + 1
    return H


# ---- 1. one pair -----------------------------------------------------------------------------------------------------------------
_THR = 1e-5
_ONE_PAIR_H = (1, 63, 64, 65, 200)


def _one_pair_case(M):
    if M is None:
        return synth.make_pair(31, n_kp=300)
    return crafted_pair(40 + M, 300, M, wrong=0.2 if M >= 63 else 0.0)


def _check_one_pair(ctx, p, H, confidence=0.0):
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=77, max_error_sq=_THR, ratio=0.7, max_dist=10.0)
    got = ctx.image_pair_essential(p["desc1"], p["kp1"], p["desc2"], p["kp2"], p["K"], prm)
    mt = ctx.match_hamming(p["desc1"], p["desc2"], ratio=0.7, max_dist=10.0)
    M = len(mt)
    assert got["n_matches"] == M and got["matches"].tobytes() == mt.tobytes()
    if M < 8:
        assert not got["ok"] and not got["valid"] and got["hypotheses_run"] == 0 and got["best_hyp"] == -1
        assert not got["R"].any() and not got["t"].any() and len(got["points"]) == 0
        return got
    uv1 = p["kp1"][mt["trainIdx"]].astype(np.float64)
    uv2 = p["kp2"][mt["queryIdx"]].astype(np.float64)
    two = ctx.two_view_essential(uv1, uv2, p["K"], prm)
    assert got["raw"] == two["raw"]
    assert got["ok"] == two["ok"] and got["hypotheses_run"] == two["hypotheses_run"]
    assert np.array_equal(got["mask"], two["mask"])
    assert got["points"].tobytes() == two["points"].tobytes() and np.array_equal(got["point_idx"], two["point_idx"])
    # the host model on the points as prep_points_kernel / match_compact normalise them
    n1, n2 = o.normalize_points(p["K"], uv1), o.normalize_points(p["K"], uv2)
    ref = em.host_ransac(n1, n2, _THR, H, capi.SAMPLER_PHILOX, 77)
    want_run = _expected_n_run(ref["count"], M, H, confidence) if confidence > 0.0 else H
    assert got["hypotheses_run"] == want_run
    if want_run < H:
        ref = em.host_ransac(n1, n2, _THR, want_run, capi.SAMPLER_PHILOX, 77)
    assert (got["best_hyp"], got["best_count"]) == (ref["best_hyp"], ref["best_count"])
    assert np.float64(got["best_residual"]).tobytes() == np.float64(ref["best_residual"]).tobytes()
    assert got["E"].tobytes() == ref["E"].tobytes()          # hence the same root of the winning hypothesis
    assert np.array_equal(got["mask"], ref["mask"])
    return got


@pytest.mark.parametrize("M", [7, 8, 9, 10, 11, 63, 64, 65, 257, None])
def test_image_pair_essential_equals_the_two_calls_and_the_host_model(ctx, M):
    p = _one_pair_case(M)
    n_valid = 0
    for H in _ONE_PAIR_H:
        got = _check_one_pair(ctx, p, H)
        assert M is None or got["n_matches"] == M
        n_valid += bool(got["valid"])
    if M == 7:
        assert n_valid == 0                                   # MVS_NO_MODEL (sfm-solve.cpp:37)
    elif M is None or M >= 63:
        assert n_valid >= 3                                   # the stage is exercised: H >= 63 finds the motion


def test_image_pair_essential_honours_the_confidence_level(ctx):
    try:
        ctx.set_essential_confidence(0.99)
        runs = [_check_one_pair(ctx, _one_pair_case(M), 200, confidence=0.99)["hypotheses_run"] for M in (None, 65, 7)]
    finally:
        ctx.set_essential_confidence(0.0)
    assert runs[0] == 64 and runs[2] == 0, runs


def test_image_pair_essential_argument_errors(ctx):
    p = synth.make_pair(1, n_kp=100)
    prm = capi.default_params(num_hypotheses=16, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-2)
    Kbad = p["K"].copy()
    Kbad[2, 0] = 0.5
    with pytest.raises(capi.MvsError) as e:
        ctx.image_pair_essential(p["desc1"], p["kp1"], p["desc2"], p["kp2"], Kbad, prm)
    assert e.value.status == capi.MVS_ERR_BAD_INTRINSICS
    with pytest.raises(capi.MvsError) as e:      # a train image with one row: visual-feature.cpp:67 needs two neighbours
        ctx.image_pair_essential(p["desc1"][:1], p["kp1"][:1], p["desc2"], p["kp2"], p["K"], prm)
    assert e.value.status == capi.MVS_ERR_INVALID_ARG
    with pytest.raises(capi.MvsError) as e:      # a call that fails leaves no n_run behind
        ctx.essential_hypotheses_run()
    assert e.value.status == capi.MVS_ERR_INVALID_ARG
    bad = capi.default_params(num_hypotheses=0)
    with pytest.raises(capi.MvsError) as e:
        ctx.image_pair_essential(p["desc1"], p["kp1"], p["desc2"], p["kp2"], p["K"], bad)
    assert e.value.status == capi.MVS_ERR_INVALID_ARG
    # too few matches for a model: false, never an abort (estimator-RANSAC.cpp:25-29)
    got = ctx.image_pair_essential(p["desc1"][:5], p["kp1"][:5], p["desc2"][:5], p["kp2"][:5], p["K"], prm)
    assert not got["ok"] and got["n_matches"] <= 5 and got["hypotheses_run"] == 0


# ---- 2. the descriptor-fed batch against the point-fed one and the host model ------------------------------------------------------
_BATCH_N = 128
_HEAVY, _FEW, _EIGHT, _FULL = 2, 3, 4, 1     # pairs with special match lists (all below P = 5)


def _family_batch(P, first=300):
    """P pairs of _BATCH_N keypoints, camera family p mod 5, global_index 3 p; pair _FEW has five matches, pair _EIGHT eight,
    pair _FULL every keypoint, and 70 % of pair _HEAVY's matches join two different points"""
    N = _BATCH_N
    fams = list(helpers.CAMERAS)
    out = dict(desc1=np.empty((P, N, 32), np.uint8), kp1=np.empty((P, N, 2), np.float32), desc2=np.empty((P, N, 32), np.uint8),
               kp2=np.empty((P, N, 2), np.float32), n1=np.full(P, N, np.int32), n2=np.full(P, N, np.int32), K=np.empty((P, 9)),
               global_index=3 * np.arange(P, dtype=np.int64))
    for p in range(P):
        K, w, h = helpers.CAMERAS[fams[p % len(fams)]]
        kw = dict(K=K, width=w, height=h)
        if p == _FEW:
            q = crafted_pair(first + p, N, 5, **kw)
        elif p == _EIGHT:
            q = crafted_pair(first + p, N, 8, **kw)
        elif p == _FULL:
            q = crafted_pair(first + p, N, N, **kw)
        elif p == _HEAVY:
            q = crafted_pair(first + p, N, 100, wrong=0.7, **kw)
        else:
            q = synth.make_pair(first + p, n_kp=N, **kw)
        out["desc1"][p], out["kp1"][p], out["desc2"][p], out["kp2"][p] = q["desc1"], q["kp1"], q["desc2"], q["kp2"]
        out["K"][p] = q["K"].reshape(9)
    return out


def _upload(b, data):
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"], data["global_index"])


def _matched_points(data, out):
    """uv1 / uv2 / m of run_points_essential from the downloaded match lists"""
    P, N = out["matches"].shape
    m = out["results"]["n_matches"].astype(np.int32)
    uv1, uv2 = np.zeros((P, N, 2)), np.zeros((P, N, 2))
    for p in range(P):
        mt = out["matches"][p][:m[p]]
        uv1[p, :m[p]] = data["kp1"][p][mt["trainIdx"]]
        uv2[p, :m[p]] = data["kp2"][p][mt["queryIdx"]]
    return uv1, uv2, m


@pytest.mark.parametrize("confidence", [0.0, 0.99])
@pytest.mark.parametrize("P", [5, 64])
def test_descriptor_fed_and_point_fed_tables_are_equal_and_the_host_models(ctx, P, confidence):
    N, H = _BATCH_N, 1000
    data = _family_batch(P)
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=900, max_error_sq=_THR, ratio=0.7, max_dist=10.0)
    b = capi.Batch(ctx, P, N, 32)
    _upload(b, data)
    try:
        ctx.set_essential_confidence(confidence)
        b.run_essential(prm)
        b.sync()
        wide, wide_run, wide_tab = b.download(), b.hypotheses_run(), b.download_essential_tables(H)
        uv1, uv2, m = _matched_points(data, wide)
        b.run_points_essential(prm, uv1, uv2, m)
        b.sync()
        plain, plain_run, plain_tab = b.download(), b.hypotheses_run(), b.download_essential_tables(H)
        with pytest.raises(capi.MvsError) as e:
            b.download_essential_tables(H - 1)               # not that run's hypothesis count
        assert e.value.status == capi.MVS_ERR_INVALID_ARG
    finally:
        ctx.set_essential_confidence(0.0)
        b.close()
    assert m[_FEW] == 5 and m[_EIGHT] == 8 and m[_FULL] == N and m[_HEAVY] == 100
    assert np.array_equal(wide_run, plain_run)
    assert np.array_equal(wide_tab[0], plain_tab[0]) and np.array_equal(wide_tab[1], plain_tab[1])
    for k in _DATA_KEYS:
        assert wide[k].tobytes() == plain[k].tobytes(), k
    assert wide["results"]["valid"].sum() >= (P + 1) // 2 and not wide["results"][_FEW]["valid"]
    # the tables' convention: nothing for a pair without eight matches and from a pair's n_run on, -1 past n_roots
    n_roots, count = wide_tab
    assert wide_run[_FEW] == 0 and not n_roots[_FEW].any() and (count[_FEW] == -1).all()
    for p in range(P):
        T = wide_run[p]
        assert not n_roots[p, T:].any() and (count[p, T:] == -1).all()
        assert ((count[p, :T] >= 0) == (np.arange(10)[None, :] < n_roots[p, :T, None])).all()
    assert n_roots.sum() > 0
    # the host model: the outlier-heavy pair and an ordinary one, tables and where the rule stops them
    for p in (_HEAVY, 0):
        n1 = o.normalize_points(data["K"][p].reshape(3, 3), uv1[p, :m[p]])
        n2 = o.normalize_points(data["K"][p].reshape(3, 3), uv2[p, :m[p]])
        ref = em.host_ransac(n1, n2, _THR, H, capi.SAMPLER_PHILOX, 900 + 3 * p)
        want = _expected_n_run(ref["count"], int(m[p]), H, confidence) if confidence > 0.0 else H
        assert wide_run[p] == want, p
        assert np.array_equal(n_roots[p, :want], ref["n_roots"][:want]) and np.array_equal(count[p, :want], ref["count"][:want])
    if confidence > 0.0:
        assert wide_run[0] == 64 and wide_run[_HEAVY] > 64, wide_run[:5]
    else:
        assert (wide_run[np.arange(P) != _FEW] == H).all()


# ---- 3. the estimators alternate on one batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [4, 64])
def test_run_and_run_essential_alternate_on_one_batch(ctx, P):
    """mvs_batch_run and mvs_batch_run_essential grow their own tables on one batch: alternated, each gives the bytes it gives as
    the first call on a fresh batch -- below the half-batch threshold and at it (64 pairs: the 8-point call runs as two halves on
    two streams).  Every byte of a download is compared but the pose (R, t, R1to2, t1to2) in the record of a pair WITHOUT a
    model: the 8-point stage does not write it, what is there is the previous call's."""
    N, H = _BATCH_N, 40
    data = _family_batch(max(P, 5))
    data = {k: v[:P] for k, v in data.items()}
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=500, max_error_sq=2e-3, ratio=0.7, max_dist=10.0)

    def new_batch():
        b = capi.Batch(ctx, P, N, 32)
        _upload(b, data)
        return b

    def run(b, name):
        getattr(b, name)(prm)
        b.sync()
        out = b.download()
        for k in ("R", "t", "R1to2", "t1to2"):
            out["results"][k][out["results"]["valid"] == 0] = 0.0
        return {k: out[k].tobytes() for k in ("matches",) + _DATA_KEYS}

    fresh = {}
    for name in ("run", "run_essential"):
        b = new_batch()
        fresh[name] = run(b, name)
        b.close()
    for name in fresh:
        valid = np.frombuffer(fresh[name]["results"], dtype=capi.RESULT_DTYPE)["valid"]
        assert not valid[_FEW] and valid.sum() >= P // 2, name
    assert fresh["run"]["matches"] == fresh["run_essential"]["matches"]
    assert fresh["run"]["results"] != fresh["run_essential"]["results"]
    b = new_batch()
    for name in ("run", "run_essential", "run", "run_essential"):
        assert run(b, name) == fresh[name], name
    b.close()


# ---- 4. the sequence ---------------------------------------------------------------------------------------------------------------
def test_seq_run_essential_equals_the_batch_and_the_oracle_join(ctx):
    F, N, H = 6, 500, 128
    seq = synth.make_sequence(F, n_kp=N, n_map=6000, noise_px=0.3)
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=4242, max_error_sq=1e-4, ratio=0.7, max_dist=10.0)
    pprm = dict(H=300, seed=99, err=2.0)
    pnp = capi.default_pnp_params(num_hypotheses=pprm["H"], seed=pprm["seed"], reproj_error=pprm["err"])
    s = capi.Sequence(ctx, F, N, 32)
    b = capi.Batch(ctx, F - 1, N, 32)
    try:
        s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
        b.upload(0, seq["desc"][:-1], seq["kp"][:-1], seq["n_kp"][:-1], seq["desc"][1:], seq["kp"][1:], seq["n_kp"][1:], seq["K"],
                 np.arange(F - 1))
        s.run_essential(prm, pnp)
        gp, gt, traj = s.download_pairs(), s.download_tracks(), s.download_trajectory()
        b.run_essential(prm)
        b.sync()
        want = b.download()
        for k in ("matches",) + _DATA_KEYS:
            assert gp[k].tobytes() == want[k].tobytes(), k
        assert np.array_equal(s.download_hypotheses_run(), np.full(F - 1, H))
        assert gp["results"]["valid"].all()
        for v in traj.values():
            assert np.isfinite(v).all()
        s.refine_pairs(sigma_px=0.5)
        refined = s.download_refined()
        assert np.isfinite(refined["refined"]["R"]).all() and np.isfinite(refined["refined"]["t"]).all()
        assert refined["refined"]["ok"].sum() >= F - 3
        ctx.set_essential_confidence(0.99)
        s.run_essential(prm, pnp)
        b.run_essential(prm)
        b.sync()
        assert np.array_equal(s.download_hypotheses_run(), b.hypotheses_run())
        assert s.download_pairs()["results"].tobytes() == b.download()["results"].tobytes()
    finally:
        ctx.set_essential_confidence(0.0)
        s.close()
        b.close()
    # the tracks: the oracle's join + pnp_solve (tests/test_sequence.py::oracle_sequence) on the device's pair outputs
    n_ok = 0
    for q in range(F - 2):
        ra, rb = gp["results"][q], gp["results"][q + 1]
        X, uv = np.zeros((0, 3)), np.zeros((0, 2))
        na, mb = int(ra["n_points"]) if ra["valid"] else 0, int(rb["n_matches"])
        if na and mb:
            idx = gp["point_idx"][q][:na]
            tbl = np.full(int(seq["n_kp"][q + 1]) + 1, -1, dtype=np.int64)
            tbl[gp["matches"][q]["queryIdx"][idx]] = np.arange(na)
            j = tbl[gp["matches"][q + 1]["trainIdx"][:mb]]
            hit = j >= 0
            X = gp["points"][q][j[hit]].reshape(-1, 3)
            uv = seq["kp"][q + 2][gp["matches"][q + 1]["queryIdx"][:mb][hit]].astype(np.float64).reshape(-1, 2)
        ref = dict(ok=False, best_hyp=-1)
        if len(X) >= 7:
            ref = o.pnp_solve(X, uv, seq["K"], o.make_pnp_params(pprm["H"], o.SAMPLER_PHILOX, pprm["seed"] + q, pprm["err"]))
        t = gt["tracks"][q]
        nc = len(X)
        assert t["n_corr"] == nc
        assert gt["corr_xyz"][q][:nc].tobytes() == X.tobytes() and gt["corr_uv"][q][:nc].tobytes() == uv.tobytes()
        assert bool(t["ok"]) == ref["ok"] and t["best_hyp"] == ref["best_hyp"]
        if ref["ok"]:
            n_ok += 1
            ni = len(ref["inliers"])
            assert t["n_inliers"] == ni and np.array_equal(gt["inlier_idx"][q][:ni], ref["inliers"])
            assert t["R"].tobytes() == ref["R"].tobytes() and t["t"].tobytes() == ref["t"].tobytes()
    assert n_ok >= F - 3


# ---- 5. the shim -------------------------------------------------------------------------------------------------------------------
def test_shim_one_pass_image_pair_equals_the_two_calls():
    shim = os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp")
    outs = {}
    for kind in ("one_pass", "two_calls"):
        exe = one_pass_exe(kind)
        deps = [SRC, shim, os.path.join(ROOT, "include", "mvslam_hip.h")]
        if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
            build_one_pass(kind)
        p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, p.stdout.decode()
        outs[kind] = p.stdout.decode().splitlines()
    assert outs["one_pass"][0] == "path five-point, one pass" and outs["two_calls"][0] == "path five-point, two calls"
    assert outs["one_pass"][1:] == outs["two_calls"][1:]
    body = outs["one_pass"][1:]
    assert body[0].startswith("pair 0 valid 1 ") and "pair 1 valid 0 inliers 0 points 0" in body
    assert "pair 2 valid 0 inliers 0 points 0" in body and sum(l.startswith("p ") for l in body) >= 100
