"""mvslam_amd/csrc/five_point.hpp compiled for the host (tests/cpp/five_point_host.cpp): the stand-alone program plain and under
ASan + UBSan, the solver against an independent numpy model on 2 000 generated samples, the semantics of the RANSAC stage on the
host model, the reference's cube, and the resource digest of the new kernels.  No GPU needed.

Bounds.  Reference against reference on this generator and seed: the numpy model in binary64 against
the same model in 50-digit mpmath differs by at most D_MODEL in a matched matrix (max-abs, matrices of Frobenius norm sqrt(2));
its matrices miss the constraints by at most R_MODEL (epipolar, det, trace).  The header is allowed ten times each."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import e5_model as em
import helpers
import oracle_lib as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N_SAMPLES = 20261018, 2000
D_MODEL = 2.0e-2                       # measured: 1.98e-2, the worst of the 2 000 samples (median 1.9e-13, 99 % below 2.4e-7)
R_MODEL = (7.5e-16, 5.8e-4, 2.4e-3)    # measured residuals of the numpy model: epipolar, |det E|, trace constraint
# the worst sample says little about the other 1 999: the same measurement's 99th percentile and median bound the bulk
D_MODEL_P99, D_MODEL_MEDIAN = 2.33e-7, 1.93e-13


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_five_point_host_program(tmp_path, sanitize):
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    exe = str(tmp_path / "five_point_host")
    subprocess.check_call(["g++", *em.HOST_FLAGS, *san, "-o", exe, em.SRC, "-lm"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "five_point samples=3006" in out and "bad=0" in out and "ERROR" not in out and "runtime error" not in out, out


def test_solver_against_the_numpy_model():
    rng = np.random.default_rng(SEED)
    skipped, worst, res, dists = 0, 0.0, np.zeros(3), []
    for s in range(N_SAMPLES):
        p1, p2, Et = em.random_sample(rng)
        ref, roots, shaky = em.model_five_point(p1, p2)
        if shaky:   # near a double root "the set of real roots" is ill-defined in binary64
            skipped += 1
            continue
        n, E = em.host_five_point(p1, p2)
        got = [E[r] for r in range(n)]
        assert np.isfinite(E).all() and not E[n:].any()
        assert len(got) == len(ref), (s, n, len(ref))
        d = em.match_sets(got, ref)
        worst = max(worst, d)
        dists.append(d)
        assert d <= 10 * D_MODEL, (s, d)
        assert min(np.abs(g - Et).max() for g in got) <= 10 * D_MODEL, s      # the true E is among them
        for g in got:
            res = np.maximum(res, em.constraint_residuals(g, p1, p2))
    print("skipped %d of %d; largest distance to the numpy model %.3e; residuals %s" % (skipped, N_SAMPLES, worst, res))
    assert skipped <= 0.05 * N_SAMPLES
    dists = np.array(dists)
    print("median %.3e, 99th percentile %.3e" % (np.median(dists), np.quantile(dists, 0.99)))
    assert np.quantile(dists, 0.99) <= 10 * D_MODEL_P99 and np.median(dists) <= 10 * D_MODEL_MEDIAN
    assert (res <= 10 * np.array(R_MODEL)).all(), res


def test_degenerate_inputs_give_no_model_or_finite_ones():
    k = np.arange(5.0)[:, None]
    rng = np.random.default_rng(3)
    same = rng.uniform(-0.5, 0.5, size=(5, 2))
    for p1, p2 in ((np.tile([0.25, -0.5], (5, 1)), np.tile([0.3, 0.1], (5, 1))),
                   (np.hstack([0.1 * k, 0.2 * k - 0.3]), np.hstack([0.1 * k + 0.05, 0.2 * k - 0.25])),
                   (same, same.copy())):
        n, E = em.host_five_point(p1, p2)
        assert 0 <= n <= 10 and np.isfinite(E).all()
    assert em.host_five_point(np.tile([0.25, -0.5], (5, 1)), np.tile([0.3, 0.1], (5, 1)))[0] == 0


def test_identity_sampler_is_matches_0_to_4_and_philox_is_the_8_point_stream():
    assert em.host_sample5(1, 2, 100, o.SAMPLER_IDENTITY) == [0, 1, 2, 3, 4]
    for h in (0, 1, 77):
        assert em.host_sample5(5, h, 300, o.SAMPLER_PHILOX) == o.sample8(5, h, 300, o.SAMPLER_PHILOX)[:5].tolist()


def _host_models(p1, p2, H, sampler, seed):
    out = []
    for h in range(H):
        idx = em.host_sample5(seed, h, len(p1), sampler)
        n, E = em.host_five_point(p1[idx], p2[idx])
        out.append([E[r] for r in range(n)])
    return out


def test_ransac_semantics_count_residual_and_tables():
    rng = np.random.default_rng(11)
    z = rng.uniform(2, 10, 60)
    X = np.stack([rng.uniform(-0.5, 0.5, 60) * z, rng.uniform(-0.5, 0.5, 60) * z, z], axis=1)
    p1, p2 = X[:, :2] / X[:, 2:], (X + [1.0, 0.1, 0.0])[:, :2] / X[:, 2:]
    p2 = p2 + rng.normal(scale=1e-4, size=p2.shape)
    p2[::4] = rng.uniform(-0.5, 0.5, size=(15, 2))
    for sampler, thr in ((o.SAMPLER_PHILOX, 1e-6), (o.SAMPLER_IDENTITY, 1e-3)):
        ref = em.host_ransac(p1, p2, thr, 40, sampler, 7)
        nr, cnt, win, best, res = em.select_models(_host_models(p1, p2, 40, sampler, 7), p1, p2, thr)
        assert np.array_equal(ref["n_roots"], nr) and np.array_equal(ref["count"], cnt)
        assert (cnt[np.arange(10)[None, :] >= nr[:, None]] == -1).all() and (cnt[np.arange(10)[None, :] < nr[:, None]] >= 0).all()
        assert (ref["best_hyp"], ref["best_root"]) == win and ref["best_count"] == best and ref["best_residual"] == res
        num, den = em.sampson_terms(ref["E"], p1, p2)
        assert np.array_equal(ref["mask"], ((den > 0) & (num <= thr * den)).astype(np.uint8))


def test_ransac_tie_order_on_constructed_ties():
    """identity sampler: every hypothesis draws matches 0 .. 4, so all H hypotheses hold the same models -- equal counts AND equal
    residuals: the smaller hypothesis id, then (among its models) count, residual and the smaller root index decide"""
    rng = np.random.default_rng(2)
    p1, p2, _ = em.random_sample(rng)
    p1, p2 = np.vstack([p1, p1[:3] + 0.01]), np.vstack([p2, p2[:3] + 0.013])
    ref = em.host_ransac(p1, p2, 1e-3, 6, o.SAMPLER_IDENTITY, 0)
    assert (ref["n_roots"] == ref["n_roots"][0]).all() and (ref["count"] == ref["count"][0]).all() and ref["best_hyp"] == 0
    nr, cnt, win, best, res = em.select_models(_host_models(p1, p2, 6, o.SAMPLER_IDENTITY, 0), p1, p2, 1e-3)
    assert win == (0, ref["best_root"]) and best == ref["best_count"] and res == ref["best_residual"]
    # count beats residual, residual beats hypothesis id, hypothesis id beats root index -- on hand-made models
    E0 = helpers.skew([1.0, 0, 0]) @ np.eye(3)
    q1 = rng.uniform(-0.5, 0.5, size=(12, 2))
    q2 = q1 + np.stack([rng.uniform(0.05, 0.2, 12), np.zeros(12)], axis=1)         # exact inliers of E0
    q2[0, 1] += 1e-3                                                                # ... one of them with a residual
    Eb = helpers.skew([1.0, 0.002, 0]) @ np.eye(3)                                  # slightly wrong: larger residual, same count
    worse = helpers.skew([0, 1.0, 0]) @ np.eye(3)                                   # few inliers
    models = [[worse, Eb], [Eb, E0], [E0, E0], [E0]]
    for select in (em.select_models, em.host_select):     # the numpy model, and the C++ host model the GPU tests compare with
        nr, cnt, win, best, res = select(models, q1, q2, 1e-4)
        assert cnt[1, 0] == cnt[1, 1] == cnt[2, 0] == best == 12 and cnt[0, 0] < 12
        assert win == (1, 1)      # Eb (0, 1) and (1, 0) come first but have the larger residual; (2, 0), (2, 1), (3, 0) tie with (1, 1)
        assert select([[worse], [E0, worse]], q1, q2, 1e-4)[2] == (1, 0)           # count beats hypothesis id
        assert select([[Eb, E0], [E0]], q1, q2, 1e-4)[2] == (0, 1)                  # residual beats root index
    a, b = em.select_models(models, q1, q2, 1e-4), em.host_select(models, q1, q2, 1e-4)
    assert np.array_equal(a[1], b[1]) and a[2:4] == b[2:4] and a[4] == b[4]         # the same counts, winner and residual bits


def test_cube_default_threshold_the_true_model_wins():
    """the reference's sfm_solve_cube (test/test-sfm.cpp:17-90): K = I, default threshold 5e-2, where many wrong models reach all
    eight points -- the residual tie-break has to pick the true one"""
    rig = helpers.two_camera_rig("cube")
    ref = em.host_ransac(rig["uv1"], rig["uv2"], 5e-2, 64, o.SAMPLER_PHILOX, 0)
    assert ref["best_count"] == 8 and (ref["count"] == 8).sum() > 1
    Etrue = em.normalise(helpers.skew(rig["T1to2"][1]) @ rig["T1to2"][0])
    assert np.abs(ref["E"] - Etrue).max() < 1e-9
    ok, R, t, pts, idx = o.recover_pose_and_points(ref["E"], rig["uv1"], rig["uv2"], ref["mask"])
    R21, t21 = o.se3_inverse(R, t)
    assert ok and idx.tolist() == list(range(8))
    assert np.abs(o.se3_ln(R21, t21) - np.array([1, 0, 0, 0, 0, 0.0])).max() < 1e-3
    assert np.abs(pts - rig["X"]).max() < 1e-3


def _constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, name
    return int(m.group(1))


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """the stage's kernels are exactly these four (no second text of one of them under another name), and what each may use"""
    path = os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")
    if not os.path.exists(path):
        pytest.fail("kernel_resources.json is missing: build the library first")
    digest = json.load(open(path))
    assert not [k for k in digest if re.search(r"e5(_|wide)", k)]
    mine = {}
    for k, v in digest.items():
        if "essential5" in k or "five_point_kernel" in k:
            m = re.match(r"_ZN3mvs(\d+)", k)                  # mvs::<name>(...), Itanium mangling
            assert m, k
            mine[k[m.end():m.end() + int(m.group(1))]] = v
    assert sorted(mine) == ["essential5_horizon_kernel", "essential5_select_kernel", "essential5_solve_count_kernel",
                            "five_point_kernel"], list(mine)
    for k, v in mine.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0, (k, v)
    v = mine["essential5_horizon_kernel"]
    assert v["sgpr_spills"] == 0 and v["static_lds_bytes"] == 0, v
    # solve + count: dynamic LDS as essential5.hip sizes it -- the solver's workspace of 64 lanes + [4 wavefronts][10 roots]
    # [64 lanes] int32 -- beside its static LDS in the 160 KB of a CU
    v = mine["essential5_solve_count_kernel"]
    assert v["sgpr_spills"] == 0, v
    csrc = os.path.join(ROOT, "mvslam_amd", "csrc")
    hdr = open(os.path.join(csrc, "five_point.hpp")).read() + open(os.path.join(csrc, "kernels.hpp")).read()
    src = open(os.path.join(csrc, "essential5.hip")).read()
    ws, roots, lanes = _constant(hdr, "kE5Ws"), _constant(hdr, "kE5MaxRoots"), _constant(hdr, "kE5HypPerBlock")
    dynamic = ws * lanes * 8 + _constant(src, "kE5Waves") * roots * lanes * 4
    assert dynamic == 141312 + 10240
    assert v["static_lds_bytes"] + dynamic <= 163840, (v, dynamic)
