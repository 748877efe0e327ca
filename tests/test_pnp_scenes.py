"""pnp_solve off the frontal scene of test_pnp.py: points behind the camera (the zc > 0 conjunct of the inlier test), total
and partial ties of the arg-best rule (most inliers, then the smaller hypothesis id), power-of-two scalings of the world, and
wide scenes (large rotations, camera inside the cloud, depths 0.2 to 50, off-centre principal point).

Every family has a CPU half on the oracle and a GPU half: the device equals the oracle byte for byte (ok, best_hyp, inliers,
the bytes of R and t) and shows the family's own property.  Bounds on the distance to the truth are 4x the worst distance
of the ORACLE over the scenes of this file (measured on the CPU, figures beside the constants); nothing is derived from the
device's output, which is held to byte equality."""
import numpy as np
import pytest

import oracle_lib as o
from test_pnp import _scene

CHUNK = 768                                   # kPnpChunk (pnp.hip): the point stream goes through LDS in chunks of 768 rows
K_FRONTAL = np.array([[525.0, 0, 320], [0, 525, 240], [0, 0, 1]])
K_WIDE = np.array([[610.0, 0, 140], [0, 590, 390], [0, 0, 1]])   # 640 x 480 image, principal point well off centre


# ------------------------------------------------------------------------------------------- shared helpers
# The generators of this file use + - * / and numpy's elementwise sqrt only (no sin / cos / exp, no BLAS product), so a scene is
# the same bytes on every machine and the distances measured below do not depend on a maths library.
def _rotation(v):
    """Cayley form of the rotation about v by 2 atan|v|: I + 2 (S + S^2) / (1 + |v|^2), S = [v]x"""
    S = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    S2 = np.array([[sum(S[i, k] * S[k, j] for k in range(3)) for j in range(3)] for i in range(3)])
    return np.eye(3) + 2.0 * (S + S2) / (1.0 + (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def _rows(R, X):
    """R x for every row x of X"""
    return X[:, 0:1] * R[:, 0] + X[:, 1:2] * R[:, 1] + X[:, 2:3] * R[:, 2]


def _project(K, R, t, X):
    """pixels and camera coordinates of world points (no cheirality assert: points may lie behind the camera)"""
    Xc = _rows(R, X) + t
    uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], axis=1)
    return uv, Xc


def _pose_err(res, R, t):
    """(max|R - R_true|, max|t - t_true| / |t_true|) of the returned camera-in-world pose against the truth (R, t: world -> camera)"""
    Rc, tc = R.T, -_rows(R.T, t[None])[0]
    return float(np.abs(res["R"] - Rc).max()), float(np.abs(res["t"] - tc).max() / np.sqrt((tc * tc).sum()))


def _assert_same_bytes(got, ref, what=""):
    assert got["ok"] == ref["ok"] and got["best_hyp"] == ref["best_hyp"], (what, got["ok"], ref["ok"], got["best_hyp"], ref["best_hyp"])
    assert np.array_equal(got["inliers"], ref["inliers"]), what
    assert got["R"].tobytes() == ref["R"].tobytes() and got["t"].tobytes() == ref["t"].tobytes(), what


def _oracle(X, uv, K, H, sampler, seed):
    return o.pnp_solve(X, uv, K, o.make_pnp_params(H, sampler, seed))


def _device(ctx, X, uv, K, H, sampler, seed):
    from mvslam_amd import capi

    return ctx.pnp_solve(X, uv, K, capi.default_pnp_params(num_hypotheses=H, sampler=sampler, seed=seed, refit=0))


_cache = {}


def _cached(key, fn):
    """scenes and oracle results are computed once and shared by the CPU and the GPU half (nothing writes to them)"""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# =========================================================================================== A. points behind the camera
def _planted_positions(n, nb):
    """nb rows of n: a block at the start, one in the middle, one at the end and, where the list is longer than one LDS chunk,
    one astride row 768; blocks that overlap are made up for by rows spread evenly over the rest of the list"""
    anchors = [0, n // 2, n] + ([CHUNK] if n > CHUNK else [])
    sz = nb // len(anchors)
    pos = set()
    for a in anchors:
        lo = min(max(a - sz // 2, 0), n - sz)
        pos.update(range(lo, lo + sz))
    need = nb - len(pos)
    if need > 0:
        rest = [i for i in range(n) if i not in pos]
        pos.update(rest[::len(rest) // need][:need])
    pos = np.array(sorted(pos))
    assert len(pos) == nb
    return pos


def _behind_scene(seed, n0, nb, noise_px):
    """n0 true correspondences of a frontal pose, 15 % of them with a uniform wrong pixel, and nb planted rows: for a true
    point with camera coordinates Xc the world point R^T (-k Xc - t), k in {0.5, 1, 3}, paired with that point's pixel.  It
    lies BEHIND the camera on the line through the pixel, so lhs <= rhs holds for it under the true pose and only zc > 0 keeps
    it out.  returns K, X, uv, R, t, planted rows, wrong rows, good rows"""
    rng = np.random.default_rng(seed)
    K = K_FRONTAL
    R = _rotation(rng.normal(size=3) * 0.04)                          # about 0.08 rad, as the frontal scenes of test_pnp.py
    t = np.array([0.2, -0.1, 0.3]) + rng.normal(size=3) * 0.05
    X0 = np.stack([rng.uniform(-2, 2, n0), rng.uniform(-1.5, 1.5, n0), rng.uniform(4, 9, n0)], axis=1)
    uv0, Xc0 = _project(K, R, t, X0)
    uv0 = uv0 + rng.normal(scale=noise_px, size=(n0, 2)) if noise_px > 0 else uv0
    n_wrong = (15 * n0) // 100
    wrong0 = np.sort(rng.choice(n0, size=n_wrong, replace=False))
    good0 = np.setdiff1d(np.arange(n0), wrong0)
    src = good0[(np.arange(nb) * 7) % len(good0)]                      # planted row j mirrors true point src[j] ...
    k = np.array([0.5, 1.0, 3.0])[np.arange(nb) % 3]                   # ... at -k Xc
    Xp = _rows(R.T, -k[:, None] * Xc0[src] - t)                        # R^T (-k Xc - t)
    uvp = uv0[src].copy()                                              # the pixel as observed (before wrong0 is overwritten)
    uv0[wrong0] = np.stack([rng.uniform(0, 640, n_wrong), rng.uniform(0, 480, n_wrong)], axis=1)
    n = n0 + nb
    planted = _planted_positions(n, nb)
    true_rows = np.setdiff1d(np.arange(n), planted)
    X, uv = np.empty((n, 3)), np.empty((n, 2))
    X[planted], uv[planted] = Xp, uvp
    X[true_rows], uv[true_rows] = X0, uv0
    return K, X, uv, R, t, planted, true_rows[wrong0], true_rows[good0]


# n0, nb, H: one group of hypotheses and 4 point parts; 2 groups; 3 groups and a list that crosses the chunk boundary; more
# planted rows than any single outlier class
BEHIND_CASES = [(40, 20, 64), (300, 150, 100), (700, 200, 129), (900, 600, 300)]
BEHIND_NOISE = [0.0, 0.01]
# Distance of the oracle's RANSAC pose (no refit) to the truth over the 4 scenes of each noise level, measured on the CPU:
#   noise 0     max|R - R_true| = 6.240e-12 (n0 = 700)   max|t - t_true| / |t_true| = 1.350e-10 (n0 = 700)
#   noise 0.01  max|R - R_true| = 6.798e-05 (n0 = 40)    max|t - t_true| / |t_true| = 1.110e-03 (n0 = 900)
# (at noise 0 the other three scenes are at 1e-13 and below: the figure is the conditioning of one winning sample.)
# The bound is 4x that worst value: the pose comes from one minimal sample and moves with the seed, a wrong pose is off by 0.1.
BEHIND_BOUND = {0.0: (4 * 6.240e-12, 4 * 1.350e-10), 0.01: (4 * 6.798e-05, 4 * 1.110e-03)}


def _behind(n0, nb, H, noise):
    def make():
        sc = _behind_scene(1000 + n0 + H, n0, nb, noise)
        return sc, _oracle(sc[1], sc[2], sc[0], H, o.SAMPLER_PHILOX, n0 * 1000 + 1)

    return _cached(("behind", n0, nb, H, noise), make)


def _check_behind(res, sc, noise):
    K, X, uv, R, t, planted, wrong, good = sc
    assert res["ok"]
    inl = set(res["inliers"].tolist())
    assert not inl & set(planted.tolist()), sorted(inl & set(planted.tolist()))    # zc > 0: none of the planted rows
    assert not inl & set(wrong.tolist())
    if noise == 0.0:
        assert set(good.tolist()) <= inl                                           # every true noise-free row
    eR, et = _pose_err(res, R, t)
    print("behind n=%d noise=%g: |dR| = %.3e  |dt|/|t| = %.3e" % (len(X), noise, eR, et))
    assert eR <= BEHIND_BOUND[noise][0] and et <= BEHIND_BOUND[noise][1], (eR, et)


def test_planted_positions_meet_every_part_and_both_sides_of_the_chunk_boundary():
    for n0, nb, H in BEHIND_CASES:
        n = n0 + nb
        pos = _planted_positions(n, nb)
        assert len(set(pos.tolist())) == nb and pos.min() == 0 and pos.max() == n - 1 and n // 2 in pos
        assert set((pos % 4).tolist()) == {0, 1, 2, 3} and set((pos % 2).tolist()) == {0, 1}   # every wavefront "part"
        if n > CHUNK:
            assert CHUNK - 1 in pos and CHUNK in pos
            assert set((pos[pos >= CHUNK] - CHUNK) % 4) == {0, 1, 2, 3}
    assert sum(n0 + nb > CHUNK for n0, nb, H in BEHIND_CASES) >= 2


@pytest.mark.parametrize("noise", BEHIND_NOISE)
@pytest.mark.parametrize("n0,nb,H", BEHIND_CASES)
def test_oracle_pnp_rejects_points_behind_the_camera(n0, nb, H, noise):
    sc, ref = _behind(n0, nb, H, noise)
    # the planted rows do satisfy the division-free test under the true pose: only the sign of zc tells them apart
    K, X, uv, R, t, planted, wrong, good = sc
    uvp, Xc = _project(K, R, t, X[planted])
    assert (Xc[:, 2] < 0).all() and np.abs(uvp - uv[planted]).max() < (1e-9 if noise == 0.0 else 0.05)
    _check_behind(ref, sc, noise)


@pytest.mark.gpu
@pytest.mark.parametrize("noise", BEHIND_NOISE)
@pytest.mark.parametrize("n0,nb,H", BEHIND_CASES)
def test_gpu_pnp_rejects_points_behind_the_camera(ctx, n0, nb, H, noise):
    from mvslam_amd import capi

    sc, ref = _behind(n0, nb, H, noise)
    got = _device(ctx, sc[1], sc[2], sc[0], H, capi.SAMPLER_PHILOX, n0 * 1000 + 1)
    _assert_same_bytes(got, ref)
    _check_behind(got, sc, noise)


def _behind_sample_scene(seed, member, k):
    """a noise-free frontal scene whose row `member` (of the identity sampler's rows 0 to 3) is a planted point at -k Xc"""
    K, X, uv, R, t, bad = _scene(seed, 40, 0.0, 0)
    X = X.copy()
    X[member] = _rows(R.T, -k * (_rows(R, X[member:member + 1]) + t) - t)[0]
    return K, X, uv


@pytest.mark.gpu
@pytest.mark.parametrize("member", [3, 0])
def test_gpu_pnp_planted_point_in_the_sample_matches_oracle(ctx, member):
    """A point behind the camera as the disambiguating 4th member of the sample (zc < 0 under every candidate, yet
    rhs = thr^2 zc^2 > 0 lets it vote: `rhs > 0.0` in p3p_select stays as it is) and as member 0 (a wrong triangle).
    Whatever the oracle answers, a model or none, the device answers the same bytes."""
    from mvslam_amd import capi

    answers = set()
    for seed in (11, 12, 13):
        for k in (0.5, 1.0, 3.0):
            K, X, uv = _behind_sample_scene(seed, member, k)
            for H in (1, 64):
                ref = _oracle(X, uv, K, H, o.SAMPLER_IDENTITY, 0)
                got = _device(ctx, X, uv, K, H, capi.SAMPLER_IDENTITY, 0)
                _assert_same_bytes(got, ref, (seed, k, H))
                answers.add(ref["ok"])
    print("planted sample member %d: oracle answers %s" % (member, sorted(answers)))


def test_oracle_pnp_planted_fourth_point_still_selects_the_true_pose():
    """member 3 behind the camera: the three triangle rows are true, and the planted row projects onto its pixel under the true
    pose, so the true pose is selected and every other row is an inlier; the planted row itself is not"""
    for seed in (11, 12, 13):
        for k in (0.5, 1.0, 3.0):
            K, X, uv = _behind_sample_scene(seed, 3, k)
            ref = _oracle(X, uv, K, 1, o.SAMPLER_IDENTITY, 0)
            assert ref["ok"] and ref["inliers"].tolist() == [i for i in range(40) if i != 3], (seed, k)


# =========================================================================================== B. ties
TIE_H = [1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 512, 1000]
TIE_N = [7, 300, 769]


def _tie_scene(n):
    """a noisy frontal scene with wrong matches whose rows 0 to 3 (the identity sampler's sample) are true correspondences"""
    K, X, uv, R, t, bad = _scene(300 + n, n, 0.01, 0 if n == 7 else n // 5)
    good = np.setdiff1d(np.arange(n), bad)[:4]
    perm = np.concatenate([good, np.setdiff1d(np.arange(n), good)])
    return K, X[perm].copy(), uv[perm].copy()


def _no_model_scene(n):
    """rows 0 to 3 are wrong matches for which P3P has no solution (the oracle reports no model: asserted in the CPU half)"""
    rng = np.random.default_rng(NO_MODEL_SEED[n])
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 9, n)], axis=1)
    uv = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], axis=1)
    return K_FRONTAL, X, uv


# first seed 0, 1, 2, ... of _no_model_scene for which the oracle's identity-sampler hypothesis has no solution
NO_MODEL_SEED = {7: 1, 300: 17, 769: 3}


def _tie_refs(n):
    def make():
        K, X, uv = _tie_scene(n)
        return (K, X, uv), {H: _oracle(X, uv, K, H, o.SAMPLER_IDENTITY, 0) for H in TIE_H}

    return _cached(("tie", n), make)


def _no_model_refs(n):
    def make():
        K, X, uv = _no_model_scene(n)
        return (K, X, uv), {H: _oracle(X, uv, K, H, o.SAMPLER_IDENTITY, 0) for H in TIE_H}

    return _cached(("nomodel", n), make)


@pytest.mark.parametrize("n", TIE_N)
def test_oracle_pnp_total_tie_keeps_hypothesis_0(n):
    (K, X, uv), refs = _tie_refs(n)
    one = refs[1]
    assert one["ok"] and one["best_hyp"] == 0 and len(one["inliers"]) >= 4
    for H in TIE_H:
        assert refs[H]["best_hyp"] == 0
        _assert_same_bytes(refs[H], one, H)


@pytest.mark.gpu
@pytest.mark.parametrize("n", TIE_N)
def test_gpu_pnp_total_tie_keeps_hypothesis_0(ctx, n):
    """identity sampler: all H hypotheses hold the same model and the same count, across lanes, wavefronts, point parts, groups
    and workgroups; the answer is hypothesis 0 and the bytes of H = 1"""
    from mvslam_amd import capi

    (K, X, uv), refs = _tie_refs(n)
    one = _device(ctx, X, uv, K, 1, capi.SAMPLER_IDENTITY, 0)
    for H in TIE_H:
        got = _device(ctx, X, uv, K, H, capi.SAMPLER_IDENTITY, 0)
        assert got["ok"] and got["best_hyp"] == 0, H
        _assert_same_bytes(got, one, H)
        _assert_same_bytes(got, refs[H], H)


@pytest.mark.parametrize("n", TIE_N)
def test_oracle_pnp_no_model_for_any_hypothesis_count(n):
    (K, X, uv), refs = _no_model_refs(n)
    for H in TIE_H:
        assert not refs[H]["ok"] and refs[H]["best_hyp"] == -1 and len(refs[H]["inliers"]) == 0, H


@pytest.mark.gpu
@pytest.mark.parametrize("n", TIE_N)
def test_gpu_pnp_no_model_for_any_hypothesis_count(ctx, n):
    """every hypothesis of every workgroup is without a model (count -1): none of them may win"""
    from mvslam_amd import capi

    (K, X, uv), refs = _no_model_refs(n)
    for H in TIE_H:
        got = _device(ctx, X, uv, K, H, capi.SAMPLER_IDENTITY, 0)
        assert not got["ok"] and got["best_hyp"] == -1, H
        _assert_same_bytes(got, refs[H], H)


# Philox: hypotheses h_a < h_b with identical samples.  (h_a, h_b): two lanes of one wavefront, two wavefronts of one block
# (hypothesis groups 0 and 1; 0 and 3), two blocks (0 and 1; 0 and 2); H = 600 makes three workgroups of 4, 4 and 2 groups
PAIR_TIES = [(5, 9), (5, 70), (60, 200), (5, 260), (130, 530)]
PAIR_H, PAIR_N, PAIR_SEED = 600, 400, 77


def _pair_tie_scene(h_a, h_b):
    """rows with 0.03 px noise and wrong matches; the four rows h_a draws are made exact (its model is the truth and collects
    every row within 0.05 px of it, which no model of a noisy sample does) and copied onto the four rows h_b draws"""
    K, X, uv, R, t, bad = _scene(900 + h_a + h_b, PAIR_N, 0.03, 80)
    X, uv = X.copy(), uv.copy()
    ia, ib = o.sample4(PAIR_SEED, h_a, PAIR_N), o.sample4(PAIR_SEED, h_b, PAIR_N)
    assert not set(ia.tolist()) & set(ib.tolist())
    uv[ia] = _project(K, R, t, X[ia])[0]
    X[ib], uv[ib] = X[ia], uv[ia]
    return K, X, uv, ia, ib


def _pair_tie(h_a, h_b):
    def make():
        K, X, uv, ia, ib = _pair_tie_scene(h_a, h_b)
        return (K, X, uv, ia, ib), _oracle(X, uv, K, PAIR_H, o.SAMPLER_PHILOX, PAIR_SEED)

    return _cached(("pair", h_a, h_b), make)


@pytest.mark.parametrize("h_a,h_b", PAIR_TIES)
def test_oracle_pnp_partial_tie_keeps_the_smaller_id(h_a, h_b):
    (K, X, uv, ia, ib), ref = _pair_tie(h_a, h_b)
    assert X[ia].tobytes() == X[ib].tobytes() and uv[ia].tobytes() == uv[ib].tobytes()   # same sample: same model, same count
    assert ref["ok"] and ref["best_hyp"] == h_a                                            # and that count is the maximum
    # h_b wins on its own count, not through h_a: with one row of h_a's sample moved 50 px away (every other model loses
    # at most that one row) the winner is h_b
    uv2 = uv.copy()
    uv2[ia[0]] += 50.0
    alone = _oracle(X, uv2, K, PAIR_H, o.SAMPLER_PHILOX, PAIR_SEED)
    assert alone["best_hyp"] == h_b


@pytest.mark.gpu
@pytest.mark.parametrize("h_a,h_b", PAIR_TIES)
def test_gpu_pnp_partial_tie_keeps_the_smaller_id(ctx, h_a, h_b):
    from mvslam_amd import capi

    (K, X, uv, ia, ib), ref = _pair_tie(h_a, h_b)
    got = _device(ctx, X, uv, K, PAIR_H, capi.SAMPLER_PHILOX, PAIR_SEED)
    assert got["best_hyp"] == h_a
    _assert_same_bytes(got, ref)


# =========================================================================================== C. power-of-two world scale
SCALES = [2.0 ** -10, 2.0 ** 10, 2.0 ** -30, 2.0 ** 30]
SCALE_SCENES = [21, 22, 23]
SCALE_N, SCALE_H = 300, 257


def _scaled(seed):
    def make():
        K, X, uv, R, t, bad = _scene(seed, SCALE_N, 0.01, 60)
        base = _oracle(X, uv, K, SCALE_H, o.SAMPLER_PHILOX, seed)
        return (K, X, uv, R, t, bad), base, {s: _oracle(s * X, uv, K, SCALE_H, o.SAMPLER_PHILOX, seed) for s in SCALES}

    return _cached(("scale", seed), make)


def _assert_covariant(scaled, base, s):
    """the result for (s X, uv, K) against the one for (X, uv, K): same decisions, same rotation, translation times s, exactly"""
    assert scaled["ok"] == base["ok"] and scaled["best_hyp"] == base["best_hyp"], s
    assert np.array_equal(scaled["inliers"], base["inliers"]), s
    assert scaled["R"].tobytes() == base["R"].tobytes(), s
    assert scaled["t"].tobytes() == (s * base["t"]).tobytes(), s


@pytest.mark.parametrize("seed", SCALE_SCENES)
def test_oracle_pnp_is_covariant_under_power_of_two_world_scale(seed):
    """The solver is built from ratios of squared side lengths, a quartic in dimensionless coefficients and a homogeneous
    inlier test, so a power-of-two scaling of the world only shifts exponents.  That holds for the world-to-camera pose
    (Rw2c, tw2c) and, since so3_rectify acts on R alone and the inversion is linear in t, for the returned camera-in-world
    pose as well: the oracle is byte-covariant for all four scales on all three scenes (no weaker form was needed)."""
    (K, X, uv, R, t, bad), base, scaled = _scaled(seed)
    assert base["ok"] and not set(base["inliers"].tolist()) & set(bad.tolist())
    for s in SCALES:
        _assert_covariant(scaled[s], base, s)
        assert scaled[s]["Rw2c"].tobytes() == base["Rw2c"].tobytes(), s
        assert scaled[s]["tw2c"].tobytes() == (s * base["tw2c"]).tobytes(), s


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SCALE_SCENES)
def test_gpu_pnp_is_covariant_under_power_of_two_world_scale(ctx, seed):
    from mvslam_amd import capi

    (K, X, uv, R, t, bad), base, scaled = _scaled(seed)
    got0 = _device(ctx, X, uv, K, SCALE_H, capi.SAMPLER_PHILOX, seed)
    _assert_same_bytes(got0, base)
    for s in SCALES:
        got = _device(ctx, s * X, uv, K, SCALE_H, capi.SAMPLER_PHILOX, seed)
        _assert_covariant(got, got0, s)
        _assert_same_bytes(got, scaled[s], s)


# =========================================================================================== D. wide scenes
def _wide_scene(seed, n, noise_px):
    """A rotation of up to 3 rad about a random axis, a camera inside the cloud (each point is in front of or behind it with
    probability 1/2), depths |zc| from 0.2 to 50 (0.2 + 49.8 w^3: a third of them below 2), an off-centre principal point.
    A point in front is seen inside the 640 x 480 image; a point behind gets a random pixel and is listed as an outlier.
    returns K, X, uv, R, t, outlier rows"""
    rng = np.random.default_rng(seed)
    K = K_WIDE
    axis = rng.normal(size=3)
    axis = axis / np.sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2])
    w = rng.uniform()
    R = _rotation(axis * (14.1 * (w * w * w)))                         # 2 atan(14.1) = 3.0 rad; the cube spreads the angles
    t = rng.normal(size=3) * 5.0
    w = rng.uniform(size=n)
    z = (0.2 + 49.8 * (w * w * w)) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    u, v = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    Xc = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], axis=1)
    X = _rows(R.T, Xc - t)                                              # R^T (Xc - t)
    uv = _project(K, R, t, X)[0]
    uv = uv + rng.normal(scale=noise_px, size=(n, 2)) if noise_px > 0 else uv
    behind = np.nonzero(z < 0)[0]
    uv[behind] = np.stack([rng.uniform(0, 640, len(behind)), rng.uniform(0, 480, len(behind))], axis=1)
    return K, X, uv, R, t, behind


WIDE_SEEDS = [0, 1, 2, 3]
WIDE_N, WIDE_H, WIDE_NOISE = [60, 800], 500, [0.0, 0.01]
# Distance of the oracle's RANSAC pose (no refit) to the truth over the 8 scenes of each noise level, measured on the CPU:
#   noise 0     max|R - R_true| = 2.328e-13 (seed 2, n = 60)   max|t - t_true| / |t_true| = 8.155e-13 (seed 2, n = 60)
#   noise 0.01  max|R - R_true| = 6.247e-05 (seed 1, n = 60)   max|t - t_true| / |t_true| = 4.905e-06 (seed 1, n = 60)
# (|t_true| is the distance of the camera centre from the world origin: several units here, about 0.4 in family A.)
# The bound is 4x that worst value (see BEHIND_BOUND).  At noise 0 the figure is the rounding error of one sample times its
# conditioning: with the depths drawn through pow() instead of w * w * w, a last-bit change of the scene, seed 2 / n = 60 gave
# 3.3e-14 instead of 2.3e-13.  Hence generators whose bytes do not depend on a maths library.
WIDE_BOUND = {0.0: (4 * 2.328e-13, 4 * 8.155e-13), 0.01: (4 * 6.247e-05, 4 * 4.905e-06)}


def _wide(seed, n, noise):
    def make():
        sc = _wide_scene(seed, n, noise)
        return sc, _oracle(sc[1], sc[2], sc[0], WIDE_H, o.SAMPLER_PHILOX, seed)

    return _cached(("wide", seed, n, noise), make)


@pytest.mark.parametrize("noise", WIDE_NOISE)
@pytest.mark.parametrize("n", WIDE_N)
@pytest.mark.parametrize("seed", WIDE_SEEDS)
def test_oracle_pnp_recovers_wide_scenes(seed, n, noise):
    """Seeds 0, 1, 2, ... in order, the first four for which the oracle recovers the truth at both sizes and both noise
    levels.  Skipped seeds: none."""
    (K, X, uv, R, t, behind), ref = _wide(seed, n, noise)
    assert 0.3 * n < len(behind) < 0.7 * n
    assert ref["ok"] and not set(ref["inliers"].tolist()) & set(behind.tolist())
    if noise == 0.0:
        assert len(ref["inliers"]) == n - len(behind)
    eR, et = _pose_err(ref, R, t)
    print("wide seed=%d n=%d noise=%g: |dR| = %.3e  |dt|/|t| = %.3e" % (seed, n, noise, eR, et))
    assert eR <= WIDE_BOUND[noise][0] and et <= WIDE_BOUND[noise][1], (eR, et)


@pytest.mark.gpu
@pytest.mark.parametrize("noise", WIDE_NOISE)
@pytest.mark.parametrize("n", WIDE_N)
@pytest.mark.parametrize("seed", WIDE_SEEDS)
def test_gpu_pnp_wide_scenes_match_oracle(ctx, seed, n, noise):
    from mvslam_amd import capi

    (K, X, uv, R, t, behind), ref = _wide(seed, n, noise)
    got = _device(ctx, X, uv, K, WIDE_H, capi.SAMPLER_PHILOX, seed)
    _assert_same_bytes(got, ref)
