"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same inputs.

Bar (BASELINE.json north_star): inlier indices / match lists / hypothesis tables BIT-EXACT;
pose and points within 1e-4 relative.  Because oracle and kernels implement the same arithmetic
contract, floating-point outputs are in fact expected to be bit-identical; the tests assert the
contractual 1e-4 and additionally the much tighter TIGHT bound so any drift is caught early.
"""
import numpy as np
import pytest

import helpers
import oracle_lib as o
from mvslam_amd import capi, synth

pytestmark = pytest.mark.gpu

REL_TOL, TIGHT = helpers.REL_TOL, helpers.TIGHT
_run_batch, _check_batch_against_oracle = helpers.run_batch, helpers.check_batch_against_oracle
_check_two_view = helpers.check_two_view


def _rand_desc(rng, n, nbytes=32):
    return rng.integers(0, 256, size=(n, nbytes), dtype=np.uint8)


# ----------------------------------------------------------------------------- matcher
@pytest.mark.parametrize("n_train,n_query,nbytes", [(2, 1, 32), (63, 65, 32), (500, 500, 32), (2000, 2000, 32),
                                                     (257, 130, 16), (300, 301, 64)])
def test_match_random_bit_exact(ctx, n_train, n_query, nbytes):
    rng = np.random.default_rng(n_train * 7919 + n_query)
    train, query = _rand_desc(rng, n_train, nbytes), _rand_desc(rng, n_query, nbytes)
    # plant true matches so that the ratio test passes for some queries
    k = min(n_train, n_query) // 2
    for i in range(k):
        query[i] = train[(i * 3) % n_train]
        query[i, rng.integers(0, nbytes)] ^= np.uint8(1 << rng.integers(0, 8))
    for ratio, max_dist in ((0.7, -1.0), (0.7, 10.0), (0.95, 200.0)):
        ref = o.match_visual_features(train, query, ratio, max_dist)
        got = ctx.match_hamming(train, query, ratio, max_dist)
        assert len(got) == len(ref)
        assert got.tobytes() == ref.tobytes()


def test_match_matrix_core_kernel_batch_bit_exact(ctx):
    """The int8-GEMM matcher (match_mfma_kernel) serves 256-bit descriptors once a batch has enough workgroups for it
    (>= 512: two per CU); the single-shot tests above run the vector kernel.  A batch of 64 ragged pairs (64 x 8 = 512
    workgroups): random descriptors with planted near-duplicates, exact duplicates in the train set (ties: the smaller
    train index must win), distances at the ratio boundary -- match lists byte-identical to the oracle for every pair.
    Round 5: with a distance limit the kernel only inserts keys below a cap C (smallest C with ratio * C > max_dist) --
    planted (d0, d1) partner pairs sit on every side of C and of max_dist, and the batch runs under five (ratio, max_dist)
    settings: the reference's (0.7, 10), no limit (the uncapped kernel), a wide limit (C = 92: random rows get close),
    a tight one, and zero."""
    rng = np.random.default_rng(4242)
    P, N = 64, 2000
    n1 = rng.integers(2, N + 1, size=P).astype(np.int32)
    n2 = rng.integers(1, N + 1, size=P).astype(np.int32)
    n1[:4] = [N, 2, 33, 257]
    n2[:4] = [N, N, 31, 1]
    d1 = rng.integers(0, 256, size=(P, N, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, size=(P, N, 32), dtype=np.uint8)
    for p in range(P):
        k = int(min(n1[p], n2[p])) // 2
        src = (np.arange(k) * 3) % n1[p]
        d2[p, :k] = d1[p, src]
        flips = rng.integers(0, 4, size=k)                       # 0 .. 3 flipped bits: distances 0 .. 3, many ties
        for j in range(k):
            for _ in range(flips[j]):
                d2[p, j, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        if n1[p] > 50:
            d1[p, 40] = d1[p, 3]                                  # duplicate train rows
            d1[p, 17] = d1[p, 3]
    # two partners at exact distances (fa, fb) from a query: a fresh row with fa / fb DISJOINT flipped bits
    combos = [(10, 14), (10, 15), (10, 16), (11, 15), (11, 16), (9, 13), (7, 10), (7, 11), (10, 10), (0, 1), (14, 15), (15, 16),
              (10, 100), (3, 4), (3, 5), (2, 4), (64, 91), (64, 92), (64, 93), (63, 90), (65, 93), (40, 57), (40, 58), (0, 0),
              (1, 1), (44, 63), (45, 64)]
    planted = 0
    for p in range(P):
        if n1[p] < 700 or n2[p] < 700:
            continue
        for i, (fa, fb) in enumerate(combos):
            row = rng.integers(0, 256, size=32, dtype=np.uint8)
            bits = rng.permutation(256)[:fa + fb]
            ra, rb = row.copy(), row.copy()
            for bit in bits[:fa]:
                ra[bit >> 3] ^= np.uint8(1 << (bit & 7))
            for bit in bits[fa:]:
                rb[bit >> 3] ^= np.uint8(1 << (bit & 7))
            # the nearer partner sometimes at the higher train index, in different 32-row tiles and lane halves
            ia, ib = 500 + 5 * i, 503 + 5 * i + 37 * (i % 3)
            if i % 2:
                ia, ib = ib, ia
            d1[p, ia], d1[p, ib], d2[p, 600 + i] = ra, rb, row
            planted += 1
    assert planted > 500
    kp = np.zeros((P, N, 2), dtype=np.float32)
    kp[..., 0] = rng.uniform(0, 640, size=(P, N))
    kp[..., 1] = rng.uniform(0, 480, size=(P, N))
    K = np.tile(synth.K_DEFAULT.reshape(1, 9), (P, 1))
    b = capi.Batch(ctx, P, N, 32)
    b.upload(0, d1, kp, n1, d2, kp, n2, K, np.arange(P, dtype=np.int64))
    for ratio, max_dist in ((0.7, 10.0), (0.7, -1.0), (0.7, 64.0), (0.9, 3.0), (0.7, 0.0)):
        prm = capi.default_params(num_hypotheses=64, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-2, ratio=ratio,
                                  max_dist=max_dist)
        b.run(prm)
        b.sync()
        out = b.download(mask=False, points=False)
        total = 0
        for p in range(P):
            ref = o.match_visual_features(d1[p, :n1[p]], d2[p, :n2[p]], ratio, max_dist)
            m = int(out["results"][p]["n_matches"])
            assert m == len(ref), (ratio, max_dist, p, m, len(ref))
            assert out["matches"][p][:m].tobytes() == ref.tobytes(), (ratio, max_dist, p)
            total += m
        assert total > 1000, (ratio, max_dist, total)
    b.close()


def test_match_ties_canonical_order(ctx):
    """Constructed ties: equal distances must resolve to the smaller train index; equal-distance matches are
    ordered by queryIdx (SURVEY 8(c) KAT 5)."""
    rng = np.random.default_rng(5)
    train = _rand_desc(rng, 64)
    train[10] = train[3]          # duplicate rows: query == train[3] ties at distance 0 with index 10
    train[40] = train[3]
    query = np.stack([train[3], train[20], train[3], train[21]])
    ref = o.match_visual_features(train, query, 0.7, -1.0)
    got = ctx.match_hamming(train, query, 0.7, -1.0)
    assert got.tobytes() == ref.tobytes()
    # d0 == d1 == 0 for the duplicated rows -> ratio test 0 < 0.7*0 fails; the unique rows pass
    assert sorted(got["queryIdx"].tolist()) == [1, 3]
    assert got["trainIdx"].tolist() == [20, 21]


def test_match_preconditions(ctx):
    rng = np.random.default_rng(1)
    with pytest.raises(capi.MvsError):
        ctx.match_hamming(_rand_desc(rng, 1), _rand_desc(rng, 4))      # < 2 train rows (reference: UB)
    with pytest.raises(capi.MvsError):
        ctx.match_hamming(_rand_desc(rng, 4), np.zeros((0, 32), np.uint8))  # invalid VisualFeature (assert)
    assert o.match_visual_features(_rand_desc(rng, 1), _rand_desc(rng, 4)) is None


# ----------------------------------------------------------------------------- device arithmetic
def test_unscaled_sqrt_div_are_ieee_exact(ctx):
    """The Jacobi loop uses hipcc's correctly rounded sqrt / div sequences WITHOUT their range-scaling steps (behind a
    range guard + recompute fallback).  Inside the guards they must be bit-identical to IEEE: checked here on 4M
    operands spread over the whole guarded exponent range, plus zeros, infinities and guard-boundary values."""
    import ctypes as C

    rng = np.random.default_rng(99)
    n = 1 << 22
    mant = rng.uniform(1.0, 2.0, size=(2, n))
    expo = rng.integers(-760, 900, size=n)
    x = np.ldexp(mant[0], expo)                                   # sqrt operands: 2^-760 .. 2^900
    y = np.ldexp(mant[1], rng.integers(-200, 200, size=n)) * rng.choice([-1.0, 1.0], size=n)
    xd = np.ldexp(mant[0], rng.integers(-200, 200, size=n)) * rng.choice([-1.0, 1.0], size=n)
    sel = rng.random(n) < 0.5
    x = np.where(sel, x, np.abs(xd))                              # half the operands exercise the division guard
    special = np.array([0.0, np.inf, 2.0 ** -767, 2.0 ** -766, 1.0, 4.0, 2.0 ** 200, 2.0 ** -200, 3.0, 1e-300])
    x[:len(special)] = special
    y[:len(special)] = [1.0, 3.0, 7.0, -2.0 ** -200, 2.0 ** 200, 3.0, 2.0 ** 200, 2.0 ** -200, -3.0, 5.0]
    counts = (C.c_ulonglong * 4)()
    # the checker lives in the diagnostics build only (the product library exports no mvs_debug_* symbol)
    assert not hasattr(capi.lib(), "mvs_debug_fastmath_check") and not hasattr(capi.lib(), "mvs_debug_set_ransac_variant")
    dbg = C.CDLL(capi.DBG_LIB_PATH)
    h = C.c_void_p()
    assert dbg.mvs_ctx_create(C.c_int(0), C.byref(h)) == 0
    dbg.mvs_ctx_destroy.argtypes = [C.c_void_p]
    st = dbg.mvs_debug_fastmath_check(h, x.ctypes.data_as(C.POINTER(C.c_double)),
                                      y.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(n), counts)
    dbg.mvs_ctx_destroy(h)
    assert st == 0
    assert counts[2] > n // 2 and counts[3] > n // 3       # the guards admitted most of the operands
    assert counts[0] == 0, "sqrt_fast differs from IEEE sqrt on %d operands" % counts[0]
    assert counts[1] == 0, "div_fast differs from IEEE division on %d operand pairs" % counts[1]


def test_rotation_parameters_are_ieee_exact(ctx):
    """The guarded pair step (unscaled sqrt sequences, divisions seeded from the square roots' by-products instead of
    v_rcp_f64, one Newton step) against the same step with the compiler's IEEE sqrt and division: rotated rows, V rows and
    norms bit for bit, on 2^25 row pairs in the regimes the solve visits -- generic, nearly orthogonal (late sweeps),
    very different norms (the null direction), equal norms, scaled by 2^-95 .. 2^95 (the whole guarded range)."""
    import ctypes as C

    dbg = C.CDLL(capi.DBG_LIB_PATH)
    h = C.c_void_p()
    assert dbg.mvs_ctx_create(C.c_int(0), C.byref(h)) == 0
    dbg.mvs_ctx_destroy.argtypes = [C.c_void_p]
    dbg.mvs_debug_pairstep_check.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_ulonglong)]
    rng = np.random.default_rng(2026)
    n = 1 << 22
    total, seed_err = 0, 0.0
    try:
        for regime in range(8):
            a = rng.normal(size=(n, 3))
            b = rng.normal(size=(n, 3))
            if regime in (1, 5):      # nearly orthogonal: the dot product is 1e-3 .. 1e-13 of the norms
                b -= (np.einsum("ij,ij->i", a, b) / np.einsum("ij,ij->i", a, a))[:, None] * a
                b += a * (10.0 ** rng.uniform(-13, -3, size=(n, 1))) * rng.choice([-1.0, 1.0], size=(n, 1))
            if regime in (2, 6):      # one row tiny
                b *= 10.0 ** rng.uniform(-17, -2, size=(n, 1))
            if regime == 3:           # equal norms: beta ~ 0, either sign
                b *= (np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1))[:, None] * (1 + rng.normal(scale=1e-15, size=(n, 1)))
            if regime in (4, 5, 6):   # common scale, up to the edge of the guarded range (row norms 2^-190 .. 2^190)
                sc = np.ldexp(1.0, rng.integers(-95, 96, size=(n, 1)) if regime == 4 else rng.integers(-60, 60, size=(n, 1)))
                a *= sc
                b *= sc
            if regime == 7:           # swapped roles (beta < 0 with a tiny first row)
                a, b = b * 10.0 ** rng.uniform(-12, 0, size=(n, 1)), a
            rows = np.ascontiguousarray(np.concatenate([a, b], axis=1))
            counts = (C.c_ulonglong * 4)()
            st = dbg.mvs_debug_pairstep_check(h, rows.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(n), counts)
            assert st == 0
            assert counts[2] == 0, "regime %d: %d rotate / skip decisions differ" % (regime, counts[2])
            assert counts[0] == 0, "regime %d: %d of %d pair steps differ from the IEEE one" % (regime, counts[0], counts[1])
            assert counts[1] > n // 3, "regime %d compared only %d steps" % (regime, counts[1])
            total += counts[1]
            seed_err = max(seed_err, float(np.frombuffer(np.uint64(counts[3]).tobytes(), dtype=np.float64)[0]))
    finally:
        dbg.mvs_ctx_destroy(h)
    print("pair steps compared bit for bit:", total, " largest error of the reciprocal estimate: 2^%.1f" % np.log2(seed_err))
    assert seed_err < 2.0 ** -45       # div_seeded's one Newton step starts from this


# ----------------------------------------------------------------------------- 8-point
def test_find_fundamental_bitwise(ctx):
    """The whole solve chain (normalise, A^T A, 9x9 + 3x3 Jacobi SVD, sqrt / div / fma) bit for bit."""
    rng = np.random.default_rng(11)
    for trial in range(40):
        p1 = rng.uniform(-0.6, 0.6, size=(8, 2))
        p2 = p1 + rng.normal(scale=0.05, size=(8, 2))
        ok_r, F_r = o.find_fundamental_matrix(p1, p2)
        ok_g, F_g = ctx.find_fundamental_matrix(p1, p2)
        assert ok_r == ok_g
        assert F_g.tobytes() == F_r.tobytes(), "trial %d: max diff %g" % (trial, np.abs(F_g - F_r).max())


def test_find_fundamental_degenerate_sample(ctx):
    p = np.tile(np.array([[0.1, 0.2]]), (8, 1))  # all points coincide -> scale == 0 (reference asserts)
    ok_r, _ = o.find_fundamental_matrix(p, p)
    ok_g, _ = ctx.find_fundamental_matrix(p, p)
    assert not ok_r and not ok_g


def _scene(seed, m, noise, outliers=0.3):
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= 0.08 / np.linalg.norm(w)
    R = o.rodrigues(w)
    t = np.array([0.3, 0.02, 0.01])
    X = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(3, 9, m)], axis=1)
    p1 = X[:, :2] / X[:, 2:3]
    X2 = (R @ X.T).T + t
    p2 = X2[:, :2] / X2[:, 2:3]
    p1 = p1 + rng.normal(scale=noise, size=p1.shape)
    p2 = p2 + rng.normal(scale=noise, size=p2.shape)
    bad = rng.random(m) < outliers
    p2[bad] = rng.uniform(-0.5, 0.5, size=(int(bad.sum()), 2))
    return p1, p2


@pytest.mark.parametrize("m,H,thr,noise", [(8, 1, 1e-3, 0.0), (9, 300, 1e-3, 1e-4), (100, 1000, 2e-3, 2e-4),
                                           (777, 2048, 1e-3, 2e-4), (1500, 513, 1e-7, 1e-3)])
def test_ransac_tables_bit_exact(ctx, m, H, thr, noise):
    """Every hypothesis' inlier count and residual sum, the winner and its mask: bit-exact."""
    p1, p2 = _scene(m * 31 + H, m, noise)
    ref = o.ransac_fundamental(p1, p2, thr, H, o.SAMPLER_PHILOX, seed=0xABCDEF12345, per_hyp=True)
    got = ctx.ransac_fundamental(p1, p2, thr, H, capi.SAMPLER_PHILOX, seed=0xABCDEF12345, per_hyp=True)
    assert np.array_equal(got["count"], ref["count"])
    assert got["residual"].tobytes() == ref["residual"].tobytes()
    assert got["best_hyp"] == ref["best_hyp"] and got["best_count"] == ref["best_count"]
    assert got["best_residual"] == ref["best_residual"]
    assert np.array_equal(got["mask"], ref["mask"])
    assert got["F"].tobytes() == ref["F"].tobytes()
    assert got["ok"] == ref["ok"]


def test_ransac_identity_sampler_is_reference_behaviour(ctx):
    """H = 1 + identity sample = the reference as shipped: one fit on the first 8 matches."""
    p1, p2 = _scene(3, 50, 1e-4, outliers=0.0)
    ref = o.ransac_fundamental(p1, p2, 1e-3, 1, o.SAMPLER_IDENTITY)
    got = ctx.ransac_fundamental(p1, p2, 1e-3, 1, capi.SAMPLER_IDENTITY)
    ok, F8 = o.find_fundamental_matrix(p1[:8], p2[:8])
    assert ok and got["F"].tobytes() == F8.tobytes() == ref["F"].tobytes()
    assert np.array_equal(got["mask"], ref["mask"]) and got["best_hyp"] == 0


def test_ransac_too_few_points(ctx):
    p1, p2 = _scene(4, 7, 0.0)
    got = ctx.ransac_fundamental(p1, p2, 1e-3, 10)
    assert not got["ok"] and got["best_hyp"] == -1     # estimator-RANSAC.cpp:25-29


# ----------------------------------------------------------------------------- sfm_solve / triangulate KATs
def test_sfm_solve_L_shape_kat(ctx):
    """test/test-sfm.cpp geometry with the L-shaped rig (the cube is degenerate for the 8-point solver,
    SURVEY section 0.3): pose.ln() == (1,0,0,0,0,0), the 8 points recovered in input order, tol 1e-3."""
    for se3 in ((1, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0.1, 0)):
        rig = helpers.two_camera_rig("L", rpy=(1.5, 0.7, 0.0), scale=0.5, se3_2to1=se3)
        prm = capi.default_params()               # H = 1, identity sampler: the reference as shipped
        got = ctx.two_view(rig["uv1"], rig["uv2"], rig["K"], prm)
        ref = o.sfm_solve(rig["uv1"], rig["uv2"], rig["K"], o.make_params(1, o.SAMPLER_IDENTITY))
        _check_two_view(got, ref, 8)
        assert got["ok"] and got["n_points"] == 8
        # the reconstruction is up to scale with |t| = 1: compare after scaling by the true baseline
        base = np.linalg.norm(rig["pose2in1"][1])
        assert np.abs(o.se3_ln(got["R"], got["t"] * base) - np.array(se3, dtype=float)).max() < 1e-3
        assert np.abs(got["points"] * base - rig["X"]).max() < 1e-3
        assert got["point_idx"].tolist() == list(range(8))


def test_sfm_triangulate_cube_kat(ctx):
    """test/test-sfm.cpp:92-155."""
    rig = helpers.two_camera_rig("cube")
    R12, t12 = rig["T1to2"]
    pts, idx = ctx.triangulate(rig["uv1"], rig["uv2"], rig["K"], R12, t12)
    ref_pts, ref_idx = o.sfm_triangulate(rig["uv1"], rig["uv2"], rig["K"], (np.eye(3), np.zeros(3)), rig["pose2in1"])
    assert idx.tolist() == ref_idx.tolist() == list(range(8))
    assert np.abs(pts - rig["X"]).max() < 1e-3
    assert helpers.rel_err(pts, ref_pts) <= TIGHT


def test_recover_pose_cube_kat(ctx):
    """test/test-sfm.cpp:17-90 with the analytic essential matrix: exercises decomposition with an EXACTLY zero
    singular value (the OpenCV random-completion path), 4-candidate selection and the pose convention."""
    rig = helpers.two_camera_rig("cube")
    R12, t12 = rig["T1to2"]
    E = helpers.skew(t12) @ R12
    got = ctx.recover_pose(E, rig["uv1"], rig["uv2"], rig["K"])
    ok, R, t, pts, idx = o.recover_pose_and_points(E, rig["uv1"], rig["uv2"])
    assert got["ok"] and ok
    assert got["point_idx"].tolist() == idx.tolist() == list(range(8))
    assert np.abs(o.se3_ln(got["R"], got["t"]) - np.array([1, 0, 0, 0, 0, 0.0])).max() < 1e-3
    assert np.abs(got["points"] - rig["X"]).max() < 1e-3
    assert helpers.rel_err(got["R1to2"], R) <= TIGHT and helpers.rel_err(got["points"], pts) <= TIGHT


def test_recover_pose_lazy_candidates_ties_and_wrong_prefix(ctx):
    """Round 5: the losers of recover_pose_and_points (sfm-solve.cpp:250-280) are triangulated on a prefix only and completed
    only while their remaining points could still take the winner's place.  Constructed correspondence lists, each point
    chosen by the candidates it survives under (from the oracle's own triangulate_points per candidate):
    exact ties between two candidates (the first in candidate order must win, strict '>' of :273), a tie at the top between a
    later prefix-best and an earlier candidate, a prefix that favours the wrong candidate, and nobody surviving."""
    rig = helpers.two_camera_rig("L", rpy=(0.3, -0.2, 0.1), scale=0.5, se3_2to1=(1, 0.2, -0.1, 0.02, 0.05, -0.03))
    R12, t12 = rig["T1to2"]
    E = helpers.skew(t12) @ R12
    Ra, Rb, t = o.decompose_essential(E)
    cands = [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]
    rng = np.random.default_rng(55)
    p1s, p2s = [], []
    for R, tt in cands:   # true correspondences of points in front of both cameras under THIS candidate (wide angle: Rb looks back)
        X = np.column_stack([rng.uniform(-20, 20, 200000), rng.uniform(-20, 20, 200000), rng.uniform(0.05, 6, 200000)])
        Y = X @ R.T + tt
        keep = Y[:, 2] > 0.05
        X, Y = X[keep][:3000], Y[keep][:3000]
        p1s.append(X[:, :2] / X[:, 2:3])
        p2s.append(Y[:, :2] / Y[:, 2:3])
    pool1 = np.concatenate(p1s + [rng.uniform(-0.6, 0.6, size=(60000, 2))])   # + random pairs: a few survive under nobody
    pool2 = np.concatenate(p2s + [rng.uniform(-0.6, 0.6, size=(60000, 2))])
    surv = np.zeros((4, len(pool1)), dtype=bool)
    for c, (R, tt) in enumerate(cands):
        _, idx = o.triangulate_points(R, tt, pool1, pool2)
        surv[c, idx] = True
    only = [np.flatnonzero(surv[c] & (surv.sum(0) == 1)) for c in range(4)]   # points surviving under candidate c alone
    none = np.flatnonzero(surv.sum(0) == 0)
    assert min(len(x) for x in only) >= 600 and len(none) >= 40
    K = np.eye(3)

    def run(spec):
        """spec: list of (candidate or None, count) runs, in order."""
        used = [0, 0, 0, 0, 0]
        sel = []
        for c, n in spec:
            src = none if c is None else only[c]
            k = 4 if c is None else c
            sel.extend(src[used[k]:used[k] + n].tolist())
            used[k] += n
        sel = np.array(sel)
        p1, p2 = pool1[sel], pool2[sel]
        got = ctx.recover_pose(E, p1, p2, K)
        ok, R, tt, pts, idx = o.recover_pose_and_points(E, p1, p2)
        assert got["ok"] == ok
        if ok:
            assert got["n_points"] == len(idx) and np.array_equal(got["point_idx"], idx)
            assert helpers.rel_err(got["R1to2"], R) <= TIGHT and helpers.rel_err(got["points"], pts) <= TIGHT
        return got, (R, tt, idx)

    # exact tie between candidates 1 and 3, both beyond the prefix: the earlier one wins
    got, (R, tt, idx) = run([(1, 300), (3, 300), (0, 50)])
    assert len(idx) == 300 and np.array_equal(R, Ra) and np.array_equal(tt, -t)
    # the prefix (64 inliers per candidate) sees only candidate 2, the total ties 2 with 0: candidate 0 (earlier) wins -> completed
    got, (R, tt, idx) = run([(2, 200), (0, 200)])
    assert len(idx) == 200 and np.array_equal(R, Ra) and np.array_equal(tt, t)
    # the prefix favours candidate 3 (64 of 64), candidate 1 wins on the whole list
    got, (R, tt, idx) = run([(3, 70), (1, 500), (None, 10)])
    assert len(idx) == 500 and np.array_equal(R, Ra) and np.array_equal(tt, -t)
    # the prefix-best wins by exactly one point over a candidate that appears only behind the prefix
    got, (R, tt, idx) = run([(2, 150), (0, 149)])
    assert len(idx) == 150 and np.array_equal(R, Rb)
    # ... and loses by one
    got, (R, tt, idx) = run([(2, 150), (0, 151)])
    assert len(idx) == 151 and np.array_equal(R, Ra)
    # fewer inliers than the prefix; nobody survives at all (recover_pose_and_points returns false)
    run([(1, 5), (0, 4)])
    got, _ = run([(None, 40)])
    assert not got["ok"]


@pytest.mark.parametrize("m,H,noise,thr", [(60, 256, 1e-4, 1e-3), (400, 1500, 2e-4, 2e-3), (1600, 700, 1e-3, 1e-2)])
def test_two_view_random_scenes(ctx, m, H, noise, thr):
    rng = np.random.default_rng(m)
    K = np.array([[525.0, 0, 320], [0, 525, 240], [0, 0, 1]])
    p1, p2 = _scene(m + 1, m, noise)
    uv1 = p1 * 525 + np.array([320, 240.0])
    uv2 = p2 * 525 + np.array([320, 240.0])
    seed = int(rng.integers(0, 2**62))
    got = ctx.two_view(uv1, uv2, K, capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=seed,
                                                        max_error_sq=thr))
    ref = o.sfm_solve(uv1, uv2, K, o.make_params(H, o.SAMPLER_PHILOX, seed, thr))
    _check_two_view(got, ref, m)
    assert ref["ok"] and ref["n_points"] > 8


def test_batch_run_points_is_a_batch_of_sfm_solve(ctx):
    """mvs_batch_run_points (round 5): the pipeline behind the matcher for a batch of caller-supplied point pairs = one
    sfm_solve (vision/sfm.hpp:30-35) per pair.  Ragged sizes incl. fewer than 8 and zero matches, two thresholds, enough pairs
    for the pre-screened stage and the two half batches: winner, count, residual sum, mask, point indices bit-exact against
    the oracle's sfm_solve of each pair, pose / points to 1e-12; and equal to the single-shot mvs_two_view."""
    K = np.array([[525.0, 0, 320], [0, 525, 240], [0, 0, 1]])
    sizes = [1600, 900, 8, 5, 0, 300, 64, 1200] + [150 + 13 * i for i in range(60)]
    P, N, H = len(sizes), 1700, 2048
    uv1 = np.zeros((P, N, 2))
    uv2 = np.zeros((P, N, 2))
    for p, m in enumerate(sizes):
        if m:
            a, c = _scene(900 + p, m, 3e-4)
            uv1[p, :m] = a * 525 + np.array([320, 240.0])
            uv2[p, :m] = c * 525 + np.array([320, 240.0])
    gidx = np.arange(40, 40 + P, dtype=np.int64)
    b = capi.Batch(ctx, P, N, 32)
    b.upload_intrinsics(0, K, gidx, count=P)
    for thr in (1e-2, 2e-3):
        prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=77, max_error_sq=thr)
        b.run_points(prm, uv1, uv2, sizes)
        b.sync()
        out = b.download()
        assert not out["matches"].view(np.uint8).any()                       # no match list on this path: rows cleared
        for p, m in enumerate(sizes):
            r = out["results"][p]
            assert r["n_matches"] == m, p
            if m < 8:
                assert not r["valid"], p
                continue
            ref = o.sfm_solve(uv1[p, :m], uv2[p, :m], K, o.make_params(H, o.SAMPLER_PHILOX, 77 + int(gidx[p]), thr))
            assert bool(r["valid"]) == ref["ok"], (thr, p)
            assert r["best_hyp"] == ref["best_hyp"] and r["best_count"] == ref["best_count"], (thr, p)
            assert r["best_residual"] == ref["best_residual"], (thr, p)
            assert np.array_equal(out["mask"][p][:m], ref["mask"][:m]), (thr, p)
            if ref["ok"]:
                n = ref["n_points"]
                assert r["n_points"] == n and np.array_equal(out["point_idx"][p][:n], ref["point_idx"]), (thr, p)
                assert np.abs(r["R"] - ref["R"]).max() <= 1e-12 and np.abs(r["t"] - ref["t"]).max() <= 1e-12, (thr, p)
                assert helpers.rel_err(out["points"][p][:n], ref["points"]) <= TIGHT, (thr, p)
        # the single-shot entry point on one of the pairs: same bits (its sampler key offset is 0: compare at gidx 0)
    b.upload_intrinsics(0, K, np.zeros(P, dtype=np.int64), count=P)
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=77, max_error_sq=1e-2)
    b.run_points(prm, uv1, uv2, sizes)
    b.sync()
    out = b.download()
    for p in (0, 5, 7):
        m = sizes[p]
        one = ctx.two_view(uv1[p, :m], uv2[p, :m], K, prm)
        r = out["results"][p]
        assert one["best_hyp"] == r["best_hyp"] and one["best_count"] == r["best_count"]
        assert one["R"].tobytes() == r["R"].tobytes() and one["t"].tobytes() == r["t"].tobytes()
        assert np.array_equal(one["mask"], out["mask"][p][:m])
    # argument checks: a count beyond the capacity, a null buffer
    with pytest.raises(capi.MvsError):
        b.run_points(prm, uv1[:1], uv2[:1], [N + 1])
    b.close()


def test_two_view_errors(ctx):
    rig = helpers.two_camera_rig("L", rpy=(1.5, 0.7, 0.0), scale=0.5)
    prm = capi.default_params()
    got = ctx.two_view(rig["uv1"][:7], rig["uv2"][:7], rig["K"], prm)       # < 8 pairs: false, never aborts
    assert not got["ok"]
    Kbad = np.array([[1, 0, 0], [0, 1, 0], [0.1, 0, 1.0]])
    with pytest.raises(capi.MvsError):
        ctx.two_view(rig["uv1"], rig["uv2"], Kbad, prm)


# ----------------------------------------------------------------------------- batched pipeline
def test_batch_pipeline_parity_healthy(ctx):
    """8 pairs x 600 keypoints, 0.5 px noise, explicit threshold: the whole path incl. triangulation."""
    prm = capi.default_params(num_hypotheses=1024, sampler=capi.SAMPLER_PHILOX, seed=0x5EED0000, max_error_sq=1e-2)
    data, out = _run_batch(ctx, 100, 8, 600, prm)
    _check_batch_against_oracle(data, out, prm)
    assert out["results"]["valid"].all() and (out["results"]["n_points"] > 100).all()


def test_batch_pipeline_parity_reference_threshold(ctx):
    """Reference threshold 5e-2/K00/K11 (sfm-solve.cpp:311): tiny inlier sets, ties broken by the residual sum --
    the regime where only a bit-exact solve chain agrees with the oracle."""
    prm = capi.default_params(num_hypotheses=1500, sampler=capi.SAMPLER_PHILOX, seed=77)
    data, out = _run_batch(ctx, 7, 6, 500, prm)
    _check_batch_against_oracle(data, out, prm)
    prm0 = capi.default_params(num_hypotheses=700, sampler=capi.SAMPLER_PHILOX, seed=78)
    data, out = _run_batch(ctx, 7, 4, 500, prm0, noise_px=0.0)
    _check_batch_against_oracle(data, out, prm0)
    assert out["results"]["valid"].all()


def test_batch_ragged_and_empty_pairs(ctx):
    """Ragged keypoint counts, an empty image, an image with one descriptor, and a pair with < 8 matches."""
    n_kp, count = 320, 6
    data = synth.make_batch(40, count, n_kp=n_kp)
    n1 = np.array([320, 200, 0, 1, 320, 64], dtype=np.int32)
    n2 = np.array([320, 320, 100, 50, 0, 7], dtype=np.int32)
    b = capi.Batch(ctx, count, n_kp, 32)
    b.upload(0, data["desc1"], data["kp1"], n1, data["desc2"], data["kp2"], n2, data["K"], data["global_index"])
    prm = capi.default_params(num_hypotheses=300, sampler=capi.SAMPLER_PHILOX, seed=5, max_error_sq=1e-2)
    b.run(prm)
    out = b.download()
    b.close()
    res = out["results"]
    for i in (2, 3, 4):   # invalid VisualFeature / < 2 train rows: no matches, no model, nothing aborts
        assert res["n_matches"][i] == 0 and not res["valid"][i]
    keep = [0, 1, 5]
    sub = {k: v[keep] for k, v in data.items()}
    sub_out = {k: v[keep] for k, v in out.items()}
    _check_batch_against_oracle(sub, sub_out, prm, n1[keep], n2[keep])


@pytest.mark.parametrize("count,thr", [(65, 1e-2), (129, 1e-2), (64, 0.0), (97, 1e-3)])
def test_half_batches_on_two_streams_equal_one_stream(ctx, count, thr):
    """A batch of >= 64 pairs runs as two halves on two streams (mvs_ctx_set_half_batches; pairs are independent,
    estimator-RANSAC.cpp:76-84 runs per pair): every output byte equals the one-stream run's, for odd counts, ragged and
    empty pairs in either half, at the bench threshold, the reference's and one in between; the first, the middle (first
    pair of the second half) and the last pair are checked against the oracle."""
    n_kp, H = 400, 2048
    data = synth.make_batch(300, count, n_kp=n_kp)
    n1, n2 = data["n1"].copy(), data["n2"].copy()
    half = (count + 1) // 2
    n1[1], n2[half + 1], n1[count - 2] = 0, 5, 123      # an empty image, a pair with < 8 matches, a ragged one
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=91, max_error_sq=thr)
    outs = []
    for halves in (True, False, True):
        ctx.set_half_batches(halves)
        try:
            b = capi.Batch(ctx, count, n_kp, 32)
            b.upload(0, data["desc1"], data["kp1"], n1, data["desc2"], data["kp2"], n2, data["K"], data["global_index"])
            b.run(prm)
            b.sync()
            outs.append(b.download())
            b.close()
        finally:
            ctx.set_half_batches(True)
    for other in outs[1:]:
        for k in ("results", "mask", "point_idx", "points", "matches"):
            res = outs[0]["results"]
            if k == "results":
                assert outs[0][k].tobytes() == other[k].tobytes()
                continue
            for i in range(count):
                n = int(res["n_matches"][i]) if k in ("mask", "matches") else int(res["n_points"][i])
                assert outs[0][k][i][:n].tobytes() == other[k][i][:n].tobytes(), (k, i)
    keep = [0, half, count - 1]
    sub = {k: v[keep] for k, v in data.items()}
    sub_out = {k: v[keep] for k, v in outs[0].items()}
    _check_batch_against_oracle(sub, sub_out, prm, n1[keep], n2[keep])


def test_full_size_pair_50k_hypotheses(ctx):
    """BASELINE config 2: one 2000-keypoint pair, 50 000 hypotheses, checked against the oracle end to end."""
    prm = capi.default_params(num_hypotheses=50000, sampler=capi.SAMPLER_PHILOX, seed=0x5EED0000, max_error_sq=1e-2)
    data, out = _run_batch(ctx, 0, 1, 2000, prm)
    _check_batch_against_oracle(data, out, prm)
    r = out["results"][0]
    assert r["valid"] and r["n_matches"] > 1400 and r["n_points"] > 900


def test_two_full_size_pairs_take_the_prescreened_stage(ctx):
    """Two pairs x 50 000 hypotheses run on the pre-screened stage (round 4: their hypotheses fill the chip more than once on
    the fused kernel); one pair and two pairs with few hypotheses stay on the fused kernel.  Same records either way: each pair
    alone (fused) == inside the two-pair launch (pre-screened) == the oracle."""
    n_kp, H = 2000, 50000
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=0x5EED0000, max_error_sq=1e-2)
    data, out = _run_batch(ctx, 700, 2, n_kp, prm)
    _check_batch_against_oracle(data, out, prm)
    b1 = capi.Batch(ctx, 1, n_kp, 32)
    for i in range(2):
        sl = slice(i, i + 1)
        b1.upload(0, data["desc1"][sl], data["kp1"][sl], data["n1"][sl], data["desc2"][sl], data["kp2"][sl], data["n2"][sl],
                  data["K"][sl], data["global_index"][sl])
        b1.run(prm)
        b1.sync()
        assert b1.download(matches=False, mask=False, points=False)["results"][0].tobytes() == out["results"][i].tobytes()
    b1.close()
    st = None
    b2 = capi.Batch(ctx, 2, n_kp, 32)
    b2.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"], data["global_index"])
    st = b2.stats(prm)
    b2.close()
    assert st["pairs_mode"] == [0, 2, 0] and 0 < st["exact_solves"] < 2000      # the pre-screened stage's own bookkeeping


def test_full_size_properties(ctx):
    """Size-independent properties at BASELINE sizes (no oracle): determinism, shard invariance (pair p gives the
    same result alone as inside a batch), mask/count consistency, cheirality of every returned point, sorted match
    lists, epipolar residual of every inlier under the returned F below the threshold."""
    prm = capi.default_params(num_hypotheses=50000, sampler=capi.SAMPLER_PHILOX, seed=0x5EED0000, max_error_sq=1e-2)
    data, out = _run_batch(ctx, 200, 3, 2000, prm)
    data1, out1 = _run_batch(ctx, 201, 1, 2000, prm)
    assert out["results"][1].tobytes() == out1["results"][0].tobytes()          # shard invariance + determinism
    assert out["matches"][1].tobytes() == out1["matches"][0].tobytes()        # whole capacity: the tails are zero
    assert np.array_equal(out["mask"][1], out1["mask"][0]) and out["points"][1].tobytes() == out1["points"][0].tobytes()
    for i in range(3):
        r = out["results"][i]
        M, n = r["n_matches"], r["n_points"]
        mt = out["matches"][i][:M]
        key = mt["distance"].astype(np.int64) * 65536 + mt["queryIdx"]
        assert (np.diff(key) > 0).all()                                          # sorted by (distance, queryIdx)
        assert len(set(mt["queryIdx"].tolist())) == M
        assert out["mask"][i][:M].sum() == r["n_inliers"] == r["best_count"]
        idx = out["point_idx"][i][:n]
        assert (np.diff(idx) > 0).all() and out["mask"][i][idx].all()            # ordered subset of the inliers
        pts = out["points"][i][:n]
        assert (pts[:, 2] > 0).all()
        z2 = (r["R1to2"] @ pts.T).T[:, 2] + r["t1to2"][2]
        assert (z2 > 0).all()                                                    # cheirality in both cameras
        Kinv = np.linalg.inv(data["K"][i].reshape(3, 3))
        x1 = (Kinv @ np.c_[data["kp1"][i][mt["trainIdx"]].astype(float), np.ones(M)].T).T
        x2 = (Kinv @ np.c_[data["kp2"][i][mt["queryIdx"]].astype(float), np.ones(M)].T).T
        res = np.abs(np.einsum("ij,jk,ik->i", x2, r["F"], x1))
        inl = out["mask"][i][:M].astype(bool)
        assert (res[inl] < 1e-2 * (1 + 1e-9)).all() and (res[~inl] > 1e-2 * (1 - 1e-9)).all()
        assert abs(np.linalg.norm(r["t1to2"]) - 1.0) < 1e-9
        assert np.abs(r["R"] @ r["R"].T - np.eye(3)).max() < 1e-9


# ----------------------------------------------------------------------------- capacity / odd sizes
@pytest.mark.parametrize("n_kp,H,desc_bytes", [(4096, 300, 32), (1000, 1, 32), (777, 257, 16), (513, 1025, 64)])
def test_batch_capacity_and_odd_sizes(ctx, n_kp, H, desc_bytes):
    """Maximum keypoint capacity (4096: more than 2048 matches go through the LDS point stream and the 2-pass bitonic
    sort), hypothesis counts that are not multiples of the workgroup size, 128- and 512-bit descriptors."""
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=31337, max_error_sq=1e-2)
    count = 2
    data = synth.make_batch(500, count, n_kp=n_kp, desc_bytes=desc_bytes, common_frac=0.9)
    b = capi.Batch(ctx, count, n_kp, desc_bytes)
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"],
             data["global_index"])
    b.run(prm)
    out = b.download()
    b.close()
    _check_batch_against_oracle(data, out, prm)
    if n_kp == 4096:
        assert (out["results"]["n_matches"] > 2048).all()


@pytest.mark.parametrize("n_kp,H,desc_bytes,count,thr", [(4096, 300, 32, 3, 1e-2), (1000, 1, 32, 4, 1e-2), (777, 257, 16, 3, 1e-2),
                                                         (513, 1025, 64, 5, 1e-2), (300, 3, 32, 3, 1e-2), (640, 2050, 32, 4, 0.0)])
def test_pruned_scoring_path_capacity_and_odd_sizes(ctx, n_kp, H, desc_bytes, count, thr):
    """The same edge sizes through the solve -> count -> select launches (batches of three or more pairs take that path;
    one or two pairs stay on the fused kernel): maximum capacity (128 KB of LDS per workgroup), hypothesis counts that
    are not multiples of 4 or 256 (partial groups of four, padded lanes), a single hypothesis, the reference threshold
    (hundreds of ties through the lane-per-hypothesis path of ransac_select)."""
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=4711, max_error_sq=thr)
    data = synth.make_batch(900, count, n_kp=n_kp, desc_bytes=desc_bytes, common_frac=0.9)
    n1, n2 = data["n1"].copy(), data["n2"].copy()
    if count >= 4:
        n2[1] = 5                      # a pair with fewer than 8 matches in the middle of the batch
    b = capi.Batch(ctx, count, n_kp, desc_bytes)
    b.upload(0, data["desc1"], data["kp1"], n1, data["desc2"], data["kp2"], n2, data["K"], data["global_index"])
    b.run(prm)
    out = b.download()
    b.close()
    _check_batch_against_oracle(data, out, prm, n1, n2)
    if count >= 4:
        assert not out["results"]["valid"][1] and out["results"]["best_hyp"][1] == -1


def test_batch_capacity_errors(ctx):
    with pytest.raises(capi.MvsError):
        capi.Batch(ctx, 1, 4097, 32)          # beyond the LDS-resident capacity
    with pytest.raises(capi.MvsError):
        capi.Batch(ctx, 1, 100, 24)           # descriptor size not 16 / 32 / 64 bytes


# ----------------------------------------------------------------------------- golden vectors (oracle-free)
def test_gpu_against_golden_vectors(ctx):
    """The committed expected outputs of tests/golden/ (match list, RANSAC tables, full image pairs) without the oracle."""
    import os

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "match_small.npz"))
    for tag in "abc":
        ratio, md = g["params_" + tag]
        assert ctx.match_hamming(g["train"], g["query"], float(ratio), float(md)).tobytes() == g["matches_" + tag].tobytes()
    g = np.load(os.path.join(gold, "ransac_small.npz"))
    r = ctx.ransac_fundamental(g["p1"], g["p2"], float(g["thr"]), int(g["H"]), capi.SAMPLER_PHILOX, int(g["seed"]), True)
    assert np.array_equal(r["count"], g["count"]) and r["residual"].tobytes() == g["residual"].tobytes()
    assert r["F"].tobytes() == g["F"].tobytes() and np.array_equal(r["mask"], g["mask"])
    assert [r["best_hyp"], r["best_count"]] == g["best"].tolist()
    g = np.load(os.path.join(gold, "image_pair_small.npz"))
    n_kp = g["desc1"].shape[1]
    b = capi.Batch(ctx, 2, n_kp, 32)
    ones = np.full(2, n_kp, dtype=np.int32)
    b.upload(0, g["desc1"], g["kp1"], ones, g["desc2"], g["kp2"], ones, g["K"], g["global_index"])
    b.run(capi.default_params(num_hypotheses=int(g["H"]), sampler=capi.SAMPLER_PHILOX, seed=int(g["seed"]),
                              max_error_sq=float(g["max_error_sq"])))
    out = b.download()
    b.close()
    for i in range(2):
        ok, M, ninl, npts, bh, bc = g["scalars_%d" % i].tolist()
        r = out["results"][i]
        assert [int(r["valid"]), r["n_matches"], r["n_inliers"], r["n_points"], r["best_hyp"], r["best_count"]] == [ok, M, ninl, npts, bh, bc]
        assert out["matches"][i][:M].tobytes() == g["matches_%d" % i].tobytes()
        assert np.array_equal(out["mask"][i][:M], g["mask_%d" % i])
        assert np.array_equal(out["point_idx"][i][:npts], g["point_idx_%d" % i])
        assert out["points"][i][:npts].tobytes() == g["points_%d" % i].tobytes()
        assert r["R"].tobytes() == g["R_%d" % i].tobytes() and r["t"].tobytes() == g["t_%d" % i].tobytes()


# ----------------------------------------------------------------------------- context workspaces
def _bytes_of(r):
    """every value of an entry point's result as raw bytes (bit-for-bit comparison)"""
    if isinstance(r, dict):
        return {k: _bytes_of(v) for k, v in r.items()}
    if isinstance(r, (list, tuple)):
        return [_bytes_of(v) for v in r]
    return np.asarray(r).tobytes()


def test_one_context_same_answers_while_its_workspaces_grow():
    """small -> clearly larger -> small again on ONE fresh context: every single-shot entry point regrows its workspace
    (and the extraction re-captures its graph for a second image shape), and the third call equals the first bit for bit.
    Both estimators' tables regrow beside each other on the one scratch batch."""
    K = np.array([[525.0, 0, 320], [0, 525, 240], [0, 0, 1]])
    rng = np.random.default_rng(31)
    images = {shape: np.kron(rng.integers(0, 256, size=(shape[0], shape[1] // 6, shape[2] // 6)).astype(np.uint8),
                             np.ones((1, 6, 6), dtype=np.uint8)) for shape in ((1, 120, 162), (2, 480, 642))}

    def run_all(c, m, H, n_kp, shape):
        rng = np.random.default_rng(m)
        p1, p2 = _scene(1000 + m, m, 2e-4)
        uv1, uv2 = p1 * 525 + np.array([320, 240.0]), p2 * 525 + np.array([320, 240.0])
        prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=9, max_error_sq=2e-3)
        pair = synth.make_pair(5 + n_kp, n_kp=n_kp)
        X = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(4, 9, m)], axis=1)
        R, t = o.rodrigues(np.array([0.02, -0.05, 0.01])), np.array([0.2, -0.1, 0.3])
        uv = o.project_points(K, R, t, X)
        Xc = X / X[:, 2:3]
        cov = np.tile(np.eye(2).reshape(4) * 0.25, (m, 1))
        ex = c.extract(images[shape], capi.default_orb_params(nfeatures=300 if shape[0] == 1 else 1500))
        # the five-point calls keep 256 hypotheses in the large round: the growth under test is in m and the 8-point tables
        prm5 = capi.default_params(num_hypotheses=min(H, 256), sampler=capi.SAMPLER_PHILOX, seed=9, max_error_sq=2e-3)
        tv = c.two_view(uv1, uv2, K, prm)
        return dict(
            two_view=tv,
            two_view_essential=c.two_view_essential(uv1, uv2, K, prm5),
            ransac_essential=c.ransac_essential(p1, p2, 2e-3, min(H, 256), capi.SAMPLER_PHILOX, seed=17, per_hyp=True),
            recover_pose=c.recover_pose(tv["E"], uv1, uv2, K, tv["mask"]),
            triangulate=c.triangulate(uv1, uv2, K, tv["R1to2"], tv["t1to2"]),
            image_pair=c.image_pair(pair["desc1"], pair["kp1"], pair["desc2"], pair["kp2"], pair["K"], prm),
            pnp_solve=c.pnp_solve(X, uv, K, capi.default_pnp_params(num_hypotheses=H // 4, seed=3)),
            sfm_refine=c.sfm_refine(Xc[:, :2] * 525 + [320, 240], cov, uv, cov, K, R, t, X),
            ransac_fundamental=c.ransac_fundamental(p1, p2, 2e-3, H, capi.SAMPLER_PHILOX, seed=17, per_hyp=True),
            # the rows past an image's n keypoints are not outputs
            extract=[(n, ex["kp"][i][:n], ex["desc"][i][:n]) for i, n in enumerate(ex["n"].tolist())])

    c = capi.Context(0)
    try:
        first = _bytes_of(run_all(c, 60, 256, 300, (1, 120, 162)))
        run_all(c, 2500, 4096, 3000, (2, 480, 642))
        again = _bytes_of(run_all(c, 60, 256, 300, (1, 120, 162)))
    finally:
        c.close()
    for name in first:
        assert again[name] == first[name], name


def _fresh(fn):
    c = capi.Context(0)
    try:
        return fn(c)
    finally:
        c.close()


def test_estimators_interleaved_on_one_context():
    """The 8-point and the five-point entry points share the context's scratch batch, its tables and the pinned arena: every
    call gives the same bits in a fixed order, in the reverse order and alone on a context of its own.  65 points are one
    past a wavefront, 70 hypotheses two five-point blocks of 64."""
    m, H, thr = 65, 70, 2e-3
    K = np.array([[525.0, 0, 320], [0, 525, 240], [0, 0, 1]])
    p1, p2 = _scene(6500, m, 1e-4, outliers=0.1)
    uv1, uv2 = p1 * 525 + np.array([320, 240.0]), p2 * 525 + np.array([320, 240.0])
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=21, max_error_sq=thr)
    pair = synth.make_pair(3, n_kp=128)
    tv = _fresh(lambda c: c.two_view(uv1, uv2, K, prm))   # step 3 alone: its E, mask and pose are the inputs of steps 5 and 6
    assert tv["ok"]
    calls = [
        lambda c: c.ransac_fundamental(p1, p2, thr, H, capi.SAMPLER_PHILOX, seed=17, per_hyp=True),
        lambda c: c.two_view_essential(uv1, uv2, K, prm),
        lambda c: c.two_view(uv1, uv2, K, prm),
        lambda c: c.ransac_essential(p1, p2, thr, H, capi.SAMPLER_PHILOX, seed=17, per_hyp=True),
        lambda c: c.recover_pose(tv["E"], uv1, uv2, K, tv["mask"]),
        lambda c: c.triangulate(uv1, uv2, K, tv["R1to2"], tv["t1to2"]),
        lambda c: c.ransac_fundamental(p1, p2, thr, H, capi.SAMPLER_PHILOX, seed=17, per_hyp=False),
        lambda c: c.image_pair(pair["desc1"], pair["kp1"], pair["desc2"], pair["kp2"], pair["K"], prm),
        lambda c: c.two_view_essential(uv1, uv2, K, prm),
    ]
    alone = [_bytes_of(_fresh(f)) for f in calls]
    forward = _fresh(lambda c: [_bytes_of(f(c)) for f in calls])
    backward = _fresh(lambda c: [_bytes_of(f(c)) for f in reversed(calls)])[::-1]
    assert alone[2] == _bytes_of(tv)
    for k in range(len(calls)):
        assert forward[k] == alone[k], k
        assert backward[k] == alone[k], k


@pytest.mark.parametrize("estimator", ["eight_point", "five_point"])
def test_two_view_and_ransac_return_codes(ctx, estimator):
    """the status of every refused call and of too few points, the same for both estimators except where noted"""
    two_view = ctx.two_view if estimator == "eight_point" else ctx.two_view_essential
    ransac = ctx.ransac_fundamental if estimator == "eight_point" else ctx.ransac_essential
    K = np.array([[525.0, 0, 320], [0, 525, 240], [0, 0, 1]])
    p1, p2 = _scene(77, 20, 1e-4)
    uv1, uv2 = p1 * 525 + np.array([320, 240.0]), p2 * 525 + np.array([320, 240.0])

    def status_of(fn, *args, **kw):
        with pytest.raises(capi.MvsError) as e:
            fn(*args, **kw)
        return e.value.status

    prm = capi.default_params(num_hypotheses=8, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=2e-3)
    assert status_of(two_view, uv1[:0], uv2[:0], K, prm) == capi.MVS_ERR_INVALID_ARG
    got = two_view(uv1[:7], uv2[:7], K, prm)
    assert not got["ok"] and got["n_matches"] == 7 and got["best_hyp"] == -1 and not got["valid"]
    assert status_of(two_view, uv1, uv2, K, capi.default_params(num_hypotheses=0)) == capi.MVS_ERR_INVALID_ARG
    assert status_of(two_view, uv1, uv2, K, capi.default_params(num_hypotheses=8, sampler=7)) == capi.MVS_ERR_INVALID_ARG
    Kbad = K.copy()
    Kbad[2, 0] = 0.1
    assert status_of(two_view, uv1, uv2, Kbad, prm) == capi.MVS_ERR_BAD_INTRINSICS
    # the RANSAC stage alone: only the five-point one validates the sampler, the 8-point one samples any non-zero value as Philox
    if estimator == "five_point":
        assert status_of(ransac, p1, p2, 2e-3, 8, sampler=7) == capi.MVS_ERR_INVALID_ARG
    else:
        odd = ransac(p1, p2, 2e-3, 8, sampler=7, seed=5, per_hyp=True)
        assert odd["ok"] and _bytes_of(odd) == _bytes_of(ransac(p1, p2, 2e-3, 8, sampler=capi.SAMPLER_PHILOX, seed=5, per_hyp=True))
    big = np.zeros((4097, 2))
    assert status_of(ransac, big, big, 2e-3, 8) == capi.MVS_ERR_CAPACITY
    assert status_of(ransac, p1, p2, 0.0, 8) == capi.MVS_ERR_INVALID_ARG
