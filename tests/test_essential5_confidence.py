"""The termination rule of the five-point RANSAC (mvs_ctx_set_essential_confidence).

CPU: e5_confident and the checkpoint sequence of mvslam_amd/csrc/five_point.hpp, compiled for the host
(tests/cpp/e5_confident_host.cpp), against the numpy statement of the rule below; the stand-alone program plain and under
ASan + UBSan; the shim with MVSLAM_ESSENTIAL_CONFIDENCE.

GPU: a pair that stops at checkpoint T returns, byte for byte, what the host model (tests/e5_model.py, unchanged) returns for
num_hypotheses = T, where T comes from applying the numpy rule to the model's count table of the full run.  Nothing here depends
on a tolerance."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import e5_model as em
import helpers
import oracle_lib as o
from mvslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "e5_confident_host.cpp")
LIBDIR = os.path.join(ROOT, "mvslam_amd", "lib")
SHIM = os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp")
SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "test_compat_essential.cpp")
SHIM_EXE = os.path.join(LIBDIR, "test_compat_essential_5pt_confidence")
REF = "/root/reference/source"

BLOCK = 64   # kE5HypPerBlock: the first checkpoint


# ---- the rule, stated independently of the header ------------------------------------------------------------------------
def checkpoints(H):
    T = [min(BLOCK, H)]
    while T[-1] < H:
        T.append(min(2 * T[-1], H))
    return T


def confident(c, M, j, p):
    """c: int array.  Every operation below is one rounded binary64 operation (numpy float64 arithmetic)."""
    c = np.asarray(c)
    w = c.astype(np.float64) / np.float64(M)
    w2 = w * w
    w5 = (w2 * w2) * w
    x = np.float64(1.0) - w5
    for _ in range(6 + j):
        x = x * x
    return (c >= 1) & (x <= np.float64(1.0) - np.float64(p))


def horizon(count, M, H, p):
    """n_run of a pair with M >= 8 matches from the count table [H][10] of the full run"""
    if p == 0:
        return H
    for j, T in enumerate(checkpoints(H)):
        if T == H or bool(confident(int(count[:T].max()), M, j, p)):
            return T
    raise AssertionError("unreachable")


# ---- CPU: the header's function -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rule_lib():
    d = tempfile.mkdtemp(prefix="e5conf_")
    so = os.path.join(d, "libe5_confident_host.so")
    subprocess.check_call(["g++", *em.HOST_FLAGS, "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.e5_confident_row.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_uint8)]
    lib.e5_confident_row.restype = None
    lib.e5_checkpoints.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    return lib


def test_e5_confident_equals_the_numpy_statement():
    lib = rule_lib()
    stops = 0
    for M in (8, 9, 150, 4096):
        c = np.arange(M + 1)
        for j in range(11):
            for p in (0.5, 0.95, 0.99, 0.999999):
                row = np.zeros(M + 1, dtype=np.uint8)
                lib.e5_confident_row(M, j, p, row.ctypes.data_as(C.POINTER(C.c_uint8)))
                ref = confident(c, M, j, p)
                assert np.array_equal(row.astype(bool), ref), (M, j, p, np.nonzero(row.astype(bool) != ref)[0][:5])
                assert not row[0] and row[M]
                stops += int(row.sum())
    assert stops > 1000     # (not vacuous: both answers occur in bulk)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_e5_confident_host_program(tmp_path, sanitize):
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    exe = str(tmp_path / "e5_confident_host")
    subprocess.check_call(["g++", *em.HOST_FLAGS, *san, "-o", exe, SRC])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "sequences=9" in out and "bad=0" in out and "ERROR" not in out and "runtime error" not in out, out


def test_checkpoint_sequence():
    lib = rule_lib()
    want = {1: [1], 63: [63], 64: [64], 65: [64, 65], 128: [64, 128], 129: [64, 128, 129],
            1000: [64, 128, 256, 512, 1000]}
    for H, seq in want.items():
        buf = (C.c_int * 40)()
        n = lib.e5_checkpoints(H, buf, 40)
        assert list(buf[:n]) == seq == checkpoints(H), H
    buf = (C.c_int * 40)()
    n = lib.e5_checkpoints(2 ** 31 - 1, buf, 40)     # no overflow on the way to the largest int
    assert list(buf[:n]) == checkpoints(2 ** 31 - 1) and n == 26


# ---- CPU: the C++ surface --------------------------------------------------------------------------------------------------
def _build_shim():
    assert os.path.exists(os.path.join(LIBDIR, "libmvslam_hip.so")), "build the HIP library first (__graft_entry__.build)"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-DMVSLAM_USE_ESSENTIAL_5POINT",
                           "-DMVSLAM_ESSENTIAL_CONFIDENCE=0.99", "-o", SHIM_EXE, SHIM_SRC, "-L", LIBDIR, "-lmvslam_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])


def test_shim_with_both_macros_compiles_and_links():
    _build_shim()
    assert os.path.exists(SHIM_EXE)


def test_the_confidence_macro_alone_names_the_setter():
    def pre(flags):
        out = subprocess.run(["g++", "-std=c++17", "-E", "-P", *flags, "-x", "c++", SHIM], stdout=subprocess.PIPE, check=True)
        text = out.stdout.decode()
        return text[text.index("namespace mvSLAM"):]    # past the C ABI header's declarations
    for five in ([], ["-DMVSLAM_USE_ESSENTIAL_5POINT"]):
        off, on = pre(five), pre(five + ["-DMVSLAM_ESSENTIAL_CONFIDENCE=0.99"])
        assert "mvs_ctx_set_essential_confidence" not in off
        assert on.count("mvs_ctx_set_essential_confidence(h.ctx, 0.99)") == 1
        assert on.count("mvs_two_view_essential(") == off.count("mvs_two_view_essential(")     # no call site added


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not present on this machine")
def test_forwarding_file_parses_with_the_confidence_macro():
    """integration/source/vision/sfm-solve.cpp against the reference's headers (as tests/test_integration_syntax.py does): with
    both macros it sets the reference's 0.99 in front of the five-point call; without MVSLAM_ESSENTIAL_CONFIDENCE it never names
    the setter"""
    tu = os.path.join(ROOT, "integration", "source", "vision", "sfm-solve.cpp")
    inc = ["-I" + REF, "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.dirname(tu)]
    for defs in (["-DUSE_OPENCV_ESSENTIAL_MATRIX", "-DMVSLAM_ESSENTIAL_CONFIDENCE"], ["-DMVSLAM_ESSENTIAL_CONFIDENCE"]):
        p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", *inc, *defs, tu], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
    text = open(tu).read()
    body = text[text.index("namespace mvSLAM"):]
    assert body.count("mvs_ctx_set_essential_confidence(hip::context(), VF_MATCH_CONFIDENCE_LEVEL)") == 1

    # the file's own conditionals (its includes come before the namespace)
    p = subprocess.run(["g++", "-std=c++11", "-E", "-P", "-DUSE_OPENCV_ESSENTIAL_MATRIX", "-x", "c++", "-"], input=body,
                       capture_output=True, text=True, check=True)
    assert "mvs_ctx_set_essential_confidence" not in p.stdout and "mvs_two_view_essential(" in p.stdout


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def scene(seed, m, outliers):
    """ideal-camera matches of a random pose, noise 1e-4, a share of wrong matches (uniform in the image of camera 2)"""
    rng = np.random.default_rng(seed)
    om = rng.normal(size=3)
    om *= rng.uniform(0.05, 0.3) / np.linalg.norm(om)
    R = o.se3_exp(np.concatenate([np.zeros(3), om]))[0]
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    z = rng.uniform(2, 10, m)
    X = np.stack([rng.uniform(-0.5, 0.5, m) * z, rng.uniform(-0.5, 0.5, m) * z, z], axis=1)
    X2 = X @ R.T + t
    p1, p2 = X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]
    p1 = p1 + rng.normal(scale=1e-4, size=p1.shape)
    p2 = p2 + rng.normal(scale=1e-4, size=p2.shape)
    bad = rng.random(m) < outliers
    p2[bad] = rng.uniform(-0.5, 0.5, size=(int(bad.sum()), 2))
    return p1, p2


THR, H_FULL, SEED = 1e-6, 1000, 3
CASES = [(0.2, 150, 0.99), (0.2, 64, 0.999999), (0.5, 64, 0.99), (0.5, 300, 0.999999), (0.5, 300, 0.5), (0.65, 150, 0.99),
         (0.65, 150, 0.5)]


@functools.lru_cache(maxsize=None)
def _scene_and_full(outliers, m):
    """(p1, p2, host model of the full run): computed once, shared by the tests, never written to"""
    p1, p2 = scene(700 + m, m, outliers)
    return p1, p2, em.host_ransac(p1, p2, THR, H_FULL, capi.SAMPLER_PHILOX, SEED)


def _expected_T(outliers, m, p, H=H_FULL):
    p1, p2, full = _scene_and_full(outliers, m)
    return horizon(full["count"][:H], m, H, p)


def test_the_cases_cover_the_first_the_last_and_two_checkpoints_between():
    Ts = {_expected_T(*c) for c in CASES}
    print("T over the cases:", sorted(Ts))
    assert BLOCK in Ts and H_FULL in Ts and len(Ts - {BLOCK, H_FULL}) >= 2, sorted(Ts)


@pytest.fixture
def conf(ctx):
    """sets the confidence level of the shared context; back to 0 (the default) afterwards"""
    yield ctx.set_essential_confidence
    ctx.set_essential_confidence(0.0)


def _same_result(a, b, keys=("best_hyp", "best_root", "best_count", "ok")):
    for k in keys:
        assert a[k] == b[k], k
    assert np.float64(a["best_residual"]).tobytes() == np.float64(b["best_residual"]).tobytes()
    assert a["E"].tobytes() == b["E"].tobytes()
    assert np.array_equal(a["mask"], b["mask"])


def _check_adaptive(ctx, conf, p1, p2, thr, H, p, T, full_tables):
    """the adaptive call against the host model at T; its tables; and the fixed call with num_hypotheses = T"""
    conf(p)
    got = ctx.ransac_essential(p1, p2, thr, H, capi.SAMPLER_PHILOX, SEED, per_hyp=True)
    conf(0.0)
    assert got["hypotheses_run"] == T
    ref = em.host_ransac(p1, p2, thr, T, capi.SAMPLER_PHILOX, SEED)
    assert (got["best_hyp"], got["best_root"], got["best_count"]) == (ref["best_hyp"], ref["best_root"], ref["best_count"])
    assert np.float64(got["best_residual"]).tobytes() == np.float64(ref["best_residual"]).tobytes()
    assert got["E"].tobytes() == ref["E"].tobytes()
    assert np.array_equal(got["mask"], ref["mask"])
    assert got["ok"] == (ref["found"] and ref["best_count"] > 0)
    nr, cnt = full_tables
    assert np.array_equal(got["n_roots"][:T], nr[:T]) and np.array_equal(got["count"][:T], cnt[:T])
    assert (got["n_roots"][T:] == 0).all() and (got["count"][T:] == -1).all()
    fixed = ctx.ransac_essential(p1, p2, thr, T, capi.SAMPLER_PHILOX, SEED, per_hyp=True)
    assert fixed["hypotheses_run"] == T
    _same_result(got, fixed)
    assert np.array_equal(got["n_roots"][:T], fixed["n_roots"]) and np.array_equal(got["count"][:T], fixed["count"])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("outliers,m,p", CASES)
def test_ransac_essential_stops_at_the_models_checkpoint(ctx, conf, outliers, m, p):
    p1, p2, full = _scene_and_full(outliers, m)
    T = _expected_T(outliers, m, p)
    got = _check_adaptive(ctx, conf, p1, p2, THR, H_FULL, p, T, (full["n_roots"], full["count"]))
    print("outliers %.2f m %d p %g: T = %d, winner %d with %d inliers (full run: %d with %d)"
          % (outliers, m, p, T, got["best_hyp"], got["best_count"], full["best_hyp"], full["best_count"]))


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 63, 64, 65, 127, 128, 129])
def test_hypothesis_count_edges(ctx, conf, H):
    p1, p2, full = _scene_and_full(0.2, 150)
    T = _expected_T(0.2, 150, 0.99, H)
    assert T == min(H, BLOCK)
    _check_adaptive(ctx, conf, p1, p2, THR, H, 0.99, T, (full["n_roots"][:H], full["count"][:H]))


@pytest.mark.gpu
def test_degenerate_samples_never_stop_early(ctx, conf):
    same = np.tile([0.1, 0.2], (20, 1))
    conf(0.99)
    got = ctx.ransac_essential(same, same, 1e-4, 200, capi.SAMPLER_PHILOX, 0, per_hyp=True)
    assert got["hypotheses_run"] == 200 and not got["ok"] and got["best_hyp"] == -1
    assert (got["n_roots"] == 0).all() and (got["count"] == -1).all() and not got["mask"].any()
    assert not ctx.ransac_essential(same[:7], same[:7], 1e-4, 200)["hypotheses_run"]      # fewer than eight matches: nothing ran


@pytest.mark.gpu
def test_two_view_essential_cube_stops_after_one_block(ctx, conf):
    """all eight points are inliers of the true model: c = M, q = 0 exactly -- and the result is the H = 64 cube's
    (tests/test_essential5_gpu.py::test_two_view_essential_cube)"""
    rig = helpers.two_camera_rig("cube")
    prm64 = capi.default_params(num_hypotheses=64, sampler=capi.SAMPLER_PHILOX, seed=0)
    prm256 = capi.default_params(num_hypotheses=256, sampler=capi.SAMPLER_PHILOX, seed=0)
    want = ctx.two_view_essential(rig["uv1"], rig["uv2"], rig["K"], prm64)
    assert want["hypotheses_run"] == 64
    assert ctx.two_view_essential(rig["uv1"], rig["uv2"], rig["K"], prm256)["hypotheses_run"] == 256
    conf(0.99)
    got = ctx.two_view_essential(rig["uv1"], rig["uv2"], rig["K"], prm256)
    assert got["hypotheses_run"] == 64
    assert got["raw"] == want["raw"] and np.array_equal(got["mask"], want["mask"])
    assert got["points"].tobytes() == want["points"].tobytes() and np.array_equal(got["point_idx"], want["point_idx"])
    assert got["ok"] and got["n_points"] == 8 and got["best_count"] == 8
    assert np.abs(o.se3_ln(got["R"].reshape(3, 3), got["t"]) - np.array([1, 0, 0, 0, 0, 0.0])).max() < 1e-3
    assert np.abs(got["points"] - rig["X"]).max() < 1e-3


@pytest.mark.gpu
def test_setter_validation_and_the_way_back_to_the_default():
    c = capi.Context(0)
    try:
        with pytest.raises(capi.MvsError) as e:
            c.essential_hypotheses_run()                       # no five-point call yet
        assert e.value.status == capi.MVS_ERR_INVALID_ARG
        p1, p2, _ = _scene_and_full(0.2, 150)
        before = c.ransac_essential(p1, p2, THR, 300, capi.SAMPLER_PHILOX, SEED, per_hyp=True)
        assert before["hypotheses_run"] == 300
        for bad in (1.0, -0.1, float("nan"), 1.5, float("inf")):
            with pytest.raises(capi.MvsError) as e:
                c.set_essential_confidence(bad)
            assert e.value.status == capi.MVS_ERR_INVALID_ARG, bad
        assert c.ransac_essential(p1, p2, THR, 300, capi.SAMPLER_PHILOX, SEED)["hypotheses_run"] == 300   # a refused value sets nothing
        c.set_essential_confidence(0.99)
        assert c.ransac_essential(p1, p2, THR, 300, capi.SAMPLER_PHILOX, SEED)["hypotheses_run"] == BLOCK
        # a call that fails before anything runs leaves no n_run behind, not the previous call's
        big = np.zeros((4097, 2))
        with pytest.raises(capi.MvsError) as e:
            c.ransac_essential(big, big, THR, 300)
        assert e.value.status == capi.MVS_ERR_CAPACITY
        with pytest.raises(capi.MvsError) as e:
            c.essential_hypotheses_run()
        assert e.value.status == capi.MVS_ERR_INVALID_ARG
        c.set_essential_confidence(0)
        after = c.ransac_essential(p1, p2, THR, 300, capi.SAMPLER_PHILOX, SEED, per_hyp=True)
        assert after["hypotheses_run"] == 300
        _same_result(before, after)
        assert np.array_equal(before["n_roots"], after["n_roots"]) and np.array_equal(before["count"], after["count"])
    finally:
        c.close()


_DOWNLOAD_KEYS = ("results", "matches", "mask", "points", "point_idx")


@pytest.mark.gpu
def test_batch_stops_each_pair_on_its_own(ctx, conf):
    P, N, H, p_conf = 64, 96, 300, 0.99
    rng = np.random.default_rng(79)
    fams = list(helpers.CAMERAS)
    Ks = np.stack([helpers.CAMERAS[fams[p % len(fams)]][0] for p in range(P)])
    m = rng.integers(8, N + 1, size=P).astype(np.int32)
    m[3] = 5
    shares = (0.2, 0.5, 0.65, 1.0)
    uv1, uv2 = np.zeros((P, N, 2)), np.zeros((P, N, 2))
    for p in range(P):
        a, b2 = scene(3000 + p, N, shares[p % 4])
        h = lambda q: np.hstack([q, np.ones((N, 1))]) @ Ks[p].T   # noqa: E731
        uv1[p], uv2[p] = h(a)[:, :2], h(b2)[:, :2]
        uv1[p, m[p]:], uv2[p, m[p]:] = 0.0, 0.0
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=500, max_error_sq=THR)
    # the model: the rule on the host model's full table of every pair, on the normalised points the device sees
    want = np.zeros(P, dtype=np.int32)
    for p in range(P):
        if m[p] >= 8:
            n1, n2 = o.normalize_points(Ks[p], uv1[p, :m[p]]), o.normalize_points(Ks[p], uv2[p, :m[p]])
            want[p] = horizon(em.host_ransac(n1, n2, THR, H, capi.SAMPLER_PHILOX, 500 + 3 * p)["count"], int(m[p]), H, p_conf)
    print("n_run over the pairs:", dict(zip(*np.unique(want, return_counts=True))))
    assert want[3] == 0 and len(set(want.tolist()) - {0}) >= 3

    def new_batch():
        b = capi.Batch(ctx, P, N, 32)
        b.upload_intrinsics(0, Ks, global_index=np.arange(P) * 3)
        return b

    def run(b, name):
        getattr(b, name)(prm, uv1, uv2, m)
        b.sync()
        out = b.download()
        for k in ("R", "t", "R1to2", "t1to2"):   # (the 8-point stage leaves the pose of a pair without a model as it was)
            out["results"][k][out["results"]["valid"] == 0] = 0.0
        return out

    def key(out):
        return {k: out[k].tobytes() for k in _DOWNLOAD_KEYS}

    b = new_batch()
    with pytest.raises(capi.MvsError) as e:
        b.hypotheses_run()                   # no five-point call on this batch yet
    assert e.value.status == capi.MVS_ERR_INVALID_ARG
    b.close()
    fresh = {}
    conf(p_conf)
    for name in ("run_points", "run_points_essential"):
        b = new_batch()
        fresh[name] = run(b, name)
        if name == "run_points_essential":
            assert np.array_equal(b.hypotheses_run(), want)
        b.close()
    out = fresh["run_points_essential"]
    # every pair: the single call under the same setting, its n_run included
    for p in range(P):
        prm1 = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=500 + 3 * p, max_error_sq=THR)
        one = ctx.two_view_essential(uv1[p, :m[p]], uv2[p, :m[p]], Ks[p], prm1)
        assert one["hypotheses_run"] == want[p], p
        assert out["results"][p].tobytes() == one["raw"], p
        assert np.array_equal(out["mask"][p][:m[p]], one["mask"]), p
        n = int(out["results"][p]["n_points"]) if out["results"][p]["valid"] else 0
        assert out["points"][p][:n].tobytes() == one["points"].tobytes(), p
        assert np.array_equal(out["point_idx"][p][:n], one["point_idx"]), p
        assert not out["mask"][p][m[p]:].any() and not out["points"][p][n:].any()
    # two runs, and the two estimators in turn on one batch: each its fresh-batch bytes
    b = new_batch()
    for name in ("run_points_essential", "run_points_essential", "run_points", "run_points_essential", "run_points"):
        assert key(run(b, name)) == key(fresh[name]), name
        if name == "run_points_essential":
            assert np.array_equal(b.hypotheses_run(), want)
    # and with the rule off the same batch runs every hypothesis again
    conf(0.0)
    run(b, "run_points_essential")
    assert np.array_equal(b.hypotheses_run(), np.where(m >= 8, H, 0))
    # the accessor speaks of the LAST call: pairs it did not reach read 0, with the rule off and on
    for p_level in (0.0, p_conf):
        conf(p_level)
        b.run_points_essential(prm, uv1[:10], uv2[:10], m[:10])
        got = b.hypotheses_run()
        assert np.array_equal(got[:10], want[:10] if p_level else np.where(m[:10] >= 8, H, 0)) and not got[10:].any()
    b.close()


@pytest.mark.gpu
def test_n_run_is_the_word_the_selection_leaves_on_the_device(ctx, conf):
    """With or without a confidence level hypotheses_run() reads what the last call's selection wrote: a call without one, on
    fewer pairs, after a call with one -- every hypothesis for eight matches or more, 0 below, and 0 (not the earlier call's
    checkpoint) for the pairs it did not reach.  H = 65 is two checkpoints, 64 and 65."""
    P, N, H, seed = 6, 16, 65, 500
    m = np.array([0, 7, 8, 9, 11, 16], dtype=np.int32)
    fams = list(helpers.CAMERAS)
    Ks = np.stack([helpers.CAMERAS[fams[p % len(fams)]][0] for p in range(P)])
    uv1, uv2 = np.zeros((P, N, 2)), np.zeros((P, N, 2))
    for p in range(P):
        a, b2 = scene(5000 + p, N, 0.2)
        h = lambda q: np.hstack([q, np.ones((N, 1))]) @ Ks[p].T   # noqa: E731
        uv1[p], uv2[p] = h(a)[:, :2], h(b2)[:, :2]
        uv1[p, m[p]:], uv2[p, m[p]:] = 0.0, 0.0
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=seed, max_error_sq=THR)
    b = capi.Batch(ctx, P, N, 32)
    try:
        b.upload_intrinsics(0, Ks, global_index=np.arange(P) * 3)
        conf(0.99)
        b.run_points_essential(prm, uv1, uv2, m)
        first = b.hypotheses_run()
        conf(0.0)
        b.run_points_essential(prm, uv1[:4], uv2[:4], m[:4])
        b.sync()
        run, (n_roots, count), out = b.hypotheses_run(), b.download_essential_tables(H), b.download()
    finally:
        b.close()
    assert not first[:2].any() and (first[2:] >= BLOCK).all(), first      # (words the second call must not hand back)
    assert run.tolist() == [0, 0, 65, 65, 0, 0]
    for p in (2, 3):
        n1, n2 = o.normalize_points(Ks[p], uv1[p, :m[p]]), o.normalize_points(Ks[p], uv2[p, :m[p]])
        ref = em.host_ransac(n1, n2, THR, H, capi.SAMPLER_PHILOX, seed + 3 * p)
        assert np.array_equal(n_roots[p], ref["n_roots"]) and np.array_equal(count[p], ref["count"]), p
        r = out["results"][p]
        assert (r["best_hyp"], r["best_count"]) == (ref["best_hyp"], ref["best_count"]), p
        assert np.float64(r["best_residual"]).tobytes() == np.float64(ref["best_residual"]).tobytes(), p
        assert r["E"].tobytes() == ref["E"].tobytes() and r["F"].tobytes() == ref["E"].tobytes(), p
        assert np.array_equal(out["mask"][p][:m[p]], ref["mask"]) and not out["mask"][p][m[p]:].any(), p


@pytest.mark.gpu
def test_sfm_solve_cube_through_the_shim_with_a_confidence_level():
    deps = [SHIM_SRC, SHIM, os.path.join(ROOT, "include", "mvslam_hip.h")]
    if not os.path.exists(SHIM_EXE) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_EXE) for d in deps):
        _build_shim()
    p = subprocess.run([SHIM_EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and "ALL PASSED five-point" in out, out
