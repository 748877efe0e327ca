"""ba_frame_pose_and_point through the drop-in shim under MVSLAM_BA_LOSS: tests/cpp/
test_compat_ba_sparse.cpp, the driver of tests/test_compat_ba_sparse.py as it is, compiled once with -DMVSLAM_BA_LOSS=1
-DMVSLAM_BA_LOSS_K=1.345 and once without.  On a five-frame problem with planted outliers the first equals
mvs_ba_refine_sparse under Huber -- with a loss every frame set goes through the sparse entry --, the second today's window
result.  The driver prints %.17g and reads repr(): both directions are exact: the cost must be equal bit for bit, the arrays
to the last bits (_same says why not more).  Compiling and linking is a CPU test; running needs the GPU."""
import os
import subprocess

import numpy as np
import pytest

import ba_robust_model as rm
import ba_sparse_model as bm
from test_compat_ba_sparse import SRC, ROOT, _write_problem

LIBDIR = os.path.join(ROOT, "mvslam_amd", "lib")
EXE = {True: os.path.join(LIBDIR, "test_compat_ba_robust_huber"), False: os.path.join(LIBDIR, "test_compat_ba_robust_none")}


def _build(robust):
    assert os.path.exists(os.path.join(LIBDIR, "libmvslam_hip.so")), "build the HIP library first (__graft_entry__.build)"
    defs = ["-DMVSLAM_BA_LOSS=1", "-DMVSLAM_BA_LOSS_K=%r" % rm.HUBER_K] if robust else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + defs + ["-o", EXE[robust], SRC, "-L", LIBDIR,
                           "-lmvslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined"])


def _fixture():
    """five frames, 60 points on tracks of 2 .. 5 frames, outliers planted as in the F = 9 and F = 24 fixtures; the ids ascend
    with the indices, so that the shim's sorted packing is the direct call's order and the two sum in the same order"""
    pb, planted = rm.plant_outliers(bm.sparse_problem(5, 5, 60, single_obs_point=False), 1005, frac=0.08)
    assert planted.sum() >= 5
    c = pb["csr"]
    F, m = 5, 60
    g = dict(K=pb["K"], poses=pb["poses"], var=pb["var"], Xg=pb["Xg"], pcov=pb["pcov"], obs_off=c["obs_off"], obs_frame=c["obs_frame"],
             obs_uv=c["obs_uv"], obs_cov=c["obs_cov"], frame_ids=100 + 3 * np.arange(F), point_ids=1000 + 7 * np.arange(m),
             obs_order=np.random.default_rng(5).permutation(len(c["obs_frame"])))
    return pb, g


def test_compat_ba_robust_compiles_and_links_with_host_compiler():
    for robust in (True, False):
        _build(robust)
        assert os.path.exists(EXE[robust])


def _run(exe, path, g):
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    frames, points, error = {}, {}, None
    for ln in out.splitlines():
        w = ln.split()
        if w[0] == "error":
            error = float(w[1])
        elif w[0] == "frame":
            frames[int(w[1])] = np.array(w[2:], float)
        elif w[0] == "point":
            points[int(w[1])] = np.array(w[2:], float)
    fr = np.stack([frames[int(i)] for i in g["frame_ids"]])
    pt = np.stack([points[int(i)] for i in g["point_ids"]])
    return error, fr, pt


@pytest.mark.gpu
def test_compat_ba_frame_pose_and_point_under_huber_and_without(ctx, tmp_path):
    from mvslam_amd import capi

    deps = [SRC, os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp"), os.path.join(ROOT, "include", "mvslam_hip.h")]
    for robust in (True, False):
        if not os.path.exists(EXE[robust]) or any(os.path.getmtime(d) > os.path.getmtime(EXE[robust]) for d in deps):
            _build(robust)
    pb, g = _fixture()
    path = str(tmp_path / "problem.txt")
    _write_problem(g, path)
    # with the macros: the sparse entry under Huber
    ctx.set_ba_loss(capi.MVS_BA_LOSS_HUBER, rm.HUBER_K)
    try:
        want = ctx.ba_refine_sparse(**bm.sparse_args(pb))
    finally:
        ctx.set_ba_loss(capi.MVS_BA_LOSS_NONE)
    none = ctx.ba_refine_sparse(**bm.sparse_args(pb))
    assert want["ok"] and none["ok"] and want["raw"] != none["raw"]
    assert np.abs(want["points"] - none["points"]).max() > 1e-6   # the loss moves the estimate: the routes can be told apart
    error, fr, pt = _run(EXE[True], path, g)
    _same("huber", error, fr, pt, want, pose_cov=True)
    # without: five frames go through the window kernel, as they did
    win = ctx.ba_refine_windows([bm.as_window(pb)])[0]
    error, fr, pt = _run(EXE[False], path, g)
    assert win["ok"]
    _same("window", error, fr, pt, win, pose_cov=False)


def _same(tag, error, fr, pt, want, pose_cov):
    """the cost bit for bit; the arrays to 1e-13 of their largest entry: they come back through the reference's classes (the
    rotation through SO3's constructor, which rectifies it again, the covariances through their symmetric types), which may
    move the last bits and nothing else.  The two routes that are compared differ by far more (asserted above)."""
    assert error == want["error"], tag
    pairs = [(fr[:, :9].reshape(5, 3, 3), want["R"]), (fr[:, 9:12], want["t"]), (pt[:, :3], want["points"]),
             (pt[:, 3:].reshape(-1, 3, 3), want["point_cov"])]
    if pose_cov:
        pairs.append((fr[:, 12:].reshape(5, 6, 6), want["pose_cov"]))
    d = [np.abs(a - b).max() / np.abs(b).max() for a, b in pairs]
    print(tag, ["%.1e" % v for v in d])
    assert max(d) <= 1e-13, (tag, d)
