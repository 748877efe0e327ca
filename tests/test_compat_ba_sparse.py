"""ba_frame_pose_and_point on twelve frames through the drop-in shim (tests/cpp/test_compat_ba_sparse.cpp): from nine frames on
the shim packs the reference's maps into an mvs_ba_sparse and calls mvs_ba_refine_sparse.  The problem
and the block model's estimate of it are the fixture tests/golden/ba_sparse_12.npz (tests/ba_sparse_model.py writes it); the
estimate that comes back through the maps is held to the bounds of tests/test_ba_sparse.py at more than eight frames
(BOUND_WIDE), the cost to 1e-9 relative.  Compiling and linking is a CPU test; running needs the GPU."""
import os
import subprocess

import numpy as np
import pytest

from test_ba_sparse_host import BOUND_WIDE
from test_ba_window import _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mvslam_amd", "lib", "test_compat_ba_sparse")
SRC = os.path.join(ROOT, "tests", "cpp", "test_compat_ba_sparse.cpp")


def _build():
    libdir = os.path.join(ROOT, "mvslam_amd", "lib")
    assert os.path.exists(os.path.join(libdir, "libmvslam_hip.so")), "build the HIP library first (__graft_entry__.build)"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", EXE, SRC, "-L", libdir, "-lmvslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])


def _write_problem(g, path):
    """the fixture as the driver's text input: ids instead of indices, the observations in the fixture's shuffled order"""
    F, m = len(g["poses"]), len(g["Xg"])
    fmt = lambda v: " ".join(repr(float(x)) for x in np.asarray(v).ravel())
    point_of = np.repeat(np.arange(m), np.diff(g["obs_off"]))
    with open(path, "w") as f:
        f.write("%d %d %d\n%s\n" % (F, m, len(g["obs_frame"]), fmt(g["K"])))
        for i in range(F):
            has = bool((g["var"][i] > 0).any())
            f.write("%d %s %d %s\n" % (g["frame_ids"][i], fmt(g["poses"][i]), has, fmt(g["var"][i])))
        for i in reversed(range(m)):
            f.write("%d %s %d %s\n" % (g["point_ids"][i], fmt(g["Xg"][i]), g["pcov"][i][0] > 0, fmt(g["pcov"][i])))
        for o in g["obs_order"]:
            f.write("%d %d %s %s\n" % (g["frame_ids"][g["obs_frame"][o]], g["point_ids"][point_of[o]], fmt(g["obs_uv"][o]),
                                       fmt(g["obs_cov"][o])))


def test_compat_ba_sparse_compiles_and_links_with_host_compiler():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_compat_ba_frame_pose_and_point_on_twelve_frames(tmp_path):
    deps = [SRC, os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp"), os.path.join(ROOT, "include", "mvslam_hip.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        _build()
    g = np.load(os.path.join(ROOT, "tests", "golden", "ba_sparse_12.npz"))
    F, m = len(g["poses"]), len(g["Xg"])
    path = str(tmp_path / "problem.txt")
    _write_problem(g, path)
    p = subprocess.run([EXE, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
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
    assert sorted(frames) == sorted(g["frame_ids"]) and sorted(points) == sorted(g["point_ids"])
    fr = np.stack([frames[int(i)] for i in g["frame_ids"]])
    pt = np.stack([points[int(i)] for i in g["point_ids"]])
    d = dict(R=np.abs(fr[:, :9].reshape(F, 3, 3) - g["R"]).max(), t=np.abs(fr[:, 9:12] - g["t"]).max(),
             points=np.abs(pt[:, :3] - g["points"]).max(),
             pose_cov=max(_rel(fr[f, 12:].reshape(6, 6), g["pose_cov"][f]) for f in range(F)),
             point_cov=_rel(pt[:, 3:].reshape(m, 3, 3), g["point_cov"]))
    cost = abs(error - float(g["error"])) / float(g["error"])
    print("shim, 12 frames: cost %.2e %s" % (cost, {k: "%.2e" % v for k, v in d.items()}))
    assert cost <= 1e-9
    for k, v in d.items():
        assert v <= BOUND_WIDE[k], (k, v, BOUND_WIDE[k])
