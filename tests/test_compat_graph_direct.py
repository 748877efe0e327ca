"""The shim's switch for the pose graphs' linear solver (MVSLAM_POSE_GRAPH_SOLVER of mvslam_amd/compat/mvslam_compat.hpp;
DESIGN.md section 4.10.4): tests/cpp/test_compat_graph_direct.cpp, built the way tests/test_compat_graph.py builds its program,
once without the macro and once with -DMVSLAM_POSE_GRAPH_SOLVER=1.  GraphOptimizer::optimize on a graph of 24 nodes goes
through the PCG in the one and through the direct solver in the other, and the poses agree within the bound of
tests/test_pg_direct.py (1e-9 on the se3 coordinates: both answers are within it of the exact minimiser)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mvslam_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "test_compat_graph_direct.cpp")
TOL = 1e-9


def _run(tag, defs):
    exe = os.path.join(LIBDIR, "test_compat_graph_direct_" + tag)
    deps = [SRC, os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp"), os.path.join(ROOT, "include", "mvslam_hip.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        assert os.path.exists(os.path.join(LIBDIR, "libmvslam_hip.so")), "build the HIP library first (__graft_entry__.build)"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + defs + ["-o", exe, SRC, "-L", LIBDIR,
                               "-lmvslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib",
                               "-Wl,--allow-shlib-undefined"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    head = out.splitlines()[0].split()
    poses = np.array([[float(x) for x in line.split()[1:]] for line in out.splitlines() if line.startswith("pose")])
    return int(head[1]), int(head[3]), poses


def test_graph_optimizer_under_both_solvers():
    s0, cg0, p0 = _run("pcg", [])
    s1, cg1, p1 = _run("direct", ["-DMVSLAM_POSE_GRAPH_SOLVER=1"])
    assert (s0, s1) == (0, 1) and cg0 > 0 and cg1 == 0
    assert p0.shape == p1.shape == (24, 6)
    gap = float(np.abs(p0 - p1).max())
    print("GraphOptimizer, PCG against direct: largest se3 coordinate difference %.3e (bound %.1e)" % (gap, TOL))
    assert gap <= TOL
