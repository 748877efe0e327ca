"""Builds and runs the C++ test of the back end's drop-in surface (tests/cpp/test_compat_graph.cpp): mvSLAM::Graph and
mvSLAM::GraphOptimizer of the shim on mvs_pose_graph_optimize -- id monotonicity, the optimiser working on a copy, the two
scenarios of the reference's test/test-graph.cpp at its tolerances.  Driven the way tests/test_compat_cpp.py drives its
program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mvslam_amd", "lib")
EXE = os.path.join(LIBDIR, "test_compat_graph")
SRC = os.path.join(ROOT, "tests", "cpp", "test_compat_graph.cpp")


def _build():
    assert os.path.exists(os.path.join(LIBDIR, "libmvslam_hip.so")), "build the HIP library first (__graft_entry__.build)"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", EXE, SRC, "-L", LIBDIR, "-lmvslam_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])


def test_compat_graph_cpp_suite():
    deps = [SRC, os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp"), os.path.join(ROOT, "include", "mvslam_hip.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        _build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and "ALL PASSED" in out, out
