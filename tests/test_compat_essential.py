"""The reference's sfm_solve_cube (test/test-sfm.cpp:17-90) through the drop-in shim, tests/cpp/test_compat_essential.cpp built
twice: with MVSLAM_USE_ESSENTIAL_5POINT sfm_solve forwards to the five-point RANSAC and the reference's assertions pass; without
the macro the same translation unit is the 8-point path (the header preprocesses to what it was); in both builds sfm_solve
returns, bit for bit, the pose of the C ABI entry it is meant to forward to.  Compiling + linking is a CPU test; running needs the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mvslam_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "test_compat_essential.cpp")
SHIM = os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp")


def _exe(five):
    return os.path.join(LIBDIR, "test_compat_essential_5pt" if five else "test_compat_essential_8pt")


def _build(five):
    assert os.path.exists(os.path.join(LIBDIR, "libmvslam_hip.so")), "build the HIP library first (__graft_entry__.build)"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *(["-DMVSLAM_USE_ESSENTIAL_5POINT"] if five else []),
                           "-o", _exe(five), SRC, "-L", LIBDIR, "-lmvslam_hip", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])


@pytest.mark.parametrize("five", [True, False], ids=["five_point", "eight_point"])
def test_compat_essential_compiles_and_links(five):
    _build(five)
    assert os.path.exists(_exe(five))


def test_the_macro_selects_the_entry_point():
    """undefined, the shim never names the five-point entries; defined, sfm_solve and ImagePair call mvs_two_view_essential"""
    def pre(flags):
        out = subprocess.run(["g++", "-std=c++17", "-E", "-P", *flags, "-x", "c++", SHIM], stdout=subprocess.PIPE, check=True)
        text = out.stdout.decode()
        return text[text.index("namespace mvSLAM"):]    # past the C ABI header's declarations
    off, on = pre([]), pre(["-DMVSLAM_USE_ESSENTIAL_5POINT"])
    assert "mvs_two_view_essential" not in off and "mvs_two_view(" in off and "mvs_image_pair(" in off
    assert on.count("mvs_two_view_essential(") == 2 and "mvs_two_view(" not in on and "mvs_image_pair(" not in on


@pytest.mark.gpu
@pytest.mark.parametrize("five", [True, False], ids=["five_point", "eight_point"])
def test_sfm_solve_cube_through_the_shim(five):
    deps = [SRC, SHIM, os.path.join(ROOT, "include", "mvslam_hip.h")]
    exe = _exe(five)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        _build(five)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and ("ALL PASSED five-point" if five else "ALL PASSED eight-point") in out, out
