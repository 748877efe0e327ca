"""CPU side of the descriptor-fed five-point entry points (mvs_image_pair_essential, mvs_batch_run_essential,
mvs_seq_run_essential and their accessors): the exported surface and the shim's MVSLAM_ESSENTIAL_ONE_PASS.  The GPU side is
tests/test_essential_paths_gpu.py; the kernels' resources are checked in tests/test_five_point_host.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mvslam_amd", "lib")
HEADER = os.path.join(ROOT, "include", "mvslam_hip.h")
SHIM = os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp")
SRC = os.path.join(ROOT, "tests", "cpp", "image_pair_one_pass.cpp")

NEW_SYMBOLS = ["mvs_image_pair_essential", "mvs_batch_run_essential", "mvs_batch_download_essential_tables",
               "mvs_seq_run_essential", "mvs_seq_download_hypotheses_run", "mvs_batch_download_hypotheses_run"]

ONE_PASS_FLAGS = {"one_pass": ["-DMVSLAM_USE_ESSENTIAL_5POINT", "-DMVSLAM_ESSENTIAL_ONE_PASS"],
                  "two_calls": ["-DMVSLAM_USE_ESSENTIAL_5POINT"], "eight_point": []}


def one_pass_exe(kind):
    return os.path.join(LIBDIR, "image_pair_one_pass_" + kind)


def build_one_pass(kind):
    assert os.path.exists(os.path.join(LIBDIR, "libmvslam_hip.so")), "build the HIP library first (__graft_entry__.build)"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *ONE_PASS_FLAGS[kind], "-o", one_pass_exe(kind), SRC,
                           "-L", LIBDIR, "-lmvslam_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib",
                           "-Wl,--allow-shlib-undefined"])


def test_the_library_exports_the_new_entry_points_and_the_header_declares_them():
    from mvslam_amd import capi

    lib = capi.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(mvs_[a-z0-9_]+)\s*\(", src))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert hasattr(lib, name) and name in capi.EXPORTS, name
    assert lib.mvs_abi_version() == 4
    assert re.search(r"^#define MVS_ABI_VERSION 4$", open(HEADER).read(), flags=re.M)
    for cls, method in ((capi.Context, "image_pair_essential"), (capi.Batch, "run_essential"),
                        (capi.Batch, "download_essential_tables"), (capi.Sequence, "run_essential"),
                        (capi.Sequence, "download_hypotheses_run")):
        assert callable(getattr(cls, method, None)), (cls.__name__, method)


def test_the_new_calls_refuse_null_handles_without_a_device():
    """the argument checks in front of any device work: no GPU needed to be told INVALID_ARG"""
    from mvslam_amd import capi

    lib = capi.lib()
    prm = capi.default_params(num_hypotheses=8)
    n = (C.c_int32 * 4)()
    assert lib.mvs_batch_run_essential(None, C.byref(prm), 1) == capi.MVS_ERR_INVALID_ARG
    assert lib.mvs_seq_run_essential(None, C.byref(prm), None) == capi.MVS_ERR_INVALID_ARG
    assert lib.mvs_seq_download_hypotheses_run(None, 0, 1, n) == capi.MVS_ERR_INVALID_ARG
    assert lib.mvs_batch_download_essential_tables(None, 0, 1, 8, n, n) == capi.MVS_ERR_INVALID_ARG
    assert lib.mvs_image_pair_essential(None, None, None, 0, None, None, 0, 32, None, C.byref(prm), None, None, None, None,
                                        None) == capi.MVS_ERR_INVALID_ARG


def _preprocessed(flags):
    out = subprocess.run(["g++", "-std=c++17", "-E", "-P", *flags, "-x", "c++", SHIM], stdout=subprocess.PIPE, check=True)
    text = out.stdout.decode()
    return text[text.index("namespace mvSLAM"):]    # past the C ABI header's declarations


def test_one_pass_macro_selects_the_one_call_and_alone_changes_nothing():
    both = _preprocessed(ONE_PASS_FLAGS["one_pass"])
    assert both.count("mvs_image_pair_essential(") == 1
    ctor = both[both.index("ImagePair(const Frame &base_frame_"):]
    ctor = ctor[:ctor.index("bool refine()")]
    assert "mvs_image_pair_essential(" in ctor and "mvs_match_hamming(" not in ctor and "mvs_two_view_essential(" not in ctor
    assert "mvs_image_pair(" not in both
    # without MVSLAM_USE_ESSENTIAL_5POINT the new macro means nothing, and without the new macro the header is what it was
    assert _preprocessed(["-DMVSLAM_ESSENTIAL_ONE_PASS"]) == _preprocessed([])
    five = _preprocessed(ONE_PASS_FLAGS["two_calls"])
    assert "mvs_image_pair_essential" not in five and "mvs_image_pair_essential" not in _preprocessed([])
    assert five.count("mvs_two_view_essential(") == 2 and five.count("mvs_match_hamming(") >= 1


@pytest.mark.parametrize("kind", list(ONE_PASS_FLAGS))
def test_the_one_pass_program_compiles_and_links(kind):
    build_one_pass(kind)
    assert os.path.exists(one_pass_exe(kind))
