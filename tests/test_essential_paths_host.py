"""CPU side of the descriptor-fed five-point entry points (mvs_image_pair_essential, mvs_batch_run_essential,
mvs_seq_run_essential and their accessors): the exported surface, the resources of the four-wavefront solve + count kernel, and
the shim's MVSLAM_ESSENTIAL_ONE_PASS.  The GPU side is tests/test_essential_paths_gpu.py.

The kernel is named e5wide_solve_count_kernel: a name holding "e5_" would be counted by
tests/test_essential5_confidence.py::test_new_kernels_need_no_scratch_and_the_horizon_kernel_no_lds, which expects exactly three
such kernels, as a name holding "essential5" would be by tests/test_five_point_host.py."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mvslam_amd", "lib")
HEADER = os.path.join(ROOT, "include", "mvslam_hip.h")
SHIM = os.path.join(ROOT, "mvslam_amd", "compat", "mvslam_compat.hpp")
SRC = os.path.join(ROOT, "tests", "cpp", "image_pair_one_pass.cpp")
CSRC = os.path.join(ROOT, "mvslam_amd", "csrc")

NEW_SYMBOLS = ["mvs_image_pair_essential", "mvs_batch_run_essential", "mvs_batch_download_essential_tables",
               "mvs_seq_run_essential", "mvs_seq_download_hypotheses_run", "mvs_batch_download_hypotheses_run"]
WIDE = "e5wide_solve_count_kernel"
CU_LDS_BYTES = 163840

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


def _constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, name
    return int(m.group(1))


def test_the_wide_kernel_spills_nothing_and_fits_the_lds_of_a_cu():
    path = os.path.join(LIBDIR, "kernel_resources.json")
    assert os.path.exists(path), "kernel_resources.json is missing: build the library first"
    digest = json.load(open(path))
    mine = {k: v for k, v in digest.items() if WIDE in k}
    assert len(mine) == 1, list(mine)
    v = next(iter(mine.values()))
    assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, v
    # dynamic LDS as essential5.hip sizes it: the solver's workspace of 64 lanes + [4 wavefronts][10 roots][64 lanes] int32
    hdr = open(os.path.join(CSRC, "five_point.hpp")).read() + open(os.path.join(CSRC, "kernels.hpp")).read()
    src = open(os.path.join(CSRC, "essential5.hip")).read()
    ws, roots, lanes = _constant(hdr, "kE5Ws"), _constant(hdr, "kE5MaxRoots"), _constant(hdr, "kE5HypPerBlock")
    waves = _constant(src, "kE5WideWaves")
    dynamic = ws * lanes * 8 + waves * roots * lanes * 4
    assert dynamic == 141312 + 10240
    assert v["static_lds_bytes"] + dynamic <= CU_LDS_BYTES, (v, dynamic)
    # the kernels of a call without a confidence level are still the three they were
    plain = [k for k in digest if "essential5" in k or "five_point_kernel" in k]
    assert len(plain) == 3, plain


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
