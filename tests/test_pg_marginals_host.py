"""CPU tests of the pose-graph marginals: the numpy model (tests/pg_marginals_model.py) against the
dense inverse, the envelope counts, the exported surface, and the host side of the library (mvslam_amd/csrc/pg_envelope.hpp)
under the address and undefined-behaviour sanitizers in a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

import pg_marginals_model as mm
import posegraph_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(mm.FIXTURES))
def test_skyline_restatement_equals_the_dense_inverse(name):
    """both float64 methods against the extended-precision inverse.  They share the conditioning of H, so the skyline
    restatement has to stay within the margin the device is given against it (8 x, floor 64 ulp) of numpy.linalg.inv, and the
    reference has to solve H X = I to far below either."""
    g = mm.FIXTURES[name]()
    N = g["node_pose"].shape[0]
    first, row_off, blocks = mm.graph_envelope(g)
    H = mm.dense_h(g)
    queries = mm.all_pairs(N)
    e_inv, e_sky, S_ref = mm.host_errors(H, first, queries)
    resid = np.abs(np.eye(6 * N) - H.astype(np.longdouble) @ S_ref.astype(np.longdouble)).max()
    print("%s: inv %.3e, skyline %.3e, |I - H S_ref| %.3e, envelope %d" % (name, e_inv, e_sky, float(resid), blocks))
    assert e_sky <= mm.bound(e_inv, 0.0)
    # S_ref is rounded to float64 once: the residual of the rounded inverse is at most cond(H)-free |H| |S| eps per entry
    assert float(resid) <= 8 * mm.EPS * float((np.abs(H) @ np.abs(S_ref)).max())
    assert row_off[-1] == blocks and all(first[i] <= i for i in range(N))
    # the factor itself: L L^T = H inside the envelope, zero outside
    rows, _ = mm.skyline_factor(H, first)
    L = np.zeros_like(H)
    for i, row in enumerate(rows):
        for c in range(int(first[i]), i + 1):
            B = row[c - int(first[i])].copy()
            if c == i:
                B[np.diag_indices(6)] = 1.0 / np.diag(B)
            L[6 * i:6 * i + 6, 6 * c:6 * c + 6] = B
    assert np.abs(L @ L.T - H).max() <= 64 * mm.EPS * np.abs(H).max() * N


def test_envelope_counts():
    for n in (1, 2, 9, 40):
        src, dst = np.arange(n - 1), np.arange(1, n)
        assert mm.envelope(n, src, dst)[2] == 2 * n - 1
        assert mm.envelope(n, dst, src)[2] == 2 * n - 1
    g = pm.star(70)
    assert mm.graph_envelope(g)[2] == 71 * 72 // 2 and (mm.graph_envelope(g)[0] == 0).all()
    first, _, blocks = mm.graph_envelope(mm.chain40())
    assert first[39] == 0 and first[34] == 5 and blocks == 79 + 38 + 28
    assert mm.envelope(4096, np.zeros(4095, dtype=int), np.arange(1, 4096))[2] > mm.MAX_ENVELOPE_BLOCKS
    ring = pm.ring(24, chords=(2,))
    assert mm.graph_envelope(ring)[2] != mm.graph_envelope(mm.FIXTURES["ring24_relabelled"]())[2]


def test_exports_equal_the_header():
    from mvslam_amd import capi

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvslam_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mvs_[a-z0-9_]+)\s*\(", src)))
    assert sorted(capi.EXPORTS) == declared
    lib = capi.lib()
    for name in ("mvs_pose_graph_marginals", "mvs_seq_pose_graph_marginals"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert lib.mvs_abi_version() == 4
    assert capi.POSE_GRAPH_MARGINALS_INFO_DTYPE.itemsize == 24
    assert capi.POSE_GRAPH_MAX_ENVELOPE_BLOCKS == mm.MAX_ENVELOPE_BLOCKS


def test_info_layout_matches_the_header(tmp_path):
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(mvs_pose_graph_marginals_info), offsetof(mvs_pose_graph_marginals_info, ok),
         offsetof(mvs_pose_graph_marginals_info, envelope_blocks), offsetof(mvs_pose_graph_marginals_info, bad_node),
         offsetof(mvs_pose_graph_marginals_info, min_pivot));
  return 0; }
'''
    (tmp_path / "p.c").write_text(probe)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "p"), str(tmp_path / "p.c")])
    v = list(map(int, subprocess.check_output([str(tmp_path / "p")]).decode().split()))
    dt = capi.POSE_GRAPH_MARGINALS_INFO_DTYPE
    assert v == [dt.itemsize] + [dt.fields[k][1] for k in ("ok", "envelope_blocks", "bad_node", "min_pivot")]


def test_host_side_under_the_sanitizers(tmp_path):
    """tests/cpp/pg_envelope_check.cpp: N = 1, a chain, the star, the 4096-node hub, a query list of length 0 and one a query
    longer than a chunk, with -fsanitize=address,undefined.  A program of its own: nothing of it is loaded into python."""
    exe = str(tmp_path / "pg_envelope_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mvslam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pg_envelope_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip() == "ok"
