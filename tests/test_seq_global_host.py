"""The global problem of a resident sequence, CPU part (mvs_seq_refine_global).

The numpy model (tests/seq_global_model.py) on a hand-written link table; its CSR through mvs_bas::check_csr and
mvs_bas::plan (tests/cpp/ba_envelope_dump.cpp as it stands, under the host sanitizers) and the gap-free shortcuts of the
device's plan against both that and the brute-force plan of tests/ba_sparse_model.py; the host's own decisions
(mvslam_amd/csrc/seq_global_host.hpp) from a stand-alone program under the host sanitizers; the sequences the GPU tests use,
shown on the oracle's pairs alone to exercise what those tests are about; the header / ctypes layout of the new struct and the
new symbols; the new kernels in the build's digest.
"""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import ba_sparse_model as bm
import oracle_lib as o
import seq_global_model as gm
import test_seq_windows as sw
import test_sequence as ts
from mvslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sequences of tests/test_seq_global.py: test_seq_windows' six frames of 300 keypoints (300 crosses the 256-keypoint chunk
# and a wavefront edge), its first three frames, and 260 frames of 96 keypoints, which cross the 256-frame chunk of the scans
SEQ_ARGS = sw.SEQ_ARGS
LONG_FRAMES = 260
LONG_ARGS = dict(n_kp=96, n_map=1000, noise_px=0.3, step=0.05)
LONG_T = 8


def _hand_pairs():
    """six frames of eight keypoints.  Chains (keypoint per frame): A 0-0-0-0-0 over frames 0 .. 4, triangulated only by its
    third link (pair 2); B 1-1-1 triangulated only by its second link; C 2-3-3-3 never triangulated; H 6-6 triangulated by
    pair 0; E starts at (frame 1, kp 2) because the row of pair 0 that leads there shares trainIdx 0 with an earlier row and is
    dropped; D starts at (1, 5); G starts in the last-but-one frame, at (4, 4); row 4 of pair 0 is no inlier."""
    def pair(k, rows, mask, point_idx):
        mt = np.zeros(len(rows), dtype=o.MATCH_DTYPE)
        mt["trainIdx"], mt["queryIdx"] = [r[0] for r in rows], [r[1] for r in rows]
        n = len(point_idx)
        return dict(valid=True, matches=mt, mask=np.array(mask, np.uint8), point_idx=np.array(point_idx, np.int64),
                    points=np.arange(3.0 * n).reshape(n, 3) + 100.0 * k + 1.0)

    return [pair(0, [(0, 0), (1, 1), (0, 2), (2, 3), (3, 4), (6, 6)], [1, 1, 1, 1, 0, 1], [5]),
            pair(1, [(1, 1), (0, 0), (3, 3), (5, 5), (2, 6)], [1, 1, 1, 1, 1], [0, 3, 4]),
            pair(2, [(0, 0), (5, 5), (3, 3)], [1, 1, 1], [0]),
            pair(3, [(0, 0)], [1], []),
            pair(4, [(4, 4)], [1], [0])]


def _hand_traj():
    R = np.stack([Rot.from_rotvec([0.1 * k, -0.2, 0.05 * k]).as_matrix() for k in range(6)])
    return dict(R=R, t=np.arange(18.0).reshape(6, 3) * 0.1, pair_scale=np.array([1.0, 1.25, 0.75, 0.5, 2.0]))


def _tracks(g):
    """[(head frame, [keypoints])] of a model problem"""
    return [(int(g["head_frame"][p]), g["obs_kp"][g["obs_off"][p]:g["obs_off"][p + 1]].tolist())
            for p in range(len(g["head_frame"]))]


def test_build_global_on_a_hand_written_link_table():
    pairs, traj = _hand_pairs(), _hand_traj()
    gs = lambda k, j: traj["R"][k] @ (traj["pair_scale"][k] * pairs[k]["points"][j]) + traj["t"][k]
    g = gm.build_global(pairs, traj, 8, 0)
    assert g["depth"][:, 0].tolist() == [0, 1, 2, 3, 4, 0] and g["depth"][1, 2] == 0   # the twin's loser starts a chain
    assert g["depth"][3, 3] == 3 and g["longest_chain"] == 5
    #                           A                     B (2nd link)    H            E            D               G (last but one)
    assert _tracks(g) == [(0, [0, 0, 0, 0, 0]), (0, [1, 1, 1]), (0, [6, 6]), (1, [2, 6]), (1, [5, 5, 5]), (4, [4, 4])]
    assert np.array_equal(g["point_guess"], np.stack([gs(2, 0), gs(1, 0), gs(0, 0), gs(1, 2), gs(1, 1), gs(4, 0)]))
    assert g["tri_link"].tolist() == [2, 1, 0, 0, 0, 0]
    assert g["obs_off"].tolist() == [0, 5, 8, 10, 12, 15, 17]
    assert g["obs_frame"].tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 0, 1, 1, 2, 1, 2, 3, 4, 5]
    # T = 2: A's piece over frames 0, 1 holds no triangulated link (it lies in the next piece) and is no point; the piece over
    # frames 2, 3 is; frame 4's keypoint has no link out and is no head.  B's only piece with a link is not triangulated.
    g2 = gm.build_global(pairs, traj, 8, 2)
    assert _tracks(g2) == [(0, [6, 6]), (1, [2, 6]), (1, [5, 5]), (2, [0, 0]), (4, [4, 4])]
    assert np.array_equal(g2["point_guess"], np.stack([gs(0, 0), gs(1, 2), gs(1, 1), gs(2, 0), gs(4, 0)]))
    # T = 3: A's triangulated link joins depth 2 to depth 3, which is the cut: neither piece is a point
    g3 = gm.build_global(pairs, traj, 8, 3)
    assert _tracks(g3) == [(0, [1, 1, 1]), (0, [6, 6]), (1, [2, 6]), (1, [5, 5, 5]), (4, [4, 4])]
    assert g3["tri_link"].tolist() == [1, 0, 0, 0, 0]
    # an invalid pair in the middle ends every chain there: A's first half has no triangulated link, its second half starts
    # again at depth 0 in frame 3 and has none either; D loses its last frame
    bad = [dict(p) for p in pairs]
    bad[2]["valid"] = False
    gb = gm.build_global(bad, traj, 8, 0)
    assert gb["depth"][3].tolist() == [0] * 8 and gb["depth"][4, 0] == 1
    assert _tracks(gb) == [(0, [1, 1, 1]), (0, [6, 6]), (1, [2, 6]), (1, [5, 5]), (4, [4, 4])]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return gm.compile_planner(tmp_path_factory.mktemp("seq_global_plan"))


@pytest.fixture(scope="module")
def oracle_pairs():
    """the oracle's pairs of the GPU tests' sequences, computed once"""
    out = {}
    for name, F, args in (("six", 6, SEQ_ARGS), ("long", LONG_FRAMES, LONG_ARGS)):
        seq = synth.make_sequence(F, **args)
        pairs, _ = ts.oracle_sequence(seq, sw.PRM, sw.PPRM, threads=4)
        out[name] = (seq, [dict(p, valid=p["ok"]) for p in pairs])
    return out


def _eye(F):
    return dict(R=np.tile(np.eye(3), (F, 1, 1)), t=np.zeros((F, 3)), pair_scale=np.ones(F - 1))


def _check_plans(planner, F, g):
    off, fr = g["obs_off"].tolist(), g["obs_frame"].tolist()
    want = planner(F, off, fr)
    assert want["check"] == [0] and want["fits"] == [1]
    mine = gm.plan_gap_free(F, g["obs_off"], g["obs_frame"], g["head_frame"])
    for k in gm.PLAN_LISTS + ("blocks", "pairs", "widest"):
        assert mine[k] == want[k], k
    first, pairs, by_frame = bm.brute_plan(F, off, fr)
    assert mine["first"] == first and mine["fr_obs"] == [x for b in by_frame for x in b]
    po, pa, pc, ro = mine["pair_off"], mine["pair_a"], mine["pair_c"], mine["row_off"]
    for i in range(F):
        for j in range(first[i], i + 1):
            b = ro[i] + j - first[i]
            assert list(zip(pa[po[b]:po[b + 1]], pc[po[b]:po[b + 1]])) == pairs.get((i, j), []), (i, j)
    return want


@pytest.mark.parametrize("T", [0, 2, 3])
def test_model_csr_passes_check_csr_and_gap_free_plan_is_the_plan(planner, oracle_pairs, T):
    """mvs_bas::check_csr accepts the model's CSR, and the gap-free shortcuts give mvs_bas::plan's lists and the brute-force
    plan's, on the hand-written table and on the six-frame sequence"""
    g = gm.build_global(_hand_pairs(), _hand_traj(), 8, T)
    _check_plans(planner, 6, g)
    seq, pairs = oracle_pairs["six"]
    g = gm.build_global(pairs, _eye(6), 300, T)
    want = _check_plans(planner, 6, g)
    assert want["widest"] == [min(T, 6) if T else g["longest_chain"]]


def test_generators_give_what_the_gpu_tests_are_about(oracle_pairs):
    """on the oracle's pairs alone.  Six frames of 300 keypoints: 5 of 5 pairs valid, 301 points and 1004 observations uncut,
    the longest chain has 6 frames (longer than the cuts T = 2 and T = 3 of the GPU test), 4 points take their guess from a
    later link than their first, and all 5 frames that hold heads hold them on both sides of keypoint 256.  260 frames of 96
    keypoints: 259 of 259 pairs valid, the longest chain has 27 frames (T = 8 cuts it), 3177 points and 13564 observations at
    T = 8, 332 of them with a later link."""
    seq, pairs = oracle_pairs["six"]
    assert all(p["valid"] for p in pairs)
    g = gm.build_global(pairs, _eye(6), 300, 0)
    hf, hk = g["head_frame"], g["head_kp"]
    both = sum(1 for f in range(6) if (hk[hf == f] < 256).any() and (hk[hf == f] >= 256).any())
    print("six frames: %d points, %d observations, longest chain %d, %d late guesses, %d frames with heads in both halves"
          % (len(hf), len(g["obs_frame"]), g["longest_chain"], (g["tri_link"] > 0).sum(), both))
    assert (len(hf), len(g["obs_frame"]), g["longest_chain"], int((g["tri_link"] > 0).sum()), both) == (301, 1004, 6, 4, 5)
    assert g["longest_chain"] > 3 and both >= 1
    for T in (2, 3):
        gt = gm.build_global(pairs, _eye(6), 300, T)
        assert np.diff(gt["obs_off"]).max() == T and (gt["head_frame"] > 0).any()
    # the first three frames, which the window agreement test uses
    g3 = gm.build_global(pairs[:2], _eye(3), 300, 3)
    assert len(g3["head_frame"]) >= 30 and (np.diff(g3["obs_off"]) == 3).any()
    seq, pairs = oracle_pairs["long"]
    assert len(pairs) == LONG_FRAMES - 1 > 256 and all(p["valid"] for p in pairs)
    g = gm.build_global(pairs, _eye(LONG_FRAMES), LONG_ARGS["n_kp"], LONG_T)
    print("long: %d points, %d observations, longest chain %d, %d late guesses"
          % (len(g["head_frame"]), len(g["obs_frame"]), g["longest_chain"], (g["tri_link"] > 0).sum()))
    assert (len(g["head_frame"]), len(g["obs_frame"]), g["longest_chain"], int((g["tri_link"] > 0).sum())) == (3177, 13564, 27, 332)
    assert g["longest_chain"] > LONG_T and (g["head_frame"] >= 256).any() and (g["head_frame"] < 256).any()


def test_host_decisions_under_the_host_sanitizers(tmp_path):
    """seq_global_host.hpp from a program of its own: the admitted cuts and every limit of the counts"""
    exe = str(tmp_path / "seq_global_limits_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mvslam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "seq_global_limits_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_seq_global_struct_layout_and_symbols():
    """mvs_seq_global_params: header <-> ctypes; the four new entry points are exported; the ABI version is still 4"""
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(mvs_seq_global_params), offsetof(mvs_seq_global_params, max_track_frames),
         offsetof(mvs_seq_global_params, reserved), offsetof(mvs_seq_global_params, sigma_px));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    P = capi.SeqGlobalParams
    assert v == [C.sizeof(P), P.max_track_frames.offset, P.reserved.offset, P.sigma_px.offset] == [16, 0, 4, 8]
    lib = capi.lib()
    for name in ("mvs_seq_refine_global", "mvs_seq_global_counts", "mvs_seq_download_global",
                 "mvs_seq_download_global_problem"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.mvs_abi_version() == 4
    dbg = subprocess.check_output(["nm", "-D", capi.DBG_LIB_PATH]).decode()
    prod = subprocess.check_output(["nm", "-D", capi.LIB_PATH]).decode()
    assert "mvs_debug_seq_global_plan" in dbg and "mvs_debug_seq_global_plan" not in prod


def test_seq_global_kernel_resources():
    """the new kernels are in the build's digest, each once, without scratch or spills: the chain walks of the count and emit
    kernels keep their state in registers"""
    res = json.load(open(os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")))
    for n in ("depth", "count", "scan", "envelope", "emit", "frames", "sort", "offsets", "gather", "rows", "pairs"):
        hits = {k: v for k, v in res.items() if "seq_glob_%s_kernel" % n in k}
        assert len(hits) == 1, n
        for k, v in hits.items():
            assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
