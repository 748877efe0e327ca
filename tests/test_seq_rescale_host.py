"""The scale of a resident sequence from depth ratios of shared points, CPU part (mvs_seq_rescale).

The header / ctypes layout of the two new structs and the two new symbols; the numpy model (tests/seq_rescale_model.py) on
hand-written tables and on exact poses with exactly triangulated points; the finding the rule answers, on the oracle's pairs
and tracks of an 80-frame sequence (nothing under test decides it); the sequences the GPU tests use, shown on the oracle's
pairs alone to exercise what those tests are about; the new kernels in the build's digest beside seq_chain_kernel's unchanged
row.
"""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as o
import seq_rescale_model as rm
import test_seq_windows as sw
import test_sequence as ts
from mvslam_amd import synth
from test_seq_global_host import LONG_ARGS, LONG_FRAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sequences of tests/test_seq_rescale.py beside test_seq_windows' six frames of 300 keypoints and test_seq_global's 260
# frames of 96: three frames of 600 keypoints, whose keypoint table crosses 256 and 512 and whose second pair has more than
# 256 points (the compaction's chunk)
WIDE_ARGS = dict(n_kp=600, n_map=1500, noise_px=0.3, step=0.1)
# seq_chain_kernel's row of the build's digest before this kernel had neighbours
CHAIN_ROW = dict(agprs=0, occupancy_waves_per_simd=5, scratch_bytes_per_lane=0, sgpr_spills=0, sgprs=62, static_lds_bytes=28352,
                 vgpr_spills=0, vgprs=78)


def twin_sequence(seq0, pairs):
    """seq0 with a copy of a keypoint of frame 3 (same descriptor, 0.25 px away) in a slot no match uses.  The keypoint is the
    new keypoint of a point of pair 2 whose base keypoint pairs 1 and 2 share: pair 2 then holds two points with that base
    keypoint (test_seq_windows' twin, one pair later and on a shared point)."""
    _, jn = rm.shared_points(pairs[1], pairs[2], seq0["kp"].shape[1])
    p2, p3 = pairs[2], pairs[3]
    i = int(p2["matches"]["queryIdx"][p2["point_idx"][jn[0]]])
    free = np.setdiff1d(np.arange(seq0["kp"].shape[1]), np.concatenate([p2["matches"]["queryIdx"], p3["matches"]["trainIdx"]]))
    c = int(free[0])
    seq = dict(seq0, desc=seq0["desc"].copy(), kp=seq0["kp"].copy())
    seq["desc"][3, c] = seq["desc"][3, i]
    seq["kp"][3, c] = seq["kp"][3, i] + np.float32([0.25, 0.0])
    return seq


def shared_twice(pairs, N):
    """keypoints that are the new keypoint of a point of pair q and the base keypoint of more than one point of pair q + 1"""
    n = 0
    for q in range(len(pairs) - 1):
        _, bq, okq = rm.point_keypoints(pairs[q], N)
        an, _, okn = rm.point_keypoints(pairs[q + 1], N)
        kps, cnt = np.unique(an[okn], return_counts=True)
        n += int(np.isin(kps[cnt > 1], bq[okq]).sum())
    return n


# ---------------------------------------------------------------------------------------------------------------------
# layout and symbols

def test_seq_rescale_struct_layout_and_symbols():
    """mvs_seq_scale_params (8 bytes) and mvs_seq_scale_step (24): header <-> ctypes; the two new entry points are declared and
    exported; the ABI version is still 4"""
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  mvs_seq_scale_params *p = 0;
  mvs_seq_scale_step *s = 0;
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(mvs_seq_scale_params), offsetof(mvs_seq_scale_params, min_common),
         sizeof(mvs_seq_scale_step), offsetof(mvs_seq_scale_step, n_used), offsetof(mvs_seq_scale_step, flag),
         offsetof(mvs_seq_scale_step, reserved), offsetof(mvs_seq_scale_step, scale),
         sizeof(mvs_seq_rescale(0, p)) + sizeof(mvs_seq_download_scale_steps(0, s)) - 2 * sizeof(mvs_status) + 1,
         MVS_SEQ_SCALE_CHAIN, MVS_SEQ_SCALE_DEPTH_RATIO, MVS_ABI_VERSION);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    P, S = capi.SeqScaleParams, capi.SCALE_STEP_DTYPE
    assert v == [8, 4, 24, 4, 8, 12, 16, 1, capi.SEQ_SCALE_CHAIN, capi.SEQ_SCALE_DEPTH_RATIO, 4]
    assert (C.sizeof(P), P.min_common.offset) == (8, 4)
    assert S.itemsize == 24 and [S.fields[k][1] for k in ("n_common", "n_used", "flag", "reserved", "scale")] == [0, 4, 8, 12, 16]
    assert S == rm.STEP_DTYPE and (capi.SEQ_SCALE_CHAIN, capi.SEQ_SCALE_DEPTH_RATIO) == (rm.RULE_CHAIN, rm.RULE_DEPTH_RATIO)
    lib = capi.lib()
    for name in ("mvs_seq_rescale", "mvs_seq_download_scale_steps"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.mvs_abi_version() == 4
    assert hasattr(capi.Sequence, "rescale") and hasattr(capi.Sequence, "download_scale_steps")


def test_seq_rescale_kernel_resources():
    """the two new kernels are in the build's digest, each once, without scratch or spills; seq_chain_kernel's row is what it
    was"""
    res = json.load(open(os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")))
    for n in ("seq_ratio_kernel", "seq_sigma_fold_kernel"):
        hits = {k: v for k, v in res.items() if n in k}
        assert len(hits) == 1, n
        for k, v in hits.items():
            assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    (chain,) = [v for k, v in res.items() if "seq_chain_kernel" in k]
    assert chain == CHAIN_ROW


# ---------------------------------------------------------------------------------------------------------------------
# the model on hand-written tables

def _pair(rows, point_z, R=None, t=(0.0, 0.0, 0.5), valid=True):
    """a pair of eight-keypoint frames: rows = (trainIdx, queryIdx) per match; point j belongs to row j and lies at
    (0.25 j, -0.5, point_z[j]) in the base camera"""
    mt = np.zeros(len(rows), dtype=o.MATCH_DTYPE)
    mt["trainIdx"], mt["queryIdx"] = [r[0] for r in rows], [r[1] for r in rows]
    n = len(point_z)
    pts = np.stack([0.25 * np.arange(n), np.full(n, -0.5), np.array(point_z, np.float64)], 1).reshape(n, 3)
    return dict(valid=valid, R=np.eye(3) if R is None else R, t=np.array(t, np.float64), matches=mt,
                point_idx=np.arange(n, dtype=np.int64), points=pts)


def _hand_pairs():
    """five frames.  Step 0: keypoints 0 .. 3 of frame 1 are shared (4 is the new keypoint of a point of pair 0 only, 6 the
    base keypoint of a point of pair 1 only); keypoint 1 is shared twice, by points 1 (ratio 3) and 2 (ratio 1) of pair 1;
    keypoint 3's point lies behind pair 1's camera.  Used ratios 2, 3, 4: an odd count.  Step 1: keypoints 0, 5, 1, 2 of
    frame 2, ratios 1, 2, 4, 8: an even count.  Step 2: two keypoints, ratios 2 and 0.5."""
    return [_pair([(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)], [2.5, 3.5, 4.5, 1.5, 9.5]),
            _pair([(0, 0), (1, 5), (1, 1), (2, 2), (3, 3), (6, 6)], [1.0, 1.0, 3.0, 1.0, -1.0, 1.0]),
            _pair([(0, 0), (5, 1), (1, 2), (2, 3), (7, 7)], [0.5, 0.25, 0.625, 0.0625, 1.0], t=(0.0, 0.0, -1.0)),
            _pair([(0, 0), (1, 1)], [0.75, 2.5], t=(0.5, 0.0, 0.0))]


def test_model_on_hand_written_tables():
    pairs = _hand_pairs()
    j, jn = rm.shared_points(pairs[0], pairs[1], 8)
    assert (j.tolist(), jn.tolist()) == ([0, 1, 2, 3], [0, 1, 3, 4])        # the twin: the smallest j' wins; ascending j'
    rho, used = rm.ratios(pairs[0], pairs[1], j, jn)
    assert used.tolist() == [True, True, True, False] and rho[:3].tolist() == [2.0, 3.0, 4.0]
    steps, traj = rm.rescale(pairs, 8, 1)
    assert steps["n_common"].tolist() == [4, 4, 2] and steps["n_used"].tolist() == [3, 4, 2]   # behind the camera: common, not used
    assert steps["flag"].tolist() == [0, 0, 0]
    assert steps["scale"].tolist() == [3.0, 2.0, 0.5]                       # lower medians: odd, even (numpy's median: 3), two
    assert traj["track_scale"].tolist() == [3.0, 2.0, 0.5] and traj["pair_scale"].tolist() == [1.0, 3.0, 6.0, 3.0]
    assert np.array_equal(traj["R"], np.tile(np.eye(3), (5, 1, 1)))
    assert traj["t"].tolist() == [[0, 0, 0], [0, 0, 0.5], [0, 0, 2.0], [0, 0, -4.0], [1.5, 0, -4.0]]
    # min_common at n_used keeps the ratio, above it the step keeps the scale
    at = rm.scale_steps(pairs, 8, 3)
    assert at["flag"].tolist() == [0, 0, 2] and at["scale"].tolist() == [3.0, 2.0, 1.0] and at["n_used"].tolist() == [3, 4, 2]
    above = rm.scale_steps(pairs, 8, 4)
    assert above["flag"].tolist() == [2, 0, 2] and above["scale"].tolist() == [1.0, 2.0, 1.0]
    assert rm.scale_steps(pairs, 8, 5)["flag"].tolist() == [2, 2, 2]
    # an invalid pair in the middle: the two steps that touch it keep the scale, the trajectory stands still across it
    bad = [dict(p) for p in pairs]
    bad[2]["valid"] = False
    steps, traj = rm.rescale(bad, 8, 1)
    assert steps["flag"].tolist() == [0, 1, 1] and steps["scale"].tolist() == [3.0, 1.0, 1.0]
    assert steps["n_common"].tolist() == [4, 0, 0] and steps["n_used"].tolist() == [3, 0, 0]
    assert traj["pair_scale"].tolist() == [1.0, 3.0, 3.0, 3.0]
    assert np.array_equal(traj["R"][3], traj["R"][2]) and np.array_equal(traj["t"][3], traj["t"][2])
    assert traj["t"][4].tolist() == [1.5, 0, 2.0]
    # a row or a keypoint outside the frame arrays is no point
    out = [dict(p) for p in pairs]
    out[1] = dict(out[1], point_idx=np.array([0, 1, 2, 3, 4, 9], np.int64))
    out[1]["matches"] = out[1]["matches"].copy()
    out[1]["matches"]["trainIdx"][0] = 8
    assert rm.scale_steps(out, 8, 1)[0].tolist()[:3] == (3, 2, 0)


def test_model_depth_is_the_third_row_of_the_inverse_pose():
    """z_a against R^T (x - t) written with numpy's matrix product, for a general rotation"""
    from scipy.spatial.transform import Rotation as Rot

    R = Rot.from_rotvec([0.3, -0.2, 0.4]).as_matrix()
    pq = _pair([(i, i) for i in range(5)], [2.5, 3.5, 4.5, 1.5, 9.5], R=R, t=(0.3, -0.1, 0.4))
    pn = _pair([(i, i) for i in range(5)], [1.0, 2.0, 3.0, 4.0, 5.0])
    j, jn = rm.shared_points(pq, pn, 8)
    rho, used = rm.ratios(pq, pn, j, jn)
    want = ((pq["points"] - pq["t"]) @ R)[:, 2] / pn["points"][:, 2]
    assert used.all() and np.abs(rho - want).max() <= 1e-15 * np.abs(want).max()


def test_model_on_exact_poses_and_points():
    """exact relative poses with unit baselines and exactly triangulated points: scale_q = b_{q+1} / b_q to 1e-12 and the
    trajectory is the truth in units of b_0"""
    rng = np.random.default_rng(5)
    F, n = 9, 40
    yaw = 0.03 * np.arange(F)
    step = 0.05 * (1.0 + 0.5 * np.sin(1.7 * np.arange(F)))               # baselines that differ from pair to pair
    c = np.cumsum(np.stack([0.5 * step, 0.1 * step, 0.866 * step], 1), 0)
    Rw = [np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]) for a in yaw]   # world -> camera
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], 1)
    cam = [(R.T, ck) for R, ck in zip(Rw, c)]                            # camera in world
    rel = lambda a, b: (cam[a][0].T @ cam[b][0], cam[a][0].T @ (cam[b][1] - cam[a][1]))
    base = [np.linalg.norm(rel(k, k + 1)[1]) for k in range(F - 1)]
    rows = [(i, i) for i in range(n)]
    pairs = []
    for k in range(F - 1):
        Xk = (X - c[k]) @ Rw[k].T / base[k]                              # frame k's camera, pair k's unit baseline
        p = _pair(rows, Xk[:, 2], R=rel(k, k + 1)[0], t=rel(k, k + 1)[1] / base[k])
        p["points"] = Xk
        pairs.append(p)
    steps, traj = rm.rescale(pairs, n, 1)
    assert np.all(steps["flag"] == 0) and np.all(steps["n_used"] == n)
    want = np.array(base[1:]) / np.array(base[:-1])
    assert np.ptp(want) > 0.5 and np.abs(steps["scale"] / want - 1.0).max() <= 1e-12
    for k in range(F):
        R, t = rel(0, k)
        assert np.abs(traj["R"][k] - R).max() <= 1e-12 and np.abs(traj["t"][k] * base[0] - t).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the finding, and the sequences of the GPU tests, on the oracle's pairs

def test_chain_collapses_and_depth_ratio_holds_on_80_frames():
    """synth.make_sequence(80, n_kp=400, n_map=4000), whose true step scales are all 1, through the oracle (H = 600,
    thr = 2e-3, PnP H = 300, err = 2.0): the chain's sigma at the last pair is below 1e-6 (measured 5.1e-24; geometric mean of
    its 78 steps 0.503), the model's lies within [1/8, 8].  Measured with the committed model: 0.1997, geometric mean of the
    steps 0.980, their log-std 0.51 -- inside the bound, outside [1/4, 4]: the lower median of 9 .. 49 ratios sits below the
    middle of an even count, 2 % a step (numpy's averaging median gives 2.11 on the same shared points, the upper median 17.2); DESIGN.md section
    4.6.1 says so."""
    seq = synth.make_sequence(80, n_kp=400, n_map=4000)
    pairs, tracks = ts.oracle_sequence(seq, dict(H=600, seed=4242, thr=2e-3), dict(H=300, seed=99, err=2.0), threads=16)
    assert all(p["ok"] for p in pairs) and all(t["ok"] for t in tracks)
    chain = o.seq_chain([p["R"] for p in pairs], [p["t"] for p in pairs], np.ones(79, np.int32), [t["R"] for t in tracks],
                        [t["t"] for t in tracks], np.ones(78, np.int32))
    steps, traj = rm.rescale([dict(p, valid=p["ok"]) for p in pairs], 400, 1)
    geo = lambda s: float(np.exp(np.mean(np.log(s))))
    print("chain: sigma_last %.3e, geometric mean of the steps %.4f, log-std %.3f" %
          (chain["pair_scale"][-1], geo(chain["track_scale"]), np.std(np.log(chain["track_scale"]))))
    print("depth ratio: sigma_last %.4f, geometric mean of the steps %.4f, log-std %.3f, n_used %d .. %d" %
          (traj["pair_scale"][-1], geo(steps["scale"]), np.std(np.log(steps["scale"])), steps["n_used"].min(),
           steps["n_used"].max()))
    assert np.all(steps["flag"] == 0)
    assert chain["pair_scale"][-1] < 1e-6
    assert 1.0 / 8.0 <= traj["pair_scale"][-1] <= 8.0


@pytest.fixture(scope="module")
def oracle_pairs():
    out = {}
    for name, F, args in (("six", 6, sw.SEQ_ARGS), ("wide", 3, WIDE_ARGS), ("long", LONG_FRAMES, LONG_ARGS)):
        seq = synth.make_sequence(F, **args)
        pairs, _ = ts.oracle_sequence(seq, sw.PRM, sw.PPRM, threads=4)
        out[name] = (seq, [dict(p, valid=p["ok"]) for p in pairs])
    return out


def test_generators_give_what_the_gpu_tests_are_about(oracle_pairs):
    """on the oracle's pairs alone.  No keypoint is shared twice in the six frames of 300 keypoints nor in the 260 frames of 96
    (the matcher seldom gives two query keypoints one train keypoint, and both must be triangulated inliers), so the GPU test
    adds a twin keypoint to the six frames: one keypoint of frame 3 shared twice.  Three frames of 600 keypoints: shared
    keypoints on both sides of 256 and of 512, and pair 1's shared points on both sides of point 256."""
    seq, pairs = oracle_pairs["six"]
    steps = rm.scale_steps(pairs, 300, 1)
    assert all(p["valid"] for p in pairs) and np.all(steps["flag"] == 0) and steps["n_used"].min() >= 50
    assert shared_twice(pairs, 300) == 0
    tw, _ = ts.oracle_sequence(twin_sequence(seq, pairs), sw.PRM, sw.PPRM, threads=4)
    tw = [dict(p, valid=p["ok"]) for p in tw]
    assert shared_twice(tw, 300) == 1 and all(p["valid"] for p in tw)
    seq, pairs = oracle_pairs["long"]
    steps = rm.scale_steps(pairs, LONG_ARGS["n_kp"], 1)
    print("long: n_used %d .. %d, %d keypoints shared twice" % (steps["n_used"].min(), steps["n_used"].max(),
                                                                shared_twice(pairs, LONG_ARGS["n_kp"])))
    assert len(steps) == LONG_FRAMES - 2 > 2 * 128 and np.all(steps["flag"] == 0)     # the fold's chunk of 128, twice
    assert shared_twice(pairs, LONG_ARGS["n_kp"]) == 0
    seq, pairs = oracle_pairs["wide"]
    assert all(p["valid"] for p in pairs)
    j, jn = rm.shared_points(pairs[0], pairs[1], 600)
    c = rm.point_keypoints(pairs[1], 600)[0][jn]
    print("wide: %d shared keypoints, pair 1 has %d points" % (len(c), len(pairs[1]["point_idx"])))
    assert (c < 256).any() and ((c >= 256) & (c < 512)).any() and (c >= 512).any()
    assert len(pairs[1]["point_idx"]) > 256 and (jn < 256).any() and (jn >= 256).any()
