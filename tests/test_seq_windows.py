"""Sliding windows of a resident sequence: mvs_seq_refine_windows / mvs_seq_download_windows.

CPU part: build_windows restates the track and window definition in numpy and is unit-tested on a hand-written link table;
the synthetic sequence the GPU tests use is shown (on the oracle's pairs alone) to give every window enough multi-frame
tracks; the header / ctypes layout of the two new structs and the three new symbols.
GPU part: the device's assembly against build_windows fed with the device's own downloaded pairs, trajectory and octaves
(integers equal, guesses to 1e-12 max(1, |X|): the project's points bound, the guess is three multiply-adds deep); the
device's solve against mvs_ba_refine_windows on host windows built from the downloaded track_kp / point_guess (byte for
byte: the same kernel on the same inputs); a twin keypoint (two inlier rows with one trainIdx), truncation, the solver's own
sanity, determinism and the refusals.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import oracle_lib as o
import test_ba_window as tw
import test_refine as tr
import test_sequence as ts
from mvslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the one sequence of this file: 6 frames of 300 keypoints over a map small enough that consecutive frames keep seeing the
# same points (test_generator_gives_every_window_multi_frame_tracks)
SEQ_ARGS = dict(n_kp=300, n_map=1500, noise_px=0.3, step=0.1)
PRM = dict(H=600, seed=4242, thr=1e-2)
PPRM = dict(H=300, seed=99, err=2.0)


def make_seq():
    return synth.make_sequence(6, **SEQ_ARGS)


# ---------------------------------------------------------------------------------------------------------------------
# the definition, in numpy

def build_links(pairs, N):
    """succ[k][i]: match row of the link out of keypoint i of frame k (-1: none); pred[k + 1][i]: the keypoint of frame k
    linked to keypoint i; row_to_point[k][r]: triangulated point of row r.  A link is an inlier row of a valid pair; of the
    rows that share a trainIdx the smallest wins."""
    P = len(pairs)
    succ, pred, rtp = -np.ones((P, N), np.int64), -np.ones((P + 1, N), np.int64), -np.ones((P, N), np.int64)
    for k, p in enumerate(pairs):
        if not p["valid"]:
            continue
        for r in range(len(p["matches"])):
            t, q = int(p["matches"]["trainIdx"][r]), int(p["matches"]["queryIdx"][r])
            if p["mask"][r] == 1 and succ[k, t] < 0:
                succ[k, t] = r
                pred[k + 1, q] = t
        rtp[k, p["point_idx"]] = np.arange(len(p["point_idx"]))
    return succ, pred, rtp


def build_windows(pairs, traj, kp, octave, F, stride, max_points):
    """pairs: per pair dict(valid, matches[n_matches], mask[n_matches], point_idx[n_points], points[n_points, 3]); traj:
    dict(R, t, pair_scale).  One dict per window: first_frame, n_tracks_found, n_points, track_kp [n_points, F],
    point_guess [n_points, 3]."""
    n_frames, N = kp.shape[0], kp.shape[1]
    succ, pred, rtp = build_links(pairs, N)
    out = []
    for w in range((n_frames - F) // stride + 1 if n_frames >= F else 0):
        a = w * stride
        tkp, guess = [], []
        for j in range(a, a + F - 1):
            for i in range(N):
                if succ[j, i] < 0 or (j > a and pred[j, i] >= 0):
                    continue
                row, g, f, cur = np.full(F, -1, np.int64), None, j, i
                while True:
                    row[f - a] = cur
                    if f == a + F - 1 or succ[f, cur] < 0:
                        break
                    r = succ[f, cur]
                    if g is None and rtp[f, r] >= 0:
                        x = pairs[f]["points"][rtp[f, r]]
                        g = traj["R"][f] @ (traj["pair_scale"][f] * x) + traj["t"][f]
                    cur = int(pairs[f]["matches"]["queryIdx"][r])
                    f += 1
                if g is not None:
                    tkp.append(row)
                    guess.append(g)
        m = min(len(tkp), max_points)
        out.append(dict(first_frame=a, n_tracks_found=len(tkp), n_points=m,
                        track_kp=np.array(tkp[:m], np.int64).reshape(m, F), point_guess=np.array(guess[:m]).reshape(m, 3)))
    return out


def host_window(win, traj, kp, octave, K, params, sigma_px):
    """the mvs_ba_window the device hands its window kernel, rebuilt on the host from a window's track_kp / point_guess"""
    a, tkp = win["first_frame"], win["track_kp"]
    m, F = tkp.shape
    poses = np.stack([np.concatenate([traj["R"][a + f].reshape(9), traj["t"][a + f]]) for f in range(F)])
    an, ps, pt = list(params.anchor_sigma), list(params.pose_sigma), params.point_sigma
    var = np.array([[s[0] * s[0]] * 3 + [s[1] * s[1]] * 3 for s in [an] + [ps] * (F - 1)])
    obs, cov, valid = [], [], []
    for f in range(F):
        seen = tkp[:, f] >= 0
        idx = np.where(seen, tkp[:, f], 0)
        sd = np.ldexp(float(sigma_px), octave[a + f][idx].astype(np.int32))
        c = sd * sd
        obs.append(np.where(seen[:, None], kp[a + f][idx].astype(np.float64), 0.0))
        cov.append(np.stack([c, np.zeros(m), np.zeros(m), c], 1))
        valid.append(seen.astype(np.uint8))
    return dict(K=K, frame_pose=poses, frame_prior_var=var, points=win["point_guess"],
                point_prior_cov=np.tile((np.eye(3) * (pt * pt)).reshape(9), (m, 1)), obs=obs, obs_cov=cov, obs_valid=valid)


def window_cost(hw, Rs, ts_, P):
    """the cost of DESIGN.md section 4.7 of a host window at (Rs, ts_, P), as test_ba_window's GPU tests evaluate it"""
    K, c = hw["K"], 0.0
    for f in range(len(hw["frame_pose"])):
        Rg, tg = hw["frame_pose"][f][:9].reshape(3, 3), hw["frame_pose"][f][9:]
        sd = 1.0 / np.sqrt(hw["frame_prior_var"][f])
        c += np.sum((Rot.from_matrix(Rg.T @ Rs[f]).as_rotvec() * sd[:3]) ** 2) + np.sum((Rg.T @ (ts_[f] - tg) * sd[3:]) ** 2)
        v = hw["obs_valid"][f].astype(bool)
        e = (tr.proj(K, Rs[f], ts_[f], P[v]) - hw["obs"][f][v]) / np.sqrt(hw["obs_cov"][f][v, :1])
        c += np.sum(e ** 2)
    return 0.5 * (c + np.sum((P - hw["points"]) ** 2 / hw["point_prior_cov"][:, :1]))


# ---------------------------------------------------------------------------------------------------------------------
# CPU

def _hand_pairs():
    """four frames of eight keypoints.  Tracks (keypoint per frame): A 0-0-0-7 triangulated by pair 0; B 1-1-1 triangulated
    only by its second link; C 2-3-3-3 never triangulated; D starts at (frame 1, kp 5); E starts at (1, 2) because the row of
    pair 0 that leads there shares trainIdx 0 with an earlier row and is dropped; G starts at (2, 4); row 4 of pair 0 is no
    inlier."""
    def pair(k, rows, mask, point_idx):
        mt = np.zeros(len(rows), dtype=o.MATCH_DTYPE)
        mt["trainIdx"], mt["queryIdx"] = [r[0] for r in rows], [r[1] for r in rows]
        n = len(point_idx)
        return dict(valid=True, matches=mt, mask=np.array(mask, np.uint8), point_idx=np.array(point_idx, np.int64),
                    points=np.arange(3.0 * n).reshape(n, 3) + 100.0 * k + 1.0)

    return [pair(0, [(0, 0), (1, 1), (0, 2), (2, 3), (3, 4)], [1, 1, 1, 1, 0], [0, 2]),
            pair(1, [(1, 1), (0, 0), (3, 3), (5, 5), (2, 6)], [1, 1, 1, 1, 1], [0, 3, 4]),
            pair(2, [(0, 7), (5, 5), (3, 3), (4, 4)], [1, 1, 1, 1], [3])]


def _hand_traj():
    R = np.stack([Rot.from_rotvec([0.1 * k, -0.2, 0.05 * k]).as_matrix() for k in range(4)])
    return dict(R=R, t=np.arange(12.0).reshape(4, 3) * 0.1, pair_scale=np.array([1.0, 1.25, 0.75]))


def test_build_windows_on_a_hand_written_link_table():
    pairs, traj = _hand_pairs(), _hand_traj()
    kp, octv = np.zeros((4, 8, 2), np.float32), np.zeros((4, 8), np.uint8)
    succ, pred, rtp = build_links(pairs, 8)
    assert succ[0, 0] == 0 and pred[1, 2] == -1 and pred[1, 0] == 0        # shared trainIdx: the smallest row wins
    assert succ[0, 3] == -1 and pred[1, 4] == -1                            # an outlier row is no link
    g = lambda k, j: traj["R"][k] @ (traj["pair_scale"][k] * pairs[k]["points"][j]) + traj["t"][k]
    (w,) = build_windows(pairs, traj, kp, octv, 4, 1, 4096)
    assert (w["first_frame"], w["n_tracks_found"], w["n_points"]) == (0, 5, 5)
    #                                      A              B (2nd link)    E (mid-window)  D (mid-window)  G
    assert w["track_kp"].tolist() == [[0, 0, 0, 7], [1, 1, 1, -1], [-1, 2, 6, -1], [-1, 5, 5, 5], [-1, -1, 4, 4]]
    assert np.array_equal(w["point_guess"], np.stack([g(0, 0), g(1, 0), g(1, 2), g(1, 1), g(2, 0)]))
    (w2,) = build_windows(pairs, traj, kp, octv, 4, 1, 2)                    # truncation keeps the first two
    assert (w2["n_tracks_found"], w2["n_points"]) == (5, 2) and w2["track_kp"].tolist() == [[0, 0, 0, 7], [1, 1, 1, -1]]
    assert np.array_equal(w2["point_guess"], w["point_guess"][:2])
    wa, wb = build_windows(pairs, traj, kp, octv, 3, 1, 4096)
    assert wa["track_kp"].tolist() == [[0, 0, 0], [1, 1, 1], [-1, 2, 6], [-1, 5, 5]]
    # frames 1 .. 3: A continues through the window without a triangulated link inside it and is dropped, B enters at
    # frame 1 although it has a predecessor there, C is never triangulated
    assert wb["first_frame"] == 1 and wb["track_kp"].tolist() == [[1, 1, -1], [2, 6, -1], [5, 5, 5], [-1, 4, 4]]
    assert np.array_equal(wb["point_guess"], np.stack([g(1, 0), g(1, 2), g(1, 1), g(2, 0)]))
    bad = [dict(p) for p in pairs]
    bad[1]["valid"] = False                                                  # an invalid pair has no links
    (w3,) = build_windows(bad, traj, kp, octv, 4, 1, 4096)
    assert w3["track_kp"].tolist() == [[0, 0, -1, -1], [-1, -1, 4, 4]]


def test_generator_gives_every_window_multi_frame_tracks():
    """on the oracle's pairs alone: every window of four frames has at least 30 points and a quarter of them are seen in
    three frames or more, so the GPU comparison below is about multi-frame tracks"""
    seq = make_seq()
    pairs, _ = ts.oracle_sequence(seq, PRM, PPRM)
    pairs = [dict(p, valid=p["ok"]) for p in pairs]
    eye = dict(R=np.tile(np.eye(3), (6, 1, 1)), t=np.zeros((6, 3)), pair_scale=np.ones(5))
    wins = build_windows(pairs, eye, seq["kp"], np.zeros((6, 300), np.uint8), 4, 1, 4096)
    assert len(wins) == 3
    for w in wins:
        seen = (w["track_kp"] >= 0).sum(1)
        print("window %d: %d points, %d seen in >= 3 frames, %d in 4" % (w["first_frame"], w["n_points"], (seen >= 3).sum(),
                                                                         (seen >= 4).sum()))
        assert w["n_points"] >= 30 and 4 * (seen >= 3).sum() >= w["n_points"]


def test_seq_window_struct_layout_and_symbols():
    """mvs_seq_window_params / mvs_seq_window_info: header <-> ctypes; the three new entry points are exported; the ABI
    version is still 4"""
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mvs_seq_window_params), offsetof(mvs_seq_window_params, stride),
         offsetof(mvs_seq_window_params, max_points), offsetof(mvs_seq_window_params, sigma_px), sizeof(mvs_seq_window_info),
         offsetof(mvs_seq_window_info, n_frames), offsetof(mvs_seq_window_info, n_points),
         offsetof(mvs_seq_window_info, n_tracks_found));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    P, I = capi.SeqWindowParams, capi.SeqWindowInfo
    assert v == [C.sizeof(P), P.stride.offset, P.max_points.offset, P.sigma_px.offset, C.sizeof(I), I.n_frames.offset,
                 I.n_points.offset, I.n_tracks_found.offset]
    assert capi.WINDOW_INFO_DTYPE.itemsize == C.sizeof(I)
    lib = capi.lib()
    for name in ("mvs_seq_refine_windows", "mvs_seq_window_count", "mvs_seq_download_windows"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.mvs_abi_version() == 4


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def _run(ctx, seq, n_kp=None, octave=None):
    """upload + mvs_seq_run; returns the open Sequence and what the builder needs of its downloads"""
    from mvslam_amd import capi

    F, N = seq["kp"].shape[0], seq["kp"].shape[1]
    s = capi.Sequence(ctx, F, N, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"] if n_kp is None else n_kp, seq["K"])
    if octave is not None:
        s.upload_octaves(0, octave)
    s.run(capi.default_params(num_hypotheses=PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=PRM["seed"], max_error_sq=PRM["thr"]),
          capi.default_pnp_params(num_hypotheses=PPRM["H"], seed=PPRM["seed"], reproj_error=PPRM["err"]))
    gp = s.download_pairs()
    pairs = []
    for k, r in enumerate(gp["results"]):
        M, n = int(r["n_matches"]), int(r["n_points"]) if r["valid"] else 0
        pairs.append(dict(valid=bool(r["valid"]), matches=gp["matches"][k][:M], mask=gp["mask"][k][:M],
                          point_idx=gp["point_idx"][k][:n], points=gp["points"][k][:n]))
    octave = np.zeros((F, N), np.uint8) if octave is None else octave
    return s, dict(pairs=pairs, traj=s.download_trajectory(), kp=seq["kp"], octave=octave, K=seq["K"])


@pytest.fixture(scope="module")
def resident(ctx):
    """the sequence of this file, run once; octaves 0 .. 2 so that the observation weights differ"""
    seq = make_seq()
    octave = (np.arange(6 * 300).reshape(6, 300) % 3).astype(np.uint8)
    s, dev = _run(ctx, seq, octave=octave)
    yield s, dev, seq
    s.close()


def _check_assembly(got, dev, F, stride, max_points):
    want = build_windows(dev["pairs"], dev["traj"], dev["kp"], dev["octave"], F, stride, max_points)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["first_frame"], g["n_frames"], g["n_points"], g["n_tracks_found"]) == \
            (w["first_frame"], F, w["n_points"], w["n_tracks_found"])
        assert np.array_equal(g["track_kp"], w["track_kp"])
        err = np.abs(g["point_guess"] - w["point_guess"])
        print("window %d: %d points, guess error %.2e" % (g["first_frame"], g["n_points"], err.max() if err.size else 0.0))
        assert np.all(err <= 1e-12 * np.maximum(1.0, np.abs(w["point_guess"])))
    return want


def _check_solve(ctx, got, dev, params, sigma_px):
    """the device's windows against mvs_ba_refine_windows on host windows built from the downloaded track_kp / point_guess"""
    some = [g for g in got if g["n_points"] > 0]
    hws = [host_window(g, dev["traj"], dev["kp"], dev["octave"], dev["K"], params, sigma_px) for g in some]
    ref = ctx.ba_refine_windows(hws, params) if hws else []
    for g, r in zip(some, ref):
        assert g["ok"] == r["ok"] and g["raw"] == r["raw"], g["first_frame"]
        assert g["points"].tobytes() == r["points"].tobytes() and g["point_cov"].tobytes() == r["point_cov"].tobytes()
    for g in got:
        if g["n_points"] == 0:
            assert not g["ok"] and g["status"] == 1 and g["raw"] == bytes(len(g["raw"]))
    return hws


@pytest.mark.gpu
@pytest.mark.parametrize("F,stride,sigma_px", [(4, 1, 0.5), (3, 2, 0.5), (6, 1, 0.5), (4, 1, 0.7)])
def test_gpu_seq_windows_assembly_and_solve(ctx, resident, F, stride, sigma_px):
    from mvslam_amd import capi

    s, dev, _ = resident
    params = capi.default_refine_params()
    s.refine_windows(F, stride, 4096, params, sigma_px)
    got = s.download_windows()
    _check_assembly(got, dev, F, stride, 4096)
    _check_solve(ctx, got, dev, params, sigma_px)
    assert all(g["ok"] and g["n_points"] >= 30 for g in got)


@pytest.mark.gpu
def test_gpu_seq_windows_twin_keypoint(ctx, resident):
    """frame 2 gets a copy of one of its matched keypoints (same descriptor, 0.25 px away) in a slot no match uses: pair 1
    then holds two inlier rows with one trainIdx, and the smaller row is the link"""
    from mvslam_amd import capi

    _, dev0, seq0 = resident
    p1, p2 = dev0["pairs"][1], dev0["pairs"][2]
    i = int(p1["matches"]["queryIdx"][p1["point_idx"][0]])
    free = np.setdiff1d(np.arange(300), np.concatenate([p1["matches"]["queryIdx"], p2["matches"]["trainIdx"]]))
    c = int(free[0])
    seq = dict(seq0, desc=seq0["desc"].copy(), kp=seq0["kp"].copy())
    seq["desc"][2, c] = seq["desc"][2, i]
    seq["kp"][2, c] = seq["kp"][2, i] + np.float32([0.25, 0.0])
    s, dev = _run(ctx, seq)
    try:
        p = dev["pairs"][1]
        rows = np.nonzero(np.isin(p["matches"]["queryIdx"], [i, c]) & (p["mask"] == 1))[0]
        assert len(rows) == 2 and len(set(p["matches"]["trainIdx"][rows])) == 1, "the twin is not two inlier rows of one trainIdx"
        params = capi.default_refine_params()
        s.refine_windows(4, 1, 4096, params, 0.5)
        got = s.download_windows()
        _check_assembly(got, dev, 4, 1, 4096)
        _check_solve(ctx, got, dev, params, 0.5)
        # the losing row's keypoint of frame 2 follows no track of the windows that hold pair 1
        loser = int(p["matches"]["queryIdx"][rows[1]])
        for g in got[:2]:
            col = g["track_kp"][:, 2 - g["first_frame"]]
            pre = g["track_kp"][:, 1 - g["first_frame"]]
            assert not np.any((col == loser) & (pre >= 0))
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_seq_windows_truncation(ctx, resident):
    from mvslam_amd import capi

    s, dev, _ = resident
    params = capi.default_refine_params()
    s.refine_windows(4, 1, 4096, params, 0.5)
    full = s.download_windows()
    s.refine_windows(4, 1, 64, params, 0.5)
    got = s.download_windows()
    _check_assembly(got, dev, 4, 1, 64)
    for g, f in zip(got, full):
        assert g["n_points"] == 64 < g["n_tracks_found"] == f["n_tracks_found"]
        assert np.array_equal(g["track_kp"], f["track_kp"][:64])
        assert g["point_guess"].tobytes() == f["point_guess"][:64].tobytes()
    _check_solve(ctx, got, dev, params, 0.5)


@pytest.mark.gpu
def test_gpu_seq_windows_solver_sanity_and_determinism(ctx, resident):
    from mvslam_amd import capi

    s, dev, _ = resident
    params = capi.default_refine_params()
    runs = []
    for _ in range(2):
        s.refine_windows(4, 1, 4096, params, 0.5)
        runs.append(s.download_windows())
    for a, b in zip(*runs):
        assert tw._bytes(a) == tw._bytes(b)
        assert a["track_kp"].tobytes() == b["track_kp"].tobytes() and a["point_guess"].tobytes() == b["point_guess"].tobytes()
    for g in runs[0]:
        hw = host_window(g, dev["traj"], dev["kp"], dev["octave"], dev["K"], params, 0.5)
        at_result = window_cost(hw, g["R"], g["t"], g["points"])
        at_guess = window_cost(hw, hw["frame_pose"][:, :9].reshape(-1, 3, 3), hw["frame_pose"][:, 9:], hw["points"])
        print("window %d: guess %.6e  result %.6e  reported %.6e  iterations %d" % (g["first_frame"], at_guess, at_result,
                                                                                    g["error"], g["iterations"]))
        assert g["ok"]
        assert abs(g["error"] - at_result) <= 1e-9 * g["error"]
        assert g["error"] <= at_guess


@pytest.mark.gpu
def test_gpu_seq_windows_refusals(ctx, resident):
    from mvslam_amd import capi

    s, dev, seq = resident

    def status_of(fn, *a):
        with pytest.raises(capi.MvsError) as e:
            fn(*a)
        return e.value.status

    for F, stride, cap in [(2, 1, 4096), (9, 1, 4096), (4, 0, 4096), (4, 1, 0), (4, 1, 4097), (7, 1, 4096)]:
        assert status_of(s.refine_windows, F, stride, cap) == capi.MVS_ERR_INVALID_ARG, (F, stride, cap)
    for sigma_px in (0.0, -0.5):
        assert status_of(s.refine_windows, 4, 1, 4096, None, sigma_px) == capi.MVS_ERR_INVALID_ARG
    wp = capi.SeqWindowParams(4, 1, 4096, 0, 0.0)               # the count is about the windows' shape alone
    assert capi.lib().mvs_seq_window_count(s._h, C.byref(wp)) == 3
    fresh = capi.Sequence(ctx, 6, 300, 32)                     # uploaded, never run
    fresh.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
    assert status_of(fresh.refine_windows, 4, 1) == capi.MVS_ERR_INVALID_ARG
    fresh.close()
    # frame 3 has four keypoints: pairs 2 and 3 are invalid; the windows assemble from the links that remain
    n_kp = seq["n_kp"].copy()
    n_kp[3] = 4
    blind, bdev = _run(ctx, seq, n_kp=n_kp)
    try:
        assert not bdev["pairs"][2]["valid"] and not bdev["pairs"][3]["valid"] and bdev["pairs"][1]["valid"]
        params = capi.default_refine_params()
        blind.refine_windows(4, 1, 4096, params, 0.5)
        got = blind.download_windows()
        _check_assembly(got, bdev, 4, 1, 4096)
        _check_solve(ctx, got, bdev, params, 0.5)
        assert all(g["ok"] or g["status"] == capi.MVS_NO_MODEL for g in got)
        assert not np.any(got[0]["track_kp"][:, 3] >= 0)        # nothing reaches frame 3
    finally:
        blind.close()
    s.refine_windows(4, 1, 4096, params, 0.5)                  # the context solves a good sequence afterwards
    assert all(g["ok"] for g in s.download_windows())
