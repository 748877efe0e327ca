"""The tracking loop of a resident sequence: mvs_seq_track and its three downloads.

CPU part: the header / ctypes layout of mvs_vo_params and mvs_track_frame and the five new symbols; the definition restated in
numpy (kept points, join with the map, gates, problem assembly, commit) and run with stand-in solvers over a hand-written pair
table with a twin trainIdx, a PnP outlier that leaves the map and new points that enter it.
GPU part: every step of the device's run replayed FROM THE DEVICE'S OWN DOWNLOADED PREVIOUS STATE (the map of frame f - 1, its
pose, the id counter), so one rounding difference cannot cascade: the integer decisions are exact, the PnP pose and inliers
are mvs_pnp_solve's bytes on the downloaded candidates, scale and new points' guesses hold to 1e-12 max(1, |x|) (three
multiply-adds deep, the bound of test_seq_windows._check_assembly), the BA is mvs_ba_refine's bytes on the downloaded problem
and map[f] holds exactly its points.  Then refit, the refined initialisation, a later init pair, the three losses that data
and arguments can cause, the refusals and determinism.

One case departs from the letter of its specification: "max_error = half the error of step 3 gives LOST_ERROR exactly there"
presumes that step 2's error is below that half.  On this generator consecutive steps have alike errors (63.4 and 93.0 in
the fixture; no generator seed of 0 .. 79 gives step 3 twice step 2's error), so that value loses step 2, which is what the
"error_half" case asserts; "error_between" puts the gate between the two errors and pins LOST_ERROR exactly at step 3.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import test_seq_windows as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRM, PPRM = sw.PRM, sw.PPRM
N_FRAMES, N_KP = 6, 300
# of the generator.  Whether a step's BA reports ok hangs on its prior-less new points: one of low parallax can run off (to 6e10
# with synth's default seed, in the device's kernel, through mvs_ba_refine and in the CPU oracle alike), the reduced system
# at lambda = 0 is then not positive definite to rounding and the step is LOST_BA -- faithfully reported, but then nothing
# is TRACKED and the test shows nothing.  The default seed loses step 2 that way, seed 6 does with the refined
# initialisation.  With seed 2 the device tracks frames 2 .. 5 in every variant below (plain, refit, refined initialisation,
# init_pair 2): 104 / 98 / 77 / 74 PnP inliers of 105 / 106 / 88 / 86 candidates, BA errors 63.4 / 93.0 / 79.1 / 58.2, so step 3
# has the larger error and the fewer inliers of the first two steps, which the gate tests need.
SEED = 2


def make_seq():
    from mvslam_amd import synth

    return synth.make_sequence(N_FRAMES, seed=SEED, **sw.SEQ_ARGS)

NOT_REACHED, INIT, TRACKED, LOST_PNP, LOST_FEW, LOST_BA, LOST_ERROR = range(7)


# ---------------------------------------------------------------------------------------------------------------------
# the definition, in numpy.  pair: dict(valid, matches[n_matches], point_idx[n_points], points[n_points, 3]) as
# test_seq_windows._run builds it; a map: dict keypoint -> (id, X)

def kept_points(pair):
    """(j, a, b) of the kept points of a pair in ascending j: point j is kept iff no j' < j has the same trainIdx"""
    out, seen = [], set()
    if not pair["valid"]:
        return out
    for j, r in enumerate(pair["point_idx"]):
        a, b = int(pair["matches"]["trainIdx"][r]), int(pair["matches"]["queryIdx"][r])
        if a not in seen:
            seen.add(a)
            out.append((j, a, b))
    return out


def vo_init(pair, points=None):
    """the map of frame k0 + 1 and the id counter behind it"""
    x = pair["points"] if points is None else points
    kept = kept_points(pair)
    return {b: (i, x[j]) for i, (j, a, b) in enumerate(kept)}, len(kept)


def vo_join(pair, map_prev):
    """candidates (a, b, X) of a step: the kept points whose base keypoint the map holds"""
    return [(a, b, map_prev[a][1]) for j, a, b in kept_points(pair) if a in map_prev]


def vo_scale(t_pnp, t_last):
    e = t_pnp - t_last
    return np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


def vo_assemble(pair, map_prev, cands, inliers, R_last, t_last, scale, next_id):
    """points (id, a, b, is_new, X) of the step's BA problem: tracked, then new"""
    pts = [(map_prev[cands[c][0]][0], cands[c][0], cands[c][1], 0, cands[c][2]) for c in inliers]
    n = 0
    for j, a, b in kept_points(pair):
        if a not in map_prev:
            y = scale * pair["points"][j]
            X = np.array([((R_last[i, 0] * y[0] + R_last[i, 1] * y[1]) + R_last[i, 2] * y[2]) + t_last[i] for i in range(3)])
            pts.append((next_id + n, a, b, 1, X))
            n += 1
    return pts


def vo_run(pairs, n_frames, k0, pnp_fn, ba_fn, min_pnp_point_count=7, max_error=0.5):
    """the whole loop over solver callbacks: pnp_fn(f, X, uv_keys) -> (ok, R, t, inliers), ba_fn(f, pts) -> (ok, error, R, t,
    points).  Returns states, maps (one dict per frame) and the per-step problems."""
    states, maps, steps = [NOT_REACHED] * n_frames, [dict() for _ in range(n_frames)], {}
    states[k0] = INIT
    if not pairs[k0]["valid"]:
        states[k0 + 1] = LOST_PNP
        return states, maps, steps
    states[k0 + 1] = INIT
    maps[k0 + 1], next_id = vo_init(pairs[k0])
    R_l, t_l = pairs[k0]["R"], pairs[k0]["t"]
    for f in range(k0 + 2, n_frames):
        pair = pairs[f - 1]
        cands = vo_join(pair, maps[f - 1])
        ok, R_p, t_p, inl = pnp_fn(f, cands) if len(cands) >= 7 else (False, None, None, [])
        if not ok:
            states[f] = LOST_PNP
            break
        if len(inl) < min_pnp_point_count:
            states[f] = LOST_FEW
            break
        pts = vo_assemble(pair, maps[f - 1], cands, inl, R_l, t_l, vo_scale(t_p, t_l), next_id)
        next_id += sum(p[3] for p in pts)
        steps[f] = dict(cands=cands, inliers=inl, points=pts)
        ok, err, R_b, t_b, P = ba_fn(f, pts)
        if not ok:
            states[f] = LOST_BA
            break
        if err > max_error:
            states[f] = LOST_ERROR
            break
        states[f], R_l, t_l = TRACKED, R_b, t_b
        maps[f] = {p[2]: (p[0], P[i]) for i, p in enumerate(pts)}
    return states, maps, steps


# ---------------------------------------------------------------------------------------------------------------------
# CPU

def test_track_struct_layout_and_symbols():
    """mvs_vo_params / mvs_track_frame: header <-> ctypes; the five new entry points are exported and the defaults are the
    reference's; the ABI version is still 4 (additions only)"""
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mvs_vo_params), offsetof(mvs_vo_params, use_refined_init),
         offsetof(mvs_vo_params, min_pnp_point_count), offsetof(mvs_vo_params, max_error), offsetof(mvs_vo_params, anchor_var),
         offsetof(mvs_vo_params, regulator_var), offsetof(mvs_vo_params, point_sigma), offsetof(mvs_vo_params, sigma_px),
         sizeof(mvs_track_frame));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(mvs_track_frame, n_cand),
         offsetof(mvs_track_frame, n_pnp_inliers), offsetof(mvs_track_frame, n_tracked), offsetof(mvs_track_frame, n_new),
         offsetof(mvs_track_frame, pnp_best_hyp), offsetof(mvs_track_frame, iterations), offsetof(mvs_track_frame, reserved),
         offsetof(mvs_track_frame, scale), offsetof(mvs_track_frame, error), offsetof(mvs_track_frame, R_pnp),
         offsetof(mvs_track_frame, t_pnp), offsetof(mvs_track_frame, R), offsetof(mvs_track_frame, t));
  printf("%d %d %d %d %d %d %d\n", MVS_TRACK_NOT_REACHED, MVS_TRACK_INIT, MVS_TRACK_TRACKED, MVS_TRACK_LOST_PNP,
         MVS_TRACK_LOST_FEW, MVS_TRACK_LOST_BA, MVS_TRACK_LOST_ERROR);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    P, T = capi.VoParams, capi.TRACK_FRAME_DTYPE
    assert v[:9] == [C.sizeof(P), P.use_refined_init.offset, P.min_pnp_point_count.offset, P.max_error.offset,
                     P.anchor_var.offset, P.regulator_var.offset, P.point_sigma.offset, P.sigma_px.offset, T.itemsize]
    assert v[9:22] == [T.fields[k][1] for k in ("n_cand", "n_pnp_inliers", "n_tracked", "n_new", "pnp_best_hyp", "iterations",
                                                "reserved", "scale", "error", "R_pnp", "t_pnp", "R", "t")]
    assert v[22:] == [capi.TRACK_NOT_REACHED, capi.TRACK_INIT, capi.TRACK_TRACKED, capi.TRACK_LOST_PNP, capi.TRACK_LOST_FEW,
                      capi.TRACK_LOST_BA, capi.TRACK_LOST_ERROR] == list(range(7))
    lib = capi.lib()
    for name in ("mvs_vo_params_default", "mvs_seq_track", "mvs_seq_download_track_frames", "mvs_seq_download_track_map",
                 "mvs_seq_download_track_step"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.mvs_abi_version() == 4
    p = capi.default_vo_params()
    assert (p.init_pair, p.use_refined_init, p.min_pnp_point_count, p.max_error) == (0, 0, 7, 0.5)
    assert list(p.anchor_var) == [1e-3, 1e-3] and list(p.regulator_var) == [1e-2, 1e-2]
    assert (p.point_sigma, p.sigma_px) == (1e-2, 0.5)


def _hand_pairs():
    """four frames of sixteen keypoints.  Pair 0 triangulates ten rows, two of them (points 3 and 7) with trainIdx 3: the
    later one is dropped, nine points start the map at frame 1's keypoints 0 .. 8.  Pair 1 carries those nine on (keypoint i
    -> i + 1) and triangulates keypoints 12 and 13 of frame 1, which the map does not hold: two new points.  Pair 2 carries
    everything on unchanged."""
    from oracle_lib import MATCH_DTYPE

    def pair(k, rows, point_idx):
        mt = np.zeros(len(rows), dtype=MATCH_DTYPE)
        mt["trainIdx"], mt["queryIdx"] = [r[0] for r in rows], [r[1] for r in rows]
        n = len(point_idx)
        return dict(valid=True, matches=mt, point_idx=np.array(point_idx, np.int64),
                    points=np.arange(3.0 * n).reshape(n, 3) + 100.0 * k + 1.0, R=np.eye(3), t=np.array([0.1 * (k + 1), 0.0, 0.0]))

    rows0 = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (3, 15), (7, 7), (8, 8), (9, 14)]
    rows1 = [(i, i + 1) for i in range(9)] + [(12, 12), (13, 13), (14, 0)]
    rows2 = [(i, i) for i in range(14)]
    return [pair(0, rows0, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]),            # row 10 is not triangulated
            pair(1, rows1, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]),        # row 11 is not triangulated
            pair(2, rows2, list(range(14)))]


def test_model_on_a_hand_written_pair_table():
    pairs = _hand_pairs()
    assert [a for _, a, _ in kept_points(pairs[0])] == [0, 1, 2, 3, 4, 5, 6, 7, 8]      # the twin (point 7, trainIdx 3) is dropped
    m1, nid = vo_init(pairs[0])
    assert nid == 9 and sorted(m1) == list(range(9)) and 15 not in m1
    assert m1[7][0] == 7 and np.array_equal(m1[7][1], pairs[0]["points"][8])             # ids are ranks among the kept points

    R_p, t_p = np.eye(3), np.array([0.5, 0.0, 0.0])

    def pnp_fn(f, cands):       # candidate 2 is the outlier of every step
        return True, R_p, t_p, [c for c in range(len(cands)) if c != 2]

    def ba_fn(f, pts):
        return True, 0.1 * f, R_p, t_p * f, np.stack([p[4] for p in pts]) + 0.5

    states, maps, steps = vo_run(pairs, 4, 0, pnp_fn, ba_fn)
    assert states == [INIT, INIT, TRACKED, TRACKED]
    s2 = steps[2]
    assert [(a, b) for a, b, _ in s2["cands"]] == [(i, i + 1) for i in range(9)]
    assert [p[:4] for p in s2["points"]] == [(i, i, i + 1, 0) for i in range(9) if i != 2] + [(9, 12, 12, 1), (10, 13, 13, 1)]
    scale = 0.4                                                                          # |t_pnp - t_last| = |0.5 - 0.1|
    assert abs(vo_scale(t_p, pairs[0]["t"]) - scale) < 1e-15
    want = vo_scale(t_p, pairs[0]["t"]) * pairs[1]["points"][9] + pairs[0]["t"]          # R_last = I
    assert np.allclose(s2["points"][8][4], want, rtol=0, atol=1e-13)
    # the outlier (keypoint 3 of frame 2) left the map, the new points entered it, everything holds the refined position
    assert sorted(maps[2]) == [1, 2] + list(range(4, 10)) + [12, 13] and maps[2][12][0] == 9
    assert np.array_equal(maps[2][1][1], m1[0][1] + 0.5)
    # next step: keypoint 3 has no map entry any more, so pair 2's point at trainIdx 3 comes back as a NEW point with a new id;
    # so do keypoints 0, 10 and 11
    s3 = steps[3]
    assert [a for a, _, _ in s3["cands"]] == [1, 2] + list(range(4, 10)) + [12, 13]
    assert [(p[0], p[1]) for p in s3["points"] if p[3]] == [(11, 0), (12, 3), (13, 10), (14, 11)]
    assert 4 not in [p[1] for p in s3["points"]]                                         # candidate 2 of this step (keypoint 4)
    # the gates
    assert vo_run(pairs, 4, 0, pnp_fn, ba_fn, min_pnp_point_count=9)[0] == [INIT, INIT, LOST_FEW, NOT_REACHED]
    assert vo_run(pairs, 4, 0, pnp_fn, ba_fn, max_error=0.25)[0] == [INIT, INIT, TRACKED, LOST_ERROR]
    assert vo_run(pairs, 4, 0, lambda f, c: (False, None, None, []), ba_fn)[0] == [INIT, INIT, LOST_PNP, NOT_REACHED]
    assert vo_run(pairs, 4, 0, pnp_fn, lambda f, p: (False, 0.0, None, None, None))[0] == [INIT, INIT, LOST_BA, NOT_REACHED]
    bad = [dict(p) for p in pairs]
    bad[1]["valid"] = False
    st, mp, _ = vo_run(bad, 4, 0, pnp_fn, ba_fn)
    assert st == [INIT, INIT, LOST_PNP, NOT_REACHED] and mp[2] == {} and mp[3] == {}
    st, mp, _ = vo_run(pairs, 4, 1, pnp_fn, ba_fn)                                      # a later init pair: ids start at 0
    assert st == [NOT_REACHED, INIT, INIT, TRACKED] and sorted(v[0] for v in mp[2].values()) == list(range(11))


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def _octaves(n_frames=N_FRAMES, n_kp=N_KP):
    return (np.arange(n_frames * n_kp).reshape(n_frames, n_kp) % 3).astype(np.uint8)


def _pnp_params(refit=0, seed=None):
    from mvslam_amd import capi

    return capi.default_pnp_params(num_hypotheses=PPRM["H"], seed=PPRM["seed"] if seed is None else seed,
                                   reproj_error=PPRM["err"], refit=refit)


def _snapshot(s):
    """everything the three downloads give, per frame"""
    fr = s.download_track_frames()
    return dict(frames=fr, steps=[s.download_track_step(f, fr[f]) for f in range(s.n_frames)],
                maps=[s.download_track_map(f) for f in range(s.n_frames)])


def _frame_bytes(snap, f):
    m = snap["maps"][f]
    return snap["frames"][f].tobytes() + snap["steps"][f]["raw"] + m["point_id"].tobytes() + m["X"].tobytes()


def _map_of(m):
    return {int(i): (int(m["point_id"][i]), m["X"][i]) for i in np.nonzero(m["point_id"] >= 0)[0]}


def _replay(ctx, snap, dev, vo, pnp, refine, init_points=None, init_pose=None):
    """every frame of a downloaded run against the definition, each step from the device's own previous state"""
    fr, k0, K = snap["frames"], vo.init_pair, dev["K"]
    kp, octv, pairs = dev["kp"], dev["octave"], dev["pairs"]
    n_frames = len(fr)
    empty = lambda f: np.all(snap["maps"][f]["point_id"] == -1) and not np.any(snap["maps"][f]["X"])
    for f in range(k0):
        assert fr[f]["state"] == NOT_REACHED and fr[f].tobytes() == bytes(fr.itemsize) and empty(f)
    assert fr[k0]["state"] == INIT and np.array_equal(fr[k0]["R"], np.eye(3)) and not np.any(fr[k0]["t"]) and empty(k0)
    p0 = pairs[k0]
    assert p0["valid"] and fr[k0 + 1]["state"] == INIT
    want_map, next_id = vo_init(p0, init_points)
    R0, t0 = (dev["results"][k0]["R"], dev["results"][k0]["t"]) if init_pose is None else init_pose
    assert fr[k0 + 1]["R"].tobytes() == R0.tobytes() and fr[k0 + 1]["t"].tobytes() == t0.tobytes()
    assert fr[k0 + 1]["n_new"] == next_id
    got = _map_of(snap["maps"][k0 + 1])
    assert sorted(got) == sorted(want_map)
    for b, (i, x) in want_map.items():
        assert got[b][0] == i and got[b][1].tobytes() == np.asarray(x).tobytes()
    ended = False
    for f in range(k0 + 2, n_frames):
        rec, st = fr[f], snap["steps"][f]
        if ended:
            assert rec.tobytes() == bytes(fr.itemsize) and empty(f) and st["raw"] == bytes(len(st["raw"]))
            continue
        pair, map_prev = pairs[f - 1], _map_of(snap["maps"][f - 1])
        R_l, t_l = fr[f - 1]["R"], fr[f - 1]["t"]
        # 1 candidates
        cands = vo_join(pair, map_prev)
        assert rec["n_cand"] == len(cands)
        assert st["cand_base_kp"].tolist() == [c[0] for c in cands] and st["cand_new_kp"].tolist() == [c[1] for c in cands]
        assert st["cand_xyz"].tobytes() == np.array([c[2] for c in cands]).reshape(-1, 3).tobytes()
        assert st["cand_uv"].tobytes() == kp[f][st["cand_new_kp"]].astype(np.float64).tobytes()
        # 2 PnP: mvs_pnp_solve on the downloaded candidates
        pp = _pnp_params(pnp.refit, pnp.seed + f)
        one = ctx.pnp_solve(st["cand_xyz"], st["cand_uv"], K, pp) if len(cands) >= 7 else dict(ok=False, best_hyp=-1)
        assert rec["pnp_best_hyp"] == one["best_hyp"]
        if not one["ok"]:
            assert rec["state"] == LOST_PNP and empty(f) and rec["n_pnp_inliers"] == 0 and rec["n_tracked"] == rec["n_new"] == 0
            ended = True
            continue
        assert rec["R_pnp"].tobytes() == one["R"].tobytes() and rec["t_pnp"].tobytes() == one["t"].tobytes()
        assert rec["n_pnp_inliers"] == len(one["inliers"]) and np.array_equal(st["pnp_inliers"], one["inliers"])
        # 3 scale
        scale = vo_scale(rec["t_pnp"], t_l)
        print("frame %d: %d candidates, %d inliers, scale %.6f (error %.1e)" % (f, len(cands), len(one["inliers"]),
                                                                             rec["scale"], abs(rec["scale"] - scale)))
        assert abs(rec["scale"] - scale) <= 1e-12 * max(1.0, abs(scale))
        # 4 gate
        if len(one["inliers"]) < vo.min_pnp_point_count:
            assert rec["state"] == LOST_FEW and empty(f) and rec["n_tracked"] == rec["n_new"] == 0
            ended = True
            continue
        # 5 points
        pts = vo_assemble(pair, map_prev, cands, [int(c) for c in one["inliers"]], R_l, t_l, scale, next_id)
        n_new = sum(p[3] for p in pts)
        next_id += n_new
        assert (rec["n_tracked"], rec["n_new"]) == (len(pts) - n_new, n_new)
        assert st["point_id"].tolist() == [p[0] for p in pts] and st["point_kp"].tolist() == [[p[1], p[2]] for p in pts]
        assert st["point_is_new"].tolist() == [p[3] for p in pts]
        want = np.array([p[4] for p in pts]).reshape(-1, 3)
        nt = len(pts) - n_new
        assert st["point_guess"][:nt].tobytes() == want[:nt].tobytes()              # tracked: the map's position
        err = np.abs(st["point_guess"][nt:] - want[nt:])
        print("frame %d: %d tracked, %d new, guess error %.2e" % (f, nt, n_new, err.max() if err.size else 0.0))
        assert np.all(err <= 1e-12 * np.maximum(1.0, np.abs(want[nt:])))
        assert st["guess_pose"][0].tobytes() == R_l.tobytes() + t_l.tobytes()
        assert st["guess_pose"][1].tobytes() == rec["R_pnp"].tobytes() + rec["t_pnp"].tobytes()
        # 6 BA: mvs_ba_refine on the downloaded problem
        a, b = st["point_kp"][:, 0], st["point_kp"][:, 1]
        cov = []
        for frame, idx in ((f - 1, a), (f, b)):
            sd = np.ldexp(float(vo.sigma_px), octv[frame][idx].astype(np.int32))
            cov.append(np.stack([sd * sd, np.zeros(len(pts)), np.zeros(len(pts)), sd * sd], 1))
        pv = vo.point_sigma * vo.point_sigma
        prior = np.where(st["point_is_new"][:, None] == 1, 0.0, np.tile((np.eye(3) * pv).reshape(9), (len(pts), 1)))
        var = [[vo.anchor_var[0]] * 3 + [vo.anchor_var[1]] * 3, [vo.regulator_var[0]] * 3 + [vo.regulator_var[1]] * 3]
        ref = ctx.ba_refine(K, st["guess_pose"], var, st["point_guess"], prior,
                            [kp[f - 1][a].astype(np.float64), kp[f][b].astype(np.float64)], cov, [st["point_is_new"], None], refine)
        ba = st["ba_frames"]
        assert bool(ba["ok"][1]) == ref["ok"] and ba["R"].tobytes() == ref["R"].tobytes() and ba["t"].tobytes() == ref["t"].tobytes()
        assert st["points_refined"].tobytes() == ref["points"].tobytes()
        assert (rec["error"], rec["iterations"]) == (ref["error"], ref["iterations"]) == (ba["error"][1], ba["iterations"][1])
        print("frame %d: BA error %.6e after %d iterations" % (f, rec["error"], rec["iterations"]))
        if not ref["ok"] or rec["error"] > vo.max_error:
            assert rec["state"] == (LOST_ERROR if ref["ok"] else LOST_BA) and empty(f) and not np.any(rec["R"])
            ended = True
            continue
        # 7 commit
        assert rec["state"] == TRACKED and rec["R"].tobytes() == ref["R"][1].tobytes() and rec["t"].tobytes() == ref["t"][1].tobytes()
        got = _map_of(snap["maps"][f])
        assert sorted(got) == sorted(int(x) for x in b)
        for i, p in enumerate(pts):
            assert got[p[2]][0] == p[0] and got[p[2]][1].tobytes() == ref["points"][i].tobytes()
        assert not np.any(snap["maps"][f]["X"][snap["maps"][f]["point_id"] < 0])


def _run(ctx, seq, **kw):
    s, dev = sw._run(ctx, seq, **kw)
    dev["results"] = s.download_pairs()["results"]
    for p, r in zip(dev["pairs"], dev["results"]):
        p["R"], p["t"] = r["R"], r["t"]
    return s, dev


@pytest.fixture(scope="module")
def resident(ctx):
    """this file's sequence: 6 frames of 300 keypoints, octaves 0 .. 2, run once"""
    seq = make_seq()
    s, dev = _run(ctx, seq, octave=_octaves())
    yield s, dev, seq
    s.close()


@pytest.fixture(scope="module")
def base(ctx, resident):
    """the run the loss tests compare with: init_pair 0, max_error 1e30"""
    from mvslam_amd import capi

    s, dev, _ = resident
    vo = capi.default_vo_params(max_error=1e30)
    s.track(vo, _pnp_params(), capi.default_refine_params())
    return vo, _snapshot(s)


@pytest.mark.gpu
def test_gpu_track_replay(ctx, resident, base):
    from mvslam_amd import capi

    _, dev, _ = resident
    vo, snap = base
    print("states", snap["frames"]["state"].tolist())
    _replay(ctx, snap, dev, vo, _pnp_params(), capi.default_refine_params())
    assert all(snap["frames"]["state"][2:4] == TRACKED), "the fixture loses track before frame 4: the test shows nothing"
    assert all(snap["frames"]["n_new"][2:4] > 0) and all(snap["frames"]["n_tracked"][2:4] >= 7)
    assert any(snap["frames"]["n_pnp_inliers"][2:4] < snap["frames"]["n_cand"][2:4])     # a PnP outlier left the map


@pytest.mark.gpu
@pytest.mark.parametrize("refit,refined", [(1, 0), (0, 1)])
def test_gpu_track_replay_refit_and_refined_init(ctx, resident, refit, refined):
    from mvslam_amd import capi

    s, dev, _ = resident
    vo, rp = capi.default_vo_params(max_error=1e30, use_refined_init=refined), capi.default_refine_params()
    pts = pose = None
    if refined:
        s.refine_pairs(rp, 0.5)
        r = s.download_refined()
        assert r["refined"]["ok"][0] == 1
        n = len(dev["pairs"][0]["point_idx"])
        pts, pose = r["points"][0][:n], (r["refined"]["R"][0], r["refined"]["t"][0])
        assert pts.tobytes() != dev["pairs"][0]["points"].tobytes()
    s.track(vo, _pnp_params(refit), rp)
    snap = _snapshot(s)
    print("states", snap["frames"]["state"].tolist())
    _replay(ctx, snap, dev, vo, _pnp_params(refit), rp, init_points=pts, init_pose=pose)
    assert all(snap["frames"]["state"][2:4] == TRACKED)


@pytest.mark.gpu
def test_gpu_track_later_init_pair_is_the_shorter_sequence(ctx, resident):
    """init_pair = 2: frames 0 - 1 are not reached, ids start at 0, and the steps are byte for byte those of a sequence that
    holds only frames 2 - 5 with the sampler keys shifted by 2 (the pairs' key is seed + pair, the PnP's seed + frame)"""
    from mvslam_amd import capi

    s, dev, seq = resident
    vo, rp = capi.default_vo_params(max_error=1e30, init_pair=2), capi.default_refine_params()
    s.track(vo, _pnp_params(), rp)
    snap = _snapshot(s)
    _replay(ctx, snap, dev, vo, _pnp_params(), rp)
    assert snap["frames"]["state"].tolist()[:5] == [NOT_REACHED, NOT_REACHED, INIT, INIT, TRACKED]
    ids = snap["maps"][3]["point_id"]
    assert sorted(ids[ids >= 0]) == list(range(int(snap["frames"]["n_new"][3])))
    short = capi.Sequence(ctx, 4, N_KP, 32)
    try:
        short.upload(0, seq["desc"][2:], seq["kp"][2:], seq["n_kp"][2:], seq["K"])
        short.upload_octaves(0, _octaves()[2:])
        short.run(capi.default_params(num_hypotheses=PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=PRM["seed"] + 2,
                                      max_error_sq=PRM["thr"]), _pnp_params(seed=PPRM["seed"] + 2))
        got = short.download_pairs()
        for k in ("results", "matches", "mask", "points", "point_idx"):
            assert got[k].tobytes() == s.download_pairs()[k][2:].tobytes(), "the shorter sequence's pairs differ: " + k
        short.track(capi.default_vo_params(max_error=1e30), _pnp_params(seed=PPRM["seed"] + 2), rp)
        ssnap = _snapshot(short)
    finally:
        short.close()
    assert _frame_bytes(snap, 4) == _frame_bytes(ssnap, 2)
    assert _frame_bytes(snap, 5) == _frame_bytes(ssnap, 3)


@pytest.mark.gpu
def test_gpu_track_lost_pnp(ctx, resident, base):
    """frame 4 has five keypoints: pairs 3 and 4 are invalid, step 4 (pair 3) finds no candidates"""
    from mvslam_amd import capi

    _, _, seq = resident
    vo, bsnap = base
    n_kp = seq["n_kp"].copy()
    n_kp[4] = 5
    s, dev = _run(ctx, seq, n_kp=n_kp, octave=_octaves())
    try:
        assert dev["pairs"][2]["valid"] and not dev["pairs"][3]["valid"]
        s.track(vo, _pnp_params(), capi.default_refine_params())
        snap = _snapshot(s)
    finally:
        s.close()
    assert snap["frames"]["state"].tolist() == [INIT, INIT, TRACKED, TRACKED, LOST_PNP, NOT_REACHED]
    _replay(ctx, snap, dev, vo, _pnp_params(), capi.default_refine_params())
    for f in range(4):
        assert _frame_bytes(snap, f) == _frame_bytes(bsnap, f), f
    assert snap["frames"][4]["n_cand"] == 0 and snap["frames"][4]["pnp_best_hyp"] == -1
    for f in (4, 5):
        assert np.all(snap["maps"][f]["point_id"] == -1) and not np.any(snap["maps"][f]["X"])
    assert snap["frames"][5].tobytes() == bytes(snap["frames"].itemsize) and snap["steps"][5]["raw"] == bytes(len(snap["steps"][5]["raw"]))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["error_half", "error_between", "few"])
def test_gpu_track_lost_error_and_lost_few(ctx, resident, base, which):
    """The gates, from the figures the base run recorded.  The earlier steps do not depend on a gate's value, so the frame that
    is lost is the first whose recorded figure misses it.
    error_half: max_error = half the error of step 3.  On this generator the errors of consecutive steps are alike (no seed
    of 0 .. 79 gives step 3 twice step 2's error in the oracle), so that value already closes the gate at step 2;
    error_between: a value between the errors of steps 2 and 3 gives LOST_ERROR exactly at step 3;
    few: min_pnp_point_count = step 3's n_pnp_inliers + 1 gives LOST_FEW exactly at step 3."""
    from mvslam_amd import capi

    s, dev, _ = resident
    vo0, bsnap = base
    bf = bsnap["frames"]
    rec = bf[3]
    assert rec["state"] == TRACKED and rec["error"] > 0.0
    if which == "few":
        vo, want = capi.default_vo_params(max_error=1e30, min_pnp_point_count=int(rec["n_pnp_inliers"]) + 1), LOST_FEW
        lost = min(f for f in range(2, N_FRAMES) if bf[f]["n_pnp_inliers"] < vo.min_pnp_point_count)
        assert lost == 3
    else:
        assert bf[2]["error"] < rec["error"]
        vo = capi.default_vo_params(max_error=0.5 * float(rec["error"]) if which == "error_half" else
                                    0.5 * (float(bf[2]["error"]) + float(rec["error"])))
        want = LOST_ERROR
        lost = min(f for f in range(2, N_FRAMES) if bf[f]["error"] > vo.max_error)
        print("errors", bf["error"][2:].tolist(), "max_error", vo.max_error, "lost at", lost)
        assert lost == (3 if which == "error_between" else 2)
    s.track(vo, _pnp_params(), capi.default_refine_params())
    snap = _snapshot(s)
    assert snap["frames"]["state"].tolist() == [INIT, INIT] + [TRACKED] * (lost - 2) + [want] + [NOT_REACHED] * (N_FRAMES - 1 - lost)
    _replay(ctx, snap, dev, vo, _pnp_params(), capi.default_refine_params())
    for f in range(lost):
        assert _frame_bytes(snap, f) == _frame_bytes(bsnap, f), f
    for f in range(lost, N_FRAMES):
        assert np.all(snap["maps"][f]["point_id"] == -1) and not np.any(snap["maps"][f]["X"])
    got, rec = snap["frames"][lost], bf[lost]
    assert (got["n_cand"], got["n_pnp_inliers"], got["scale"]) == (rec["n_cand"], rec["n_pnp_inliers"], rec["scale"])
    if want == LOST_ERROR:
        assert (got["error"], got["iterations"]) == (rec["error"], rec["iterations"])


@pytest.mark.gpu
def test_gpu_track_refusals_determinism_and_no_side_effects(ctx, resident):
    from mvslam_amd import capi

    s, dev, seq = resident

    def status_of(fn, *a):
        with pytest.raises(capi.MvsError) as e:
            fn(*a)
        return e.value.status

    before = (s.download_pairs(), s.download_tracks(), s.download_trajectory())
    vo, rp = capi.default_vo_params(max_error=1e30), capi.default_refine_params()
    runs = []
    for _ in range(2):
        s.track(vo, _pnp_params(), rp)
        snap = _snapshot(s)
        runs.append(b"".join(_frame_bytes(snap, f) for f in range(N_FRAMES)))
    assert runs[0] == runs[1]
    after = (s.download_pairs(), s.download_tracks(), s.download_trajectory())
    for x, y in zip(before, after):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k
    bad = [dict(init_pair=-1), dict(init_pair=N_FRAMES - 1), dict(sigma_px=0.0), dict(sigma_px=-0.5), dict(point_sigma=0.0),
           dict(anchor_var=(0.0, 1e-3)), dict(anchor_var=(1e-3, -1.0)), dict(regulator_var=(0.0, 1e-2)),
           dict(regulator_var=(1e-2, 0.0))]
    for kw in bad:
        assert status_of(s.track, capi.default_vo_params(**kw), _pnp_params(), rp) == capi.MVS_ERR_INVALID_ARG, kw
    s.track(capi.default_vo_params(init_pair=N_FRAMES - 2), _pnp_params(), rp)          # the last pair is a legal init pair
    assert s.download_track_frames()["state"].tolist() == [NOT_REACHED] * 4 + [INIT, INIT]
    for frame in (-1, N_FRAMES):
        assert status_of(s.download_track_map, frame) == capi.MVS_ERR_INVALID_ARG
        assert status_of(s.download_track_step, frame, snap["frames"][0]) == capi.MVS_ERR_INVALID_ARG
    fresh = capi.Sequence(ctx, N_FRAMES, N_KP, 32)                                       # uploaded, never run
    try:
        fresh.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
        fresh.upload_octaves(0, _octaves())
        assert status_of(fresh.track, vo, _pnp_params(), rp) == capi.MVS_ERR_INVALID_ARG
        assert status_of(fresh.download_track_frames) == capi.MVS_ERR_INVALID_ARG
        fresh.run(capi.default_params(num_hypotheses=PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=PRM["seed"],
                                      max_error_sq=PRM["thr"]), _pnp_params())
        # run, but no mvs_seq_refine_pairs results are resident
        assert status_of(fresh.track, capi.default_vo_params(use_refined_init=1), _pnp_params(), rp) == capi.MVS_ERR_INVALID_ARG
        fresh.track(vo, _pnp_params(), rp)                  # another sequence, same data and parameters: the fixture's bytes
        snap2 = _snapshot(fresh)
        assert b"".join(_frame_bytes(snap2, f) for f in range(N_FRAMES)) == runs[0]
        # refined pairs belong to the run they refined: a second run makes use_refined_init illegal again
        fresh.refine_pairs(rp, 0.5)
        fresh.track(capi.default_vo_params(max_error=1e30, use_refined_init=1), _pnp_params(), rp)
        fresh.run(capi.default_params(num_hypotheses=PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=PRM["seed"],
                                      max_error_sq=PRM["thr"]), _pnp_params())
        assert status_of(fresh.track, capi.default_vo_params(use_refined_init=1), _pnp_params(), rp) == capi.MVS_ERR_INVALID_ARG
        assert status_of(fresh.download_track_frames) == capi.MVS_ERR_INVALID_ARG      # nor are the last run's tracking results
    finally:
        fresh.close()
