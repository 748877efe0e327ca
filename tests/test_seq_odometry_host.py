"""VisualOdometer::add_frame over a resident sequence (mvs_seq_run_lags, mvs_seq_odometry): the CPU part.

The header / ctypes layout of mvs_vo_init_params and mvs_odo_frame, the new symbols and MVS_TRACK_INITIALIZING; and the
definition of the state machine restated in numpy (the frame queue, the held pairs, ImagePair::update, check_image_pair, the
choice, reset) and run over hand-written pair tables with stand-in solvers.  tests/test_seq_odometry.py replays the device's
run against the same functions.

A table is tables[lag][b] = dict(valid, count, ssd, ok, error, R, t): pair (b, b + lag)'s validity, n_points and match_ssd,
and its refinement's ok / error / pose.

One branch the definition has cannot be reached by a run: "a passing held pair whose pair frame is not f is skipped".  A held
pair (b, p) is entered or replaced while frame p is processed, the gates' values do not change afterwards, and the scan of
frame p itself would have initialised from it (or from an older entry).  odo_choose is therefore also called directly on a
hand-built held table.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import test_seq_track as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_REACHED, INIT, TRACKED, LOST_PNP, LOST_FEW, LOST_BA, LOST_ERROR, INITIALIZING = range(8)
LOST = (LOST_PNP, LOST_FEW, LOST_BA, LOST_ERROR)
INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# the definition, in numpy

def so3_ln_sq(R):
    """squared norm of SO3::ln (mvslam_compat.hpp:176-184) in its operation order"""
    c = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
    c = -1.0 if c < -1.0 else (1.0 if c > 1.0 else c)
    theta = float(np.arccos(c))
    v = (R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1])
    A = (1.0 + theta * theta / 6.0) * 0.5 if theta < 1e-5 else 0.5 * theta / float(np.sin(theta))
    w = [x * A for x in v]
    return (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]


def odo_check(h, b, tables, gates):
    """check_image_pair of a held pair: (code, rot_sq, abs_tz); code 0 passed, else the first failing gate in the order of
    visual-odometer.cpp:353-379"""
    if not h["valid"]:
        return 1, 0.0, 0.0
    e = tables[h["lag"]][b]
    rot_sq, abs_tz = so3_ln_sq(np.asarray(e["R"])), abs(float(e["t"][2]))
    if h["count"] < gates["min_inliers"]:
        return 2, rot_sq, abs_tz
    if h["error"] > gates["max_error"]:
        return 3, rot_sq, abs_tz
    if rot_sq > gates["max_rot"] * gates["max_rot"]:
        return 4, rot_sq, abs_tz
    if abs_tz > gates["max_tz"]:
        return 5, rot_sq, abs_tz
    return 0, rot_sq, abs_tz


def odo_newest(f, tables):
    """held[f - 1] as frame f enters it: the adjacent pair, refined when valid"""
    e = tables[1][f - 1]
    h = dict(pair=f, lag=1, valid=bool(e["valid"]), count=int(e["count"]) if e["valid"] else 0,
             ssd=int(e["ssd"]) if e["valid"] else 0, error=INF, refined=False)
    if h["valid"]:
        h["valid"] = h["refined"] = bool(e["ok"])
        if e["ok"]:
            h["error"] = float(e["error"])
    return h


def odo_update(h, b, f, tables):
    """ImagePair::update of held[b] with the lagged pair (b, f): the entry afterwards and whether it was replaced"""
    e = tables[f - b][b]
    if not e["valid"]:
        return h, False
    if e["count"] < h["count"] or e["ssd"] < h["ssd"]:
        return h, False
    err = float(e["error"]) if e["ok"] else INF
    if err < h["error"]:
        return dict(pair=f, lag=f - b, valid=True, count=int(e["count"]), ssd=int(e["ssd"]), error=err, refined=True), True
    return h, False


def odo_choose(held, qf, f, tables, gates):
    """the scan, oldest first: (chosen base or -1, gate code of the newest pair, rot_sq, abs_tz)"""
    code_new, rot, tz = 0, 0.0, 0.0
    for b in range(qf, f):
        code, r2, az = odo_check(held[b], b, tables, gates)
        if b == f - 1:
            code_new, rot, tz = code, r2, az
        if code == 0 and held[b]["pair"] == f:
            return b, 0, r2, az
    return -1, code_new, rot, tz


def odo_run(tables, n_frames, Q, gates, step_fn, init_fn=None):
    """the whole state machine.  step_fn(f) -> the state the tracking step of frame f ends in (TRACKED or LOST_*);
    init_fn(f, b, lag) is told about every initialisation.  Returns states, one record per frame (the fields of
    mvs_odo_frame) and the held table as it stood after every frame."""
    states = [NOT_REACHED] * n_frames
    recs = [dict(mode_after=0, segment=-1, init_base=-1, queue_first=0, n_updated=0, gate_fail=0, rot_sq=0.0, abs_tz=0.0)]
    held, held_log = {}, [{}]
    tracking, q0, seg = False, 0, -1
    for f in range(1, n_frames):
        qf = max(q0, f - Q)
        rec = dict(mode_after=0, segment=seg, init_base=-1, queue_first=qf, n_updated=0, gate_fail=0, rot_sq=0.0, abs_tz=0.0)
        if tracking:
            states[f] = step_fn(f)
            assert states[f] == TRACKED or states[f] in LOST
            tracking = states[f] == TRACKED
            rec["mode_after"] = int(tracking)
            q0 = max(q0, f - Q + 1) if tracking else f     # reset() keeps the lost frame
            if not tracking:
                held = {}
        else:
            held[f - 1] = odo_newest(f, tables)
            for b in range(qf, f - 1):
                held[b], replaced = odo_update(held[b], b, f, tables)
                rec["n_updated"] += int(replaced)
            b, rec["gate_fail"], rec["rot_sq"], rec["abs_tz"] = odo_choose(held, qf, f, tables, gates)
            if b >= 0:
                seg += 1
                tracking = True
                rec.update(mode_after=1, segment=seg, init_base=b)
                if states[b] not in LOST:
                    states[b] = INIT
                states[f] = INIT
                if init_fn:
                    init_fn(f, b, held[b]["lag"])
            else:
                states[f] = INITIALIZING
            q0 = max(q0, f - Q + 1)
            held = {k: v for k, v in held.items() if k >= q0}
        recs.append(rec)
        held_log.append({k: dict(v) for k, v in held.items()})
    return states, recs, held_log


# ---------------------------------------------------------------------------------------------------------------------
# tests

def test_odometry_struct_layout_and_symbols():
    """mvs_vo_init_params / mvs_odo_frame: header <-> ctypes; the new entry points are exported, the defaults are the
    reference's, MVS_TRACK_INITIALIZING is 7 and the ABI version is still 4"""
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(mvs_vo_init_params), offsetof(mvs_vo_init_params, frame_queue_size),
         offsetof(mvs_vo_init_params, min_match_inlier_count), offsetof(mvs_vo_init_params, max_rotation_magnitude),
         offsetof(mvs_vo_init_params, max_translation_z));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mvs_odo_frame), offsetof(mvs_odo_frame, mode_after),
         offsetof(mvs_odo_frame, segment), offsetof(mvs_odo_frame, init_base), offsetof(mvs_odo_frame, queue_first),
         offsetof(mvs_odo_frame, n_updated), offsetof(mvs_odo_frame, gate_fail), offsetof(mvs_odo_frame, rot_sq),
         offsetof(mvs_odo_frame, abs_tz));
  printf("%d %d\n", MVS_TRACK_INITIALIZING, MVS_TRACK_LOST_ERROR);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    P, T = capi.VoInitParams, capi.ODO_FRAME_DTYPE
    assert v[:5] == [C.sizeof(P), P.frame_queue_size.offset, P.min_match_inlier_count.offset, P.max_rotation_magnitude.offset,
                     P.max_translation_z.offset]
    assert v[5:14] == [T.itemsize] + [T.fields[k][1] for k in ("mode_after", "segment", "init_base", "queue_first", "n_updated",
                                                               "gate_fail", "rot_sq", "abs_tz")]
    assert v[14:] == [capi.TRACK_INITIALIZING, capi.TRACK_LOST_ERROR] == [7, 6]
    lib = capi.lib()
    for name in ("mvs_seq_run_lags", "mvs_seq_download_lag_pairs", "mvs_seq_download_lag_refined", "mvs_vo_init_params_default",
                 "mvs_seq_odometry", "mvs_seq_download_odometry_frames"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.mvs_abi_version() == 4
    p = capi.default_vo_init_params()
    assert (p.frame_queue_size, p.min_match_inlier_count, p.max_rotation_magnitude, p.max_translation_z) == (10, 20, 0.1, 0.1)


GATES = dict(min_inliers=20, max_error=0.5, max_rot=0.1, max_tz=0.1)


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def good(**kw):
    """a pair that passes every gate of GATES"""
    e = dict(valid=True, count=30, ssd=100, ok=True, error=0.3, R=rot_z(0.01), t=np.array([1.0, 0.0, 0.01]))
    e.update(kw)
    return e


BAD = dict(valid=False, count=0, ssd=0, ok=False, error=0.0, R=np.eye(3), t=np.zeros(3))


def make_tables(n_frames, max_lag, entries):
    """every pair invalid except entries[(lag, b)]"""
    return {d: [dict(entries.get((d, b), BAD)) for b in range(n_frames - d)] for d in range(1, max_lag + 1)}


def always(state):
    return lambda f: state


def test_so3_ln_sq():
    assert so3_ln_sq(np.eye(3)) == 0.0
    for a in (1e-7, 1e-3, 0.1, 1.0, 3.0):                      # both branches of A
        assert abs(so3_ln_sq(rot_z(a)) - a * a) <= 1e-9 * a * a
    assert abs(so3_ln_sq(rot_z(0.2) @ rot_z(-0.05)) - 0.15 ** 2) <= 1e-12


def test_model_initialises_at_the_first_pair_and_tracks():
    states, recs, _ = odo_run(make_tables(5, 2, {(1, 0): good()}), 5, 2, GATES, always(TRACKED))
    assert states == [INIT, INIT, TRACKED, TRACKED, TRACKED]
    assert [r["segment"] for r in recs] == [-1, 0, 0, 0, 0] and [r["mode_after"] for r in recs] == [0, 1, 1, 1, 1]
    assert recs[1]["init_base"] == 0 and recs[1]["gate_fail"] == 0 and recs[1]["n_updated"] == 0
    assert abs(recs[1]["rot_sq"] - 1e-4) < 1e-12 and recs[1]["abs_tz"] == 0.01
    assert [r["queue_first"] for r in recs] == [0, 0, 0, 1, 2]


def test_model_gate_failures_in_order_on_the_newest_pair():
    """frames 1 .. 5: the newest pair fails gate 1 .. 5; frame 6 initialises.  A pair that fails two gates reports the first."""
    fails = {(1, 0): BAD, (1, 1): good(count=19), (1, 2): good(error=0.6), (1, 3): good(R=rot_z(0.11)),
             (1, 4): good(t=np.array([1.0, 0.0, -0.2])), (1, 5): good()}
    states, recs, _ = odo_run(make_tables(7, 2, fails), 7, 2, GATES, always(TRACKED))
    assert [r["gate_fail"] for r in recs] == [0, 1, 2, 3, 4, 5, 0]
    assert states == [NOT_REACHED] + [INITIALIZING] * 4 + [INIT, INIT] and recs[6]["init_base"] == 5
    assert recs[1]["rot_sq"] == 0.0 and abs(recs[4]["rot_sq"] - 0.0121) < 1e-12 and recs[5]["abs_tz"] == 0.2
    both = dict(fails)
    both[(1, 1)] = good(count=19, error=0.6, R=rot_z(0.5))
    assert odo_run(make_tables(7, 2, both), 7, 2, GATES, always(TRACKED))[1][2]["gate_fail"] == 2
    # a refinement with ok = 0 makes the newest pair invalid
    assert odo_run(make_tables(3, 2, {(1, 0): good(ok=False)}), 3, 2, GATES, always(TRACKED))[1][1]["gate_fail"] == 1
    # max_error "off"
    assert odo_run(make_tables(3, 2, {(1, 0): good(error=1e9)}), 3, 2, dict(GATES, max_error=INF), always(TRACKED))[0][1] == INIT


def test_model_update_refusals():
    """held[0] is valid but rotates too far, so nothing initialises and frames 2 .. 4 offer (0, f): refused for count, for
    ssd, for an error that is not smaller; then one that is accepted -- and initialises with base 0 at lag 5"""
    far = rot_z(0.3)
    e = {(1, 0): good(R=far), (2, 0): good(count=29, error=0.1), (3, 0): good(ssd=99, error=0.1), (4, 0): good(error=0.3),
         (5, 0): good(count=30, ssd=100, error=0.29)}
    states, recs, held = odo_run(make_tables(7, 5, e), 7, 6, GATES, always(TRACKED))
    assert [r["n_updated"] for r in recs] == [0, 0, 0, 0, 0, 1, 0]
    for f in (2, 3, 4):
        assert held[f][0] == held[1][0] and held[f][0]["pair"] == 1 and held[f][0]["lag"] == 1
    assert recs[5]["init_base"] == 0 and states == [INIT] + [INITIALIZING] * 4 + [INIT, TRACKED]
    assert [r["gate_fail"] for r in recs[1:5]] == [4, 1, 1, 1]
    # a candidate whose refinement failed counts as +inf and never replaces, not even an unrefined-invalid entry
    e2 = {(2, 0): good(ok=False)}
    _, recs2, held2 = odo_run(make_tables(4, 3, e2), 4, 3, GATES, always(TRACKED))
    assert recs2[2]["n_updated"] == 0 and not held2[2][0]["valid"]


def test_model_update_replaces_an_invalid_pair_and_initialises_with_an_older_base():
    states, recs, held = odo_run(make_tables(5, 2, {(2, 0): good(), (1, 2): good(), (1, 3): good()}), 5, 2, GATES, always(TRACKED))
    assert not held[1][0]["valid"] and (held[1][0]["count"], held[1][0]["ssd"], held[1][0]["error"]) == (0, 0, INF)
    assert recs[2]["n_updated"] == 1 and recs[2]["init_base"] == 0 and recs[2]["gate_fail"] == 0
    assert states == [INIT, INITIALIZING, INIT, TRACKED, TRACKED]                # frame 1 keeps INITIALIZING


def test_model_skips_a_passing_pair_whose_pair_frame_is_older():
    tables = make_tables(4, 3, {(1, 0): good(), (1, 2): good()})
    held = {0: dict(pair=1, lag=1, valid=True, count=30, ssd=100, error=0.3, refined=True), 1: odo_newest(2, tables),
            2: odo_newest(3, tables)}
    assert odo_check(held[0], 0, tables, GATES)[0] == 0
    assert odo_choose(held, 0, 3, tables, GATES)[0] == 2                           # 0 passes but pairs with frame 1; 1 is invalid
    held[2]["valid"] = False
    assert odo_choose(held, 0, 3, tables, GATES)[:2] == (-1, 1)


def test_model_loss_and_reinitialisation_from_the_lost_frame():
    e = {(1, b): good() for b in range(7)}
    lost_at = {3: LOST_BA}
    states, recs, _ = odo_run(make_tables(8, 2, e), 8, 2, GATES, lambda f: lost_at.get(f, TRACKED))
    assert states == [INIT, INIT, TRACKED, LOST_BA, INIT, TRACKED, TRACKED, TRACKED]   # the lost frame keeps its state
    assert [r["segment"] for r in recs] == [-1, 0, 0, 0, 1, 1, 1, 1]
    assert [r["mode_after"] for r in recs] == [0, 1, 1, 0, 1, 1, 1, 1]
    assert recs[4]["init_base"] == 3 and recs[4]["queue_first"] == 3
    # the pair behind the lost frame is bad: the queue starts at the lost frame and a lagged pair from it initialises
    e2 = dict(e)
    e2[(1, 3)], e2[(1, 4)], e2[(2, 3)] = BAD, BAD, good()
    states, recs, _ = odo_run(make_tables(8, 2, e2), 8, 2, GATES, lambda f: lost_at.get(f, TRACKED))
    assert states == [INIT, INIT, TRACKED, LOST_BA, INITIALIZING, INIT, TRACKED, TRACKED]
    assert recs[5]["init_base"] == 3 and recs[5]["n_updated"] == 1 and recs[5]["queue_first"] == 3
    # every kind of loss resets
    for kind in LOST:
        assert odo_run(make_tables(5, 2, e), 5, 2, GATES, lambda f: kind if f == 2 else TRACKED)[0] == [INIT, INIT, kind, INIT, TRACKED]


def test_model_queue_drops_its_oldest_frame_and_never_initialises():
    for Q, want in ((2, [0, 0, 0, 1, 2, 3]), (3, [0, 0, 0, 0, 1, 2])):
        states, recs, held = odo_run(make_tables(6, 3, {}), 6, Q, GATES, always(TRACKED))
        assert states == [NOT_REACHED] + [INITIALIZING] * 5
        assert [r["queue_first"] for r in recs] == want
        assert all(r["segment"] == -1 and r["mode_after"] == 0 and r["init_base"] == -1 and r["gate_fail"] == 1 for r in recs[1:])
        for f in range(1, 6):
            assert sorted(held[f]) == list(range(max(0, f - Q + 1), f))            # at most Q frames stay queued
    # a lagged pair one frame beyond the queue's reach is never offered: (0, 3) at Q = 2
    e = {(3, 0): good()}
    assert odo_run(make_tables(6, 3, e), 6, 2, GATES, always(TRACKED))[0] == [NOT_REACHED] + [INITIALIZING] * 5
    assert odo_run(make_tables(6, 3, e), 6, 3, GATES, always(TRACKED))[0][:4] == [INIT, INITIALIZING, INITIALIZING, INIT]


def test_model_with_stand_in_solvers_is_the_tracking_loop():
    """gates open, every lag-1 pair valid: the state machine around stand-in solvers gives the states and maps of
    test_seq_track.vo_run on its hand-written pair table"""
    pairs = st._hand_pairs()
    R_p, t_p = np.eye(3), np.array([0.5, 0.0, 0.0])
    pnp_fn = lambda f, cands: (True, R_p, t_p, [c for c in range(len(cands)) if c != 2])
    ba_fn = lambda f, pts: (True, 0.1 * f, R_p, t_p * f, np.stack([p[4] for p in pts]) + 0.5)
    want_states, want_maps, _ = st.vo_run(pairs, 4, 0, pnp_fn, ba_fn)
    tables = make_tables(4, 2, {(1, k): dict(valid=True, count=len(p["point_idx"]), ssd=0, ok=True, error=0.0, R=p["R"], t=p["t"])
                                for k, p in enumerate(pairs)})
    maps, loop = [dict() for _ in range(4)], dict(next_id=0)

    def init_fn(f, b, lag):
        assert lag == 1
        maps[f], n = st.vo_init(pairs[b])
        loop.update(R=pairs[b]["R"], t=pairs[b]["t"], next_id=loop["next_id"] + n)

    def step_fn(f):
        cands = st.vo_join(pairs[f - 1], maps[f - 1])
        ok, R, t, inl = pnp_fn(f, cands)
        pts = st.vo_assemble(pairs[f - 1], maps[f - 1], cands, inl, loop["R"], loop["t"], st.vo_scale(t, loop["t"]), loop["next_id"])
        loop["next_id"] += sum(p[3] for p in pts)
        ok, err, R_b, t_b, P = ba_fn(f, pts)
        loop.update(R=R_b, t=t_b)
        maps[f] = {p[2]: (p[0], P[i]) for i, p in enumerate(pts)}
        return TRACKED

    states, recs, _ = odo_run(tables, 4, 2, dict(min_inliers=0, max_error=INF, max_rot=INF, max_tz=INF), step_fn, init_fn)
    assert states == want_states == [INIT, INIT, TRACKED, TRACKED]
    for f in range(4):
        assert sorted(maps[f]) == sorted(want_maps[f])
        for b in maps[f]:
            assert maps[f][b][0] == want_maps[f][b][0] and np.array_equal(maps[f][b][1], want_maps[f][b][1])
