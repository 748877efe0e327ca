"""Latency of VisualOdometer::add_frame over a resident sequence, two routes:

  (a) mvs_seq_odometry: one call; initialisation from the frame queue, tracking, reset and re-initialisation of every frame
      on the device, timed with HIP events on the context's stream -- one pair of events around the whole call;
  (b) what a caller could do before: a host loop that calls mvs_seq_track(init_pair, refined initialisation), downloads the
      frame records, picks the next init_pair behind the loss (the first valid pair whose refinement is ok, from the lost
      frame on -- what Q = 2 with open gates does) and calls again until the sequence ends.  Wall clock: the round trips and the
      memsets of every call are the point.  The ratio quoted compares wall clock with wall clock (the one call is also
      timed that way: call, then wait for the stream).

mvs_seq_run_lags is timed separately (HIP events, one call).  Method of tools/vo_track_latency.py: one warm-up call, five
calls, all five quoted.  Also runs the five tsukuba frames (tests/golden/tsukuba_gray.npz) with the reference's default gates
and Q = 10 and reports which pair initialises and the pose of frame 4; reported, not asserted.
Writes profiles/vo_odometry_latency.json.  Usage: python tools/vo_odometry_latency.py [--frames 1000] [--kp 2000] [--queue 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvslam_amd import capi  # noqa: E402
from mvslam_amd import synth  # noqa: E402

STATES = ["NOT_REACHED", "INIT", "TRACKED", "LOST_PNP", "LOST_FEW", "LOST_BA", "LOST_ERROR", "INITIALIZING"]
OPEN = 1e30


def histogram(states):
    return {STATES[v]: int(np.sum(states == v)) for v in range(len(STATES)) if np.any(states == v)}


def recall_loop(s, vo_kw, pnp, rp, ok_pair):
    """route (b): returns (states of every frame, calls, wall ms, kernel launches enqueued).  A call with init pair k0 enqueues
    vo_init_kernel and the step's eight kernels for frames k0 + 2 .. n_frames - 1."""
    NF = s.n_frames
    states = np.zeros(NF, np.int32)
    t0 = time.perf_counter()
    k0, calls, launches = 0, 0, 0
    while k0 <= NF - 2:
        while k0 <= NF - 2 and not ok_pair[k0]:
            k0 += 1
        if k0 > NF - 2:
            break
        s.track(capi.default_vo_params(init_pair=k0, use_refined_init=1, **vo_kw), pnp, rp)
        fr = s.download_track_frames()
        calls += 1
        launches += 1 + 8 * (NF - k0 - 2)
        lost = [f for f in range(k0 + 2, NF) if fr[f]["state"] >= 3]
        end = lost[0] if lost else NF - 1
        states[k0:end + 1] = np.where(states[k0:end + 1] >= 3, states[k0:end + 1], fr["state"][k0:end + 1])
        if not lost:
            break
        k0 = lost[0]                                   # reset() keeps the lost frame: it is the next base
    return states, calls, (time.perf_counter() - t0) * 1e3, launches


def tsukuba(ctx):
    g = np.load(os.path.join(ROOT, "tests", "golden", "tsukuba_gray.npz"))
    imgs, K = g["images"], g["K"]
    s = capi.Sequence(ctx, len(imgs), 512, 32)
    s.upload_images(0, imgs, K, capi.default_orb_params())
    prm = capi.default_params(num_hypotheses=2000, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-3, max_dist=50.0)
    pnp = capi.default_pnp_params(num_hypotheses=100, seed=7, reproj_error=0.05)
    s.run(prm, pnp)
    s.run_lags(prm, len(imgs) - 1)
    s.odometry(capi.default_vo_params(), capi.default_vo_init_params(), pnp, capi.default_refine_params())
    fr, od = s.download_track_frames(), s.download_odometry_frames()
    inits = [(int(od[f]["init_base"]), f) for f in range(len(fr)) if od[f]["init_base"] >= 0]
    out = dict(states=[STATES[int(x)] for x in fr["state"]], initialising_pairs=inits, gate_fail=od["gate_fail"].tolist(),
               n_updated=od["n_updated"].tolist(), rot_sq=od["rot_sq"].tolist(), abs_tz=od["abs_tz"].tolist(),
               frame4_state=STATES[int(fr[4]["state"])], frame4_R=fr[4]["R"].tolist(), frame4_t=fr[4]["t"].tolist())
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--hyp", type=int, default=4096, help="two-view hypotheses per pair")
    ap.add_argument("--queue", type=int, default=3, help="frame_queue_size Q")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x5E9, help="of the generator")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_odometry_latency.json"))
    args = ap.parse_args()
    import torch

    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream.cuda_stream)
    NF, N, Q = args.frames, args.kp, args.queue

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    seq = synth.make_sequence(NF, n_kp=N, seed=args.seed)
    s = capi.Sequence(ctx, NF, N, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
    pnp = capi.default_pnp_params(num_hypotheses=100, seed=2, reproj_error=1.5)
    prm = capi.default_params(num_hypotheses=args.hyp, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=2e-3)
    s.run(prm, pnp)
    rp = capi.default_refine_params()
    s.run_lags(prm, Q, refine_params=rp)               # warm-up: the lag batches are created here
    ctx._check(capi.lib().mvs_seq_sync(s._h), "mvs_seq_sync")
    ms_lags = [timed(lambda: s.run_lags(prm, Q, refine_params=rp)) for _ in range(args.steps)]
    vo_kw = dict(max_error=OPEN)                       # the error gate is off, as in tools/vo_track_latency.py
    vo = capi.default_vo_params(**vo_kw)
    ip = capi.default_vo_init_params(frame_queue_size=Q, min_match_inlier_count=0, max_rotation_magnitude=OPEN,
                                     max_translation_z=OPEN)
    s.odometry(vo, ip, pnp, rp)                        # warm-up
    ctx._check(capi.lib().mvs_seq_sync(s._h), "mvs_seq_sync")
    ms_a = [timed(lambda: s.odometry(vo, ip, pnp, rp)) for _ in range(args.steps)]

    def wall_a():                                      # the clock route (b) is read with: call, then wait for the stream
        t0 = time.perf_counter()
        s.odometry(vo, ip, pnp, rp)
        ctx._check(capi.lib().mvs_seq_sync(s._h), "mvs_seq_sync")
        return (time.perf_counter() - t0) * 1e3

    ms_a_wall = [wall_a() for _ in range(args.steps)]
    fr, od = s.download_track_frames(), s.download_odometry_frames()
    processed = NF - 1
    launches = 8 + (3 if pnp.refit else 0) + 2
    gp, gr = s.download_lag_pairs(1), s.download_lag_refined(1, points=False)
    ok_pair = (gp["results"]["valid"] != 0) & (gr["refined"]["ok"] != 0)
    recall_loop(s, vo_kw, pnp, rp, ok_pair)            # warm-up
    runs_b = [recall_loop(s, vo_kw, pnp, rp, ok_pair) for _ in range(args.steps)]
    st_b, calls_b = runs_b[0][0], runs_b[0][1]
    ms_b = [r[2] for r in runs_b]
    res = dict(frames=NF, keypoints=N, frame_queue_size=Q, two_view_hypotheses=args.hyp, pnp_hypotheses=pnp.num_hypotheses,
               states=histogram(fr["state"]), segments=int(od["segment"].max()) + 1, frames_tracked=int(np.sum(fr["state"] == 2)),
               lagged_initialisations=int(np.sum((od["init_base"] >= 0) & (od["init_base"] < np.arange(NF) - 1))),
               pairs_updated=int(od["n_updated"].sum()),
               launches_per_frame=launches, launches_per_call=1 + 2 + launches * (NF - 2), memsets_per_call=3,
               run_lags_ms=dict(hip_events=ms_lags, best=min(ms_lags), lags=Q, pairs=sum(NF - d for d in range(2, Q + 1))),
               odometry_ms=dict(hip_events=ms_a, best=min(ms_a), wall=ms_a_wall, best_wall=min(ms_a_wall),
                                per_processed_frame=min(ms_a) / processed),
               recall_loop_ms=dict(wall=ms_b, best=min(ms_b), calls=calls_b, per_processed_frame=min(ms_b) / processed,
                                   states=histogram(st_b), launches_total=int(runs_b[0][3]),
                                   launches_first_call=1 + 8 * (NF - 2), memsets_per_call=2, memsets_total=2 * calls_b),
               recall_loop_over_one_call_wall=min(ms_b) / min(ms_a_wall), tsukuba=tsukuba(ctx))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
