"""Latency of the tracking loop of a resident sequence, two routes:

  (a) mvs_seq_track: join, PnP, assembly, BA and commit of every frame on the device, timed with HIP events on the context's
      stream -- one pair of events around the whole call, no synchronisation inside;
  (b) the host loop a caller had to write before: download the pairs once, then per frame join with the map in numpy,
      mvs_pnp_solve, pack the two-frame problem, mvs_ba_refine, update the map -- wall clock, the round trips are the point.

Both routes must track the same frames with the same point counts and end at the same pose (1e-6), or the tool fails.  Also
runs the tracker over the reference's five tsukuba frames (tests/golden/tsukuba_gray.npz) and records how far it gets and the
last pose; the reference's expectation there (test/test-visual-odometer.cpp) rests on OpenCV's ORB, so it is reported only.
Writes profiles/vo_track_latency.json.  Usage: python tools/vo_track_latency.py [--frames 1000] [--kp 2000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvslam_amd import capi, synth  # noqa: E402


def kept(gp, k):
    """(j, a, b) arrays of the kept points of pair k: the first point of every trainIdx"""
    r = gp["results"][k]
    if not r["valid"]:
        z = np.zeros(0, np.int64)
        return z, z, z
    n = int(r["n_points"])
    mt = gp["matches"][k][gp["point_idx"][k][:n]]
    a, first = np.unique(mt["trainIdx"], return_index=True)
    j = np.sort(first)
    return j, mt["trainIdx"][j].astype(np.int64), mt["queryIdx"][j].astype(np.int64)


def host_loop(ctx, gp, kp, K, vo, pnp, rp, last):
    """route (b) for frames 2 .. last; returns per-frame records and the wall time"""
    N = kp.shape[1]
    t0 = time.perf_counter()
    j, a, b = kept(gp, 0)
    mid, mX = -np.ones(N, np.int64), np.zeros((N, 3))
    mid[b], mX[b] = np.arange(len(j)), gp["points"][0][j]
    next_id, R_l, t_l = len(j), gp["results"][0]["R"].copy(), gp["results"][0]["t"].copy()
    var = [[vo.anchor_var[0]] * 3 + [vo.anchor_var[1]] * 3, [vo.regulator_var[0]] * 3 + [vo.regulator_var[1]] * 3]
    pv, c = vo.point_sigma * vo.point_sigma, vo.sigma_px * vo.sigma_px
    out = []
    for f in range(2, last + 1):
        j, a, b = kept(gp, f - 1)
        has = mid[a] >= 0
        ca, cb = a[has], b[has]
        rec = dict(frame=f, n_cand=int(len(ca)), state="LOST_PNP")
        out.append(rec)
        if len(ca) < 7:
            break
        p = capi.default_pnp_params(num_hypotheses=pnp.num_hypotheses, seed=pnp.seed + f, reproj_error=pnp.reproj_error,
                                    refit=pnp.refit)
        one = ctx.pnp_solve(mX[ca], kp[f][cb].astype(np.float64), K, p)
        if not one["ok"]:
            break
        inl = one["inliers"]
        rec.update(n_pnp_inliers=int(len(inl)), state="LOST_FEW")
        if len(inl) < vo.min_pnp_point_count:
            break
        e = one["t"] - t_l
        scale = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        nj, na, nb = j[~has], a[~has], b[~has]
        Xn = (scale * gp["points"][f - 1][nj]) @ R_l.T + t_l
        pa, pb = np.concatenate([ca[inl], na]), np.concatenate([cb[inl], nb])
        pid = np.concatenate([mid[ca[inl]], next_id + np.arange(len(nj))])
        new = np.concatenate([np.zeros(len(inl), np.uint8), np.ones(len(nj), np.uint8)])
        m = len(pa)
        prior = np.where(new[:, None] == 1, 0.0, np.tile((np.eye(3) * pv).reshape(9), (m, 1)))
        cov = np.tile([c, 0.0, 0.0, c], (m, 1))
        ref = ctx.ba_refine(K, np.stack([np.concatenate([R_l.reshape(9), t_l]), np.concatenate([one["R"].reshape(9), one["t"]])]),
                            var, np.concatenate([mX[ca[inl]], Xn]), prior,
                            [kp[f - 1][pa].astype(np.float64), kp[f][pb].astype(np.float64)], [cov, cov], [new, None], rp)
        rec.update(n_tracked=int(len(inl)), n_new=int(len(nj)), error=ref["error"], state="LOST_BA")
        if not ref["ok"]:
            break
        rec["state"] = "LOST_ERROR"
        if ref["error"] > vo.max_error:
            break
        rec["state"] = "TRACKED"
        next_id += len(nj)
        R_l, t_l = ref["R"][1], ref["t"][1]
        mid, mX = -np.ones(N, np.int64), np.zeros((N, 3))
        mid[pb], mX[pb] = pid, ref["points"]
    return out, (time.perf_counter() - t0) * 1e3, R_l, t_l


STATES = ["NOT_REACHED", "INIT", "TRACKED", "LOST_PNP", "LOST_FEW", "LOST_BA", "LOST_ERROR"]


def tsukuba(ctx):
    g = np.load(os.path.join(ROOT, "tests", "golden", "tsukuba_gray.npz"))
    imgs, K = g["images"], g["K"]
    s = capi.Sequence(ctx, len(imgs), 512, 32)
    s.upload_images(0, imgs, K, capi.default_orb_params())
    s.run(capi.default_params(num_hypotheses=2000, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-3, max_dist=50.0),
          capi.default_pnp_params(num_hypotheses=100, seed=7, reproj_error=0.05))
    out = {}
    for name, err, max_error in (("reference_gates", 0.05, 0.5), ("pnp_1px_no_error_gate", 1.0, 1e30)):
        s.track(capi.default_vo_params(max_error=max_error), capi.default_pnp_params(num_hypotheses=100, seed=7, reproj_error=err),
                capi.default_refine_params())
        fr = s.download_track_frames()
        last = max(f for f in range(len(fr)) if fr[f]["state"] in (1, 2))
        out[name] = dict(states=[STATES[int(x)] for x in fr["state"]], n_cand=fr["n_cand"].tolist(),
                         n_pnp_inliers=fr["n_pnp_inliers"].tolist(), error=fr["error"].tolist(), scale=fr["scale"].tolist(),
                         last_frame_with_a_pose=int(last), last_R=fr[last]["R"].tolist(), last_t=fr[last]["t"].tolist())
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--hyp", type=int, default=4096, help="two-view hypotheses per pair (the pairs are not timed)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=200, help="frames the host loop walks (its time is per frame)")
    ap.add_argument("--seed", type=int, default=0x5E9, help="of the generator")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vo_track_latency.json"))
    args = ap.parse_args()
    import torch

    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream.cuda_stream)
    NF, N = args.frames, args.kp
    seq = synth.make_sequence(NF, n_kp=N, seed=args.seed)
    s = capi.Sequence(ctx, NF, N, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
    pnp = capi.default_pnp_params(num_hypotheses=100, seed=2, reproj_error=1.5)   # 100 = the reference's iterationsCount
    s.run(capi.default_params(num_hypotheses=args.hyp, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=2e-3), pnp)
    # the error gate is off: at this generator's 0.5 px noise the BA's error is tens per step, far above the reference's 0.5
    vo, rp = capi.default_vo_params(max_error=1e30), capi.default_refine_params()
    s.track(vo, pnp, rp)                                       # warm-up: workspace growth, code object load
    ctx._check(capi.lib().mvs_seq_sync(s._h), "mvs_seq_sync")
    ms_a = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        s.track(vo, pnp, rp)
        e1.record(stream)
        e1.synchronize()
        ms_a.append(e0.elapsed_time(e1))
    fr = s.download_track_frames()
    reached = int(np.sum(fr["state"] != 0))
    tracked = int(np.sum(fr["state"] == 2))
    last = max(f for f in range(NF) if fr[f]["state"] in (1, 2))
    # (b) over the first frames the device reached, the lost one included
    upto = min(last + 1, NF - 1, args.host_frames + 1)
    t0 = time.perf_counter()
    gp = s.download_pairs()
    ms_download = (time.perf_counter() - t0) * 1e3
    host, ms_b, R_h, t_h = host_loop(ctx, gp, seq["kp"], seq["K"], vo, pnp, rp, upto)
    same = all(h["state"] == STATES[int(fr[h["frame"]]["state"])] and h["n_cand"] == fr[h["frame"]]["n_cand"] and
               h.get("n_new", 0) == fr[h["frame"]]["n_new"] for h in host)
    done = [h["frame"] for h in host if h["state"] == "TRACKED"]
    at = done[-1] if done else 1
    pose_diff = float(max(np.abs(R_h - fr[at]["R"]).max(), np.abs(t_h - fr[at]["t"]).max()))
    steps_run, steps_live = NF - 2, max(0, min(last + 1, NF - 1) - 1)   # live: steps that did work (the lost one included)
    launches = 8 + (3 if pnp.refit else 0)
    live = slice(2, last + 1)
    mean = lambda a: float(np.mean(a[live])) if last >= 2 else 0.0
    # a run that ends early leaves dead steps (kernels that read the state word and leave) in the device figure: per-step times
    # and the speed-up are quoted only when every step was live
    whole = steps_live == steps_run
    res = dict(frames=NF, keypoints=N, pnp_hypotheses=pnp.num_hypotheses, frames_reached=reached, frames_tracked=tracked,
               last_state=STATES[int(fr[min(last + 1, NF - 1)]["state"])], steps_launched=steps_run, steps_live=steps_live,
               points_per_step=dict(tracked=mean(fr["n_tracked"]), new=mean(fr["n_new"])), ba_iterations_mean=mean(fr["iterations"]),
               launches_per_step=launches, launches_per_call=1 + launches * steps_run, memsets_per_call=2,
               cleared_bytes_per_call=int(NF) * (141 * int(N) + 1500),
               device_route_ms=dict(hip_events=ms_a, best=min(ms_a), per_step=min(ms_a) / steps_run if whole else None),
               host_route_ms=dict(frames=len(host), download_pairs=ms_download, loop=ms_b, per_step=ms_b / max(1, len(host))),
               routes_track_the_same=bool(same), host_device_pose_difference=pose_diff,
               speedup_per_step=(ms_b / max(1, len(host))) / (min(ms_a) / steps_run) if whole else None, tsukuba=tsukuba(ctx))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    s.close()
    ctx.close()
    if not same or pose_diff > 1e-6:
        sys.exit("the two routes differ: same frames %s, pose difference %s" % (same, pose_diff))


if __name__ == "__main__":
    main()
