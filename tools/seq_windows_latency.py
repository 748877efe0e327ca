"""Latency of bundle-adjusting the sliding windows of a resident sequence, two routes:

  (a) mvs_seq_refine_windows: links, assembly and solve on the device, timed with HIP events on the context's stream;
  (b) the host route: download the pairs and the trajectory, chain the matches into tracks and pack mvs_ba_window structs in
      (vectorised) numpy, mvs_ba_refine_windows -- wall clock, the round trip is the point.

Both routes must build the same track tables and solve to the same results, or the tool fails.  Writes
profiles/seq_windows_latency.json.  Usage: python tools/seq_windows_latency.py [--frames 1000] [--kp 2000]
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


def links(gp, N):
    """succ / pred / row_to_point of every pair (smallest row wins a shared trainIdx), vectorised"""
    P = len(gp["results"])
    succ, pred, rtp = -np.ones((P, N), np.int64), -np.ones((P + 1, N), np.int64), -np.ones((P, N), np.int64)
    for k, r in enumerate(gp["results"]):
        if not r["valid"]:
            continue
        M, n = int(r["n_matches"]), int(r["n_points"])
        mt = gp["matches"][k][:M]
        rows = np.nonzero(gp["mask"][k][:M] == 1)[0]
        t, first = np.unique(mt["trainIdx"][rows], return_index=True)   # rows ascend: the first occurrence is the smallest row
        win = rows[first]
        succ[k, t] = win
        pred[k + 1, mt["queryIdx"][win]] = t
        rtp[k, gp["point_idx"][k][:n]] = np.arange(n)
    return succ, pred, rtp


def pack_windows(gp, traj, kp, F, stride, max_points, params, sigma_px, K):
    """the windows of mvs_seq_refine_windows as host problems for Context.ba_refine_windows (octave 0 everywhere)"""
    n_frames, N = kp.shape[0], kp.shape[1]
    succ, pred, rtp = links(gp, N)
    query = gp["matches"]["queryIdx"]
    an, ps, pt = list(params.anchor_sigma), list(params.pose_sigma), params.point_sigma
    var = np.array([[s[0] * s[0]] * 3 + [s[1] * s[1]] * 3 for s in [an] + [ps] * (F - 1)])
    c = (sigma_px * sigma_px)
    out, tables = [], []
    for a in range(0, n_frames - F + 1, stride):
        tks, gs = [], []
        for j in range(a, a + F - 1):
            heads = np.nonzero((succ[j] >= 0) & ((pred[j] < 0) | (j == a)))[0]
            n = len(heads)
            tk = -np.ones((n, F), np.int64)
            cur, alive = heads.copy(), np.ones(n, bool)
            tri_k, tri_j = -np.ones(n, np.int64), np.zeros(n, np.int64)
            for f in range(j, a + F):
                tk[alive, f - a] = cur[alive]
                if f == a + F - 1:
                    break
                r = np.where(alive, succ[f, cur], -1)
                alive &= r >= 0
                r = np.where(alive, r, 0)
                p = np.where(alive, rtp[f, r], -1)
                new = alive & (tri_k < 0) & (p >= 0)
                tri_k[new], tri_j[new] = f, p[new]
                cur = np.where(alive, query[f, r], 0)
            keep = tri_k >= 0
            k_, j_ = tri_k[keep], tri_j[keep]
            x = gp["points"][k_, j_] * traj["pair_scale"][k_][:, None]
            gs.append(np.einsum("nab,nb->na", traj["R"][k_], x) + traj["t"][k_])
            tks.append(tk[keep])
        tk, g = np.concatenate(tks)[:max_points], np.concatenate(gs)[:max_points]
        m = len(tk)
        tables.append(tk)
        if m == 0:
            out.append(None)
            continue
        seen = tk >= 0
        obs = [np.where(seen[:, f:f + 1], kp[a + f][np.where(seen[:, f], tk[:, f], 0)].astype(np.float64), 0.0) for f in range(F)]
        cov = np.tile([c, 0.0, 0.0, c], (m, 1))
        out.append(dict(K=K, frame_pose=np.concatenate([traj["R"][a:a + F].reshape(F, 9), traj["t"][a:a + F]], 1),
                        frame_prior_var=var, points=g, point_prior_cov=np.tile((np.eye(3) * (pt * pt)).reshape(9), (m, 1)),
                        obs=obs, obs_cov=[cov] * F, obs_valid=[seen[:, f].astype(np.uint8) for f in range(F)]))
    return out, tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--max-points", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one untimed pass of route (a) and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_windows_latency.json"))
    args = ap.parse_args()
    import torch

    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream.cuda_stream)
    NF, N, F = args.frames, args.kp, args.window
    seq = synth.make_sequence(NF, n_kp=N, n_map=10 * N, noise_px=0.3, step=0.05)
    s = capi.Sequence(ctx, NF, N, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
    s.run(capi.default_params(num_hypotheses=1024, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=2e-3),
          capi.default_pnp_params(num_hypotheses=256, seed=2, reproj_error=1.5))
    params = capi.default_refine_params()
    s.refine_windows(F, args.stride, args.max_points, params, 0.5)      # warm-up: workspace growth, code object load
    ctx._check(capi.lib().mvs_seq_sync(s._h), "mvs_seq_sync")
    if args.once:
        s.close()
        ctx.close()
        return
    ms_a = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        s.refine_windows(F, args.stride, args.max_points, params, 0.5)
        e1.record(stream)
        e1.synchronize()
        ms_a.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    dev = s.download_windows()
    ms_a_download = (time.perf_counter() - t0) * 1e3
    # (b): everything a caller of the parent commit has to do
    ms_b = []
    for _ in range(max(1, args.steps // 2)):
        t0 = time.perf_counter()
        gp, traj = s.download_pairs(), s.download_trajectory()
        t1 = time.perf_counter()
        wins, tables = pack_windows(gp, traj, seq["kp"], F, args.stride, args.max_points, params, 0.5, seq["K"])
        t2 = time.perf_counter()
        host = ctx.ba_refine_windows([w for w in wins if w is not None], params)
        t3 = time.perf_counter()
        ms_b.append(dict(download=(t1 - t0) * 1e3, pack=(t2 - t1) * 1e3, refine_windows=(t3 - t2) * 1e3, total=(t3 - t0) * 1e3))
    same = all(np.array_equal(d["track_kp"], t) for d, t in zip(dev, tables))
    # route (b) works out its own guesses (numpy's order of operations, an ulp from the device's), so the solutions are
    # compared, not their bytes: the same windows solve, to the same cost (1e-9 relative) and poses (1e-8)
    it = iter(host)
    agree, not_ok = True, []
    for d, w in zip(dev, wins):
        h = None if w is None else next(it)
        if not d["ok"]:
            not_ok.append(dict(first_frame=d["first_frame"], n_points=d["n_points"], iterations=d["iterations"],
                               host_ok=bool(h and h["ok"])))
        if h is None:
            agree &= not d["ok"]
        elif h["ok"] != d["ok"]:
            agree = False
        elif d["ok"]:
            agree &= bool(abs(h["error"] - d["error"]) <= 1e-9 * d["error"] and np.abs(h["R"] - d["R"]).max() <= 1e-8 and
                          np.abs(h["t"] - d["t"]).max() <= 1e-8)
    best_b = min(ms_b, key=lambda r: r["total"])
    res = dict(frames=NF, keypoints=N, window_frames=F, stride=args.stride, max_points=args.max_points, windows=len(dev),
               points_per_window=dict(min=min(d["n_points"] for d in dev), max=max(d["n_points"] for d in dev),
                                      mean=float(np.mean([d["n_points"] for d in dev]))),
               windows_ok=sum(d["ok"] for d in dev),
               device_route_ms=dict(hip_events=ms_a, best=min(ms_a), download_windows_wall=ms_a_download),
               host_route_ms=dict(runs=ms_b, best=best_b), routes_build_the_same_tracks=bool(same),
               routes_solve_to_the_same_result=bool(agree), windows_not_ok=not_ok, speedup=best_b["total"] / min(ms_a))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    s.close()
    ctx.close()
    if not (same and agree):   # a speed-up is only worth quoting for equal work
        sys.exit("the two routes differ: same tracks %s, same results %s" % (same, agree))


if __name__ == "__main__":
    main()
