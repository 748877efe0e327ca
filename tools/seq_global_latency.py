"""Latency of the global bundle adjustment of a resident sequence, two routes:

  (a) mvs_seq_refine_global: links, depths, counts, the problem, the plan and the solve on the device -- the call is
      synchronous, so wall clock; a second timing with max_iterations = 0 (assembly, plan, the first cost and the one
      factorisation at lambda = 0) separates the assembly and the plan from the LM iterations;
  (b) the host route: download the pairs and the trajectory, chain the tracks and pack the CSR in (vectorised) numpy,
      mvs_ba_refine_sparse, which plans on the host and uploads -- wall clock, the round trip is the point.

Both routes must build identical CSR lists (obs_off, obs_frame, obs_kp, head_frame, head_kp), or the tool fails.  Writes
profiles/seq_global_latency.json.  Usage: python tools/seq_global_latency.py [--frames 1000] [--kp 2000] [--track-frames 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mvslam_amd import capi, synth  # noqa: E402
from seq_windows_latency import links  # noqa: E402


def build_global(gp, traj, N, T):
    """tests/seq_global_model.py's build_global, vectorised over the heads of a frame"""
    n_frames = len(gp["results"]) + 1
    succ, pred, rtp = links(gp, N)
    query = gp["matches"]["queryIdx"]
    depth = np.zeros((n_frames, N), np.int64)
    for f in range(1, n_frames):
        has = pred[f] >= 0
        depth[f, has] = depth[f - 1, pred[f, has]] + 1
    off, fr, kps, hf, hk, guess = [np.zeros(1, np.int64)], [], [], [], [], []
    total = 0
    for j in range(n_frames - 1):
        heads = np.nonzero((succ[j] >= 0) & ((depth[j] % T == 0) if T else (depth[j] == 0)))[0]
        n = len(heads)
        if n == 0:
            continue
        cur, alive, length = heads.copy(), np.ones(n, bool), np.ones(n, np.int64)
        tri_k, tri_j = -np.ones(n, np.int64), np.zeros(n, np.int64)
        cols = [heads.copy()]
        f = j
        while f < n_frames - 1 and (T == 0 or len(cols) < T):
            r = np.where(alive, succ[f, cur], -1)
            alive = alive & (r >= 0)
            if not alive.any():
                break
            r = np.where(alive, r, 0)
            p = np.where(alive, rtp[f, r], -1)
            new = alive & (tri_k < 0) & (p >= 0)
            tri_k[new], tri_j[new] = f, p[new]
            cur = np.where(alive, query[f, r], 0)
            length += alive
            cols.append(np.where(alive, cur, -1))
            f += 1
        keep = tri_k >= 0
        tk, ln, k_, j_ = np.stack(cols, 1)[keep], length[keep], tri_k[keep], tri_j[keep]
        seen = np.arange(tk.shape[1])[None, :] < ln[:, None]
        fr.append((j + np.arange(tk.shape[1]))[None, :].repeat(len(tk), 0)[seen])
        kps.append(tk[seen])
        off.append(total + np.cumsum(ln))
        total += int(ln.sum())
        hf.append(np.full(len(tk), j))
        hk.append(heads[keep])
        x = gp["points"][k_, j_] * traj["pair_scale"][k_][:, None]
        guess.append(np.einsum("nab,nb->na", traj["R"][k_], x) + traj["t"][k_])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return dict(obs_off=cat(off, np.int32), obs_frame=cat(fr, np.int32), obs_kp=cat(kps, np.int32), head_frame=cat(hf, np.int32),
                head_kp=cat(hk, np.int32), point_guess=np.concatenate(guess) if guess else np.zeros((0, 3)))


def sparse_args(prob, traj, kp, K, params, sigma_px):
    """the arguments of Context.ba_refine_sparse for an assembled problem (octave 0 everywhere)"""
    F, P, O = len(traj["R"]), len(prob["head_frame"]), len(prob["obs_frame"])
    an, ps, pt = list(params.anchor_sigma), list(params.pose_sigma), params.point_sigma
    var = np.array([[s[0] * s[0]] * 3 + [s[1] * s[1]] * 3 for s in [an] + [ps] * (F - 1)])
    c = sigma_px * sigma_px
    return dict(K=K, frame_pose=np.concatenate([traj["R"].reshape(F, 9), traj["t"]], 1), frame_prior_var=var,
                points=prob["point_guess"], point_prior_cov=np.tile((np.eye(3) * (pt * pt)).reshape(9), (P, 1)),
                obs_off=prob["obs_off"], obs_frame=prob["obs_frame"],
                obs_uv=kp[prob["obs_frame"], prob["obs_kp"]].astype(np.float64), obs_cov=np.tile([c, 0.0, 0.0, c], (O, 1)),
                params=params, pose_cov=False, point_cov=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--track-frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one untimed pass of route (a) and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_global_latency.json"))
    args = ap.parse_args()
    ctx = capi.Context(0)
    NF, N, T = args.frames, args.kp, args.track_frames
    seq = synth.make_sequence(NF, n_kp=N, n_map=10 * N, noise_px=0.3, step=0.05)
    s = capi.Sequence(ctx, NF, N, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
    s.run(capi.default_params(num_hypotheses=1024, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=2e-3),
          capi.default_pnp_params(num_hypotheses=256, seed=2, reproj_error=1.5))
    params = capi.default_refine_params()
    res = s.refine_global(T, params, 0.5)      # warm-up: workspace growth, code object load
    if args.once:
        s.close()
        ctx.close()
        return
    zero = capi.default_refine_params(max_iterations=0)
    ms_a, ms_a0 = [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        s.refine_global(T, zero, 0.5)
        t1 = time.perf_counter()
        res = s.refine_global(T, params, 0.5)
        t2 = time.perf_counter()
        ms_a0.append((t1 - t0) * 1e3)
        ms_a.append((t2 - t1) * 1e3)
    t0 = time.perf_counter()
    dev = s.download_global_problem()
    est = s.download_global(pose_cov=False, point_cov=False)
    ms_a_download = (time.perf_counter() - t0) * 1e3
    # (b): everything a caller of the parent commit has to do
    ms_b = []
    for _ in range(max(1, args.steps // 2)):
        t0 = time.perf_counter()
        gp, traj = s.download_pairs(), s.download_trajectory()
        t1 = time.perf_counter()
        prob = build_global(gp, traj, N, T)
        kw = sparse_args(prob, traj, seq["kp"], seq["K"], params, 0.5)
        t2 = time.perf_counter()
        host = ctx.ba_refine_sparse(**kw)
        t3 = time.perf_counter()
        ms_b.append(dict(download=(t1 - t0) * 1e3, chain_and_pack=(t2 - t1) * 1e3, refine_sparse=(t3 - t2) * 1e3,
                         total=(t3 - t0) * 1e3))
    same = all(np.array_equal(dev[k], prob[k]) for k in ("obs_off", "obs_frame", "obs_kp", "head_frame", "head_kp"))
    # route (b) works out its own guesses (numpy's order of operations, an ulp from the device's), so the records are compared,
    # not their bytes: the same verdict and, where it solves, the same cost (1e-9 relative) and poses (1e-8)
    agree = bool(host["ok"] == res["ok"])
    if agree and res["ok"]:
        agree = bool(abs(host["error"] - res["error"]) <= 1e-9 * res["error"] and np.abs(host["R"] - est["R"]).max() <= 1e-8 and
                     np.abs(host["t"] - est["t"]).max() <= 1e-8)
    best_b = min(ms_b, key=lambda r: r["total"])
    rec = {k: res[k] for k in ("ok", "iterations", "rejected_steps", "failed_solves", "error_initial", "error", "envelope_blocks",
                               "widest_row", "n_points", "n_obs")}
    out = dict(frames=NF, keypoints=N, max_track_frames=T, result=rec,
               device_route_ms=dict(wall=ms_a, best=min(ms_a), zero_iterations_wall=ms_a0, assembly_plan_and_one_factorisation=min(ms_a0),
                                    lm_iterations=min(ms_a) - min(ms_a0), download_problem_and_estimate_wall=ms_a_download),
               host_route_ms=dict(runs=ms_b, best=best_b), routes_build_the_same_csr=bool(same),
               routes_solve_to_the_same_result=agree, host_over_device=best_b["total"] / min(ms_a))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))
    s.close()
    ctx.close()
    if not same:   # the comparison is only worth quoting for equal work
        sys.exit("the two routes build different CSR lists")


if __name__ == "__main__":
    main()
