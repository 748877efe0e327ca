"""Latency of mvs_ba_refine_sparse on a long synthetic sequence.  Not a test, not part of bench.py.

The problem: mvslam_amd/synth.py's trajectory (make_sequence's path and yaw), camera and corridor map; every frame keeps up to
--tracks visible map points (synth's stable pseudo-random subset), and the frames a map point is kept in are cut into chains of
at most --max-track consecutive frames, each chain one point of the bundle adjustment -- so the reduced camera system is a band
of that width.  Frame 0 is anchored, frame 1 carries the scale-fixing prior, no point has a prior; the guesses are the truth
perturbed.  The call is timed with the wall clock around it (it ends with its own synchronisation): one warm-up call, then
--runs calls; the record gives every run, the median, the LM iterations and the time per iteration (total / (iterations + 1):
the covariance-free call builds and factorises once more at the estimate).

    python tools/ba_sparse_latency.py [--frames 1000] [--tracks 2000] [--runs 5] [--cov] [--out profiles/ba_sparse_latency.json]

The share of the single-workgroup factorisation comes from a kernel trace of one run of this tool (rocprofv3 --kernel-trace
--stats -- python tools/ba_sparse_latency.py --runs 1); --stats-csv reads that table into the record.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvslam_amd import capi, synth  # noqa: E402


def chain_problem(n_frames, tracks, max_track, n_map, seed=0x5E9, noise_px=0.5, width=640, height=480, step=0.05, yaw_step=0.005):
    K = synth.K_DEFAULT
    rng = np.random.default_rng(seed)
    L = step * n_frames
    Xw = np.stack([rng.uniform(-6, 6 + 0.5 * L, n_map), rng.uniform(-3, 3, n_map), rng.uniform(2, 12 + L, n_map)], axis=1)
    poses, fr_l, id_l, uv_l = [], [], [], []
    for f in range(n_frames):
        yaw, c = yaw_step * f, synth._path_centre(step, f)
        R = np.array([[np.cos(yaw), 0, -np.sin(yaw)], [0, 1, 0], [np.sin(yaw), 0, np.cos(yaw)]])   # world -> camera
        Xc = (Xw - c) @ R.T
        z = Xc[:, 2]
        uvp = Xc @ K.T
        uv = uvp[:, :2] / np.where(z[:, None] > 0.1, uvp[:, 2:3], 1.0)
        vis = (z > 1.0) & (uv[:, 0] >= 1) & (uv[:, 0] < width - 1) & (uv[:, 1] >= 1) & (uv[:, 1] < height - 1)
        ids = np.nonzero(vis)[0]
        if len(ids) > tracks:
            ids = np.sort(ids[np.argsort((ids * 2654435761) % 1000003)[:tracks]])
        fr_l.append(np.full(len(ids), f))
        id_l.append(ids)
        uv_l.append(uv[ids] + rng.normal(scale=noise_px, size=(len(ids), 2)))
        poses.append(np.concatenate([R.T.reshape(9), c]))   # camera in world
    fr, ids, uv = np.concatenate(fr_l), np.concatenate(id_l), np.concatenate(uv_l)
    order = np.lexsort((fr, ids))
    fr, ids, uv = fr[order], ids[order], uv[order]
    brk = np.ones(len(fr), bool)
    brk[1:] = (ids[1:] != ids[:-1]) | (fr[1:] != fr[:-1] + 1)
    run = np.cumsum(brk) - 1
    pos = np.arange(len(fr)) - np.nonzero(brk)[0][run]
    chain = run * (n_frames + 1) + pos // max_track          # a key per chain, ascending
    _, first, counts = np.unique(chain, return_index=True, return_counts=True)
    keep = np.repeat(counts >= 2, counts)                    # a chain of one observation holds nothing
    fr, uv, map_id = fr[keep], uv[keep], ids[first[counts >= 2]]
    counts = counts[counts >= 2]
    obs_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    poses = np.stack(poses)
    X = Xw[map_id]
    var = np.zeros((n_frames, 6))
    var[0], var[1] = 1e-5, 1e-2
    guess = poses.copy()
    for f in range(1, n_frames):
        w = rng.normal(0, 2e-3, 3)
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        E = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)
        guess[f, :9] = (poses[f, :9].reshape(3, 3) @ E).reshape(9)
        guess[f, 9:] += rng.normal(0, 5e-3, 3)
    return dict(K=K, frame_pose=guess, frame_prior_var=var, points=X + rng.normal(0, 5e-3, X.shape), point_prior_cov=None,
                obs_off=obs_off, obs_frame=fr.astype(np.int32), obs_uv=uv,
                obs_cov=np.tile((np.eye(2) * noise_px ** 2).reshape(4), (len(fr), 1)))


def factor_share(path):
    """the percentage column of rocprofv3's kernel_stats table, per kernel of this path"""
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    pick = {}
    for r in rows:
        for n in ("pgd_factor_kernel", "pgd_solve_kernel", "pgd_assemble_kernel", "bas_schur_kernel", "bas_frame_kernel",
                  "bas_selinv_kernel"):
            if n in r["Name"]:
                pick[n] = round(100.0 * float(r["TotalDurationNs"]) / tot, 2)
    return pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--tracks", type=int, default=2000)
    ap.add_argument("--max-track", type=int, default=8)
    ap.add_argument("--map", type=int, default=0, help="map points (0: 150 per frame, at least 20000)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cov", action="store_true", help="ask for the covariances as well")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.perf_counter()
    pb = chain_problem(a.frames, a.tracks, a.max_track, a.map or max(20000, 150 * a.frames))
    t_build = time.perf_counter() - t0
    ctx = capi.Context(0)
    runs, res = [], None
    for k in range(a.runs + 1):
        t0 = time.perf_counter()
        res = ctx.ba_refine_sparse(pose_cov=a.cov, point_cov=a.cov, **pb)
        if k:
            runs.append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    n_obs = len(pb["obs_frame"])
    med = float(np.median(runs))
    rec = dict(what="mvs_ba_refine_sparse, wall clock around the call (host planning, uploads, LM loop, downloads)",
               frames=a.frames, points=len(pb["points"]), observations=n_obs, observations_per_frame=round(n_obs / a.frames, 1),
               max_track=a.max_track, covariances=bool(a.cov), status=int(res["status"]), iterations=res["iterations"],
               rejected_steps=res["rejected_steps"], failed_solves=res["failed_solves"], envelope_blocks=res["envelope_blocks"],
               widest_row=res["widest_row"], error_initial=res["error_initial"], error=res["error"], runs_ms=[round(x, 3) for x in runs],
               median_ms=round(med, 3), min_ms=round(min(runs), 3), ms_per_iteration=round(med / (res["iterations"] + 1), 3),
               problem_build_s=round(t_build, 2), warmup_calls=1,
               yardstick="mvs_seq_refine_windows: 22.5 ms for 249 windows of the 1000-frame run (DESIGN 4.7.1); context, not a pass mark")
    if a.stats_csv:
        rec["kernel_share_percent"] = factor_share(a.stats_csv)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
