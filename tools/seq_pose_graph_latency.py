"""Latency of the pose graph of a resident sequence, three things:

  build     mvs_seq_build_pose_graph: the two assembly kernels, HIP events on the context's stream;
  optimise  mvs_seq_optimize_pose_graph at cg_chunk_iterations 0, 16, 64 and 256 -- HIP events around the call and wall clock;
            chunk 0 is the launch sequence the library had before the chunked enqueue, in the same binary;
  host      the round trip the two calls replace: download the trajectory and the lag tables, assemble the graph in numpy
            (vectorised; the positive-definite test is numpy's Cholesky), mvs_pose_graph_optimize through host pointers.

One warm-up, then `--steps` calls each; the figure quoted is the best, all of them are recorded.  Every optimise call must
return the bytes of chunk 0, and the host route's graph must have the device graph's edges, or the tool fails.  Also
recorded, asserting nothing: the distance of the trajectory and of the optimised nodes to the generator's ground truth after
a similarity alignment of the camera centres.
Writes profiles/seq_pose_graph_latency.json.  Usage: python tools/seq_pose_graph_latency.py [--frames 1000] [--kp 2000]
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

CHUNKS = (0, 16, 64, 256)


def host_assemble(traj, pairs, refined, max_lag):
    """the definition, vectorised per lag (values to rounding, not to the byte: numpy's own summation orders)"""
    R, t = traj["R"], traj["t"]
    F = len(R)
    src, dst, Z, cov = [], [], [], []
    for d in range(1, max_lag + 1):
        res, ref = pairs[d]["results"][:F - d], refined[d]["refined"][:F - d]
        k = np.arange(F - d)
        q = np.einsum("kji,kj->ki", R[k], t[k + d] - t[k])
        with np.errstate(all="ignore"):
            s = np.linalg.norm(q, axis=1) / np.linalg.norm(ref["t"], axis=1)
        f = np.concatenate([np.ones((F - d, 3)), np.repeat(s[:, None], 3, axis=1)], axis=1)
        C = f[:, :, None] * ref["pose_cov"] * f[:, None, :]
        keep = (res["valid"] != 0) & (ref["ok"] != 0) & np.isfinite(s) & (s > 0)
        for i in np.nonzero(keep)[0]:
            try:
                np.linalg.cholesky(np.tril(C[i]) + np.tril(C[i], -1).T)
            except np.linalg.LinAlgError:
                keep[i] = False
        k = k[keep]
        src.append(k), dst.append(k + d)
        Z.append(np.concatenate([ref["R"][keep].reshape(-1, 9), s[keep, None] * ref["t"][keep]], axis=1))
        cov.append(C[keep].reshape(-1, 36))
    return dict(node_pose=np.concatenate([R.reshape(F, 9), t], axis=1), edge_src=np.concatenate(src).astype(np.int32),
                edge_dst=np.concatenate(dst).astype(np.int32), edge_pose=np.concatenate(Z), edge_cov=np.concatenate(cov), anchor=0)


def centres(poses12):
    """camera centres of poses (R, t) = frame in frame 0: the translations"""
    return np.asarray(poses12).reshape(-1, 12)[:, 9:]


def aligned_distance(est, truth):
    """RMS and largest distance between two point tracks after the best similarity (Umeyama) of `est` onto `truth`"""
    a, b = est - est.mean(0), truth - truth.mean(0)
    U, D, Vt = np.linalg.svd(b.T @ a / len(a))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    Rm = U @ S @ Vt
    c = np.trace(np.diag(D) @ S) / (a * a).sum() * len(a)
    r = np.linalg.norm(c * a @ Rm.T - b, axis=1)
    return dict(rms=float(np.sqrt(np.mean(r * r))), max=float(r.max()), scale=float(c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--max-lag", type=int, default=3)
    ap.add_argument("--hyp", type=int, default=4096, help="two-view hypotheses per pair (the pairs are not timed)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x5E9, help="of the generator")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_pose_graph_latency.json"))
    args = ap.parse_args()
    import torch

    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream.cuda_stream)
    NF, N, L = args.frames, args.kp, args.max_lag
    seq = synth.make_sequence(NF, n_kp=N, seed=args.seed)
    s = capi.Sequence(ctx, NF, N, 32)
    s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
    prm = capi.default_params(num_hypotheses=args.hyp, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=2e-3)
    s.run(prm, capi.default_pnp_params(num_hypotheses=100, seed=2, reproj_error=1.5))
    s.run_lags(prm, L)
    sync = lambda: ctx._check(capi.lib().mvs_seq_sync(s._h), "mvs_seq_sync")
    sync()
    sigma = (0.05, 0.5)   # the fallback keeps a sequence with a failed adjacent pair in one piece

    def timed(fn):
        """(HIP-event ms, wall ms, what fn returned) of one call on the context's stream"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    build = lambda: s.build_pose_graph(L, chain_sigma=sigma)
    timed(build)
    ms_build = [timed(build)[:2] for _ in range(args.steps)]
    g = s.download_pose_graph()
    optimise, base = {}, None
    for chunk in CHUNKS:
        p = capi.default_pose_graph_params(cg_chunk_iterations=chunk)
        call = lambda: s.optimize_pose_graph(p)
        timed(call)
        runs = [timed(call) for _ in range(args.steps)]
        status, res = runs[-1][2]
        blob = res.tobytes() + (s.download_pose_graph_poses().tobytes() if status == capi.MVS_OK else b"")
        base = blob if base is None else base
        if blob != base:
            sys.exit("cg_chunk_iterations = %d does not return the bytes of 0" % chunk)
        optimise[str(chunk)] = dict(hip_events_ms=[r[0] for r in runs], wall_ms=[r[1] for r in runs],
                                    best_wall_ms=min(r[1] for r in runs), status=int(status),
                                    result={k: (int(res[k]) if k not in ("error", "error_initial") else float(res[k]))
                                            for k in res.dtype.names})
    opt_poses = s.download_pose_graph_poses() if optimise["0"]["status"] == capi.MVS_OK else None

    def host_route():
        t = [time.perf_counter()]
        traj = s.download_trajectory()
        pairs = {d: s.download_lag_pairs(d) for d in range(1, L + 1)}
        refined = {d: s.download_lag_refined(d, points=False) for d in range(1, L + 1)}
        t.append(time.perf_counter())
        hg = host_assemble(traj, pairs, refined, L)
        t.append(time.perf_counter())
        st, res, poses = ctx.pose_graph_optimize(hg)
        t.append(time.perf_counter())
        return [(b - a) * 1e3 for a, b in zip(t, t[1:])], hg, st, res, poses

    host_route()
    host = [host_route() for _ in range(args.steps)]
    hg = host[-1][1]
    measured = g["edge_kind"] == 0
    same_edges = (hg["edge_src"].tolist() == g["edge_src"][measured].tolist() and
                  hg["edge_dst"].tolist() == g["edge_dst"][measured].tolist())
    truth = np.array([-R.T @ t for R, t in seq["poses"]])   # camera centres in the world
    traj = s.download_trajectory()
    res = dict(frames=NF, keypoints=N, max_lag=L, two_view_hypotheses=args.hyp, steps=args.steps,
               candidate_slots=L * NF - L * (L + 1) // 2, edges=int(g["n_edges"]),
               edges_per_lag=np.bincount(g["edge_lag"], minlength=L + 1)[1:].tolist(),
               chain_fallback_edges=int((g["edge_kind"] == 1).sum()), chain_sigma=list(sigma),
               build_ms=dict(hip_events=[b[0] for b in ms_build], wall=[b[1] for b in ms_build], best=min(b[0] for b in ms_build)),
               optimise=optimise,
               host_route_ms=dict(download=[h[0][0] for h in host], numpy_assembly=[h[0][1] for h in host],
                                  pose_graph_optimize=[h[0][2] for h in host], best_total=min(sum(h[0]) for h in host),
                                  status=int(host[-1][2]), same_measured_edges=bool(same_edges)),
               ground_truth=dict(trajectory=aligned_distance(traj["t"], truth),
                                 optimised=aligned_distance(centres(opt_poses), truth) if opt_poses is not None else None))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    s.close()
    ctx.close()
    if not same_edges:
        sys.exit("the host route's graph has other edges than the device's")


if __name__ == "__main__":
    main()
