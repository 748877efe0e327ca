"""Latency of the pose-graph back end (mvs_pose_graph_optimize), wall clock around the call
(uploads, the host's LM decisions and the download are part of what a caller waits for):

  (a) one graph of 1000 nodes on a noisy circle, edges (i, i + 1), (i, i + 2), (i, i + 3) and twenty loop closures: the
      large path -- ms per call, LM iterations, CG iterations;
  (b) a batch of 512 graphs of 8 nodes: the dense path, one launch -- ms per batch.

Reported, never asserted.  Writes profiles/pose_graph_latency.json.  Usage: python tools/pose_graph_latency.py [--repeat 5]
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


def rot(w):
    """Exp of an axis-angle vector (Rodrigues)"""
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / th ** 2) * (K @ K)


def circle(n, chords, closures, seed=1, noise=0.01, guess_noise=0.05):
    """n poses on a noisy circle of radius 3: edges (i, i + 1) and (i, i + c) for every chord length c plus `closures`
    edges across the circle; every edge measures X_src^-1 X_dst with `noise`, covariance noise^2 I; the initial values are
    the true poses moved by `guess_noise` (node 0, the anchor, exactly)"""
    rng = np.random.default_rng(seed)
    R, t = [], []
    for i in range(n):
        a = 2.0 * np.pi * i / n
        R.append(rot([0, 0, a + np.pi / 2]) @ rot([0.2 * np.sin(3 * a), 0.1 * np.cos(2 * a), 0.0]))
        t.append(np.array([3.0 * np.cos(a), 3.0 * np.sin(a), 0.3 * np.sin(2 * a)]))
    edges = [(i, (i + c) % n) for c in (1,) + tuple(chords) for i in range(n)]
    for a in rng.integers(0, n, size=closures):
        b = int((a + n // 2 + rng.integers(-n // 8, n // 8 + 1)) % n)
        if b != int(a):
            edges.append((int(a), b))
    Z = np.zeros((len(edges), 12))
    for k, (s, d) in enumerate(edges):
        Z[k, :9] = (R[s].T @ R[d] @ rot(rng.normal(size=3) * noise)).reshape(9)
        Z[k, 9:] = R[s].T @ (t[d] - t[s]) + rng.normal(size=3) * noise
    pose = np.zeros((n, 12))
    for i in range(n):
        d = rng.normal(size=6) * (guess_noise if i else 0.0)
        pose[i, :9] = (R[i] @ rot(d[:3])).reshape(9)
        pose[i, 9:] = t[i] + R[i] @ d[3:]
    e = np.asarray(edges, dtype=np.int32)
    return dict(node_pose=pose, edge_src=np.ascontiguousarray(e[:, 0]), edge_dst=np.ascontiguousarray(e[:, 1]), edge_pose=Z,
                edge_cov=np.tile((np.eye(6) * noise * noise).reshape(36), (len(edges), 1)), anchor=0)


def timed(fn, repeat):
    fn()   # warm-up: workspace growth, code object load
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    ctx = capi.Context(0)
    big = circle(1000, (2, 3), 20)
    (st, res, _), ts = timed(lambda: ctx.pose_graph_optimize(big), a.repeat)
    one = dict(nodes=1000, edges=int(len(big["edge_src"])), status=int(st), ok=int(res["ok"]), ms_per_call_median=float(np.median(ts)),
               ms_per_call_min=float(min(ts)), lm_iterations=int(res["iterations"]), cg_iterations=int(res["cg_iterations"]),
               rejected_steps=int(res["rejected_steps"]), error_initial=float(res["error_initial"]), error=float(res["error"]))
    small = [circle(8, (2,), 0, seed=100 + s) for s in range(512)]
    (st, res, _), ts = timed(lambda: ctx.pose_graph_optimize_batch(small), a.repeat)
    batch = dict(graphs=512, nodes=8, edges=int(len(small[0]["edge_src"])), status=int(st), ok=int(res["ok"].sum()),
                 ms_per_batch_median=float(np.median(ts)), ms_per_batch_min=float(min(ts)),
                 lm_iterations_mean=float(res["iterations"].mean()))
    ctx.close()
    out = dict(what="wall clock of mvs_pose_graph_optimize / _batch on one MI355X, transfers included", repeat=a.repeat,
               one_graph_1000_nodes=one, batch_512_graphs_of_8_nodes=batch)
    path = os.path.join(ROOT, "profiles", "pose_graph_latency.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
