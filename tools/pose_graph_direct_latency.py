#!/usr/bin/env python3
"""The direct LM step against the PCG on the two 1000-frame sequence graphs -> profiles/pose_graph_direct.json (DESIGN.md
section 4.10.4).

The two cases of tools/seq_pose_graph_latency.py and tools/pose_graph_marginals_latency.py: `--frames` frames with lags <= 3,
and synth.make_loop_sequence with its loop edges; and, because the scaled factorisation fails on both, posegraph_model.ring of
the same size, whose scale does not drift.  Each resident graph is optimised under MVS_PG_SOLVER_PCG with
cg_chunk_iterations = 64 (the header's recommended setting) and under MVS_PG_SOLVER_DIRECT, alternating in one process: one
call of each that warms up, then `--repeat` calls of each, timed with HIP events on the context's stream and with the wall
clock around the whole call.  Recorded per case: ok, LM iterations and rejected steps of both solvers, the envelope and its
widest row, the times, the pose gap between the two answers, and what mvs_ctx_pose_graph_direct_info says of the last direct
call (failed solves, the node of the first failed pivot, the smallest pivot).  Nothing is asserted.

usage: pose_graph_direct_latency.py [--frames 1000] [--kp 2000] [--out profiles/pose_graph_direct.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mvslam_amd import capi, synth  # noqa: E402


class _HostGraph:
    """a host-pointer graph behind the two calls _case makes of a resident sequence"""

    def __init__(self, ctx, g):
        self.ctx, self.g, self.n_frames, self.poses = ctx, g, g["node_pose"].shape[0], None

    def optimize_pose_graph(self, pgp):
        status, res, self.poses = self.ctx.pose_graph_optimize(self.g, params=pgp)
        return status, res

    def download_pose_graph_poses(self):
        return self.poses

    def download_pose_graph(self):
        return dict(self.g, n_edges=len(self.g["edge_src"]), edge_kind=np.zeros(len(self.g["edge_src"]), dtype=np.int32))


def _one(ctx, s, stream, solver, pgp):
    ctx.set_pose_graph_solver(solver)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    status, res = s.optimize_pose_graph(pgp)
    e1.record(stream)
    e1.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    poses = s.download_pose_graph_poses() if res["ok"] else None
    return dict(status=int(status), res=res, poses=poses, event_ms=float(e0.elapsed_time(e1)), wall_ms=float(wall))


def _case(ctx, s, stream, repeat):
    import pg_marginals_model as mm
    import posegraph_model as pm

    pgp = capi.default_pose_graph_params(cg_chunk_iterations=64)
    solvers = (("pcg64", capi.MVS_PG_SOLVER_PCG), ("direct", capi.MVS_PG_SOLVER_DIRECT))
    runs = {name: [] for name, _ in solvers}
    last = {}
    for k in range(repeat + 1):                       # the first pass of each warms up (and grows the workspace)
        for name, solver in solvers:
            r = _one(ctx, s, stream, solver, pgp)
            if k:
                runs[name].append(r)
            last[name] = r
    ctx.set_pose_graph_solver(capi.MVS_PG_SOLVER_PCG)
    info = ctx.pose_graph_direct_info()
    g = s.download_pose_graph()
    first, _, blocks = mm.graph_envelope(g)
    widths = np.arange(s.n_frames) - first + 1
    out = dict(nodes=int(s.n_frames), edges=int(g["n_edges"]), loop_edges=int((g["edge_kind"] == 2).sum()),
               envelope_blocks=int(info["envelope_blocks"]), envelope_blocks_model=int(blocks), widest_row=int(info["widest_row"]),
               widest_row_model=int(widths.max()), failed_solves=int(info["failed_solves"]), bad_node=int(info["bad_node"]),
               min_pivot=float(info["min_pivot"]), failed_pivot=float(info["failed_pivot"]))
    for name, _ in solvers:
        res = last[name]["res"]
        ev, wall = [r["event_ms"] for r in runs[name]], [r["wall_ms"] for r in runs[name]]
        out[name] = dict(status=last[name]["status"], ok=int(res["ok"]), iterations=int(res["iterations"]),
                         rejected_steps=int(res["rejected_steps"]), cg_iterations=int(res["cg_iterations"]),
                         error_initial=float(res["error_initial"]), error=float(res["error"]), event_ms=ev, wall_ms=wall,
                         event_ms_median=float(np.median(ev)), wall_ms_median=float(np.median(wall)),
                         event_ms_spread=float(max(ev) - min(ev)),
                         same_bytes_every_call=bool(all(r["res"].tobytes() == res.tobytes() for r in runs[name])))
    if last["pcg64"]["poses"] is not None and last["direct"]["poses"] is not None:
        rot, trans = pm.pose_distance(last["pcg64"]["poses"], last["direct"]["poses"])
        out["pose_gap"] = dict(rotation=rot, translation=trans)
    else:
        out["pose_gap"] = None
    out["ok"] = bool(out["pcg64"]["ok"] and out["direct"]["ok"])
    # the comparison means something only where the direct solver solved: a run whose every factorisation failed is short
    out["direct_solved_steps"] = out["direct"]["iterations"] - out["failed_solves"]
    out["direct_below_pcg64_by_more_than_its_spread"] = bool(
        out["pcg64"]["event_ms_median"] - out["direct"]["event_ms_median"] > out["pcg64"]["event_ms_spread"]) \
        if out["direct_solved_steps"] > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--min-gap", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_direct.json"))
    a = ap.parse_args()
    F, N = a.frames, a.kp
    ctx = capi.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    prm = capi.default_params(num_hypotheses=256, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-2, ratio=0.7, max_dist=10.0)
    out = dict(device=torch.cuda.get_device_name(0), frames=F, keypoints=N, repeat=a.repeat,
               pcg="MVS_PG_SOLVER_PCG, cg_chunk_iterations 64", direct="MVS_PG_SOLVER_DIRECT")
    # 1: lags <= 3
    data = synth.make_sequence(F, n_kp=N)
    s = capi.Sequence(ctx, F, N, 32)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    s.run(prm, capi.default_pnp_params())
    s.run_lags(prm, 3)
    s.build_pose_graph(3, chain_sigma=(0.05, 0.5))
    out["lags3"] = _case(ctx, s, stream, a.repeat)
    s.close()
    print("lags3", json.dumps(out["lags3"]), file=sys.stderr, flush=True)
    # 2: the loop sequence with its loop edges
    data = synth.make_loop_sequence(F, n_kp=N)
    s = capi.Sequence(ctx, F, N, 32)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    s.run(prm, capi.default_pnp_params())
    s.run_lags(prm, 2)
    s.build_pose_graph(2, chain_sigma=(0.05, 0.5))
    s.loop_scores(0.7, 10.0, a.min_gap)
    s.select_loops(60, 1, 256)
    s.verify_loops(prm)
    s.add_loop_edges(loop_sigma=(0.02, 0.2))
    out["loops"] = _case(ctx, s, stream, a.repeat)
    s.close()
    print("loops", json.dumps(out["loops"]), file=sys.stderr, flush=True)
    # 3: a graph of the same size that does factorise: a ring with chords through the host-pointer call (uploads included on
    # both sides).  The closing edges make the last rows reach back to node 0.
    import posegraph_model as pm

    out["ring"] = _case(ctx, _HostGraph(ctx, pm.ring(F, chords=(2, 3))), stream, a.repeat)
    print("ring", json.dumps(out["ring"]), file=sys.stderr, flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
