#!/usr/bin/env python3
"""Times and errors of the pose-graph marginals on one GPU -> profiles/pose_graph_marginals.json.

Two sequences: `--frames` frames with lags <= 3, and synth.make_loop_sequence with its loop edges (the case of
tools/profile_loop_scores.py).  The marginals calls have no timing hook in the ABI, so the phases are separated from
outside, with HIP events on the context's stream around whole calls:
  assemble_factor_ms  the call with the one query (N - 1, N - 1): assembly, factorisation, and a solve of a single row;
  all_diagonal_ms     the call with every diagonal block;
  solves_ms           their difference.
Each is the median of `--repeat` calls after one that warms up.  The envelope size is recorded with them.  `fixtures` holds, per
fixture of tests/pg_marginals_model.py at the optimised poses, the largest block error of the device, of numpy.linalg.inv and
of the model's skyline restatement against the extended-precision inverse.  Nothing here is asserted: a call that ends in
MVS_NO_MODEL (ok 0, bad_node the row of the failed pivot) is recorded as it is, and its times are those of a factorisation that
stopped there.

usage: pose_graph_marginals_latency.py [--frames 1000] [--kp 2000] [--out profiles/pose_graph_marginals.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mvslam_amd import capi, synth  # noqa: E402


def _timed(stream, fn, repeat):
    times, last = [], None
    for _ in range(repeat + 1):     # the first pass warms up (and grows the workspace)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        last = fn()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times[1:])), [float(t) for t in times[1:]], last


def _marginals(s, stream, repeat):
    N = s.n_frames
    one_ms, one_runs, (st, info, _) = _timed(stream, lambda: s.pose_graph_marginals(queries=[(N - 1, N - 1)]), repeat)
    all_ms, all_runs, (st2, info2, cov) = _timed(stream, lambda: s.pose_graph_marginals(), repeat)
    g = s.download_pose_graph()
    import pg_marginals_model as mm
    first, _, blocks = mm.graph_envelope(g)
    widths = np.arange(N) - first + 1
    ev = np.array([np.linalg.eigvalsh(c.reshape(6, 6)) for c in g["edge_cov"]])
    return dict(status=[int(st), int(st2)], ok=int(info2["ok"]), bad_node=int(info2["bad_node"]), nodes=N,
                edge_cov_eigenvalues=[float(ev.min()), float(ev.max())], edges=int(g["n_edges"]),
                loop_edges=int((g["edge_kind"] == 2).sum()), envelope_blocks=int(info2["envelope_blocks"]),
                envelope_blocks_model=int(blocks), sum_width_squared=int((widths.astype(np.int64) ** 2).sum()),
                widest_row=int(widths.max()), min_pivot=float(info2["min_pivot"]), assemble_factor_ms=one_ms,
                assemble_factor_ms_runs=one_runs, all_diagonal_ms=all_ms, all_diagonal_ms_runs=all_runs,
                solves_ms=all_ms - one_ms, queries=N,
                largest_sigma_trace=float(np.einsum("nii->n", cov).max()) if info2["ok"] else None)


def _fixture_errors(ctx):
    import pg_marginals_model as mm

    out = {}
    for name, make in mm.FIXTURES.items():
        g = make()
        st, res, X = ctx.pose_graph_optimize(g)
        N = X.shape[0]
        queries = mm.all_pairs(N)
        first, _, blocks = mm.graph_envelope(g)
        e_inv, e_sky, S_ref = mm.host_errors(mm.dense_h(g, X), first, queries)
        _, info, cov = ctx.pose_graph_marginals(g, poses=X, queries=queries)
        out[name] = dict(nodes=N, envelope_blocks=int(info["envelope_blocks"]), device=float(mm.block_errors(cov, S_ref, queries).max()),
                         inv=e_inv, skyline_model=e_sky, bound=mm.bound(e_inv, e_sky))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--min-gap", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_marginals.json"))
    a = ap.parse_args()
    F, N = a.frames, a.kp
    ctx = capi.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    prm = capi.default_params(num_hypotheses=256, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-2, ratio=0.7, max_dist=10.0)
    pgp = capi.default_pose_graph_params(cg_chunk_iterations=64)
    out = dict(device=torch.cuda.get_device_name(0), frames=F, keypoints=N)
    # 1: lags <= 3
    data = synth.make_sequence(F, n_kp=N)
    s = capi.Sequence(ctx, F, N, 32)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    s.run(prm, capi.default_pnp_params())
    s.run_lags(prm, 3)
    s.build_pose_graph(3, chain_sigma=(0.05, 0.5))
    status, res = s.optimize_pose_graph(pgp)
    out["lags3"] = dict(optimize_status=int(status), **(_marginals(s, stream, a.repeat) if res["ok"] else {}))
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
    status, res = s.optimize_pose_graph(pgp)
    out["loops"] = dict(optimize_status=int(status), **(_marginals(s, stream, a.repeat) if res["ok"] else {}))
    s.close()
    print("loops", json.dumps(out["loops"]), file=sys.stderr, flush=True)
    out["fixtures"] = _fixture_errors(ctx)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
