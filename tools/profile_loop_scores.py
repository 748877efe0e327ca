#!/usr/bin/env python3
"""Times of the loop-closure path on one GPU -> profiles/loop_scores.json.

  scores      loop_scores_mfma_kernel over all frame pairs at least min_gap apart, HIP events on the context's stream;
  matcher     match_mfma_kernel on a batch holding the pairs (k, k + min_gap) of the same frames: what a lag batch of the
              sequence runs, per-launch events of mvs_batch_time_kernels;
  end_to_end  scores, selection, verification, edges and optimisation on the sequence, wall clock.

usage: profile_loop_scores.py [--frames 1000] [--kp 2000] [--min-gap 30] [--out profiles/loop_scores.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvslam_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--min-gap", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_scores.json"))
    a = ap.parse_args()
    F, N, gap = a.frames, a.kp, a.min_gap
    data = synth.make_loop_sequence(F, n_kp=N)
    ctx = capi.Context(0)
    ratio, max_dist = 0.7, 10.0
    prm = capi.default_params(num_hypotheses=256, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-2, ratio=ratio,
                              max_dist=max_dist)
    s = capi.Sequence(ctx, F, N, 32)
    s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
    stream = torch.cuda.ExternalStream(ctx.stream)
    n_pairs = (F - gap) * (F - gap + 1) // 2
    times = []
    for _ in range(a.repeat + 1):     # the first pass warms up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        s.loop_scores(ratio, max_dist, gap)
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times = times[1:]
    scores_ms = float(np.median(times))
    # the matcher on the pairs of lag `gap`
    P = F - gap
    b = capi.Batch(ctx, P, N, 32)
    b.upload(0, data["desc"][:P], data["kp"][:P], data["n_kp"][:P], data["desc"][gap:], data["kp"][gap:], data["n_kp"][gap:],
             np.tile(data["K"].reshape(1, 9), (P, 1)), np.arange(P, dtype=np.int64))
    b.time_kernels(prm, 2)
    tk = b.time_kernels(prm, a.repeat)
    match_ms = float(sum(ms for name, ms in tk if name.startswith("match_") and "compact" not in name))
    match_kernel = [name for name, _ in tk if name.startswith("match_") and "compact" not in name]
    assert match_kernel == ["match_mfma_kernel<true>"], match_kernel
    b.run(prm)
    b.sync()
    lag_matches = b.download(matches=False, mask=False, points=False)["results"]["n_matches"]
    table = s.download_loop_scores()
    assert np.array_equal(np.diagonal(table, offset=gap), lag_matches), "scores differ from the pair pipeline's n_matches"
    b.close()
    # end to end
    s.run(prm, capi.default_pnp_params())
    s.run_lags(prm, 2)
    s.build_pose_graph(2, chain_sigma=(0.05, 0.5))
    s.sync()
    t0 = time.perf_counter()
    s.loop_scores(ratio, max_dist, gap)
    s.select_loops(60, 1, 256)
    s.verify_loops(prm)
    s.add_loop_edges(loop_sigma=(0.02, 0.2))
    status, res = s.optimize_pose_graph(capi.default_pose_graph_params(cg_chunk_iterations=64))
    t_loop = time.perf_counter() - t0
    cd = s.download_loop_candidates()
    out = dict(
        device=torch.cuda.get_device_name(0), frames=F, keypoints=N, min_gap=gap, ratio=ratio, max_dist=max_dist,
        frame_pairs=n_pairs, loop_scores_ms=scores_ms, loop_scores_ms_runs=[float(t) for t in times],
        loop_scores_us_per_pair=1e3 * scores_ms / n_pairs,
        matcher=dict(kernel=match_kernel[0], pairs=P, ms=match_ms, us_per_pair=1e3 * match_ms / P),
        ratio_loop_over_matcher=(scores_ms / n_pairs) / (match_ms / P),
        end_to_end=dict(scores_select_verify_edges_optimize_s=t_loop,
                        candidates_kept=int(cd["n_kept"]), candidates_found=int(cd["n_found"]),
                        loop_edges=int(cd["cand"]["accepted"].sum()), optimize_status=int(status),
                        optimize=dict(ok=int(res["ok"]), iterations=int(res["iterations"]), cg_iterations=int(res["cg_iterations"]),
                                      error_initial=float(res["error_initial"]), error=float(res["error"]))))
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    s.close()
    ctx.close()


if __name__ == "__main__":
    main()
