"""Work for the kernel-time figures of DESIGN.md section 4.9: 512 pairs x 2000 keypoints of the bench's generator, matched once on
the device, then their matched image points through mvs_batch_run_points_essential (five-point RANSAC) and, as the yardstick,
through mvs_batch_run_points (8-point RANSAC) at H = 1 000 and H = 10 000, three runs each after a warm-up.  The five-point
path runs once per confidence level (mvs_ctx_set_essential_confidence): 0 -- every hypothesis -- and 0.99, the reference's
VF_MATCH_CONFIDENCE_LEVEL, by default; `--confidence 0` or `--confidence 0.99` runs one leg alone, and each leg prints the
distribution of n_run (the checkpoint each pair stopped at) over the pairs.  The C ABI has no event-timed entry for the
five-point call, so KERNEL time is read from a kernel trace of this script, one leg per trace so that the rows are that leg's:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o e5 -- python tools/essential5_latency.py --confidence 0.99

(rows essential5_solve_count_kernel and essential5_select_kernel -- with a confidence level also essential5_horizon_kernel, and
one solve + count call per round -- against the ransac_* rows of OUT/**/e5_kernel_stats.csv: calls, total and average ns; both paths share prep_points_kernel, finalize_model_kernel,
triangulate_kernel and finalize_select_kernel).  What the script itself prints is host wall time around upload + launch + sync
-- not kernel time."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvslam_amd import capi, synth  # noqa: E402

PAIRS, N_KP = 512, 2000


def main():
    argv = sys.argv[1:]
    levels = (0.0, 0.99)
    if "--confidence" in argv:
        k = argv.index("--confidence")
        levels = tuple(float(v) for v in argv[k + 1].split(","))
        del argv[k:k + 2]
    pairs = int(argv[0]) if argv else PAIRS
    ctx = capi.Context(0)
    data = synth.make_batch(0, pairs, n_kp=N_KP)
    b = capi.Batch(ctx, pairs, N_KP)
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"], data["global_index"])
    prm = capi.default_params(num_hypotheses=256, sampler=capi.SAMPLER_PHILOX, seed=synth.SEED_BASE, max_error_sq=1e-2)
    b.run(prm)     # the matcher's output is the input of both paths
    b.sync()
    out = b.download(mask=False, points=False)
    m = out["results"]["n_matches"].astype(np.int32)
    uv1, uv2 = np.zeros((pairs, N_KP, 2)), np.zeros((pairs, N_KP, 2))
    for p in range(pairs):
        mt = out["matches"][p][:m[p]]
        uv1[p, :m[p]] = data["kp1"][p][mt["trainIdx"]]
        uv2[p, :m[p]] = data["kp2"][p][mt["queryIdx"]]
    print("%d pairs, %d .. %d matches (mean %.0f)" % (pairs, m.min(), m.max(), m.mean()), flush=True)
    for H in (1000, 10000):
        prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=synth.SEED_BASE, max_error_sq=1e-2)
        legs = [("mvs_batch_run_points_essential p = %g" % p, b.run_points_essential, p) for p in levels]
        for name, run, p in legs + [("mvs_batch_run_points", b.run_points, None)]:
            if p is not None:
                ctx.set_essential_confidence(p)
            run(prm, uv1, uv2, m)   # warm-up: code objects, per-hypothesis tables
            b.sync()
            if p is not None:
                n_run, n_pairs = np.unique(b.hypotheses_run(), return_counts=True)
                print("H = %5d  %-40s n_run: %s" % (H, name, ", ".join("%d pairs at %d" % (c, t) for t, c in zip(n_run, n_pairs))),
                      flush=True)
            for k in range(3):
                t0 = time.perf_counter()
                run(prm, uv1, uv2, m)
                b.sync()
                dt = time.perf_counter() - t0
                res = b.download(matches=False, mask=False, points=False)["results"]
                print("H = %5d  %-40s run %d  %9.2f ms (host wall: upload + launch + sync), %d valid, %d inliers"
                      % (H, name, k, 1e3 * dt, int(res["valid"].sum()), int(res["n_inliers"].sum())), flush=True)
        ctx.set_essential_confidence(0.0)
    b.close()
    ctx.close()


if __name__ == "__main__":
    main()
