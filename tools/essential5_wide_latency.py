"""Kernel time of the two solve + count layouts of the five-point RANSAC on the same input, in one process:
512 pairs x 2000 keypoints of the bench's generator, threshold 1e-2, H = 1000, at confidence 0 and 0.99.

  wide    e5wide_solve_count_kernel (four wavefronts count a workgroup's 64 hypotheses) inside mvs_batch_run_essential;
  plain   essential5_solve_count_kernel (+ e5_solve_count_rounds_kernel under a confidence level), one wavefront, inside
          mvs_batch_run_points_essential fed with the very matches the wide run produced.

Per confidence level: one warm-up of each, then RUNS alternations wide, plain, wide, plain, ...  Kernel time comes from a kernel
trace of this script, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o e5wide -- python tools/essential5_wide_latency.py
    python tools/essential5_wide_latency.py --parse OUT

--parse reads OUT/**/*kernel_trace.csv, takes the solve + count dispatches in time order, cuts them into the runs of the
schedule above (one launch per run without a confidence level, one per checkpoint with one) and prints, per level, each run's
summed kernel time, and whether the slowest wide run beats the fastest plain run.  No GPU is needed to parse."""
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS, N_KP, H, RUNS = 512, 2000, 1000, 3
LEVELS = (0.0, 0.99)
WIDE = "e5wide_solve_count_kernel"
PLAIN = ("essential5_solve_count_kernel", "e5_solve_count_rounds_kernel")


def checkpoints(h):
    out, t = [min(64, h)], min(64, h)
    while t < h:
        t = h if t >= h - t else 2 * t
        out.append(t)
    return out


def measure():
    from mvslam_amd import capi, synth

    ctx = capi.Context(0)
    data = synth.make_batch(0, PAIRS, n_kp=N_KP)
    b = capi.Batch(ctx, PAIRS, N_KP)
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"], data["global_index"])
    prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=synth.SEED_BASE, max_error_sq=1e-2)
    keys = ("results", "mask", "points", "point_idx")
    uv1 = uv2 = m = None
    for p in LEVELS:
        ctx.set_essential_confidence(p)
        for k in range(1 + RUNS):   # k = 0: the warm-up of both
            b.run_essential(prm)
            b.sync()
            wide = b.download()
            if m is None:
                m = wide["results"]["n_matches"].astype(np.int32)
                uv1, uv2 = np.zeros((PAIRS, N_KP, 2)), np.zeros((PAIRS, N_KP, 2))
                for q in range(PAIRS):
                    mt = wide["matches"][q][:m[q]]
                    uv1[q, :m[q]] = data["kp1"][q][mt["trainIdx"]]
                    uv2[q, :m[q]] = data["kp2"][q][mt["queryIdx"]]
                print("%d pairs, %d .. %d matches (mean %.0f)" % (PAIRS, m.min(), m.max(), m.mean()), flush=True)
            wide_run = b.hypotheses_run()
            b.run_points_essential(prm, uv1, uv2, m)
            b.sync()
            plain, plain_run = b.download(), b.hypotheses_run()
            same = all(wide[x].tobytes() == plain[x].tobytes() for x in keys) and np.array_equal(wide_run, plain_run)
            t, c = np.unique(wide_run, return_counts=True)
            print("p = %g run %d: %d valid, outputs identical: %s, n_run: %s"
                  % (p, k, int(wide["results"]["valid"].sum()), same, ", ".join("%d pairs at %d" % (n, v) for v, n in zip(t, c))),
                  flush=True)
    ctx.set_essential_confidence(0.0)
    b.close()
    ctx.close()


def parse(root):
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))
    assert files, "no *kernel_trace.csv under " + root
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            low = {k.lower(): v for k, v in r.items()}
            rows.append((int(low["start_timestamp"]), int(low["end_timestamp"]), low["kernel_name"]))
    rows.sort()
    wide = [e - s for s, e, n in rows if WIDE in n]
    plain = [e - s for s, e, n in rows if any(x in n for x in PLAIN)]
    per_run = {0.0: 1, 0.99: len(checkpoints(H))}
    want = sum(per_run[p] * (1 + RUNS) for p in LEVELS)
    assert len(wide) == want and len(plain) == want, (len(wide), len(plain), want)
    out, at = {}, 0
    for p in LEVELS:
        n = per_run[p]
        leg = {}
        for name, d in (("wide", wide), ("plain", plain)):
            runs = [sum(d[at + k * n:at + (k + 1) * n]) / 1e6 for k in range(1 + RUNS)]
            leg[name] = dict(warmup_ms=runs[0], runs_ms=runs[1:], launches_per_run=n)
        at += n * (1 + RUNS)
        leg["wide_slowest_ms"], leg["plain_fastest_ms"] = max(leg["wide"]["runs_ms"]), min(leg["plain"]["runs_ms"])
        leg["wide_kept"] = leg["wide_slowest_ms"] < leg["plain_fastest_ms"]
        leg["speedup_of_means"] = float(np.mean(leg["plain"]["runs_ms"]) / np.mean(leg["wide"]["runs_ms"]))
        out["p=%g" % p] = leg
    print(json.dumps(dict(pairs=PAIRS, keypoints=N_KP, hypotheses=H, threshold=1e-2, what="solve + count kernel ms per run",
                          legs=out), indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        measure()
