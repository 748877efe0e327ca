"""Work for the kernel-time figures of DESIGN.md section 4.7: batches of 512 windows through mvs_ba_refine_windows at F = 4 and
F = 8, m = 1000, three runs each after a warm-up, and mvs_batch_refine's 512 pairs (2000 keypoints) as the yardstick, three
runs.  The C ABI has no event-timed entry for the window call (it uploads, launches, synchronises and downloads in one call),
so KERNEL time is read from a kernel trace of this script:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o win -- python tools/time_ba_windows.py

(rows refine_window_kernel and refine_kernel<2> of OUT/**/win_kernel_stats.csv: calls, total and average ns).  What the script
itself prints is host wall time of the whole call, transfers and host packing included -- not kernel time."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvslam_amd import capi, synth  # noqa: E402


def proj(K, R, t, X):
    q = (X - t) @ R
    xn = q[:, :2] / q[:, 2:3]
    return np.stack([K[0, 0] * xn[:, 0] + K[0, 1] * xn[:, 1] + K[0, 2], K[1, 1] * xn[:, 1] + K[1, 2]], axis=1)


def window(seed, F, m, sig=0.5):
    """F cameras on a track in front of m points, each point seen by a random 2 .. F of them, priors on half the points, an
    anchor on frame 0 and a regulariser on frame 1; guesses 5e-3 off the truth"""
    rng = np.random.default_rng(seed)
    K = synth.K_DEFAULT
    X = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(4, 9, m)], 1)
    poses, obs, valid = [], [], np.zeros((F, m), np.uint8)
    for f in range(F):
        R, t = synth._rodrigues(rng.normal(0, 0.03, 3)), np.array([0.3 * f, 0.02 * f, 0.05 * f])
        obs.append(proj(K, R, t, X) + rng.normal(0, sig, (m, 2)))
        Rg = R if f == 0 else R @ synth._rodrigues(rng.normal(0, 5e-3, 3))
        poses.append(np.concatenate([Rg.reshape(9), t if f == 0 else t + rng.normal(0, 5e-3, 3)]))
    for i in range(m):
        valid[rng.choice(F, int(rng.integers(2, F + 1)), replace=False), i] = 1
    pcov = np.zeros((m, 9))
    pcov[rng.random(m) < 0.5] = (np.eye(3) * 1e-4).reshape(9)
    var = np.zeros((F, 6))
    var[0], var[1] = 1e-5, 1e-2
    cov = np.tile((np.eye(2) * sig ** 2).reshape(4), (m, 1))
    return dict(K=K, frame_pose=np.stack(poses), frame_prior_var=var, points=X + rng.normal(0, 5e-3, X.shape),
                point_prior_cov=pcov, obs=obs, obs_cov=[cov] * F, obs_valid=list(valid))


def main():
    ctx = capi.Context(0)
    for F in (4, 8):
        distinct = [window(1000 + s, F, 1000) for s in range(8)]
        batch = [distinct[p % 8] for p in range(512)]
        ctx.ba_refine_windows(batch[:8])   # warm-up: code object, workspace
        for run in range(3):
            t0 = time.perf_counter()
            out = ctx.ba_refine_windows(batch)
            dt = time.perf_counter() - t0
            print("F = %d m = 1000 x 512 windows: run %d  %.1f ms per call (host wall, transfers included), iterations %s, ok %d"
                  % (F, run, 1e3 * dt, sorted(set(r["iterations"] for r in out)), sum(r["ok"] for r in out)), flush=True)
    # the yardstick: ImagePair::refine of 512 resident pairs (refine_kernel<2>)
    data = synth.make_batch(0, 512, n_kp=2000)
    b = capi.Batch(ctx, 512, 2000)
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"], data["global_index"])
    b.run(capi.default_params(num_hypotheses=2000, sampler=capi.SAMPLER_PHILOX, seed=synth.SEED_BASE, max_error_sq=1e-2))
    b.sync()
    rp = capi.default_refine_params()
    b.refine(rp, 0.5)
    b.sync()
    for run in range(3):
        t0 = time.perf_counter()
        b.refine(rp, 0.5)
        b.sync()
        print("mvs_batch_refine 512 pairs: run %d  %.3f ms (host wall around launch + sync)" % (run, 1e3 * (time.perf_counter() - t0)),
              flush=True)
    b.close()
    ctx.close()


if __name__ == "__main__":
    main()
