"""Two full-size sequences for the consumers of a resident sequence: FULL, 4 frames at the capacity
of 4096 keypoints, and WORK, 5 frames of 2000 keypoints, the benchmark's frame size (not a multiple of 256; the capacity is
2000, not rounded up), and a loop sequence of 2000 keypoints.  Both come from synth.make_sequence with the ratios of
test_seq_windows.SEQ_ARGS (n_map = 2.5 n_kp, step 0.1, noise 0.3 px), so that a keypoint usually survives three frames, and
the generator seed of test_seq_track.py; the hypothesis counts are test_seq_windows.PRM / PPRM and test_seq_odometry's.

tests/test_seq_fullsize_host.py shows on the CPU oracle alone that they reach the paths small frames never reach;
tests/test_seq_fullsize.py runs every consumer on them against its existing model.
"""
import numpy as np

import oracle_lib as o
import test_seq_track as st
import test_seq_windows as sw
import test_sequence as ts
from mvslam_amd import synth

# FULL flips a quarter of the descriptor bits the generator flips by default: at its default of 0.02 two views of a map point
# lie 10 bits apart on average, the matcher's max_dist = 10 drops half of them, a pair has 1800 points and no point index
# reaches 2048; at 0.005 a pair has 3200 points.  WORK keeps the default, as the benchmark's sequence does.
FULL_FRAMES, FULL_ARGS = 4, dict(n_kp=4096, n_map=10240, noise_px=0.3, step=0.1, flip_p=0.005, seed=st.SEED)
WORK_FRAMES, WORK_ARGS = 5, dict(n_kp=2000, n_map=5000, noise_px=0.3, step=0.1, seed=st.SEED)
SEQS = dict(FULL=(FULL_FRAMES, FULL_ARGS), WORK=(WORK_FRAMES, WORK_ARGS))
MAX_LAG = 2
SIGMA_PX = 0.5

# the loop sequence: test_seq_loops.LOOP_ARGS at 2000 keypoints.  Frame f of the return leg revisits frame 2 H - 1 - f,
# H = ceil(F / 2): 10 frames is the smallest count with a revisit test_seq_loops.LOOP_GAP = 8 frames or more behind its
# outbound frame (frame 9 revisits frame 0; with 9 frames the widest gap is 7).  At that gap the table has three entries,
# (0, 8), (0, 9) and (1, 9): the revisit and its two neighbours (tests/test_seq_fullsize_host.py shows it on the model).
LOOP_FRAMES = 10
LOOP_ARGS = dict(shift=0.1, seed=st.SEED, n_kp=2000, n_map=5000, noise_px=0.3, step=0.5, yaw_step=0.08)


def make(name):
    F, args = SEQS[name]
    return synth.make_sequence(F, **args)


def make_loop():
    return synth.make_loop_sequence(LOOP_FRAMES, **LOOP_ARGS)


def octaves(n_frames, n_kp):
    """test_seq_track._octaves for any frame size: octaves 0 .. 2, so that the observation weights differ"""
    return (np.arange(n_frames * n_kp).reshape(n_frames, n_kp) % 3).astype(np.uint8)


def oracle_lagged(seq, lag, threads=16):
    """the oracle's pairs (k, k + lag) with test_seq_windows.PRM, as records with `valid`"""
    F, K = len(seq["n_kp"]), seq["K"]

    def pair(k):
        op = o.make_params(sw.PRM["H"], o.SAMPLER_PHILOX, sw.PRM["seed"] + k, sw.PRM["thr"])
        a, b = seq["n_kp"][k], seq["n_kp"][k + lag]
        return o.image_pair(seq["desc"][k][:a], seq["kp"][k][:a], seq["desc"][k + lag][:b], seq["kp"][k + lag][:b], K, op,
                            0.7, 10.0)

    return [dict(p, valid=p["ok"]) for p in ts._pool(pair, F - lag, threads)]


def oracle_tables(seq, lagged, threads=16):
    """seq_graph_model's tables from the oracle alone: per lag, the pair and its refinement (oracle_lib.sfm_refine on the
    triangulated matches, observation covariances (SIGMA_PX 2^octave)^2 I as the device weighs them)"""
    F, N = seq["kp"].shape[0], seq["kp"].shape[1]
    octv = octaves(F, N)
    tables = {}
    for d, pairs in lagged.items():
        def refine(k, d=d, pairs=pairs):
            p = pairs[k]
            if not p["valid"]:
                return dict(valid=False, ok=False, n_points=0, error=0.0, R=np.eye(3), t=np.zeros(3), pose_cov=np.zeros((6, 6)))
            mt = p["matches"][p["point_idx"]]
            a, b = mt["trainIdx"], mt["queryIdx"]
            cov = []
            for frame, idx in ((k, a), (k + d, b)):
                sd = np.ldexp(SIGMA_PX, octv[frame][idx].astype(np.int32))
                cov.append(np.stack([sd * sd, np.zeros(len(idx)), np.zeros(len(idx)), sd * sd], 1))
            r = o.sfm_refine(seq["kp"][k][a].astype(np.float64), cov[0], seq["kp"][k + d][b].astype(np.float64), cov[1],
                             seq["K"], p["R"], p["t"], p["points"])
            return dict(valid=True, ok=r["ok"], n_points=len(p["point_idx"]), error=r["error"], R=r["R"], t=r["t"],
                        pose_cov=r["pose_cov"])

        tables[d] = ts._pool(refine, len(pairs), threads)
    return tables


def oracle_trajectory(pairs, tracks):
    """the chain's trajectory of the oracle's pairs and tracks"""
    return o.seq_chain([p["R"] for p in pairs], [p["t"] for p in pairs], np.array([p["ok"] for p in pairs], np.int32),
                       [t.get("R", np.eye(3)) for t in tracks], [t.get("t", np.zeros(3)) for t in tracks],
                       np.array([t["ok"] for t in tracks], np.int32))
