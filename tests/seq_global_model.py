"""The global problem of a resident sequence, in numpy (mvs_seq_refine_global).

build_global restates the definition the device is held to: links (test_seq_windows.build_links, section 4.7.1's), depths,
heads, tracks whole or cut into pieces of T frames, the points among them and their guesses, and the CSR by point.
plan_gap_free restates the plan of the sparse solver with the shortcuts tracks without gaps allow (what seq_global.hip
computes); tests/test_seq_global_host.py pins it against the brute-force plan and against mvs_bas::plan itself.
sparse_args turns an assembled problem into the arguments of Context.ba_refine_sparse: the host route to the same solve.
"""
import os
import subprocess

import numpy as np

from test_seq_windows import build_links

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def depths(pred):
    """depth[f][i]: 0 if no link arrives at keypoint i of frame f, else the depth of its predecessor + 1"""
    depth = np.zeros(pred.shape, np.int64)
    for f in range(1, pred.shape[0]):
        has = pred[f] >= 0
        depth[f, has] = depth[f - 1, pred[f, has]] + 1
    return depth


def build_global(pairs, traj, N, T=0):
    """pairs: per pair dict(valid, matches, mask, point_idx, points) as test_seq_windows.build_windows reads them; traj:
    dict(R, t, pair_scale).  T = 0: uncut tracks, else pieces of T frames.  Returns obs_off [P + 1], obs_frame / obs_kp [O],
    head_frame / head_kp [P], point_guess [P, 3], all in the order the definition gives -- points by (head frame, head
    keypoint), a point's observations by frame -- plus depth, tri_link [P] (which of the point's links, counted from 0, gave
    the guess) and longest_chain (frames of the longest chain of links, point or not)."""
    assert T == 0 or 2 <= T <= 4096
    n_frames = len(pairs) + 1
    succ, pred, rtp = build_links(pairs, N)
    depth = depths(pred)
    off, fr, kps, hf, hk, guess, tri = [0], [], [], [], [], [], []
    for j in range(n_frames - 1):
        for i in range(N):
            if succ[j, i] < 0 or (depth[j, i] % T != 0 if T else depth[j, i] != 0):
                continue
            track, g, g_link, f, cur = [i], None, -1, j, i
            while (T == 0 or len(track) < T) and f < n_frames - 1 and succ[f, cur] >= 0:
                r = succ[f, cur]
                if g is None and rtp[f, r] >= 0:
                    x = pairs[f]["points"][rtp[f, r]]
                    g, g_link = traj["R"][f] @ (traj["pair_scale"][f] * x) + traj["t"][f], len(track) - 1
                cur = int(pairs[f]["matches"]["queryIdx"][r])
                f += 1
                track.append(cur)
            if g is None:
                continue
            assert len(track) >= 2
            fr += list(range(j, j + len(track)))
            kps += track
            off.append(len(fr))
            hf.append(j)
            hk.append(i)
            guess.append(g)
            tri.append(g_link)
    return dict(obs_off=np.array(off, np.int32), obs_frame=np.array(fr, np.int32), obs_kp=np.array(kps, np.int32),
                head_frame=np.array(hf, np.int32), head_kp=np.array(hk, np.int32),
                point_guess=np.array(guess, float).reshape(-1, 3), depth=depth, tri_link=np.array(tri, np.int64),
                longest_chain=int(depth.max()) + 1)


def plan_gap_free(F, obs_off, obs_frame, head_frame):
    """every list of mvs_bas::plan for tracks without gaps, by the shortcuts of DESIGN.md section 4.7.5: a frame's list in
    ascending index is in head-frame order; first[i] is the smallest head frame in frame i's list; the pairs of block (i, j),
    j < i, are the entries of frame i's list whose point starts at or before j, paired with the observation that lies
    j - head_frame behind the point's first; their number is a running sum over a histogram of i - head_frame."""
    P, O = len(obs_off) - 1, len(obs_frame)
    obs_point = np.repeat(np.arange(P), np.diff(obs_off))
    by_frame = [[o for o in range(O) if obs_frame[o] == f] for f in range(F)]
    first = [min([int(head_frame[obs_point[o]]) for o in by_frame[i]] + [i]) for i in range(F)]
    row_off = [0]
    for i in range(F):
        row_off.append(row_off[-1] + i - first[i] + 1)
    last = [max(i for i in range(F) if first[i] <= j <= i) for j in range(F)]
    pair_off, pa, pc = [0], [], []
    for i in range(F):
        hist = np.zeros(i + 2, np.int64)
        for o in by_frame[i]:
            hist[i - head_frame[obs_point[o]]] += 1
        for j in range(first[i], i + 1):
            n = int(hist[i - j:].sum()) if j < i else 0          # points that started at or before frame j
            heads = [int(head_frame[obs_point[o]]) for o in by_frame[i]]
            assert heads == sorted(heads)
            take = [o for o in by_frame[i] if head_frame[obs_point[o]] <= j] if j < i else []
            assert len(take) == n and take == by_frame[i][:n]     # a prefix of the frame's list
            pa += take
            pc += [int(obs_off[obs_point[o]] + j - head_frame[obs_point[o]]) for o in take]
            pair_off.append(len(pa))
    return dict(first=first, row_off=row_off, blk_row=[i for i in range(F) for _ in range(first[i], i + 1)], last=last,
                obs_point=[int(p) for p in obs_point], fr_off=[int(x) for x in np.cumsum([0] + [len(b) for b in by_frame])],
                fr_obs=[o for b in by_frame for o in b], pair_off=pair_off, pair_a=pa, pair_c=pc, blocks=[row_off[-1]],
                pairs=[len(pa)], widest=[max(i - first[i] + 1 for i in range(F))])


PLAN_LISTS = ("first", "row_off", "blk_row", "last", "obs_point", "fr_off", "fr_obs", "pair_off", "pair_a", "pair_c")


def compile_planner(directory, sanitize=True):
    """tests/cpp/ba_envelope_dump.cpp as it stands, a program of its own (with the host sanitizers unless told otherwise).
    Returns run(F, obs_off, obs_frame) -> {name: list}: mvs_bas::check_csr and every list of mvs_bas::plan."""
    exe = os.path.join(str(directory), "ba_envelope_dump")
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "mvslam_amd", "csrc"), "-o", exe,
                                                          os.path.join(ROOT, "tests", "cpp", "ba_envelope_dump.cpp")])

    def run(F, obs_off, obs_frame):
        path = os.path.join(str(directory), "problem.txt")
        with open(path, "w") as f:
            f.write("%d %d %d\n%s\n%s\n" % (F, len(obs_off) - 1, len(obs_frame), " ".join(map(str, obs_off)),
                                           " ".join(map(str, obs_frame))))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        out = {}
        for ln in r.stdout.splitlines():
            w = ln.split()
            out[w[0]] = [int(x) for x in w[1:]]
        return out

    return run


def sparse_args(prob, traj, kp, octave, K, params, sigma_px):
    """keyword arguments of Context.ba_refine_sparse for an assembled problem (the model's, or a device's download): the
    trajectory as poses and prior means, frame 0 with anchor_sigma and the others with pose_sigma, every point with the prior
    point_sigma^2 I at its guess, observations = the keypoints with the covariance (sigma_px * 2^octave)^2 I"""
    F = len(traj["R"])
    poses = np.concatenate([np.asarray(traj["R"], float).reshape(F, 9), np.asarray(traj["t"], float)], axis=1)
    an, ps, pt = list(params.anchor_sigma), list(params.pose_sigma), params.point_sigma
    var = np.array([[s[0] * s[0]] * 3 + [s[1] * s[1]] * 3 for s in [an] + [ps] * (F - 1)])
    fr, kpi = prob["obs_frame"], prob["obs_kp"]
    P = len(prob["head_frame"])
    sd = np.ldexp(float(sigma_px), np.minimum(octave[fr, kpi].astype(np.int32), 30))
    c = sd * sd
    return dict(K=K, frame_pose=poses, frame_prior_var=var, points=prob["point_guess"],
                point_prior_cov=np.tile((np.eye(3) * (pt * pt)).reshape(9), (P, 1)), obs_off=prob["obs_off"],
                obs_frame=prob["obs_frame"], obs_uv=kp[fr, kpi].astype(np.float64),
                obs_cov=np.stack([c, np.zeros_like(c), np.zeros_like(c), c], 1), params=params)
