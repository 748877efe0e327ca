"""The depth-ratio scale rule of a resident sequence, in numpy (mvs_seq_rescale, MVS_SEQ_SCALE_DEPTH_RATIO; DESIGN.md
section 4.6.1).

scale_steps restates the definition the device is held to, operation by operation: the shared points of two consecutive pairs
(the smallest point of pair q + 1 per keypoint wins), their two depths in frame q + 1, the lower median of the ratios.
trajectory restates the fold: sigma as a sequential product, G_{k+1} = G_k o (R_k, sigma_k t_k) in seq_chain_kernel's compose
order, from the pairs alone.  Every floating-point operation is a separate numpy ufunc call or a Python float operation (one
IEEE binary64 rounding each, nothing fused), so the results are the device's bits.

A pair is a dict(valid, R [3, 3], t [3], matches, point_idx [n_points], points [n_points, 3]); pairs_of_download builds the
list from Sequence.download_pairs().
"""
import numpy as np

STEP_DTYPE = np.dtype([("n_common", "<i4"), ("n_used", "<i4"), ("flag", "<i4"), ("reserved", "<i4"), ("scale", "<f8")])
RULE_CHAIN, RULE_DEPTH_RATIO = 0, 1
FLAG_OK, FLAG_INVALID_PAIR, FLAG_FEW = 0, 1, 2


def pairs_of_download(gp):
    """the model's pairs from Sequence.download_pairs()"""
    pairs = []
    for k, r in enumerate(gp["results"]):
        M, n = int(r["n_matches"]), int(r["n_points"]) if r["valid"] else 0
        pairs.append(dict(valid=bool(r["valid"]), R=np.array(r["R"], np.float64).reshape(3, 3),
                          t=np.array(r["t"], np.float64).reshape(3), matches=gp["matches"][k][:M],
                          point_idx=gp["point_idx"][k][:n], points=gp["points"][k][:n]))
    return pairs


def point_keypoints(pair, N):
    """(a, b, ok) per point of a pair: base keypoint (frame k), new keypoint (frame k + 1), and whether the match row and both
    keypoints lie inside the frame arrays.  An invalid pair has no points."""
    if not pair["valid"]:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, bool)
    r = np.asarray(pair["point_idx"], np.int64)[:N]
    ok = (r >= 0) & (r < min(N, len(pair["matches"])))
    rr = np.where(ok, r, 0)
    mt = pair["matches"]
    a = mt["trainIdx"].astype(np.int64)[rr] if len(mt) else np.zeros(len(r), np.int64)
    b = mt["queryIdx"].astype(np.int64)[rr] if len(mt) else np.zeros(len(r), np.int64)
    ok &= (a >= 0) & (a < N) & (b >= 0) & (b < N)
    return a, b, ok


def shared_points(pq, pn, N):
    """(j, j') of the points pairs q and q + 1 share, by ascending j': keypoint c of frame q + 1 is the new keypoint of point
    j of pair q and the base keypoint of point j' of pair q + 1; of several j' with one base keypoint the smallest wins."""
    _, bq, okq = point_keypoints(pq, N)
    an, _, okn = point_keypoints(pn, N)
    at = np.full(N, -1, np.int64)            # point of pair q at each keypoint of frame q + 1 (b is unique per row)
    at[bq[okq]] = np.nonzero(okq)[0]
    first = np.full(N, -1, np.int64)         # the smallest point of pair q + 1 per base keypoint
    for jn in np.nonzero(okn)[0][::-1]:
        first[an[jn]] = jn
    js, jns = [], []
    for jn in np.nonzero(okn)[0]:
        c = an[jn]
        if first[c] == jn and at[c] >= 0:
            js.append(at[c])
            jns.append(jn)
    return np.array(js, np.int64), np.array(jns, np.int64)


def ratios(pq, pn, j, jn):
    """(rho, used) of the shared points: z_a = the depth in frame q + 1 of pair q's point, z_b = that of pair q + 1's"""
    R, t = pq["R"], pq["t"]
    x = np.asarray(pq["points"], np.float64).reshape(-1, 3)[j].reshape(-1, 3)
    d0, d1, d2 = x[:, 0] - t[0], x[:, 1] - t[1], x[:, 2] - t[2]
    za = (R[0, 2] * d0 + R[1, 2] * d1) + R[2, 2] * d2
    zb = np.asarray(pn["points"], np.float64).reshape(-1, 3)[jn].reshape(-1, 3)[:, 2]
    used = np.isfinite(za) & (za > 0) & np.isfinite(zb) & (zb > 0)
    with np.errstate(all="ignore"):
        rho = za / np.where(used, zb, 1.0)
    return rho, used


def scale_steps(pairs, N, min_common):
    """the n_frames - 2 step records of MVS_SEQ_SCALE_DEPTH_RATIO"""
    steps = np.zeros(max(len(pairs) - 1, 0), STEP_DTYPE)
    for q in range(len(steps)):
        pq, pn = pairs[q], pairs[q + 1]
        steps[q]["scale"] = 1.0
        if not (pq["valid"] and pn["valid"]):
            steps[q]["flag"] = FLAG_INVALID_PAIR
            continue
        j, jn = shared_points(pq, pn, N)
        rho, used = ratios(pq, pn, j, jn)
        n = int(used.sum())
        steps[q]["n_common"], steps[q]["n_used"] = len(j), n
        if n < min_common:
            steps[q]["flag"] = FLAG_FEW
            continue
        steps[q]["scale"] = np.sort(rho[used])[(n - 1) // 2]      # the lower median
    return steps


def compose(AR, At, R, t, sig):
    """A o (R, sig t) in seq_chain_kernel's order: s = sig t first, then (A0 c0 + A1 c1) + A2 c2 (+ A.t)"""
    s = sig * t
    oR = (AR[:, 0:1] * R[0] + AR[:, 1:2] * R[1]) + AR[:, 2:3] * R[2]
    ot = ((AR[:, 0] * s[0] + AR[:, 1] * s[1]) + AR[:, 2] * s[2]) + At
    return oR, ot


def trajectory(pairs, scale):
    """dict(R, t, pair_scale, track_scale) as mvs_seq_download_trajectory gives them after a rescale: sigma_0 = 1,
    sigma_{q+1} = sigma_q scale_q in order; G_0 = I, G_{k+1} = G_k o (R_k, sigma_k t_k); an invalid pair is the identity"""
    P = len(pairs)
    sigma = np.ones(P)
    for q in range(P - 1):
        sigma[q + 1] = sigma[q] * scale[q]
    R, t = np.zeros((P + 1, 3, 3)), np.zeros((P + 1, 3))
    R[0] = np.eye(3)
    for k, p in enumerate(pairs):
        pr, pt = (p["R"], p["t"]) if p["valid"] else (np.eye(3), np.zeros(3))
        R[k + 1], t[k + 1] = compose(R[k], t[k], pr, pt, sigma[k])
    return dict(R=R, t=t, pair_scale=sigma, track_scale=np.array(scale, np.float64).reshape(max(P - 1, 0)))


def rescale(pairs, N, min_common=1):
    """(steps, trajectory) of mvs_seq_rescale(MVS_SEQ_SCALE_DEPTH_RATIO, min_common)"""
    steps = scale_steps(pairs, N, min_common)
    return steps, trajectory(pairs, steps["scale"])
