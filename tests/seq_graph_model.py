"""The pose graph of a resident sequence in numpy: the definition mvs_seq_build_pose_graph implements (include/mvslam_hip.h,
DESIGN.md section 4.10.1), operation by operation, so that the device's arrays can be compared byte for byte.

Input: the trajectory (R [F, 3, 3], t [F, 3]: Sequence.download_trajectory()) and, per lag d, one record per base frame k <
F - d with the fields valid, ok, n_points, error, R, t, pose_cov (tables_from_downloads() makes them from
Sequence.download_lag_pairs / download_lag_refined).  Output: the graph, its edges in slot order (ascending (d, k)).

Every value is a chain of single binary64 operations in the order the header writes them.  The one place where the device
uses fused multiply-adds is the 6 x 6 Cholesky test (pg_prep_kernel's); it only decides, so the model repeats its fused
operations exactly, in rational arithmetic, and the decision is the device's even at a pivot that is zero to rounding."""
import math
from fractions import Fraction

import numpy as np

KIND_MEASURED, KIND_CHAIN = 0, 1
f64 = np.float64


def slot_offset(n_frames, d):
    """first slot of lag d: slots are (1, 0) .. (1, F - 2), (2, 0) .. (2, F - 3), ..."""
    return (d - 1) * n_frames - d * (d - 1) // 2


def n_slots(n_frames, max_lag):
    return max_lag * n_frames - max_lag * (max_lag + 1) // 2


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def chol6_ok(S):
    """chol_packed<6> of posegraph.hip on the lower triangle of S (6 x 6): are all six pivots > 0 and finite?"""
    S = np.asarray(S, dtype=np.float64).reshape(6, 6)
    if not all(math.isfinite(S[r, c]) for r in range(6) for c in range(r + 1)):
        return False   # a pivot of that row is then not a positive finite number (inf - inf, or -inf)
    L = [[float(S[r, c]) for c in range(6)] for r in range(6)]
    try:
        for j in range(6):
            d = L[j][j]
            for k in range(j):
                d = _fma(-L[j][k], L[j][k], d)
            if not (d > 0.0 and d < math.inf):
                return False
            inv = float(f64(1.0) / np.sqrt(f64(d)))
            L[j][j] = inv
            for i in range(j + 1, 6):
                v = L[i][j]
                for k in range(j):
                    v = _fma(-L[i][k], L[j][k], v)
                L[i][j] = float(f64(v) * f64(inv))
                if not math.isfinite(L[i][j]):
                    return False   # it enters row i's pivot squared
    except OverflowError:
        return False
    return True


def trajectory_step(R, t, k, d):
    """q = R_k^T (t_{k+d} - t_k), in the device's order"""
    Rk = np.asarray(R[k], dtype=np.float64).reshape(3, 3)
    D = [f64(t[k + d][i]) - f64(t[k][i]) for i in range(3)]
    return [(Rk[0, i] * D[0] + Rk[1, i] * D[1]) + Rk[2, i] * D[2] for i in range(3)]


def candidate(R, t, k, d, rec, min_points=0, max_error=1e30):
    """the measured edge of slot (d, k), or None: (Z [12], cov [36], scale)"""
    if not (rec["valid"] and rec["ok"]):
        return None
    if not int(rec["n_points"]) >= int(min_points):
        return None
    if not f64(rec["error"]) <= f64(max_error):
        return None
    with np.errstate(all="ignore"):
        q = trajectory_step(R, t, k, d)
        u = [f64(x) for x in np.asarray(rec["t"], dtype=np.float64).reshape(3)]
        s = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        if not (s > 0.0 and s < np.inf):
            return None
        C = np.asarray(rec["pose_cov"], dtype=np.float64).reshape(6, 6)
        f = [f64(1.0)] * 3 + [s] * 3
        cov = np.array([[(f[i] * C[i, j]) * f[j] for j in range(6)] for i in range(6)], dtype=np.float64)
        if not chol6_ok(cov):
            return None
        Z = np.concatenate([np.asarray(rec["R"], dtype=np.float64).reshape(9), np.array([s * u[0], s * u[1], s * u[2]])])
    return Z, cov.reshape(36), float(s)


def chain_edge(R, t, k, chain_sigma):
    """the fallback edge (k, k + 1): Z = G_k^-1 G_{k+1} with R_k^T in front, S = diag(sigma_r^2 I, sigma_t^2 I)"""
    Rk, Rn = np.asarray(R[k], dtype=np.float64).reshape(3, 3), np.asarray(R[k + 1], dtype=np.float64).reshape(3, 3)
    Z = np.zeros(12)
    for i in range(3):
        for j in range(3):
            Z[3 * i + j] = (Rk[0, i] * Rn[0, j] + Rk[1, i] * Rn[1, j]) + Rk[2, i] * Rn[2, j]
    Z[9:] = trajectory_step(R, t, k, 1)
    v = [f64(chain_sigma[0]) * f64(chain_sigma[0]), f64(chain_sigma[1]) * f64(chain_sigma[1])]
    return Z, np.diag([v[0]] * 3 + [v[1]] * 3).reshape(36), 1.0


def build(R, t, tables, max_lag, min_points=0, max_error=1e30, chain_sigma=(0.0, 0.0)):
    """the graph of the sequence: node_pose [F, 12], edge_src / edge_dst / edge_lag / edge_kind (int32), edge_pose [E, 12],
    edge_cov [E, 36], edge_scale [E], n_edges, anchor = 0; also slots = [(d, k)] of the edges"""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    F = R.shape[0]
    chain_on = chain_sigma[0] > 0.0 and chain_sigma[1] > 0.0
    src, dst, lag, kind, Z, cov, scale, slots = [], [], [], [], [], [], [], []
    for d in range(1, max_lag + 1):
        assert len(tables[d]) >= F - d
        for k in range(F - d):
            e, kd = candidate(R, t, k, d, tables[d][k], min_points, max_error), KIND_MEASURED
            if e is None and d == 1 and chain_on:
                e, kd = chain_edge(R, t, k, chain_sigma), KIND_CHAIN
            if e is None:
                continue
            src.append(k), dst.append(k + d), lag.append(d), kind.append(kd), slots.append((d, k))
            Z.append(e[0]), cov.append(e[1]), scale.append(e[2])
    i32 = lambda a: np.array(a, dtype=np.int32)
    return dict(node_pose=np.concatenate([R.reshape(F, 9), t.reshape(F, 3)], axis=1), edge_src=i32(src), edge_dst=i32(dst),
                edge_lag=i32(lag), edge_kind=i32(kind), edge_pose=np.array(Z, dtype=np.float64).reshape(-1, 12),
                edge_cov=np.array(cov, dtype=np.float64).reshape(-1, 36), edge_scale=np.array(scale, dtype=np.float64),
                n_edges=len(src), anchor=0, slots=slots)


def tables_from_downloads(pairs, refined):
    """pairs[d] = Sequence.download_lag_pairs(d), refined[d] = Sequence.download_lag_refined(d, point_cov=...)"""
    out = {}
    for d in pairs:
        out[d] = [dict(valid=bool(r["valid"]), ok=bool(q["ok"]), n_points=int(r["n_points"]), error=float(q["error"]), R=q["R"],
                       t=q["t"], pose_cov=q["pose_cov"]) for r, q in zip(pairs[d]["results"], refined[d]["refined"])]
    return out


GRAPH_KEYS = ("node_pose", "edge_src", "edge_dst", "edge_pose", "edge_cov", "edge_lag", "edge_kind", "edge_scale")


def same_bytes(a, b):
    """the keys of GRAPH_KEYS (and the count) that differ between two graphs"""
    bad = [k for k in GRAPH_KEYS if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]
    return bad + (["n_edges"] if int(a["n_edges"]) != int(b["n_edges"]) else [])
