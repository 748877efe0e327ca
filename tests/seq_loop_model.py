"""Loop closures of a resident sequence in numpy: the definitions of mvs_seq_loop_scores, mvs_seq_select_loops and
mvs_seq_add_loop_edges (include/mvslam_hip.h), so that the device's table, list and graph arrays
can be compared entry for entry and byte for byte.  The edge arithmetic is seq_graph_model's with (k, k + d) = (i, j)."""
import numpy as np

from seq_graph_model import chol6_ok, f64, trajectory_step

KIND_LOOP = 2


def hamming(train, query):
    """[n_train, n_query] Hamming distances of two uint8 descriptor arrays: |a| + |b| - 2 a.b on the unpacked bits (small
    integers: exact in binary32)"""
    a = np.unpackbits(train, axis=1).astype(np.float32)
    b = np.unpackbits(query, axis=1).astype(np.float32)
    return (a.sum(axis=1)[:, None] + b.sum(axis=1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)


def pair_score(train, query, ratio, max_dist):
    """queries that pass the matcher's test against the trains: n_train >= 2, (double)(float)D0 < ratio (double)(float)D1,
    max_dist < 0 or (double)(float)D0 <= max_dist; D0 <= D1 the two smallest distances with multiplicity"""
    if len(train) < 2 or len(query) < 1:
        return 0
    d = np.sort(hamming(train, query), axis=0)[:2]          # [2, n_query]
    d0 = d[0].astype(np.float32).astype(np.float64)
    d1 = d[1].astype(np.float32).astype(np.float64)
    ok = d0 < f64(ratio) * d1
    if not max_dist < 0:
        ok &= d0 <= f64(max_dist)
    return int(ok.sum())


def scores(desc, n_kp, ratio, max_dist, min_gap):
    """the [F, F] table: row i (base / train), column j (query), zero unless j - i >= min_gap"""
    F = len(n_kp)
    out = np.zeros((F, F), dtype=np.int32)
    for j in range(F):
        for i in range(0, j - min_gap + 1):
            out[i, j] = pair_score(desc[i][:n_kp[i]], desc[j][:n_kp[j]], ratio, max_dist)
    return out


def select(score, min_score, top_k, max_candidates):
    """(list of (i, j, score) cut at max_candidates, uncut count): per j the top_k entries with score >= min_score by
    descending score then ascending i; the list by ascending j"""
    F = score.shape[0]
    full = []
    for j in range(F):
        row = sorted(((-int(score[i, j]), i) for i in range(j) if score[i, j] >= min_score))[:top_k]
        full += [(i, j, -s) for s, i in row]
    return full[:max_candidates], len(full)


def loop_edge(R, t, i, j, rec, min_points=0, max_error=1e30, loop_sigma=(0.0, 0.0)):
    """the edge of candidate (i, j), or None: (Z [12], cov [36], scale).  The gates and the scaling of
    seq_graph_model.candidate; then loop_sigma^2 on the diagonal (where loop_sigma > 0); then the Cholesky test"""
    if not (rec["valid"] and rec["ok"]):
        return None
    if not int(rec["n_points"]) >= int(min_points):
        return None
    if not f64(rec["error"]) <= f64(max_error):
        return None
    with np.errstate(all="ignore"):
        q = trajectory_step(R, t, i, j - i)
        u = [f64(x) for x in np.asarray(rec["t"], dtype=np.float64).reshape(3)]
        s = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        if not (s > 0.0 and s < np.inf):
            return None
        C = np.asarray(rec["pose_cov"], dtype=np.float64).reshape(6, 6)
        f = [f64(1.0)] * 3 + [s] * 3
        cov = np.array([[(f[a] * C[a, b]) * f[b] for b in range(6)] for a in range(6)], dtype=np.float64)
        for a in range(6):
            sg = f64(loop_sigma[a // 3])
            if sg > 0.0:
                cov[a, a] = cov[a, a] + sg * sg
        if not chol6_ok(cov):
            return None
        Z = np.concatenate([np.asarray(rec["R"], dtype=np.float64).reshape(9), np.array([s * u[0], s * u[1], s * u[2]])])
    return Z, cov.reshape(36), float(s)


def add_loop_edges(built, R, t, cand, recs, **kw):
    """`built` (a graph of seq_graph_model.build or a download cut to the built edges) with the accepted candidates appended
    in candidate order; also accepted [len(cand)]"""
    g = {k: np.array(v, copy=True) for k, v in built.items() if isinstance(v, np.ndarray)}
    src, dst, lag, kind, Z, cov, scale, acc = [], [], [], [], [], [], [], []
    for (i, j, _), rec in zip(cand, recs):
        e = loop_edge(R, t, i, j, rec, **kw)
        acc.append(0 if e is None else 1)
        if e is None:
            continue
        src.append(i), dst.append(j), lag.append(j - i), kind.append(KIND_LOOP)
        Z.append(e[0]), cov.append(e[1]), scale.append(e[2])
    i32 = lambda a: np.array(a, dtype=np.int32)
    g["edge_src"] = np.concatenate([g["edge_src"], i32(src)])
    g["edge_dst"] = np.concatenate([g["edge_dst"], i32(dst)])
    g["edge_lag"] = np.concatenate([g["edge_lag"], i32(lag)])
    g["edge_kind"] = np.concatenate([g["edge_kind"], i32(kind)])
    g["edge_pose"] = np.concatenate([g["edge_pose"], np.array(Z, dtype=np.float64).reshape(-1, 12)])
    g["edge_cov"] = np.concatenate([g["edge_cov"], np.array(cov, dtype=np.float64).reshape(-1, 36)])
    g["edge_scale"] = np.concatenate([g["edge_scale"], np.array(scale, dtype=np.float64)])
    g["n_edges"] = len(g["edge_src"])
    g["anchor"] = 0
    return g, np.array(acc, dtype=np.int32)


def records(results, refined):
    """the per-candidate records loop_edge reads, from Sequence.download_loop_candidates(pairs=True)"""
    return [dict(valid=bool(r["valid"]), ok=bool(q["ok"]), n_points=int(r["n_points"]), error=float(q["error"]), R=q["R"],
                 t=q["t"], pose_cov=q["pose_cov"]) for r, q in zip(results, refined)]
