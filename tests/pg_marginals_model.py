"""numpy model of the pose-graph marginals (include/mvslam_hip.h mvs_pose_graph_marginals), on top
of posegraph_model's residuals:

    H = J_a^T W_a J_a + sum_k J_k^T W_k J_k  at the poses X, no lambda;   Sigma = H^-1.

It provides the dense H, the envelope, a float64 restatement of the device's skyline factorisation and forward solves (the
same operations in the same order, block by block -- numpy has no fused multiply-add, so not the same bits) and an
extended-precision Sigma_ref: the float64 inverse improved by Newton steps X <- X (2 I - H X) with the residual in
numpy.longdouble (exactly summed products where longdouble is only 64 bits wide).

It also holds the fixtures and the error measure the host and the GPU tests share."""
import math

import numpy as np

import posegraph_model as pm

EPS = 2.0 ** -52
FLOOR = 64 * EPS          # of the accuracy bound
MARGIN = 8.0              # the device against the larger of the two float64 host methods
MAX_ENVELOPE_BLOCKS = 1 << 21


def dense_h(g, poses=None, anchor_sigma=pm.ANCHOR_SIGMA):
    """the 6N x 6N H of the contract at `poses` (None: the graph's node_pose)"""
    X = np.asarray(g["node_pose"] if poses is None else poses, dtype=np.float64).reshape(-1, 12)
    wa = np.repeat(1.0 / np.asarray(anchor_sigma, dtype=np.float64), 3)
    _, J = pm._residuals(g, pm.whitening(g["edge_cov"]), wa, X, True)
    return J.T @ J


def envelope(n_nodes, src, dst):
    """(first, row_off, blocks): first[i] = the smallest of i and its neighbours; row i stores the blocks first[i] .. i"""
    first = np.arange(n_nodes, dtype=np.int64)
    for s, d in zip(src, dst):
        lo, hi = min(int(s), int(d)), max(int(s), int(d))
        first[hi] = min(first[hi], lo)
    width = np.arange(n_nodes) - first + 1
    row_off = np.concatenate([[0], np.cumsum(width)])
    return first, row_off, int(width.sum())


def graph_envelope(g):
    return envelope(g["node_pose"].shape[0], g["edge_src"], g["edge_dst"])


def _chol6(S):
    """chol_packed's statements on a 6 x 6 block: the lower factor with 1 / l_jj on the diagonal, and the pivots"""
    L = np.zeros((6, 6))
    piv = np.zeros(6)
    for j in range(6):
        d = S[j, j] - float(L[j, :j] @ L[j, :j])
        piv[j] = d
        if not (d > 0.0 and np.isfinite(d)):
            raise np.linalg.LinAlgError("pivot")
        inv = 1.0 / math.sqrt(d)
        L[j, j] = inv
        for i in range(j + 1, 6):
            L[i, j] = (S[i, j] - float(L[i, :j] @ L[j, :j])) * inv
    return L, piv


def skyline_factor(H, first):
    """H = L L^T inside the envelope, row by row as pgm_factor_kernel: returns (rows, min_pivot) with rows[i] the blocks
    first[i] .. i of L, [w_i, 6, 6]; a diagonal block holds 1 / l_jj on its diagonal.  Raises LinAlgError on a pivot."""
    N = len(first)
    rows, min_d = [], np.inf
    for i in range(N):
        f = int(first[i])
        row = np.array([H[6 * i:6 * i + 6, 6 * c:6 * c + 6] for c in range(f, i + 1)])
        for c in range(f, i):
            Lcc = rows[c][c - int(first[c])]
            B, Y = row[c - f], np.zeros((6, 6))
            for q in range(6):
                Y[:, q] = (B[:, q] - Y[:, :q] @ Lcc[q, :q]) * Lcc[q, q]
            row[c - f] = Y
            for cp in range(c + 1, i + 1):
                fc = int(first[cp])
                if fc > c:
                    continue
                M = rows[cp][c - fc] if cp < i else Y
                row[cp - f] = row[cp - f] - Y @ M.T
        L, piv = _chol6(row[i - f])
        min_d = min(min_d, float(piv.min()))
        row[i - f] = L
        rows.append(row)
    return rows, math.sqrt(min_d)


def skyline_columns(rows, first, n):
    """L^-1 E_n as pgm_solve_kernel computes it: [N, 6, 6], zero above row n"""
    N = len(first)
    Y = np.zeros((N, 6, 6))
    for r in range(n, N):
        f = int(first[r])
        k0 = max(f, n)
        rhs = np.eye(6) if r == n else np.zeros((6, 6))
        if r > k0:
            rhs = rhs - np.einsum("kab,kbc->ac", rows[r][k0 - f:r - f], Y[k0:r])
        Lrr = rows[r][r - f]
        for m in range(6):
            Y[r, m] = (rhs[m] - Lrr[m, :m] @ Y[r, :m]) * Lrr[m, m]
    return Y


def skyline_cov(H, first, queries):
    """the float64 restatement: Sigma_ij = (L^-1 E_i)^T (L^-1 E_j) for every query, [n, 6, 6]"""
    rows, _ = skyline_factor(H, first)
    cols = {}
    out = np.zeros((len(queries), 6, 6))
    for n, (i, j) in enumerate(queries):
        for v in (int(i), int(j)):
            if v not in cols:
                cols[v] = skyline_columns(rows, first, v)
        hi = max(int(i), int(j))
        out[n] = np.einsum("rma,rmb->ab", cols[int(i)][hi:], cols[int(j)][hi:])
    return out


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker), elementwise"""
    p = a * b
    def split(x):
        t = 134217729.0 * x
        hi = t - (t - x)
        return hi, x - hi
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _residual(H, X):
    """I - H X, accurate well beyond float64: in longdouble where that is wider, from exactly summed products otherwise"""
    n = H.shape[0]
    if np.finfo(np.longdouble).eps < 1e-18:
        R = np.eye(n, dtype=np.longdouble) - H.astype(np.longdouble) @ X
        return R
    Xh = np.asarray(X[0], dtype=np.float64)
    Xl = np.asarray(X[1], dtype=np.float64)
    R = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            p, e = _two_prod(H[i], Xh[:, j])
            R[i, j] = math.fsum([1.0 if i == j else 0.0] + (-p).tolist() + (-e).tolist() + (-(H[i] * Xl[:, j])).tolist())
    return R


def sigma_ref(H, steps=4):
    """H^-1 to well below a float64 ulp of its entries (of its largest entries, per row and column scaling aside): returned
    as float64 after the Newton steps have converged in the wider format"""
    X0 = np.linalg.inv(H)
    wide = np.finfo(np.longdouble).eps < 1e-18
    X = X0.astype(np.longdouble) if wide else (X0, np.zeros_like(X0))
    for _ in range(steps):
        R = _residual(H, X)
        if wide:
            X = X + (X.astype(np.float64) @ R.astype(np.float64)).astype(np.longdouble)
        else:
            corr = X[0] @ R
            hi = X[0] + corr
            X = (hi, X[1] + ((X[0] - hi) + corr))
        if float(np.abs(R).max()) < 1e-17:
            break
    return np.asarray(X if wide else X[0] + X[1], dtype=np.float64)


def block(S, i, j):
    return S[6 * i:6 * i + 6, 6 * j:6 * j + 6]


def block_errors(cov, S_ref, queries):
    """err of every queried block: |cov - ref|_F / sqrt(|ref_ii|_F |ref_jj|_F)"""
    out = np.zeros(len(queries))
    for n, (i, j) in enumerate(queries):
        ref = block(S_ref, int(i), int(j))
        scale = math.sqrt(np.linalg.norm(block(S_ref, int(i), int(i))) * np.linalg.norm(block(S_ref, int(j), int(j))))
        out[n] = np.linalg.norm(np.asarray(cov[n]).reshape(6, 6) - ref) / scale
    return out


def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(n)]


def host_errors(H, first, queries, S_ref=None):
    """(largest block error of numpy.linalg.inv(H), of the skyline restatement, Sigma_ref) over `queries`"""
    S_ref = sigma_ref(H) if S_ref is None else S_ref
    Sinv = np.linalg.inv(H)
    e_inv = block_errors([block(Sinv, i, j) for i, j in queries], S_ref, queries).max()
    e_sky = block_errors(skyline_cov(H, first, queries), S_ref, queries).max()
    return float(e_inv), float(e_sky), S_ref


def bound(e_inv, e_sky):
    """what the device is held to: 8 x the larger of the two float64 host methods, never below 64 ulp"""
    return max(MARGIN * max(e_inv, e_sky), FLOOR)


# ---- fixtures: name -> graph, each named for what it breaks --------------------------------------------------------------------
def chain40():
    """40 nodes out along x and back beside the way out, edges (i, i + 1), and two closures across the gap: (0, 39) and
    (5, 34).  Rows 39 and 34 reach far back, every other row is two blocks wide."""
    rng = np.random.default_rng(4040)
    truth = []
    for i in range(40):
        out = i < 20
        x = 0.5 * i if out else 0.5 * (39 - i)
        truth.append(pm.se3([0.05 * np.sin(0.7 * i), 0.04 * np.cos(0.5 * i), 0.0 if out else np.pi],
                            [x, 0.0 if out else 0.4, 0.02 * i]))
    truth = np.array(truth)
    edges = [(i, i + 1) for i in range(39)] + [(0, 39), (5, 34)]
    Z = [pm.compose(pm.between(truth[s], truth[d]), pm.se3(rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.01))
         for s, d in edges]
    guess = np.array([truth[0]] + [pm.retract(truth[i], rng.normal(size=6) * 0.05) for i in range(1, 40)])
    return pm.graph(guess, edges, Z, pm.full_cov(rng, len(edges)))


RING24_PERM = [(7 * i + 3) % 24 for i in range(24)]

FIXTURES = {
    "one_node": lambda: pm.dense_size(1),                       # no edge: the anchor prior alone
    "two_nodes": lambda: pm.trivial()[0],
    "triangle": lambda: pm.triangle(0)[0],
    "ring24": lambda: pm.ring(24, chords=(2,)),                 # the last rows reach back to node 0: long and short rows
    "star70": pm.star,                                          # full lower triangle, row widths 1 .. 71
    "all_pairs16": pm.all_pairs16,                              # 272 edges on 16 nodes: long term lists per block
    "ring17": lambda: pm.ring(17, chords=(2,)),                 # dense_size's graph one node past the optimiser's dense path
    "full_cov": pm.full_cov_graph,
    "near_pi_ring": lambda: pm.near_pi_ring()[0],
    "ring24_relabelled": lambda: pm.relabelled(pm.ring(24, chords=(2,)), RING24_PERM),   # the blocks permute, another envelope
    "chain40": chain40,
}
