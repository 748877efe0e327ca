"""numpy model of the direct LM step of the pose graphs' large path (include/mvslam_hip.h
mvs_ctx_set_pose_graph_solver), on top of posegraph_model's residuals and LM rule:

    A = H + lambda I inside its block envelope;  A_ii = C_i C_i^T;  A~_ij = C_i^-1 A_ij C_j^-T, A~_ii = I;
    A~ = L L^T in the skyline;  L y = -C^-1 g;  L^T z = y;  delta_i = C_i^-T z_i.

A float64 restatement: the same operations block by block, not the same bits (numpy has no fused multiply-add).  A pivot that
is not finite and positive, of a diagonal block or of the skyline, raises numpy.linalg.LinAlgError, which optimize_direct
treats as posegraph_model.optimize treats it under solver="exact".

There is no fixture of its own: a chain whose scale drifts by a factor r has a scaled matrix whose condition number grows as
1 / r^2 (the lever arm of an early rotation over the tail), so "the unscaled factorisation fails, the scaled one succeeds and
the run converges" holds for no size and ratio."""
import numpy as np

import pg_marginals_model as pgm
import posegraph_model as pm


def _chol6(S):
    """C and C^-1 of a 6 x 6 block by chol_packed's statements; LinAlgError on a pivot"""
    L, _ = pgm._chol6(S)                      # 1 / l_jj on the diagonal
    C = L.copy()
    C[np.diag_indices(6)] = 1.0 / np.diag(L)
    return C, np.linalg.inv(C)


def scaled_system(A, b, first):
    """(A~ dense with everything outside the envelope dropped, b~, Cinv [N, 6, 6]) of A x = b"""
    N = len(first)
    Cinv = np.zeros((N, 6, 6))
    for i in range(N):
        Cinv[i] = _chol6(A[6 * i:6 * i + 6, 6 * i:6 * i + 6])[1]
    As, bs = np.zeros_like(A), np.zeros_like(b)
    for i in range(N):
        bs[6 * i:6 * i + 6] = Cinv[i] @ b[6 * i:6 * i + 6]
        for j in range(int(first[i]), i):
            blk = Cinv[i] @ A[6 * i:6 * i + 6, 6 * j:6 * j + 6] @ Cinv[j].T
            As[6 * i:6 * i + 6, 6 * j:6 * j + 6] = blk
            As[6 * j:6 * j + 6, 6 * i:6 * i + 6] = blk.T
        As[6 * i:6 * i + 6, 6 * i:6 * i + 6] = np.eye(6)
    return As, bs, Cinv


def skyline_solve(rows, first, b):
    """L y = b, then L^T z = y with the rows in descending order, on pgm.skyline_factor's rows (a diagonal block holds
    1 / l_jj on its diagonal)"""
    N = len(first)
    y = np.array(b, dtype=np.float64).reshape(N, 6)

    def diag(i):
        L = rows[i][i - int(first[i])].copy()
        L[np.diag_indices(6)] = 1.0 / np.diag(L)
        return np.tril(L)
    for i in range(N):
        f = int(first[i])
        t = y[i].copy()
        for c in range(f, i):
            t = t - rows[i][c - f] @ y[c]
        y[i] = np.linalg.solve(diag(i), t)
    for i in range(N - 1, -1, -1):
        f = int(first[i])
        y[i] = np.linalg.solve(diag(i).T, y[i])
        for c in range(f, i):
            y[c] = y[c] - rows[i][c - f].T @ y[i]
    return y.reshape(-1)


def solve(A, b, first, info=None):
    """x of A x = b by the scaled skyline factorisation; raises LinAlgError on a pivot.  info (a dict) receives min_pivot."""
    As, bs, Cinv = scaled_system(A, b, first)
    rows, min_pivot = pgm.skyline_factor(As, first)
    if info is not None:
        info["min_pivot"] = min(info.get("min_pivot", np.inf), min_pivot)
    z = skyline_solve(rows, first, bs).reshape(-1, 6)
    return np.einsum("nji,nj->ni", Cinv, z).reshape(-1)


def system(g, poses=None, lam=None, anchor_sigma=pm.ANCHOR_SIGMA):
    """(H + lam I, -J^T r) of the contract at `poses` (None: the initial values; lam None: lambda_initial)"""
    X = np.asarray(g["node_pose"] if poses is None else poses, dtype=np.float64).reshape(-1, 12)
    wa = np.repeat(1.0 / np.asarray(anchor_sigma, dtype=np.float64), 3)
    r, J = pm._residuals(g, pm.whitening(g["edge_cov"]), wa, X, True)
    lam = pm.LM_DEFAULT["lambda_initial"] if lam is None else lam
    return J.T @ J + lam * np.eye(J.shape[1]), -(J.T @ r)


def optimize_direct(g, lm=None, anchor_sigma=pm.ANCHOR_SIGMA):
    """posegraph_model.optimize's LM rule with the scaled skyline solve as the linear solver; the same record, cg_iterations
    0, and `min_pivot` (the smallest over the factorisations that completed)"""
    lm = dict(pm.LM_DEFAULT, **(lm or {}))
    poses = np.array(g["node_pose"], dtype=np.float64).reshape(-1, 12)
    N = poses.shape[0]
    fail = dict(ok=0, iterations=0, cg_iterations=0, rejected_steps=0, error_initial=0.0, error=0.0, poses=None,
                exit="failed", trace=[], min_pivot=0.0)
    if not pm.connected(g):
        return fail
    try:
        W = pm.whitening(g["edge_cov"])
    except np.linalg.LinAlgError:
        return fail
    wa = np.repeat(1.0 / np.asarray(anchor_sigma, dtype=np.float64), 3)
    first, _, _ = pgm.graph_envelope(g)

    def cost(P):
        with np.errstate(over="ignore", invalid="ignore"):
            return float(np.sum(pm._residuals(g, W, wa, P, False) ** 2))
    cur = cost0 = cost(poses)
    lam, it, rejected = lm["lambda_initial"], 0, 0
    if not np.isfinite(cur):
        return fail
    trace, why, info = [], "max_iterations", {}
    while it < lm["max_iterations"]:
        r, J = pm._residuals(g, W, wa, poses, True)
        A = J.T @ J + lam * np.eye(6 * N)
        solved, cand, accepted = True, 0.0, False
        try:
            with np.errstate(all="ignore"):
                dx = solve(A, -(J.T @ r), first, info)
        except np.linalg.LinAlgError:
            solved = False
        if solved:
            new = np.array([pm.retract(poses[i], dx[6 * i:6 * i + 6]) for i in range(N)])
            cand = cost(new)
            accepted = cand <= cur
        it += 1
        trace.append(dict(cur=cur, cand=cand, solved=solved, accepted=accepted, lam=lam, cg=0, cg_status=None))
        if accepted:
            poses = new
            dec = 0.5 * (cur - cand)
            done = dec <= lm["abs_tol"] or dec <= lm["rel_tol"] * (0.5 * cur)
            cur = cand
            lam = lam / lm["lambda_factor"]
            if done:
                why = "converged"
                break
        else:
            rejected += 1
            inc = 0.5 * (cand - cur)
            if solved and (inc <= lm["abs_tol"] or inc <= lm["rel_tol"] * (0.5 * cur)):
                why = "stalled"
                break
            lam = lam * lm["lambda_factor"]
            if lam > lm["lambda_upper"]:
                why = "lambda_upper"
                break
    return dict(ok=1, iterations=it, cg_iterations=0, rejected_steps=rejected, error_initial=0.5 * cost0, error=0.5 * cur,
                poses=poses, exit=why, trace=trace, min_pivot=float(info.get("min_pivot", 0.0)))
