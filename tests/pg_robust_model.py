"""numpy model of the pose graphs' robust edge losses (include/mvslam_hip.h
mvs_ctx_set_pose_graph_loss), on top of tests/posegraph_model.py, which it leaves as it is.

With s_k = |r_k|^2, the squared norm of edge k's whitened residual, and x = sqrt(s):

    cost = 1/2 [ |e_anchor|^2 + sum_{k < first_edge} s_k + sum_{k >= first_edge} rho2(s_k) ]

    NONE    rho2 = s                                   w = 1
    HUBER   rho2 = s if x <= k else (2 k) x - k k      w = 1 if x <= k else k / x
    CAUCHY  rho2 = (k k) log1p(s / (k k))              w = (k k) / (k k + s)

Iteratively reweighted least squares: a robustified edge enters the normal equations as sqrt(w) r, sqrt(w) A_src,
sqrt(w) A_dst; the LM rule of posegraph_model.optimize runs on the robust cost.  It also holds the fixtures the host and the
GPU tests share."""
import numpy as np

import posegraph_model as m

NONE, HUBER, CAUCHY = 0, 1, 2


def loss(s, kind, k):
    """(w, rho2) of one edge, in the contract's order of operations"""
    s = float(s)
    if kind == NONE:
        return 1.0, s
    x = float(np.sqrt(s))
    if kind == HUBER:
        if x <= k:
            return 1.0, s
        return k / x, (2.0 * k) * x - k * k
    k2 = k * k
    return k2 / (k2 + s), k2 * float(np.log1p(s / k2))


def _edge_terms(r, E, kind, k, first_edge):
    """s, w and rho2 of the E edges from the stacked whitened residuals r (6 (E + 1): the anchor's last)"""
    s = np.sum(r[:6 * E].reshape(E, 6) ** 2, axis=1)
    w, rho = np.ones(E), s.copy()
    for e in range(min(max(first_edge, 0), E), E):
        w[e], rho[e] = loss(s[e], kind, k)
    return s, w, rho


def edge_stats(g, poses=None, kind=NONE, k=1.0, first_edge=0):
    """(chi2, weight) of every edge at `poses` (None: the graph's node_pose): mvs_pose_graph_edge_stats"""
    P = np.asarray(g["node_pose"] if poses is None else poses, dtype=np.float64).reshape(-1, 12)
    E = len(g["edge_src"])
    r = m._residuals(g, m.whitening(g["edge_cov"]), np.zeros(6), P, False)
    s, w, _ = _edge_terms(r, E, kind, k, first_edge)
    return s, w


def cost(g, poses, kind=NONE, k=1.0, first_edge=0, anchor_sigma=m.ANCHOR_SIGMA):
    """twice the robust error at `poses`"""
    wa = np.repeat(1.0 / np.asarray(anchor_sigma, dtype=np.float64), 3)
    E = len(g["edge_src"])
    r = m._residuals(g, m.whitening(g["edge_cov"]), wa, np.asarray(poses, dtype=np.float64).reshape(-1, 12), False)
    return float(np.sum(_edge_terms(r, E, kind, k, first_edge)[2]) + np.sum(r[6 * E:] ** 2))


def gradient(g, poses, kind=NONE, k=1.0, first_edge=0, anchor_sigma=m.ANCHOR_SIGMA):
    """gradient of the robust error (half the cost) at `poses`: J^T diag(w) r, which is what the reweighted normal equations
    have on their right-hand side"""
    wa = np.repeat(1.0 / np.asarray(anchor_sigma, dtype=np.float64), 3)
    E = len(g["edge_src"])
    r, J = m._residuals(g, m.whitening(g["edge_cov"]), wa, np.asarray(poses, dtype=np.float64).reshape(-1, 12), True)
    w = np.concatenate([np.repeat(_edge_terms(r, E, kind, k, first_edge)[1], 6), np.ones(6)])
    return J.T @ (w * r)


def optimize(g, loss=NONE, k=1.0, first_edge=0, lm=None, anchor_sigma=m.ANCHOR_SIGMA, solver="exact", cg_rel_tol=m.CG_REL_TOL,
             cg_max_iterations=0, h_apply="dense"):
    """posegraph_model.optimize's LM loop, statement for statement, on the robust cost and the reweighted linearisation;
    the same record comes back, `trace` included (posegraph_model.decision_margin reads it)."""
    kind = loss
    lm = dict(m.LM_DEFAULT, **(lm or {}))
    poses = np.array(g["node_pose"], dtype=np.float64).reshape(-1, 12)
    N, E = poses.shape[0], len(g["edge_src"])
    fail = dict(ok=0, iterations=0, cg_iterations=0, rejected_steps=0, error_initial=0.0, error=0.0, poses=None,
                exit="failed", trace=[])
    if not m.connected(g):
        return fail
    try:
        W = m.whitening(g["edge_cov"])
    except np.linalg.LinAlgError:
        return fail
    wa = np.repeat(1.0 / np.asarray(anchor_sigma, dtype=np.float64), 3)
    cg_max = cg_max_iterations or 6 * N

    def cost_at(P):
        with np.errstate(over="ignore", invalid="ignore"):
            r = m._residuals(g, W, wa, P, False)
            return float(np.sum(_edge_terms(r, E, kind, k, first_edge)[2]) + np.sum(r[6 * E:] ** 2))
    cur = cost0 = cost_at(poses)
    lam, it, rejected, cg_total = lm["lambda_initial"], 0, 0, 0
    if not np.isfinite(cur):
        return fail
    E6, a6 = 6 * E, 6 * int(g.get("anchor", 0))
    trace, why = [], "max_iterations"
    while it < lm["max_iterations"]:
        r, J = m._residuals(g, W, wa, poses, True)
        sw = np.concatenate([np.repeat(np.sqrt(_edge_terms(r, E, kind, k, first_edge)[1]), 6), np.ones(6)])
        r, J = r * sw, J * sw[:, None]
        H = J.T @ J + lam * np.eye(6 * N)
        b = -(J.T @ r)
        solved, cand, n_cg, status = True, 0.0, 0, None
        if solver == "exact":
            try:
                L = np.linalg.cholesky(H)
                dx = np.linalg.solve(L.T, np.linalg.solve(L, b))
            except np.linalg.LinAlgError:
                solved = False
        else:
            apply = None
            if h_apply == "edges":
                Je, Ha, l_ = J[:E6], J[E6:, a6:a6 + 6].T @ J[E6:, a6:a6 + 6], lam

                def apply(p):
                    q = Je.T @ (Je @ p)
                    q[a6:a6 + 6] += Ha @ p[a6:a6 + 6]
                    return q + l_ * p
            dx, n_cg, status = m.pcg(H, b, cg_rel_tol, cg_max, apply)
            cg_total += n_cg
            solved = status != 2
        accepted = False
        if solved:
            new = np.array([m.retract(poses[i], dx[6 * i:6 * i + 6]) for i in range(N)])
            cand = cost_at(new)
            accepted = cand <= cur
        it += 1
        trace.append(dict(cur=cur, cand=cand, solved=solved, accepted=accepted, lam=lam, cg=n_cg, cg_status=status))
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
    return dict(ok=1, iterations=it, cg_iterations=cg_total, rejected_steps=rejected, error_initial=0.5 * cost0,
                error=0.5 * cur, poses=poses, exit=why, trace=trace)


# ---- fixtures ---------------------------------------------------------------------------------------------------------
GROSS = m.se3([0.0, 0.3, 0.8], [1.0, -0.5, 0.3])   # what the two wrong loop edges are off by


def outlier_ring(n, full=False):
    """ring(n) with chords of length 2 (2 n clean edges) and two more edges, (1, n // 2) and (3, n - 2), whose measurements
    are composed on the right with GROSS: two accepted wrong revisits.  The clean edges come first: first_edge = 2 n."""
    g = m.ring(n, chords=(2,), full=full, extra_edges=[(1, n // 2), (3, n - 2)])
    E = len(g["edge_src"])
    assert E == 2 * n + 2
    for e in (E - 2, E - 1):
        g["edge_pose"][e] = m.compose(g["edge_pose"][e], GROSS)
    return g


def without_outliers(g):
    """the same graph (measurements, covariances, initial values) without its last two edges"""
    E = len(g["edge_src"]) - 2
    return m.graph(g["node_pose"], np.stack([g["edge_src"], g["edge_dst"]], axis=1)[:E], g["edge_pose"][:E], g["edge_cov"][:E],
                   anchor=int(g.get("anchor", 0)))


HUBER_K, CAUCHY_K, CAUCHY_ALL_K = 1.345, 1.0, 3.0

# name -> (graph, keywords of optimize without the solver).  "n12" runs on the dense path, the others on the large one.
FIXTURES = {
    "n12_cauchy": (lambda: outlier_ring(12), dict(loss=CAUCHY, k=CAUCHY_K, first_edge=24)),
    "n12_huber": (lambda: outlier_ring(12), dict(loss=HUBER, k=HUBER_K, first_edge=24)),
    "n12_full_cauchy": (lambda: outlier_ring(12, full=True), dict(loss=CAUCHY, k=CAUCHY_K, first_edge=24)),
    "n12_cauchy3_all": (lambda: outlier_ring(12), dict(loss=CAUCHY, k=CAUCHY_ALL_K, first_edge=0)),
    "n17_cauchy": (lambda: outlier_ring(17), dict(loss=CAUCHY, k=CAUCHY_K, first_edge=34)),
    "n17_huber": (lambda: outlier_ring(17), dict(loss=HUBER, k=HUBER_K, first_edge=34)),
    "n20_cauchy": (lambda: outlier_ring(20), dict(loss=CAUCHY, k=CAUCHY_K, first_edge=40)),
    "n20_huber": (lambda: outlier_ring(20), dict(loss=HUBER, k=HUBER_K, first_edge=40)),
    "n20_cauchy3_all": (lambda: outlier_ring(20), dict(loss=CAUCHY, k=CAUCHY_ALL_K, first_edge=0)),
}
MARGIN = 1e3   # posegraph_model.decision_margin a fixture needs before its iterations / rejected_steps are asserted


def dense(name):
    return name.startswith("n12")


def model_solver(name, direct=False):
    """the model's linear solver that stands for the device's path: exact for the dense path and the direct solver, PCG else"""
    return "exact" if dense(name) or direct else "pcg"
