"""numpy model of the Sim(3) pose-graph contract (include/mvslam_hip.h mvs_sim3_graph_optimize).

A node is X = (R, t, s), 13 numbers, x_w = s R x + t.  An edge (src, dst, Z = (Rz, tz, sz), S 7 x 7) measures
Xs^-1 Xd = (Rs^T Rd, Rs^T (td - ts) / ss, sd / ss); with q = Rs^T (td - ts) / ss

    cost = 1/2 [ |e_anchor|^2_Sa + sum_k |e_k|^2_Sk ],   e_k = ( Log(Rz^T Rs^T Rd),  Rz^T (q - tz),  log sd - log ss - log sz ),

tangent order (rotation, translation, log-scale), right perturbation R <- R Exp(dw), t <- t + s R dv, s <- s exp(ds).  The
anchor is posegraph_model's pose prior plus log s - log s0.  The Levenberg-Marquardt rule is posegraph_model.optimize's,
restated here with 7 unknowns per node; `solver="pcg"` replaces the exact solve by the block-Jacobi (7 x 7) preconditioned
conjugate gradient the device's large path runs, default budget 7 N.

It also holds `lift`, the rule by which mvs_seq_optimize_pose_graph_sim3 turns an SE(3) graph into a Sim(3) one, and the
fixtures the host and the GPU tests share."""
import numpy as np

import posegraph_model as pm
from posegraph_model import hat, so3_exp, so3_jrinv, so3_log

LM_DEFAULT = pm.LM_DEFAULT
ANCHOR_SIGMA = (1e-4, 1e-4, 1e-4)
CG_REL_TOL = 1e-10


def split(p):
    p = np.asarray(p, dtype=np.float64).reshape(13)
    return p[:9].reshape(3, 3), p[9:12], float(p[12])


def join(R, t, s):
    return np.concatenate([np.asarray(R).reshape(9), np.asarray(t).reshape(3), [float(s)]])


def sim3(w, v, s=1.0):
    """(Exp(w), v, s)"""
    return join(so3_exp(w), np.asarray(v, dtype=np.float64), s)


def retract(p, dx):
    R, t, s = split(p)
    return join(R @ so3_exp(dx[:3]), t + s * (R @ dx[3:6]), s * np.exp(dx[6]))


def compose(a, b):
    Ra, ta, sa = split(a)
    Rb, tb, sb = split(b)
    return join(Ra @ Rb, ta + sa * (Ra @ tb), sa * sb)


def between(a, b):
    """a^-1 b: what an edge (a -> b) measures"""
    Ra, ta, sa = split(a)
    Rb, tb, sb = split(b)
    return join(Ra.T @ Rb, Ra.T @ (tb - ta) / sa, sb / sa)


def edge_error(Z, Ps, Pd, jac=False):
    """unwhitened error of one edge and, when asked, d e / d src and d e / d dst (7 x 7 each)"""
    Rz, tz, sz = split(Z)
    Rs, ts, ss = split(Ps)
    Rd, td, sd = split(Pd)
    Rsd = Rs.T @ Rd
    E = Rz.T @ Rsd
    ew = so3_log(E)
    q = Rs.T @ (td - ts) / ss
    e = np.concatenate([ew, Rz.T @ (q - tz), [(np.log(sd) - np.log(ss)) - np.log(sz)]])
    if not jac:
        return e
    Jri = so3_jrinv(ew)
    Js, Jd = np.zeros((7, 7)), np.zeros((7, 7))
    Js[:3, :3] = -Jri @ Rsd.T
    Js[3:6, :3] = Rz.T @ hat(q)
    Js[3:6, 3:6] = -Rz.T
    Js[3:6, 6] = -(Rz.T @ q)
    Js[6, 6] = -1.0
    Jd[:3, :3] = Jri
    Jd[3:6, 3:6] = (sd / ss) * E
    Jd[6, 6] = 1.0
    return e, Js, Jd


def prior_error(P0, P, jac=False):
    R0, t0, s0 = split(P0)
    R, t, s = split(P)
    Re = R0.T @ R
    ew = so3_log(Re)
    e = np.concatenate([ew, R0.T @ (t - t0), [np.log(s) - np.log(s0)]])
    if not jac:
        return e
    J = np.zeros((7, 7))
    J[:3, :3] = so3_jrinv(ew)
    J[3:6, 3:6] = s * Re
    J[6, 6] = 1.0
    return e, J


def chol7_ok(cov):
    """the device's test of one covariance (chol_packed<7> on the lower triangle): every pivot finite and > 0"""
    S = np.tril(np.asarray(cov, dtype=np.float64).reshape(7, 7))
    S = S + np.tril(S, -1).T
    L = np.zeros((7, 7))
    for j in range(7):
        d = S[j, j] - float(L[j, :j] @ L[j, :j])
        if not (d > 0.0 and np.isfinite(d)):
            return False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 7):
            L[i, j] = (S[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    return True


def whitening(cov):
    """W = L^-1 of cov = L L^T per edge, from the lower triangle; raises numpy.linalg.LinAlgError if one is not positive
    definite"""
    out = []
    for c in np.asarray(cov, dtype=np.float64).reshape(-1, 7, 7):
        if not chol7_ok(c):
            raise np.linalg.LinAlgError("covariance not positive definite")
        S = np.tril(c) + np.tril(c, -1).T
        out.append(np.linalg.inv(np.linalg.cholesky(S)))
    return np.array(out).reshape(-1, 7, 7)


def connected(g):
    return pm.connected(dict(node_pose=g["node_sim3"], edge_src=g["edge_src"], edge_dst=g["edge_dst"], anchor=g.get("anchor", 0)))


def _residuals(g, W, wa, nodes, jac):
    N, E, a = nodes.shape[0], len(g["edge_src"]), int(g.get("anchor", 0))
    r = np.zeros(7 * (E + 1))
    J = np.zeros((7 * (E + 1), 7 * N)) if jac else None
    for k in range(E):
        s, d = int(g["edge_src"][k]), int(g["edge_dst"][k])
        if jac:
            e, Js, Jd = edge_error(g["edge_sim3"][k], nodes[s], nodes[d], True)
            J[7 * k:7 * k + 7, 7 * s:7 * s + 7] = W[k] @ Js
            J[7 * k:7 * k + 7, 7 * d:7 * d + 7] = W[k] @ Jd
        else:
            e = edge_error(g["edge_sim3"][k], nodes[s], nodes[d])
        r[7 * k:7 * k + 7] = W[k] @ e
    if jac:
        e, Ja = prior_error(g["node_sim3"][a], nodes[a], True)
        J[7 * E:, 7 * a:7 * a + 7] = wa[:, None] * Ja
    else:
        e = prior_error(g["node_sim3"][a], nodes[a])
    r[7 * E:] = wa * e
    return (r, J) if jac else r


def pcg(H, b, rel_tol, max_iterations):
    """block-Jacobi (7 x 7 diagonal blocks) preconditioned CG of H x = b from x = 0: posegraph_model.pcg's recursion and
    stopping rules.  Returns (x, iterations, status): 1 converged, 0 out of iterations, 2 broke down."""
    n = H.shape[0]
    try:
        Mi = np.array([np.linalg.inv(H[i:i + 7, i:i + 7]) for i in range(0, n, 7)])
        for i in range(0, n, 7):
            np.linalg.cholesky(H[i:i + 7, i:i + 7])
    except np.linalg.LinAlgError:
        return np.zeros(n), 0, 2
    prec = lambda v: np.einsum("nij,nj->ni", Mi, v.reshape(-1, 7)).reshape(-1)
    x, r = np.zeros(n), b.copy()
    z = prec(r)
    p = z.copy()
    rz, gn = float(r @ z), np.sqrt(float(b @ b))
    if gn == 0.0:
        return x, 0, 1
    for it in range(1, max_iterations + 1):
        q = H @ p
        pq = float(p @ q)
        if not (pq > 0.0 and np.isfinite(pq)):
            return x, it - 1, 2
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = prec(r)
        rzn, rn = float(r @ z), np.sqrt(float(r @ r))
        if rn <= rel_tol * gn:
            return x, it, 1
        if not rzn > 0.0:
            return x, it, 2
        p = z + (rzn / rz) * p
        rz = rzn
    return x, max_iterations, 0 if np.sqrt(float(r @ r)) < gn else 2


def optimize(g, lm=None, anchor_sigma=ANCHOR_SIGMA, solver="exact", cg_rel_tol=CG_REL_TOL, cg_max_iterations=0):
    """the contract, in numpy.  Returns dict(ok, iterations, cg_iterations, rejected_steps, error_initial, error, nodes) and,
    for a run that started, `exit` and `trace` as posegraph_model.optimize (decision_margin reads the trace)."""
    lm = dict(LM_DEFAULT, **(lm or {}))
    nodes = np.array(g["node_sim3"], dtype=np.float64).reshape(-1, 13)
    N = nodes.shape[0]
    fail = dict(ok=0, iterations=0, cg_iterations=0, rejected_steps=0, error_initial=0.0, error=0.0, nodes=None,
                exit="failed", trace=[])
    if not connected(g):
        return fail
    try:
        W = whitening(g["edge_cov"])
    except np.linalg.LinAlgError:
        return fail
    wa = np.repeat(1.0 / np.asarray(anchor_sigma, dtype=np.float64), [3, 3, 1])
    cg_max = cg_max_iterations or 7 * N

    def cost(P):
        with np.errstate(over="ignore", invalid="ignore"):
            return float(np.sum(_residuals(g, W, wa, P, False) ** 2))
    cur = cost0 = cost(nodes)
    lam, it, rejected, cg_total = lm["lambda_initial"], 0, 0, 0
    if not np.isfinite(cur):
        return fail
    trace, why = [], "max_iterations"
    while it < lm["max_iterations"]:
        r, J = _residuals(g, W, wa, nodes, True)
        H = J.T @ J + lam * np.eye(7 * N)
        b = -(J.T @ r)
        solved, cand, n_cg, status = True, 0.0, 0, None
        if solver == "exact":
            try:
                L = np.linalg.cholesky(H)
                dx = np.linalg.solve(L.T, np.linalg.solve(L, b))
            except np.linalg.LinAlgError:
                solved = False
        else:
            dx, n_cg, status = pcg(H, b, cg_rel_tol, cg_max)
            cg_total += n_cg
            solved = status != 2
        accepted = False
        if solved:
            with np.errstate(over="ignore", invalid="ignore"):
                new = np.array([retract(nodes[i], dx[7 * i:7 * i + 7]) for i in range(N)])
            cand = cost(new)
            accepted = cand <= cur
        it += 1
        trace.append(dict(cur=cur, cand=cand, solved=solved, accepted=accepted, lam=lam, cg=n_cg, cg_status=status))
        if accepted:
            nodes = new
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
                error=0.5 * cur, nodes=nodes, exit=why, trace=trace)


decision_margin = pm.decision_margin


def pose_distance(A, B):
    """posegraph_model.pose_distance extended by the scale: the largest rotation angle of R1^T R2, the largest |t1 - t2| and
    the largest |log s1 - log s2| over the nodes of two tables"""
    A, B = np.asarray(A).reshape(-1, 13), np.asarray(B).reshape(-1, 13)
    rot, trans = pm.pose_distance(A[:, :12], B[:, :12])
    return rot, trans, float(np.abs(np.log(A[:, 12]) - np.log(B[:, 12])).max())


def lift(graph6, scale_sigma):
    """mvs_seq_optimize_pose_graph_sim3's rule: node k -> (G_k, 1), edge e -> Z = (Rz, tz, 1) and
    S7 = blockdiag(S6, scale_sigma[kind_e] * scale_sigma[kind_e]) with zero cross terms; copies and that one multiply, so the
    bytes are the device's.  graph6: posegraph_model's keys plus edge_kind (0 measured, 1 fallback, 2 loop)."""
    node = np.asarray(graph6["node_pose"], dtype=np.float64).reshape(-1, 12)
    Z = np.asarray(graph6["edge_pose"], dtype=np.float64).reshape(-1, 12)
    cov = np.asarray(graph6["edge_cov"], dtype=np.float64).reshape(-1, 6, 6)
    kind = np.asarray(graph6["edge_kind"], dtype=np.int64).reshape(-1)
    sig = np.asarray(scale_sigma, dtype=np.float64).reshape(3)
    E = len(kind)
    c7 = np.zeros((E, 7, 7))
    c7[:, :6, :6] = cov
    c7[:, 6, 6] = sig[kind] * sig[kind]
    return dict(node_sim3=np.ascontiguousarray(np.hstack([node, np.ones((node.shape[0], 1))])),
                edge_src=np.ascontiguousarray(graph6["edge_src"], dtype=np.int32),
                edge_dst=np.ascontiguousarray(graph6["edge_dst"], dtype=np.int32),
                edge_sim3=np.ascontiguousarray(np.hstack([Z, np.ones((E, 1))])),
                edge_cov=np.ascontiguousarray(c7.reshape(E, 49)), anchor=int(graph6.get("anchor", 0)))


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def graph(node_sim3, edges, edge_sim3, edge_cov, anchor=0):
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return dict(node_sim3=np.ascontiguousarray(node_sim3, dtype=np.float64).reshape(-1, 13),
                edge_src=np.ascontiguousarray(e[:, 0]), edge_dst=np.ascontiguousarray(e[:, 1]),
                edge_sim3=np.ascontiguousarray(edge_sim3, dtype=np.float64).reshape(-1, 13),
                edge_cov=np.ascontiguousarray(edge_cov, dtype=np.float64).reshape(-1, 49), anchor=anchor)


def iso_cov(sigma2, n):
    return np.tile((np.eye(7) * sigma2).reshape(49), (n, 1))


def full_cov(rng, n, scale=1e-2):
    """A A^T + 1e-4 I with a seeded random A"""
    out = np.zeros((n, 49))
    for k in range(n):
        A = rng.normal(size=(7, 7)) * scale
        out[k] = (A @ A.T + 1e-4 * np.eye(7)).reshape(49)
    return out


def _noise(rng, sigma):
    return sim3(rng.normal(size=3) * sigma, rng.normal(size=3) * sigma, np.exp(rng.normal() * sigma))


def pair():
    """two nodes of scales 1 and 1.7, node 1 guessed 1.2 x too far and 1.3 x too large, one exact edge.  (graph, truth)"""
    truth = np.array([sim3([0, 0, 0], [0, 0, 0], 1.0), sim3([0.2, -0.1, 0.3], [1, 0.5, -0.2], 1.7)])
    guess = np.array([truth[0], sim3([0.2, -0.1, 0.3], [1.2, 0.6, -0.24], 1.7 * 1.3)])
    return graph(guess, [(0, 1)], [between(truth[0], truth[1])], iso_cov(0.01, 1)), truth


# the first eight seeds whose decisions in the model are at least 100 units of eps * cost from the rounding of the cost
# (decision_margin); tests/test_sim3_graph_host.py asserts DENSE_MARGIN of each
TRIANGLE_SEEDS = (2, 11, 20, 35, 36, 37, 43, 56)
DENSE_MARGIN = 50.0


def triangle(seed, sigma=0.01):
    """posegraph_model.triangle with inconsistent scales: three steps of (120 degrees about z, 1 along x, scale 1.1) composed
    on the right and measured with sigma noise, values by dead reckoning, and the loop closed by an identity edge of scale 1
    from the last node to the origin, which the three scale steps (1.1^3 = 1.331) contradict.  4 nodes, 4 edges."""
    rng = np.random.default_rng(3000 + seed)
    M = sim3([0, 0, 2.0 * np.pi / 3.0], [1, 0, 0], 1.1)
    guess, edges, Z = [sim3([0, 0, 0], [0, 0, 0])], [], []
    for i in range(3):
        meas = compose(M, _noise(rng, sigma))
        guess.append(compose(guess[-1], meas))
        edges.append((i, i + 1))
        Z.append(meas)
    edges.append((3, 0))
    Z.append(sim3([0, 0, 0], [0, 0, 0]))
    return graph(guess, edges, Z, iso_cov(sigma * sigma, 4))


def ring_truth(n):
    """posegraph_model.ring's poses with a scale that swings between 0.74 and 1.35 around the ring"""
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / n
        R = so3_exp([0, 0, a + np.pi / 2]) @ so3_exp([0.2 * np.sin(3 * a), 0.1 * np.cos(2 * a), 0.0])
        out.append(join(R, [3.0 * np.cos(a), 3.0 * np.sin(a), 0.3 * np.sin(2 * a)], np.exp(0.3 * np.sin(a + 1.0))))
    return np.array(out)


def ring(n, chords=(2,), seed=0, noise=0.01, guess_noise=0.05, full=True, extra_edges=()):
    """posegraph_model.ring over Sim(3): edges (i, i + 1) and (i, i + c) per chord length c, measurements with `noise` on all
    seven components, initial values off by `guess_noise` except node 0, full covariances A A^T + 1e-4 I when `full`"""
    rng = np.random.default_rng(4000 + 31 * n + seed)
    truth = ring_truth(n)
    edges = [(i, (i + 1) % n) for i in range(n)]
    for c in chords:
        edges += [(i, (i + c) % n) for i in range(n) if (i + c) % n != i]
    edges += list(extra_edges)
    Z = [compose(between(truth[s], truth[d]), _noise(rng, noise)) for s, d in edges]
    guess = np.array([truth[0]] + [retract(truth[i], rng.normal(size=7) * guess_noise) for i in range(1, n)])
    cov = full_cov(rng, len(edges)) if full else iso_cov(noise * noise, len(edges))
    return graph(guess, edges, Z, cov)


# seeds of the ring fixtures compared with the model, per size the first one whose decision_margin is >= 100 (at 8 also for
# the relabelled graph, at 17 also for the exact solve)
RING_SEED = {2: 5, 5: 4, 6: 2, 8: 6, 16: 0, 17: 0}


def dense_ring(n):
    return ring(n, chords=(2,) if n >= 4 else (), seed=RING_SEED[n])


def full_cov_graph():
    """6 nodes, 9 edges (ring + three chords), every covariance full"""
    g = ring(6, chords=(), seed=RING_SEED[6], extra_edges=[(0, 2), (1, 4), (3, 5)])
    assert len(g["edge_src"]) == 9
    return g


# seed and guess noise: Newton's last step must fall between the rounding of the cost and the tolerances; at the rings' 0.05
# none of 60 seeds does, at 0.02 the first one does
ALL_PAIRS_SEED, ALL_PAIRS_GUESS = 0, 0.02


def all_pairs16():
    """16 nodes, an edge for every ordered pair: 240 edges, every pair joined in both directions"""
    n = 16
    pairs = [(s, d) for s in range(n) for d in range(n) if s != d]
    return ring(n, chords=(), seed=ALL_PAIRS_SEED, guess_noise=ALL_PAIRS_GUESS, extra_edges=[p for p in pairs if p[1] != (p[0] + 1) % n])


PARALLEL_SEED, PARALLEL_GUESS = 0, 0.02   # chosen as ALL_PAIRS_SEED


def parallel16():
    """16 nodes, every ordered pair plus the ring and the chords of length 2 once more with fresh noise: 272 edges, so the dense
    path's strided loops over the edges take a second trip, and parallel edges join the same nodes in both directions"""
    n = 16
    pairs = [(s, d) for s in range(n) for d in range(n) if s != d]
    g = ring(n, chords=(2,), seed=PARALLEL_SEED, guess_noise=PARALLEL_GUESS, extra_edges=pairs)
    assert len(g["edge_src"]) == 272
    return g


def relabelled(g, perm):
    """the same graph with node i renamed perm[i]; the anchor follows its node"""
    perm = np.asarray(perm, dtype=np.int64)
    nodes = np.empty_like(g["node_sim3"])
    nodes[perm] = g["node_sim3"]
    return graph(nodes, np.stack([perm[g["edge_src"]], perm[g["edge_dst"]]], axis=1), g["edge_sim3"], g["edge_cov"],
                 anchor=int(perm[int(g.get("anchor", 0))]))


ANCHOR5_PERM = [(3 * i + 5) % 8 for i in range(8)]


def anchor5():
    """dense_ring(8) with node i renamed (3 i + 5) mod 8: the anchor is node 5"""
    return relabelled(dense_ring(8), ANCHOR5_PERM)


def star(spokes=70):
    """one hub (node 0, the anchor) with `spokes` spokes of scales 0.5 .. 2: a long CSR row, leaves with one edge"""
    rng = np.random.default_rng(177)
    truth = [sim3([0, 0, 0], [0, 0, 0], 1.0)]
    for i in range(spokes):
        a = 2.0 * np.pi * i / spokes
        truth.append(sim3([0.1 * np.sin(a), 0.2 * np.cos(a), a], [2.0 * np.cos(a), 2.0 * np.sin(a), 0.1 * i / spokes],
                          0.5 * 4.0 ** (i / (spokes - 1.0))))
    truth = np.array(truth)
    edges = [(0, i + 1) if i % 2 == 0 else (i + 1, 0) for i in range(spokes)]
    Z = [compose(between(truth[s], truth[d]), _noise(rng, 0.01)) for s, d in edges]
    guess = np.array([truth[0]] + [retract(truth[i], rng.normal(size=7) * 0.05) for i in range(1, spokes + 1)])
    return graph(guess, edges, Z, full_cov(rng, spokes))


DRIFT_N, DRIFT_SEED, DRIFT_STEP = 40, 0, (0.01, 0.01, 0.02)   # per-step perturbation of the chain: rotation, translation, log-scale


def drift_ring():
    """The scale-drift fixture: 40 nodes on posegraph_model.ring's circle whose scale grows by 2^(1/40) per node (a factor of
    1.97 from node 0 to node 39).  Edges: the odometry (i, i + 1), i < 39, and ONE loop edge (39, 0); every measurement is
    exactly Xs^-1 Xd of the truth and has an isotropic covariance, so the Sim(3) optimum is the truth with zero cost.
    Initial values: chained from node 0 (at the truth, the anchor) along the odometry, every step perturbed by DRIFT_STEP -- the
    scale of the chain random-walks away from the truth.  Returns (graph, truth, graph6): graph6 is the SE(3) graph a monocular
    back end would build from the same numbers, scales dropped: the same rotations and translations as initial values, and
    every edge's translation in world units of the drifted chain, s_src(chain) tz."""
    n = DRIFT_N
    rng = np.random.default_rng(5000 + DRIFT_SEED)
    base = pm.ring(n, chords=(), noise=0.0, guess_noise=0.0)["node_pose"]      # the circle, at the truth
    truth = np.array([join(base[i, :9], base[i, 9:], 2.0 ** (i / float(n))) for i in range(n)])
    edges = [(i, i + 1) for i in range(n - 1)] + [(n - 1, 0)]
    Z = np.array([between(truth[s], truth[d]) for s, d in edges])
    guess = [truth[0]]
    for i in range(n - 1):
        step = np.concatenate([rng.normal(size=3) * DRIFT_STEP[0], rng.normal(size=3) * DRIFT_STEP[1], [rng.normal() * DRIFT_STEP[2]]])
        guess.append(retract(compose(guess[-1], Z[i]), step))
    guess = np.array(guess)
    g = graph(guess, edges, Z, iso_cov(1e-4, n))
    Z6 = np.array([np.concatenate([Z[k, :9], guess[s, 12] * Z[k, 9:12]]) for k, (s, d) in enumerate(edges)])
    g6 = pm.graph(guess[:, :12], edges, Z6, pm.iso_cov(1e-4, n))
    return g, truth, g6


def disconnected():
    """triangle(0) without its last two edges: node 3 hangs on nothing"""
    g = triangle(0)
    return graph(g["node_sim3"], [(0, 1), (1, 2)], g["edge_sim3"][:2], g["edge_cov"][:2])


def indefinite(g, edge):
    g = dict(g, edge_cov=g["edge_cov"].copy())
    g["edge_cov"][edge] = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0]).reshape(49)
    return g


DENSE_FIXTURES = {"pair": lambda: pair()[0], "full_cov": full_cov_graph, "all_pairs16": all_pairs16, "parallel16": parallel16,
                  "anchor5": anchor5, "ring16": lambda: dense_ring(16), "ring5": lambda: dense_ring(5)}
# ring257: more nodes than a workgroup has threads, so the one-workgroup kernels of the conjugate gradient take a second trip
PCG_FIXTURES = {"ring17": lambda: dense_ring(17), "star70": star, "drift_ring40": lambda: drift_ring()[0],
                "ring257": lambda: ring(257, chords=(7, 40), seed=0)}
