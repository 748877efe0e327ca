"""numpy models of the sparse bundle adjustment's robust losses (include/mvslam_hip.h
mvs_ctx_set_ba_loss), on tests/ba_sparse_model.py's generator and test_ba_window's block model, which stay as they are.

Observation o has the whitened residual r_o (2), s_o = |r_o|^2, x = sqrt(s_o):

    cost = 1/2 [ pose priors + point priors + sum_o rho2(s_o) ]

    NONE    rho2 = s                                   w = 1
    HUBER   rho2 = s if x <= k else (2 k) x - k k      w = 1 if x <= k else k / x
    CAUCHY  rho2 = (k k) log1p(s / (k k))              w = (k k) / (k k + s)

(A) solve_irls: iteratively reweighted least squares.  Observation o enters every sum of the block normal equations with
    sqrt(w) r, sqrt(w) Jc, sqrt(w) Jp, i.e. with the information matrix w W_o; the LM rule is capi_ba.hip's bas_solve, statement
    for statement, on the robust cost.  Covariances: the blocks of the inverse of the reweighted system at the estimate.
(B) solve_scipy: scipy's least_squares on the RESCALED residuals r_o sqrt(rho2(s_o) / s_o), whose squared norms are rho2, with
    their exact Jacobian (g I + ((w s - rho2) / (s^2 g)) r r^T) J_o, g = sqrt(rho2 / s) -- a Gauss-Newton method on other
    residuals, nothing is reweighted.  (scipy's own loss= acts per scalar residual, not per 2-vector: it is not this cost.)
    Its covariances are (A)'s formula evaluated at ITS minimiser: the contract defines them by the reweighted linearisation.

full=True (tests/ba_fullcov_model.py's problems): pb["cov"] and pb["pcov"] hold full covariances, and every observation is
whitened by the Cholesky factor of its own information matrix W = L L^T, r_w = L^T r, s = r^T W r (_obs_lin_full); with the
default every function computes what it did.

It also holds the outlier fixtures the host and the GPU tests share, each computed once."""
import functools
import os

import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation as Rot

import ba_sparse_model as bm
import test_ba_window as tw

NONE, HUBER, CAUCHY = 0, 1, 2
NAMES = {NONE: "none", HUBER: "huber", CAUCHY: "cauchy"}
# on the norm x of the whitened 2-vector.  Huber: about the 95 % quantile of x for a clean observation (2.448), so that nearly
# every clean observation lies in the quadratic zone.  (At the scalar constant 1.345, 40 % of the clean observations lie in
# the linear zone, where the loss has no curvature along the residual; the points that two close frames hold weakly then
# made IRLS creep: at F = 24 the model still had a Newton step of 1.2e-6 in the points after 1000 iterations.)  Cauchy: the
# usual 95 %-efficiency constant.
HUBER_K, CAUCHY_K = 2.5, 2.3849
K_OF = {NONE: 1.0, HUBER: HUBER_K, CAUCHY: CAUCHY_K}
# bas_solve's rule with tolerances of zero: IRLS converges linearly, so the default stop (a decrease of 1e-12 of the cost)
# would leave the estimate short of the minimum by more than the models differ; with zero the loop ends where rounding
# decides the accept / reject, by lambda passing lambda_upper; 16 .. 130 iterations on the fixtures, 1000 is the cap
LM = dict(max_iterations=1000, lambda_initial=1e-5, lambda_factor=10.0, lambda_upper=1e5, rel_tol=0.0, abs_tol=0.0)


def loss(s, kind, k):
    """(w, rho2) of the observations with the squared norms s, in the contract's order of operations"""
    s = np.asarray(s, dtype=np.float64)
    if kind == NONE:
        return np.ones_like(s), s.copy()
    if kind == HUBER:
        x = np.sqrt(s)
        inside = x <= k
        xs = np.where(inside, 1.0, x)
        return np.where(inside, 1.0, k / xs), np.where(inside, s, (2.0 * k) * x - k * k)
    k2 = k * k
    return k2 / (k2 + s), k2 * np.log1p(s / k2)


# ---- the generator's problems with planted outliers -------------------------------------------------------------------
def plant_outliers(pb, seed, frac=0.05, lo=30.0, hi=100.0, min_track=4):
    """about frac of the observations displaced by lo .. hi px in a random direction: one observation each of a fixed subset of
    the tracks of at least min_track frames whose point has a prior.  (A two-frame track cannot tell which of its observations
    is wrong, and a slide along the epipolar line is absorbed by its point: no estimator separates those.  Without a prior a
    point of four observations still follows its outlier far enough under Huber, whose pull does not fade, that IRLS and the
    scipy model stopped at estimates 0.6 apart in such points after 300 iterations, and a clean observation reached x = 45.)
    Returns the new dict and the planted mask in CSR order."""
    rng = np.random.default_rng(seed)
    F, m = len(pb["poses"]), len(pb["Xg"])
    valid = np.stack(pb["valid"]).astype(bool)
    n_obs = int(valid.sum())
    long_tracks = np.flatnonzero((valid.sum(0) >= min_track) & pb["has_prior"])
    n_plant = min(int(round(frac * n_obs)), len(long_tracks))
    chosen = rng.choice(long_tracks, n_plant, replace=False)
    obs = [o.copy() for o in pb["obs"]]
    planted = np.zeros((F, m), bool)
    for i in chosen:
        f = int(rng.choice(np.flatnonzero(valid[:, i])))
        ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(lo, hi)
        obs[f][i] += mag * np.array([np.cos(ang), np.sin(ang)])
        planted[f, i] = True
    out = dict(pb, obs=obs)
    out["csr"] = bm.to_csr(out)
    return out, csr_order(out, planted)


def csr_order(pb, per_frame):
    """a [F, m] array over (frame, point) as the vector over the observations in CSR order (by point, frames ascending)"""
    valid = np.stack(pb["valid"]).astype(bool)
    return np.asarray(per_frame).T[valid.T]


SEED = {9: 9, 24: 24}   # test_ba_sparse.WIDE_SEED's


@functools.lru_cache(maxsize=None)
def outlier_problem(F):
    """test_ba_sparse._wide(F)'s problem (m = 300, tracks of 2 .. 5 frames, a point with one observation, a frame held by its
    prior alone, at F = 24 a track over frames 0 and F - 1) with planted outliers"""
    pb = bm.sparse_problem(SEED[F], F, 300, lone_frame=F // 2, long_track=F == 24)
    return plant_outliers(pb, 1000 + F)


# ---- linearisation ---------------------------------------------------------------------------------------------------
def _obs_lin(pb, Rs, ts, P, f):
    """frame f's observations: point indices, whitened residuals (n, 2), Jc (n, 2, 6), Jp (n, 2, 3) -- test_ba_window.
    model_blocks' statements"""
    K, sig = pb["K"], pb["sig"]
    v = np.flatnonzero(pb["valid"][f])
    q = (P[v] - ts[f]) @ Rs[f]
    iz = 1.0 / q[:, 2]
    x, y = q[:, 0] * iz, q[:, 1] * iz
    r = np.stack([K[0, 0] * x + K[0, 1] * y + K[0, 2], K[1, 1] * y + K[1, 2]], 1) - pb["obs"][f][v]
    Aq = np.zeros((len(q), 2, 3))
    Aq[:, 0, 0], Aq[:, 0, 1], Aq[:, 0, 2] = K[0, 0] * iz, K[0, 1] * iz, -(K[0, 0] * x + K[0, 1] * y) * iz
    Aq[:, 1, 1], Aq[:, 1, 2] = K[1, 1] * iz, -K[1, 1] * y * iz
    Sq = np.zeros((len(q), 3, 3))
    Sq[:, 0, 1], Sq[:, 0, 2], Sq[:, 1, 0] = -q[:, 2], q[:, 1], q[:, 2]
    Sq[:, 1, 2], Sq[:, 2, 0], Sq[:, 2, 1] = -q[:, 0], -q[:, 1], q[:, 0]
    return v, r / sig, np.concatenate([Aq @ Sq, -Aq], axis=2) / sig, (Aq @ Rs[f].T) / sig


def _obs_lin_full(pb, Rs, ts, P, f, Lo):
    """_obs_lin for full covariances: every observation is whitened by the Cholesky factor L of its own information matrix
    W = L L^T (Lo: test_ba_window.full_whiteners), r_w = L^T r, so that s = |r_w|^2 = r^T W r, and the Jacobians likewise"""
    v, r, Jc, Jp = _obs_lin(dict(pb, sig=1.0), Rs, ts, P, f)
    LT = Lo[f][v].transpose(0, 2, 1)
    return v, np.einsum("nij,nj->ni", LT, r), LT @ Jc, LT @ Jp


def _prior_only(pb):
    return dict(pb, valid=[np.zeros(len(pb["Xg"]), np.uint8)] * len(pb["poses"]))


def robust_blocks(pb, Rs, ts, P, kind, k, full=False):
    """test_ba_window.model_blocks under a loss: the robust error and the blocks of the REWEIGHTED normal equations.
    full: pb["cov"] and pb["pcov"] are full covariances (test_ba_window.model_blocks' `full`; _obs_lin_full)"""
    F = len(pb["poses"])
    cost, A, gc, D, gp, W = tw.model_blocks(_prior_only(pb), Rs, ts, P, full)   # the priors, never robustified
    cost = 2.0 * cost
    Lo = tw.full_whiteners(pb)[0] if full else None
    for f in range(F):
        v, r, Jc, Jp = _obs_lin_full(pb, Rs, ts, P, f, Lo) if full else _obs_lin(pb, Rs, ts, P, f)
        w, rho = loss(np.sum(r * r, axis=1), kind, k)
        A[f] += np.einsum("n,nia,nib->ab", w, Jc, Jc)
        gc[f] += np.einsum("n,nia,ni->a", w, Jc, r)
        D[v] += np.einsum("n,nia,nib->nab", w, Jp, Jp)
        gp[v] += np.einsum("n,nia,ni->na", w, Jp, r)
        W[f][v] = np.einsum("n,nia,nib->nab", w, Jc, Jp)
        cost += np.sum(rho)
    return 0.5 * cost, A, gc, D, gp, W


def robust_cost(pb, Rs, ts, P, kind, k, full=False):
    return robust_blocks(pb, Rs, ts, P, kind, k, full)[0]


def obs_stats(pb, Rs, ts, P, kind=NONE, k=1.0, full=False):
    """(chi2, weight) of every observation in CSR order at the given values: mvs_ba_sparse_obs_stats.  An observation whose
    point is not in front of its camera has the fixed residual (2 fx, 2 fx).  full: s = r^T W r with W the inverse of the
    symmetric part of the observation's own pb["cov"] entry (None: identity), no factorisation."""
    F, m = len(pb["poses"]), len(P)
    s = np.zeros((F, m))
    for f in range(F):
        with np.errstate(divide="ignore", invalid="ignore"):
            v, r, _, _ = _obs_lin(dict(pb, sig=1.0) if full else pb, Rs, ts, P, f)
        behind = ~(((P[v] - ts[f]) @ Rs[f])[:, 2] > 0.0)
        if full:
            r[behind] = 2.0 * pb["K"][0, 0]
            C = np.tile(np.eye(2), (len(v), 1, 1)) if pb["cov"][f] is None else np.asarray(pb["cov"][f], float)[v].reshape(-1, 2, 2)
            s[f, v] = np.einsum("ni,nij,nj->n", r, np.linalg.inv(0.5 * (C + C.transpose(0, 2, 1))), r)
            continue
        r[behind] = 2.0 * pb["K"][0, 0] / pb["sig"]
        s[f, v] = np.sum(r * r, axis=1)
    s = csr_order(pb, s)
    return s, loss(s, kind, k)[0]


def _guess(pb):
    F = len(pb["poses"])
    return (np.stack([pb["poses"][f][:9].reshape(3, 3) for f in range(F)]), np.stack([pb["poses"][f][9:] for f in range(F)]),
            pb["Xg"].copy())


def _reduce(F, A, D, W):
    Di = np.linalg.inv(D)
    Y = np.einsum("fnab,nbc->fnac", W, Di)
    S = -np.einsum("fnac,gndc->fagd", Y, W).reshape(6 * F, 6 * F)
    for f in range(F):
        S[6 * f:6 * f + 6, 6 * f:6 * f + 6] += A[f]
    return Di, Y, S


def reweighted_cov(pb, sol, kind, k, full=False):
    """pose_cov / point_cov of the reweighted linearisation at sol's values (test_ba_window.model_solve_blocks' statements)"""
    F, m = len(pb["poses"]), len(pb["Xg"])
    _, A, gc, D, gp, W = robust_blocks(pb, sol["R"], sol["t"], sol["points"], kind, k, full)
    Di, Y, S = _reduce(F, A, D, W)
    Si = np.linalg.inv(S)
    Yn = Y.transpose(1, 0, 2, 3).reshape(m, 6 * F, 3)
    return (np.stack([Si[6 * f:6 * f + 6, 6 * f:6 * f + 6] for f in range(F)]), Di + np.einsum("nac,ab,nbd->ncd", Yn, Si, Yn))


def newton_step(pb, sol, kind, k, full=False):
    """ba_sparse_model.newton_step on the weighted system: the largest entry of the step of the poses and of the points that
    the reweighted normal equations still ask for at sol, and the condition number of the reduced camera system"""
    F = len(pb["poses"])
    _, A, gc, D, gp, W = robust_blocks(pb, sol["R"], sol["t"], sol["points"], kind, k, full)
    Di, Y, S = _reduce(F, A, D, W)
    dc = np.linalg.solve(S, -(gc - np.einsum("fnac,nc->fa", Y, gp)).reshape(6 * F)).reshape(F, 6)
    dp = -np.einsum("nab,nb->na", Di, gp + np.einsum("fnab,fa->nb", W, dc))
    return np.abs(dc).max(), np.abs(dp).max(), np.linalg.cond(S)


# ---- (A) IRLS under bas_solve's LM rule --------------------------------------------------------------------------------
def solve_irls(pb, kind=NONE, k=1.0, lm=None, full=False):
    lm = dict(LM, **(lm or {}))
    F = len(pb["poses"])
    Rs, ts, P = _guess(pb)
    cur, A, gc, D, gp, W = robust_blocks(pb, Rs, ts, P, kind, k, full)
    guess, lam, it, rejected = cur, lm["lambda_initial"], 0, 0
    while it < lm["max_iterations"]:
        it += 1
        try:
            Di, Y, S = _reduce(F, A, D + lam * np.eye(3), W)
            S = S + lam * np.eye(6 * F)
            dc = np.linalg.solve(S, -(gc - np.einsum("fnac,nc->fa", Y, gp)).reshape(6 * F)).reshape(F, 6)
            dp = -np.einsum("nab,nb->na", Di, gp + np.einsum("fnab,fa->nb", W, dc))
            Rn = np.stack([Rs[f] @ Rot.from_rotvec(dc[f, :3]).as_matrix() for f in range(F)])
            tn = np.stack([ts[f] + Rs[f] @ dc[f, 3:] for f in range(F)])
            Pn = P + dp
            new = robust_blocks(pb, Rn, tn, Pn, kind, k, full)
            cand = new[0]
        except np.linalg.LinAlgError:   # a failed solve: lambda grows (bas_solve counts it in failed_solves)
            cand = np.inf
        if not np.isfinite(cand):
            lam = lam * lm["lambda_factor"]
            if lam > lm["lambda_upper"]:
                break
            continue
        if cand <= cur:
            dec = cur - cand
            done = dec <= lm["abs_tol"] or dec <= lm["rel_tol"] * cur
            Rs, ts, P = Rn, tn, Pn
            cur, A, gc, D, gp, W = new
            lam = lam / lm["lambda_factor"]
            if done:
                break
        else:
            rejected += 1
            inc = cand - cur
            if inc <= lm["abs_tol"] or inc <= lm["rel_tol"] * cur:
                break
            lam = lam * lm["lambda_factor"]
            if lam > lm["lambda_upper"]:
                break
    out = dict(error=cur, error_guess=guess, R=Rs, t=ts, points=P, iterations=it, rejected_steps=rejected)
    out["pose_cov"], out["point_cov"] = reweighted_cov(pb, out, kind, k, full)
    return out


# ---- (B) scipy on the rescaled residuals -------------------------------------------------------------------------------
def solve_scipy(pb, kind=NONE, k=1.0, full=False):
    F, m = len(pb["poses"]), len(pb["Xg"])
    Lo, Lp = tw.full_whiteners(pb) if full else (None, None)
    Rg, tg, _ = _guess(pb)
    wsd = [np.where(pb["var"][f] > 0, 1.0 / np.sqrt(np.where(pb["var"][f] > 0, pb["var"][f], 1.0)), 0.0) for f in range(F)]
    hp = pb["has_prior"].astype(float)
    n_obs = [int(np.count_nonzero(pb["valid"][f])) for f in range(F)]
    n_rows, n_cols = 6 * F + 2 * sum(n_obs) + 3 * m, 6 * F + 3 * m

    def unpack(x):
        Rs = np.stack([Rg[f] @ Rot.from_rotvec(x[6 * f:6 * f + 3]).as_matrix() for f in range(F)])
        return Rs, np.stack([x[6 * f + 3:6 * f + 6] for f in range(F)]), x[6 * F:].reshape(m, 3)

    def rescale(r):
        s = np.sum(r * r, axis=1)
        w, rho = loss(s, kind, k)
        ss = np.where(s > 1e-300, s, 1.0)
        g = np.where(s > 1e-300, np.sqrt(rho / ss), 1.0)
        c = np.where(s > 1e-300, (w * s - rho) / (ss * ss * g), 0.0)
        return g, c

    def fun(x, want_jac=False):
        Rs, ts, P = unpack(x)
        res = np.zeros(n_rows)
        J = np.zeros((n_rows, n_cols)) if want_jac else None
        row = 0
        for f in range(F):
            phi = x[6 * f:6 * f + 3]
            res[row:row + 3] = phi * wsd[f][:3]
            res[row + 3:row + 6] = (Rg[f].T @ (ts[f] - tg[f])) * wsd[f][3:]
            if want_jac:
                J[row:row + 3, 6 * f:6 * f + 3] = np.diag(wsd[f][:3])
                J[row + 3:row + 6, 6 * f + 3:6 * f + 6] = wsd[f][3:, None] * Rg[f].T
            row += 6
            v, r, Jc, Jp = _obs_lin_full(pb, Rs, ts, P, f, Lo) if full else _obs_lin(pb, Rs, ts, P, f)
            g, c = rescale(r)
            res[row:row + 2 * len(v)] = (g[:, None] * r).ravel()
            if want_jac:
                M = g[:, None, None] * np.eye(2) + c[:, None, None] * np.einsum("ni,nj->nij", r, r)
                # local (right) perturbation -> the global coordinates: d omega = Jr(phi) d phi, d v = Rs^T d t
                G = np.zeros((6, 6))
                G[:3, :3] = np.linalg.inv(tw._jr_inv(phi))
                G[3:, 3:] = Rs[f].T
                Jcg, Jpg = M @ (Jc @ G), M @ Jp
                for a in range(len(v)):
                    J[row + 2 * a:row + 2 * a + 2, 6 * f:6 * f + 6] = Jcg[a]
                    J[row + 2 * a:row + 2 * a + 2, 6 * F + 3 * v[a]:6 * F + 3 * v[a] + 3] = Jpg[a]
            row += 2 * len(v)
        if full:   # the point priors whitened as the observations are: L^T (P - Xg)
            res[row:] = np.einsum("mji,mj->mi", Lp, P - pb["Xg"]).ravel()
            if want_jac:
                for i in range(m):
                    J[row + 3 * i:row + 3 * i + 3, 6 * F + 3 * i:6 * F + 3 * i + 3] = Lp[i].T
                return J
            return res
        res[row:] = (((P - pb["Xg"]) / 1e-2) * hp[:, None]).ravel()
        if want_jac:
            J[row:, 6 * F:] = np.kron(np.diag(hp / 1e-2), np.eye(3))
            return J
        return res

    x0 = np.concatenate([np.concatenate([np.zeros(3), tg[f]]) for f in range(F)] + [pb["Xg"].ravel()])
    sol = least_squares(fun, x0, jac=lambda x: fun(x, True), xtol=1e-15, ftol=1e-15, gtol=1e-15, method="trf", x_scale="jac")
    Rs, ts, P = unpack(sol.x)
    out = dict(error=0.5 * np.sum(sol.fun ** 2), error_guess=0.5 * np.sum(fun(x0) ** 2), R=Rs, t=ts, points=P.copy())
    out["pose_cov"], out["point_cov"] = reweighted_cov(pb, out, kind, k, full)
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_robust_model_a.npz")
CASES = [(9, HUBER), (9, CAUCHY), (24, HUBER), (24, CAUCHY), (9, NONE)]
_KEYS = ("R", "t", "points", "pose_cov", "point_cov", "error", "error_guess", "iterations", "rejected_steps")


@functools.lru_cache(maxsize=None)
def model_a(F, kind):
    """model (A)'s estimate of outlier_problem(F) under `kind` with K_OF's constant and LM, as `python tests/ba_robust_model.py`
    recorded it in tests/golden/ba_robust_model_a.npz (minutes of numpy at F = 24; test_ba_robust_host recomputes the quickest
    case and compares)"""
    z = np.load(GOLDEN)
    return {q: z["%d_%s_%s" % (F, NAMES[kind], q)] for q in _KEYS}


def truth_distance(pb, sol):
    """largest distance of the estimated camera centres and of the points from the generator's ground truth"""
    return max(np.abs(sol["t"] - np.stack(pb["t_true"])).max(), np.abs(sol["points"] - pb["X"]).max())


if __name__ == "__main__":
    rec = {}
    for F, kind in CASES:
        pb, planted = outlier_problem(F)
        a = solve_irls(pb, kind, K_OF[kind])
        s, w = obs_stats(pb, a["R"], a["t"], a["points"], kind, K_OF[kind])
        print("F = %d %s: iterations %d rejected %d error %.12e newton step (poses, points, cond) %s" % (
            F, NAMES[kind], a["iterations"], a["rejected_steps"], a["error"],
            ["%.1e" % v for v in newton_step(pb, a, kind, K_OF[kind])]))
        print("    w: planted max %.4f clean min %.4f   distance from the truth %.3e" % (w[planted].max(), w[~planted].min(),
                                                                                       truth_distance(pb, a)), flush=True)
        for q in _KEYS:
            rec["%d_%s_%s" % (F, NAMES[kind], q)] = np.asarray(a[q])
    np.savez_compressed(GOLDEN, **rec)
