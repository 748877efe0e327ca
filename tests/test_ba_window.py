"""Bundle adjustment of windows of up to eight frames: mvs_ba_refine_window / mvs_ba_refine_windows.

CPU part: a numpy / scipy model of the F-frame cost (whitened residual vector -> scipy.optimize.least_squares, covariances
from the inverse of J^T J at the optimum), pinned at F = 2 against the committed oracle before it is trusted; the header /
ctypes layout of mvs_ba_window and the two new symbols.
At m = 4096 scipy's dense Jacobian (37 000 x 12 000 and more) is out of reach: there the reference is model_solve_blocks, the
same residual vector linearised analytically and solved by Gauss-Newton on the block-sparse normal equations, itself pinned
against the scipy model at m = 12 and m = 200.
GPU part: the window kernel through the C ABI against the committed oracle (a decoupled third frame), against the models, and
against itself (permutations, repeated runs, batch against single calls), plus the refusals.

Bounds of the comparison with the scipy model (test_gpu_window_matches_scipy_model): the cost agrees to 1e-9 relative (the
project's bound).  For poses, points and covariances the distance between scipy and the EXISTING oracle was measured on this
file's generator at F = 2 (reference against reference, CPU only, test_model_to_oracle_distance_sets_the_bounds prints it):
over seeds 0 .. 5 at m = 12 and seeds 0, 1 at m = 200 the largest distances were 4.4e-10 (rotation entries), 3.7e-9
(translation), 7.6e-8 (points), 5.0e-9 relative (pose covariance) and 5.7e-8 relative (point covariance).  The GPU bounds are
ten times those figures: conditioning worsens with weakly observed frames.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation as Rot

import oracle_lib as o
import test_refine as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured scipy <-> oracle distance at F = 2 (module docstring), and the bounds the GPU results are held to
MEASURED = dict(R=4.4e-10, t=3.7e-9, points=7.6e-8, pose_cov=5.0e-9, point_cov=5.7e-8)
BOUND = {k: 10.0 * v for k, v in MEASURED.items()}

K_GENERAL = np.array([[525.0, 1.5, 320.0], [0.0, 510.0, 240.0], [0.0, 0.0, 1.0]])


def window_problem(seed, F, m, K=K_GENERAL, sig=0.5, rot_sig=5e-3, far=1.0):
    """F cameras along a gently turning track in front of m points; ragged visibility (each point seen by 2 .. F frames,
    every tenth by one frame only, and those have a prior), priors on about half of the other points, an anchor on
    frame 0 and a scale-fixing prior on frame 1 (ba.cpp:43), no prior on the other frames.  Guesses: the truth perturbed
    by 5e-3 in translation and points and by rot_sig in rotation, all times `far` (the same random draws at every factor)."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(4, 9, m)], 1)
    R, t = [Rot.from_rotvec([0.02, -0.1, 0.03]).as_matrix()], [np.array([0.4, -0.1, 0.2])]
    for f in range(1, F):
        R.append(R[-1] @ Rot.from_rotvec(rng.normal(0, 0.02, 3)).as_matrix())
        t.append(t[-1] + np.array([0.3, 0.02, 0.05]) + rng.normal(0, 0.01, 3))
    obs = [tr.proj(K, R[f], t[f], X) + rng.normal(0, sig, (m, 2)) for f in range(F)]
    valid = np.zeros((F, m), np.uint8)
    has_prior = rng.random(m) < 0.5
    for i in range(m):
        if F == 1 or i % 10 == 9:
            valid[rng.integers(0, F), i] = 1
            has_prior[i] = True
        else:
            valid[rng.choice(F, int(rng.integers(2, F + 1)), replace=False), i] = 1
    pcov = np.zeros((m, 9))
    pcov[has_prior] = (np.eye(3) * 1e-2 ** 2).reshape(9)
    cov = np.tile((np.eye(2) * sig ** 2).reshape(4), (m, 1))
    Xg = X + far * rng.normal(0, 5e-3, X.shape)
    poses = []
    for f in range(F):
        Rg = R[f] if f == 0 else R[f] @ Rot.from_rotvec(far * rng.normal(0, rot_sig, 3)).as_matrix()
        tg = t[f] if f == 0 else t[f] + far * rng.normal(0, 5e-3, 3)
        poses.append(np.concatenate([Rg.reshape(9), tg]))
    var = np.zeros((F, 6))
    var[0] = 1e-5
    if F > 1:
        var[1] = 1e-2
    return dict(K=K, X=X, poses=np.stack(poses), var=var, Xg=Xg, pcov=pcov, obs=obs, cov=[cov] * F,
                valid=[valid[f] for f in range(F)], has_prior=has_prior, sig=sig, R_true=R, t_true=t)


def as_window(pb):
    return dict(K=pb["K"], frame_pose=pb["poses"], frame_prior_var=pb["var"], points=pb["Xg"], point_prior_cov=pb["pcov"],
                obs=pb["obs"], obs_cov=pb["cov"], obs_valid=pb["valid"])


def full_whiteners(pb):
    """Cholesky factors of the information matrices of a problem with full covariances: Lo[f] [m, 2, 2] from pb["cov"][f]
    (None: identity; the two off-diagonal entries averaged, as the device, the host helper and the oracle do) and Lp
    [m, 3, 3] from pb["pcov"] (None or a first entry <= 0: no prior, zero).  info = L L^T, whitened residual L^T e."""
    F, m = len(pb["poses"]), len(pb["Xg"])
    Lo = []
    for f in range(F):
        if pb["cov"][f] is None:
            Lo.append(np.tile(np.eye(2), (m, 1, 1)))
        else:
            S = np.asarray(pb["cov"][f], float).reshape(m, 2, 2)
            Lo.append(np.linalg.cholesky(np.linalg.inv(0.5 * (S + S.transpose(0, 2, 1)))))
    Lp = np.zeros((m, 3, 3))
    if pb["pcov"] is not None:
        S = np.asarray(pb["pcov"], float).reshape(m, 3, 3)
        has = S[:, 0, 0] > 0
        Lp[has] = np.linalg.cholesky(np.linalg.inv(0.5 * (S[has] + S[has].transpose(0, 2, 1))))
    return Lo, Lp


def _wt(L, e):
    return np.einsum("mji,mj->mi", L, e)


def model_solve(pb, cov=True, full=False):
    """The F-frame cost of DESIGN.md section 4.7 minimised by scipy (trf, all tolerances 1e-15), as
    test_refine._check_ba_minimiser does for two frames; covariances from inv(J^T J) at the optimum, J by central
    differences in the local (rotation, translation; right perturbation) parametrisation, as test_refine._check_covariances.
    full: whiten every observation and point prior with the Cholesky factor of its own information matrix (pb["cov"],
    pb["pcov"]; full_whiteners) instead of the scalars pb["sig"] and 1e-2."""
    F, m = len(pb["poses"]), len(pb["Xg"])
    Lo, Lp = full_whiteners(pb) if full else (None, None)
    K, sig = pb["K"], pb["sig"]
    Rg = [pb["poses"][f][:9].reshape(3, 3) for f in range(F)]
    tg = [pb["poses"][f][9:] for f in range(F)]
    wsd = [np.where(pb["var"][f] > 0, 1.0 / np.sqrt(np.where(pb["var"][f] > 0, pb["var"][f], 1.0)), 0.0) for f in range(F)]

    def whiten(Rs, ts, P):
        r = []
        for f in range(F):
            r += [Rot.from_matrix(Rg[f].T @ Rs[f]).as_rotvec() * wsd[f][:3], Rg[f].T @ (ts[f] - tg[f]) * wsd[f][3:]]
            if full:
                e = _wt(Lo[f], tr.proj(K, Rs[f], ts[f], P) - pb["obs"][f])
            else:
                e = (tr.proj(K, Rs[f], ts[f], P) - pb["obs"][f]) / sig
            r.append(e.ravel() if pb["valid"][f] is None else (e * pb["valid"][f][:, None]).ravel())
        if full:
            r.append(_wt(Lp, P - pb["Xg"]).ravel())
        else:
            r.append((((P - pb["Xg"]) / 1e-2) * pb["has_prior"][:, None]).ravel())
        return np.concatenate(r)

    def resid(x):
        Rs = [Rg[f] @ Rot.from_rotvec(x[6 * f:6 * f + 3]).as_matrix() for f in range(F)]
        ts = [x[6 * f + 3:6 * f + 6] for f in range(F)]
        return whiten(Rs, ts, x[6 * F:].reshape(m, 3))

    x0 = np.concatenate([np.concatenate([np.zeros(3), tg[f]]) for f in range(F)] + [pb["Xg"].ravel()])
    sol = least_squares(resid, x0, xtol=1e-15, ftol=1e-15, gtol=1e-15, method="trf", jac="3-point", x_scale="jac")
    Rs = np.stack([Rg[f] @ Rot.from_rotvec(sol.x[6 * f:6 * f + 3]).as_matrix() for f in range(F)])
    ts = np.stack([sol.x[6 * f + 3:6 * f + 6] for f in range(F)])
    P = sol.x[6 * F:].reshape(m, 3)
    out = dict(error=0.5 * np.sum(sol.fun ** 2), error_guess=0.5 * np.sum(resid(x0) ** 2), R=Rs, t=ts, points=P)
    if cov:
        def local(d):
            Rl = [Rs[f] @ Rot.from_rotvec(d[6 * f:6 * f + 3]).as_matrix() for f in range(F)]
            tl = [ts[f] + Rs[f] @ d[6 * f + 3:6 * f + 6] for f in range(F)]
            return whiten(Rl, tl, P + d[6 * F:].reshape(m, 3))

        n, hh = 6 * F + 3 * m, 1e-6
        J = np.empty((len(sol.fun), n))
        e = np.zeros(n)
        for k in range(n):
            e[k] = hh
            J[:, k] = (local(e) - local(-e)) / (2 * hh)
            e[k] = 0.0
        Cf = np.linalg.inv(J.T @ J)
        out["pose_cov"] = np.stack([Cf[6 * f:6 * f + 6, 6 * f:6 * f + 6] for f in range(F)])
        out["point_cov"] = np.stack([Cf[6 * F + 3 * i:6 * F + 3 * i + 3, 6 * F + 3 * i:6 * F + 3 * i + 3] for i in range(m)])
    return out


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _jr_inv(phi):
    """inverse right Jacobian of SO(3): d Log(R Exp(d)) / d d at Log(R) = phi"""
    th = np.linalg.norm(phi)
    S = _skew(phi)
    g = 1.0 / 12.0 if th < 1e-6 else 1.0 / th ** 2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return np.eye(3) + 0.5 * S + g * (S @ S)


def model_blocks(pb, Rs, ts, P, full=False):
    """The same whitened residual vector as model_solve's, linearised ANALYTICALLY in the local parametrisation (rotation,
    translation; right perturbation) and kept as the blocks of its sparse Jacobian: per frame the prior rows (6 x 6), per
    observation Jc (2 x 6) and Jp (2 x 3), per point the prior rows.  Returns the cost and the blocks of J^T J and J^T r:
    A (F x 6 x 6), gc (F x 6), D (m x 3 x 3), gp (m x 3), W (F x m x 6 x 3).  full: as model_solve."""
    F, m = len(pb["poses"]), len(pb["Xg"])
    Lo, Lp = full_whiteners(pb) if full else (None, None)
    K, sig = pb["K"], pb["sig"]
    A, gc = np.zeros((F, 6, 6)), np.zeros((F, 6))
    D, gp, W = np.zeros((m, 3, 3)), np.zeros((m, 3)), np.zeros((F, m, 6, 3))
    cost = 0.0
    for f in range(F):
        Rg, tg = pb["poses"][f][:9].reshape(3, 3), pb["poses"][f][9:]
        w = np.where(pb["var"][f] > 0, 1.0 / np.sqrt(np.where(pb["var"][f] > 0, pb["var"][f], 1.0)), 0.0)
        phi = Rot.from_matrix(Rg.T @ Rs[f]).as_rotvec()
        e = np.concatenate([phi * w[:3], (Rg.T @ (ts[f] - tg)) * w[3:]])
        Jpr = np.zeros((6, 6))
        Jpr[:3, :3] = w[:3, None] * _jr_inv(phi)
        Jpr[3:, 3:] = w[3:, None] * (Rg.T @ Rs[f])
        A[f] += Jpr.T @ Jpr
        gc[f] += Jpr.T @ e
        cost += e @ e
        v = np.ones(m, bool) if pb["valid"][f] is None else pb["valid"][f].astype(bool)
        q = (P[v] - ts[f]) @ Rs[f]
        iz = 1.0 / q[:, 2]
        x, y = q[:, 0] * iz, q[:, 1] * iz
        r = np.stack([K[0, 0] * x + K[0, 1] * y + K[0, 2], K[1, 1] * y + K[1, 2]], 1) - pb["obs"][f][v]
        Aq = np.zeros((len(q), 2, 3))
        Aq[:, 0, 0], Aq[:, 0, 1], Aq[:, 0, 2] = K[0, 0] * iz, K[0, 1] * iz, -(K[0, 0] * x + K[0, 1] * y) * iz
        Aq[:, 1, 1], Aq[:, 1, 2] = K[1, 1] * iz, -K[1, 1] * y * iz
        Sq = np.zeros((len(q), 3, 3))                      # [q]x: q' = q + q x dw
        Sq[:, 0, 1], Sq[:, 0, 2], Sq[:, 1, 0] = -q[:, 2], q[:, 1], q[:, 2]
        Sq[:, 1, 2], Sq[:, 2, 0], Sq[:, 2, 1] = -q[:, 0], -q[:, 1], q[:, 0]
        if full:
            LT = Lo[f][v].transpose(0, 2, 1)
            Jc = LT @ np.concatenate([Aq @ Sq, -Aq], axis=2)
            Jp = LT @ (Aq @ Rs[f].T)
            r = _wt(Lo[f][v], r)
        else:
            Jc = np.concatenate([Aq @ Sq, -Aq], axis=2) / sig  # (n, 2, 6)
            Jp = (Aq @ Rs[f].T) / sig                          # (n, 2, 3)
            r = r / sig
        A[f] += np.einsum("nia,nib->ab", Jc, Jc)
        gc[f] += np.einsum("nia,ni->a", Jc, r)
        D[v] += np.einsum("nia,nib->nab", Jp, Jp)
        gp[v] += np.einsum("nia,ni->na", Jp, r)
        W[f][v] = np.einsum("nia,nib->nab", Jc, Jp)
        cost += np.sum(r * r)
    if full:
        ep = _wt(Lp, P - pb["Xg"])
        D += Lp @ Lp.transpose(0, 2, 1)
        gp += np.einsum("mij,mj->mi", Lp, ep)
        cost += np.sum(ep * ep)
        return 0.5 * cost, A, gc, D, gp, W
    hp = pb["has_prior"].astype(float)
    ep = (P - pb["Xg"]) / 1e-2 * hp[:, None]
    D += (hp / 1e-4)[:, None, None] * np.eye(3)
    gp += ep / 1e-2
    cost += np.sum(ep * ep)
    return 0.5 * cost, A, gc, D, gp, W


def model_solve_blocks(pb, cov=True, full=False):
    """The minimiser of the same cost by Gauss-Newton on the block-sparse normal equations (points eliminated block by block),
    for sizes where scipy's dense Jacobian is out of reach; steps are halved while the cost does not decrease, and the
    iteration ends two steps after a step stops changing the cost.  Covariances: the blocks of inv(J^T J) by the same
    elimination.  test_block_model_agrees_with_scipy_model pins it against model_solve."""
    F, m = len(pb["poses"]), len(pb["Xg"])
    Rs = np.stack([pb["poses"][f][:9].reshape(3, 3) for f in range(F)])
    ts = np.stack([pb["poses"][f][9:] for f in range(F)])
    P = pb["Xg"].copy()

    def reduce(A, gc, D, gp, W):
        Di = np.linalg.inv(D)
        Y = np.einsum("fnab,nbc->fnac", W, Di)
        S = -np.einsum("fnac,gndc->fagd", Y, W).reshape(6 * F, 6 * F)
        for f in range(F):
            S[6 * f:6 * f + 6, 6 * f:6 * f + 6] += A[f]
        return Di, Y, S

    cur, A, gc, D, gp, W = model_blocks(pb, Rs, ts, P, full)
    guess, flat = cur, 0
    for _ in range(60):
        Di, Y, S = reduce(A, gc, D, gp, W)
        b = -(gc - np.einsum("fnac,nc->fa", Y, gp)).reshape(6 * F)
        dc = np.linalg.solve(S, b).reshape(F, 6)
        dp = -np.einsum("nab,nb->na", Di, gp + np.einsum("fnab,fa->nb", W, dc))
        step, moved = 1.0, False
        while step > 1e-4:
            Rn = np.stack([Rs[f] @ Rot.from_rotvec(step * dc[f, :3]).as_matrix() for f in range(F)])
            tn = np.stack([ts[f] + Rs[f] @ (step * dc[f, 3:]) for f in range(F)])
            Pn = P + step * dp
            new = model_blocks(pb, Rn, tn, Pn, full)
            if new[0] <= cur:
                moved = True
                break
            step *= 0.5
        if not moved:
            break
        flat = flat + 1 if cur - new[0] <= 1e-15 * cur else 0
        Rs, ts, P = Rn, tn, Pn
        cur, A, gc, D, gp, W = new
        if flat >= 2:
            break
    out = dict(error=cur, error_guess=guess, R=Rs, t=ts, points=P)
    if cov:
        Di, Y, S = reduce(A, gc, D, gp, W)
        Si = np.linalg.inv(S)
        out["pose_cov"] = np.stack([Si[6 * f:6 * f + 6, 6 * f:6 * f + 6] for f in range(F)])
        Yn = Y.transpose(1, 0, 2, 3).reshape(m, 6 * F, 3)          # rows of W D^-1 per point
        out["point_cov"] = Di + np.einsum("nac,ab,nbd->ncd", Yn, Si, Yn)
    return out


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


def _distances(got, want):
    d = dict(R=np.abs(got["R"] - want["R"]).max(), t=np.abs(got["t"] - want["t"]).max(),
             points=np.abs(got["points"] - want["points"]).max(),
             pose_cov=max(_rel(got["pose_cov"][f], want["pose_cov"][f]) for f in range(len(want["pose_cov"]))),
             point_cov=_rel(got["point_cov"], want["point_cov"]))
    return d


# ---------------------------------------------------------------------------------------------------------------------
# CPU

def test_model_agrees_with_oracle_on_the_two_frame_generator():
    """the numpy model is pinned before it is trusted: test_refine's general two-frame problem, that file's oracle <-> scipy
    bounds (cost 1e-9 relative, pose 1e-8, points 1e-7)"""
    pb = tr.track_refine_problem(3, 24, 5)
    want = o.ba_refine(pb["K"], pb["poses"], pb["var"], pb["Xg"], pb["pcov"], pb["obs"], pb["cov"], pb["valid"])
    got = model_solve(pb, cov=False)
    assert want["ok"]
    assert abs(got["error"] - want["error"]) <= 1e-9 * want["error"]
    assert np.abs(got["R"] - want["R"]).max() < 1e-8 and np.abs(got["t"] - want["t"]).max() < 1e-8
    assert np.abs(got["points"] - want["points"]).max() < 1e-7


@pytest.mark.parametrize("m", [12, 200])
def test_model_to_oracle_distance_sets_the_bounds(m):
    """reference against reference on this file's generator at F = 2: prints the distances the module docstring quotes; the
    two references themselves stay inside the bounds derived from them"""
    worst = dict.fromkeys(MEASURED, 0.0)
    for seed in range(6 if m == 12 else 2):
        pb = window_problem(seed, 2, m)
        want = o.ba_refine(pb["K"], pb["poses"], pb["var"], pb["Xg"], pb["pcov"], pb["obs"], pb["cov"], pb["valid"])
        got = model_solve(pb)
        assert want["ok"] and abs(got["error"] - want["error"]) <= 1e-9 * want["error"]
        for k, v in _distances(got, want).items():
            worst[k] = max(worst[k], v)
    print("scipy <-> oracle at F = 2, m = %d: %s" % (m, {k: "%.2e" % v for k, v in worst.items()}))
    for k in MEASURED:
        assert worst[k] <= BOUND[k], (k, worst[k])


@pytest.mark.parametrize("F,m", [(4, 12), (3, 200)])
def test_block_model_agrees_with_scipy_model(F, m):
    """the block-sparse model (the reference at m = 4096) against the scipy model where both run: the same cost to 1e-9
    relative, everything else within the measured scipy <-> oracle distance times ten (BOUND)"""
    pb = window_problem(10 * F + 1, F, m)
    a, b = model_solve_blocks(pb), model_solve(pb)
    d = _distances(a, b)
    print("block model <-> scipy at F = %d, m = %d: cost %.2e %s" % (F, m, abs(a["error"] - b["error"]) / b["error"],
                                                                     {k: "%.2e" % v for k, v in d.items()}))
    assert abs(a["error"] - b["error"]) <= 1e-9 * b["error"]
    for k, v in d.items():
        assert v <= BOUND[k], (k, v)


def test_window_struct_layout_and_symbols():
    """mvs_ba_window: header <-> ctypes; the two new entry points are exported; the ABI version is still 4"""
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(mvs_ba_window), offsetof(mvs_ba_window, n_points), offsetof(mvs_ba_window, K),
         offsetof(mvs_ba_window, point_prior_cov), offsetof(mvs_ba_window, obs), offsetof(mvs_ba_window, obs_cov),
         offsetof(mvs_ba_window, obs_valid));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    W = capi.BaWindow
    assert v == [C.sizeof(W), W.n_points.offset, W.K.offset, W.point_prior_cov.offset, W.obs.offset, W.obs_cov.offset,
                 W.obs_valid.offset]
    lib = capi.lib()
    assert hasattr(lib, "mvs_ba_refine_window") and hasattr(lib, "mvs_ba_refine_windows")
    assert lib.mvs_abi_version() == 4


def test_window_kernel_resources():
    """from the code object's digest: no scratch, and static LDS within 64 KB"""
    import json

    res = json.load(open(os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")))
    hits = {k: v for k, v in res.items() if "refine_window_kernel" in k}
    assert len(hits) == 1
    for k, v in hits.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0, (k, v)
        assert v["static_lds_bytes"] <= 64 * 1024, (k, v)


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def _with_decoupled_frame(pb, seed):
    """the two-frame problem plus a third frame with a prior, a guess and no valid observation"""
    rng = np.random.default_rng(seed)
    m = len(pb["Xg"])
    p2 = np.concatenate([Rot.from_rotvec(rng.normal(0, 0.2, 3)).as_matrix().reshape(9), rng.normal(0, 1.0, 3)])
    var2 = np.array([1e-3, 2e-3, 3e-3, 4e-2, 5e-2, 6e-2])
    return dict(K=pb["K"], frame_pose=np.vstack([pb["poses"], p2]), frame_prior_var=np.vstack([pb["var"], var2]),
                points=pb["Xg"], point_prior_cov=pb["pcov"], obs=pb["obs"] + [rng.uniform(0, 600, (m, 2))],
                obs_cov=pb["cov"] + [None], obs_valid=pb["valid"] + [np.zeros(m, np.uint8)]), p2, var2


@pytest.mark.gpu
@pytest.mark.parametrize("m,n_new,seed", [(24, 5, 3), (400, 60, 4), (1500, 0, 5)])
def test_gpu_window_decoupled_third_frame_matches_oracle(ctx, m, n_new, seed):
    """the NEW kernel (F = 3) against the COMMITTED oracle at test_gpu_ba_refine_matches_oracle's bounds: the third frame
    does not enter the cost of the other two"""
    pb = tr.track_refine_problem(seed, m, n_new)
    want = o.ba_refine(pb["K"], pb["poses"], pb["var"], pb["Xg"], pb["pcov"], pb["obs"], pb["cov"], pb["valid"])
    w, p2, var2 = _with_decoupled_frame(pb, seed)
    got = ctx.ba_refine_windows([w])[0]
    assert got["ok"] and want["ok"] and got["status"] == 0
    print("error %.3e  R %.3e  t %.3e  points %.3e" % (abs(got["error"] - want["error"]) / want["error"],
          np.abs(got["R"][:2] - want["R"]).max(), np.abs(got["t"][:2] - want["t"]).max(),
          np.abs(got["points"] - want["points"]).max()))
    assert abs(got["error"] - want["error"]) <= 1e-10 * want["error"]
    assert np.abs(got["R"][:2] - want["R"]).max() < 1e-9 and np.abs(got["t"][:2] - want["t"]).max() < 1e-9
    assert np.abs(got["points"] - want["points"]).max() < 1e-8
    for f in range(2):
        tr._close(got["pose_cov"][f], want["pose_cov"][f], 1e-6, "pose_cov[%d]" % f)
    tr._close(got["point_cov"], want["point_cov"], 1e-6, "point_cov")
    # frame 2 comes back at its guess, with its prior variance as covariance
    assert np.abs(got["R"][2].reshape(9) - p2[:9]).max() < 1e-12 and np.abs(got["t"][2] - p2[9:]).max() < 1e-12
    tr._close(got["pose_cov"][2], np.diag(var2), 1e-9, "pose_cov[2]")


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 2])
def test_gpu_window_of_one_or_two_frames_is_mvs_ba_refine(ctx, F):
    pb = tr.track_refine_problem(4, 400, 60)
    if F == 1:
        pb = dict(pb, poses=pb["poses"][1:], var=pb["var"][1:], obs=pb["obs"][1:], cov=pb["cov"][1:], valid=[None],
                  pcov=np.tile((np.eye(3) * 1e-4).reshape(9), (400, 1)))
    a = ctx.ba_refine(pb["K"], pb["poses"], pb["var"], pb["Xg"], pb["pcov"], pb["obs"], pb["cov"], pb["valid"])
    b = ctx.ba_refine_window(pb["K"], pb["poses"], pb["var"], pb["Xg"], pb["pcov"], pb["obs"], pb["cov"], pb["valid"])
    assert a["ok"] and b["ok"]
    for k in ("R", "t", "pose_cov", "points", "point_cov"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["error"] == b["error"] and a["iterations"] == b["iterations"]


@pytest.mark.gpu
@pytest.mark.parametrize("m", [12, 200, 4096])
@pytest.mark.parametrize("F", [3, 4, 6, 8])
def test_gpu_window_matches_scipy_model(ctx, F, m):
    """general K, ragged visibility, mixed point priors, anchor + scale-fixing prior: against the numpy / scipy model
    (m = 4096: against the block-sparse model, module docstring).  Cost 1e-9 relative; the other bounds are BOUND (ten times
    the measured scipy <-> oracle distance, module docstring)."""
    pb = window_problem(10 * F + 1, F, m)
    want = model_solve(pb) if m <= 200 else model_solve_blocks(pb)
    got = ctx.ba_refine_windows([as_window(pb)])[0]
    assert got["ok"]
    d = _distances(got, want)
    print("F = %d m = %d: cost %.3e  %s  iterations %d" % (F, m, abs(got["error"] - want["error"]) / want["error"],
                                                            {k: "%.2e" % v for k, v in d.items()}, got["iterations"]))
    assert abs(got["error"] - want["error"]) <= 1e-9 * want["error"]
    for k, v in d.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


@pytest.mark.gpu
@pytest.mark.parametrize("F,m", [(4, 200), (8, 4096)])
def test_gpu_window_permutation_invariance(ctx, F, m):
    """permuting frames 1 .. F - 1 and permuting points permutes the outputs (bounds of the scipy comparison)"""
    pb = window_problem(7, F, m)
    rng = np.random.default_rng(1)
    fp = np.concatenate([[0], 1 + rng.permutation(F - 1)])
    pp = rng.permutation(m)
    q = dict(pb, poses=pb["poses"][fp], var=pb["var"][fp], Xg=pb["Xg"][pp], pcov=pb["pcov"][pp],
             obs=[pb["obs"][f][pp] for f in fp], cov=[pb["cov"][f][pp] for f in fp], valid=[pb["valid"][f][pp] for f in fp])
    a, b = ctx.ba_refine_windows([as_window(pb), as_window(q)])
    assert a["ok"] and b["ok"]
    assert abs(a["error"] - b["error"]) <= 1e-9 * a["error"]
    d = _distances(dict(R=b["R"], t=b["t"], points=b["points"], pose_cov=b["pose_cov"], point_cov=b["point_cov"]),
                   dict(R=a["R"][fp], t=a["t"][fp], points=a["points"][pp], pose_cov=a["pose_cov"][fp], point_cov=a["point_cov"][pp]))
    print({k: "%.2e" % v for k, v in d.items()})
    for k, v in d.items():
        assert v <= BOUND[k], (k, v)


def _mixed_batch(n):
    shapes = [(3, 12), (8, 200), (2, 50), (5, 333), (1, 40), (4, 4096), (6, 31), (7, 64), (3, 1000), (8, 33)]
    out = []
    for p in range(n):
        F, m = shapes[p % len(shapes)]
        if p >= len(shapes):
            m = min(m, 300)
        pb = window_problem(100 + p, F, m)
        if F == 1:
            pb["pcov"] = np.tile((np.eye(3) * 1e-4).reshape(9), (m, 1))
        out.append(as_window(pb))
    return out


def _bytes(r):
    return r["raw"] + r["points"].tobytes() + r["point_cov"].tobytes()


@pytest.mark.gpu
def test_gpu_window_batch_is_deterministic_and_equals_single_calls(ctx):
    """two runs of a batch of 64 mixed windows give identical bytes, and the batch equals the 64 single calls byte for byte"""
    batch = _mixed_batch(64)
    a = ctx.ba_refine_windows(batch)
    b = ctx.ba_refine_windows(batch)
    assert all(r["ok"] for r in a)
    assert [_bytes(r) for r in a] == [_bytes(r) for r in b]
    for p, w in enumerate(batch):
        s = ctx.ba_refine_window(w["K"], w["frame_pose"], w["frame_prior_var"], w["points"], w["point_prior_cov"], w["obs"],
                                 w["obs_cov"], w["obs_valid"])
        assert s["ok"] and _bytes(s) == _bytes(a[p]), p


@pytest.mark.gpu
def test_gpu_window_improves_on_chained_pairs(ctx):
    """five frames, 1 px noise, guesses perturbed as test_refine.l_shape_refine_problem does (5e-3 translation, 1e-2
    rotation, points 5e-3), the generator's mixed point priors: the window's final error is no larger than the error at the
    guess and no larger than the error of the state that refining consecutive pairs separately with mvs_sfm_refine and
    chaining them gives (with whichever pair's points serve that state best)"""
    F, m = 5, 300
    pb = window_problem(21, F, m, sig=1.0, rot_sig=1e-2)
    pb["valid"] = [np.ones(m, np.uint8) for _ in range(F)]
    K = pb["K"]
    Rg = [pb["poses"][f][:9].reshape(3, 3) for f in range(F)]
    tg = [pb["poses"][f][9:] for f in range(F)]

    def cost(Rs, ts, P):
        c = 0.0
        for f in range(F):
            sd = np.where(pb["var"][f] > 0, 1.0 / np.sqrt(np.where(pb["var"][f] > 0, pb["var"][f], 1.0)), 0.0)
            c += np.sum((Rot.from_matrix(Rg[f].T @ Rs[f]).as_rotvec() * sd[:3]) ** 2) + np.sum((Rg[f].T @ (ts[f] - tg[f]) * sd[3:]) ** 2)
            c += np.sum(((tr.proj(K, Rs[f], ts[f], P) - pb["obs"][f]) / pb["sig"]) ** 2)
        return 0.5 * (c + np.sum((((P - pb["Xg"]) / 1e-2) * pb["has_prior"][:, None]) ** 2))

    got = ctx.ba_refine_windows([as_window(pb)])[0]
    assert got["ok"]
    assert abs(got["error"] - cost(got["R"], got["t"], got["points"])) <= 1e-9 * got["error"]
    assert got["error"] <= cost(Rg, tg, pb["Xg"])
    # consecutive pairs, each in its first camera's frame, chained into the world frame
    Rc, tc, Ps = [Rg[0]], [tg[0]], []
    for f in range(F - 1):
        Rrel, trel = Rg[f].T @ Rg[f + 1], Rg[f].T @ (tg[f + 1] - tg[f])
        Xl = (pb["Xg"] - tg[f]) @ Rg[f]
        r = ctx.sfm_refine(pb["obs"][f], pb["cov"][f], pb["obs"][f + 1], pb["cov"][f + 1], K, Rrel, trel, Xl)
        assert r["ok"]
        Rc.append(Rc[f] @ r["R"])
        tc.append(tc[f] + Rc[f] @ r["t"])
        Ps.append(r["points"] @ Rc[f].T + tc[f])
    chained = min(cost(Rc, tc, P) for P in Ps)
    print("guess %.6e  chained pairs %.6e  window %.6e" % (cost(Rg, tg, pb["Xg"]), chained, got["error"]))
    assert got["error"] <= chained


@pytest.mark.gpu
def test_gpu_window_refusals(ctx):
    """legal calls that must be refused cleanly, and the context solves a good problem afterwards"""
    from mvslam_amd import capi

    pb = window_problem(5, 4, 60)
    good = as_window(pb)
    # no priors at all: the gauge is free
    free = dict(good, frame_prior_var=np.zeros((4, 6)), point_prior_cov=None,
                obs_valid=[np.ones(60, np.uint8)] * 4)
    r = ctx.ba_refine_windows([free])[0]
    assert not r["ok"] and r["status"] == capi.MVS_NO_MODEL and r["iterations"] <= capi.default_refine_params().max_iterations
    # a point nobody observes and that has no prior
    valid = [v.copy() for v in pb["valid"]]
    pcov = pb["pcov"].copy()
    for v in valid:
        v[7] = 0
    pcov[7] = 0.0
    r = ctx.ba_refine_windows([dict(good, obs_valid=valid, point_prior_cov=pcov)])[0]
    assert not r["ok"] and r["status"] == capi.MVS_NO_MODEL
    # a batch with one bad window reports it and still solves the others
    rs = ctx.ba_refine_windows([good, free, good])
    assert [x["ok"] for x in rs] == [True, False, True]
    assert [x["status"] for x in rs] == [capi.MVS_OK, capi.MVS_NO_MODEL, capi.MVS_OK]
    assert _bytes(rs[0]) == _bytes(rs[2])

    # frames held by nothing but their observations and a prior of variance 1e6 are weakly but legitimately constrained:
    # the pivot rule must not refuse them, and the answer is the model's
    weak = dict(pb, var=np.vstack([pb["var"][:2], np.full((2, 6), 1e6)]))
    r = ctx.ba_refine_windows([as_window(weak)])[0]
    want = model_solve(weak)
    assert r["ok"] and abs(r["error"] - want["error"]) <= 1e-9 * want["error"]
    for k, v in _distances(r, want).items():
        assert v <= BOUND[k], (k, v)

    def status_of(w):
        with pytest.raises(capi.MvsError) as e:
            ctx.ba_refine_windows([w])
        return e.value.status

    nine = window_problem(5, 8, 20)
    w9 = as_window(nine)
    w9 = dict(w9, frame_pose=np.vstack([w9["frame_pose"], w9["frame_pose"][:1]]),
              frame_prior_var=np.vstack([w9["frame_prior_var"], np.zeros((1, 6))]), obs=w9["obs"] + w9["obs"][:1],
              obs_cov=w9["obs_cov"] + [None], obs_valid=w9["obs_valid"] + w9["obs_valid"][:1])
    assert status_of(w9) == -4                                     # MVS_ERR_CAPACITY
    Kbad = pb["K"].copy()
    Kbad[2, 0] = 1e-3
    assert status_of(dict(good, K=Kbad)) == -5                      # MVS_ERR_BAD_INTRINSICS
    big = window_problem(5, 3, 4097)
    assert status_of(as_window(big)) == -4
    empty = dict(good, points=np.zeros((0, 3)), point_prior_cov=None, obs=[np.zeros((0, 2))] * 4, obs_cov=None, obs_valid=None)
    assert status_of(empty) == -1                                   # MVS_ERR_INVALID_ARG
    again = ctx.ba_refine_windows([good])[0]
    assert again["ok"] and _bytes(again) == _bytes(rs[0])
