"""Problems and reference solvers of the sparse bundle adjustment (mvs_ba_refine_sparse).

sparse_problem builds chains of short tracks over consecutive frames in both forms: the dense dict test_ba_window's models
read (and, for F <= 8, as_window turns into an mvs_ba_window), and the CSR by point the sparse entry takes.  The solvers are
test_ba_window's, which are generic in F: model_solve (scipy) and model_solve_blocks (Gauss-Newton on the block-sparse normal
equations); tests/test_ba_sparse_host.py pins one against the other on this generator before the GPU is held to either.
"""
import numpy as np
from scipy.spatial.transform import Rotation as Rot

import test_ba_window as tw
import test_refine as tr

K_GENERAL = tw.K_GENERAL


def sparse_problem(seed, F, m, max_track=5, min_track=2, lone_frame=None, long_track=False, single_obs_point=True, sig=0.5, rot_sig=5e-3,
                   far=1.0, prior_frac=0.5):
    """F cameras along test_ba_window.window_problem's gently turning track, m points, each seen by min_track .. max_track consecutive
    frames (of the frames that see anything) starting at a frame that sweeps the sequence, so that every frame is covered.
    lone_frame: that frame observes nothing and is held by a prior of its own.  long_track: point 1 is seen by frames 0 and
    F - 1 only.  single_obs_point: point 0 has one observation and a prior.  Priors: an anchor on frame 0, a scale-fixing prior
    on frame 1, on about prior_frac of the points.  Returns the dense dict (window_problem's keys) with the CSR under "csr"."""
    rng = np.random.default_rng(seed)
    R, t = [Rot.from_rotvec([0.02, -0.1, 0.03]).as_matrix()], [np.array([0.4, -0.1, 0.2])]
    for f in range(1, F):
        R.append(R[-1] @ Rot.from_rotvec(rng.normal(0, 0.02, 3)).as_matrix())
        t.append(t[-1] + np.array([0.3, 0.02, 0.05]) + rng.normal(0, 0.01, 3))
    seeing = [f for f in range(F) if f != lone_frame]
    n_see = len(seeing)
    valid = np.zeros((F, m), np.uint8)
    X = np.zeros((m, 3))
    has_prior = rng.random(m) < prior_frac
    for i in range(m):
        L = int(rng.integers(min_track, max_track + 1)) if n_see > 1 else 1
        L = min(L, n_see)
        s = (i * max(n_see - 1, 1)) // max(m - 1, 1)
        s = min(s, n_see - L)
        fr = seeing[s:s + L]
        if single_obs_point and i == 0:
            fr = fr[:1]
            has_prior[i] = True
        if long_track and i == 1 and F > 2:
            fr = [0, F - 1]
        if len(fr) < 2:
            has_prior[i] = True
        valid[fr, i] = 1
        mid = 0.5 * (t[fr[0]] + t[fr[-1]])
        X[i] = mid + R[fr[len(fr) // 2]] @ np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(4, 9)])
    obs = [tr.proj(K_GENERAL, R[f], t[f], X) + rng.normal(0, sig, (m, 2)) for f in range(F)]
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
    if lone_frame is not None:
        var[lone_frame] = [1e-3, 2e-3, 3e-3, 4e-2, 5e-2, 6e-2]
    pb = dict(K=K_GENERAL, X=X, poses=np.stack(poses), var=var, Xg=Xg, pcov=pcov, obs=obs, cov=[cov] * F,
              valid=[valid[f] for f in range(F)], has_prior=has_prior, sig=sig, R_true=R, t_true=t)
    pb["csr"] = to_csr(pb)
    return pb


def to_csr(pb):
    """the dense dict's observations as mvs_ba_sparse's CSR by point: obs_off, obs_frame (ascending), obs_uv, obs_cov"""
    F, m = len(pb["poses"]), len(pb["Xg"])
    valid = np.stack([np.ones(m, np.uint8) if v is None else np.asarray(v) for v in pb["valid"]])
    off, fr, uv, cv = [0], [], [], []
    for i in range(m):
        for f in range(F):
            if valid[f, i]:
                fr.append(f)
                uv.append(pb["obs"][f][i])
                cv.append(np.eye(2).reshape(4) if pb["cov"][f] is None else np.asarray(pb["cov"][f])[i])
        off.append(len(fr))
    return dict(obs_off=np.array(off, np.int32), obs_frame=np.array(fr, np.int32), obs_uv=np.array(uv, float).reshape(-1, 2),
                obs_cov=np.array(cv, float).reshape(-1, 4))


def sparse_args(pb):
    """keyword arguments of capi.Context.ba_refine_sparse"""
    c = pb["csr"]
    return dict(K=pb["K"], frame_pose=pb["poses"], frame_prior_var=pb["var"], points=pb["Xg"], point_prior_cov=pb["pcov"],
                obs_off=c["obs_off"], obs_frame=c["obs_frame"], obs_uv=c["obs_uv"], obs_cov=c["obs_cov"])


as_window = tw.as_window
solve_blocks = tw.model_solve_blocks
solve_scipy = tw.model_solve
distances = tw._distances


def brute_plan(F, obs_off, obs_frame):
    """the envelope and the term lists of the reduced camera system, stated directly: first[i] = the smallest frame that shares a
    point with frame i; for every block (i, j), j < i, the (observation of i, observation of j) pairs in point order"""
    first = list(range(F))
    pairs = {}
    for p in range(len(obs_off) - 1):
        obs = range(obs_off[p], obs_off[p + 1])
        for a in obs:
            for c in obs:
                i, j = int(obs_frame[a]), int(obs_frame[c])
                first[i] = min(first[i], j)
                if j < i:
                    pairs.setdefault((i, j), []).append((a, c))
    by_frame = [[o for o in range(len(obs_frame)) if obs_frame[o] == f] for f in range(F)]
    return first, pairs, by_frame


def newton_step(pb, sol):
    """how far the model's estimate `sol` is from a stationary point: the largest entry of the Newton step of the poses and of
    the points there (test_ba_window.model_blocks, points eliminated block by block), and the condition number of the reduced
    camera system"""
    F = len(pb["poses"])
    _, A, gc, D, gp, W = tw.model_blocks(pb, sol["R"], sol["t"], sol["points"])
    Di = np.linalg.inv(D)
    Y = np.einsum("fnab,nbc->fnac", W, Di)
    S = -np.einsum("fnac,gndc->fagd", Y, W).reshape(6 * F, 6 * F)
    for f in range(F):
        S[6 * f:6 * f + 6, 6 * f:6 * f + 6] += A[f]
    b = -(gc - np.einsum("fnac,nc->fa", Y, gp)).reshape(6 * F)
    dc = np.linalg.solve(S, b).reshape(F, 6)
    dp = -np.einsum("nab,nb->na", Di, gp + np.einsum("fnab,fa->nb", W, dc))
    return np.abs(dc).max(), np.abs(dp).max(), np.linalg.cond(S)


def write_compat_fixture(path):
    """tests/golden/ba_sparse_12.npz: a 12-frame problem of this generator under arbitrary frame and point ids, and the block
    model's estimate of it (python tests/ba_sparse_model.py writes it; tests/test_compat_ba_sparse.py reads it)"""
    F, m = 12, 80
    pb = sparse_problem(12, F, m, lone_frame=6)
    sol = solve_blocks(pb)
    print("newton step left at the model's estimate: poses %.1e points %.1e, cond %.1e" % newton_step(pb, sol))
    rng = np.random.default_rng(12)
    c = pb["csr"]
    np.savez_compressed(path, K=pb["K"], poses=pb["poses"], var=pb["var"], Xg=pb["Xg"], pcov=pb["pcov"], obs_off=c["obs_off"],
                        obs_frame=c["obs_frame"], obs_uv=c["obs_uv"], obs_cov=c["obs_cov"],
                        frame_ids=100 + 3 * np.arange(F), point_ids=1000 + 7 * rng.permutation(m),
                        obs_order=rng.permutation(len(c["obs_frame"])), R=sol["R"], t=sol["t"], points=sol["points"],
                        pose_cov=sol["pose_cov"], point_cov=sol["point_cov"], error=sol["error"])


if __name__ == "__main__":
    import os

    write_compat_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_sparse_12.npz"))
