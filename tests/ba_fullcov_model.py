"""Sparse bundle-adjustment problems with FULL covariances (mvs_ba_refine_sparse, mvs_ba_sparse_obs_stats; DESIGN.md sections
4.7.4 and 4.7.6): tests/ba_sparse_model.py's generator with a different full SPD 2 x 2 covariance on every observation
(test_refine_edges.full_cov2: axes of 0.5 .. 3 sig at a uniform angle, so a ratio of up to 6 in the standard deviations and
correlation coefficients of both signs up to 0.95) and a full SPD 3 x 3 prior on every point that has one
(test_refine_edges.full_cov3 at the generator's 1e-4), so that the off-diagonal information entry W1 the isotropic problems
leave at zero takes part in every sum.

References.  Without a loss: test_ba_window.model_solve_blocks / model_solve with full=True, as they are.  Under a loss:
ba_robust_model's two models with full=True.  tests/test_ba_fullcov_host.py pins them against each other on these problems,
checks that each has converged, and that every problem tells a negated or a zeroed off-diagonal from the true one by more
than the bound the device is held to.

python tests/ba_fullcov_model.py writes tests/golden/ba_fullcov_model_a.npz, model (A)'s estimates of the outlier problem."""
import functools
import os

import numpy as np

import ba_robust_model as rm
import ba_sparse_model as bm
import test_ba_window as tw
import test_refine_edges as te

ASYM = 0.03   # the off-diagonal entries of the asymmetric variant lie up to that far apart (relative)


def with_full_cov(pb, seed, asym=0.0, sig=None):
    """pb (ba_sparse_model.sparse_problem) with its covariances replaced: one full 2 x 2 covariance per observation, a full
    3 x 3 prior covariance on the points that have a prior (zero rows elsewhere: no prior)"""
    F, m = len(pb["poses"]), len(pb["Xg"])
    rng = np.random.default_rng(7000 + seed)
    cov = [te.full_cov2(rng, m, pb["sig"] if sig is None else sig, asym) for _ in range(F)]
    pcov = te.full_cov3(rng, m, 1e-4, asym)
    pcov[~pb["has_prior"]] = 0.0
    out = dict(pb, cov=cov, pcov=pcov)
    out["csr"] = bm.to_csr(out)
    return out


def symmetrised(pb):
    """the problem whose off-diagonal entries are the averages of pb's"""
    cov = []
    for c in pb["cov"]:
        c = c.copy()
        c[:, 1] = c[:, 2] = 0.5 * (c[:, 1] + c[:, 2])
        cov.append(c)
    S = pb["pcov"].reshape(-1, 3, 3)
    out = dict(pb, cov=cov, pcov=(0.5 * (S + S.transpose(0, 2, 1))).reshape(-1, 9))
    out["csr"] = bm.to_csr(out)
    return out


def off_diagonal(pb, factor):
    """the power check's problems: every observation covariance with its off-diagonal entries times `factor` (-1: the
    correlation's sign is wrong; 0: it is dropped; both stay SPD)"""
    cov = []
    for c in pb["cov"]:
        c = c.copy()
        c[:, 1:3] *= factor
        cov.append(c)
    out = dict(pb, cov=cov)
    out["csr"] = bm.to_csr(out)
    return out


def prior_off_diagonal_dropped(pb):
    """every point prior covariance reduced to its diagonal (SPD still)"""
    pcov = pb["pcov"].copy()
    pcov[:, [1, 2, 3, 5, 6, 7]] = 0.0
    return dict(pb, pcov=pcov)


# Seeds, picked on the CPU so that the block model's remaining Newton step (newton_step below) is under 1e-9 in poses and
# points; tests/test_ba_fullcov_host.py asserts it and its docstring has the figures.
SEED = {(3, 12): 3, (8, 40): 8, (9, 300): 9, (24, 300): 324}
CASES = list(SEED)


@functools.lru_cache(maxsize=None)
def problem(F, m, asym=0.0):
    """(3, 12) and (8, 40): tracks of up to F frames, as test_ba_sparse._small.  (9, 300): tracks of 2 .. 5 frames.  (24, 300):
    also a frame held by its prior alone and a track over frames 0 and F - 1.  Each with a point of one observation."""
    seed = SEED[(F, m)]
    if F <= 8:
        pb = bm.sparse_problem(seed, F, m, max_track=F)
    else:
        pb = bm.sparse_problem(seed, F, m, lone_frame=F // 2 if F == 24 else None, long_track=F == 24)
    return with_full_cov(pb, seed, asym)


@functools.lru_cache(maxsize=None)
def solution(F, m):
    """the block model's estimate of problem(F, m)"""
    return tw.model_solve_blocks(problem(F, m), full=True)


def newton_step(pb, sol):
    """ba_sparse_model.newton_step with full covariances"""
    return rm.newton_step(pb, sol, rm.NONE, 1.0, full=True)


def cost_at_guess(pb):
    return tw.model_blocks(pb, *rm._guess(pb), full=True)[0]


# ---- no point priors, no observation covariances -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def no_point_prior_problem():
    """F = 9, m = 40, every point on at least two frames, no prior on any point: the frame priors alone hold the gauge"""
    pb = bm.sparse_problem(23, 9, 40, single_obs_point=False, prior_frac=0.0)
    assert not pb["has_prior"].any() and np.stack(pb["valid"]).sum(0).min() >= 2
    return with_full_cov(pb, 23)


@functools.lru_cache(maxsize=None)
def unit_cov_problem(F=9, m=40):
    """sig = 1 and identity observation covariances (what obs_cov = NULL means), full point priors"""
    pb = with_full_cov(bm.sparse_problem(29, F, m, sig=1.0), 29)
    out = dict(pb, cov=[np.tile(np.eye(2).reshape(4), (m, 1))] * F)
    out["csr"] = bm.to_csr(out)
    return out


# ---- planted outliers ----------------------------------------------------------------------------------------------------
# Under a loss IRLS ends where rounding decides its accept / reject, which left 1e-9 .. 1e-8 of Newton step in the points on
# most seeds (about a hundred were tried); each loss has the seed and the shortest track at which its model (A) is
# stationary to 1e-9.  Without a loss the statistics use Huber's problem.
OUTLIER = {rm.NONE: dict(seed=45, min_track=2), rm.HUBER: dict(seed=45, min_track=2), rm.CAUCHY: dict(seed=81, min_track=3)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_fullcov_model_a.npz")
_KEYS = ("R", "t", "points", "pose_cov", "point_cov", "error", "error_guess", "iterations", "rejected_steps")


@functools.lru_cache(maxsize=None)
def _outlier_problem(seed, min_track):
    pb = with_full_cov(bm.sparse_problem(seed, 9, 300, min_track=min_track), 100 + seed)
    return rm.plant_outliers(pb, 1000 + seed)


def outlier_problem(kind):
    """problem(9, 300)'s kind with ba_robust_model.plant_outliers' displaced observations (the whitened displacement depends on
    the observation's own covariance: 30 .. 100 px across axes of 0.25 .. 1.5 px); the planted mask with it"""
    return _outlier_problem(**OUTLIER[kind])


@functools.lru_cache(maxsize=None)
def model_a(kind):
    """model (A)'s estimate of outlier_problem(kind) under `kind` with ba_robust_model.K_OF's constant and LM, as recorded in
    tests/golden/ba_fullcov_model_a.npz (test_ba_fullcov_host recomputes it and compares)"""
    z = np.load(GOLDEN)
    return {q: z["%s_%s" % (rm.NAMES[kind], q)] for q in _KEYS}


if __name__ == "__main__":
    rec = {}
    for kind in (rm.HUBER, rm.CAUCHY):
        pb, planted = outlier_problem(kind)
        a = rm.solve_irls(pb, kind, rm.K_OF[kind], full=True)
        s, w = rm.obs_stats(pb, a["R"], a["t"], a["points"], kind, rm.K_OF[kind], full=True)
        print("%s: iterations %d rejected %d error %.12e newton step (poses, points, cond) %s" % (
            rm.NAMES[kind], a["iterations"], a["rejected_steps"], a["error"],
            ["%.1e" % v for v in rm.newton_step(pb, a, kind, rm.K_OF[kind], full=True)]))
        print("    w: planted max %.4f clean min %.4f" % (w[planted].max(), w[~planted].min()), flush=True)
        for q in _KEYS:
            rec["%s_%s" % (rm.NAMES[kind], q)] = np.asarray(a[q])
    np.savez_compressed(GOLDEN, **rec)
