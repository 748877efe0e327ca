"""Sparse bundle adjustment with full covariances, CPU part: the reference models against each other on
tests/ba_fullcov_model.py's problems, their convergence, and the POWER of every problem -- what the device is held to in
tests/test_ba_fullcov.py is measured and derived here, none of it comes from a device result.

Without a loss.  F <= 8 (F = 3, m = 12 and F = 8, m = 40, the device's problems): block model against scipy
(test_ba_window.model_solve_blocks / model_solve, full=True) gave at most R 1.6e-11, t 9.9e-11, points 2.2e-9, pose_cov 1.4e-9,
point_cov 8.5e-9 -- inside test_ba_window.MEASURED, so section 4.7's bounds (test_ba_window.BOUND) hold these two as they hold
the isotropic ones.  F > 8: the dense scipy model is out of reach at m = 300, so, as tests/test_ba_sparse_host.py does, the
distance is measured at m = 60 on the same generator with the same covariances (F = 9 seeds 0 and 8, F = 24 seed 13: of the
seeds 0 .. 13 those at which the block model is stationary to 1e-9 with room to spare; scipy was left with up to 6.8e-9 in the
poses and 4.5e-8 in the points at F = 24, which is what the distance shows).  The largest distances were 1.20e-9 (rotation),
6.78e-9 (translation), 5.04e-8 (points), 2.43e-8 relative (pose covariance) and 3.64e-8 relative (point covariance):
MEASURED_FULLCOV, rounded up; the device is held to ten times that (BOUND_FULLCOV) and to 1e-9 relative in the cost.

Under a loss (F = 9, m = 300, planted outliers; ba_robust_model.solve_irls / solve_scipy, full=True): model (A) against model
(B) on ba_fullcov_model.outlier_problem (one seed per loss, see there):
    loss    rotation  translation  points    pose_cov (rel)  point_cov (rel)  cost (rel)  Newton step left at A, at B (poses, points)
    Huber   7.03e-10  3.40e-09     3.17e-08  7.08e-09        1.51e-08         4.2e-16     7.6e-11 6.5e-10,  1.8e-09 1.7e-08
    Cauchy  1.08e-10  1.42e-10     7.22e-09  5.33e-10        3.82e-09         2.0e-15     1.6e-11 6.3e-10,  4.8e-11 2.6e-09
MEASURED_FULLCOV_ROBUST is the larger of each column, rounded up; the device is held to model (A) within ten times that
(BOUND_FULLCOV_ROBUST).  Model (A)'s weights there: planted at most 0.0782 (Huber) and 0.0088 (Cauchy), clean at least 0.6975
and 0.1781; W_SPLIT_FULLCOV lies in the gap with a factor of two to spare either side.

Convergence: the Newton step the (reweighted) normal equations still ask for at each reference the device is compared with
is below 1e-9 in poses and points (NEWTON); the seeds were picked for that and are recorded in ba_fullcov_model.

Power: each problem is solved again with the off-diagonal entries of every observation covariance negated, and zeroed.  The
estimate moves by 2e-3 .. 2e-2 in the translations and 4e-2 .. 9e-1 in the points, four orders of magnitude and more beyond the bounds, and
the cost at the guess by 8e-4 .. 3e-1 relative: a wrong sign of W1, a dropped W1 or swapped W0 / W2 cannot pass.  Reducing the
point priors to their diagonals moves the points by 2e-3 and more.
"""
import numpy as np
import pytest

import ba_fullcov_model as fm
import ba_robust_model as rm
import ba_sparse_model as bm
import test_ba_window as tw

# block model <-> scipy at F in {9, 24}, m = 60, full covariances (the module docstring), rounded up
MEASURED_FULLCOV = dict(R=1.3e-9, t=6.8e-9, points=5.1e-8, pose_cov=2.5e-8, point_cov=3.7e-8)
BOUND_FULLCOV = {k: 10.0 * v for k, v in MEASURED_FULLCOV.items()}
# model (A) <-> model (B) on the outlier problem under Huber and Cauchy, rounded up
MEASURED_FULLCOV_ROBUST = dict(R=7.1e-10, t=3.5e-9, points=3.2e-8, pose_cov=7.1e-9, point_cov=1.6e-8)
BOUND_FULLCOV_ROBUST = {k: 10.0 * v for k, v in MEASURED_FULLCOV_ROBUST.items()}
NEWTON = 1e-9
# between model (A)'s largest weight over the planted observations and its smallest over the clean ones
W_SPLIT_FULLCOV = {rm.HUBER: 0.25, rm.CAUCHY: 0.04}


def _report(tag, a, b):
    d = bm.distances(a, b)
    cost = abs(float(a["error"]) - b["error"]) / b["error"]
    print("%s: cost %.2e %s" % (tag, cost, {k: "%.2e" % v for k, v in d.items()}))
    return cost, d


def _moved(tag, pb, ref, other, bound, solve):
    """the power of pb: `other`, the same problem with wrong off-diagonals, has an estimate further from pb's than the bound
    in the translations or the points; returns the relative change of the cost at the guess"""
    d = bm.distances(solve(other), ref)
    dc = abs(fm.cost_at_guess(other) - fm.cost_at_guess(pb)) / fm.cost_at_guess(pb)
    print("%s: cost at the guess %.2e %s" % (tag, dc, {k: "%.2e" % v for k, v in d.items()}))
    assert d["t"] > bound["t"] or d["points"] > bound["points"], (tag, d)
    return dc


@pytest.mark.parametrize("F,m", [(3, 12), (8, 40)])
def test_models_pinned_at_up_to_eight_frames(F, m):
    """the device's two small problems: block model against scipy inside test_ba_window.BOUND"""
    pb = fm.problem(F, m)
    cost, d = _report("F = %d, m = %d" % (F, m), fm.solution(F, m), tw.model_solve(pb, full=True))
    assert cost <= 1e-9
    for k, v in d.items():
        assert v <= tw.BOUND[k], (k, v)


@pytest.mark.parametrize("F,seeds", [(9, (0, 8)), (24, (13,))])
def test_models_at_more_than_eight_frames(F, seeds):
    """reference against reference at m = 60: prints the distances MEASURED_FULLCOV records; both models are stationary, stay
    inside the bounds derived from the record and agree in the cost to 1e-9 relative"""
    worst = dict.fromkeys(MEASURED_FULLCOV, 0.0)
    for seed in seeds:
        pb = fm.with_full_cov(bm.sparse_problem(seed, F, 60, lone_frame=F // 2, long_track=F == 24), seed)
        a, b = tw.model_solve_blocks(pb, full=True), tw.model_solve(pb, full=True)
        cost, d = _report("F = %d, m = 60, seed %d" % (F, seed), a, b)
        na, nb = fm.newton_step(pb, a), fm.newton_step(pb, b)
        print("    newton step left: block model %.1e %.1e scipy %.1e %.1e" % (na[0], na[1], nb[0], nb[1]))
        assert cost <= 1e-9 and max(na[0], na[1]) < NEWTON
        for k, v in d.items():
            worst[k] = max(worst[k], v)
    print("worst at F = %d: %s" % (F, {k: "%.2e" % v for k, v in worst.items()}))
    for k in MEASURED_FULLCOV:
        assert worst[k] <= BOUND_FULLCOV[k], (k, worst[k])


def _problems():
    out = {"F = %d, m = %d" % c: (lambda c=c: fm.problem(*c)) for c in fm.CASES}
    out["asymmetric"] = lambda: fm.problem(9, 300, fm.ASYM)
    out["no point priors"] = fm.no_point_prior_problem
    return out


@pytest.mark.parametrize("name", list(_problems()))
def test_references_have_converged_and_the_problems_have_power(name):
    """every problem of the device tests that has full observation covariances: the block model is stationary to 1e-9, and a
    negated or zeroed off-diagonal moves its estimate beyond the device's bound and the cost at the guess by more than 1e-6
    relative; so does reducing the point priors to their diagonals (the estimate only: at the guess a prior costs nothing)"""
    pb = _problems()[name]()
    F = len(pb["poses"])
    bound = tw.BOUND if F <= 8 else BOUND_FULLCOV
    solve = lambda q: tw.model_solve_blocks(q, full=True)
    ref = solve(pb)
    dc, dp, cond = fm.newton_step(pb, ref)
    print("%s: newton step left %.1e %.1e, cond %.1e" % (name, dc, dp, cond))
    assert dc < NEWTON and dp < NEWTON
    for tag, factor in (("negated", -1.0), ("zeroed", 0.0)):
        assert _moved("%s, off-diagonals %s" % (name, tag), pb, ref, fm.off_diagonal(pb, factor), bound, solve) > 1e-6
    if pb["has_prior"].any():
        _moved("%s, priors' off-diagonals zeroed" % name, pb, ref, fm.prior_off_diagonal_dropped(pb), bound, solve)


def test_identity_covariance_reference_has_converged():
    pb = fm.unit_cov_problem(9, 40)
    ref = tw.model_solve_blocks(dict(pb, cov=[None] * 9), full=True)
    dc, dp, _ = fm.newton_step(pb, ref)
    print("newton step left %.1e %.1e" % (dc, dp))
    assert dc < NEWTON and dp < NEWTON
    # None is the identity in the model
    assert ref["error"] == tw.model_solve_blocks(pb, full=True)["error"]


def test_covariances_are_full_and_asymmetric_input_is_averaged():
    """the generator delivers what the issue asks for: anisotropy up to 6 in the standard deviations, correlation coefficients of
    both signs up to 0.9 and beyond, a scale around sig^2; and the model reads an asymmetric matrix as its symmetric part"""
    c = fm.problem(9, 300)["csr"]["obs_cov"]
    rho = c[:, 1] / np.sqrt(c[:, 0] * c[:, 3])
    ev = np.linalg.eigvalsh(c.reshape(-1, 2, 2))
    print("rho %.3f .. %.3f, |rho| > 0.5: %d of %d (%d negative); axis ratio up to %.2f; median variance %.3f" % (
        rho.min(), rho.max(), (np.abs(rho) > 0.5).sum(), len(rho), (rho < -0.5).sum(), np.sqrt(ev[:, 1] / ev[:, 0]).max(),
        np.median(ev)))
    assert np.array_equal(c[:, 1], c[:, 2]) and ev.min() > 0
    assert rho.min() < -0.85 and rho.max() > 0.85 and (rho < -0.5).sum() > 100 and (rho > 0.5).sum() > 100
    assert 5.0 < np.sqrt(ev[:, 1] / ev[:, 0]).max() <= 6.0 and 0.25 * 0.25 < np.median(ev) < 4 * 0.25
    assert len(np.unique(c, axis=0)) == len(c)
    pa = fm.problem(9, 300, fm.ASYM)
    ps = fm.symmetrised(pa)
    ca = pa["csr"]["obs_cov"]
    assert np.median(np.abs(ca[:, 1] - ca[:, 2]) / np.abs(ps["csr"]["obs_cov"][:, 1])) > 0.01
    a, s = (tw.model_blocks(q, *rm._guess(q), full=True) for q in (pa, ps))
    assert all(np.array_equal(x, y) for x, y in zip(a, s))


# ---- under a loss --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_a_fresh():
    return {kind: rm.solve_irls(fm.outlier_problem(kind)[0], kind, rm.K_OF[kind], full=True) for kind in (rm.HUBER, rm.CAUCHY)}


@pytest.mark.parametrize("kind", [rm.HUBER, rm.CAUCHY])
def test_model_a_reproduces_its_record_and_has_converged(model_a_fresh, kind):
    pb, _ = fm.outlier_problem(kind)
    a, rec = model_a_fresh[kind], fm.model_a(kind)
    assert a["iterations"] < rm.LM["max_iterations"]
    assert a["iterations"] == int(rec["iterations"]) and a["rejected_steps"] == int(rec["rejected_steps"])
    for q in ("R", "t", "points", "pose_cov", "point_cov"):
        assert np.allclose(a[q], rec[q], rtol=1e-9, atol=1e-12), q
    assert abs(a["error"] - float(rec["error"])) <= 1e-12 * a["error"]
    dc, dp, _ = rm.newton_step(pb, rec, kind, rm.K_OF[kind], full=True)
    print("%s: %d iterations, newton step left: poses %.1e points %.1e" % (rm.NAMES[kind], a["iterations"], dc, dp))
    assert dc < NEWTON and dp < NEWTON


@pytest.mark.parametrize("kind", [rm.HUBER, rm.CAUCHY])
def test_robust_models_agree(kind):
    """model (A), the recorded IRLS estimate, against model (B), scipy on the rescaled whitened residuals: prints the distances
    MEASURED_FULLCOV_ROBUST records; the costs agree to 1e-9 relative"""
    pb, _ = fm.outlier_problem(kind)
    k = rm.K_OF[kind]
    a, b = fm.model_a(kind), rm.solve_scipy(pb, kind, k, full=True)
    cost, d = _report(rm.NAMES[kind], a, b)
    nb = rm.newton_step(pb, b, kind, k, full=True)
    print("    newton step left at (B): %.1e %.1e" % (nb[0], nb[1]))
    assert cost <= 1e-9
    assert abs(float(a["error_guess"]) - b["error_guess"]) <= 1e-12 * b["error_guess"]
    for q, v in d.items():
        assert v <= BOUND_FULLCOV_ROBUST[q], (q, v)


@pytest.mark.parametrize("kind", [rm.HUBER, rm.CAUCHY])
def test_robust_problem_has_power_and_separates_planted_from_clean(kind):
    pb, planted = fm.outlier_problem(kind)
    k = rm.K_OF[kind]
    a = fm.model_a(kind)
    solve = lambda q: rm.solve_irls(q, kind, k, full=True)
    for tag, factor in (("negated", -1.0), ("zeroed", 0.0)):
        other = fm.off_diagonal(pb, factor)
        d = bm.distances(solve(other), a)
        g = rm._guess(pb)
        c0, c1 = rm.robust_cost(pb, *g, kind, k, full=True), rm.robust_cost(other, *g, kind, k, full=True)
        print("%s, off-diagonals %s: cost at the guess %.2e %s" % (rm.NAMES[kind], tag, abs(c1 - c0) / c0, {q: "%.2e" % v for q, v in d.items()}))
        assert d["t"] > BOUND_FULLCOV_ROBUST["t"] or d["points"] > BOUND_FULLCOV_ROBUST["points"]
        assert abs(c1 - c0) > 1e-6 * c0
    s, w = rm.obs_stats(pb, a["R"], a["t"], a["points"], kind, k, full=True)
    print("%s: planted %d of %d, w planted max %.4f, w clean min %.4f" % (rm.NAMES[kind], planted.sum(), len(planted),
                                                                       w[planted].max(), w[~planted].min()))
    assert abs(planted.sum() / len(planted) - 0.05) < 0.01
    assert w[planted].max() < 0.5 * W_SPLIT_FULLCOV[kind] and 2.0 * W_SPLIT_FULLCOV[kind] < w[~planted].min()


def test_statistics_model_behind_the_camera_and_cost():
    """sum rho2(chi2) + priors is the robust cost with full covariances; behind its camera an observation has
    s = 4 fx^2 (W0 + 2 W1 + W2); chi2 computed from W equals the squared norm of the Cholesky-whitened residual"""
    from test_ba_robust_host import behind_fixture

    pb, _ = fm.outlier_problem(rm.NONE)
    Rs, ts, P = rm._guess(pb)
    for kind in (rm.NONE, rm.HUBER, rm.CAUCHY):
        k = rm.K_OF[kind]
        s, _ = rm.obs_stats(pb, Rs, ts, P, kind, k, full=True)
        priors = 2.0 * rm.robust_blocks(rm._prior_only(pb), Rs, ts, P, kind, k, full=True)[0]
        want = rm.robust_cost(pb, Rs, ts, P, kind, k, full=True)
        assert abs(0.5 * (np.sum(rm.loss(s, kind, k)[1]) + priors) - want) <= 1e-12 * want
    P2, o = behind_fixture(pb)
    s, _ = rm.obs_stats(pb, Rs, ts, P2, full=True)
    C = pb["csr"]["obs_cov"][o].reshape(2, 2)
    W = np.linalg.inv(C)
    want = 4.0 * pb["K"][0, 0] ** 2 * (W[0, 0] + 2.0 * W[0, 1] + W[1, 1])
    assert abs(s[o] - want) <= 1e-12 * want and abs(W[0, 1]) > 0.05 * np.sqrt(W[0, 0] * W[1, 1])
