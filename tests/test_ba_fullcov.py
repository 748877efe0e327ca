"""Sparse bundle adjustment with full covariances on the device: mvs_ba_refine_sparse and mvs_ba_sparse_obs_stats (DESIGN.md
sections 4.7.4 and 4.7.6) through the C ABI on tests/ba_fullcov_model.py's problems, where every observation has its own full
2 x 2 covariance and every point prior a full 3 x 3 one, so that the off-diagonal information entry W1 takes part in the cost,
the point elimination, the camera blocks, the gradient, the statistics and the IRLS product w W1 -- and where
tests/test_ba_fullcov_host.py has shown that a negated or a dropped off-diagonal moves the estimate by far more than the bounds.

Bounds (test_ba_fullcov_host.py measures and derives them; none comes from a device result).  F <= 8: test_ba_window.BOUND, for
the sparse entry and the window kernel on the same problem.  F > 8 without a loss: BOUND_FULLCOV.  Under a loss:
BOUND_FULLCOV_ROBUST, against model (A).  The cost agrees to 1e-9 relative everywhere.  Statistics: test_ba_robust's tolerances,
|d chi2| <= 1e-9 max(1, chi2) and |d w| <= 1e-9.  NULL covariance arrays and asymmetric input are held to byte equality with
their explicit counterparts.
"""
import numpy as np
import pytest

import ba_fullcov_model as fm
import ba_robust_model as rm
import ba_sparse_model as bm
import test_ba_window as tw
from test_ba_fullcov_host import BOUND_FULLCOV, BOUND_FULLCOV_ROBUST, W_SPLIT_FULLCOV
from test_ba_robust import _params, _poses, ba_loss
from test_ba_robust_host import behind_fixture
from test_ba_sparse import _compare


def _bound(F):
    return tw.BOUND if F <= 8 else BOUND_FULLCOV


@pytest.mark.gpu
@pytest.mark.parametrize("F,m", fm.CASES)
def test_gpu_sparse_full_covariances_match_the_model(ctx, F, m):
    """estimate, cost, cost at the guess and both covariances against the block model; up to eight frames the window kernel on
    the same problem against the same model: two device implementations, one reference"""
    pb, want = fm.problem(F, m), fm.solution(F, m)
    got = ctx.ba_refine_sparse(**bm.sparse_args(pb))
    assert got["status"] == 0 and got["ok"] and got["bad_frame"] == -1 and got["failed_solves"] == 0
    print("error_initial %.12e model %.12e" % (got["error_initial"], want["error_guess"]))
    assert abs(got["error_initial"] - want["error_guess"]) <= 1e-9 * want["error_guess"]
    assert F != 24 or got["widest_row"] == F
    _compare("sparse, full covariances, F = %d, m = %d" % (F, m), got, want, _bound(F))
    if F <= 8:
        win = ctx.ba_refine_windows([bm.as_window(pb)])[0]
        assert win["ok"]
        _compare("window, full covariances, F = %d, m = %d" % (F, m), win, want, _bound(F))


@pytest.mark.gpu
def test_gpu_sparse_asymmetric_off_diagonals_are_averaged(ctx):
    """off-diagonal entries a few per cent apart, in the observation covariances and the point priors, give the bytes of
    their averages"""
    pa = fm.problem(9, 300, fm.ASYM)
    ps = fm.symmetrised(pa)
    ca, cs = pa["csr"]["obs_cov"], ps["csr"]["obs_cov"]
    assert np.median(np.abs(ca[:, 1] - ca[:, 2]) / np.abs(cs[:, 1])) > 0.01 and np.array_equal(cs[:, 1], cs[:, 2])
    assert np.abs(pa["pcov"][:, 1] - pa["pcov"][:, 3]).max() > 0.01 * np.abs(ps["pcov"][:, 1]).max()
    a, s = ctx.ba_refine_sparse(**bm.sparse_args(pa)), ctx.ba_refine_sparse(**bm.sparse_args(ps))
    assert a["ok"] and a["raw"] == s["raw"]
    sa, ss = ctx.ba_sparse_obs_stats(**bm.sparse_args(pa)), ctx.ba_sparse_obs_stats(**bm.sparse_args(ps))
    assert sa[0] == 0 and sa[1].tobytes() == ss[1].tobytes()
    _compare("asymmetric input", a, bm.solve_blocks(ps, full=True), BOUND_FULLCOV)


@pytest.mark.gpu
def test_gpu_sparse_without_observation_covariances_is_identity(ctx):
    """obs_cov = NULL: the bytes of an explicit array of identities, in the solve (F = 9, also against the model) and in the
    statistics (F = 3, also against numpy)"""
    pb = fm.unit_cov_problem(9, 40)
    args = bm.sparse_args(pb)
    assert np.array_equal(args["obs_cov"], np.tile([1.0, 0.0, 0.0, 1.0], (len(args["obs_cov"]), 1)))
    explicit = ctx.ba_refine_sparse(**args)
    null = ctx.ba_refine_sparse(**dict(args, obs_cov=None))
    assert explicit["ok"] and null["raw"] == explicit["raw"]
    _compare("obs_cov = NULL", null, bm.solve_blocks(dict(pb, cov=[None] * 9), full=True), BOUND_FULLCOV)
    pb = fm.unit_cov_problem(3, 12)
    args = bm.sparse_args(pb)
    st, chi2, w = ctx.ba_sparse_obs_stats(**args)
    st2, chi2n, wn = ctx.ba_sparse_obs_stats(**dict(args, obs_cov=None))
    assert st == 0 and st2 == 0 and chi2n.tobytes() == chi2.tobytes() and wn.tobytes() == w.tobytes()
    want, _ = rm.obs_stats(dict(pb, cov=[None] * 3), *rm._guess(pb), full=True)
    assert want.min() > 0 and np.all(np.abs(chi2n - want) <= 1e-9 * np.maximum(1.0, want))


@pytest.mark.gpu
def test_gpu_sparse_without_point_priors(ctx):
    """point_prior_cov = NULL, rows of zeros, and rows whose first entry is <= 0 whatever else they hold: no prior on any
    point, the same bytes, and the model's estimate with the gauge held by the frame priors alone; the statistics take
    NULL beside real observations"""
    pb = fm.no_point_prior_problem()
    args = bm.sparse_args(pb)
    assert not args["point_prior_cov"].any() and np.diff(args["obs_off"]).min() >= 2
    zeros = ctx.ba_refine_sparse(**args)
    null = ctx.ba_refine_sparse(**dict(args, point_prior_cov=None))
    junk = np.random.default_rng(0).uniform(0.5, 2.0, args["point_prior_cov"].shape)
    junk[::2, 0], junk[1::2, 0] = 0.0, -1.0
    nonpos = ctx.ba_refine_sparse(**dict(args, point_prior_cov=junk))
    assert zeros["status"] == 0 and zeros["ok"] and null["raw"] == zeros["raw"] and nonpos["raw"] == zeros["raw"]
    _compare("no point priors", null, bm.solve_blocks(dict(pb, pcov=None), full=True), BOUND_FULLCOV)
    st, chi2, _ = ctx.ba_sparse_obs_stats(**dict(args, point_prior_cov=None))
    want, _ = rm.obs_stats(pb, *rm._guess(pb), full=True)
    assert st == 0 and chi2.tobytes() == ctx.ba_sparse_obs_stats(**args)[1].tobytes()
    assert np.all(np.abs(chi2 - want) <= 1e-9 * np.maximum(1.0, want))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [rm.NONE, rm.HUBER, rm.CAUCHY])
def test_gpu_statistics_with_full_covariances(ctx, kind):
    """chi2 = r^T W r and w(chi2) at the guess, at an estimate, and with a point behind one of its cameras, whose fixed
    residual (2 fx, 2 fx) meets the whole of W: s = 4 fx^2 (W0 + 2 W1 + W2); under a loss the robust cost at the guess"""
    from mvslam_amd import capi

    pb, planted = fm.outlier_problem(kind)
    k, args = rm.K_OF[kind], bm.sparse_args(pb)
    Rs, tt, P = rm._guess(pb)
    a = fm.model_a(rm.HUBER if kind == rm.NONE else kind)
    P2, o = behind_fixture(pb)
    with ba_loss(ctx, kind, k):
        got = ctx.ba_refine_sparse(params=capi.default_refine_params(max_iterations=0), pose_cov=False, point_cov=False, **args)
        at_guess = ctx.ba_sparse_obs_stats(**args)
        at_estimate = ctx.ba_sparse_obs_stats(poses=_poses(a), points_at=a["points"], **args)
        behind = ctx.ba_sparse_obs_stats(points_at=P2, **args)
    want0 = rm.robust_cost(pb, Rs, tt, P, kind, k, full=True)
    print("error_initial %.12e model %.12e" % (got["error_initial"], want0))
    assert abs(got["error_initial"] - want0) <= 1e-9 * want0
    priors = 2.0 * rm.robust_blocks(rm._prior_only(pb), Rs, tt, P, kind, k, full=True)[0]
    assert abs(0.5 * (np.sum(rm.loss(at_guess[1], kind, k)[1]) + priors) - got["error_initial"]) <= 1e-9 * got["error_initial"]
    for tag, (st, s_got, w_got), (s_want, w_want) in (
            ("guess", at_guess, rm.obs_stats(pb, Rs, tt, P, kind, k, full=True)),
            ("estimate", at_estimate, rm.obs_stats(pb, a["R"], a["t"], a["points"], kind, k, full=True)),
            ("behind", behind, rm.obs_stats(pb, Rs, tt, P2, kind, k, full=True))):
        ds, dw = np.abs(s_got - s_want) / np.maximum(1.0, s_want), np.abs(w_got - w_want)
        print("%s %s: chi2 %.2e weight %.2e" % (rm.NAMES[kind], tag, ds.max(), dw.max()))
        assert st == 0 and ds.max() <= 1e-9 and dw.max() <= 1e-9
    C = pb["csr"]["obs_cov"][o].reshape(2, 2)
    W = np.linalg.inv(0.5 * (C + C.T))
    s_o = 4.0 * pb["K"][0, 0] ** 2 * (W[0, 0] + 2.0 * W[0, 1] + W[1, 1])
    assert abs(W[0, 1]) > 0.05 * np.sqrt(W[0, 0] * W[1, 1])   # this observation's W1 counts
    assert np.isfinite(behind[1][o]) and abs(behind[1][o] - s_o) <= 1e-9 * s_o
    if kind == rm.NONE:
        assert np.array_equal(at_guess[2], np.ones(len(planted)))
    else:
        we = at_estimate[2]
        print("w planted max %.4f clean min %.4f" % (we[planted].max(), we[~planted].min()))
        assert np.all(we[planted] < W_SPLIT_FULLCOV[kind]) and np.all(we[~planted] > W_SPLIT_FULLCOV[kind])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [rm.HUBER, rm.CAUCHY])
def test_gpu_robust_full_covariances_match_model(ctx, kind):
    """F = 9 with planted outliers: estimate, robust cost and the covariances of the reweighted system against model (A) under
    the same LM parameters; the estimate's own weights separate the planted observations from the clean ones"""
    pb, planted = fm.outlier_problem(kind)
    want, args = fm.model_a(kind), bm.sparse_args(pb)
    with ba_loss(ctx, kind, rm.K_OF[kind]):
        got = ctx.ba_refine_sparse(params=_params(), **args)
        st, _, w = ctx.ba_sparse_obs_stats(poses=_poses(got), points_at=got["points"], **args)
    assert got["status"] == 0 and got["ok"] and got["failed_solves"] == 0
    cost = abs(got["error"] - float(want["error"])) / float(want["error"])
    d = bm.distances(got, want)
    print("%s: %d iterations (%d rejected; model %d, %d), cost %.2e %s" % (
        rm.NAMES[kind], got["iterations"], got["rejected_steps"], int(want["iterations"]), int(want["rejected_steps"]), cost,
        {q: "%.2e" % v for q, v in d.items()}))
    assert abs(got["error_initial"] - float(want["error_guess"])) <= 1e-9 * float(want["error_guess"])
    assert cost <= 1e-9
    for q, v in d.items():
        assert v <= BOUND_FULLCOV_ROBUST[q], (q, v, BOUND_FULLCOV_ROBUST[q])
    assert st == 0 and np.all(w[planted] < W_SPLIT_FULLCOV[kind]) and np.all(w[~planted] > W_SPLIT_FULLCOV[kind])


@pytest.mark.gpu
def test_gpu_huber_at_1e30_returns_the_bytes_of_none_with_full_covariances(ctx):
    """w = 1 exactly: the IRLS product w W is W in all three entries"""
    from mvslam_amd import capi

    args = bm.sparse_args(fm.problem(9, 300))
    none = ctx.ba_refine_sparse(**args)
    with ba_loss(ctx, capi.MVS_BA_LOSS_HUBER, 1e30):
        big = ctx.ba_refine_sparse(**args)
    assert none["ok"] and big["raw"] == none["raw"]
    with ba_loss(ctx, capi.MVS_BA_LOSS_HUBER, rm.HUBER_K):
        assert ctx.ba_refine_sparse(**args)["raw"] != none["raw"]


@pytest.mark.gpu
def test_gpu_sparse_full_covariances_are_deterministic(ctx):
    args = bm.sparse_args(fm.problem(24, 300))
    a, b = ctx.ba_refine_sparse(**args), ctx.ba_refine_sparse(**args)
    assert a["ok"] and a["raw"] == b["raw"]
