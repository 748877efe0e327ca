"""Robust losses of the sparse bundle adjustment on the device (mvs_ctx_set_ba_loss, mvs_ba_sparse_obs_stats; DESIGN.md section
4.7.6) through the C ABI.  Plumbing: Huber at k = 1e30 has w = 1 and rho2 = s exactly, so every output byte is that of
MVS_BA_LOSS_NONE.  Statistics against tests/ba_robust_model.py: |d chi2| <= 1e-9 max(1, chi2) (residuals carry a few ulp of
10^3 px and W <= 4, so d s ~ 4 x 1e-12; generous on purpose), |d w| <= 1e-9, and the planted / clean separation
test_ba_robust_host read off the model, for every observation.  The Gaussian estimate is further from the generator's truth
than the robust ones by at least half the margin the model shows.  The estimate, the covariances and the cost are held to
model (A) within ten times the model-to-model distances of test_ba_robust_host (BOUND_ROBUST), the cost to 1e-9 relative.  Iteration counts are not asserted: near the minimum the
IRLS accept / reject decision is the rounding's (section 4.10.5)."""
import contextlib

import numpy as np
import pytest

import ba_robust_model as rm
import ba_sparse_model as bm
import test_ba_sparse as ts
from test_ba_robust_host import BOUND_ROBUST, OFFSET_MARGIN, W_SPLIT, behind_fixture


@contextlib.contextmanager
def ba_loss(ctx, kind, k=1.0):
    from mvslam_amd import capi

    ctx.set_ba_loss(kind, k)
    try:
        yield
    finally:
        ctx.set_ba_loss(capi.MVS_BA_LOSS_NONE)


def _params():
    from mvslam_amd import capi

    return capi.default_refine_params(**rm.LM)


def _poses(sol):
    return np.concatenate([np.asarray(sol["R"]).reshape(-1, 9), np.asarray(sol["t"]).reshape(-1, 3)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("F,m", [(24, 300), (3, 12)])
def test_gpu_huber_at_1e30_returns_the_bytes_of_none(ctx, F, m):
    """about a thousand observations (the per-observation kernels cross a workgroup) and fewer than one wavefront; and NONE
    after a loss returns the bytes of NONE"""
    from mvslam_amd import capi

    pb = ts._wide(24)[0] if F == 24 else ts._small(3, 12)[0]
    args = bm.sparse_args(pb)
    none = ctx.ba_refine_sparse(**args)
    n_obs = len(pb["csr"]["obs_frame"])
    assert none["ok"] and (n_obs > 256 if F == 24 else n_obs < 64)
    with ba_loss(ctx, capi.MVS_BA_LOSS_HUBER, 1e30):
        big = ctx.ba_refine_sparse(**args)
    assert big["raw"] == none["raw"]
    with ba_loss(ctx, capi.MVS_BA_LOSS_CAUCHY, 2.0):
        other = ctx.ba_refine_sparse(**args)
    assert other["ok"] and other["raw"] != none["raw"]
    assert ctx.ba_refine_sparse(**args)["raw"] == none["raw"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [rm.NONE, rm.HUBER, rm.CAUCHY])
def test_gpu_robust_is_deterministic(ctx, kind):
    pb, _ = rm.outlier_problem(9)
    args = bm.sparse_args(pb)
    with ba_loss(ctx, kind, rm.K_OF[kind]):
        a, b = ctx.ba_refine_sparse(**args), ctx.ba_refine_sparse(**args)
        sa, sb = ctx.ba_sparse_obs_stats(**args), ctx.ba_sparse_obs_stats(**args)
    assert a["ok"] and a["raw"] == b["raw"]
    assert sa[0] == 0 and sa[1].tobytes() == sb[1].tobytes() and sa[2].tobytes() == sb[2].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [9, 24])
@pytest.mark.parametrize("kind", [rm.HUBER, rm.CAUCHY])
def test_gpu_robust_cost_at_the_guess_and_statistics(ctx, F, kind):
    """error_initial is the model's robust cost at the guess; the statistics at the guess reproduce it; at the model's
    estimate chi2 and weights are the model's and the weights separate planted from clean"""
    pb, planted = rm.outlier_problem(F)
    k, args = rm.K_OF[kind], bm.sparse_args(pb)
    Rs, tt, P = rm._guess(pb)
    want0 = rm.robust_cost(pb, Rs, tt, P, kind, k)
    from mvslam_amd import capi

    with ba_loss(ctx, kind, k):
        got = ctx.ba_refine_sparse(params=capi.default_refine_params(max_iterations=0), pose_cov=False, point_cov=False, **args)
        st, chi2, w = ctx.ba_sparse_obs_stats(**args)
        a = rm.model_a(F, kind)
        st2, chi2e, we = ctx.ba_sparse_obs_stats(poses=_poses(a), points_at=a["points"], **args)
    print("error_initial %.12e model %.12e" % (got["error_initial"], want0))
    assert abs(got["error_initial"] - want0) <= 1e-9 * want0
    assert st == 0 and st2 == 0
    priors = 2.0 * rm.robust_blocks(rm._prior_only(pb), Rs, tt, P, kind, k)[0]
    assert abs(0.5 * (np.sum(rm.loss(chi2, kind, k)[1]) + priors) - got["error_initial"]) <= 1e-9 * got["error_initial"]
    for tag, (s_got, w_got), (s_want, w_want) in (("guess", (chi2, w), rm.obs_stats(pb, Rs, tt, P, kind, k)),
                                                  ("estimate", (chi2e, we), rm.obs_stats(pb, a["R"], a["t"], a["points"], kind, k))):
        ds, dw = np.abs(s_got - s_want) / np.maximum(1.0, s_want), np.abs(w_got - w_want)
        print("%s: chi2 %.2e weight %.2e" % (tag, ds.max(), dw.max()))
        assert ds.max() <= 1e-9 and dw.max() <= 1e-9
    print("w planted max %.4f clean min %.4f" % (we[planted].max(), we[~planted].min()))
    assert np.all(we[planted] < W_SPLIT[kind]) and np.all(we[~planted] > W_SPLIT[kind])


@pytest.mark.gpu
@pytest.mark.parametrize("F", [9, 24])
@pytest.mark.parametrize("kind", [rm.HUBER, rm.CAUCHY])
def test_gpu_robust_matches_model(ctx, F, kind):
    """the estimate, both covariances and the final cost against model (A) under the same LM parameters: ten times the model-
    to-model distances test_ba_robust_host records, the cost to 1e-9 relative"""
    pb, _ = rm.outlier_problem(F)
    want = rm.model_a(F, kind)
    with ba_loss(ctx, kind, rm.K_OF[kind]):
        got = ctx.ba_refine_sparse(params=_params(), **bm.sparse_args(pb))
    assert got["status"] == 0 and got["ok"] and got["failed_solves"] == 0
    cost = abs(got["error"] - float(want["error"])) / float(want["error"])
    d = bm.distances(got, want)
    print("F = %d %s: %d iterations (%d rejected; model %d, %d), cost %.2e %s" % (
        F, rm.NAMES[kind], got["iterations"], got["rejected_steps"], int(want["iterations"]), int(want["rejected_steps"]), cost,
        {q: "%.2e" % v for q, v in d.items()}))
    assert abs(got["error_initial"] - float(want["error_guess"])) <= 1e-9 * float(want["error_guess"])
    assert cost <= 1e-9
    for q, v in d.items():
        assert v <= BOUND_ROBUST[q], (q, v, BOUND_ROBUST[q])


@pytest.mark.gpu
def test_gpu_statistics_without_a_loss_and_behind_the_camera(ctx):
    pb, _ = rm.outlier_problem(9)
    args = bm.sparse_args(pb)
    P2, o = behind_fixture(pb)
    st, chi2, w = ctx.ba_sparse_obs_stats(points_at=P2, **args)
    want, _ = rm.obs_stats(pb, *rm._guess(pb)[:2], P2)
    assert st == 0 and np.array_equal(w, np.ones(len(w)))
    assert np.isfinite(chi2[o]) and chi2[o] == 2.0 * (2.0 * pb["K"][0, 0]) ** 2 * (1.0 / pb["sig"] ** 2)
    assert np.all(np.abs(chi2 - want) <= 1e-9 * np.maximum(1.0, want))
    st, chi2n, wn = ctx.ba_sparse_obs_stats(weight=False, **args)
    assert st == 0 and wn is None and chi2n.tobytes() == ctx.ba_sparse_obs_stats(**args)[1].tobytes()


@pytest.mark.gpu
def test_gpu_gaussian_estimate_is_further_from_the_truth(ctx):
    """F = 9: without a loss the planted observations drag the estimate; half the model's margin is demanded"""
    pb, planted = rm.outlier_problem(9)
    args, d = bm.sparse_args(pb), {}
    for kind in (rm.NONE, rm.HUBER, rm.CAUCHY):
        with ba_loss(ctx, kind, rm.K_OF[kind]):
            got = ctx.ba_refine_sparse(params=_params(), **args)
            assert got["ok"] and got["error"] <= got["error_initial"]
            d[kind] = rm.truth_distance(pb, got)
            if kind != rm.NONE:   # the estimate's own weights separate planted from clean as well
                st, _, w = ctx.ba_sparse_obs_stats(poses=_poses(got), points_at=got["points"], **args)
                assert st == 0 and np.all(w[planted] < W_SPLIT[kind]) and np.all(w[~planted] > W_SPLIT[kind])
    print({rm.NAMES[k]: "%.3f" % v for k, v in d.items()})
    assert d[rm.NONE] - max(d[rm.HUBER], d[rm.CAUCHY]) >= 0.5 * OFFSET_MARGIN


@pytest.mark.gpu
def test_gpu_ba_loss_refusals(ctx):
    from mvslam_amd import capi

    pb, _ = rm.outlier_problem(9)
    args = bm.sparse_args(pb)
    with ba_loss(ctx, capi.MVS_BA_LOSS_CAUCHY, 2.0):
        kept = ctx.ba_refine_sparse(pose_cov=False, point_cov=False, **args)["raw"]
        for bad in ((3, 1.0), (-1, 1.0), (capi.MVS_BA_LOSS_HUBER, 0.0), (capi.MVS_BA_LOSS_HUBER, -1.0),
                    (capi.MVS_BA_LOSS_CAUCHY, float("nan")), (capi.MVS_BA_LOSS_CAUCHY, float("inf"))):
            with pytest.raises(capi.MvsError) as e:
                ctx.set_ba_loss(*bad)
            assert e.value.status == capi.MVS_ERR_INVALID_ARG
        assert ctx.ba_refine_sparse(pose_cov=False, point_cov=False, **args)["raw"] == kept   # the earlier setting is kept
    # the statistics call refuses what mvs_ba_refine_sparse refuses, with nothing written
    fr = pb["csr"]["obs_frame"].copy()
    k = int(np.flatnonzero(np.diff(pb["csr"]["obs_off"]) >= 2)[0])
    o = pb["csr"]["obs_off"][k]
    fr[o], fr[o + 1] = fr[o + 1], fr[o]
    off = pb["csr"]["obs_off"].copy()
    off[-1] -= 1
    uv = pb["csr"]["obs_uv"].copy()
    uv[3, 1] = np.nan
    for kw, want in ((dict(obs_frame=fr), capi.MVS_ERR_INVALID_ARG), (dict(obs_off=off), capi.MVS_ERR_INVALID_ARG),
                     (dict(obs_uv=uv), capi.MVS_ERR_INVALID_ARG), (dict(n_frames=4097), capi.MVS_ERR_CAPACITY)):
        a = dict(args)
        a.update(kw)
        st, chi2, w = ctx.ba_sparse_obs_stats(**a)
        assert st == want and not chi2.any() and not w.any(), kw
    import ctypes as C

    chi2 = np.zeros(4)
    lib = capi.lib()
    assert lib.mvs_ba_sparse_obs_stats(ctx._h, None, None, None, chi2.ctypes.data_as(C.POINTER(C.c_double)), None) == capi.MVS_ERR_INVALID_ARG
    pbs, _keep, _, _, _ = capi._ba_sparse_problem(n_frames=None, **args)
    assert lib.mvs_ba_sparse_obs_stats(ctx._h, C.byref(pbs), None, None, None, None) == capi.MVS_ERR_INVALID_ARG
    pbs.obs_uv = None
    assert lib.mvs_ba_sparse_obs_stats(ctx._h, C.byref(pbs), None, None, chi2.ctypes.data_as(C.POINTER(C.c_double)), None) == capi.MVS_ERR_INVALID_ARG
    assert not chi2.any()


@pytest.mark.gpu
def test_gpu_window_calls_ignore_the_ba_loss(ctx):
    from mvslam_amd import capi

    pb, _ = ts._small(8, 300)
    none = ctx.ba_refine_windows([bm.as_window(pb)])[0]
    with ba_loss(ctx, capi.MVS_BA_LOSS_CAUCHY, rm.CAUCHY_K):
        got = ctx.ba_refine_windows([bm.as_window(pb)])[0]
    assert none["ok"] and got["raw"] == none["raw"] and got["points"].tobytes() == none["points"].tobytes()
    assert got["point_cov"].tobytes() == none["point_cov"].tobytes()
