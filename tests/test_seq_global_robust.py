"""The global bundle adjustment of a resident sequence under the robust losses (mvs_ctx_set_ba_loss, mvs_seq_global_obs_stats;
DESIGN.md section 4.7.6): test_seq_global's 6 frames of 300 keypoints at T = 0 and T = 3.  Record, poses, points and both
covariances of mvs_seq_refine_global equal Context.ba_refine_sparse under the same loss on the problem rebuilt from the
download, byte for byte; the resident statistics equal mvs_ba_sparse_obs_stats on that problem and the downloaded estimate;
Huber at k = 1e30 equals MVS_BA_LOSS_NONE; mvs_seq_refine_windows does not see the switch."""
import numpy as np
import pytest

import ba_robust_model as rm
import seq_global_model as gm
import test_seq_global as sg
import test_seq_windows as sw
from test_ba_robust import ba_loss
from test_seq_global import resident  # noqa: F401  (the module's fixture: the sequence, run once)


def _global_bytes(s, res):
    return s.download_global()["raw"] + res["raw"]


def _check_stats(ctx, s, dev, got, params, sigma_px, kind):
    out = s.download_global()
    chi2, w = s.global_obs_stats()
    args = gm.sparse_args(got, dev["traj"], dev["kp"], dev["octave"], dev["K"], params, sigma_px)
    args.pop("params")
    poses = np.concatenate([out["R"].reshape(-1, 9), out["t"]], axis=1)
    st, chi2h, wh = ctx.ba_sparse_obs_stats(poses=poses, points_at=out["points"], **args)
    assert st == 0 and len(chi2) == s.global_counts()[1]
    assert chi2.tobytes() == chi2h.tobytes() and w.tobytes() == wh.tobytes()
    assert np.all(np.isfinite(chi2)) and np.all(chi2 >= 0.0)
    if kind == rm.NONE:
        assert np.array_equal(w, np.ones(len(w)))
    else:
        assert np.allclose(w, rm.loss(chi2, kind, rm.K_OF[kind])[0], rtol=0, atol=1e-12) and w.min() < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("T", [0, 3])
def test_gpu_seq_global_under_a_loss_equals_the_host_route(ctx, resident, T):  # noqa: F811
    from mvslam_amd import capi

    s, dev, _ = resident
    params = capi.default_refine_params()
    none = s.refine_global(T, params, 0.5)
    none_bytes = _global_bytes(s, none)
    got = s.download_global_problem()
    _check_stats(ctx, s, dev, got, params, 0.5, rm.NONE)
    for kind in (rm.HUBER, rm.CAUCHY):
        with ba_loss(ctx, kind, rm.K_OF[kind]):
            res = s.refine_global(T, params, 0.5)
            sg._check_solve(ctx, s, dev, got, res, params, 0.5)
            _check_stats(ctx, s, dev, got, params, 0.5, kind)
            assert _global_bytes(s, res) != none_bytes
    with ba_loss(ctx, rm.HUBER, 1e30):
        res = s.refine_global(T, params, 0.5)
        assert _global_bytes(s, res) == none_bytes
    assert _global_bytes(s, s.refine_global(T, params, 0.5)) == none_bytes


@pytest.mark.gpu
def test_gpu_seq_global_under_a_loss_after_the_essential_run(ctx, resident):  # noqa: F811
    from mvslam_amd import capi

    _, _, seq = resident
    F, N = seq["kp"].shape[0], seq["kp"].shape[1]
    s = capi.Sequence(ctx, F, N, 32)
    try:
        s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
        s.run_essential(capi.default_params(num_hypotheses=sw.PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=sw.PRM["seed"],
                                            max_error_sq=sw.PRM["thr"]),
                        capi.default_pnp_params(num_hypotheses=sw.PPRM["H"], seed=sw.PPRM["seed"], reproj_error=sw.PPRM["err"]))
        dev = dict(traj=s.download_trajectory(), kp=seq["kp"], octave=np.zeros((F, N), np.uint8), K=seq["K"])
        params = capi.default_refine_params()
        none = s.refine_global(0, params, 0.7)
        none_bytes = _global_bytes(s, none)
        got = s.download_global_problem()
        for kind in (rm.HUBER, rm.CAUCHY):
            with ba_loss(ctx, kind, rm.K_OF[kind]):
                res = s.refine_global(0, params, 0.7)
                sg._check_solve(ctx, s, dev, got, res, params, 0.7)
                _check_stats(ctx, s, dev, got, params, 0.7, kind)
        with ba_loss(ctx, rm.HUBER, 1e30):
            assert _global_bytes(s, s.refine_global(0, params, 0.7)) == none_bytes
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_seq_global_obs_stats_refusals(ctx, resident):  # noqa: F811
    """before any global call on the run, after a run that invalidated it, and after a call that ended ok = 0"""
    from mvslam_amd import capi

    _, _, seq = resident
    s, _dev = sw._run(ctx, seq)
    try:
        def refused():
            with pytest.raises(capi.MvsError) as e:
                s.global_obs_stats()
            return e.value.status == capi.MVS_ERR_INVALID_ARG

        assert refused()                                   # no global call yet
        assert s.refine_global(0)["ok"]
        chi2, w = s.global_obs_stats()
        assert len(chi2) == s.global_counts()[1] and np.array_equal(w, np.ones(len(w)))
        s.run(capi.default_params(num_hypotheses=sw.PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=sw.PRM["seed"],
                                  max_error_sq=sw.PRM["thr"]),
              capi.default_pnp_params(num_hypotheses=sw.PPRM["H"], seed=sw.PPRM["seed"], reproj_error=sw.PPRM["err"]))
        assert refused()                                   # the run invalidated it
    finally:
        s.close()
    # no frame has eight keypoints: no point, the global call ends with MVS_NO_MODEL and ok = 0
    s, _dev = sw._run(ctx, seq, n_kp=np.full(6, 4, np.int32))
    try:
        res = s.refine_global(0)
        assert res["status"] == capi.MVS_NO_MODEL and not res["ok"]
        assert refused()
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_seq_refine_windows_ignores_the_ba_loss(ctx, resident):  # noqa: F811
    s, _, _ = resident
    s.refine_windows(4, 1, 512)
    none = b"".join(w["raw"] + w["points"].tobytes() + w["point_cov"].tobytes() for w in s.download_windows())
    with ba_loss(ctx, rm.CAUCHY, rm.CAUCHY_K):
        s.refine_windows(4, 1, 512)
        got = b"".join(w["raw"] + w["points"].tobytes() + w["point_cov"].tobytes() for w in s.download_windows())
    assert len(none) > 0 and got == none
