"""Sparse bundle adjustment of up to 4096 frames on the device: mvs_ba_refine_sparse through the C ABI
against the reference models of tests/ba_sparse_model.py.

Bounds.  F <= 8: section 4.7's (test_ba_window.BOUND: 4.4e-9 rotation, 3.7e-8 translation, 7.6e-7 points, 5.0e-8 / 5.7e-7
relative covariances), for the sparse entry AND the window path on the same problem.  F > 8: ten times the model-to-model
distances tests/test_ba_sparse_host.py measured on this generator (BOUND_WIDE: 6.5e-9, 4.7e-8, 9.4e-7, 8.4e-8, 2.8e-7).  The
cost agrees to 1e-9 relative everywhere.  Every reference is computed once per module and shared.
"""
import functools
import json
import os

import numpy as np
import pytest

import ba_sparse_model as bm
import test_ba_window as tw
from test_ba_sparse_host import BOUND_WIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = [(3, 12), (3, 300), (8, 12), (8, 300)]
WIDE = [9, 24, 40]


@functools.lru_cache(maxsize=None)
def _small(F, m):
    pb = bm.sparse_problem(10 * F + (m > 12), F, m, max_track=F)
    return pb, bm.solve_blocks(pb)


# Seeds of the F > 8 problems.  The block model's own convergence was checked on the CPU (bm.newton_step: the Newton step that
# is left at the model's estimate): 2 .. 5 observations hold some points weakly, and the model's remaining step in the points was
# 3.4e-9 (seed 40), 1.7e-10 (41), 7.0e-9 (42), 8.9e-9 (43), 1.0e-8 (44) at F = 40; 41, the smallest, is used.
WIDE_SEED = {9: 9, 24: 24, 40: 41}


@functools.lru_cache(maxsize=None)
def _wide(F):
    """m = 300, tracks of 2 .. 5 frames, a point with one observation and a prior, a frame held only by its prior, and at
    F = 24 one track over frames 0 and F - 1"""
    pb = bm.sparse_problem(WIDE_SEED[F], F, 300, lone_frame=F // 2, long_track=F == 24)
    return pb, bm.solve_blocks(pb)


def _compare(tag, got, want, bound):
    cost = abs(got["error"] - want["error"]) / want["error"]
    d = bm.distances(got, want)
    print("%s: cost %.2e %s" % (tag, cost, {k: "%.2e" % v for k, v in d.items()}))
    assert cost <= 1e-9, (tag, cost)
    for k, v in d.items():
        assert v <= bound[k], (tag, k, v, bound[k])


@pytest.mark.gpu
@pytest.mark.parametrize("F,m", SMALL)
def test_gpu_sparse_and_window_agree_with_the_model(ctx, F, m):
    """up to eight frames: the sparse entry and mvs_ba_refine_window on the same problem, each against the model (their bytes
    differ: the summation orders do)"""
    pb, want = _small(F, m)
    got = ctx.ba_refine_sparse(**bm.sparse_args(pb))
    assert got["status"] == 0 and got["ok"] and got["bad_frame"] == -1
    assert abs(got["error_initial"] - want["error_guess"]) <= 1e-9 * want["error_guess"]
    _compare("sparse F = %d, m = %d" % (F, m), got, want, tw.BOUND)
    win = ctx.ba_refine_windows([bm.as_window(pb)])[0]
    assert win["ok"]
    _compare("window F = %d, m = %d" % (F, m), win, want, tw.BOUND)


@pytest.mark.gpu
@pytest.mark.parametrize("F", WIDE)
def test_gpu_sparse_matches_block_model_beyond_eight_frames(ctx, F):
    pb, want = _wide(F)
    got = ctx.ba_refine_sparse(**bm.sparse_args(pb))
    assert got["status"] == 0 and got["ok"]
    first, _, _ = bm.brute_plan(F, pb["csr"]["obs_off"], pb["csr"]["obs_frame"])
    assert got["envelope_blocks"] == sum(i - first[i] + 1 for i in range(F))
    assert got["widest_row"] == max(i - first[i] + 1 for i in range(F)) and (F != 24 or got["widest_row"] == F)
    assert F != 40 or first[F - 1] > 0   # rows whose envelope does not start at 0
    _compare("sparse F = %d, m = 300" % F, got, want, BOUND_WIDE)


@pytest.mark.gpu
def test_gpu_sparse_is_deterministic(ctx):
    pb, _ = _wide(24)
    a = ctx.ba_refine_sparse(**bm.sparse_args(pb))
    b = ctx.ba_refine_sparse(**bm.sparse_args(pb))
    assert a["ok"] and a["raw"] == b["raw"]


@functools.lru_cache(maxsize=None)
def _overshoot():
    """a start from which a Gauss-Newton step overshoots: guesses 30 times further off, rotations by 0.6 rad (sigma), a prior
    on every point so that a point that lands behind a camera keeps a block the model can invert.  Checked on the CPU: the
    model runs from here and the Newton step left at its estimate is below 1e-9 (bm.newton_step)."""
    pb = bm.sparse_problem(9, 9, 300, lone_frame=4, far=30.0, rot_sig=2e-2, prior_frac=1.0)
    return pb, bm.solve_blocks(pb)


@pytest.mark.gpu
def test_gpu_sparse_rejected_steps_still_reach_the_minimum(ctx):
    """lambda_initial = 1e-12 on a badly perturbed start, default tolerances: steps overshoot and are rejected, lambda grows
    until a step is accepted again, and the estimate is the model's.  The trace is read from outside as test_refine_edges
    does: with max_iterations = k the call stops behind step k, and step k was rejected exactly when the error behind k equals
    the error behind k - 1.  A rejected step must be followed by an accepted one that lowers the cost."""
    from mvslam_amd import capi

    pb, want = _overshoot()
    args = bm.sparse_args(pb)
    got = ctx.ba_refine_sparse(params=capi.default_refine_params(lambda_initial=1e-12), **args)
    print("iterations %d rejected %d failed %d" % (got["iterations"], got["rejected_steps"], got["failed_solves"]))
    assert got["status"] == 0 and got["ok"] and got["rejected_steps"] > 0 and got["failed_solves"] == 0
    _compare("rejected steps", got, want, BOUND_WIDE)
    err = [got["error_initial"]]
    for k in range(1, got["iterations"] + 1):
        r = ctx.ba_refine_sparse(params=capi.default_refine_params(lambda_initial=1e-12, max_iterations=k), pose_cov=False,
                                 point_cov=False, **args)
        assert r["iterations"] == k
        err.append(r["error"])
        assert r["rejected_steps"] == sum(err[j] == err[j - 1] for j in range(1, k + 1))
    pattern = "".join("R" if err[k] == err[k - 1] else "A" for k in range(1, len(err)))
    print("trace", pattern)
    assert err[-1] == got["error"] and all(err[k] <= err[k - 1] for k in range(1, len(err)))
    first_r = pattern.index("R")
    assert "A" in pattern[first_r:] and err[-1] < err[first_r + 1]   # the loop recovers from the rejected steps


@pytest.mark.gpu
def test_gpu_sparse_refusals(ctx):
    from mvslam_amd import capi

    pb, _ = _wide(9)
    args = bm.sparse_args(pb)

    def status(**kw):
        a = dict(args)
        a.update(kw)
        try:
            return ctx.ba_refine_sparse(**a)
        except capi.MvsError as e:
            return e.status

    # no prior at all: the gauge is free
    r = status(frame_prior_var=np.zeros_like(pb["var"]), point_prior_cov=None)
    assert r["status"] == capi.MVS_NO_MODEL and not r["ok"]
    assert not r["R"].any() and not r["points"].any() and not r["pose_cov"].any() and not r["point_cov"].any()   # untouched
    # a point without observation or prior
    off = np.concatenate([pb["csr"]["obs_off"], pb["csr"]["obs_off"][-1:]])
    r = status(points=np.vstack([pb["Xg"], [[0.0, 0.0, 5.0]]]), point_prior_cov=np.vstack([pb["pcov"], np.zeros((1, 9))]),
               obs_off=off)
    assert r["status"] == capi.MVS_NO_MODEL and not r["ok"] and not r["R"].any()
    assert status(n_frames=4097) == capi.MVS_ERR_CAPACITY
    fr = pb["csr"]["obs_frame"].copy()
    k = int(np.flatnonzero(np.diff(pb["csr"]["obs_off"]) >= 2)[0])
    o = pb["csr"]["obs_off"][k]
    fr[o], fr[o + 1] = fr[o + 1], fr[o]
    assert status(obs_frame=fr) == capi.MVS_ERR_INVALID_ARG
    uv = pb["csr"]["obs_uv"].copy()
    uv[3, 1] = np.nan
    assert status(obs_uv=uv) == capi.MVS_ERR_INVALID_ARG
    off = pb["csr"]["obs_off"].copy()
    off[-1] -= 1
    assert status(obs_off=off) == capi.MVS_ERR_INVALID_ARG


@pytest.mark.gpu
def test_gpu_sparse_refuses_an_envelope_beyond_the_skyline_limit(ctx):
    """4096 frames on chains of 2 .. 5, plus points that frame 0 shares with frame 4095 and every frame from 1024 on (the one
    point of frames 0 and 4095 alone widens one row: 4096 blocks more, far from the limit): more than 2^21 blocks,
    MVS_ERR_CAPACITY before any launch"""
    from mvslam_amd import capi

    F = 4096
    rng = np.random.default_rng(0)
    off, fr = [0], []
    for i in range(2000):
        L = int(rng.integers(2, 6))
        s = int(rng.integers(0, F - L + 1))
        fr += list(range(s, s + L))
        off.append(len(fr))
    for k in [F - 1] + list(range(1024, F - 1)):
        fr += [0, k]
        off.append(len(fr))
    m, n = len(off) - 1, len(fr)
    poses = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (F, 1))
    with pytest.raises(capi.MvsError) as e:
        ctx.ba_refine_sparse(K=tw.K_GENERAL, frame_pose=poses, frame_prior_var=np.ones((F, 6)), points=np.ones((m, 3)),
                             point_prior_cov=None, obs_off=off, obs_frame=fr, obs_uv=np.zeros((n, 2)))
    assert e.value.status == capi.MVS_ERR_CAPACITY


@pytest.mark.gpu
def test_gpu_nine_frame_window_is_still_refused(ctx):
    from mvslam_amd import capi

    pb, _ = _wide(9)
    with pytest.raises(capi.MvsError) as e:
        ctx.ba_refine_windows([bm.as_window(pb)])
    assert e.value.status == capi.MVS_ERR_CAPACITY


def test_sparse_kernel_resources():
    """the new kernels are in the build's digest, without scratch; pg_direct.hip's four are still the only ones of their kind"""
    res = json.load(open(os.path.join(ROOT, "mvslam_amd", "lib", "kernel_resources.json")))
    names = ["bas_lin_kernel", "bas_point_kernel", "bas_z_kernel", "bas_prior_kernel", "bas_frame_kernel", "bas_schur_kernel",
             "bas_zd_kernel", "bas_update_kernel", "bas_terms_kernel", "bas_reduce_kernel", "bas_selinv_kernel",
             "bas_pose_cov_kernel", "bas_zs_kernel", "bas_y_kernel", "bas_point_cov_kernel"]
    for n in names:
        hits = {k: v for k, v in res.items() if n in k}
        assert len(hits) == 1, n
        for k, v in hits.items():
            assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0, (k, v)
    for n in ("pgd_scale_kernel", "pgd_assemble_kernel", "pgd_factor_kernel", "pgd_solve_kernel"):
        assert len([k for k in res if n in k]) == 1, n
