"""The global bundle adjustment of a resident sequence on the device: mvs_seq_refine_global and its downloads (DESIGN.md
section 4.7.5), against the numpy model of tests/seq_global_model.py and against the host route through mvs_ba_refine_sparse.

Assembly: the downloaded problem equals the model fed the device's own downloaded pairs, trajectory and octaves -- integers
equal, guesses to 1e-12 max(1, |X|), section 4.7.1's bound for the same three multiply-adds.  Plan: every list the device
built equals mvs_bas::plan (tests/cpp/ba_envelope_dump.cpp) on the downloaded CSR.  Solve: record, poses, points and both
covariances equal Context.ba_refine_sparse on the problem rebuilt from the download, byte for byte (the same solver on the
same inputs and lists).  tests/test_seq_global_host.py shows on the CPU that the sequences exercise what is compared here.
"""
import ctypes as C

import numpy as np
import pytest

import seq_global_model as gm
import test_seq_windows as sw
from mvslam_amd import synth
from test_seq_global_host import LONG_ARGS, LONG_FRAMES, LONG_T


@pytest.fixture(scope="module")
def resident(ctx):
    """test_seq_windows' sequence (6 frames of 300 keypoints), run once; octaves 0 .. 2 so that the observation weights differ"""
    seq = sw.make_seq()
    octave = (np.arange(6 * 300).reshape(6, 300) % 3).astype(np.uint8)
    s, dev = sw._run(ctx, seq, octave=octave)
    yield s, dev, seq
    s.close()


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return gm.compile_planner(tmp_path_factory.mktemp("seq_global_plan"), sanitize=False)


def _n_kp(dev):
    return dev["kp"].shape[1]


def _check_assembly(s, dev, T):
    got = s.download_global_problem()
    want = gm.build_global(dev["pairs"], dev["traj"], _n_kp(dev), T)
    for k in ("obs_off", "obs_frame", "obs_kp", "head_frame", "head_kp"):
        assert np.array_equal(got[k], want[k]), k
    err = np.abs(got["point_guess"] - want["point_guess"])
    print("T = %d: %d points, %d observations, guess error %.2e" % (T, len(want["head_frame"]), len(want["obs_frame"]), err.max()))
    assert np.all(err <= 1e-12 * np.maximum(1.0, np.abs(want["point_guess"])))
    assert np.array_equal(got["obs_uv"], dev["kp"][got["obs_frame"], got["obs_kp"]].astype(np.float64))
    assert s.global_counts() == (len(want["head_frame"]), len(want["obs_frame"]))
    return got, want


def _device_plan(s):
    from mvslam_amd import capi

    dbg = capi.dbg_lib()
    counts = np.zeros(6, np.int64)
    null = [None] * 10
    assert dbg.mvs_debug_seq_global_plan(s._h, counts.ctypes.data_as(C.c_void_p), *null) == 0
    F, _, O, B, NP, widest = (int(x) for x in counts)
    size = dict(first=F, row_off=F + 1, blk_row=B, last=F, obs_point=O, fr_off=F + 1, fr_obs=O, pair_off=B + 1, pair_a=NP,
                pair_c=NP)
    out = {k: np.full(size[k], -7, np.int32) for k in gm.PLAN_LISTS}
    assert dbg.mvs_debug_seq_global_plan(s._h, None, *[out[k].ctypes.data_as(C.c_void_p) for k in gm.PLAN_LISTS]) == 0
    out = {k: v.tolist() for k, v in out.items()}
    out.update(blocks=[B], pairs=[NP], widest=[widest])
    return out


def _check_plan(s, planner, got):
    F = s.n_frames
    want = planner(F, got["obs_off"].tolist(), got["obs_frame"].tolist())
    assert want["check"] == [0] and want["fits"] == [1]
    plan = _device_plan(s)
    for k in gm.PLAN_LISTS + ("blocks", "pairs", "widest"):
        assert plan[k] == want[k], k
    return want


def _check_solve(ctx, s, dev, got, res, params, sigma_px, must_solve=True):
    """the device route against the host route through mvs_ba_refine_sparse on the problem rebuilt from the download: status,
    record and every output array, byte for byte.  must_solve: ok = 1 is demanded as well."""
    ref = ctx.ba_refine_sparse(**gm.sparse_args(got, dev["traj"], dev["kp"], dev["octave"], dev["K"], params, sigma_px))
    out = s.download_global()
    print("error %.6e -> %.6e in %d iterations (%d rejected), envelope %d blocks, widest row %d"
          % (res["error_initial"], res["error"], res["iterations"], res["rejected_steps"], res["envelope_blocks"],
             res["widest_row"]))
    assert res["status"] == ref["status"] == out["status"] and res["ok"] == ref["ok"]
    assert not must_solve or (res["status"] == 0 and res["ok"])
    assert res["error"] <= res["error_initial"]
    assert out["raw"] + res["raw"] == ref["raw"]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("T", [0, 2, 3, 8])
def test_gpu_seq_global_assembly_plan_and_solve(ctx, resident, planner, T):
    from mvslam_amd import capi

    s, dev, _ = resident
    params = capi.default_refine_params()
    res = s.refine_global(T, params, 0.5)
    got, want = _check_assembly(s, dev, T)
    plan = _check_plan(s, planner, got)
    _check_solve(ctx, s, dev, got, res, params, 0.5)
    # uncut and cut differ: a row of the envelope is as wide as the longest track
    widest = min(T, 6) if T in (2, 3) else want["longest_chain"]
    assert res["widest_row"] == plan["widest"][0] == int(np.diff(want["obs_off"]).max()) == widest
    assert res["envelope_blocks"] == plan["blocks"][0]
    assert len(want["head_frame"]) >= 100 and all(p["valid"] for p in dev["pairs"])


@pytest.mark.gpu
def test_gpu_seq_global_long_sequence_crosses_the_frame_chunks(ctx, planner):
    """260 frames of 96 keypoints at T = 8: the scans over the frames run in chunks of 256, which is what this case is about
    (assembly and plan).  With 96 keypoints a frame the trajectory's scale chain does not hold over 260 frames (measured: an
    initial error of 1.5e15, every one of the 11 LM steps a failed solve, ok = 0), so the problem is not one a solver can be
    asked to solve: the two routes are held to the same record and the same untouched outputs, not to ok = 1."""
    from mvslam_amd import capi

    seq = synth.make_sequence(LONG_FRAMES, **LONG_ARGS)
    s, dev = sw._run(ctx, seq)
    try:
        assert all(p["valid"] for p in dev["pairs"])
        params = capi.default_refine_params()
        res = s.refine_global(LONG_T, params, 0.5)
        got, want = _check_assembly(s, dev, LONG_T)
        assert want["longest_chain"] > LONG_T and (want["head_frame"] >= 256).any()
        _check_plan(s, planner, got)
        _check_solve(ctx, s, dev, got, res, params, 0.5, must_solve=False)
        assert res["widest_row"] == LONG_T
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_seq_global_names_the_tracks_of_one_window(ctx, resident):
    """three frames, T = 3, against mvs_seq_refine_windows with F = 3 and one window: the same tracks, the same guesses"""
    from mvslam_amd import capi

    _, _, seq = resident
    three = dict(seq, desc=seq["desc"][:3], kp=seq["kp"][:3], n_kp=seq["n_kp"][:3])
    s, dev = sw._run(ctx, three)
    try:
        params = capi.default_refine_params()
        s.refine_windows(3, 1, 4096, params, 0.5)
        (win,) = s.download_windows()
        res = s.refine_global(3, params, 0.5)
        got = s.download_global_problem()
        assert res["ok"] and win["n_points"] == win["n_tracks_found"] == len(got["head_frame"]) >= 30
        tkp = np.full((len(got["head_frame"]), 3), -1, np.int32)
        p = np.repeat(np.arange(len(got["head_frame"])), np.diff(got["obs_off"]))
        tkp[p, got["obs_frame"]] = got["obs_kp"]
        assert np.array_equal(tkp, win["track_kp"])
        assert got["point_guess"].tobytes() == win["point_guess"].tobytes()
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_seq_global_is_deterministic(ctx, resident):
    from mvslam_amd import capi

    s, _, _ = resident
    runs = []
    for _ in range(2):
        res = s.refine_global(3, capi.default_refine_params(), 0.5)
        prob = s.download_global_problem()
        runs.append(res["raw"] + s.download_global()["raw"] + b"".join(prob[k].tobytes() for k in sorted(prob)) +
                    b"".join(np.array(v, np.int64).tobytes() for _, v in sorted(_device_plan(s).items())))
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_gpu_seq_global_after_the_essential_run(ctx, resident, planner):
    from mvslam_amd import capi

    _, _, seq = resident
    F, N = seq["kp"].shape[0], seq["kp"].shape[1]
    s = capi.Sequence(ctx, F, N, 32)
    try:
        s.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
        s.run_essential(capi.default_params(num_hypotheses=sw.PRM["H"], sampler=capi.SAMPLER_PHILOX, seed=sw.PRM["seed"],
                                            max_error_sq=sw.PRM["thr"]),
                        capi.default_pnp_params(num_hypotheses=sw.PPRM["H"], seed=sw.PPRM["seed"], reproj_error=sw.PPRM["err"]))
        gp = s.download_pairs()
        pairs = []
        for k, r in enumerate(gp["results"]):
            M, n = int(r["n_matches"]), int(r["n_points"]) if r["valid"] else 0
            pairs.append(dict(valid=bool(r["valid"]), matches=gp["matches"][k][:M], mask=gp["mask"][k][:M],
                              point_idx=gp["point_idx"][k][:n], points=gp["points"][k][:n]))
        dev = dict(pairs=pairs, traj=s.download_trajectory(), kp=seq["kp"], octave=np.zeros((F, N), np.uint8), K=seq["K"])
        params = capi.default_refine_params()
        res = s.refine_global(0, params, 0.7)
        got, want = _check_assembly(s, dev, 0)
        assert len(want["head_frame"]) >= 100
        _check_plan(s, planner, got)
        _check_solve(ctx, s, dev, got, res, params, 0.7)
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_seq_global_refusals(ctx, resident):
    """every refusal of the header.  No capacity breach is reachable at test size (the smallest is 2^20 points); the limits
    are exercised on the host side by tests/cpp/seq_global_limits_check.cpp."""
    from mvslam_amd import capi

    s, dev, seq = resident

    def status_of(fn, *a, **kw):
        with pytest.raises(capi.MvsError) as e:
            fn(*a, **kw)
        return e.value.status

    for T in (1, -1, 4097):
        assert status_of(s.refine_global, T) == capi.MVS_ERR_INVALID_ARG, T
    for sigma_px in (0.0, -0.5, float("nan")):
        assert status_of(s.refine_global, 0, None, sigma_px) == capi.MVS_ERR_INVALID_ARG
    for bad in (dict(lambda_factor=1.0), dict(point_sigma=0.0), dict(max_iterations=-1), dict(anchor_sigma=(0.0, 1e-5))):
        assert status_of(s.refine_global, 0, capi.default_refine_params(**bad)) == capi.MVS_ERR_INVALID_ARG, bad
    fresh = capi.Sequence(ctx, 6, 300, 32)                     # uploaded, never run
    fresh.upload(0, seq["desc"], seq["kp"], seq["n_kp"], seq["K"])
    assert status_of(fresh.refine_global, 0) == capi.MVS_ERR_INVALID_ARG
    assert status_of(fresh.global_counts) == capi.MVS_ERR_INVALID_ARG
    assert status_of(fresh.download_global_problem) == capi.MVS_ERR_INVALID_ARG
    fresh.close()
    # no frame has eight keypoints: every pair is invalid, there is no link and no point -- MVS_NO_MODEL, downloads untouched
    blind, bdev = sw._run(ctx, seq, n_kp=np.full(6, 4, np.int32))
    try:
        assert not any(p["valid"] for p in bdev["pairs"])
        res = blind.refine_global(0)
        assert res["status"] == capi.MVS_NO_MODEL and not res["ok"] and (res["n_points"], res["n_obs"]) == (0, 0)
        out = blind.download_global()
        assert out["status"] == capi.MVS_NO_MODEL and not any(np.any(out[k]) for k in ("R", "t", "points", "pose_cov", "point_cov"))
    finally:
        blind.close()
    # frame 3 has four keypoints: pairs 2 and 3 are invalid and end every chain; frame 3 is held by its prior alone
    n_kp = seq["n_kp"].copy()
    n_kp[3] = 4
    cut, cdev = sw._run(ctx, seq, n_kp=n_kp)
    try:
        assert not cdev["pairs"][2]["valid"] and not cdev["pairs"][3]["valid"] and cdev["pairs"][1]["valid"]
        params = capi.default_refine_params()
        res = cut.refine_global(0, params, 0.5)
        got, _ = _check_assembly(cut, cdev, 0)
        assert not np.any(got["obs_frame"] == 3)
        _check_solve(ctx, cut, cdev, got, res, params, 0.5)
    finally:
        cut.close()
    assert s.refine_global(0)["ok"]                              # the context solves a good sequence afterwards
