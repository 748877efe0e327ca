"""Marginal covariances of a pose graph on the device (pg_marginals.hip): mvs_pose_graph_marginals
and mvs_seq_pose_graph_marginals against tests/pg_marginals_model.py.

Accuracy.  For block (i, j), err = |S_dev - S_ref|_F / sqrt(|S_ref,ii|_F |S_ref,jj|_F) with S_ref the extended-precision inverse
of the model's H.  No tolerance is fixed in advance: per fixture the same error is measured for two float64 host methods,
numpy.linalg.inv(H) and the model's skyline restatement, and the device has to stay within 8 x the larger of the two, never
below 64 * 2^-52.  Every block of every fixture is queried (at most 71 x 71), at the initial values and at the poses
mvs_pose_graph_optimize returns.  A failing test prints the three errors.

Every graph has at most 71 nodes; the sequences are the 300-keypoint fixtures of tests/test_seq_loops.py and
tests/test_seq_pose_graph.py."""
import numpy as np
import pytest

import pg_marginals_model as mm
import posegraph_model as pm

_CASES = {}


def _case(ctx, name, at):
    """one fixture at its initial values or at the device's optimum: the host references (computed once, read only) and the
    device's answer to every query (i, j)"""
    key = (name, at)
    if key in _CASES:
        return _CASES[key]
    from mvslam_amd import capi

    g = mm.FIXTURES[name]()
    X = g["node_pose"]
    if at == "optimised":
        st, res, X = ctx.pose_graph_optimize(g)
        assert st == capi.MVS_OK and res["ok"] == 1
    N = X.shape[0]
    queries = mm.all_pairs(N)
    first, _, blocks = mm.graph_envelope(g)
    H = mm.dense_h(g, X)
    e_inv, e_sky, S_ref = mm.host_errors(H, first, queries)
    st, info, cov = ctx.pose_graph_marginals(g, poses=X, queries=queries)
    assert st == capi.MVS_OK and info["ok"] == 1 and info["bad_node"] == -1
    c = dict(g=g, X=X, N=N, queries=queries, first=first, blocks=blocks, H=H, S_ref=S_ref, e_inv=e_inv, e_sky=e_sky, cov=cov,
             info=info)
    for v in (X, H, S_ref, cov):
        v.setflags(write=False)
    _CASES[key] = c
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("at", ["initial", "optimised"])
@pytest.mark.parametrize("name", list(mm.FIXTURES))
def test_gpu_blocks_within_the_host_methods(ctx, name, at):
    c = _case(ctx, name, at)
    err = mm.block_errors(c["cov"], c["S_ref"], c["queries"])
    worst = int(np.argmax(err))
    limit = mm.bound(c["e_inv"], c["e_sky"])
    print("%s %s: device %.3e at block %s, inv %.3e, skyline model %.3e, bound %.3e, envelope %d, min pivot %.3e"
          % (name, at, err[worst], c["queries"][worst], c["e_inv"], c["e_sky"], limit, c["info"]["envelope_blocks"],
             c["info"]["min_pivot"]))
    assert np.isfinite(c["cov"]).all()
    assert err[worst] <= limit
    assert c["info"]["envelope_blocks"] == c["blocks"]
    # min_pivot: the smallest diagonal entry of L, against the model's factor.  A pivot is an entry of a Schur complement: its
    # relative rounding error is bounded by a small multiple of cond(H) eps, in both computations
    _, min_pivot = mm.skyline_factor(c["H"], c["first"])
    assert abs(c["info"]["min_pivot"] - min_pivot) <= 64 * np.linalg.cond(c["H"]) * mm.EPS * min_pivot


@pytest.mark.gpu
def test_gpu_one_node_is_the_anchor_prior(ctx):
    from mvslam_amd import capi

    g = mm.FIXTURES["one_node"]()
    for sigma in ((1e-4, 1e-4), (0.3, 2.0), (0.017, 1e-3)):
        st, info, cov = ctx.pose_graph_marginals(g, anchor_sigma=sigma)
        assert st == capi.MVS_OK and info["ok"] == 1 and info["envelope_blocks"] == 1 and cov.shape == (1, 6, 6)
        want = np.diag([sigma[0] ** 2] * 3 + [sigma[1] ** 2] * 3)
        ulp = np.spacing(np.diag(want))
        print(sigma, (np.diag(cov[0]) - np.diag(want)) / ulp)
        assert (np.abs(np.diag(cov[0]) - np.diag(want)) <= 4 * ulp).all()
        # off the diagonal R0^T R of a rotation with itself is zero to rounding only: 4 ulp of the diagonal's entries, too
        assert (np.abs(cov[0] - np.diag(np.diag(cov[0]))) <= 4 * ulp.max()).all()
        assert abs(info["min_pivot"] - 1.0 / max(sigma)) <= 1e-12 / max(sigma)


PROPERTY_FIXTURES = ["ring24", "star70", "chain40", "all_pairs16"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PROPERTY_FIXTURES)
def test_gpu_bytes_do_not_depend_on_the_query_list(ctx, name):
    c = _case(ctx, name, "optimised")
    g, X, N, full = c["g"], c["X"], c["N"], c["cov"].reshape(c["N"], c["N"], 6, 6)
    # the all-diagonal default, an explicit list of the diagonal, and the diagonal of the all-pairs call
    _, info, dflt = ctx.pose_graph_marginals(g, poses=X)
    _, _, expl = ctx.pose_graph_marginals(g, poses=X, queries=[(i, i) for i in range(N)])
    assert dflt.shape == (N, 6, 6) and dflt.tobytes() == expl.tobytes()
    assert dflt.tobytes() == np.ascontiguousarray(full[np.arange(N), np.arange(N)]).tobytes()
    # shuffled, with duplicates
    rng = np.random.default_rng(3)
    q = np.array(c["queries"])[rng.permutation(N * N)[:60]]
    q = np.concatenate([q, q[:7], q[::-1][:5]])
    _, _, got = ctx.pose_graph_marginals(g, poses=X, queries=q)
    for n, (i, j) in enumerate(q):
        assert got[n].tobytes() == full[i, j].tobytes(), (i, j)
    # transposes and symmetry, bit for bit
    for i in range(N):
        assert full[i, i].tobytes() == np.ascontiguousarray(full[i, i].T).tobytes(), i
        for j in range(i):
            assert full[j, i].tobytes() == np.ascontiguousarray(full[i, j].T).tobytes(), (i, j)
    # two calls
    _, info2, again = ctx.pose_graph_marginals(g, poses=X, queries=c["queries"])
    assert again.tobytes() == c["cov"].tobytes() and info2.tobytes() == c["info"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ring24", "chain40", "full_cov"])
def test_gpu_a_rigid_motion_of_the_world_changes_nothing(ctx, name):
    """right-perturbation covariances do not see a rigid motion: the moved graph at the moved poses against the reference of
    the graph where it was, held to the bound the host methods reach on the moved H against that same reference"""
    from mvslam_amd import capi

    c = _case(ctx, name, "optimised")
    gm_, Xm = pm.moved(c["g"]), pm.moved_poses(c["X"])
    e_inv, e_sky, _ = mm.host_errors(mm.dense_h(gm_, Xm), c["first"], c["queries"], c["S_ref"])
    st, info, cov = ctx.pose_graph_marginals(gm_, poses=Xm, queries=c["queries"])
    err = mm.block_errors(cov, c["S_ref"], c["queries"]).max()
    print("%s moved: device %.3e, inv %.3e, skyline model %.3e" % (name, err, e_inv, e_sky))
    assert st == capi.MVS_OK and info["ok"] == 1
    assert err <= mm.bound(e_inv, e_sky)


@pytest.mark.gpu
def test_gpu_envelope_counts(ctx):
    chain = pm.ring(30, chords=())
    chain = pm.graph(chain["node_pose"], np.stack([chain["edge_src"], chain["edge_dst"]], axis=1)[:29], chain["edge_pose"][:29],
                     chain["edge_cov"][:29])
    _, info, _ = ctx.pose_graph_marginals(chain, queries=[(29, 29)])
    assert info["envelope_blocks"] == 2 * 30 - 1
    _, info, _ = ctx.pose_graph_marginals(pm.star(70), queries=[(0, 0)])
    assert info["envelope_blocks"] == 71 * 72 // 2
    g = mm.FIXTURES["ring24_relabelled"]()
    assert _case(ctx, "ring24_relabelled", "initial")["info"]["envelope_blocks"] == mm.graph_envelope(g)[2] \
        != _case(ctx, "ring24", "initial")["info"]["envelope_blocks"]


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _filled(n):
    return np.full((n, 6, 6), -7.25)


@pytest.mark.gpu
def test_gpu_no_model_leaves_the_output_alone(ctx):
    from mvslam_amd import capi

    ring = pm.ring(24, chords=(2,))
    for g in (pm.indefinite(ring, 5), pm.indefinite(ring, 0), pm.disconnected()):
        out = _filled(g["node_pose"].shape[0])
        st, info, cov = ctx.pose_graph_marginals(g, cov_out=out)
        assert st == capi.MVS_NO_MODEL and info["ok"] == 0
        assert cov is out and out.tobytes() == _filled(len(out)).tobytes()
    # the context still works
    st, info, _ = ctx.pose_graph_marginals(ring)
    assert st == capi.MVS_OK and info["ok"] == 1


def _status_of(fn, *a, **kw):
    from mvslam_amd import capi

    try:
        return fn(*a, **kw)[0]
    except capi.MvsError as e:
        return e.status


@pytest.mark.gpu
def test_gpu_argument_and_capacity_errors(ctx):
    from mvslam_amd import capi

    g = pm.ring(24, chords=(2,))
    I, CAP = capi.MVS_ERR_INVALID_ARG, capi.MVS_ERR_CAPACITY
    for q in ([(-1, 0)], [(0, -1)], [(24, 0)], [(3, 24)], [(0, 0), (5, 24)]):
        assert _status_of(ctx.pose_graph_marginals, g, queries=q) == I, q
    assert _status_of(ctx.pose_graph_marginals, g, anchor_sigma=(0.0, 1e-4)) == I
    assert _status_of(ctx.pose_graph_marginals, g, anchor_sigma=(1e-4, -1.0)) == I
    bad = g["node_pose"].copy()
    bad[3, 10] = np.nan
    assert _status_of(ctx.pose_graph_marginals, g, poses=bad) == I
    assert _status_of(ctx.pose_graph_marginals, dict(g, anchor=24)) == I
    # 4097 nodes; 4096 nodes all joined to node 0: 8.4 M envelope blocks, refused before anything is launched
    def hub(n):
        eye = pm.se3([0, 0, 0], [0, 0, 0])
        edges = np.stack([np.zeros(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)], axis=1)
        return pm.graph(np.tile(eye, (n, 1)), edges, np.tile(eye, (n - 1, 1)), pm.iso_cov(0.01, n - 1))

    assert _status_of(ctx.pose_graph_marginals, hub(4097), queries=[(0, 0)]) == CAP
    assert _status_of(ctx.pose_graph_marginals, hub(4096), queries=[(0, 0)]) == CAP
    assert _status_of(ctx.pose_graph_marginals, g, queries=[(23, 0)]) == capi.MVS_OK


@pytest.mark.gpu
def test_gpu_min_pivot_on_a_loose_anchor(ctx):
    from mvslam_amd import capi

    g = pm.loose_anchor(17)
    st, info, cov = ctx.pose_graph_marginals(g, anchor_sigma=pm.LOOSE_SIGMA)
    H = mm.dense_h(g, anchor_sigma=pm.LOOSE_SIGMA)
    first = mm.graph_envelope(g)[0]
    _, want = mm.skyline_factor(H, first)
    print("min pivot", info["min_pivot"], "model", want)
    assert st == capi.MVS_OK and info["ok"] == 1 and info["bad_node"] == -1
    assert abs(info["min_pivot"] - want) <= 64 * np.linalg.cond(H) * mm.EPS * want
    # the loose prior shows in the anchor's own covariance
    assert cov[0][0, 0] > 0.5 * pm.LOOSE_SIGMA[0] ** 2 and cov[0][5, 5] > 0.5 * pm.LOOSE_SIGMA[1] ** 2


# ---- the sequence call --------------------------------------------------------------------------------------------------------
def _seq_equals_host(ctx, s, queries=None):
    from mvslam_amd import capi

    g, X = s.download_pose_graph(), s.download_pose_graph_poses()
    st, info, cov = s.pose_graph_marginals(queries=queries)
    st2, info2, cov2 = ctx.pose_graph_marginals(g, poses=X, queries=queries)
    assert st == st2 == capi.MVS_OK and info["ok"] == 1
    assert info.tobytes() == info2.tobytes() and cov.tobytes() == cov2.tobytes()
    assert np.isfinite(cov).all()
    return g, info, cov


@pytest.mark.gpu
def test_gpu_sequence_with_loop_edges(ctx):
    import test_lane_join as lj
    import test_seq_loops as tl
    from mvslam_amd import capi, synth

    I = capi.MVS_ERR_INVALID_ARG
    data = synth.make_loop_sequence(tl.LOOP_FRAMES, **tl.LOOP_ARGS)
    s = capi.Sequence(ctx, tl.LOOP_FRAMES, tl.N_KP, 32)
    try:
        s.upload(0, data["desc"], data["kp"], data["n_kp"], data["K"])
        s.upload_octaves(0, tl.st._octaves(tl.LOOP_FRAMES))
        s.loop_scores(tl.MATCH["ratio"], tl.MATCH["max_dist"], tl.LOOP_GAP)
        s.select_loops(tl.LOOP_MIN_SCORE, tl.LOOP_TOP_K, tl.LOOP_CAP)
        s.run(tl._two_view(), tl.so._pnp())
        s.run_lags(tl._two_view(), 2)
        assert _status_of(s.pose_graph_marginals) == I                    # no graph
        s.verify_loops(tl._two_view())
        s.build_pose_graph(2)
        s.add_loop_edges(loop_sigma=(0.02, 0.2))
        assert _status_of(s.pose_graph_marginals) == I                    # a graph, not optimised
        st, res = s.optimize_pose_graph()
        assert st == capi.MVS_OK and res["ok"] == 1
        g, info, cov = _seq_equals_host(ctx, s)
        assert (g["edge_kind"] == 2).sum() >= 1, "no loop edge: the test shows less than it says"
        first, _, blocks = mm.graph_envelope(g)
        print("loop graph: edges", g["n_edges"], "envelope", info["envelope_blocks"], "min pivot", info["min_pivot"])
        assert info["envelope_blocks"] == blocks > 3 * tl.LOOP_FRAMES - 3      # the loop edges widen rows beyond lag 2
        q = [(0, 23), (23, 0), (7, 7), (12, 3)]
        _, _, some = _seq_equals_host(ctx, s, q)
        assert some[2].tobytes() == cov[7].tobytes() and some[0].tobytes() == np.ascontiguousarray(some[1].T).tobytes()
        # a call made while a half-batch lane is open: the same bytes as after sync
        b = lj._batch(ctx, lj._data("uniform"))
        try:
            b.run(lj._prm())
            _, _, open_lane = s.pose_graph_marginals()
            b.sync()
            s.sync()
            _, _, synced = s.pose_graph_marginals()
        finally:
            b.close()
        assert open_lane.tobytes() == synced.tobytes() == cov.tobytes()
        # new edges, then a new run: refused again
        s.add_loop_edges()
        assert _status_of(s.pose_graph_marginals) == I
        s.optimize_pose_graph()
        assert _status_of(s.pose_graph_marginals) == capi.MVS_OK
        s.run_lags(tl._two_view(), 2)
        assert _status_of(s.pose_graph_marginals) == I
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_sequence_of_twenty_frames(ctx):
    import test_seq_pose_graph as sp
    from mvslam_amd import capi

    s = sp._open(ctx, 20)
    try:
        s.build_pose_graph(3)
        assert _status_of(s.pose_graph_marginals) == capi.MVS_ERR_INVALID_ARG
        st, res = s.optimize_pose_graph()
        assert st == capi.MVS_OK
        g, info, cov = _seq_equals_host(ctx, s)
        # against the model, as for the host-pointer fixtures
        X = s.download_pose_graph_poses()
        queries = [(i, i) for i in range(20)]
        H = mm.dense_h(g, X)
        e_inv, e_sky, S_ref = mm.host_errors(H, mm.graph_envelope(g)[0], queries)
        err = mm.block_errors(cov, S_ref, queries).max()
        print("seq20: device %.3e, inv %.3e, skyline model %.3e, envelope %d" % (err, e_inv, e_sky, info["envelope_blocks"]))
        assert err <= mm.bound(e_inv, e_sky)
        _seq_equals_host(ctx, s, [(19, 0), (0, 19), (4, 5)])
    finally:
        s.close()
