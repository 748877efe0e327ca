"""GPU tests of the robust edge losses on the pose graph of a resident sequence (mvs_seq_optimize_pose_graph under
mvs_ctx_set_pose_graph_loss with MVS_PG_LOSS_LOOP_EDGES, mvs_seq_pose_graph_edge_stats): the
resident calls against the host-graph calls on the downloaded graph, byte for byte, on the 24-frame loop sequence of
tests/test_seq_loops.py."""
import pytest

import pg_robust_model as rm
import test_seq_loops as sl
from test_seq_loops import loop_seq  # noqa: F401  (the module-scoped fixture, one instance for this module)

pytestmark = pytest.mark.gpu


def _refused(fn):
    from mvslam_amd import capi

    with pytest.raises(capi.MvsError) as e:
        fn()
    assert e.value.status == capi.MVS_ERR_INVALID_ARG


def test_loop_edges_loss_on_a_resident_graph(ctx, loop_seq):  # noqa: F811
    from mvslam_amd import capi

    s, _ = loop_seq
    LOOPS = capi.MVS_PG_LOSS_LOOP_EDGES
    try:
        s.verify_loops(sl._two_view())
        built = sl._built(s)
        _refused(s.pose_graph_edge_stats)                                   # before any optimisation
        # no loop edges added: MVS_PG_LOSS_LOOP_EDGES selects no edge and returns the bytes of MVS_PG_LOSS_NONE
        st0, res0 = s.optimize_pose_graph()
        poses0 = s.download_pose_graph_poses()
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_CAUCHY, rm.CAUCHY_K, LOOPS)
        st1, res1 = s.optimize_pose_graph()
        assert st0 == st1 == capi.MVS_OK and res0.tobytes() == res1.tobytes()
        assert poses0.tobytes() == s.download_pose_graph_poses().tobytes()
        st, chi2, weight = s.pose_graph_edge_stats()
        assert st == capi.MVS_OK and chi2.shape == (built["n_edges"],) and (weight == 1.0).all() and (chi2 >= 0.0).all()
        # with loop edges: exactly the edges of kind 2 get the loss
        s.add_loop_edges(loop_sigma=(0.02, 0.2))
        _refused(s.pose_graph_edge_stats)                                   # the optimised state was cleared
        g = s.download_pose_graph()
        first = int((g["edge_kind"] != 2).sum())
        assert first == built["n_edges"] < g["n_edges"] and (g["edge_kind"][first:] == 2).all()
        st, res = s.optimize_pose_graph()
        poses = s.download_pose_graph_poses()
        st_s, chi2_s, weight_s = s.pose_graph_edge_stats()
        for loss, k in ((capi.MVS_PG_LOSS_CAUCHY, rm.CAUCHY_K), (capi.MVS_PG_LOSS_HUBER, rm.HUBER_K)):
            ctx.set_pose_graph_loss(loss, k, LOOPS)
            st, res = s.optimize_pose_graph()
            poses = s.download_pose_graph_poses()
            st_s, chi2_s, weight_s = s.pose_graph_edge_stats()
            _refused(lambda: ctx.pose_graph_optimize(g))                    # a host graph has no loop edges to stand for
            ctx.set_pose_graph_loss(loss, k, first)
            st_h, res_h, poses_h = ctx.pose_graph_optimize(g)
            st_e, chi2_h, weight_h = ctx.pose_graph_edge_stats(g, poses_h)
            print("loss %d: error %.6g -> %.6g, iterations %d, weights of the loop edges %s" % (
                loss, res["error_initial"], res["error"], res["iterations"], weight_s[first:]))
            assert st == st_h == st_s == st_e == capi.MVS_OK and res["ok"] == 1
            assert res.tobytes() == res_h.tobytes() and poses.tobytes() == poses_h.tobytes()
            assert chi2_s.tobytes() == chi2_h.tobytes() and weight_s.tobytes() == weight_h.tobytes()
            assert (weight_s[:first] == 1.0).all() and ((weight_s[first:] > 0.0) & (weight_s[first:] <= 1.0)).all()
        # back to no loss
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_NONE)
        st_n, res_n = s.optimize_pose_graph()
        assert st_n == capi.MVS_OK and res_n["ok"] == 1
        # after a failed optimisation: a graph with no edge at all
        s.build_pose_graph(2, min_points=10 ** 6)
        st_f, res_f = s.optimize_pose_graph()
        assert st_f == capi.MVS_NO_MODEL and res_f["ok"] == 0
        _refused(s.pose_graph_edge_stats)
    finally:
        ctx.set_pose_graph_loss(capi.MVS_PG_LOSS_NONE)
        s.build_pose_graph(2)                                               # what the fixture's other users start from
