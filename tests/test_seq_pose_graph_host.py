"""CPU tests of the pose graph of a resident sequence: the new symbols and struct layouts, the
numpy definition tests/seq_graph_model.py on hand-written tables (every gate alone, the degenerate scales, a covariance that
is not positive definite, the chain fallback, the edge order), the covariance rule, and a graph the model builds from exact
relative poses, which must cost nothing at its own nodes."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import posegraph_model as pm
import seq_graph_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seq_graph_symbols_and_struct_layout():
    """fails without the feature: the entry points are exported, mvs_seq_graph_params is laid out as the ctypes mirror says,
    and cg_chunk_iterations sits where `reserved` sat (offset 112 of a 120-byte struct: nothing moved)"""
    from mvslam_amd import capi

    lib = capi.lib()
    for name in ("mvs_seq_build_pose_graph", "mvs_seq_optimize_pose_graph", "mvs_seq_download_pose_graph",
                 "mvs_seq_download_pose_graph_poses"):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
    assert lib.mvs_abi_version() == 4
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(mvs_seq_graph_params), offsetof(mvs_seq_graph_params, max_lag),
         offsetof(mvs_seq_graph_params, min_points), offsetof(mvs_seq_graph_params, max_error),
         offsetof(mvs_seq_graph_params, chain_sigma));
  printf("%zu %zu %zu\n", sizeof(mvs_pose_graph_params), offsetof(mvs_pose_graph_params, cg_max_iterations),
         offsetof(mvs_pose_graph_params, cg_chunk_iterations));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    S, P = capi.SeqGraphParams, capi.PoseGraphParams
    assert v[:5] == [C.sizeof(S), S.max_lag.offset, S.min_points.offset, S.max_error.offset, S.chain_sigma.offset] == [32, 0, 4, 8, 16]
    assert v[5:] == [C.sizeof(P), P.cg_max_iterations.offset, P.cg_chunk_iterations.offset]
    # the old `reserved`: the int32 behind cg_max_iterations, the last four bytes of the struct
    assert v[7] == v[6] + 4 == v[5] - 4
    p = capi.default_pose_graph_params()
    assert p.cg_chunk_iterations == 0
    assert capi.default_pose_graph_params(cg_chunk_iterations=16).cg_chunk_iterations == 16


# ---- hand-written tables --------------------------------------------------------------------------------------------------
def _rot(w):
    return pm.so3_exp(np.asarray(w, dtype=np.float64))


def _trajectory(F=5):
    """frames stepping by (0.5 + 0.1 k) along a turning heading: every step has another length"""
    R, t = [np.eye(3)], [np.zeros(3)]
    for k in range(F - 1):
        R.append(R[-1] @ _rot([0.02 * (k + 1), -0.03, 0.05]))
        t.append(t[-1] + R[-2] @ np.array([0.1 * k, 0.05, 0.5 + 0.1 * k]))
    return np.array(R), np.array(t)


def _cov(seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(6, 6)) * 1e-2
    return A @ A.T + 1e-4 * np.eye(6)


def _tables(R, t, max_lag, noise_seed=3):
    """every pair good: the true relative rotation, a UNIT translation along the true one, 50 points, error 1"""
    F, out = len(R), {}
    for d in range(1, max_lag + 1):
        out[d] = []
        for k in range(F - d):
            rel = pm.between(pm.join(R[k], t[k]), pm.join(R[k + d], t[k + d]))
            u = rel[9:] / np.linalg.norm(rel[9:])
            out[d].append(dict(valid=True, ok=True, n_points=50, error=1.0, R=rel[:9].reshape(3, 3), t=u,
                               pose_cov=_cov(noise_seed + 10 * d + k)))
    return out


def test_model_edge_order_and_values():
    R, t = _trajectory(5)
    tb = _tables(R, t, 3)
    g = gm.build(R, t, tb, 3)
    assert g["slots"] == [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1)]
    assert g["n_edges"] == gm.n_slots(5, 3) == 9 and [gm.slot_offset(5, d) for d in (1, 2, 3)] == [0, 4, 7]
    assert g["edge_src"].tolist() == [k for _, k in g["slots"]] and g["edge_dst"].tolist() == [k + d for d, k in g["slots"]]
    assert g["edge_lag"].tolist() == [d for d, _ in g["slots"]] and not g["edge_kind"].any()
    assert g["node_pose"].tobytes() == np.concatenate([R.reshape(5, 9), t], axis=1).tobytes()
    for e, (d, k) in enumerate(g["slots"]):
        step = np.linalg.norm(R[k].T @ (t[k + d] - t[k]))
        assert abs(g["edge_scale"][e] - step) <= 1e-14 * step            # |u| = 1: the scale is the trajectory's step
        assert np.abs(g["edge_pose"][e][9:] - R[k].T @ (t[k + d] - t[k])).max() <= 1e-14
        assert g["edge_pose"][e][:9].tobytes() == np.ascontiguousarray(tb[d][k]["R"]).tobytes()
        s = g["edge_scale"][e]
        D = np.diag([1, 1, 1, s, s, s])
        assert np.abs(g["edge_cov"][e].reshape(6, 6) - D @ tb[d][k]["pose_cov"] @ D).max() <= 1e-16
        assert g["edge_cov"][e].reshape(6, 6)[:3, :3].tobytes() == np.ascontiguousarray(tb[d][k]["pose_cov"][:3, :3]).tobytes()


def _dropped(R, t, tb, max_lag=2, **kw):
    full = [(d, k) for d in range(1, max_lag + 1) for k in range(len(R) - d)]
    got = gm.build(R, t, tb, max_lag, **kw)["slots"]
    assert [s for s in full if s in got] == got
    return [s for s in full if s not in got]


def test_model_every_gate_alone():
    R, t = _trajectory(5)
    for field, value in (("valid", False), ("ok", False)):
        tb = _tables(R, t, 2)
        tb[2][1][field] = value
        assert _dropped(R, t, tb) == [(2, 1)], field
    tb = _tables(R, t, 2)
    tb[1][2]["n_points"] = 19
    assert _dropped(R, t, tb, min_points=19) == [] and _dropped(R, t, tb, min_points=20) == [(1, 2)]
    assert _dropped(R, t, tb, min_points=51) == [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2)]   # 50 elsewhere
    tb = _tables(R, t, 2)
    tb[2][0]["error"] = 2.5
    assert _dropped(R, t, tb, max_error=2.5) == [] and _dropped(R, t, tb, max_error=2.4999) == [(2, 0)]
    tb[2][0]["error"] = float("nan")
    assert _dropped(R, t, tb) == [(2, 0)]                                   # NaN <= 1e30 is false
    tb[2][0]["error"] = float("inf")
    assert _dropped(R, t, tb) == [(2, 0)]


def test_model_degenerate_scales_and_covariances():
    R, t = _trajectory(5)
    tb = _tables(R, t, 2)
    tb[1][1]["t"] = np.zeros(3)                  # zero-length tau: s = x / 0 = inf
    assert _dropped(R, t, tb) == [(1, 1)]
    R2, t2 = R.copy(), t.copy()
    t2[3] = t2[2]                                # a zero trajectory step: s = 0 for (1, 2); (2, 1) spans the same step as (1, 1)
    tb = _tables(R, t, 2)
    assert _dropped(R2, t2, tb) == [(1, 2)]
    tb[1][1]["t"] = np.zeros(3)
    t2 = t.copy()
    t2[2] = t2[1]                                # a zero step over a zero-length tau: 0 / 0 = NaN for (1, 1)
    assert _dropped(R2, t2, tb) == [(1, 1)]
    for bad in (np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]), np.zeros((6, 6)), np.full((6, 6), 1.0),
                np.diag([1.0, 1.0, 1.0, 1.0, 1.0, np.inf]), np.diag([1.0, np.nan, 1.0, 1.0, 1.0, 1.0])):
        tb = _tables(R, t, 2)
        tb[2][2]["pose_cov"] = bad
        assert _dropped(R, t, tb) == [(2, 2)], bad
    # only the lower triangle is looked at, as in the solver
    tb = _tables(R, t, 2)
    tb[2][2]["pose_cov"] = tb[2][2]["pose_cov"].copy()
    tb[2][2]["pose_cov"][0, 5] = np.nan
    assert _dropped(R, t, tb) == []
    assert gm.chol6_ok(_cov(0)) and not gm.chol6_ok(-_cov(0))
    # the fused pivots: 1 - (1 - 2^-30)^2 needs the unrounded product
    S = np.eye(6)
    S[1, 0] = S[0, 1] = 1.0 - 2.0 ** -30
    assert gm.chol6_ok(S)
    S[1, 1] = (1.0 - 2.0 ** -30) ** 2            # rounded square: below the exact one, so the fused pivot is negative
    assert (S[1, 0] * S[1, 0] == S[1, 1]) and not gm.chol6_ok(S)


def test_model_chain_fallback():
    R, t = _trajectory(5)
    tb = _tables(R, t, 2)
    tb[1][1]["valid"] = False
    tb[2][0]["ok"] = False
    off = gm.build(R, t, tb, 2)
    assert (1, 1) not in off["slots"] and (2, 0) not in off["slots"] and not off["edge_kind"].any()
    for sig in ((0.0, 0.1), (0.1, 0.0), (-1.0, 0.1)):
        assert gm.build(R, t, tb, 2, chain_sigma=sig)["slots"] == off["slots"]          # both must be > 0
    on = gm.build(R, t, tb, 2, chain_sigma=(0.01, 0.2))
    assert on["slots"] == [(1, 0), (1, 1), (1, 2), (1, 3), (2, 1), (2, 2)]                 # in slot (1, 1); lag 2 gets none
    e = on["slots"].index((1, 1))
    assert on["edge_kind"].tolist() == [0, 1, 0, 0, 0, 0] and on["edge_scale"][e] == 1.0
    assert (on["edge_src"][e], on["edge_dst"][e], on["edge_lag"][e]) == (1, 2, 1)
    want = pm.between(pm.join(R[1], t[1]), pm.join(R[2], t[2]))
    assert np.abs(on["edge_pose"][e] - want).max() <= 1e-15
    assert on["edge_cov"][e].tobytes() == np.diag([0.01 * 0.01] * 3 + [0.2 * 0.2] * 3).reshape(36).tobytes()
    # the other edges are the ones without the fallback
    keep = [i for i, s in enumerate(on["slots"]) if s != (1, 1)]
    for k in ("edge_pose", "edge_cov", "edge_scale", "edge_src", "edge_dst"):
        assert on[k][keep].tobytes() == off[k].tobytes(), k
    assert pm.connected(on) and pm.connected(off)
    tb[2][0]["valid"] = tb[2][1]["valid"] = False                          # now nothing bridges frames 1 | 2
    assert not pm.connected(gm.build(R, t, tb, 2)) and pm.connected(gm.build(R, t, tb, 2, chain_sigma=(0.01, 0.2)))


def test_covariance_rule():
    """scaling the translation of a measurement by s scales the translational error by s (right perturbation t + R dv): the
    Mahalanobis norm must not change, e^T S^-1 e = e'^T S'^-1 e' with e' = D e, S' = D S D, D = diag(1, 1, 1, s, s, s).  Both
    sides are evaluated through solves of systems with condition numbers up to 1e4 (A A^T + 1e-4 I with |A| ~ 1e-2): their
    rounding error is about cond * eps ~ 1e-12 in the worst case of this family, observed two orders below; asserted at the
    1e-12 the definition states."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for i in range(200):
        S = _cov(100 + i)
        s = float(np.exp(rng.uniform(-3.0, 3.0)))
        e = rng.normal(size=6)
        rec = dict(valid=True, ok=True, n_points=1, error=0.0, R=np.eye(3), t=np.array([0.0, 0.0, 1.0]), pose_cov=S)
        Rt, tt = np.array([np.eye(3), np.eye(3)]), np.array([[0.0, 0.0, 0.0], [0.0, 0.0, s]])
        Z, Sp, sc = gm.candidate(Rt, tt, 0, 1, rec)
        assert sc == s and Z[11] == s
        Sp = Sp.reshape(6, 6)
        Sp = np.tril(Sp) + np.tril(Sp, -1).T
        ep = np.concatenate([e[:3], s * e[3:]])
        a, b = e @ np.linalg.solve(S, e), ep @ np.linalg.solve(Sp, ep)
        worst = max(worst, abs(a - b) / a)
    assert worst <= 1e-12, worst


def test_exact_relative_poses_cost_nothing():
    """nodes = a true trajectory (posegraph_model's ring, its noiseless poses), pairs = the exact relative poses with unit
    translations: the scale gives every edge its length back and the graph's cost at its nodes is rounding.  Bound: an edge's
    error is at most ~50 roundings of poses of size 3, 2e-14; whitened by covariances >= 1e-4 I that is 2e-12 per component;
    squared and summed over 3 lags x 12 edges x 6 components, halved: 5e-22.  Asserted at 1e-20."""
    n, L = 12, 3
    truth = []
    for i in range(n):
        a = 2.0 * np.pi * i / n * 0.6
        Rm = pm.so3_exp([0, 0, a + np.pi / 2]) @ pm.so3_exp([0.2 * np.sin(3 * a), 0.1 * np.cos(2 * a), 0.0])
        truth.append(pm.join(Rm, [3.0 * np.cos(a), 3.0 * np.sin(a), 0.3 * np.sin(2 * a)]))
    truth = np.array(truth)
    R, t = truth[:, :9].reshape(n, 3, 3), truth[:, 9:]
    g = gm.build(R, t, _tables(R, t, L), L)
    assert g["n_edges"] == gm.n_slots(n, L) and pm.connected(g)
    W = pm.whitening(g["edge_cov"])
    wa = np.repeat(1.0 / np.asarray(pm.ANCHOR_SIGMA), 3)
    r = pm._residuals(g, W, wa, g["node_pose"], False)
    assert 0.5 * float(r @ r) <= 1e-20, 0.5 * float(r @ r)
    res = pm.optimize(g)
    assert res["ok"] and res["error"] <= 1e-20 and pm.pose_distance(res["poses"], truth)[1] <= 1e-9
