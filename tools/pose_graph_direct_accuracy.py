"""Writes profiles/pose_graph_direct_vs_exact.json: the numpy model of the direct LM step (tests/pg_direct_model.py, the
block-scaled skyline solve) against the model with numpy's dense Cholesky (tests/posegraph_model.py, solver="exact") on the
fixtures of the direct path.  The largest rotation and translation gaps are what the GPU tolerance of tests/test_pg_direct.py
rests on; tests/test_pg_direct_host.py asserts that a fresh computation does not exceed what is committed.  CPU only.

    python tools/pose_graph_direct_accuracy.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pg_direct_model as dm          # noqa: E402
import pg_marginals_model as pgm      # noqa: E402
import posegraph_model as pm          # noqa: E402


def fixtures():
    """name -> (make, keywords of optimize): what tests/test_pg_direct.py runs on the device"""
    out = {"ring17": (lambda: pm.ring(17), {}), "star70": (pm.star, {}), "ring200": (lambda: pm.ring(200, chords=(5,)), {}),
           "ring257": (lambda: pm.ring(257, chords=(7, 40)), {}),
           "ring24_relabelled": (pgm.FIXTURES["ring24_relabelled"], {}), "chain40": (pgm.chain40, {}),
           "near_pi_ring": (lambda: pm.near_pi_ring()[0], {}), "ring40": (lambda: pm.ring(40), {}),
           "ring17_a16": (lambda: pm.permuted_ring("ring17_a16"), {}), "ring17_a9": (lambda: pm.permuted_ring("ring17_a9"), {}),
           "far_off20": (lambda: pm.far_off(20), {}), "far_off20_two": (lambda: pm.far_off(20), dict(lm=dict(max_iterations=2)))}
    for name in ("loose_anchor17", "loose_anchor17_swapped", "lambda_upper20"):
        out[name] = pm.PARAM_RUNS[name]
    return out


def measure():
    rows, rot, trans = {}, 0.0, 0.0
    for name, (make, kw) in fixtures().items():
        g = make()
        a, b = pm.optimize(g, **kw), dm.optimize_direct(g, **kw)
        dr, dt = pm.pose_distance(a["poses"], b["poses"])
        _, _, blocks = pgm.graph_envelope(g)
        rows[name] = dict(nodes=int(g["node_pose"].shape[0]), edges=int(len(g["edge_src"])), envelope_blocks=blocks,
                          iterations_exact=a["iterations"], iterations_direct=b["iterations"], rejected_exact=a["rejected_steps"],
                          rejected_direct=b["rejected_steps"], exit_exact=a["exit"], exit_direct=b["exit"], rotation=dr,
                          translation=dt, error_exact=a["error"], error_direct=b["error"], min_pivot=b["min_pivot"],
                          decision_margin=min(pm.decision_margin(b, kw.get("lm")), 1e300))
        rot, trans = max(rot, dr), max(trans, dt)
    return dict(what="numpy model, the block-scaled skyline solve against numpy's dense Cholesky as the linear solver of the LM "
                     "step: largest pose difference", rotation=rot, translation=trans, fixtures=rows)


if __name__ == "__main__":
    out = measure()
    with open(os.path.join(ROOT, "profiles", "pose_graph_direct_vs_exact.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "fixtures"}))
    for k, v in out["fixtures"].items():
        print(k, v["nodes"], v["envelope_blocks"], "%.2e %.2e" % (v["rotation"], v["translation"]), v["iterations_exact"],
              v["iterations_direct"], v["rejected_exact"], v["rejected_direct"], v["exit_direct"], "%.3g" % v["decision_margin"])
