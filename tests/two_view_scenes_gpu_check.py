#!/usr/bin/env python3
"""GPU check of the RANSAC pre-screen on the scene families of tests/two_view_scenes.py, hypothesis by hypothesis (run by
tests/test_two_view_scenes.py in its own process with MVS_USE_DEBUG_LIB=1; the checks are tests/prescreen_gpu_check.py's).

One point-fed pair per family (300 matches, 512 hypotheses) in one batch.  At threshold 1e-2, for every hypothesis of every pair
and both record precisions:
  * the state byte is 0 exactly when the oracle rejects the sample;
  * a certified record satisfies  | r_i(F_J) - r_i(F~) | <= band  for every match i, and  U >= count_J >= L.
At 1e-2 and 2e-3, per pair: the stage forced exact, forced pre-screened (both precisions, both matrix-core counting variants)
and with the probe deciding gives identical bytes, and those equal the oracle's sfm_solve.
A degenerate family that certifies little is correct behaviour: only the sideways control must certify more than half (asserted
by the calling test); the certified share and the probe's choice are reported per family and threshold.
Prints one JSON line with the statistics; exit code 0 = all checks passed."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MVS_USE_DEBUG_LIB"] = "1"
import helpers  # noqa: E402
import oracle_lib as o  # noqa: E402
import prescreen_gpu_check as pc  # noqa: E402
import two_view_scenes as tv  # noqa: E402
from mvslam_amd import capi  # noqa: E402


def main():
    fams = list(tv.FAMILIES)
    P, N, H, m = len(fams), 320, tv.H, tv.M
    K = tv.synth.K_DEFAULT
    scenes = [tv.scene(tv.SCENE_SEED, m, f) for f in fams]
    uv1 = np.zeros((P, N, 2))
    uv2 = np.zeros((P, N, 2))
    for p, sc in enumerate(scenes):
        uv1[p, :m], uv2[p, :m] = sc["uv1"], sc["uv2"]
    pts = [(o.normalize_points(K, sc["uv1"]), o.normalize_points(K, sc["uv2"])) for sc in scenes]
    sizes = [m] * P
    gidx = np.arange(P, dtype=np.int64) * 3
    ctx = capi.Context(0)
    lib = capi.lib()
    b = capi.Batch(ctx, P, N, 32)
    b.upload_intrinsics(0, K, gidx, count=P)
    stats = dict(viol=0, count_viol=0, families={f: {} for f in fams}, probe_mode={f: {} for f in fams},
                 certified_share={f: {} for f in fams})
    for thr in tv.THRESHOLDS:
        prm = capi.default_params(num_hypotheses=H, sampler=capi.SAMPLER_PHILOX, seed=tv.SAMPLER_SEED, max_error_sq=thr)
        run = lambda: b.run_points(prm, uv1, uv2, sizes)   # noqa: E731
        run()
        b.sync()
        for pmode in (2, 1):
            st = lib.mvs_debug_prescreen_only(b._h, C.byref(prm), C.c_int(P), C.c_int(pmode))
            assert st == 0, st
            for p, fam in enumerate(fams):
                state = np.zeros(H, dtype=np.uint8)
                info = (C.c_int32 * 4)()
                st = lib.mvs_debug_read_hyp_rec(b._h, C.c_int(p), C.c_int(H), None, state.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                None, info)
                assert st == 0 and info[0] == pmode
                stats["certified_share"][fam]["%g/%d" % (thr, pmode)] = round(float((state == 1).mean()), 4)
                if thr != 1e-2:
                    continue
                s = dict(hyp=0, invalid=0, certified=0, need_exact=0, worst_ratio=0.0, viol=0, count_viol=0)
                pc.check_pair_records(lib, b, p, H, pmode, thr, pts[p][0], pts[p][1], tv.SAMPLER_SEED + int(gidx[p]), s)
                stats["families"][fam][str(pmode)] = s
                stats["viol"] += s["viol"]
                stats["count_viol"] += s["count_viol"]
        # the whole stage in every mode; the probe's choice per pair is read behind the run that let it decide
        lib.mvs_debug_set_count_dense(C.c_int(1))
        lib.mvs_debug_set_prescreen_force(C.c_int(-1))
        run()
        b.sync()
        for p, fam in enumerate(fams):
            info = (C.c_int32 * 4)()
            assert lib.mvs_debug_read_hyp_rec(b._h, C.c_int(p), C.c_int(1), None, None, None, info) == 0
            stats["probe_mode"][fam]["%g" % thr] = int(info[0])
        outs = pc.run_every_mode(lib, b, run, stats)
        lib.mvs_debug_set_count_dense(C.c_int(1))
        lib.mvs_debug_set_prescreen_force(C.c_int(1))
        run()
        b.sync()
        chk = b.download()
        for p in range(P):
            pc.check_dense_counts(lib, b, p, H, thr, pts[p][0], pts[p][1], chk["results"][p], stats)
        lib.mvs_debug_set_prescreen_force(C.c_int(-1))
        lib.mvs_debug_set_count_dense(C.c_int(1))
        pc.assert_modes_equal(outs, thr)
        for p, fam in enumerate(fams):
            ref = o.sfm_solve(uv1[p, :m], uv2[p, :m], K, o.make_params(H, o.SAMPLER_PHILOX, tv.SAMPLER_SEED + int(gidx[p]), thr))
            r, tag = outs[1]["results"][p], (fam, thr)
            assert r["n_matches"] == m and bool(r["valid"]) == bool(ref["ok"]), tag
            assert r["best_hyp"] == ref["best_hyp"] and r["best_count"] == ref["best_count"], tag
            assert r["best_residual"] == ref["best_residual"], tag
            assert np.array_equal(outs[1]["mask"][p][:m], ref["mask"][:m]), tag
            if ref["ok"]:
                n = ref["n_points"]
                assert r["n_points"] == n and np.array_equal(outs[1]["point_idx"][p][:n], ref["point_idx"]), tag
                assert helpers.rel_err(r["R"], ref["R"]) <= helpers.TIGHT and helpers.rel_err(r["t"], ref["t"]) <= helpers.TIGHT, tag
                assert helpers.rel_err(outs[1]["points"][p][:n], ref["points"]) <= helpers.TIGHT, tag
    b.close()
    ctx.close()
    print(json.dumps(stats))
    assert stats["viol"] == 0 and stats["count_viol"] == 0


if __name__ == "__main__":
    main()
