"""Loop closures without a GPU: tests/seq_loop_model.py against a second brute force, the selection order, the layouts of
the new ABI structs, synth.make_loop_sequence's revisits, and synth.make_sequence's unchanged bytes."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import seq_loop_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute_score(train, query, ratio, max_dist):
    """bit by bit, query by query, with an insertion that keeps the two smallest distances with multiplicity"""
    if len(train) < 2:
        return 0
    tb = [int.from_bytes(r.tobytes(), "little") for r in train]
    n = 0
    for qr in query:
        q = int.from_bytes(qr.tobytes(), "little")
        d0 = d1 = 1 << 30
        for t in tb:
            d = bin(q ^ t).count("1")
            if d < d0:
                d0, d1 = d, d0
            elif d < d1:
                d1 = d
        f0, f1 = float(np.float32(d0)), float(np.float32(d1))
        if f0 < ratio * f1 and (max_dist < 0 or f0 <= max_dist):
            n += 1
    return n


def test_model_scores_equal_a_second_brute_force():
    rng = np.random.default_rng(1)
    counts = np.array([40, 33, 1, 0, 37], dtype=np.int32)
    for nbytes in (16, 32, 64):
        desc = rng.integers(0, 256, size=(5, 40, nbytes), dtype=np.uint8)
        for f in range(1, 5):
            for r in range(0, 20, 2):
                bits = np.unpackbits(desc[0, r])
                bits[rng.choice(bits.size, size=int(rng.integers(0, 12)), replace=False)] ^= 1
                desc[f, r] = np.packbits(bits)
        desc[0, 1] = desc[0, 0]      # two trains at one distance: D1 = D0, the ratio test fails for their partners
        for ratio, max_dist in ((0.7, -1.0), (0.7, 10.0), (0.9, 3.0), (0.7, 0.0)):
            for gap in (1, 3):
                got = lm.scores(desc, counts, ratio, max_dist, gap)
                for j in range(5):
                    for i in range(5):
                        want = _brute_score(desc[i][:counts[i]], desc[j][:counts[j]], ratio, max_dist) if j - i >= gap else 0
                        assert got[i, j] == want, (nbytes, ratio, max_dist, gap, i, j)
        assert lm.scores(desc, counts, 0.7, -1.0, 1)[0, 1] >= 5
        assert lm.pair_score(desc[0][:2], desc[1][:1], 0.7, -1.0) == 0, "a partner of the duplicated rows passed the ratio test"


def test_selection_order_ties_and_cut():
    sc = np.zeros((6, 6), dtype=np.int32)
    sc[0, 3], sc[1, 3], sc[2, 3] = 5, 9, 5
    sc[0, 4], sc[1, 4], sc[2, 4], sc[3, 4] = 7, 7, 7, 2
    sc[2, 5] = 3
    full, found = lm.select(sc, 3, 2, 100)
    assert full == [(1, 3, 9), (0, 3, 5), (0, 4, 7), (1, 4, 7), (2, 5, 3)] and found == 5
    cut, found = lm.select(sc, 3, 2, 3)
    assert cut == full[:3] and found == 5
    assert lm.select(sc, 10, 2, 100) == ([], 0)
    assert lm.select(sc, 1, 1, 100)[0] == [(1, 3, 9), (0, 4, 7), (2, 5, 3)]


def test_struct_layouts_of_the_loop_types():
    from mvslam_amd import capi

    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "mvslam_hip.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(mvs_loop_select_params), sizeof(mvs_loop_candidate), sizeof(mvs_loop_edge_params));
  printf("%zu %zu %zu\n", offsetof(mvs_loop_select_params, min_score), offsetof(mvs_loop_select_params, top_k),
         offsetof(mvs_loop_select_params, max_candidates));
  printf("%zu %zu %zu %zu\n", offsetof(mvs_loop_candidate, i), offsetof(mvs_loop_candidate, j),
         offsetof(mvs_loop_candidate, score), offsetof(mvs_loop_candidate, accepted));
  printf("%zu %zu %zu\n", offsetof(mvs_loop_edge_params, min_points), offsetof(mvs_loop_edge_params, max_error),
         offsetof(mvs_loop_edge_params, loop_sigma));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        v = list(map(int, subprocess.check_output([os.path.join(d, "p")]).decode().split()))
    S, E, D = capi.LoopSelectParams, capi.LoopEdgeParams, capi.LOOP_CANDIDATE_DTYPE
    assert v[0:3] == [C.sizeof(S), D.itemsize, C.sizeof(E)] == [16, 16, 32]
    assert v[3:6] == [S.min_score.offset, S.top_k.offset, S.max_candidates.offset]
    assert v[6:10] == [D.fields[k][1] for k in ("i", "j", "score", "accepted")]
    assert v[10:13] == [E.min_points.offset, E.max_error.offset, E.loop_sigma.offset]
    for name in ("mvs_seq_loop_scores", "mvs_seq_download_loop_scores", "mvs_seq_select_loops", "mvs_seq_verify_loops",
                 "mvs_seq_add_loop_edges", "mvs_seq_download_loop_candidates"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)


def test_make_loop_sequence_revisits_its_outbound_frames():
    from mvslam_amd import synth

    F, shift = 11, 0.1
    s = synth.make_loop_sequence(F, shift=shift, n_kp=64, n_map=2000)
    out = synth.make_sequence(6, n_kp=64, n_map=2000)
    centre = lambda p: -p[0].T @ p[1]
    H = (F + 1) // 2
    assert s["revisit"].tolist() == [-1] * H + list(range(H - 1, H - 1 - (F - H), -1))
    for f in range(F):
        g = int(s["revisit"][f])
        if g < 0:
            assert np.allclose(s["poses"][f][0], out["poses"][f][0]) and np.allclose(centre(s["poses"][f]), centre(out["poses"][f]))
            continue
        d = centre(s["poses"][f]) - centre(s["poses"][g])
        assert np.allclose(s["poses"][f][0], s["poses"][g][0]), "a revisit looks another way"
        assert abs(np.linalg.norm(d) - shift) < 1e-12 and abs(d[1]) < 1e-15
        assert abs(d @ (centre(s["poses"][1]) - centre(s["poses"][0]))) < 1e-12, "the shift is not sideways"
    assert s["desc"].shape == (F, 64, 32) and s["kp"].dtype == np.float32 and (s["n_kp"] == 64).all()
    # a revisit sees its outbound frame's map points again: many more descriptor matches than a random frame pair
    sc = lm.scores(s["desc"], s["n_kp"], 0.7, 64.0, 1)
    f = F - 2
    assert sc[s["revisit"][f], f] >= 15


def test_make_sequence_bytes_are_unchanged():
    from mvslam_amd import synth

    s = synth.make_sequence(6, n_kp=64, n_map=2000, seed=0x5E9)
    h = hashlib.sha256()
    for k in ("desc", "kp", "n_kp", "K"):
        h.update(s[k].tobytes())
    for R, t in s["poses"]:
        h.update(R.tobytes())
        h.update(t.tobytes())
    assert h.hexdigest() == "ca37208b0c517877dc8a5888e3f0f06c0dc67e8f71a42cbd1f0a0ea7ba86b052"
