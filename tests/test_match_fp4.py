"""The FP4 matrix-core matcher (match_mfma_kernel) against the oracle at the edges of its arithmetic.

The kernel computes Hamming distances as an e2m1 GEMM whose binary32 accumulators start at the row's key base
(|t| + 257) * 4096 + index and leave key = (|t| + 257 - 2 dot) * 4096 + index.  That is exact only if the matrix core sums
exactly; these cases put the largest and smallest keys, the top of the index field, ties across tiles and around the cap
of the capped variant, and partly padded tiles through it, and compare every match list byte for byte with the oracle.

Every batch has 512 matrix-core workgroups (32 pairs at max_kp 4096, 64 at 2048), the launch rule's threshold (two per CU),
so the matrix-core kernel serves it; max_dist < 0 takes the uncapped variant (match_mfma_kernel<false>), the other settings the
capped one (match_mfma_kernel<true>, cap C = the smallest integer distance with ratio * C > max_dist).
"""
import numpy as np
import pytest

import helpers
import oracle_lib as o
from mvslam_amd import capi, synth

pytestmark = pytest.mark.gpu

P, N = 32, 4096                      # max_kp = 4096: train index 4095 is the top of the key's 12-bit index field
P2, N2 = 64, 2048                    # the other cases: 8 workgroups per pair
MM_QUERIES_PER_GROUP = 256
ONES, ZEROS = np.full(32, 255, dtype=np.uint8), np.zeros(32, dtype=np.uint8)

# (ratio, max_dist): no limit (uncapped variant), then caps C = 15, 21, 4 and 81
SETTINGS = ((0.7, -1.0), (0.7, 10.0), (1.0, 20.0), (0.9, 3.0), (0.75, 60.0))


def _flip(row, bits):
    r = row.copy()
    for bit in bits:
        r[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return r


def _run(ctx, d1, d2, n1, n2, settings, desc_bytes=32, matrix_core=True, oracle=None):
    """every pair of a batch against the oracle's match list, byte for byte, at every (ratio, max_dist) of `settings`.
    matrix_core: the batch must have at least 512 matrix-core workgroups (True) or fewer (False: the vector kernel serves
    256-bit descriptors too); oracle(p, ratio, max_dist): the oracle's list of pair p, if the caller keeps one"""
    P, N = d1.shape[:2]
    assert (-(-N // MM_QUERIES_PER_GROUP) * P >= 512) == matrix_core
    if oracle is None:
        oracle = lambda p, ratio, max_dist: o.match_visual_features(d1[p, :n1[p]], d2[p, :n2[p]], ratio, max_dist)
    assert np.all(n1 >= 2)                                # the oracle's ratio test needs two trains
    rng = np.random.default_rng(99)
    kp = np.zeros((P, N, 2), dtype=np.float32)
    kp[..., 0] = rng.uniform(0, 640, size=(P, N))
    kp[..., 1] = rng.uniform(0, 480, size=(P, N))
    K = np.tile(synth.K_DEFAULT.reshape(1, 9), (P, 1))
    b = capi.Batch(ctx, P, N, desc_bytes)
    try:
        b.upload(0, d1, kp, n1, d2, kp, n2, K, np.arange(P, dtype=np.int64))
        for ratio, max_dist in settings:
            prm = capi.default_params(num_hypotheses=64, sampler=capi.SAMPLER_PHILOX, seed=1, max_error_sq=1e-2, ratio=ratio,
                                      max_dist=max_dist)
            b.run(prm)
            b.sync()
            out = b.download(mask=False, points=False)
            refs = helpers.threads(lambda p: oracle(p, ratio, max_dist), list(range(P)))
            total = 0
            for p in range(P):
                ref = refs[p]
                assert ref is not None, (ratio, max_dist, p)
                m = int(out["results"][p]["n_matches"])
                got = out["matches"][p][:m]
                if m != len(ref) or got.tobytes() != ref.tobytes():   # the difference, printed before the assertion
                    g = {(int(x["queryIdx"]), int(x["trainIdx"]), float(x["distance"])) for x in got}
                    r = {(int(x["queryIdx"]), int(x["trainIdx"]), float(x["distance"])) for x in ref}
                    print("ratio %g max_dist %g pair %d n1 %d n2 %d: device only %s, oracle only %s"
                          % (ratio, max_dist, p, n1[p], n2[p], sorted(g - r)[:12], sorted(r - g)[:12]))
                assert m == len(ref), (ratio, max_dist, p, m, len(ref))
                assert out["matches"][p][:m].tobytes() == ref.tobytes(), (ratio, max_dist, p)
                total += m
            assert total > 0, (ratio, max_dist)
    finally:
        b.close()


def test_match_fp4_key_extremes(ctx):
    """All-ones and all-zero descriptors and train index 4095 at max_kp = 4096.  An all-ones query against the all-ones
    train row has dot = |t| = 256: the smallest key (distance field 1); an all-zero query against it: the largest (field
    513, index 4095).  Pair 0: random rows with the extremes planted at the top of the index field; pair 1: every train row
    all-ones but one with a cleared bit, every query all-ones or all-zero (all ties at equal distance); pair 2: every train
    row all-zero but row 4095 all-ones; pair 3: every descriptor all-zero (every distance 0: nothing passes)."""
    rng = np.random.default_rng(2026)
    d1 = rng.integers(0, 256, size=(P, N, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, size=(P, N, 32), dtype=np.uint8)
    n1 = np.full(P, N, dtype=np.int32)
    n2 = np.full(P, N, dtype=np.int32)
    d1[0, 4095], d1[0, 4094] = ONES, ZEROS
    d2[0, 0:8], d2[0, 8:16], d2[0, 4095] = ONES, ZEROS, ONES
    d2[0, 16] = _flip(ONES, [5])                          # distance 1 from row 4095
    d1[1] = _flip(ONES, [0])
    d1[1, 4095] = ONES
    d2[1, 0::2], d2[1, 1::2] = ONES, ZEROS
    d1[2] = ZEROS
    d1[2, 4095] = ONES
    d2[2, 0::3], d2[2, 1::3], d2[2, 2::3] = ONES, ZEROS, _flip(ZEROS, [255])
    d1[3], d2[3] = ZEROS, ZEROS
    for p in range(4, P):                                 # the extremes once in every tile position of the last tile
        r = 4064 + p
        d1[p, r] = ONES
        d2[p, :4] = ONES
        d2[p, 4:8] = ZEROS
        d1[p, 100] = ZEROS
    _run(ctx, d1, d2, n1, n2, SETTINGS)


def test_match_fp4_ties_across_tiles_and_cap(ctx):
    """A query with two or three partners at planted distances: equal distances in different 32-row tiles, in the two lane
    halves of a tile and straddling a tile boundary, at and around every cap C and every max_dist of SETTINGS (the nearer
    partner sometimes at the higher index).  Ties at the nearest distance must reject the query (D0 == D1); one apart, the
    ratio and the limit decide.  Capped and uncapped variants, five (ratio, max_dist) settings."""
    rng = np.random.default_rng(77)
    d1 = rng.integers(0, 256, size=(P2, N2, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, size=(P2, N2, 32), dtype=np.uint8)
    n1 = rng.integers(1900, N2 + 1, size=P2).astype(np.int32)
    n2 = rng.integers(1000, N2 + 1, size=P2).astype(np.int32)
    dists = [0, 1, 2, 3, 4, 5, 9, 10, 14, 15, 20, 21, 59, 60, 80, 81]
    combos = [(d, d) for d in dists] + [(d, d + 1) for d in dists] + [(d + 1, d) for d in dists[:8]]
    # the two rows of a combo, within its own 44 rows: the same position of two tiles, two tiles and the other lane half
    # (a tile's row r sits in lane half (r >> 2) & 1), the two sides of a tile boundary
    spans = [(0, 32), (3, 40), (31, 32), (5, 41), (2, 38)]
    for p in range(P2):
        for i, (fa, fb) in enumerate(combos):
            row = rng.integers(0, 256, size=32, dtype=np.uint8)
            bits = rng.permutation(256)[:fa + fb]
            ra, rb = _flip(row, bits[:fa]), _flip(row, bits[fa:])
            a, s = spans[(i + p) % len(spans)]
            ia, ib = 44 * i + a, 44 * i + s
            if (i + p) % 2:
                ia, ib = ib, ia
            d1[p, ia], d1[p, ib], d2[p, i] = ra, rb, row
        # three rows at distance 10 in three tiles and one at 9 (even pairs: the 9 wins) or 10 (odd: a four-way tie)
        row = rng.integers(0, 256, size=32, dtype=np.uint8)
        for r in (1856, 1888, 1890):
            d1[p, r] = _flip(row, rng.permutation(256)[:10])
        d1[p, 1899] = _flip(row, rng.permutation(256)[:9 + p % 2])
        d2[p, 900] = row
    _run(ctx, d1, d2, n1, n2, SETTINGS)


def test_match_fp4_ragged_last_tile(ctx):
    """Train counts that leave the last 32-row tile partly padding (1 to 31 real rows), query counts off the 32- and
    256-query grids; each pair's true partners sit in the partial tile, including its last real row, and a padded row's
    all-zero bits (which an all-zero query would match at distance 0 if padding were live) face all-zero queries."""
    rng = np.random.default_rng(3)
    d1 = rng.integers(0, 256, size=(P2, N2, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, size=(P2, N2, 32), dtype=np.uint8)
    n1 = np.array([32 * rng.integers(2, N2 // 32) + 1 + (p % 31) for p in range(P2)], dtype=np.int32)
    n1[0], n1[1] = N2 - 1, 33
    n2 = np.array([rng.integers(1, N2 + 1) for _ in range(P2)], dtype=np.int32)
    n2[0], n2[1] = N2 - 31, 257
    for p in range(P2):
        last0 = (n1[p] - 1) // 32 * 32
        d1[p, n1[p]:] = ZEROS                                 # rows past the end (never read: they are padding)
        k = min(int(n2[p]), 24)
        for j in range(k):
            r = last0 + j % (n1[p] - last0)
            if j == 0:
                r = n1[p] - 1
            d2[p, j] = _flip(d1[p, r], rng.permutation(256)[:j % 6])
        if n2[p] > 30:
            d2[p, 30] = ZEROS
    _run(ctx, d1, d2, n1, n2, SETTINGS)
