"""The vector matcher (match_topk_kernel<DW>, DW = 4, 8, 16) against the oracle at its tile, chunk and key edges.

The kernel stages the trains through a 64 KiB tile of shared memory: 4096 rows of 16 bytes, 2048 of 32, 1024 of 64.  Its 16
wavefronts split a tile into chunks of ceil(rows / 16) rows, each lane keeps the two smallest keys (distance << 16 | train
index) of its query across tiles, and the 16 partial lists are merged at the end.  The cases below put, at max_kp = 4096,
  1 the nearest and second-nearest train on the two sides of every tile edge (and of chunk edges and the ends of the index
    range, which is all a 16-byte batch with its single tile has), equal or one bit apart, at 0, 1 and around every cap of
    SETTINGS; three trains at one distance in different tiles and a fourth at that distance or one bit nearer;
  2 train counts that leave 1, 15, 17, ... rows in the last tile (most wavefronts then have no row), partners in its first
    and last real row, all-zero padding behind them facing all-zero queries, and query counts around the 64-query block;
  3 the largest and the smallest key, the top of the index field, and pairs in which every distance ties
through it at 16, 32 and 64 bytes, and compare every match list byte for byte with the oracle.  Every batch is small enough
(fewer than 512 matrix-core workgroups) that 32-byte descriptors take the vector kernel too.

The data and the oracle's lists are made once per (case, descriptor size); the tests without the gpu mark show on the oracle
alone that every case gives matches at every setting and that the planted ties are rejected."""
import functools

import numpy as np
import pytest

import oracle_lib as o
import test_match_fp4 as mf
from test_match_fp4 import SETTINGS, _flip

N = 4096
SIZES = (16, 32, 64)
CAPS = (15, 21, 4, 81)               # the caps C of SETTINGS (test_match_fp4.py)
PLANTED = sorted({0, 1} | {c + e for c in CAPS for e in (-1, 0, 1)})
assert max(PLANTED) + 2 < 8 * min(SIZES)


def _random(rng, P, db):
    return (rng.integers(0, 256, size=(P, N, db), dtype=np.uint8), rng.integers(0, 256, size=(P, N, db), dtype=np.uint8))


def _edges(db):
    """pairs of train rows either side of every tile edge; in a single tile: of the middle chunk edge; and always of the
    first chunk edge and the two ends of the index range"""
    rows = 65536 // db
    inner = [(k * rows - 1, k * rows) for k in range(1, N // rows)] or [(2047, 2048)]
    chunk = -(-min(rows, N) // 16)
    return inner + [(chunk - 1, chunk), (0, N - 1)]


def tile_boundaries(db):
    """Pair p's edge rows a < b differ in s = p bits (0: the same row twice; 1; 2), so a query made from row a by flipping
    some of those bits and some others has any wanted distances (fa, fb) with fa - fb = s (mod 2): pair 0 and pair 2 hold
    the ties at every planted distance, pair 1 the distances one apart in both orders (the nearer train at the higher index
    and beyond the edge, or in the earlier tile).  Then the four-train cases, rows a quarter of the index range apart (four
    tiles at 64 bytes, two at 32, four chunks of the one tile at 16): three at distance d and the fourth at d - 1 or at d.
    Returns (d1, d2, n1, n2, ties): ties = the (pair, query) whose two nearest trains are equally far."""
    rng = np.random.default_rng(4096 + db)
    P, nbits = 3, 8 * db
    d1, d2 = _random(rng, P, db)
    for p in range(P):                                    # true partners too, so that every setting has matches to compare
        for q in range(2000, 3000):
            d2[p, q] = _flip(d1[p, (q * 7) % N], rng.permutation(nbits)[:q % 6])
    ties = []
    for p in range(P):
        q = 0
        for a, b in _edges(db):
            perm = rng.permutation(nbits)
            S, rest = perm[:p], perm[p:]
            d1[p, b] = _flip(d1[p, a], S)
            for d in PLANTED:
                for fa, fb in ((d, d), (d, d + 1), (d + 1, d), (d, d + 2), (d + 2, d)):
                    if (fa - fb - p) % 2 or abs(fa - fb) > p:
                        continue
                    na = (p + fa - fb) // 2               # flipped bits of S: fa = na + nb, fb = p - na + nb
                    nb = fa - na
                    if nb < 0:
                        continue
                    d2[p, q] = _flip(d1[p, a], list(S[:na]) + list(rest[:nb]))
                    if fa == fb:
                        ties.append((p, q))
                    q += 1
        for i, d in enumerate((1, 4, 10, 15, 21, 81)):
            for tie in (False, True):
                row = rng.integers(0, 256, size=db, dtype=np.uint8)
                base = 100 + 4 * i + 2 * tie
                for t in range(3):
                    d1[p, t * (N // 4) + base + (t + p) % 2] = _flip(row, rng.permutation(nbits)[:d])
                d1[p, 3 * (N // 4) + base] = _flip(row, rng.permutation(nbits)[:d if tie else d - 1])
                d2[p, q] = row
                if tie:
                    ties.append((p, q))
                q += 1
        assert q < 2000
    n = np.full(P, N, dtype=np.int32)
    return d1, d2, n, n.copy(), ties


def short_last_tile(db):
    """One pair per (n1, n2).  Query 0's partner is the last real train row, query 1's row 0 of the last tile, the next 22
    go round the last tile's rows (0 to 5 bits away); rows past n1 are all-zero and queries 30 and n2 - 1 are all-zero: were
    padding live, they would match it at distance 0."""
    rows = 65536 // db
    n1s = sorted({min(v, N) for v in (rows + 1, rows + 15, rows + 17, 2 * rows - 1, N - 1)})
    n2s = (1, 63, 64, 65, N - 1)
    combos = [(a, b) for a in n1s for b in n2s]
    rng = np.random.default_rng(17 + db)
    P, nbits = len(combos), 8 * db
    d1, d2 = _random(rng, P, db)
    for p, (a, b) in enumerate(combos):
        last0 = (a - 1) // rows * rows
        d1[p, a:] = 0
        for j in range(min(b, 24)):
            r = a - 1 if j == 0 else last0 if j == 1 else last0 + j % (a - last0)
            d2[p, j] = _flip(d1[p, r], rng.permutation(nbits)[:j % 6])
        if b > 30:
            d2[p, 30], d2[p, b - 1] = 0, 0
    n1 = np.array([a for a, _ in combos], dtype=np.int32)
    n2 = np.array([b for _, b in combos], dtype=np.int32)
    return d1, d2, n1, n2, []


def key_extremes(db):
    """Pair 0: random rows, train 4095 all-ones and 4094 all-zero, queries all-ones, all-zero and one bit from all-ones.
    Pair 1: every train all-ones less one bit but train 4095 all-ones, queries all-ones (distance 0 at the top index, the
    second at 1) or all-zero (every distance ties).  Pair 2: every train all-zero but train 4095 all-ones; an all-ones
    query has distances 0 and 8 * desc_bytes, the largest value of the key's distance half, an all-zero query ties at 0.
    Pair 3: every train all-zero but train 4095 with one bit set: the two keys of an all-ones query hold the largest
    distance and the one below it.  Pair 4: every descriptor all-zero; nothing may pass.  Pair 5: every train is one row R
    but one, in the second tile where there is one, that differs from it in one bit; queries R (all ties) and that row."""
    rng = np.random.default_rng(2026 + db)
    P, nbits = 6, 8 * db
    ONES, ZEROS = np.full(db, 255, dtype=np.uint8), np.zeros(db, dtype=np.uint8)
    d1, d2 = _random(rng, P, db)
    d1[0, N - 1], d1[0, N - 2] = ONES, ZEROS
    d2[0, 0:8], d2[0, 8:16], d2[0, N - 1], d2[0, 16] = ONES, ZEROS, ONES, _flip(ONES, [5])
    d1[1] = _flip(ONES, [0])
    d1[1, N - 1] = ONES
    d2[1, 0::2], d2[1, 1::2] = ONES, ZEROS
    d1[2] = ZEROS
    d1[2, N - 1] = ONES
    d2[2, 0::3], d2[2, 1::3], d2[2, 2::3] = ONES, ZEROS, _flip(ZEROS, [nbits - 1])
    d1[3] = ZEROS
    d1[3, N - 1] = _flip(ZEROS, [3])
    d2[3, 0::2], d2[3, 1::2] = ONES, _flip(ZEROS, [3])
    d1[4], d2[4] = ZEROS, ZEROS
    row = rng.integers(0, 256, size=db, dtype=np.uint8)
    odd = (65536 // db + 3) % N
    d1[5], d2[5] = row, row
    d1[5, odd] = _flip(row, [nbits // 2])
    d2[5, 1::2] = d1[5, odd]
    n = np.full(P, N, dtype=np.int32)
    ties = [(1, 1), (1, N - 1), (2, 1), (5, 0), (5, N - 2)] + [(4, q) for q in (0, 63, 64, N - 1)]
    return d1, d2, n, n.copy(), ties


CASES = dict(tile_boundaries=tile_boundaries, short_last_tile=short_last_tile, key_extremes=key_extremes)


@functools.lru_cache(maxsize=None)
def _case(name, db):
    """the data of a case and a cache of the oracle's lists: made once, read by every test"""
    d1, d2, n1, n2, ties = CASES[name](db)
    for a in (d1, d2, n1, n2):
        a.setflags(write=False)
    lists = {}

    def oracle(p, ratio, max_dist):
        key = (p, ratio, max_dist)
        if key not in lists:
            lists[key] = o.match_visual_features(d1[p, :n1[p]], d2[p, :n2[p]], ratio, max_dist)
        return lists[key]

    return d1, d2, n1, n2, ties, oracle


@pytest.mark.parametrize("db", SIZES)
@pytest.mark.parametrize("name", list(CASES))
def test_cases_are_not_vacuous(name, db):
    d1, d2, n1, n2, ties, oracle = _case(name, db)
    P = len(n1)
    assert -(-N // mf.MM_QUERIES_PER_GROUP) * P < 512 and np.all(n1 >= 2) and np.all(n1 <= N) and np.all(n2 <= N)
    assert name == "short_last_tile" or len(ties) >= 9
    for ratio, max_dist in SETTINGS:
        lists = [oracle(p, ratio, max_dist) for p in range(P)]
        assert all(m is not None for m in lists)
        assert sum(len(m) for m in lists) > 0, (ratio, max_dist)
        for p, q in ties:
            assert q not in lists[p]["queryIdx"], (ratio, max_dist, p, q)
    if name == "tile_boundaries":         # one bit apart, the planted queries match the rows on both sides of every edge
        for ratio, max_dist in SETTINGS:
            m = oracle(1, ratio, max_dist)
            got = set(m["trainIdx"][m["queryIdx"] < 2000].tolist())
            assert {r for e in _edges(db) for r in e} <= got, (ratio, max_dist)
    if name == "short_last_tile":         # the last real row and row 0 of the last tile are matched; padding never is
        rows = 65536 // db
        for p in range(P):
            m = oracle(p, 0.7, -1.0)
            assert (n1[p] - 1) in m["trainIdx"] and m["trainIdx"].max() < n1[p]
            assert n2[p] < 2 or (n1[p] - 1) // rows * rows in m["trainIdx"]
            assert not (n2[p] > 30 and 30 in m["queryIdx"])
    if name == "key_extremes":
        m = oracle(2, 0.7, -1.0)
        assert len(m) == len(range(0, N, 3)) and np.all(m["trainIdx"] == N - 1) and np.all(m["distance"] == 0)
        for ratio, max_dist in SETTINGS:  # pair 3: the all-ones queries (even) never pass, the others always
            assert len(oracle(4, ratio, max_dist)) == 0
            assert np.array_equal(oracle(3, ratio, max_dist)["queryIdx"], np.arange(1, N, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("db", SIZES)
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_vector_matcher_equals_the_oracle(ctx, name, db):
    d1, d2, n1, n2, _, oracle = _case(name, db)
    mf._run(ctx, d1, d2, n1, n2, SETTINGS, desc_bytes=db, matrix_core=False, oracle=oracle)
