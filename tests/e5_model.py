"""Shared by the five-point tests: the host build of mvslam_amd/csrc/five_point.hpp (tests/cpp/five_point_host.cpp as a shared
object, loaded with ctypes), an independent numpy model of the minimal solver, and a numpy model of the RANSAC semantics.

The numpy model shares no arithmetic with the header: null space from numpy.linalg.svd, the ten cubic constraints by polynomial
arithmetic on coefficient arrays, the elimination by numpy.linalg.solve, the tenth-degree polynomial by numpy.polymul, its roots
by numpy.roots (companion-matrix eigenvalues); real roots are those with |Im z| <= 1e-8 |z|.  With backend="mp" the same model
runs in 50-digit mpmath (used once, to measure the model's own error: DESIGN.md section 4.9)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "five_point_host.cpp")
HOST_FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-Wall", "-Wno-unknown-pragmas"]


@functools.lru_cache(maxsize=None)
def host_lib():
    d = tempfile.mkdtemp(prefix="e5host_")
    so = os.path.join(d, "libfive_point_host.so")
    subprocess.check_call(["g++", *HOST_FLAGS, "-shared", "-fPIC", "-o", so, SRC, "-lm"])
    lib = C.CDLL(so)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    lib.e5_five_point.argtypes = [dp, dp, dp]
    lib.e5_sample5.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_int, ip]
    lib.e5_ransac.argtypes = [dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_uint64, dp, bp, ip, ip, ip, dp,
                              C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.e5_select.argtypes = [dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, dp, C.c_int, C.c_double, ip, ip, dp]
    lib.e5_count.argtypes = [dp, dp, C.c_int, C.c_double]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def host_five_point(p1, p2):
    p1 = np.ascontiguousarray(p1, dtype=np.float64).reshape(10)
    p2 = np.ascontiguousarray(p2, dtype=np.float64).reshape(10)
    E = np.zeros((10, 3, 3))
    n = host_lib().e5_five_point(_dp(p1), _dp(p2), _dp(E))
    return n, E


def host_sample5(seed, hyp, M, sampler):
    idx = (C.c_int * 5)()
    host_lib().e5_sample5(seed, hyp, M, sampler, idx)
    return list(idx)


def host_ransac(p1, p2, thr, H, sampler, seed):
    """the host model of the RANSAC stage: the header's solver and Sampson rule, the device's sampler, a sequential selection"""
    p1, p2 = np.asarray(p1, dtype=np.float64).reshape(-1, 2), np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    m = len(p1)
    P = np.ascontiguousarray(np.hstack([p1, p2]))
    E = np.zeros((3, 3))
    mask = np.zeros(max(m, 1), dtype=np.uint8)
    bh, bt, bc, br = C.c_int(), C.c_int(), C.c_int(), C.c_double()
    nr = np.zeros(H, dtype=np.int32)
    cnt = np.zeros((H, 10), dtype=np.int32)
    got = host_lib().e5_ransac(_dp(P), m, thr, H, sampler, seed, _dp(E), mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(bh),
                               C.byref(bt), C.byref(bc), C.byref(br), nr.ctypes.data_as(C.POINTER(C.c_int32)),
                               cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    return dict(found=bool(got), E=E, mask=mask[:m], best_hyp=bh.value, best_root=bt.value, best_count=bc.value,
                best_residual=br.value, n_roots=nr, count=cnt)


def host_select(models, p1, p2, thr):
    """the host model's selection (e5_select of five_point_host.cpp) over SUPPLIED models: models[h] = list of 3 x 3 matrices.
    Same return value as select_models() below."""
    p1, p2 = np.asarray(p1, dtype=np.float64).reshape(-1, 2), np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    P = np.ascontiguousarray(np.hstack([p1, p2]))
    H, m = len(models), len(p1)
    tab = np.zeros((H, 10, 9))
    nr = np.array([len(ms) for ms in models], dtype=np.int32)
    cnt = -np.ones((H, 10), dtype=np.int32)
    for h, ms in enumerate(models):
        for r, E in enumerate(ms):
            tab[h, r] = np.asarray(E, dtype=np.float64).reshape(9)
            cnt[h, r] = host_lib().e5_count(_dp(tab[h, r]), _dp(P), m, thr)
    bh, bt, br = C.c_int(), C.c_int(), C.c_double()
    i32 = C.POINTER(C.c_int32)
    best = host_lib().e5_select(_dp(tab), nr.ctypes.data_as(i32), cnt.ctypes.data_as(i32), H, _dp(P), m, thr, C.byref(bh),
                                C.byref(bt), C.byref(br))
    return nr, cnt, ((bh.value, bt.value) if best >= 0 else None), max(best, 0), br.value


# ---- numpy model of the RANSAC semantics (count, residual, tie order) on given models -------------------------------------
def sampson_terms(E, p1, p2):
    E = np.asarray(E, dtype=np.float64).reshape(9)
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    a0 = (E[0] * x1 + E[1] * y1) + E[2]
    a1 = (E[3] * x1 + E[4] * y1) + E[5]
    a2 = (E[6] * x1 + E[7] * y1) + E[8]
    b0 = (E[0] * x2 + E[3] * y2) + E[6]
    b1 = (E[1] * x2 + E[4] * y2) + E[7]
    r = (x2 * a0 + y2 * a1) + a2
    return r * r, ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1


def select_models(models, p1, p2, thr):
    """models[h] = list of 3 x 3 matrices (root order).  Returns (n_roots, count[H][10], winner (hyp, root), count, residual)."""
    H = len(models)
    nr = np.array([len(ms) for ms in models], dtype=np.int32)
    cnt = -np.ones((H, 10), dtype=np.int32)
    inl = {}
    for h, ms in enumerate(models):
        for r, E in enumerate(ms):
            num, den = sampson_terms(E, p1, p2)
            ok = (den > 0.0) & (num <= thr * den)
            cnt[h, r] = int(ok.sum())
            inl[h, r] = (ok, num, den)
    best = cnt.max() if H else -1
    if best < 0:
        return nr, cnt, None, 0, 0.0
    win, wres = None, None
    for h in range(H):
        for r in range(nr[h]):
            if cnt[h, r] != best:
                continue
            ok, num, den = inl[h, r]
            s = 0.0
            for i in np.nonzero(ok)[0]:   # ONE sequential binary64 sum, i ascending
                s = s + num[i] / den[i]
            if win is None or s < wres:
                win, wres = (h, r), s
    return nr, cnt, win, int(best), wres


# ---- the independent model of the minimal solver -----------------------------------------------------------------------------
_LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_QUAD = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 2, 0), (0, 1, 1), (0, 1, 0), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
_CUB = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0), (1, 0, 2),
        (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def _mul(a, ma, b, mb, mo, zero):
    out = [zero] * len(mo)
    for i, ea in enumerate(ma):
        for j, eb in enumerate(mb):
            k = mo.index(_add(ea, eb))
            out[k] = out[k] + a[i] * b[j]
    return out


def normalise(E):
    E = np.asarray(E, dtype=np.float64).reshape(9)
    E = E * (np.sqrt(2.0) / np.sqrt((E * E).sum()))
    k = int(np.argmax(np.abs(E)))
    return (E if E[k] > 0 else -E).reshape(3, 3)


def design_matrix(p1, p2):
    p1, p2 = np.asarray(p1).reshape(5, 2), np.asarray(p2).reshape(5, 2)
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    one = np.ones(5)
    return np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, one], axis=1)


def model_five_point(p1, p2, backend="np"):
    """Returns (list of normalised E for the real roots, ascending z; z roots as complex array; flag: near a double root)."""
    A = design_matrix(p1, p2)
    if backend == "np":
        N = np.linalg.svd(A)[2][5:9]           # rows: X, Y, Z, W
        zero, conv = 0.0, float
    else:
        import mpmath as mp
        mp.mp.dps = 50
        U, S, V = mp.svd_r(mp.matrix(A.tolist()), full_matrices=True)
        N = [[V[5 + j, e] for e in range(9)] for j in range(4)]
        zero, conv = mp.mpf(0), mp.mpf
    ent = [[N[v][e] for v in range(4)] for e in range(9)]    # linear polynomial of entry e
    half = conv(1) / 2

    def q(a, b):
        return _mul(ent[a], _LIN, ent[b], _LIN, _QUAD, zero)

    def sub(a, b):
        return [x - y for x, y in zip(a, b)]

    def addl(*ps):
        out = list(ps[0])
        for p in ps[1:]:
            out = [x + y for x, y in zip(out, p)]
        return out

    rows = []
    c0, c1, c2 = sub(q(4, 8), q(5, 7)), sub(q(5, 6), q(3, 8)), sub(q(3, 7), q(4, 6))
    rows.append(addl(*[_mul(c, _QUAD, ent[j], _LIN, _CUB, zero) for j, c in enumerate((c0, c1, c2))]))
    tr = addl(*[q(e, e) for e in range(9)])
    for i in range(3):
        lam = []
        for k in range(3):
            l = addl(*[q(3 * i + m, 3 * k + m) for m in range(3)])
            if k == i:
                l = [x - half * t for x, t in zip(l, tr)]
            lam.append(l)
        for j in range(3):
            rows.append(addl(*[_mul(lam[k], _QUAD, ent[3 * k + j], _LIN, _CUB, zero) for k in range(3)]))
    if backend == "np":
        Mx = np.array(rows, dtype=np.float64)
        Rr = np.linalg.solve(Mx[:, :10], Mx[:, 10:])
        pm, pa, ps = np.polymul, np.polyadd, np.polysub
    else:
        Mx = mp.matrix(rows)
        cols = [mp.lu_solve(Mx[:, :10], Mx[:, 10 + j]) for j in range(10)]
        Rr = [[cols[j][i] for j in range(10)] for i in range(10)]

        def pm(a, b):
            out = [zero] * (len(a) + len(b) - 1)
            for i, x in enumerate(a):
                for j, y in enumerate(b):
                    out[i + j] = out[i + j] + x * y
            return out

        def pa(a, b):
            n = max(len(a), len(b))
            a, b = [zero] * (n - len(a)) + list(a), [zero] * (n - len(b)) + list(b)
            return [x + y for x, y in zip(a, b)]

        def ps(a, b):
            return pa(a, [-x for x in b])
    B = []
    for i in range(3):
        a, b = Rr[4 + 2 * i], Rr[5 + 2 * i]
        # descending powers of z
        B.append(([-b[0], a[0] - b[1], a[1] - b[2], a[2]], [-b[3], a[3] - b[4], a[4] - b[5], a[5]],
                  [-b[6], a[6] - b[7], a[7] - b[8], a[8] - b[9], a[9]]))
    p1_ = ps(pm(B[0][1], B[1][2]), pm(B[0][2], B[1][1]))
    p2_ = ps(pm(B[0][2], B[1][0]), pm(B[0][0], B[1][2]))
    p3_ = ps(pm(B[0][0], B[1][1]), pm(B[0][1], B[1][0]))
    c = pa(pa(pm(p1_, B[2][0]), pm(p2_, B[2][1])), pm(p3_, B[2][2]))
    if backend == "np":
        roots = np.roots(c)
        pv = np.polyval
    else:
        roots = mp.polyroots(c, maxsteps=500, extraprec=400)
        pv = lambda p, z: mp.polyval(p, z)   # noqa: E731
        roots_c = np.array([complex(r) for r in roots])
    rc = roots if backend == "np" else roots_c
    az = np.abs(rc)
    rel_im = np.abs(rc.imag) / np.maximum(az, 1e-300)
    shaky = bool(np.any((rel_im > 1e-8) & (rel_im < 1e-4)))
    for i in range(len(rc)):
        for j in range(i):
            if abs(rc[i] - rc[j]) <= 1e-6 * max(az[i], az[j]):
                shaky = True
    out = []
    order = np.argsort(rc.real)
    for i in order:
        if rel_im[i] > 1e-8:
            continue
        z = roots[i].real
        d = pv(p3_, z)
        x, y = pv(p1_, z) / d, pv(p2_, z) / d
        E = [ent[e][0] * x + ent[e][1] * y + ent[e][2] * z + ent[e][3] for e in range(9)]
        out.append(normalise([float(v) for v in E]) if backend == "np" else E)
    if backend != "np":
        import mpmath as mp
        outn = []
        for E in out:
            f = mp.sqrt(sum(v * v for v in E))
            outn.append(normalise([float(v * mp.sqrt(2) / f) for v in E]))
        out = outn
    return out, rc, shaky


def random_sample(rng):
    """a random pose with |omega| <= 0.3, unit baseline, depths in [2, 10]: (p1, p2, true E normalised)"""
    om = rng.normal(size=3)
    om *= rng.uniform(0, 0.3) / np.linalg.norm(om)
    th = np.linalg.norm(om)
    Kx = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    R = np.eye(3) + (np.sin(th) / th) * Kx + ((1 - np.cos(th)) / th ** 2) * (Kx @ Kx) if th > 0 else np.eye(3)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    z = rng.uniform(2, 10, size=5)
    X = np.stack([rng.uniform(-0.5, 0.5, 5) * z, rng.uniform(-0.5, 0.5, 5) * z, z], axis=1)
    X2 = X @ R.T + t
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:], normalise(tx @ R)


def match_sets(A, B):
    """greedy one-to-one matching of two equally long lists of 3 x 3 matrices by max-abs distance; returns the largest distance"""
    if len(A) != len(B):
        return np.inf
    left = list(range(len(B)))
    worst = 0.0
    for a in A:
        d = [np.abs(a - B[j]).max() for j in left]
        k = int(np.argmin(d))
        worst = max(worst, d[k])
        left.pop(k)
    return worst


def constraint_residuals(E, p1, p2):
    """(largest |x2^T E x1| over the five points, |det E|, max |2 E E^T E - tr(E E^T) E|) of a normalised E"""
    h1 = np.hstack([p1, np.ones((5, 1))])
    h2 = np.hstack([p2, np.ones((5, 1))])
    epi = np.abs(np.einsum("ij,jk,ik->i", h2, E, h1)).max()
    EEt = E @ E.T
    return epi, abs(np.linalg.det(E)), np.abs(2 * EEt @ E - np.trace(EEt) * E).max()
