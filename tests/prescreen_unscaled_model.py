"""numpy model of the pre-screen with RELAXED roots and quotients on the way to F~: the sixteen
Hartley distances, the two scale quotients, the eight column norms and reflector scales of the Householder QR, the pivot
reciprocals and the norm / reciprocal of the verified singular triplet are taken within a stated multiple of u instead of
correctly rounded (prescreen.hpp sqrt_relaxed_h, rcp_relaxed).  Everything else is tests/prescreen_model.py, imported and
not restated; the constants that pay for the relaxation (RHO_C, TRIP_E) are the device's new ones.

The relaxed sequences are evaluated in the device's operation order with an exact fma (rational arithmetic, one rounding).
What a CPU cannot reproduce is the hardware's seed: v_rsq_f64 / v_rcp_f64 are modelled as the true value times (1 + e),
|e| <= 2^-26 (assumption (A3), the one sqrt_fast / div_fast already make).  `Seeds` picks e: +2^-26, -2^-26 or random."""
import os
import re
from fractions import Fraction

import numpy as np

import prescreen_model as pm

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvslam_amd", "csrc", "prescreen.hpp")


def header_constant(name):
    """`constexpr double <name> = <literal>;` of prescreen.hpp, decimal or hexadecimal floating literal"""
    m = re.search(r"constexpr\s+double\s+%s\s*=\s*([-+0-9a-fA-FxXpP.]+)\s*;" % re.escape(name), open(HEADER).read())
    assert m, "prescreen.hpp has no constexpr double %s" % name
    return float.fromhex(m.group(1)) if "x" in m.group(1).lower() else float(m.group(1))


U = pm.U
SEED_E = 2.0 ** -26
# the device's own constants, read from its header: the model cannot drift from what is compiled
RHO_C = header_constant("kPsRhoC")      # rho = RHO_C sqrt(S): 1603 u ||A||_F (1548 u + 4.1 u of the relaxed column norms + 50.2 u of A - A~)
TRIP_E = header_constant("kPsTrip")     # kappa: 1e-12 + 1e-14 for de-normalising with scales within SCALE_U u of the exact path's
SCALE_U = header_constant("kPsScaleU")  # | s~ / s - 1 | <= SCALE_U u
Q_MIN = header_constant("kPsQMin")      # range test of the relaxed normalisation: every radicand >= Q_MIN, both means of roots < SC_MAX
SC_MAX = header_constant("kPsScMax")


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


class Seeds:
    """relative error of the next hardware seed: mode 'plus' / 'minus' (the extremes) or 'rand' (uniform in +-2^-26)"""

    def __init__(self, mode="rand", seed=1):
        self.mode, self.rng = mode, np.random.default_rng(seed)

    def __call__(self):
        if self.mode == "plus":
            return SEED_E
        if self.mode == "minus":
            return -SEED_E
        return float(self.rng.uniform(-SEED_E, SEED_E))


def sqrt_relaxed_h(x, seeds):
    """prescreen.hpp sqrt_relaxed_h: (g, h), g within 1.01 u of sqrt(x), h the unrefined half reciprocal root"""
    y = float(1.0 / np.sqrt(x)) * (1.0 + seeds())
    g = x * y
    h = y * 0.5
    r = fma(-h, g, 0.5)
    g = fma(g, r, g)
    d = fma(-g, g, x)
    return fma(d, h, g), h


def rcp_relaxed(x, seeds):
    """prescreen.hpp rcp_relaxed: within 3.01 u of 1 / x"""
    r = (1.0 / x) * (1.0 + seeds())
    return fma(r, fma(-x, r, 1.0), r)


def rcp_from_h(g, h):
    """1 / g from the half reciprocal root the square root left behind + one Newton step against g: within 3.1 u"""
    r = h + h
    return fma(r, fma(-g, r, 1.0), r)


def hartley(px, py, seeds):
    """sample_norm_nz of prescreen.hpp in its order of operations.  Returns (a, b, s, mx, my, qmin, sc)."""
    mx = my = 0.0
    for i in range(8):
        mx += px[i]
        my += py[i]
    mx *= 0.125
    my *= 0.125
    dx, dy = px - mx, py - my
    q = dx * dx + dy * dy
    if not (q.min() >= Q_MIN) or not np.isfinite(q).all():   # (the device computes on and discards: inf / NaN sums fail its test)
        return dx, dy, np.nan, mx, my, float(q.min()), np.nan
    sc = 0.0
    for i in range(8):
        sc += sqrt_relaxed_h(float(q[i]), seeds)[0]
    sc *= 0.125
    s = float(np.sqrt(2.0)) * rcp_relaxed(sc, seeds)
    return dx * s, dy * s, s, mx, my, float(q.min()), sc


def householder_null(A, seeds):
    """pm.householder_null with the device's relaxed column norm, reflector scale and pivot reciprocal.
    Returns n (9,), R (8, 8), rd (8,) = the reciprocal pivots."""
    C = A.T.copy()
    vs, betas, rd = [], [], np.zeros(8)
    for k in range(8):
        x = C[k:, k]
        ss = 0.0
        for xi in x:
            ss = fma(float(xi), float(xi), ss)
        nrm, hn = sqrt_relaxed_h(ss, seeds)
        alpha = -nrm if x[0] >= 0 else nrm
        v = x.copy()
        v[0] = x[0] - alpha
        vv = nrm * (nrm + abs(x[0]))
        iv = rcp_from_h(nrm, hn)
        rd[k] = -iv if x[0] >= 0 else iv
        beta = rcp_relaxed(vv, seeds)
        for j in range(k + 1, 8):
            t = beta * (v * C[k:, j]).sum()
            C[k:, j] -= t * v
        C[k, k] = alpha
        C[k + 1:, k] = 0.0
        vs.append(v)
        betas.append(beta)
    n = np.zeros(9)
    n[8] = 1.0
    for k in range(7, -1, -1):
        v = vs[k]
        t = betas[k] * (v * n[k:]).sum()
        n[k:] -= t * v
    return n, C[:8, :8], rd


def tri_inverse_fro(R, rd):
    """||R^-1||_F by back substitution with multiplications by the reciprocal pivots rd (the device's form)"""
    Y = np.zeros_like(R)
    for j in range(8):
        Y[j, j] = rd[j]
        for i in range(j - 1, -1, -1):
            Y[i, j] = -((R[i, i + 1:j + 1] * Y[i + 1:j + 1, j]).sum() * rd[i])
    return float(np.sqrt((Y * Y).sum()))


def rank2(f, seeds, v=None):
    """pm.rank2 with the relaxed norm of w = G v and its reciprocal from the root's by-product (prescreen_rank2)"""
    G = f.reshape(3, 3)
    if v is None:
        v = np.linalg.eigh(G.T @ G)[1][:, 0]
    v = v / np.sqrt((v * v).sum())
    w = G @ v
    X = G - np.outer(w, v)
    sg2 = float((w * w).sum())
    sgc, hs = sqrt_relaxed_h(max(sg2, 2.0 ** -380), seeds)
    sig = 0.0 if sg2 < 2.0 ** -380 else sgc
    if sig >= 2.0 ** -190:
        u = w * rcp_from_h(sgc, hs)
        r2 = G.T @ u - sig * v
        eps2 = float(np.sqrt((r2 * r2).sum())) * (1 + 1e-14)
    else:
        eps2 = np.inf
    if eps2 < sig:
        e, sig_e, extra = eps2 + TRIP_E, sig, eps2 + TRIP_E
    else:
        e, sig_e, extra = sig + TRIP_E, 0.0, TRIP_E
    _, _, _, _, s2lb = pm.rank2(f, v)          # the second-singular-value bound is unchanged (same X)
    return X, e, sig_e, extra, s2lb


def prescreen(x1, y1, x2, y2, bbox, seeds=None, v3=None):
    """pm.prescreen with the relaxed sequences and the constants that pay for them.  A sample outside the relaxed
    normalisation's range test takes the old model unchanged, like the device's wave-uniform fall-back."""
    seeds = seeds or Seeds()
    a1, b1, s1, m1x, m1y, qm1, sc1 = hartley(np.asarray(x1, float), np.asarray(y1, float), seeds)
    a2, b2, s2, m2x, m2y, qm2, sc2 = hartley(np.asarray(x2, float), np.asarray(y2, float), seeds)
    if not (min(qm1, qm2) >= Q_MIN) or not (sc1 + sc2 < SC_MAX):
        out = pm.prescreen(x1, y1, x2, y2, bbox, v3)
        out["fallback"] = True
        return out
    out = dict(ok=True, screenable=False, F=None, band=np.inf, fallback=False, s=(s1, s2))
    A = pm.design(a1, b1, a2, b2)
    S = float((A * A).sum()) * (1 + 1e-12)
    n, R, rd = householder_null(A, seeds)
    rho = RHO_C * np.sqrt(S)
    out.update(A=A, n=n, rho=rho)
    yf = tri_inverse_fro(R, rd)
    if not np.isfinite(yf):
        return out
    z = 16.0 * U * np.sqrt(S) * yf
    if not (z < 0.5):
        return out
    sig8 = (1.0 - z) / yf * (1 - 1e-13) - 4e-14 * np.sqrt(S)
    if not (sig8 > 0):
        return out
    eta_j = 1.01 * pm.TAU_C * S / (sig8 * sig8) + pm.ETA_Q
    eta_a = 1.5 * rho / sig8 + 1e-13
    Fn, e3, sig_e, extra, s2lb = rank2(n, seeds, v3)
    eta = eta_j + eta_a + e3 + pm.SVD3_E
    delta = s2lb - extra - sig_e - eta
    out.update(sig8_lb=sig8, eta=eta, delta=delta, sig_e=sig_e, s2lb=s2lb)
    if not (delta > 0 and eta < 1e-3):
        return out
    dfn = (2.0 + 2.0 * (sig_e + 3 * eta) / delta) * eta + extra + pm.SVD3_E
    x1lo, x1hi, y1lo, y1hi, x2lo, x2hi, y2lo, y2hi = bbox
    d1x = max(abs(m1x - x1lo), abs(m1x - x1hi))
    d1y = max(abs(m1y - y1lo), abs(m1y - y1hi))
    d2x = max(abs(m2x - x2lo), abs(m2x - x2hi))
    d2y = max(abs(m2y - y2lo), abs(m2y - y2hi))
    N1 = np.sqrt(1 + s1 * s1 * (d1x * d1x + d1y * d1y))
    N2 = np.sqrt(1 + s2 * s2 * (d2x * d2x + d2y * d2y))
    e1x = max(abs(x1lo), abs(x1hi)) + abs(m1x)
    e1y = max(abs(y1lo), abs(y1hi)) + abs(m1y)
    e2x = max(abs(x2lo), abs(x2hi)) + abs(m2x)
    e2y = max(abs(y2lo), abs(y2hi)) + abs(m2y)
    N1p = np.sqrt(1 + s1 * s1 * (e1x * e1x + e1y * e1y))
    N2p = np.sqrt(1 + s2 * s2 * (e2x * e2x + e2y * e2y))
    band = (dfn * N1 * N2 * (1 + 1e-9) + 64 * U * N1p * N2p) * (1 + 1e-9)
    F = pm.denormalise(Fn, s1, m1x, m1y, s2, m2x, m2y)
    out.update(F=F, band=float(band), dfn=dfn, Fn=Fn, screenable=bool(np.isfinite(band)))
    return out
