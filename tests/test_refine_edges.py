"""Refinement at the inputs the other modules leave out: full covariances, rejected LM steps and the limits.

The GPU tests of test_refine.py, test_ba_window.py, test_intrinsics.py and test_seq_windows.py feed the refinement kernels isotropic
covariances (every off-diagonal information entry is zero), guesses so close that no Levenberg-Marquardt step is ever
rejected, and the default limits.  This module feeds them what is left:
  * a full 2 x 2 covariance per observation (also with its two off-diagonal entries a few per cent apart: device, host helper
    and oracle all average them), full SPD 3 x 3 point priors, six distinct prior variances per frame;
  * committed TRACE CASES whose oracle trace rejects steps: far guesses (20 to 200 times the usual) and mostly weak priors.
    The accept (A) / reject (R) pattern is read from outside: the solve is cut at max_iterations = k for every k, and step k
    was rejected exactly when the cost at k equals the cost at k - 1.  On the device every rejected k must leave every
    output byte-identical to k - 1, the pattern must be the oracle's, and every k is compared with the oracle at that k;
  * the exits: max_iterations (0 included), lambda > lambda_upper, lambda_initial = 1e-12, lambda_factor = 2, loose tolerances.

CPU part.  The scipy model and the block model of test_ba_window.py (extended there by `full=True`: whitening with the
Cholesky factor of each information matrix) are pinned at F = 2 against the oracle on this module's inputs; the oracle's
covariances are pinned against a finite-difference Hessian with anisotropic weights; every trace case is held to its committed
pattern, to its shape, to robustness (the same pattern over eight runs whose guesses are jittered by a relative 1e-15) and to
the absence of near-ties (ARAR runs).

MEASURED: the largest model <-> oracle distances at F = 2 over _f2_inputs() (gentle guesses with full covariances, symmetric
and asymmetric, m = 12 and 200; weak priors from a guess 20 times further out), scipy model and block model together:
  R 1.7e-9   t 1.1e-8   points 1.1e-7   pose_cov 6.6e-8 (relative)   point_cov 9.2e-8 (relative)
The GPU bounds of the comparisons with the models are ten times those figures (BOUND; the project's rule); the cost is held
to 1e-9 relative as in test_ba_window.py.

Bounds of the comparisons with the oracle: test_refine.py's (EXISTING).  The same jittered runs give each trace case's own
sensitivity, the oracle-to-oracle spread of cost, poses, points and covariances over all k; where ten times that spread
exceeds the existing bound, ten times the spread is the case's bound and the spread is recorded with the case.  That happens
once: "sfm12_first" (cost 1.7e-11 relative and t 1.2e-11, so 1.7e-10 and 1.2e-10 instead of 1e-10).  No bound comes from a
device result.
"""
import numpy as np
import pytest
import oracle_lib as o
import test_ba_window as bw
import test_refine as tr

# models <-> oracle at F = 2 with full covariances (test_extended_models_are_pinned_against_the_oracle_with_full_covariances)
MEASURED = dict(R=1.7e-9, t=1.1e-8, points=1.1e-7, pose_cov=6.6e-8, point_cov=9.2e-8)
BOUND = {k: 10.0 * v for k, v in MEASURED.items()}
SPREAD_SFM12_FIRST = dict(cost=1.7e-11, t=1.2e-11)    # measured oracle-to-oracle spread of the case "sfm12_first"

K_PIX = np.array([[525.0, 0, 320], [0, 525, 240], [0, 0, 1]])
WEAK = dict(point_sigma=1.0, pose_sigma=(1.0, 1.0))


# ---------------------------------------------------------------------------------------------------------------------
# generators

def full_cov2(rng, m, sig, asym=0.0):
    """[m, 4] full 2 x 2 covariances R(th) diag(a^2, b^2) R(th)^T, th uniform, a and b uniform in [0.5, 3] sig, all drawn per
    point.  asym: the two off-diagonal entries are pushed apart by up to that relative amount (everybody averages them)."""
    th = rng.uniform(0, np.pi, m)
    a, b = sig * rng.uniform(0.5, 3, m), sig * rng.uniform(0.5, 3, m)
    c, s = np.cos(th), np.sin(th)
    C = np.empty((m, 4))
    C[:, 0] = c * c * a * a + s * s * b * b
    C[:, 3] = s * s * a * a + c * c * b * b
    C[:, 1] = C[:, 2] = c * s * (a * a - b * b)
    if asym:
        e = asym * rng.uniform(0.5, 1.0, m)
        C[:, 1] *= 1.0 + e
        C[:, 2] *= 1.0 - 0.5 * e
    return C


def full_cov3(rng, m, scale=1e-4, asym=0.0):
    """[m, 9] full SPD 3 x 3 covariances, as test_refine.pnp_problem builds them"""
    A = rng.normal(0, 1, (m, 3, 3))
    C = scale * (np.eye(3) + 0.2 * (A @ A.transpose(0, 2, 1)))
    if asym:
        C = C * (1.0 + asym * np.triu(np.ones((3, 3)), 1) - 0.5 * asym * np.tril(np.ones((3, 3)), -1))
    return C.reshape(m, 9)


VAR_ANCHOR = np.array([1.0, 1.7, 0.6, 2.2, 0.8, 1.3]) * 1e-5     # six distinct variances on the anchored frame
VAR_SCALE = np.array([0.7, 1.9, 1.2, 0.5, 2.4, 1.0])             # ... and (times a level) on the scale-fixing frame


def sfm_case(seed, m, far=1.0, asym=0.0, pix=False, same_cov=False):
    pb = tr.two_view_problem(seed, m, K=K_PIX if pix else None, sig=0.5 if pix else None, baseline=0.3 if pix else 1.0,
                             depth=(2.0, 10.0) if pix else (2.0, 4.0), far=far)
    rng = np.random.default_rng(1000 + seed)
    c1 = full_cov2(rng, m, pb["sig"], asym)
    c2 = c1 if same_cov else full_cov2(rng, m, pb["sig"], asym)
    return dict(entry="sfm", args=[pb["p1"], c1, pb["p2"], c2, pb["K"], pb["Rg"], pb["tg"], pb["Xg"]], guess=(5, 6, 7), pb=pb)


def pnp_case(seed, m, far=1.0, asym=0.0):
    pb = tr.pnp_problem(seed, m, far=far)
    rng = np.random.default_rng(2000 + seed)
    icov = full_cov2(rng, m, pb["sig"], asym)
    return dict(entry="pnp", args=[pb["X"], pb["wcov"], pb["uv"], icov, pb["K"], pb["Rg"], pb["tg"]], guess=(0, 5, 6), pb=pb)


def ba_case(seed, m, n_new, far=1.0, asym=0.0, var_level=1e-2):
    """test_refine.track_refine_problem with full covariances per image, full SPD point priors (none on the new points) and
    six distinct prior variances per frame"""
    pb = tr.track_refine_problem(seed, m, n_new, far=far)
    rng = np.random.default_rng(3000 + seed)
    cov = [full_cov2(rng, m, pb["sig"], asym), full_cov2(rng, m, pb["sig"], asym)]
    pcov = full_cov3(rng, m, 1e-4, asym)
    pcov[~pb["has_prior"]] = 0.0
    var = np.stack([VAR_ANCHOR, VAR_SCALE * var_level])
    pb = dict(pb, cov=cov, pcov=pcov, var=var)
    return dict(entry="ba", args=[pb["K"], pb["poses"], var, pb["Xg"], pcov, pb["obs"], cov, pb["valid"]], guess=(1, 3), pb=pb)


def run(who, case, args=None, **kw):
    """the case through its entry point of `who` (the oracle module or a device context) with refine parameters kw"""
    if who is o:
        prm = o.make_refine_params(**kw)
    else:
        from mvslam_amd import capi
        prm = capi.default_refine_params(**kw)
    fn = getattr(who, {"sfm": "sfm_refine", "pnp": "pnp_refine", "ba": "ba_refine", "win": "ba_refine_window"}[case["entry"]])
    return fn(*(case["args"] if args is None else args), params=prm)


OUT_KEYS = ("R", "t", "points", "pose_cov", "point_cov")


def same_bytes(a, b):
    return a["error"] == b["error"] and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in OUT_KEYS if k in a)


def trace(who, case, args=None, **kw):
    """The solve cut at max_iterations = 0, 1, ... up to its own end: the results per k, and the accept / reject pattern
    seen from outside -- step k was rejected exactly when the cost at k equals the cost at k - 1 while iterations == k."""
    n = run(who, case, args, **kw)["iterations"]
    res = [run(who, case, args, **dict(kw, max_iterations=k)) for k in range(n + 1)]
    assert [r["iterations"] for r in res] == list(range(n + 1))
    pat = "".join("R" if res[k]["error"] == res[k - 1]["error"] else "A" for k in range(1, n + 1))
    return res, pat


def jittered(case, j):
    """the case with its guesses moved by a relative 1e-15 (a few ulps), jitter number j"""
    rng = np.random.default_rng(7000 + j)
    args = list(case["args"])
    for i in case["guess"]:
        a = np.asarray(args[i], float)
        args[i] = a * (1.0 + 1e-15 * rng.uniform(-1, 1, a.shape))
    return args


def no_near_tie(pat):
    """at most two consecutive alternations anywhere but the final stop"""
    body = pat[:-1]
    return "ARAR" not in body and "RARA" not in body


def distances(got, want):
    """absolute for cost (relative), poses and points; relative to the largest entry for covariances"""
    d = dict(cost=abs(got["error"] - want["error"]) / max(abs(want["error"]), 1e-300),
             R=np.abs(got["R"] - want["R"]).max(), t=np.abs(got["t"] - want["t"]).max())
    if "points" in want:
        d["points"] = np.abs(got["points"] - want["points"]).max()
        d["point_cov"] = bw._rel(got["point_cov"], want["point_cov"])
    pc_g, pc_w = np.asarray(got["pose_cov"]).reshape(-1, 6, 6), np.asarray(want["pose_cov"]).reshape(-1, 6, 6)
    d["pose_cov"] = max(bw._rel(pc_g[f], pc_w[f]) for f in range(len(pc_w)))
    return d


def win_case(seed, F, m, far=1.0, weak=False, asym=0.0, rot_only_third=False):
    """test_ba_window.window_problem with a full covariance per observation, full SPD point priors where it has priors, six
    distinct variances on the anchored and on the scale-fixing frame; weak: point priors and the scale-fixing prior at
    sigma ~ 1; rot_only_third: frame 2 (which the observations fix) gets a prior on its rotation only"""
    pb = bw.window_problem(seed, F, m, far=far)
    rng = np.random.default_rng(4000 + seed)
    cov = [full_cov2(rng, m, pb["sig"], asym) for _ in range(F)]
    pcov = full_cov3(rng, m, 1.0 if weak else 1e-4, asym)
    pcov[~pb["has_prior"]] = 0.0
    var = pb["var"].copy()
    var[0] = VAR_ANCHOR
    if F > 1:
        var[1] = VAR_SCALE * (1.0 if weak else 1e-2)
    if rot_only_third:
        var[2] = [1e-3, 2e-3, 3e-3, 0.0, 0.0, 0.0]
    return dict(pb, cov=cov, pcov=pcov, var=var)


def win_args(pb):
    return [pb["K"], pb["poses"], pb["var"], pb["Xg"], pb["pcov"], pb["obs"], pb["cov"], pb["valid"]]


# ---------------------------------------------------------------------------------------------------------------------
# the committed trace cases (chosen once, by hand, on the CPU oracle; test_trace_case_meets_its_conditions holds them to it)
#   pattern   the oracle's accept / reject pattern
#   spread    only where ten times the oracle-to-oracle spread under a 1e-15 jitter of the guess exceeds the existing bound
#             of that quantity: the measured spread; the case's bound is then ten times it

TRACES = {
    # (a) rejected steps, then accepted ones, convergence; (b) max_iterations 3 cuts after an accepted, 7 after a rejected step
    "sfm12": dict(make=lambda: sfm_case(7, 12, far=80), kw=WEAK, pattern="AAARRRRRRRRAAAAAAAAAAA", spread={}),
    "sfm12_factor2": dict(make=lambda: sfm_case(7, 12, far=80), kw=dict(WEAK, lambda_factor=2.0),
                          pattern="AAARRRRRRRRRRRRRRRRRRRRAAAAAAAAAAAA", spread={}),
    # (d) a rejected first step (lambda_initial = 1e-12 on a far guess)
    "sfm12_first": dict(make=lambda: sfm_case(28, 12, far=60), kw=dict(WEAK, lambda_initial=1e-12),
                        pattern="RRRRRRRRRRRRRRAAAAAAAAAAAAAAA", spread=dict(SPREAD_SFM12_FIRST)),
    "sfm769": dict(make=lambda: sfm_case(5, 769, far=60), kw=WEAK, pattern="RRRRRRRAAAAAAAAAA", spread={}),
    "sfm1100": dict(make=lambda: sfm_case(4, 1100, far=60), kw=WEAK, pattern="ARRRRRRRAAAAAAAAA", spread={}),
    "pnp7": dict(make=lambda: pnp_case(14, 7, far=200), kw=WEAK, pattern="ARRRRRRRRAAAAAA", spread={}),
    "pnp12": dict(make=lambda: pnp_case(14, 12, far=200), kw=WEAK, pattern="AARRRRRRRRRRAAAAAAA", spread={}),
    # (c) leaves through lam > lambda_upper by itself, past the resident cap of one frame
    "pnp961_upper": dict(make=lambda: pnp_case(15, 961, far=200), kw=WEAK, pattern="AARRRRRRRRRRRR", spread={}),
    "ba12": dict(make=lambda: ba_case(1, 12, 3, far=60, var_level=1.0), kw={}, pattern="AARRRRRAAAAAAAAAAAAA", spread={}),
    "ba769": dict(make=lambda: ba_case(7, 769, 100, far=60, var_level=1.0), kw={}, pattern="RRRRRRAAAAAAAAA", spread={}),
    "ba1100_upper": dict(make=lambda: ba_case(7, 1100, 100, far=40, var_level=1.0), kw={}, pattern="ARRRRRRRRRRR", spread={}),
}
SHAPES = dict(converges=("sfm12", "sfm12_factor2", "sfm12_first", "sfm769", "sfm1100", "pnp7", "pnp12", "ba12", "ba769"),
              upper=("pnp961_upper", "ba1100_upper"), first_rejected=("sfm12_first", "sfm769", "ba769"))

EXISTING = dict(sfm=dict(cost=1e-10, R=1e-10, t=1e-10, points=1e-9, pose_cov=1e-7, point_cov=1e-7),
                pnp=dict(cost=1e-10, R=1e-10, t=1e-10, pose_cov=1e-7),
                ba=dict(cost=1e-10, R=1e-9, t=1e-9, points=1e-8, pose_cov=1e-6, point_cov=1e-6))
N_JITTER = 8


def bounds_of(name):
    """test_refine's bounds for the entry point; ten times the recorded spread where that is larger"""
    t = TRACES[name]
    b = dict(EXISTING[t["make"]()["entry"]])
    for k, v in t["spread"].items():
        b[k] = max(b[k], 10.0 * v)
    return b


_cache = {}


def oracle_trace(name):
    """(case, results per k, pattern) of a committed case, computed once per session"""
    if name not in _cache:
        case = TRACES[name]["make"]()
        _cache[name] = (case,) + trace(o, case, **TRACES[name]["kw"])
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the extended models and checks, pinned reference against reference

def _f2_inputs():
    """the F = 2 inputs the model <-> oracle distance is measured on: full covariances and priors at a gentle guess (what
    the GPU comparisons with the models use), and the weak-prior far-guess kind of the oracle-free window traces"""
    out = [win_case(seed, 2, 12) for seed in range(4)] + [win_case(seed, 2, 12, asym=0.03) for seed in (4, 5)]
    out += [win_case(0, 2, 200), win_case(1, 2, 200, asym=0.03)]
    out += [win_case(seed, 2, 12, far=20, weak=True) for seed in range(3)] + [win_case(0, 2, 200, far=20, weak=True)]
    return out


def test_extended_models_are_pinned_against_the_oracle_with_full_covariances():
    """reference against reference at F = 2: cost 1e-9 relative; the largest scipy <-> oracle and block model <-> oracle
    distances are printed (MEASURED quotes them) and stay inside the bounds derived from them"""
    worst = dict.fromkeys(MEASURED, 0.0)
    for pb in _f2_inputs():
        want = o.ba_refine(*win_args(pb))
        assert want["ok"]
        for got in (bw.model_solve(pb, full=True), bw.model_solve_blocks(pb, full=True)):
            assert abs(got["error"] - want["error"]) <= 1e-9 * want["error"]
            for k, v in bw._distances(got, want).items():
                worst[k] = max(worst[k], v)
    print("models <-> oracle at F = 2, full covariances: %s" % {k: "%.2e" % v for k, v in worst.items()})
    for k in MEASURED:
        assert worst[k] <= BOUND[k], (k, worst[k])
        assert worst[k] >= 0.1 * MEASURED[k], (k, worst[k], "MEASURED is stale")


def test_scalar_path_of_the_models_is_the_special_case():
    """isotropic covariances through the full path give what the scalar path gives (two scipy runs: test_ba_window's bounds)"""
    pb = bw.window_problem(3, 3, 12)
    a, b = bw.model_solve(pb, cov=False), bw.model_solve(pb, cov=False, full=True)
    assert abs(a["error"] - b["error"]) <= 1e-9 * a["error"] and np.abs(a["points"] - b["points"]).max() <= bw.BOUND["points"]
    c, d = bw.model_solve_blocks(pb), bw.model_solve_blocks(pb, full=True)
    assert abs(c["error"] - d["error"]) <= 1e-9 * c["error"] and bw._rel(d["point_cov"], c["point_cov"]) <= bw.BOUND["point_cov"]


@pytest.mark.parametrize("asym", [0.0, 0.03])
def test_oracle_covariances_match_finite_difference_hessian_with_anisotropic_weights(asym):
    pb = tr.two_view_problem(2, 10)
    rng = np.random.default_rng(11)
    tr._check_covariances(pb, full_cov2(rng, 10, pb["sig"], asym), full_cov2(rng, 10, pb["sig"], asym))


def test_asymmetric_covariance_is_its_symmetric_part():
    """oracle: off-diagonal entries a few per cent apart give bit for bit what their average gives"""
    case = sfm_case(3, 12, asym=0.03)
    sym = list(case["args"])
    for i in (1, 3):
        c = sym[i].copy()
        assert np.abs(c[:, 1] - c[:, 2]).max() > 0.01 * np.abs(c[:, 1]).max()
        c[:, 1] = c[:, 2] = 0.5 * (c[:, 1] + c[:, 2])
        sym[i] = c
    assert same_bytes(run(o, case), run(o, case, sym))


def _measure(name):
    case, res, pat = oracle_trace(name)
    spread = {}
    for j in range(N_JITTER):
        rj, pj = trace(o, case, jittered(case, j), **TRACES[name]["kw"])
        assert pj == pat and len(rj) == len(res), (name, j, pj)
        for a, b in zip(rj, res):
            assert a["ok"] == b["ok"]
            for k, v in distances(a, b).items():
                spread[k] = max(spread.get(k, 0.0), v)
    return spread


@pytest.mark.parametrize("name", list(TRACES))
def test_trace_case_meets_its_conditions(name):
    """the committed pattern and shape; the same pattern and iteration count under eight 1e-15 jitters of the guess; no
    near-tie; the oracle-to-oracle spread that fixes the case's bounds"""
    case, res, pat = oracle_trace(name)
    t = TRACES[name]
    assert pat == t["pattern"] and no_near_tie(pat)
    assert all(r["ok"] and np.isfinite(r["error"]) for r in res)
    full = run(o, case, **t["kw"])
    assert full["ok"] and full["iterations"] == len(pat) < 100 and same_bytes(full, res[-1])
    if name in SHAPES["converges"]:
        assert "RA" in pat and pat.endswith("AAA")
    if name in SHAPES["upper"]:     # the last rejection raised lambda past lambda_upper (1e5)
        n_a, n_r = pat.count("A"), pat.count("R")
        assert pat.endswith("R") and 1e-5 * 10.0 ** (n_r - n_a) > 1e5 >= 1e-5 * 10.0 ** (n_r - n_a - 1)
    if name in SHAPES["first_rejected"]:
        assert pat[0] == "R"
    spread = _measure(name)
    print("%s: spread %s" % (name, {k: "%.1e" % v for k, v in spread.items()}))
    for k, v in spread.items():
        existing = EXISTING[case["entry"]][k]
        if k in t["spread"]:
            assert 10.0 * t["spread"][k] > existing and v <= 2.0 * t["spread"][k], (k, v)
        else:
            assert 10.0 * v <= existing, (k, v, "needs a recorded spread")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: refine_kernel (one and two frames) against the oracle

def _hold(got, want, bound, what):
    assert got["ok"] == want["ok"] and got["iterations"] == want["iterations"], (what, got["ok"], got["iterations"], want["iterations"])
    assert np.isfinite(got["error"])
    d = distances(got, want) if want["ok"] else {k: v for k, v in distances(got, want).items() if not k.endswith("_cov")}
    print("%s: %s" % (what, {k: "%.1e" % v for k, v in d.items()}))
    for k, v in d.items():
        assert v <= bound[k], (what, k, v, bound[k])


@pytest.mark.gpu
@pytest.mark.parametrize("m,asym", [(1, 0.0), (12, 0.0), (12, 0.03), (767, 0.0), (768, 0.0), (769, 0.03), (1100, 0.0)])
def test_gpu_sfm_refine_full_covariances(ctx, m, asym):
    """a different full covariance per point and per image (swapped images or a wrong off-diagonal sign change the answer)"""
    case = sfm_case(40 + m, m, asym=asym, pix=m > 12)
    want = run(o, case)
    assert want["ok"]
    _hold(run(ctx, case), want, EXISTING["sfm"], "sfm m = %d" % m)
    if m == 12:   # the inputs do tell the two images apart: the oracle with the covariances swapped is elsewhere
        a = case["args"]
        swapped = run(o, case, [a[0], a[3], a[2], a[1]] + a[4:])
        assert np.abs(swapped["t"] - want["t"]).max() > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("m,asym", [(7, 0.03), (959, 0.0), (960, 0.0), (961, 0.03)])
def test_gpu_pnp_refine_full_covariances(ctx, m, asym):
    case = pnp_case(50 + m, m, asym=asym)
    want = run(o, case)
    assert want["ok"]
    _hold(run(ctx, case), want, EXISTING["pnp"], "pnp m = %d" % m)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n_new,asym", [(24, 5, 0.03), (769, 100, 0.0)])
def test_gpu_ba_refine_full_covariances_and_priors(ctx, m, n_new, asym):
    """full 2 x 2 and 3 x 3 covariances, six distinct prior variances per frame, missing observations, prior-less points"""
    case = ba_case(60 + m, m, n_new, asym=asym)
    want = run(o, case)
    assert want["ok"]
    _hold(run(ctx, case), want, EXISTING["ba"], "ba m = %d" % m)


@pytest.mark.gpu
def test_gpu_ba_refine_point_held_by_one_strongly_anisotropic_observation(ctx):
    """a point that arrives without a prior loses one of its two observations, and the one left has a 20 : 1 covariance
    ellipse: with nothing else the point would be free along its ray (no model), so it gets a weak prior (sigma 0.5) and is
    then held by the cross terms of that single observation"""
    case = ba_case(61, 24, 5)
    K, poses, var, Xg, pcov, obs, cov, valid = case["args"]
    i = int(np.nonzero(~case["pb"]["has_prior"])[0][0])
    valid = [valid[0].copy(), valid[1].copy()]
    valid[0][i], valid[1][i] = 0, 1
    cov = [cov[0], cov[1].copy()]
    c, s, a, b = np.cos(0.6), np.sin(0.6), 5.0, 0.25
    cov[1][i] = [c * c * a * a + s * s * b * b, c * s * (a * a - b * b), c * s * (a * a - b * b), s * s * a * a + c * c * b * b]
    pcov = pcov.copy()
    pcov[i] = (np.eye(3) * 0.25).reshape(9)
    args = [K, poses, var, Xg, pcov, obs, cov, valid]
    want = run(o, case, args)
    assert want["ok"]
    _hold(run(ctx, case, args), want, EXISTING["ba"], "one anisotropic observation")


def _device_trace(ctx, name, case=None, sel=None):
    """the committed case on the device, cut at every k: pattern, rejected steps byte-identical, every k against the oracle"""
    ocase, ores, opat = oracle_trace(name)
    case = case or ocase
    kw, bound = TRACES[name]["kw"], bounds_of(name)
    res = [run(ctx, case, **dict(kw, max_iterations=k)) for k in range(len(ores))]
    pat = "".join("R" if res[k]["error"] == res[k - 1]["error"] else "A" for k in range(1, len(res)))
    assert pat == opat, (name, pat, opat)
    for k, (got, want) in enumerate(zip(res, ores)):
        if k and pat[k - 1] == "R":
            assert same_bytes(got, res[k - 1]), (name, k)
        _hold(sel(got) if sel else got, want, bound, "%s k = %d" % (name, k))
    full = run(ctx, case, **kw)
    assert full["ok"] and full["iterations"] == len(opat) and same_bytes(full, res[-1])
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRACES))
def test_gpu_trace_follows_the_oracle_step_by_step(ctx, name):
    """max_iterations = 0 (the guess with its cost and covariances), 1, 2, ... to the end of the trace: ok, iterations, cost,
    poses, points and covariances against the oracle at the same k; the same accept / reject pattern; every rejected step
    leaves every output byte-identical (the points past the resident cap included)"""
    _device_trace(ctx, name)


@pytest.mark.gpu
def test_gpu_limits(ctx):
    """stops at lambda_upper and at max_iterations, loose tolerances (lambda_factor = 2 is the trace case sfm12_factor2): ok = 1, a finite cost, the oracle's iteration count and the
    oracle's state and covariances at the exit"""
    case, ores, pat = oracle_trace("sfm12")
    # three accepted steps leave lambda at 1e-8; five rejected ones raise it to 1e-3, past 3e-4
    kw = dict(WEAK, lambda_upper=3e-4)
    want = run(o, case, **kw)
    assert want["ok"] and want["iterations"] == 8 and same_bytes(want, ores[8])
    _hold(run(ctx, case, **kw), want, bounds_of("sfm12"), "lambda_upper = 3e-4")
    for k in (3, 7):    # just after an accepted, just after a rejected step
        got = run(ctx, case, **dict(WEAK, max_iterations=k))
        assert got["ok"] and got["iterations"] == k and np.isfinite(got["error"])
    for c in (sfm_case(52, 12), sfm_case(41, 769, pix=True), pnp_case(51, 961)):
        tight, loose = run(o, c), run(o, c, rel_tol=1e-5, abs_tol=1e-5)
        assert loose["ok"] and loose["iterations"] < tight["iterations"]
        got = run(ctx, c, rel_tol=1e-5, abs_tol=1e-5)
        # stopped early, the state is an iterate, not the minimum: as far from the oracle's as any iterate of a gentle solve
        _hold(got, loose, EXISTING[c["entry"]], "loose tolerances")


@pytest.mark.gpu
def test_gpu_batch_refine_passes_its_params_on(ctx):
    """Batch.refine with weak priors and max_iterations = 3 against the oracle with the same parameters"""
    from mvslam_amd import capi, synth

    n_pairs, n_kp = 3, 600
    data = synth.make_batch(0, n_pairs, n_kp=n_kp)
    rng = np.random.default_rng(6)
    oct1 = rng.integers(0, 4, size=(n_pairs, n_kp)).astype(np.uint8)
    oct2 = rng.integers(0, 4, size=(n_pairs, n_kp)).astype(np.uint8)
    b = capi.Batch(ctx, n_pairs, n_kp)
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"], data["global_index"])
    b.upload_octaves(0, oct1, oct2)
    b.run(capi.default_params(num_hypotheses=2048, sampler=capi.SAMPLER_PHILOX, seed=11, max_error_sq=1e-2))
    b.refine(params=capi.default_refine_params(max_iterations=3, **WEAK), sigma_px=0.5)
    b.sync()
    out = b.download()
    ref = b.download_refined(points=True, point_cov=True)
    b.close()
    n_checked = 0
    for p in range(n_pairs):
        r = out["results"][p]
        if not r["valid"]:
            continue
        n = int(r["n_points"])
        mt = out["matches"][p][out["point_idx"][p][:n]]
        p1, p2 = data["kp1"][p][mt["trainIdx"]].astype(np.float64), data["kp2"][p][mt["queryIdx"]].astype(np.float64)
        s1 = 0.5 * 2.0 ** oct1[p][mt["trainIdx"]].astype(np.float64)
        s2 = 0.5 * 2.0 ** oct2[p][mt["queryIdx"]].astype(np.float64)
        cov1, cov2 = (s1 * s1)[:, None] * np.eye(2).reshape(1, 4), (s2 * s2)[:, None] * np.eye(2).reshape(1, 4)
        args = (p1, cov1, p2, cov2, synth.K_DEFAULT, r["R"], r["t"], out["points"][p][:n])
        want = o.sfm_refine(*args, params=o.make_refine_params(max_iterations=3, **WEAK))
        got = ref["refined"][p]
        assert got["ok"] == 1 and want["ok"] and got["iterations"] == want["iterations"] == 3
        assert abs(got["error"] - want["error"]) <= 1e-9 * want["error"]
        assert np.abs(got["R"] - want["R"]).max() < 1e-9 and np.abs(got["t"] - want["t"]).max() < 1e-9
        assert np.abs(ref["points"][p][:n] - want["points"]).max() < 1e-8
        tr._close(got["pose_cov"], want["pose_cov"], 1e-6, "pose_cov")
        tr._close(ref["point_cov"][p][:n], want["point_cov"], 1e-6, "point_cov")
        # and the parameters matter: the default solve of the same pair ends elsewhere
        assert abs(o.sfm_refine(*args)["error"] - want["error"]) > 1e-6 * want["error"]
        n_checked += 1
    assert n_checked >= 2


# ---------------------------------------------------------------------------------------------------------------------
# GPU: refine_window_kernel (three to eight frames)

def _hold_model(got, want):
    assert got["ok"] and got["status"] == 0
    d = bw._distances(got, want)
    print("cost %.2e %s iterations %d" % (abs(got["error"] - want["error"]) / want["error"], {k: "%.2e" % v for k, v in d.items()},
                                          got["iterations"]))
    assert abs(got["error"] - want["error"]) <= 1e-9 * want["error"]
    for k, v in d.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


@pytest.mark.gpu
@pytest.mark.parametrize("F,m", [(3, 12), (3, 200), (8, 12), (8, 200), (4, 4096)])
def test_gpu_window_full_covariances_match_the_models(ctx, F, m):
    """full observation covariances (asymmetric input at F = 8), full point priors, distinct prior variances, at F = 3 a
    rotation-only prior on the third frame: against the scipy model, at m = 4096 against the block model; bounds BOUND"""
    pb = win_case(10 * F + 2, F, m, asym=0.03 if F == 8 else 0.0, rot_only_third=F == 3)
    want = bw.model_solve(pb, full=True) if m <= 200 else bw.model_solve_blocks(pb, full=True)
    _hold_model(ctx.ba_refine_windows([bw.as_window(pb)])[0], want)


@pytest.mark.gpu
def test_gpu_window_host_information_helpers(ctx):
    """one window whose obs_cov is absent for one frame, full for another and asymmetric for a third"""
    pb = win_case(33, 3, 40)
    rng = np.random.default_rng(5)
    pb["cov"] = [None, pb["cov"][1], full_cov2(rng, 40, pb["sig"], asym=0.05)]
    # frame 0 is weighted with the identity: its noise must be of that size for the problem to stay the same kind
    pb["obs"] = list(pb["obs"])
    pb["obs"][0] = tr.proj(pb["K"], pb["R_true"][0], pb["t_true"][0], pb["X"]) + rng.normal(0, 1.0, (40, 2))
    _hold_model(ctx.ba_refine_windows([bw.as_window(pb)])[0], bw.model_solve(pb, full=True))


def _first_two(r):
    return dict(r, R=r["R"][:2], t=r["t"][:2], pose_cov=r["pose_cov"][:2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ba12", "ba769"])
def test_gpu_window_decoupled_third_frame_follows_the_oracle_trace(ctx, name):
    """the window kernel at F = 3 with a third frame that sees nothing and keeps its prior: on the two coupled frames and
    the points it takes the oracle's decisions, step by step, on a trace case with full covariances"""
    case = oracle_trace(name)[0]
    w, p2, var2 = bw._with_decoupled_frame(case["pb"], 9)
    wcase = dict(entry="win", args=[w[k] for k in ("K", "frame_pose", "frame_prior_var", "points", "point_prior_cov", "obs",
                                                   "obs_cov", "obs_valid")])
    res = _device_trace(ctx, name, wcase, _first_two)
    assert np.abs(res[-1]["R"][2].reshape(9) - p2[:9]).max() < 1e-12 and np.abs(res[-1]["t"][2] - p2[9:]).max() < 1e-12
    tr._close(res[-1]["pose_cov"][2], np.diag(var2), 1e-9, "pose_cov[2]")


FAR_WINDOWS = {3: dict(seed=32, m=40, far=20), 8: dict(seed=82, m=40, far=20)}


def test_far_windows_have_one_minimum_two_methods_find():
    """the oracle-free window traces start far out with weak priors: scipy's trust region and the block model's damped
    Gauss-Newton, two different methods, end at the same minimum, so the device has no other to find"""
    for F, c in FAR_WINDOWS.items():
        pb = win_case(c["seed"], F, c["m"], far=c["far"], weak=True)
        a, b = bw.model_solve(pb, full=True), bw.model_solve_blocks(pb, full=True)
        assert a["error"] < 0.1 * a["error_guess"] and abs(a["error"] - b["error"]) <= 1e-9 * a["error"]
        for k, v in bw._distances(b, a).items():
            assert v <= BOUND[k], (F, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [3, 8])
def test_gpu_window_trace_without_an_oracle(ctx, F):
    """far guess, weak priors: the cost never rises from k to k + 1, a k that leaves the cost unchanged leaves every output
    byte-identical, and the converged result is the scipy model's minimum (BOUND)"""
    c = FAR_WINDOWS[F]
    pb = win_case(c["seed"], F, c["m"], far=c["far"], weak=True)
    case = dict(entry="win", args=win_args(pb))
    full = run(ctx, case)
    assert full["ok"] and full["iterations"] < 100
    res = [run(ctx, case, max_iterations=k) for k in range(full["iterations"] + 1)]
    pat = ""
    for k in range(1, len(res)):
        assert res[k]["ok"] and res[k]["iterations"] == k and res[k]["error"] <= res[k - 1]["error"], k
        same = res[k]["error"] == res[k - 1]["error"]
        assert not same or same_bytes(res[k], res[k - 1]), k
        pat += "R" if same else "A"
    print("F = %d: %s" % (F, pat))
    assert same_bytes(full, res[-1])
    _hold_model(dict(full, status=0), bw.model_solve(pb, full=True))


@pytest.mark.gpu
def test_gpu_window_batch_of_gentle_and_far_windows_equals_single_calls(ctx):
    """a window that rejects steps does not disturb its neighbours: the batch equals the single calls byte for byte"""
    pbs = [win_case(71, 3, 12), win_case(32, 3, 40, far=20, weak=True), win_case(72, 5, 300), oracle_trace("ba769")[0]["pb"],
           win_case(82, 8, 40, far=20, weak=True), win_case(73, 8, 33), oracle_trace("ba12")[0]["pb"]]
    batch = ctx.ba_refine_windows([bw.as_window(pb) for pb in pbs])
    its = []
    for pb, r in zip(pbs, batch):
        s = ctx.ba_refine_window(*win_args(pb))
        assert s["ok"] and r["ok"] and bw._bytes(s) == bw._bytes(r)
        its.append(r["iterations"])
    assert its[3] == len(TRACES["ba769"]["pattern"]) and its[6] == len(TRACES["ba12"]["pattern"])


@pytest.mark.gpu
def test_gpu_window_limits(ctx):
    """max_iterations and lambda_upper exits of the window kernel: ok = 1, status MVS_OK, a finite cost"""
    from mvslam_amd import capi

    c = FAR_WINDOWS[3]
    w = bw.as_window(win_case(c["seed"], 3, c["m"], far=c["far"], weak=True))
    full = ctx.ba_refine_windows([w])[0]
    for k in (0, 2):
        r = ctx.ba_refine_windows([w], params=capi.default_refine_params(max_iterations=k))[0]
        assert r["ok"] and r["status"] == capi.MVS_OK and np.isfinite(r["error"]), k
        assert r["iterations"] == k < full["iterations"] and r["error"] >= full["error"]
    # the decoupled-frame trace case leaves through lambda_upper where the oracle does
    case = oracle_trace("ba12")[0]
    want = run(o, case, lambda_upper=3e-4)
    wd = bw._with_decoupled_frame(case["pb"], 9)[0]
    got = ctx.ba_refine_windows([wd], params=capi.default_refine_params(lambda_upper=3e-4))[0]
    assert want["ok"] and want["iterations"] == 6 and got["status"] == capi.MVS_OK   # two accepted, four rejected: 1e-3 > 3e-4
    _hold(_first_two(got), want, bounds_of("ba12"), "window lambda_upper")
