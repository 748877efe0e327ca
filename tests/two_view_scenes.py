"""Two-view scenes off the sideways one (a plain helper module, like helpers.py).

Every other two-view fixture of the suite moves the camera sideways by a few per cent of the depth, turns it by less than 0.1 rad
and looks at a box of depths 2 .. 10: the epipole is far outside the image, the 8-point matrix has rank 8, all four (R, t)
candidates but one put every point behind a camera, nothing is dropped by the triangulation.  motion_scene() restates
test_gpu_parity._scene -- X uniform in [-2, 2] x [-1.5, 1.5] x [3, 9], a random axis scaled to 0.08 rad, t = (0.3, 0.02, 0.01),
outliers redrawn in [-0.5, 0.5]^2 -- and each family changes ONE thing of it.  One default_rng(seed), drawn from in one fixed
order whatever the family (a family that replaces a drawn value still draws it), so two families of one seed share everything
they do not change."""
import numpy as np

import oracle_lib as o
from mvslam_amd import synth

T_SIDE = np.array([0.3, 0.02, 0.01])

FAMILIES = ("side", "forward", "backward", "large_rotation", "roll90", "planar", "near_planar", "pure_rotation",
            "tiny_baseline", "far", "mixed_far")
# degenerate for eight points (rank of the 8-point matrix <= 7, or a baseline below the noise): no accuracy claim
DEGENERATE = ("planar", "near_planar", "pure_rotation", "tiny_baseline")
WELL_POSED = tuple(f for f in FAMILIES if f not in DEGENERATE)


def motion_scene(seed, m, family, noise=3e-4, outliers=0.3):
    """dict(uv1, uv2: pixels at synth.K_DEFAULT [m][2]; p1, p2: the ideal coordinates; R, t, X: the true motion
    (x2 = R x1 + t) and the points in camera 1; bad: the outlier flags; K)"""
    assert family in FAMILIES, family
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= 0.08 / np.linalg.norm(w)
    t = T_SIDE.copy()
    X = np.stack([rng.uniform(-2, 2, m), rng.uniform(-1.5, 1.5, m), rng.uniform(3, 9, m)], axis=1)
    dz = rng.normal(scale=0.02, size=m)          # near_planar's relief
    n1 = rng.normal(size=(m, 2))
    n2 = rng.normal(size=(m, 2))
    bad = rng.random(m) < outliers
    wrong = rng.uniform(-0.5, 0.5, size=(m, 2))
    if family == "forward":
        t = np.array([0.01, 0.02, 0.3])          # the epipole inside the image
    elif family == "backward":
        t = np.array([0.01, 0.02, -0.3])
    elif family == "large_rotation":
        w = np.array([0.05, 0.6, 0.1])
        t = np.array([-2.5, 0.0, 1.0])
    elif family == "roll90":
        w = np.array([0.0, 0.0, np.pi / 2])
    elif family in ("planar", "near_planar"):
        X[:, 2] = 5.0 + 0.2 * X[:, 0] - 0.1 * X[:, 1]
        if family == "near_planar":
            X[:, 2] += dz
    elif family == "pure_rotation":
        t = np.zeros(3)
    elif family == "tiny_baseline":
        t = t * 1e-3
    elif family == "far":
        X = X * 100.0                            # Z uniform in [300, 900]: parallax of the order of the noise
    elif family == "mixed_far":
        X[m // 2:] *= 1000.0                     # depths over three orders of magnitude
    R = o.rodrigues(w)
    p1 = X[:, :2] / X[:, 2:3]
    X2 = (R @ X.T).T + t
    assert (X2[:, 2] > 0).all()                  # every true point in front of both cameras
    p2 = X2[:, :2] / X2[:, 2:3]
    p1 = p1 + noise * n1
    p2 = p2 + noise * n2
    p2[bad] = wrong[bad]
    K = synth.K_DEFAULT
    c = np.array([K[0, 2], K[1, 2]])
    f = np.array([K[0, 0], K[1, 1]])
    return dict(uv1=p1 * f + c, uv2=p2 * f + c, p1=p1, p2=p2, R=R, t=t, X=X, bad=bad, K=K)


def essential_of(sc):
    """the analytic E = [t]x R of a scene"""
    t = sc["t"]
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]]) @ sc["R"]


def candidates(E):
    """the four (R, t) of the oracle's decompose_essential in recover_pose_and_points' order (sfm-solve.cpp:250-280)"""
    Ra, Rb, t = o.decompose_essential(E)
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


# The branch-condition cases shared by the host and the GPU tests: 300 matches, 512 hypotheses, 30 % outliers, 3e-4 noise.
# SCENE_SEED is the first seed at which every condition of test_two_view_scenes_host.py holds at once (how many points the
# winner keeps on a degenerate family depends on which of the near-equivalent models the sampler meets: seed 1 keeps 182 of
# planar's 184 inliers at 2e-3, seed 2 splits them 97 : 83).
M, H, SAMPLER_SEED = 300, 512, 11
SCENE_SEED = 2
THRESHOLDS = (1e-2, 2e-3)
# the tie regime: noise-free inliers under the reference threshold (max_error_sq = 0 selects 5e-2 / K00 / K11): hundreds of
# hypotheses tie on the count and the residual sum decides.  The oracle's `ok` per family, measured by
# test_two_view_scenes_host.py::test_tie_regime_flags_are_the_recorded_ones and asserted there.
TIE_OK = {"side": True, "forward": True, "backward": True, "large_rotation": True, "roll90": True, "planar": True,
          "near_planar": True, "pure_rotation": True, "tiny_baseline": True, "far": True, "mixed_far": True}


def tie_scene(family):
    return scene(SCENE_SEED, M, family, 0.0, 0.3)


_CACHE = {}


def scene(seed, m, family, noise=3e-4, outliers=0.3):
    """motion_scene, computed once per argument tuple and shared (callers leave it unchanged)"""
    key = (seed, m, family, noise, outliers)
    if key not in _CACHE:
        _CACHE[key] = motion_scene(*key)
    return _CACHE[key]
