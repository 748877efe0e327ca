"""Shared fixtures of the reference's tests, restated as data generators (test/unit-test-helper.cpp:42-79)."""
import numpy as np

import oracle_lib as o

CUBE = np.array([[-1, -1, -1], [-1, -1, 1], [-1, 1, -1], [-1, 1, 1], [1, -1, -1], [1, -1, 1], [1, 1, -1], [1, 1, 1.0]])
L_SHAPE = np.array([[1, 0, 0], [0, 0, 0], [0, 2, 0], [1, 0, 3], [0, 0, 3], [0, 2, 3], [0.5, 0, 1.5], [0, 1, 1.5]])


def rig_points(kind, rpy, translation, scale):
    """get_rig_points(type, SO3(roll, pitch, yaw), t, scale): p = R * (scale * p) + t."""
    P = CUBE if kind == "cube" else L_SHAPE
    R = o.so3_from_rpy(*rpy)
    return (R @ (scale * P).T).T + np.asarray(translation, dtype=float)


def two_camera_rig(kind, rpy=(0.0, 0.0, 0.0), translation=(0.6, 0.0, 3.0), scale=1.0, se3_2to1=(1, 0, 0, 0, 0, 0)):
    """The geometry of test/test-sfm.cpp:17-42: K = I, camera 1 at the origin, camera 2 = exp(se3_2to1)."""
    K = np.eye(3)
    R21, t21 = o.se3_exp(np.asarray(se3_2to1, dtype=float))  # pose of camera 2 in camera 1
    R12, t12 = o.se3_inverse(R21, t21)                        # world (= camera 1) -> camera 2
    X = rig_points(kind, rpy, translation, scale)
    uv1 = o.project_points(K, np.eye(3), np.zeros(3), X)
    uv2 = o.project_points(K, R12, t12, X)
    return dict(K=K, X=X, uv1=uv1, uv2=uv2, pose2in1=(R21, t21), T1to2=(R12, t12))


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def rel_err(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    d = np.abs(a - b).max() if a.size else 0.0
    s = max(np.abs(b).max() if b.size else 0.0, 1e-300)
    return d / s


def threads(fn, items, n=16):
    """[fn(x) for x in items] on n host threads (the oracle's ctypes calls release the GIL)"""
    import threading

    out, err = [None] * len(items), []

    def work(k0):
        try:
            for k in range(k0, len(items), n):
                out[k] = fn(items[k])
        except Exception as e:   # surface oracle-side failures in the main thread
            err.append(e)

    ths = [threading.Thread(target=work, args=(k,)) for k in range(min(n, len(items)))]
    [t.start() for t in ths]
    [t.join() for t in ths]
    if err:
        raise err[0]
    return out


# ----------------------------------------------------------------------------- camera catalogue
# Every other fixture of the suite uses one camera (synth.K_DEFAULT, or the identity): fx == fy, no skew, the principal
# point at the image centre, and the same K for every pair of a batch.  These families break each of those in turn.
def camera(fx, fy, skew, cx, cy):
    return np.array([[fx, skew, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


CAMERAS = {   # name -> (K, width, height)
    "default": (camera(525.0, 525.0, 0.0, 320.0, 240.0), 640, 480),
    "aniso_skew": (camera(700.0, 420.0, 35.0, 300.0, 260.0), 640, 480),   # fx != fy, skew, principal point off centre
    "offcentre": (camera(525.0, 525.0, 0.0, 10.0, 470.0), 640, 480),     # principal point in a corner: a one-sided box
    "wide": (camera(120.0, 120.0, 0.0, 640.0, 480.0), 1280, 960),        # box about +-5.3 x +-4.0 in ideal coordinates
    "tele": (camera(4000.0, 4000.0, 0.0, 320.0, 240.0), 640, 480),       # box about +-0.08
}
FAMILIES = list(CAMERAS)
# refinement problems have no image size: skewed and anisotropic, and a short lens with the principal point far off centre
K_REFINE = {"aniso_skew": CAMERAS["aniso_skew"][0], "wide_offcentre": camera(120.0, 140.0, 0.0, 20.0, 460.0)}


def family_of(global_index):
    """pair i of a mixed batch uses family i mod 5"""
    return FAMILIES[int(global_index) % len(FAMILIES)]


def make_family_pair(pair_index, family, **kw):
    from mvslam_amd import synth

    K, w, h = CAMERAS[family]
    return synth.make_pair(pair_index, K=K, width=w, height=h, **kw)


def mixed_batch(first, count, n_kp=2000, **kw):
    """synth.make_batch's layout for pairs [first, first + count), pair i drawn with camera family_of(i): a per-pair K
    that changes from one pair to the next; plus each pair's family and ground-truth motion."""
    desc_bytes = kw.get("desc_bytes", 32)
    out = dict(
        desc1=np.empty((count, n_kp, desc_bytes), dtype=np.uint8), kp1=np.empty((count, n_kp, 2), dtype=np.float32),
        desc2=np.empty((count, n_kp, desc_bytes), dtype=np.uint8), kp2=np.empty((count, n_kp, 2), dtype=np.float32),
        n1=np.full(count, n_kp, dtype=np.int32), n2=np.full(count, n_kp, dtype=np.int32),
        K=np.empty((count, 9)), global_index=np.arange(first, first + count, dtype=np.int64),
        family=np.empty(count, dtype=object), R_1to2=np.empty((count, 3, 3)), t_1to2=np.empty((count, 3)))
    for i in range(count):
        fam = family_of(first + i)
        p = make_family_pair(first + i, fam, n_kp=n_kp, **kw)
        out["desc1"][i], out["kp1"][i], out["desc2"][i], out["kp2"][i] = p["desc1"], p["kp1"], p["desc2"], p["kp2"]
        out["K"][i] = p["K"].reshape(9)
        out["family"][i] = fam
        out["R_1to2"][i], out["t_1to2"][i] = p["R_1to2"], p["t_1to2"]
    return out


def take(data, idx):
    """pairs idx of a batch dict, in that order (their global indices travel with them)"""
    return {k: v[np.asarray(idx)] for k, v in data.items()}


# ----------------------------------------------------------------------------- batched pipeline against the oracle
REL_TOL = 1e-4   # north_star tolerance for pose / points
TIGHT = 1e-12    # what the shared arithmetic contract actually delivers


def run_batch(ctx, first, count, n_kp, prm, data=None, **gen):
    """one resident batch: upload, run, download (synth.make_batch(first, count) unless data is given)"""
    from mvslam_amd import capi, synth

    data = synth.make_batch(first, count, n_kp=n_kp, **gen) if data is None else data
    b = capi.Batch(ctx, count, n_kp, 32)
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"],
             data["global_index"])
    b.run(prm)
    b.sync()
    out = b.download()
    b.close()
    return data, out


def check_batch_against_oracle(data, out, prm, n1=None, n2=None, n_threads=1):
    """every pair of a downloaded batch against the oracle's image_pair with its own K and sampler key; returns the
    oracle's records"""
    count = len(out["results"])

    def ref(i):
        a1 = data["n1"][i] if n1 is None else n1[i]
        a2 = data["n2"][i] if n2 is None else n2[i]
        oprm = o.make_params(prm.num_hypotheses, prm.sampler, prm.seed + int(data["global_index"][i]),
                             prm.max_error_sq, prm.min_inliers)
        return o.image_pair(data["desc1"][i][:a1], data["kp1"][i][:a1], data["desc2"][i][:a2], data["kp2"][i][:a2],
                            data["K"][i].reshape(3, 3), oprm, prm.ratio, prm.max_dist)

    refs = threads(ref, list(range(count)), n_threads)
    for i, ref in enumerate(refs):
        r = out["results"][i]
        M = ref["n_matches"]
        assert r["n_matches"] == M
        assert out["matches"][i][:M].tobytes() == ref["matches"].tobytes()           # match list: bit-exact
        assert bool(r["valid"]) == ref["ok"]
        assert r["best_hyp"] == ref["best_hyp"] and r["best_count"] == ref["best_count"]
        assert np.array_equal(out["mask"][i][:M], ref["mask"])                        # inlier set: bit-exact
        if ref["ok"]:
            n = ref["n_points"]
            assert r["n_points"] == n and r["n_inliers"] == ref["n_inliers"]
            assert np.array_equal(out["point_idx"][i][:n], ref["point_idx"])
            assert rel_err(out["points"][i][:n], ref["points"]) <= REL_TOL
            assert rel_err(r["R"], ref["R"]) <= REL_TOL and rel_err(r["t"], ref["t"]) <= REL_TOL
            assert rel_err(out["points"][i][:n], ref["points"]) <= TIGHT
            assert rel_err(r["R"], ref["R"]) <= TIGHT and rel_err(r["t"], ref["t"]) <= TIGHT
    return refs


def check_two_view(got, ref, m):
    assert got["ok"] == ref["ok"]
    assert got["best_hyp"] == ref["best_hyp"] and got["best_count"] == ref["best_count"]
    assert np.array_equal(got["mask"], ref["mask"][:m])                  # inlier indices: bit-exact
    if ref["ok"]:
        assert np.array_equal(got["point_idx"], ref["point_idx"])         # surviving indices: bit-exact
        for k in ("R", "t", "E", "F", "R1to2", "t1to2"):
            assert rel_err(got[k], ref[k]) <= REL_TOL, k
            assert rel_err(got[k], ref[k]) <= TIGHT, k
        assert rel_err(got["points"], ref["points"]) <= REL_TOL
        assert rel_err(got["points"], ref["points"]) <= TIGHT
