// test_compat_ba_sparse.cpp -- ba_frame_pose_and_point (vision/ba.hpp:25-36) on MORE than eight frames through the drop-in shim:
// the maps are packed into an mvs_ba_sparse by the shim (hip::ba_sparse_) and solved by mvs_ba_refine_sparse (DESIGN.md section
// 4.7.4).  The problem comes from a text file tests/test_compat_ba_sparse.py writes from the fixture
// tests/golden/ba_sparse_12.npz; the estimates are printed, one record per line, and compared there with the values the Python
// model wrote to the fixture.  Frame and point ids are arbitrary and the observations are inserted frame by frame in the file's
// order, so the shim's sorting and its by-point lists are what carries them to the right place.
//   input:  F m n / K (9) / F x: id pose (12) has_prior var (6) / m x: id guess (3) has_prior cov (9) /
//           n x: frame_id point_id u v cov (4)
//   output: "error e" / "frame id R (9) t (3) cov (36)" / "point id x (3) cov (9)"
#include <cstdio>

#include "../../mvslam_amd/compat/mvslam_compat.hpp"

using namespace mvSLAM;

static bool rd(std::FILE *f, double *v, int n)
{
    for (int k = 0; k < n; ++k)
        if (std::fscanf(f, "%lf", &v[k]) != 1)
            return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f)
        return 2;
    int F = 0, m = 0, n = 0;
    if (std::fscanf(f, "%d %d %d", &F, &m, &n) != 3)
        return 2;
    CameraIntrinsics K;
    if (!rd(f, K.m, 9))
        return 2;
    std::unordered_set<Id::Type> fid, pid;
    std::unordered_map<Id::Type, Transformation> guess;
    std::unordered_map<Id::Type, TransformationUncertainty> fprior;
    std::unordered_map<Id::Type, Point3> pguess;
    std::unordered_map<Id::Type, Point3Uncertainty> pprior;
    std::unordered_map<Id::Type, PointIdToPoint2Estimate> fobs;
    for (int i = 0; i < F; ++i) {
        unsigned long id;
        int has;
        double p[12], var[6];
        if (std::fscanf(f, "%lu", &id) != 1 || !rd(f, p, 12) || std::fscanf(f, "%d", &has) != 1 || !rd(f, var, 6))
            return 2;
        Matrix3Type R;
        std::memcpy(R.m, p, sizeof(R.m));
        fid.insert(id);
        guess[id] = SE3(SO3(R, SO3::already_rectified_t()), Vector3Type(p[9], p[10], p[11]));
        if (has) {
            TransformationUncertainty C;
            for (int k = 0; k < 6; ++k)
                C(k, k) = var[k];
            fprior[id] = C;
        }
    }
    for (int i = 0; i < m; ++i) {
        unsigned long id;
        int has;
        double x[3], c[9];
        if (std::fscanf(f, "%lu", &id) != 1 || !rd(f, x, 3) || std::fscanf(f, "%d", &has) != 1 || !rd(f, c, 9))
            return 2;
        pid.insert(id);
        pguess[id] = Point3(x[0], x[1], x[2]);
        if (has) {
            Point3Uncertainty C;
            std::memcpy(C.m, c, sizeof(C.m));
            pprior[id] = C;
        }
    }
    for (int i = 0; i < n; ++i) {
        unsigned long a, b;
        double v[6];
        if (std::fscanf(f, "%lu %lu", &a, &b) != 2 || !rd(f, v, 6))
            return 2;
        Point2Uncertainty C;
        std::memcpy(C.m, v + 2, 4 * sizeof(double));
        fobs[a][b] = Point2Estimate(Point2(v[0], v[1]), C);
    }
    std::fclose(f);
    std::unordered_map<Id::Type, TransformationEstimate> fest;
    std::unordered_map<Id::Type, Point3Estimate> pest;
    ScalarType err = -1;
    try {
        ba_frame_pose_and_point(K, fid, pid, guess, fprior, pguess, pprior, fobs, fest, pest, err);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 1;
    }
    std::printf("error %.17g\n", err);
    for (const auto &kv : fest) {
        std::printf("frame %lu", (unsigned long)kv.first);
        const Matrix3Type R = kv.second.mean().rotation().get_matrix();
        const Vector3Type t = kv.second.mean().translation();
        for (int k = 0; k < 9; ++k)
            std::printf(" %.17g", R.m[k]);
        for (int k = 0; k < 3; ++k)
            std::printf(" %.17g", t[k]);
        for (int k = 0; k < 36; ++k)
            std::printf(" %.17g", kv.second.covar().m[k]);
        std::printf("\n");
    }
    for (const auto &kv : pest) {
        std::printf("point %lu", (unsigned long)kv.first);
        for (int k = 0; k < 3; ++k)
            std::printf(" %.17g", kv.second.mean()[k]);
        for (int k = 0; k < 9; ++k)
            std::printf(" %.17g", kv.second.covar().m[k]);
        std::printf("\n");
    }
    return 0;
}
