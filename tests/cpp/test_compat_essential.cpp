// The reference's headline test sfm_solve_cube (test/test-sfm.cpp:17-90) through the drop-in shim
// (mvslam_amd/compat/mvslam_compat.hpp).  Compiled twice by tests/test_compat_essential.py:
//   - with -DMVSLAM_USE_ESSENTIAL_5POINT (the analogue of the reference's USE_OPENCV_ESSENTIAL_MATRIX): sfm_solve is the
//     five-point RANSAC and the reference's assertions hold -- pose.ln() == (1, 0, 0, 0, 0, 0), the eight points in order, 1e-3;
//   - without it: the same translation unit is the 8-point path.
// Either way the pose sfm_solve returns is, bit for bit, the one of the C ABI entry the build is meant to forward to
// (mvs_two_view_essential / mvs_two_view), and the two entries give different records on this rig.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#ifdef MVSLAM_USE_ESSENTIAL_5POINT
#define E5_EXPECTED 1
#else
#define E5_EXPECTED 0
#endif
#include "../../mvslam_amd/compat/mvslam_compat.hpp"

static int g_fail = 0;
#define ASSERT_TRUE(c) do { if (!(c)) { std::printf("  FAILED %s:%d  %s\n", __FILE__, __LINE__, #c); ++g_fail; return; } } while (0)
#define RUN(t) do { int before = g_fail; std::printf("[ RUN  ] %s\n", #t); t(); std::printf(g_fail == before ? "[  OK  ] %s\n" : "[ FAIL ] %s\n", #t); } while (0)

using namespace mvSLAM;

struct Rig
{
    CameraIntrinsics K = Matrix3Type::Identity();
    CameraExtrinsics P1, P2;
    std::vector<Point3> X;
    std::vector<ImagePoint> ip1, ip2;
};
static Rig make_rig(bool cube)
{   // test/test-sfm.cpp:19-42, test/unit-test-helper.cpp:42-79
    Rig r;
    std::vector<Vector3Type> p;
    if (cube) {
        for (int x = -1; x <= 1; x += 2) for (int y = -1; y <= 1; y += 2) for (int z = -1; z <= 1; z += 2) p.emplace_back(x, y, z);
    } else {
        p = {{1, 0, 0}, {0, 0, 0}, {0, 2, 0}, {1, 0, 3}, {0, 0, 3}, {0, 2, 3}, {0.5, 0.0, 1.5}, {0.0, 1.0, 1.5}};
    }
    const SO3 rot = cube ? SO3(0.0, 0.0, 0.0) : SO3(1.5, 0.7, 0.0);
    const ScalarType scale = cube ? 1.0 : 0.5;
    for (auto &q : p)
        q = rot * Vector3Type(scale * q[0], scale * q[1], scale * q[2]) + Vector3Type(0.6, 0.0, 3.0);
    Vector6Type se3_2to1{1, 0, 0, 0, 0, 0};
    r.P2 = SE3::exp(se3_2to1).inverse();
    r.X = p;
    r.ip1 = PinholeCamera(r.K, r.P1).project_points(r.X);
    r.ip2 = PinholeCamera(r.K, r.P2).project_points(r.X);
    return r;
}

// the assertions of test-sfm.cpp:60-90; false instead of a failure so that the 8-point build can assert the opposite
static bool cube_assertions_hold(const Rig &r, bool solved, const Transformation &pose2in1, const std::vector<Point3> &points,
                                 const std::vector<size_t> &idx)
{
    const ScalarType tol = 0.001;
    if (!solved || points.size() != r.X.size())
        return false;
    const Vector6Type expect{1, 0, 0, 0, 0, 0}, got = pose2in1.ln();
    for (int i = 0; i < 6; ++i)
        if (!(std::fabs(expect[i] - got[i]) <= tol))
            return false;
    for (size_t i = 0; i < points.size(); ++i) {
        if (idx[i] != i)
            return false;
        for (int j = 0; j < 3; ++j)
            if (!(std::fabs(r.X[i][j] - points[i][j]) <= tol))
                return false;
    }
    return true;
}

static void set_search()
{
    // the estimator's own search: 64 hypotheses of the keyed sampler (cv::findEssentialMat runs its own RANSAC loop; the first
    // five cube points alone, four of them on one face, are a degenerate sample)
    hip::ransac_config().num_hypotheses = 64;
    hip::ransac_config().sampler = MVS_SAMPLER_PHILOX;
    hip::ransac_config().seed = 0;
}

static void sfm_solve_cube()
{
    set_search();
    Rig r = make_rig(true);
    Transformation pose2in1;
    std::vector<Point3> points;
    std::vector<size_t> idx;
    const bool solved = sfm_solve(r.ip1, r.ip2, r.K, pose2in1, points, idx);
    hip::ransac_config() = hip::RansacConfig();
#if E5_EXPECTED
    ASSERT_TRUE(cube_assertions_hold(r, solved, pose2in1, points, idx));
#else
    (void)cube_assertions_hold;   // the cube pins nothing on the 8-point path: its design matrix has rank 7
    (void)solved;
#endif
}

static void sfm_solve_forwards_to_the_entry_of_this_build()
{
    set_search();
    Rig r = make_rig(true);
    Transformation pose2in1;
    std::vector<Point3> points;
    std::vector<size_t> idx;
    const bool solved = sfm_solve(r.ip1, r.ip2, r.K, pose2in1, points, idx);
    const mvs_params prm = make_params_();
    hip::ransac_config() = hip::RansacConfig();
    const int m = (int)r.ip1.size();
    std::vector<double> pts(3 * (size_t)m);
    std::vector<int64_t> ix(m);
    double R5[9], t5[3], R8[9], t8[3];
    int n5 = 0, n8 = 0;
    mvs_pair_result res5, res8;
    const mvs_status s5 = mvs_two_view_essential(hip::context(), &r.ip1[0].x, &r.ip2[0].x, m, r.K.data(), &prm, R5, t5, pts.data(),
                                                 ix.data(), &n5, nullptr, &res5);
    const mvs_status s8 = mvs_two_view(hip::context(), &r.ip1[0].x, &r.ip2[0].x, m, r.K.data(), &prm, R8, t8, pts.data(), ix.data(),
                                       &n8, nullptr, &res8);
    ASSERT_TRUE(s5 == MVS_OK);
    ASSERT_TRUE(std::memcmp(res5.E, res8.E, sizeof(res5.E)) != 0);   // two estimators: two different records
    const bool want_ok = E5_EXPECTED ? s5 == MVS_OK : s8 == MVS_OK;
    ASSERT_TRUE(solved == want_ok);
    if (solved) {
        const Transformation want = se3_from_arrays_(E5_EXPECTED ? R5 : R8, E5_EXPECTED ? t5 : t8);
        const Vector6Type a = pose2in1.ln(), b = want.ln();
        for (int i = 0; i < 6; ++i) ASSERT_TRUE(a[i] == b[i]);
        ASSERT_TRUE((int)points.size() == (E5_EXPECTED ? n5 : n8));
    }
}

static void sfm_solve_L_shape_on_either_path()
{
    set_search();
    Rig r = make_rig(false);
    Transformation pose2in1;
    std::vector<Point3> points;
    std::vector<size_t> idx;
    const bool solved = sfm_solve(r.ip1, r.ip2, r.K, pose2in1, points, idx);
    hip::ransac_config() = hip::RansacConfig();
    ASSERT_TRUE(cube_assertions_hold(r, solved, pose2in1, points, idx));
}

int main()
{
    try {
        RUN(sfm_solve_cube);
        RUN(sfm_solve_forwards_to_the_entry_of_this_build);
        RUN(sfm_solve_L_shape_on_either_path);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION: %s\n", e.what());
        return 2;
    }
    if (g_fail)
        std::printf("%d FAILED\n", g_fail);
    else
        std::printf("ALL PASSED %s\n", E5_EXPECTED ? "five-point" : "eight-point");
    return g_fail ? 1 : 0;
}
