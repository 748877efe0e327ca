// The shim's ImagePair constructor on two synthetic pairs, printed bit for bit: valid, the pose, the matched points and their
// keypoint indices.  tests/test_essential_paths_gpu.py builds this file with MVSLAM_USE_ESSENTIAL_5POINT twice -- with and
// without MVSLAM_ESSENTIAL_ONE_PASS (one mvs_image_pair_essential call against mvs_match_hamming + mvs_two_view_essential) --
// and compares everything behind the first line; it also compiles with neither macro (the 8-point mvs_image_pair).
//   usage: image_pair_one_pass
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../mvslam_amd/compat/mvslam_compat.hpp"

using namespace mvSLAM;

static uint64_t bits(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, sizeof(u));
    return u;
}

// n_kp keypoints of a camera pair 0.3 m apart with a small yaw; the first n_match of them carry the same descriptor in both
// images, the others independent random ones (no match under the distance bound)
static void print_pair(int id, int n_kp, int n_match)
{
    std::mt19937_64 rng(7 + id);
    std::normal_distribution<double> noise(0.0, 0.5);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    CameraIntrinsics K = CameraIntrinsics::Identity();
    K(0, 0) = 525; K(1, 1) = 525; K(0, 2) = 320; K(1, 2) = 240;
    const double yaw = 0.03, c = std::cos(yaw), s = std::sin(yaw);
    std::vector<KeyPoint> k1(n_kp), k2(n_kp);
    Mat8u d1, d2;
    d1.cols = d2.cols = 32; d1.rows = d2.rows = n_kp;
    d1.data.resize((size_t)n_kp * 32); d2.data.resize((size_t)n_kp * 32);
    for (int i = 0; i < n_kp; ++i) {
        const double Z = 2 + 8 * U(rng), X = (U(rng) - 0.5) * Z, Y = (U(rng) - 0.5) * 0.8 * Z;
        const double X2 = c * X - s * Z - 0.3, Z2 = s * X + c * Z;
        k1[i] = KeyPoint{};
        k2[i] = KeyPoint{};
        k1[i].pt.x = (float)(525 * X / Z + 320 + noise(rng)); k1[i].pt.y = (float)(525 * Y / Z + 240 + noise(rng));
        k2[i].pt.x = (float)(525 * X2 / Z2 + 320 + noise(rng)); k2[i].pt.y = (float)(525 * Y / Z2 + 240 + noise(rng));
        for (int b = 0; b < 32; ++b) {
            const uint8_t v = (uint8_t)(rng() & 0xff);
            d1.data[(size_t)i * 32 + b] = v;
            d2.data[(size_t)i * 32 + b] = i < n_match ? v : (uint8_t)(rng() & 0xff);
        }
    }
    Frame f1{1, VisualFeature(k1, d1, 640, 480)}, f2{2, VisualFeature(k2, d2, 640, 480)};
    ImagePair ip(f1, f2, K);
    std::printf("pair %d valid %d inliers %u points %zu\n", id, ip.valid ? 1 : 0, ip.valid ? ip.match_inlier_count : 0u,
                ip.matched_points.size());
    if (!ip.valid)
        return;
    const Matrix3Type R = ip.T_pair_to_base.rotation().get_matrix();
    const Vector3Type t = ip.T_pair_to_base.translation();
    for (int k = 0; k < 9; ++k)
        std::printf("R%d %016" PRIx64 "\n", k, bits(R.m[k]));
    for (int k = 0; k < 3; ++k)
        std::printf("t%d %016" PRIx64 "\n", k, bits(t[k]));
    for (const auto &mp : ip.matched_points)
        std::printf("p %zu %zu %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", mp.vf_idx_in_base, mp.vf_idx_in_pair,
                    bits(mp.position[0]), bits(mp.position[1]), bits(mp.position[2]));
}

int main()
{
#if defined(MVSLAM_USE_ESSENTIAL_5POINT) && defined(MVSLAM_ESSENTIAL_ONE_PASS)
    std::printf("path five-point, one pass\n");
#elif defined(MVSLAM_USE_ESSENTIAL_5POINT)
    std::printf("path five-point, two calls\n");
#else
    std::printf("path eight-point, one pass\n");
#endif
    hip::ransac_config().num_hypotheses = 128;
    hip::ransac_config().sampler = MVS_SAMPLER_PHILOX;
    hip::ransac_config().seed = 1;
    hip::ransac_config().max_error_sq = 1e-2;
    print_pair(0, 400, 280);   // a model
    print_pair(1, 120, 7);     // seven matches: none
    print_pair(2, 120, 0);     // no match at all
    return 0;
}
