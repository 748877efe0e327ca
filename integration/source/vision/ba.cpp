// Replaces source/vision/ba.cpp of the reference (ba_frame_pose_and_point :26-156; decl vision/ba.hpp:25-36) -- the one
// translation unit of the front end that talks to GTSAM.  The same cost (diagonal pose priors, point priors, one
// projection factor per observation with the keypoint's covariance) is minimised by the library's batched
// Schur-complement Levenberg-Marquardt kernel; marginal covariances from the linearised system at the
// estimate, final_error = the optimiser's error, as :130-155.  Supported: frame sets of 1 to 4096 frames -- what the
// reference builds (sfm-refine.cpp:20-139, pnp-refine.cpp:14-108, VisualOdometer::track_refine visual-odometer.cpp:618-800:
// one or two frames), sliding windows of up to eight on top of it (mvs_ba_refine_window), and from nine frames on the
// sparse problem of mvs_ba_refine_sparse, where an observation a frame lacks is simply absent.
// With this file in place sfm-refine.cpp, pnp-refine.cpp and visual-odometer.cpp stay untouched and GTSAM leaves the
// front end's link line.
#include <vision/ba.hpp>

#include <algorithm>
#include <cassert>
#include <cstring>
#include <stdexcept>

#include "mvslam-hip-glue.hpp"

namespace mvSLAM
{
void ba_frame_pose_and_point(const CameraIntrinsics &ci, const std::unordered_set<Id::Type> &frame_id,
                             const std::unordered_set<Id::Type> &point_id,
                             const std::unordered_map<Id::Type, Transformation> &frame_pose_guess,
                             const std::unordered_map<Id::Type, TransformationUncertainty> &frame_pose_prior,
                             const std::unordered_map<Id::Type, Point3> &point_guess,
                             const std::unordered_map<Id::Type, Point3Uncertainty> &point_prior,
                             const std::unordered_map<Id::Type, PointIdToPoint2Estimate> &frame_observation,
                             std::unordered_map<Id::Type, TransformationEstimate> &frame_pose_estimate,
                             std::unordered_map<Id::Type, Point3Estimate> &point_estimate, ScalarType &final_error)
{
    assert(frame_id.size() > 0 && frame_id.size() <= 4096);   // ba.cpp:39; mvs_ba_refine_sparse's capacity
    assert(point_id.size() > 0);
    assert(frame_pose_guess.size() == frame_id.size() && point_guess.size() == point_id.size());
    assert(frame_pose_prior.size() + point_prior.size() >= 2);   // ba.cpp:43
    std::vector<Id::Type> fids(frame_id.begin(), frame_id.end()), pids(point_id.begin(), point_id.end());
    std::sort(fids.begin(), fids.end());
    std::sort(pids.begin(), pids.end());
    const int F = (int)fids.size(), m = (int)pids.size();
    std::unordered_map<Id::Type, int> pidx;
    for (int i = 0; i < m; ++i)
        pidx[pids[i]] = i;
    std::vector<double> pose(12 * (size_t)F), var(6 * (size_t)F, 0.0), pts(3 * (size_t)m), pcov(9 * (size_t)m, 0.0);
    for (int f = 0; f < F; ++f) {
        const Transformation &T = frame_pose_guess.at(fids[f]);
        hip::to_row_major(T.rotation().get_matrix(), &pose[12 * (size_t)f]);
        const Vector3Type t = T.translation();
        std::memcpy(&pose[12 * (size_t)f + 9], t.data(), 3 * sizeof(double));
        auto pr = frame_pose_prior.find(fids[f]);
        if (pr != frame_pose_prior.end())
            for (int k = 0; k < 6; ++k)          // the reference's priors are diagonal (sfm-refine.cpp:58-78)
                var[6 * (size_t)f + k] = pr->second(k, k);
    }
    for (int i = 0; i < m; ++i) {
        std::memcpy(&pts[3 * (size_t)i], point_guess.at(pids[i]).data(), 3 * sizeof(double));
        auto pr = point_prior.find(pids[i]);
        if (pr != point_prior.end())
            std::memcpy(&pcov[9 * (size_t)i], pr->second.data(), 9 * sizeof(double));         // symmetric 3x3
    }
    double Kr[9];
    hip::to_row_major(ci, Kr);
    mvs_refine_params prm;
    mvs_refine_params_default(&prm);
    std::vector<mvs_refine_result> res(F);
    std::vector<double> po(3 * (size_t)m), pc(9 * (size_t)m);
    if (F <= 8) {
        std::vector<std::vector<double>> obs(F), ocov(F);
        std::vector<std::vector<uint8_t>> valid(F);
        std::vector<const double *> obs_p(F), ocov_p(F);
        std::vector<const uint8_t *> valid_p(F);
        for (int f = 0; f < F; ++f) {
            obs[f].assign(2 * (size_t)m, 0.0);
            ocov[f].assign(4 * (size_t)m, 0.0);
            valid[f].assign(m, 0);
            auto ob = frame_observation.find(fids[f]);
            if (ob != frame_observation.end())
                for (const auto &kv : ob->second) {
                    const int i = pidx.at(kv.first);
                    std::memcpy(&obs[f][2 * i], kv.second.mean().data(), 2 * sizeof(double));
                    std::memcpy(&ocov[f][4 * i], kv.second.covar().data(), 4 * sizeof(double));   // symmetric 2x2
                    valid[f][i] = 1;
                }
            obs_p[f] = obs[f].data();
            ocov_p[f] = ocov[f].data();
            valid_p[f] = valid[f].data();
        }
        mvs_ba_window pb;
        std::memset(&pb, 0, sizeof(pb));
        pb.n_frames = F;
        pb.n_points = m;
        pb.K = Kr;
        pb.frame_pose = pose.data();
        pb.frame_prior_var = var.data();
        pb.points = pts.data();
        pb.point_prior_cov = pcov.data();
        pb.obs = obs_p.data();
        pb.obs_cov = ocov_p.data();
        pb.obs_valid = valid_p.data();
        if (mvs_ba_refine_window(hip::context(), &pb, &prm, res.data(), po.data(), pc.data()) != MVS_OK)
            throw std::runtime_error("ba_frame_pose_and_point: indeterminate system");   // GTSAM throws here as well
    } else {
        // nine frames and more: the observations of every point in ascending frame order (mvs_ba_sparse)
        std::vector<int32_t> off((size_t)m + 1, 0);
        for (int f = 0; f < F; ++f) {
            auto ob = frame_observation.find(fids[f]);
            if (ob != frame_observation.end())
                for (const auto &kv : ob->second)
                    ++off[(size_t)pidx.at(kv.first) + 1];
        }
        for (int i = 0; i < m; ++i)
            off[(size_t)i + 1] += off[(size_t)i];
        const size_t n = (size_t)off[(size_t)m];
        std::vector<int32_t> fr(n), at(off.begin(), off.end() - 1);
        std::vector<double> uv(2 * n), cv(4 * n);
        for (int f = 0; f < F; ++f) {
            auto ob = frame_observation.find(fids[f]);
            if (ob == frame_observation.end())
                continue;
            for (const auto &kv : ob->second) {
                const size_t o = (size_t)at[(size_t)pidx.at(kv.first)]++;
                fr[o] = f;
                std::memcpy(&uv[2 * o], kv.second.mean().data(), 2 * sizeof(double));
                std::memcpy(&cv[4 * o], kv.second.covar().data(), 4 * sizeof(double));
            }
        }
        mvs_ba_sparse pb;
        std::memset(&pb, 0, sizeof(pb));
        pb.n_frames = F, pb.n_points = m, pb.n_obs = (int32_t)n;
        pb.K = Kr;
        pb.frame_pose = pose.data(), pb.frame_prior_var = var.data(), pb.points = pts.data(), pb.point_prior_cov = pcov.data();
        pb.obs_off = off.data(), pb.obs_frame = fr.data(), pb.obs_uv = uv.data(), pb.obs_cov = cv.data();
        mvs_ba_sparse_result sr;
        std::vector<double> fp(12 * (size_t)F), fc(36 * (size_t)F);
        if (mvs_ba_refine_sparse(hip::context(), &pb, &prm, &sr, fp.data(), po.data(), fc.data(), pc.data()) != MVS_OK)
            throw std::runtime_error("ba_frame_pose_and_point: indeterminate system");
        for (int f = 0; f < F; ++f) {
            res[f].ok = 1, res[f].iterations = sr.iterations, res[f].error = sr.error;
            std::memcpy(res[f].R, &fp[12 * (size_t)f], 9 * sizeof(double));
            std::memcpy(res[f].t, &fp[12 * (size_t)f + 9], 3 * sizeof(double));
            std::memcpy(res[f].pose_cov, &fc[36 * (size_t)f], 36 * sizeof(double));
        }
    }
    frame_pose_estimate.clear();
    for (int f = 0; f < F; ++f) {
        TransformationUncertainty C;
        std::memcpy(C.data(), res[f].pose_cov, 36 * sizeof(double));                   // symmetric 6x6, tangent order
        frame_pose_estimate[fids[f]] = TransformationEstimate(hip::se3_from_arrays(res[f].R, res[f].t), C);   // (rotation, translation) as ba.cpp:141
    }
    point_estimate.clear();
    for (int i = 0; i < m; ++i) {
        Point3Uncertainty C;
        std::memcpy(C.data(), &pc[9 * (size_t)i], 9 * sizeof(double));
        point_estimate[pids[i]] = Point3Estimate(Point3(po[3 * i], po[3 * i + 1], po[3 * i + 2]), C);
    }
    final_error = res[0].error;
}
}  // namespace mvSLAM
