// One graph of more than 16 nodes through mvSLAM::GraphOptimizer of the shim (mvslam_amd/compat/mvslam_compat.hpp).  Compiled
// twice by tests/test_compat_graph_direct.py, with and without -DMVSLAM_POSE_GRAPH_SOLVER=1; prints the solver's CG iteration
// count and every optimised pose as its se3 coordinates, which the test compares.
#include <cstdio>
#include <random>
#include <vector>

#include "../../mvslam_amd/compat/mvslam_compat.hpp"

using namespace mvSLAM;

int main()
{
    const int n = 24;
    const ScalarType sigma = 0.01;
    std::mt19937 rng(7);
    std::normal_distribution<double> noise(0.0, sigma);
    const SE3 step(SO3(0.0, 0.0, 2.0 * M_PI / n), Vector3Type{0.5, 0.0, 0.02});
    SE3 origin;
    Graph graph(origin);
    std::vector<BackEndTypes::NodeId> ids{graph.get_origin_node_id()};
    const TransformationUncertainty uncertainty = sqr(sigma) * TransformationUncertainty::Identity();
    auto noisy = [&](const SE3 &m) {
        Vector6Type d;
        for (int k = 0; k < 6; ++k)
            d[k] = noise(rng);
        return m * SE3::exp(d);
    };
    SE3 reckoned = origin;
    for (int i = 1; i < n; ++i) {
        const SE3 mean = noisy(step);
        reckoned = reckoned * mean;
        const auto id = graph.add_pose_node(reckoned);
        graph.add_transformation_edge(ids.back(), id, TransformationEstimate(mean, uncertainty));
        if (i >= 2)
            graph.add_transformation_edge(ids[i - 2], id, TransformationEstimate(noisy(step * step), uncertainty));
        ids.push_back(id);
    }
    GraphOptimizer optimizer(graph);
    optimizer.optimize();
    if (!optimizer.update_graph(graph) || optimizer.result().ok != 1)
        return 1;
    std::printf("solver %d cg_iterations %d iterations %d\n", MVSLAM_POSE_GRAPH_SOLVER, optimizer.result().cg_iterations,
                optimizer.result().iterations);
    for (auto id : ids) {
        const Vector6Type v = graph.get_pose_node_value(id).ln();
        std::printf("pose %.17g %.17g %.17g %.17g %.17g %.17g\n", v[0], v[1], v[2], v[3], v[4], v[5]);
    }
    return 0;
}
