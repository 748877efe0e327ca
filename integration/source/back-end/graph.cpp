// Replaces source/back-end/graph.cpp of the reference (Graph :96-226, GraphOptimizer :228-293; decl back-end/graph.hpp): the
// gtsam::NonlinearFactorGraph + Values pair becomes plain node and edge tables, and GraphOptimizer::optimize -- GTSAM's
// LevenbergMarquardtOptimizer over PriorFactor + BetweenFactor<Pose3> -- becomes mvs_pose_graph_optimize.
// The edge keeps GTSAM's meaning (its mean measures X_src^-1 X_dst, its covariance goes over unchanged, :153-155); the
// origin is anchored at GRAPH_ANCHOR_STDDEV = 1e-4 (:83, the library's default).  print() only prints the tables.
// The id generators (BackEndTypes::generate_*_id) stay where they are, in back-end/data-type.cpp, which is not replaced.
#include <back-end/graph.hpp>

#include <cassert>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

#include "../vision/mvslam-hip-glue.hpp"

namespace mvSLAM
{
class GraphImpl
{
public:
    struct Node { BackEndTypes::NodeId id; BackEndTypes::PoseNodeValue value; };
    struct Edge { BackEndTypes::EdgeId id; BackEndTypes::NodeId src, dst; BackEndTypes::TransformationEdgeValue value; };
    BackEndTypes::GraphId id = Id::INVALID;
    BackEndTypes::NodeId origin_node_id = Id::INVALID;
    std::vector<Node> nodes;     // insertion order = node index of the C ABI
    std::vector<Edge> edges;
    std::unordered_map<BackEndTypes::NodeId, size_t> index;
    std::unordered_set<BackEndTypes::EdgeId> edge_ids;
};

Graph::Graph(const BackEndTypes::PoseNodeValue &origin) : m_impl(new GraphImpl())
{
    m_impl->id = BackEndTypes::generate_graph_id();
    m_impl->origin_node_id = add_pose_node(origin);
}
Graph::~Graph() { delete m_impl; }

BackEndTypes::NodeId Graph::add_pose_node(const BackEndTypes::PoseNodeValue &P)
{
    const BackEndTypes::NodeId id = BackEndTypes::generate_node_id();
    m_impl->index[id] = m_impl->nodes.size();
    m_impl->nodes.push_back(GraphImpl::Node{id, P});
    return id;
}

BackEndTypes::EdgeId Graph::add_transformation_edge(BackEndTypes::NodeId src, BackEndTypes::NodeId dst,
                                                    const BackEndTypes::TransformationEdgeValue &T)
{
    assert(has_node(src) && has_node(dst));
    const BackEndTypes::EdgeId id = BackEndTypes::generate_edge_id();
    m_impl->edge_ids.insert(id);
    m_impl->edges.push_back(GraphImpl::Edge{id, src, dst, T});
    return id;
}

bool Graph::has_node(BackEndTypes::NodeId node_id) const { return node_id != Id::INVALID && m_impl->index.count(node_id) == 1; }
bool Graph::has_edge(BackEndTypes::EdgeId edge_id) const { return edge_id != Id::INVALID && m_impl->edge_ids.count(edge_id) == 1; }

BackEndTypes::PoseNodeValue Graph::get_pose_node_value(BackEndTypes::NodeId node_id) const
{
    assert(has_node(node_id));
    return m_impl->nodes[m_impl->index.at(node_id)].value;
}

std::unordered_map<BackEndTypes::NodeId, BackEndTypes::PoseNodeValue> Graph::get_all_pose_node_value() const
{
    std::unordered_map<BackEndTypes::NodeId, BackEndTypes::PoseNodeValue> out;
    for (const auto &n : m_impl->nodes)
        out[n.id] = n.value;
    return out;
}

bool Graph::reconcile_with(Graph &) { return false; }   // the reference asserts "NOT implemented yet" (:196-208)
BackEndTypes::GraphId Graph::get_id() const { return m_impl->id; }
BackEndTypes::NodeId Graph::get_origin_node_id() const { return m_impl->origin_node_id; }
void Graph::print(const char *s) const
{
    std::printf("%s\ngraph %zu: %zu nodes, %zu edges\n", s, (size_t)m_impl->id, m_impl->nodes.size(), m_impl->edges.size());
}

class GraphOptimizerImpl
{
public:
    GraphImpl graph;   // the deep copy (graph.hpp:84-89)
    bool optimized = false;
};

GraphOptimizer::GraphOptimizer(const Graph &g) : m_impl(new GraphOptimizerImpl()) { m_impl->graph = *g.m_impl; }
GraphOptimizer::~GraphOptimizer() { delete m_impl; }

void GraphOptimizer::optimize()
{
    GraphImpl &G = m_impl->graph;
    const size_t N = G.nodes.size(), E = G.edges.size();
    std::vector<double> np(12 * N), ep(12 * E), ec(36 * E), out(12 * N);
    std::vector<int32_t> src(E), dst(E);
    auto put = [](const Transformation &T, double *p) {
        hip::to_row_major(T.rotation().get_matrix(), p);
        for (int k = 0; k < 3; ++k)
            p[9 + k] = T.translation()[k];
    };
    for (size_t i = 0; i < N; ++i)
        put(G.nodes[i].value, &np[12 * i]);
    for (size_t k = 0; k < E; ++k) {
        src[k] = (int32_t)G.index.at(G.edges[k].src);
        dst[k] = (int32_t)G.index.at(G.edges[k].dst);
        put(G.edges[k].value.mean(), &ep[12 * k]);
        const TransformationUncertainty &C = G.edges[k].value.covar();
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c)
                ec[36 * k + 6 * r + c] = C(r, c);
    }
    mvs_pose_graph pg{};
    pg.n_nodes = (int32_t)N, pg.n_edges = (int32_t)E;
    pg.node_pose = np.data(), pg.edge_src = src.data(), pg.edge_dst = dst.data();
    pg.edge_pose = ep.data(), pg.edge_cov = ec.data();
    pg.anchor_node = (int32_t)G.index.at(G.origin_node_id);
    mvs_pose_graph_params prm;
    mvs_pose_graph_params_default(&prm);
    mvs_pose_graph_result res{};
    const mvs_status st = mvs_pose_graph_optimize(hip::context(), &pg, &prm, &res, out.data());
    if (st == MVS_NO_MODEL)
        return;   // a graph the library cannot solve keeps its values; update_graph() then returns false
    if (st != MVS_OK)   // arguments, capacity, runtime: the failures the shim's GraphOptimizer throws on as well
        throw std::runtime_error(std::string("GraphOptimizer::optimize: ") + mvs_status_str(st));
    for (size_t i = 0; i < N; ++i)
        G.nodes[i].value = hip::se3_from_arrays(&out[12 * i], &out[12 * i + 9]);
    m_impl->optimized = true;
}

bool GraphOptimizer::update_graph(Graph &g)
{
    if (!m_impl->optimized)
        return false;
    for (const auto &n : m_impl->graph.nodes) {   // only nodes known to both; nothing is added (graph.hpp:99-108)
        auto it = g.m_impl->index.find(n.id);
        if (it != g.m_impl->index.end())
            g.m_impl->nodes[it->second].value = n.value;
    }
    return true;
}
}  // namespace mvSLAM
