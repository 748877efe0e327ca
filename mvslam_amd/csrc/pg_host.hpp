// pg_host.hpp -- what the host decides about a pose graph before anything is launched (capi_graph.hip; DESIGN.md section
// 4.10): finite input, endpoints in range, connectivity, the incidence list of the large path, the arguments of the robust
// loss.  Plain C++ with no HIP in it, so that tests/cpp/pg_host_check.cpp and tests/cpp/pg_loss_args_check.cpp can run it under
// the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mvs_pg {

inline bool all_finite(const double *v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i]))
            return false;
    return true;
}

// the scale of every Sim(3) record (13 doubles: R, t, s) is > 0 (mvs_sim3_graph_optimize; the records are finite already)
inline bool sim3_scales_positive(const double *v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!(v[13 * i + 12] > 0.0))
            return false;
    return true;
}
// mvs_seq_optimize_pose_graph_sim3's scale_sigma: one per edge kind, each finite and > 0
inline bool scale_sigmas_ok(const double *sigma)
{
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(sigma[i]) || !(sigma[i] > 0.0))
            return false;
    return true;
}

// mvs_ctx_set_pose_graph_loss's arguments: a loss of 0 (none), 1 (Huber) or 2 (Cauchy); with a loss, a constant k that is
// finite and > 0; first_edge >= -1 (-1: the loop edges of a resident graph)
inline bool loss_args_ok(int loss, double k, int32_t first_edge)
{
    if (loss < 0 || loss > 2 || first_edge < -1)
        return false;
    return loss == 0 || (std::isfinite(k) && k > 0.0);
}
// mvs_ctx_set_ba_loss's arguments: the same rule for the loss and its constant; a bundle
// adjustment has no first_edge
inline bool ba_loss_args_ok(int loss, double k)
{
    return loss_args_ok(loss, k, 0);
}
// may a call on a host graph run under this setting?  It has no loop edges for first_edge = -1 to stand for.
inline bool loss_fits_host_graph(int loss, int32_t first_edge)
{
    return loss == 0 || first_edge >= 0;
}

// every edge joins two different nodes of [0, n_nodes).  The two functions below index by the endpoints: they are called on
// edges that have passed this check only.
inline bool edges_in_range(int n_nodes, int n_edges, const int32_t *src, const int32_t *dst)
{
    for (int k = 0; k < n_edges; ++k)
        if (src[k] < 0 || src[k] >= n_nodes || dst[k] < 0 || dst[k] >= n_nodes || src[k] == dst[k])
            return false;
    return true;
}

// does a path of edges join every node to the anchor?  (With lambda on the diagonal a floating component would not break
// the linear solve: its gauge freedom only leaves the values where they are.  So the topology is checked, exactly.)
inline bool pose_graph_connected(int n_nodes, int n_edges, const int32_t *src, const int32_t *dst, int anchor)
{
    std::vector<int> parent((size_t)n_nodes);
    for (int i = 0; i < n_nodes; ++i)
        parent[(size_t)i] = i;
    auto find = [&](int a) {
        while (parent[(size_t)a] != a)
            a = parent[(size_t)a] = parent[(size_t)parent[(size_t)a]];
        return a;
    };
    for (int k = 0; k < n_edges; ++k)
        parent[(size_t)find(src[k])] = find(dst[k]);
    const int root = find(anchor);
    for (int i = 0; i < n_nodes; ++i)
        if (find(i) != root)
            return false;
    return true;
}

// CSR list of the incident edges of every node, in edge order: node i has inc[off[i]] .. inc[off[i + 1] - 1], an entry
// 2 k for the edge k that leaves it and 2 k + 1 for the edge k that ends in it.
inline void incidence_csr(int n_nodes, int n_edges, const int32_t *src, const int32_t *dst, std::vector<int32_t> &off,
                          std::vector<int32_t> &inc)
{
    const size_t N = (size_t)n_nodes, E = (size_t)n_edges;
    off.assign(N + 1, 0);
    inc.assign(2 * E, 0);
    for (size_t k = 0; k < E; ++k) {
        ++off[(size_t)src[k] + 1];
        ++off[(size_t)dst[k] + 1];
    }
    for (size_t i = 0; i < N; ++i)
        off[i + 1] += off[i];
    std::vector<int32_t> fill(off.begin(), off.end() - 1);
    for (size_t k = 0; k < E; ++k) {
        inc[(size_t)fill[(size_t)src[k]]++] = (int32_t)(2 * k);
        inc[(size_t)fill[(size_t)dst[k]]++] = (int32_t)(2 * k + 1);
    }
}

}  // namespace mvs_pg
