// Stand-alone check of the pose-graph back end's pure host logic (mvslam_amd/csrc/pg_host.hpp): finite input, endpoints in
// range, connectivity and the incidence list of the large path.  tests/test_pose_graph_host.py builds it with
// -fsanitize=address,undefined and runs it; it needs no GPU and loads nothing.  Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pg_host.hpp"

using namespace mvs_pg;
using Edges = std::vector<int32_t>;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// edges in range; connected as expected; the CSR arrays against the incidence list found edge by edge
static void check_graph(int N, const Edges &src, const Edges &dst, int anchor, bool joined)
{
    const int E = (int)src.size();
    const int32_t *s = E ? src.data() : nullptr, *d = E ? dst.data() : nullptr;
    CHECK(edges_in_range(N, E, s, d));
    CHECK(pose_graph_connected(N, E, s, d, anchor) == joined);
    std::vector<int32_t> off(3, 7), inc(5, 7);   // stale contents must not survive
    incidence_csr(N, E, s, d, off, inc);
    CHECK((int)off.size() == N + 1 && (int)inc.size() == 2 * E && off[0] == 0 && off[(size_t)N] == 2 * E);
    for (int i = 0; i < N; ++i) {
        std::vector<int32_t> brute;
        for (int k = 0; k < E; ++k) {
            if (src[(size_t)k] == i)
                brute.push_back(2 * k);
            if (dst[(size_t)k] == i)
                brute.push_back(2 * k + 1);
        }
        CHECK(off[(size_t)i + 1] - off[(size_t)i] == (int)brute.size());
        for (size_t j = 0; j < brute.size(); ++j)
            CHECK(inc[(size_t)off[(size_t)i] + j] == brute[j]);
    }
}

int main()
{
    check_graph(1, {}, {}, 0, true);                                   // N = 1, E = 0, null edge pointers
    check_graph(6, {0, 1, 2, 3, 4}, {1, 2, 3, 4, 5}, 3, true);         // a chain
    for (int anchor : {0, 4})                                          // two components, the anchor in either one
        check_graph(6, {0, 1, 3, 4}, {1, 2, 4, 5}, anchor, false);
    check_graph(4, {0, 1, 0, 1, 2, 3, 2}, {1, 0, 1, 2, 3, 2, 1}, 2, true);   // duplicates and both orientations
    check_graph(3, {0, 1, 0}, {1, 0, 1}, 0, false);                    // ... that still leave node 2 out
    {
        const int N = 4096;                                            // a hub: node 7 joined to every other node
        Edges src, dst;
        for (int i = 0; i < N; ++i)
            if (i != 7) {
                src.push_back(i % 2 ? 7 : i);
                dst.push_back(i % 2 ? i : 7);
            }
        check_graph(N, src, dst, N - 1, true);
    }
    // endpoints outside [0, N) and loops: refused, and nothing else is called on them
    const int32_t bad[][2] = {{-1, 0}, {0, -1}, {3, 0}, {0, 3}, {1, 1}};
    for (const auto &e : bad) {
        const Edges src = {0, e[0]}, dst = {1, e[1]};
        CHECK(!edges_in_range(3, 2, src.data(), dst.data()));
        CHECK(edges_in_range(3, 1, src.data(), dst.data()));           // the edge in front of it alone is fine
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double v[4] = {0.0, -1.5, 1e308, 5e-324};
    CHECK(all_finite(nullptr, 0) && all_finite(v, 4));
    for (double x : {inf, -inf, nan})
        for (size_t at = 0; at < 4; ++at) {
            double w[4] = {v[0], v[1], v[2], v[3]};
            w[at] = x;
            CHECK(!all_finite(w, 4) && all_finite(w, at));
        }
    std::puts("ok");
    return 0;
}
