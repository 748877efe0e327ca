// Stand-alone check of the argument rules of mvs_ctx_set_pose_graph_loss (mvslam_amd/csrc/pg_host.hpp: loss_args_ok,
// loss_fits_host_graph).  tests/test_pg_robust_host.py builds it with -fsanitize=address,undefined and runs it; it needs no
// GPU and loads nothing.  Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "pg_host.hpp"

using namespace mvs_pg;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();
    // the three losses, with a constant that is finite and positive, from any first edge >= -1
    for (int loss = 0; loss <= 2; ++loss)
        for (int32_t first : {-1, 0, 1, 24, imax})
            for (double k : {1.0, 1.345, 1e-300, 1e30, std::numeric_limits<double>::denorm_min()})
                CHECK(loss_args_ok(loss, k, first));
    // no other loss
    for (int loss : {-1, 3, 7, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()})
        CHECK(!loss_args_ok(loss, 1.0, 0));
    // with a loss, k must be finite and > 0; without one it is not looked at
    for (double k : {0.0, -0.0, -1.0, nan, inf, -inf}) {
        CHECK(!loss_args_ok(1, k, 0));
        CHECK(!loss_args_ok(2, k, 0));
        CHECK(loss_args_ok(0, k, 0));
    }
    // first_edge < -1, under every loss
    for (int loss = 0; loss <= 2; ++loss)
        for (int32_t first : {-2, -3, imin})
            CHECK(!loss_args_ok(loss, 1.0, first));
    // a host graph has no loop edges for -1 to stand for; under "none" the value is not looked at
    CHECK(loss_fits_host_graph(0, -1) && loss_fits_host_graph(0, 0) && loss_fits_host_graph(0, 5));
    for (int loss = 1; loss <= 2; ++loss) {
        CHECK(!loss_fits_host_graph(loss, -1));
        CHECK(loss_fits_host_graph(loss, 0) && loss_fits_host_graph(loss, 40) && loss_fits_host_graph(loss, imax));
    }
    std::puts("ok");
    return 0;
}
