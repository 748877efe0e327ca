// Stand-alone check of the argument rules of mvs_ctx_set_ba_loss (mvslam_amd/csrc/pg_host.hpp: ba_loss_args_ok).
// tests/test_ba_robust_host.py builds it with -fsanitize=address,undefined and runs it; it needs no GPU and loads nothing.
// Exit status 0 and "ok" on success.
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
    // the three losses, with a constant that is finite and positive
    for (int loss = 0; loss <= 2; ++loss)
        for (double k : {1.0, 1.345, 2.3849, 1e-300, 1e30, std::numeric_limits<double>::denorm_min(),
                         std::numeric_limits<double>::max()})
            CHECK(ba_loss_args_ok(loss, k));
    // no other loss
    for (int loss : {-1, 3, 7, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()})
        CHECK(!ba_loss_args_ok(loss, 1.0));
    // with a loss, k must be finite and > 0; without one it is not looked at
    for (double k : {0.0, -0.0, -1.0, -1e-300, nan, inf, -inf}) {
        CHECK(!ba_loss_args_ok(1, k));
        CHECK(!ba_loss_args_ok(2, k));
        CHECK(ba_loss_args_ok(0, k));
    }
    // the wrapper is the pose graphs' rule at first_edge = 0
    for (int loss = -1; loss <= 3; ++loss)
        for (double k : {-1.0, 0.0, 1.0, nan, inf})
            CHECK(ba_loss_args_ok(loss, k) == loss_args_ok(loss, k, 0));
    std::puts("ok");
    return 0;
}
