// seq_global_limits_check.cpp -- runs the host decisions of mvs_seq_refine_global (mvslam_amd/csrc/seq_global_host.hpp; DESIGN.md
// section 4.7.5) on the CPU: which track cuts are admitted, and what the device's counts mean for the limits of the sparse
// solver.  No capacity breach is reachable at test size on the device, so this program is where the limits are exercised.
// Built with the host sanitizers and run as a program of its own (tests/test_seq_global_host.py).
#include <cstdio>

#include "seq_global_host.hpp"

static int failures = 0;
#define CHECK(x)                                             \
    do {                                                     \
        if (!(x)) {                                          \
            std::printf("FAILED line %d: %s\n", __LINE__, #x); \
            ++failures;                                      \
        }                                                    \
    } while (0)

int main()
{
    using namespace mvs_seqg;
    CHECK(track_frames_ok(0) && track_frames_ok(2) && track_frames_ok(8) && track_frames_ok(4096));
    CHECK(!track_frames_ok(1) && !track_frames_ok(-1) && !track_frames_ok(4097) && !track_frames_ok(INT32_MIN));
    const int64_t one = 1;
    CHECK(counts_status(6, 300, 1000, 21, 900) == kFits);
    CHECK(counts_status(4096, one << 20, one << 23, one << 21, one << 28) == kFits);        // every limit is inclusive
    CHECK(counts_status(4097, 300, 1000, 21, 900) == kTooLarge);
    CHECK(counts_status(6, (one << 20) + 1, 1000, 21, 900) == kTooLarge);
    CHECK(counts_status(6, 300, (one << 23) + 1, 21, 900) == kTooLarge);
    CHECK(counts_status(6, 300, 1000, (one << 21) + 1, 900) == kTooLarge);
    CHECK(counts_status(6, 300, 1000, 21, (one << 28) + 1) == kTooLarge);
    CHECK(counts_status(6, 300, 1000, 21, one << 40) == kTooLarge);                          // the pair total is 64-bit
    CHECK(counts_status(6, 0, 0, 6, 0) == kNoPoints);
    CHECK(counts_status(4096, 0, 0, (one << 21) + 1, 0) == kTooLarge);                       // a breach outranks an empty problem
    if (failures)
        std::printf("failures %d\n", failures);
    else
        std::printf("ok\n");
    return failures ? 1 : 0;
}
