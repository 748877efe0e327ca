// Host build of the device sampler (mvslam_amd/csrc/sampler.hpp: Philox4x32-10 + the 8-of-M draw) against the CPU oracle's
// orc_sample8, index by index and in order.  The header is plain C++ apart from __umulhi, which is defined here.
// Built and run by tests/test_sample8_host.py (once more with -fsanitize=address,undefined); exit code 0 = all equal.
#include <stdint.h>
#include <stdio.h>

#define MVS_DEV static inline
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }
#include "../../mvslam_amd/csrc/sampler.hpp"

extern "C" void orc_sample8(uint64_t seed, uint32_t hyp, int M, int sampler, int *idx);

int main()
{
    const int Ms[] = {8, 9, 10, 64, 1576, 4096, (1 << 24) - 1};
    const uint64_t seeds[] = {0ull, 0x5EED0000ull, 0xFEDCBA9876543210ull};
    long checked = 0, bad = 0;
    for (int M : Ms)
        for (uint64_t seed : seeds)
            for (uint32_t h = 0; h < 4096u; ++h) {
                int got[8], want[8];
                mvs::sample8(seed, h, M, 1, got);
                orc_sample8(seed, h, M, 1, want);
                bool same = true;
                for (int k = 0; k < 8; ++k) {
                    same = same && got[k] == want[k];
                    // distinct and in range, whatever the oracle says
                    same = same && got[k] >= 0 && got[k] < M;
                    for (int j = 0; j < k; ++j)
                        same = same && got[j] != got[k];
                }
                ++checked;
                if (!same && bad++ < 5)
                    printf("MISMATCH M=%d seed=%llx hyp=%u: got %d %d %d %d %d %d %d %d want %d %d %d %d %d %d %d %d\n", M,
                           (unsigned long long)seed, h, got[0], got[1], got[2], got[3], got[4], got[5], got[6], got[7], want[0],
                           want[1], want[2], want[3], want[4], want[5], want[6], want[7]);
            }
    // the identity sampler of the reference
    int id[8];
    mvs::sample8(1, 2, 100, 0, id);
    for (int k = 0; k < 8; ++k)
        bad += id[k] != k;
    printf("sample8 checked=%ld bad=%ld\n", checked, bad);
    return bad == 0 ? 0 : 1;
}
