// sampler.hpp -- Philox4x32-10 and the 8-of-M sampler of the RANSAC kernels (included by device_math.hpp).
//
// Integer code only, and plain C++ apart from __umulhi: a host translation unit that defines MVS_DEV and __umulhi before
// including this file gets the same functions (tests/cpp/sample8_host.cpp compares them with the CPU oracle's sampler for
// every draw).  The sample stream is contract.
#pragma once
#include <stdint.h>
#ifndef MVS_DEV
#include <hip/hip_runtime.h>
#define MVS_DEV __device__ __forceinline__
#endif

namespace mvs {

// ---------------------------------------------------------------------------------
// Philox4x32-10 and the 8-of-M sampler
// ---------------------------------------------------------------------------------
MVS_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                           uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // one 64-bit product each (v_mad_u64_u32) instead of a high and a low 32-bit multiply: full-width integer multiplies
        // issue at a quarter of the vector rate, and the two Philox calls of a sample were 80 of them
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

MVS_DEV uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
MVS_DEV uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
// median of three, in the form the backend selects v_med3_u32 for
MVS_DEV uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) { return umax32(umin32(a, b), umin32(umax32(a, b), c)); }

// idx[k]: k-th draw = slot (w_k * (M - k)) >> 32 among the not yet chosen indices.
MVS_DEV void sample8(uint64_t seed, uint32_t hyp, int M, int sampler, int (&idx)[8])
{
    if (sampler == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            idx[k] = k;
        return;
    }
    uint32_t w[8];
    {
        uint32_t o[4];
        philox4x32_10(hyp, 0u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
        w[0] = o[0]; w[1] = o[1]; w[2] = o[2]; w[3] = o[3];
        philox4x32_10(hyp, 1u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
        w[4] = o[0]; w[5] = o[1]; w[6] = o[2]; w[7] = o[3];
    }
    // sorted[0 .. k): the k indices drawn so far, ascending and distinct, with static indices only.  Every loop runs over
    // that live prefix alone (no sentinels, so no compare or select for slots not yet filled)
    uint32_t sorted[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // slot -> index: step over every earlier index at or below the running value (ascending order: the walk of the
        // prefix IS the correction)
        uint32_t r = __umulhi(w[k], (uint32_t)(M - k));
#pragma unroll
        for (int t = 0; t < k; ++t)
            r += r >= sorted[t] ? 1u : 0u;
        idx[k] = (int)r;
        // insert r (distinct from all of sorted[0 .. k)): the new entry t is the median of its old neighbours t - 1, t and r
        // -- one operation per slot where a compare-and-swap chain takes two; the last draw is not inserted
        if (k < 7) {
            if (k > 0)
                sorted[k] = umax32(sorted[k - 1], r);
#pragma unroll
            for (int t = k - 1; t > 0; --t)
                sorted[t] = umed3(sorted[t - 1], sorted[t], r);
            sorted[0] = k > 0 ? umin32(sorted[0], r) : r;
        }
    }
}

}  // namespace mvs
