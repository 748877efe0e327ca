// match_fp4.hpp -- what the two matrix-core Hamming kernels share: match_mfma_kernel (kernels.hip, one image pair per
// workgroup column) and loop_scores_mfma_kernel (loop.hip, one query block against a run of base frames).  The constants of
// the FP4 key, the bit -> e2m1 unpack and the top-2 insertion; the exactness argument stands above match_mfma_kernel.
#pragma once
#include "kernels.hpp"

namespace mvs {

constexpr int kMmBlocks = 2;                         // 32-query blocks per wavefront: every A fragment read feeds kMmBlocks chains
constexpr int kMmQueries = 256;                      // queries per workgroup
constexpr int kMmThreads = 64 * kMmQueries / (32 * kMmBlocks);
constexpr int kMmRowBytes = 128 + 16;                // unpacked row of a train tile (256 nibbles), padded: a ds_read_b128 of 16
                                                     // rows at a 36-dword stride covers all 64 banks once
constexpr int kMmKeyShift = 12;                      // key = distance field << 12 | train index: one product is -(2 << 12)
constexpr int kMmKeyBias = 257;                      // distance field = |t| + 257 - 2 dot >= 1
constexpr uint32_t kMmKeyNone = 0x4b800000u;         // 2^24 as a float: the key of no row
constexpr int kMmScaleTrain = 127 + 13, kMmScaleQuery = 127;   // E8M0 block scales: 2^13 and 2^0
static_assert(kMaxKp <= (1 << kMmKeyShift), "the train index must fit below the distance field of a match_mfma key");
static_assert((kMmKeyBias + 256 + 1) << kMmKeyShift <= (1 << 22), "match_mfma keys must stay exact binary32 integers");
static_assert(kMmThreads <= 256 && 256 % kMmThreads == 0, "the staging maps 32 rows x 8 dwords onto the workgroup");
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// 32 bits -> 32 e2m1 nibbles, each 0 or +1.0 (0b0010): output dword j holds byte j, nibble 2 i = bit 8 j + i, nibble 2 i + 1 =
// bit 8 j + 4 + i.  A nibble times 0x00408102 (= 2 x 0x00204081) has bit i of the nibble at positions i + 7 k + 1 (k = 0..3: no
// two terms meet, no carries); the mask keeps bit 1 of every byte, and the high nibble's bits go four above the low one's.  The
// product is a 4-bit by 23-bit one: v_mul_u32_u24 (full rate; v_mul_lo_u32 issues at a quarter of it).  The merge is inline
// asm: hipcc otherwise folds the high nibble's shift into its multiplier (0x04081020, past 24 bits: v_mul_lo_u32).
__device__ __forceinline__ uint32_t lshl4_or(uint32_t hi, uint32_t lo)
{
    uint32_t r;
    asm("v_lshl_or_b32 %0, %1, 4, %2" : "=v"(r) : "v"(hi), "v"(lo));
    return r;
}
__device__ __forceinline__ v4i unpack32_fp4(uint32_t bits)
{
    v4i r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t lo = __umul24((bits >> (8 * j)) & 0xfu, 0x00408102u) & 0x02020202u;
        const uint32_t hi = __umul24((bits >> (8 * j + 4)) & 0xfu, 0x00408102u) & 0x02020202u;
        r[j] = (int)lshl4_or(hi, lo);
    }
    return r;
}

// The matrix-core kernels read their accumulators with compiler-visible min / max only (hipcc forms v_min3_u32 itself): the
// hazard recognizer inserts no wait states in front of inline asm, and an inline-asm v_med3_u32 straight after the last MFMA
// of a chain read accumulator registers the matrix core had not finished writing (nondeterministic lists).
__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) { return min(min(a, b), c); }
__device__ __forceinline__ void key_insert_mm(uint32_t &k0, uint32_t &k1, uint32_t k)
{
    k1 = min(k1, max(k0, k));
    k0 = min(k0, k);
}

// The cap of the CAPPED kernels: the smallest integer distance C with ratio * C > max_dist, evaluated exactly as the kernels
// evaluate the ratio test (float distance -> double); -1 when the call has no distance limit (max_dist < 0), no usable
// ratio, or a limit so wide that random rows would reach it (Hamming distances of unrelated 256-bit descriptors are 128 +- 8).
inline int match_cap_distance(double ratio, double max_dist)
{
    if (!(max_dist >= 0.0) || !(ratio > 0.0))
        return -1;
    for (int c = 0; c <= 96; ++c)
        if (ratio * (double)(float)c > max_dist)
            return c;
    return -1;
}

}  // namespace mvs
