// ba_envelope.hpp -- the host side of the sparse bundle adjustment (ba_sparse.hip), the sibling of
// pg_envelope.hpp: the block skyline of the reduced camera system, the observations of every frame, and for every block of
// the envelope the pairs of observations whose product it sums.  Plain C++ with no HIP in it, so that
// tests/cpp/ba_envelope_dump.cpp can run it on the CPU (and under the host sanitizers).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pg_envelope.hpp"

namespace mvs_bas {

constexpr int kMaxFrames = 4096;
constexpr int kMaxPoints = 1 << 20;
constexpr int kMaxObs = 1 << 23;
constexpr int64_t kMaxPairs = int64_t(1) << 28;   // 2 GiB of index lists

// 0: fine.  1: obs_off is not monotone from 0 to n_obs.  2: obs_frame out of range or not strictly ascending within a point.
inline int check_csr(int n_frames, int n_points, int n_obs, const int32_t *obs_off, const int32_t *obs_frame)
{
    if (obs_off[0] != 0 || obs_off[n_points] != n_obs)
        return 1;
    for (int p = 0; p < n_points; ++p)
        if (obs_off[p + 1] < obs_off[p] || obs_off[p + 1] > n_obs)
            return 1;
    for (int p = 0; p < n_points; ++p)
        for (int32_t o = obs_off[p]; o < obs_off[p + 1]; ++o) {
            if (obs_frame[o] < 0 || obs_frame[o] >= n_frames)
                return 2;
            if (o > obs_off[p] && obs_frame[o] <= obs_frame[o - 1])
                return 2;
        }
    return 0;
}

struct Plan {
    int64_t blocks = 0;                      // of the envelope; beyond mvs_pgm::kMaxEnvelopeBlocks nothing else is filled
    int64_t pairs = 0;                       // of observations, summed over all points; beyond kMaxPairs the lists are not filled
    int widest = 0;                          // the widest row in blocks
    std::vector<int32_t> first, row_off;     // as mvs_pgm::envelope
    std::vector<int32_t> blk_row;            // [blocks] the row of every block
    std::vector<int32_t> last;               // [F] the last row whose envelope reaches column j (>= j)
    std::vector<int32_t> obs_point;          // [n_obs]
    std::vector<int32_t> fr_off, fr_obs;     // [F + 1], [n_obs]: the observations of every frame in ascending index
    // block b (row i > column j) sums Z_a Z_c^T over pair_a / pair_c [pair_off[b] .. pair_off[b + 1]): a an observation of
    // frame i, c the observation of frame j of the same point, in point order.  A diagonal block has no pairs: its sum runs
    // over fr_obs.
    std::vector<int32_t> pair_off, pair_a, pair_c;
    bool fits() const { return blocks <= mvs_pgm::kMaxEnvelopeBlocks && pairs <= kMaxPairs; }
};

// The input has passed check_csr.  first[i] = the smallest frame that shares a point with frame i: the first observation of
// the points frame i sees (a point's frames ascend).
inline Plan plan(int n_frames, int n_points, int n_obs, const int32_t *obs_off, const int32_t *obs_frame)
{
    Plan P;
    const size_t F = (size_t)n_frames;
    std::vector<int32_t> f(F);
    for (int i = 0; i < n_frames; ++i)
        f[(size_t)i] = i;
    for (int p = 0; p < n_points; ++p) {
        const int32_t b = obs_off[p], e = obs_off[p + 1];
        if (e - b < 2)
            continue;
        const int32_t lo = obs_frame[b];
        for (int32_t o = b + 1; o < e; ++o)
            f[(size_t)obs_frame[o]] = std::min(f[(size_t)obs_frame[o]], lo);
        P.pairs += (int64_t)(e - b) * (e - b - 1) / 2;
    }
    for (int i = 0; i < n_frames; ++i)
        P.blocks += (int64_t)i - f[(size_t)i] + 1;
    if (!P.fits())
        return P;
    P.first.swap(f);
    P.row_off.assign(F + 1, 0);
    for (int i = 0; i < n_frames; ++i) {
        const int w = i - P.first[(size_t)i] + 1;
        P.row_off[(size_t)i + 1] = P.row_off[(size_t)i] + w;
        P.widest = std::max(P.widest, w);
    }
    P.blk_row.resize((size_t)P.blocks);
    P.last.resize(F);
    for (int i = 0; i < n_frames; ++i) {
        for (int32_t b = P.row_off[(size_t)i]; b < P.row_off[(size_t)i + 1]; ++b)
            P.blk_row[(size_t)b] = i;
        for (int j = P.first[(size_t)i]; j <= i; ++j)
            P.last[(size_t)j] = i;   // rows ascend: the last writer is the largest
    }
    // observations by frame (counting sort: ascending index inside a frame)
    P.obs_point.resize((size_t)n_obs);
    P.fr_off.assign(F + 1, 0);
    for (int p = 0; p < n_points; ++p)
        for (int32_t o = obs_off[p]; o < obs_off[p + 1]; ++o) {
            P.obs_point[(size_t)o] = p;
            ++P.fr_off[(size_t)obs_frame[o] + 1];
        }
    for (size_t i = 0; i < F; ++i)
        P.fr_off[i + 1] += P.fr_off[i];
    P.fr_obs.resize((size_t)n_obs);
    {
        std::vector<int32_t> at(P.fr_off.begin(), P.fr_off.end() - 1);
        for (int32_t o = 0; o < n_obs; ++o)
            P.fr_obs[(size_t)at[(size_t)obs_frame[o]]++] = o;
    }
    // pairs by block (counting sort over the points in order: point order inside a block)
    auto blk = [&](int32_t r, int32_t c) { return (size_t)(P.row_off[(size_t)r] + (c - P.first[(size_t)r])); };
    P.pair_off.assign((size_t)P.blocks + 1, 0);
    for (int p = 0; p < n_points; ++p)
        for (int32_t a = obs_off[p] + 1; a < obs_off[p + 1]; ++a)
            for (int32_t c = obs_off[p]; c < a; ++c)
                ++P.pair_off[blk(obs_frame[a], obs_frame[c]) + 1];
    for (size_t b = 0; b < (size_t)P.blocks; ++b)
        P.pair_off[b + 1] += P.pair_off[b];
    P.pair_a.resize((size_t)P.pairs);
    P.pair_c.resize((size_t)P.pairs);
    {
        std::vector<int32_t> at(P.pair_off.begin(), P.pair_off.end() - 1);
        for (int p = 0; p < n_points; ++p)
            for (int32_t a = obs_off[p] + 1; a < obs_off[p + 1]; ++a)
                for (int32_t c = obs_off[p]; c < a; ++c) {
                    const size_t k = (size_t)at[blk(obs_frame[a], obs_frame[c])]++;
                    P.pair_a[k] = a;
                    P.pair_c[k] = c;
                }
    }
    return P;
}

}  // namespace mvs_bas
