// pg_envelope.hpp -- the host side of the pose-graph marginals (pg_marginals.hip) and of the direct
// LM step (pg_direct.hip; section 4.10.4): the block skyline of H, the per-block edge lists of its assembly, the blocks' rows
// and slots, and the chunking of the queries.  Plain C++ with no HIP in it, so that tests/cpp/pg_envelope_check.cpp and
// tests/cpp/pg_direct_plan_check.cpp can run it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace mvs_pgm {

constexpr int64_t kMaxEnvelopeBlocks = int64_t(1) << 21;   // 604 MB of 288-byte blocks
constexpr int kYCols = 12;                                 // columns of one query's solve: 6 per node, two nodes
constexpr size_t kYBudgetBytes = size_t(256) << 20;        // bound of the solves' y workspace
constexpr int kMaxChunk = 4096;                            // queries of one launch at most (bounds the output staging)

// Nodes in their natural order; first[i] = the smallest of i and its neighbours; row i of the block lower triangle stores
// the blocks first[i] .. i, block (i, c) at row_off[i] + (c - first[i]).  Returns the number of blocks; first and row_off
// (n_nodes + 1 entries, the last one the total) are filled only when the count is within kMaxEnvelopeBlocks.
inline int64_t envelope(int n_nodes, int n_edges, const int32_t *src, const int32_t *dst, std::vector<int32_t> &first,
                        std::vector<int32_t> &row_off)
{
    std::vector<int32_t> f((size_t)n_nodes);
    for (int i = 0; i < n_nodes; ++i)
        f[(size_t)i] = i;
    for (int k = 0; k < n_edges; ++k) {
        const int32_t lo = std::min(src[k], dst[k]), hi = std::max(src[k], dst[k]);
        f[(size_t)hi] = std::min(f[(size_t)hi], lo);
    }
    int64_t total = 0;
    for (int i = 0; i < n_nodes; ++i)
        total += (int64_t)i - f[(size_t)i] + 1;
    if (total > kMaxEnvelopeBlocks)
        return total;
    row_off.assign((size_t)n_nodes + 1, 0);
    for (int i = 0; i < n_nodes; ++i)
        row_off[(size_t)i + 1] = row_off[(size_t)i] + (i - f[(size_t)i] + 1);
    first.swap(f);
    return total;
}

// The blocks of H that some term touches, each with its terms in edge order: slot s is block slot_blk[s] (an index into the
// skyline) and sums codes[slot_off[s] .. slot_off[s + 1]).  A code is 4 * edge + kind for the edge's product
//   kind 0: A_src^T A_src (diagonal block of src)      kind 2: A_src^T A_dst (src is the row: src > dst)
//   kind 1: A_dst^T A_dst (diagonal block of dst)      kind 3: A_dst^T A_src (dst is the row)
// and -1 for the anchor prior, the last term of the anchor's diagonal block.
struct BlockLists {
    std::vector<int32_t> slot_blk, slot_off, codes;
};
inline BlockLists block_lists(int n_edges, int anchor, const int32_t *src, const int32_t *dst, const std::vector<int32_t> &first,
                              const std::vector<int32_t> &row_off)
{
    auto blk = [&](int32_t r, int32_t c) { return row_off[(size_t)r] + (c - first[(size_t)r]); };
    std::vector<std::pair<int32_t, int32_t>> terms;
    terms.reserve(3 * (size_t)n_edges + 1);
    for (int k = 0; k < n_edges; ++k) {
        const int32_t s = src[k], d = dst[k];
        terms.emplace_back(blk(s, s), 4 * k);
        terms.emplace_back(blk(d, d), 4 * k + 1);
        terms.emplace_back(s > d ? blk(s, d) : blk(d, s), 4 * k + (s > d ? 2 : 3));
    }
    terms.emplace_back(blk(anchor, anchor), -1);
    std::stable_sort(terms.begin(), terms.end(),
                     [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) { return a.first < b.first; });
    BlockLists out;
    out.codes.reserve(terms.size());
    for (size_t t = 0; t < terms.size(); ++t) {
        if (t == 0 || terms[t].first != terms[t - 1].first) {
            out.slot_blk.push_back(terms[t].first);
            out.slot_off.push_back((int32_t)t);
        }
        out.codes.push_back(terms[t].second);
    }
    out.slot_off.push_back((int32_t)terms.size());
    return out;
}

// What the direct LM step (pg_direct.hip) needs of the envelope beyond the above: for every block
// its row (its column is first[row] + its place in the row) and its slot in `lists`, -1 for a block no term touches (fill
// only); the widest row in blocks.
struct DirectPlan {
    std::vector<int32_t> blk_row, blk_slot;
    int widest = 0;
};
inline DirectPlan direct_plan(int n_nodes, const std::vector<int32_t> &first, const std::vector<int32_t> &row_off, const BlockLists &lists)
{
    DirectPlan out;
    const size_t blocks = n_nodes > 0 ? (size_t)row_off[(size_t)n_nodes] : 0;
    out.blk_row.resize(blocks);
    out.blk_slot.assign(blocks, -1);
    for (int i = 0; i < n_nodes; ++i) {
        out.widest = std::max(out.widest, i - first[(size_t)i] + 1);
        for (int32_t b = row_off[(size_t)i]; b < row_off[(size_t)i + 1]; ++b)
            out.blk_row[(size_t)b] = i;
    }
    for (size_t s = 0; s < lists.slot_blk.size(); ++s)
        out.blk_slot[(size_t)lists.slot_blk[s]] = (int32_t)s;
    return out;
}

// queries of one launch: each owns n_nodes * 6 * kYCols doubles of y, the chunk's y stays within kYBudgetBytes (one query is
// always admitted: 2.4 MB at 4096 nodes)
inline int query_chunk(int n_nodes)
{
    const size_t per = (size_t)n_nodes * 6 * kYCols * sizeof(double);
    return (int)std::min<size_t>((size_t)kMaxChunk, std::max<size_t>(1, kYBudgetBytes / per));
}

// the query list of a call: the caller's, or every diagonal block when n_query = 0 and both lists are null.  False for a
// list that is missing or an index out of range.
inline bool expand_queries(int n_nodes, int n_query, const int32_t *qi, const int32_t *qj, std::vector<int32_t> &out_i,
                           std::vector<int32_t> &out_j)
{
    out_i.clear();
    out_j.clear();
    if (n_query == 0 && !qi && !qj) {
        for (int i = 0; i < n_nodes; ++i) {
            out_i.push_back(i);
            out_j.push_back(i);
        }
        return true;
    }
    if (n_query < 1 || !qi || !qj)
        return false;
    for (int k = 0; k < n_query; ++k) {
        if (qi[k] < 0 || qi[k] >= n_nodes || qj[k] < 0 || qj[k] >= n_nodes)
            return false;
        out_i.push_back(qi[k]);
        out_j.push_back(qj[k]);
    }
    return true;
}

}  // namespace mvs_pgm
