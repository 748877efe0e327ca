// Stand-alone check of the host side of the pose-graph marginals (mvslam_amd/csrc/pg_envelope.hpp): the envelope, the per-block
// term lists and the query chunking.  tests/test_pg_marginals_host.py builds it with -fsanitize=address,undefined and runs it;
// it needs no GPU and loads nothing.  Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_envelope.hpp"

using namespace mvs_pgm;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// every term of every edge sits in exactly one slot, inside the envelope, in edge order; the anchor's closes its block
static void check_lists(int N, int anchor, const std::vector<int32_t> &src, const std::vector<int32_t> &dst)
{
    const int E = (int)src.size();
    std::vector<int32_t> first, row_off;
    const int64_t blocks = envelope(N, E, src.data(), dst.data(), first, row_off);
    CHECK(blocks <= kMaxEnvelopeBlocks && (int)first.size() == N && (int)row_off.size() == N + 1 && row_off[(size_t)N] == blocks);
    for (int i = 0; i < N; ++i)
        CHECK(first[(size_t)i] >= 0 && first[(size_t)i] <= i);
    const BlockLists L = block_lists(E, anchor, src.data(), dst.data(), first, row_off);
    CHECK(L.slot_off.size() == L.slot_blk.size() + 1 && (size_t)L.slot_off.back() == L.codes.size());
    CHECK(L.codes.size() == 3 * (size_t)E + 1);
    std::vector<int> seen(4 * (size_t)E, 0);
    int anchors = 0;
    for (size_t s = 0; s < L.slot_blk.size(); ++s) {
        CHECK(L.slot_blk[s] >= 0 && L.slot_blk[s] < blocks);
        CHECK(s == 0 || L.slot_blk[s] > L.slot_blk[s - 1]);
        CHECK(L.slot_off[s] < L.slot_off[s + 1]);
        for (int c = L.slot_off[s]; c < L.slot_off[s + 1]; ++c) {
            const int code = L.codes[(size_t)c];
            if (code < 0) {
                CHECK(c == L.slot_off[s + 1] - 1 && L.slot_blk[s] == row_off[(size_t)anchor] + anchor - first[(size_t)anchor]);
                ++anchors;
                continue;
            }
            CHECK(code < 4 * E);
            CHECK(c == L.slot_off[s] || L.codes[(size_t)c - 1] < code);   // edge order inside a block
            const int k = code >> 2, kind = code & 3, a = src[(size_t)k], b = dst[(size_t)k];
            const int r = kind == 0 ? a : kind == 1 ? b : kind == 2 ? a : b;
            const int cl = kind == 0 ? a : kind == 1 ? b : kind == 2 ? b : a;
            CHECK(r >= cl && cl >= first[(size_t)r]);
            CHECK(L.slot_blk[s] == row_off[(size_t)r] + cl - first[(size_t)r]);
            ++seen[(size_t)code];
        }
    }
    CHECK(anchors == 1);
    for (int k = 0; k < E; ++k) {
        CHECK(seen[4 * (size_t)k] == 1 && seen[4 * (size_t)k + 1] == 1);
        CHECK(seen[4 * (size_t)k + 2] + seen[4 * (size_t)k + 3] == 1);
    }
}

int main()
{
    std::vector<int32_t> first, row_off, qi, qj;
    // N = 1: one block, the anchor's term alone
    CHECK(envelope(1, 0, nullptr, nullptr, first, row_off) == 1 && first[0] == 0 && row_off[1] == 1);
    check_lists(1, 0, {}, {});
    // a chain: 2 N - 1 blocks
    {
        std::vector<int32_t> s, d;
        for (int i = 0; i + 1 < 9; ++i)
            s.push_back(i % 2 ? i + 1 : i), d.push_back(i % 2 ? i : i + 1);   // both directions
        CHECK(envelope(9, 8, s.data(), d.data(), first, row_off) == 17);
        check_lists(9, 4, s, d);
    }
    // the star: every node joined to node 0, N (N + 1) / 2 blocks, with a parallel edge
    {
        const int N = 71;
        std::vector<int32_t> s, d;
        for (int i = 1; i < N; ++i)
            s.push_back(i % 2 ? 0 : i), d.push_back(i % 2 ? i : 0);
        s.push_back(0), d.push_back(5);
        CHECK(envelope(N, (int)s.size(), s.data(), d.data(), first, row_off) == N * (N + 1) / 2);
        check_lists(N, 0, s, d);
    }
    // 4096 nodes on one hub: over the capacity, nothing filled in
    {
        const int N = 4096;
        std::vector<int32_t> s((size_t)N - 1, 0), d;
        for (int i = 1; i < N; ++i)
            d.push_back(i);
        first.clear(), row_off.clear();
        CHECK(envelope(N, N - 1, s.data(), d.data(), first, row_off) == (int64_t)N * (N + 1) / 2);
        CHECK((int64_t)N * (N + 1) / 2 > kMaxEnvelopeBlocks && first.empty() && row_off.empty());
    }
    // queries: a list of length 0 is every diagonal block; out-of-range indices and missing lists are refused
    CHECK(expand_queries(5, 0, nullptr, nullptr, qi, qj) && qi.size() == 5 && qj[4] == 4 && qi[4] == 4);
    {
        const int32_t a[3] = {0, 4, 2}, b[3] = {4, 4, 0}, bad_lo[1] = {-1}, bad_hi[1] = {5}, zero[1] = {0};
        CHECK(expand_queries(5, 3, a, b, qi, qj) && qi.size() == 3 && qi[1] == 4 && qj[2] == 0);
        CHECK(!expand_queries(5, 1, bad_lo, zero, qi, qj) && !expand_queries(5, 1, zero, bad_hi, qi, qj));
        CHECK(!expand_queries(5, 1, nullptr, zero, qi, qj) && !expand_queries(5, 0, a, nullptr, qi, qj));
        CHECK(!expand_queries(5, -1, a, b, qi, qj));
    }
    // chunks: the y workspace of a chunk stays within its bound, and a list one longer than a chunk takes a second launch
    for (int N : {1, 2, 70, 1000, 4096}) {
        const int chunk = query_chunk(N);
        CHECK(chunk >= 1 && chunk <= kMaxChunk);
        CHECK(chunk == 1 || (size_t)chunk * (size_t)N * 6 * kYCols * sizeof(double) <= kYBudgetBytes);
        const int nq = chunk + 1;
        int launches = 0, covered = 0;
        for (int off = 0; off < nq; off += chunk) {
            const int n = std::min(chunk, nq - off);
            CHECK(n >= 1 && n <= chunk);
            covered += n;
            ++launches;
        }
        CHECK(launches == 2 && covered == nq);
    }
    CHECK(query_chunk(4096) == 113);
    std::puts("ok");
    return 0;
}
