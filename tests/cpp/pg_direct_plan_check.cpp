// pg_direct_plan_check.cpp -- mvs_pgm::direct_plan of mvslam_amd/csrc/pg_envelope.hpp (the host planning of the direct LM step,
// DESIGN.md section 4.10.4) against a brute-force restatement, built with the host sanitizers and run as a program of its own
// by tests/test_pg_direct_host.py.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "pg_envelope.hpp"

#define REQUIRE(x)                                                  \
    do {                                                            \
        if (!(x)) {                                                 \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); \
            return 1;                                               \
        }                                                           \
    } while (0)

static int check(int n, const std::vector<int32_t> &src, const std::vector<int32_t> &dst, int anchor, int64_t want_blocks, int want_widest)
{
    const int e = (int)src.size();
    std::vector<int32_t> first, row_off;
    const int64_t blocks = mvs_pgm::envelope(n, e, src.data(), dst.data(), first, row_off);
    REQUIRE(blocks == want_blocks);
    if (blocks > mvs_pgm::kMaxEnvelopeBlocks) {
        REQUIRE(first.empty() && row_off.empty());   // nothing is planned for a graph that is refused
        return 0;
    }
    const mvs_pgm::BlockLists lists = mvs_pgm::block_lists(e, anchor, src.data(), dst.data(), first, row_off);
    const mvs_pgm::DirectPlan plan = mvs_pgm::direct_plan(n, first, row_off, lists);
    REQUIRE((int64_t)plan.blk_row.size() == blocks && (int64_t)plan.blk_slot.size() == blocks);
    REQUIRE(plan.widest == want_widest);
    // brute force: the blocks some term touches
    std::map<std::pair<int, int>, int> touched;
    for (int k = 0; k < e; ++k) {
        touched[{src[k], src[k]}]++;
        touched[{dst[k], dst[k]}]++;
        touched[{std::max(src[k], dst[k]), std::min(src[k], dst[k])}]++;
    }
    touched[{anchor, anchor}]++;
    int64_t b = 0, n_touched = 0;
    for (int i = 0; i < n; ++i) {
        REQUIRE(first[i] <= i && row_off[i] == b);
        for (int c = first[i]; c <= i; ++c, ++b) {
            REQUIRE(plan.blk_row[b] == i);
            const auto it = touched.find({i, c});
            const int slot = plan.blk_slot[b];
            if (it == touched.end()) {
                REQUIRE(slot == -1);
                continue;
            }
            ++n_touched;
            REQUIRE(slot >= 0 && slot < (int)lists.slot_blk.size() && lists.slot_blk[slot] == b);
            REQUIRE(lists.slot_off[slot + 1] - lists.slot_off[slot] == it->second);   // every term of the block, once
        }
    }
    REQUIRE(b == blocks && n_touched == (int64_t)lists.slot_blk.size() && n_touched == (int64_t)touched.size());
    return 0;
}

int main()
{
    // one node, no edge
    if (check(1, {}, {}, 0, 1, 1))
        return 1;
    // a chain with a chord and a closure, parallel edges in both orientations, the anchor in the middle
    if (check(6, {0, 1, 2, 3, 4, 2, 1, 5, 0}, {1, 2, 3, 4, 5, 1, 2, 0, 5}, 3, 1 + 2 + 2 + 2 + 2 + 6, 6))
        return 1;
    // a hub at the last node: every row but the last is one block wide, nothing fills
    {
        std::vector<int32_t> s, d;
        for (int i = 0; i < 39; ++i) {
            s.push_back(39);
            d.push_back(i);
        }
        if (check(40, s, d, 39, 39 + 40, 40))
            return 1;
    }
    // a hub at node 0: the full lower triangle; the 4096-node one is refused and nothing is planned
    for (int n : {70, 2047, 4096}) {
        std::vector<int32_t> s, d;
        for (int i = 1; i < n; ++i) {
            s.push_back(i % 2 ? 0 : i);
            d.push_back(i % 2 ? i : 0);
        }
        if (check(n, s, d, 0, (int64_t)n * (n + 1) / 2, n))
            return 1;
    }
    std::printf("ok\n");
    return 0;
}
