// join_check.cpp -- the index arithmetic of the union of PTO graphs (po_rrt_amd/csrc/porrt_join.hpp) against plain loops, on the
// host: random member sizes with zeros and single nodes, sizes whose products with B straddle the pass limit and 2^32, the pass
// cuts, the member of every union index at the segment boundaries, and the id translation there and back.  Built with the address
// and undefined-behaviour sanitizers by tests/test_plan_batch_cpu.py.
#include "../po_rrt_amd/csrc/porrt_join.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace porrt;

static int failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); if (++failures > 20) std::exit(1); } \
    } while (0)

// the member of index i by a walk over the members
static uint32_t member_by_loop(const std::vector<uint64_t> &off, uint64_t i) {
    for (uint32_t q = 0; q + 1 < off.size(); ++q)
        if (off[q] <= i && i < off[q + 1]) return q;
    return ~0u;
}

// the pass that starts at `first`, in 128-bit arithmetic
static uint32_t pass_end_by_loop(const std::vector<uint64_t> &nodes, const std::vector<uint64_t> &edges, uint32_t first, uint64_t B, uint64_t limit_in) {
    const unsigned __int128 limit = limit_in < kJoinBeliefNodesLimit ? limit_in : kJoinBeliefNodesLimit;
    unsigned __int128 bn = 0, ed = 0;
    uint32_t q = first;
    while (q < nodes.size()) {
        const unsigned __int128 bn2 = bn + (unsigned __int128)nodes[q] * B, ed2 = ed + edges[q];
        if (q > first && (bn2 > limit || ed2 > (unsigned __int128)kJoinEdgesLimit)) break;
        bn = bn2; ed = ed2;
        ++q;
    }
    return q;
}

static void check_members(const std::vector<uint64_t> &sizes, uint64_t B) {
    const uint32_t n = (uint32_t)sizes.size();
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t q = 0; q < n; ++q) off[q + 1] = off[q] + sizes[q];
    for (uint32_t q = 0; q < n; ++q) {
        if (!sizes[q]) continue;
        // the segment's first and last index, and their neighbours
        const uint64_t probe[4] = {off[q], off[q + 1] - 1, off[q] + (sizes[q] > 1 ? 1 : 0), off[q + 1] - (sizes[q] > 1 ? 2 : 1)};
        for (uint64_t i : probe) {
            CHECK(join_member_of(off.data(), n, i) == q);
            CHECK(member_by_loop(off, i) == q);
            // belief node ids: every belief of the node, there and back
            for (uint64_t b : {(uint64_t)0, B / 2, B - 1}) {
                const uint64_t own = (i - off[q]) * B + b, uni = join_union_id(off[q], B, own);
                CHECK(uni == i * B + b);
                CHECK(join_own_id(off[q], B, uni) == own);
                CHECK(join_member_of_belief_node(off.data(), n, B, uni) == q);
            }
        }
    }
    if (off[n] && off[n] <= 4096)
        for (uint64_t i = 0; i < off[n]; ++i) CHECK(join_member_of(off.data(), n, i) == member_by_loop(off, i));
}

static void check_passes(const std::vector<uint64_t> &nodes, const std::vector<uint64_t> &edges, uint64_t B, uint64_t limit) {
    const uint32_t n = (uint32_t)nodes.size();
    uint32_t passes = 0;
    for (uint32_t first = 0; first < n;) {
        const uint32_t end = join_pass_end(nodes.data(), edges.data(), n, first, B, limit);
        CHECK(end > first && end <= n);
        CHECK(end == pass_end_by_loop(nodes, edges, first, B, limit));
        // the rule itself: within the bounds unless the pass is one member; the next member would not have fitted
        unsigned __int128 bn = 0, ed = 0;
        for (uint32_t q = first; q < end; ++q) { bn += (unsigned __int128)nodes[q] * B; ed += edges[q]; }
        const unsigned __int128 lim = limit < kJoinBeliefNodesLimit ? limit : kJoinBeliefNodesLimit;
        if (end - first > 1) CHECK(bn <= lim && ed <= (unsigned __int128)kJoinEdgesLimit);
        if (end < n) CHECK(bn + (unsigned __int128)nodes[end] * B > lim || ed + edges[end] > (unsigned __int128)kJoinEdgesLimit);
        first = end;
        ++passes;
    }
    CHECK(passes >= 1 || n == 0);
}

int main() {
    std::mt19937_64 rng(20240607);
    CHECK(join_mul_sat(0, ~0ull) == 0 && join_mul_sat(~0ull, 2) == ~0ull && join_mul_sat(1ull << 32, 1ull << 31) == 1ull << 63);
    CHECK(join_mul_sat(1ull << 32, 1ull << 32) == ~0ull && join_add_sat(~0ull - 1, 1) == ~0ull && join_add_sat(~0ull, 5) == ~0ull && join_add_sat(3, 4) == 7);
    // members: zeros, single nodes, small and large sizes
    for (int trial = 0; trial < 400; ++trial) {
        const uint32_t n = 1 + (uint32_t)(rng() % 70);
        const uint64_t B = 1 + rng() % (trial % 3 ? 9 : 729);
        std::vector<uint64_t> sizes(n);
        for (uint64_t &s : sizes) {
            switch (rng() % 5) {
            case 0: s = 0; break;
            case 1: s = 1; break;
            case 2: s = 2 + rng() % 60; break;
            default: s = 1 + rng() % 20000; break;
            }
        }
        check_members(sizes, B);
        // one member only, and all members empty but one
        check_members({sizes[0] ? sizes[0] : 1}, B);
        std::vector<uint64_t> lone(n, 0);
        lone[rng() % n] = 1 + rng() % 5;
        check_members(lone, B);
    }
    {
        // many members: more than the search's low strides, offsets beyond 2^32
        std::vector<uint64_t> sizes(5000);
        for (uint64_t &s : sizes) s = rng() % 3 ? 1 + rng() % 3000000 : 0;
        check_members(sizes, 16);
        check_members(std::vector<uint64_t>(4097, 1), 3);
    }
    // passes: sums that straddle the limit and 2^32
    for (int trial = 0; trial < 2000; ++trial) {
        const uint32_t n = 1 + (uint32_t)(rng() % 40);
        const uint64_t B = 1 + rng() % (trial % 2 ? 16 : 729);
        std::vector<uint64_t> nodes(n), edges(n);
        const bool huge = trial % 5 == 0;
        for (uint32_t q = 0; q < n; ++q) {
            nodes[q] = huge ? (rng() % 4 ? 1 + rng() % (1ull << 29) : 1 + rng() % 100) : 1 + rng() % 20000;
            edges[q] = huge && rng() % 3 == 0 ? rng() % (1ull << 32) : nodes[q] * (rng() % 12);
        }
        uint64_t limit;
        switch (trial % 6) {
        case 0: limit = 1; break;
        case 1: limit = kJoinBeliefNodesDefault; break;
        case 2: limit = ~0ull; break;                                  // clamped to 2^32 - 2
        case 3: limit = nodes[0] * B; break;                           // member 0 fits exactly
        case 4: limit = nodes[0] * B + (n > 1 ? nodes[1] * B - 1 : 0); break;      // member 1 misses by one
        default: limit = 1 + rng() % (1ull << 33); break;
        }
        check_passes(nodes, edges, B, limit);
    }
    {
        // exactly at 2^32: a sum of 2^32 - 2 belief nodes is one pass, one more node cuts it
        const uint64_t B = 2;
        std::vector<uint64_t> nodes = {(1ull << 30), (1ull << 30) - 1, 1}, edges = {0, 0, 0};
        CHECK(join_pass_end(nodes.data(), edges.data(), 3, 0, B, ~0ull) == 2);
        nodes[1] -= 1;
        CHECK(join_pass_end(nodes.data(), edges.data(), 3, 0, B, ~0ull) == 3);
        // a member that alone exceeds every bound is a pass of its own, products beyond 64 bits included
        nodes = {1ull << 40, 5, 1ull << 63};
        CHECK(join_pass_end(nodes.data(), edges.data(), 3, 0, 1ull << 30, ~0ull) == 1);
        CHECK(join_pass_end(nodes.data(), edges.data(), 3, 1, 1ull << 30, ~0ull) == 2);
        CHECK(join_pass_end(nodes.data(), edges.data(), 3, 2, 1ull << 30, ~0ull) == 3);
        // the edge bound
        nodes = {10, 10, 10}; edges = {1ull << 31, (1ull << 31) - 1, 1};
        CHECK(join_pass_end(nodes.data(), edges.data(), 3, 0, 1, 1ull << 27) == 2);
        edges[2] = 0;
        CHECK(join_pass_end(nodes.data(), edges.data(), 3, 0, 1, 1ull << 27) == 3);
    }
    if (failures) { std::printf("join_check: %d failures\n", failures); return 1; }
    std::printf("join_check ok\n");
    return 0;
}
