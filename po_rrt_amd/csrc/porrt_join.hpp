// porrt_join.hpp -- index arithmetic of the disjoint union of several PTO graphs (porrt_plan_batch.hpp).
//
// porrt_plan_belief_space_batch lays the members of a pass end to end: member q's node j is union node off[q] + j, its edge e is
// union edge eoff[q] + e, and its belief node id (node * B + belief) is union id off[q] * B + id.  What is in here is plain integer
// arithmetic, the same for the gather kernels and for a host program that checks it against loops (tests/join_check.cpp); nothing in
// it touches memory other than the arrays it is handed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PORRT_JOIN_HD __host__ __device__ inline
#else
#define PORRT_JOIN_HD inline
#endif

namespace porrt {

// option "plan_batch_max_belief_nodes".  Measured, not reasoned: on the recorded problem (map_4, 30 members of about a million belief
// nodes each) passes of four members took 307 ms, of one 530, of eight 354, all thirty in one 462; the difference is in the cost
// sweeps (a level of the union is swept until its slowest member's costs stand, and the sweep kernel is chosen by the union's rows).
constexpr uint64_t kJoinBeliefNodesDefault = 1ull << 22;
// A belief graph holds fewer than 2^32 - 1 belief nodes (its lists store ids in 32 bits, and porrt_build_belief_graph refuses
// N * B >= 2^32 - 1), a PTO graph fewer than 2^32 edges (the edge order numbers them in 32 bits): a pass never holds more.
constexpr uint64_t kJoinBeliefNodesLimit = 0xFFFFFFFEull;
constexpr uint64_t kJoinEdgesLimit = 0xFFFFFFFFull;

// a * b, or 2^64 - 1 where the product does not fit
PORRT_JOIN_HD uint64_t join_mul_sat(uint64_t a, uint64_t b) {
    if (a == 0 || b == 0) return 0;
    return a > ~0ull / b ? ~0ull : a * b;
}
PORRT_JOIN_HD uint64_t join_add_sat(uint64_t a, uint64_t b) { return a > ~0ull - b ? ~0ull : a + b; }

// The pass that starts at member `first` (< n) ends before the member this returns (> first): members are taken in order while the
// belief nodes of the pass, the sum of nodes[q] * B, stay at or below max_belief_nodes (clamped to kJoinBeliefNodesLimit) and its
// edges at or below kJoinEdgesLimit.  A member that alone exceeds a bound is a pass of its own: the stages that follow accept or
// refuse it exactly as they do for a single context.
PORRT_JOIN_HD uint32_t join_pass_end(const uint64_t *nodes, const uint64_t *edges, uint32_t n, uint32_t first, uint64_t B, uint64_t max_belief_nodes) {
    const uint64_t limit = max_belief_nodes < kJoinBeliefNodesLimit ? max_belief_nodes : kJoinBeliefNodesLimit;
    uint64_t bn = 0, ed = 0;
    uint32_t q = first;
    for (; q < n; ++q) {
        bn = join_add_sat(bn, join_mul_sat(nodes[q], B));
        ed = join_add_sat(ed, edges[q]);
        if ((bn > limit || ed > kJoinEdgesLimit) && q > first) break;
    }
    return q;
}

// Member of union index i < off[n]: the largest q < n with off[q] <= i (off: n + 1 ascending entries, off[0] = 0).  Members without
// entries are stepped over: their offset equals their successor's.  32 trips whatever n and the sizes are.
PORRT_JOIN_HD uint32_t join_member_of(const uint64_t *off, uint32_t n, uint64_t i) {
    uint32_t q = 0;
    for (uint32_t step = 0x80000000u; step >= 1u; step >>= 1) {
        const uint64_t k = (uint64_t)q + step;
        if (k < n && off[k] <= i) q = (uint32_t)k;
    }
    return q;
}

// belief node ids: a member's own id (node * B + belief) and the union's
PORRT_JOIN_HD uint64_t join_union_id(uint64_t node_off, uint64_t B, uint64_t own_id) { return node_off * B + own_id; }
PORRT_JOIN_HD uint64_t join_own_id(uint64_t node_off, uint64_t B, uint64_t union_id) { return union_id - node_off * B; }
// member of a union belief node id < off[n] * B
PORRT_JOIN_HD uint32_t join_member_of_belief_node(const uint64_t *off, uint32_t n, uint64_t B, uint64_t union_id) { return join_member_of(off, n, union_id / B); }

} // namespace porrt
