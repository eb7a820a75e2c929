// porrt_mm_recipe.hpp -- the arithmetic of porrt_mm_plan_batch (porrt_mm_plan_batch.hpp) that needs no device.
//
// The recipe.  Every mode of one multi-modal PRM plan clones the planner's never-advanced continuous sampler
// (map_shelves_tamp_prm.rs:206,254), so the k-th random point of ANY mode of plan p is the same point P_p[k].  A mode's node list is
// therefore written as 32-bit codes instead of coordinates: a code below 2^31 is k, an index into the plan's stream prefix P_p; a
// code with the top bit set names one of the explicit points (the planning start, goal states, observation samples -- an observation
// sample and its copies in the destination modes share one entry).  The host draws P_p once per plan, to the largest random count of
// its modes; the device expands codes into coordinates (k_mm_points), and mm_recipe_point is the same expansion on the host.
//
// The union.  The plans of a pass lie end to end: plan p's roadmap node j of mode m is union node noff[p] + mode_off_p[m] + j, and that
// number minus noff[p] is the plan's own belief node id (porrt_mmplan.hpp).  mm_pass_end cuts the passes, mm_plan_of finds the plan
// of a union node by a search of fixed length.
//
// Plain integer arithmetic on the arrays it is handed, shared by the engine and by tests/mm_recipe_check.cpp, which checks it against
// loops under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define PORRT_MMR_HD __host__ __device__ inline
#else
#define PORRT_MMR_HD inline
#endif

namespace porrt {

constexpr uint32_t kMmCodeExplicit = 0x80000000u;
constexpr uint32_t kMmCodeIndexMask = 0x7FFFFFFFu;
// option "mm_plan_batch_max_nodes": plans share a pass while their roadmap nodes stay at or below this (BASELINE.md has the sweep)
constexpr uint64_t kMmBatchNodesDefault = 1ull << 23;
// a pass's belief graph numbers its nodes in 31 bits (porrt_mm_build_belief_graph refuses 2^31 - 1 and more)
constexpr uint64_t kMmBatchNodesLimit = 0x7FFFFFFEull;
constexpr uint32_t kMmBatchPlansLimit = 65536;

PORRT_MMR_HD uint32_t mm_code_random(uint32_t k) { return k & kMmCodeIndexMask; }
PORRT_MMR_HD uint32_t mm_code_explicit(uint32_t k) { return kMmCodeExplicit | (k & kMmCodeIndexMask); }
PORRT_MMR_HD bool mm_code_is_explicit(uint32_t code) { return (code & kMmCodeExplicit) != 0; }
PORRT_MMR_HD uint32_t mm_code_index(uint32_t code) { return code & kMmCodeIndexMask; }

// One code into a point: false, and nothing read, when the index is outside its array.
PORRT_MMR_HD bool mm_recipe_point(uint32_t code, const double *prefix_x, const double *prefix_y, uint64_t prefix_len, const double *explicit_x,
                                  const double *explicit_y, uint64_t n_explicit, double *x, double *y) {
    const uint32_t k = mm_code_index(code);
    if (mm_code_is_explicit(code)) {
        if (k >= n_explicit) return false;
        *x = explicit_x[k]; *y = explicit_y[k];
    } else {
        if (k >= prefix_len) return false;
        *x = prefix_x[k]; *y = prefix_y[k];
    }
    return true;
}

// The recorder: what grow_mm_prm's add_sample calls become.  Node ids are the positions in the mode's code list, as in the single path.
struct MmRecipeMode {
    std::vector<uint32_t> codes;
    uint32_t n_random = 0;                          // random points so far: the next one is P[n_random]
};
struct MmRecipe {
    std::vector<MmRecipeMode> modes;
    std::vector<double> ex, ey;                     // the plan's explicit points
    bool overflow = false;                          // an index left 31 bits: the plan cannot be recorded
    size_t add_mode() { modes.emplace_back(); return modes.size() - 1; }
    // a new explicit point; the entry to hand to add_explicit_node (once per node that sits there)
    uint32_t add_point(double x, double y) {
        if (ex.size() >= kMmCodeIndexMask) { overflow = true; return 0; }
        ex.push_back(x); ey.push_back(y);
        return (uint32_t)(ex.size() - 1);
    }
    uint64_t add_explicit_node(size_t mode, uint32_t point) {
        modes[mode].codes.push_back(mm_code_explicit(point));
        return modes[mode].codes.size() - 1;
    }
    uint64_t add_random_node(size_t mode) {
        MmRecipeMode &m = modes[mode];
        if (m.n_random >= kMmCodeIndexMask) { overflow = true; return 0; }
        m.codes.push_back(mm_code_random(m.n_random++));
        return m.codes.size() - 1;
    }
    uint32_t prefix_len() const {                   // the plan's largest random count over its modes
        uint32_t n = 0;
        for (const MmRecipeMode &m : modes) n = m.n_random > n ? m.n_random : n;
        return n;
    }
    uint64_t nodes() const {
        uint64_t n = 0;
        for (const MmRecipeMode &m : modes) n += m.codes.size();
        return n;
    }
};

PORRT_MMR_HD uint64_t mm_add_sat(uint64_t a, uint64_t b) { return a > ~0ull - b ? ~0ull : a + b; }

// The pass that starts at plan `first` (< n) ends before the plan this returns (> first): plans are taken in order while the sum of
// their roadmap nodes stays at or below max_nodes (clamped to kMmBatchNodesLimit).  A plan that alone exceeds the bound is a pass of its
// own: the stages that follow accept or refuse it as they do a single plan.
PORRT_MMR_HD uint32_t mm_pass_end(const uint64_t *nodes, uint32_t n, uint32_t first, uint64_t max_nodes) {
    const uint64_t limit = max_nodes < kMmBatchNodesLimit ? max_nodes : kMmBatchNodesLimit;
    uint64_t sum = 0;
    uint32_t q = first;
    for (; q < n; ++q) {
        sum = mm_add_sat(sum, nodes[q]);
        if (sum > limit && q > first) break;
    }
    return q;
}

// Plan of union node i < off[n]: the largest q < n with off[q] <= i (off: n + 1 ascending entries, off[0] = 0).  Plans without nodes
// are stepped over.  32 trips whatever n and the sizes are.
PORRT_MMR_HD uint32_t mm_plan_of(const uint64_t *off, uint32_t n, uint64_t i) {
    uint32_t q = 0;
    for (uint32_t step = 0x80000000u; step >= 1u; step >>= 1) {
        const uint64_t k = (uint64_t)q + step;
        if (k < n && off[k] <= i) q = (uint32_t)k;
    }
    return q;
}
// belief node ids: the plan's own (mode_off + roadmap node) and the union's
PORRT_MMR_HD uint64_t mm_union_id(uint64_t node_off, uint64_t own_id) { return node_off + own_id; }
PORRT_MMR_HD uint64_t mm_own_id(uint64_t node_off, uint64_t union_id) { return union_id - node_off; }

} // namespace porrt
