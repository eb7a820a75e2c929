// porrt_bnb_search.hpp -- what is one plan's own in the TAMP-RRT branch and bound (porrt_tamp.hpp, DESIGN.md sections 17 and 28):
// the node table, the belief table, the stack, the bound and the best leaf, the plan's discrete sampler and its counters.  Plain
// C++, no HIP: tests/bnb_search_check.cpp builds it on its own under the sanitizers, with a stub in place of the device.
//
// The search is tamp_plan's loop cut into the three operations porrt_astar::run drives (porrt_astar_search.hpp): per round it
// REPLAYS -- closes the nodes popped last round in the sequential order: a child is pushed iff its expected cost is below the best
// leaf's so far, the others count as pruned, a popped node without remaining zones is a leaf and the last leaf of the lowest cost
// wins -- then SELECTS: pops up to W nodes off the stack and makes one child per remaining zone of each, with a fresh shuffle per
// child from the plan's own discrete sampler, in the order tamp_plan draws them.  A child has its id from the moment it is made.
// Whoever drives the search computes a ChildRecord per child and gives it back with take().  The first child of a wave, in the
// sequential order, whose record has no path fails the search when the wave is replayed.  Nothing in a search depends on another
// search: run() may mix the edges of many in one chunk.
#pragma once

#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "porrt_astar_search.hpp"
#include "porrt_pcg64.hpp"

namespace porrt_bnb {

using porrt_astar::ChildRecord;
using porrt_astar::Edge;                       // child e (a node id) of node u of search `plan`; i = its place among u's children

// shuffle (map_shelves_tamp_rrt.rs:20-32): draw an index, swap_remove it
template <class Rng>
static inline std::vector<uint32_t> shuffled(const std::vector<uint32_t> &v, Rng &rng) {
    std::vector<uint32_t> to = v, out;
    out.reserve(v.size());
    while (!to.empty()) {
        const size_t i = (size_t)rng.gen_range_usize(to.size());
        out.push_back(to[i]);
        to[i] = to.back();
        to.pop_back();
    }
    return out;
}

// a fresh shuffle of `remaining` without zone t: one per child
template <class Rng>
static inline std::vector<uint32_t> remaining_without(const std::vector<uint32_t> &remaining, uint32_t t, Rng &rng) {
    std::vector<uint32_t> out;
    for (uint32_t z : shuffled(remaining, rng)) if (z != t) out.push_back(z);
    return out;
}

struct Node {
    int32_t target = -1;
    int64_t parent = -1;
    std::vector<uint32_t> remaining;           // the zones still to visit, as shuffled for this node
    double ox = 0, oy = 0;                     // observation_state
    double rp = 1.0, ec = 0.0;
    uint32_t belief = 0;                       // row of the search's belief table (the children of a node share theirs)
    uint64_t h = 0;                            // stream seed of the edge into this node
    uint32_t obs_off = 0, obs_len = 0, pick_off = 0, pick_len = 0;
    uint32_t status = porrt_astar::kChildOk;   // of its two queries
    int64_t first_kid = -1;                    // its children are the ids first_kid .. first_kid + remaining.size()
    bool pushed = false;                       // it went onto the stack (the root does)
};

class Search {
public:
    enum State { kLive, kSolved, kFailed, kExhausted };

    uint32_t nw = 0;
    std::vector<Node> nodes;
    std::vector<double> beliefs;               // rows of nw: row 0 the prior, one more per node that made children
    std::vector<int64_t> stack;
    double best = std::numeric_limits<double>::infinity();
    int64_t best_leaf = -1;
    State state = kLive;
    int64_t fail_node = -1;                    // kFailed: the child whose query found no path, its zone, 0 = observation / 1 = pickup
    int32_t fail_zone = -1, fail_query = -1;
    uint64_t waves = 0, queries = 0, pruned = 0;
    Pcg64 rng{};                               // the plan's discrete sampler

    void begin(const double start[2], const double *prior, uint32_t n_zones, uint64_t seed, uint64_t discrete_seed) {
        nw = n_zones;
        nodes.assign(1, Node());
        beliefs.assign(prior, prior + nw);
        stack.assign(1, 0);
        popped_.clear();
        best = std::numeric_limits<double>::infinity();
        best_leaf = -1;
        state = kLive; fail_node = -1; fail_zone = fail_query = -1; waves = queries = pruned = 0;
        rng.seed_from_u64(discrete_seed);
        Node &root = nodes[0];
        std::vector<uint32_t> all(nw);
        for (uint32_t z = 0; z < nw; ++z) all[z] = z;
        root.remaining = shuffled(all, rng);
        root.ox = start[0]; root.oy = start[1];
        root.h = seed;
        root.pushed = true;
    }

    const double *belief_row(uint32_t row) const { return beliefs.data() + (size_t)row * nw; }
    // what the driver's device side asks of an edge, whichever search it drives
    uint32_t zone_of(const Edge &ed) const { return (uint32_t)nodes[(size_t)ed.e].target; }
    double edge_rp(const Edge &ed) const { return nodes[(size_t)ed.e].rp; }
    const double *edge_belief(const Edge &ed) const { return belief_row(nodes[(size_t)ed.e].belief); }
    unsigned long long edge_remaining(const Edge &) const { return 0ull; }       // no heuristic here: the priority is not used

    // closes the wave popped last round (TampBound::close per node, after the failure rule over the whole wave)
    State replay() {
        if (state != kLive) return state;
        for (int64_t uid : popped_) {
            const Node &u = nodes[(size_t)uid];
            for (size_t i = 0; i < u.remaining.size(); ++i) {
                const Node &v = nodes[(size_t)u.first_kid + i];
                if (v.status == porrt_astar::kChildOk) continue;
                fail_node = u.first_kid + (int64_t)i; fail_zone = v.target; fail_query = v.status == porrt_astar::kChildNoObs ? 0 : 1;
                popped_.clear();
                return state = kFailed;
            }
        }
        for (int64_t uid : popped_) {
            const Node &u = nodes[(size_t)uid];
            for (size_t i = 0; i < u.remaining.size(); ++i) {
                Node &v = nodes[(size_t)u.first_kid + i];
                if (v.ec < best) { stack.push_back(u.first_kid + (int64_t)i); v.pushed = true; }
                else ++pruned;
            }
            if (u.remaining.empty()) {
                if (u.ec < best) best = u.ec;
                if (best_leaf < 0 || u.ec <= nodes[(size_t)best_leaf].ec) best_leaf = uid;      // the last equal leaf wins
            }
        }
        popped_.clear();
        if (stack.empty()) state = best_leaf >= 0 ? kSolved : kExhausted;
        return state;
    }

    // After a replay that left the search live: pops up to `wave` nodes and makes their children in the sequential order, with
    // tamp_plan's shuffle draws; one Edge per child is appended to `edges`.  A wave of leaves appends none.  Returns the nodes popped.
    size_t select(uint32_t wave, uint32_t plan, std::vector<Edge> &edges) {
        while (!stack.empty() && popped_.size() < wave) { popped_.push_back(stack.back()); stack.pop_back(); }
        ++waves;
        for (int64_t uid : popped_) {
            const std::vector<uint32_t> rem_u = nodes[(size_t)uid].remaining;
            if (rem_u.empty()) continue;
            const Node &u0 = nodes[(size_t)uid];
            const std::pair<std::vector<double>, double> vb = porrt_astar::child_belief(belief_row(u0.belief), u0.target, u0.rp, nw);
            const uint32_t row = (uint32_t)(beliefs.size() / nw);
            beliefs.insert(beliefs.end(), vb.first.begin(), vb.first.end());
            nodes[(size_t)uid].first_kid = (int64_t)nodes.size();
            for (uint32_t i = 0; i < rem_u.size(); ++i) {
                Node v;
                v.remaining = remaining_without(rem_u, rem_u[i], rng);
                v.belief = row; v.rp = vb.second;
                v.target = (int32_t)rem_u[i];
                v.parent = uid;
                v.h = porrt_astar::edge_seed(nodes[(size_t)uid].h, rem_u[i]);
                edges.push_back({plan, uid, (int64_t)nodes.size(), i});
                nodes.push_back(std::move(v));
            }
        }
        return popped_.size();
    }

    void take(const Edge &ed, const ChildRecord &rec) {
        Node &v = nodes[(size_t)ed.e];
        v.ec = rec.ec; v.ox = rec.ox; v.oy = rec.oy;
        v.obs_off = rec.obs_off; v.obs_len = rec.obs_len; v.pick_off = rec.pick_off; v.pick_len = rec.pick_len;
        v.status = rec.status;
        queries += rec.status == porrt_astar::kChildNoObs ? 1u : 2u;          // the pickup query runs only where the zone was seen
    }

    std::vector<int64_t> chain() const {       // root .. best leaf
        std::vector<int64_t> out;
        for (int64_t k = best_leaf; k >= 0; k = nodes[(size_t)k].parent) out.push_back(k);
        std::reverse(out.begin(), out.end());
        return out;
    }

private:
    std::vector<int64_t> popped_;              // the wave whose children are out, in pop order
};

} // namespace porrt_bnb
