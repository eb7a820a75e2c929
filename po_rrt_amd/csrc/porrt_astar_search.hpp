// porrt_astar_search.hpp -- what is one plan's own in the TAMP-RRT A* search (porrt_tamp_astar.hpp, DESIGN.md sections 23 and 25):
// the node and expansion tables, the belief table, the queue, the replay, the selection of a wave, taking a child's record back and
// the failure rule -- and the rounds that drive many searches of one type in lockstep (these, or porrt_bnb_search.hpp's).  Plain
// C++, no HIP: tests/astar_search_check.cpp builds it on its own under the sanitizers, with a stub in place of the device.
//
// A search never grows anything itself.  Per round it REPLAYS (pops while the top of its queue is a leaf or already has its
// children; popping gives the children their ids and pushes them), then SELECTS up to W expandable queue entries and hands out
// one Edge per child of each; whoever drives it computes a ChildRecord per edge and gives it back with take().  The children
// enter the queue only when their parent is popped, so the pop sequence, every id, ec and priority are those of W = 1 whatever
// was selected beside; a child without a path fails the search only when its parent is popped, with the id the child would have
// got.  Nothing in a search depends on another search: run() may mix the edges of many in one chunk.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <tuple>
#include <utility>
#include <vector>

#include "porrt_astar_queue.hpp"

namespace porrt_astar {

static inline uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// stream seed of the edge into the child of zone t of a node whose own seed is h
static inline uint64_t edge_seed(uint64_t h, uint32_t t) { return splitmix64(h ^ ((uint64_t)t + 1)); }

static inline void normalize(std::vector<double> &b) {
    double s = 0.0;
    for (double p : b) s = s + p;
    for (double &p : b) p = p / s;
}

static inline double transition_probability(const double *parent, const double *child, uint32_t nw) {     // common.rs:188-190
    double s = 0.0;
    for (uint32_t w = 0; w < nw; ++w) s = s + (child[w] > 0.0 ? parent[w] : 0.0);
    return s;
}

// a child's belief and reaching probability: the parent's belief with the parent's target zeroed, normalised
static inline std::pair<std::vector<double>, double> child_belief(const double *belief, int32_t target, double rp, uint32_t nw) {
    std::vector<double> b(belief, belief + nw);
    if (target >= 0) b[(size_t)target] = 0.0;
    normalize(b);
    const double q = transition_probability(belief, b.data(), nw);
    return {std::move(b), rp * q};
}

enum : uint32_t { kChildOk = 0, kChildNoObs = 1, kChildNoPick = 2 };     // a record's status: which query found no path

struct ChildRecord {                           // what the search keeps of a child's two queries
    double ec = 0.0, priority = 0.0, ox = 0.0, oy = 0.0;
    uint32_t obs_off = 0, obs_len = 0, pick_off = 0, pick_len = 0;       // its two paths, wherever the driver keeps them
    uint32_t status = kChildOk;
};

struct Node {
    int32_t target = -1;
    int64_t parent = -1;
    unsigned long long remaining = 0;          // bit z: zone z still to visit (always walked in ascending order)
    double ox = 0, oy = 0;                     // observation_state
    double rp = 1.0, ec = 0.0, priority = 0.0;
    uint32_t belief = 0;                       // row of the search's belief table
    uint64_t h = 0;                            // stream seed of the edge into this node
    uint32_t obs_off = 0, obs_len = 0, pick_off = 0, pick_len = 0;
    int64_t kids = -1;                         // its expansion, once selected
    bool popped = false;
};

struct Expansion {                             // the children of one node, before they have ids
    uint32_t belief = 0;
    double rp = 0.0;
    std::vector<uint32_t> zone;
    std::vector<ChildRecord> rec;
};

struct Edge {                                  // child i of expansion e of node u of search `plan`
    uint32_t plan;
    int64_t u, e;
    uint32_t i;
};

class Search {
public:
    enum State { kLive, kSolved, kFailed, kExhausted };

    uint32_t nw = 0;
    std::vector<Node> nodes;
    std::vector<Expansion> exps;
    std::vector<double> beliefs;               // rows of nw: row 0 the prior, one more per expansion
    State state = kLive;
    int64_t solution = -1;
    int64_t fail_node = -1;                    // kFailed: the id the child would have got, its zone, 0 = observation / 1 = pickup
    int32_t fail_zone = -1, fail_query = -1;
    uint64_t waves = 0, queries = 0;           // rounds in which it selected; queries run for its edges

    void begin(const double start[2], const double *prior, uint32_t n_zones, uint64_t seed) {
        nw = n_zones;
        nodes.assign(1, Node());
        exps.clear();
        beliefs.assign(prior, prior + nw);
        queue_.clear();
        state = kLive; solution = -1; fail_node = -1; fail_zone = fail_query = -1; waves = queries = 0;
        Node &root = nodes[0];
        root.remaining = nw >= 64 ? ~0ull : ((1ull << nw) - 1ull);
        root.ox = start[0]; root.oy = start[1];
        root.h = seed;
        queue_.push(0.0, 0);
    }

    const double *belief_row(uint32_t row) const { return beliefs.data() + (size_t)row * nw; }
    // what the driver's device side asks of an edge, whichever search it drives
    uint32_t zone_of(const Edge &ed) const { return exps[(size_t)ed.e].zone[ed.i]; }
    double edge_rp(const Edge &ed) const { return exps[(size_t)ed.e].rp; }
    const double *edge_belief(const Edge &ed) const { return belief_row(exps[(size_t)ed.e].belief); }
    unsigned long long edge_remaining(const Edge &ed) const { return nodes[(size_t)ed.u].remaining & ~(1ull << zone_of(ed)); }
    bool expandable(uint64_t id) const { return nodes[(size_t)id].remaining && nodes[(size_t)id].kids < 0; }

    // pops while the top is a leaf or has its children; ids are given here
    State replay() {
        if (state != kLive) return state;
        while (!queue_.empty()) {
            const int64_t uid = (int64_t)queue_.top().id;
            if (expandable((uint64_t)uid)) return state;
            queue_.pop();
            nodes[(size_t)uid].popped = true;
            if (nodes[(size_t)uid].kids >= 0) {
                const Expansion &E = exps[(size_t)nodes[(size_t)uid].kids];
                for (uint32_t i = 0; i < E.zone.size(); ++i) {
                    const ChildRecord &o = E.rec[i];
                    if (o.status != kChildOk) {
                        fail_node = (int64_t)nodes.size(); fail_zone = (int32_t)E.zone[i]; fail_query = o.status == kChildNoObs ? 0 : 1;
                        return state = kFailed;
                    }
                    Node v;
                    const Node &u = nodes[(size_t)uid];
                    v.target = (int32_t)E.zone[i]; v.parent = uid;
                    v.remaining = u.remaining & ~(1ull << E.zone[i]);
                    v.ox = o.ox; v.oy = o.oy; v.rp = E.rp; v.ec = o.ec; v.priority = o.priority;
                    v.belief = E.belief;
                    v.h = edge_seed(u.h, E.zone[i]);
                    v.obs_off = o.obs_off; v.obs_len = o.obs_len; v.pick_off = o.pick_off; v.pick_len = o.pick_len;
                    queue_.push(v.priority, (uint64_t)nodes.size());
                    nodes.push_back(v);
                }
            }
            if (!nodes[(size_t)uid].remaining) { solution = uid; return state = kSolved; }
        }
        return state = kExhausted;
    }

    // After a replay that left the search live: the top and the next best queue entries without children, up to `wave` in all, get
    // their expansions; one Edge per child is appended to `edges`, in node then zone order.  Returns the nodes selected.
    size_t select(uint32_t wave, uint32_t plan, std::vector<Edge> &edges) {
        std::vector<QueueEntry> held;
        size_t taken = 0;
        while (!queue_.empty() && taken < wave) {
            const QueueEntry e = queue_.pop();
            held.push_back(e);
            if (!expandable(e.id)) continue;
            const int64_t ei = open_expansion((int64_t)e.id);
            nodes[(size_t)e.id].kids = ei;
            for (uint32_t i = 0; i < exps[(size_t)ei].zone.size(); ++i) edges.push_back({plan, (int64_t)e.id, ei, i});
            ++taken;
        }
        for (const QueueEntry &e : held) queue_.push(e.priority, e.id);
        if (taken) ++waves;
        return taken;
    }

    void take(const Edge &ed, const ChildRecord &rec) {
        exps[(size_t)ed.e].rec[ed.i] = rec;
        queries += rec.status == kChildNoObs ? 1u : 2u;          // the pickup query runs only where the zone was seen
    }

    uint64_t speculated() const {              // expansions whose node was never popped
        uint64_t n = 0;
        for (const Node &v : nodes) if (v.kids >= 0 && !v.popped) ++n;
        return n;
    }
    std::vector<int64_t> chain() const {       // root .. solution
        std::vector<int64_t> out;
        for (int64_t k = solution; k >= 0; k = nodes[(size_t)k].parent) out.push_back(k);
        std::reverse(out.begin(), out.end());
        return out;
    }

private:
    Queue queue_;

    int64_t open_expansion(int64_t uid) {
        const Node &u = nodes[(size_t)uid];
        Expansion E;
        std::vector<double> vb;
        std::tie(vb, E.rp) = child_belief(belief_row(u.belief), u.target, u.rp, nw);
        E.belief = (uint32_t)(beliefs.size() / nw);
        beliefs.insert(beliefs.end(), vb.begin(), vb.end());
        for (uint32_t z = 0; z < nw; ++z) if ((u.remaining >> z) & 1ull) E.zone.push_back(z);
        E.rec.resize(E.zone.size());
        exps.push_back(std::move(E));
        return (int64_t)exps.size() - 1;
    }
};

// The driver of n searches of one type, in rounds: every live search replays; solved, failed and exhausted ones leave; the rest
// select their wave; all selected edges, in plan then node then zone order, are cut into chunks of `chunk` rows wherever the cut
// falls, and expand(edges, e0, m, out) fills out[0 .. m) for edges[e0 .. e0 + m) -- a negative return ends the run with that code --
// before the records go back to their searches.  `rounds` counts the rounds that expanded something; a round in which the live
// searches selected nothing to expand (a branch and bound that popped only leaves) just goes on to the next replay.
// SearchT (Search here, porrt_bnb::Search): State with kLive, replay(), select(wave, plan, edges), take(edge, record).
template <class SearchT, class Expand>
static int run(std::vector<SearchT> &S, uint32_t wave, size_t chunk, uint64_t &rounds, Expand expand) {
    std::vector<Edge> edges;
    std::vector<ChildRecord> out;
    if (wave == 0) wave = 1;
    if (chunk == 0) chunk = 1;
    while (true) {
        edges.clear();
        bool live = false;
        for (uint32_t p = 0; p < S.size(); ++p)
            if (S[p].replay() == SearchT::kLive) { live = true; S[p].select(wave, p, edges); }
        if (!live) return 0;
        if (edges.empty()) continue;
        ++rounds;
        for (size_t e0 = 0; e0 < edges.size(); e0 += chunk) {
            const uint32_t m = (uint32_t)std::min(chunk, edges.size() - e0);
            out.assign(m, ChildRecord());
            const int r = expand((const std::vector<Edge> &)edges, e0, m, out.data());
            if (r < 0) return r;
            for (uint32_t i = 0; i < m; ++i) S[edges[e0 + i].plan].take(edges[e0 + i], out[i]);
        }
    }
}

} // namespace porrt_astar
