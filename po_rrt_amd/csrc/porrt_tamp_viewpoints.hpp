// porrt_tamp_viewpoints.hpp -- MapShelfDomainTampRRT::plan(.., TampSearch::BranchAndBoundMultipleViewPoints)
// (src/map_shelves_tamp_rrt.rs:293-430) with its RRT queries grown and all their solutions gathered on the device (DESIGN.md
// section 21).
//
// The search is the branch and bound of porrt_tamp.hpp with one difference: the observation query of a (node, zone) pair keeps
// every solution of its tree (RRT::plan_several, rrt.rs:95-100: every distinct way into the zone's visibility disk), and each of
// them -- a viewpoint -- becomes a child of its own, with a pickup query from where it ends.  The reference walks the viewpoints in
// the order of a HashSet; here they are walked in ASCENDING NODE ID, one of the orders the reference may take (not one we can claim
// it took).  max_viewpoints (ours, not the reference's): 0 keeps all; n > 0 keeps, per observation query, the n solutions of lowest
// cost (ties: the lower id), still walked in ascending id.
//
// Streams ("tamp_streams"):
//   0  one continuous stream on the lead context: per (node, zone) the observation query, then the pickup queries of its
//      viewpoints in ascending id; set back on return.
//   1  (default) the observation query of (u, t) runs on a stream seeded ho = splitmix64(u.h ^ (t + 1)) (root h = the sampler seed),
//      the pickup query of the viewpoint of rank j (0-based, in the kept list) on h = splitmix64(ho ^ ((j + 1) << 32)), which is also
//      the child's h.  Unlike BranchAndBound the pickup does not continue the observation stream: one observation tree feeds many
//      pickups.  A node's cost is a function of its (zone, rank) prefix alone, so the best cost is the same at every "tamp_wave".
#pragma once

#include "porrt_solutions.hpp"

namespace {

struct VpSolutions {                              // the solutions of the rows of one gather, concatenated row by row
    std::vector<uint64_t> first;                  // row q: solutions [first[q], first[q + 1])
    std::vector<uint64_t> ids, lens, off;         // per solution; its states are xy[2 * off[s] .. 2 * (off[s] + lens[s]))
    std::vector<double> costs, xy;
};

static int vp_gather_solutions(porrt_ctx *c, TampState &T, porrt_ctx *const *ctxs, uint32_t n, VpSolutions &S) {
    const double t0 = now_s();
    SolGather G;
    int r = solutions_select(c, T, ctxs, n, G);
    if (r < 0) return r;
    S.ids.assign(G.n_solutions, 0); S.lens.assign(G.n_solutions, 0); S.costs.assign(G.n_solutions, 0.0);
    S.xy.assign(2 * (size_t)G.n_states, 0.0);
    if ((r = solutions_write(c, T, G, S.ids.data(), S.lens.data(), S.costs.data(), S.xy.data())) < 0) return r;
    S.first.assign(n + 1, 0);
    for (uint32_t q = 0; q < n; ++q) S.first[q + 1] = S.first[q] + (G.rows[q].status == kSolOk ? G.rows[q].count : 0u);
    S.off.assign(G.n_solutions, 0);
    uint64_t at = 0;
    for (uint64_t s = 0; s < G.n_solutions; ++s) { S.off[s] = at; at += S.lens[s]; }
    T.vinfo.solutions_s += now_s() - t0;
    return PORRT_OK;
}

// the kept viewpoints of row q, ascending id
static std::vector<uint64_t> vp_keep(const VpSolutions &S, uint32_t q, uint32_t max_viewpoints) {
    std::vector<uint64_t> k;
    for (uint64_t s = S.first[q]; s < S.first[q + 1]; ++s) k.push_back(s);
    if (max_viewpoints && k.size() > max_viewpoints) {
        std::stable_sort(k.begin(), k.end(), [&](uint64_t a, uint64_t b) { return S.costs[a] < S.costs[b]; });   // ties stay in id order
        k.resize(max_viewpoints);
        std::sort(k.begin(), k.end());
    }
    return k;
}

struct VpEdge {                                   // one (node, zone) pair of a wave
    int64_t u;
    uint32_t t;
    std::vector<uint32_t> remaining;
    std::vector<double> belief;
    double rp;
    uint64_t ho;
    std::vector<int64_t> kids;
};

static int64_t tamp_plan_viewpoints(porrt_ctx *c, const double start[2], const double *belief, uint32_t nw, double max_step, double search_radius,
                                    uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t K, uint32_t max_viewpoints) {
    TampFrame F;
    int r = F.begin(c, start, belief, nw, max_step, search_radius, n_iter_min, n_iter_max, goal_radius, K);
    if (r < 0) return r;
    TampState &T = *F.T;
    T.vinfo.max_viewpoints = max_viewpoints;
    std::vector<TampNode> nodes{tamp_root(c, start, belief, nw)};
    std::vector<uint32_t> rank_of(1, 0);
    TampBound B;
    std::vector<std::vector<double>> paths;
    std::vector<double> costs;
    std::vector<char> ok;
    // a child of edge e from the solution s of S, with its pickup path still to come
    auto add_child = [&](VpEdge &e, const VpSolutions &S, uint64_t s, uint32_t rank) {
        TampNode v;
        v.target = (int32_t)e.t; v.parent = e.u;
        v.remaining = e.remaining; v.belief = e.belief; v.rp = e.rp;
        v.h = porrt_astar::splitmix64(e.ho ^ (((uint64_t)rank + 1) << 32));
        v.path_obs.assign(S.xy.begin() + 2 * S.off[s], S.xy.begin() + 2 * (S.off[s] + S.lens[s]));
        v.obs_cost = S.costs[s];
        v.ox = v.path_obs[v.path_obs.size() - 2]; v.oy = v.path_obs.back();
        e.kids.push_back((int64_t)nodes.size());
        nodes.push_back(std::move(v));
        rank_of.push_back(rank);
    };
    auto count_viewpoints = [&](uint64_t found, uint64_t kept) {
        T.vinfo.viewpoints_found += found; T.vinfo.viewpoints_kept += kept;
        T.vinfo.largest_set = std::max<uint64_t>(T.vinfo.largest_set, found);
    };
    while (!B.stack.empty()) {
        const std::vector<int64_t> popped = B.pop(F.wave);
        ++T.info.waves;
        // the (node, zone) pairs in the sequential order, with their shuffles
        std::vector<VpEdge> edges;
        std::vector<std::pair<int64_t, std::pair<size_t, size_t>>> made;      // node, its range of edges
        for (int64_t uid : popped) {
            const size_t e0 = edges.size();
            const TampNode &u = nodes[(size_t)uid];
            for (uint32_t t : u.remaining) {
                VpEdge e;
                e.u = uid; e.t = t;
                e.remaining = tamp_remaining_without(u.remaining, t, c->drng);
                std::tie(e.belief, e.rp) = porrt_astar::child_belief(u.belief.data(), u.target, u.rp, nw);
                e.ho = porrt_astar::edge_seed(u.h, t);
                edges.push_back(std::move(e));
            }
            made.push_back({uid, {e0, edges.size()}});
        }
        if (F.streams == 0) {
            for (VpEdge &e : edges) {
                const double st[2] = {nodes[(size_t)e.u].ox, nodes[(size_t)e.u].oy};
                r = F.grow_lead(st, e.t, 0);
                ++T.vinfo.observation_queries;
                if (r < 0) return r;
                porrt_ctx *one = c;
                VpSolutions S;
                if ((r = vp_gather_solutions(c, T, &one, 1, S)) < 0) return r;
                const std::vector<uint64_t> kept = vp_keep(S, 0, max_viewpoints);
                count_viewpoints(S.first[1], kept.size());
                for (uint32_t j = 0; j < kept.size(); ++j) {
                    const int64_t vid = (int64_t)nodes.size();
                    add_child(e, S, kept[j], j);
                    const double ps[2] = {nodes[(size_t)vid].ox, nodes[(size_t)vid].oy};
                    r = F.grow_lead(ps, e.t, 1);
                    ++T.vinfo.pickup_queries;
                    if (r < 0) return r;
                    if ((r = tamp_gather(c, T, &one, 1, paths, costs, ok)) < 0) return r;
                    if (!ok[0]) return tamp_fail(c, T, vid, (int32_t)e.t, 1);
                    nodes[(size_t)vid].path_pick = std::move(paths[0]); nodes[(size_t)vid].pick_cost = costs[0];
                }
            }
        } else {
            // the observation queries, all solutions of all rows gathered on the device
            for (size_t e0 = 0; e0 < edges.size(); e0 += F.pool_cap) {
                const uint32_t m = (uint32_t)std::min<size_t>(F.pool_cap, edges.size() - e0);
                if ((r = tamp_ensure_pool(c, T, m)) < 0) return r;
                std::vector<double> starts(2 * (size_t)m);
                for (uint32_t i = 0; i < m; ++i) { starts[2 * i] = nodes[(size_t)edges[e0 + i].u].ox; starts[2 * i + 1] = nodes[(size_t)edges[e0 + i].u].oy; }
                r = F.grow_rows(T.pool.data(), m, starts.data(), [&](uint32_t i) { return F.seed_and_goal(T.pool[i], edges[e0 + i].ho, edges[e0 + i].t, 0); });
                T.vinfo.observation_queries += m;
                if (r < 0) return r;
                VpSolutions S;
                if ((r = vp_gather_solutions(c, T, T.pool.data(), m, S)) < 0) return r;
                for (uint32_t i = 0; i < m; ++i) {              // ids in the sequential order: (node, zone, rank)
                    const std::vector<uint64_t> kept = vp_keep(S, i, max_viewpoints);
                    count_viewpoints(S.first[i + 1] - S.first[i], kept.size());
                    for (uint32_t j = 0; j < kept.size(); ++j) add_child(edges[e0 + i], S, kept[j], j);
                }
            }
            // the pickup queries of every kept viewpoint, each on a stream of its own: one observation tree feeds many pickups
            std::vector<int64_t> kids;
            for (const VpEdge &e : edges) kids.insert(kids.end(), e.kids.begin(), e.kids.end());
            for (size_t k0 = 0; k0 < kids.size(); k0 += F.pool_cap) {
                const uint32_t m = (uint32_t)std::min<size_t>(F.pool_cap, kids.size() - k0);
                if ((r = tamp_ensure_pool(c, T, m)) < 0) return r;
                std::vector<double> starts(2 * (size_t)m);
                for (uint32_t i = 0; i < m; ++i) { starts[2 * i] = nodes[(size_t)kids[k0 + i]].ox; starts[2 * i + 1] = nodes[(size_t)kids[k0 + i]].oy; }
                r = F.grow_rows(T.pool.data(), m, starts.data(), [&](uint32_t i) {
                    const TampNode &v = nodes[(size_t)kids[k0 + i]];
                    return F.seed_and_goal(T.pool[i], v.h, (uint32_t)v.target, 1);
                });
                T.vinfo.pickup_queries += m;
                if (r < 0) return r;
                if ((r = tamp_gather(c, T, T.pool.data(), m, paths, costs, ok)) < 0) return r;
                for (uint32_t i = 0; i < m; ++i) {
                    TampNode &v = nodes[(size_t)kids[k0 + i]];
                    if (!ok[i]) return tamp_fail(c, T, kids[k0 + i], v.target, 1);      // the first one in the sequential order
                    v.path_pick = std::move(paths[i]); v.pick_cost = costs[i];
                }
            }
        }
        T.info.search_nodes = nodes.size();
        // push the children, record the leaves: the sequential order
        for (const auto &mk : made) {
            std::vector<int64_t> kids;
            for (size_t ei = mk.second.first; ei < mk.second.second; ++ei) kids.insert(kids.end(), edges[ei].kids.begin(), edges[ei].kids.end());
            B.close(T, nodes, mk.first, kids);
        }
    }
    T.info.search_nodes = nodes.size();
    if (B.best_leaf < 0) {                                 // expect("No solution found!") (:423)
        c->set_err("No solution found! (no search node reached a leaf: an observation query without solutions makes no children)");
        return PORRT_ERR_NO_PATH;
    }
    T.vinfo.n_ranks = 0;
    for (int64_t k : tamp_chain(nodes, B.best_leaf)) if (k > 0) T.vinfo.ranks[T.vinfo.n_ranks++] = rank_of[(size_t)k];
    return F.finish(nodes, B.best_leaf, T.vinfo.solutions_s);
}

} // namespace
