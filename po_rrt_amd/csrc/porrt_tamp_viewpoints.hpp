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
    const double t_start = now_s();
    if (!c->has_grid || c->zones.empty() || c->domain != PORRT_DOMAIN_SHELF) { c->set_err("tamp: needs a shelf map with zones (porrt_set_grid, porrt_set_zones)"); return PORRT_ERR_INVALID; }
    if (!start || !belief || nw != (uint32_t)c->n_zones) { c->set_err("tamp: n_worlds must equal the number of zones"); return PORRT_ERR_INVALID; }
    double sum = 0.0;
    for (uint32_t w = 0; w < nw; ++w) sum = sum + belief[w];
    if (!(std::fabs(sum - 1.0) < 0.001)) { c->set_err("tamp: the prior does not sum to 1 (check_belief_state, common.rs:390)"); return PORRT_ERR_INVALID; }
    if (K == 0 || K > 4096) { c->set_err("batch_K must be in 1..4096"); return PORRT_ERR_INVALID; }
    if (!(goal_radius >= 0.0)) { c->set_err("tamp: goal_radius"); return PORRT_ERR_INVALID; }
    TampState &T = tamp_state(c);
    T.valid = false;
    memset(&T.info, 0, sizeof T.info);
    memset(&T.vinfo, 0, sizeof T.vinfo);
    T.info.fail_node = -1; T.info.fail_zone = -1; T.info.fail_query = -1;
    T.vinfo.max_viewpoints = max_viewpoints;
    T.nw = nw;
    const uint32_t streams = c->opt_tamp_streams ? 1u : 0u;
    const uint32_t wave = streams ? std::max<uint32_t>(1u, c->opt_tamp_wave) : 1u;
    const uint32_t pool_cap = std::max<uint32_t>(1u, c->opt_tamp_pool);
    T.info.streams = streams; T.info.wave = wave;
    const uint32_t nz = (uint32_t)c->n_zones;
    std::vector<TampNode> nodes(1);
    std::vector<uint32_t> rank_of(1, 0);
    {
        TampNode &root = nodes[0];
        std::vector<uint32_t> all(nz);
        for (uint32_t z = 0; z < nz; ++z) all[z] = z;
        root.remaining = tamp_shuffled(all, c->drng);
        root.ox = start[0]; root.oy = start[1];
        root.belief.assign(belief, belief + nw);
        root.h = c->s_seed;
    }
    std::vector<int64_t> stack{0};
    double best = std::numeric_limits<double>::infinity();
    int64_t best_leaf = -1;
    const Pcg64 crng0 = c->crng;
    struct Restore { porrt_ctx *c; Pcg64 s; bool on; ~Restore() { if (on) c->crng = s; } } restore{c, crng0, streams == 0};
    std::vector<std::vector<double>> paths;
    std::vector<double> costs;
    std::vector<char> ok;
    const uint64_t m1 = 1;
    // a child of edge e from the solution s of S, with its pickup path still to come
    auto add_child = [&](VpEdge &e, const VpSolutions &S, uint64_t s, uint32_t rank) {
        TampNode v;
        v.target = (int32_t)e.t; v.parent = e.u;
        v.remaining = e.remaining; v.belief = e.belief; v.rp = e.rp;
        v.h = tamp_splitmix64(e.ho ^ (((uint64_t)rank + 1) << 32));
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
    while (!stack.empty()) {
        std::vector<int64_t> popped;
        while (!stack.empty() && popped.size() < wave) { popped.push_back(stack.back()); stack.pop_back(); }
        ++T.info.waves;
        // the (node, zone) pairs in the sequential order, with their shuffles
        std::vector<VpEdge> edges;
        std::vector<std::pair<int64_t, std::pair<size_t, size_t>>> made;      // node, its range of edges
        for (int64_t uid : popped) {
            const size_t e0 = edges.size();
            const TampNode &u = nodes[(size_t)uid];
            for (uint32_t t : u.remaining) {
                std::vector<uint32_t> sh = tamp_shuffled(u.remaining, c->drng);
                VpEdge e;
                e.u = uid; e.t = t;
                for (uint32_t z : sh) if (z != t) e.remaining.push_back(z);
                e.belief = u.belief;
                if (u.target >= 0) e.belief[(size_t)u.target] = 0.0;
                tamp_normalize(e.belief);
                e.rp = u.rp * tamp_transition_probability(u.belief.data(), e.belief.data(), nw);
                e.ho = tamp_splitmix64(u.h ^ ((uint64_t)t + 1));
                edges.push_back(std::move(e));
            }
            made.push_back({uid, {e0, edges.size()}});
        }
        if (streams == 0) {
            for (VpEdge &e : edges) {
                double t0 = now_s();
                int r = porrt_set_observation_goal(c, e.t);
                T.info.goals_s += now_s() - t0;
                if (r < 0) return r;
                const double st[2] = {nodes[(size_t)e.u].ox, nodes[(size_t)e.u].oy};
                t0 = now_s();
                r = c->grow(st, max_step, search_radius, n_iter_min, n_iter_max, K, PORRT_MODE_RRT);
                T.info.grow_s += now_s() - t0;
                ++T.info.queries; ++T.vinfo.observation_queries;
                if (r < 0) return r;
                porrt_ctx *one = c;
                VpSolutions S;
                if ((r = vp_gather_solutions(c, T, &one, 1, S)) < 0) return r;
                const std::vector<uint64_t> kept = vp_keep(S, 0, max_viewpoints);
                count_viewpoints(S.first[1], kept.size());
                for (uint32_t j = 0; j < kept.size(); ++j) {
                    const int64_t vid = (int64_t)nodes.size();
                    add_child(e, S, kept[j], j);
                    t0 = now_s();
                    r = porrt_set_square_goal(c, c->zone_pos[e.t], &m1, 1, goal_radius);
                    T.info.goals_s += now_s() - t0;
                    if (r < 0) return r;
                    const double ps[2] = {nodes[(size_t)vid].ox, nodes[(size_t)vid].oy};
                    t0 = now_s();
                    r = c->grow(ps, max_step, search_radius, n_iter_min, n_iter_max, K, PORRT_MODE_RRT);
                    T.info.grow_s += now_s() - t0;
                    ++T.info.queries; ++T.vinfo.pickup_queries;
                    if (r < 0) return r;
                    if ((r = tamp_gather(c, T, &one, 1, paths, costs, ok)) < 0) return r;
                    if (!ok[0]) return tamp_fail(c, T, vid, (int32_t)e.t, 1);
                    nodes[(size_t)vid].path_pick = std::move(paths[0]); nodes[(size_t)vid].pick_cost = costs[0];
                }
            }
        } else {
            // the observation queries, all solutions of all rows gathered on the device
            for (size_t e0 = 0; e0 < edges.size(); e0 += pool_cap) {
                const uint32_t m = (uint32_t)std::min<size_t>(pool_cap, edges.size() - e0);
                int r = tamp_ensure_pool(c, T, m);
                if (r < 0) return r;
                std::vector<double> starts(2 * (size_t)m);
                double t0 = now_s();
                for (uint32_t i = 0; i < m; ++i) {
                    const VpEdge &e = edges[e0 + i];
                    if ((r = porrt_set_sampler(T.pool[i], c->s_low, c->s_up, e.ho)) < 0) return r;
                    if ((r = porrt_set_observation_goal(T.pool[i], e.t)) < 0) return r;
                    starts[2 * i] = nodes[(size_t)e.u].ox; starts[2 * i + 1] = nodes[(size_t)e.u].oy;
                }
                T.info.goals_s += now_s() - t0;
                t0 = now_s();
                r = porrt_grow_batch(T.pool.data(), m, starts.data(), max_step, search_radius, n_iter_min, n_iter_max, K, PORRT_MODE_RRT);
                T.info.grow_s += now_s() - t0;
                T.info.queries += m; T.vinfo.observation_queries += m;
                if (r < 0) { c->set_err(T.pool[0]->err); return r; }
                VpSolutions S;
                if ((r = vp_gather_solutions(c, T, T.pool.data(), m, S)) < 0) return r;
                for (uint32_t i = 0; i < m; ++i) {              // ids in the sequential order: (node, zone, rank)
                    const std::vector<uint64_t> kept = vp_keep(S, i, max_viewpoints);
                    count_viewpoints(S.first[i + 1] - S.first[i], kept.size());
                    for (uint32_t j = 0; j < kept.size(); ++j) add_child(edges[e0 + i], S, kept[j], j);
                }
            }
            // the pickup queries of every kept viewpoint
            std::vector<int64_t> kids;
            for (const VpEdge &e : edges) kids.insert(kids.end(), e.kids.begin(), e.kids.end());
            for (size_t k0 = 0; k0 < kids.size(); k0 += pool_cap) {
                const uint32_t m = (uint32_t)std::min<size_t>(pool_cap, kids.size() - k0);
                int r = tamp_ensure_pool(c, T, m);
                if (r < 0) return r;
                std::vector<double> starts(2 * (size_t)m);
                double t0 = now_s();
                for (uint32_t i = 0; i < m; ++i) {
                    const TampNode &v = nodes[(size_t)kids[k0 + i]];
                    if ((r = porrt_set_sampler(T.pool[i], c->s_low, c->s_up, v.h)) < 0) return r;
                    if ((r = porrt_set_square_goal(T.pool[i], c->zone_pos[v.target], &m1, 1, goal_radius)) < 0) return r;
                    starts[2 * i] = v.ox; starts[2 * i + 1] = v.oy;
                }
                T.info.goals_s += now_s() - t0;
                t0 = now_s();
                r = porrt_grow_batch(T.pool.data(), m, starts.data(), max_step, search_radius, n_iter_min, n_iter_max, K, PORRT_MODE_RRT);
                T.info.grow_s += now_s() - t0;
                T.info.queries += m; T.vinfo.pickup_queries += m;
                if (r < 0) { c->set_err(T.pool[0]->err); return r; }
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
            const TampNode &u = nodes[(size_t)mk.first];
            for (size_t ei = mk.second.first; ei < mk.second.second; ++ei)
                for (int64_t vid : edges[ei].kids) {
                    TampNode &v = nodes[(size_t)vid];
                    v.ec = u.ec + v.rp * (v.obs_cost + v.belief[(size_t)v.target] * v.pick_cost);
                    if (v.ec < best) stack.push_back(vid);
                    else ++T.info.pruned;
                }
            if (u.remaining.empty()) {
                if (u.ec < best) best = u.ec;
                if (best_leaf < 0 || u.ec <= nodes[(size_t)best_leaf].ec) best_leaf = mk.first;
            }
        }
    }
    T.info.search_nodes = nodes.size();
    if (best_leaf < 0) {                                   // expect("No solution found!") (:423)
        c->set_err("No solution found! (no search node reached a leaf: an observation query without solutions makes no children)");
        return PORRT_ERR_NO_PATH;
    }
    T.info.search_cost = nodes[(size_t)best_leaf].ec;
    T.info.n_order = 0; T.vinfo.n_ranks = 0;
    {
        std::vector<int64_t> chain;
        for (int64_t k = best_leaf; k > 0; k = nodes[(size_t)k].parent) chain.push_back(k);
        std::reverse(chain.begin(), chain.end());
        for (int64_t k : chain) {
            T.info.zone_order[T.info.n_order++] = (uint32_t)nodes[(size_t)k].target;
            T.vinfo.ranks[T.vinfo.n_ranks++] = rank_of[(size_t)k];
        }
    }
    restore.on = false;
    if (streams == 0) c->crng = crng0;
    const int r = tamp_build_policy(c, T, nodes, best_leaf);
    if (r < 0) return r;
    T.valid = true;
    T.info.pool = (uint32_t)T.pool.size();
    T.info.total_s = now_s() - t_start;
    T.info.search_s = T.info.total_s - T.info.grow_s - T.info.path_s - T.info.shortcut_s - T.info.pool_s - T.info.goals_s - T.vinfo.solutions_s;
    return (int64_t)T.parents.size();
}

} // namespace
