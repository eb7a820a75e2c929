// porrt_tamp_bnb_batch.hpp -- porrt_tamp_rrt_plan_batch: many branch-and-bound plans (porrt_tamp.hpp,
// "tamp_search" 0) on one map in one call.  Plan p is tamp_plan's search from starts[p] with prior priors[p], its per-edge streams
// rooted at seeds[p] and its shuffles drawn from a discrete sampler of its own, seeded discrete_seeds[p]; with per-edge streams it
// is, bit for bit, the plan it is alone on a fresh context seeded alike, at the same "tamp_wave".
//
// What is one plan's own -- node table, stack, bound, leaf rule, discrete sampler, counters -- is porrt_bnb::Search
// (porrt_bnb_search.hpp, host only).  The rounds are porrt_astar::run and the device side is SearchRun (porrt_tamp_astar.hpp), both
// shared with the A* batch: the rows of all plans ride in the same porrt_grow_batch, their paths stay in one arena, one
// k_astar_children per chunk brings a 64-byte record per child down (its ec is tamp_plan's expression in tamp_plan's order; its
// priority is not used), and one k_astar_chain / k_tamp_shortcut launch ends the chains of every plan that holds a leaf.
#pragma once

#include "porrt_bnb_search.hpp"

namespace {

using BnbSearch = porrt_bnb::Search;

static int64_t tamp_plan_bnb_batch(porrt_ctx *c, uint32_t n_plans, const double *starts, const double *priors, const uint64_t *seeds,
                                   const uint64_t *discrete_seeds, uint32_t nw, double max_step, double search_radius, uint64_t n_iter_min,
                                   uint64_t n_iter_max, double goal_radius, uint32_t K) {
    if (n_plans == 0 || n_plans > 65536u) { c->set_err("tamp batch: n_plans must be in 1..65536"); return PORRT_ERR_INVALID; }
    if (!starts || !priors) { c->set_err("tamp batch: starts and priors"); return PORRT_ERR_INVALID; }
    if (!c->opt_tamp_streams) { c->set_err("tamp batch: needs per-edge streams (tamp_streams 1): one continuous stream cannot be shared by plans"); return PORRT_ERR_INVALID; }
    if (c->opt_tamp_search != 0) {
        c->set_err(c->opt_tamp_search == 1 ? "tamp: TampSearch::AStar has an entry point of its own: porrt_tamp_rrt_plan_astar"
                                           : "tamp: TampSearch::BranchAndBoundMultipleViewPoints has an entry point of its own: porrt_tamp_rrt_plan_viewpoints");
        return PORRT_ERR_INVALID;
    }
    TampFrame F;
    int r = F.begin(c, starts, priors, nw, max_step, search_radius, n_iter_min, n_iter_max, goal_radius, K, [&](int stage) -> int {
        if (stage != 0) return PORRT_OK;
        if (astar_check_zones(c, nw) < 0) return PORRT_ERR_INVALID;      // k_astar_children's zone mask
        for (uint32_t p = 0; p < n_plans; ++p) {                // every plan's prior, before anything runs (zero entries are allowed)
            const double *b = priors + (size_t)p * nw;
            double sum = 0.0;
            for (uint32_t w = 0; w < nw; ++w) sum = sum + b[w];
            if (!(std::fabs(sum - 1.0) < 0.001)) { c->set_err("tamp batch: plan " + std::to_string(p) + ": the prior does not sum to 1 (check_belief_state, common.rs:390)"); return PORRT_ERR_INVALID; }
        }
        return PORRT_OK;
    });
    if (r < 0) return r;
    TampState &T = *F.T;
    AstarState &A = astar_state(T);
    memset(&A.info, 0, sizeof A.info);
    A.parents.clear(); A.targets.clear(); A.ec.clear(); A.priority.clear();      // the last single plan is replaced
    A.batch.clear();
    A.batch_nw = nw;
    A.batch_bnb = true;

    std::vector<BnbSearch> S(n_plans);
    for (uint32_t p = 0; p < n_plans; ++p) {
        const uint64_t seed = seeds ? seeds[p] : c->s_seed;
        S[p].begin(starts + 2 * (size_t)p, priors + (size_t)p * nw, nw, seed, discrete_seeds ? discrete_seeds[p] : seed);
    }
    SearchRun<BnbSearch> R{c, F, T, A, S, true, "tamp"};
    if ((r = R.begin()) < 0) return r;
    r = porrt_astar::run(S, F.wave, F.pool_cap, T.info.waves,
                         [&](const std::vector<AstarEdge> &edges, size_t e0, uint32_t m, AstarChildRecord *out) { return R.expand_chunk(edges, e0, m, out); });
    A.info.arena_states = A.arena_cap;
    for (const BnbSearch &s : S) { T.info.search_nodes += s.nodes.size(); T.info.pruned += s.pruned; }
    if (r < 0) return r;

    std::vector<AstarBatchPlan> plans(n_plans);
    std::vector<uint32_t> solved;
    std::vector<TampPolicyArrays> arrays;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const BnbSearch &s = S[p];
        AstarBatchPlan &B = plans[p];
        porrt_tamp_batch_plan &rec = B.rec;
        memset(&rec, 0, sizeof rec);
        rec.status = s.state == BnbSearch::kSolved ? PORRT_OK : PORRT_ERR_NO_PATH;
        rec.fail_node = s.fail_node; rec.fail_zone = s.fail_zone; rec.fail_query = s.fail_query;
        rec.search_nodes = s.nodes.size(); rec.queries = s.queries; rec.waves = s.waves;
        B.pruned = s.pruned;
        for (const porrt_bnb::Node &n : s.nodes) { B.node_parents.push_back(n.parent); B.node_targets.push_back(n.target); B.node_ec.push_back(n.ec); B.node_pushed.push_back(n.pushed ? 1 : 0); }
        if (s.state != BnbSearch::kSolved) continue;
        rec.search_cost = s.nodes[(size_t)s.best_leaf].ec;
        rec.n_order = astar_zone_order(s, rec.zone_order);
        solved.push_back(p);
        arrays.push_back(TampPolicyArrays{B.xy, B.beliefs, B.parents, B.leaf});
    }
    if (!solved.empty()) {
        std::vector<double> expected;
        if ((r = R.policies(solved, arrays, expected)) < 0) return r;
        for (size_t i = 0; i < solved.size(); ++i) {
            plans[solved[i]].rec.expected_cost = expected[i];
            plans[solved[i]].rec.policy_nodes = plans[solved[i]].parents.size();
        }
    }
    A.batch = std::move(plans);
    F.close(A.info.children_s);
    return (int64_t)solved.size();
}

} // namespace
