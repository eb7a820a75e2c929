// MapShelfDomainTampRRT::plan_batch of the C++ mirror (include/porrt.hpp) against plan(.., TampSearch::BranchAndBound) alone on
// planners seeded alike, plan for plan and bit for bit; built and run by tests/test_gpu_tamp_bnb_batch.py.
// usage: bnb_batch_mirror <map.pgm> <zone_ids.pgm> <n_worlds>
#include "../include/porrt.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace po_rrt;

static bool same(const Policy &a, const Policy &b) {
    if (a.nodes.size() != b.nodes.size() || a.leafs != b.leafs || std::memcmp(&a.expected_costs, &b.expected_costs, 8)) return false;
    for (size_t k = 0; k < a.nodes.size(); ++k) {
        const PolicyNode &x = a.nodes[k], &y = b.nodes[k];
        if (std::memcmp(x.state.data(), y.state.data(), 16) || x.parent != y.parent || x.children != y.children) return false;
        if (x.belief_state.size() != y.belief_state.size() || std::memcmp(x.belief_state.data(), y.belief_state.data(), 8 * x.belief_state.size())) return false;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    try {
        auto m = MapShelfDomain::open(argv[1], {-1.0, -1.0}, {1.0, 1.0});
        m.add_zones(argv[2], 0.5);
        const size_t nw = std::strtoull(argv[3], nullptr, 10);
        const std::vector<State> starts{{0.0, -1.0}, {-0.6, -0.9}, {0.0, -1.0}};
        const std::vector<BeliefState> priors(3, BeliefState(nw, 1.0 / (double)nw));
        const std::vector<uint64_t> seeds{0, 1, 0}, dseeds{0, 5, 0};
        MapShelfDomainTampRRT lead(ContinuousSampler({-1.0, -1.0}, {1.0, 1.0}, 7), DiscreteSampler(7), m, 0.05);
        lead.context().check(porrt_set_option(lead.context().get(), "tamp_wave", 7));
        const auto batch = lead.plan_batch(starts, priors, seeds, dseeds, 0.1, 2.0, 2500, 10000);
        if (batch.n_ok != 3 || batch.policies.size() != 3 || batch.plans.size() != 3 || batch.pruned.size() != 3) { std::fprintf(stderr, "n_ok %zu\n", batch.n_ok); return 1; }
        for (size_t p = 0; p < 3; ++p) {
            MapShelfDomainTampRRT one(ContinuousSampler({-1.0, -1.0}, {1.0, 1.0}, seeds[p]), DiscreteSampler(dseeds[p]), m, 0.05);
            one.context().check(porrt_set_option(one.context().get(), "tamp_wave", 7));
            const Policy alone = one.plan(starts[p], priors[p], 0.1, 2.0, 2500, 10000, TampSearch::BranchAndBound);
            const porrt_tamp_info i = one.info();
            const porrt_tamp_batch_plan &r = batch.plans[p];
            if (!same(batch.policies[p], alone) || r.status != PORRT_OK || std::memcmp(&r.search_cost, &i.search_cost, 8) || r.queries != i.queries ||
                r.waves != i.waves || batch.pruned[p] != i.pruned || r.speculated != 0 || r.search_nodes != i.search_nodes || r.n_order != i.n_order ||
                std::memcmp(r.zone_order, i.zone_order, 4 * r.n_order) || r.policy_nodes != alone.nodes.size()) {
                std::fprintf(stderr, "plan %zu differs from the single plan\n", p);
                return 1;
            }
        }
        if (!same(batch.policies[0], batch.policies[2])) { std::fprintf(stderr, "the repeat differs\n"); return 1; }
        std::printf("bnb_batch_mirror ok\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
