// The reference driver's multi-modal PRM run (src/main.rs:546-575, test_plan_tamp_mm_prm_on_map_benchmark_2_goals) with the C++
// mirror: MapShelfDomainTampPRM::plan from (0, -1) on a uniform prior, max_step 0.1, search_radius 2, then PartialShortCut.
// Prints the expected costs, the policies' sizes and the time of the whole run.
// usage: plan_tamp_prm <map.pgm> <zone_ids.pgm> <n_worlds> <n_iter_per_belief> <refine_iterations> [seed]
#include "../include/porrt.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: %s map.pgm zone_ids.pgm n_worlds n_iter_per_belief refine_iterations [seed]\n", argv[0]); return 2; }
    using namespace po_rrt;
    try {
        auto m = MapShelfDomain::open(argv[1], {-1.0, -1.0}, {1.0, 1.0});
        m.add_zones(argv[2], 0.5);
        const size_t nw = std::strtoull(argv[3], nullptr, 10), n_iter = std::strtoull(argv[4], nullptr, 10), n_refine = std::strtoull(argv[5], nullptr, 10);
        const uint64_t seed = argc > 6 ? std::strtoull(argv[6], nullptr, 10) : 0;
        MapShelfDomainTampPRM tamp_prm(ContinuousSampler({-1.0, -1.0}, {1.0, 1.0}, seed), DiscreteSampler(seed), m);
        const auto t0 = std::chrono::steady_clock::now();
        const Policy policy = tamp_prm.plan({0.0, -1.0}, BeliefState(nw, 1.0 / (double)nw), 0.1, 2.0, n_iter);
        const Policy refined = tamp_prm.refine_policy(n_refine);
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("policy %zu nodes, %zu leafs, expected cost %.17g\nrefined %zu nodes, expected cost %.17g\ntotal %.3f s\n", policy.nodes.size(),
                    policy.leafs.size(), policy.expected_costs, refined.nodes.size(), refined.expected_costs, s);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
