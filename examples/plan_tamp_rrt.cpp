// The reference driver's TAMP-RRT run (src/main.rs:523-545, 612-633) with the C++ mirror: MapShelfDomainTampRRT::plan(..,
// TampSearch::BranchAndBound) from (0, -1) on a uniform prior, max_step 0.1, search_radius 2, n_iter_min 2500, n_iter_max 10000,
// goal radius 0.05.  Prints the expected costs before and after the shortcut, the zone order, the search's size and its time.
// usage: plan_tamp_rrt <map.pgm> <zone_ids.pgm> <n_worlds> [seed] [tamp_streams] [tamp_wave]
#include "../include/porrt.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s map.pgm zone_ids.pgm n_worlds [seed] [tamp_streams] [tamp_wave]\n", argv[0]); return 2; }
    using namespace po_rrt;
    try {
        auto m = MapShelfDomain::open(argv[1], {-1.0, -1.0}, {1.0, 1.0});
        m.add_zones(argv[2], 0.5);
        const size_t nw = std::strtoull(argv[3], nullptr, 10);
        const uint64_t seed = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 0;
        MapShelfDomainTampRRT tamp_rrt(ContinuousSampler({-1.0, -1.0}, {1.0, 1.0}, seed), DiscreteSampler(seed), m, 0.05);
        if (argc > 5) tamp_rrt.context().check(porrt_set_option(tamp_rrt.context().get(), "tamp_streams", std::strtoll(argv[5], nullptr, 10)));
        if (argc > 6) tamp_rrt.context().check(porrt_set_option(tamp_rrt.context().get(), "tamp_wave", std::strtoll(argv[6], nullptr, 10)));
        const auto t0 = std::chrono::steady_clock::now();
        const Policy policy = tamp_rrt.plan({0.0, -1.0}, BeliefState(nw, 1.0 / (double)nw), 0.1, 2.0, 2500, 10000, TampSearch::BranchAndBound);
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const porrt_tamp_info i = tamp_rrt.info();
        std::printf("best expected cost before shortcut %.17g\npolicy %zu nodes, %zu leafs, expected cost after shortcut %.17g\nzone order", i.search_cost,
                    policy.nodes.size(), policy.leafs.size(), policy.expected_costs);
        for (uint32_t k = 0; k < i.n_order; ++k) std::printf(" %u", i.zone_order[k]);
        std::printf("\nsearch nodes %llu, queries %llu, waves %llu\ntotal %.3f s\n", (unsigned long long)i.search_nodes, (unsigned long long)i.queries,
                    (unsigned long long)i.waves, s);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
