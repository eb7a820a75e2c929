// policy_graph_mirror.cpp -- the C++ mirror of get_policy_graph (include/porrt.hpp): the free policy_graph() on the reference's
// two-world diamond (pto_graph.rs:591-606), and PTO::get_policy_graph() on a grown graph against the mirror's own PTOGraph: the pruned
// lists are the kept entries of the original children and parents lists, in order, and remove_edge's rule holds between them.
// usage: policy_graph_mirror <map.pgm> <zone_ids.pgm>
#include "../include/porrt.hpp"
#include <cmath>
#include <cstdio>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "policy_graph_mirror: %s fails (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s map.pgm zone_ids.pgm\n", argv[0]); return 2; }
    using namespace po_rrt;
    try {
        // the diamond with two worlds: 0-1, 0-2, 1-3, 2-3 both ways; node 1 is valid in world 1 only, node 2 in world 0 only
        const double s2 = std::sqrt(2.0), inf = std::numeric_limits<double>::infinity();
        const std::vector<std::vector<uint32_t>> children = {{1, 2}, {0, 3}, {0, 3}, {1, 2}};
        const std::vector<std::vector<double>> costs = {{s2 + s2, inf, s2, 0.0}, {s2 + s2, s2, inf, 0.0}};
        std::vector<uint8_t> keep, how;
        struct porrt_policy_graph_info info;
        const auto pruned = policy_graph(children, costs, &keep, &how, &info);
        CHECK(pruned[3] == (std::vector<uint32_t>{1, 2}) && pruned[1] == (std::vector<uint32_t>{3}) && pruned[2] == (std::vector<uint32_t>{3}));
        CHECK(keep.size() == 8 && how.size() == 8 && info.entries == 8);
        uint64_t kept = 0;
        for (uint8_t k : keep) kept += k;
        CHECK(info.kept == kept);

        auto m = MapShelfDomain::open(argv[1], {-1.0, -1.0}, {1.0, 1.0});
        m.add_zones(argv[2], 0.5);
        SquareGoal goal({{{0.68, -0.45}, 0b01}, {{0.68, 0.38}, 0b10}}, 0.05);
        PTO pto(ContinuousSampler({-1.0, -1.0}, {1.0, 1.0}, 0), DiscreteSampler(0), m);
        pto.batch_K = 256;
        CHECK(pto.grow_graph({-0.8, -0.8}, goal, 0.05, 5.0, 1, 100000));
        pto.plan_qmdp();
        const PTO::PolicyGraph g = pto.get_policy_graph();
        const size_t n = pto.graph.nodes.size();
        CHECK(g.children.size() == n && g.parents.size() == n);
        size_t e = 0, n_kept = 0;
        for (size_t u = 0; u < n; ++u) {
            std::vector<uint32_t> want;
            for (const PTOEdge &c : pto.graph.nodes[u].children) { if (g.keep[e]) want.push_back((uint32_t)c.id); ++e; }
            CHECK(g.children[u] == want);
            n_kept += want.size();
        }
        CHECK(e == g.keep.size() && e == g.info.entries && n_kept == g.info.kept && n_kept > 0 && n_kept < e);
        // remove_edge (pto_graph.rs:214-217): p stays among parents[x] iff x stays among children[p]
        for (size_t x = 0; x < n; ++x) {
            std::vector<uint32_t> want;
            for (const PTOEdge &p : pto.graph.nodes[x].parents) {
                const auto &cs = g.children[p.id];
                if (std::find(cs.begin(), cs.end(), (uint32_t)x) != cs.end()) want.push_back((uint32_t)p.id);
            }
            CHECK(g.parents[x] == want);
        }
        uint64_t by_how = 0;
        for (uint64_t h : g.info.how) by_how += h;
        CHECK(by_how == g.info.entries && g.info.how[5] == 0);
        std::printf("policy_graph_mirror ok: %zu nodes, %zu entries, %zu kept, %llu by the simplex\n", n, e, n_kept, (unsigned long long)g.info.residual);
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 1;
    }
    return 0;
}
