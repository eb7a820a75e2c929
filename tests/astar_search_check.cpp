// One plan's search and the driver of many (po_rrt_amd/csrc/porrt_astar_search.hpp) on the host, with a deterministic stub in place of
// the device: a child's record is hashed from its stream seed, which is a function of (plan seed, zone prefix) alone, and some
// children find no path.  Exit status 0 and "astar_search_check ok" when every case agrees; built with
// -fsanitize=address,undefined by tests/test_tamp_astar_batch_cpu.py.
//
// Checked: searches driven in lockstep -- 1, 2 and 7 of them, 3 to 6 zones, chunks of 1, 5 and 64 rows, widths 1, 3 and 64 -- give
// each the node table, solution and failure of that search alone at width 1, and the queries, waves and `speculated` of that
// search alone at the same width; a failed child that is never popped fails nothing; bit-equal priorities pop in ascending id.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../po_rrt_amd/csrc/porrt_astar_search.hpp"

using porrt_astar::ChildRecord;
using porrt_astar::Edge;
using porrt_astar::Search;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 20) std::fprintf(stderr, "astar_search_check: line %d: %s\n", __LINE__, #c); } } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

enum Mode { kHashed, kTies };
static const double kZone[6][2] = {{-0.8, 0.7}, {-0.3, 0.6}, {0.2, 0.8}, {0.7, 0.5}, {-0.6, -0.2}, {0.5, -0.4}};

// the stub: what the two queries of an edge and k_astar_children would give, from the searches' tables alone
struct Stub {
    std::vector<Search> &S;
    Mode mode;
    uint32_t fail_one_in;                      // a child fails when its hash is a multiple of this (0: never)
    uint64_t calls = 0, rows = 0;
    size_t largest = 0;

    int operator()(const std::vector<Edge> &edges, size_t e0, uint32_t m, ChildRecord *out) {
        ++calls; rows += m;
        if (m > largest) largest = m;
        for (uint32_t i = 0; i < m; ++i) {
            const Edge &ed = edges[e0 + i];
            const Search &s = S[ed.plan];
            const porrt_astar::Node &u = s.nodes[(size_t)ed.u];
            const porrt_astar::Expansion &E = s.exps[(size_t)ed.e];
            const uint32_t t = E.zone[ed.i];
            const uint64_t h = porrt_astar::splitmix64(porrt_astar::edge_seed(u.h, t));
            ChildRecord &r = out[i];
            if (fail_one_in && h % fail_one_in == 0) { r.status = (h >> 20) & 1u ? porrt_astar::kChildNoObs : porrt_astar::kChildNoPick; continue; }
            const double obs = 0.05 + (double)(h & 0xFFFFu) / 65536.0, pick = 0.05 + (double)((h >> 16) & 0xFFFFu) / 131072.0;
            r.ox = -1.0 + 2.0 * (double)((h >> 32) & 0xFFFu) / 4096.0;
            r.oy = -1.0 + 2.0 * (double)((h >> 44) & 0xFFFu) / 4096.0;
            r.obs_off = (uint32_t)(h >> 40); r.obs_len = 3; r.pick_off = (uint32_t)(h >> 8); r.pick_len = 2;
            const double *b = s.belief_row(E.belief);
            if (mode == kTies) {                 // every node of a depth has the same priority, and the depths are in order
                r.ec = u.ec + 1.0;
                r.priority = r.ec;
                continue;
            }
            r.ec = u.ec + E.rp * (obs + b[t] * pick);
            double hz = 0.0;
            const unsigned long long rem = u.remaining & ~(1ull << t);
            for (uint32_t z = 0; z < s.nw; ++z) {
                if (!((rem >> z) & 1ull)) continue;
                const double dx = kZone[z][0] - r.ox, dy = kZone[z][1] - r.oy;
                hz = hz + b[z] * std::sqrt(dx * dx + dy * dy);
            }
            r.priority = r.ec + E.rp * hz;
        }
        return 0;
    }
};

static std::vector<Search> make(uint32_t n) {
    std::vector<Search> S(n);
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t nz = 3u + p % 4u;
        std::vector<double> prior(nz);
        double sum = 0.0;
        for (uint32_t z = 0; z < nz; ++z) { prior[z] = 1.0 + (double)((p + 2u * z) % 3u); sum += prior[z]; }
        for (double &x : prior) x /= sum;
        const double start[2] = {-0.5 + 0.1 * p, -1.0};
        S[p].begin(start, prior.data(), nz, 1000u + 17u * p);
    }
    return S;
}

static uint64_t drive(std::vector<Search> &S, uint32_t wave, size_t chunk, Mode mode, uint32_t fail_one_in, size_t *largest = nullptr) {
    Stub stub{S, mode, fail_one_in};
    uint64_t rounds = 0;
    const int r = porrt_astar::run(S, wave, chunk, rounds, [&](const std::vector<Edge> &e, size_t e0, uint32_t m, ChildRecord *out) { return stub(e, e0, m, out); });
    CHECK(r == 0);
    if (largest) *largest = stub.largest;
    return rounds;
}

static void same_search(const Search &a, const Search &b) {
    CHECK(a.state == b.state && a.solution == b.solution);
    CHECK(a.fail_node == b.fail_node && a.fail_zone == b.fail_zone && a.fail_query == b.fail_query);
    CHECK(a.nodes.size() == b.nodes.size());
    for (size_t k = 0; k < a.nodes.size() && k < b.nodes.size(); ++k) {
        CHECK(a.nodes[k].parent == b.nodes[k].parent && a.nodes[k].target == b.nodes[k].target);
        CHECK(same_bits(a.nodes[k].ec, b.nodes[k].ec) && same_bits(a.nodes[k].priority, b.nodes[k].priority));
        CHECK(a.nodes[k].obs_off == b.nodes[k].obs_off && a.nodes[k].pick_off == b.nodes[k].pick_off && a.nodes[k].h == b.nodes[k].h);
    }
}

// the stated order from the node table alone: pop the lowest (priority, id); the popped node's children are exactly the next ids
static void replay_table(const Search &s) {
    std::vector<std::vector<size_t>> kids(s.nodes.size());
    for (size_t k = 1; k < s.nodes.size(); ++k) { CHECK(s.nodes[k].parent >= 0 && (size_t)s.nodes[k].parent < k); kids[(size_t)s.nodes[k].parent].push_back(k); }
    std::vector<size_t> open{0};
    size_t next = 1;
    while (!open.empty()) {
        size_t best = 0;
        for (size_t i = 1; i < open.size(); ++i) {
            const double pa = s.nodes[open[i]].priority, pb = s.nodes[open[best]].priority;
            if (pa < pb || (!(pb < pa) && open[i] < open[best])) best = i;
        }
        const size_t u = open[best];
        open.erase(open.begin() + (ptrdiff_t)best);
        for (size_t i = 0; i < kids[u].size(); ++i) { CHECK(kids[u][i] == next + i); open.push_back(kids[u][i]); }
        next += kids[u].size();
        if (!s.nodes[u].remaining) { CHECK(s.state == Search::kSolved && (size_t)s.solution == u && next == s.nodes.size()); return; }
        if (kids[u].size() < (size_t)__builtin_popcountll(s.nodes[u].remaining)) {      // a failing child: it and its later siblings were not made
            CHECK(s.state == Search::kFailed && next == s.nodes.size() && s.fail_node == (int64_t)next);
            return;
        }
    }
    CHECK(false);
}

int main() {
    const uint32_t counts[] = {1, 2, 7}, widths[] = {1, 3, 64};
    const size_t chunks[] = {1, 5, 64};
    uint64_t solved_beside_failed_speculation = 0, failed_searches = 0, solved_searches = 0, cuts_inside_children = 0;
    for (Mode mode : {kHashed, kTies})
        for (uint32_t fail_one_in : {0u, 9u})
            for (uint32_t n : counts) {
                // every search alone, at width 1 and at the widths under test
                std::vector<Search> alone1 = make(n);
                for (uint32_t p = 0; p < n; ++p) {
                    std::vector<Search> one{alone1[p]};
                    drive(one, 1, 1u << 20, mode, fail_one_in);
                    alone1[p] = one[0];
                    CHECK(alone1[p].state == Search::kSolved || alone1[p].state == Search::kFailed);
                    CHECK(alone1[p].speculated() == 0);
                    replay_table(alone1[p]);
                }
                for (uint32_t W : widths) {
                    std::vector<Search> aloneW = make(n);
                    for (uint32_t p = 0; p < n; ++p) {
                        std::vector<Search> one{aloneW[p]};
                        drive(one, W, 1u << 20, mode, fail_one_in);
                        aloneW[p] = one[0];
                    }
                    for (size_t chunk : chunks) {
                        std::vector<Search> S = make(n);
                        size_t largest = 0;
                        const uint64_t rounds = drive(S, W, chunk, mode, fail_one_in, &largest);
                        CHECK(largest <= chunk);
                        uint64_t most = 0;
                        for (uint32_t p = 0; p < n; ++p) {
                            same_search(S[p], alone1[p]);
                            same_search(S[p], aloneW[p]);
                            CHECK(S[p].queries == aloneW[p].queries && S[p].waves == aloneW[p].waves && S[p].speculated() == aloneW[p].speculated());
                            most = std::max(most, S[p].waves);
                            if (S[p].state == Search::kFailed) { ++failed_searches; CHECK(S[p].fail_node == (int64_t)S[p].nodes.size()); }
                            if (S[p].state != Search::kSolved) continue;
                            ++solved_searches;
                            CHECK(S[p].chain().size() == S[p].nw + 1u && S[p].fail_node == -1);
                            for (const porrt_astar::Node &v : S[p].nodes) {
                                if (v.kids < 0 || v.popped) continue;
                                for (const ChildRecord &r : S[p].exps[(size_t)v.kids].rec) if (r.status != porrt_astar::kChildOk) { ++solved_beside_failed_speculation; break; }
                            }
                        }
                        CHECK(rounds == most);                 // the call's rounds are those of its longest search
                        if (chunk == 5 && n > 1) ++cuts_inside_children;
                    }
                }
            }
    CHECK(solved_searches > 0 && failed_searches > 0);
    CHECK(solved_beside_failed_speculation > 0);               // a failed child that was never popped failed nothing
    CHECK(cuts_inside_children > 0);

    // bit-equal priorities pop in ascending id: with every priority of a depth equal, the search is breadth first in id order
    {
        std::vector<Search> S = make(4);
        drive(S, 3, 5, kTies, 0);
        for (const Search &s : S) {
            CHECK(s.state == Search::kSolved);
            for (size_t k = 1; k < s.nodes.size(); ++k) CHECK(s.nodes[k].parent >= s.nodes[k - 1].parent);     // parents popped in id order
            // the solution is the first node of full depth, which is the lowest id among the leaves
            for (size_t k = 0; k < (size_t)s.solution; ++k) CHECK(s.nodes[k].remaining != 0);
            // -0.0 and +0.0 are equal: nothing to pop before the root here, but the root's priority is +0.0 and pops first
            CHECK(s.nodes[0].popped);
        }
    }
    if (failures) { std::fprintf(stderr, "astar_search_check: %d failures\n", failures); return 1; }
    std::printf("astar_search_check ok\n");
    return 0;
}
