// One plan's branch and bound (po_rrt_amd/csrc/porrt_bnb_search.hpp) and the driver of many (porrt_astar::run, as a template over the
// search type) on the host, with a deterministic stub in place of the device: a child's record is hashed from its stream seed,
// which is a function of (plan seed, zone prefix) alone, and some children find no path.  Exit status 0 and "bnb_search_check ok"
// when every case agrees; built with -fsanitize=address,undefined by tests/test_tamp_bnb_batch_cpu.py.
//
// Checked: searches driven in lockstep -- 1, 2 and 7 of them, 3 to 6 zones, chunks of 1, 5 and 64 rows, widths 1, 3 and 64 -- give
// each the node table, best leaf, failure, pruned, queries and waves of that search alone at the same width, and of the loop of
// porrt_tamp.hpp's tamp_plan written out once more below (pop a wave, make the children with their shuffles, run the queries, fail
// at the first child without a path, close in the sequential order); leaves of bit-equal cost are resolved last-wins; a plan of
// one zone ends in one round; a prior with a zero entry prunes its NaN leaves, as that loop does.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../po_rrt_amd/csrc/porrt_bnb_search.hpp"

using porrt_astar::ChildRecord;
using porrt_astar::Edge;
using porrt_bnb::Search;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 20) std::fprintf(stderr, "bnb_search_check: line %d: %s\n", __LINE__, #c); } } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

enum Mode { kHashed, kTies };

// the stub: what the two queries of the edge into zone t below a node (stream seed uh, cost uec) and k_astar_children would give
static ChildRecord record(uint64_t uh, uint32_t t, double uec, double rp, double bt, Mode mode, uint32_t fail_one_in) {
    const uint64_t h = porrt_astar::splitmix64(porrt_astar::edge_seed(uh, t));
    ChildRecord r;
    if (fail_one_in && h % fail_one_in == 0) { r.status = (h >> 20) & 1u ? porrt_astar::kChildNoObs : porrt_astar::kChildNoPick; return r; }
    const double obs = 0.05 + (double)(h & 0xFFFFu) / 65536.0, pick = 0.05 + (double)((h >> 16) & 0xFFFFu) / 131072.0;
    r.ox = -1.0 + 2.0 * (double)((h >> 32) & 0xFFFu) / 4096.0;
    r.oy = -1.0 + 2.0 * (double)((h >> 44) & 0xFFFu) / 4096.0;
    r.obs_off = (uint32_t)(h >> 40); r.obs_len = 3; r.pick_off = (uint32_t)(h >> 8); r.pick_len = 2;
    r.ec = mode == kTies ? uec + 1.0 : uec + rp * (obs + bt * pick);          // kTies: every node of a depth costs the same
    return r;
}

struct Stub {
    std::vector<Search> &S;
    Mode mode;
    uint32_t fail_one_in;
    size_t largest = 0;
    int operator()(const std::vector<Edge> &edges, size_t e0, uint32_t m, ChildRecord *out) {
        if (m > largest) largest = m;
        for (uint32_t i = 0; i < m; ++i) {
            const Edge &ed = edges[e0 + i];
            const Search &s = S[ed.plan];
            const uint32_t t = s.zone_of(ed);
            CHECK(ed.e > ed.u && s.nodes[(size_t)ed.e].parent == ed.u && s.nodes[(size_t)ed.u].remaining[ed.i] == t);
            CHECK(s.nodes[(size_t)ed.e].h == porrt_astar::edge_seed(s.nodes[(size_t)ed.u].h, t));
            out[i] = record(s.nodes[(size_t)ed.u].h, t, s.nodes[(size_t)ed.u].ec, s.edge_rp(ed), s.edge_belief(ed)[t], mode, fail_one_in);
        }
        return 0;
    }
};

struct Problem {
    uint32_t nz;
    std::vector<double> prior;
    double start[2];
    uint64_t seed, dseed;
};

static Problem problem(uint32_t p, uint32_t nz) {
    Problem q;
    q.nz = nz;
    q.prior.resize(nz);
    double sum = 0.0;
    for (uint32_t z = 0; z < nz; ++z) { q.prior[z] = 1.0 + (double)((p + 2u * z) % 3u); sum += q.prior[z]; }
    for (double &x : q.prior) x /= sum;
    q.start[0] = -0.5 + 0.1 * p; q.start[1] = -1.0;
    q.seed = 1000u + 17u * p;
    q.dseed = p % 2u ? 77u + p : q.seed;       // a discrete seed of its own for every other plan
    return q;
}

static std::vector<Problem> problems(uint32_t n) {
    std::vector<Problem> P;
    for (uint32_t p = 0; p < n; ++p) P.push_back(problem(p, 3u + p % 4u));
    return P;
}

static std::vector<Search> make(const std::vector<Problem> &P) {
    std::vector<Search> S(P.size());
    for (size_t p = 0; p < P.size(); ++p) S[p].begin(P[p].start, P[p].prior.data(), P[p].nz, P[p].seed, P[p].dseed);
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

// tamp_plan's loop, in one piece
struct RefNode {
    int32_t target = -1;
    int64_t parent = -1;
    std::vector<uint32_t> remaining;
    std::vector<double> belief;
    double rp = 1.0, ec = 0.0;
    uint64_t h = 0;
    ChildRecord rec;
    bool pushed = false;
};
struct Ref {
    std::vector<RefNode> nodes;
    int64_t best_leaf = -1, first_leaf = -1, fail_node = -1;
    int32_t fail_zone = -1, fail_query = -1;
    uint64_t waves = 0, queries = 0, pruned = 0, equal_leaves = 0;
};

static std::vector<uint32_t> ref_shuffled(std::vector<uint32_t> to, Pcg64 &rng) {
    std::vector<uint32_t> out;
    while (!to.empty()) {
        const size_t i = (size_t)rng.gen_range_usize(to.size());
        out.push_back(to[i]);
        to[i] = to.back();
        to.pop_back();
    }
    return out;
}

static Ref reference(const Problem &q, uint32_t wave, Mode mode, uint32_t fail_one_in) {
    Ref R;
    Pcg64 rng;
    rng.seed_from_u64(q.dseed);
    RefNode root;
    std::vector<uint32_t> all(q.nz);
    for (uint32_t z = 0; z < q.nz; ++z) all[z] = z;
    root.remaining = ref_shuffled(all, rng);
    root.belief = q.prior;
    root.h = q.seed;
    root.pushed = true;
    R.nodes.push_back(root);
    std::vector<int64_t> stack{0};
    double best = std::numeric_limits<double>::infinity();
    while (!stack.empty()) {
        std::vector<int64_t> popped;
        while (!stack.empty() && popped.size() < wave) { popped.push_back(stack.back()); stack.pop_back(); }
        ++R.waves;
        std::vector<int64_t> edges;
        for (int64_t uid : popped) {
            const std::vector<uint32_t> rem_u = R.nodes[(size_t)uid].remaining;
            for (uint32_t t : rem_u) {
                RefNode v;
                for (uint32_t z : ref_shuffled(rem_u, rng)) if (z != t) v.remaining.push_back(z);
                const RefNode &u = R.nodes[(size_t)uid];
                v.belief = u.belief;
                if (u.target >= 0) v.belief[(size_t)u.target] = 0.0;
                double s = 0.0;
                for (double x : v.belief) s = s + x;
                for (double &x : v.belief) x = x / s;
                double tp = 0.0;
                for (uint32_t w = 0; w < q.nz; ++w) tp = tp + (v.belief[w] > 0.0 ? u.belief[w] : 0.0);
                v.rp = u.rp * tp;
                v.target = (int32_t)t; v.parent = uid;
                v.h = porrt_astar::edge_seed(u.h, t);
                edges.push_back((int64_t)R.nodes.size());
                R.nodes.push_back(v);
            }
        }
        for (int64_t vid : edges) {
            RefNode &v = R.nodes[(size_t)vid];
            const RefNode &u = R.nodes[(size_t)v.parent];
            v.rec = record(u.h, (uint32_t)v.target, u.ec, v.rp, v.belief[(size_t)v.target], mode, fail_one_in);
            if (v.rec.status != porrt_astar::kChildOk) {
                R.fail_node = vid; R.fail_zone = v.target; R.fail_query = v.rec.status == porrt_astar::kChildNoObs ? 0 : 1;
                return R;
            }
            R.queries += 2;
        }
        for (int64_t uid : popped) {
            const RefNode &u = R.nodes[(size_t)uid];
            for (int64_t vid = 0; vid < (int64_t)R.nodes.size(); ++vid) {
                RefNode &v = R.nodes[(size_t)vid];
                if (v.parent != uid) continue;
                v.ec = v.rec.ec;
                if (v.ec < best) { stack.push_back(vid); v.pushed = true; }
                else ++R.pruned;
            }
            if (u.remaining.empty()) {
                if (u.ec < best) best = u.ec;
                if (R.first_leaf < 0) R.first_leaf = uid;
                if (R.best_leaf >= 0 && same_bits(u.ec, R.nodes[(size_t)R.best_leaf].ec)) ++R.equal_leaves;
                if (R.best_leaf < 0 || u.ec <= R.nodes[(size_t)R.best_leaf].ec) R.best_leaf = uid;
            }
        }
    }
    return R;
}

static void same_search(const Search &a, const Search &b) {
    CHECK(a.state == b.state && a.best_leaf == b.best_leaf && same_bits(a.best, b.best));
    CHECK(a.fail_node == b.fail_node && a.fail_zone == b.fail_zone && a.fail_query == b.fail_query);
    CHECK(a.pruned == b.pruned && a.queries == b.queries && a.waves == b.waves);
    CHECK(a.nodes.size() == b.nodes.size());
    for (size_t k = 0; k < a.nodes.size() && k < b.nodes.size(); ++k) {
        const porrt_bnb::Node &x = a.nodes[k], &y = b.nodes[k];
        CHECK(x.parent == y.parent && x.target == y.target && x.remaining == y.remaining && x.pushed == y.pushed && x.status == y.status);
        CHECK(same_bits(x.ec, y.ec) && same_bits(x.rp, y.rp) && same_bits(x.ox, y.ox) && same_bits(x.oy, y.oy));
        CHECK(x.obs_off == y.obs_off && x.pick_off == y.pick_off && x.h == y.h);
    }
}

static void same_as_reference(const Search &s, const Ref &R) {
    CHECK(s.nodes.size() == R.nodes.size());
    CHECK(s.fail_node == R.fail_node && s.fail_zone == R.fail_zone && s.fail_query == R.fail_query);
    CHECK((s.state == Search::kFailed) == (R.fail_node >= 0));
    if (s.state == Search::kFailed) {
        CHECK(s.fail_node < (int64_t)s.nodes.size());            // the failing child is one of the wave's, which are all made
    } else {
        CHECK(s.best_leaf == R.best_leaf && s.pruned == R.pruned && s.queries == R.queries && s.waves == R.waves);
        CHECK((s.state == Search::kSolved) == (R.best_leaf >= 0) && (s.state == Search::kExhausted) == (R.best_leaf < 0));
    }
    for (size_t k = 0; k < s.nodes.size() && k < R.nodes.size(); ++k) {
        const porrt_bnb::Node &x = s.nodes[k];
        const RefNode &y = R.nodes[k];
        CHECK(x.parent == y.parent && x.target == y.target && x.remaining == y.remaining && x.h == y.h && same_bits(x.rp, y.rp));
        for (uint32_t w = 0; w < s.nw; ++w) CHECK(same_bits(s.belief_row(x.belief)[w], y.belief[w]));
        if (s.state != Search::kFailed) CHECK(same_bits(x.ec, y.ec) && x.pushed == y.pushed && x.obs_off == y.rec.obs_off);
    }
}

int main() {
    const uint32_t counts[] = {1, 2, 7}, widths[] = {1, 3, 64};
    const size_t chunks[] = {1, 5, 64};
    uint64_t failed_searches = 0, solved_searches = 0, solved_beside_failed = 0, pruned_total = 0, last_won = 0;
    for (Mode mode : {kHashed, kTies})
        for (uint32_t fail_one_in : {0u, 31u})
            for (uint32_t n : counts) {
                const std::vector<Problem> P = problems(n);
                for (uint32_t W : widths) {
                    std::vector<Search> alone = make(P);
                    std::vector<Ref> refs;
                    for (uint32_t p = 0; p < n; ++p) {
                        std::vector<Search> one{alone[p]};
                        drive(one, W, 1u << 20, mode, fail_one_in);
                        alone[p] = one[0];
                        CHECK(alone[p].state == Search::kSolved || alone[p].state == Search::kFailed);
                        refs.push_back(reference(P[p], W, mode, fail_one_in));
                        same_as_reference(alone[p], refs.back());
                        if (refs.back().fail_node < 0 && refs.back().equal_leaves) {
                            // leaves of bit-equal cost: the last one closed holds the policy, not the first
                            CHECK(alone[p].best_leaf == refs.back().best_leaf);
                            if (refs.back().best_leaf != refs.back().first_leaf) ++last_won;
                        }
                    }
                    for (size_t chunk : chunks) {
                        std::vector<Search> S = make(P);
                        size_t largest = 0;
                        drive(S, W, chunk, mode, fail_one_in, &largest);
                        CHECK(largest <= chunk);
                        bool any_failed = false;
                        for (uint32_t p = 0; p < n; ++p) {
                            same_search(S[p], alone[p]);
                            pruned_total += S[p].pruned;
                            if (S[p].state == Search::kFailed) { ++failed_searches; any_failed = true; }
                            if (S[p].state != Search::kSolved) continue;
                            ++solved_searches;
                            CHECK(S[p].chain().size() == S[p].nw + 1u && S[p].chain()[0] == 0 && S[p].fail_node == -1);
                            CHECK(S[p].nodes[(size_t)S[p].best_leaf].remaining.empty() && same_bits(S[p].nodes[(size_t)S[p].best_leaf].ec, S[p].best));
                        }
                        if (any_failed) for (uint32_t p = 0; p < n; ++p) if (S[p].state == Search::kSolved) ++solved_beside_failed;
                    }
                }
            }
    CHECK(solved_searches > 0 && failed_searches > 0 && solved_beside_failed > 0);
    CHECK(pruned_total > 0);
    CHECK(last_won > 0);                                         // somewhere the last of equal leaves was not the first

    // a plan of one zone: the root's only child is the leaf; one round expands something
    {
        std::vector<Problem> P{problem(0, 1)};
        for (uint32_t W : widths) {
            std::vector<Search> S = make(P);
            const uint64_t rounds = drive(S, W, 64, kHashed, 0);
            CHECK(rounds == 1 && S[0].state == Search::kSolved && S[0].nodes.size() == 2 && S[0].best_leaf == 1 && S[0].queries == 2 && S[0].waves == 2);
            same_as_reference(S[0], reference(P[0], W, kHashed, 0));
        }
    }
    // a prior with a zero entry is allowed: an order that leaves a zero zone for last has beliefs 0 / 0 at its leaf, whose cost is
    // NaN and never below the bound; the other orders are searched as the loop searches them
    {
        std::vector<Problem> P{problem(0, 4), problem(1, 4)};
        P[1].prior = {0.5, 0.0, 0.25, 0.25};
        for (uint32_t W : widths) {
            std::vector<Search> S = make(P);
            drive(S, W, 5, kHashed, 0);
            CHECK(S[0].state == Search::kSolved && S[1].state == Search::kSolved);
            bool nan_pruned = false;
            for (const porrt_bnb::Node &v : S[1].nodes) if (v.ec != v.ec) { nan_pruned = true; CHECK(!v.pushed); }
            CHECK(nan_pruned);
            same_as_reference(S[0], reference(P[0], W, kHashed, 0));
            same_as_reference(S[1], reference(P[1], W, kHashed, 0));
        }
    }
    if (failures) { std::fprintf(stderr, "bnb_search_check: %d failures\n", failures); return 1; }
    std::printf("bnb_search_check ok\n");
    return 0;
}
