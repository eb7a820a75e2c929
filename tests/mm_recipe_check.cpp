// mm_recipe_check.cpp -- the device-free arithmetic of porrt_mm_plan_batch (po_rrt_amd/csrc/porrt_mm_recipe.hpp) against plain loops:
// the recipe (codes + one stream prefix per plan + explicit points) expands to exactly the points a loop that draws per mode from a
// clone of the plan's sampler produces; the union of several plans (codes rebased as the engine rebases them) expands the same and
// its ids translate there and back; the pass cuts equal a loop's; bad codes are refused without a read.  A program of its own, built
// with -fsanitize=address,undefined by tests/test_mm_plan_batch_cpu.py: every array below has its exact size on the heap.
#include "../po_rrt_amd/csrc/porrt_mm_recipe.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace porrt;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// a copyable stream with redraws, standing in for the planner's sampler: what matters is that a clone repeats it
struct Stream {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double range(double lo, double hi) {
        for (;;) {
            const double v = lo + (hi - lo) * (double)(next() >> 11) * (1.0 / 9007199254740992.0);
            if ((next() & 7) == 0) continue;                     // a redraw now and then: part of the stream
            if (v < hi) return v;
        }
    }
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

struct Plain { std::vector<std::vector<double>> xy; };           // per mode, the points in add_sample order

// One plan of the shape of grow_mm_prm's loop: n_outer rounds of (a mode, 190 random points, up to 10 observation samples that go to
// the mode and to up to two destination modes, which are created on demand with or without a goal state of their own).  The plain
// loop draws per mode from a clone; the recipe records.
static void make_plan(uint64_t seed, size_t max_modes, size_t n_outer, Plain &plain, MmRecipe &rec, std::vector<double> &px, std::vector<double> &py) {
    const Stream planner{seed * 77 + 1};
    Stream pick{seed * 1315423911ull + 7}, zone{0};
    std::vector<Stream> clones;
    std::vector<std::vector<size_t>> dest;                       // per mode: its destination modes so far
    auto add_mode = [&]() { clones.push_back(planner); plain.xy.emplace_back(); dest.emplace_back(); rec.add_mode(); return clones.size() - 1; };
    auto add_explicit = [&](size_t m, uint32_t point, double x, double y) {
        plain.xy[m].push_back(x); plain.xy[m].push_back(y);
        CHECK(rec.add_explicit_node(m, point) == plain.xy[m].size() / 2 - 1);
    };
    add_mode();
    add_explicit(0, rec.add_point(0.25, -1.0), 0.25, -1.0);      // the planning start
    for (size_t i = 0; i < n_outer; ++i) {
        const size_t m = (size_t)(pick.next() % clones.size());
        for (int s = 0; s < 190; ++s) {
            const double x = clones[m].range(-1.0, 1.0), y = clones[m].range(-0.5, 0.75);
            plain.xy[m].push_back(x); plain.xy[m].push_back(y);
            CHECK(rec.add_random_node(m) == plain.xy[m].size() / 2 - 1);
        }
        for (int j = 0; j < 10; ++j) {
            if (pick.next() % 5 == 0) continue;
            while (dest[m].size() < 2 && clones.size() < max_modes && pick.next() % 3 != 0) {
                const size_t nm = add_mode();
                dest[m].push_back(nm);
                if (pick.next() % 2) { const double gx = zone.range(-1, 1), gy = zone.range(-1, 1); add_explicit(nm, rec.add_point(gx, gy), gx, gy); }
            }
            const double ox = zone.range(-1, 1), oy = zone.range(-1, 1);
            const uint32_t point = rec.add_point(ox, oy);
            add_explicit(m, point, ox, oy);
            for (size_t d : dest[m]) add_explicit(d, point, ox, oy);
        }
    }
    CHECK(!rec.overflow);
    Stream once = planner;                                        // the prefix: one draw for the whole plan
    const uint32_t L = rec.prefix_len();
    px.resize(L); py.resize(L);
    for (uint32_t k = 0; k < L; ++k) { px[k] = once.range(-1.0, 1.0); py[k] = once.range(-0.5, 0.75); }
}

struct PlanData { Plain plain; MmRecipe rec; std::vector<double> px, py; };

static void check_round_trip(PlanData &p, bool want_mode_without_random) {
    CHECK(p.rec.modes.size() == p.plain.xy.size());
    uint64_t nodes = 0;
    bool none = false;
    uint32_t longest = 0;
    for (size_t m = 0; m < p.rec.modes.size(); ++m) {
        const std::vector<uint32_t> &codes = p.rec.modes[m].codes;
        CHECK(codes.size() == p.plain.xy[m].size() / 2);
        none |= p.rec.modes[m].n_random == 0;
        longest = p.rec.modes[m].n_random > longest ? p.rec.modes[m].n_random : longest;
        for (size_t t = 0; t < codes.size(); ++t) {
            double x = 0, y = 0;
            CHECK(mm_recipe_point(codes[t], p.px.data(), p.py.data(), p.px.size(), p.rec.ex.data(), p.rec.ey.data(), p.rec.ex.size(), &x, &y));
            CHECK(same_bits(x, p.plain.xy[m][2 * t]) && same_bits(y, p.plain.xy[m][2 * t + 1]));
        }
        nodes += codes.size();
    }
    CHECK(nodes == p.rec.nodes() && longest == p.rec.prefix_len() && p.px.size() == longest);
    if (want_mode_without_random) CHECK(none);
    // codes one past either array are refused, and nothing is read (the arrays end exactly there)
    double x = 7, y = 7;
    CHECK(!mm_recipe_point(mm_code_random((uint32_t)p.px.size()), p.px.data(), p.py.data(), p.px.size(), p.rec.ex.data(), p.rec.ey.data(), p.rec.ex.size(), &x, &y));
    CHECK(!mm_recipe_point(mm_code_explicit((uint32_t)p.rec.ex.size()), p.px.data(), p.py.data(), p.px.size(), p.rec.ex.data(), p.rec.ey.data(), p.rec.ex.size(), &x, &y));
    CHECK(!mm_recipe_point(mm_code_explicit(kMmCodeIndexMask), p.px.data(), p.py.data(), p.px.size(), p.rec.ex.data(), p.rec.ey.data(), p.rec.ex.size(), &x, &y));
    CHECK(x == 7 && y == 7);
}

// the union of a pass as the engine lays it out: modes end to end, explicit codes rebased by the plan's first explicit point, every
// mode with its plan's prefix offset and length
static void check_union(std::vector<PlanData> &ps) {
    const uint32_t n = (uint32_t)ps.size();
    std::vector<uint64_t> noff(n + 1, 0);
    std::vector<uint32_t> seg{0}, pref_off, pref_len, codes, plan_of_mode;
    std::vector<double> px, py, ex, ey;
    for (uint32_t q = 0; q < n; ++q) {
        const uint64_t p0 = px.size(), e0 = ex.size();
        for (const MmRecipeMode &m : ps[q].rec.modes) {
            for (uint32_t c : m.codes) codes.push_back(mm_code_is_explicit(c) ? mm_code_explicit((uint32_t)(e0 + mm_code_index(c))) : c);
            seg.push_back((uint32_t)codes.size());
            pref_off.push_back((uint32_t)p0); pref_len.push_back((uint32_t)ps[q].px.size()); plan_of_mode.push_back(q);
        }
        px.insert(px.end(), ps[q].px.begin(), ps[q].px.end()); py.insert(py.end(), ps[q].py.begin(), ps[q].py.end());
        ex.insert(ex.end(), ps[q].rec.ex.begin(), ps[q].rec.ex.end()); ey.insert(ey.end(), ps[q].rec.ey.begin(), ps[q].rec.ey.end());
        noff[q + 1] = codes.size();
    }
    size_t mode = 0;
    for (uint64_t i = 0; i < codes.size(); ++i) {
        while (seg[mode + 1] <= i) ++mode;                        // the plain way to a node's mode
        const uint32_t q = plan_of_mode[mode];
        CHECK(mm_plan_of(noff.data(), n, i) == q);
        const uint64_t own = mm_own_id(noff[q], i);
        CHECK(own < ps[q].rec.nodes() && mm_union_id(noff[q], own) == i);
        // the plan's own id back to (mode, node) of the plan, by a loop
        uint64_t at = 0;
        size_t pm = 0;
        while (at + ps[q].rec.modes[pm].codes.size() <= own) at += ps[q].rec.modes[pm++].codes.size();
        const size_t t = (size_t)(own - at);
        double x = 0, y = 0;
        const uint32_t k = mm_code_index(codes[i]);
        if (mm_code_is_explicit(codes[i])) { CHECK(k < ex.size()); x = ex[k]; y = ey[k]; }
        else { CHECK(k < pref_len[mode] && (uint64_t)pref_off[mode] + k < px.size()); x = px[pref_off[mode] + k]; y = py[pref_off[mode] + k]; }
        CHECK(same_bits(x, ps[q].plain.xy[pm][2 * t]) && same_bits(y, ps[q].plain.xy[pm][2 * t + 1]));
    }
    // plans without nodes are stepped over
    const uint64_t off[] = {0, 0, 5, 5, 5, 9};
    const uint32_t want[] = {1, 1, 1, 1, 1, 4, 4, 4, 4};
    for (uint64_t i = 0; i < 9; ++i) CHECK(mm_plan_of(off, 5, i) == want[i]);
}

static void check_pass_cuts() {
    Stream r{42};
    for (int round = 0; round < 2000; ++round) {
        const uint32_t n = 1 + (uint32_t)(r.next() % 12);
        std::vector<uint64_t> nodes(n);
        for (uint64_t &v : nodes) v = r.next() % 4 == 0 ? 0 : r.next() % 5000;
        if (round % 7 == 0) nodes[r.next() % n] = 20000;                                        // a plan larger than the bound
        if (round % 97 == 0) nodes[r.next() % n] = ~0ull - 3;                                   // sums that would wrap
        const uint64_t bound = round % 11 == 0 ? 1 : round % 13 == 0 ? ~0ull : 1 + r.next() % 9000;
        const uint64_t limit = bound < kMmBatchNodesLimit ? bound : kMmBatchNodesLimit;
        uint32_t covered = 0;
        for (uint32_t first = 0; first < n;) {
            const uint32_t end = mm_pass_end(nodes.data(), n, first, bound);
            CHECK(end > first && end <= n);
            unsigned __int128 sum = 0;
            for (uint32_t q = first; q < end; ++q) sum += nodes[q];
            CHECK(sum <= limit || end == first + 1);                                             // within the bound, or one plan alone
            if (end < n) CHECK(sum + nodes[end] > limit);                                        // and the next plan would not have fitted
            covered += end - first;
            first = end;
        }
        CHECK(covered == n);
    }
    const uint64_t four[] = {3000, 3100, 3050, 3200};
    CHECK(mm_pass_end(four, 4, 0, 1) == 1 && mm_pass_end(four, 4, 3, 1) == 4);
    CHECK(mm_pass_end(four, 4, 0, 6100) == 2 && mm_pass_end(four, 4, 2, 6250) == 4);
    CHECK(mm_pass_end(four, 4, 0, kMmBatchNodesDefault) == 4);
}

int main() {
    // the three seeded shapes of the GPU tests: three modes of about a thousand nodes; fifteen modes, tens of thousands of nodes; more
    // than a thousand modes, most of them smaller than a wave and some without a random point
    struct Shape { size_t max_modes, n_outer; bool none; } shapes[3] = {{3, 15, false}, {15, 150, false}, {1364, 60, true}};
    for (const Shape &sh : shapes) {
        std::vector<PlanData> ps(3);
        for (size_t q = 0; q < ps.size(); ++q) {
            make_plan(1000 * sh.max_modes + q, sh.max_modes, sh.n_outer, ps[q].plain, ps[q].rec, ps[q].px, ps[q].py);
            check_round_trip(ps[q], sh.none);
        }
        check_union(ps);
    }
    check_pass_cuts();
    CHECK(mm_code_index(mm_code_explicit(5)) == 5 && mm_code_is_explicit(mm_code_explicit(0)) && !mm_code_is_explicit(mm_code_random(kMmCodeIndexMask)));
    std::printf("mm_recipe_check ok\n");
    return 0;
}
