// The open list of the TAMP-RRT A* search (po_rrt_amd/csrc/porrt_astar_queue.hpp) against a stable sort, on the host.
// Exit status 0 and "astar_queue_check ok" when every case agrees; built with -fsanitize=address,undefined by
// tests/test_tamp_astar_cpu.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../po_rrt_amd/csrc/porrt_astar_queue.hpp"

using porrt_astar::Queue;
using porrt_astar::QueueEntry;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 20) std::fprintf(stderr, "astar_queue_check: line %d: %s\n", __LINE__, #c); } } while (0)

// the stated order without the heap: entries in ascending id, then a STABLE sort by priority alone
static std::vector<QueueEntry> sorted(std::vector<QueueEntry> v) {
    std::sort(v.begin(), v.end(), [](const QueueEntry &a, const QueueEntry &b) { return a.id < b.id; });
    std::stable_sort(v.begin(), v.end(), [](const QueueEntry &a, const QueueEntry &b) { return a.priority < b.priority; });
    return v;
}

static bool same(const QueueEntry &a, const QueueEntry &b) { return a.id == b.id && a.priority == b.priority; }

static double draw_priority(std::mt19937_64 &rng, uint32_t distinct) {
    const double inf = std::numeric_limits<double>::infinity();
    const uint32_t k = (uint32_t)(rng() % (distinct + 3u));
    if (k == distinct) return 0.0;
    if (k == distinct + 1u) return -0.0;
    if (k == distinct + 2u) return inf;
    return 0.25 * (double)k;                      // few distinct values: many bit-equal priorities
}

// all pushes, then all pops
static void check_bulk(uint64_t seed, size_t n, uint32_t distinct) {
    std::mt19937_64 rng(seed);
    std::vector<QueueEntry> all;
    std::vector<uint64_t> ids(n);
    for (size_t i = 0; i < n; ++i) ids[i] = i;
    std::shuffle(ids.begin(), ids.end(), rng);    // the order of the pushes must not matter
    Queue q;
    for (size_t i = 0; i < n; ++i) {
        const QueueEntry e{draw_priority(rng, distinct), ids[i]};
        all.push_back(e);
        q.push(e.priority, e.id);
    }
    CHECK(q.size() == n);
    const std::vector<QueueEntry> want = sorted(all);
    for (size_t i = 0; i < n; ++i) {
        CHECK(!q.empty());
        CHECK(same(q.top(), want[i]));
        const QueueEntry got = q.pop();
        CHECK(same(got, want[i]));
    }
    CHECK(q.empty());
}

// pops between the pushes: the model is a vector that is searched for its minimum
static void check_interleaved(uint64_t seed, size_t steps, uint32_t distinct) {
    std::mt19937_64 rng(seed);
    Queue q;
    std::vector<QueueEntry> model;
    uint64_t next_id = 0;
    for (size_t s = 0; s < steps; ++s) {
        const bool push = model.empty() || (rng() % 3u) != 0u;
        if (push) {
            const uint32_t burst = 1u + (uint32_t)(rng() % 4u);
            for (uint32_t b = 0; b < burst; ++b) {
                const QueueEntry e{draw_priority(rng, distinct), next_id++};
                model.push_back(e);
                q.push(e.priority, e.id);
            }
        } else {
            const std::vector<QueueEntry> want = sorted(model);
            const QueueEntry got = q.pop();
            CHECK(same(got, want[0]));
            for (size_t i = 0; i < model.size(); ++i)
                if (model[i].id == want[0].id) { model.erase(model.begin() + (long)i); break; }
        }
        CHECK(q.size() == model.size());
    }
    const std::vector<QueueEntry> want = sorted(model);
    for (const QueueEntry &w : want) CHECK(same(q.pop(), w));
    CHECK(q.empty());
}

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    {   // the zeros are equal: the id decides, whichever sign came first
        Queue q;
        q.push(-0.0, 5); q.push(0.0, 2); q.push(-0.0, 9); q.push(0.0, 7); q.push(-1.0, 11); q.push(inf, 1); q.push(inf, 0); q.push(1e300, 3);
        const uint64_t want[] = {11, 2, 5, 7, 9, 3, 0, 1};
        for (uint64_t w : want) CHECK(q.pop().id == w);
        CHECK(q.empty());
        q.push(0.0, 4); q.push(-0.0, 3);
        CHECK(std::signbit(q.top().priority) && q.top().id == 3);
        q.clear();
        CHECK(q.empty() && q.size() == 0);
    }
    {   // one entry, and a queue that is emptied and used again
        Queue q;
        q.push(2.5, 0);
        CHECK(q.pop().id == 0 && q.empty());
        q.push(1.0, 2); q.push(1.0, 1);
        CHECK(q.pop().id == 1 && q.pop().id == 2 && q.empty());
    }
    for (uint64_t seed = 0; seed < 40; ++seed) {
        check_bulk(seed, 1 + (size_t)(seed * 37 % 700), 1u + (uint32_t)(seed % 6));
        check_interleaved(1000 + seed, 600, 1u + (uint32_t)(seed % 5));
    }
    check_bulk(77, 5000, 3);
    if (failures) { std::fprintf(stderr, "astar_queue_check: %d failures\n", failures); return 1; }
    std::printf("astar_queue_check ok\n");
    return 0;
}
