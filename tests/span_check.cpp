// The index arithmetic of the flat rewire commit (po_rrt_amd/csrc/porrt_span.hpp) against plain loops, on the host.
// The device's first wave builds the prefix with a shuffle scan over its 64 lanes; here the same network runs over an array.
// Exit status 0 and "span_check ok" when every case agrees; built with -fsanitize=address,undefined by tests/test_span_arithmetic_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../po_rrt_amd/csrc/porrt_span.hpp"

using namespace porrt;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures++ < 20) std::fprintf(stderr, "span_check: line %d: %s\n", __LINE__, #c); } } while (0)

// rank_before of porrt_device.hpp, as a loop over bits
static uint32_t rank_loop(const std::vector<unsigned long long> &vm, uint32_t k) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < k; ++i) r += (uint32_t)((vm[i >> 6] >> (i & 63u)) & 1ull);
    return r;
}

// one row's step: K sample slots, `limit` of them run by the row, stored counts and valid bits as given
static void check_step(uint32_t K, uint32_t limit, uint32_t cap, const std::vector<uint32_t> &stored, const std::vector<unsigned long long> &vm) {
    const uint32_t vwords = (K + 63u) / 64u;
    for (uint32_t k0 = 0; k0 < K; k0 += kSpan) {
        if (k0 >= limit) break;                                  // the workgroup returns
        unsigned long long words[kSpanWords];
        for (uint32_t w = 0; w < kSpanWords; ++w) {
            const uint32_t wi = (k0 >> 6) + w;
            words[w] = wi < vwords ? vm[wi] : 0ull;
        }
        // the first wave: lane sums, inclusive scan by the shuffle network, the lanes' parts of the prefix
        std::vector<uint32_t> prefix(kSpan + 1u, 0xDEADBEEFu);
        uint32_t c[64][kSpanPer], s[64], incl[64];
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            s[lane] = 0;
            for (uint32_t u = 0; u < kSpanPer; ++u) {
                const uint32_t t = lane * kSpanPer + u, k = k0 + t;
                const uint32_t st = k < limit ? stored[k] : 0u;
                c[lane][u] = span_count(st, cap, span_valid(words, t), k, limit);
                s[lane] += c[lane][u];
            }
            incl[lane] = s[lane];
        }
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            uint32_t v[64];
            for (uint32_t lane = 0; lane < 64u; ++lane) v[lane] = lane >= off ? incl[lane - off] : incl[lane];
            for (uint32_t lane = 0; lane < 64u; ++lane) if (lane >= off) incl[lane] += v[lane];
        }
        for (uint32_t lane = 0; lane < 64u; ++lane) span_prefix_lane(prefix.data(), lane, c[lane], incl[lane] - s[lane]);
        // the plain loop
        std::vector<uint32_t> want_cnt(kSpan, 0u);
        uint32_t run = 0;
        for (uint32_t t = 0; t < kSpan; ++t) {
            const uint32_t k = k0 + t;
            const bool valid = k < K && ((vm[k >> 6] >> (k & 63u)) & 1ull);
            if (k < limit && valid) want_cnt[t] = stored[k] < cap ? stored[k] : cap;
            CHECK(prefix[t] == run);
            run += want_cnt[t];
            if (k < limit && valid) CHECK(rank_loop(vm, k0) + span_rank_in(words, t) == rank_loop(vm, k));
        }
        CHECK(prefix[kSpan] == run);
        CHECK(run <= kSpan * cap);
        // every record finds its sample, and its place in the sample's list lies below the clamped count
        uint32_t r = 0;
        for (uint32_t t = 0; t < kSpan; ++t)
            for (uint32_t a = 0; a < want_cnt[t]; ++a, ++r) {
                const uint32_t f = span_find(prefix.data(), r);
                CHECK(f == t);
                CHECK(f < kSpan && r - prefix[f] == a && a < cap && k0 + f < limit);
            }
        CHECK(r == run);
    }
}

int main() {
    std::mt19937_64 rng(20241);
    const uint32_t Ks[] = {64u, 100u, 128u, 192u, 512u, 1024u, 4096u};
    for (uint32_t K : Ks) {
        const uint32_t vwords = (K + 63u) / 64u;
        for (int rep = 0; rep < 24; ++rep) {
            const uint32_t cap = rep % 3 == 0 ? 64u : (rep % 3 == 1 ? 512u : 7u);
            // the row's own end of the step: the whole step, cut inside a span, cut on a span's edge, three samples, none
            uint32_t limit = K;
            if (rep % 6 == 1) limit = (uint32_t)(rng() % (K + 1u));
            if (rep % 6 == 2) limit = K >= kSpan ? kSpan : K;
            if (rep % 6 == 3) limit = 3u < K ? 3u : K;
            if (rep % 6 == 4) limit = 0u;
            std::vector<uint32_t> stored(K);
            std::vector<unsigned long long> vm(vwords, 0ull);
            for (uint32_t k = 0; k < K; ++k) {
                const unsigned mode = rep < 4 ? (unsigned)rep : (unsigned)(rng() % 6u);
                uint32_t v;
                if (mode == 0) v = 0u;                                     // no records
                else if (mode == 1) v = cap;                               // at the cap
                else if (mode == 2) v = cap + 1u + (uint32_t)(rng() % 1000u);      // an overflowed list: clamped
                else if (mode == 3) v = 0xFFFFFFFFu - (uint32_t)(rng() % 3u);      // garbage must not become an address
                else v = (uint32_t)(rng() % 9u);                           // a grown tree's few
                stored[k] = v;
                // (valid bits whatever the row's own end: one at or beyond it must still count no records -- and no rank below the end sees it)
                if (rng() % 8u != 0u) vm[k >> 6] |= 1ull << (k & 63u);
            }
            if (rep == 5) for (auto &w : vm) w = 0ull;                     // a step without a valid sample
            check_step(K, limit, cap, stored, vm);
        }
    }
    if (failures) { std::fprintf(stderr, "span_check: %d failures\n", failures); return 1; }
    std::puts("span_check ok");
    return 0;
}
