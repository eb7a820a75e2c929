// porrt_span.hpp -- index arithmetic of the flat rewire commit (k_nn2's commit role and k_commit_flat, porrt_group.hpp).
//
// A commit workgroup takes a span of kSpan consecutive samples of its row and runs one lane per candidate RECORD of the span:
// record r belongs to the sample k with prefix[k] <= r < prefix[k + 1], prefix being the exclusive prefix sum of the samples'
// clamped candidate counts.  What is in here is plain integer arithmetic, the same for the device and for a host program that
// checks it against a loop (tests/span_check.cpp); nothing in it touches memory other than the arrays it is handed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PORRT_HD __host__ __device__ inline
#else
#define PORRT_HD inline
#endif

namespace porrt {

constexpr uint32_t kSpan = 128u;                  // samples per commit workgroup: a power of two, a multiple of 64 (whole valid words)
constexpr uint32_t kSpanWords = kSpan / 64u;
constexpr uint32_t kSpanPer = kSpan / 64u;        // samples per lane of the wave that builds the prefix
static_assert((kSpan & (kSpan - 1u)) == 0u && kSpan % 64u == 0u, "kSpan");

// candidate records of a sample, as commit_rrt_sample sees them: the stored count clamped to the list's capacity (cand_count), none
// for a sample without its valid bit or at or beyond the row's own end of the step (row_nb)
PORRT_HD uint32_t span_count(uint32_t stored, uint32_t cap, bool valid, uint32_t k, uint32_t limit) {
    if (k >= limit || !valid) return 0u;
    return stored < cap ? stored : cap;
}

// valid bit of the span's sample t (words: the kSpanWords words of the step's valid mask that cover the span)
PORRT_HD bool span_valid(const unsigned long long *words, uint32_t t) { return (words[t >> 6] >> (t & 63u)) & 1ull; }

// valid samples of the span before its sample t: with the valid samples before the span (rank_before of the span's first sample)
// the number rank_before returns for the sample
PORRT_HD uint32_t span_rank_in(const unsigned long long *words, uint32_t t) {
    uint32_t r = 0;
    for (uint32_t w = 0; w < kSpanWords; ++w) {
        if (w < (t >> 6)) r += (uint32_t)__builtin_popcountll(words[w]);
        else if (w == (t >> 6)) r += (uint32_t)__builtin_popcountll(words[w] & ((1ull << (t & 63u)) - 1ull));
    }
    return r;
}

// One lane's part of the prefix: the lane holds the counts of samples lane * kSpanPer .. + kSpanPer - 1 and `excl`, the sum of the
// counts of all samples before them (an exclusive scan of the lanes' sums); lane 63 also writes the total.
PORRT_HD void span_prefix_lane(uint32_t *prefix, uint32_t lane, const uint32_t *cnt, uint32_t excl) {
    for (uint32_t u = 0; u < kSpanPer; ++u) {
        prefix[lane * kSpanPer + u] = excl;
        excl += cnt[u];
    }
    if (lane == 63u) prefix[kSpan] = excl;
}

// sample of record r < prefix[kSpan]: the largest k < kSpan with prefix[k] <= r (samples without records are stepped over: their
// prefix equals their successor's).  log2(kSpan) trips whatever the counts are.
PORRT_HD uint32_t span_find(const uint32_t *prefix, uint32_t r) {
    uint32_t k = 0;
    for (uint32_t step = kSpan >> 1; step >= 1u; step >>= 1)
        if (prefix[k + step] <= r) k += step;
    return k;
}

} // namespace porrt
