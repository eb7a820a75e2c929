// porrt_refine_batch.hpp -- refine_solution(PartialShortCut(n)) (specified in porrt_refine.hpp) of one policy or many in one call:
// decomposition, shortcuts, recomposition and expected costs on the device (porrt_bg_refine_policies / porrt_mm_refine_policies /
// porrt_refine_policies; porrt_bg_refine_policy / porrt_mm_refine_policy / porrt_refine_policy are batches of one).
//
// The policies lie end to end: policy q is rows pol_off[q] .. pol_off[q + 1] of the node arrays, parents index into the policy.
// Every work array is indexed the same way (a policy works in its own rows of global scratch, so its size is bounded by memory
// alone); a policy's long pieces go to rows pol_off[q] / 3 .. of the long-piece arrays (it has at most a third of its nodes of them).
//
//   k_refine_policies_decompose   one wave per policy.  Child counts (integer atomics), sibling lists in ascending id order, then lane 0
//                                 walks Policy::decompose (common.rs:85-129): pieces in FIFO order, the piece table doubling as the
//                                 FIFO (entry i holds its start node and the row its start hangs from until piece i is laid out).
//                                 It writes, per refined row, the policy node it came from, its parent (recompose :324-393 with the
//                                 `if is_start .. else if is_end` quirk: the successors of a one-node piece get no parent) and its
//                                 leaf flag; per piece offset, length and successors; per piece of >= 3 nodes a RefinePolPiece and
//                                 its length (the host makes one table of draws per distinct length from those).  A piece whose
//                                 nodes carry different beliefs makes the policy status 3.  The lanes then gather the states.
//   k_refine_policies_shortcut    refine_shortcut_piece (porrt_refine.hpp) per piece of >= 3 nodes of every policy, longest first;
//                                 a raster fault is OR-ed into the owning policy's word and the other pieces run on.
//   k_refine_policies_offsets     one workgroup: final status per policy, ref_off = running sum of the surviving policies' rows.
//   k_refine_policies_recompose   one wave per policy: the rows go out packed (original ids through the row -> node map); the
//                                 lanes compute every edge's transition probability and length, lane 0 the expected cost
//                                 (common.rs:131-154) in the order of the reference's recursion: p from the root down, then the
//                                 pieces last to first, each folding its successors' starts in ascending order from 0.0 and
//                                 walking up to its own start.  (A parent's id is below its children's in the recomposed layout;
//                                 only a branching end has more than one child, and those are the starts of consecutive pieces.)
#pragma once
#include "porrt_refine.hpp"
#include "porrt_host.hpp"
#include <functional>

namespace porrt {

constexpr uint32_t kRefineShortLdsNodes = 256;   // the short-piece instantiation: 2 x 2 KiB per wave
constexpr uint32_t kRefNone = 0xFFFFFFFFu;

struct RefinePolPiece {
    uint32_t off;            // first state of the piece in x / y (a row of the whole batch)
    uint32_t len;            // nodes (>= 3)
    uint32_t draws;          // first draw of its length (filled in from the launch entry)
    uint32_t belief;         // row of compat
    uint32_t policy;         // the policy whose fault word it reports to
};

struct RefinePolAny {        // every piece of a policy, at row pol_off[q] + i
    uint32_t off;            // first refined row within the policy (before the piece is laid out: its start node)
    int32_t hang;            // refined row its start hangs from, -1: none (the root, or the one-node quirk)
    uint32_t len;
    uint32_t succ0, nsucc;   // the pieces its last node's children start (consecutive)
};

struct RefinePolRecord { uint32_t rows, pieces, longs, status; };

struct RefinePolConst {
    // in
    const unsigned long long *pol_off;   // [n + 1]
    const double *in_xy;                 // 2 per node
    const unsigned long long *in_orig;
    const int32_t *in_parent;            // within the policy, -1 for its node 0
    const uint32_t *in_belief;           // belief row per node
    const double *beliefs;               // [rows][nw]
    uint32_t nw, n_policies;
    // work
    uint2 *link;                         // per node: (children, first child)
    uint32_t *next;                      // next sibling
    uint32_t *src;                       // refined row -> policy node
    int32_t *par;                        // refined row -> parent row within the policy
    uint8_t *leaf;
    RefinePolAny *any;
    RefinePolPiece *longs;               // [total / 3 + 1]
    uint32_t *long_len;                  //   their lengths alone (downloaded)
    RefinePolRecord *rec;                // per policy (downloaded)
    double *x, *y;                       // piece states, refined in place
    double *wq, *wt, *wp, *wv;           // per refined row: transition probability, length then term, p, value
    uint32_t *pol_err;                   // per policy: ERR_RASTER of its shortcuts
    // out (packed)
    unsigned long long *ref_off;         // [n + 1]
    double *cost;
    uint8_t *status;
    double *out_xy;
    unsigned long long *out_orig;
    long long *out_parent;
    uint8_t *out_leaf;
};

__global__ __launch_bounds__(64) void k_refine_policies_decompose(RefinePolConst c) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint64_t base = c.pol_off[q];
    const uint32_t n = (uint32_t)(c.pol_off[q + 1] - base);
    if (lane == 0) c.pol_err[q] = 0u;
    if (n == 0) {                                                    // no policy to refine
        if (lane == 0) c.rec[q] = RefinePolRecord{0u, 0u, 0u, 1u};
        return;
    }
    uint2 *link = c.link + base;
    uint32_t *next = c.next + base, *src = c.src + base;
    const int32_t *parent = c.in_parent + base;
    const uint32_t *belief = c.in_belief + base;
    for (uint32_t k = lane; k < n; k += 64) { link[k] = make_uint2(0u, kRefNone); next[k] = kRefNone; }
    __syncthreads();
    for (uint32_t k = 1 + lane; k < n; k += 64) atomicAdd(&link[parent[k]].x, 1u);
    __syncthreads();
    // first child / next sibling in ascending id order: an only child links itself; the children of a branching node are pushed on
    // their parent's list from the highest id down, by lane 0 alone (64 candidates found per pass)
    for (uint32_t top = n; top > 1;) {
        const uint32_t lo = top > 65 ? top - 64 : 1;                 // nodes lo .. top - 1, lane l takes top - 1 - l
        const uint32_t k = top - 1 - lane;
        const bool mine = lane < top - lo;
        const uint32_t p = mine ? (uint32_t)parent[k] : 0u;
        const uint32_t nc = mine ? link[p].x : 0u;
        if (mine && nc == 1u) link[p].y = k;
        unsigned long long multi = __ballot(mine && nc >= 2u);
        while (multi) {
            const int l = __ffsll((long long)multi) - 1;             // lowest lane first: the highest id
            multi &= multi - 1ull;
            const uint32_t kk = (uint32_t)__shfl((int)k, l), pp = (uint32_t)__shfl((int)p, l);
            if (lane == 0) { next[kk] = link[pp].y; link[pp].y = kk; }
        }
        top = lo;
    }
    __syncthreads();
    if (lane == 0) {
        RefinePolAny *any = c.any + base;
        int32_t *par = c.par + base;
        uint8_t *leaf = c.leaf + base;
        RefinePolPiece *longs = c.longs + base / 3;
        uint32_t *long_len = c.long_len + base / 3;
        uint32_t n_pieces = 1, rows = 0, n_long = 0, status = 0;
        any[0].off = 0u; any[0].hang = -1;
        for (uint32_t i = 0; i < n_pieces; ++i) {
            uint32_t cur = any[i].off;
            const int32_t hang = any[i].hang;
            const uint32_t r0 = rows, b0 = belief[cur];
            uint32_t len = 0, succ0 = 0, nsucc = 0;
            for (;;) {
                const uint2 lk = link[cur];
                const uint32_t b = belief[cur];
                if (b != b0) {                                       // decompose's assert_eq! on the beliefs along a piece
                    bool same = true;
                    for (uint32_t w = 0; w < c.nw; ++w)
                        same = same && __double_as_longlong(c.beliefs[(size_t)b * c.nw + w]) == __double_as_longlong(c.beliefs[(size_t)b0 * c.nw + w]);
                    if (!same) status = 3u;
                }
                src[rows] = cur;
                par[rows] = len == 0 ? hang : (int32_t)rows - 1;
                ++rows; ++len;
                if (lk.x == 1u) { leaf[rows - 1] = 0; cur = lk.y; continue; }       // simple forward
                leaf[rows - 1] = (lk.x == 0u || len == 1u) ? 1 : 0;  // final node; a one-node piece that branches gets no edges
                if (lk.x >= 2u) {                                    // branching: its children start the next pieces, in order
                    succ0 = n_pieces;
                    const int32_t end = len >= 2u ? (int32_t)rows - 1 : -1;
                    for (uint32_t ch = lk.y; ch != kRefNone; ch = next[ch]) { any[n_pieces].off = ch; any[n_pieces].hang = end; ++n_pieces; }
                    nsucc = n_pieces - succ0;
                }
                break;
            }
            any[i].off = r0; any[i].len = len; any[i].succ0 = succ0; any[i].nsucc = nsucc;
            if (len >= 3u) {
                longs[n_long] = RefinePolPiece{(uint32_t)base + r0, len, 0u, b0, q};
                long_len[n_long] = len;
                ++n_long;
            }
        }
        c.rec[q] = RefinePolRecord{rows, n_pieces, status ? 0u : n_long, status};
    }
    __syncthreads();
    const uint32_t rows = c.rec[q].rows;
    for (uint32_t r = lane; r < rows; r += 64) {                     // build_path_piece: the states in piece order
        const uint32_t k = src[r];
        c.x[base + r] = c.in_xy[2 * (base + k)];
        c.y[base + r] = c.in_xy[2 * (base + k) + 1];
    }
}

struct RefinePolLaunch {
    RefineConst rc;                      // raster, draws, compat, x / y, n_iter (pieces and err unused)
    const RefinePolPiece *longs;
    const uint2 *order;                  // per workgroup: (row of longs, first draw of its length), longest piece first
    uint32_t *pol_err;
    uint32_t first;                      // first entry of order this launch takes
};

template <uint32_t kLds>
__global__ __launch_bounds__(64) void k_refine_policies_shortcut(RefinePolLaunch c) {
    const uint2 e = c.order[c.first + blockIdx.x];
    RefinePolPiece pc = c.longs[e.x];
    pc.draws = e.y;
    refine_shortcut_piece<false, kLds>(c.rc, pc, c.pol_err + pc.policy);
}

// status: what the decomposition found, else 2 when a shortcut of the policy met a raster fault; ref_off: the survivors packed
__global__ __launch_bounds__(256) void k_refine_policies_offsets(RefinePolConst c) {
    __shared__ unsigned long long part[256];
    __shared__ unsigned long long carry;
    const uint32_t t = threadIdx.x;
    if (t == 0) { carry = 0ull; c.ref_off[0] = 0ull; }
    __syncthreads();
    for (uint32_t q0 = 0; q0 < c.n_policies; q0 += 256) {
        const uint32_t q = q0 + t;
        unsigned long long v = 0ull;
        if (q < c.n_policies) {
            const RefinePolRecord r = c.rec[q];
            const uint32_t st = r.status ? r.status : (c.pol_err[q] ? 2u : 0u);
            c.status[q] = (uint8_t)st;
            v = st ? 0ull : r.rows;
        }
        part[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const unsigned long long add = t >= d ? part[t - d] : 0ull;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        if (q < c.n_policies) c.ref_off[q + 1] = carry + part[t];
        __syncthreads();
        if (t == 255) carry += part[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_refine_policies_recompose(RefinePolConst c) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    if (c.status[q]) {
        if (lane == 0) c.cost[q] = 0.0;
        return;
    }
    const uint64_t base = c.pol_off[q], ob = c.ref_off[q];
    const RefinePolRecord rec = c.rec[q];
    const uint32_t *src = c.src + base;
    const int32_t *par = c.par + base;
    double *wq = c.wq + base, *wt = c.wt + base, *wp = c.wp + base, *wv = c.wv + base;
    for (uint32_t r = lane; r < rec.rows; r += 64) {
        const double x = c.x[base + r], y = c.y[base + r];
        const uint32_t k = src[r];
        const int32_t p = par[r];
        c.out_xy[2 * (ob + r)] = x; c.out_xy[2 * (ob + r) + 1] = y;
        c.out_orig[ob + r] = c.in_orig[base + k];
        c.out_parent[ob + r] = (long long)p;
        c.out_leaf[ob + r] = c.leaf[base + r];
        double qv = 0.0, d = 0.0;
        if (p >= 0) {
            const double *pb = c.beliefs + (size_t)c.in_belief[base + src[p]] * c.nw, *cb = c.beliefs + (size_t)c.in_belief[base + k] * c.nw;
            for (uint32_t w = 0; w < c.nw; ++w) qv = qv + (cb[w] > 0.0 ? pb[w] : 0.0);       // transition_probability (common.rs:187-190)
            double dx = x - c.x[base + p], d2 = 0.0;                                          // norm2 (pto_graph.rs:150)
            d2 += dx * dx;
            dx = y - c.y[base + p];
            d2 += dx * dx;
            d = sqrt(d2);
        }
        wq[r] = qv; wt[r] = d;
    }
    __syncthreads();
    if (lane != 0) return;
    const RefinePolAny *any = c.any + base;
    for (uint32_t i = 0; i < rec.pieces; ++i) {                      // p of every row and the term of the edge into it
        const RefinePolAny a = any[i];
        const int32_t hang = par[a.off];
        double p = 1.0;
        if (hang >= 0) { p = wp[hang] * wq[a.off]; wt[a.off] = p * wt[a.off]; }
        wp[a.off] = p;
        for (uint32_t r = a.off + 1; r < a.off + a.len; ++r) {
            p = p * wq[r];
            wt[r] = p * wt[r];
            wp[r] = p;
        }
    }
    for (uint32_t i = rec.pieces; i-- > 0;) {                        // a node's value: acc += term + ret(child) over its children in order
        const RefinePolAny a = any[i];
        double acc = 0.0;
        if (a.len >= 2u)
            for (uint32_t s = a.succ0; s < a.succ0 + a.nsucc; ++s) {
                const uint32_t rs = any[s].off;
                acc += wt[rs] + wv[rs];
            }
        for (uint32_t r = a.off + a.len - 1; r > a.off; --r) {
            const double below = wt[r] + acc;
            acc = 0.0;
            acc += below;
        }
        wv[a.off] = acc;
    }
    c.cost[q] = wv[0];
}

// ------------------------------------------------------------------------------------------------ host side

// The policies in, laid end to end as above: node k has state xy[2k..], parent parents[k] within its policy (-1 for its row 0, the root;
// children in ascending id order), original id original[k] (passed through) and belief row belief[k] of beliefs (n_rows x nw) with
// compatibility bits compat[row].
struct RefinePoliciesIn {
    uint64_t n;
    const uint64_t *pol_off;                                         // [n + 1]
    const double *xy; const int64_t *parents; const uint64_t *original; const uint32_t *belief;     // per node
    const double *beliefs; uint32_t n_rows, nw; const unsigned long long *compat;                  // per belief row
};
// The answers out: per policy ref_off, status and expected cost; the four node arrays are filled when cap holds the total.
struct RefinePoliciesOut {
    uint64_t *ref_off; uint8_t *status; double *cost;
    double *xy; uint64_t *original; int64_t *parents; uint8_t *leaf; uint64_t cap;
};
// What the refiner keeps between calls.
struct RefineHost {
    GrowScratch scratch;                             // slot 0: raster, slots 2-4: a call's uploads, draws and answers
    hipEvent_t ev[2] = {nullptr, nullptr};           // around a call's shortcut launches (the TAMP shortcut's too, porrt_tamp.hpp)
    std::vector<uint8_t> stage;
    uint64_t raster_gen = 0;                         // the raster slot 0 holds (0 = none)
    hipError_t events() { hipError_t e = hipSuccess; for (int k = 0; k < 2 && e == hipSuccess; ++k) if (!ev[k]) e = hipEventCreate(&ev[k]); return e; }
    hipEvent_t rp_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};     // between the stages of a Reparent round (porrt_reparent.hpp; slots 5-9 are its)
    hipError_t rp_events() { hipError_t e = hipSuccess; for (int k = 0; k < 5 && e == hipSuccess; ++k) if (!rp_ev[k]) e = hipEventCreate(&rp_ev[k]); return e; }
    void free_device() {
        scratch.free_all();
        for (int k = 0; k < 2; ++k) { if (ev[k]) (void)hipEventDestroy(ev[k]); ev[k] = nullptr; }
        for (int k = 0; k < 5; ++k) { if (rp_ev[k]) (void)hipEventDestroy(rp_ev[k]); rp_ev[k] = nullptr; }
    }
};

// partial_shortcut's draws for a piece of len >= 3 nodes: DiscreteSampler::new() (Pcg64, seed 0), then per iteration
// (s | joint << 31, e) (pto_policy_refiner.rs:172-175; the TAMP planner's shortcut draws the same sequence, map_shelves_tamp_rrt.rs:576-584)
static void shortcut_draws(uint64_t len, uint64_t n_iter, uint2 *out) {
    Pcg64 rng;
    rng.seed_from_u64(0);
    for (uint64_t it = 0; it < n_iter; ++it) {
        const uint32_t joint = (uint32_t)rng.gen_range_usize(2);
        const uint32_t s = (uint32_t)rng.gen_range_usize(len - 2);
        const uint32_t e = s + 2 + (uint32_t)rng.gen_range_usize(len - s - 2);
        out[it] = make_uint2(s | (joint << 31), e);
    }
}

// What the decomposition of a call leaves: the device tables (pc; the raster view g sits at the start of d, the compatibility rows at
// d + o_cp), and on the host per policy its record and per long piece its length.
struct RefineDecomposed {
    RefinePolConst pc{};
    uint8_t *d = nullptr;
    size_t o_cp = 0;
    uint64_t T = 0;                                                  // policy nodes in all
    std::vector<uint8_t> first;
    const RefinePolRecord *rec = nullptr;
    const uint32_t *long_len = nullptr;
};

// Checks the policies of `in`, uploads them with g and decomposes them (k_refine_policies_decompose), into slot 2 of h's scratch.
// Returns 0, an error code (err says why), or 1 when the policies are all empty (nothing uploaded).
static int refine_decompose(RefineHost &h, const std::string &W_, const RefinePoliciesIn &in, const RefinePoliciesOut &out, const RunConst &g, hipStream_t stream,
                            RefineDecomposed &dc, std::string &err) {
    const uint64_t n = in.n;
    const uint32_t n_rows = in.n_rows, nw = in.nw;
    if (!in.pol_off || !out.ref_off || (n && (!out.status || !out.cost))) { err = W_ + "pol_off, ref_off, status and expected_costs"; return PORRT_ERR_INVALID; }
    if (n >= (1ull << 31) || in.pol_off[0] != 0) { err = W_ + "fewer than 2^31 policies, pol_off[0] = 0"; return PORRT_ERR_INVALID; }
    for (uint64_t q = 0; q < n; ++q)
        if (in.pol_off[q + 1] < in.pol_off[q]) { err = W_ + "pol_off must not decrease"; return PORRT_ERR_INVALID; }
    const uint64_t T = in.pol_off[n];
    dc.T = T;
    if (T >= (1ull << 31)) { err = W_ + "fewer than 2^31 nodes in all"; return PORRT_ERR_INVALID; }
    if (T && (!in.xy || !in.parents || !in.original || !in.belief || !in.beliefs || !n_rows || !nw)) { err = W_ + "the policies' arrays"; return PORRT_ERR_INVALID; }
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    // the upload: RunConst | pol_off | compat | beliefs | xy | original ids | parents (checked, 32 bits) | belief rows
    const size_t o_off = up16(sizeof(RunConst)), o_cp = o_off + up16((n + 1) * 8), o_bel = o_cp + up16((size_t)n_rows * 8),
                 o_xy = o_bel + up16((size_t)n_rows * nw * 8), o_or = o_xy + up16(T * 16), o_pa = o_or + up16(T * 8), o_br = o_pa + up16(T * 4),
                 up_bytes = o_br + up16(T * 4);
    h.stage.resize(up_bytes);
    uint8_t *stage = h.stage.data();
    {
        int32_t *pa = (int32_t *)(stage + o_pa);
        for (uint64_t q = 0; q < n; ++q) {
            const uint64_t b = in.pol_off[q], m = in.pol_off[q + 1] - b;
            for (uint64_t k = 0; k < m; ++k) {
                const int64_t p = in.parents[b + k];
                if (in.belief[b + k] >= n_rows) { err = W_ + "a belief row out of range (policy " + std::to_string(q) + ")"; return PORRT_ERR_INVALID; }
                if (k == 0 ? p != -1 : (p < 0 || (uint64_t)p >= m || (uint64_t)p == k)) {
                    err = W_ + "a parent out of range, or a row 0 that is no root (policy " + std::to_string(q) + ")";
                    return PORRT_ERR_INVALID;
                }
                pa[b + k] = (int32_t)p;
            }
        }
    }
    if (T == 0) return 1;
    memcpy(stage, &g, sizeof g);
    memcpy(stage + o_off, in.pol_off, (n + 1) * 8);
    memcpy(stage + o_cp, in.compat, (size_t)n_rows * 8);
    memcpy(stage + o_bel, in.beliefs, (size_t)n_rows * nw * 8);
    memcpy(stage + o_xy, in.xy, T * 16);
    memcpy(stage + o_or, in.original, T * 8);
    memcpy(stage + o_br, in.belief, T * 4);
    // the work arrays behind it; the first download (records | lengths of the long pieces) in one piece at the end
    const size_t L = T / 3 + 1;
    size_t at = up_bytes;
    auto take = [&](size_t bytes) { const size_t o = at; at += up16(bytes); return o; };
    const size_t w_link = take(T * 8), w_next = take(T * 4), w_src = take(T * 4), w_par = take(T * 4), w_leaf = take(T), w_any = take(T * sizeof(RefinePolAny)),
                 w_longs = take(L * sizeof(RefinePolPiece)), w_x = take(T * 8), w_y = take(T * 8), w_q = take(T * 8), w_t = take(T * 8), w_p = take(T * 8),
                 w_v = take(T * 8), w_err = take(n * 4), w_rec = take(n * sizeof(RefinePolRecord)), w_len = take(L * 4), bytes = at;
    uint8_t *d = nullptr;
    HIPCHK_ERR(h.scratch.get(2, d, bytes));
    RefinePolConst &pc = dc.pc;
    pc.pol_off = (const unsigned long long *)(d + o_off); pc.in_xy = (const double *)(d + o_xy); pc.in_orig = (const unsigned long long *)(d + o_or);
    pc.in_parent = (const int32_t *)(d + o_pa); pc.in_belief = (const uint32_t *)(d + o_br); pc.beliefs = (const double *)(d + o_bel);
    pc.nw = nw; pc.n_policies = (uint32_t)n;
    pc.link = (uint2 *)(d + w_link); pc.next = (uint32_t *)(d + w_next); pc.src = (uint32_t *)(d + w_src); pc.par = (int32_t *)(d + w_par);
    pc.leaf = d + w_leaf; pc.any = (RefinePolAny *)(d + w_any); pc.longs = (RefinePolPiece *)(d + w_longs); pc.long_len = (uint32_t *)(d + w_len);
    pc.rec = (RefinePolRecord *)(d + w_rec); pc.x = (double *)(d + w_x); pc.y = (double *)(d + w_y);
    pc.wq = (double *)(d + w_q); pc.wt = (double *)(d + w_t); pc.wp = (double *)(d + w_p); pc.wv = (double *)(d + w_v);
    pc.pol_err = (uint32_t *)(d + w_err);
    HIPCHK_ERR(hipMemcpyAsync(d, stage, up_bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_refine_policies_decompose, dim3((uint32_t)n), dim3(64), 0, stream, pc);
    HIPCHK_ERR(hipGetLastError());
    dc.first.resize(bytes - w_rec);
    HIPCHK_ERR(hipMemcpyAsync(dc.first.data(), d + w_rec, bytes - w_rec, hipMemcpyDeviceToHost, stream));
    HIPCHK_ERR(hipStreamSynchronize(stream));
    dc.d = d; dc.o_cp = o_cp;
    dc.rec = (const RefinePolRecord *)dc.first.data();
    dc.long_len = (const uint32_t *)(dc.first.data() + (w_len - w_rec));
    return 0;
}

// PTOPolicyRefiner::refine_solution(PartialShortCut(n_iter)) (pto_policy_refiner.rs:87-124) of the policies of `in`, checked on the raster
// g describes (all zero: no grid).  Everything on the device: one upload, the decomposition, one small download (per policy its counts,
// per piece of >= 3 nodes its length; refine_decompose, shared with the Reparent strategy of porrt_reparent.hpp), one table of draws per
// distinct length (the draws do not depend on the commits) uploaded with the launch order (longest piece first), the shortcuts of all
// pieces in one launch (short_lds: pieces of <= kRefineShortLdsNodes nodes in a launch of their own), offsets, recomposition with the
// expected costs, one download.  out.cap = 0 launches no shortcut kernel.  Fills info (counts and times of this call) and, where a
// policy's status is not 0 or the call fails, err (prefixed with who).  Returns the refined nodes of the policies with status 0.
static int64_t refine_policies(RefineHost &h, const char *who, const RefinePoliciesIn &in, uint64_t n_iter, const RefinePoliciesOut &out, const RunConst &g,
                               bool short_lds, hipStream_t stream, struct porrt_refine_policies_info &info, std::string &err) {
    const double t0 = now_s();
    const uint64_t n = in.n;
    const std::string W_ = std::string(who) + ": ";
    if (n_iter >= (1ull << 31)) { err = W_ + "at most 2^31 - 1 iterations"; return PORRT_ERR_INVALID; }
    RefineDecomposed dc;
    const int dr_ = refine_decompose(h, W_, in, out, g, stream, dc, err);
    if (dr_ < 0) return dr_;
    info = {};
    info.policies = n;
    out.ref_off[0] = 0;
    if (dr_ == 1) {                                                  // nothing but empty policies: no launch
        for (uint64_t q = 0; q < n; ++q) { out.ref_off[q + 1] = 0; out.status[q] = 1; out.cost[q] = 0.0; }
        if (n) err = W_ + "policy 0: no policy to refine";
        info.ms_wall = 1e3 * (now_s() - t0);
        return 0;
    }
    const bool shortcuts = out.cap != 0 && n_iter != 0;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    RefinePolConst &pc = dc.pc;
    uint8_t *const d = dc.d;
    const size_t o_cp = dc.o_cp;
    const RefinePolRecord *rec = dc.rec;
    const uint32_t *long_len = dc.long_len;
    // the launch order (longest first) and one table of draws per distinct length
    uint64_t M = 0;
    std::vector<uint64_t> keys;                                      // length << 32 | row of longs
    for (uint64_t q = 0; q < n; ++q) {
        if (rec[q].status) continue;
        M += rec[q].rows;
        info.pieces += rec[q].pieces;
        for (uint32_t j = 0; j < rec[q].longs; ++j) {
            const uint64_t row = in.pol_off[q] / 3 + j;
            keys.push_back((uint64_t)long_len[row] << 32 | row);
        }
    }
    std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
    std::vector<std::pair<uint32_t, uint32_t>> len_at;               // (length, first draw), longest first
    for (uint64_t k : keys)
        if (len_at.empty() || len_at.back().first != (uint32_t)(k >> 32)) {
            if (shortcuts && (len_at.size() + 1) * n_iter > (1ull << 26)) { err = W_ + "more than 2^26 draws (iterations x distinct piece lengths)"; return PORRT_ERR_CAPACITY; }
            len_at.push_back({(uint32_t)(k >> 32), (uint32_t)(len_at.size() * n_iter)});
        }
    info.distinct_lengths = len_at.size();
    double ms_device = 0.0;
    if (shortcuts && !keys.empty()) {
        if (!g.has_grid) { err = W_ + "the refiner checks transitions on the context's grid (porrt_set_grid)"; return PORRT_ERR_INVALID; }
        const size_t nd = len_at.size() * n_iter, o_dr = up16(keys.size() * sizeof(uint2)), bytes2 = o_dr + nd * sizeof(uint2);
        std::vector<uint8_t> second(bytes2);
        uint2 *order = (uint2 *)second.data(), *dr = (uint2 *)(second.data() + o_dr);
        size_t li = 0, n_big = 0;
        for (size_t k = 0; k < keys.size(); ++k) {
            const uint32_t len = (uint32_t)(keys[k] >> 32);
            while (len_at[li].first != len) ++li;
            order[k] = make_uint2((uint32_t)keys[k], len_at[li].second);
            if (len > kRefineShortLdsNodes) ++n_big;
        }
        for (const auto &la : len_at) shortcut_draws(la.first, n_iter, dr + la.second);
        uint8_t *d2 = nullptr;
        HIPCHK_ERR(h.scratch.get(4, d2, bytes2));
        HIPCHK_ERR(h.events());
        RefinePolLaunch ln{};
        ln.rc.rc = (const RunConst *)d; ln.rc.draws = (const uint2 *)(d2 + o_dr); ln.rc.compat = (const unsigned long long *)(d + o_cp);
        ln.rc.x = pc.x; ln.rc.y = pc.y; ln.rc.n_pieces = (uint32_t)keys.size(); ln.rc.n_iter = (uint32_t)n_iter;
        ln.longs = pc.longs; ln.order = (const uint2 *)d2; ln.pol_err = pc.pol_err;
        HIPCHK_ERR(hipMemcpyAsync(d2, second.data(), bytes2, hipMemcpyHostToDevice, stream));
        HIPCHK_ERR(hipEventRecord(h.ev[0], stream));
        const size_t n_first = short_lds ? n_big : keys.size();
        if (n_first) {
            ln.first = 0;
            hipLaunchKernelGGL(k_refine_policies_shortcut<kRefineLdsNodes>, dim3((uint32_t)n_first), dim3(64), 0, stream, ln);
            HIPCHK_ERR(hipGetLastError());
        }
        if (n_first < keys.size()) {                                 // the short pieces: a quarter of the LDS per wave
            ln.first = (uint32_t)n_first;
            hipLaunchKernelGGL(k_refine_policies_shortcut<kRefineShortLdsNodes>, dim3((uint32_t)(keys.size() - n_first)), dim3(64), 0, stream, ln);
            HIPCHK_ERR(hipGetLastError());
        }
        HIPCHK_ERR(hipEventRecord(h.ev[1], stream));
        info.shortcut_pieces = keys.size();
    }
    // offsets, recomposition and costs; the answers packed in one block: ref_off | cost | status | xy | original ids | parents | leafs
    const size_t r_off = 0, r_cost = r_off + up16((n + 1) * 8), r_st = r_cost + up16(n * 8), r_xy = r_st + up16(n), r_or = r_xy + up16(M * 16),
                 r_pa = r_or + up16(M * 8), r_lf = r_pa + up16(M * 8), bytes3 = r_lf + up16(M);
    uint8_t *d3 = nullptr;
    HIPCHK_ERR(h.scratch.get(3, d3, bytes3));
    pc.ref_off = (unsigned long long *)(d3 + r_off); pc.cost = (double *)(d3 + r_cost); pc.status = d3 + r_st; pc.out_xy = (double *)(d3 + r_xy);
    pc.out_orig = (unsigned long long *)(d3 + r_or); pc.out_parent = (long long *)(d3 + r_pa); pc.out_leaf = d3 + r_lf;
    hipLaunchKernelGGL(k_refine_policies_offsets, dim3(1), dim3(256), 0, stream, pc);
    HIPCHK_ERR(hipGetLastError());
    hipLaunchKernelGGL(k_refine_policies_recompose, dim3((uint32_t)n), dim3(64), 0, stream, pc);
    HIPCHK_ERR(hipGetLastError());
    std::vector<uint8_t> third(bytes3);
    HIPCHK_ERR(hipMemcpyAsync(third.data(), d3, bytes3, hipMemcpyDeviceToHost, stream));
    HIPCHK_ERR(hipStreamSynchronize(stream));
    if (info.shortcut_pieces) {
        float ms = 0.0f;
        HIPCHK_ERR(hipEventElapsedTime(&ms, h.ev[0], h.ev[1]));
        ms_device = (double)ms;
    }
    memcpy(out.ref_off, third.data() + r_off, (n + 1) * 8);
    memcpy(out.cost, third.data() + r_cost, n * 8);
    memcpy(out.status, third.data() + r_st, n);
    const uint64_t total = out.ref_off[n];
    if (total && total <= out.cap) {
        if (out.xy) memcpy(out.xy, third.data() + r_xy, total * 16);
        if (out.original) memcpy(out.original, third.data() + r_or, total * 8);
        if (out.parents) memcpy(out.parents, third.data() + r_pa, total * 8);
        if (out.leaf) memcpy(out.leaf, third.data() + r_lf, total);
    }
    for (uint64_t q = 0; q < n; ++q) info.ok += out.status[q] == 0;
    for (uint64_t q = 0; q < n; ++q)
        if (out.status[q]) {
            static const char *const what[4] = {"", "no policy to refine", "a shortcut reads outside the raster, a door pixel without zone id or two zones on one segment (the reference panics)",
                                                "a piece whose nodes carry different beliefs (the reference asserts, common.rs:102)"};
            err = W_ + "policy " + std::to_string(q) + ": " + what[out.status[q] & 3];
            break;
        }
    info.nodes = total;
    info.ms_device = ms_device;
    info.ms_wall = 1e3 * (now_s() - t0);
    return (int64_t)total;
}

// Rows of a refined policy: decompose reaches a node iff its chain of parents ends at node 0, and recompose gives every node reached
// one row (a piece left unconnected by the one-node quirk keeps its rows).  -1: parents that refine_policies refuses.
static int64_t refine_rows(uint64_t n, const int64_t *parents) {
    if (n && parents[0] != -1) return -1;
    std::vector<uint8_t> mark(n, 0);                                 // 1 reached, 2 not (or being walked: a cycle is not reached)
    std::vector<uint64_t> chain;
    int64_t rows = n ? 1 : 0;
    if (n) mark[0] = 1;
    for (uint64_t k = 1; k < n; ++k) {
        chain.clear();
        uint64_t j = k;
        for (; !mark[j]; j = (uint64_t)parents[j]) {
            if (parents[j] < 0 || (uint64_t)parents[j] >= n || (uint64_t)parents[j] == j) return -1;
            mark[j] = 2;
            chain.push_back(j);
        }
        if (mark[j] == 1) { for (uint64_t c : chain) mark[c] = 1; rows += (int64_t)chain.size(); }
    }
    return rows;
}

// One policy (in.n = 1): a batch of one.  Returns the number of nodes of the refined policy always and fills the arrays of out (its
// ref_off, status and cost are this function's) when out.cap holds it; a smaller cap is the sizing form, answered on the host (no launch,
// info untouched; the beliefs are checked by the call that fills).  A status other than 0 is an error code, err says which.
static int64_t refine_policy(RefineHost &h, const RefinePoliciesIn &in, uint64_t n_iter, RefinePoliciesOut out, double *expected_cost, const RunConst &g,
                             bool short_lds, hipStream_t stream, struct porrt_refine_policies_info &info, std::string &err) {
    const int64_t rows = refine_rows(in.pol_off[1], in.parents);
    if (rows >= 0 && out.cap < (uint64_t)rows) return rows;
    uint64_t ref_off[2] = {0, 0};
    uint8_t status = 0;
    double cost = 0.0;
    out.ref_off = ref_off; out.status = &status; out.cost = &cost;
    const int64_t m = refine_policies(h, "refine_policy", in, n_iter, out, g, short_lds, stream, info, err);
    if (m < 0) return m;
    if (status) return status == 2 ? PORRT_ERR_RASTER : PORRT_ERR_INVALID;      // (refine_policies has set the message)
    if (expected_cost) *expected_cost = cost;
    return m;
}

} // namespace porrt
