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

} // namespace porrt
