// porrt_reparent.hpp -- PTOPolicyRefiner::refine_solution(RefinmentStrategy::Reparent(radius)) (src/pto_policy_refiner.rs:87-124) of one
// policy or many in one call (porrt_bg_reparent_policies / porrt_reparent_policies; porrt_bg_reparent_policy is a batch of one).
//
// The policy is cut into pieces as for PartialShortCut (Policy::decompose; k_refine_policies_decompose of porrt_refine_batch.hpp).  Per piece:
//
//   build_tree (:209-279).  The tree starts as the piece's path: tree id = position, parent = the node before, edge cost = norm2 of the
//   two states; `visited` = the path's belief-graph ids.  Then for every PATH node a, in order, a FIFO starting as [(a, its id g)]: a
//   popped (tree_id, g) walks children(g) in list order; a child c not visited with norm2(a.state, c.state) <= radius -- measured from
//   the path node a, not from tree_id -- is added with parent tree_id and THAT distance as its edge cost, and marked visited; then every
//   child cc of c not visited at that moment is pushed as (new tree id, cc).  So cc itself is never tested: its children are, and hang
//   from c.  A cc visited at push time never has its children examined through c.  tree.belief_state_id is the belief of the piece's first
//   node, tree.leaf the last path node.
//   reparent(tree, kd, 0.5 * radius) (:281-322).  Every node is pushed with priority dist_from_root (:55-64: the parents upward,
//   cost += link.cost from 0.0, recomputed on every use -- the order of the sum is part of the result).  Pop the least; its neighbours
//   are all tree nodes within 0.5 * radius (itself and copies included) that is_transition_valid(node, neighbour, tree belief) lets it
//   reach; d = dist_from_root(node) and every neighbour's dist_from_root are taken before any change; then every neighbour with
//   d + norm2(node, neighbour) < its own gets (node, that cost) as parent and is pushed with the tested sum.  The priorities of its
//   descendants stay as they were.
//   recompose (:324-393).  A piece gives the parent chain from tree.leaf up to the root, reversed -- shorter or longer than the piece
//   was; every node carries its own belief-graph id and that node's belief (the expected cost uses them as they are).  The one-node
//   quirk of porrt_refine.hpp stays.
//
// OURS, NOT THE REFERENCE'S.  The reference's queue runs over a wrapper whose Ord never returns Equal (common.rs:231-253): the order of
// bit-equal priorities is whatever the priority_queue crate's heap makes of it.  Here:
//   * among bit-equal priorities the node of the LOWEST TREE ID is popped;
//   * a push on a node in the queue replaces its priority, higher or lower; on a node already popped it inserts it again (the crate's
//     documented push, recalled);
//   * no kd-tree: the neighbour order only orders the pushes of one pop, which under the two rules above changes nothing;
//   * caps, per piece and independent of what else is in the call (every piece works in a slot of its own, sized by the cap alone):
//     a tree of more than C = "reparent_max_tree_nodes" nodes, a FIFO of more than 16 C entries at a time, or more than 256 C pairs of tree
//     nodes within 0.5 * radius of each other make the policy status 4; more than "reparent_max_pops_per_node" (64) x tree nodes pops
//     status 5.  (Why the loop is believed to end: f64 addition of non-negatives is monotone, so a node's upward sum is never below an
//     ancestor's and the strict < never hangs an ancestor under its descendant; that it ENDS is not proven, hence the cap.  The upward
//     walks are bounded by the tree size all the same: a walk that does not end makes status 5, it never hangs.)
// A policy's status: 3 from the decomposition; else over its pieces 4, else 2 (a raster fault in any node's transition checks: every node
// is popped at least once, so the checks are made for all nodes before the loop), else 5, else 0.
//
// Device.  Jobs = the pieces of the policies the decomposition accepted.  They run in rounds of as many slots as kReparentBudget holds;
// per round, all on the stream with one small download at its end (the jobs' records, for the chain lengths):
//   k_reparent_tube       one wave per piece: path, then the FIFO in order; the lanes stride over a popped entry's children (visited test
//                         in a hash set of the slot, distance in f64), the hits are added in lane order (= list order; a duplicate id
//                         in one children list is visited at its second occurrence), the pushes of an added child see the adds before
//                         it and keep their order through a ballot prefix.
//   k_reparent_near<0/1>  one wave per tree node, all nodes of all pieces of the round: count of the tree nodes in range (<0>), then
//                         after k_reparent_scan's offsets the transition checks of those and the valid ones in ascending order (<1>).
//                         A fault is OR-ed into the job's flags.
//   k_reparent_pop        one workgroup per piece: argmin over (priority, id), the upward walks one neighbour per thread, barrier,
//                         commits and pushes.  (parent, cost, priority) in LDS up to kReparentLdsNodes nodes, in the slot's global
//                         arrays through the same code beyond.  It ends with the chain from the leaf.
//   k_reparent_emit       the chains' states and ids into the pool of recomposed rows (grown by the host between rounds as needed).
// Then k_reparent_recompose, one wave per policy: rows, parents, leafs and the expected cost in the order of the reference's recursion
// (as k_refine_policies_recompose does it, with the pieces' new lengths and every row's own belief).
#pragma once
#include "porrt_refine_batch.hpp"

namespace porrt {

constexpr uint32_t kReparentLdsNodes = 1024;         // (parent, cost, priority) of a tree in LDS: 20 KiB per workgroup
constexpr uint32_t kReparentFifoPerNode = 16, kReparentPairsPerNode = 256;
constexpr uint32_t kReparentMaxTreeNodesLimit = 1u << 15;
constexpr size_t kReparentBudget = (size_t)1 << 30;  // bytes of slots per round
enum : uint32_t { RP_CAP = 1u, RP_RASTER = 2u, RP_POPS = 4u };

// The belief graph on the device: node g has state (nx, ny)[g / B], belief row bvec ? bvec[g] : g % B, children child_id[child_off[g] ..]
struct ReparentGraph {
    const double *nx, *ny;
    const uint32_t *bvec;
    const unsigned long long *child_off;
    const uint32_t *child_id;
    uint32_t B;
    unsigned long long n;
};

struct ReparentJob { uint32_t policy, piece; };
struct ReparentRec { uint32_t n_tree, n_path, flags, chain, pairs, pops, reparents, in_range; };

struct ReparentConst {
    RefinePolConst pc;                   // the decomposition's tables
    ReparentGraph gr;
    const RunConst *rc;
    const unsigned long long *compat;    // per belief row
    const ReparentJob *jobs;
    ReparentRec *rec;                    // per job
    uint32_t first;                      // first job of this round (slot s works on job first + s)
    uint32_t C, H, hash_shift, F, fifo_live, pairs_cap, pops_per_node;
    double radius, half;
    // slots
    double *tx, *ty, *tcost, *prio;      // [C] each
    uint32_t *tg, *tpar, *ncnt, *chain;  // [C]
    uint32_t *noff;                      // [C + 1]
    uint32_t *hash;                      // [H]
    uint2 *fifo;                         // [F]
    uint32_t *nbr;                       // [pairs_cap]
    uint8_t *win;                        // [C]
    // the pool of recomposed rows and where a job's chain goes in it
    double *px, *py;
    uint32_t *pg;
    const unsigned long long *pool_off;  // per job
};

__device__ __forceinline__ double rp_norm2(double ax, double ay, double bx, double by) {    // norm2 (pto_graph.rs:150): a -> b
    double dx = bx - ax, d2 = 0.0;
    d2 += dx * dx;
    dx = by - ay;
    d2 += dx * dx;
    return sqrt(d2);
}
__device__ __forceinline__ uint32_t rp_hash(uint32_t g, uint32_t shift) { return (g * 2654435761u) >> shift; }
__device__ __forceinline__ bool rp_seen(const uint32_t *hash, uint32_t mask, uint32_t shift, uint32_t g) {
    for (uint32_t h = rp_hash(g, shift);; h = (h + 1u) & mask) {     // at most C < H / 2 keys: an empty entry is always met
        const uint32_t v = hash[h];
        if (v == g) return true;
        if (v == kRefNone) return false;
    }
}
__device__ __forceinline__ void rp_insert(uint32_t *hash, uint32_t mask, uint32_t shift, uint32_t g) {
    for (uint32_t h = rp_hash(g, shift);; h = (h + 1u) & mask) {
        const uint32_t v = atomicCAS(&hash[h], kRefNone, g);
        if (v == kRefNone || v == g) return;
    }
}

__global__ __launch_bounds__(64) void k_reparent_tube(ReparentConst c) {
    const uint32_t slot = blockIdx.x, lane = threadIdx.x;
    const ReparentJob job = c.jobs[c.first + slot];
    ReparentRec *rec = c.rec + c.first + slot;
    const uint64_t base = c.pc.pol_off[job.policy];
    const RefinePolAny a = c.pc.any[base + job.piece];
    const uint32_t *src = c.pc.src + base + a.off;
    const unsigned long long *orig = c.pc.in_orig + base;
    const ReparentGraph &gr = c.gr;
    double *tx = c.tx + (size_t)slot * c.C, *ty = c.ty + (size_t)slot * c.C, *tcost = c.tcost + (size_t)slot * c.C;
    uint32_t *tg = c.tg + (size_t)slot * c.C, *tpar = c.tpar + (size_t)slot * c.C, *hash = c.hash + (size_t)slot * c.H;
    uint2 *fifo = c.fifo + (size_t)slot * c.F;
    const uint32_t n_path = a.len, hmask = c.H - 1u, fmask = c.F - 1u, shift = c.hash_shift;
    if (n_path > c.C) {
        if (lane == 0) *rec = ReparentRec{0u, n_path, RP_CAP, 0u, 0u, 0u, 0u, 0u};
        return;
    }
    for (uint32_t h = lane; h < c.H; h += 64) hash[h] = kRefNone;
    __syncthreads();
    for (uint32_t r = lane; r < n_path; r += 64) {                   // the path
        const uint32_t g = (uint32_t)orig[src[r]];
        const double x = gr.nx[g / gr.B], y = gr.ny[g / gr.B];
        tx[r] = x; ty[r] = y; tg[r] = g;
        tpar[r] = r ? r - 1u : kRefNone;
        double cost = 0.0;
        if (r) {
            const uint32_t gp = (uint32_t)orig[src[r - 1]];
            cost = rp_norm2(gr.nx[gp / gr.B], gr.ny[gp / gr.B], x, y);
        }
        tcost[r] = cost;
        rp_insert(hash, hmask, shift, g);
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t n = n_path;
    bool over = false;
    for (uint32_t p = 0; p < n_path && !over; ++p) {                 // the offsprings of path node p (nodes = tree.nodes.clone(): the path alone)
        const double ax = tx[p], ay = ty[p];
        uint32_t head = 0, tail = 1;
        if (lane == 0) fifo[0] = make_uint2(p, tg[p]);
        __syncthreads();
        while (head != tail && !over) {
            const uint2 e = fifo[head & fmask];
            ++head;
            const unsigned long long cb = gr.child_off[e.y], ce = gr.child_off[e.y + 1];
            for (unsigned long long k0 = cb; k0 < ce && !over; k0 += 64) {
                const unsigned long long k = k0 + lane;
                uint32_t ch = kRefNone;
                double sx = 0.0, sy = 0.0, d = 0.0;
                bool hit = false;
                if (k < ce) {
                    ch = gr.child_id[k];
                    if (!rp_seen(hash, hmask, shift, ch)) {
                        sx = gr.nx[ch / gr.B]; sy = gr.ny[ch / gr.B];
                        d = rp_norm2(ax, ay, sx, sy);                // from the PATH node
                        hit = d <= c.radius;
                    }
                }
                unsigned long long hits = __ballot(hit);
                while (hits && !over) {                              // the adds in list order
                    const int l = __ffsll((long long)hits) - 1;
                    hits &= hits - 1ull;
                    const uint32_t chl = (uint32_t)__shfl((int)ch, l);
                    if (rp_seen(hash, hmask, shift, chl)) continue;  // the same id earlier in this list
                    if (n >= c.C) { over = true; break; }
                    if ((int)lane == l) {
                        tx[n] = sx; ty[n] = sy; tg[n] = ch; tpar[n] = e.x; tcost[n] = d;
                        rp_insert(hash, hmask, shift, ch);
                    }
                    __syncthreads();
                    const uint32_t id = n++;
                    const unsigned long long gb = gr.child_off[chl], ge = gr.child_off[chl + 1];
                    for (unsigned long long m0 = gb; m0 < ge; m0 += 64) {    // its children not visited at this moment
                        const unsigned long long m = m0 + lane;
                        uint32_t cc = 0;
                        bool want = false;
                        if (m < ge) { cc = gr.child_id[m]; want = !rp_seen(hash, hmask, shift, cc); }
                        const unsigned long long w = __ballot(want);
                        if (want) fifo[(tail + (uint32_t)__popcll(w & below)) & fmask] = make_uint2(id, cc);
                        tail += (uint32_t)__popcll(w);
                        if (tail - head > c.fifo_live) break;        // (entries may have been overwritten: the piece is given up)
                    }
                    if (tail - head > c.fifo_live) over = true;
                    __syncthreads();
                }
            }
        }
    }
    if (lane == 0) *rec = ReparentRec{over ? 0u : n, n_path, over ? (uint32_t)RP_CAP : 0u, 0u, 0u, 0u, 0u, 0u};
}

// kFill = false: ncnt[i] = tree nodes within `half` of node i.  kFill = true (after k_reparent_scan): the transition checks of those; the
// valid ones go to nbr[noff[i] ..] in ascending order and ncnt[i] becomes their number.
template <bool kFill>
__global__ __launch_bounds__(256) void k_reparent_near(ReparentConst c) {
    const uint32_t slot = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ReparentRec *rec = c.rec + c.first + slot;
    if (rec->flags & RP_CAP) return;
    const uint32_t n = rec->n_tree;
    const double *tx = c.tx + (size_t)slot * c.C, *ty = c.ty + (size_t)slot * c.C;
    uint32_t *ncnt = c.ncnt + (size_t)slot * c.C, *nbr = c.nbr + (size_t)slot * c.pairs_cap;
    const uint32_t *noff = c.noff + (size_t)slot * (c.C + 1);
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long compat = 0ull;
    TableGrid grid;
    if (kFill) {
        const ReparentJob job = c.jobs[c.first + slot];
        const uint64_t base = c.pc.pol_off[job.policy];
        const RefinePolAny a = c.pc.any[base + job.piece];
        compat = c.compat[c.pc.in_belief[base + c.pc.src[base + a.off]]];          // tree.belief_state_id: the piece's first node
        grid.p = c.rc->cls; grid.W = c.rc->W;
    }
    for (uint32_t i = blockIdx.y * 4u + wave; i < n; i += gridDim.y * 4u) {
        const double x = tx[i], y = ty[i];
        const uint32_t at = kFill ? noff[i] : 0u;
        uint32_t count = 0;
        bool fault = false;
        for (uint32_t j0 = 0; j0 < n; j0 += 64) {
            const uint32_t j = j0 + lane;
            bool ok = false;
            if (j < n) {
                const double ux = tx[j], uy = ty[j];
                ok = rp_norm2(x, y, ux, uy) <= c.half;
                if (kFill && ok) {
                    const uint32_t st = refine_transition(*c.rc, grid, x, y, ux, uy, compat);
                    fault = fault || st == 2u;
                    ok = st == 0u;
                }
            }
            const unsigned long long m = __ballot(ok);
            if (kFill && ok) nbr[at + count + (uint32_t)__popcll(m & below)] = j;
            count += (uint32_t)__popcll(m);
        }
        if (lane == 0) ncnt[i] = count;
        if (kFill) {
            if (lane == 0 && count) atomicAdd(&rec->pairs, count);
            if (__ballot(fault) && lane == 0) atomicOr(&rec->flags, RP_RASTER);
        }
    }
}

// noff = running sum of ncnt; more pairs in range than the slot holds: RP_CAP
__global__ __launch_bounds__(256) void k_reparent_scan(ReparentConst c) {
    __shared__ unsigned long long part[256];
    __shared__ unsigned long long carry;
    const uint32_t slot = blockIdx.x, t = threadIdx.x;
    ReparentRec *rec = c.rec + c.first + slot;
    if (rec->flags & RP_CAP) return;
    const uint32_t n = rec->n_tree;
    const uint32_t *ncnt = c.ncnt + (size_t)slot * c.C;
    uint32_t *noff = c.noff + (size_t)slot * (c.C + 1);
    if (t == 0) carry = 0ull;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < n; i0 += 256) {
        const uint32_t i = i0 + t;
        const unsigned long long v = i < n ? ncnt[i] : 0ull;
        part[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const unsigned long long add = t >= d ? part[t - d] : 0ull;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        const unsigned long long before = carry + part[t] - v;
        if (i < n) noff[i] = before > c.pairs_cap ? c.pairs_cap : (uint32_t)before;
        __syncthreads();
        if (t == 255) carry += part[255];
        __syncthreads();
    }
    if (t == 0) {
        noff[n] = carry > c.pairs_cap ? c.pairs_cap : (uint32_t)carry;
        rec->in_range = noff[n];
        if (carry > c.pairs_cap) rec->flags |= RP_CAP;
    }
}

// dist_from_root (:55-64): upward, cost += link.cost from 0.0.  ok = false when the walk has not ended after n steps (never, if the
// tree is one).
__device__ __forceinline__ double rp_walk(const uint32_t *par, const double *cost, uint32_t i, uint32_t n, bool &ok) {
    double s = 0.0;
    uint32_t steps = 0;
    for (uint32_t p = par[i]; p != kRefNone; p = par[i]) {
        if (++steps > n) { ok = false; break; }
        s += cost[i];
        i = p;
    }
    return s;
}

__global__ __launch_bounds__(256) void k_reparent_pop(ReparentConst c) {
    __shared__ uint32_t l_par[kReparentLdsNodes];
    __shared__ double l_cost[kReparentLdsNodes], l_prio[kReparentLdsNodes];
    __shared__ double r_p[4];
    __shared__ uint32_t r_i[4];
    __shared__ uint32_t s_bad;
    const uint32_t slot = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    ReparentRec *rec = c.rec + c.first + slot;
    if (rec->flags) {                                                // (uniform: written by the kernels before this one)
        if (t == 0) rec->chain = 0u;
        return;
    }
    const uint32_t n = rec->n_tree, n_path = rec->n_path;
    const double *tx = c.tx + (size_t)slot * c.C, *ty = c.ty + (size_t)slot * c.C;
    const uint32_t *ncnt = c.ncnt + (size_t)slot * c.C, *noff = c.noff + (size_t)slot * (c.C + 1), *nbr = c.nbr + (size_t)slot * c.pairs_cap;
    uint8_t *win = c.win + (size_t)slot * c.C;
    uint32_t *chain = c.chain + (size_t)slot * c.C;
    const bool in_lds = n <= kReparentLdsNodes;
    uint32_t *par = in_lds ? l_par : c.tpar + (size_t)slot * c.C;
    double *cost = in_lds ? l_cost : c.tcost + (size_t)slot * c.C;
    double *prio = in_lds ? l_prio : c.prio + (size_t)slot * c.C;
    if (in_lds)
        for (uint32_t i = t; i < n; i += 256) { l_par[i] = c.tpar[(size_t)slot * c.C + i]; l_cost[i] = c.tcost[(size_t)slot * c.C + i]; }
    if (t == 0) s_bad = 0u;
    __syncthreads();
    bool ok = true;
    for (uint32_t i = t; i < n; i += 256) prio[i] = rp_walk(par, cost, i, n, ok);     // push every node
    if (!ok) s_bad = 1u;
    __syncthreads();
    const unsigned long long limit = (unsigned long long)c.pops_per_node * n;
    unsigned long long pops = 0;
    uint32_t reparents = 0, flags = 0;
    for (;;) {
        // the least (priority, id) in the queue; a priority is never negative, -1.0 marks a node that is not in it
        double bp = 0.0;
        uint32_t bi = kRefNone;
        for (uint32_t i = t; i < n; i += 256) {
            const double p = prio[i];
            if (p >= 0.0 && (bi == kRefNone || p < bp)) { bp = p; bi = i; }
        }
        for (int off = 32; off; off >>= 1) {
            const double op = __shfl_down(bp, off);
            const uint32_t oi = (uint32_t)__shfl_down((int)bi, off);
            if (oi != kRefNone && (bi == kRefNone || op < bp || (op == bp && oi < bi))) { bp = op; bi = oi; }
        }
        if (lane == 0) { r_p[wave] = bp; r_i[wave] = bi; }
        __syncthreads();
        bp = r_p[0]; bi = r_i[0];
        for (uint32_t w = 1; w < 4; ++w) {
            const double op = r_p[w];
            const uint32_t oi = r_i[w];
            if (oi != kRefNone && (bi == kRefNone || op < bp || (op == bp && oi < bi))) { bp = op; bi = oi; }
        }
        if (bi == kRefNone) break;
        if (s_bad || pops == limit) { flags = RP_POPS; break; }
        ++pops;
        const double x = tx[bi], y = ty[bi];
        const uint32_t cnt = ncnt[bi];
        const uint32_t *nb = nbr + noff[bi];
        const double d = rp_walk(par, cost, bi, n, ok);              // the snapshots: its own sum and every neighbour's, before any change
        for (uint32_t k = t; k < cnt; k += 256) {
            const uint32_t j = nb[k];
            const double snap = rp_walk(par, cost, j, n, ok);
            const double nd = d + rp_norm2(x, y, tx[j], ty[j]);
            win[k] = nd < snap ? 1 : 0;
        }
        if (!ok) s_bad = 1u;
        __syncthreads();
        if (t == 0) prio[bi] = -1.0;                                 // popped (it is never its own better parent: d + 0 < d is false)
        for (uint32_t k = t; k < cnt; k += 256)
            if (win[k]) {
                const uint32_t j = nb[k];
                const double cst = rp_norm2(x, y, tx[j], ty[j]);
                par[j] = bi; cost[j] = cst;
                prio[j] = d + cst;                                   // the tested sum, not a fresh walk
                ++reparents;
            }
        __syncthreads();
    }
    if (reparents) atomicAdd(&rec->reparents, reparents);
    if (t == 0) {
        uint32_t len = 0;
        if (!flags) {                                                // recompose's chain: tree.leaf (the last PATH node) up to the root, reversed
            len = 1;
            for (uint32_t i = n_path - 1u; par[i] != kRefNone && len <= n; i = par[i]) ++len;
            if (len > n) { flags = RP_POPS; len = 0; }
            uint32_t i = n_path - 1u;
            for (uint32_t k = len; k-- > 0;) { chain[k] = i; i = par[i]; }
        }
        rec->chain = len;
        rec->pops = (uint32_t)(pops > 0xFFFFFFFFull ? 0xFFFFFFFFull : pops);
        if (flags) rec->flags |= flags;
    }
}

__global__ __launch_bounds__(64) void k_reparent_emit(ReparentConst c) {
    const uint32_t slot = blockIdx.x, lane = threadIdx.x;
    const ReparentRec rec = c.rec[c.first + slot];
    if (rec.flags) return;
    const unsigned long long at = c.pool_off[c.first + slot];
    const uint32_t *chain = c.chain + (size_t)slot * c.C;
    for (uint32_t k = lane; k < rec.chain; k += 64) {
        const uint32_t i = chain[k];
        c.px[at + k] = c.tx[(size_t)slot * c.C + i];
        c.py[at + k] = c.ty[(size_t)slot * c.C + i];
        c.pg[at + k] = c.tg[(size_t)slot * c.C + i];
    }
}

struct ReparentOut {
    const unsigned long long *pol_off;   // the input policies
    const RefinePolAny *any;
    const RefinePolRecord *prec;
    const uint32_t *job_first;           // per policy: its first job (kRefNone: not recomposed)
    const ReparentRec *rec;
    const unsigned long long *pool_off;
    const double *px, *py;
    const uint32_t *pg;
    ReparentGraph gr;
    const double *beliefs;
    uint32_t nw;
    uint32_t *w_off;                     // per job: first row of its chain within the policy
    int32_t *w_hang;                     //          the row its start hangs from, -1: none
    double *wq, *wt, *wp, *wv;           // per output row
    const unsigned long long *ref_off;
    double *cost;
    double *out_xy;
    unsigned long long *out_orig;
    long long *out_parent;
    uint8_t *out_leaf;
};

__global__ __launch_bounds__(64) void k_reparent_recompose(ReparentOut c) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint32_t j0 = c.job_first[q];
    if (j0 == kRefNone) {
        if (lane == 0) c.cost[q] = 0.0;
        return;
    }
    const uint64_t base = c.pol_off[q], ob = c.ref_off[q];
    const uint32_t pieces = c.prec[q].pieces;
    const RefinePolAny *any = c.any + base;
    const ReparentRec *rec = c.rec + j0;
    uint32_t *w_off = c.w_off + j0;
    int32_t *w_hang = c.w_hang + j0;
    double *wq = c.wq + ob, *wt = c.wt + ob, *wp = c.wp + ob, *wv = c.wv + ob;
    if (lane == 0) {
        uint32_t rows = 0;
        for (uint32_t i = 0; i < pieces; ++i) { w_off[i] = rows; rows += rec[i].chain; }
        w_hang[0] = -1;
        for (uint32_t i = 0; i < pieces; ++i) {                      // the skeleton; a one-node chain has a start and no end (:348-366)
            const int32_t end = rec[i].chain >= 2u ? (int32_t)(w_off[i] + rec[i].chain - 1u) : -1;
            for (uint32_t s = any[i].succ0; s < any[i].succ0 + any[i].nsucc; ++s) w_hang[s] = end;
        }
    }
    __syncthreads();
    for (uint32_t i = 0; i < pieces; ++i) {
        const uint32_t off = w_off[i], len = rec[i].chain;
        const unsigned long long at = c.pool_off[j0 + i];
        const bool ends = any[i].nsucc == 0u || len == 1u;
        for (uint32_t k = lane; k < len; k += 64) {
            const uint64_t r = ob + off + k;
            c.out_xy[2 * r] = c.px[at + k]; c.out_xy[2 * r + 1] = c.py[at + k];
            c.out_orig[r] = c.pg[at + k];
            c.out_parent[r] = k ? (long long)(off + k - 1u) : (long long)w_hang[i];
            c.out_leaf[r] = (k + 1u == len && ends) ? 1 : 0;
        }
    }
    __syncthreads();
    const uint32_t rows = w_off[pieces - 1] + rec[pieces - 1].chain;
    for (uint32_t r = lane; r < rows; r += 64) {
        const long long p = c.out_parent[ob + r];
        double qv = 0.0, d = 0.0;
        if (p >= 0) {
            const uint32_t g = (uint32_t)c.out_orig[ob + r], gp = (uint32_t)c.out_orig[ob + p];
            const double *cb = c.beliefs + (size_t)(c.gr.bvec ? c.gr.bvec[g] : g % c.gr.B) * c.nw;
            const double *pb = c.beliefs + (size_t)(c.gr.bvec ? c.gr.bvec[gp] : gp % c.gr.B) * c.nw;
            for (uint32_t w = 0; w < c.nw; ++w) qv = qv + (cb[w] > 0.0 ? pb[w] : 0.0);          // transition_probability (common.rs:187-190)
            d = rp_norm2(c.out_xy[2 * (ob + p)], c.out_xy[2 * (ob + p) + 1], c.out_xy[2 * (ob + r)], c.out_xy[2 * (ob + r) + 1]);
        }
        wq[r] = qv; wt[r] = d;
    }
    __syncthreads();
    if (lane != 0) return;
    for (uint32_t i = 0; i < pieces; ++i) {                          // p of every row and the term of the edge into it
        const uint32_t off = w_off[i], len = rec[i].chain;
        const int32_t hang = w_hang[i];
        double p = 1.0;
        if (hang >= 0) { p = wp[hang] * wq[off]; wt[off] = p * wt[off]; }
        wp[off] = p;
        for (uint32_t r = off + 1; r < off + len; ++r) {
            p = p * wq[r];
            wt[r] = p * wt[r];
            wp[r] = p;
        }
    }
    for (uint32_t i = pieces; i-- > 0;) {                            // a node's value: acc += term + ret(child) over its children in order
        const uint32_t off = w_off[i], len = rec[i].chain;
        double acc = 0.0;
        if (len >= 2u)
            for (uint32_t s = any[i].succ0; s < any[i].succ0 + any[i].nsucc; ++s) {
                const uint32_t rs = w_off[s];
                acc += wt[rs] + wv[rs];
            }
        for (uint32_t r = off + len - 1; r > off; --r) {
            const double below = wt[r] + acc;
            acc = 0.0;
            acc += below;
        }
        wv[off] = acc;
    }
    c.cost[q] = wv[0];
}

// ------------------------------------------------------------------------------------------------ host side

// The answers of a call, kept (on the context: what porrt_bg_get_reparented_policies hands out again)
struct ReparentResult {
    bool valid = false;
    uint64_t tag = ~0ull, stamp = ~0ull;
    std::vector<uint64_t> off;                       // [policies + 1]
    std::vector<uint8_t> status;
    std::vector<double> cost;
    std::vector<double> xy;
    std::vector<uint64_t> original;
    std::vector<int64_t> parent;
    std::vector<uint8_t> leaf;
};

static const char *const kReparentStatusText[6] = {
    "", "no policy to refine",
    "a transition check reads outside the raster, a door pixel without zone id or two zones on one segment (the reference panics)",
    "a piece whose nodes carry different beliefs (the reference asserts, common.rs:102)",
    "a piece's tree, its FIFO or its pairs in range exceed what reparent_max_tree_nodes allows",
    "a piece's loop made more than reparent_max_pops_per_node x tree nodes pops"};

// refine_solution(Reparent(radius)) of the policies of `in` (their original ids are belief-graph ids of gr, a graph on the device; xy and
// belief hold the graph's states and belief rows of the policy nodes), checked on the raster g describes.  C: "reparent_max_tree_nodes".
// The answers go to res (always, whatever their size); info gets the counts and times of the call; err what went wrong (a policy's nonzero
// status included).  Returns the recomposed nodes of the policies with status 0.
static int64_t reparent_policies(RefineHost &h, const char *who, const ReparentGraph &gr, const RefinePoliciesIn &in, double radius, uint32_t C, uint32_t pops_per_node,
                                 ReparentResult &res, const RunConst &g, hipStream_t stream, struct porrt_reparent_policies_info &info, std::string &err) {
    const double t0 = now_s();
    const uint64_t n = in.n;
    const std::string W_ = std::string(who) + ": ";
    res.valid = false;
    if (!(radius >= 0.0) || std::isinf(radius)) { err = W_ + "the radius must be finite and not negative"; return PORRT_ERR_INVALID; }
    if (C < 1 || C > kReparentMaxTreeNodesLimit || pops_per_node < 1 || pops_per_node > 64) { err = W_ + "reparent_max_tree_nodes: 1 .. 2^15, reparent_max_pops_per_node: 1 .. 64"; return PORRT_ERR_INVALID; }
    if (in.pol_off && n < (1ull << 31))
        for (uint64_t k = 0, T = in.pol_off[n]; in.original && k < T; ++k)
            if (in.original[k] >= gr.n) { err = W_ + "an original id that is no node of the graph"; return PORRT_ERR_INVALID; }
    res.off.assign(n + 1, 0); res.status.assign(n, 0); res.cost.assign(n, 0.0);
    res.xy.clear(); res.original.clear(); res.parent.clear(); res.leaf.clear();
    RefinePoliciesOut out{res.off.data(), res.status.data(), res.cost.data(), nullptr, nullptr, nullptr, nullptr, 0};
    RefineDecomposed dc;
    const int dr = refine_decompose(h, W_, in, out, g, stream, dc, err);
    if (dr < 0) return dr;
    info = {};
    info.policies = n;
    if (dr == 1) {                                                   // nothing but empty policies: no launch
        for (uint64_t q = 0; q < n; ++q) res.status[q] = 1;
        if (n) err = W_ + "policy 0: no policy to refine";
        res.valid = true;
        info.ms_wall = 1e3 * (now_s() - t0);
        return 0;
    }
    if (!g.has_grid) { err = W_ + "the refiner checks transitions on the context's grid (porrt_set_grid)"; return PORRT_ERR_INVALID; }
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    // the jobs: the pieces of the policies the decomposition accepted, in policy order
    std::vector<ReparentJob> jobs;
    std::vector<uint32_t> job_first(n, kRefNone);
    for (uint64_t q = 0; q < n; ++q) {
        const RefinePolRecord &r = dc.rec[q];
        res.status[q] = (uint8_t)r.status;
        if (r.status) continue;
        job_first[q] = (uint32_t)jobs.size();
        for (uint32_t i = 0; i < r.pieces; ++i) jobs.push_back(ReparentJob{(uint32_t)q, i});
        info.pieces += r.pieces;
    }
    const size_t J = jobs.size();
    if (J >= (1ull << 31)) { err = W_ + "fewer than 2^31 pieces in all"; return PORRT_ERR_INVALID; }
    // a slot: everything a piece needs, sized by C alone
    uint32_t H = 2, hbits = 1;
    while (H < 2 * C) { H <<= 1; ++hbits; }
    uint32_t F = 1;
    while (F < kReparentFifoPerNode * C) F <<= 1;
    const uint32_t P = kReparentPairsPerNode * C;
    const size_t slot_bytes = (size_t)C * (4 * 8 + 4 * 4 + 1) + (size_t)(C + 1) * 4 + (size_t)H * 4 + (size_t)F * 8 + (size_t)P * 4 + 16 * 16;
    const size_t S = std::max<size_t>(1, std::min<size_t>(J, kReparentBudget / slot_bytes));
    std::vector<ReparentRec> rec(J);
    std::vector<unsigned long long> pool_off(J + 1, 0ull);
    uint8_t *dj = nullptr, *ds = nullptr;
    const size_t j_jobs = 0, j_rec = j_jobs + up16(J * sizeof(ReparentJob)), j_pool = j_rec + up16(J * sizeof(ReparentRec)), j_first = j_pool + up16(J * 8),
                 j_woff = j_first + up16(n * 4), j_hang = j_woff + up16(J * 4), j_bytes = j_hang + up16(J * 4);
    HIPCHK_ERR(h.scratch.get(5, dj, j_bytes));
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up16(bytes); return o; };
    const size_t s_tx = take(S * C * 8), s_ty = take(S * C * 8), s_tc = take(S * C * 8), s_pr = take(S * C * 8), s_tg = take(S * C * 4), s_tp = take(S * C * 4),
                 s_nc = take(S * C * 4), s_ch = take(S * C * 4), s_no = take(S * (size_t)(C + 1) * 4), s_ha = take(S * (size_t)H * 4), s_fi = take(S * (size_t)F * 8),
                 s_nb = take(S * (size_t)P * 4), s_wi = take(S * C);
    HIPCHK_ERR(h.scratch.get(6, ds, at));
    HIPCHK_ERR(h.rp_events());
    ReparentConst c{};
    c.pc = dc.pc; c.gr = gr; c.rc = (const RunConst *)dc.d; c.compat = (const unsigned long long *)(dc.d + dc.o_cp);
    c.jobs = (const ReparentJob *)(dj + j_jobs); c.rec = (ReparentRec *)(dj + j_rec); c.pool_off = (const unsigned long long *)(dj + j_pool);
    c.C = C; c.H = H; c.hash_shift = 32u - hbits; c.F = F; c.fifo_live = kReparentFifoPerNode * C; c.pairs_cap = P; c.pops_per_node = pops_per_node;
    c.radius = radius; c.half = 0.5 * radius;
    c.tx = (double *)(ds + s_tx); c.ty = (double *)(ds + s_ty); c.tcost = (double *)(ds + s_tc); c.prio = (double *)(ds + s_pr);
    c.tg = (uint32_t *)(ds + s_tg); c.tpar = (uint32_t *)(ds + s_tp); c.ncnt = (uint32_t *)(ds + s_nc); c.chain = (uint32_t *)(ds + s_ch);
    c.noff = (uint32_t *)(ds + s_no); c.hash = (uint32_t *)(ds + s_ha); c.fifo = (uint2 *)(ds + s_fi); c.nbr = (uint32_t *)(ds + s_nb); c.win = ds + s_wi;
    if (J) HIPCHK_ERR(hipMemcpyAsync(dj + j_jobs, jobs.data(), J * sizeof(ReparentJob), hipMemcpyHostToDevice, stream));
    // the pool of recomposed rows: x | y | id.  It starts with a row per policy node going in (a chain is longer than its piece only
    // through rounding or copies) and is grown to what is needed, contents kept, when a round's chains do not fit
    int pool_slot = 7;
    size_t pool_rows = 0;
    uint8_t *dp = nullptr;
    auto pool_view = [&](uint8_t *p, size_t rows) { c.px = (double *)p; c.py = (double *)(p + up16(rows * 8)); c.pg = (uint32_t *)(p + 2 * up16(rows * 8)); };
    auto pool_bytes = [&](size_t rows) { return 2 * up16(rows * 8) + up16(rows * 4); };
    {
        pool_rows = std::max<size_t>(1, dc.T);
        HIPCHK_ERR(h.scratch.get(pool_slot, dp, pool_bytes(pool_rows)));
        pool_view(dp, pool_rows);
    }
    uint64_t total_rows = 0;
    const uint32_t near_y = (uint32_t)std::min<size_t>(64, (C + 3) / 4);
    for (size_t j0 = 0; j0 < J; j0 += S) {
        const uint32_t m = (uint32_t)std::min(S, J - j0);
        c.first = (uint32_t)j0;
        HIPCHK_ERR(hipEventRecord(h.rp_ev[0], stream));
        hipLaunchKernelGGL(k_reparent_tube, dim3(m), dim3(64), 0, stream, c);
        HIPCHK_ERR(hipGetLastError());
        HIPCHK_ERR(hipEventRecord(h.rp_ev[1], stream));
        hipLaunchKernelGGL(k_reparent_near<false>, dim3(m, near_y), dim3(256), 0, stream, c);
        hipLaunchKernelGGL(k_reparent_scan, dim3(m), dim3(256), 0, stream, c);
        hipLaunchKernelGGL(k_reparent_near<true>, dim3(m, near_y), dim3(256), 0, stream, c);
        HIPCHK_ERR(hipGetLastError());
        HIPCHK_ERR(hipEventRecord(h.rp_ev[2], stream));
        hipLaunchKernelGGL(k_reparent_pop, dim3(m), dim3(256), 0, stream, c);
        HIPCHK_ERR(hipGetLastError());
        HIPCHK_ERR(hipEventRecord(h.rp_ev[3], stream));
        HIPCHK_ERR(hipMemcpyAsync(rec.data() + j0, dj + j_rec + j0 * sizeof(ReparentRec), m * sizeof(ReparentRec), hipMemcpyDeviceToHost, stream));
        HIPCHK_ERR(hipStreamSynchronize(stream));
        for (uint32_t k = 0; k < m; ++k) {
            pool_off[j0 + k] = total_rows;
            if (!rec[j0 + k].flags) total_rows += rec[j0 + k].chain;
        }
        if (total_rows > pool_rows) {                                // grow the pool, keeping what the rounds before wrote
            const size_t new_rows = total_rows;
            const double *ox = c.px, *oy = c.py;
            const uint32_t *og = c.pg;
            uint8_t *np = nullptr;
            pool_slot = pool_slot == 7 ? 8 : 7;
            HIPCHK_ERR(h.scratch.get(pool_slot, np, pool_bytes(new_rows)));
            pool_view(np, new_rows);
            const size_t kept = (size_t)pool_off[j0];
            if (kept) {
                HIPCHK_ERR(hipMemcpyAsync(c.px, ox, kept * 8, hipMemcpyDeviceToDevice, stream));
                HIPCHK_ERR(hipMemcpyAsync(c.py, oy, kept * 8, hipMemcpyDeviceToDevice, stream));
                HIPCHK_ERR(hipMemcpyAsync(c.pg, og, kept * 4, hipMemcpyDeviceToDevice, stream));
            }
            pool_rows = new_rows;
        }
        HIPCHK_ERR(hipMemcpyAsync(dj + j_pool + j0 * 8, pool_off.data() + j0, m * 8, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_reparent_emit, dim3(m), dim3(64), 0, stream, c);
        HIPCHK_ERR(hipGetLastError());
        float ms[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < 3; ++k) HIPCHK_ERR(hipEventElapsedTime(&ms[k], h.rp_ev[k], h.rp_ev[k + 1]));
        info.ms_tube += ms[0]; info.ms_neighbours += ms[1]; info.ms_pop += ms[2];
        ++info.rounds;
    }
    // the policies' statuses and where their rows go
    uint64_t M = 0;
    for (uint64_t q = 0; q < n; ++q) {
        uint32_t st = res.status[q], flags = 0;
        uint64_t rows = 0;
        if (!st) {
            for (uint32_t i = 0; i < dc.rec[q].pieces; ++i) {
                const ReparentRec &r = rec[job_first[q] + i];
                flags |= r.flags;
                rows += r.chain;
                info.tree_nodes += r.n_tree; info.max_tree = std::max<uint64_t>(info.max_tree, r.n_tree);
                info.pairs += r.pairs; info.pops += r.pops; info.reparents += r.reparents;
            }
            st = (flags & RP_CAP) ? 4u : (flags & RP_RASTER) ? 2u : (flags & RP_POPS) ? 5u : 0u;
        }
        res.status[q] = (uint8_t)st;
        if (st) { job_first[q] = kRefNone; rows = 0; }
        res.off[q + 1] = res.off[q] + rows;
        M += rows;
    }
    if (M >= (1ull << 31)) { err = W_ + "fewer than 2^31 recomposed nodes in all"; return PORRT_ERR_CAPACITY; }
    // recomposition and costs; in: ref_off | work rows; out: cost | xy | original ids | parents | leafs
    const size_t r_off = 0, r_q = r_off + up16((n + 1) * 8), r_t = r_q + up16(M * 8), r_p = r_t + up16(M * 8), r_v = r_p + up16(M * 8), r_cost = r_v + up16(M * 8),
                 r_xy = r_cost + up16(n * 8), r_or = r_xy + up16(M * 16), r_pa = r_or + up16(M * 8), r_lf = r_pa + up16(M * 8), bytes3 = r_lf + up16(M);
    uint8_t *d3 = nullptr;
    HIPCHK_ERR(h.scratch.get(9, d3, bytes3));
    ReparentOut ro{};
    ro.pol_off = dc.pc.pol_off; ro.any = dc.pc.any; ro.prec = dc.pc.rec; ro.job_first = (const uint32_t *)(dj + j_first); ro.rec = c.rec; ro.pool_off = c.pool_off;
    ro.px = c.px; ro.py = c.py; ro.pg = c.pg; ro.gr = gr; ro.beliefs = dc.pc.beliefs; ro.nw = in.nw;
    ro.w_off = (uint32_t *)(dj + j_woff); ro.w_hang = (int32_t *)(dj + j_hang);
    ro.wq = (double *)(d3 + r_q); ro.wt = (double *)(d3 + r_t); ro.wp = (double *)(d3 + r_p); ro.wv = (double *)(d3 + r_v);
    ro.ref_off = (const unsigned long long *)(d3 + r_off); ro.cost = (double *)(d3 + r_cost); ro.out_xy = (double *)(d3 + r_xy);
    ro.out_orig = (unsigned long long *)(d3 + r_or); ro.out_parent = (long long *)(d3 + r_pa); ro.out_leaf = d3 + r_lf;
    HIPCHK_ERR(hipMemcpyAsync(dj + j_first, job_first.data(), n * 4, hipMemcpyHostToDevice, stream));
    HIPCHK_ERR(hipMemcpyAsync(d3 + r_off, res.off.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream));
    HIPCHK_ERR(hipEventRecord(h.rp_ev[0], stream));
    hipLaunchKernelGGL(k_reparent_recompose, dim3((uint32_t)n), dim3(64), 0, stream, ro);
    HIPCHK_ERR(hipGetLastError());
    HIPCHK_ERR(hipEventRecord(h.rp_ev[1], stream));
    std::vector<uint8_t> third(bytes3 - r_cost);
    HIPCHK_ERR(hipMemcpyAsync(third.data(), d3 + r_cost, bytes3 - r_cost, hipMemcpyDeviceToHost, stream));
    HIPCHK_ERR(hipStreamSynchronize(stream));
    {
        float ms = 0.0f;
        HIPCHK_ERR(hipEventElapsedTime(&ms, h.rp_ev[0], h.rp_ev[1]));
        info.ms_recompose = ms;
    }
    memcpy(res.cost.data(), third.data(), n * 8);
    res.xy.resize(2 * M); res.original.resize(M); res.parent.resize(M); res.leaf.resize(M);
    if (M) {
        memcpy(res.xy.data(), third.data() + (r_xy - r_cost), M * 16);
        memcpy(res.original.data(), third.data() + (r_or - r_cost), M * 8);
        memcpy(res.parent.data(), third.data() + (r_pa - r_cost), M * 8);
        memcpy(res.leaf.data(), third.data() + (r_lf - r_cost), M);
    }
    for (uint64_t q = 0; q < n; ++q) info.ok += res.status[q] == 0;
    for (uint64_t q = 0; q < n; ++q)
        if (res.status[q]) { err = W_ + "policy " + std::to_string(q) + ": " + kReparentStatusText[res.status[q] < 6 ? res.status[q] : 0]; break; }
    res.valid = true;
    info.nodes = M;
    info.ms_wall = 1e3 * (now_s() - t0);
    return (int64_t)M;
}

// copies a result into the caller's arrays (the node arrays when cap holds the total)
static int64_t reparent_copy_out(const ReparentResult &res, uint64_t *ref_off, uint8_t *status, double *expected_costs, double *xy, uint64_t *original_ids,
                                 int64_t *parents, uint8_t *is_leaf, uint64_t cap) {
    const uint64_t n = res.status.size(), total = res.off.back();
    if (ref_off) memcpy(ref_off, res.off.data(), (n + 1) * 8);
    if (n && status) memcpy(status, res.status.data(), n);
    if (n && expected_costs) memcpy(expected_costs, res.cost.data(), n * 8);
    if (total && total <= cap) {
        if (xy) memcpy(xy, res.xy.data(), total * 16);
        if (original_ids) memcpy(original_ids, res.original.data(), total * 8);
        if (parents) memcpy(parents, res.parent.data(), total * 8);
        if (is_leaf) memcpy(is_leaf, res.leaf.data(), total);
    }
    return (int64_t)total;
}

} // namespace porrt
