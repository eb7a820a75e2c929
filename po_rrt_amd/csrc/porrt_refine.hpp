// porrt_refine.hpp -- PTOPolicyRefiner::refine_solution(RefinmentStrategy::PartialShortCut(n)) (src/pto_policy_refiner.rs:87-124).
//
// The policy is cut into pieces (Policy::decompose, common.rs:85-129): breadth-first from policy node 0, a piece follows single
// children until a node with 0 or >= 2 children; the children of a branching node start the next pieces, in children order.
// Every piece of >= 3 nodes is shortcut on its own (partial_shortcut, pto_policy_refiner.rs:158-207): with a fresh
// DiscreteSampler::new() (Pcg64, seed 0) per piece, n iterations of
//     joint = gen_range(0..2), s = gen_range(0..len-2), e = s + 2 + gen_range(0..len-s-2)
//     candidate(j) = state(j) with [joint] = a * (1 - l) + b * l,  l = (j - s) / (e - s),  a, b = [joint] of nodes s and e,  j in [s, e)
//     commit all of [s, e) iff every transition candidate(j) -> candidate(j + 1) and candidate(e - 1) -> state(e) is valid
// where valid = both states have a validity (state_validity) and the segment's validity (transition_validator) is compatible
// with the piece's belief (is_transition_valid, :395-423).  The draws never depend on the commits, so they are a function of
// the piece length alone: the host makes them once per distinct length (shortcut_draws, porrt_refine_batch.hpp) and uploads them.
//
// Device (refine_shortcut_piece): one wave per piece of >= 3 nodes, all pieces of a call in one launch.  The iterations run in
// order inside the wave; per iteration the lanes stride over [s, e), each forms its candidate and the next one, classifies the
// two states and the segment with the growth's own state_class / traversed_class (summed-area table first), the verdict is
// reduced across the wave (first rejected transition in path order: the reference's `&&` stops there, so a raster fault behind
// it is never reached), and the lanes that own the nodes commit.  Piece states live in LDS up to kLds nodes; longer pieces work
// in place in global memory (the same code through a generic pointer).
//
// The pieces are put back together (recompose, :324-393) in piece order, nodes in path order: inside a piece each node is the child
// of the one before, then the skeleton edges from the end of piece i to the start of each piece its last node's children start.  The
// expected cost is the recursion of common.rs:131-154 from node 0: the sum over the children in ascending id order of
// p * q * cost + rec(p * q, child), q = transition_probability (common.rs:187-190), cost = norm2 (pto_graph.rs:150).
// Quirk kept from the reference: recompose records a piece's start with `if is_start .. else if is_end` (:348-366), so a
// one-node piece has a start but no end.  When such a piece branches, its skeleton edges are never added: its successor
// pieces keep no parent (parents = -1) and the one node becomes a leaf.  Nodes the walk from node 0 does not reach belong to no piece.
//
// This file holds what the shortcut of one piece needs, shared with the TAMP planner's path shortcut (k_tamp_shortcut,
// porrt_tamp.hpp).  Decomposition, launch order, recomposition and expected costs are the kernels of porrt_refine_batch.hpp, one
// policy or many: they are this specification's only implementation (the single calls are batches of one).
#pragma once
#include "porrt_device.hpp"

#include <cmath>
#include <string>
#include <vector>

namespace porrt {

constexpr uint32_t kRefineLdsNodes = 1024;       // piece states kept in LDS: 2 x 8 KiB per wave

struct RefinePiece {
    uint32_t off;            // first state of the piece in RefineConst::x / y
    uint32_t len;            // nodes (>= 3)
    uint32_t draws;          // first draw of its length in RefineConst::draws
    uint32_t belief;         // row of RefineConst::compat
};

struct RefineConst {
    const RunConst *rc;                  // raster, summed-area table, domain, validities
    const RefinePiece *pieces;
    const uint2 *draws;                  // per distinct length, n_iter entries: (s | joint << 31, e)
    const unsigned long long *compat;    // per belief: bit v = compatible with world validity v
    double *x, *y;                       // piece states, refined in place
    uint32_t *err;
    uint32_t n_pieces, n_iter;
};

// is_transition_valid (pto_policy_refiner.rs:395-423): 0 valid, 1 rejected, 2 raster fault (the reference panics there).
// The reference evaluates both state validities and only then, when both are Some, the segment.  Here the segment is classified
// beside the states (its loads go out with theirs: one trip to memory fewer per iteration) and its fault counts only where the
// reference would have looked at it.
__device__ __forceinline__ uint32_t refine_transition(const RunConst &rc, const TableGrid &grid, double fx, double fy, double tx, double ty,
                                                      unsigned long long compat) {
    uint32_t err = 0;
    const int vf = class_to_validity(rc, state_class(rc, fx, fy, &err));
    const int vt = class_to_validity(rc, state_class(rc, tx, ty, &err));
    const uint32_t err_states = err;
    const int v = class_to_validity(rc, traversed_class(rc, grid, fx, fy, tx, ty, &err));
    if (err_states) return 2u;
    if (vf < 0 || vt < 0) return 1u;
    if (err) return 2u;
    return (v >= 0 && ((compat >> v) & 1ull)) ? 0u : 1u;
}

// interpolate (pto_policy_refiner.rs:160-162) at lambda = (j - s) as f64 / (e - s) as f64
__device__ __forceinline__ double refine_lerp(double a, double b, uint32_t j, uint32_t s, uint32_t e) {
    const double lambda = (double)(j - s) / (double)(e - s);
    return a * (1.0 - lambda) + b * lambda;
}

// kTamp: MapShelfDomainTampRRT::shortcut (map_shelves_tamp_rrt.rs:565-617) instead -- the same draws (a fresh DiscreteSampler::new()
// per path, n = 100), one wave per path, but a transition is valid iff its traversed space is Free (RTTFuncs, :43-45: no state
// check, no belief) and the step from the last candidate into node e is not checked at all.
//
// One piece on one wave.  Piece: RefinePiece, or a descriptor with the same off / len / draws / belief (the batch refiner's carries
// its policy too, porrt_refine_batch.hpp); kLds: the piece states kept in LDS (a second, smaller array for a launch of short pieces
// only); err: the word a raster fault is OR-ed into.  c gives the raster, the draws, the compatibilities, the states and n_iter.
template <bool kTamp, uint32_t kLds, class Piece>
__device__ __forceinline__ void refine_shortcut_piece(const RefineConst &c, const Piece &pc, uint32_t *err_word) {
    __shared__ double lx[kLds], ly[kLds];
    const uint32_t lane = threadIdx.x;
    const RunConst &rc = *c.rc;
    const bool in_lds = pc.len <= kLds;
    double *X = in_lds ? lx : c.x + pc.off;
    double *Y = in_lds ? ly : c.y + pc.off;
    if (in_lds)
        for (uint32_t j = lane; j < pc.len; j += 64) { lx[j] = as_global(c.x)[pc.off + j]; ly[j] = as_global(c.y)[pc.off + j]; }
    __syncthreads();
    TableGrid grid;
    grid.p = rc.cls; grid.W = rc.W;
    const unsigned long long compat = kTamp ? 0ull : as_global(c.compat)[pc.belief];
    const uint2 *dr = c.draws + pc.draws;
    bool fault = false;
    uint2 ahead = make_uint2(0u, 2u);             // the draws do not depend on the commits: lane l holds the draw of iteration it0 + l
    for (uint32_t it = 0; it < c.n_iter && !fault; ++it) {
        if ((it & 63u) == 0u) ahead = it + lane < c.n_iter ? dr[it + lane] : make_uint2(0u, 2u);
        const uint2 d = make_uint2((uint32_t)__shfl((int)ahead.x, (int)(it & 63u)), (uint32_t)__shfl((int)ahead.y, (int)(it & 63u)));
        const uint32_t s = d.x & 0x7FFFFFFFu, e = d.y;
        const bool jy = (d.x >> 31) != 0u;
        double *J = jy ? Y : X;                   // the joint that moves
        const double a = J[s], b = J[e];
        bool commit = true;
        for (uint32_t j0 = s; j0 < e; j0 += 64) {
            const uint32_t j = j0 + lane;
            uint32_t st = 0;
            if (j < e) {
                double fx = X[j], fy = Y[j], tx = X[j + 1], ty = Y[j + 1];
                const double cj = refine_lerp(a, b, j, s, e);
                if (jy) fy = cj; else fx = cj;
                if (j + 1 < e) {                  // the next candidate; the last one goes to node e itself
                    const double cn = refine_lerp(a, b, j + 1, s, e);
                    if (jy) ty = cn; else tx = cn;
                }
                if (!kTamp) {
                    st = refine_transition(rc, grid, fx, fy, tx, ty, compat);
                } else if (j + 1 < e) {           // the TAMP shortcut never looks at the step into node e
                    uint32_t terr = 0;
                    const int cls = traversed_class(rc, grid, fx, fy, tx, ty, &terr);
                    st = terr ? 2u : (cls == CLS_FREE ? 0u : 1u);
                }
            }
            const unsigned long long bad = __ballot(st != 0u);
            if (bad) {                            // the first transition in path order decides: rejected, or a fault
                const int first = __ffsll((long long)bad) - 1;
                fault = __shfl((int)st, first) == 2;
                commit = false;
                break;
            }
        }
        if (commit)
            for (uint32_t j = s + lane; j < e; j += 64) J[j] = refine_lerp(a, b, j, s, e);
        __syncthreads();
    }
    if (in_lds)
        for (uint32_t j = lane; j < pc.len; j += 64) { as_global(c.x)[pc.off + j] = lx[j]; as_global(c.y)[pc.off + j] = ly[j]; }
    if (fault && lane == 0) atomicOr(err_word, ERR_RASTER);
}

// the TAMP planner's launch (porrt_tamp.hpp): one wave per path, RefineConst::pieces / n_pieces / err are its alone
__global__ __launch_bounds__(64) void k_tamp_shortcut(RefineConst c) { refine_shortcut_piece<true, kRefineLdsNodes>(c, c.pieces[blockIdx.x], c.err); }

} // namespace porrt
