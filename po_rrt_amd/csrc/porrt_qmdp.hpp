// porrt_qmdp.hpp -- the QMDP policy extractor (src/qmdp_policy_extractor.rs) on the device.
//
// plan_qmdp (:23-35): one dijkstra per world over PTOGraphWorldView (pto_graph.rs:245-303) from that world's final nodes
// (pto_reachability.rs:58-63).  Its fixpoint:
//     dist_w[n] = 0                                         n final for world w
//     dist_w[u] = min over v in children(u) of dist_w[v] + norm2(u, v)        u valid in world w (validities[nodes[u].validity_id][w])
//     dist_w[u] = +inf                                      otherwise
// The view filters the PARENT u of a relaxation (graph.parents(v) keeps the parents whose own validity has the world), not the
// edge's validity and not v.
//
// Layout: ONE graph, n_worlds cost fields over it, node-major: cost[n * Wp + w], Wp = n_worlds rounded up to 16 (the padding
// stays +inf).  A 16-lane group owns a dirty node u: it walks children(u) once, computes norm2(u, v) once per child, and lane l
// relaxes world l, l + 16, ..: the child's costs come in as one coalesced 128-byte read per 16 worlds, and an adjacency entry
// costs 4 B + 8 B per world per sweep.  One dirty byte per node; an improvement in ANY world marks the node's parents.
//
// Order of evaluation: as for PRM::plan_path (porrt_prm.hpp) the relaxation is monotone -- a value only ever falls, each value
// is dist[v] + norm2 of some child v in f64, and a node stays dirty until it has been evaluated against its children's current
// values -- so every order of evaluation, the reference's queue (which re-pushes on improvement) included, ends in the same
// fixpoint, bit for bit.  A reader that meets a child's cost while its owner lowers it reads the old or the new value (8-byte
// stores); the owner marks the reader dirty for the next sweep either way.
//
// react_qmdp (:38-123): get_common_path by one wave per query, get_path by one wave per (query, world), both in two passes
// (count, then write) as k_prm_walk.
#pragma once
#include "../../include/porrt_hip.h"
#include "porrt_device.hpp"
#include <string>

namespace porrt {

constexpr uint32_t kQmdpLanes = 16;                       // lanes per node of the sweep
constexpr uint32_t kQmdpMaxPlanes = 4;                    // 64 worlds / 16 lanes
constexpr uint32_t kQmdpWalkOver = 0xFFFFFFFFu;           // a walk that would emit more than L states

// cost planes at their start: 0 where the node is final for the world (zero[n]: reach & final mask of a final node), +inf elsewhere
__global__ __launch_bounds__(256) void k_qmdp_init(uint32_t N, uint32_t Wp, const unsigned long long *__restrict__ zero, double *__restrict__ cost) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)N * Wp) return;
    const uint32_t n = (uint32_t)(i / Wp), w = (uint32_t)(i % Wp);
    cost[i] = (w < 64u && ((zero[n] >> w) & 1ull)) ? 0.0 : __builtin_huge_val();
}

// One sweep: the 16-lane group g of the grid owns node g.  valid[u]: the worlds in which node u is valid.  par_off / par_id: who
// has u among its children (to be evaluated again when u improves); on a PTO graph every edge goes both ways and the lists are
// the children lists.  flags[slot] = 1 when any cost fell (plain stores: every writer writes 1).
__global__ __launch_bounds__(256) void k_qmdp_sweep(uint32_t N, uint32_t Wp, const unsigned long long *__restrict__ child_off,
                                                    const uint32_t *__restrict__ child_id, const unsigned long long *__restrict__ par_off,
                                                    const uint32_t *__restrict__ par_id, const double *__restrict__ nx, const double *__restrict__ ny,
                                                    const unsigned long long *__restrict__ valid, double *__restrict__ cost,
                                                    uint8_t *__restrict__ dirty_in, uint8_t *__restrict__ dirty_out, uint32_t *__restrict__ flags, uint32_t slot) {
    const uint32_t u = (blockIdx.x * blockDim.x + threadIdx.x) / kQmdpLanes, l = threadIdx.x % kQmdpLanes;
    const bool work = u < N && as_global(dirty_in)[u] != 0;
    bool improved = false;
    if (work) {
        const uint32_t planes = Wp / kQmdpLanes;
        double *mine = cost + (size_t)u * Wp + l;
        double old[kQmdpMaxPlanes], best[kQmdpMaxPlanes];
#pragma unroll
        for (uint32_t j = 0; j < kQmdpMaxPlanes; ++j) old[j] = best[j] = j < planes ? as_global(mine)[j * kQmdpLanes] : 0.0;
        const double xu = as_global(nx)[u], yu = as_global(ny)[u];
        const unsigned long long a0 = as_global(child_off)[u], a1 = as_global(child_off)[u + 1];
        for (unsigned long long k = a0; k < a1; ++k) {
            const uint32_t v = as_global(child_id)[k];
            const double d = sqrt(dist2(xu, yu, as_global(nx)[v], as_global(ny)[v]));         // cost_evaluator(u.state, v.state) = norm2
            const double *theirs = cost + (size_t)v * Wp + l;
#pragma unroll
            for (uint32_t j = 0; j < kQmdpMaxPlanes; ++j)
                if (j < planes) {
                    const double a = as_global(theirs)[j * kQmdpLanes] + d;                    // dist[v] + cost(u, v)
                    best[j] = a < best[j] ? a : best[j];
                }
        }
        const unsigned long long vu = as_global(valid)[u];
#pragma unroll
        for (uint32_t j = 0; j < kQmdpMaxPlanes; ++j) {
            const uint32_t w = l + j * kQmdpLanes;
            // the view keeps u as a parent only where u itself is valid; a final node's 0 stays (nothing is below 0)
            if (j < planes && w < 64u && ((vu >> w) & 1ull) && old[j] != 0.0 && best[j] < old[j]) {
                as_global(mine)[j * kQmdpLanes] = best[j];
                improved = true;
            }
        }
    }
    // (all lanes of the wave are here: the ballot is taken outside the divergent part)
    const unsigned long long ballot = __ballot(improved);
    if (!work) return;
    if (l == 0) as_global(dirty_in)[u] = 0;
    const uint32_t grp = (threadIdx.x & 63u) / kQmdpLanes;
    if ((ballot >> (grp * kQmdpLanes)) & 0xFFFFull) {
        const unsigned long long p0 = as_global(par_off)[u], p1 = as_global(par_off)[u + 1];
        for (unsigned long long k = p0 + l; k < p1; k += kQmdpLanes) as_global(dirty_out)[as_global(par_id)[k]] = 1;
        if (l == 0) as_global(flags)[slot] = 1;
    }
}

// node-major planes -> the interface's world-major rows: out[w * N + n] = cost[n * Wp + w]
__global__ __launch_bounds__(256) void k_qmdp_rows(uint32_t N, uint32_t W, uint32_t Wp, const double *__restrict__ cost, double *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)N * W) return;
    const uint32_t w = (uint32_t)(i / N), n = (uint32_t)(i % N);
    out[i] = cost[(size_t)n * Wp + w];
}

struct QmdpWalk {
    uint32_t N, W, Wp, nq, L;
    const unsigned long long *child_off;
    const uint32_t *child_id;
    const double *nx, *ny, *cost;
    const uint32_t *start;            // [nq] nearest node of the query's start
    const double *belief;             // [nq * W]
    const double *horizon;            // [nq]
    uint32_t *clen;                   // [nq] states of the common path (kQmdpWalkOver: more than L)
    uint32_t *end_id;                 // [nq] the node the common path ended on (not part of it)
    uint32_t *plen;                   // [nq * W] states of get_path (kQmdpWalkOver: more than L)
    const unsigned long long *off;    // [nq * W] write pass: first state of paths[w] of query q
    double *out;
};

// get_common_path (:65-87) with get_best_expected_child (:90-108), one wave per query.  Lanes stride the children list; a lane sums
// its child's expected cost over the worlds in order (E = 0.0; E += cost[w][child] * belief[w]: no contraction) and keeps its
// first child with E below its best so far, which starts at +inf: a NaN (inf * 0.0) or +inf never qualifies.  The butterfly keeps
// the least (E, list position) -- the first strict minimum of the whole list.  Without a winner the walk goes to node 0 with cost
// +inf (the reference's initial values).  WRITE = false counts (clen, end_id); WRITE = true writes the states into the common
// prefix of all W paths of the query (lane w writes world w, w + 64 never exists: W <= 64).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_qmdp_common(QmdpWalk p) {
    const uint32_t q = (blockIdx.x * blockDim.x + threadIdx.x) / 64u, lane = threadIdx.x & 63u;
    if (q >= p.nq) return;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    if (WRITE && as_global(p.clen)[q] == kQmdpWalkOver) return;
    const double *B = p.belief + (size_t)q * p.W;
    const double H = as_global(p.horizon)[q];
    double *o = (WRITE && lane < p.W) ? p.out + 2 * as_global(p.off)[(size_t)q * p.W + lane] : nullptr;
    uint32_t id = as_global(p.start)[q], cnt = 0;
    double acc = 0.0, best = __builtin_huge_val();
    bool over = false;
    while (acc < H && best > 0.0) {
        if (cnt >= p.L) { over = true; break; }
        const double xn = as_global(p.nx)[id], yn = as_global(p.ny)[id];
        if (WRITE && o) { o[2 * (size_t)cnt] = xn; o[2 * (size_t)cnt + 1] = yn; }
        ++cnt;
        const unsigned long long a0 = as_global(p.child_off)[id], a1 = as_global(p.child_off)[id + 1];
        double bc = __builtin_huge_val();
        uint32_t bp = kNone;
        for (unsigned long long k = a0 + lane; k < a1; k += 64u) {
            const double *C = p.cost + (size_t)as_global(p.child_id)[k] * p.Wp;
            double E = 0.0;
            for (uint32_t w = 0; w < p.W; ++w) E += as_global(C)[w] * as_global(B)[w];
            if (E < bc) { bc = E; bp = (uint32_t)(k - a0); }
        }
        wave_first_min(bc, bp);
        const uint32_t c = bp == kNone ? 0u : as_global(p.child_id)[a0 + bp];
        acc += sqrt(dist2(xn, yn, as_global(p.nx)[c], as_global(p.ny)[c]));
        id = c;
        best = bp == kNone ? __builtin_huge_val() : bc;
    }
    if (!WRITE && lane == 0) { p.clen[q] = over ? kQmdpWalkOver : cnt; p.end_id[q] = id; }
}

// get_path (:51-62) with get_best_child (:110-123), one wave per (query, world): from the node the common path ended on, while its
// cost in the world is above 0 push it and go to the first child of strictly least cost[w][child] (the child's cost alone; from
// (+inf, node 0): no child below +inf sends the walk to node 0).  The node of cost 0 is not pushed.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_qmdp_path(QmdpWalk p) {
    const uint32_t j = (blockIdx.x * blockDim.x + threadIdx.x) / 64u, lane = threadIdx.x & 63u;
    if (j >= p.nq * p.W) return;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const uint32_t q = j / p.W, w = j % p.W;
    const uint32_t cl = as_global(p.clen)[q];
    if (cl == kQmdpWalkOver) { if (!WRITE && lane == 0) p.plen[j] = 0; return; }
    if (WRITE && as_global(p.plen)[j] == kQmdpWalkOver) return;
    double *o = WRITE ? p.out + 2 * (as_global(p.off)[j] + cl) : nullptr;
    const double *D = p.cost + w;
    uint32_t id = as_global(p.end_id)[q], cnt = 0;
    bool over = false;
    while (as_global(D)[(size_t)id * p.Wp] > 0.0) {
        if (cnt >= p.L) { over = true; break; }
        if (WRITE && lane == 0) { o[2 * (size_t)cnt] = as_global(p.nx)[id]; o[2 * (size_t)cnt + 1] = as_global(p.ny)[id]; }
        ++cnt;
        const unsigned long long a0 = as_global(p.child_off)[id], a1 = as_global(p.child_off)[id + 1];
        double bc = __builtin_huge_val();
        uint32_t bp = kNone;
        for (unsigned long long k = a0 + lane; k < a1; k += 64u) {
            const double c = as_global(D)[(size_t)as_global(p.child_id)[k] * p.Wp];
            if (c < bc) { bc = c; bp = (uint32_t)(k - a0); }
        }
        wave_first_min(bc, bp);
        id = bp == kNone ? 0u : as_global(p.child_id)[a0 + bp];
    }
    if (!WRITE && lane == 0) p.plen[j] = over ? kQmdpWalkOver : cnt;
}

// The cost planes of a graph whose arrays are on the device: init, then sweeps until one changes nothing (sweep_to_fixpoint: eight
// between two looks at the flags, as PRM::plan_path's; the planes are its one row).  zero / valid: one word per node.  dirty: 2 * N
// bytes, flags: 8 words.
static int qmdp_solve(uint32_t N, uint32_t Wp, const unsigned long long *child_off, const uint32_t *child_id, const unsigned long long *par_off,
                      const uint32_t *par_id, const double *nx, const double *ny, const unsigned long long *zero, const unsigned long long *valid,
                      double *cost, uint8_t *dirty, uint32_t *flags, hipStream_t stream, uint64_t &sweeps, std::string &err) {
    uint8_t *dirty_ab[2] = {dirty, dirty + N};
    const size_t cells = (size_t)N * Wp;
    hipLaunchKernelGGL(k_qmdp_init, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, N, Wp, zero, cost);
    hipError_t e = hipMemsetAsync(dirty_ab[0], 1, N, stream);        // the first sweep evaluates every node
    if (e == hipSuccess) e = hipMemsetAsync(dirty_ab[1], 0, N, stream);
    if (e != hipSuccess) { err = std::string("qmdp: dirty flags: ") + hipGetErrorString(e); return PORRT_ERR_DEVICE; }
    const dim3 grid((unsigned)(((size_t)N * kQmdpLanes + 255) / 256));
    return sweep_to_fixpoint(stream, flags, 1, 0,
        [&](uint32_t k, int cur) {
            hipLaunchKernelGGL(k_qmdp_sweep, grid, dim3(256), 0, stream, N, Wp, child_off, child_id, par_off, par_id, nx, ny, valid, cost,
                               dirty_ab[cur], dirty_ab[cur ^ 1], flags, k);
        },
        [](const std::vector<uint32_t> &) { return hipSuccess; }, "qmdp", sweeps, err);
}

// porrt_qmdp_plan's result on a context: the planes stay on the device for porrt_qmdp_react; they belong to the graph of
// results_tag `tag` (a new growth makes them stale).
struct QmdpState {
    bool valid = false;
    uint64_t tag = ~0ull;
    uint32_t N = 0, W = 0, Wp = 0;
    double *d_cost = nullptr;
    struct porrt_qmdp_info info = {};
};

} // namespace porrt
