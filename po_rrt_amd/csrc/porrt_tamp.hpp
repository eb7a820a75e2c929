// porrt_tamp.hpp -- MapShelfDomainTampRRT::plan(.., TampSearch::BranchAndBound) (src/map_shelves_tamp_rrt.rs:159-291), the
// reference's third planner, with its RRT queries grown on the device.
//
// The search is the reference's depth-first branch and bound over zone orders: a stack of search nodes; a popped node makes one
// child per remaining zone (a fresh shuffle of its remaining zones per child, from the planner's discrete sampler), runs two RRT
// queries per child (to see the zone, then to pick the object up from where it was seen), and pushes the child iff its expected
// cost is below the best leaf's so far.  A popped node without remaining zones is a leaf; among leaves of the lowest cost the last
// popped one wins (BTreeMap::insert replaces an equal key).  The policy is the chain root .. best leaf, every path shortcut
// (:565-617, k_tamp_shortcut) and the expected cost of common.rs:131-154.
//
// Two stream modes ("tamp_streams"):
//   0  the reference's: one context (the lead) grows every query in order, its continuous stream running on across the queries;
//      the stream is set back to its value at entry when the plan returns (the reference's RRT starts from a clone of the sampler).
//   1  (default) one stream per search edge: the edge with zone prefix z_1 .. z_d runs its two queries back to back on a context
//      seeded with h_d, h_0 = the lead's sampler seed, h_k = splitmix64(h_{k-1} ^ (z_k + 1)).  A node's cost is then a function of its
//      prefix alone and only grows along a branch, so the best leaf does not depend on the order of expansion: up to "tamp_wave"
//      nodes are popped at once, all their children's observation queries grow in one porrt_grow_batch on worker contexts of a pool
//      ("tamp_pool" contexts, made on first use, kept across calls, freed with the lead), their best paths are gathered on the
//      device (k_best_path), the pickup queries grow in a second batch, and the children are pushed in the sequential order.
// Both modes draw the shuffles from the lead's discrete sampler (porrt_set_discrete_seed; RRT growth never draws from it), which
// runs on across plans.
// Many such plans on one map in one call, each with a discrete sampler of its own, are porrt_tamp_bnb_batch.hpp (DESIGN.md
// section 28); the search cut into operations a driver of many can call is porrt_bnb_search.hpp.
#pragma once

#include <algorithm>
#include <functional>
#include <memory>
#include <tuple>
#include <utility>
#include <vector>

#include "porrt_astar_search.hpp"
#include "porrt_bnb_search.hpp"

namespace {

constexpr uint32_t kTampPathSlot = 1024;      // states of one query's best path (a longer one is PORRT_ERR_CAPACITY, never cut short)
constexpr uint32_t kTampShortcutIterations = 100;   // map_shelves_tamp_rrt.rs:581

// the stream and belief arithmetic of a search edge (splitmix64, edge_seed, normalize, transition_probability, child_belief) is that
// of the host-only porrt_astar_search.hpp, the shuffles are those of porrt_bnb_search.hpp: one statement of each for the searches

struct TampNode {
    int32_t target = -1;
    int64_t parent = -1;
    std::vector<uint32_t> remaining;
    double ox = 0, oy = 0;                     // observation_state
    double rp = 1.0, ec = 0.0;
    std::vector<double> belief;
    uint64_t h = 0;                            // stream seed of the edge into this node (tamp_streams = 1)
    std::vector<double> path_obs, path_pick;   // root first, x y interleaved
    double obs_cost = 0, pick_cost = 0;
};

// The slots of TampState::scratch and who owns each; a new user takes a new name at the end.
enum TampSlot : size_t {
    kSlotBestMeta = 0,        // tamp_gather: BestPath per row
    kSlotPathArena,           // tamp_gather: the rows' paths
    kSlotPathCursor,          // tamp_gather: the arena's cursor
    kSlotShortcut,            // tamp_shortcut_device: its staging area
    kSlotSolIds,              // solutions_select (porrt_solutions.hpp): id arena
    kSlotSolLens,             //   lengths beside the ids
    kSlotSolRows,             //   SolRow per row
    kSlotSolCursor,           //   the id arena's cursor
    kSlotSolBases,            // solutions_write: SolBase per row
    kSlotSolOut,              //   ids | lens | costs
    kSlotSolXy,               //   states
    kSlotAstarCursor,         // tamp_plan_astar (porrt_tamp_astar.hpp): the plan arena's cursor
    kSlotAstarZonePos,        //   zone positions
    kSlotAstarChildIn,        //   k_astar_children: AstarChildIn per child
    kSlotAstarBeliefs,        //   belief rows of a wave
    kSlotAstarChildOut,       //   AstarChildOut per child
    kSlotAstarPick,           //   BestPath per pickup row
    // the A* plan's BestPath per observation row shares tamp_gather's buffer: safe because tamp_plan_astar gathers with
    // tamp_best_paths into its own arena and never calls tamp_gather, and no other call runs on the context during a plan
    kSlotAstarObs = kSlotBestMeta,
};

struct TampState {
    int device = 0;
    std::vector<porrt_ctx *> pool;
    uint64_t pool_raster_gen = 0;
    GrowScratch scratch;                       // slots: TampSlot
    bool valid = false;
    uint32_t nw = 0;
    std::vector<double> xy, beliefs;
    std::vector<int64_t> parents;
    std::vector<uint8_t> leaf;
    porrt_tamp_info info;
    porrt_tamp_viewpoints_info vinfo;          // what porrt_tamp_rrt_plan_viewpoints adds (porrt_tamp_viewpoints.hpp); zero after a plan of the other kind
    std::shared_ptr<void> astar;               // what porrt_tamp_rrt_plan_astar keeps (porrt_tamp_astar.hpp): path arena, search nodes, its info
    TampState() { memset(&info, 0, sizeof info); memset(&vinfo, 0, sizeof vinfo); info.fail_node = -1; info.fail_zone = -1; info.fail_query = -1; }
    ~TampState() {
        for (porrt_ctx *p : pool) porrt_destroy(p);
        (void)hipSetDevice(device);
        scratch.free_all();
    }
};

static TampState &tamp_state(porrt_ctx *c) {
    if (!c->tamp) {
        TampState *t = new TampState();
        t->device = c->device;
        c->tamp = std::shared_ptr<void>(t, [](void *q) { delete (TampState *)q; });
    }
    return *(TampState *)c->tamp.get();
}

// a worker context sees what the lead sees: raster, zones, sampler box
static void tamp_copy_domain(porrt_ctx *d, const porrt_ctx *s) {
    d->occ = s->occ; d->zones = s->zones;
    d->W = s->W; d->H = s->H;
    d->low[0] = s->low[0]; d->low[1] = s->low[1]; d->up[0] = s->up[0]; d->up[1] = s->up[1]; d->ppm = s->ppm;
    d->domain = s->domain; d->has_grid = s->has_grid;
    d->visibility = s->visibility;
    d->n_zones = s->n_zones; d->n_worlds = s->n_worlds; d->n_validities = s->n_validities;
    memcpy(d->zone_pos, s->zone_pos, sizeof d->zone_pos);
    memcpy(d->validities, s->validities, sizeof d->validities);
    d->s_low[0] = s->s_low[0]; d->s_low[1] = s->s_low[1]; d->s_up[0] = s->s_up[0]; d->s_up[1] = s->s_up[1];
    d->opt_box_table = s->opt_box_table;
    d->cls_dirty = true;
    ++d->raster_gen;
}

static int tamp_ensure_pool(porrt_ctx *c, TampState &T, uint32_t want) {
    if (T.pool_raster_gen != c->raster_gen) {
        for (porrt_ctx *p : T.pool) tamp_copy_domain(p, c);
        T.pool_raster_gen = c->raster_gen;
    }
    if (T.pool.size() >= want) return PORRT_OK;
    const double t0 = now_s();
    while (T.pool.size() < want) {
        porrt_ctx *p = porrt_create(c->device);
        if (!p) { c->set_err("tamp: a worker context could not be created"); return PORRT_ERR_DEVICE; }
        tamp_copy_domain(p, c);
        T.pool.push_back(p);
    }
    T.pool_raster_gen = c->raster_gen;
    T.info.pool_s += now_s() - t0;
    return PORRT_OK;
}

// k_best_cost + k_best_path of the rows ctxs[0 .. n) after their growth, on c's stream: one launch triple per run of the argument
// (porrt_batch_run), a context outside a run alone.  Row q's path is appended to `arena` through the cursor *d_cur in a slot of
// kTampPathSlot states, its record goes to d_meta[q]; nothing is downloaded.
static int tamp_best_paths(porrt_ctx *c, porrt_ctx *const *ctxs, uint32_t n, double2 *arena, uint32_t *d_cur, BestPath *d_meta) {
    hipStream_t st = c->stream;
    for (uint32_t q0 = 0; q0 < n;) {
        const BatchRows B = porrt_batch_rows(ctxs, n, q0);
        if (B.rows == 1 && !ctxs[q0]->have_results) { c->set_err("tamp: a query has no results"); return PORRT_ERR_INVALID; }
        hipLaunchKernelGGL(k_best_path_reset, dim3(1, B.rows), dim3(64), 0, st, B.rcp);
        hipLaunchKernelGGL(k_best_cost, dim3(1, B.rows), dim3(1024), 0, st, B.rcp, B.steps);
        hipLaunchKernelGGL(k_best_path, dim3(1, B.rows), dim3(64), 0, st, B.rcp, q0, kTampPathSlot, arena, d_cur, d_meta);
        HIPCHK_CTX(c, hipGetLastError());
        q0 += B.rows;
    }
    return PORRT_OK;
}

// The best path of every row ctxs[0 .. n) after its growth (rrt.rs:183-193, 223-227): tamp_best_paths into scratch, one download
// of the rows' descriptors, one of the paths.  paths[q] root first; ok[q] = 0 for "No solution found".
static int tamp_gather(porrt_ctx *c, TampState &T, porrt_ctx *const *ctxs, uint32_t n, std::vector<std::vector<double>> &paths,
                       std::vector<double> &costs, std::vector<char> &ok) {
    const double t0 = now_s();
    HIPCHK_CTX(c, hipSetDevice(c->device));
    BestPath *d_meta = nullptr;
    double2 *d_arena = nullptr;
    uint32_t *d_cur = nullptr;
    HIPCHK_CTX(c, T.scratch.get(kSlotBestMeta, d_meta, n));
    HIPCHK_CTX(c, T.scratch.get(kSlotPathArena, d_arena, (size_t)n * kTampPathSlot));
    HIPCHK_CTX(c, T.scratch.get(kSlotPathCursor, d_cur, 1));
    hipStream_t st = c->stream;
    HIPCHK_CTX(c, hipMemsetAsync(d_cur, 0, sizeof(uint32_t), st));
    const int rb = tamp_best_paths(c, ctxs, n, d_arena, d_cur, d_meta);
    if (rb < 0) return rb;
    std::vector<BestPath> meta(n);
    HIPCHK_CTX(c, hipMemcpyAsync(meta.data(), d_meta, n * sizeof(BestPath), hipMemcpyDeviceToHost, st));
    HIPCHK_CTX(c, hipStreamSynchronize(st));
    size_t total = 0;
    for (const BestPath &b : meta) if (b.status == 0) total = std::max<size_t>(total, (size_t)b.off + b.len);
    std::vector<double2> arena(total);
    if (total) {
        HIPCHK_CTX(c, hipMemcpyAsync(arena.data(), d_arena, total * sizeof(double2), hipMemcpyDeviceToHost, st));
        HIPCHK_CTX(c, hipStreamSynchronize(st));
    }
    paths.assign(n, {});
    costs.assign(n, 0.0);
    ok.assign(n, 0);
    for (uint32_t q = 0; q < n; ++q) {
        const BestPath &b = meta[q];
        if (b.status == 3) { c->set_err("tamp: a best path longer than its slot of " + std::to_string(kTampPathSlot) + " states"); return PORRT_ERR_CAPACITY; }
        if (b.status == 1) continue;
        if (b.status == 2) {                     // k_best_cost's scratch was too small: the host walk
            double hc = 0;
            const uint64_t len = porrt_best_solution(ctxs[q], nullptr, 0, &hc);
            if (!len) continue;
            paths[q].resize(2 * len);
            porrt_best_solution(ctxs[q], paths[q].data(), len, &hc);
            costs[q] = hc; ok[q] = 1;
            continue;
        }
        paths[q].resize(2 * (size_t)b.len);
        for (uint32_t k = 0; k < b.len; ++k) { paths[q][2 * k] = arena[b.off + k].x; paths[q][2 * k + 1] = arena[b.off + k].y; }
        costs[q] = b.cost; ok[q] = 1;
    }
    T.info.path_s += now_s() - t0;
    return PORRT_OK;
}

// the device-resident input form of tamp_shortcut_device: path i is `len` states of `arena` from paths[i].src on (k_astar_chain
// copies them into the staging planes; paths[i].dst is filled in here)
struct TampChainSource {
    const double2 *arena = nullptr;
    std::vector<AstarChainPath> paths;
    hipEvent_t ev = nullptr;                   // the caller's: recorded before k_astar_chain
    double chain_s = 0.0;                      // out: k_astar_chain on the device
};

// shortcut (map_shelves_tamp_rrt.rs:565-617) of every path, in place: one wave per path of >= 3 states, one launch.  With `src` the
// states come from the device (xy is only written: every path as it leaves the shortcut, the short ones copied).
static int tamp_shortcut_device(porrt_ctx *c, TampState &T, std::vector<double> &xy, const std::vector<uint64_t> &off, double *dev_s,
                                TampChainSource *src = nullptr) {
    const size_t n_paths = off.size() - 1, ns = off.back();
    std::vector<RefinePiece> longs;
    std::vector<std::pair<uint32_t, uint32_t>> len_at;
    std::unordered_map<uint32_t, uint32_t> draws_of;
    const uint32_t n_iter = kTampShortcutIterations;
    for (size_t i = 0; i < n_paths; ++i) {
        const uint64_t len = off[i + 1] - off[i];
        if (len <= 2) continue;                  // :570-572
        if (len >= (1ull << 31)) { c->set_err("tamp_shortcut: a path of 2^31 states or more"); return PORRT_ERR_INVALID; }
        auto found = draws_of.find((uint32_t)len);
        uint32_t at;
        if (found == draws_of.end()) { at = (uint32_t)(len_at.size() * n_iter); len_at.push_back({(uint32_t)len, at}); draws_of[(uint32_t)len] = at; }
        else at = found->second;
        longs.push_back({(uint32_t)off[i], (uint32_t)len, at, 0u});
    }
    if (dev_s) *dev_s = 0.0;
    if (longs.empty() && (!src || ns == 0)) return PORRT_OK;
    if (ns >= (1ull << 31)) { c->set_err("tamp_shortcut: too many states"); return PORRT_ERR_INVALID; }
    HIPCHK_CTX(c, hipSetDevice(c->device));
    RunConst g;
    memset(&g, 0, sizeof g);
    const int r = c->refine_raster(g);
    if (r) return r;
    // one staging area: RunConst | paths | draws | x | y | error word
    auto up8 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t nd = len_at.size() * n_iter;
    const size_t o_pc = up8(sizeof(RunConst)), o_dr = o_pc + up8(longs.size() * sizeof(RefinePiece)), o_x = o_dr + up8(nd * sizeof(uint2)),
                 o_y = o_x + ns * 8, o_err = o_y + ns * 8, o_cp = o_err + 16, bytes = o_cp + (src ? n_paths * sizeof(AstarChainPath) : 0);
    std::vector<uint8_t> stage(bytes, 0);
    memcpy(stage.data(), &g, sizeof g);
    memcpy(stage.data() + o_pc, longs.data(), longs.size() * sizeof(RefinePiece));
    uint2 *dr = (uint2 *)(stage.data() + o_dr);
    for (const auto &la : len_at) shortcut_draws(la.first, n_iter, dr + la.second);      // DiscreteSampler::new() per path (:576-584)
    double *sx = (double *)(stage.data() + o_x), *sy = (double *)(stage.data() + o_y);
    if (src) {
        for (size_t i = 0; i < n_paths; ++i) { src->paths[i].dst = (uint32_t)off[i]; src->paths[i].len = (uint32_t)(off[i + 1] - off[i]); }
        memcpy(stage.data() + o_cp, src->paths.data(), n_paths * sizeof(AstarChainPath));
    } else {
        for (size_t k = 0; k < ns; ++k) { sx[k] = xy[2 * k]; sy[k] = xy[2 * k + 1]; }
    }
    uint8_t *d = nullptr;
    HIPCHK_CTX(c, T.scratch.get(kSlotShortcut, d, bytes));
    HIPCHK_CTX(c, c->refine.events());
    RefineConst rc{};
    rc.rc = (const RunConst *)d; rc.pieces = (const RefinePiece *)(d + o_pc); rc.compat = nullptr;
    rc.draws = (const uint2 *)(d + o_dr); rc.x = (double *)(d + o_x); rc.y = (double *)(d + o_y); rc.err = (uint32_t *)(d + o_err);
    rc.n_pieces = (uint32_t)longs.size(); rc.n_iter = n_iter;
    if (src) {                                   // the planes are filled on the device: everything but them goes up
        HIPCHK_CTX(c, hipMemcpyAsync(d, stage.data(), o_x, hipMemcpyHostToDevice, c->stream));
        HIPCHK_CTX(c, hipMemcpyAsync(d + o_err, stage.data() + o_err, bytes - o_err, hipMemcpyHostToDevice, c->stream));
        HIPCHK_CTX(c, hipEventRecord(src->ev, c->stream));
        hipLaunchKernelGGL(k_astar_chain, dim3((uint32_t)n_paths), dim3(64), 0, c->stream, (const AstarChainPath *)(d + o_cp), src->arena, rc.x, rc.y);
        HIPCHK_CTX(c, hipGetLastError());
    } else {
        HIPCHK_CTX(c, hipMemcpyAsync(d, stage.data(), bytes, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK_CTX(c, hipEventRecord(c->refine.ev[0], c->stream));
    if (rc.n_pieces) hipLaunchKernelGGL(k_tamp_shortcut, dim3(rc.n_pieces), dim3(64), 0, c->stream, rc);
    HIPCHK_CTX(c, hipGetLastError());
    HIPCHK_CTX(c, hipEventRecord(c->refine.ev[1], c->stream));
    HIPCHK_CTX(c, hipMemcpyAsync(stage.data() + o_x, d + o_x, o_cp - o_x, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_CTX(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIPCHK_CTX(c, hipEventElapsedTime(&ms, c->refine.ev[0], c->refine.ev[1]));
    if (dev_s) *dev_s = 1e-3 * (double)ms;
    if (src) {
        HIPCHK_CTX(c, hipEventElapsedTime(&ms, src->ev, c->refine.ev[0]));
        src->chain_s = 1e-3 * (double)ms;
    }
    uint32_t err = 0;
    memcpy(&err, stage.data() + o_err, 4);
    if (err) { c->set_err("tamp_shortcut: a segment reads outside the raster (the reference panics)"); return PORRT_ERR_RASTER; }
    for (size_t k = 0; k < ns; ++k) { xy[2 * k] = sx[k]; xy[2 * k + 1] = sy[k]; }
    return PORRT_OK;
}

static std::vector<uint32_t> tamp_shuffled(const std::vector<uint32_t> &v, Pcg64 &rng) { return porrt_bnb::shuffled(v, rng); }     // :20-32

// Policy::compute_expected_costs_to_goals (common.rs:131-154) from node 0: sum over the children in order of
// p * q * cost + rec(p * q, child), q = transition_probability (common.rs:187-190), cost = norm2 (pto_graph.rs:150).
// Children in ascending id order.  Evaluated with an explicit stack (a piece can be long).
template <class ProbOf>
static inline double tamp_expected_cost(const std::vector<int64_t> &parent, const std::vector<double> &xy, ProbOf q_of) {
    const size_t n = parent.size();
    if (n == 0) return 0.0;
    std::vector<uint32_t> off(n + 1, 0), ids;
    for (size_t k = 0; k < n; ++k) if (parent[k] >= 0) ++off[(size_t)parent[k] + 1];
    for (size_t k = 0; k < n; ++k) off[k + 1] += off[k];
    ids.resize(off[n]);
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    for (size_t k = 0; k < n; ++k) if (parent[k] >= 0) ids[fill[(size_t)parent[k]]++] = (uint32_t)k;
    struct Frame { uint32_t id, next; double p, acc, term; };
    std::vector<Frame> st{{0u, off[0], 1.0, 0.0, 0.0}};
    double ret = 0.0;
    while (true) {
        Frame &f = st.back();
        if (f.next < off[f.id + 1]) {
            const uint32_t c = ids[f.next++];
            const double q = q_of(f.id, c);
            double dx = xy[2 * c] - xy[2 * f.id], d2 = 0.0;
            d2 += dx * dx;
            dx = xy[2 * c + 1] - xy[2 * f.id + 1];
            d2 += dx * dx;
            f.term = f.p * q * std::sqrt(d2);
            const double pq = f.p * q;
            st.push_back({c, off[c], pq, 0.0, 0.0});
            continue;
        }
        ret = f.acc;
        st.pop_back();
        if (st.empty()) return ret;
        st.back().acc += st.back().term + ret;
    }
}

// The policy arrays of one plan, wherever they are kept: the single plans keep them in TampState, a batch per plan.
struct TampPolicyArrays {
    std::vector<double> &xy, &beliefs;
    std::vector<int64_t> &parents;
    std::vector<uint8_t> &leaf;
};

// the assembly half of build_policy (:619-663) for one chain of `depth` search nodes after the shortcut: node i's observation path
// is the states [off[2i], off[2i + 1]) of xy, its pickup path [off[2i + 1], off[2i + 2]); target[i] and belief[i] are the node's.
// Returns the policy's expected cost.
static double tamp_assemble_policy(uint32_t nw, size_t depth, const int32_t *target, const double *const *belief, const std::vector<double> &xy,
                                   const uint64_t *off, TampPolicyArrays P) {
    P.xy.clear(); P.parents.clear(); P.leaf.clear(); P.beliefs.clear();
    auto add = [&](double x, double y, const double *b, bool is_leaf) {
        P.xy.push_back(x); P.xy.push_back(y);
        P.parents.push_back(-1);
        P.leaf.push_back(is_leaf ? 1 : 0);
        P.beliefs.insert(P.beliefs.end(), b, b + nw);
        return (int64_t)P.parents.size() - 1;
    };
    int64_t last_obs = 0;
    for (size_t i = 0; i < depth; ++i) {
        int64_t prev = last_obs;
        for (uint64_t k = off[2 * i]; k < off[2 * i + 1]; ++k) {
            const int64_t id = add(xy[2 * k], xy[2 * k + 1], belief[i], false);
            if (id != prev) P.parents[(size_t)id] = prev;
            prev = id;
        }
        last_obs = prev;
        const uint64_t p0 = off[2 * i + 1], p1 = off[2 * i + 2];
        std::vector<double> b(belief[i], belief[i] + nw);
        if (p1 > p0) {
            for (uint32_t w = 0; w < nw; ++w) if ((int32_t)w != target[i]) b[w] = 0.0;
            porrt_astar::normalize(b);
        }
        for (uint64_t k = p0; k < p1; ++k) {
            const int64_t id = add(xy[2 * k], xy[2 * k + 1], b.data(), k + 1 == p1);
            if (id != prev) P.parents[(size_t)id] = prev;
            prev = id;
        }
    }
    return tamp_expected_cost(P.parents, P.xy, [&](uint32_t a, uint32_t b2) {
        return porrt_astar::transition_probability(P.beliefs.data() + (size_t)a * nw, P.beliefs.data() + (size_t)b2 * nw, nw);
    });
}

// build_policy (:619-663) on the chain root .. leaf: the shortcut of its paths on the device, then the assembly.
static int tamp_build_policy(porrt_ctx *c, TampState &T, const std::vector<TampNode> &nodes, int64_t leaf_id) {
    std::vector<int64_t> chain;
    for (int64_t k = leaf_id; k >= 0; k = nodes[(size_t)k].parent) chain.push_back(k);
    std::reverse(chain.begin(), chain.end());
    std::vector<double> xy;
    std::vector<uint64_t> off{0};
    std::vector<int32_t> target;
    std::vector<const double *> belief;
    for (int64_t k : chain) {
        const TampNode &sn = nodes[(size_t)k];
        xy.insert(xy.end(), sn.path_obs.begin(), sn.path_obs.end());
        off.push_back(xy.size() / 2);
        xy.insert(xy.end(), sn.path_pick.begin(), sn.path_pick.end());
        off.push_back(xy.size() / 2);
        target.push_back(sn.target);
        belief.push_back(sn.belief.data());
    }
    const double t0 = now_s();
    double dev_s = 0.0;
    const int r = tamp_shortcut_device(c, T, xy, off, &dev_s);
    if (r < 0) return r;
    T.info.shortcut_s = now_s() - t0;
    T.info.expected_cost = tamp_assemble_policy(T.nw, chain.size(), target.data(), belief.data(), xy, off.data(), {T.xy, T.beliefs, T.parents, T.leaf});
    return PORRT_OK;
}

static int tamp_fail(porrt_ctx *c, TampState &T, int64_t node, int32_t zone, int32_t query) {
    T.info.fail_node = node; T.info.fail_zone = zone; T.info.fail_query = query;
    c->set_err(std::string(query == 0 ? "no observation path found!" : "no pickup path found!") + " (search node " + std::to_string(node) +
               ", zone " + std::to_string(zone) + ")");
    return PORRT_ERR_NO_PATH;
}

// ---- what the three searches (this file, porrt_tamp_viewpoints.hpp, porrt_tamp_astar.hpp) share: DESIGN.md section 17

// a fresh shuffle of `remaining` without zone t: one per child, from the discrete sampler (the branch-and-bound searches only)
static std::vector<uint32_t> tamp_remaining_without(const std::vector<uint32_t> &remaining, uint32_t t, Pcg64 &rng) {
    return porrt_bnb::remaining_without(remaining, t, rng);
}

static std::vector<int64_t> tamp_chain(const std::vector<TampNode> &nodes, int64_t leaf) {     // root .. leaf
    std::vector<int64_t> chain;
    for (int64_t k = leaf; k >= 0; k = nodes[(size_t)k].parent) chain.push_back(k);
    std::reverse(chain.begin(), chain.end());
    return chain;
}

// One plan's frame: the entry checks and the reset of the state (begin), the growth parameters and the two ways to grow queries
// with their accounting (grow_lead, grow_rows), the guard of the lead's continuous stream, and the end of a plan (finish).
struct TampFrame {
    porrt_ctx *c = nullptr;
    TampState *T = nullptr;
    double max_step = 0, search_radius = 0, goal_radius = 0;
    uint64_t n_iter_min = 0, n_iter_max = 0;
    uint32_t K = 0, nw = 0, streams = 0, wave = 1, pool_cap = 1;
    const double t_start = now_s();
    Pcg64 crng0{};
    bool restore = false;                      // tamp_streams = 0: the lead's stream is set back however the plan ends
    TampFrame() = default;
    TampFrame(const TampFrame &) = delete;
    ~TampFrame() { if (restore) c->crng = crng0; }

    // The checks every search makes, in their order, then the state of a plan that has begun.  own(stage) holds the checks of one
    // search alone at their places among the common ones: stage 0 after the zone count, stage 1 after the prior's sum.
    int begin(porrt_ctx *ctx, const double start[2], const double *belief, uint32_t n_worlds, double max_step_, double search_radius_,
              uint64_t n_iter_min_, uint64_t n_iter_max_, double goal_radius_, uint32_t K_, const std::function<int(int)> &own = nullptr) {
        c = ctx;
        if (!c->has_grid || c->zones.empty() || c->domain != PORRT_DOMAIN_SHELF) { c->set_err("tamp: needs a shelf map with zones (porrt_set_grid, porrt_set_zones)"); return PORRT_ERR_INVALID; }
        if (!start || !belief || n_worlds != (uint32_t)c->n_zones) { c->set_err("tamp: n_worlds must equal the number of zones"); return PORRT_ERR_INVALID; }
        int r = own ? own(0) : PORRT_OK;
        if (r < 0) return r;
        double sum = 0.0;
        for (uint32_t w = 0; w < n_worlds; ++w) sum = sum + belief[w];
        if (!(std::fabs(sum - 1.0) < 0.001)) { c->set_err("tamp: the prior does not sum to 1 (check_belief_state, common.rs:390)"); return PORRT_ERR_INVALID; }
        if ((r = own ? own(1) : PORRT_OK) < 0) return r;
        if (K_ == 0 || K_ > 4096) { c->set_err("batch_K must be in 1..4096"); return PORRT_ERR_INVALID; }
        if (!(goal_radius_ >= 0.0)) { c->set_err("tamp: goal_radius"); return PORRT_ERR_INVALID; }
        max_step = max_step_; search_radius = search_radius_; goal_radius = goal_radius_;
        n_iter_min = n_iter_min_; n_iter_max = n_iter_max_; K = K_; nw = n_worlds;
        T = &tamp_state(c);
        T->valid = false;
        memset(&T->info, 0, sizeof T->info);
        memset(&T->vinfo, 0, sizeof T->vinfo);
        T->info.fail_node = -1; T->info.fail_zone = -1; T->info.fail_query = -1;
        T->nw = nw;
        streams = c->opt_tamp_streams ? 1u : 0u;
        wave = streams ? std::max<uint32_t>(1u, c->opt_tamp_wave) : 1u;
        pool_cap = std::max<uint32_t>(1u, c->opt_tamp_pool);
        T->info.streams = streams; T->info.wave = wave;
        crng0 = c->crng;
        restore = streams == 0;
        return PORRT_OK;
    }

    // the goal of a query on context x: which = 0 to see the zone, 1 to pick the object up at it
    int set_goal(porrt_ctx *x, uint32_t zone, int which) const {
        const uint64_t m1 = 1;
        return which == 0 ? porrt_set_observation_goal(x, zone) : porrt_set_square_goal(x, c->zone_pos[zone], &m1, 1, goal_radius);
    }
    // the same on a stream of its own: a worker context seeded for one search edge
    int seed_and_goal(porrt_ctx *x, uint64_t seed, uint32_t zone, int which) const {
        const int r = porrt_set_sampler(x, c->s_low, c->s_up, seed);
        return r < 0 ? r : set_goal(x, zone, which);
    }

    // one query on the lead, its stream running on
    int grow_lead(const double start[2], uint32_t zone, int which) {
        double t0 = now_s();
        int r = set_goal(c, zone, which);
        T->info.goals_s += now_s() - t0;
        if (r < 0) return r;
        t0 = now_s();
        r = c->grow(start, max_step, search_radius, n_iter_min, n_iter_max, K, PORRT_MODE_RRT);
        T->info.grow_s += now_s() - t0;
        ++T->info.queries;
        return r;
    }
    // m queries in one porrt_grow_batch on ctxs[0 .. m) from starts; set_row(i) gives row i its goal (and its seed, where the
    // search wants a fresh stream: that differs between the searches on purpose)
    template <class SetRow>
    int grow_rows(porrt_ctx *const *ctxs, uint32_t m, const double *starts, SetRow set_row) {
        double t0 = now_s();
        int r = PORRT_OK;
        for (uint32_t i = 0; i < m; ++i) if ((r = set_row(i)) < 0) return r;
        T->info.goals_s += now_s() - t0;
        t0 = now_s();
        r = porrt_grow_batch(ctxs, m, starts, max_step, search_radius, n_iter_min, n_iter_max, K, PORRT_MODE_RRT);
        T->info.grow_s += now_s() - t0;
        T->info.queries += m;
        if (r < 0) c->set_err(ctxs[0]->err);
        return r;
    }

    // The end of a plan that found `leaf`: search cost and zone order of the chain root .. leaf, the lead's stream set back, the
    // policy, the times.  extra_s: time the search accounts for outside search_s.
    int64_t finish(const std::vector<TampNode> &nodes, int64_t leaf, double extra_s = 0.0) {
        porrt_tamp_info &I = T->info;
        I.search_cost = nodes[(size_t)leaf].ec;
        I.n_order = 0;
        for (int64_t k : tamp_chain(nodes, leaf)) if (nodes[(size_t)k].parent >= 0) I.zone_order[I.n_order++] = (uint32_t)nodes[(size_t)k].target;
        if (restore) { c->crng = crng0; restore = false; }
        const int r = tamp_build_policy(c, *T, nodes, leaf);
        if (r < 0) return r;
        T->valid = true;
        close(extra_s);
        return (int64_t)T->parents.size();
    }
    // the pool and the seconds of a call that ends
    void close(double extra_s = 0.0) {
        porrt_tamp_info &I = T->info;
        I.pool = (uint32_t)T->pool.size();
        I.total_s = now_s() - t_start;
        I.search_s = I.total_s - I.grow_s - I.path_s - I.shortcut_s - I.pool_s - I.goals_s - extra_s;
    }
};

// the root of the branch-and-bound searches: every zone remaining, in a first shuffle
static TampNode tamp_root(porrt_ctx *c, const double start[2], const double *belief, uint32_t nw) {
    TampNode root;
    std::vector<uint32_t> all((size_t)c->n_zones);
    for (uint32_t z = 0; z < all.size(); ++z) all[z] = z;
    root.remaining = tamp_shuffled(all, c->drng);
    root.ox = start[0]; root.oy = start[1];
    root.belief.assign(belief, belief + nw);
    root.h = c->s_seed;
    return root;
}

// The branch and bound itself: the stack, the best leaf's cost so far and the leaf that holds it.
struct TampBound {
    std::vector<int64_t> stack{0};
    double best = std::numeric_limits<double>::infinity();
    int64_t best_leaf = -1;
    std::vector<int64_t> pop(uint32_t wave) {
        std::vector<int64_t> popped;
        while (!stack.empty() && popped.size() < wave) { popped.push_back(stack.back()); stack.pop_back(); }
        return popped;
    }
    // node uid has been expanded; kids are its children in the sequential order, their queries done.  A child is pushed iff its
    // expected cost is below the best leaf's so far; among leaves of the lowest cost the last one wins.
    void close(TampState &T, std::vector<TampNode> &nodes, int64_t uid, const std::vector<int64_t> &kids) {
        const TampNode &u = nodes[(size_t)uid];
        for (int64_t vid : kids) {
            TampNode &v = nodes[(size_t)vid];
            v.ec = u.ec + v.rp * (v.obs_cost + v.belief[(size_t)v.target] * v.pick_cost);
            if (v.ec < best) stack.push_back(vid);
            else ++T.info.pruned;
        }
        if (u.remaining.empty()) {
            if (u.ec < best) best = u.ec;
            if (best_leaf < 0 || u.ec <= nodes[(size_t)best_leaf].ec) best_leaf = uid;
        }
    }
};

static int64_t tamp_plan(porrt_ctx *c, const double start[2], const double *belief, uint32_t nw, double max_step, double search_radius,
                         uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t K) {
    TampFrame F;
    if (c->opt_tamp_search != 0) {
        c->set_err(c->opt_tamp_search == 1 ? "tamp: TampSearch::AStar has an entry point of its own: porrt_tamp_rrt_plan_astar"
                                           : "tamp: TampSearch::BranchAndBoundMultipleViewPoints has an entry point of its own: porrt_tamp_rrt_plan_viewpoints");
        return PORRT_ERR_INVALID;
    }
    int r = F.begin(c, start, belief, nw, max_step, search_radius, n_iter_min, n_iter_max, goal_radius, K);
    if (r < 0) return r;
    TampState &T = *F.T;
    std::vector<TampNode> nodes{tamp_root(c, start, belief, nw)};
    TampBound B;
    std::vector<std::vector<double>> paths;
    std::vector<double> costs;
    std::vector<char> ok;
    while (!B.stack.empty()) {
        const std::vector<int64_t> popped = B.pop(F.wave);
        ++T.info.waves;
        // children in the sequential order, with their shuffles
        std::vector<std::pair<int64_t, std::vector<int64_t>>> made;
        std::vector<int64_t> edges;
        for (int64_t uid : popped) {
            std::vector<int64_t> kids;
            const std::vector<uint32_t> rem_u = nodes[(size_t)uid].remaining;
            for (uint32_t t : rem_u) {
                TampNode v;
                v.remaining = tamp_remaining_without(rem_u, t, c->drng);
                const TampNode &u = nodes[(size_t)uid];
                std::tie(v.belief, v.rp) = porrt_astar::child_belief(u.belief.data(), u.target, u.rp, nw);
                v.target = (int32_t)t;
                v.parent = uid;
                v.h = porrt_astar::edge_seed(u.h, t);
                kids.push_back((int64_t)nodes.size());
                edges.push_back((int64_t)nodes.size());
                nodes.push_back(std::move(v));
            }
            made.push_back({uid, std::move(kids)});
        }
        T.info.search_nodes = nodes.size();
        // the queries
        if (F.streams == 0) {
            for (int64_t vid : edges) {
                TampNode &v = nodes[(size_t)vid];
                const TampNode &u = nodes[(size_t)v.parent];
                for (int which = 0; which < 2; ++which) {
                    const double st[2] = {which == 0 ? u.ox : v.ox, which == 0 ? u.oy : v.oy};
                    if ((r = F.grow_lead(st, (uint32_t)v.target, which)) < 0) return r;
                    porrt_ctx *one = c;
                    if ((r = tamp_gather(c, T, &one, 1, paths, costs, ok)) < 0) return r;
                    if (!ok[0]) return tamp_fail(c, T, vid, v.target, which);
                    if (which == 0) {
                        v.path_obs = std::move(paths[0]); v.obs_cost = costs[0];
                        v.ox = v.path_obs[v.path_obs.size() - 2]; v.oy = v.path_obs.back();
                    } else {
                        v.path_pick = std::move(paths[0]); v.pick_cost = costs[0];
                    }
                }
            }
        } else {
            for (size_t e0 = 0; e0 < edges.size(); e0 += F.pool_cap) {
                const uint32_t m = (uint32_t)std::min<size_t>(F.pool_cap, edges.size() - e0);
                if ((r = tamp_ensure_pool(c, T, m)) < 0) return r;
                std::vector<double> starts(2 * (size_t)m);
                for (uint32_t i = 0; i < m; ++i) {
                    const TampNode &u = nodes[(size_t)nodes[(size_t)edges[e0 + i]].parent];
                    starts[2 * i] = u.ox; starts[2 * i + 1] = u.oy;
                }
                r = F.grow_rows(T.pool.data(), m, starts.data(), [&](uint32_t i) {
                    const TampNode &v = nodes[(size_t)edges[e0 + i]];
                    return F.seed_and_goal(T.pool[i], v.h, (uint32_t)v.target, 0);
                });
                if (r < 0) return r;
                if ((r = tamp_gather(c, T, T.pool.data(), m, paths, costs, ok)) < 0) return r;
                uint32_t first_bad = m;
                for (uint32_t i = 0; i < m && first_bad == m; ++i) if (!ok[i]) first_bad = i;
                for (uint32_t i = 0; i < first_bad; ++i) {
                    TampNode &v = nodes[(size_t)edges[e0 + i]];
                    v.path_obs = std::move(paths[i]); v.obs_cost = costs[i];
                    v.ox = v.path_obs[v.path_obs.size() - 2]; v.oy = v.path_obs.back();
                    starts[2 * i] = v.ox; starts[2 * i + 1] = v.oy;
                }
                // the pickup queries of the rows before the first failure, on the same contexts: their streams run on
                const uint32_t mp = first_bad;
                if (mp) {
                    r = F.grow_rows(T.pool.data(), mp, starts.data(), [&](uint32_t i) { return F.set_goal(T.pool[i], (uint32_t)nodes[(size_t)edges[e0 + i]].target, 1); });
                    if (r < 0) return r;
                    if ((r = tamp_gather(c, T, T.pool.data(), mp, paths, costs, ok)) < 0) return r;
                    for (uint32_t i = 0; i < mp; ++i) {
                        TampNode &v = nodes[(size_t)edges[e0 + i]];
                        if (!ok[i]) return tamp_fail(c, T, edges[e0 + i], v.target, 1);
                        v.path_pick = std::move(paths[i]); v.pick_cost = costs[i];
                    }
                }
                if (first_bad < m) return tamp_fail(c, T, edges[e0 + first_bad], nodes[(size_t)edges[e0 + first_bad]].target, 0);
            }
        }
        // push the children, record the leaves: the sequential order
        for (const auto &mk : made) B.close(T, nodes, mk.first, mk.second);
    }
    T.info.search_nodes = nodes.size();
    return F.finish(nodes, B.best_leaf);
}

} // namespace
