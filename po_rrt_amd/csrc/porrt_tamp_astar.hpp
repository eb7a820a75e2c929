// porrt_tamp_astar.hpp -- MapShelfDomainTampRRT::plan(.., TampSearch::AStar) (plan_astar, src/map_shelves_tamp_rrt.rs:432-563) with
// its RRT* queries grown on the device and their paths kept there.
//
// The reference's loop: a priority queue of search nodes; the node u of lowest priority is popped and makes one child per remaining
// zone IN ORDER (the root's zones are 0 .. n, a child's are its parent's without its own: A* draws no shuffle, the discrete sampler
// is not touched).  Per child v of zone t:
//     v.belief = u.belief with u.target zeroed, normalised;  v.rp = u.rp * transition_probability(u.belief, v.belief)
//     observation query from u.observation_state, pickup query from where the zone was seen
//     v.ec = u.ec + v.rp * (obs_cost + v.belief[t] * pickup_cost)
//     h = fold from 0.0 over v.remaining in order: h + v.belief[z] * norm2(v.observation_state, zone_pos[z])
//     priority = v.ec + v.rp * h
// A popped node without remaining zones is the solution and ends the loop (:546-550): the first popped leaf wins.  build_policy and
// the shortcut are those of porrt_tamp.hpp.
//
// OURS, not the reference's: Priority's Ord never says Equal (common.rs:235-239), so the reference's order among equal priorities is
// its heap's, not the algorithm's.  Here (porrt_astar_queue.hpp) bit-equal priorities pop in ASCENDING SEARCH NODE ID, ids given
// in the sequential order: a node's children get the next ids, in zone order, at the moment the node is popped.  +0.0 and -0.0 are
// equal.  A prior with an entry that is not > 0 is PORRT_ERR_INVALID at entry: below the last positive zone the reference's
// normalisation divides 0 by 0 and every priority is NaN, for which Ord is no order.
//
// Streams ("tamp_streams") as in porrt_tamp.hpp: 0 = the lead's own stream across the queries in the sequential order, set back on
// return, wave forced to 1; 1 (default) = one stream per search edge, h = splitmix64(u.h ^ (t + 1)), both queries back to back on it.
// In mode 1 a node's cost and priority are functions of its zone prefix alone, which allows SPECULATION ("tamp_wave" = W): the queue
// is kept; pops are replayed while the top is a leaf or already has its children computed (popping gives the children their ids and
// pushes them); when the top has no computed children, it and the next best non-leaf queue entries without children, up to W in all,
// are expanded together -- all their observation queries in one porrt_grow_batch (chunked by "tamp_pool"), then all their pickup
// queries -- and the children are kept at the parent.  They enter the queue only when their parent is popped in the replay, so the
// pop sequence, every id, ec and priority, and the policy are those of W = 1; only queries, waves and `speculated` differ.  A query
// without a path fails the plan only when its parent is popped; fail_node is the id the child would have got.
//
// Device: the paths of all children stay in an arena that lives across the waves of a plan (k_best_path appends through the arena's
// cursor, which is not reset per gather); k_astar_children turns a wave's BestPath records into one record per child (ec, priority,
// observation state, costs, arena offsets), the only thing the search fetches besides the observation queries' own records (the
// pickup batch starts from the observation end states, which porrt_grow_batch takes from the host); k_astar_chain copies the
// 2 x depth paths of the winning chain into the shortcut's staging planes, where k_tamp_shortcut runs on them unchanged.
//
// What is one plan's own -- tables, queue, replay, selection, the failure rule -- is porrt_astar::Search, and the rounds are
// porrt_astar::run (porrt_astar_search.hpp, host only).  This file is the device side of those rounds (SearchRun, a template over
// the search type: AstarRun here, the branch and bound's in porrt_tamp_bnb_batch.hpp) and the two callers: tamp_plan_astar, the
// driver with one plan, and tamp_plan_astar_batch, the same driver over many plans on one map whose rows
// share the batches, the arena, one k_astar_children per chunk and one k_astar_chain / k_tamp_shortcut at the end.  With per-edge
// streams a plan of a batch is, bit for bit, the plan it is alone.
#pragma once

#include "porrt_astar_search.hpp"

namespace {

using AstarSearch = porrt_astar::Search;
using AstarEdge = porrt_astar::Edge;
using AstarChildRecord = porrt_astar::ChildRecord;

struct AstarBatchPlan {                        // one plan of the last batch call, of either search
    porrt_tamp_batch_plan rec;
    uint64_t pruned = 0;                       // branch and bound: children not pushed
    std::vector<double> xy, beliefs;           // its policy (empty for a failed plan)
    std::vector<int64_t> parents;
    std::vector<uint8_t> leaf;
    std::vector<int64_t> node_parents;         // its search nodes, in id order
    std::vector<int32_t> node_targets;
    std::vector<double> node_ec, node_priority;      // priority: A* only
    std::vector<uint8_t> node_pushed;          // branch and bound only
};

struct AstarState {
    double2 *arena = nullptr;                  // path arena of the running call; kept across calls, its cursor is not
    size_t arena_cap = 0;                      // states
    size_t cursor_ub = 0;                      // no gather has written at or beyond this state
    hipEvent_t ev = nullptr;
    porrt_tamp_astar_info info;
    std::vector<int64_t> parents;              // the last single plan's search nodes, in id order
    std::vector<int32_t> targets;
    std::vector<double> ec, priority;
    std::vector<AstarBatchPlan> batch;         // the last batch call's plans
    uint32_t batch_nw = 0;
    bool batch_bnb = false;                    // the last batch was porrt_tamp_rrt_plan_batch (porrt_tamp_bnb_batch.hpp)
    AstarState() { memset(&info, 0, sizeof info); }
    ~AstarState() {
        if (arena) (void)hipFree(arena);
        if (ev) (void)hipEventDestroy(ev);
    }
};

static AstarState &astar_state(TampState &T) {
    if (!T.astar) T.astar = std::shared_ptr<void>(new AstarState(), [](void *q) { delete (AstarState *)q; });
    return *(AstarState *)T.astar.get();
}

// room for `states` states: the arena grows by allocating and copying device to device, never by cutting a path
static int astar_arena_reserve(porrt_ctx *c, AstarState &A, size_t states) {
    if (states <= A.arena_cap) return PORRT_OK;
    if (states >= (1ull << 32)) { c->set_err("tamp astar: the path arena would pass 2^32 states"); return PORRT_ERR_CAPACITY; }
    const size_t cap = std::min<size_t>(std::max<size_t>(states, 2 * A.arena_cap), (1ull << 32) - 1);
    double2 *p = nullptr;
    if (hipMalloc((void **)&p, cap * sizeof(double2)) != hipSuccess) {
        (void)hipGetLastError();
        c->set_err("tamp astar: the path arena cannot grow to " + std::to_string(cap) + " states");
        return PORRT_ERR_CAPACITY;
    }
    if (A.arena) {
        const size_t keep = std::min(A.cursor_ub, A.arena_cap);
        if (keep) HIPCHK_CTX(c, hipMemcpyAsync(p, A.arena, keep * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK_CTX(c, hipStreamSynchronize(c->stream));
        (void)hipFree(A.arena);
        ++A.info.arena_grown;
    }
    A.arena = p; A.arena_cap = cap;
    return PORRT_OK;
}

// tamp_best_paths of the rows ctxs[0 .. n) into the call's arena through its running cursor, the records to d_meta[0 .. n) on the
// device: nothing is downloaded here
static int astar_gather(porrt_ctx *c, TampState &T, AstarState &A, porrt_ctx *const *ctxs, uint32_t n, uint32_t *d_cur, BestPath *d_meta) {
    const double t0 = now_s();
    int r = astar_arena_reserve(c, A, A.cursor_ub + (size_t)n * kTampPathSlot);
    if (r < 0 || (r = tamp_best_paths(c, ctxs, n, A.arena, d_cur, d_meta)) < 0) return r;
    A.cursor_ub += (size_t)n * kTampPathSlot;
    T.info.path_s += now_s() - t0;
    return PORRT_OK;
}

// The device side of one call over the searches S: the arena and what the kernels read call-wide (begin), the records of a chunk
// of edges of any of the searches (expand_chunk, and expand_sequential for the one plan on the lead's own stream), and the end of
// every search that found its leaf (policies).  `named`: errors name the plan they came from (a batch).
// SearchT is porrt_astar::Search or porrt_bnb::Search (porrt_tamp_bnb_batch.hpp): nodes with ox, oy, h, ec, target, belief and the
// arena offsets of their two paths, belief_row(), chain(), and per edge zone_of, edge_rp, edge_belief, edge_remaining.
template <class SearchT>
struct SearchRun {
    porrt_ctx *c;
    TampFrame &F;
    TampState &T;
    AstarState &A;
    std::vector<SearchT> &S;
    bool named;
    const char *tag = "tamp astar";            // what the errors begin with
    uint32_t nw = 0;
    hipStream_t st = nullptr;
    uint32_t *d_cur = nullptr;
    double2 *d_zpos = nullptr;

    std::string of_plan(uint32_t p) const { return named ? " (plan " + std::to_string(p) + ")" : std::string(); }

    int begin() {
        nw = F.nw;
        HIPCHK_CTX(c, hipSetDevice(c->device));
        if (!A.ev) HIPCHK_CTX(c, hipEventCreate(&A.ev));
        st = c->stream;
        A.cursor_ub = 0;
        const int r = astar_arena_reserve(c, A, std::max<size_t>(kTampPathSlot, c->opt_tamp_arena_states));
        if (r < 0) return r;
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarCursor, d_cur, 1));
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarZonePos, d_zpos, nw));
        HIPCHK_CTX(c, hipMemsetAsync(d_cur, 0, sizeof(uint32_t), st));
        std::vector<double2> zp(nw);
        for (uint32_t z = 0; z < nw; ++z) zp[z] = make_double2(c->zone_pos[z][0], c->zone_pos[z][1]);
        HIPCHK_CTX(c, hipMemcpyAsync(d_zpos, zp.data(), nw * sizeof(double2), hipMemcpyHostToDevice, st));
        HIPCHK_CTX(c, hipStreamSynchronize(st));
        return PORRT_OK;
    }

    int bad_record(uint32_t status, uint32_t plan) {
        c->set_err(std::string(tag) + (status == kAstarSlot ? ": a best path longer than its slot of " + std::to_string(kTampPathSlot) + " states"
                                                            : std::string(": the best-cost scratch of a query overflowed")) + of_plan(plan));
        return PORRT_ERR_CAPACITY;
    }

    // the records of edges[e0 .. e0 + m): rows of the two BestPath arrays -> one k_astar_children launch -> out[0 .. m)
    int children(const std::vector<AstarEdge> &edges, size_t e0, uint32_t m, const std::vector<uint32_t> &pick_row, const BestPath *d_obs,
                 const BestPath *d_pick, AstarChildRecord *out) {
        const double t0 = now_s();
        std::vector<AstarChildIn> in(m);
        std::vector<double> bl;
        uint32_t rows = 0;                                     // belief rows uploaded: one per run of edges of one expansion
        for (uint32_t i = 0; i < m; ++i) {
            const AstarEdge &ed = edges[e0 + i];
            const SearchT &s = S[ed.plan];
            if (i == 0 || edges[e0 + i - 1].plan != ed.plan || edges[e0 + i - 1].u != ed.u) {      // the children of a node share a belief
                bl.insert(bl.end(), s.edge_belief(ed), s.edge_belief(ed) + nw);
                ++rows;
            }
            AstarChildIn &a = in[i];
            a.parent_ec = s.nodes[(size_t)ed.u].ec; a.rp = s.edge_rp(ed);
            a.remaining = s.edge_remaining(ed);
            a.obs_row = i; a.pick_row = pick_row[i];
            a.belief_row = rows - 1; a.target = s.zone_of(ed);
        }
        AstarChildIn *d_in = nullptr;
        double *d_bl = nullptr;
        AstarChildOut *d_out = nullptr;
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarChildIn, d_in, m));
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarBeliefs, d_bl, bl.size()));
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarChildOut, d_out, m));
        HIPCHK_CTX(c, hipMemcpyAsync(d_in, in.data(), m * sizeof(AstarChildIn), hipMemcpyHostToDevice, st));
        HIPCHK_CTX(c, hipMemcpyAsync(d_bl, bl.data(), bl.size() * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_astar_children, dim3((m + 63u) / 64u), dim3(64), 0, st, d_in, m, d_obs, d_pick, d_bl, nw, d_zpos, d_cur, d_out);
        HIPCHK_CTX(c, hipGetLastError());
        std::vector<AstarChildOut> got(m);
        HIPCHK_CTX(c, hipMemcpyAsync(got.data(), d_out, m * sizeof(AstarChildOut), hipMemcpyDeviceToHost, st));
        HIPCHK_CTX(c, hipStreamSynchronize(st));
        A.cursor_ub = got[0].cursor;                           // exact: nothing has been gathered since
        A.info.arena_used = got[0].cursor;
        for (uint32_t i = 0; i < m; ++i) {
            const AstarChildOut &o = got[i];
            if (o.status == kAstarSlot || o.status == kAstarScratch) return bad_record(o.status, edges[e0 + i].plan);
            AstarChildRecord &r = out[i];
            r.ec = o.ec; r.priority = o.priority; r.ox = o.ox; r.oy = o.oy;
            r.obs_off = o.obs_off; r.obs_len = o.obs_len; r.pick_off = o.pick_off; r.pick_len = o.pick_len;
            r.status = o.status == kAstarOk ? porrt_astar::kChildOk : o.status == kAstarNoObs ? porrt_astar::kChildNoObs : porrt_astar::kChildNoPick;
        }
        A.info.children_s += now_s() - t0;
        return PORRT_OK;
    }

    // the observation records of m rows (those of edges[e0 ..)): the pickup queries start from their end states
    int fetch_obs(const BestPath *d_obs, uint32_t m, std::vector<BestPath> &meta, const std::vector<AstarEdge> &edges, size_t e0) {
        const double t0 = now_s();
        meta.resize(m);
        HIPCHK_CTX(c, hipMemcpyAsync(meta.data(), d_obs, m * sizeof(BestPath), hipMemcpyDeviceToHost, st));
        HIPCHK_CTX(c, hipStreamSynchronize(st));
        size_t end = 0;
        for (uint32_t i = 0; i < m; ++i) {
            const BestPath &b = meta[i];
            if (b.status >= 2u) return bad_record(b.status == 3u ? (uint32_t)kAstarSlot : (uint32_t)kAstarScratch, edges[e0 + i].plan);
            if (b.status == 0u) end = std::max<size_t>(end, (size_t)b.off + b.len);
        }
        if (end) A.cursor_ub = end;                            // exact: the cursor only grows, and these rows were the last to move it
        T.info.path_s += now_s() - t0;
        return PORRT_OK;
    }

    // tamp_streams = 0 (one plan, one node per round): the node's children one after the other on the lead.  The node is the top of
    // the queue and is popped next, so the first query without a path ends the plan.
    int expand_sequential(const std::vector<AstarEdge> &edges, size_t e0, uint32_t m, AstarChildRecord *out) {
        const SearchT &s = S[edges[e0].plan];
        const auto &u = s.nodes[(size_t)edges[e0].u];
        BestPath *d_obs = nullptr, *d_pick = nullptr;
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarObs, d_obs, m));
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarPick, d_pick, m));
        std::vector<uint32_t> pick_row(m);
        std::vector<BestPath> meta;
        porrt_ctx *one = c;
        for (uint32_t i = 0; i < m; ++i) {
            const uint32_t t = s.zone_of(edges[e0 + i]);
            pick_row[i] = i;
            double st2[2] = {u.ox, u.oy};
            for (int which = 0; which < 2; ++which) {
                int rr = F.grow_lead(st2, t, which);
                if (rr < 0) return rr;
                if ((rr = astar_gather(c, T, A, &one, 1, d_cur, (which == 0 ? d_obs : d_pick) + i)) < 0) return rr;
                if ((rr = fetch_obs((which == 0 ? d_obs : d_pick) + i, 1, meta, edges, e0 + i)) < 0) return rr;
                if (meta[0].status == 1u) return tamp_fail(c, T, (int64_t)s.nodes.size() + i, (int32_t)t, which);
                st2[0] = meta[0].end_x; st2[1] = meta[0].end_y;
            }
        }
        return children(edges, e0, m, pick_row, d_obs, d_pick, out);
    }

    // tamp_streams = 1: the rows edges[e0 .. e0 + m), of whichever searches, together: one observation batch, one gather, one record
    // download, one pickup batch on the rows that saw their zone, one gather, one k_astar_children
    int expand_chunk(const std::vector<AstarEdge> &edges, size_t e0, uint32_t m, AstarChildRecord *out) {
        int rr = tamp_ensure_pool(c, T, m);
        if (rr < 0) return rr;
        BestPath *d_obs = nullptr, *d_pick = nullptr;
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarObs, d_obs, m));
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarPick, d_pick, m));
        auto node_of = [&](size_t e) -> const auto & { return S[edges[e].plan].nodes[(size_t)edges[e].u]; };
        auto zone_of = [&](size_t e) { return S[edges[e].plan].zone_of(edges[e]); };
        auto grown = [&](int r) {
            if (r < 0 && named) c->set_err(std::string(tag) + " batch: the growth of a chunk holding plans " + std::to_string(edges[e0].plan) + " .. " +
                                           std::to_string(edges[e0 + m - 1].plan) + " failed: " + c->err);
            return r;
        };
        std::vector<double> starts(2 * (size_t)m);
        for (uint32_t i = 0; i < m; ++i) { starts[2 * i] = node_of(e0 + i).ox; starts[2 * i + 1] = node_of(e0 + i).oy; }
        rr = F.grow_rows(T.pool.data(), m, starts.data(), [&](uint32_t i) {
            return F.seed_and_goal(T.pool[i], porrt_astar::edge_seed(node_of(e0 + i).h, zone_of(e0 + i)), zone_of(e0 + i), 0);
        });
        if (rr < 0) return grown(rr);
        if ((rr = astar_gather(c, T, A, T.pool.data(), m, d_cur, d_obs)) < 0) return rr;
        std::vector<BestPath> meta;
        if ((rr = fetch_obs(d_obs, m, meta, edges, e0)) < 0) return rr;
        // the pickup queries of the rows that saw their zone, on the same contexts: their streams run on
        std::vector<porrt_ctx *> sub;
        std::vector<uint32_t> pick_row(m, 0xFFFFFFFFu), sub_zone;
        std::vector<double> pstarts;
        for (uint32_t i = 0; i < m; ++i) {
            if (meta[i].status != 0u) continue;
            pick_row[i] = (uint32_t)sub.size();
            sub.push_back(T.pool[i]);
            sub_zone.push_back(zone_of(e0 + i));
            pstarts.push_back(meta[i].end_x); pstarts.push_back(meta[i].end_y);
        }
        if (!sub.empty()) {
            const uint32_t mp = (uint32_t)sub.size();
            if ((rr = F.grow_rows(sub.data(), mp, pstarts.data(), [&](uint32_t j) { return F.set_goal(sub[j], sub_zone[j], 1); })) < 0) return grown(rr);
            if ((rr = astar_gather(c, T, A, sub.data(), mp, d_cur, d_pick)) < 0) return rr;
        }
        return children(edges, e0, m, pick_row, d_obs, d_pick, out);
    }

    // The end of the searches `solved`, all of which found their leaf: one k_astar_chain and one k_tamp_shortcut launch over the
    // 2 x depth paths of all their chains (the draws per path length are shared, as within one plan), then the assembly and the
    // expected cost per plan on the host, into out[i] / expected[i] for solved[i].
    int policies(const std::vector<uint32_t> &solved, const std::vector<TampPolicyArrays> &out, std::vector<double> &expected) {
        std::vector<std::vector<int64_t>> chains;
        std::vector<uint64_t> off{0};
        TampChainSource src;
        src.arena = A.arena; src.ev = A.ev;
        for (uint32_t p : solved) {
            chains.push_back(S[p].chain());
            for (int64_t k : chains.back()) {
                const auto &n = S[p].nodes[(size_t)k];
                off.push_back(off.back() + n.obs_len);
                src.paths.push_back({n.obs_off, n.obs_len, 0u, 0u});
                off.push_back(off.back() + n.pick_len);
                src.paths.push_back({n.pick_off, n.pick_len, 0u, 0u});
            }
        }
        std::vector<double> xy(2 * (size_t)off.back(), 0.0);      // only written: the paths are on the device
        const double t0 = now_s();
        const int r = tamp_shortcut_device(c, T, xy, off, nullptr, &src);
        if (r < 0) return r;
        T.info.shortcut_s = now_s() - t0;
        A.info.chain_s = src.chain_s;
        expected.assign(solved.size(), 0.0);
        size_t at = 0;
        for (size_t i = 0; i < solved.size(); ++i) {
            const SearchT &s = S[solved[i]];
            std::vector<int32_t> target;
            std::vector<const double *> belief;
            for (int64_t k : chains[i]) { target.push_back(s.nodes[(size_t)k].target); belief.push_back(s.belief_row(s.nodes[(size_t)k].belief)); }
            expected[i] = tamp_assemble_policy(nw, chains[i].size(), target.data(), belief.data(), xy, off.data() + at, out[i]);
            at += 2 * chains[i].size();
        }
        return PORRT_OK;
    }
};

using AstarRun = SearchRun<AstarSearch>;

template <class SearchT>
static uint32_t astar_zone_order(const SearchT &s, uint32_t *order) {
    uint32_t n = 0;
    for (int64_t k : s.chain()) if (s.nodes[(size_t)k].parent >= 0) order[n++] = (uint32_t)s.nodes[(size_t)k].target;
    return n;
}

static int astar_check_zones(porrt_ctx *c, uint32_t nw) {
    if (nw > 64) { c->set_err("tamp astar: at most 64 zones"); return PORRT_ERR_INVALID; }
    return PORRT_OK;
}

// the driver (porrt_astar::run) with one plan: the only one that may run on the lead's own stream
static int64_t tamp_plan_astar(porrt_ctx *c, const double start[2], const double *belief, uint32_t nw, double max_step, double search_radius,
                               uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t K) {
    TampFrame F;
    int r = F.begin(c, start, belief, nw, max_step, search_radius, n_iter_min, n_iter_max, goal_radius, K, [&](int stage) -> int {
        if (stage == 0) return astar_check_zones(c, nw);
        for (uint32_t w = 0; w < nw; ++w)
            if (!(belief[w] > 0.0)) { c->set_err("tamp astar: every entry of the prior must be > 0 (below the last positive zone every priority would be NaN)"); return PORRT_ERR_INVALID; }
        return PORRT_OK;
    });
    if (r < 0) return r;
    TampState &T = *F.T;
    AstarState &A = astar_state(T);
    memset(&A.info, 0, sizeof A.info);
    A.parents.clear(); A.targets.clear(); A.ec.clear(); A.priority.clear();

    std::vector<AstarSearch> S(1);
    AstarSearch &s = S[0];
    s.begin(start, belief, nw, c->s_seed);
    // the nodes as they stand go to the state whichever way the plan ends (porrt_tamp_astar_nodes)
    struct Keep {
        AstarState &A; TampState &T; const AstarSearch &s;
        ~Keep() {
            for (const porrt_astar::Node &n : s.nodes) { A.parents.push_back(n.parent); A.targets.push_back(n.target); A.ec.push_back(n.ec); A.priority.push_back(n.priority); }
            T.info.search_nodes = s.nodes.size();
            A.info.arena_states = A.arena_cap;
        }
    } keep{A, T, s};
    AstarRun R{c, F, T, A, S, false};
    if ((r = R.begin()) < 0) return r;
    if (F.streams == 0)
        r = porrt_astar::run(S, 1u, ~(size_t)0, T.info.waves,
                             [&](const std::vector<AstarEdge> &edges, size_t e0, uint32_t m, AstarChildRecord *out) { return R.expand_sequential(edges, e0, m, out); });
    else
        r = porrt_astar::run(S, F.wave, F.pool_cap, T.info.waves,
                             [&](const std::vector<AstarEdge> &edges, size_t e0, uint32_t m, AstarChildRecord *out) { return R.expand_chunk(edges, e0, m, out); });
    if (r < 0) return r;
    if (s.state == AstarSearch::kFailed) return tamp_fail(c, T, s.fail_node, s.fail_zone, s.fail_query);
    if (s.state != AstarSearch::kSolved) { c->set_err("No solution found!"); return PORRT_ERR_NO_PATH; }
    A.info.speculated = s.speculated();
    porrt_tamp_info &I = T.info;
    I.search_cost = s.nodes[(size_t)s.solution].ec;
    I.n_order = astar_zone_order(s, I.zone_order);
    if (F.restore) { c->crng = F.crng0; F.restore = false; }
    std::vector<double> expected;
    if ((r = R.policies({0u}, {TampPolicyArrays{T.xy, T.beliefs, T.parents, T.leaf}}, expected)) < 0) return r;
    I.expected_cost = expected[0];
    T.valid = true;
    F.close(A.info.children_s);
    return (int64_t)T.parents.size();
}

// porrt_tamp_rrt_plan_astar_batch: the driver over n_plans searches that share map, zones and parameters.
// Plan p is the search of tamp_plan_astar with root stream seed seeds[p]; its rows ride in the same porrt_grow_batch as the others'.
static int64_t tamp_plan_astar_batch(porrt_ctx *c, uint32_t n_plans, const double *starts, const double *priors, const uint64_t *seeds, uint32_t nw,
                                     double max_step, double search_radius, uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t K) {
    if (n_plans == 0 || n_plans > 65536u) { c->set_err("tamp astar batch: n_plans must be in 1..65536"); return PORRT_ERR_INVALID; }
    if (!starts || !priors) { c->set_err("tamp astar batch: starts and priors"); return PORRT_ERR_INVALID; }
    if (!c->opt_tamp_streams) { c->set_err("tamp astar batch: needs per-edge streams (tamp_streams 1): one continuous stream cannot be shared by plans"); return PORRT_ERR_INVALID; }
    TampFrame F;
    int r = F.begin(c, starts, priors, nw, max_step, search_radius, n_iter_min, n_iter_max, goal_radius, K, [&](int stage) -> int {
        if (stage != 0) return PORRT_OK;
        if (astar_check_zones(c, nw) < 0) return PORRT_ERR_INVALID;
        for (uint32_t p = 0; p < n_plans; ++p) {                // every plan's prior, before anything runs
            const double *b = priors + (size_t)p * nw;
            double sum = 0.0;
            for (uint32_t w = 0; w < nw; ++w) sum = sum + b[w];
            if (!(std::fabs(sum - 1.0) < 0.001)) { c->set_err("tamp astar batch: plan " + std::to_string(p) + ": the prior does not sum to 1 (check_belief_state, common.rs:390)"); return PORRT_ERR_INVALID; }
            for (uint32_t w = 0; w < nw; ++w)
                if (!(b[w] > 0.0)) { c->set_err("tamp astar batch: plan " + std::to_string(p) + ": every entry of the prior must be > 0"); return PORRT_ERR_INVALID; }
        }
        return PORRT_OK;
    });
    if (r < 0) return r;
    TampState &T = *F.T;
    AstarState &A = astar_state(T);
    memset(&A.info, 0, sizeof A.info);
    A.parents.clear(); A.targets.clear(); A.ec.clear(); A.priority.clear();      // the last single plan is replaced
    A.batch.clear();
    A.batch_nw = nw;
    A.batch_bnb = false;

    std::vector<AstarSearch> S(n_plans);
    for (uint32_t p = 0; p < n_plans; ++p) S[p].begin(starts + 2 * (size_t)p, priors + (size_t)p * nw, nw, seeds ? seeds[p] : c->s_seed);
    AstarRun R{c, F, T, A, S, true};
    if ((r = R.begin()) < 0) return r;
    r = porrt_astar::run(S, F.wave, F.pool_cap, T.info.waves,
                         [&](const std::vector<AstarEdge> &edges, size_t e0, uint32_t m, AstarChildRecord *out) { return R.expand_chunk(edges, e0, m, out); });
    A.info.arena_states = A.arena_cap;
    for (const AstarSearch &s : S) T.info.search_nodes += s.nodes.size();
    if (r < 0) return r;

    std::vector<AstarBatchPlan> plans(n_plans);
    std::vector<uint32_t> solved;
    std::vector<TampPolicyArrays> arrays;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const AstarSearch &s = S[p];
        AstarBatchPlan &B = plans[p];
        porrt_tamp_batch_plan &rec = B.rec;
        memset(&rec, 0, sizeof rec);
        rec.status = s.state == AstarSearch::kSolved ? PORRT_OK : PORRT_ERR_NO_PATH;
        rec.fail_node = s.fail_node; rec.fail_zone = s.fail_zone; rec.fail_query = s.fail_query;
        rec.search_nodes = s.nodes.size(); rec.queries = s.queries; rec.waves = s.waves;
        for (const porrt_astar::Node &n : s.nodes) { B.node_parents.push_back(n.parent); B.node_targets.push_back(n.target); B.node_ec.push_back(n.ec); B.node_priority.push_back(n.priority); }
        if (s.state != AstarSearch::kSolved) continue;
        rec.speculated = s.speculated();
        A.info.speculated += rec.speculated;
        rec.search_cost = s.nodes[(size_t)s.solution].ec;
        rec.n_order = astar_zone_order(s, rec.zone_order);
        solved.push_back(p);
        arrays.push_back(TampPolicyArrays{B.xy, B.beliefs, B.parents, B.leaf});
    }
    if (!solved.empty()) {
        std::vector<double> expected;
        if ((r = R.policies(solved, arrays, expected)) < 0) return r;
        for (size_t i = 0; i < solved.size(); ++i) {
            plans[solved[i]].rec.expected_cost = expected[i];
            plans[solved[i]].rec.policy_nodes = plans[solved[i]].parents.size();
        }
    }
    A.batch = std::move(plans);
    F.close(A.info.children_s);
    return (int64_t)solved.size();
}

// the shortcut's device-resident input form on explicit paths: they are put into the arena as a plan's gathers would leave them
static int tamp_shortcut_resident(porrt_ctx *c, TampState &T, std::vector<double> &xy, const std::vector<uint64_t> &off) {
    AstarState &A = astar_state(T);
    const size_t ns = off.back();
    HIPCHK_CTX(c, hipSetDevice(c->device));
    if (!A.ev) HIPCHK_CTX(c, hipEventCreate(&A.ev));
    A.cursor_ub = 0;
    const int r = astar_arena_reserve(c, A, std::max<size_t>(ns, 1));
    if (r < 0) return r;
    std::vector<double2> up(ns);
    for (size_t k = 0; k < ns; ++k) up[k] = make_double2(xy[2 * k], xy[2 * k + 1]);
    if (ns) HIPCHK_CTX(c, hipMemcpyAsync(A.arena, up.data(), ns * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    HIPCHK_CTX(c, hipStreamSynchronize(c->stream));
    TampChainSource src;
    src.arena = A.arena; src.ev = A.ev;
    for (size_t i = 0; i + 1 < off.size(); ++i) src.paths.push_back({(uint32_t)off[i], (uint32_t)(off[i + 1] - off[i]), 0u, 0u});
    std::fill(xy.begin(), xy.end(), 0.0);
    return tamp_shortcut_device(c, T, xy, off, nullptr, &src);
}

} // namespace
