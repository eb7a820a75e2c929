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
#pragma once

#include "porrt_astar_queue.hpp"

namespace {

struct AstarNode {
    int32_t target = -1;
    int64_t parent = -1;
    unsigned long long remaining = 0;          // bit z: zone z still to visit (always walked in ascending order)
    double ox = 0, oy = 0;                     // observation_state
    double rp = 1.0, ec = 0.0, priority = 0.0;
    uint32_t belief = 0;                       // row of the plan's belief table
    uint64_t h = 0;                            // stream seed of the edge into this node (tamp_streams = 1)
    uint32_t obs_off = 0, obs_len = 0, pick_off = 0, pick_len = 0;   // its two paths in the arena
    int64_t kids = -1;                         // its expansion, once computed
    bool popped = false;
};

struct AstarExpansion {                        // the children of one node, before they have ids
    uint32_t belief = 0;
    double rp = 0.0;
    std::vector<uint32_t> zone;
    std::vector<AstarChildOut> rec;
};

struct AstarState {
    double2 *arena = nullptr;                  // path arena of the running plan; kept across plans, its cursor is not
    size_t arena_cap = 0;                      // states
    size_t cursor_ub = 0;                      // no gather has written at or beyond this state
    hipEvent_t ev = nullptr;
    porrt_tamp_astar_info info;
    std::vector<int64_t> parents;              // the last plan's search nodes, in id order
    std::vector<int32_t> targets;
    std::vector<double> ec, priority;
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

// tamp_best_paths of the rows ctxs[0 .. n) into the plan's arena through its running cursor, the records to d_meta[0 .. n) on the
// device: nothing is downloaded here
static int astar_gather(porrt_ctx *c, TampState &T, AstarState &A, porrt_ctx *const *ctxs, uint32_t n, uint32_t *d_cur, BestPath *d_meta) {
    const double t0 = now_s();
    int r = astar_arena_reserve(c, A, A.cursor_ub + (size_t)n * kTampPathSlot);
    if (r < 0 || (r = tamp_best_paths(c, ctxs, n, A.arena, d_cur, d_meta)) < 0) return r;
    A.cursor_ub += (size_t)n * kTampPathSlot;
    T.info.path_s += now_s() - t0;
    return PORRT_OK;
}

static int astar_bad_record(porrt_ctx *c, uint32_t status) {
    c->set_err(status == kAstarSlot ? "tamp astar: a best path longer than its slot of " + std::to_string(kTampPathSlot) + " states"
                                    : std::string("tamp astar: the best-cost scratch of a query overflowed"));
    return PORRT_ERR_CAPACITY;
}

static int64_t tamp_plan_astar(porrt_ctx *c, const double start[2], const double *belief, uint32_t nw, double max_step, double search_radius,
                               uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t K) {
    TampFrame F;
    int r = F.begin(c, start, belief, nw, max_step, search_radius, n_iter_min, n_iter_max, goal_radius, K, [&](int stage) -> int {
        if (stage == 0) {
            if (nw > 64) { c->set_err("tamp astar: at most 64 zones"); return PORRT_ERR_INVALID; }
            return PORRT_OK;
        }
        for (uint32_t w = 0; w < nw; ++w)
            if (!(belief[w] > 0.0)) { c->set_err("tamp astar: every entry of the prior must be > 0 (below the last positive zone every priority would be NaN)"); return PORRT_ERR_INVALID; }
        return PORRT_OK;
    });
    if (r < 0) return r;
    TampState &T = *F.T;
    AstarState &A = astar_state(T);
    memset(&A.info, 0, sizeof A.info);
    A.parents.clear(); A.targets.clear(); A.ec.clear(); A.priority.clear();
    const uint32_t nz = nw;

    HIPCHK_CTX(c, hipSetDevice(c->device));
    if (!A.ev) HIPCHK_CTX(c, hipEventCreate(&A.ev));
    hipStream_t st = c->stream;
    A.cursor_ub = 0;
    if ((r = astar_arena_reserve(c, A, std::max<size_t>(kTampPathSlot, c->opt_tamp_arena_states))) < 0) return r;
    uint32_t *d_cur = nullptr;
    double2 *d_zpos = nullptr;
    HIPCHK_CTX(c, T.scratch.get(kSlotAstarCursor, d_cur, 1));
    HIPCHK_CTX(c, T.scratch.get(kSlotAstarZonePos, d_zpos, nz));
    HIPCHK_CTX(c, hipMemsetAsync(d_cur, 0, sizeof(uint32_t), st));
    {
        std::vector<double2> zp(nz);
        for (uint32_t z = 0; z < nz; ++z) zp[z] = make_double2(c->zone_pos[z][0], c->zone_pos[z][1]);
        HIPCHK_CTX(c, hipMemcpyAsync(d_zpos, zp.data(), nz * sizeof(double2), hipMemcpyHostToDevice, st));
        HIPCHK_CTX(c, hipStreamSynchronize(st));
    }

    std::vector<AstarNode> nodes(1);
    std::vector<AstarExpansion> exps;
    std::vector<double> beliefs(belief, belief + nw);         // row 0: the prior
    {
        AstarNode &root = nodes[0];
        root.remaining = nz == 64 ? ~0ull : ((1ull << nz) - 1ull);
        root.ox = start[0]; root.oy = start[1];
        root.h = c->s_seed;
    }
    // the nodes as they stand go to the state whichever way the plan ends (porrt_tamp_astar_nodes)
    struct Keep {
        AstarState &A; TampState &T; const std::vector<AstarNode> &nodes;
        ~Keep() {
            for (const AstarNode &n : nodes) { A.parents.push_back(n.parent); A.targets.push_back(n.target); A.ec.push_back(n.ec); A.priority.push_back(n.priority); }
            T.info.search_nodes = nodes.size();
            A.info.arena_states = A.arena_cap;
        }
    } keep{A, T, nodes};

    // the expansion of node uid gets its belief row and reaching probability; returns its index
    auto open_expansion = [&](int64_t uid) {
        const AstarNode &u = nodes[(size_t)uid];
        AstarExpansion E;
        std::vector<double> vb;
        std::tie(vb, E.rp) = tamp_child_belief(beliefs.data() + (size_t)u.belief * nw, u.target, u.rp, nw);
        E.belief = (uint32_t)(beliefs.size() / nw);
        beliefs.insert(beliefs.end(), vb.begin(), vb.end());
        for (uint32_t z = 0; z < nz; ++z) if ((u.remaining >> z) & 1ull) E.zone.push_back(z);
        E.rec.resize(E.zone.size());
        exps.push_back(std::move(E));
        return (int64_t)exps.size() - 1;
    };

    struct Edge { int64_t u; int64_t e; uint32_t i; };        // child i of expansion e of node u
    // the records of edges[e0 .. e0 + m): rows of the two BestPath arrays -> k_astar_children -> the expansions
    auto children = [&](const std::vector<Edge> &edges, size_t e0, uint32_t m, const std::vector<uint32_t> &pick_row, const BestPath *d_obs,
                        const BestPath *d_pick) -> int {
        const double t0 = now_s();
        std::vector<AstarChildIn> in(m);
        std::vector<double> bl;
        std::vector<int64_t> row_of;                           // expansion of each uploaded belief row
        for (uint32_t i = 0; i < m; ++i) {
            const Edge &ed = edges[e0 + i];
            const AstarNode &u = nodes[(size_t)ed.u];
            const AstarExpansion &E = exps[(size_t)ed.e];
            if (row_of.empty() || row_of.back() != ed.e) {
                row_of.push_back(ed.e);
                bl.insert(bl.end(), beliefs.begin() + (size_t)E.belief * nw, beliefs.begin() + (size_t)(E.belief + 1) * nw);
            }
            AstarChildIn &a = in[i];
            a.parent_ec = u.ec; a.rp = E.rp;
            a.remaining = u.remaining & ~(1ull << E.zone[ed.i]);
            a.obs_row = i; a.pick_row = pick_row[i];
            a.belief_row = (uint32_t)row_of.size() - 1; a.target = E.zone[ed.i];
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
        std::vector<AstarChildOut> out(m);
        HIPCHK_CTX(c, hipMemcpyAsync(out.data(), d_out, m * sizeof(AstarChildOut), hipMemcpyDeviceToHost, st));
        HIPCHK_CTX(c, hipStreamSynchronize(st));
        A.cursor_ub = out[0].cursor;                           // exact: nothing has been gathered since
        A.info.arena_used = out[0].cursor;
        for (uint32_t i = 0; i < m; ++i) {
            if (out[i].status == kAstarSlot || out[i].status == kAstarScratch) return astar_bad_record(c, out[i].status);
            exps[(size_t)edges[e0 + i].e].rec[edges[e0 + i].i] = out[i];
        }
        A.info.children_s += now_s() - t0;
        return PORRT_OK;
    };
    // the observation records of m rows: the pickup queries start from their end states
    auto fetch_obs = [&](const BestPath *d_obs, uint32_t m, std::vector<BestPath> &meta) -> int {
        const double t0 = now_s();
        meta.resize(m);
        HIPCHK_CTX(c, hipMemcpyAsync(meta.data(), d_obs, m * sizeof(BestPath), hipMemcpyDeviceToHost, st));
        HIPCHK_CTX(c, hipStreamSynchronize(st));
        size_t end = 0;
        for (const BestPath &b : meta) {
            if (b.status >= 2u) return astar_bad_record(c, b.status == 3u ? (uint32_t)kAstarSlot : (uint32_t)kAstarScratch);
            if (b.status == 0u) end = std::max<size_t>(end, (size_t)b.off + b.len);
        }
        if (end) A.cursor_ub = end;                            // exact: the cursor only grows, and these rows were the last to move it
        T.info.path_s += now_s() - t0;
        return PORRT_OK;
    };

    // tamp_streams = 0: node uid's children one after the other on the lead.  uid is the top of the queue and is popped next, so
    // the first query without a path ends the plan.
    auto expand_sequential = [&](int64_t uid) -> int64_t {
        const int64_t ei = open_expansion(uid);
        nodes[(size_t)uid].kids = ei;
        const uint32_t m = (uint32_t)exps[(size_t)ei].zone.size();
        BestPath *d_obs = nullptr, *d_pick = nullptr;
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarObs, d_obs, m));
        HIPCHK_CTX(c, T.scratch.get(kSlotAstarPick, d_pick, m));
        std::vector<Edge> edges;
        std::vector<uint32_t> pick_row(m);
        std::vector<BestPath> meta;
        porrt_ctx *one = c;
        for (uint32_t i = 0; i < m; ++i) {
            const uint32_t t = exps[(size_t)ei].zone[i];
            edges.push_back({uid, ei, i});
            pick_row[i] = i;
            double st2[2] = {nodes[(size_t)uid].ox, nodes[(size_t)uid].oy};
            for (int which = 0; which < 2; ++which) {
                int rr = F.grow_lead(st2, t, which);
                if (rr < 0) return rr;
                if ((rr = astar_gather(c, T, A, &one, 1, d_cur, (which == 0 ? d_obs : d_pick) + i)) < 0) return rr;
                if ((rr = fetch_obs((which == 0 ? d_obs : d_pick) + i, 1, meta)) < 0) return rr;
                if (meta[0].status == 1u) return tamp_fail(c, T, (int64_t)nodes.size() + i, (int32_t)t, which);
                st2[0] = meta[0].end_x; st2[1] = meta[0].end_y;
            }
        }
        return children(edges, 0, m, pick_row, d_obs, d_pick);
    };

    // tamp_streams = 1: the nodes of `batch` together, chunked by the pool
    auto expand_wave = [&](const std::vector<int64_t> &batch) -> int64_t {
        std::vector<Edge> edges;
        for (int64_t uid : batch) {
            const int64_t ei = open_expansion(uid);
            nodes[(size_t)uid].kids = ei;
            for (uint32_t i = 0; i < exps[(size_t)ei].zone.size(); ++i) edges.push_back({uid, ei, i});
        }
        std::vector<BestPath> meta;
        auto zone_of = [&](size_t e) { return exps[(size_t)edges[e].e].zone[edges[e].i]; };
        for (size_t e0 = 0; e0 < edges.size(); e0 += F.pool_cap) {
            const uint32_t m = (uint32_t)std::min<size_t>(F.pool_cap, edges.size() - e0);
            int rr = tamp_ensure_pool(c, T, m);
            if (rr < 0) return rr;
            BestPath *d_obs = nullptr, *d_pick = nullptr;
            HIPCHK_CTX(c, T.scratch.get(kSlotAstarObs, d_obs, m));
            HIPCHK_CTX(c, T.scratch.get(kSlotAstarPick, d_pick, m));
            std::vector<double> starts(2 * (size_t)m);
            for (uint32_t i = 0; i < m; ++i) { starts[2 * i] = nodes[(size_t)edges[e0 + i].u].ox; starts[2 * i + 1] = nodes[(size_t)edges[e0 + i].u].oy; }
            rr = F.grow_rows(T.pool.data(), m, starts.data(), [&](uint32_t i) {
                return F.seed_and_goal(T.pool[i], tamp_edge_seed(nodes[(size_t)edges[e0 + i].u].h, zone_of(e0 + i)), zone_of(e0 + i), 0);
            });
            if (rr < 0) return rr;
            if ((rr = astar_gather(c, T, A, T.pool.data(), m, d_cur, d_obs)) < 0) return rr;
            if ((rr = fetch_obs(d_obs, m, meta)) < 0) return rr;
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
                if ((rr = F.grow_rows(sub.data(), mp, pstarts.data(), [&](uint32_t j) { return F.set_goal(sub[j], sub_zone[j], 1); })) < 0) return rr;
                if ((rr = astar_gather(c, T, A, sub.data(), mp, d_cur, d_pick)) < 0) return rr;
            }
            if ((rr = children(edges, e0, m, pick_row, d_obs, d_pick)) < 0) return rr;
        }
        return PORRT_OK;
    };

    porrt_astar::Queue queue;
    queue.push(0.0, 0);
    int64_t solution = -1;
    while (solution < 0 && !queue.empty()) {
        // the replay: pops while the top is a leaf or has its children
        while (!queue.empty()) {
            const int64_t uid = (int64_t)queue.top().id;
            if (nodes[(size_t)uid].remaining && nodes[(size_t)uid].kids < 0) break;
            queue.pop();
            nodes[(size_t)uid].popped = true;
            if (nodes[(size_t)uid].kids >= 0) {
                const AstarExpansion &E = exps[(size_t)nodes[(size_t)uid].kids];
                for (uint32_t i = 0; i < E.zone.size(); ++i) {
                    const AstarChildOut &o = E.rec[i];
                    if (o.status != kAstarOk) return tamp_fail(c, T, (int64_t)nodes.size(), (int32_t)E.zone[i], o.status == kAstarNoObs ? 0 : 1);
                    AstarNode v;
                    const AstarNode &u = nodes[(size_t)uid];
                    v.target = (int32_t)E.zone[i]; v.parent = uid;
                    v.remaining = u.remaining & ~(1ull << E.zone[i]);
                    v.ox = o.ox; v.oy = o.oy; v.rp = E.rp; v.ec = o.ec; v.priority = o.priority;
                    v.belief = E.belief;
                    v.h = tamp_edge_seed(u.h, E.zone[i]);
                    v.obs_off = o.obs_off; v.obs_len = o.obs_len; v.pick_off = o.pick_off; v.pick_len = o.pick_len;
                    queue.push(v.priority, (uint64_t)nodes.size());
                    nodes.push_back(v);
                }
            }
            if (!nodes[(size_t)uid].remaining) { solution = uid; break; }
        }
        if (solution >= 0 || queue.empty()) break;
        // the top has no children yet: it and the next best entries like it
        std::vector<porrt_astar::QueueEntry> held;
        std::vector<int64_t> batch;
        while (!queue.empty() && batch.size() < F.wave) {
            const porrt_astar::QueueEntry e = queue.pop();
            held.push_back(e);
            if (nodes[(size_t)e.id].remaining && nodes[(size_t)e.id].kids < 0) batch.push_back((int64_t)e.id);
        }
        for (const porrt_astar::QueueEntry &e : held) queue.push(e.priority, e.id);
        ++T.info.waves;
        const int64_t rr = F.streams == 0 ? expand_sequential(batch[0]) : expand_wave(batch);
        if (rr < 0) return rr;
    }
    if (solution < 0) { c->set_err("No solution found!"); return PORRT_ERR_NO_PATH; }
    for (const AstarNode &n : nodes) if (n.kids >= 0 && !n.popped) ++A.info.speculated;
    std::vector<int64_t> chain;
    for (int64_t k = solution; k >= 0; k = nodes[(size_t)k].parent) chain.push_back(k);
    std::reverse(chain.begin(), chain.end());
    // the chain as TampNodes for the frame's finish: the paths stay on the device, tamp_build_policy sees their lengths
    std::vector<TampNode> cn(chain.size());
    TampChainSource src;
    src.arena = A.arena; src.ev = A.ev;
    for (size_t i = 0; i < chain.size(); ++i) {
        const AstarNode &n = nodes[(size_t)chain[i]];
        cn[i].target = n.target; cn[i].parent = (int64_t)i - 1; cn[i].ec = n.ec;
        cn[i].belief.assign(beliefs.begin() + (size_t)n.belief * nw, beliefs.begin() + (size_t)(n.belief + 1) * nw);
        cn[i].path_obs.assign(2 * (size_t)n.obs_len, 0.0);
        cn[i].path_pick.assign(2 * (size_t)n.pick_len, 0.0);
        src.paths.push_back({n.obs_off, n.obs_len, 0u, 0u});
        src.paths.push_back({n.pick_off, n.pick_len, 0u, 0u});
    }
    const int64_t n = F.finish(cn, (int64_t)cn.size() - 1, &src, A.info.children_s);
    if (n >= 0) A.info.chain_s = src.chain_s;
    return n;
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
