// porrt_plan_batch.hpp -- PTO::plan_belief_space (pto.rs:152-182) for many grown contexts in one call.
//
// The belief-graph kernels, the cost sweeps and the policy walk work on a node count, coordinate arrays and CSR lists, so a disjoint
// union of the members' PTO graphs is a PTO graph to them: member q's node j is union node noff[q] + j, its belief node id `id` is
// union id noff[q] * B + id (porrt_join.hpp).  No edge joins two members, the cost relaxation is monotone in f64 and every other
// stage works node by node or policy by policy, so a member's answers on the union are bit for bit its answers alone.
//
// A helper context owned by the leader (ctxs[0]) adopts the union as its PTO results -- the way grow_prm installs a roadmap -- and
// runs the stages of a single context on it, unchanged: build_belief_graph, compute_expected_costs, extract_policies with the starts
// noff[q] * B, and the refinement of those policies.  The union is gathered on the device (k_join_nodes, k_join_edges: one launch
// each for all the members of a pass, every thread finding its member by a fixed-length search over the offsets); the adjacency
// order needs the kd pre-order ranks PER MEMBER (a kd-tree over all the coordinates is not the members' own trees): from the members'
// cached host trees, or (option plan_batch_host_ranks = 0) from k_seg_kd_ranks with one segment per member.  One edge_order_build
// then serves the whole union: a rank is only ever compared inside one node's bucket, and a bucket holds nodes of one member.
// The members are not changed (their host caches of the tree may be filled); the answers live on the leader.
#pragma once
#include "porrt_join.hpp"

namespace {

struct JoinMember {
    const double *nx, *ny;
    const uint8_t *vid, *finalflag;
    const unsigned long long *finalmask;
    const uint32_t *efrom, *eto, *etv;
};
struct JoinConst {
    const JoinMember *members;
    const uint64_t *noff, *eoff;          // [n + 1]
    uint32_t n;
    double *nx, *ny;
    uint8_t *vid, *finalflag;
    unsigned long long *finalmask;
    uint32_t *efrom, *eto, *etv;
};

// union node i = node i - noff[q] of member q
__global__ __launch_bounds__(256) void k_join_nodes(JoinConst j) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= j.noff[j.n]) return;
    const uint32_t q = join_member_of(j.noff, j.n, i);
    const uint64_t k = i - j.noff[q];
    const JoinMember m = j.members[q];
    j.nx[i] = as_global(m.nx)[k]; j.ny[i] = as_global(m.ny)[k];
    j.vid[i] = as_global(m.vid)[k]; j.finalflag[i] = as_global(m.finalflag)[k];
    j.finalmask[i] = as_global(m.finalmask)[k];
}
// union edge e = edge e - eoff[q] of member q, both ends shifted by noff[q]
__global__ __launch_bounds__(256) void k_join_edges(JoinConst j) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= j.eoff[j.n]) return;
    const uint32_t q = join_member_of(j.eoff, j.n, e);
    const uint64_t k = e - j.eoff[q];
    const JoinMember m = j.members[q];
    const uint32_t shift = (uint32_t)j.noff[q];
    j.efrom[e] = as_global(m.efrom)[k] + shift; j.eto[e] = as_global(m.eto)[k] + shift;
    j.etv[e] = as_global(m.etv)[k];
}

struct PlanBatchState {
    int device = 0;
    porrt_ctx *helper = nullptr;
    uint64_t helper_raster_gen = 0;            // the leader's raster the helper carries
    GrowScratch scratch;                       // 0: member descriptors, 1 / 2: node / edge offsets, 3-8: the device ranks' segments and scratch
    bool valid = false;
    // the last call's answers, all passes
    std::vector<uint64_t> off;
    std::vector<uint8_t> status, rstatus, leaf;
    std::vector<double> cost, rcost, xy;
    std::vector<uint64_t> original;
    std::vector<int64_t> parent;
    // the last pass: its members' costs stay on the helper
    std::vector<porrt_ctx *> last_members;
    uint32_t last_first = 0;
    std::vector<uint64_t> last_noff;
    uint64_t last_B = 0;
    struct porrt_plan_batch_info info;
    PlanBatchState() { memset(&info, 0, sizeof info); }
    ~PlanBatchState() {
        if (helper) porrt_destroy(helper);
        (void)hipSetDevice(device);
        scratch.free_all();
    }
};

PlanBatchState &plan_batch_state(porrt_ctx *c) {
    if (!c->plan_batch) {
        PlanBatchState *t = new PlanBatchState();
        t->device = c->device;
        c->plan_batch = std::shared_ptr<void>(t, [](void *q) { delete (PlanBatchState *)q; });
    }
    return *(PlanBatchState *)c->plan_batch.get();
}

// what the members must share with the leader: the raster, its frame, the zones and the visibility (tens of kilobytes, on the host)
bool plan_batch_same_domain(const porrt_ctx *a, const porrt_ctx *b) {
    return a->has_grid == b->has_grid && a->W == b->W && a->H == b->H && a->domain == b->domain && a->low[0] == b->low[0] && a->low[1] == b->low[1] &&
           a->up[0] == b->up[0] && a->up[1] == b->up[1] && a->visibility == b->visibility && a->occ == b->occ && a->zones == b->zones;
}

// the kd pre-order rank of every node of member m (sequential KdTree::add in id order), from its cached host tree
void plan_batch_host_ranks(const HostKd *kd, size_t N, uint32_t *rank) {
    std::vector<int> stack;
    uint32_t next = 0;
    if (N) stack.push_back(0);
    while (!stack.empty()) {
        const int n = stack.back();
        stack.pop_back();
        rank[n] = next++;
        if (kd->right[n] >= 0) stack.push_back(kd->right[n]);      // left subtree first (popped first)
        if (kd->left[n] >= 0) stack.push_back(kd->left[n]);
    }
}

// One pass: members ms[0 .. n) as one union on the helper h, through every stage; the answers are appended to S.
int plan_batch_pass(porrt_ctx *lead, PlanBatchState &S, porrt_ctx *const *ms, uint32_t n, const double *start_belief, uint32_t n_worlds, uint64_t B,
                    uint64_t refine_iterations) {
    porrt_ctx *h = S.helper;
    std::vector<uint64_t> noff(n + 1, 0), eoff(n + 1, 0);
    for (uint32_t q = 0; q < n; ++q) { noff[q + 1] = noff[q] + ms[q]->n_nodes; eoff[q + 1] = eoff[q] + ms[q]->counters.n_edges; }
    const size_t N = (size_t)noff[n], E = (size_t)eoff[n];
    if (N >= 0x7FFFFFFFull || E > kJoinEdgesLimit) { lead->set_err("plan_belief_space_batch: a member's graph is too large"); return PORRT_ERR_CAPACITY; }
    auto fail = [&](int r) { lead->set_err("plan_belief_space_batch: " + h->err); return r; };
    auto dev_fail = [&](const char *what, hipError_t e) {
        lead->set_err(std::string("plan_belief_space_batch: ") + what + ": " + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? PORRT_ERR_CAPACITY : PORRT_ERR_DEVICE;
    };
#define PB_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return dev_fail(#expr, e_); } while (0)
    double t0 = now_s();
    // ---- the helper adopts the union as its PTO results (cf. grow_prm)
    h->have_results = false;
    h->batch_leader = nullptr;
    h->bg.release();
    h->dp.release();
    ++h->results_tag;
    (void)h->d_nx.reserve(N); (void)h->d_ny.reserve(N); (void)h->d_vid.reserve(N); (void)h->d_finalflag.reserve(N); (void)h->d_finalmask.reserve(N);
    (void)h->d_cnt.reserve(1); (void)h->d_rc.reserve(1); (void)h->d_cls.reserve(cls_bytes(h->W, h->H));
    (void)h->d_efrom.reserve(E + 1); (void)h->d_eto.reserve(E + 1); (void)h->d_etv.reserve(E + 1);
    int r = h->layout_buffers();
    if (r) return r == PORRT_ERR_DEVICE ? (lead->set_err("plan_belief_space_batch: the union's buffers could not be allocated: " + h->err), PORRT_ERR_CAPACITY) : fail(r);
    if ((r = h->build_cls())) return fail(r);
    hipStream_t s = h->stream;
    memset(&h->rc, 0, sizeof h->rc);
    h->rc.nx = h->d_nx.p; h->rc.ny = h->d_ny.p; h->rc.vid = h->d_vid.p;
    h->raster_view(h->rc, h->d_cls.p);
    h->rc.all_worlds = ones(h->n_worlds);
    h->rc.visibility = h->visibility;
    PB_HIP(hipMemcpyAsync(h->d_rc.p, &h->rc, sizeof h->rc, hipMemcpyHostToDevice, s));
    std::vector<JoinMember> tab(n);
    for (uint32_t q = 0; q < n; ++q) {
        const porrt_ctx *m = ms[q];
        tab[q] = JoinMember{m->d_nx.p, m->d_ny.p, m->d_vid.p, m->d_finalflag.p, m->d_finalmask.p, m->d_efrom.p, m->d_eto.p, m->d_etv.p};
    }
    JoinConst j{};
    JoinMember *d_tab = nullptr;
    uint64_t *d_noff = nullptr, *d_eoff = nullptr;
    PB_HIP(S.scratch.get(0, d_tab, n)); PB_HIP(S.scratch.get(1, d_noff, n + 1)); PB_HIP(S.scratch.get(2, d_eoff, n + 1));
    PB_HIP(hipMemcpyAsync(d_tab, tab.data(), n * sizeof(JoinMember), hipMemcpyHostToDevice, s));
    PB_HIP(hipMemcpyAsync(d_noff, noff.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    PB_HIP(hipMemcpyAsync(d_eoff, eoff.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    j.members = d_tab; j.noff = d_noff; j.eoff = d_eoff; j.n = n;
    j.nx = h->d_nx.p; j.ny = h->d_ny.p; j.vid = h->d_vid.p; j.finalflag = h->d_finalflag.p; j.finalmask = h->d_finalmask.p;
    j.efrom = h->d_efrom.p; j.eto = h->d_eto.p; j.etv = h->d_etv.p;
    const dim3 block(256);
    if (N) hipLaunchKernelGGL(k_join_nodes, dim3((unsigned)((N + 255) / 256)), block, 0, s, j);
    if (E) hipLaunchKernelGGL(k_join_edges, dim3((unsigned)((E + 255) / 256)), block, 0, s, j);
    // one download: the union's states (the policies' states), validity ids, final flags and masks (the final belief nodes)
    h->h_nx.resize(N); h->h_ny.resize(N); h->h_vid.resize(N); h->h_finalflag.resize(N); h->h_finalmask.resize(N);
    h->h_parent.assign(N, -1); h->h_reach.assign(N, 0ull);
    PB_HIP(hipMemcpyAsync(h->h_nx.data(), h->d_nx.p, N * 8, hipMemcpyDeviceToHost, s));
    PB_HIP(hipMemcpyAsync(h->h_ny.data(), h->d_ny.p, N * 8, hipMemcpyDeviceToHost, s));
    PB_HIP(hipMemcpyAsync(h->h_vid.data(), h->d_vid.p, N, hipMemcpyDeviceToHost, s));
    PB_HIP(hipMemcpyAsync(h->h_finalflag.data(), h->d_finalflag.p, N, hipMemcpyDeviceToHost, s));
    PB_HIP(hipMemcpyAsync(h->h_finalmask.data(), h->d_finalmask.p, N * 8, hipMemcpyDeviceToHost, s));
    PB_HIP(hipStreamSynchronize(s));
    PB_HIP(hipGetLastError());
    h->h_final_ids.clear();
    for (size_t i = 0; i < N; ++i) if (h->h_finalflag[i]) h->h_final_ids.push_back(i);
    memset(&h->counters, 0, sizeof h->counters);
    h->counters.n_edges = (uint32_t)E;
    h->counters.n_final = (uint32_t)h->h_final_ids.size();
    h->mode = PORRT_MODE_PTO;
    h->n_nodes = N; h->n_iter = 0; h->n_steps = 0;
    h->complete = false;
    memset(&h->metrics, 0, sizeof h->metrics);
    h->have_results = true;
    h->downloaded_tag = h->results_tag;
    h->got = porrt_ctx::DL_TREE | porrt_ctx::DL_MASKS;
    S.info.ms_join += 1e3 * (now_s() - t0);

    // ---- the adjacency order: ranks per member, one edge order over the union
    t0 = now_s();
    std::string e;
    if (lead->opt_plan_batch_host_ranks) {
        for (uint32_t q = 0; q < n; ++q)
            if ((r = ms[q]->download(porrt_ctx::DL_TREE))) { lead->set_err("plan_belief_space_batch: a member's tree: " + ms[q]->err); return r; }
        std::vector<uint32_t> rank(N, 0);
        const unsigned nt = std::max(1u, std::min<unsigned>(std::min<unsigned>(8u, n), std::max(1u, std::thread::hardware_concurrency())));
        std::vector<uint8_t> threw(nt, 0);
        auto work = [&](unsigned t) {
            try {
                for (uint32_t q = t; q < n; q += nt) plan_batch_host_ranks(host_kd_of(ms[q]), (size_t)ms[q]->n_nodes, rank.data() + noff[q]);
            } catch (...) { threw[t] = 1; }
        };
        {
            struct Joiner { std::vector<std::thread> th; ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); } } pool;
            for (unsigned t = 1; t < nt; ++t) pool.th.emplace_back(work, t);
            work(0);
        }
        for (uint8_t t : threw) if (t) { lead->set_err("plan_belief_space_batch: out of host memory for the members' kd-trees"); return PORRT_ERR_NOMEM; }
        r = edge_order_build(h->eo, h->results_tag, N, E, h->d_efrom.p, h->d_eto.p, h->d_etv.p, &rank, nullptr, nullptr, s, e);
    } else {
        std::vector<uint32_t> seg(n + 1);
        for (uint32_t q = 0; q <= n; ++q) seg[q] = (uint32_t)noff[q];
        uint32_t *d_seg = nullptr, *d_aux = nullptr, *d_sz = nullptr, *d_rank = nullptr;
        int *d_child = nullptr, *d_par = nullptr;
        PB_HIP(S.scratch.get(3, d_seg, n + 1)); PB_HIP(S.scratch.get(4, d_child, 2 * N)); PB_HIP(S.scratch.get(5, d_par, N));
        PB_HIP(S.scratch.get(6, d_aux, N)); PB_HIP(S.scratch.get(7, d_sz, N)); PB_HIP(S.scratch.get(8, d_rank, N));
        PB_HIP(hipMemcpyAsync(d_seg, seg.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_seg_kd_ranks, dim3(n), block, 0, s, (const double *)h->d_nx.p, (const double *)h->d_ny.p, (const uint32_t *)d_seg, d_child, d_par, d_aux, d_sz,
                           d_rank);
        r = edge_order_build(h->eo, h->results_tag, N, E, h->d_efrom.p, h->d_eto.p, h->d_etv.p, nullptr, nullptr, nullptr, s, e, d_rank);
    }
    if (r) { lead->set_err("plan_belief_space_batch: " + e); return r == PORRT_ERR_DEVICE && e.find("hipMalloc") != std::string::npos ? PORRT_ERR_CAPACITY : r; }
    S.info.ms_edge_order += 1e3 * (now_s() - t0);

    // ---- the stages of a single context, on the union
    t0 = now_s();
    if ((r = h->build_belief_graph(start_belief, n_worlds))) return r == PORRT_ERR_DEVICE && h->err.find("hipMalloc") != std::string::npos ? fail(PORRT_ERR_CAPACITY) : fail(r);
    if (h->bg.B != B) { lead->set_err("plan_belief_space_batch: the belief space changed between the planning of the passes and the build"); return PORRT_ERR_INVALID; }
    S.info.ms_belief_graph += 1e3 * (now_s() - t0);
    S.info.belief_edges += h->bg.n_edges;
    S.info.ms_device += 1e3 * h->bg.t_device;
    t0 = now_s();
    if ((r = h->compute_expected_costs())) return r == PORRT_ERR_DEVICE && h->err.find("hipMalloc") != std::string::npos ? fail(PORRT_ERR_CAPACITY) : fail(r);
    S.info.ms_costs += 1e3 * (now_s() - t0);
    S.info.final_belief_nodes += h->n_final_belief_nodes;
    S.info.ms_device += 1e3 * h->dp.t_device;
    t0 = now_s();
    std::vector<uint64_t> starts(n), poff(n + 1);
    std::vector<uint8_t> pstatus(n);
    std::vector<double> pcost(n);
    for (uint32_t q = 0; q < n; ++q) starts[q] = join_union_id(noff[q], B, 0);
    const int64_t total = h->extract_policies(starts.data(), n, poff.data(), pstatus.data(), pcost.data(), nullptr, nullptr, nullptr, 0);
    if (total < 0) return fail((int)total);
    S.info.ms_policies += 1e3 * (now_s() - t0);
    S.info.ms_device += h->policies.info.ms_device;
    const PoliciesResult &pol = h->policies;
    const size_t q0 = S.status.size();               // members answered by the passes before
    uint64_t base = S.off.back();
    S.status.insert(S.status.end(), pstatus.begin(), pstatus.end());
    S.cost.insert(S.cost.end(), pcost.begin(), pcost.end());
    if (refine_iterations == 0) {
        for (uint32_t q = 0; q < n; ++q) {
            S.rstatus.push_back(1); S.rcost.push_back(0.0);
            for (uint64_t k = poff[q]; k < poff[q + 1]; ++k) {
                const uint64_t node = pol.original[k] / B;
                S.xy.push_back(h->h_nx[node]); S.xy.push_back(h->h_ny[node]);
                S.original.push_back(join_own_id(noff[q], B, pol.original[k]));
                S.parent.push_back(pol.parent[k]);
                S.leaf.push_back(pol.leaf[k]);
            }
            S.off.push_back(base + poff[q + 1]);
        }
    } else {
        t0 = now_s();
        const uint64_t cap = std::max<uint64_t>((uint64_t)total, 1);
        std::vector<uint64_t> roff(n + 1), roid(cap);
        std::vector<uint8_t> rst(n), rleaf(cap);
        std::vector<double> rc(n), rxy(2 * cap);
        std::vector<int64_t> rpar(cap);
        porrt_ctx::RefineInBuf buf;
        const int64_t rt = h->refine_call("plan_belief_space_batch", false, h->refine_in(pol, buf), refine_iterations,
                                          RefinePoliciesOut{roff.data(), rst.data(), rc.data(), rxy.data(), roid.data(), rpar.data(), rleaf.data(), cap}, nullptr);
        if (rt < 0) return fail((int)rt);
        if ((uint64_t)rt > cap) { lead->set_err("plan_belief_space_batch: the refinement returned more nodes than went in"); return PORRT_ERR_INVALID; }
        S.info.ms_refine += 1e3 * (now_s() - t0);
        S.info.ms_device += h->refp_info.ms_device;
        for (uint32_t q = 0; q < n; ++q) {
            S.rstatus.push_back(rst[q]); S.rcost.push_back(rc[q]);
            for (uint64_t k = roff[q]; k < roff[q + 1]; ++k) {
                S.xy.push_back(rxy[2 * k]); S.xy.push_back(rxy[2 * k + 1]);
                S.original.push_back(join_own_id(noff[q], B, roid[k]));
                S.parent.push_back(rpar[k]);
                S.leaf.push_back(rleaf[k]);
            }
            S.off.push_back(base + roff[q + 1]);
        }
    }
    for (uint32_t q = 0; q < n; ++q) S.info.policies_ok += S.status[q0 + q] == 0 ? 1 : 0;
    S.info.graph_nodes += N; S.info.graph_edges += E; S.info.belief_nodes += (uint64_t)N * B;
    S.last_first = (uint32_t)q0;
    S.last_noff = noff;
    S.last_B = B;
    S.last_members.assign(ms, ms + n);
#undef PB_HIP
    return PORRT_OK;
}

// copies the kept answers into the caller's arrays (the node arrays when cap holds the total)
int64_t plan_batch_copy_out(const PlanBatchState &S, uint64_t *pol_off, uint8_t *status, double *expected_costs, uint8_t *refine_status, double *refined_costs,
                            double *xy, uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, uint64_t cap) {
    const uint64_t n = S.status.size(), total = S.off.back();
    if (pol_off) memcpy(pol_off, S.off.data(), (n + 1) * sizeof(uint64_t));
    if (n && status) memcpy(status, S.status.data(), n);
    if (n && expected_costs) memcpy(expected_costs, S.cost.data(), n * sizeof(double));
    if (n && refine_status) memcpy(refine_status, S.rstatus.data(), n);
    if (n && refined_costs) memcpy(refined_costs, S.rcost.data(), n * sizeof(double));
    if (total && total <= cap) {
        if (xy) memcpy(xy, S.xy.data(), 2 * total * sizeof(double));
        if (original_ids) memcpy(original_ids, S.original.data(), total * sizeof(uint64_t));
        if (parents) memcpy(parents, S.parent.data(), total * sizeof(int64_t));
        if (is_leaf) memcpy(is_leaf, S.leaf.data(), total);
    }
    return (int64_t)total;
}

int64_t plan_belief_space_batch(porrt_ctx *const *ctxs, uint32_t n_ctx, const double *start_belief, uint32_t n_worlds, uint64_t refine_iterations, uint64_t *pol_off,
                                uint8_t *status, double *expected_costs, uint8_t *refine_status, double *refined_costs, double *xy, uint64_t *original_ids,
                                int64_t *parents, uint8_t *is_leaf, uint64_t cap) {
    porrt_ctx *lead = ctxs[0];
    const double t_call = now_s();
    // ---- refusals, before any launch
    auto refuse = [&](const std::string &what) { lead->set_err("plan_belief_space_batch: " + what); return (int64_t)PORRT_ERR_INVALID; };
    if (lead->plan_batch) ((PlanBatchState *)lead->plan_batch.get())->valid = false;
    if (!pol_off || !status || !expected_costs || !start_belief) return refuse("start_belief, pol_off, status and expected_costs are needed");
    if (refine_iterations >= (1ull << 31)) return refuse("refine_iterations must be below 2^31");
    {
        std::vector<const porrt_ctx *> sorted(ctxs, ctxs + n_ctx);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return refuse("the same context is given twice");
    }
    for (uint32_t q = 0; q < n_ctx; ++q) {
        const porrt_ctx *m = ctxs[q];
        const std::string who = "member " + std::to_string(q);
        if (m->device != lead->device) return refuse(who + " is on another device");
        if (!m->have_results || m->mode != PORRT_MODE_PTO) return refuse(who + " holds no PTO graph (porrt_grow / porrt_grow_batch, mode PORRT_MODE_PTO)");
        if (q && !plan_batch_same_domain(lead, m)) return refuse(who + ": its raster, frame, domain kind, zones or visibility differ from member 0's");
        if ((int)n_worlds != m->n_worlds) return refuse(who + ": the start belief needs one probability per world");
    }
    {
        double s = 0.0;                                  // assert_belief_state_validity (common.rs:279-281), as porrt_build_belief_graph sums it
        for (uint32_t w = 0; w < n_worlds; ++w) s = start_belief[w] + s;
        if (!(std::fabs(s - 1.0) < 0.000001)) return refuse("start belief state does not sum to 1");
    }
    if (hipSetDevice(lead->device) != hipSuccess) { lead->set_err("plan_belief_space_batch: hipSetDevice"); return PORRT_ERR_DEVICE; }
    PlanBatchState &S = plan_batch_state(lead);
    if (!S.helper) {
        S.helper = porrt_create(lead->device);
        if (!S.helper) { lead->set_err("plan_belief_space_batch: the helper context could not be created"); return PORRT_ERR_DEVICE; }
    }
    porrt_ctx *h = S.helper;
    if (S.helper_raster_gen != lead->raster_gen) { tamp_copy_domain(h, lead); S.helper_raster_gen = lead->raster_gen; }
    if (h->opt_box_table != lead->opt_box_table) { h->opt_box_table = lead->opt_box_table; h->cls_dirty = true; }
    h->opt_dp_sweeps = lead->opt_dp_sweeps; h->opt_dp_wide_rows = lead->opt_dp_wide_rows; h->opt_policy_max_nodes = lead->opt_policy_max_nodes;
    h->opt_refine_short_lds = lead->opt_refine_short_lds;
    // the number of beliefs, which the cut into passes needs: the reachable beliefs of the prior, kept by the helper for the builds
    std::string e;
    int r = belief_cache_fill(h->bg.cache, h->domain, h->n_zones, h->n_validities, h->n_worlds, h->validities, start_belief, e);
    if (r) { lead->set_err("plan_belief_space_batch: " + e); return r; }
    const uint64_t B = h->bg.cache.space.size();
    S.off.assign(1, 0);
    S.status.clear(); S.rstatus.clear(); S.leaf.clear(); S.cost.clear(); S.rcost.clear(); S.xy.clear(); S.original.clear(); S.parent.clear();
    S.last_members.clear();
    memset(&S.info, 0, sizeof S.info);
    S.info.members = n_ctx; S.info.beliefs = B;
    std::vector<uint64_t> nodes(n_ctx), edges(n_ctx);
    for (uint32_t q = 0; q < n_ctx; ++q) { nodes[q] = ctxs[q]->n_nodes; edges[q] = ctxs[q]->counters.n_edges; }
    for (uint32_t first = 0; first < n_ctx;) {
        const uint32_t end = join_pass_end(nodes.data(), edges.data(), n_ctx, first, B, lead->opt_plan_batch_max_belief_nodes);
        if ((r = plan_batch_pass(lead, S, ctxs + first, end - first, start_belief, n_worlds, B, refine_iterations))) return r;
        ++S.info.passes;
        first = end;
    }
    S.info.policy_nodes = S.off.back();
    S.info.ms_wall = 1e3 * (now_s() - t_call);
    S.valid = true;
    for (uint32_t q = 0; q < n_ctx; ++q)
        if (S.status[q]) { lead->set_err("plan_belief_space_batch: member " + std::to_string(q) + ": " + kPolStatusText[S.status[q] < 5 ? S.status[q] : 0]); break; }
    return plan_batch_copy_out(S, pol_off, status, expected_costs, refine_status, refined_costs, xy, original_ids, parents, is_leaf, cap);
}

} // namespace
