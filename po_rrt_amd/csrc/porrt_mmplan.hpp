// porrt_mmplan.hpp -- the rest of MapShelfDomainTampPRM::plan (src/map_shelves_tamp_prm.rs:310-326) after grow_mm_prm:
// build_belief_graph (:395-473), compute_expected_costs_to_goals (:475-477, conditional_dijkstra) and extract_policy (:479-485).
//
// The mode-product belief graph.  Belief node id = mode_off[m] + roadmap node (modes in mode order, nodes in add_sample order), so
// node 0 is the planning start and the node coordinates are the roadmaps' own, already on the device end to end (roadmaps_of_modes).
// Its edges, in the reference's add_edge order:
//   * observation edges first: for each transition, each [from, to] pair; the from node becomes an Observation node;
//   * then action edges: for each mode, each node that is not an Observation node, one edge per roadmap child in PTONode::children
//     order.  prm.rs:96-103 adds all nbr -> new edges, then all new -> nbr edges, so node u's roadmap children are e.from of the
//     forward edges e.to == u (u's own segment of the forward list), then e.to of the edges e.from == u: by forward-edge position.
// So a node's children are ordered by a key -- the pair index for an observation node, the forward-edge position for an action
// node -- and a node's parents by the global add_edge order: pair index k for an observation parent, P + u for an action parent u
// (action edges come node by node).  Count, scan, scatter (atomic cursors), then one wave per node orders its bucket by the key
// (k_eo_segsort).  No host loop over edges.
//
// The expected costs by level.  Action edges never leave a mode, and every observation edge leads to a mode with fewer possible
// worlds (checked on the transitions; the general sweeps otherwise).  So the modes are grouped into levels by their number of possible
// worlds and the levels finished from the fewest worlds up, one launch per level and one workgroup per mode (k_mm_level): first the
// mode's observation nodes take their sum over the finished deeper levels, then the mode's roadmap relaxes to its fixpoint with
// workgroup barriers between sweeps -- in LDS when the mode fits (kMmLdsNodes), on global memory otherwise.  The relaxation is the
// monotone fixpoint of porrt_dp.hpp, so it ends in the general sweeps' bits.  Measured, it loses to the general sweeps (a mode's chain of
// barrier-separated sweeps runs on one CU while the sweeps spread every level over the whole GPU): it is an option ("mm_levels"), the
// sweeps are the default.
#pragma once

namespace porrt {

constexpr uint32_t kMmLdsNodes = 6400;               // 8 bytes of cost + 2 mark bytes per node: 64000 B of LDS per workgroup

enum : uint32_t { MM_ERR_PAIR = 1, MM_ERR_EDGE = 2, MM_ERR_LEAVES_MODE = 4, MM_ERR_NO_FIXPOINT = 8 };

struct MmBgConst {
    uint32_t NT, n_modes, n_tr;
    uint32_t P;                                      // observation pairs
    const uint32_t *mode_off;                        // [n_modes + 1]
    const uint32_t *mode_bid;                        // [n_modes] belief id (index in reachable_belief_states)
    const unsigned long long *edge_off;              // [NT + 1] forward edges of new node i (global node index)
    const uint32_t *efrom;                           // [E] neighbour, index within the mode
    const unsigned long long *pairs;                 // [P][2] [from node, to node] within their modes
    const uint32_t *tr_off, *tr_from, *tr_to;        // [n_tr + 1] first pair of each transition; its modes
    uint8_t *types;
    uint32_t *mode_of, *bid;                         // [NT] mode and belief id of every node
    uint32_t *cnt_c, *cnt_p, *cur_c, *cur_p;         // [NT]
    const unsigned long long *child_off, *par_off;   // [NT + 1]
    uint32_t *ckey, *cval, *pkey, *pval;             // buckets before ordering
    uint32_t *err;
};

__device__ __forceinline__ uint32_t mm_upper(const uint32_t *a, uint32_t n, uint32_t v) {      // first index k in [0, n) with a[k] > v
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (as_global(a)[mid] > v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// every node: its mode, belief id, type Action (add_node, :405-411)
__global__ __launch_bounds__(256) void k_mmbg_nodes(MmBgConst g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.NT) return;
    const uint32_t m = mm_upper(g.mode_off, g.n_modes + 1, i) - 1;
    g.mode_of[i] = m;
    g.bid[i] = as_global(g.mode_bid)[m];
    g.types[i] = BG_ACTION;
}

// observation pairs (:421-438): a node that is missing in its mode is the reference's HashMap index panic
template <bool FILL>
__global__ __launch_bounds__(256) void k_mmbg_pairs(MmBgConst g) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= g.P) return;
    const uint32_t t = mm_upper(g.tr_off, g.n_tr + 1, k) - 1;
    const uint32_t mf = as_global(g.tr_from)[t], mt = as_global(g.tr_to)[t];
    const unsigned long long lf = as_global(g.pairs)[2 * (size_t)k], lt = as_global(g.pairs)[2 * (size_t)k + 1];
    const uint32_t f0 = as_global(g.mode_off)[mf], t0 = as_global(g.mode_off)[mt];
    if (lf >= as_global(g.mode_off)[mf + 1] - f0 || lt >= as_global(g.mode_off)[mt + 1] - t0) { atomicOr(g.err, MM_ERR_PAIR); return; }
    const uint32_t u = f0 + (uint32_t)lf, v = t0 + (uint32_t)lt;
    if (!FILL) {
        g.types[u] = BG_OBSERVATION;
        atomicAdd(&g.cnt_c[u], 1u);
        atomicAdd(&g.cnt_p[v], 1u);
    } else {
        const unsigned long long c = g.child_off[u] + atomicAdd(&g.cur_c[u], 1u), p = g.par_off[v] + atomicAdd(&g.cur_p[v], 1u);
        g.ckey[c] = k; g.cval[c] = v;
        g.pkey[p] = k; g.pval[p] = u;
    }
}

// roadmap edges (:441-470): forward edge e = (f -> i) is the roadmap child i of f and the roadmap child f of i; each becomes an action
// edge when its source is not an Observation node
template <bool FILL>
__global__ __launch_bounds__(256) void k_mmbg_roadmap(MmBgConst g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.NT) return;
    const uint32_t b = as_global(g.mode_off)[as_global(g.mode_of)[i]];
    const bool ia = as_global(g.types)[i] == BG_ACTION;
    const unsigned long long e0 = as_global(g.edge_off)[i], e1 = as_global(g.edge_off)[i + 1];
    uint32_t own_c = 0, own_p = 0;
    for (unsigned long long e = e0; e < e1; ++e) {
        const uint32_t lf = as_global(g.efrom)[e];
        if (lf >= i - b) { atomicOr(g.err, MM_ERR_EDGE); return; }
        const uint32_t f = b + lf;
        const bool fa = as_global(g.types)[f] == BG_ACTION;
        if (!FILL) {
            own_c += ia ? 1u : 0u;
            own_p += fa ? 1u : 0u;
            if (fa) atomicAdd(&g.cnt_c[f], 1u);
            if (ia) atomicAdd(&g.cnt_p[f], 1u);
        } else {
            if (ia) {                                                    // i -> f
                const unsigned long long c = g.child_off[i] + atomicAdd(&g.cur_c[i], 1u), p = g.par_off[f] + atomicAdd(&g.cur_p[f], 1u);
                g.ckey[c] = (uint32_t)e; g.cval[c] = f;
                g.pkey[p] = g.P + i; g.pval[p] = i;
            }
            if (fa) {                                                    // f -> i
                const unsigned long long c = g.child_off[f] + atomicAdd(&g.cur_c[f], 1u), p = g.par_off[i] + atomicAdd(&g.cur_p[i], 1u);
                g.ckey[c] = (uint32_t)e; g.cval[c] = i;
                g.pkey[p] = g.P + f; g.pval[p] = f;
            }
        }
    }
    if (!FILL) {
        if (own_c) atomicAdd(&g.cnt_c[i], own_c);
        if (own_p) atomicAdd(&g.cnt_p[i], own_p);
    }
}

// ---- expected costs, one level (modes of one number of possible worlds) per launch, one workgroup per mode
struct MmLevelConst {
    DpConst g;                                       // explicit layout: bvec = mode of the node, beliefs = the modes' belief rows
    const uint32_t *mode_off, *modes;                // modes of this level
    uint32_t lds_cap;                                // modes of at most this many nodes relax in LDS
    uint8_t *mark[2];                                // [NT] marks of the global-memory path
    uint32_t *err;
    unsigned long long *sweeps;                      // [0] sweeps summed over modes, [1] the most sweeps of one mode
};

// dist as the workgroup shares it: single-copy atomic loads and stores (a sweep reads what another lane of it may be writing)
template <bool LDS>
__device__ __forceinline__ double mm_ld(const double *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool LDS>
__device__ __forceinline__ void mm_st(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Relaxes the action nodes of [m0, m0 + n) to their fixpoint: D = the mode's costs (LDS or its slice of dist), M0 / M1 = marks.
// A node is evaluated in the sweep after one of its children improved (the first sweep: mm_mark_sources); it takes
// min over children (norm2 + dist), the arithmetic of k_dp_sweep's action branch.
template <bool LDS>
__device__ void mm_relax(const MmLevelConst &L, uint32_t m0, uint32_t n, double *D, uint8_t *M0, uint8_t *M1) {
    const DpConst &g = L.g;
    uint32_t sweep = 0;
    for (;; ++sweep) {
        uint8_t *cur = (sweep & 1u) ? M1 : M0, *nxt = (sweep & 1u) ? M0 : M1;
        bool any = false;
        for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) {
            if (!cur[v]) continue;
            cur[v] = 0;
            const uint32_t u = m0 + v;
            if (as_global(g.types)[u] != BG_ACTION) continue;
            const double ux = as_global(g.nx)[u], uy = as_global(g.ny)[u];
            double alt = __builtin_huge_val();
            const unsigned long long c0 = as_global(g.child_off)[u], c1 = as_global(g.child_off)[u + 1];
            for (unsigned long long c = c0; c < c1; ++c) {
                const uint32_t w = as_global(g.child_id)[c];
                if (w - m0 >= n) { atomicOr(L.err, MM_ERR_LEAVES_MODE); continue; }
                const double cost = sqrt(dist2(ux, uy, as_global(g.nx)[w], as_global(g.ny)[w]));
                const double a = cost + mm_ld<LDS>(D + (w - m0));
                alt = a < alt ? a : alt;
            }
            if (alt < mm_ld<LDS>(D + v)) {
                mm_st<LDS>(D + v, alt);
                any = true;
                for (unsigned long long e = as_global(g.par_off)[u]; e < as_global(g.par_off)[u + 1]; ++e) {
                    const uint32_t p = as_global(g.par_id)[e];
                    if (p - m0 < n) nxt[p - m0] = 1;                      // (observation parents live in other modes)
                }
            }
        }
        if (!__syncthreads_or(any)) break;
        if (sweep > (1u << 22)) { if (threadIdx.x == 0) atomicOr(L.err, MM_ERR_NO_FIXPOINT); break; }
    }
    if (threadIdx.x == 0) {
        atomicAdd(&L.sweeps[0], (unsigned long long)(sweep + 1u));
        atomicMax(&L.sweeps[1], (unsigned long long)(sweep + 1u));
    }
}

// the first sweep's marks: the mode's parents of every node that already has a finite cost (finals, observation nodes that reach a goal)
// -- a mode without one ends after a sweep that evaluates nothing
__device__ __forceinline__ void mm_mark_sources(const DpConst &g, uint32_t m0, uint32_t n, uint8_t *M0) {
    for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) {
        const uint32_t u = m0 + v;
        if (!(as_global(g.dist)[u] < __builtin_huge_val())) continue;
        for (unsigned long long e = as_global(g.par_off)[u]; e < as_global(g.par_off)[u + 1]; ++e) {
            const uint32_t p = as_global(g.par_id)[e];
            if (p - m0 < n) M0[p - m0] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void k_mm_level(MmLevelConst L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mm_lds[];
    const DpConst &g = L.g;
    const uint32_t m = as_global(L.modes)[blockIdx.x];
    const uint32_t m0 = as_global(L.mode_off)[m], n = as_global(L.mode_off)[m + 1] - m0;
    // observation nodes: the sum over their children, all in finished deeper levels (k_dp_sweep's observation branch)
    for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) {
        const uint32_t u = m0 + v;
        if (as_global(g.types)[u] != BG_OBSERVATION) continue;
        const double ux = as_global(g.nx)[u], uy = as_global(g.ny)[u];
        const uint32_t urow = as_global(g.bvec)[u];
        double alt = 0.0;
        for (unsigned long long c = as_global(g.child_off)[u]; c < as_global(g.child_off)[u + 1]; ++c) {
            const uint32_t w = as_global(g.child_id)[c];
            const uint32_t vrow = as_global(g.bvec)[w];
            double p = 0.0;                                           // transition_probability (common.rs:187-190)
            for (uint32_t k = 0; k < g.nw; ++k)
                p = p + (as_global(g.beliefs)[(size_t)vrow * g.nw + k] > 0.0 ? as_global(g.beliefs)[(size_t)urow * g.nw + k] : 0.0);
            if (!(p > 0.0)) atomicOr(&g.flags[0], DP_ERR_ZERO_PROBABILITY);   // assert!(p > 0.0)
            const double cost = sqrt(dist2(ux, uy, as_global(g.nx)[w], as_global(g.ny)[w]));
            alt = alt + p * (cost + as_global(g.dist)[w]);
        }
        if (alt < as_global(g.dist)[u]) g.dist[u] = alt;
    }
    __syncthreads();
    if (n <= L.lds_cap) {
        double *D = (double *)mm_lds;
        uint8_t *M0 = mm_lds + (size_t)L.lds_cap * 8, *M1 = M0 + L.lds_cap;
        for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) {
            D[v] = g.dist[m0 + v];
            M0[v] = 0;
            M1[v] = 0;
        }
        __syncthreads();
        mm_mark_sources(g, m0, n, M0);
        __syncthreads();
        mm_relax<true>(L, m0, n, D, M0, M1);
        __syncthreads();
        for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) g.dist[m0 + v] = D[v];
    } else {
        uint8_t *M0 = L.mark[0] + m0, *M1 = L.mark[1] + m0;
        for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) { M0[v] = 0; M1[v] = 0; }
        __syncthreads();
        mm_mark_sources(g, m0, n, M0);
        __syncthreads();
        mm_relax<false>(L, m0, n, g.dist + m0, M0, M1);
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct MmPlanState {
    // the belief graph (valid for mm_gen == the mode tree's generation)
    bool valid = false;
    uint64_t gen = 0;
    size_t NT = 0, n_modes = 0;
    uint32_t nw = 0;
    unsigned long long n_edges = 0;
    std::vector<uint32_t> mode_off, mode_bid, support;           // per mode: first node, belief id, number of possible worlds
    std::vector<double> beliefs;                                 // [n_modes][nw] the modes' own belief vectors
    std::vector<unsigned long long> finals;                      // final belief nodes, in mode order
    bool support_shrinks = false;                                // every transition leads to a mode with fewer possible worlds
    DpConst c{};                                                 // device arrays of the graph (explicit layout)
    uint32_t *d_mode_off = nullptr, *d_bid = nullptr;
    double t_build = 0, t_build_device = 0;
    // the expected costs (valid for costs_gen == gen)
    DpState dp;
    uint64_t costs_gen = ~0ull;
    uint32_t levels = 0, launches = 0;
    unsigned long long level_sweeps = 0, max_mode_sweeps = 0;
    double t_costs = 0, t_costs_device = 0, t_extract = 0, t_refine = 0, t_refine_device = 0, t_grow = 0;
    uint32_t lds_cap = kMmLdsNodes;                              // option "mm_lds_nodes"
    bool use_levels = false;                                     // option "mm_levels": the level schedule (slower than the sweeps)
    void release() { valid = false; dp.release(); costs_gen = ~0ull; }
};

static inline uint32_t mm_mode_of(const MmPlanState &s, uint64_t node) {
    return (uint32_t)(std::upper_bound(s.mode_off.begin(), s.mode_off.end(), (uint32_t)node) - s.mode_off.begin()) - 1;
}

// Level schedule on the graph of s (finals and dist slots set up by the caller's DpState): modes grouped by their number of possible
// worlds, fewest first; one k_mm_level launch per level.
static int mm_run_levels(MmPlanState &s, DpConst c, const std::vector<unsigned long long> &finals, uint8_t *d_mark0, uint8_t *d_mark1,
                         uint32_t *d_modes, unsigned long long *d_sweeps, hipStream_t st, std::string &err) {
    DpState &dp = s.dp;
    dp.release();
    const double t0 = bg_now();
    const size_t n = (size_t)c.n;
    if (dp.dist_cap < n) {
        if (dp.d_dist) (void)hipFree(dp.d_dist);
        dp.d_dist = nullptr; dp.dist_cap = 0;
        DP_HIP(hipMalloc((void **)&dp.d_dist, (n + n / 8 + 1) * sizeof(double)));
        dp.dist_cap = n + n / 8 + 1;
    }
    if (!dp.d_flags) DP_HIP(hipMalloc((void **)&dp.d_flags, (1 + kDpGroup) * sizeof(uint32_t)));
    if (dp.finals_cap < finals.size() + 1) {
        if (dp.d_finals) (void)hipFree(dp.d_finals);
        dp.d_finals = nullptr; dp.finals_cap = 0;
        DP_HIP(hipMalloc((void **)&dp.d_finals, (finals.size() + 1) * 2 * sizeof(unsigned long long)));
        dp.finals_cap = (finals.size() + 1) * 2;
    }
    c.dist = dp.d_dist;
    c.flags = dp.d_flags;
    // levels: modes by number of possible worlds, mode order inside a level
    std::vector<uint32_t> order(s.n_modes);
    for (uint32_t m = 0; m < s.n_modes; ++m) order[m] = m;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return s.support[a] < s.support[b]; });
    std::vector<std::pair<uint32_t, uint32_t>> levels;
    for (size_t i = 0; i < order.size();) {
        size_t j = i;
        while (j < order.size() && s.support[order[j]] == s.support[order[i]]) ++j;
        levels.push_back({(uint32_t)i, (uint32_t)j});
        i = j;
    }
    ScopedEvents<2> evs;
    DP_HIP(evs.create());
    DP_HIP(hipEventRecord(evs.e[0], st));
    DP_HIP(hipMemcpyAsync(d_modes, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    DP_HIP(hipMemsetAsync(dp.d_flags, 0, (1 + kDpGroup) * sizeof(uint32_t), st));
    DP_HIP(hipMemsetAsync(d_sweeps, 0, 2 * sizeof(unsigned long long) + sizeof(uint32_t), st));
    const dim3 block(256);
    hipLaunchKernelGGL(k_dp_fill, dim3((unsigned)((n + 255) / 256)), block, 0, st, dp.d_dist, (unsigned long long)n, __builtin_huge_val());
    if (!finals.empty()) {
        DP_HIP(hipMemcpyAsync(dp.d_finals, finals.data(), finals.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_dp_set_finals, dim3((unsigned)((finals.size() + 255) / 256)), block, 0, st, c, (const unsigned long long *)dp.d_finals,
                           (unsigned long long)finals.size(), d_mark0);
    }
    MmLevelConst L{};
    L.g = c; L.mode_off = s.d_mode_off; L.lds_cap = s.lds_cap; L.mark[0] = d_mark0; L.mark[1] = d_mark1;
    L.sweeps = d_sweeps; L.err = (uint32_t *)(d_sweeps + 2);
    uint32_t launches = 0;
    for (const auto &lv : levels) {
        bool fits = false;
        for (uint32_t k = lv.first; k < lv.second && !fits; ++k) fits = s.mode_off[order[k] + 1] - s.mode_off[order[k]] <= s.lds_cap;
        L.modes = d_modes + lv.first;
        hipLaunchKernelGGL(k_mm_level, dim3(lv.second - lv.first), block, fits ? (size_t)s.lds_cap * 10 : 0, st, L);
        ++launches;
    }
    DP_HIP(hipEventRecord(evs.e[1], st));
    unsigned long long h[3] = {0, 0, 0};
    uint32_t h_flag = 0;
    DP_HIP(hipMemcpyAsync(h, d_sweeps, 2 * sizeof(unsigned long long) + sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DP_HIP(hipMemcpyAsync(&h_flag, dp.d_flags, sizeof h_flag, hipMemcpyDeviceToHost, st));
    DP_HIP(hipStreamSynchronize(st));
    DP_HIP(hipGetLastError());
    const uint32_t merr = (uint32_t)(h[2] & 0xFFFFFFFFull);
    if (h_flag & DP_ERR_ZERO_PROBABILITY) { err = "assert!(p > 0.0) failed (belief_graph.rs:128)"; return PORRT_ERR_INVALID; }
    if (merr & MM_ERR_LEAVES_MODE) { err = "expected costs: an action edge leaves its mode"; return PORRT_ERR_DEVICE; }
    if (merr & MM_ERR_NO_FIXPOINT) { err = "conditional_dijkstra: no fixpoint after 4M sweeps of a mode"; return PORRT_ERR_DEVICE; }
    float ms = 0;
    DP_HIP(hipEventElapsedTime(&ms, evs.e[0], evs.e[1]));
    s.levels = (uint32_t)levels.size();
    s.launches = launches;
    s.level_sweeps = h[0];
    s.max_mode_sweeps = h[1];
    dp.n = n;
    dp.last = c;
    dp.layered = true;
    dp.sweeps = (uint32_t)h[1];
    dp.sweep_rows = 0;
    dp.t_device = 1e-3 * (double)ms;
    dp.t_total = bg_now() - t0;
    dp.valid = true;
    return PORRT_OK;
}

} // namespace porrt
