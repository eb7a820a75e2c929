// porrt_policy.hpp -- extract_policy (src/belief_graph.rs:184-267) from many start belief nodes, walked on the device: one
// wave per query, one call for all of them (porrt_bg_extract_policies, porrt_mm_extract_policies, porrt_extract_policies).  The
// single extraction from belief node 0 (porrt_bg_extract_policy, porrt_mm_extract_policy) is a call with that one start.
//
// The expected costs the sweeps of porrt_dp.hpp leave on the device are costs-to-goal of EVERY belief node, so the policy
// from any of them is determined; nothing in the reference's walk needs the host.  Per popped (policy node, belief node):
//   * the children are clustered by belief id, clusters in ascending id order (the BTreeMap): found here by repeated
//     "least (belief id, position in the row) above the last id" reductions over the row;
//   * within a cluster p = transition_probability(node, the cluster's FIRST child) (common.rs:187-190, summed in world
//     order) and the winner is the first child in children order of strictly least p * (norm2 + dist[child]), starting
//     from (+inf, first child): a reduction on (cost, position) over the children whose cost is below +inf -- a cluster
//     of +inf / NaN costs keeps its first child;
//   * winners become policy nodes in cluster order; the non-leaf ones are pushed, the last pushed is expanded first.
// The LIFO only ever holds policy nodes already written: it is a chain through the nodes (`next`).  The walk is depth
// first, so the belief nodes on the way from the root to a node popped at depth d are path[0 .. d): the reference has no
// memory and never ends once its best child leads back onto that path; here that is status 2, found by a lane-parallel
// scan of `path`.
//
// Sizing: a pooled single pass.  Every query of a launch owns a slice of one pool (policy nodes and path); a policy that
// outgrows its slice is walked again in a later launch with a slice 16 times as long, up to option "policy_max_nodes"
// (then: status 4).  A finished launch's policies are packed on the device (k_pol_pack) and fetched in one copy.
#pragma once
#include "porrt_dp.hpp"

namespace porrt {

enum : uint32_t { POL_OK = 0, POL_NO_COST = 1, POL_OWN_PATH = 2, POL_ASSERT = 3, POL_CAPACITY = 4, POL_SLICE = 255 /* internal: walk again with a longer slice */ };

constexpr uint32_t kPolNone = 0xFFFFFFFFu;
constexpr uint32_t kPolRowCache = 512;                // children of the popped node kept in LDS (12 KiB per wave); longer rows read the rest again
constexpr uint32_t kPolRowMax = 65535;                // a longer row is status 4 (the limit of the single extraction)
constexpr uint64_t kPolPoolNodes = 1ull << 22;        // policy nodes of one launch, all queries together
constexpr uint32_t kPolMinSlice = 64;
constexpr uint64_t kPolMaxNodesLimit = 1ull << 24;

struct PolNode {
    uint32_t original;                                // belief node
    uint32_t parent;                                  // policy node, kPolNone for the root
    uint32_t next;                                    // the LIFO: the policy node below this one
    uint32_t depth_leaf;                              // depth | is_leaf << 31
};
struct PolQuery { unsigned long long start, base; uint32_t cap, pad; };    // slice [base, base + cap) of the pool
struct PolAnswer { double cost; uint32_t count, status; };

__device__ __forceinline__ unsigned long long pol_wave_min(unsigned long long v) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
        const unsigned long long o = (unsigned long long)hi << 32 | lo;
        v = o < v ? o : v;
    }
    return v;
}

// One wave (= one workgroup) per query.  Everything that steers the walk (top, count, status) is wave-uniform.
template <bool IMPLICIT>
__global__ __launch_bounds__(64) void k_pol_walk(DpConst g, const uint32_t *__restrict__ bid, const PolQuery *__restrict__ qs, uint32_t nq, uint32_t max_nodes,
                                                 PolNode *pool, uint32_t *path_pool, PolAnswer *__restrict__ ans) {
    __shared__ uint32_t s_child[kPolRowCache], s_key[kPolRowCache];
    __shared__ double s_term[kPolRowCache], s_dist[kPolRowCache];
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    if (q >= nq) return;
    const PolQuery Q = qs[q];
    PolNode *nodes = pool + Q.base;
    uint32_t *path = path_pool + Q.base;
    const double d_start = as_global(g.dist)[Q.start];
    uint32_t status = POL_OK, count = 0, top = kPolNone;
    if (!(d_start - d_start == 0.0)) status = POL_NO_COST;            // +-inf, NaN
    else if (Q.cap == 0) status = POL_SLICE;
    else {
        if (lane == 0) { PolNode r; r.original = (uint32_t)Q.start; r.parent = kPolNone; r.next = kPolNone; r.depth_leaf = 0; nodes[0] = r; }
        count = 1; top = 0;
    }
    __syncthreads();
    // what the lanes need of child j of the popped node
    struct Child { uint32_t id, key; double term, dist; };
    while (top != kPolNone && status == POL_OK) {                     // every turn pops a node written once: at most cap turns
        const PolNode nd = nodes[top];
        const uint32_t k = top, bn = nd.original, depth = nd.depth_leaf & 0x7FFFFFFFu;
        top = nd.next;
        bool on_path = false;
        for (uint32_t j = lane; j < depth; j += 64) on_path |= path[j] == bn;
        if (__any(on_path)) { status = POL_OWN_PATH; break; }
        if (lane == 0) path[depth] = bn;                              // depth < count <= cap
        const unsigned long long c0 = as_global(g.child_off)[bn], c1 = as_global(g.child_off)[bn + 1];
        if (c1 - c0 > kPolRowMax) { status = POL_CAPACITY; break; }
        const uint32_t cnt = (uint32_t)(c1 - c0);
        double ux, uy;
        uint32_t urow;
        dp_state<IMPLICIT>(g, bn, ux, uy, urow);
        const double dist_bn = as_global(g.dist)[bn];
        auto load = [&](uint32_t j) {
            Child c;
            c.id = as_global(g.child_id)[c0 + j];
            double vx, vy;
            uint32_t vrow;
            dp_state<IMPLICIT>(g, c.id, vx, vy, vrow);
            c.key = IMPLICIT ? vrow : as_global(bid)[c.id];
            c.dist = as_global(g.dist)[c.id];
            c.term = sqrt(dist2(ux, uy, vx, vy)) + c.dist;            // norm2(node, child) + dist[child]
            return c;
        };
        auto key_of = [&](uint32_t j) { return j < kPolRowCache ? s_key[j] : load(j).key; };
        for (uint32_t j = lane; j < cnt && j < kPolRowCache; j += 64) {
            const Child c = load(j);
            s_child[j] = c.id; s_key[j] = c.key; s_term[j] = c.term; s_dist[j] = c.dist;
        }
        __syncthreads();
        long long last = -1;
        for (uint32_t turn = 0; turn < cnt; ++turn) {                 // at most one cluster per child
            unsigned long long m = ~0ull;                             // least (belief id, position) above the last id
            for (uint32_t j = lane; j < cnt; j += 64) {
                const uint32_t key = key_of(j);
                const unsigned long long cand = (unsigned long long)key << 32 | j;
                if ((long long)key > last && cand < m) m = cand;
            }
            m = pol_wave_min(m);
            if (m == ~0ull) break;
            const uint32_t key = (uint32_t)(m >> 32), first = (uint32_t)m;
            last = (long long)key;
            const uint32_t first_id = first < kPolRowCache ? s_child[first] : load(first).id;
            const uint32_t vrow = IMPLICIT ? key : as_global(g.bvec)[first_id];
            double p = 0.0;                                           // transition_probability (common.rs:187-190)
            for (uint32_t w = 0; w < g.nw; ++w)
                p = p + (as_global(g.beliefs)[(size_t)vrow * g.nw + w] > 0.0 ? as_global(g.beliefs)[(size_t)urow * g.nw + w] : 0.0);
            double bc = __builtin_huge_val();
            uint32_t bp = kPolNone;
            for (uint32_t j = lane; j < cnt; j += 64) {
                if (key_of(j) != key) continue;
                const double c = p * (j < kPolRowCache ? s_term[j] : load(j).term);
                if (c < bc) { bc = c; bp = j; }                       // strictly less: the lane keeps its earliest minimum
            }
            wave_first_min(bc, bp);                                   // (cost, position): the first minimum of the row wins
            const uint32_t win = bp == kPolNone ? first : bp;         // nothing below +inf: best_id stays the first child
            uint32_t win_id;
            double win_dist;
            if (win < kPolRowCache) { win_id = s_child[win]; win_dist = s_dist[win]; }
            else { const Child c = load(win); win_id = c.id; win_dist = c.dist; }
            if (!(p > 0.0)) { status = POL_ASSERT; break; }           // assert!(p > 0.0) (:250)
            if (!(p * win_dist <= dist_bn)) { status = POL_ASSERT; break; }     // (:261)
            if (count >= max_nodes) { status = POL_CAPACITY; break; }
            if (count >= Q.cap) { status = POL_SLICE; break; }
            const bool leaf = win_dist == 0.0;
            if (lane == 0) {
                PolNode o;
                o.original = win_id; o.parent = k; o.next = leaf ? kPolNone : top; o.depth_leaf = (depth + 1u) | (leaf ? 0x80000000u : 0u);
                nodes[count] = o;
            }
            if (!leaf) top = count;
            ++count;
        }
        __syncthreads();
    }
    if (lane == 0) {
        PolAnswer a;
        a.cost = d_start; a.status = status; a.count = status == POL_OK ? count : 0u;
        ans[q] = a;
    }
}

// the policies of a launch's finished queries, packed: query i's nodes to rows off[i] .. off[i] + count
__global__ __launch_bounds__(256) void k_pol_pack(const PolQuery *__restrict__ qs, const PolAnswer *__restrict__ ans, const unsigned long long *__restrict__ off,
                                                  uint32_t nq, const PolNode *__restrict__ pool, uint32_t *__restrict__ original, int32_t *__restrict__ parent,
                                                  uint8_t *__restrict__ leaf) {
    const uint32_t q = blockIdx.x;
    if (q >= nq) return;
    const uint32_t count = as_global(ans)[q].count;
    const unsigned long long base = as_global(qs)[q].base, o = as_global(off)[q];
    for (uint32_t j = threadIdx.x; j < count; j += blockDim.x) {
        const PolNode nd = pool[base + j];
        original[o + j] = nd.original;
        parent[o + j] = nd.parent == kPolNone ? -1 : (int32_t)nd.parent;
        leaf[o + j] = (uint8_t)(nd.depth_leaf >> 31);
    }
}

// ------------------------------------------------------------------------------------------------ host side

struct PoliciesResult {
    bool valid = false;
    uint64_t tag = ~0ull, stamp = ~0ull;              // what the graph and costs were when the call ran (the getters' staleness test)
    std::vector<uint64_t> off;                        // [queries + 1]
    std::vector<uint8_t> status;
    std::vector<double> cost;
    std::vector<uint64_t> original;
    std::vector<int64_t> parent;
    std::vector<uint8_t> leaf;
    std::vector<double> xy;                           // multi-modal graph only
    struct porrt_policies_info info = {};
};

static const char *const kPolStatusText[5] = {"", "its expected cost is not finite: no policy from there",
                                              "the walk returns to a belief node on its own path (zero-cost edges between nodes at one place); the reference does not terminate here",
                                              "an assertion of the reference fails (p > 0.0, belief_graph.rs:250, or p * dist[best] <= dist[node], :261)",
                                              "the policy exceeds policy_max_nodes, or a belief node has more than 65535 children"};

// Walks the policies from starts[0 .. n) on the graph and costs of c (c.dist set; bid = clustering key per node, explicit layout only).
// Slots 0-7 of sc are used.  first_slice: the slice of the first round (0 = the pool shared out among the queries).
// Fills everything of out but tag / stamp / xy / valid.
static int pol_extract(GrowScratch &sc, const DpConst &c, bool implicit, const uint32_t *d_bid, const uint64_t *starts, uint64_t n, uint64_t max_nodes,
                       uint64_t first_slice, hipStream_t s, PoliciesResult &out, std::string &err) {
    const double t0 = bg_now();
    out.valid = false;
    out.off.assign(n + 1, 0); out.status.assign(n, 0); out.cost.assign(n, 0.0);
    out.original.clear(); out.parent.clear(); out.leaf.clear(); out.xy.clear();
    out.info = {};
    out.info.queries = n;
    if (n >= (1ull << 31)) { err = "extract_policies: fewer than 2^31 queries"; return PORRT_ERR_INVALID; }
    for (uint64_t q = 0; q < n; ++q)
        if (starts[q] >= c.n) { err = "extract_policies: start " + std::to_string(q) + " is no belief node of the graph"; return PORRT_ERR_INVALID; }
    ScopedEvents<4> evs;
    DP_HIP(evs.create());
    double ms_device = 0.0;
    std::vector<uint64_t> pending(n), again;
    for (uint64_t q = 0; q < n; ++q) pending[q] = q;
    // per query: where its nodes sit in the launch-by-launch staging arrays
    std::vector<uint64_t> at(n, 0), count(n, 0);
    std::vector<uint32_t> st_original;
    std::vector<int32_t> st_parent;
    std::vector<uint8_t> st_leaf;
    std::vector<PolQuery> hq;
    std::vector<PolAnswer> ha;
    std::vector<unsigned long long> hoff;
    uint64_t slice = 0;
    while (!pending.empty()) {
        // slice of this round: first_slice or the pool shared out, at least kPolMinSlice; 16 times the last round's; never above max_nodes
        const uint64_t share = first_slice ? first_slice : kPolPoolNodes / pending.size();
        uint64_t want = slice ? slice * 16 : (share > kPolMinSlice ? share : kPolMinSlice);
        if (want > max_nodes) want = max_nodes;
        slice = want;
        const uint64_t per_launch = kPolPoolNodes / slice ? kPolPoolNodes / slice : 1;
        again.clear();
        for (uint64_t b0 = 0; b0 < pending.size(); b0 += per_launch) {
            const uint64_t nb = std::min<uint64_t>(per_launch, pending.size() - b0), pool_nodes = nb * slice;
            PolNode *d_pool = nullptr;
            uint32_t *d_path = nullptr, *d_original = nullptr;
            int32_t *d_parent = nullptr;
            uint8_t *d_leaf = nullptr;
            PolQuery *d_q = nullptr;
            PolAnswer *d_a = nullptr;
            unsigned long long *d_off = nullptr;
            if (sc.get(0, d_pool, pool_nodes) != hipSuccess || sc.get(1, d_path, pool_nodes) != hipSuccess || sc.get(2, d_original, pool_nodes) != hipSuccess ||
                sc.get(3, d_parent, pool_nodes) != hipSuccess || sc.get(4, d_leaf, pool_nodes) != hipSuccess || sc.get(5, d_q, nb) != hipSuccess ||
                sc.get(6, d_a, nb) != hipSuccess || sc.get(7, d_off, nb) != hipSuccess) {
                (void)hipGetLastError();
                err = "extract_policies: cannot allocate the pool of policy nodes";
                return PORRT_ERR_CAPACITY;
            }
            hq.resize(nb); ha.resize(nb); hoff.resize(nb);
            for (uint64_t i = 0; i < nb; ++i) { hq[i].start = starts[pending[b0 + i]]; hq[i].base = i * slice; hq[i].cap = (uint32_t)slice; hq[i].pad = 0; }
            DP_HIP(hipMemcpyAsync(d_q, hq.data(), nb * sizeof(PolQuery), hipMemcpyHostToDevice, s));
            DP_HIP(hipEventRecord(evs.e[0], s));
            if (implicit) hipLaunchKernelGGL(k_pol_walk<true>, dim3((unsigned)nb), dim3(64), 0, s, c, d_bid, (const PolQuery *)d_q, (uint32_t)nb, (uint32_t)max_nodes, d_pool, d_path, d_a);
            else hipLaunchKernelGGL(k_pol_walk<false>, dim3((unsigned)nb), dim3(64), 0, s, c, d_bid, (const PolQuery *)d_q, (uint32_t)nb, (uint32_t)max_nodes, d_pool, d_path, d_a);
            DP_HIP(hipEventRecord(evs.e[1], s));
            DP_HIP(hipMemcpyAsync(ha.data(), d_a, nb * sizeof(PolAnswer), hipMemcpyDeviceToHost, s));
            DP_HIP(hipStreamSynchronize(s));
            DP_HIP(hipGetLastError());
            unsigned long long total = 0;
            for (uint64_t i = 0; i < nb; ++i) {
                const uint64_t q = pending[b0 + i];
                hoff[i] = total;
                out.cost[q] = ha[i].cost;
                if (ha[i].status == POL_SLICE) {
                    if (slice < max_nodes) { again.push_back(q); ha[i].count = 0; continue; }
                    ha[i].status = POL_CAPACITY;                      // (not reached: max_nodes is tested first)
                }
                out.status[q] = (uint8_t)ha[i].status;
                count[q] = ha[i].status == POL_OK ? ha[i].count : 0;
                at[q] = st_original.size() + total;
                total += count[q];
            }
            float ms = 0;
            DP_HIP(hipEventElapsedTime(&ms, evs.e[0], evs.e[1]));
            ms_device += (double)ms;
            if (total) {
                const size_t old = st_original.size();
                st_original.resize(old + total); st_parent.resize(old + total); st_leaf.resize(old + total);
                // (a query to be walked again packs nothing: its count on the device is 0 -- status 255 -- too)
                DP_HIP(hipMemcpyAsync(d_off, hoff.data(), nb * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
                DP_HIP(hipEventRecord(evs.e[2], s));
                hipLaunchKernelGGL(k_pol_pack, dim3((unsigned)nb), dim3(256), 0, s, (const PolQuery *)d_q, (const PolAnswer *)d_a, (const unsigned long long *)d_off,
                                   (uint32_t)nb, (const PolNode *)d_pool, d_original, d_parent, d_leaf);
                DP_HIP(hipEventRecord(evs.e[3], s));
                DP_HIP(hipMemcpyAsync(st_original.data() + old, d_original, total * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
                DP_HIP(hipMemcpyAsync(st_parent.data() + old, d_parent, total * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                DP_HIP(hipMemcpyAsync(st_leaf.data() + old, d_leaf, total, hipMemcpyDeviceToHost, s));
                DP_HIP(hipStreamSynchronize(s));
                DP_HIP(hipGetLastError());
                DP_HIP(hipEventElapsedTime(&ms, evs.e[2], evs.e[3]));
                ms_device += (double)ms;
            }
        }
        pending.swap(again);
    }
    uint64_t total = 0, ok = 0, longest = 0;
    for (uint64_t q = 0; q < n; ++q) { out.off[q] = total; total += count[q]; ok += out.status[q] == POL_OK; longest = std::max(longest, count[q]); }
    out.off[n] = total;
    out.original.resize(total); out.parent.resize(total); out.leaf.resize(total);
    for (uint64_t q = 0; q < n; ++q)
        for (uint64_t j = 0; j < count[q]; ++j) {
            out.original[out.off[q] + j] = st_original[at[q] + j];
            out.parent[out.off[q] + j] = st_parent[at[q] + j];
            out.leaf[out.off[q] + j] = st_leaf[at[q] + j];
        }
    out.info.ok = ok; out.info.nodes = total; out.info.max_nodes = longest;
    out.info.ms_device = ms_device;
    out.info.ms_wall = 1e3 * (bg_now() - t0);
    for (uint64_t q = 0; q < n; ++q)
        if (out.status[q]) {
            err = "extract_policies: query " + std::to_string(q) + " (start " + std::to_string(starts[q]) + "), status " + std::to_string(out.status[q]) + ": " +
                  kPolStatusText[out.status[q] <= 4 ? out.status[q] : 4];
            break;
        }
    return PORRT_OK;
}

// The single extraction (PTO::extract_policy, pto.rs:277-283): the policy from belief node 0 as a batch of one, into a result of the
// caller's (one query; tag / stamp / xy / valid are the caller's to set).  Its limit is kPolMaxNodesLimit policy nodes; the first walk
// gets kPolSingleSlice of them (a lone query's share of the pool would be all of it), a longer policy is walked again as any query
// that outgrows its slice.
constexpr uint64_t kPolSingleSlice = 512;
static int pol_extract_root(GrowScratch &sc, const DpState &st, bool implicit, const uint32_t *d_bid, hipStream_t s, PoliciesResult &res, std::string &err) {
    const uint64_t root = 0;
    const int r = pol_extract(sc, st.last, implicit, d_bid, &root, 1, kPolMaxNodesLimit, kPolSingleSlice, s, res, err);
    if (r) return r;
    const uint32_t status = res.status[0];
    if (status) {
        err = std::string("extract_policy: ") + (status == POL_NO_COST    ? "no policy from the root (its expected cost is not finite; the reference does not terminate here)"
                                                 : status == POL_CAPACITY ? "more than 2^24 policy nodes, or a belief node with more than 65535 children"
                                                                          : kPolStatusText[status]);
        return status == POL_CAPACITY ? PORRT_ERR_CAPACITY : PORRT_ERR_INVALID;
    }
    err.clear();
    return PORRT_OK;
}

} // namespace porrt
