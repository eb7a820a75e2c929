// porrt_solutions.hpp -- RRT::get_solutions (src/rrt.rs:195-246) of many grown trees, on the device.
//
// The reference keeps, of a tree's final nodes F, the "firstly final" ones: from every f in F it moves up while the parent is in F
// (a missing parent reads as id 0, which is never in F: only added nodes are pushed, rrt.rs:165-167), so the set is exactly the
// final nodes whose parent is not final.  It returns the set in HashSet order; here it comes in ASCENDING NODE ID, one of the orders
// the reference may take.  Each solution is the path root .. node and its cost folded from 0.0 in path order (rrt.rs:223-227), the
// arithmetic of k_best_cost.
//
// Two launches, one workgroup of four waves per row (blockIdx.y = row of the batch's RunConst array, as k_best_cost):
//   k_solutions_select  counts the row's solutions, takes a block of the shared id arena (the one atomic: it places the row, it
//                       orders nothing inside it), compacts the ids in ascending order (64-bit ballot and popcount prefix inside a
//                       wave, wave offsets through LDS, a running base per stride), then one lane per solution walks to the root
//                       for its length.  Descriptor per row: count, states, status.
//   k_solutions_write   after the host has read the descriptors and sized the outputs (nothing is truncated): scans the lengths to
//                       offsets, one lane per solution writes its states root first and then sums the cost from the root outwards,
//                       reading what it wrote.  Rows land where the host put them: concatenated in the order of the argument.
#pragma once

#include <vector>

namespace {

enum : uint32_t { kSolOk = 0, kSolNone = 1, kSolGuard = 2, kSolArena = 3 };   // SolRow::status
constexpr uint32_t kSolThreads = 256, kSolWaves = kSolThreads / 64;

struct SolRow {
    unsigned long long n_states;
    uint32_t count, status, id_base, pad;
};
struct SolBase { unsigned long long sol, state; };      // where a row's solutions and states start in the outputs

__device__ __forceinline__ bool sol_first_final(const RunConst &rc, uint32_t f) {
    auto gff = as_global(rc.final_flag);
    if (!gff[f]) return false;
    const int p = as_global(rc.parent)[f];
    return !gff[p > 0 ? p : 0];                         // unwrap_or(0)
}

__global__ __launch_bounds__(256) void k_solutions_select(const RunConst *__restrict__ rcp, uint32_t nsteps, uint32_t row0, uint32_t *__restrict__ ids,
                                                          uint32_t *__restrict__ lens, uint32_t id_cap, uint32_t *__restrict__ cursor, SolRow *__restrict__ out) {
    const RunConst &rc = rcp[blockIdx.y];
    const uint32_t n_nodes = as_global(rc.n_at)[nsteps];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ uint32_t s_wave[kSolWaves], s_base, s_guard[kSolWaves];
    __shared__ unsigned long long s_sum[kSolWaves];
    // the row's count, then its block of the arena
    uint32_t cnt = 0;
    for (uint32_t f0 = 0; f0 < n_nodes; f0 += kSolThreads) {
        const uint32_t f = f0 + threadIdx.x;
        cnt += (uint32_t)__popcll(__ballot(f < n_nodes && sol_first_final(rc, f)));
    }
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    uint32_t total = 0;
    for (uint32_t w = 0; w < kSolWaves; ++w) total += s_wave[w];
    if (threadIdx.x == 0) s_base = total ? atomicAdd(cursor, total) : 0u;
    __syncthreads();
    const uint32_t base = s_base;
    if (total == 0 || (unsigned long long)base + total > id_cap) {
        if (threadIdx.x == 0) out[row0 + blockIdx.y] = SolRow{0ull, total, total ? kSolArena : kSolNone, base, 0u};
        return;
    }
    // ordered compaction
    uint32_t running = 0;
    for (uint32_t f0 = 0; f0 < n_nodes; f0 += kSolThreads) {
        const uint32_t f = f0 + threadIdx.x;
        const bool sel = f < n_nodes && sol_first_final(rc, f);
        const unsigned long long b = __ballot(sel);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < kSolWaves; ++w) { const uint32_t c = s_wave[w]; all += c; if (w < wave) before += c; }
        if (sel) ids[base + running + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = f;
        running += all;
        __syncthreads();
    }
    // lengths: one lane per solution
    auto gpar = as_global(rc.parent);
    unsigned long long sum = 0;
    uint32_t guard = 0;
    for (uint32_t j = threadIdx.x; j < total; j += kSolThreads) {
        uint32_t L = 0;
        for (int p = (int)ids[base + j]; p >= 0; p = gpar[p]) { ++L; if (L > n_nodes) break; }
        if (L > n_nodes) { guard = 1; L = 0; }
        lens[base + j] = L;
        sum += L;
    }
    for (uint32_t d = 32; d > 0; d >>= 1) { sum += __shfl_down(sum, d, 64); guard |= __shfl_down(guard, d, 64); }
    if (lane == 0) { s_sum[wave] = sum; s_guard[wave] = guard; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        uint32_t g = 0;
        for (uint32_t w = 0; w < kSolWaves; ++w) { s += s_sum[w]; g |= s_guard[w]; }
        out[row0 + blockIdx.y] = SolRow{s, total, g ? kSolGuard : kSolOk, base, 0u};
    }
}

__global__ __launch_bounds__(256) void k_solutions_write(const RunConst *__restrict__ rcp, uint32_t row0, const uint32_t *__restrict__ ids,
                                                         const uint32_t *__restrict__ lens, const SolRow *__restrict__ rows, const SolBase *__restrict__ bases,
                                                         unsigned long long *__restrict__ o_ids, unsigned long long *__restrict__ o_lens,
                                                         double *__restrict__ o_costs, double2 *o_xy) {
    const RunConst &rc = rcp[blockIdx.y];
    const SolRow r = rows[row0 + blockIdx.y];
    if (r.status != kSolOk) return;
    const SolBase at = bases[row0 + blockIdx.y];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ uint32_t s_wave[kSolWaves];
    auto gpar = as_global(rc.parent);
    auto gx = as_global(rc.nx), gy = as_global(rc.ny);
    unsigned long long running = 0;
    for (uint32_t j0 = 0; j0 < r.count; j0 += kSolThreads) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t L = j < r.count ? lens[r.id_base + j] : 0u;
        uint32_t incl = L;                               // inclusive scan of the wave's lengths
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < kSolWaves; ++w) { const uint32_t c = s_wave[w]; all += c; if (w < wave) before += c; }
        if (j < r.count) {
            const uint32_t f = ids[r.id_base + j];
            const unsigned long long off = at.state + running + before + (incl - L);
            uint32_t q = L;
            for (int p = (int)f; p >= 0 && q > 0; p = gpar[p]) o_xy[off + --q] = make_double2(gx[p], gy[p]);
            double sum = 0.0;
            for (uint32_t a = 0; a + 1 < L; ++a) {
                const double2 u = o_xy[off + a], v = o_xy[off + a + 1];
                sum += sqrt(dist2(u.x, u.y, v.x, v.y));
            }
            o_ids[at.sol + j] = f; o_lens[at.sol + j] = L; o_costs[at.sol + j] = sum;
        }
        running += all;
        __syncthreads();
    }
}

// one call's selection: the runs it was launched in, the rows' descriptors and where each row's output starts
struct SolGather {
    struct Run { const RunConst *rcp; uint32_t q0, rows, steps; };
    std::vector<Run> runs;
    std::vector<SolRow> rows;
    std::vector<SolBase> bases;
    uint64_t n_solutions = 0, n_states = 0;
    uint32_t *d_ids = nullptr, *d_lens = nullptr;
    SolRow *d_rows = nullptr;
};

// Launch 1 on every row of ctxs[0 .. n) and one small download.  A run of the argument (porrt_batch_run) gets one launch; other
// contexts go one by one.  Scratch: the kSlotSol* slots of the calling context's TampState.
static int solutions_select(porrt_ctx *c, TampState &T, porrt_ctx *const *ctxs, uint32_t n, SolGather &G) {
    HIPCHK_CTX(c, hipSetDevice(c->device));
    uint64_t id_cap = 0;
    for (uint32_t q = 0; q < n; ++q) {
        const porrt_ctx *x = ctxs[q];
        if (x->device != c->device) { c->set_err("solutions: contexts of one device"); return PORRT_ERR_INVALID; }
        if (!x->have_results || x->mm.valid || x->mode != PORRT_MODE_RRT) { c->set_err("solutions: a context without an RRT* tree (porrt_grow or porrt_grow_batch with PORRT_MODE_RRT first)"); return PORRT_ERR_INVALID; }
        id_cap += x->n_nodes;
    }
    if (id_cap >= (1ull << 31)) { c->set_err("solutions: more than 2^31 nodes in one call"); return PORRT_ERR_CAPACITY; }
    uint32_t *d_cur = nullptr;
    HIPCHK_CTX(c, T.scratch.get(kSlotSolIds, G.d_ids, id_cap));
    HIPCHK_CTX(c, T.scratch.get(kSlotSolLens, G.d_lens, id_cap));
    HIPCHK_CTX(c, T.scratch.get(kSlotSolRows, G.d_rows, n));
    HIPCHK_CTX(c, T.scratch.get(kSlotSolCursor, d_cur, 1));
    hipStream_t st = c->stream;
    HIPCHK_CTX(c, hipMemsetAsync(d_cur, 0, sizeof(uint32_t), st));
    G.runs.clear();
    for (uint32_t q0 = 0; q0 < n;) {
        const BatchRows B = porrt_batch_rows(ctxs, n, q0);
        const SolGather::Run R{B.rcp, q0, B.rows, B.steps};
        hipLaunchKernelGGL(k_solutions_select, dim3(1, R.rows), dim3(kSolThreads), 0, st, R.rcp, R.steps, R.q0, G.d_ids, G.d_lens, (uint32_t)id_cap, d_cur, G.d_rows);
        HIPCHK_CTX(c, hipGetLastError());
        G.runs.push_back(R);
        q0 += R.rows;
    }
    G.rows.resize(n);
    HIPCHK_CTX(c, hipMemcpyAsync(G.rows.data(), G.d_rows, n * sizeof(SolRow), hipMemcpyDeviceToHost, st));
    HIPCHK_CTX(c, hipStreamSynchronize(st));
    G.bases.resize(n);
    G.n_solutions = G.n_states = 0;
    for (uint32_t q = 0; q < n; ++q) {
        const SolRow &r = G.rows[q];
        if (r.status == kSolGuard) { c->set_err("solutions: a parent chain longer than the tree (row " + std::to_string(q) + ")"); return PORRT_ERR_DEVICE; }
        if (r.status == kSolArena) { c->set_err("solutions: the id arena was too small (row " + std::to_string(q) + ")"); return PORRT_ERR_CAPACITY; }
        G.bases[q] = SolBase{G.n_solutions, G.n_states};
        if (r.status == kSolOk) { G.n_solutions += r.count; G.n_states += r.n_states; }
    }
    return PORRT_OK;
}

// Launch 2 and the downloads: ids, lens, costs hold G.n_solutions entries, xy 2 * G.n_states doubles.
static int solutions_write(porrt_ctx *c, TampState &T, const SolGather &G, uint64_t *ids, uint64_t *lens, double *costs, double *xy) {
    if (!G.n_solutions) return PORRT_OK;
    const size_t n = G.rows.size();
    SolBase *d_bases = nullptr;
    unsigned long long *d_oi = nullptr;                  // ids | lens | costs, n_solutions each
    double2 *d_xy = nullptr;
    HIPCHK_CTX(c, T.scratch.get(kSlotSolBases, d_bases, n));
    HIPCHK_CTX(c, T.scratch.get(kSlotSolOut, d_oi, 3 * (size_t)G.n_solutions));
    HIPCHK_CTX(c, T.scratch.get(kSlotSolXy, d_xy, (size_t)G.n_states));
    unsigned long long *d_ol = d_oi + G.n_solutions;
    double *d_oc = (double *)(d_ol + G.n_solutions);
    hipStream_t st = c->stream;
    HIPCHK_CTX(c, hipMemcpyAsync(d_bases, G.bases.data(), n * sizeof(SolBase), hipMemcpyHostToDevice, st));
    for (const SolGather::Run &R : G.runs) {
        hipLaunchKernelGGL(k_solutions_write, dim3(1, R.rows), dim3(kSolThreads), 0, st, R.rcp, R.q0, (const uint32_t *)G.d_ids, (const uint32_t *)G.d_lens,
                           (const SolRow *)G.d_rows, (const SolBase *)d_bases, d_oi, d_ol, d_oc, d_xy);
        HIPCHK_CTX(c, hipGetLastError());
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t) && sizeof(double2) == 2 * sizeof(double), "output layouts");
    HIPCHK_CTX(c, hipMemcpyAsync(ids, d_oi, G.n_solutions * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_CTX(c, hipMemcpyAsync(lens, d_ol, G.n_solutions * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_CTX(c, hipMemcpyAsync(costs, d_oc, G.n_solutions * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_CTX(c, hipMemcpyAsync(xy, d_xy, G.n_states * 16, hipMemcpyDeviceToHost, st));
    HIPCHK_CTX(c, hipStreamSynchronize(st));
    return PORRT_OK;
}

} // namespace
