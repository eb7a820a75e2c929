// porrt_policy_graph.hpp -- get_policy_graph (src/pto_graph.rs:363-419) on the device: an edge u -> t of the PTO graph stays
// iff some belief exists under which t is at least as good as every other child of u.
//
// Per adjacency entry (u, t), over V = the worlds where t's QMDP cost is finite, with one row per rival o (a child of u whose id is
// not t's): d_o[w] = c_w[t] - c_w[o], 0 where c_w[o] is +inf.  Kept iff  v* = min over beliefs b on V of max_o d_o . b  <= 0.
//   how 0  V empty: pruned                               k_pg_classify
//   how 1  a world w with d_o[w] <= 0 for every rival: kept (b = e_w)
//   how 2  a rival with d_o[w] > 0 on all of V: pruned
//   how 3 / 4 / 5  kept / pruned / out of pivots (kept) by the simplex      k_pg_simplex
//
// The simplex walks vertices of {b >= 0, sum b = 1, d_o . b - v <= 0} downhill in v: |V| + 1 active constraints, one per slot,
// M = the inverse of their matrix ((|V|+1)^2 doubles in LDS), Bland's rule by constraint id (bound of the w-th world of V: w;
// rival at list position j: 64 + j).  Every sum over worlds is a serial loop in world order without contraction, and every
// choice among lanes is an exact minimum or maximum with the lower id on ties, so tests/policy_graph_ref.py repeats it bit for bit.
#pragma once
#include "../../include/porrt_hip.h"
#include "porrt_host.hpp"
#include "porrt_device.hpp"
#include <string>
#include <vector>

namespace porrt {

constexpr uint32_t kPgRival0 = 64;                       // constraint id of the rival at list position 0
constexpr uint8_t kPgPending = 255;                      // how of an entry that goes to the simplex
constexpr uint32_t kPgTileDoubles = 4096;                // cost rows of one LDS tile of k_pg_classify: 4096 / Wp rivals
constexpr uint32_t kPgBatch = 8;                         // entries a 16-lane group carries through the tiles at once
constexpr double kPgInf = __builtin_huge_val();

__host__ __device__ inline size_t pg_classify_lds(uint32_t Wp) {
    const size_t rows = kPgTileDoubles / Wp;
    return rows * (Wp + 1) * sizeof(double) + rows * sizeof(uint32_t);       // rows padded by one double: lanes on distinct banks
}
__host__ __device__ inline size_t pg_simplex_lds(uint32_t W) {
    const size_t k = W + 1;
    return (k * k + 3 * k + 64) * sizeof(double) + 2 * 64 * sizeof(uint32_t);          // M, b, p, u, c[t] on V; slot ids, worlds of V
}

// Steps 0-2.  One workgroup per node u; its children's cost rows pass through LDS in tiles; a 16-lane group carries kPgBatch
// entries at a time, its lanes striding the rivals of the tile.  Lane result per entry: the worlds where d <= 0 (ANDed over its
// rivals) and whether one of its rivals has d > 0 on all of V.
__global__ __launch_bounds__(256) void k_pg_classify(uint32_t W, uint32_t Wp, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ id,
                                                     const double *__restrict__ cost, uint8_t *__restrict__ how, uint32_t *__restrict__ piv,
                                                     unsigned long long *__restrict__ res_e, uint32_t *__restrict__ res_u, unsigned long long *n_res) {
    extern __shared__ __attribute__((aligned(16))) char pg_smem[];
    const uint32_t rows = kPgTileDoubles / Wp, stride = Wp + 1;
    double *tile = (double *)pg_smem;
    uint32_t *tile_id = (uint32_t *)(tile + (size_t)rows * stride);
    const uint32_t u = blockIdx.x, grp = threadIdx.x / 16u, l = threadIdx.x % 16u;
    const unsigned long long a0 = as_global(off)[u], deg = as_global(off)[u + 1] - a0;
    for (unsigned long long e0 = 0; e0 < deg; e0 += 16ull * kPgBatch) {
        unsigned long long le[kPgBatch], V[kPgBatch];
        uint32_t t[kPgBatch];
        bool dom[kPgBatch], live[kPgBatch];
#pragma unroll
        for (uint32_t i = 0; i < kPgBatch; ++i) {
            const unsigned long long e = e0 + grp + 16ull * i;
            live[i] = e < deg;
            t[i] = live[i] ? as_global(id)[a0 + e] : 0u;
            unsigned long long m = 0;
            if (live[i])
                for (uint32_t w = l; w < W; w += 16u)
                    if (as_global(cost)[(size_t)t[i] * Wp + w] != kPgInf) m |= 1ull << w;
            for (uint32_t o = 8; o; o >>= 1) m |= __shfl_xor(m, o, 16);
            V[i] = m;
            le[i] = ~0ull;
            dom[i] = false;
        }
        for (unsigned long long r0 = 0; r0 < deg; r0 += rows) {
            const uint32_t nr = (uint32_t)(deg - r0 < rows ? deg - r0 : rows);
            __syncthreads();
            for (uint32_t x = threadIdx.x; x < nr * Wp; x += 256u) {
                const uint32_t r = x / Wp, w = x % Wp;
                tile[(size_t)r * stride + w] = as_global(cost)[(size_t)as_global(id)[a0 + r0 + r] * Wp + w];
            }
            for (uint32_t r = threadIdx.x; r < nr; r += 256u) tile_id[r] = as_global(id)[a0 + r0 + r];
            __syncthreads();
#pragma unroll
            for (uint32_t i = 0; i < kPgBatch; ++i) {
                if (!live[i]) continue;
                const double *ct = cost + (size_t)t[i] * Wp;
                for (uint32_t r = l; r < nr; r += 16u) {
                    if (tile_id[r] == t[i]) continue;                        // other_edge.id != to_edge.id
                    const double *row = tile + (size_t)r * stride;
                    unsigned long long m = 0;
                    bool allpos = true;
                    for (uint32_t w = 0; w < W; ++w) {
                        if (!((V[i] >> w) & 1ull)) continue;
                        const double co = row[w];
                        if (co == kPgInf) { m |= 1ull << w; allpos = false; continue; }     // the reference leaves the term out: d = 0
                        const double d = as_global(ct)[w] - co;
                        if (d <= 0.0) m |= 1ull << w;
                        if (!(d > 0.0)) allpos = false;
                    }
                    le[i] &= m;
                    dom[i] = dom[i] || allpos;
                }
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < kPgBatch; ++i) {
            unsigned long long m = le[i];
            int d = dom[i] ? 1 : 0;
            for (uint32_t o = 8; o; o >>= 1) { m &= __shfl_xor(m, o, 16); d |= __shfl_xor(d, o, 16); }
            if (live[i] && l == 0) {
                const unsigned long long e = a0 + e0 + grp + 16ull * i;
                const uint8_t h = V[i] == 0 ? 0 : (m & V[i]) ? 1 : d ? 2 : kPgPending;
                how[e] = h;
                piv[e] = 0;
                if (h == kPgPending) {
                    const unsigned long long k = atomicAdd(n_res, 1ull);
                    res_e[k] = e;
                    res_u[k] = u;
                }
            }
        }
    }
}

__device__ __forceinline__ double pg_wave_max(double x) {
    for (uint32_t o = 32; o; o >>= 1) { const double y = __shfl_xor(x, o); x = y > x ? y : x; }
    return x;
}
__device__ __forceinline__ unsigned long long pg_wave_min(unsigned long long x) {
    for (uint32_t o = 32; o; o >>= 1) { const unsigned long long y = __shfl_xor(x, o); x = y < x ? y : x; }
    return x;
}

// Step 3.  One wave (one workgroup) per residual entry.
__global__ __launch_bounds__(64) void k_pg_simplex(uint32_t W, uint32_t Wp, uint32_t max_pivots, double tol, double eps,
                                                   const unsigned long long *__restrict__ off, const uint32_t *__restrict__ id,
                                                   const double *__restrict__ cost, const unsigned long long *__restrict__ res_e,
                                                   const uint32_t *__restrict__ res_u, uint8_t *__restrict__ how, uint32_t *__restrict__ piv) {
    extern __shared__ __attribute__((aligned(16))) char pg_smem[];
    const uint32_t lane = threadIdx.x;
    const unsigned long long e = as_global(res_e)[blockIdx.x];
    const uint32_t u = as_global(res_u)[blockIdx.x], t = as_global(id)[e];
    const unsigned long long a0 = as_global(off)[u];
    const uint32_t deg = (uint32_t)(as_global(off)[u + 1] - a0);
    // V, compacted in world order
    const double c_own = lane < W ? as_global(cost)[(size_t)t * Wp + lane] : kPgInf;
    const unsigned long long Vm = __ballot(c_own != kPgInf);
    const uint32_t n = (uint32_t)__popcll(Vm), k = n + 1;
    double *M = (double *)pg_smem, *b = M + (size_t)k * k, *p = b + k, *uu = p + k, *ct = uu + k;
    uint32_t *act = (uint32_t *)(ct + 64), *vw = act + 64;
    if (c_own != kPgInf) {
        const uint32_t cw = (uint32_t)__popcll(Vm & ((1ull << lane) - 1ull));
        vw[cw] = lane;
        ct[cw] = c_own;
    }
    for (uint32_t x = lane; x < k * k; x += 64u) M[x] = 0.0;
    __syncthreads();
    auto dval = [&](uint32_t o, uint32_t w) -> double {
        const double co = as_global(cost)[(size_t)o * Wp + vw[w]];
        return co == kPgInf ? 0.0 : ct[w] - co;
    };
    // scale = max |d|; the first rival with the greatest d in the first world of V
    double scale = 0.0, d00 = -kPgInf;
    uint32_t j0 = 0xFFFFFFFFu;
    for (uint32_t j = lane; j < deg; j += 64u) {
        const uint32_t o = as_global(id)[a0 + j];
        if (o == t) continue;
        for (uint32_t w = 0; w < n; ++w) {
            const double d = dval(o, w), a = fabs(d);
            scale = a > scale ? a : scale;
            if (w == 0 && d > d00) { d00 = d; j0 = j; }
        }
    }
    scale = pg_wave_max(scale);
    {
        const double best = pg_wave_max(d00);
        j0 = (uint32_t)pg_wave_min(d00 == best ? (unsigned long long)j0 : ~0ull);
        d00 = best;
    }
    const uint32_t o0 = as_global(id)[a0 + j0];
    if (lane == 0) { M[(size_t)n * k] = -1.0; M[n] = 1.0; M[(size_t)n * k + n] = d00; b[0] = 1.0; act[0] = kPgRival0 + j0; }
    else if (lane < n) {
        M[(size_t)lane * k + lane] = 1.0;
        M[lane] = -1.0;
        M[(size_t)n * k + lane] = dval(o0, lane) - d00;
        b[lane] = 0.0;
        act[lane] = lane;
    }
    __syncthreads();
    const double lim = tol * scale;
    double v = d00;
    uint32_t pivots = 0;
    uint8_t h;
    for (;;) {
        if (v <= lim) { h = 3; break; }
        // leaving slot: the lowest constraint id whose multiplier has the wrong sign
        unsigned long long key = ~0ull;
        if (lane < n) {
            const double lam = M[(size_t)n * k + lane];
            const uint32_t a = act[lane];
            if (a >= kPgRival0 ? lam > eps : lam < -(eps * scale)) key = ((unsigned long long)a << 32) | lane;
        }
        key = pg_wave_min(key);
        if (key == ~0ull) { h = 4; break; }                                  // an optimum with v > lim
        if (pivots >= max_pivots) { h = 5; break; }
        const uint32_t i = (uint32_t)key;
        const bool leaving_rival = (uint32_t)(key >> 32) >= kPgRival0;
        for (uint32_t w = lane; w < k; w += 64u) p[w] = leaving_rival ? -M[(size_t)w * k + i] : M[(size_t)w * k + i];
        __syncthreads();
        double pb1 = 0.0, pmax = 0.0;
        for (uint32_t w = 0; w < n; ++w) {
            const double a = fabs(p[w]);
            pb1 = pb1 + a;
            pmax = a > pmax ? a : pmax;
        }
        const double pn = p[n], g_lim = eps * (scale * pb1 + fabs(pn)), b_lim = -(eps * pmax);
        auto active = [&](uint32_t cid) -> bool {
            for (uint32_t s = 0; s < n; ++s) if (act[s] == cid) return true;
            return false;
        };
        // ratio test: the least step, the lowest id on ties
        double bt = kPgInf;
        uint32_t bid = 0xFFFFFFFFu;
        if (lane < n && p[lane] < b_lim && !active(lane)) {
            const double bw = b[lane];
            bt = (bw > 0.0 ? bw : 0.0) / -p[lane];
            bid = lane;
        }
        for (uint32_t j = lane; j < deg; j += 64u) {
            const uint32_t o = as_global(id)[a0 + j];
            if (o == t || active(kPgRival0 + j)) continue;
            double r = 0.0, g = 0.0;
            for (uint32_t w = 0; w < n; ++w) {
                const double d = dval(o, w);
                r = r + d * b[w];
                g = g + d * p[w];
            }
            r = r - v;
            g = g - pn;
            if (g > g_lim) {
                const double num = -r > 0.0 ? -r : 0.0, tt = num / g;
                if (tt < bt) { bt = tt; bid = kPgRival0 + j; }
            }
        }
        {
            // lexicographic minimum of (step, id): steps are >= 0, so their bit patterns order as integers
            double tm = bt;
            for (uint32_t o = 32; o; o >>= 1) { const double y = __shfl_xor(tm, o); tm = y < tm ? y : tm; }
            bid = (uint32_t)pg_wave_min(bt == tm ? (unsigned long long)bid : ~0ull);
            bt = tm;
        }
        if (bid == 0xFFFFFFFFu) { h = 5; break; }                            // nothing blocks (rounding): undecided, kept
        __syncthreads();
        if (lane < n) b[lane] = b[lane] + bt * p[lane];
        v = v + bt * pn;
        // the entering constraint against every slot's direction
        if (bid < kPgRival0) {
            for (uint32_t s = lane; s < k; s += 64u) uu[s] = M[(size_t)bid * k + s];
        } else {
            const uint32_t o = as_global(id)[a0 + (bid - kPgRival0)];
            for (uint32_t s = lane; s < k; s += 64u) {
                double acc = 0.0;
                for (uint32_t w = 0; w < n; ++w) acc = acc + dval(o, w) * M[(size_t)w * k + s];
                uu[s] = acc - M[(size_t)n * k + s];
            }
        }
        __syncthreads();
        const double pe = uu[i];
        for (uint32_t w = lane; w < k; w += 64u) p[w] = M[(size_t)w * k + i] / pe;
        __syncthreads();
        for (uint32_t x = lane; x < k * k; x += 64u) {
            const uint32_t w = x / k, s = x % k;
            M[x] = s == i ? p[w] : M[x] - p[w] * uu[s];
        }
        if (lane == 0) act[i] = bid;
        __syncthreads();
        if (lane < n && act[lane] < kPgRival0) b[act[lane]] = 0.0;             // an active bound holds exactly
        __syncthreads();
        ++pivots;
    }
    if (lane == 0) { how[e] = h; piv[e] = pivots; }
}

__device__ __forceinline__ bool pg_kept(uint8_t h) { return h == 1 || h == 3 || h == 5; }

// keep[e] from how[e]; pkeep[e] for entry j of parents[x] (= children[x] on a PTO graph: every edge goes both ways, pushed
// together): parent p survives iff the entry (p, x) survived (remove_edge, pto_graph.rs:214-217; every copy of (p, x) has one
// decision).  One wave per node x.
__global__ __launch_bounds__(256) void k_pg_flags(uint32_t N, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ id,
                                                  const uint8_t *__restrict__ how, uint8_t *__restrict__ keep, uint8_t *__restrict__ pkeep) {
    const uint32_t x = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (x >= N) return;
    const unsigned long long a0 = as_global(off)[x], a1 = as_global(off)[x + 1];
    for (unsigned long long e = a0 + lane; e < a1; e += 64u) {
        keep[e] = pg_kept(as_global(how)[e]) ? 1 : 0;
        if (pkeep) {
            const uint32_t p = as_global(id)[e];
            uint8_t f = 0;                                                   // (no entry (p, x): not a both-ways graph; the parent goes)
            for (unsigned long long q = as_global(off)[p], q1 = as_global(off)[p + 1]; q < q1; ++q)
                if (as_global(id)[q] == x) { f = pg_kept(as_global(how)[q]) ? 1 : 0; break; }
            pkeep[e] = f;
        }
    }
}

// Ordered compaction of a CSR by flags, as porrt_solutions' (count, prefix sum, ordered writes).  WRITE = false: cnt[x] = flagged
// entries of node x.  WRITE = true: they go to out_id[out_off[x] ..] in list order.  One wave per node.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_pg_compact(uint32_t N, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ id,
                                                    const uint8_t *__restrict__ flag, unsigned long long *__restrict__ cnt,
                                                    const unsigned long long *__restrict__ out_off, uint32_t *__restrict__ out_id) {
    const uint32_t x = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (x >= N) return;
    const unsigned long long a0 = as_global(off)[x], a1 = as_global(off)[x + 1];
    unsigned long long at = WRITE ? as_global(out_off)[x] : 0ull;
    for (unsigned long long e0 = a0; e0 < a1; e0 += 64u) {
        const unsigned long long e = e0 + lane;
        const bool f = e < a1 && as_global(flag)[e] != 0;
        const unsigned long long ballot = __ballot(f);
        if (WRITE && f) out_id[at + (unsigned long long)__popcll(ballot & ((1ull << lane) - 1ull))] = as_global(id)[e];
        at += (unsigned long long)__popcll(ballot);
    }
    if (!WRITE && lane == 0) cnt[x] = at;
}

// exclusive prefix sum of cnt[0 .. N) into out[0 .. N]: one workgroup, a contiguous chunk per thread
__global__ __launch_bounds__(256) void k_pg_scan(uint32_t N, const unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long part[256];
    const uint32_t chunk = (N + 255u) / 256u, x0 = threadIdx.x * chunk, x1 = x0 + chunk < N ? x0 + chunk : N;
    unsigned long long s = 0;
    for (uint32_t x = x0; x < x1; ++x) s += as_global(cnt)[x];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (uint32_t q = 0; q < 256u; ++q) { const unsigned long long c = part[q]; part[q] = run; run += c; }
        out[N] = run;
    }
    __syncthreads();
    s = part[threadIdx.x];
    for (uint32_t x = x0; x < x1; ++x) { out[x] = s; s += as_global(cnt)[x]; }
}

// ---- host side: the three passes on device arrays
struct PgDevice {
    uint32_t N, W, Wp;
    unsigned long long E;
    const unsigned long long *off;        // [N + 1]
    const uint32_t *id;                   // [E]
    const double *cost;                   // [N * Wp]
    uint8_t *how, *keep, *pkeep;          // [E]; pkeep may be null (no parents lists)
    uint32_t *piv;                        // [E]
    unsigned long long *res_e;            // [E]
    uint32_t *res_u;                      // [E]
    unsigned long long *n_res;            // [1]
    unsigned long long *cnt;              // [N]
    unsigned long long *c_off, *p_off;    // [N + 1]
    uint32_t *c_id, *p_id;                // [E]
};

// classify, simplex, compaction (children, and parents where d.pkeep is set); counts and times into info.  how and piv come back
// in h_how / h_piv.
static int pg_run(const PgDevice &d, uint32_t max_pivots, hipStream_t stream, std::vector<uint8_t> &h_how, std::vector<uint32_t> &h_piv,
                  struct porrt_policy_graph_info &info, std::string &err) {
    info = {};
    info.entries = d.E;
    h_how.assign(d.E, 0);
    h_piv.assign(d.E, 0);
    if (!d.N) return PORRT_OK;
    ScopedEvents<6> evs;
    HIPCHK_ERR(evs.create());
    double t0 = now_s();
    HIPCHK_ERR(hipMemsetAsync(d.n_res, 0, sizeof(unsigned long long), stream));
    HIPCHK_ERR(hipEventRecord(evs.e[0], stream));
    hipLaunchKernelGGL(k_pg_classify, dim3(d.N), dim3(256), pg_classify_lds(d.Wp), stream, d.W, d.Wp, d.off, d.id, d.cost, d.how, d.piv, d.res_e, d.res_u,
                       d.n_res);
    HIPCHK_ERR(hipEventRecord(evs.e[1], stream));
    unsigned long long n_res = 0;
    HIPCHK_ERR(hipMemcpyAsync(&n_res, d.n_res, sizeof n_res, hipMemcpyDeviceToHost, stream));
    HIPCHK_ERR(hipStreamSynchronize(stream));
    HIPCHK_ERR(hipGetLastError());
    info.ms_classify_wall = 1e3 * (now_s() - t0);
    t0 = now_s();
    HIPCHK_ERR(hipEventRecord(evs.e[2], stream));
    if (n_res) {
        if (n_res > 0x7FFFFFFFull) { err = "policy_graph: more than 2^31 - 1 entries for the simplex"; return (int)PORRT_ERR_CAPACITY; }
        hipLaunchKernelGGL(k_pg_simplex, dim3((unsigned)n_res), dim3(64), pg_simplex_lds(d.W), stream, d.W, d.Wp, max_pivots, (double)PORRT_POLICY_GRAPH_TOL,
                           (double)PORRT_POLICY_GRAPH_EPS, d.off, d.id, d.cost, (const unsigned long long *)d.res_e, (const uint32_t *)d.res_u, d.how, d.piv);
    }
    HIPCHK_ERR(hipEventRecord(evs.e[3], stream));
    HIPCHK_ERR(hipStreamSynchronize(stream));
    HIPCHK_ERR(hipGetLastError());
    info.ms_simplex_wall = 1e3 * (now_s() - t0);
    t0 = now_s();
    HIPCHK_ERR(hipEventRecord(evs.e[4], stream));
    const dim3 ngrid((d.N + 3u) / 4u);
    hipLaunchKernelGGL(k_pg_flags, ngrid, dim3(256), 0, stream, d.N, d.off, d.id, (const uint8_t *)d.how, d.keep, d.pkeep);
    for (int side = 0; side < (d.pkeep ? 2 : 1); ++side) {
        const uint8_t *flag = side ? d.pkeep : d.keep;
        unsigned long long *o_off = side ? d.p_off : d.c_off;
        uint32_t *o_id = side ? d.p_id : d.c_id;
        hipLaunchKernelGGL(k_pg_compact<false>, ngrid, dim3(256), 0, stream, d.N, d.off, d.id, flag, d.cnt, (const unsigned long long *)nullptr, (uint32_t *)nullptr);
        hipLaunchKernelGGL(k_pg_scan, dim3(1), dim3(256), 0, stream, d.N, (const unsigned long long *)d.cnt, o_off);
        hipLaunchKernelGGL(k_pg_compact<true>, ngrid, dim3(256), 0, stream, d.N, d.off, d.id, flag, (unsigned long long *)nullptr, (const unsigned long long *)o_off, o_id);
    }
    HIPCHK_ERR(hipEventRecord(evs.e[5], stream));
    if (d.E) {
        HIPCHK_ERR(hipMemcpyAsync(h_how.data(), d.how, d.E, hipMemcpyDeviceToHost, stream));
        HIPCHK_ERR(hipMemcpyAsync(h_piv.data(), d.piv, d.E * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    HIPCHK_ERR(hipStreamSynchronize(stream));
    HIPCHK_ERR(hipGetLastError());
    info.ms_compact_wall = 1e3 * (now_s() - t0);
    float ms = 0;
    HIPCHK_ERR(hipEventElapsedTime(&ms, evs.e[0], evs.e[1])); info.ms_classify_device = ms;
    HIPCHK_ERR(hipEventElapsedTime(&ms, evs.e[2], evs.e[3])); info.ms_simplex_device = ms;
    HIPCHK_ERR(hipEventElapsedTime(&ms, evs.e[4], evs.e[5])); info.ms_compact_device = ms;
    info.residual = n_res;
    for (unsigned long long e = 0; e < d.E; ++e) {
        const uint8_t h = h_how[e];
        if (h > 5) { err = "policy_graph: an entry was left undecided"; return (int)PORRT_ERR_DEVICE; }
        ++info.how[h];
        info.kept += (h == 1 || h == 3 || h == 5) ? 1 : 0;
        info.pivots_total += h_piv[e];
        info.pivots_max = h_piv[e] > info.pivots_max ? h_piv[e] : info.pivots_max;
    }
    return PORRT_OK;
}

// porrt_qmdp_policy_graph's result on a context (host copies; they belong to the graph and plan of `tag`)
struct PolicyGraphState {
    bool valid = false;
    uint64_t tag = 0;
    std::vector<uint8_t> keep, how;
    std::vector<uint64_t> child_off, parent_off;
    std::vector<uint32_t> child_ids, parent_ids;
    struct porrt_policy_graph_info info = {};
};

}  // namespace porrt
