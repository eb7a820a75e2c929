// porrt_mm_plan_batch.hpp -- MapShelfDomainTampPRM::plan (map_shelves_tamp_prm.rs:310-326) and PartialShortCut for many problems on
// one map in one call: many (start, prior, sampler seed, discrete seed) on the context's raster, zones and sampler box.
//
// A mode's roadmap depends on its ordered point list alone, and roadmaps_of_modes already lays the modes of ONE plan end to end (a
// per-node segment start, a segment table); the modes of many plans are more segments.  The mode-product belief graph has no edge
// between plans, the cost relaxation is monotone in f64, the policy walk from a plan's node 0 stays in the plan and the refiner
// treats each policy alone (the arguments of porrt_plan_batch.hpp), so a plan's answers on the union are bit for bit its answers alone.
//
// Host: grow_mm_prm's loop per plan, on up to 8 threads, RECORDING instead of drawing (porrt_mm_recipe.hpp): every mode clones the
// planner's never-advanced continuous sampler, so the k-th random point of any mode of plan p is P_p[k]; a mode is a list of codes
// (index into P_p, or one of the explicit points: start, goal states, observation samples and their copies), and P_p is drawn once.
// Device, per pass: k_mm_points expands the codes into the slots the roadmap pass reads (4 bytes a node go up instead of 16, plus
// the prefixes), mm_roadmaps_connect builds every roadmap and leaves the edges on the device, mm_build_belief_graph_device builds the
// belief graph of the union (transitions' mode ids and finals shifted by the plan's offsets on the host while they are laid end to
// end), the general sweeps, pol_extract from the plans' first nodes, the refiner with one belief row per union mode.
// A helper context owned by ctx carries the union: ctx's own growth, belief graph, costs, policy and samplers are not touched.
#pragma once
#include "porrt_mm_recipe.hpp"

namespace {

struct MmPointsConst {
    uint32_t NT, n_modes;
    const uint32_t *seg;                     // [n_modes + 1] first union node of every mode
    const uint32_t *codes;                   // [NT]
    const uint32_t *pref_off, *pref_len;     // [n_modes] the mode's plan: where its prefix starts in px / py, and its length
    const double *px, *py, *ex, *ey;
    uint32_t n_prefix, n_explicit;
    double *x, *y;
    uint32_t *base;
    uint32_t *err;
};

// One thread per union node: its mode by a search of the segment table, its code into a point.  Neighbouring nodes of a mode mostly
// name neighbouring prefix entries (a run of 190 random points), so the wave's loads of px / py are as contiguous as its stores.
// Every index is checked against its array before the load; a bad code sets the error bit and loads nothing.
__global__ __launch_bounds__(256) void k_mm_points(MmPointsConst g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.NT) return;
    const uint32_t up = mm_upper(g.seg, g.n_modes + 1, i);
    if (up == 0 || up > g.n_modes) { atomicOr(g.err, 1u); return; }
    const uint32_t m = up - 1;
    const uint32_t code = as_global(g.codes)[i];
    const uint32_t k = mm_code_index(code);
    double x = 0.0, y = 0.0;
    if (mm_code_is_explicit(code)) {
        if (k >= g.n_explicit) { atomicOr(g.err, 1u); return; }
        x = as_global(g.ex)[k]; y = as_global(g.ey)[k];
    } else {
        const uint32_t off = as_global(g.pref_off)[m], len = as_global(g.pref_len)[m];
        if (k >= len || (uint64_t)off + k >= g.n_prefix) { atomicOr(g.err, 1u); return; }
        x = as_global(g.px)[off + k]; y = as_global(g.py)[off + k];
    }
    g.x[i] = x; g.y[i] = y;
    g.base[i] = as_global(g.seg)[m];
}

// out[k] = a[idx[k]], out[n + k] = b[idx[k]]: the edge offsets at the plans' boundaries (the per-plan counts)
__global__ __launch_bounds__(256) void k_mm_gather2(const unsigned long long *a, const unsigned long long *b, const uint64_t *idx, uint32_t n, unsigned long long *out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    out[k] = as_global(a)[idx[k]];
    out[n + k] = as_global(b)[idx[k]];
}

// one plan's recorded mode tree
struct MmBatchMode {
    std::vector<double> belief;
    double reaching_probability = 0;
    std::vector<int> remaining;
    std::vector<int64_t> there, not_there;
    std::vector<uint64_t> finals;
    uint32_t bid = 0;
};
struct MmBatchPlan {
    MmRecipe rec;
    std::vector<MmBatchMode> modes;
    std::vector<MmTransition> tr;
    std::vector<double> px, py;              // P_p, to the largest random count of the plan's modes
    std::vector<uint32_t> mode_off;          // [modes + 1] the plan's own belief node ids
    uint64_t n_beliefs = 0, nodes = 0, n_pairs = 0, n_finals = 0;
    int r = PORRT_OK;
    std::string err;
};

// grow_mm_prm's loop (porrt_engine.hip) as a recorder: the discrete and the zone sampler are used exactly as there, no continuous draw
// is made per mode, and the plan's stream prefix is drawn once at the end.
void mm_batch_record(const porrt_ctx *c, const double start[2], const double *prior, uint32_t nw, uint64_t n_iter_per_belief, Pcg64 crng, Pcg64 drng,
                     MmBatchPlan &out) {
    using namespace mmprm;
    BeliefSpace bs;
    bs.domain = c->domain; bs.nz = c->n_zones; bs.nw = nw; bs.validities = c->validities;
    if ((out.r = bs.reach_from(prior, out.err))) return;
    out.n_beliefs = bs.size();
    MmRecipe &rec = out.rec;
    Pcg64 zone_sampler;
    zone_sampler.seed_from_u64(0);
    std::unordered_map<uint64_t, size_t> mode_hash_map;
    auto add_mode = [&](const std::vector<int> &remaining, double reach_p, const std::vector<double> &belief) {
        MmBatchMode m;
        mode_hash_map[BeliefSpace::hash_of(belief.data(), nw)] = out.modes.size();
        m.belief = belief; m.reaching_probability = reach_p; m.remaining = remaining;
        m.there.assign(64, -1); m.not_there.assign(64, -1);
        out.modes.push_back(std::move(m));
        rec.add_mode();
        return out.modes.size() - 1;
    };
    auto get_transitions = [&](size_t mode_id, int zone, size_t tids[2]) -> int {
        int n_out = 0;
        if (is_final(out.modes[mode_id].belief)) return 0;
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<int64_t> &map = pass == 0 ? out.modes[mode_id].there : out.modes[mode_id].not_there;
            if (map[zone] >= 0) { tids[n_out++] = (size_t)map[zone]; continue; }
            const MmBatchMode &mode = out.modes[mode_id];
            std::vector<double> sb;
            double reach_p;
            if (pass == 0) {
                sb.assign(nw, 0.0);
                sb[zone] = 1.0;
                normalize(sb);
                reach_p = mode.reaching_probability * transition_probability(mode.belief, sb);
            } else {
                sb = mode.belief;
                sb[zone] = 0.0;
                reach_p = mode.reaching_probability * transition_probability(mode.belief, sb);
                double sum = 0.0;
                for (double v : sb) sum = sum + v;
                if (!(sum > 0.0)) return -1;
                normalize(sb);
            }
            int64_t succ = -1;
            {
                const auto it = mode_hash_map.find(BeliefSpace::hash_of(sb.data(), nw));
                if (it != mode_hash_map.end()) succ = (int64_t)it->second;
            }
            if (succ < 0) {
                std::vector<int> remaining;
                for (int z : mode.remaining) if (z != zone) remaining.push_back(z);
                succ = (int64_t)add_mode(remaining, reach_p, sb);
                int goal_zone = -1;
                if (pass == 0) goal_zone = zone;
                else for (uint32_t w = 0; w < nw; ++w) if (sb[w] == 1.0) { goal_zone = (int)w; break; }
                if (goal_zone >= 0)
                    out.modes[succ].finals.push_back(rec.add_explicit_node((size_t)succ, rec.add_point(c->zone_pos[goal_zone][0], c->zone_pos[goal_zone][1])));
            }
            MmTransition t;
            t.zone = (uint32_t)zone; t.from = (uint32_t)mode_id; t.to = (uint32_t)succ; t.observation = 1;
            out.tr.push_back(std::move(t));
            (pass == 0 ? out.modes[mode_id].there : out.modes[mode_id].not_there)[zone] = (int64_t)out.tr.size() - 1;
            tids[n_out++] = out.tr.size() - 1;
        }
        return n_out;
    };
    {
        std::vector<int> remaining(c->n_zones);
        for (int z = 0; z < c->n_zones; ++z) remaining[z] = z;
        add_mode(remaining, 1.0, std::vector<double>(prior, prior + nw));
        rec.add_explicit_node(0, rec.add_point(start[0], start[1]));
    }
    const uint64_t total = n_iter_per_belief * out.n_beliefs;
    const uint64_t n_outer = (uint64_t)((double)total / 200.0);
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (uint64_t i = 0; i < n_outer; ++i) {
        const size_t mode_id = (size_t)drng.gen_range_usize(out.modes.size());
        for (int s = 0; s < 190; ++s) rec.add_random_node(mode_id);
        for (int j = 0; j < 10; ++j) {
            if (out.modes[mode_id].remaining.empty()) continue;
            const size_t zi = (size_t)drng.gen_range_usize(out.modes[mode_id].remaining.size());
            const int zone = out.modes[mode_id].remaining[zi];
            size_t tids[2];
            const int nt = get_transitions(mode_id, zone, tids);
            if (nt < 0) { out.err = "belief without mass (the reference asserts)"; out.r = PORRT_ERR_INVALID; return; }
            (void)zone_sampler.gen_range_f64(0.0, c->visibility);
            const double angle = zone_sampler.gen_range_f64(0.0, two_pi);
            double sn, cs;
            ::sincos(angle, &sn, &cs);
            double ts[2] = {c->zone_pos[zone][0] + c->visibility * cs, c->zone_pos[zone][1] + c->visibility * sn};
            for (int d = 0; d < 2; ++d) {
                const double lo = c->s_low[d], hi = c->s_up[d] - 0.0001;
                if (ts[d] < lo) ts[d] = lo;
                if (ts[d] > hi) ts[d] = hi;
            }
            const uint32_t point = rec.add_point(ts[0], ts[1]);       // the observation sample and its copies: one entry
            const uint64_t obs = rec.add_explicit_node(mode_id, point);
            for (int k = 0; k < nt; ++k) {
                MmTransition &t = out.tr[tids[k]];
                const uint64_t dst = rec.add_explicit_node(t.to, point);
                t.pairs.push_back(obs); t.pairs.push_back(dst);
            }
        }
        if (rec.overflow) { out.err = "more than 2^31 points in one plan"; out.r = PORRT_ERR_CAPACITY; return; }
    }
    // the plan's stream prefix, once (gen_range_f64's redraws included: they are part of the stream)
    const uint32_t L = rec.prefix_len();
    out.px.resize(L); out.py.resize(L);
    for (uint32_t k = 0; k < L; ++k) {
        out.px[k] = crng.gen_range_f64(c->s_low[0], c->s_up[0]);
        out.py[k] = crng.gen_range_f64(c->s_low[1], c->s_up[1]);
    }
    // the belief id of every mode (belief_states_to_id[hash(belief)], :400), the plan's own belief node ids, the counts
    out.mode_off.assign(out.modes.size() + 1, 0);
    uint64_t at = 0;
    for (size_t m = 0; m < out.modes.size(); ++m) {
        const auto f = bs.by_hash.find(BeliefSpace::hash_of(out.modes[m].belief.data(), nw));
        if (f == bs.by_hash.end()) { out.err = "a mode's belief is not a reachable belief state (the reference panics, :400)"; out.r = PORRT_ERR_INVALID; return; }
        out.modes[m].bid = f->second;
        out.mode_off[m] = (uint32_t)at;
        at += rec.modes[m].codes.size();
        if (at >= 0x7FFFFFFFull) { out.err = "more than 2^31 belief nodes"; out.r = PORRT_ERR_CAPACITY; return; }
        out.n_finals += out.modes[m].finals.size();
    }
    out.mode_off[out.modes.size()] = (uint32_t)at;
    out.nodes = at;
    for (const MmTransition &t : out.tr) out.n_pairs += t.pairs.size() / 2;
}

struct MmPlanBatchState {
    int device = 0;
    porrt_ctx *helper = nullptr;
    uint64_t helper_raster_gen = 0;
    GrowScratch scratch;                       // 0 a pass's inputs (one upload), 7 error word, 8 / 9 gather
    void *stage = nullptr;                     // pinned host memory the inputs of a pass are laid out in: one copy, off the runtime's pageable path
    size_t stage_cap = 0;
    hipError_t stage_reserve(size_t bytes) {
        if (bytes <= stage_cap) return hipSuccess;
        if (stage) (void)hipHostFree(stage);
        stage = nullptr; stage_cap = 0;
        const hipError_t e = hipHostMalloc(&stage, bytes + bytes / 8, hipHostMallocDefault);
        if (e == hipSuccess) stage_cap = bytes + bytes / 8;
        return e;
    }
    bool valid = false;
    // the last call's answers, all passes
    std::vector<uint64_t> off;
    std::vector<uint8_t> status, rstatus, leaf;
    std::vector<double> cost, rcost, xy;
    std::vector<uint64_t> original;
    std::vector<int64_t> parent;
    std::vector<porrt_mm_batch_plan> plans;
    // the last pass: its plans' costs stay on the helper
    uint32_t last_first = 0;
    std::vector<uint64_t> last_noff;
    struct porrt_mm_plan_batch_info info;
    MmPlanBatchState() { memset(&info, 0, sizeof info); }
    ~MmPlanBatchState() {
        if (helper) porrt_destroy(helper);
        (void)hipSetDevice(device);
        if (stage) (void)hipHostFree(stage);
        scratch.free_all();
    }
};

MmPlanBatchState &mm_plan_batch_state(porrt_ctx *c) {
    if (!c->mm_plan_batch) {
        MmPlanBatchState *t = new MmPlanBatchState();
        t->device = c->device;
        c->mm_plan_batch = std::shared_ptr<void>(t, [](void *q) { delete (MmPlanBatchState *)q; });
    }
    return *(MmPlanBatchState *)c->mm_plan_batch.get();
}

// One pass: plans ps[0 .. n) as one union on the helper, through every stage; the answers are appended to S.
int mm_plan_batch_pass(porrt_ctx *lead, MmPlanBatchState &S, const MmBatchPlan *ps, uint32_t n, uint32_t nw, double max_step, double search_radius,
                       uint64_t refine_iterations) {
    porrt_ctx *h = S.helper;
    auto fail = [&](int r) { lead->set_err("mm_plan_batch: " + h->err); return r == PORRT_ERR_DEVICE && h->err.find("hipMalloc") != std::string::npos ? (int)PORRT_ERR_CAPACITY : r; };
    auto dev_fail = [&](const char *what, hipError_t e) {
        lead->set_err(std::string("mm_plan_batch: ") + what + ": " + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? PORRT_ERR_CAPACITY : PORRT_ERR_DEVICE;
    };
#define MB_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return dev_fail(#expr, e_); } while (0)
    double t0 = now_s();
    // ---- the union's tables
    std::vector<uint64_t> noff(n + 1, 0);
    uint64_t M64 = 0, n_prefix = 0, n_explicit = 0, n_pairs = 0, n_tr = 0, n_finals = 0;
    size_t max_n = 0;
    for (uint32_t q = 0; q < n; ++q) {
        noff[q + 1] = noff[q] + ps[q].nodes;
        M64 += ps[q].modes.size(); n_prefix += ps[q].px.size(); n_explicit += ps[q].rec.ex.size(); n_pairs += ps[q].n_pairs; n_tr += ps[q].tr.size();
        n_finals += ps[q].n_finals;
    }
    const uint64_t NT = noff[n];
    if (NT + 1 >= 0x7FFFFFFFull || M64 >= 0x7FFFFFFFull || n_prefix >= 0xFFFFFFFFull || n_explicit >= kMmCodeIndexMask || n_pairs + NT >= 0xFFFFFFFFull || n_tr >= 0xFFFFFFFFull) {
        lead->set_err("mm_plan_batch: a plan is too large for one pass (2^31 nodes, 2^32 pairs)");
        return PORRT_ERR_CAPACITY;
    }
    const uint32_t M = (uint32_t)M64;
    // what goes up, laid out in the pinned stage: codes | prefix offset, prefix length per mode | segment table | prefixes | explicit points
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_codes = 0, o_poff = o_codes + up16(NT * 4), o_plen = o_poff + up16((size_t)M * 4), o_seg = o_plen + up16((size_t)M * 4),
                 o_px = o_seg + up16((size_t)(M + 1) * 4), o_py = o_px + up16(n_prefix * 8), o_ex = o_py + up16(n_prefix * 8), o_ey = o_ex + up16(n_explicit * 8),
                 stage_bytes = o_ey + up16(n_explicit * 8);
    MB_HIP(S.stage_reserve(stage_bytes));
    uint8_t *const stage = (uint8_t *)S.stage;
    uint32_t *const codes = (uint32_t *)(stage + o_codes), *const pref_off = (uint32_t *)(stage + o_poff), *const pref_len = (uint32_t *)(stage + o_plen),
                   *const seg = (uint32_t *)(stage + o_seg);
    double *const px = (double *)(stage + o_px), *const py = (double *)(stage + o_py), *const ex = (double *)(stage + o_ex), *const ey = (double *)(stage + o_ey);
    std::vector<uint32_t> tr_off(n_tr + 1, 0), tr_from(n_tr), tr_to(n_tr);
    std::vector<unsigned long long> pairs;
    pairs.reserve(2 * n_pairs);
    MmPlanState &s = h->mmp;
    h->mm.clear();
    ++h->mm.gen;
    s.release();
    h->mm.nw = nw;
    s.nw = nw; s.n_modes = M; s.NT = NT;
    s.mode_off.assign(M + 1, 0); s.mode_bid.assign(M, 0); s.support.assign(M, 0); s.beliefs.assign((size_t)M * nw, 0.0);
    s.finals.clear(); s.finals.reserve(n_finals);
    s.support_shrinks = true;
    s.use_levels = false;                                // the level schedule is not offered in the batch
    {
        uint32_t m0 = 0, t0i = 0;
        uint64_t p0 = 0, e0 = 0;
        for (uint32_t q = 0; q < n; ++q) {
            const MmBatchPlan &pl = ps[q];
            for (size_t m = 0; m < pl.modes.size(); ++m) {
                const uint32_t um = m0 + (uint32_t)m;
                const uint64_t first = noff[q] + pl.mode_off[m];
                const std::vector<uint32_t> &cd = pl.rec.modes[m].codes;
                seg[um] = (uint32_t)first;
                pref_off[um] = (uint32_t)p0; pref_len[um] = (uint32_t)pl.px.size();
                for (size_t t = 0; t < cd.size(); ++t) codes[first + t] = mm_code_is_explicit(cd[t]) ? mm_code_explicit((uint32_t)(e0 + mm_code_index(cd[t]))) : cd[t];
                max_n = std::max(max_n, cd.size());
                s.mode_bid[um] = pl.modes[m].bid;
                for (uint32_t w = 0; w < nw; ++w) { s.beliefs[(size_t)um * nw + w] = pl.modes[m].belief[w]; s.support[um] += pl.modes[m].belief[w] > 0.0 ? 1u : 0u; }
                for (uint64_t f : pl.modes[m].finals) s.finals.push_back(first + f);
            }
            for (size_t t = 0; t < pl.tr.size(); ++t) {
                const MmTransition &tr = pl.tr[t];
                tr_off[t0i + t] = (uint32_t)(pairs.size() / 2); tr_from[t0i + t] = m0 + tr.from; tr_to[t0i + t] = m0 + tr.to;
                pairs.insert(pairs.end(), tr.pairs.begin(), tr.pairs.end());
                if (!(s.support[m0 + tr.to] < s.support[m0 + tr.from])) s.support_shrinks = false;
            }
            std::copy(pl.px.begin(), pl.px.end(), px + p0); std::copy(pl.py.begin(), pl.py.end(), py + p0);
            std::copy(pl.rec.ex.begin(), pl.rec.ex.end(), ex + e0); std::copy(pl.rec.ey.begin(), pl.rec.ey.end(), ey + e0);
            m0 += (uint32_t)pl.modes.size(); t0i += (uint32_t)pl.tr.size(); p0 += pl.px.size(); e0 += pl.rec.ex.size();
        }
        seg[M] = (uint32_t)NT;
        tr_off[n_tr] = (uint32_t)(pairs.size() / 2);
        s.mode_off.assign(seg, seg + M + 1);
    }
    S.info.ms_host += 1e3 * (now_s() - t0);

    // ---- the points: codes, prefixes and explicit points up, k_mm_points into the roadmap pass's slots
    t0 = now_s();
    hipStream_t st = h->stream;
    MmRoadmapDev d{};
    int r = h->mm_roadmaps_prepare(NT, M, max_n, max_step, search_radius, d);
    if (r) return fail(r);
    MmPointsConst g{};
    uint8_t *d_in = nullptr;
    uint32_t *d_err = nullptr;
    MB_HIP(S.scratch.get(0, d_in, stage_bytes)); MB_HIP(S.scratch.get(7, d_err, 1));
    MB_HIP(hipMemcpyAsync(d_in, stage, stage_bytes, hipMemcpyHostToDevice, st));
    MB_HIP(hipMemsetAsync(d_err, 0, sizeof(uint32_t), st));
    S.info.upload_bytes += stage_bytes;
    d.seg = (uint32_t *)(d_in + o_seg);                      // the roadmap pass reads the segment table where it went up
    g.NT = (uint32_t)NT; g.n_modes = M; g.seg = d.seg; g.codes = (const uint32_t *)(d_in + o_codes); g.pref_off = (const uint32_t *)(d_in + o_poff);
    g.pref_len = (const uint32_t *)(d_in + o_plen); g.px = (const double *)(d_in + o_px); g.py = (const double *)(d_in + o_py);
    g.ex = (const double *)(d_in + o_ex); g.ey = (const double *)(d_in + o_ey); g.n_prefix = (uint32_t)n_prefix; g.n_explicit = (uint32_t)n_explicit;
    g.x = d.x; g.y = d.y; g.base = d.base; g.err = d_err;
    ScopedEvents<4> evs;
    MB_HIP(evs.create());
    MB_HIP(hipEventRecord(evs.e[2], st));
    hipLaunchKernelGGL(k_mm_points, dim3((unsigned)((NT + 255) / 256)), dim3(256), 0, st, g);
    MB_HIP(hipEventRecord(evs.e[3], st));
    S.info.ms_points += 1e3 * (now_s() - t0);

    // ---- every roadmap of the pass, the edges left on the device
    t0 = now_s();
    if ((r = h->mm_roadmaps_connect(d, NT, M, evs.e[0], evs.e[1]))) return fail(r);
    uint32_t h_err[2] = {0, 0};
    MB_HIP(hipMemcpyAsync(&h_err[0], d_err, 4, hipMemcpyDeviceToHost, st));
    MB_HIP(hipMemcpyAsync(&h_err[1], d.err, 4, hipMemcpyDeviceToHost, st));
    MB_HIP(hipStreamSynchronize(st));
    MB_HIP(hipGetLastError());
    if (h_err[0]) { lead->set_err("mm_plan_batch: a node's code names a point its plan does not have"); return PORRT_ERR_DEVICE; }
    if (h_err[1] & ERR_RASTER) {
        lead->set_err("mm_plan_batch: raster access the reference would panic on (image::get_pixel out of range, door pixel without zone, two zones on one segment)");
        return PORRT_ERR_RASTER;
    }
    {
        float ms = 0, ms2 = 0;
        MB_HIP(hipEventElapsedTime(&ms, evs.e[0], evs.e[1]));
        MB_HIP(hipEventElapsedTime(&ms2, evs.e[2], evs.e[3]));
        S.info.ms_device += (double)ms + (double)ms2;
    }
    h->have_results = false;
    h->mm.n_beliefs = 0;
    h->mm.valid = true;
    h->mm.dev_edges = true;
    S.info.ms_roadmaps += 1e3 * (now_s() - t0);

    // ---- the stages of a single plan, on the union
    t0 = now_s();
    if ((r = h->mm_build_belief_graph_device(tr_off, tr_from, tr_to, pairs, t0))) return fail(r);
    // the per-plan counts: forward edges and belief edges between the plans' boundaries
    std::vector<unsigned long long> bounds(2 * (size_t)(n + 1));
    {
        uint64_t *d_idx = nullptr;
        unsigned long long *d_out = nullptr;
        MB_HIP(S.scratch.get(8, d_idx, n + 1)); MB_HIP(S.scratch.get(9, d_out, 2 * (size_t)(n + 1)));
        MB_HIP(hipMemcpyAsync(d_idx, noff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mm_gather2, dim3((n + 1 + 255) / 256), dim3(256), 0, st, (const unsigned long long *)d.off, (const unsigned long long *)s.c.child_off,
                           (const uint64_t *)d_idx, n + 1, d_out);
        MB_HIP(hipMemcpyAsync(bounds.data(), d_out, bounds.size() * 8, hipMemcpyDeviceToHost, st));
        MB_HIP(hipStreamSynchronize(st));
    }
    S.info.ms_belief_graph += 1e3 * (now_s() - t0);
    S.info.ms_device += 1e3 * s.t_build_device;
    t0 = now_s();
    h->opt_dp_sweeps = lead->opt_dp_sweeps;
    if ((r = h->mm_compute_expected_costs())) return fail(r);
    S.info.ms_costs += 1e3 * (now_s() - t0);
    S.info.ms_device += 1e3 * s.dp.t_device;
    t0 = now_s();
    std::vector<uint64_t> starts(noff.begin(), noff.begin() + n);
    PoliciesResult &pol = h->mm_policies;
    {
        std::string e;
        if ((r = pol_extract(h->policies_scratch, s.dp.last, false, s.d_bid, starts.data(), n, h->opt_policy_max_nodes, 0, st, pol, e))) {
            lead->set_err("mm_plan_batch: " + e);
            return r == PORRT_ERR_DEVICE && e.find("hipMalloc") != std::string::npos ? (int)PORRT_ERR_CAPACITY : r;
        }
    }
    // the policy nodes' states: the recipe again, on the host
    const uint64_t total = pol.off[n];
    pol.xy.resize(2 * total);
    for (uint32_t q = 0; q < n; ++q) {
        const MmBatchPlan &pl = ps[q];
        for (uint64_t k = pol.off[q]; k < pol.off[q + 1]; ++k) {
            const uint64_t own = mm_own_id(noff[q], pol.original[k]);
            const uint32_t m = (uint32_t)(std::upper_bound(pl.mode_off.begin(), pl.mode_off.end(), (uint32_t)own) - pl.mode_off.begin()) - 1;
            if (own >= pl.nodes || m >= pl.modes.size() ||
                !mm_recipe_point(pl.rec.modes[m].codes[own - pl.mode_off[m]], pl.px.data(), pl.py.data(), pl.px.size(), pl.rec.ex.data(), pl.rec.ey.data(), pl.rec.ex.size(),
                                 &pol.xy[2 * k], &pol.xy[2 * k + 1])) {
                lead->set_err("mm_plan_batch: a policy node outside its plan");
                return PORRT_ERR_DEVICE;
            }
        }
    }
    pol.tag = s.gen; pol.stamp = h->mm_costs_runs;
    pol.valid = true;
    S.info.ms_policies += 1e3 * (now_s() - t0);
    S.info.ms_device += pol.info.ms_device;
    const size_t q0 = S.status.size();
    const uint64_t base = S.off.back();
    S.status.insert(S.status.end(), pol.status.begin(), pol.status.end());
    S.cost.insert(S.cost.end(), pol.cost.begin(), pol.cost.end());
    if (refine_iterations == 0) {
        for (uint32_t q = 0; q < n; ++q) {
            S.rstatus.push_back(1); S.rcost.push_back(0.0);
            for (uint64_t k = pol.off[q]; k < pol.off[q + 1]; ++k) {
                S.xy.push_back(pol.xy[2 * k]); S.xy.push_back(pol.xy[2 * k + 1]);
                S.original.push_back(mm_own_id(noff[q], pol.original[k]));
                S.parent.push_back(pol.parent[k]);
                S.leaf.push_back(pol.leaf[k]);
            }
            S.off.push_back(base + pol.off[q + 1]);
        }
    } else {
        t0 = now_s();
        const uint64_t cap = std::max<uint64_t>(total, 1);
        std::vector<uint64_t> roff(n + 1), roid(cap);
        std::vector<uint8_t> rst(n), rleaf(cap);
        std::vector<double> rc(n), rxy(2 * cap);
        std::vector<int64_t> rpar(cap);
        porrt_ctx::RefineInBuf buf;
        const int64_t rt = h->refine_call("mm_plan_batch", false, h->mm_refine_in(pol, buf), refine_iterations,
                                          RefinePoliciesOut{roff.data(), rst.data(), rc.data(), rxy.data(), roid.data(), rpar.data(), rleaf.data(), cap}, nullptr);
        if (rt < 0) return fail((int)rt);
        if ((uint64_t)rt > cap) { lead->set_err("mm_plan_batch: the refinement returned more nodes than went in"); return PORRT_ERR_INVALID; }
        S.info.ms_refine += 1e3 * (now_s() - t0);
        S.info.ms_device += h->refp_info.ms_device;
        for (uint32_t q = 0; q < n; ++q) {
            S.rstatus.push_back(rst[q]); S.rcost.push_back(rc[q]);
            for (uint64_t k = roff[q]; k < roff[q + 1]; ++k) {
                S.xy.push_back(rxy[2 * k]); S.xy.push_back(rxy[2 * k + 1]);
                S.original.push_back(mm_own_id(noff[q], roid[k]));
                S.parent.push_back(rpar[k]);
                S.leaf.push_back(rleaf[k]);
            }
            S.off.push_back(base + roff[q + 1]);
        }
    }
    for (uint32_t q = 0; q < n; ++q) {
        const MmBatchPlan &pl = ps[q];
        porrt_mm_batch_plan c{};
        c.modes = pl.modes.size(); c.transitions = pl.tr.size(); c.beliefs = pl.n_beliefs; c.nodes = pl.nodes;
        c.forward_edges = bounds[q + 1] - bounds[q]; c.belief_edges = bounds[n + 1 + q + 1] - bounds[n + 1 + q]; c.finals = pl.n_finals; c.pass = S.info.passes;
        S.plans.push_back(c);
        S.info.policies_ok += S.status[q0 + q] == 0 ? 1 : 0;
        S.info.prefix_points += pl.px.size(); S.info.explicit_points += pl.rec.ex.size();
    }
    S.info.modes += M; S.info.transitions += n_tr; S.info.nodes += NT; S.info.forward_edges += d.E; S.info.belief_edges += s.n_edges; S.info.finals += n_finals;
    S.last_first = (uint32_t)q0;
    S.last_noff = noff;
#undef MB_HIP
    return PORRT_OK;
}

int64_t mm_plan_batch_copy_out(const MmPlanBatchState &S, uint64_t *pol_off, uint8_t *status, double *expected_costs, uint8_t *refine_status, double *refined_costs,
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

int64_t mm_plan_batch(porrt_ctx *lead, uint32_t n_plans, const double *starts, const double *priors, const uint64_t *sampler_seeds, const uint64_t *discrete_seeds,
                      uint32_t n_worlds, double max_step, double search_radius, uint64_t n_iter_per_belief, uint64_t refine_iterations, uint64_t *pol_off,
                      uint8_t *status, double *expected_costs, uint8_t *refine_status, double *refined_costs, double *xy, uint64_t *original_ids, int64_t *parents,
                      uint8_t *is_leaf, uint64_t cap) {
    const double t_call = now_s();
    // ---- refusals, before any launch
    auto refuse = [&](const std::string &what) { lead->set_err("mm_plan_batch: " + what); return (int64_t)PORRT_ERR_INVALID; };
    if (lead->mm_plan_batch) ((MmPlanBatchState *)lead->mm_plan_batch.get())->valid = false;
    if (n_plans < 1 || n_plans > kMmBatchPlansLimit) return refuse("1 .. 65536 plans");
    if (!starts || !priors) return refuse("starts and priors are needed");
    if (!pol_off || !status || !expected_costs) return refuse("pol_off, status and expected_costs are needed");
    if (!lead->has_grid || lead->domain != PORRT_DOMAIN_SHELF || lead->n_zones == 0) return refuse("a shelf domain with zones (porrt_set_grid + porrt_set_zones)");
    if (n_worlds != (uint32_t)lead->n_worlds) return refuse("the priors need one probability per world of the context");
    if (!(max_step > 0.0) || !(search_radius > 0.0)) return refuse("bad PRM parameters");
    if (refine_iterations >= (1ull << 31)) return refuse("refine_iterations must be below 2^31");
    for (uint32_t p = 0; p < n_plans; ++p) {
        double sum = 0.0;                                    // check_belief_state, as grow_mm_prm sums it
        for (uint32_t w = 0; w < n_worlds; ++w) sum += priors[(size_t)p * n_worlds + w];
        if (std::fabs(sum - 1.0) > 1e-6) return refuse("plan " + std::to_string(p) + ": belief state does not sum to 1 (check_belief_state)");
    }
    // ---- the mode trees, recorded: plans are independent, on up to 8 host threads
    double t0 = now_s();
    std::vector<MmBatchPlan> plans(n_plans);
    {
        const unsigned nt = std::max(1u, std::min<unsigned>(std::min<unsigned>(8u, n_plans), std::max(1u, std::thread::hardware_concurrency())));
        std::vector<uint8_t> threw(nt, 0);
        auto work = [&](unsigned t) {
            try {
                for (uint32_t p = t; p < n_plans; p += nt) {
                    Pcg64 cr = lead->crng, dr = lead->drng;
                    if (sampler_seeds) cr.seed_from_u64(sampler_seeds[p]);
                    if (discrete_seeds) dr.seed_from_u64(discrete_seeds[p]);
                    mm_batch_record(lead, starts + 2 * (size_t)p, priors + (size_t)p * n_worlds, n_worlds, n_iter_per_belief, cr, dr, plans[p]);
                }
            } catch (...) { threw[t] = 1; }
        };
        {
            struct Joiner { std::vector<std::thread> th; ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); } } pool;
            for (unsigned t = 1; t < nt; ++t) pool.th.emplace_back(work, t);
            work(0);
        }
        for (uint8_t t : threw) if (t) { lead->set_err("mm_plan_batch: out of host memory for the mode trees"); return PORRT_ERR_NOMEM; }
    }
    for (uint32_t p = 0; p < n_plans; ++p)
        if (plans[p].r) { lead->set_err("mm_plan_batch: plan " + std::to_string(p) + ": " + plans[p].err); return plans[p].r; }
    const double ms_trees = 1e3 * (now_s() - t0);
    if (hipSetDevice(lead->device) != hipSuccess) { lead->set_err("mm_plan_batch: hipSetDevice"); return PORRT_ERR_DEVICE; }
    MmPlanBatchState &S = mm_plan_batch_state(lead);
    if (!S.helper) {
        S.helper = porrt_create(lead->device);
        if (!S.helper) { lead->set_err("mm_plan_batch: the helper context could not be created"); return PORRT_ERR_DEVICE; }
    }
    porrt_ctx *h = S.helper;
    if (S.helper_raster_gen != lead->raster_gen) { tamp_copy_domain(h, lead); S.helper_raster_gen = lead->raster_gen; }
    h->visibility = lead->visibility;
    for (int d = 0; d < 2; ++d) { h->s_low[d] = lead->s_low[d]; h->s_up[d] = lead->s_up[d]; }
    if (h->opt_box_table != lead->opt_box_table) { h->opt_box_table = lead->opt_box_table; h->cls_dirty = true; }
    h->opt_dp_sweeps = lead->opt_dp_sweeps; h->opt_dp_wide_rows = lead->opt_dp_wide_rows; h->opt_policy_max_nodes = lead->opt_policy_max_nodes;
    h->opt_refine_short_lds = lead->opt_refine_short_lds;
    S.off.assign(1, 0);
    S.status.clear(); S.rstatus.clear(); S.leaf.clear(); S.cost.clear(); S.rcost.clear(); S.xy.clear(); S.original.clear(); S.parent.clear(); S.plans.clear();
    S.last_noff.clear();
    memset(&S.info, 0, sizeof S.info);
    S.info.plans = n_plans;
    S.info.ms_host = ms_trees;
    std::vector<uint64_t> nodes(n_plans);
    for (uint32_t p = 0; p < n_plans; ++p) nodes[p] = plans[p].nodes;
    for (uint32_t first = 0; first < n_plans;) {
        const uint32_t end = mm_pass_end(nodes.data(), n_plans, first, lead->opt_mm_plan_batch_max_nodes);
        const int r = mm_plan_batch_pass(lead, S, plans.data() + first, end - first, n_worlds, max_step, search_radius, refine_iterations);
        if (r) return r;
        ++S.info.passes;
        first = end;
    }
    S.info.policy_nodes = S.off.back();
    S.info.ms_wall = 1e3 * (now_s() - t_call);
    S.valid = true;
    for (uint32_t p = 0; p < n_plans; ++p)
        if (S.status[p]) { lead->set_err("mm_plan_batch: plan " + std::to_string(p) + ": " + kPolStatusText[S.status[p] < 5 ? S.status[p] : 0]); break; }
    return mm_plan_batch_copy_out(S, pol_off, status, expected_costs, refine_status, refined_costs, xy, original_ids, parents, is_leaf, cap);
}

} // namespace
