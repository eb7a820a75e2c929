// porrt_launch.hpp -- one launch sequence of the RRT* / belief-space growth (host code): the rows its kernels go to, the launch forms
// in force and how far the steps, the rewire commit and the kd chain beside them have come.  A context has one, porrt_ctx::seq, and
// begin() is the only place that resets it.  Streams, events, the event pool and the options stay in the context (`cx`).  The
// methods are defined in porrt_engine.hip, below the kernels they launch.
#pragma once
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

struct porrt_ctx;

// The choices in force for a launch sequence: made by porrt_ctx::launch_forms from the options, fixed by LaunchSeq::begin.
struct LaunchForms {
    uint32_t group = 0;        // lanes per sample of the group kernels (16 / 32 / 64), 0 = the one-wave-per-sample kernels
    bool pipe = false;         // pipelined steps (k_step_rrt / k_file_commit): q_* in two halves
    bool lag = false;          // one kernel per step (k_step1_rrt) on the pipelined layout
    bool kd_lazy = false;      // only the goal path of the kd order beside the steps; the structure after them if a tie asks
};

// A lane count 16 / 32 / 64 (anything else: 64) as a compile-time constant: f(std::integral_constant<int, GL>)
template <class F> inline void with_lanes(uint32_t lanes, F &&f) {
    if (lanes == 16u) f(std::integral_constant<int, 16>{});
    else if (lanes == 32u) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

// k_kd_claim of a group: by group size, rows and kd_claim_threads (ByRows); a single query's side stream (<kClaimMax, true>);
// the plain <2048> / <kClaimMax> pair of the persistent loop, whatever kd_claim_threads says
enum class KdClaim { ByRows, SingleSide, Plain };
// what follows the claim on the group's stream: nothing (the hints ride in the next group's locate), k_kd_hint, k_kd_hint_fix
enum class KdThen { Nothing, Hint, HintFix };
using LaunchRows = std::pair<const RunConst *, uint32_t>;      // a RunConst array (one row of the grid per entry) and its rows

// Which forms of the kd side chain a launch sequence launched: the bits of LaunchSeq::kd_forms_run (view "kd_forms_run", documented
// in porrt_hip.h).  Host bookkeeping for the tests: no launch depends on it.
enum KdForm : uint32_t {
    kKdfClaimOne2048 = 1u << 0,         // k_kd_claim<2048>                      (one row, the engine's workgroup size)
    kKdfClaimOneMax = 1u << 1,          // k_kd_claim<kClaimMax>
    kKdfClaimRows1024x256 = 1u << 2,    // k_kd_claim<CAP, false, TPB>, one workgroup per row: CAP x TPB
    kKdfClaimRows1024x512 = 1u << 3,
    kKdfClaimRows1024x1024 = 1u << 4,
    kKdfClaimRows2048x256 = 1u << 5,
    kKdfClaimRows2048x512 = 1u << 6,
    kKdfClaimRows2048x1024 = 1u << 7,
    kKdfClaimRowsMaxx512 = 1u << 8,
    kKdfClaimRowsMaxx1024 = 1u << 9,
    kKdfClaimSingleSide = 1u << 10,     // k_kd_claim<kClaimMax, true>: a single query's side stream
    kKdfLocate1 = 1u << 11,             // k_kd_locate<1>: one thread per node
    kKdfLocate64 = 1u << 12,            // k_kd_locate<64>: one wave per node
    kKdfHintsRide = 1u << 13,           // a group's hints and the deferred ties rode in the next group's locate kernel
    kKdfHint = 1u << 14,                // k_kd_hint after a group's claim
    kKdfHintFix = 1u << 15,             // k_kd_hint_fix after a group's claim (kd_inline: on the main stream)
    kKdfTieFixBeside = 1u << 16,        // k_tie_fix<256> on the side stream after a group, beside the steps
    kKdfBuiltAfter = 1u << 17,          // groups launched after the steps on the main stream (kd_after, or kd_lazy when a tie asked)
    kKdfAll = (1u << 18) - 1u
};

struct LaunchSeq {
    porrt_ctx &cx;
    explicit LaunchSeq(porrt_ctx &c) : cx(c) {}
    // ---- fixed by begin(): the rows, the geometry, the forms (by their names in the launch code)
    const RunConst *rcp = nullptr;
    uint32_t Q = 1, K = 0, vwords = 0;
    int mode = 0;
    size_t lds_bytes = 0;
    uint32_t opt_group = 0;
    bool pipe_on = false, lag_on = false, kd_lazy = false;
    uint32_t kd_group = 1;             // steps per kd insertion
    int kd_built_after = 0;            // 1: a tie of this sequence needed the whole kd structure, built after the steps
    uint32_t kd_forms_run = 0;         // KdForm bits of what this sequence launched (a replayed capture: of what the capture launched)
    // ---- advanced per step
    uint32_t commit_pend_b = 0xFFFFFFFFu, commit_pend_nb = 0;      // step whose rewire phase 2 rides in the next search kernel
    uint32_t lag_near_done = 0xFFFFFFFFu, pipe_near_done = 0xFFFFFFFFu;    // one kernel per step / pipelined: the step whose search (and filing) is already launched
    uint32_t kd_b0 = 0, kd_last_b = 0, kd_last_nb = 0, kd_gidx = 0;        // steps [kd_b0, kd_last_b] wait for their kd group
    uint32_t kd_hint_b0 = 0, kd_hint_ns = 0;   // the group whose hints and deferred ties ride in the next group's locate kernel
    bool kd_pend[3] = {false, false, false};   // ev_kd[] of a group that the main stream has not waited for yet
    bool gt_pend = false;                      // gtrack_side: a k_gtrack is in flight on the side stream (its event: ev_kd[gt_par])
    uint32_t gt_par = 0;
    bool side_active = false;                  // something was launched that join_side has to join or settle
    bool kd_build_now = false;                 // kd_full_build is launching the structure after the steps

    void begin(const RunConst *rows, uint32_t n_rows, uint32_t K_, int mode_, size_t lds, const LaunchForms &f);
    // The rows the next launches go to.  Only the driver that began the sequence switches them (a batch's compacted rows, the rows
    // that asked for the kd structure) and it switches back before it reads results.  Returns the rows in force before.
    LaunchRows switch_rows(const RunConst *rows, uint32_t n_rows) { const LaunchRows was(rcp, Q); rcp = rows; Q = n_rows; return was; }
    void restore_rows(const LaunchRows &was) { rcp = was.first; Q = was.second; }
    // A member of a batch only prepares.  (An accident kept: its "pipeline" reads 0 afterwards while its "group_lanes", "kd_lazy" and
    // "kd_built_after" still read its last sequence of its own -- ask the batch's first context.)
    void prepared_as_member() { pipe_on = lag_on = false; }

    void launch_step(uint32_t b, uint32_t i0, uint32_t nb, bool prof, size_t &ev_used, uint32_t nxt_i0, uint32_t nxt_nb);
    uint32_t launch_steps(uint64_t n_iter, bool prof, size_t &ev_used);     // every step of n_iter iterations, then join_side
    int replay_steps(uint64_t n_iter, double *t_capture);                   // the same as the context's cached hipGraph
    int launch_coop(uint32_t n_steps, uint64_t n_iter);
    void flush_commit();
    void join_side();
    int kd_full_build(const std::vector<std::pair<uint32_t, uint32_t>> &segs);

private:
    void rewind_kd();
    void steps_ran(uint32_t b) { kd_b0 = b; kd_last_b = b ? b - 1 : 0; }   // ... by a graph or the persistent loop, kd groups and join included
    void launch_kd_group();
    void kd_group_on(hipStream_t st, uint32_t b0, uint32_t ns, uint32_t nb_last, uint32_t wait, uint32_t hint_b0, uint32_t hint_ns, KdClaim claim, KdThen then);
    void tie_fix_on(hipStream_t st);
};
