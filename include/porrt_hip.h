/*
 * porrt_hip.h -- C ABI of the MI355X-native batched belief-space RRT expansion
 * engine (libporrt_hip.so).  Plain pointers and sizes only; no torch / HIP types.
 *
 * It is the drop-in for ONE path of cambyse/po-rrt: the grow/extend loop
 *     RRT::grow_tree   src/rrt.rs:102-174  (RRT* with best-parent + rewire)
 *     PTO::grow_graph  src/pto.rs:55-139   (belief-space RRG + Reachability)
 * instantiated for the reference's grid-backed domains
 *     MapShelfDomain   src/map_shelves_io.rs:65-203,459-488 (RTTFuncs adapter
 *                      src/map_shelves_tamp_rrt.rs:35-47)
 *     Map (doors)      src/map_io.rs:67-241,482-513
 * and its declarative goals (SquareGoal src/common.rs:304-350, ObservationGoal
 * src/rrt.rs:325-341).  The reference's trait callbacks (RTTFuncs rrt.rs:64-76,
 * PTOFuncs pto_graph.rs:121-168, GoalFuncs common.rs:294-302) are opaque host
 * closures, so the engine takes their DATA (grid, zones, goal table, sampler box
 * and seed) instead of their code.  The style follows the reference's own C
 * boundary (src/pto_c.rs:63-270: opaque handle, setters, plan, getters) without
 * callbacks and without taking ownership of caller memory.
 *
 * Conventions: every call returns 0 on success or a negative PORRT_ERR_* code
 * (porrt_last_error() gives the text); nothing panics across the boundary; the
 * caller owns all host buffers; one context drives one GPU and is not
 * thread-safe (it mirrors `&mut self` of RRT::plan, rrt.rs:88); sampler state
 * persists across porrt_grow calls on one context (the reference reuses one RRT
 * object for many plans, src/map_shelves_tamp_rrt.rs:196-232).
 *
 * Limits: states are 2-D (every grid-backed domain of the reference is); at most 64 worlds (one
 * u64 mask per node; the reference's largest case has 16) and 64 goals; batch_K in 1..4096; rasters
 * up to 2^32 pixels; iteration counts below 2^31.  Capacities inside (neighbour lists, edge and
 * deferred-tie pools) grow on demand: the run is replayed from the saved sampler state, results do
 * not depend on it.
 */
#ifndef PORRT_HIP_H
#define PORRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct porrt_ctx porrt_ctx;

enum {
    PORRT_OK = 0,
    PORRT_INCOMPLETE = 1,           /* PTO: "final nodes are not reached for each world" (pto.rs:137) */
    PORRT_ERR_INVALID = -1,         /* bad argument / call order */
    PORRT_ERR_INVALID_START = -2,   /* pto.rs:61 expect("Start from a valid state!") */
    PORRT_ERR_RASTER = -3,          /* pixel access outside the map, door pixel without zone id, or a
                                       segment crossing two zones: the reference panics there
                                       (image get_pixel; map_io.rs:233) */
    PORRT_ERR_DEVICE = -4,          /* HIP runtime error */
    PORRT_ERR_CAPACITY = -5,        /* a neighbour list outgrew its capacity even after regrowth */
    PORRT_ERR_NO_DEVICE = -6,
    PORRT_ERR_IO = -7,              /* a file could not be opened / written (the reference panics: "Impossible to open image") */
    PORRT_ERR_PEER = -8,            /* porrt_exchange_best: another rank of the collective failed; no rank went on */
    PORRT_ERR_NOMEM = -9,           /* a host allocation failed (std::bad_alloc never crosses the boundary) */
    PORRT_ERR_NO_PATH = -10         /* porrt_tamp_rrt_plan: a query found no path (the reference panics: "no observation path found!" /
                                       "no pickup path found!"); porrt_tamp_rrt_get_info names the search node, the zone and the query */
};

enum { PORRT_DOMAIN_SHELF = 0, PORRT_DOMAIN_DOOR = 1 };   /* MapShelfDomain / Map */
enum { PORRT_MODE_RRT = 0, PORRT_MODE_PTO = 1, PORRT_MODE_PRM = 2 };   /* RRT::grow_tree / PTO::grow_graph / PRM::grow_graph (results only) */

/* ---- lifetime.  Replaces: RRT::new (rrt.rs:84-86) / PTO::new (pto.rs:37-53) --------- */
porrt_ctx  *porrt_create(int device);      /* NULL when no HIP device is usable */
void        porrt_destroy(porrt_ctx *ctx);
const char *porrt_last_error(const porrt_ctx *ctx);

/* ---- domain data.  Replaces: MapShelfDomain::open/build (map_shelves_io.rs:80-94),
 * Map::open/build (map_io.rs:82-96): ppm = W / (up[0] - low[0]); raster row-major,
 * occ[i*W + j] = img.get_pixel(j, i). */
int porrt_set_grid(porrt_ctx *ctx, const uint8_t *occ, uint32_t W, uint32_t H,
                   const double low[2], const double up[2], int domain);
/* Replaces: add_zones (map_shelves_io.rs:106-148, map_io.rs:113-161): zone raster
 * (255 = none), zone centroids, worlds and world validities are derived inside. */
int porrt_set_zones(porrt_ctx *ctx, const uint8_t *zone_ids, double visibility);

/* ---- samplers.  Replaces: ContinuousSampler::new + DiscreteSampler::new
 * (sample_space.rs:13-21,45-49; the reference hard-codes seed 0).  The stream is
 * rand_pcg Pcg64::seed_from_u64(seed) with rand 0.8 gen_range, generated on the GPU. */
int porrt_set_sampler(porrt_ctx *ctx, const double low[2], const double up[2], uint64_t seed);
int porrt_set_discrete_seed(porrt_ctx *ctx, uint64_t seed);
/* Inject the stream instead: xy[2*i..] is the i-th value ContinuousSampler::sample()
 * would return (goal-biased iterations consume none, rrt.rs:176-181); worlds[i] is
 * the i-th DiscreteSampler::sample() value (one per iteration, pto.rs:142). */
int porrt_set_samples(porrt_ctx *ctx, const double *xy, size_t n);
int porrt_set_worlds(porrt_ctx *ctx, const uint32_t *worlds, size_t n);

/* ---- goals.  Replaces: SquareGoal::new (common.rs:310-333); bit w of masks[g] is
 * world w of the goal's validity.  ObservationGoal (rrt.rs:325-341). */
int porrt_set_square_goal(porrt_ctx *ctx, const double *centers /* G*2 */, const uint64_t *masks,
                          uint32_t G, double l1_radius);
int porrt_set_observation_goal(porrt_ctx *ctx, uint32_t zone_id);

/* ---- the hot path.  Replaces: RRT::grow_tree (rrt.rs:102-174) when mode is
 * PORRT_MODE_RRT and PTO::grow_graph (pto.rs:55-139) when PORRT_MODE_PTO.
 * batch_K samples are expanded per step against the tree as it stands at the start
 * of the step; batch_K = 1 is the reference's loop.  Returns PORRT_OK,
 * PORRT_INCOMPLETE (PTO only) or an error.
 * Replays: the call runs the growth again, from the sampler state it was entered with, when a neighbour list overflowed (the lists
 * grow: "cand_cap"), when a float draw of the device sampler would have been redrawn (again with the exact host stream), when the
 * PTO edge pool overflowed ("edge_per_node" * 4) and when the pool of deferred equal-cost parents overflowed ("tie_pool_ids", or
 * the default pool, * 4); at most 12 attempts.  The results are those of the attempt that went through.
 * What a failed growth leaves: after PORRT_ERR_CAPACITY (a pool that may grow no more, the region page pool, the attempts used up)
 * the context has NO results -- the getters answer as on a context that never grew -- and its samplers stand where the call found
 * them; likewise after every other error that leaves no results ("injected sample stream exhausted", a device error).
 * PORRT_ERR_RASTER of a porrt_grow keeps the results and the sampler state of the run that met it. */
int porrt_grow(porrt_ctx *ctx, const double start[2], double max_step, double search_radius,
               uint64_t n_iter_min, uint64_t n_iter_max, uint32_t batch_K, int mode);

/* The same growth for several contexts of ONE device at once -- the form in which the reference's many-query caller uses the path:
 * the TAMP search runs rrt.plan(.., n_iter_min 2500, n_iter_max 10000) twice per search edge (map_shelves_tamp_rrt.rs:224,232,355,
 * 367,492,500; main.rs:532), thousands of independent queries.  Their dependent-load chains overlap inside each kernel launch (one
 * grid row per context) instead of queueing behind each other.  Every context runs the loop of rrt.rs:109 / pto.rs:67,
 *     while i < n_iter_min || (no solution yet && i < n_iter_max),
 * on its own: a member whose loop has ended drops out of the later launches (a row mask kept on the device), the others go on.
 * starts = n_ctx x 2.  Every context keeps its own map, goal, sampler state and results, exactly as after n_ctx porrt_grow calls
 * with the same arguments; the getters are per context.  Contexts must not be used concurrently elsewhere during the call.
 * Returns the worst member code (PORRT_INCOMPLETE if a PTO member's final set is incomplete).
 * Only the neighbour lists are regrown for a batch.  A member whose draw would have been redrawn (PORRT_ERR_INVALID, "grow this
 * context on its own") or whose edge or deferred-tie pool overflowed (PORRT_ERR_CAPACITY) fails the call, as does any other negative
 * member code; then EVERY context of the call is as the call found it -- sampler and world streams, injected stream positions --
 * except that none has results and none belongs to a batch: each can be grown on its own, or the batch again, as if the call had
 * not been made.  (A call refused for its arguments before a context was begun on leaves that context untouched, results included.)
 * porrt_grow_batch_each: the same with n_iter_min[q], n_iter_max[q] per context. */
int porrt_grow_batch(porrt_ctx *const *ctxs, uint32_t n_ctx, const double *starts, double max_step,
                     double search_radius, uint64_t n_iter_min, uint64_t n_iter_max, uint32_t batch_K, int mode);
int porrt_grow_batch_each(porrt_ctx *const *ctxs, uint32_t n_ctx, const double *starts, double max_step,
                          double search_radius, const uint64_t *n_iter_min, const uint64_t *n_iter_max, uint32_t batch_K, int mode);

/* ---- results, copied into caller-owned buffers (query the sizes first).
 * Replaces: RRTTree{nodes: Vec<RRTNode{state,parent_id,dist_from_root}>} (rrt.rs:14-22)
 * and the final ids returned by grow_tree (rrt.rs:103,165-167). */
uint64_t porrt_num_nodes(const porrt_ctx *ctx);
uint64_t porrt_num_iterations(const porrt_ctx *ctx);
int      porrt_get_tree(const porrt_ctx *ctx, double *xy /* N*2 */, int64_t *parent /* -1 = root */,
                        double *dist_root);
/* The same for n contexts of one device at once (the trees of a porrt_grow_batch): worker threads with pinned staging
 * and copy streams of their own overlap the device-to-host copies with laying the trees out in the caller's arrays
 * (xy[q]: N_q*2 doubles, parent[q]: N_q, dist_root[q]: N_q; an array of pointers, or single entries, may be NULL). */
int      porrt_get_trees(porrt_ctx *const *ctxs, uint32_t n_ctx, double *const *xy, int64_t *const *parent,
                         double *const *dist_root);
/* A caller that fetches trees again and again into the same arrays can hand those arrays to the device once: porrt_host_pin page-locks
 * [p, p + bytes) and maps it for the GPU (hipHostRegister), and a porrt_get_trees whose every output array lies inside pinned ranges
 * lets ONE kernel write all the trees straight into the caller's arrays in their final layout -- no staging copies, no host threads
 * re-packing them.  The range must stay allocated until porrt_host_unpin (a freed and re-used address would be written through the
 * old mapping).  Arrays that are not pinned take the staged path above; the results are the same. */
int      porrt_host_pin(void *p, size_t bytes);
int      porrt_host_unpin(void *p);
uint64_t porrt_num_final(const porrt_ctx *ctx);
int      porrt_get_final_ids(const porrt_ctx *ctx, uint64_t *ids);
int      porrt_get_final_masks(const porrt_ctx *ctx, uint64_t *masks);
/* PTO mode.  Replaces: Reachability::reachability (pto_reachability.rs:54-56),
 * PTONode.validity_id and the PTOGraph edges (pto_graph.rs:171-207): forward edges
 * (neighbour -> new node) in the order the reference adds them (pto.rs:103-114): new nodes
 * ascending, and for one new node its neighbours in the order KdTree::nearest_neighbors lists
 * them (kd pre-order, nearest_neighbor.rs:101-117) -- so that adjacency lists rebuilt from it
 * equal the reference's element for element.  The reference also stores each reverse edge with
 * the same validity id (pto.rs:117-120).  The order is restored on the device when the edges are
 * first asked for (the edges are dealt into one bucket per node and each bucket is ordered by one
 * wave, by the nodes' kd pre-order ranks, which the host supplies from a kd-tree over the node
 * coordinates); the growth itself does not need it. */
int      porrt_get_reach(const porrt_ctx *ctx, uint64_t *masks /* N */);
int      porrt_get_node_validity(const porrt_ctx *ctx, uint32_t *validity_ids /* N */);
uint64_t porrt_num_edges(const porrt_ctx *ctx);
int      porrt_get_edges(const porrt_ctx *ctx, uint32_t *from, uint32_t *to, uint32_t *validity_id);
int      porrt_is_final_set_complete(const porrt_ctx *ctx);   /* pto_reachability.rs:81-90 */
/* derived domain data (map_shelves_io.rs:113,132-148; map_io.rs:121-126) */
int      porrt_n_worlds(const porrt_ctx *ctx);
int      porrt_get_validities(const porrt_ctx *ctx, uint64_t *masks /* <= 65 */);
int      porrt_get_zone_positions(const porrt_ctx *ctx, double *xy /* <= 64*2 */);

/* Host side of RRT::plan (get_best_solution rrt.rs:183-193, get_path_to 48-61,
 * get_path_cost 223-227): length of the best path (0 = "No solution found");
 * path_xy may be NULL to query the length. */
uint64_t porrt_best_solution(const porrt_ctx *ctx, double *path_xy, uint64_t cap, double *cost);
/* The cost (and final node) of that path alone, evaluated on the device without fetching the tree: same
 * arithmetic, same first-minimum rule, bit-identical cost.  Lets a caller that holds many trees on the GPU
 * (porrt_grow_batch) pick the one worth downloading.  Returns 1, or 0 for "No solution found". */
int      porrt_best_cost(const porrt_ctx *ctx, double *cost, uint64_t *final_id);
/* The same for the n contexts of the last porrt_grow_batch, in one launch (one workgroup per context);
 * costs[q] = +inf where context q has no solution.  Other sets of contexts are evaluated one after the other. */
int      porrt_best_cost_batch(porrt_ctx *const *ctxs, uint32_t n_ctx, double *costs);

/* ---- PRM* roadmap growth: PRM::init(start) + PRM::grow_graph(max_step, search_radius, n_iter) (src/prm.rs:33-109) on a
 * grid-backed domain.  Every sample becomes a node (the reference neither steers nor checks the state; validity id 0),
 * connected both ways to the earlier nodes within heuristic_radius(graph size) whose transition the domain's
 * transition_validator accepts.  The roadmap depends on the sample stream only, so the whole of it is evaluated at once
 * with the reference's sequential semantics (no batch size).  Samples: the context's sampler (its state moves on by
 * n_iter draws) or the injected stream.  Results through the getters of a PTO graph: porrt_num_nodes (n_iter + 1, node 0
 * = start), porrt_get_tree (coordinates; parents -1), porrt_num_edges / porrt_get_edges (the forward edges neighbour ->
 * new node in the reference's adjacency order; PTOGraph gets add_edge(from, to, 0) and add_edge(to, from, 0), the third
 * array is what transition_validator returned).  The edge list starts at 256 edges per node; a roadmap with more (its edges are
 * counted before they are written) is grown again from the same sampler state with a list of the counted size, up to 2^30 edges
 * (PORRT_ERR_CAPACITY beyond). */
int      porrt_grow_prm(porrt_ctx *ctx, const double start[2], double max_step, double search_radius, uint64_t n_iter);
/* PRM::plan_path (src/prm.rs:111-123) on that roadmap: the kd-tree's nearest nodes of start and goal
 * (nearest_neighbor.rs:48-91), dijkstra from the goal (src/pto_graph.rs:275-303; run as device sweeps to the same
 * fixpoint), extract_path (pto_graph.rs:305-326).  Returns the number of states of the path (0 = start and goal are not
 * connected: the reference returns an empty Vec); path_xy receives min(cap, that number) states. */
int64_t  porrt_prm_plan_path(porrt_ctx *ctx, const double start[2], const double goal[2], double *path_xy, uint64_t cap);
/* PRM::plan_path (src/prm.rs:111-123) for n start/goal pairs on the roadmap of the last porrt_grow_prm, in one call.
 * Query i is answered exactly as porrt_prm_plan_path(ctx, starts + 2i, goals + 2i, ..) would answer it: the same nearest nodes
 * (nearest_neighbor.rs:48-91, on the host), dijkstra from the goal (pto_graph.rs:275-303) as device sweeps of one row of costs per
 * distinct goal node -- queries that share a goal node share a row; rows run in passes of at most option "prm_rows" (default 256)
 * rows, fewer when a pass's costs would not fit the device memory budget -- and extract_path (pto_graph.rs:305-326) on the device,
 * one wave per query.  path_off (n + 1 entries) is always written: the states of query i are rows path_off[i] .. path_off[i+1] of
 * path_xy.  An empty range means that start and goal are not connected.  The states are written only if the total fits in cap
 * (counted in states).  The return value is the total, or a negative error: no roadmap on the context, a walk that meets a
 * zero-length cycle (PORRT_ERR_INVALID; porrt_last_error names the query), PORRT_ERR_CAPACITY when the device buffers of a pass
 * cannot be allocated (never a truncated answer).  n = 0 returns 0 and writes path_off[0] = 0. */
int64_t  porrt_prm_plan_paths(porrt_ctx *ctx, const double *starts, const double *goals, uint64_t n,
                              uint64_t *path_off, double *path_xy, uint64_t cap);
/* The states of the last porrt_prm_plan_paths, without recomputing them (same total and same cap rule).  It is an error once the
 * roadmap has changed (a new growth on the context) or before the first call. */
int64_t  porrt_prm_get_paths(const porrt_ctx *ctx, double *path_xy, uint64_t cap);
/* Counts and times of the last porrt_prm_plan_paths: queries, rows (distinct goal nodes), sweeps (summed over the passes), passes;
 * milliseconds on the device (HIP events over the passes), wall (the whole call) and of the nearest-node searches.  The struct
 * shares its name with the function, as struct stat does with stat(): C++ callers write `struct porrt_prm_paths_info`. */
struct porrt_prm_paths_info { uint64_t queries, rows, sweeps, passes; double ms_device, ms_wall, ms_nearest; };
int      porrt_prm_paths_info(const porrt_ctx *ctx, struct porrt_prm_paths_info *out);

/* ---- belief-space expansion: PTO::build_belief_graph (src/pto.rs:185-259) on the graph of the last
 * porrt_grow(mode PORRT_MODE_PTO) of this context, with PTOFuncs::reachable_belief_states (map_io.rs:515-546,
 * map_shelves_io.rs:490-520), PTOFuncs::observe (map_io.rs:281-300, map_shelves_io.rs:242-265) and
 * compute_compatibility (common.rs:266-276).  start_belief: one probability per world, summing to 1
 * (assert_belief_state_validity, common.rs:279-281).
 * Belief node id = graph node * n_beliefs + belief id -- the order of BeliefGraph::add_node at pto.rs:198-201;
 * node_to_belief_nodes[node][belief] is Some(that id) iff the belief is compatible with the node's validity, i.e. iff
 * the pair can have edges.  Children / parents come back as CSR lists in the reference's Vec::push order.
 * The lists stay on the device for the rows that follow; the getters copy them out.
 * Errors: the panics of the path ("no id corresponding to this belief state", hash collisions, raster faults in the
 * visibility raycast) become negative return codes. */
int      porrt_build_belief_graph(porrt_ctx *ctx, const double *start_belief, uint32_t n_worlds);
uint64_t porrt_bg_num_beliefs(const porrt_ctx *ctx);                 /* reachable_belief_states().len() */
uint64_t porrt_bg_num_nodes(const porrt_ctx *ctx);                   /* n graph nodes * n beliefs */
uint64_t porrt_bg_num_edges(const porrt_ctx *ctx);
int      porrt_bg_get_beliefs(const porrt_ctx *ctx, double *out /* n_beliefs * n_worlds */);
int      porrt_bg_get_observable_zones(const porrt_ctx *ctx, uint64_t *masks /* per graph node: bit z = zone z seen */);
int      porrt_bg_get_node_types(const porrt_ctx *ctx, uint8_t *types /* 0 Unknown, 1 Action, 2 Observation (belief_graph.rs:13-17) */);
int      porrt_bg_get_children(const porrt_ctx *ctx, uint64_t *off /* n_nodes + 1 */, uint32_t *ids /* n_edges, may be NULL */);
int      porrt_bg_get_parents(const porrt_ctx *ctx, uint64_t *off, uint32_t *ids);
/* seconds of the last build: [0] total, [1] device kernels (HIP events), [2] host tables, [3] reachable beliefs,
 * [4] observation fold table, [5] adjacency lists, [6] device allocation + uploads, [7] fetching the PTO edges */
int      porrt_bg_get_seconds(const porrt_ctx *ctx, double *out, uint32_t n);

/* ---- expected costs to the goals over the belief graph: PTO::compute_expected_costs_to_goals (src/pto.rs:261-275) =
 * the final belief nodes (final graph nodes x beliefs compatible with the node and with its finality), then
 * conditional_dijkstra (src/belief_graph.rs:89-175) with cost_evaluator = norm2 (the PTOFuncs default,
 * pto_graph.rs:150-152).  Runs on the belief graph of the last porrt_build_belief_graph, on the device; the costs stay
 * there.  Bit-identical to the reference's queue-driven loop (the relaxation is monotone in f64: every order ends in
 * the same fixpoint).  +inf = no policy from that belief node. */
int      porrt_bg_compute_expected_costs(porrt_ctx *ctx);
int      porrt_bg_get_expected_costs(const porrt_ctx *ctx, double *out /* porrt_bg_num_nodes() */);
int      porrt_bg_expected_cost_of(const porrt_ctx *ctx, uint64_t belief_node, double *out);   /* [0] = policy.expected_costs */
int      porrt_bg_get_dp_info(const porrt_ctx *ctx, double *total_s, double *device_s, uint32_t *sweeps);
/* belief nodes the sweeps of the last run passed over, summed over the sweeps (a sweep reads and writes a level's change flags and the
 * costs of the rows that changed: the unit of that row's roofline in bench.py) */
uint64_t porrt_bg_get_dp_sweep_rows(const porrt_ctx *ctx);
/* PTO::extract_policy (src/pto.rs:277-283; extract_policy / get_best_expected_children src/belief_graph.rs:177-263) from
 * belief node 0.  Policy node k (in Policy::add_node order; node 0 is the root) has original_node_id original_ids[k],
 * parent parents[k] (-1 for the root) and is a leaf (expected cost 0) iff is_leaf[k]; its state and belief follow from
 * the id (graph node id / n_beliefs, belief id % n_beliefs).  Returns the number of policy nodes; the arrays are filled
 * when cap holds them (call with cap 0 to size them).  *expected_costs = policy.expected_costs.  The walk runs on the
 * device as porrt_bg_extract_policies with the one start 0 (into a result of its own: what porrt_bg_get_policies and
 * porrt_policies_info hand out stays the last batched call's), up to 2^24 policy nodes whatever option
 * "policy_max_nodes" says.  PORRT_ERR_INVALID when the root has no finite expected cost or the walk returns to a belief
 * node on its own path (the reference would not terminate) or an assertion of the reference fails; PORRT_ERR_CAPACITY
 * beyond 2^24 policy nodes or 65535 children of one node. */
int64_t  porrt_bg_extract_policy(porrt_ctx *ctx, uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, uint64_t cap, double *expected_costs);
/* conditional_dijkstra on an explicit belief graph given as host arrays (the form of the reference's own tests,
 * belief_graph.rs:502-567): node i has state xy[2i..], belief vector beliefs[belief_row[i]], type types[i]
 * (1 Action, 2 Observation), children / parents as CSR in add_edge order.  No context needed.
 * parent_* must be the transpose of child_* (BeliefGraph::add_edge pushes both): the reference relaxes an action node from
 * the parents list of the node it popped, the device pulls it from its own children list, and a graph in which the two
 * lists disagree has no defined answer.  A node whose type is neither 1 nor 2, or an observation node with a child of
 * transition probability 0, is the reference's panic (PORRT_ERR_INVALID) only if one of its children gets a finite cost;
 * otherwise it is never relaxed and stays at +inf.
 * Every array is checked on the host before a device is looked for; PORRT_ERR_INVALID when n == 0 or n >= 2^32 - 1, a
 * required array is NULL (finals with n_final > 0; child_ids / parent_ids when their offsets announce entries),
 * n_belief_rows == 0 or n_worlds == 0, child_off[0] or parent_off[0] != 0, an offset array decreases,
 * belief_row[i] >= n_belief_rows, or a child id, parent id or final >= n. */
int      porrt_conditional_dijkstra(int device, uint64_t n, const double *xy, const uint32_t *belief_row, const double *beliefs,
                                    uint32_t n_belief_rows, uint32_t n_worlds, const uint8_t *types,
                                    const uint64_t *child_off, const uint32_t *child_ids, const uint64_t *parent_off, const uint32_t *parent_ids,
                                    const uint64_t *finals, uint64_t n_final, double *dist);

/* ---- policies from many belief nodes in one call: extract_policy / get_best_expected_children (src/belief_graph.rs:184-267)
 * started at belief node starts[q] instead of node 0, for n starts, walked on the device (one wave per query, porrt_policy.hpp).
 * The expected costs of the last porrt_bg_compute_expected_costs are costs-to-goal of every belief node, so no new build and no
 * new sweeps are needed.  Query q's root is policy node 0 with original id starts[q] and is_leaf 0, whatever its cost (:192);
 * children are clustered by belief id, clusters in ascending id order; within a cluster p = transition_probability(node, the
 * cluster's first child) (common.rs:187-190) and the winner is the first child in children order of strictly least
 * p * (norm2(node, child) + dist[child]), a cluster of +inf / NaN costs keeping its first child; winners become policy nodes in
 * cluster order, is_leaf = (dist[child] == 0.0), and the non-leaf ones are expanded last pushed first.  For starts[q] = 0 the
 * policy is, node for node, that of porrt_bg_extract_policy.
 * A start at a final node (dist 0) is walked exactly as the reference would walk it, not special-cased: its root is no leaf and
 * is expanded; whether that ends in status 0 or 3 follows from the graph (a child of positive cost fails :261).
 * status[q]: 0 OK; 1 dist[starts[q]] is not finite, no policy from there; 2 the walk returns to a belief node on its own path
 * (the reference does not terminate); 3 an assertion of the reference fails (p > 0.0, :250, or p * dist[best] <= dist[node],
 * :261); 4 the policy would exceed option "policy_max_nodes" (1 .. 2^24, default 65536) or a node has more than 65535 children.
 * A query whose status is not 0 contributes no policy nodes and does not void the others; porrt_last_error names the first one.
 * pol_off (n + 1 entries), status and expected_costs (dist[starts[q]]) are always written: the nodes of query q are rows
 * pol_off[q] .. pol_off[q + 1] of original_ids / parents / is_leaf, parents[k] an index into the same policy (-1 for its root).
 * The node arrays are written only if the total fits in cap.  Returns the total number of policy nodes, or a negative error:
 * PORRT_ERR_INVALID for a start >= porrt_bg_num_nodes, or when the belief graph or its costs are missing or stale (a regrowth, a
 * new belief graph without new costs); PORRT_ERR_CAPACITY when the device pool cannot be allocated.  n = 0 returns 0 and writes
 * pol_off[0] = 0.  The policy porrt_bg_refine_policy refines stays that of the last porrt_bg_extract_policy; the policies of this
 * call are refined together by porrt_bg_refine_policies (or one at a time through porrt_refine_policy). */
int64_t  porrt_bg_extract_policies(porrt_ctx *ctx, const uint64_t *starts, uint64_t n, uint64_t *pol_off, uint8_t *status,
                                   double *expected_costs, uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, uint64_t cap);
/* The nodes of the last porrt_bg_extract_policies, without recomputing them (same total, same cap rule).  An error before the
 * first call and once the graph, the belief graph or the costs have changed. */
int64_t  porrt_bg_get_policies(const porrt_ctx *ctx, uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, uint64_t cap);
/* The same on the multi-modal belief graph and the costs of the last porrt_mm_compute_expected_costs, clustered by the nodes'
 * belief ids (porrt_mm_bg_get_graph); xy (2 per node, may be NULL) receives the nodes' states as porrt_mm_extract_policy gives
 * them.  The policy porrt_mm_refine_policy refines stays that of the last porrt_mm_extract_policy. */
int64_t  porrt_mm_extract_policies(porrt_ctx *ctx, const uint64_t *starts, uint64_t n, uint64_t *pol_off, uint8_t *status,
                                   double *expected_costs, uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, double *xy, uint64_t cap);
int64_t  porrt_mm_get_policies(const porrt_ctx *ctx, uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, double *xy, uint64_t cap);
/* The same on an explicit belief graph given as host arrays, as porrt_conditional_dijkstra takes it (the walk reads neither the
 * node types nor the parents lists): node i has state xy[2i..], belief vector beliefs[belief_row[i]], clustering key
 * belief_ids[i] and expected cost dist[i] (any doubles: +inf and NaN follow the rules above).  The reference's own policy
 * assertions on its two known-answer graphs (belief_graph.rs:531-543, 563-566) run on the device through this entry.
 * policy_max_nodes: 1 .. 2^24, 0 = 65536.  No context needed. */
int64_t  porrt_extract_policies(int device, uint64_t n_nodes, const double *xy, const uint32_t *belief_row, const double *beliefs,
                                uint32_t n_belief_rows, uint32_t n_worlds, const uint32_t *belief_ids, const uint64_t *child_off,
                                const uint32_t *child_ids, const double *dist, const uint64_t *starts, uint64_t n, uint64_t policy_max_nodes,
                                uint64_t *pol_off, uint8_t *status, double *expected_costs, uint64_t *original_ids, int64_t *parents,
                                uint8_t *is_leaf, uint64_t cap);
/* Counts and times of the last porrt_bg_extract_policies or porrt_mm_extract_policies of the context, whichever ran last: queries,
 * those with status 0, policy nodes in all, nodes of the longest policy; milliseconds on the device (HIP events around the
 * kernels) and wall (the whole call).  C++ callers write `struct porrt_policies_info` (the name is the function's too). */
struct porrt_policies_info { uint64_t queries, ok, nodes, max_nodes; double ms_device, ms_wall; };
int      porrt_policies_info(const porrt_ctx *ctx, struct porrt_policies_info *out);

/* ---- policy refinement: PTOPolicyRefiner::refine_solution(RefinmentStrategy::PartialShortCut(n_iterations))
 * (src/pto_policy_refiner.rs:87-124; pto_c.rs:217-218 runs it inside plan()).  The policy is cut into pieces (Policy::decompose,
 * common.rs:85-129: breadth-first from node 0, a piece runs until a node with 0 or >= 2 children); every piece of >= 3 nodes is
 * shortcut with a fresh DiscreteSampler::new() (Pcg64 seed 0), n_iterations times: interpolate one joint over a random interval and
 * keep it when every transition of the interval is valid under the piece's belief (is_transition_valid :395-423 -- state_validity,
 * transition_validator, compute_compatibility); pieces of <= 2 nodes are left alone.  The pieces are put back together (recompose
 * :324-393): pieces in order, each piece's nodes in path order, then the skeleton edges from the end of a piece to the starts of the
 * pieces after it; expected_costs by common.rs:131-154 (norm2).  Deterministic: bit for bit the reference's output.
 * Quirk kept: recompose marks a piece's first node as its start and only a LATER node as its end (`if is_start .. else if is_end`,
 * :348-366), so a one-node piece that branches gets no skeleton edges -- the pieces after it keep parent -1 and it becomes a leaf.
 * RefinmentStrategy::Reparent is offered through entry points of its own, with rules of ours where the reference's text pins
 * none: porrt_bg_reparent_policies below.
 *
 * porrt_bg_refine_policy refines the policy the last porrt_bg_extract_policy handed out (an error if there is none, or if the graph
 * was regrown, the belief graph rebuilt or the expected costs recomputed since).  Refined node k has state xy[2k..], original id
 * original_ids[k] (that of the policy node it came from), parent parents[k] (-1 for the root and for a piece start left unconnected
 * by the quirk) and is a leaf (no children) iff is_leaf[k].  Returns the number of nodes; the arrays and *expected_costs are filled
 * when cap holds them (call with a smaller cap, 0 for one, to size them: that call does no device work and checks the parents
 * alone).  It is porrt_bg_refine_policies' path with one policy and a result of its own (what porrt_refine_policies_info hands out
 * stays the last batched call's): a raster fault is PORRT_ERR_RASTER, a piece whose nodes carry different beliefs
 * PORRT_ERR_INVALID.  n_iterations < 2^31; iterations x distinct piece lengths <= 2^26. */
int64_t  porrt_bg_refine_policy(porrt_ctx *ctx, uint64_t n_iterations, double *xy, uint64_t *original_ids, int64_t *parents,
                                uint8_t *is_leaf, uint64_t cap, double *expected_costs);
/* The same on a policy given as host arrays, checked on the context's raster with its world validities: node i has state xy[2i..],
 * parent parents[i] (-1 for node 0, the root; children in ascending id order), original id original_ids[i] (passed through) and
 * belief vector beliefs[belief_row[i]] (n_belief_rows x n_worlds, n_worlds = porrt_n_worlds(ctx)).  Nodes not reached from node 0
 * belong to no piece and are dropped, as in the reference. */
int64_t  porrt_refine_policy(porrt_ctx *ctx, uint64_t n, const double *xy, const int64_t *parents, const uint64_t *original_ids,
                             const uint32_t *belief_row, const double *beliefs, uint32_t n_belief_rows, uint32_t n_worlds,
                             uint64_t n_iterations, double *out_xy, uint64_t *out_original_ids, int64_t *out_parents,
                             uint8_t *out_is_leaf, uint64_t cap, double *expected_costs);
/* seconds of the last refinement that filled its arrays: total (host and device) and the kernel alone (HIP events; 0 when no piece
 * has 3 nodes or n_iterations is 0) */
int      porrt_bg_get_refine_info(const porrt_ctx *ctx, double *total_s, double *device_s);

/* ---- the refinement of many policies in one call: decomposition, shortcuts, recomposition and expected costs on the device.
 * porrt_bg_refine_policies refines the policies of the context's last porrt_bg_extract_policies, porrt_mm_refine_policies those
 * of its last porrt_mm_extract_policies (an error when there is none, or once the graph, the belief graph or the expected costs
 * have changed since: the test of porrt_bg_get_policies / porrt_mm_get_policies).  Neither touches the policy that
 * porrt_bg_refine_policy / porrt_mm_refine_policy refines nor what porrt_bg_get_refine_info reports.
 * porrt_refine_policies takes n_policies policies laid end to end: policy q is rows pol_off[q] .. pol_off[q + 1] (pol_off[0] = 0) of
 * xy / parents / original_ids / belief_row, parents are indices WITHIN the policy (-1 for its row 0, children in ascending id
 * order), beliefs as in porrt_refine_policy; it is checked on the context's raster with its world validities.
 * Policy q's output equals, bit for bit, what porrt_refine_policy returns for policy q given alone -- states, original ids,
 * parents, leaf flags and expected cost, every quirk included (one-node pieces have no end, nodes not reached from row 0 are
 * dropped, pieces of <= 2 nodes are untouched, a fresh DiscreteSampler::new() per piece).
 * status[q]: 0 refined; 1 no policy to refine (the extraction's status was not 0, or an empty policy): no nodes, cost +0.0;
 * 2 a shortcut of this policy reads outside the raster, a door pixel without zone id or two zones on one segment (the single
 * call's PORRT_ERR_RASTER): no nodes; 3 a piece whose nodes carry different beliefs (the single call's PORRT_ERR_INVALID,
 * common.rs:102): no nodes.  A policy with nonzero status does not void the others; porrt_last_error names the first one.
 * ref_off (n + 1 entries), status and expected_costs are always written: refined policy q is rows ref_off[q] .. ref_off[q + 1] of
 * xy (2 per node) / original_ids / parents / is_leaf, parents[k] an index into the same policy (-1 for the root and for a piece
 * start left unconnected by the quirk).  The node arrays are written only if the total fits in cap; the total is never more than
 * the policies' nodes going in.  Returns the total, or a negative error, found on the host before any launch: PORRT_ERR_INVALID for
 * a parent out of range, a row 0 whose parent is not -1, a belief row out of range, n_iterations >= 2^31 or 2^31 nodes or more in
 * all; PORRT_ERR_CAPACITY for more than 2^26 draws (n_iterations x distinct piece lengths of the whole batch).
 * cap = 0 is the sizing call: it launches no shortcut kernel, so ref_off and status 0 / 1 / 3 are final, status 2 cannot show and
 * expected_costs are those of the policies as they went in.  n = 0 returns 0 and writes ref_off[0] = 0.
 * One upload, the decomposition (one wave per policy), one small download (the lengths of the pieces of >= 3 nodes: the draws are
 * made on the host, one table per distinct length of the whole batch), the shortcuts of every piece in one launch (longest first),
 * recomposition and costs (one wave per policy), one download, on the context's stream. */
int64_t  porrt_bg_refine_policies(porrt_ctx *ctx, uint64_t n_iterations, uint64_t *ref_off, uint8_t *status, double *expected_costs,
                                  double *xy, uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, uint64_t cap);
int64_t  porrt_mm_refine_policies(porrt_ctx *ctx, uint64_t n_iterations, uint64_t *ref_off, uint8_t *status, double *expected_costs,
                                  double *xy, uint64_t *belief_node_ids, int64_t *parents, uint8_t *is_leaf, uint64_t cap);
int64_t  porrt_refine_policies(porrt_ctx *ctx, uint64_t n_policies, const uint64_t *pol_off, const double *xy, const int64_t *parents,
                               const uint64_t *original_ids, const uint32_t *belief_row, const double *beliefs, uint32_t n_belief_rows,
                               uint32_t n_worlds, uint64_t n_iterations, uint64_t *ref_off, uint8_t *status, double *expected_costs,
                               double *out_xy, uint64_t *out_original_ids, int64_t *out_parents, uint8_t *out_is_leaf, uint64_t cap);
/* Counts and times of the context's last batch refinement: policies given, those with status 0, pieces of the policies that were
 * decomposed (status 0 or 2), the pieces of >= 3 nodes the shortcut launch took (0 when n_iterations or cap was 0), refined nodes
 * returned, distinct lengths among the pieces of >= 3 nodes; milliseconds of the shortcut launch (HIP events, 0 without one: what
 * porrt_bg_get_refine_info calls device_s) and of the whole call. */
struct porrt_refine_policies_info { uint64_t policies, ok, pieces, shortcut_pieces, nodes, distinct_lengths; double ms_device, ms_wall; };
int      porrt_refine_policies_info(const porrt_ctx *ctx, struct porrt_refine_policies_info *out);

/* ---- PTO::plan_belief_space (src/pto.rs:152-182) for many grown contexts of one device in one call: the second half of the loops
 * the reference's experiments run (main.rs:40-68: one map, one prior, a new sample stream per run), after porrt_grow_batch has
 * served the first.  Member q's answer is, bit for bit, what the same context gives alone through
 *     porrt_build_belief_graph(ctx, start_belief, n_worlds); porrt_bg_compute_expected_costs;
 *     porrt_bg_extract_policies with the one start 0; porrt_bg_refine_policies(refine_iterations) when refine_iterations > 0.
 * A helper context owned by ctxs[0] (the leader) adopts the disjoint union of the members' PTO graphs, gathered on the device, and
 * runs those stages once on it; no edge joins two members, so every member's costs and policy on the union are its own.
 * status[q]: the extraction's status (0 .. 4, as porrt_bg_extract_policies documents them; 1 covers a root without finite cost: no
 * final node, an incomplete final set after a PORRT_INCOMPLETE growth); expected_costs[q]: the root's cost; refine_status[q] and
 * refined_costs[q] (either may be NULL): those of porrt_bg_refine_policies, 1 and +0.0 when refine_iterations is 0.  Policy q is rows
 * pol_off[q] .. pol_off[q + 1] of xy (2 per node: the states) / original_ids (the member's OWN belief node ids, graph node *
 * n_beliefs + belief) / parents / is_leaf: the refined policy when refine_iterations > 0, the extracted one otherwise.  A member with
 * nonzero status contributes no rows and does not void the others; porrt_last_error(ctxs[0]) names the first.  pol_off (n_ctx + 1),
 * status and expected_costs are always written, the node arrays only if the total fits cap (cap = 0 sizes).  Returns the total number
 * of policy nodes, or a negative error.  n_ctx = 0 returns 0 and writes pol_off[0] = 0.
 * PORRT_ERR_INVALID before any launch (porrt_last_error(ctxs[0]) names the member): a NULL array or member, the same context twice,
 * members on different devices, a member without PTO results, n_worlds not the members' own, a prior that does not sum to 1,
 * members whose domain data differ from the leader's (W, H, low, up, the domain kind, the occupancy and zone bytes, the visibility:
 * compared on the host).  Goals, starts, seeds, batch_K and node counts may differ; the graphs may come from porrt_grow_batch or from
 * single porrt_grow calls.  An error of a stage (a raster fault of the visibility raycast, say) is the call's error.
 * The members stay as they are: their trees and any belief graph, costs, policies or refinements they hold are neither read as
 * results nor changed (the host copies of their trees may be fetched).  The answers are snapshots kept on the leader:
 * porrt_plan_batch_get_policies and porrt_plan_batch_info hand them out again, a later regrowth of a member does not invalidate them.
 * Members are taken in order into a pass -- one union -- while the sum of their nodes x n_beliefs stays at or below option
 * "plan_batch_max_belief_nodes" (default 2^22, at most 2^32 - 2); a member that alone exceeds it runs alone.  The answers do not
 * depend on the cut, the time does: a level of a pass's cost sweeps goes on until its slowest member's costs stand, and small passes
 * pay a pass's fixed costs more often (BASELINE.md has the measurement behind the default).  PORRT_ERR_CAPACITY when a pass's device buffers cannot be allocated (never a truncated answer).
 * porrt_plan_batch_get_expected_costs copies member `member`'s cost vector (its nodes x n_beliefs doubles, what
 * porrt_bg_get_expected_costs gives for the context alone) from the device: members of the LAST pass only, PORRT_ERR_INVALID
 * otherwise.  All three getters are an error before the first successful call.  The dynamic programming's schedule and
 * "policy_max_nodes" are read from the leader's options; "plan_batch_host_ranks" (default 1) takes the adjacency order's kd ranks
 * from the members' host kd-trees, 0 makes them on the device, a workgroup per member.
 * Info: counts summed over the passes (graph nodes and edges, belief nodes and edges, final belief nodes, members with status 0,
 * policy nodes returned) and milliseconds: the whole call, gathering the union (with its download), the adjacency order (ranks
 * included), the belief graph, the costs, the policy walk, the refinement -- host clock around stages that end in a synchronise --
 * and the HIP-event times those stages report themselves, summed. */
int64_t  porrt_plan_belief_space_batch(porrt_ctx *const *ctxs, uint32_t n_ctx, const double *start_belief, uint32_t n_worlds,
                                       uint64_t refine_iterations, uint64_t *pol_off, uint8_t *status, double *expected_costs,
                                       uint8_t *refine_status, double *refined_costs, double *xy, uint64_t *original_ids, int64_t *parents,
                                       uint8_t *is_leaf, uint64_t cap);
int64_t  porrt_plan_batch_get_policies(const porrt_ctx *leader, uint64_t *pol_off, double *xy, uint64_t *original_ids, int64_t *parents,
                                       uint8_t *is_leaf, uint64_t cap);
int      porrt_plan_batch_get_expected_costs(const porrt_ctx *leader, uint32_t member, double *out);
struct porrt_plan_batch_info {
    uint64_t members, passes, graph_nodes, graph_edges, beliefs, belief_nodes, belief_edges, final_belief_nodes, policies_ok, policy_nodes;
    double ms_wall, ms_join, ms_edge_order, ms_belief_graph, ms_costs, ms_policies, ms_refine, ms_device;
};
int      porrt_plan_batch_info(const porrt_ctx *leader, struct porrt_plan_batch_info *out);

/* ---- MapShelfDomainTampPRM::plan (map_shelves_tamp_prm.rs:310-326) followed by PartialShortCut(refine_iterations), for n_plans
 * problems on the context's map in one call: what main_baseline_comparison (main.rs:100-166) runs n_runs times per problem size, and
 * what a replanner runs from many candidate starts and priors after an observation.  Plan p is, bit for bit, what a fresh context
 * with the same raster, zones and sampler box gives after porrt_set_sampler(.., sampler_seeds[p]), porrt_set_discrete_seed(
 * discrete_seeds[p]), porrt_mm_plan(starts + 2 p, priors + n_worlds p, ..) and, when refine_iterations > 0, porrt_mm_refine_policy:
 * the extraction's status and the root's expected cost, the refinement's status and cost, the policy's states, ids (the plan's OWN
 * belief node ids: mode offset + roadmap node), parents and leaf flags, the plan's whole cost vector and its counts.  The zone
 * sampler is a fresh seed-0 stream per plan, as per single call.  sampler_seeds NULL: every plan clones the context's current
 * continuous state; discrete_seeds NULL: every plan starts from a copy of the context's current discrete state (whatever
 * sampler_seeds says).  The context's samplers are not advanced, and its last single
 * growth, belief graph, costs and policy stay valid: a helper context owned by ctx carries the work.
 * How: every mode of a plan clones the planner's never-advanced sampler, so the k-th random point of any mode of plan p is one
 * point P_p[k].  The host runs grow_mm_prm's loop per plan (up to 8 threads) recording 32-bit codes -- an index into P_p or one of
 * the explicit points (start, goal states, observation samples) -- and draws P_p once; the device expands them (k_mm_points), builds
 * every roadmap of a pass in one launch sequence, the belief graph of the union, the expected costs, the policies from the plans'
 * first nodes and their refinements.  Plans are taken in order into a pass while the sum of their roadmap nodes stays at or below
 * option "mm_plan_batch_max_nodes" (default 2^23, at most 2^31 - 2); a plan that alone exceeds it is a pass of its own.  The answers
 * do not depend on the cut.
 * status[p]: that of porrt_mm_extract_policies, 0 .. 4 (1: the root has no finite cost: no rows, the other plans stand);
 * refine_status / refined_costs (either may be NULL) as porrt_plan_belief_space_batch gives them (1 and +0.0 when refine_iterations is
 * 0).  Policy p is rows pol_off[p] .. pol_off[p + 1].  pol_off (n_plans + 1), status and expected_costs are always written, the node
 * arrays only if the total fits cap (cap = 0 sizes).  Returns the total number of policy nodes, or a negative error.
 * PORRT_ERR_INVALID before any launch (porrt_last_error names the plan): n_plans outside 1 .. 65536, NULL starts / priors / pol_off /
 * status / expected_costs, n_worlds not the context's, no shelf domain with zones, a prior that does not sum to 1 (summed as
 * porrt_grow_mm_prm sums it), a belief without mass in a mode tree, a mode's belief that is not reachable.  PORRT_ERR_CAPACITY: an
 * allocation that fails, or a pass of 2^31 nodes, 2^32 edges or 2^32 pairs; never a truncated answer.  A raster fault fails the call.
 * porrt_mm_plan_batch_get_policies hands the kept answers out again; porrt_mm_plan_batch_get_expected_costs copies plan `plan`'s cost
 * vector (its nodes doubles: what porrt_mm_get_expected_costs gives for the plan alone), plans of the LAST pass only;
 * porrt_mm_plan_batch_get_plan the plan's counts (modes, transitions, reachable beliefs, roadmap nodes = belief nodes, forward roadmap
 * edges, belief edges, final belief nodes) and the pass it ran in.  All four getters are an error before the first successful call.
 * Info: sums over the passes, and milliseconds: the whole call, the host's mode trees and union tables, the points (uploads and
 * k_mm_points), the roadmaps, the belief graph, the costs, the policy walk, the refinement -- host clock around stages that end in a
 * synchronise -- and the HIP-event times those stages report themselves, summed. */
int64_t  porrt_mm_plan_batch(porrt_ctx *ctx, uint32_t n_plans, const double *starts, const double *priors, const uint64_t *sampler_seeds,
                             const uint64_t *discrete_seeds, uint32_t n_worlds, double max_step, double search_radius,
                             uint64_t n_iter_per_belief, uint64_t refine_iterations, uint64_t *pol_off, uint8_t *status, double *expected_costs,
                             uint8_t *refine_status, double *refined_costs, double *xy, uint64_t *original_ids, int64_t *parents,
                             uint8_t *is_leaf, uint64_t cap);
int64_t  porrt_mm_plan_batch_get_policies(const porrt_ctx *ctx, uint64_t *pol_off, double *xy, uint64_t *original_ids, int64_t *parents,
                                          uint8_t *is_leaf, uint64_t cap);
int      porrt_mm_plan_batch_get_expected_costs(const porrt_ctx *ctx, uint32_t plan, double *out);
struct porrt_mm_batch_plan {
    uint64_t modes, transitions, beliefs, nodes, forward_edges, belief_edges, finals, pass;
};
int      porrt_mm_plan_batch_get_plan(const porrt_ctx *ctx, uint32_t plan, struct porrt_mm_batch_plan *out);
struct porrt_mm_plan_batch_info {
    uint64_t plans, passes, modes, transitions, nodes, prefix_points, explicit_points, forward_edges, belief_edges, finals, policies_ok, policy_nodes,
             upload_bytes;
    double ms_wall, ms_host, ms_points, ms_roadmaps, ms_belief_graph, ms_costs, ms_policies, ms_refine, ms_device;
};
int      porrt_mm_plan_batch_info(const porrt_ctx *ctx, struct porrt_mm_plan_batch_info *out);

/* ---- the other strategy: PTOPolicyRefiner::refine_solution(RefinmentStrategy::Reparent(radius)) (pto_policy_refiner.rs:209-322), of
 * one policy or many in one call, on the device.  Per piece of the policy (the decomposition above): build_tree makes the piece's path
 * a tree and adds belief-graph offsprings within `radius` of a path node; reparent pops the tree's nodes by distance from the root and
 * hangs every valid neighbour within 0.5 * radius (is_transition_valid under the belief of the piece's first node) under the popped
 * node when that is strictly shorter; recompose takes the chain from the piece's last path node up to the root.  States never move: a
 * recomposed node is a belief-graph node, original_ids[k] is ITS id and the expected cost uses ITS belief; a piece may come out shorter
 * or longer than it went in, so the output is not bounded by the input.  What reads like mistakes in the reference is reproduced (an
 * offspring is measured from the path node and its edge costs that distance; a grandchild is never tested itself, its children are and
 * hang from its parent; the visited filter at push time; the upward sum `cost += link.cost` recomputed on every use; priorities of a
 * reparented node's descendants stay stale; the one-node quirk above).
 * OURS, NOT THE REFERENCE'S, because the reference's text does not pin them (its queue orders priorities with an Ord that never says
 * Equal, common.rs:231-253, so bit-equal priorities pop in whatever order the priority_queue crate's heap leaves them):
 *   - among bit-equal priorities the node with the LOWEST TREE ID is popped (tree ids: the path in order, then offsprings as added);
 *   - a push on a node in the queue replaces its priority, higher or lower; on a node already popped it inserts it again (the crate's
 *     documented push, recalled, not verified);
 *   - no kd-tree is built: the order of a node's neighbours only orders the pushes of one pop, which changes nothing under these rules;
 *   - two caps that make a policy fail loudly, per piece and independent of what else the call holds: option
 *     "reparent_max_tree_nodes" (C, default 16384, 1 .. 2^15): a tree of more than C nodes, more than 16 C entries in build_tree's FIFO
 *     at a time, or more than 256 C pairs of tree nodes within 0.5 * radius of each other are status 4; more pops than
 *     "reparent_max_pops_per_node" (default 64, 1 .. 64) x the tree's nodes are status 5 (the loop is believed to end, not proven to).
 *
 * porrt_bg_reparent_policies works on the policies of the last porrt_bg_extract_policies, under the staleness rule of
 * porrt_bg_refine_policies.  status[q]: 0 refined; 1 nothing to refine; 2 a transition check reads outside the raster, a door pixel
 * without zone id or two zones on one segment (every node's checks are made, as every node is popped at least once); 3 a piece whose
 * input nodes carry different beliefs; 4 and 5 the caps.  Precedence: 3, then over the policy's pieces 4, 2, 5.  A policy with nonzero
 * status has no nodes and cost +0.0 and does not void the others; porrt_last_error names the first.  The call always does the device
 * work and keeps the result on the context; it writes ref_off (n + 1), status and expected_costs, returns the total number of nodes
 * and writes the node arrays only when cap holds the total.  porrt_bg_get_reparented_policies hands the kept result out again without
 * recomputing (an error when there is none or once the graph, the belief graph or the expected costs have changed).
 * porrt_bg_reparent_policy refines the policy of the last porrt_bg_extract_policy: a batch of one through the same path with a result
 * of its own; status 2 is PORRT_ERR_RASTER, 3 PORRT_ERR_INVALID, 4 and 5 PORRT_ERR_CAPACITY; the arrays are written when cap holds them.
 * porrt_reparent_policies is the explicit form: the belief graph as host arrays (node g: state xy[2g..], belief vector
 * beliefs[belief_row[g]], children child_ids[child_off[g] .. child_off[g + 1]] in list order, as porrt_extract_policies takes them),
 * the policies laid end to end (pol_off; original_ids = belief-graph node ids, parents within the policy, -1 for its row 0); states
 * and beliefs come from the graph; checked on the context's raster with its world validities.  PORRT_ERR_INVALID before any launch for
 * an id, child or parent out of range, non-finite states, n_worlds != porrt_n_worlds(ctx), or a radius that is negative, NaN or
 * infinite.  radius = 0.0 is legal: only zero-distance children and copies take part. */
int64_t  porrt_bg_reparent_policies(porrt_ctx *ctx, double radius, uint64_t *ref_off, uint8_t *status, double *expected_costs, double *xy,
                                    uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, uint64_t cap);
int64_t  porrt_bg_get_reparented_policies(const porrt_ctx *ctx, uint64_t *ref_off, uint8_t *status, double *expected_costs, double *xy,
                                          uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf, uint64_t cap);
int64_t  porrt_bg_reparent_policy(porrt_ctx *ctx, double radius, double *xy, uint64_t *original_ids, int64_t *parents, uint8_t *is_leaf,
                                  uint64_t cap, double *expected_costs);
int64_t  porrt_reparent_policies(porrt_ctx *ctx, uint64_t n_nodes, const double *xy, const uint32_t *belief_row, const double *beliefs,
                                 uint32_t n_belief_rows, uint32_t n_worlds, const uint64_t *child_off, const uint32_t *child_ids,
                                 uint64_t n_policies, const uint64_t *pol_off, const uint64_t *original_ids, const int64_t *parents,
                                 double radius, uint64_t *ref_off, uint8_t *status, double *expected_costs, double *out_xy,
                                 uint64_t *out_original_ids, int64_t *out_parents, uint8_t *out_is_leaf, uint64_t cap);
/* Counts and times of the context's last porrt_bg_reparent_policies or porrt_reparent_policies: policies given, those with status 0,
 * pieces worked on, tree nodes in all and of the largest tree, valid-neighbour pairs, pops, reparents, nodes returned, rounds (of as
 * many pieces as the scratch budget holds); milliseconds per stage (HIP events: build_tree, the neighbour relation, the pop loops,
 * recomposition with costs) and of the whole call. */
struct porrt_reparent_policies_info {
    uint64_t policies, ok, pieces, tree_nodes, max_tree, pairs, pops, reparents, nodes, rounds;
    double ms_tube, ms_neighbours, ms_pop, ms_recompose, ms_wall;
};
int      porrt_reparent_policies_info(const porrt_ctx *ctx, struct porrt_reparent_policies_info *out);

/* ---- the QMDP policy extractor: QMdpPolicyExtractor (src/qmdp_policy_extractor.rs) on the graph of the last
 * porrt_grow(mode PORRT_MODE_PTO) of this context -- no belief graph: one cost-to-goal field per world and a greedy walk.
 *
 * porrt_qmdp_plan is plan_qmdp (qmdp_policy_extractor.rs:23-35): for every world w, cost_to_goals[w] = dijkstra
 * (pto_graph.rs:275-303) over PTOGraphWorldView{world: w} (pto_graph.rs:245-271: a node is relaxed only where its own validity
 * has the world) from Reachability::get_final_nodes_for_world(w) (pto_reachability.rs:58-63).  All worlds are solved in one set
 * of device sweeps over cost planes interleaved per node; any evaluation order ends in the reference's fixpoint, bit for bit.
 * The costs stay on the device.  PORRT_ERR_INVALID with "We should have final node ids for each world" when a world has no final
 * node (:28-30), or when the context holds no PTO graph.  get_policy_graph (pto_graph.rs:363-419) is porrt_qmdp_policy_graph below. */
int      porrt_qmdp_plan(porrt_ctx *ctx);
/* out[w * N + id] = cost_to_goals[w][id], n_worlds * N doubles, N = porrt_num_nodes(ctx); +inf where no final node of w is reached */
int      porrt_qmdp_get_costs(const porrt_ctx *ctx, double *out);
/* Counts and times of the last porrt_qmdp_plan and the last porrt_qmdp_react after it: nodes, edges (adjacency entries: every
 * PTO edge counts both ways), worlds, sweeps, queries; milliseconds on the device (HIP events) and wall for each, and of the
 * nearest-node searches of the react call.  C++ callers write `struct porrt_qmdp_info` (the name is the function's too). */
struct porrt_qmdp_info { uint64_t nodes, edges, worlds, sweeps, queries; double ms_plan_device, ms_plan_wall, ms_react_device, ms_react_wall, ms_nearest; };
int      porrt_qmdp_info(const porrt_ctx *ctx, struct porrt_qmdp_info *out);
/* react_qmdp (qmdp_policy_extractor.rs:38-49) for n queries in one call.  Query q: kd_start = the nearest graph node of
 * starts[2q..] (nearest_neighbor.rs:48-91, all nodes, on the host); get_common_path (:65-87) follows get_best_expected_child
 * (:90-108: the first child of strictly least sum over the worlds of cost[w][child] * belief[w], summed in world order; a NaN
 * -- inf * 0.0 -- or +inf never wins, and without a winner the walk goes to node 0 with cost +inf) while the accumulated norm2 is
 * below common_horizons[q] and the last expected cost is above 0; then for every world get_path (:51-62) follows get_best_child
 * (:110-123: the first child of strictly least cost[w][child]) from the node the common path ended on while its cost is above 0.
 * The node a walk ends on is not part of it.  paths[w] of query q = common path ++ get_path: rows path_off[q * n_worlds + w] ..
 * path_off[q * n_worlds + w + 1] of path_xy, the first common_len[q] of them the common path.  path_off (n * n_worlds + 1) and
 * common_len (n) are always written; the states only if the total fits cap (counted in states); the return value is the total.
 * n = 0 returns 0 and writes path_off[0] = 0.
 * Errors (PORRT_ERR_INVALID): n_worlds != porrt_n_worlds(ctx) ("belief state size should match the number of worlds", :66-68);
 * no porrt_qmdp_plan since the last growth on the context; a walk that would emit more than option "qmdp_max_states" states
 * (default 1 << 16) -- the reference does not terminate on such input (a walk parked on node 0 with nothing finite below it, a
 * zero-length hop between duplicates); porrt_last_error names the query and the world. */
int64_t  porrt_qmdp_react(porrt_ctx *ctx, const double *starts, const double *beliefs, uint32_t n_worlds, const double *common_horizons,
                          uint64_t n, uint64_t *path_off, uint64_t *common_len, double *path_xy, uint64_t cap);
/* plan_qmdp's costs on an explicit graph given as host arrays (the form of the reference's dijkstra tests, pto_graph.rs:626-678):
 * node i has state xy[2i..] and validity validities[node_validity[i]] (one word of world bits each, n_worlds <= 64), children as
 * CSR in push order, and world w has the final nodes final_ids[final_off[w] .. final_off[w + 1]].  out[w * n + id].  A world
 * without finals is all +inf (pto_graph.rs:658-667).  No context needed. */
int      porrt_qmdp_costs(int device, uint64_t n, const double *xy, const uint32_t *node_validity, const uint64_t *validities,
                          uint32_t n_validities, uint32_t n_worlds, const uint64_t *child_off, const uint32_t *child_ids,
                          const uint64_t *final_off, const uint64_t *final_ids, double *out);

/* ---- get_policy_graph (pto_graph.rs:363-419; QMdpPolicyExtractor::get_policy_graph, qmdp_policy_extractor.rs:125-127): the PTO
 * graph pruned to the edges that are the right decision under some belief.  For an adjacency entry (u, t): V = the worlds where
 * cost_to_goals[w][t] is finite; one row per entry o of children(u) with o != t (by id; duplicates give duplicate rows):
 * d_o[w] = cost[w][t] - cost[w][o] for w in V, 0 where cost[w][o] is +inf (the reference leaves the term out).  The entry is kept iff
 * some b >= 0 on V with sum b = 1 has d_o . b <= 0 for every o, i.e. the game value v* = min_b max_o d_o . b is <= 0.  The cost of
 * the edge u -> t itself is not in the LP (the reference's rule).  Every decision is taken on the original graph.
 * how[e], one byte per entry in push order (kept iff 1, 3 or 5):
 *   0 V empty: pruned.   1 some world w of V has d_o[w] <= 0 for all o: kept.   2 some rival has d_o[w] > 0 on all of V: pruned.
 *   3 / 4  the f64 simplex of DESIGN.md section 26 (Bland's rule, serial sums in world order, no contraction) reached
 *          v <= PORRT_POLICY_GRAPH_TOL * scale: kept / stopped at an optimum above it: pruned; scale = max |d_o[w]| of the entry.
 *   5 option "policy_graph_max_pivots" (default 4096) used up: undecided, kept -- pruning happens only on proof.
 * PORRT_POLICY_GRAPH_TOL is this interface's own tolerance (the reference solves through the minilp crate, whose tolerances are its
 * own): the f64 value is within 1e-12 * scale of the exact one on the inputs of tests/test_policy_graph_cpu.py, and an entry with
 * 0 < v* <= 2 * TOL * scale (a tie in exact arithmetic that rounding of the costs opened) may go either way.
 * PORRT_POLICY_GRAPH_EPS: multipliers, rates and pivot elements below it (relative) count as zero inside the simplex. */
#define PORRT_POLICY_GRAPH_TOL 1e-9
#define PORRT_POLICY_GRAPH_EPS 1e-13
/* Counts: entries, kept, entries per how value, residual (entries that went to the simplex), pivots in total and the most of one
 * entry.  Milliseconds on the device (HIP events) and wall for the three passes: classify (how 0-2), simplex, compaction. */
struct porrt_policy_graph_info {
    uint64_t entries, kept, how[6], residual, pivots_total, pivots_max;
    double ms_classify_device, ms_classify_wall, ms_simplex_device, ms_simplex_wall, ms_compact_device, ms_compact_wall;
};
/* On the graph and the costs of the last porrt_qmdp_plan of this context.  PORRT_ERR_INVALID without a porrt_qmdp_plan since the
 * last growth (the rule of porrt_qmdp_react). */
int      porrt_qmdp_policy_graph(porrt_ctx *ctx);
/* The result of the last porrt_qmdp_policy_graph; any pointer may be NULL.  keep, how: one byte per adjacency entry of the original
 * graph in push order (2 * edges).  child_off (N + 1) / child_ids (kept entries): the pruned children lists in push order.
 * parent_off / parent_ids: the pruned parents lists -- parents[x] of a PTO graph has the order of children[x], and its entry p
 * survives iff the entry (p, x) survived (remove_edge, pto_graph.rs:214-217). */
int      porrt_qmdp_policy_graph_get(const porrt_ctx *ctx, uint8_t *keep, uint8_t *how, uint64_t *child_off, uint32_t *child_ids,
                                     uint64_t *parent_off, uint32_t *parent_ids);
int      porrt_qmdp_policy_graph_info(const porrt_ctx *ctx, struct porrt_policy_graph_info *out);
/* The same decision on explicit host arrays (the form of the reference's tests, pto_graph.rs:574-623), no context: children as CSR
 * in push order, costs[w * n + id].  keep, how: child_off[n] bytes each; keep, how and info may be NULL.  Children only: the push
 * order of the parents lists cannot be recovered from a children CSR.  PORRT_ERR_INVALID for a NaN or -inf cost, an id >= n, or
 * n_worlds outside 1 .. 64.  max_pivots is fixed at the default here. */
int      porrt_policy_graph(int device, uint64_t n, uint32_t n_worlds, const uint64_t *child_off, const uint32_t *child_ids,
                            const double *costs, uint8_t *keep, uint8_t *how, struct porrt_policy_graph_info *info);

/* ---- measurement */
typedef struct {
    uint64_t n_iter;          /* iterations run */
    uint64_t n_nodes;         /* tree size incl. root */
    uint64_t n_steps;         /* batched steps launched */
    uint64_t n_tie_fallbacks; /* equal-cost parent ties not covered by the goal-path rule (expected 0) */
    double   total_s;         /* wall time of porrt_grow */
    double   setup_s;         /* part of total_s: host tables + uploads (radius table, worlds) */
    double   device_s;        /* HIP-event time from first to last kernel of the growth loop */
    double   scan_s;          /* HIP-event time summed over the near-search kernel (NN + steer + radius search;
                                 only filled when profiling is enabled) */
    uint64_t scan_launches;
    double   scan_pairs;      /* sample x node pairs those searches answer (2 * K * N_b per step) */
    double   scan_bytes;      /* algorithmic bytes of those searches */
    double   connect_s;       /* HIP-event time summed over the connect kernel (profiling only) */
} porrt_metrics;
int porrt_get_metrics(const porrt_ctx *ctx, porrt_metrics *out);
/* options: "profile" (0/1 per-kernel HIP events), "cand_cap" (initial neighbour-list
 * capacity per sample), "edge_per_node" and "tie_pool_ids" (TEST SEAMS, the same kind of initial capacity: the PTO edge pool holds
 * (n_iter_max + 2) * edge_per_node + 4096 edges, 1 .. 65536, default 256; the pool of deferred equal-cost parents holds tie_pool_ids
 * node ids, 1 .. 2^30, or with the default 0 max(2^20, 16 * n_iter_max); a porrt_grow whose pool overflows multiplies the one in
 * force by 4 and runs again, see "Replays" below; a context that has grown before keeps its larger edge buffers),
 * "graph" (0/1 replay the growth loop as a hipGraph), "kd_group" (steps whose
 * new nodes enter the tie-order structure together; 0 = chosen from batch_K), "group_lanes" (RRT*
 * step kernels: 16 / 32 / 64 lanes per sample, 0 = one wave per sample, -1 = chosen from the number
 * of contexts advanced together), "batch_streams" (on the FIRST context of a porrt_grow_batch: the
 * sub-batches it advances side by side, each on its own streams; 0 = 2 from 32 contexts on, else 1),
 * "pipeline" (RRT* steps of the one-wave-per-sample kernels, i.e. of a single query: 0 = search, connect, commit one after the
 * other; 1 = step b + 1 is searched while step b is connected, in one launch, the filing and the rewire commit in a second;
 * 4 (default) = ONE launch per step: the filing of a step's nodes and its rewire commit run beside the next step's kernels
 * (batch_K <= 1024, else as 1); 2 = all steps in one persistent cooperative launch with barriers over the grid (measured: far
 * slower on eight XCDs, kept for the record), "kd_after" (1 = the tie-order structure is built after the last step instead of
 * beside the steps: measured slower), "kd_lazy" (RRT*, batches and the default form of a single query: 1 (default; 2 is accepted and means the same) =
 * beside the steps only the goal path of the reference's kd-tree is kept -- it orders every tie between copies of the goal point and
 * their parent -- and the whole structure is built after the steps in the rare run where two other nodes tie; 0 = the whole structure
 * beside the steps on a second stream), "kd_claim_threads", "kd_ride", "kd_inline", "early_wave_steps", "dp_sweeps", "dp_wide_rows" (the layered
 * expected costs sweep a level of N * W rows with the wide kernel when N * W >= this, with the split one otherwise; default 2 << 20,
 * 0 = every level wide), "conn_wg_waves" (the group kernels' connect pass: 1, default: k_conn2 with one wave per workgroup, so that a finished
 * wave gives back its slot and its LDS lists whatever its neighbours still do, and the step's single workgroups -- page filing, goal-point copies,
 * goal path -- as k_conn2_riders, a kernel of its own on the same stream; 4 = everything in one kernel of four-wave workgroups, k_conn2_wg4),
 * "conn_riders_first" (1, default: k_conn2_riders before k_conn2 of its step; 0 = after it), "riders_fast" (developer option: 1, default: the
 * step's single workgroups in their short forms -- the page filing and the goal path with their loads in one round trip, the goal copies' radius
 * search by all four waves; 0 = the forms they had beside a long connect pass; 0 or 1), "nn_wg_waves" (waves per workgroup of k_nn2: 4,
 * default, or 1), "commit_flat" (the group kernels' rewire commit: 1, default: a workgroup takes 128 consecutive samples of its row and runs one
 * lane per candidate record -- k_nn2's commit workgroups and k_commit_flat after the last step; 0 = a group of lanes per sample, k_commit2 after
 * the last step), "compact_rows" (1, default: a
 * porrt_grow_batch whose members end at different steps launches its later steps on the members that still have work), "gtrack_side" (1 = a single query's goal-path workgroup as a kernel
 * of its own on the side stream; measured slower, 0 is the default: a workgroup of the step kernel), "box_table"
 * (1, default: the group and roadmap kernels answer "is this segment free" from a summed-area table of the raster when the bounding
 * box of its end pixels holds free pixels only, and walk it otherwise; 0 = always walk), "prm_rows" (porrt_prm_plan_paths: rows of
 * costs swept together in one pass, 1 .. 4096, default 256), "prm_xcd_rows" (1, default: a row's sweep workgroups are placed together
 * on one XCD; 0 = the plain grid order).  None of them changes a result.  "qmdp_max_states" (porrt_qmdp_react: a walk that would emit
 * more states than this is an error, 1 .. 2^31 - 1, default 1 << 16) is a safety bound: the reference does not terminate there.
 * "policy_graph_max_pivots" (porrt_qmdp_policy_graph: an entry whose simplex would need more pivots is left undecided and kept, how 5;
 * 0 .. 2^31 - 1, default 4096) is a bound of the same kind: no entry of the measured graphs came near it.  "policy_max_nodes" (porrt_bg_extract_policies,
 * porrt_mm_extract_policies: a policy that would have more nodes is status 4, 1 .. 2^24, default 1 << 16) is one too.
 * "refine_short_lds" (the batch refiner, default 1: the pieces of <= 256 nodes run in a launch of their own whose waves take 4 KiB
 * of LDS instead of 16; 0 = every piece in one launch; the results are the same bits).
 * "draw_max_fragments" (a canvas made after it is set: the fragments of one pass of a draw call, 1 .. 2^30, default 2^24 -- two arrays of
 * 8-byte records, 256 MiB; a call with more runs in several passes over consecutive lines, a single longer line in a pass of its own) and
 * "draw_heavy_cap" (a pixel with more records than this in a pass is ordered by one wave -- up to 64 records -- or by a workgroup through LDS
 * instead of by one lane, 1 .. 1024, default 16; the workgroup sorts 1024 records a trip) are TEST SEAMS at small values, like cand_cap: the image is the same bits. */
int porrt_set_option(porrt_ctx *ctx, const char *name, int64_t value);
/* what was in force: "launch_mode" (the last porrt_grow_batch led by this context: 0 = one launch sequence, G = G sequences side by
 * side on streams chosen by measurement, -G = G sequences on the contexts' own streams -- the probe found no parallel set, e.g. under a
 * profiler that serialises kernels), "pipeline", "group_lanes", "kd_lazy", "kd_built_after" (1: a tie of the last grow -- of the batch
 * this context led -- needed the whole kd structure, which was built after its steps), "kd_lca_steps" (this context's own need: 1 + the
 * last step with a tie that took that structure, 0 = none), "kd_forms_run" (which forms of the kd side chain the last grow -- of the batch this
 * context led -- launched, for tests that must know what they covered; a grow that replays a captured sequence reports its capture's.  Bits 0 .. 10: the
 * instantiation of k_kd_claim -- 0: <2048> and 1: <4096>, one row with the engine's workgroup; 2 .. 9: one workgroup per row, nodes x threads 1024 x 256,
 * 1024 x 512, 1024 x 1024, 2048 x 256, 2048 x 512, 2048 x 1024, 4096 x 512, 4096 x 1024; 10: a single query's side stream, the new nodes' coordinates in
 * LDS.  11: k_kd_locate with one thread per node, 12: with one wave per node.  13: a group's hints and the deferred ties rode in the next group's locate
 * kernel.  14: k_kd_hint and 15: k_kd_hint_fix after a group's claim.  16: k_tie_fix on the side stream after a group, beside the steps.  17: groups
 * launched after the steps, by "kd_after" or because a tie asked under "kd_lazy"), "compactions" (how often the last batch this context led gathered the
 * members still running), "n_heavy" (samples of this context's last grow with more hits than their LDS list holds: served by a whole wave
 * from the lists in memory), "conn_wg_waves", "conn_riders_first", "riders_fast", "tim0" .. "tim15" (developer builds with -DPORRT_TIMING: the phase
 * timers of this context's last growth, 0 otherwise), "nn_wg_waves", "commit_flat", "cand_cap" (the neighbour-list capacity in force: larger than what was set after a call whose lists overflowed and which was replayed),
 * "edge_per_node" and "tie_pool_ids" (likewise: what the last attempt ran with; tie_pool_ids stays 0 while the default pool is in force),
 * "tie_pooled_ids" and "tie_records" (the last growth's last attempt: node ids that deferred ties asked the pool for, and their records), "dp_wide_rows", "dp_levels" and "dp_wide_levels" (the levels of the last layered expected costs, 0 when the
 * general sweeps ran; bit k of the mask: level k -- k-th smallest number of possible worlds -- ran the wide kernel) */
int porrt_get_option(const porrt_ctx *ctx, const char *name, int64_t *value);

/* Device arithmetic self-test: sqrt and divide of n doubles on the GPU versus the host's correctly
 * rounded results; both mismatch counts must be 0 for bit-exact parity (rrt.rs costs, common.rs:218). */
int porrt_selftest(porrt_ctx *ctx, uint64_t n, uint64_t *sqrt_mismatch, uint64_t *div_mismatch);

/* ---- multi-modal PRM growth: MapShelfDomainTampPRM::grow_mm_prm (src/map_shelves_tamp_prm.rs:328-393; ModeTree :135-283,
 * sample_observation_of_zone :482-493) on a shelf domain with zones.  One PRM* roadmap per mode (belief); the reference's loop
 * decides on the host which point goes to which mode in which order (the context's discrete sampler moves on; every mode
 * clones the continuous sampler's current state, which is NOT advanced -- the reference's behaviour; the zone sampler is a
 * fresh seed-0 stream per call), then each mode's roadmap is built at once on the GPU from its ordered points.  Results:
 * per mode its belief, reaching probability, nodes (add_sample order), forward edges (neighbour -> new node, the reference's
 * adjacency order; the reverse edge is implied, prm.rs:96-103) and final node ids; per transition the observed zone, the two
 * modes, the observation flag as the reference stores it and the [node in from-mode, node in to-mode] pairs.  After this
 * call the single-graph getters (porrt_get_tree ...) have no results. */
int      porrt_grow_mm_prm(porrt_ctx *ctx, const double start[2], const double *initial_belief, uint32_t n_worlds, double max_step,
                           double search_radius, uint64_t n_iter_per_belief);
uint64_t porrt_mm_num_modes(const porrt_ctx *ctx);
uint64_t porrt_mm_num_transitions(const porrt_ctx *ctx);
uint64_t porrt_mm_num_beliefs(const porrt_ctx *ctx);          /* reachable belief states of the prior (the sample budget's factor) */
int      porrt_mm_get_mode(const porrt_ctx *ctx, uint64_t mode, double *belief /* n_worlds */, double *reaching_probability, uint64_t *n_nodes,
                           uint64_t *n_edges, uint64_t *n_final);
int      porrt_mm_get_mode_graph(const porrt_ctx *ctx, uint64_t mode, double *xy, uint32_t *edge_from, uint32_t *edge_to, uint64_t *final_ids);
int      porrt_mm_get_transition(const porrt_ctx *ctx, uint64_t t, uint32_t *zone, uint32_t *from_mode, uint32_t *to_mode, int *observation, uint64_t *n_pairs);
int      porrt_mm_get_transition_pairs(const porrt_ctx *ctx, uint64_t t, uint64_t *pairs /* 2 * n_pairs */);
int      porrt_mm_get_seconds(const porrt_ctx *ctx, double *host_s, double *roadmap_s, double *device_s);

/* ---- the rest of MapShelfDomainTampPRM::plan (map_shelves_tamp_prm.rs:310-326) on the modes of the last porrt_grow_mm_prm.
 * porrt_mm_build_belief_graph: build_belief_graph (:395-473) on the device.  Belief node id = mode_offsets[m] + roadmap node
 * (node 0 = the planning start); every node carries its mode's belief and the belief id of that belief (its index in
 * reachable_belief_states, the key get_best_expected_children clusters by, belief_graph.rs:229-236); observation edges (transition
 * pairs, in order; their from nodes become Observation nodes) come before action edges (roadmap children of the nodes that are not
 * Observation nodes, PTONode::children order); children and parents lists are in add_edge order.  Finals: each mode's
 * final_node_ids, in mode order.  A pair naming a node its mode does not have (the reference panics) is PORRT_ERR_INVALID.
 * porrt_mm_bg_get_graph: any pointer may be NULL; child_off / parent_off hold num_nodes + 1 entries, mode_offsets num_modes + 1. */
int      porrt_mm_build_belief_graph(porrt_ctx *ctx);
uint64_t porrt_mm_bg_num_nodes(const porrt_ctx *ctx);
uint64_t porrt_mm_bg_num_edges(const porrt_ctx *ctx);
uint64_t porrt_mm_bg_num_finals(const porrt_ctx *ctx);
int      porrt_mm_bg_get_graph(const porrt_ctx *ctx, uint64_t *child_off, uint32_t *child_ids, uint64_t *parent_off, uint32_t *parent_ids,
                               uint8_t *types, uint32_t *belief_ids, uint64_t *mode_offsets, uint64_t *finals);
/* compute_expected_costs_to_goals (:475-477): conditional_dijkstra (belief_graph.rs:89-175) with norm2 and transition_probability
 * (common.rs:187-190), bit for bit, by the general sweeps.  Option "mm_levels" = 1: modes finished level by level instead (fewest
 * possible worlds first, a workgroup per mode; same bits, measured slower) when every observation shrinks the possible worlds and
 * "dp_sweeps" is off.  Option "mm_lds_nodes": the largest mode that relaxes in LDS there (the others relax on global memory). */
int      porrt_mm_compute_expected_costs(porrt_ctx *ctx);
int      porrt_mm_get_expected_costs(const porrt_ctx *ctx, double *out /* num_nodes */);
/* extract_policy (:479-485, belief_graph.rs:177-263) from belief node 0: returns the policy's node count (or a negative error) and
 * fills the arrays when cap holds them (cap 0: sizing): belief node ids, parents (-1 = root), leaf flags, states (2 per node), and
 * the root's expected cost.  An infinite root cost, or a walk that returns to a node on its own path, is an error (the reference
 * does not terminate there). */
int64_t  porrt_mm_extract_policy(porrt_ctx *ctx, uint64_t *belief_node_ids, int64_t *parents, uint8_t *is_leaf, double *xy, uint64_t cap,
                                 double *expected_cost);
/* PTOPolicyRefiner::refine_solution(PartialShortCut(n_iterations)) (pto_policy_refiner.rs:87-124) of the policy the last
 * porrt_mm_extract_policy walked -- the reference driver's PartialShortCut(1500) after plan (main.rs:546-575).  Same outputs and
 * sizing as porrt_bg_refine_policy. */
int64_t  porrt_mm_refine_policy(porrt_ctx *ctx, uint64_t n_iterations, double *xy, uint64_t *belief_node_ids, int64_t *parents, uint8_t *is_leaf,
                                uint64_t cap, double *expected_cost);
/* plan (:310-326): porrt_grow_mm_prm, porrt_mm_build_belief_graph, porrt_mm_compute_expected_costs, porrt_mm_extract_policy; returns the
 * policy's node count (fetch it with porrt_mm_extract_policy).  A new porrt_grow_mm_prm makes graph, costs and policy stale: using them
 * is an error. */
int64_t  porrt_mm_plan(porrt_ctx *ctx, const double start[2], const double *initial_belief, uint32_t n_worlds, double max_step,
                       double search_radius, uint64_t n_iter_per_belief);
/* seconds of the last steps, up to n of: grow (porrt_mm_plan), build, build on the device, expected costs, on the device, policy walk,
 * refine, refine on the device */
int      porrt_mm_get_plan_seconds(const porrt_ctx *ctx, double *out, uint32_t n);
/* the last expected-cost run: levels, launches (level schedule: one per level; general sweeps: sweeps), sweeps (level schedule: summed
 * over the modes), 1 = level schedule */
int      porrt_mm_get_dp_info(const porrt_ctx *ctx, uint32_t *levels, uint32_t *launches, uint64_t *sweeps, int *level_schedule);

/* ---- on-disk formats either side of the path (host code; no GPU needed).
 * porrt_read_pgm: the raster MapShelfDomain::open / Map::open load (image::open -> ImageLuma8,
 * map_shelves_io.rs:88-103, map_io.rs:90-105): P2 / P5 (P1 / P4 as 0 / 255), '#' comments in the header, samples as
 * stored (no rescaling by maxval), row-major from the top -- what porrt_set_grid / porrt_set_zones take.  Files the
 * reference rejects with "Wrong image format!" (maxval > 255 -> 16-bit gray, colour) give PORRT_ERR_INVALID.  Call with
 * out = NULL for the size. */
int porrt_read_pgm(const char *path, uint8_t *out /* W*H or NULL */, uint32_t *W, uint32_t *H);
int porrt_read_pgm_mem(const uint8_t *bytes, size_t n, uint8_t *out, uint32_t *W, uint32_t *H);
/* PTOGraph JSON (pto_graph.rs:22-118 save / load): {"nodes": [{"state", "validity_id", "parents": [{"id",
 * "validity_id"}], "children": [..]}], "validities": [[bool]]} in serde_json's pretty form.  The writer takes CSR
 * adjacency; porrt_graph_save_json writes the graph of the context's last PTO grow / PRM roadmap with the lists as the
 * reference holds them.  The reader hands the file back as the same arrays (query the sizes, then porrt_graph_file_get
 * with caller buffers; any pointer may be NULL). */
typedef struct porrt_graph_file porrt_graph_file;
int porrt_graph_write_json(const char *path, uint64_t n_nodes, const double *xy, const uint64_t *node_validity, const uint64_t *child_off,
                           const uint64_t *child_id, const uint64_t *child_validity, const uint64_t *parent_off, const uint64_t *parent_id,
                           const uint64_t *parent_validity, uint64_t n_validities, uint64_t n_worlds, const uint8_t *validities /* [n_validities][n_worlds] 0/1 */);
int porrt_graph_save_json(const porrt_ctx *ctx, const char *path);
porrt_graph_file *porrt_graph_load_json(const char *path, char *err /* may be NULL */, size_t err_cap);   /* NULL on failure */
void     porrt_graph_file_free(porrt_graph_file *g);
uint64_t porrt_graph_file_num_nodes(const porrt_graph_file *g);
uint64_t porrt_graph_file_num_children(const porrt_graph_file *g);
uint64_t porrt_graph_file_num_parents(const porrt_graph_file *g);
uint64_t porrt_graph_file_num_validities(const porrt_graph_file *g);
uint64_t porrt_graph_file_num_worlds(const porrt_graph_file *g);
int      porrt_graph_file_get(const porrt_graph_file *g, double *xy, uint64_t *node_validity, uint64_t *child_off, uint64_t *child_id,
                              uint64_t *child_validity, uint64_t *parent_off, uint64_t *parent_id, uint64_t *parent_validity, uint8_t *validities);

/* ---- the reference's figures, drawn on the device: the drawing half of MapShelfDomain / Map (map_shelves_io.rs:276-457; map_io.rs:303-479
 * is the same text with one other alpha), the tail of every driver and integration test of the reference: m.resize(5); m.draw_full_graph(..);
 * m.draw_zones_observability(); m.draw_policy(..); m.save(path) (pto.rs:313-317), or draw_tree / draw_path (rrt.rs:299-303).
 * Canvas: the context's occupancy raster as RGB8 (Map::build: ImageLuma8 -> to_rgb8, the three channels equal), resized by
 * image::imageops::resize(.., FilterType::Nearest) at an integer factor -- block replication, dst(j, i) = src(j / f, i / f) -- with
 * ppm *= factor as f64 (one rounding; factor 1 leaves it alone), low unchanged and the resized height in to_pixel_coordinates (:276-286).  It
 * also takes the context's zone positions and visibility distance, and its options "draw_max_fragments" and "draw_heavy_cap", as they stand at
 * porrt_canvas_create.  It lives on the context's device and outlives the context; it may be drawn on from any context of that device with the
 * same raster geometry (W, H, low, ppm, domain kind), PORRT_ERR_INVALID otherwise.
 * draw_line(a, b, color, alpha: f32) (:359-375): both ends through to_pixel_coordinates (the growth's saturating `as u32`), cast `as f32` with
 * (i, j) as (x, y), line_drawing::XiaolinWu::<f32, i32> over them; a pair outside the image is skipped, a pair inside blends per channel
 *     ((1.0 - a) * old as f32 + a * new as f32) as u8,   a = alpha * line_alpha,
 * in f32 without contraction, truncated and saturated.  The result at a pixel depends on the ORDER in which a call's lines reach it, so every
 * call is an ordered list of lines composited in exactly the reference's order (porrt_draw.hpp: count, scan, scatter, a resolve that orders each
 * pixel's records by the line's place and applies them in that order): bit for bit the sequential loop's image.
 *     call                          lines, in draw order                                                          colour        alpha
 *     draw_tree (:313-321)          nodes in id order; a node with a parent gives parent -> node                   TEAL          0.3
 *     draw_full_graph (:389-400)    nodes in id order; each node's children in push order (the lists             GRAY5         0.25 shelf domain,
 *                                   porrt_graph_save_json writes; both directions: a PRM roadmap's reverse                      0.15 door domain
 *                                   edge is in the lists the reference holds, prm.rs:96-103); from -> to                         (map_io.rs:420)
 *     draw_policy (:323-341)        nodes in id order; a node with more than one child first a circle of         NAVY circle,  1.0
 *                                   radius 0.025, then a line to each child (children in ascending id: the        BLACK lines
 *                                   order extract_policy and recompose number them in)
 *     draw_path (:288-292)          consecutive states                                                            caller's      1.0
 *     draw_zones_observability      one circle of radius visibility_distance per zone position, zone order        TEAL          1.0
 *       (:452-456)
 *     draw_circle (:377-387)        50 segments between xy + r * (cos, sin)(k * 2 pi / 50), k = 0 .. 50: the 51 points are made on the host
 *                                   with its libm, never on the device
 * XiaolinWu and the Nearest resize are third-party arithmetic recalled from the crates, as Bresenham is (README, parity paragraph).
 * Ours, not the reference's: a line with a non-finite coordinate is PORRT_ERR_INVALID and the canvas is left unchanged (the reference casts NaN to
 * pixel 0 and draws); a line with a pixel end beyond 2^24 is PORRT_ERR_INVALID and the canvas is left unchanged (the reference would walk billions
 * of pixels, and f32 no longer holds the integers); a canvas of more than 16384 pixels a side is PORRT_ERR_CAPACITY, as is a call of 2^31 lines.
 * Whatever a call refuses it refuses before it touches the image.
 * porrt_canvas_create returns NULL on failure: porrt_last_error(ctx) has the text and porrt_get_option(ctx, "draw_create_status") the code
 * (factor 0 or no grid: PORRT_ERR_INVALID; over the cap: PORRT_ERR_CAPACITY).  On its first use a canvas checks the device's f32 divide (the
 * gradient dy / dx) against the host's on 65536 quotients of integers up to 2^24; if one differs, gradients go through the f64 divide, which
 * porrt_selftest checks and which rounds an f32 quotient correctly (porrt_draw_info.gradient_by_f64).
 * porrt_canvas_draw_tree and porrt_canvas_draw_full_graph make their lines on the device from the context's resident arrays: no node or edge
 * array is downloaded.  porrt_canvas_draw_full_graph needs the context's adjacency lists (the ones porrt_get_edges and the belief-graph build use);
 * when the context has not made them for this graph yet, this call makes and caches them, with the kd pre-order ranks built on the device whatever
 * option "host_ranks" says (a few flag words come back per 32 levels of the kd-tree, nothing else) -- that first call is slower.
 * The two calls take `const porrt_ctx *` because the context's results are not changed; they do fill its caches (the adjacency order) and
 * porrt_canvas_create writes its error text and "draw_create_status": like every call on a context they must not run beside another call on it.
 * porrt_canvas_get_rgb: H * W * 3 bytes, row-major from the top.  porrt_canvas_save_png / porrt_write_png: 8-bit RGB PNG with stored deflate
 * blocks (no compression, no zlib): the same pixels as the reference's m.save(path), not the same bytes.  porrt_write_png needs no device.
 * porrt_canvas_get_info: the last draw call -- lines (places in the order, the nodes without parent of draw_tree included), fragments (pixel
 * visits inside the image), passes, the most records one pixel held in one pass, the pixels not resolved by a single lane (heavy_pixels) and
 * those of them that one wave resolved (wave_pixels: at most 64 records; the others took a workgroup), both summed over the passes,
 * and seconds: the whole call on the host clock, and HIP events around the count (with the per-line scan), the pixel scan, the scatter and
 * the resolve, summed over the passes. */
typedef struct porrt_canvas porrt_canvas;
struct porrt_draw_info { uint64_t lines, fragments, passes, heaviest_pixel, heavy_pixels, wave_pixels, gradient_by_f64; double s_total, s_count, s_scan, s_scatter, s_resolve; };
porrt_canvas *porrt_canvas_create(const porrt_ctx *ctx, uint32_t factor);   /* Map::open + resize(factor) */
void porrt_canvas_destroy(porrt_canvas *canvas);
const char *porrt_canvas_last_error(const porrt_canvas *canvas);
int  porrt_canvas_size(const porrt_canvas *canvas, uint32_t *W, uint32_t *H);
int  porrt_canvas_draw_lines(porrt_canvas *canvas, const double *ab /* n*4: a, b */, uint64_t n, const uint8_t rgb[3], float alpha);
int  porrt_canvas_draw_path(porrt_canvas *canvas, const double *xy /* n*2 */, uint64_t n, const uint8_t rgb[3]);
int  porrt_canvas_draw_circles(porrt_canvas *canvas, const double *xy /* n*2 */, uint64_t n, double radius, const uint8_t rgb[3]);
int  porrt_canvas_draw_tree(porrt_canvas *canvas, const porrt_ctx *ctx);          /* the tree of ctx's last porrt_grow(mode PORRT_MODE_RRT) */
int  porrt_canvas_draw_full_graph(porrt_canvas *canvas, const porrt_ctx *ctx);    /* its PTO graph or PRM roadmap */
int  porrt_canvas_draw_zones_observability(porrt_canvas *canvas);
int  porrt_canvas_draw_policy(porrt_canvas *canvas, const double *xy /* n*2 */, const int64_t *parent /* -1 = root */, uint64_t n);
int  porrt_canvas_get_rgb(const porrt_canvas *canvas, uint8_t *rgb /* H*W*3 */);
int  porrt_canvas_save_png(const porrt_canvas *canvas, const char *path);
int  porrt_write_png(const char *path, const uint8_t *rgb, uint32_t W, uint32_t H);
int  porrt_canvas_get_info(const porrt_canvas *canvas, struct porrt_draw_info *out);

/* ---- the one exchange of a query-sharded job (the reference is one process and has no
 * counterpart).  Queries are independent: query q runs on rank q mod world, nothing is communicated
 * while trees grow.  At the end, per map: ncclAllGather of one 16-byte entry per rank, the first minimum of
 * (cost, rank) wins, and the winner's node arrays are broadcast device to device (RCCL over xGMI) into
 * buffers the communicator owns on every rank.  Rendezvous is the caller's: rank 0 makes the id, its 128
 * bytes travel by whatever channel the host program has (MPI, a file, torch.distributed ...). */
#define PORRT_UNIQUE_ID_BYTES 128
typedef struct porrt_comm porrt_comm;
typedef struct {
    double  cost;            /* best path cost (RRT::get_best_solution, rrt.rs:183-193); +inf = no solution */
    int32_t rank;            /* owner; -1 in a result = nobody solved this map */
    int32_t n_nodes;         /* size of that tree */
} porrt_best_entry;
int         porrt_comm_unique_id(uint8_t id[PORRT_UNIQUE_ID_BYTES]);
porrt_comm *porrt_comm_create(int device, int rank, int world, const uint8_t id[PORRT_UNIQUE_ID_BYTES]);   /* NULL on failure */
void        porrt_comm_destroy(porrt_comm *comm);
const char *porrt_comm_last_error(const porrt_comm *comm);
/* ctxs[q] (contexts of mode PORRT_MODE_RRT) planned on map map_ids[q] (< n_maps); every rank passes the same n_maps.
 * winners[m] is the same on every rank afterwards.  Collective: all ranks of the communicator must call it -- and a rank
 * whose own part fails (bad argument, a context without a tree, allocation) still takes part: before each data step the
 * ranks all-gather a status word, and either all go on or all return -- the failing rank its own code, the others
 * PORRT_ERR_PEER (porrt_comm_last_error names the rank); ranks called with different n_maps all get PORRT_ERR_INVALID. */
int      porrt_exchange_best(porrt_comm *comm, porrt_ctx *const *ctxs, uint32_t n_ctx, const uint32_t *map_ids,
                             uint32_t n_maps, porrt_best_entry *winners);
/* The collective part alone, for a caller that keeps its own best tree per map: mine[m] = (cost, n_nodes) of this rank's best tree of map m
 * (n_nodes 0 = none; the rank field is filled in), views[m] = where its arrays live (device pointers); the same protocol, results and
 * getters as porrt_exchange_best, which is this after evaluating the contexts. */
struct porrt_tree_device_view_s;
int      porrt_exchange_tables(porrt_comm *comm, const porrt_best_entry *mine, const struct porrt_tree_device_view_s *views,
                               uint32_t n_maps, porrt_best_entry *winners);
/* No rank leaves the sequence alone: once the first agreement is through, a rank whose HIP or RCCL call fails, whose RCCL reports an
 * asynchronous error, or whose step is not finished after the time-out (default 120 s) ABORTS the communicator (ncclCommAbort) before
 * it returns, so that the peers' pending collectives fail instead of waiting; every wait polls the stream and RCCL's error state,
 * none blocks for good.  The communicator is unusable afterwards (every call returns PORRT_ERR_DEVICE): the job makes a new one. */
int      porrt_comm_usable(const porrt_comm *comm);            /* 1, or 0 once a collective step failed on this rank */
int      porrt_comm_set_timeout_ms(porrt_comm *comm, int ms);
/* for the CPU tests of that protocol (no RCCL, no device): a stand-in communicator, and the function every failure of the real
 * path goes through -- stage 0 = a local failure before the first agreement (a status word; returns `code`, the communicator stays
 * usable), stage >= 1 = at or after it (the communicator is aborted); porrt_comm_test_aborts counts the aborts */
porrt_comm *porrt_comm_test_new(int rank, int world);
/* ... and a communicator over a transport the test brings: the exchange's whole sequence (agreements, all-gather, decision, the
 * broadcasts from whichever rank wins, the getters) then runs between CPU processes on host memory -- tests/test_sharding_gloo.py drives
 * it with two ranks over gloo.  Every function returns 0 or an error; "device" buffers are what alloc returns. */
typedef struct {
    void *self;
    int   (*all_gather)(void *self, const void *send, void *recv, size_t bytes_per_rank);     /* recv: world x bytes, rank order */
    int   (*broadcast)(void *self, const void *send, void *recv, size_t bytes, int root);     /* send is read on the root only */
    void *(*alloc)(void *self, size_t bytes);
    void  (*release)(void *self, void *p);
    int   (*fetch)(void *self, void *host_dst, const void *src, size_t bytes);
    int   (*abort)(void *self);                                                               /* may be NULL */
} porrt_comm_ops;
porrt_comm *porrt_comm_test_new_ops(int rank, int world, const porrt_comm_ops *ops);          /* ops must outlive the communicator */
int      porrt_comm_test_fail(porrt_comm *comm, int stage, int code /* < 0 */);
int      porrt_comm_test_aborts(const porrt_comm *comm);
uint64_t porrt_exchange_num_nodes(const porrt_comm *comm, uint32_t map);
int      porrt_exchange_get_tree(const porrt_comm *comm, uint32_t map, double *xy, int64_t *parent, double *dist_root);
/* step 2 of the exchange on its own (pure host code): all[r * n_maps + m] -> win_rank[m] */
int      porrt_exchange_decide(const porrt_best_entry *all, uint32_t world, uint32_t n_maps, int32_t *win_rank);
/* the status decision on its own (pure host code): words[2r] = code of rank r (0 or negative), words[2r+1] = its n_maps;
 * returns what rank my_rank must return (above), *bad_rank = the first failing / disagreeing rank or -1 */
int      porrt_exchange_agree(const int32_t *words /* world x 2 */, uint32_t world, uint32_t my_rank, int32_t *bad_rank);

/* The grown tree where it lives: device pointers into the context's arena (valid until the context's
 * next grow or its destruction).  n_nodes = 0 when there are no results. */
typedef struct porrt_tree_device_view_s {
    const double *nx, *ny, *dist_root;
    const int32_t *parent;       /* -1 = root */
    uint64_t n_nodes;
} porrt_tree_device_view;
porrt_tree_device_view porrt_tree_device(const porrt_ctx *ctx);

/* ---- MapShelfDomainTampRRT::plan(.., TampSearch::BranchAndBound) (map_shelves_tamp_rrt.rs:159-291) on the
 * context's shelf map and zones: a depth-first branch and bound over zone orders whose edges are two RRT* queries each (to see the
 * zone: ObservationGoal; then to the zone's position: SquareGoal of half-width goal_radius), grown on the device with batch_K, then
 * build_policy (:619-663): every path of the best chain shortcut (:565-617, 100 iterations) and the policy's expected cost.
 * Options: "tamp_streams" 0 = one continuous stream across the search in the reference's order (the context's own; set back to
 * its value at entry on return), 1 (default) = one stream per search edge, seeded from the context's sampler seed and the edge's
 * zone prefix (splitmix64), which makes the result independent of the expansion order; "tamp_wave" (mode 1) search nodes popped at
 * once, their queries grown together; "tamp_pool" worker contexts that grow them (made on first use, freed with this context);
 * "tamp_search" 0 = BranchAndBound, 1 = AStar and 2 = BranchAndBoundMultipleViewPoints are refused (PORRT_ERR_INVALID): the
 * reference's order among equal priorities / its HashSet walk cannot be pinned.  Both searches are offered with a stated order
 * through entry points of their own: porrt_tamp_rrt_plan_astar and porrt_tamp_rrt_plan_viewpoints below.
 * The shuffles draw from the context's discrete sampler, which runs on across plans.  The context's goal is replaced.
 * Returns the policy's node count, PORRT_ERR_INVALID (n_worlds != zones, a prior whose sum is not within 0.001 of 1),
 * PORRT_ERR_NO_PATH, or another error. */
typedef struct {
    double   search_cost;        /* best expected cost of the search, before the shortcut */
    double   expected_cost;      /* the policy's, after it */
    uint64_t search_nodes, queries, waves, pruned;     /* pruned = children not pushed */
    uint32_t n_order;            /* zones of the best leaf, in the order they are visited */
    uint32_t zone_order[64];
    int64_t  fail_node;          /* PORRT_ERR_NO_PATH: the search node whose query found no path (-1 otherwise) */
    int32_t  fail_zone;          /*   its zone */
    int32_t  fail_query;         /*   0 = observation, 1 = pickup */
    double   total_s, grow_s, path_s, shortcut_s, search_s, pool_s, goals_s;   /* seconds: wall, growth, best paths, shortcut, host
                                    search, worker creation, setting the queries' samplers and goals */
    uint32_t streams, wave, pool, pad;
} porrt_tamp_info;
int64_t  porrt_tamp_rrt_plan(porrt_ctx *ctx, const double start[2], const double *initial_belief, uint32_t n_worlds, double max_step,
                             double search_radius, uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t batch_K);
/* the last plan's policy: n = node count; xy n*2, parents n (-1 = root), is_leaf n, beliefs n x n_worlds.  With cap < n only the
 * count (and the cost) is returned.  Any pointer may be NULL. */
int64_t  porrt_tamp_rrt_policy(const porrt_ctx *ctx, double *xy, int64_t *parents, uint8_t *is_leaf, double *beliefs, uint64_t cap,
                               double *expected_cost);
int      porrt_tamp_rrt_get_info(const porrt_ctx *ctx, porrt_tamp_info *out);
/* the best path of every context of the last porrt_grow_batch (or porrt_grow) on the device (k_best_cost + k_best_path: no tree is
 * downloaded); the paths concatenated root first into xy (cap states), lens[q] = 0 for "No solution found", costs[q] (may be NULL;
 * +inf without a solution).  PORRT_ERR_CAPACITY if one path has more than 1024 states or xy holds fewer than their sum. */
int      porrt_best_paths(porrt_ctx *const *ctxs, uint32_t n_ctx, double *xy, uint64_t cap, uint64_t *lens, double *costs);
/* the planner's shortcut on explicit paths, on the device: path i = states [offsets[i], offsets[i + 1]) of xy (n x 2); out like xy */
int      porrt_tamp_shortcut_paths(porrt_ctx *ctx, const double *xy, const uint64_t *offsets, uint64_t n_paths, double *out);

/* ---- RRT::get_solutions (src/rrt.rs:195-246) of many grown RRT* trees in one device call: every "firstly
 * final" node of a tree -- a final node whose parent is not final -- with its path from the root and that path's cost (folded from
 * 0.0 in path order, rrt.rs:223-227).  The reference returns them in the order of a HashSet; here they come in ASCENDING NODE ID.
 * n_solutions[q], n_states[q]: solutions of context q and the states of all their paths (either may be NULL).  With ids == NULL the
 * call is a size query.  Otherwise the solutions come concatenated context by context, ascending id within a context: ids, lens
 * (states per path) and costs hold cap_solutions entries, xy cap_states states (x y), the paths root first one after another.
 * Nothing is truncated: PORRT_ERR_CAPACITY if a cap is too small.  Runs of the argument that are exactly a leader's last
 * porrt_grow_batch get one launch; other contexts go one by one.  A context without a solution has count 0 (no error).
 * PORRT_ERR_INVALID for NULL, a context without results or with PTO / PRM results.  No tree is downloaded. */
int      porrt_solutions(porrt_ctx *const *ctxs, uint32_t n_ctx, uint64_t *n_solutions, uint64_t *n_states, uint64_t *ids, uint64_t *lens,
                         double *costs, uint64_t cap_solutions, double *xy, uint64_t cap_states);

/* ---- MapShelfDomainTampRRT::plan(.., TampSearch::BranchAndBoundMultipleViewPoints) (map_shelves_tamp_rrt.rs:293-430, DESIGN.md
 * section 21): the branch and bound of porrt_tamp_rrt_plan in which the observation query of a (search node, zone) pair keeps all
 * its solutions (RRT::plan_several) and every one of them -- a viewpoint -- becomes a child, with a pickup query of its own.
 * A separate entry point on purpose: porrt_tamp_rrt_plan with "tamp_search" 2 stays refused, because the reference walks the
 * viewpoints in the order of a HashSet.  What is offered here is the reference's search with that set walked in ASCENDING NODE ID:
 * one of the orders the reference may take, not one we can claim it took.
 * max_viewpoints is ours, not the reference's: 0 keeps all viewpoints (the reference); n > 0 keeps, per observation query, the n
 * solutions of lowest cost (ties: the lower id), still walked in ascending id.
 * "tamp_streams" 0: one continuous stream; per (node, zone) the observation query, then its viewpoints' pickup queries in ascending
 * id.  1 (default): the observation query of (u, t) runs on a stream seeded ho = splitmix64(u.h ^ (t + 1)) (root h = the sampler
 * seed), the pickup query of the viewpoint of rank j (0-based, in the kept list) on h = splitmix64(ho ^ ((j + 1) << 32)), which is
 * the child's h: the pickup does NOT continue the observation stream (unlike BranchAndBound).  "tamp_wave", "tamp_pool" as above.
 * An observation query without solutions makes no children (no error); a pickup query without a path is PORRT_ERR_NO_PATH
 * (fail_query 1, fail_node = the id the child would have got); a search without a leaf is PORRT_ERR_NO_PATH with fail_node -1.
 * The policy and the info come through porrt_tamp_rrt_policy / porrt_tamp_rrt_get_info: a later plan of either kind replaces the
 * earlier one. */
typedef struct {
    uint64_t observation_queries, pickup_queries;
    uint64_t viewpoints_found, viewpoints_kept;    /* solutions of all observation queries; those left after max_viewpoints */
    uint64_t largest_set;                          /* the most solutions one observation query gave */
    double   solutions_s;                          /* seconds spent gathering solutions (porrt_solutions' device path) */
    uint32_t max_viewpoints;
    uint32_t n_ranks;                              /* levels of the best leaf */
    uint32_t ranks[64];                            /* the viewpoint rank chosen at each of them (beside zone_order) */
} porrt_tamp_viewpoints_info;                      /* all zero after porrt_tamp_rrt_plan */
int64_t  porrt_tamp_rrt_plan_viewpoints(porrt_ctx *ctx, const double start[2], const double *initial_belief, uint32_t n_worlds, double max_step,
                                        double search_radius, uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t batch_K,
                                        uint32_t max_viewpoints);
int      porrt_tamp_rrt_get_viewpoints_info(const porrt_ctx *ctx, porrt_tamp_viewpoints_info *out);

/* ---- MapShelfDomainTampRRT::plan(.., TampSearch::AStar) (plan_astar, map_shelves_tamp_rrt.rs:432-563): a
 * best-first search over zone orders.  The node of lowest priority is popped and makes one child per remaining zone in zone order
 * (no shuffle: the discrete sampler is not touched), two RRT* queries per child as in porrt_tamp_rrt_plan;
 *     ec = u.ec + rp * (obs_cost + belief[t] * pickup_cost),  priority = ec + rp * sum_z belief[z] * norm2(observation_state, zone_pos[z])
 * over the child's remaining zones in order; the first popped node without remaining zones is the solution.
 * A separate entry point on purpose: porrt_tamp_rrt_plan with "tamp_search" 1 stays refused, because the reference's Priority never
 * compares Equal (common.rs:235-239) and its order among equal priorities is its heap's.  OURS, not the reference's:
 *   - bit-equal priorities pop in ASCENDING SEARCH NODE ID; a node's children get the next ids, in zone order, when the node is
 *     popped; +0.0 and -0.0 are equal;
 *   - a prior with an entry that is not > 0 is PORRT_ERR_INVALID (the reference's priorities would all be NaN below the last
 *     positive zone).
 * "tamp_streams" 0: the context's own stream across the queries in the sequential order, set back on return, one node per wave.
 * 1 (default): the per-edge streams of porrt_tamp_rrt_plan.  A node's cost and priority are then functions of its zone prefix, and
 * "tamp_wave" = W speculates: when the top of the queue has no computed children, it and the next best non-leaf entries without
 * children (up to W) are expanded in one pair of batches; the children enter the queue only when their parent is popped.  At every
 * W the policy, zone_order, search_cost, search_nodes and every node's id, ec and priority are those of W = 1; queries, waves and
 * `speculated` differ.  A query without a path is PORRT_ERR_NO_PATH only when its parent is popped: fail_node = the id the child
 * would have got, fail_zone / fail_query = the first failing child in zone order (the observation query fails before the pickup).
 * The paths of all children stay on the device in an arena ("tamp_arena_states": its initial capacity in states, >= 1024; it grows
 * between gathers, PORRT_ERR_CAPACITY if it cannot); only the winning chain's paths are ever copied out of it.
 * The policy and the info come through porrt_tamp_rrt_policy / porrt_tamp_rrt_get_info (pruned = 0; waves = rounds of expansion). */
typedef struct {
    uint64_t speculated;         /* expansions whose node was never popped */
    uint64_t arena_states;       /* capacity of the path arena after the plan */
    uint64_t arena_used;         /* states the plan's paths took in it */
    uint64_t arena_grown;        /* times it grew during the plan */
    double   children_s;         /* seconds: uploading, running and fetching k_astar_children */
    double   chain_s;            /* seconds on the device: k_astar_chain */
} porrt_tamp_astar_info;         /* describes the last porrt_tamp_rrt_plan_astar */
int64_t  porrt_tamp_rrt_plan_astar(porrt_ctx *ctx, const double start[2], const double *initial_belief, uint32_t n_worlds, double max_step,
                                   double search_radius, uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t batch_K);
int      porrt_tamp_rrt_get_astar_info(const porrt_ctx *ctx, porrt_tamp_astar_info *out);
/* the search nodes of the last porrt_tamp_rrt_plan_astar in id order (also after PORRT_ERR_NO_PATH: the nodes made so far):
 * parents (-1 = root), targets (zone; -1 = root), ec, priority.  Returns their count; with cap below it nothing is written. */
int64_t  porrt_tamp_astar_nodes(const porrt_ctx *ctx, int64_t *parents, int32_t *targets, double *ec, double *priority, uint64_t cap);
/* ---- many A* plans on one map in one call.  Plan p is the search of porrt_tamp_rrt_plan_astar from
 * starts[p] with prior priors[p] and root stream seed seeds[p] (NULL: the context's sampler seed for every plan); its worker streams
 * are splitmix64 of that seed and the zone prefix, the sampler box is the context's.  Map, zones and every numeric parameter are
 * shared.  Needs "tamp_streams" 1: every plan of a batch is then, bit for bit, the plan porrt_tamp_rrt_plan_astar gives alone on a
 * context whose sampler seed is seeds[p] -- policy, costs, zone order, every search node, and queries / waves / speculated at the
 * same "tamp_wave".  The plans' searches run in rounds: every live search replays and selects its wave ("tamp_wave" per plan), and
 * the selected edges of all plans, in plan then node then zone order, go through porrt_grow_batch in chunks of "tamp_pool" rows;
 * their paths share one arena ("tamp_arena_states": its first capacity), and the chains of all plans that found a leaf are shortcut
 * in one launch.
 * Returns the number of plans that found a policy (0 is no error), or a negative code.  PORRT_ERR_NO_PATH is per plan (status,
 * fail_* by the rule above; the nodes made so far stay readable; the other plans go on).  Everything else fails the call and names
 * the plan in porrt_last_error where one is to blame: PORRT_ERR_INVALID before anything runs (a prior whose sum is off or with an
 * entry not > 0, n_worlds != zones, n_plans outside 1..65536, NULL starts or priors, "tamp_streams" 0), PORRT_ERR_CAPACITY from the
 * arena or a path slot, device errors, and whatever porrt_grow_batch answers.
 * The call leaves the context's continuous stream, its discrete sampler and its goal-independent state alone.  It replaces the
 * context's last single plan: porrt_tamp_rrt_policy then answers as after a failed plan and porrt_tamp_astar_nodes gives 0 nodes;
 * porrt_tamp_rrt_get_info holds the call's totals (queries, waves = rounds of the driver, search_nodes, the seconds, pool) and
 * porrt_tamp_rrt_get_astar_info the call's arena figures, children_s, chain_s and the sum of `speculated`.  The results live on
 * the context until the next batch call or porrt_destroy. */
typedef struct {
    int32_t  status;                 /* PORRT_OK or PORRT_ERR_NO_PATH */
    int32_t  fail_zone, fail_query;  /* as porrt_tamp_info; -1 when status is PORRT_OK */
    int64_t  fail_node;
    double   search_cost, expected_cost;
    uint64_t search_nodes, queries, waves, speculated;   /* this plan's own: those of the single plan at the same tamp_wave */
    uint64_t policy_nodes;           /* 0 for a failed plan */
    uint32_t n_order, pad;
    uint32_t zone_order[64];
} porrt_tamp_batch_plan;
int64_t  porrt_tamp_rrt_plan_astar_batch(porrt_ctx *ctx, uint32_t n_plans, const double *starts /* n x 2 */,
                                         const double *priors /* n x n_worlds */, const uint64_t *seeds /* n, or NULL */, uint32_t n_worlds,
                                         double max_step, double search_radius, uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius,
                                         uint32_t batch_K);
int      porrt_tamp_batch_get_plan(const porrt_ctx *ctx, uint32_t plan, porrt_tamp_batch_plan *out);
/* plan `plan` of the last batch: its policy as porrt_tamp_rrt_policy gives it (PORRT_ERR_INVALID for a failed plan), its search
 * nodes as porrt_tamp_astar_nodes gives them (also of a failed plan) */
int64_t  porrt_tamp_batch_policy(const porrt_ctx *ctx, uint32_t plan, double *xy, int64_t *parents, uint8_t *is_leaf, double *beliefs,
                                 uint64_t cap, double *expected_cost);
int64_t  porrt_tamp_batch_astar_nodes(const porrt_ctx *ctx, uint32_t plan, int64_t *parents, int32_t *targets, double *ec, double *priority,
                                      uint64_t cap);
/* ---- many branch-and-bound plans on one map in one call.  Plan p is the search of porrt_tamp_rrt_plan
 * ("tamp_search" 0) from starts[p] with prior priors[p].  Its root stream seed is seeds[p] (NULL: the context's sampler seed for
 * every plan) and its per-edge streams are splitmix64 of that seed and the zone prefix, as under "tamp_streams" 1.  Its shuffles
 * draw from a discrete sampler of the plan's own, seeded discrete_seeds[p] (NULL: seeds[p], which is what porrt_set_sampler(.., seed)
 * leaves in a fresh context).  Map, zones, sampler box and every numeric parameter are shared.
 * Needs "tamp_streams" 1 and "tamp_search" 0 (PORRT_ERR_INVALID otherwise, the latter with porrt_tamp_rrt_plan's message).  Every
 * plan of a batch is then, bit for bit, the plan porrt_tamp_rrt_plan gives alone on a fresh context whose sampler seed is seeds[p]
 * and whose discrete seed is discrete_seeds[p], at the same "tamp_wave" with "tamp_streams" 1: policy states, parents, leaf flags
 * and beliefs, search_cost, expected_cost, zone_order, search_nodes, queries, waves and pruned -- whatever else is in the batch,
 * whatever "tamp_pool" is and wherever a chunk is cut.  The searches run in the rounds of the A* batch above: every live plan
 * closes its last wave and pops its next ("tamp_wave" nodes per plan), and the children of all plans, in plan then node then zone
 * order, go through porrt_grow_batch in chunks of "tamp_pool" rows; their paths share one arena ("tamp_arena_states": its first
 * capacity; it is never reclaimed during a call), and the chains of all plans that hold a leaf are shortcut in one launch.  A caller
 * of large batches sets "tamp_wave" 8 and "tamp_pool" 2048: narrower waves leave the rows empty even with 100 plans, wider ones
 * run up to 2.3 times the queries (DESIGN.md section 28 has the measurements).
 * Returns the number of plans that found a policy (0 is no error), or a negative code.  PORRT_ERR_NO_PATH is per plan and follows
 * the single plan's rule: the plan fails at the first child of its wave, in the sequential order, whose observation query or
 * (observation found) pickup query has no path; fail_node is that child's id, search_nodes the nodes made up to and including that
 * wave.  A failed plan's queries and waves are not pinned (the single plan stops mid-chunk, a batch cannot).  The other plans go
 * on.  Everything else fails the call and names the plan in porrt_last_error where one is to blame: PORRT_ERR_INVALID before
 * anything runs (a prior whose sum is not within 0.001 of 1 -- zero entries are allowed here --, n_worlds != zones, n_plans outside
 * 1..65536, NULL starts or priors), PORRT_ERR_CAPACITY from the arena or a path slot, device errors, and whatever
 * porrt_grow_batch answers.
 * The call leaves the context's continuous stream, its goal-independent state and ITS DISCRETE SAMPLER alone -- unlike
 * porrt_tamp_rrt_plan, whose shuffles move the context's discrete sampler.  It replaces the context's last single plan
 * (porrt_tamp_rrt_policy then answers as after a failed plan) and the last batch of either kind.  The per-plan results come through
 * porrt_tamp_batch_get_plan (speculated = 0) and porrt_tamp_batch_policy above, `pruned` through porrt_tamp_batch_get_pruned
 * (porrt_tamp_batch_plan has no room for it; 0 after an A* batch).  porrt_tamp_rrt_get_info holds the call's totals (queries,
 * waves = rounds of the driver, search_nodes, pruned, the seconds, pool) and porrt_tamp_rrt_get_astar_info the arena figures. */
int64_t  porrt_tamp_rrt_plan_batch(porrt_ctx *ctx, uint32_t n_plans, const double *starts /* n x 2 */,
                                   const double *priors /* n x n_worlds */, const uint64_t *seeds /* n, or NULL */,
                                   const uint64_t *discrete_seeds /* n, or NULL */, uint32_t n_worlds, double max_step,
                                   double search_radius, uint64_t n_iter_min, uint64_t n_iter_max, double goal_radius, uint32_t batch_K);
int      porrt_tamp_batch_get_pruned(const porrt_ctx *ctx, uint32_t plan, uint64_t *pruned);
/* the search nodes of plan `plan` of the last porrt_tamp_rrt_plan_batch in id order (a node has its id from the moment it is made;
 * also of a failed plan: every node made up to and including the failing wave): parents (-1 = root), targets (zone; -1 = root), ec
 * (0 for a child whose query found no path), pushed (1 = it went onto the stack, 0 = pruned or never closed).  Returns their count;
 * with cap below it nothing is written.  PORRT_ERR_INVALID after an A* batch, as porrt_tamp_batch_astar_nodes is after a
 * branch-and-bound batch. */
int64_t  porrt_tamp_batch_bnb_nodes(const porrt_ctx *ctx, uint32_t plan, int64_t *parents, int32_t *targets, double *ec, uint8_t *pushed,
                                    uint64_t cap);
/* porrt_tamp_shortcut_paths through the shortcut's device-resident input form: the paths are first put into the A* search's arena
 * and reach the shortcut's staging planes by k_astar_chain, as the winning chain of a plan does.  Same result, bit for bit. */
int      porrt_tamp_shortcut_paths_resident(porrt_ctx *ctx, const double *xy, const uint64_t *offsets, uint64_t n_paths, double *out);

#ifdef __cplusplus
}
#endif
#endif
