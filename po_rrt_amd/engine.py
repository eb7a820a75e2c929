"""ctypes binding of libporrt_hip.so -- the C ABI declared in include/porrt_hip.h.

This is plumbing only: every method forwards to one exported symbol.  There is no CPU
fallback; constructing an Engine without the HIP library or without a GPU raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libporrt_hip.so")

MODE_RRT, MODE_PTO = 0, 1
DOMAIN_SHELF, DOMAIN_DOOR = 0, 1
OK, INCOMPLETE = 0, 1

_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")

# every symbol include/porrt_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "porrt_create", "porrt_destroy", "porrt_last_error", "porrt_set_grid", "porrt_set_zones", "porrt_set_sampler",
    "porrt_set_discrete_seed", "porrt_set_samples", "porrt_set_worlds", "porrt_set_square_goal",
    "porrt_set_observation_goal", "porrt_grow", "porrt_grow_batch", "porrt_grow_batch_each", "porrt_grow_prm", "porrt_prm_plan_path", "porrt_prm_plan_paths", "porrt_prm_get_paths", "porrt_prm_paths_info", "porrt_num_nodes", "porrt_num_iterations", "porrt_get_tree", "porrt_get_trees",
    "porrt_num_final", "porrt_get_final_ids", "porrt_get_final_masks", "porrt_get_reach", "porrt_get_node_validity",
    "porrt_num_edges", "porrt_get_edges", "porrt_is_final_set_complete", "porrt_n_worlds", "porrt_get_validities",
    "porrt_get_zone_positions", "porrt_best_solution", "porrt_best_cost", "porrt_best_cost_batch", "porrt_get_metrics", "porrt_set_option", "porrt_get_option", "porrt_selftest",
    "porrt_build_belief_graph", "porrt_bg_num_beliefs", "porrt_bg_num_nodes", "porrt_bg_num_edges", "porrt_bg_get_beliefs",
    "porrt_bg_get_observable_zones", "porrt_bg_get_node_types", "porrt_bg_get_children", "porrt_bg_get_parents", "porrt_bg_get_seconds",
    "porrt_bg_compute_expected_costs", "porrt_bg_get_expected_costs", "porrt_bg_expected_cost_of", "porrt_bg_get_dp_info", "porrt_bg_get_dp_sweep_rows", "porrt_bg_extract_policy", "porrt_conditional_dijkstra",
    "porrt_bg_refine_policy", "porrt_refine_policy", "porrt_bg_get_refine_info",
    "porrt_comm_unique_id", "porrt_comm_create", "porrt_comm_destroy", "porrt_comm_last_error", "porrt_exchange_best", "porrt_exchange_num_nodes",
    "porrt_exchange_get_tree", "porrt_exchange_decide", "porrt_exchange_agree", "porrt_tree_device",
    "porrt_host_pin", "porrt_host_unpin", "porrt_exchange_tables", "porrt_comm_test_new_ops", "porrt_comm_usable", "porrt_comm_set_timeout_ms", "porrt_comm_test_new", "porrt_comm_test_fail", "porrt_comm_test_aborts",
    "porrt_grow_mm_prm", "porrt_mm_num_modes", "porrt_mm_num_transitions", "porrt_mm_num_beliefs", "porrt_mm_get_mode", "porrt_mm_get_mode_graph",
    "porrt_mm_get_transition", "porrt_mm_get_transition_pairs", "porrt_mm_get_seconds",
    "porrt_mm_build_belief_graph", "porrt_mm_bg_num_nodes", "porrt_mm_bg_num_edges", "porrt_mm_bg_num_finals", "porrt_mm_bg_get_graph",
    "porrt_mm_compute_expected_costs", "porrt_mm_get_expected_costs", "porrt_mm_extract_policy", "porrt_mm_refine_policy", "porrt_mm_plan",
    "porrt_mm_get_plan_seconds", "porrt_mm_get_dp_info",
    "porrt_read_pgm", "porrt_read_pgm_mem", "porrt_graph_write_json", "porrt_graph_save_json", "porrt_graph_load_json", "porrt_graph_file_free",
    "porrt_graph_file_num_nodes", "porrt_graph_file_num_children", "porrt_graph_file_num_parents", "porrt_graph_file_num_validities",
    "porrt_graph_file_num_worlds", "porrt_graph_file_get",
    "porrt_tamp_rrt_plan", "porrt_tamp_rrt_policy", "porrt_tamp_rrt_get_info", "porrt_tamp_shortcut_paths", "porrt_best_paths",
    "porrt_solutions", "porrt_tamp_rrt_plan_viewpoints", "porrt_tamp_rrt_get_viewpoints_info",
    "porrt_tamp_rrt_plan_astar", "porrt_tamp_rrt_get_astar_info", "porrt_tamp_astar_nodes", "porrt_tamp_shortcut_paths_resident",
    "porrt_tamp_rrt_plan_astar_batch", "porrt_tamp_batch_get_plan", "porrt_tamp_batch_policy", "porrt_tamp_batch_astar_nodes",
    "porrt_tamp_rrt_plan_batch", "porrt_tamp_batch_get_pruned", "porrt_tamp_batch_bnb_nodes",
    "porrt_qmdp_plan", "porrt_qmdp_get_costs", "porrt_qmdp_info", "porrt_qmdp_react", "porrt_qmdp_costs",
    "porrt_qmdp_policy_graph", "porrt_qmdp_policy_graph_get", "porrt_qmdp_policy_graph_info", "porrt_policy_graph",
    "porrt_bg_extract_policies", "porrt_bg_get_policies", "porrt_mm_extract_policies", "porrt_mm_get_policies", "porrt_extract_policies",
    "porrt_policies_info",
    "porrt_bg_refine_policies", "porrt_mm_refine_policies", "porrt_refine_policies", "porrt_refine_policies_info",
    "porrt_bg_reparent_policies", "porrt_bg_get_reparented_policies", "porrt_bg_reparent_policy", "porrt_reparent_policies",
    "porrt_reparent_policies_info",
    "porrt_plan_belief_space_batch", "porrt_plan_batch_get_policies", "porrt_plan_batch_get_expected_costs", "porrt_plan_batch_info",
    "porrt_mm_plan_batch", "porrt_mm_plan_batch_get_policies", "porrt_mm_plan_batch_get_expected_costs", "porrt_mm_plan_batch_get_plan",
    "porrt_mm_plan_batch_info",
    "porrt_canvas_create", "porrt_canvas_destroy", "porrt_canvas_last_error", "porrt_canvas_size", "porrt_canvas_draw_lines", "porrt_canvas_draw_path",
    "porrt_canvas_draw_circles", "porrt_canvas_draw_tree", "porrt_canvas_draw_full_graph", "porrt_canvas_draw_zones_observability",
    "porrt_canvas_draw_policy", "porrt_canvas_get_rgb", "porrt_canvas_save_png", "porrt_write_png", "porrt_canvas_get_info",
]


class Metrics(C.Structure):
    _fields_ = [("n_iter", C.c_uint64), ("n_nodes", C.c_uint64), ("n_steps", C.c_uint64),
                ("n_tie_fallbacks", C.c_uint64), ("total_s", C.c_double), ("setup_s", C.c_double),
                ("device_s", C.c_double), ("scan_s", C.c_double), ("scan_launches", C.c_uint64),
                ("scan_pairs", C.c_double), ("scan_bytes", C.c_double), ("connect_s", C.c_double)]


class TampInfo(C.Structure):
    """porrt_tamp_info"""
    _fields_ = [("search_cost", C.c_double), ("expected_cost", C.c_double), ("search_nodes", C.c_uint64), ("queries", C.c_uint64),
                ("waves", C.c_uint64), ("pruned", C.c_uint64), ("n_order", C.c_uint32), ("zone_order", C.c_uint32 * 64),
                ("fail_node", C.c_int64), ("fail_zone", C.c_int32), ("fail_query", C.c_int32),
                ("total_s", C.c_double), ("grow_s", C.c_double), ("path_s", C.c_double), ("shortcut_s", C.c_double),
                ("search_s", C.c_double), ("pool_s", C.c_double), ("goals_s", C.c_double),
                ("streams", C.c_uint32), ("wave", C.c_uint32), ("pool", C.c_uint32), ("pad", C.c_uint32)]


class TampAstarInfo(C.Structure):
    """porrt_tamp_astar_info"""
    _fields_ = [("speculated", C.c_uint64), ("arena_states", C.c_uint64), ("arena_used", C.c_uint64), ("arena_grown", C.c_uint64),
                ("children_s", C.c_double), ("chain_s", C.c_double)]


class TampBatchPlan(C.Structure):
    """porrt_tamp_batch_plan"""
    _fields_ = [("status", C.c_int32), ("fail_zone", C.c_int32), ("fail_query", C.c_int32), ("fail_node", C.c_int64),
                ("search_cost", C.c_double), ("expected_cost", C.c_double), ("search_nodes", C.c_uint64), ("queries", C.c_uint64),
                ("waves", C.c_uint64), ("speculated", C.c_uint64), ("policy_nodes", C.c_uint64), ("n_order", C.c_uint32),
                ("pad", C.c_uint32), ("zone_order", C.c_uint32 * 64)]


class TampViewpointsInfo(C.Structure):
    """porrt_tamp_viewpoints_info"""
    _fields_ = [("observation_queries", C.c_uint64), ("pickup_queries", C.c_uint64), ("viewpoints_found", C.c_uint64),
                ("viewpoints_kept", C.c_uint64), ("largest_set", C.c_uint64), ("solutions_s", C.c_double),
                ("max_viewpoints", C.c_uint32), ("n_ranks", C.c_uint32), ("ranks", C.c_uint32 * 64)]


class PrmPathsInfo(C.Structure):
    """struct porrt_prm_paths_info"""
    _fields_ = [("queries", C.c_uint64), ("rows", C.c_uint64), ("sweeps", C.c_uint64), ("passes", C.c_uint64),
                ("ms_device", C.c_double), ("ms_wall", C.c_double), ("ms_nearest", C.c_double)]


class QmdpInfo(C.Structure):
    """struct porrt_qmdp_info"""
    _fields_ = [("nodes", C.c_uint64), ("edges", C.c_uint64), ("worlds", C.c_uint64), ("sweeps", C.c_uint64), ("queries", C.c_uint64),
                ("ms_plan_device", C.c_double), ("ms_plan_wall", C.c_double), ("ms_react_device", C.c_double), ("ms_react_wall", C.c_double),
                ("ms_nearest", C.c_double)]


class PolicyGraphInfo(C.Structure):
    """struct porrt_policy_graph_info"""
    _fields_ = [("entries", C.c_uint64), ("kept", C.c_uint64), ("how", C.c_uint64 * 6), ("residual", C.c_uint64),
                ("pivots_total", C.c_uint64), ("pivots_max", C.c_uint64),
                ("ms_classify_device", C.c_double), ("ms_classify_wall", C.c_double), ("ms_simplex_device", C.c_double),
                ("ms_simplex_wall", C.c_double), ("ms_compact_device", C.c_double), ("ms_compact_wall", C.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "how" else getattr(self, k)) for k, _ in self._fields_}


class PoliciesInfo(C.Structure):
    """struct porrt_policies_info"""
    _fields_ = [("queries", C.c_uint64), ("ok", C.c_uint64), ("nodes", C.c_uint64), ("max_nodes", C.c_uint64),
                ("ms_device", C.c_double), ("ms_wall", C.c_double)]


class RefinePoliciesInfo(C.Structure):
    """struct porrt_refine_policies_info"""
    _fields_ = [("policies", C.c_uint64), ("ok", C.c_uint64), ("pieces", C.c_uint64), ("shortcut_pieces", C.c_uint64), ("nodes", C.c_uint64),
                ("distinct_lengths", C.c_uint64), ("ms_device", C.c_double), ("ms_wall", C.c_double)]


class ReparentPoliciesInfo(C.Structure):
    """struct porrt_reparent_policies_info"""
    _fields_ = [(k, C.c_uint64) for k in ("policies", "ok", "pieces", "tree_nodes", "max_tree", "pairs", "pops", "reparents", "nodes", "rounds")] + \
               [(k, C.c_double) for k in ("ms_tube", "ms_neighbours", "ms_pop", "ms_recompose", "ms_wall")]


class PlanBatchInfo(C.Structure):
    """struct porrt_plan_batch_info"""
    _fields_ = [(k, C.c_uint64) for k in ("members", "passes", "graph_nodes", "graph_edges", "beliefs", "belief_nodes", "belief_edges",
                                          "final_belief_nodes", "policies_ok", "policy_nodes")] + \
               [(k, C.c_double) for k in ("ms_wall", "ms_join", "ms_edge_order", "ms_belief_graph", "ms_costs", "ms_policies", "ms_refine", "ms_device")]


class MmBatchPlan(C.Structure):
    """struct porrt_mm_batch_plan"""
    _fields_ = [(k, C.c_uint64) for k in ("modes", "transitions", "beliefs", "nodes", "forward_edges", "belief_edges", "finals", "pass_")]


class MmPlanBatchInfo(C.Structure):
    """struct porrt_mm_plan_batch_info"""
    _fields_ = [(k, C.c_uint64) for k in ("plans", "passes", "modes", "transitions", "nodes", "prefix_points", "explicit_points", "forward_edges",
                                          "belief_edges", "finals", "policies_ok", "policy_nodes", "upload_bytes")] + \
               [(k, C.c_double) for k in ("ms_wall", "ms_host", "ms_points", "ms_roadmaps", "ms_belief_graph", "ms_costs", "ms_policies", "ms_refine",
                                          "ms_device")]


class DrawInfo(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("fragments", C.c_uint64), ("passes", C.c_uint64), ("heaviest_pixel", C.c_uint64),
                ("heavy_pixels", C.c_uint64), ("wave_pixels", C.c_uint64), ("gradient_by_f64", C.c_uint64), ("s_total", C.c_double), ("s_count", C.c_double),
                ("s_scan", C.c_double), ("s_scatter", C.c_double), ("s_resolve", C.c_double)]


class colors:
    """the reference's colour table (map_shelves_io.rs:25-48, map_io.rs the same)"""
    BLACK, WHITE = (0, 0, 0), (255, 255, 255)
    RED, LIME, BLUE = (255, 0, 0), (0, 255, 0), (0, 0, 255)
    YELLOW, CYAN, MAGENTA = (255, 255, 0), (0, 255, 255), (255, 0, 255)
    MAROON, OLIVE, GREEN = (128, 0, 0), (128, 128, 0), (0, 128, 0)
    PURPLE, TEAL, NAVY = (128, 0, 128), (0, 128, 128), (0, 0, 128)
    GRAY1, GRAY2, GRAY3, GRAY4 = (30, 30, 30), (60, 60, 60), (90, 90, 90), (120, 120, 120)
    GRAY5, GRAY6, GRAY7, GRAY8 = (150, 150, 150), (180, 180, 180), (210, 210, 210), (240, 240, 240)


class TreeDeviceView(C.Structure):
    _fields_ = [("nx", C.c_void_p), ("ny", C.c_void_p), ("dist_root", C.c_void_p), ("parent", C.c_void_p), ("n_nodes", C.c_uint64)]


BEST_ENTRY = np.dtype([("cost", np.float64), ("rank", np.int32), ("n_nodes", np.int32)])      # porrt_best_entry, 16 bytes
UNIQUE_ID_BYTES = 128


class PorrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("porrt error %d: %s" % (code, msg))
        self.code = code


_LIB = None


def load_library():
    """dlopen the in-tree HIP library; fails loudly when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    sig("porrt_create", vp, C.c_int)
    sig("porrt_destroy", None, vp)
    sig("porrt_last_error", C.c_char_p, vp)
    sig("porrt_set_grid", C.c_int, vp, _u8p, C.c_uint32, C.c_uint32, _f64p, _f64p, C.c_int)
    sig("porrt_set_zones", C.c_int, vp, _u8p, C.c_double)
    sig("porrt_set_sampler", C.c_int, vp, _f64p, _f64p, C.c_uint64)
    sig("porrt_set_discrete_seed", C.c_int, vp, C.c_uint64)
    sig("porrt_set_samples", C.c_int, vp, _f64p, C.c_size_t)
    sig("porrt_set_worlds", C.c_int, vp, _u32p, C.c_size_t)
    sig("porrt_set_square_goal", C.c_int, vp, _f64p, _u64p, C.c_uint32, C.c_double)
    sig("porrt_set_observation_goal", C.c_int, vp, C.c_uint32)
    sig("porrt_grow", C.c_int, vp, _f64p, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int)
    sig("porrt_grow_batch", C.c_int, C.POINTER(C.c_void_p), C.c_uint32, _f64p, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int)
    sig("porrt_grow_batch_each", C.c_int, C.POINTER(C.c_void_p), C.c_uint32, _f64p, C.c_double, C.c_double, _u64p, _u64p, C.c_uint32, C.c_int)
    sig("porrt_num_nodes", C.c_uint64, vp)
    sig("porrt_num_iterations", C.c_uint64, vp)
    sig("porrt_get_tree", C.c_int, vp, _f64p, _i64p, _f64p)
    sig("porrt_get_trees", C.c_int, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p))
    sig("porrt_num_final", C.c_uint64, vp)
    sig("porrt_get_final_ids", C.c_int, vp, _u64p)
    sig("porrt_get_final_masks", C.c_int, vp, _u64p)
    sig("porrt_get_reach", C.c_int, vp, _u64p)
    sig("porrt_get_node_validity", C.c_int, vp, _u32p)
    sig("porrt_num_edges", C.c_uint64, vp)
    sig("porrt_get_edges", C.c_int, vp, _u32p, _u32p, _u32p)
    sig("porrt_is_final_set_complete", C.c_int, vp)
    sig("porrt_n_worlds", C.c_int, vp)
    sig("porrt_get_validities", C.c_int, vp, _u64p)
    sig("porrt_get_zone_positions", C.c_int, vp, _f64p)
    sig("porrt_best_solution", C.c_uint64, vp, vp, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_best_cost", C.c_int, vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64))
    sig("porrt_grow_prm", C.c_int, vp, _f64p, C.c_double, C.c_double, C.c_uint64)
    sig("porrt_prm_plan_path", C.c_int64, vp, _f64p, _f64p, C.c_void_p, C.c_uint64)
    sig("porrt_prm_plan_paths", C.c_int64, vp, _f64p, _f64p, C.c_uint64, _u64p, C.c_void_p, C.c_uint64)
    sig("porrt_prm_get_paths", C.c_int64, vp, C.c_void_p, C.c_uint64)
    sig("porrt_prm_paths_info", C.c_int, vp, C.POINTER(PrmPathsInfo))
    sig("porrt_build_belief_graph", C.c_int, vp, _f64p, C.c_uint32)
    sig("porrt_bg_num_beliefs", C.c_uint64, vp)
    sig("porrt_bg_num_nodes", C.c_uint64, vp)
    sig("porrt_bg_num_edges", C.c_uint64, vp)
    sig("porrt_bg_get_beliefs", C.c_int, vp, _f64p)
    sig("porrt_bg_get_observable_zones", C.c_int, vp, _u64p)
    sig("porrt_bg_get_node_types", C.c_int, vp, _u8p)
    sig("porrt_bg_get_children", C.c_int, vp, _u64p, C.c_void_p)
    sig("porrt_bg_get_parents", C.c_int, vp, _u64p, C.c_void_p)
    sig("porrt_bg_get_seconds", C.c_int, vp, _f64p, C.c_uint32)
    sig("porrt_bg_compute_expected_costs", C.c_int, vp)
    sig("porrt_bg_get_expected_costs", C.c_int, vp, _f64p)
    sig("porrt_bg_expected_cost_of", C.c_int, vp, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_bg_get_dp_info", C.c_int, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32))
    sig("porrt_bg_get_dp_sweep_rows", C.c_uint64, vp)
    sig("porrt_bg_extract_policy", C.c_int64, vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_conditional_dijkstra", C.c_int, C.c_int, C.c_uint64, _f64p, _u32p, _f64p, C.c_uint32, C.c_uint32, _u8p, _u64p, _u32p, _u64p, _u32p,
        _u64p, C.c_uint64, _f64p)
    sig("porrt_bg_refine_policy", C.c_int64, vp, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_refine_policy", C.c_int64, vp, C.c_uint64, _f64p, _i64p, _u64p, _u32p, _f64p, C.c_uint32, C.c_uint32, C.c_uint64,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_bg_get_refine_info", C.c_int, vp, C.POINTER(C.c_double), C.POINTER(C.c_double))
    sig("porrt_best_cost_batch", C.c_int, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_double))
    sig("porrt_get_metrics", C.c_int, vp, C.POINTER(Metrics))
    sig("porrt_set_option", C.c_int, vp, C.c_char_p, C.c_int64)
    sig("porrt_get_option", C.c_int, vp, C.c_char_p, C.POINTER(C.c_int64))
    sig("porrt_selftest", C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
    sig("porrt_comm_unique_id", C.c_int, C.c_void_p)
    sig("porrt_comm_create", vp, C.c_int, C.c_int, C.c_int, C.c_void_p)
    sig("porrt_comm_destroy", None, vp)
    sig("porrt_comm_last_error", C.c_char_p, vp)
    sig("porrt_exchange_best", C.c_int, vp, C.POINTER(C.c_void_p), C.c_uint32, _u32p, C.c_uint32, C.c_void_p)
    sig("porrt_exchange_num_nodes", C.c_uint64, vp, C.c_uint32)
    sig("porrt_exchange_get_tree", C.c_int, vp, C.c_uint32, _f64p, _i64p, _f64p)
    sig("porrt_exchange_decide", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)
    sig("porrt_exchange_agree", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32))
    sig("porrt_tree_device", TreeDeviceView, vp)
    sig("porrt_host_pin", C.c_int, vp, C.c_size_t)
    sig("porrt_host_unpin", C.c_int, vp)
    sig("porrt_exchange_tables", C.c_int, vp, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p)
    sig("porrt_comm_test_new_ops", vp, C.c_int, C.c_int, C.c_void_p)
    sig("porrt_comm_usable", C.c_int, vp)
    sig("porrt_comm_set_timeout_ms", C.c_int, vp, C.c_int)
    sig("porrt_comm_test_new", vp, C.c_int, C.c_int)
    sig("porrt_comm_test_fail", C.c_int, vp, C.c_int, C.c_int)
    sig("porrt_comm_test_aborts", C.c_int, vp)
    sig("porrt_grow_mm_prm", C.c_int, vp, _f64p, _f64p, C.c_uint32, C.c_double, C.c_double, C.c_uint64)
    for nm in ("modes", "transitions", "beliefs"):
        sig("porrt_mm_num_" + nm, C.c_uint64, vp)
    sig("porrt_mm_get_mode", C.c_int, vp, C.c_uint64, _f64p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
    sig("porrt_mm_get_mode_graph", C.c_int, vp, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
    sig("porrt_mm_get_transition", C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_uint64))
    sig("porrt_mm_get_transition_pairs", C.c_int, vp, C.c_uint64, C.c_void_p)
    sig("porrt_mm_get_seconds", C.c_int, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
    sig("porrt_mm_build_belief_graph", C.c_int, vp)
    for nm in ("nodes", "edges", "finals"):
        sig("porrt_mm_bg_num_" + nm, C.c_uint64, vp)
    sig("porrt_mm_bg_get_graph", C.c_int, vp, *([C.c_void_p] * 8))
    sig("porrt_mm_compute_expected_costs", C.c_int, vp)
    sig("porrt_mm_get_expected_costs", C.c_int, vp, _f64p)
    sig("porrt_mm_extract_policy", C.c_int64, vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_mm_refine_policy", C.c_int64, vp, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_mm_plan", C.c_int64, vp, _f64p, _f64p, C.c_uint32, C.c_double, C.c_double, C.c_uint64)
    sig("porrt_mm_get_plan_seconds", C.c_int, vp, _f64p, C.c_uint32)
    sig("porrt_mm_get_dp_info", C.c_int, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int))
    sig("porrt_read_pgm", C.c_int, C.c_char_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
    sig("porrt_read_pgm_mem", C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
    sig("porrt_graph_write_json", C.c_int, C.c_char_p, C.c_uint64, _f64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, C.c_uint64, C.c_uint64, _u8p)
    sig("porrt_graph_save_json", C.c_int, vp, C.c_char_p)
    sig("porrt_graph_load_json", vp, C.c_char_p, C.c_char_p, C.c_size_t)
    sig("porrt_graph_file_free", None, vp)
    for nm in ("nodes", "children", "parents", "validities", "worlds"):
        sig("porrt_graph_file_num_" + nm, C.c_uint64, vp)
    sig("porrt_graph_file_get", C.c_int, vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
    sig("porrt_tamp_rrt_plan", C.c_int64, vp, _f64p, _f64p, C.c_uint32, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_double, C.c_uint32)
    sig("porrt_tamp_rrt_policy", C.c_int64, vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_tamp_rrt_get_info", C.c_int, vp, C.POINTER(TampInfo))
    sig("porrt_tamp_rrt_plan_viewpoints", C.c_int64, vp, _f64p, _f64p, C.c_uint32, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_double,
        C.c_uint32, C.c_uint32)
    sig("porrt_tamp_rrt_get_viewpoints_info", C.c_int, vp, C.POINTER(TampViewpointsInfo))
    sig("porrt_tamp_rrt_plan_astar", C.c_int64, vp, _f64p, _f64p, C.c_uint32, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_double,
        C.c_uint32)
    sig("porrt_tamp_rrt_get_astar_info", C.c_int, vp, C.POINTER(TampAstarInfo))
    sig("porrt_tamp_astar_nodes", C.c_int64, vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_tamp_shortcut_paths_resident", C.c_int, vp, C.c_void_p, _u64p, C.c_uint64, C.c_void_p)
    sig("porrt_tamp_rrt_plan_astar_batch", C.c_int64, vp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_double,
        C.c_uint64, C.c_uint64, C.c_double, C.c_uint32)
    sig("porrt_tamp_batch_get_plan", C.c_int, vp, C.c_uint32, C.POINTER(TampBatchPlan))
    sig("porrt_tamp_batch_policy", C.c_int64, vp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double))
    sig("porrt_tamp_batch_astar_nodes", C.c_int64, vp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_tamp_rrt_plan_batch", C.c_int64, vp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double,
        C.c_double, C.c_uint64, C.c_uint64, C.c_double, C.c_uint32)
    sig("porrt_tamp_batch_get_pruned", C.c_int, vp, C.c_uint32, C.POINTER(C.c_uint64))
    sig("porrt_tamp_batch_bnb_nodes", C.c_int64, vp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_solutions", C.c_int, C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
        C.c_void_p, C.c_uint64)
    sig("porrt_best_paths", C.c_int, C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_uint64, _u64p, _f64p)
    sig("porrt_tamp_shortcut_paths", C.c_int, vp, C.c_void_p, _u64p, C.c_uint64, C.c_void_p)
    sig("porrt_qmdp_plan", C.c_int, vp)
    sig("porrt_qmdp_get_costs", C.c_int, vp, _f64p)
    sig("porrt_qmdp_info", C.c_int, vp, C.POINTER(QmdpInfo))
    sig("porrt_qmdp_react", C.c_int64, vp, _f64p, _f64p, C.c_uint32, _f64p, C.c_uint64, _u64p, _u64p, C.c_void_p, C.c_uint64)
    sig("porrt_qmdp_policy_graph", C.c_int, vp)
    sig("porrt_qmdp_policy_graph_get", C.c_int, vp, vp, vp, vp, vp, vp, vp)
    sig("porrt_qmdp_policy_graph_info", C.c_int, vp, C.POINTER(PolicyGraphInfo))
    sig("porrt_policy_graph", C.c_int, C.c_int, C.c_uint64, C.c_uint32, _u64p, _u32p, vp, vp, vp, C.POINTER(PolicyGraphInfo))
    sig("porrt_qmdp_costs", C.c_int, C.c_int, C.c_uint64, _f64p, _u32p, _u64p, C.c_uint32, C.c_uint32, _u64p, _u32p, _u64p, _u64p, _f64p)
    sig("porrt_bg_extract_policies", C.c_int64, vp, _u64p, C.c_uint64, _u64p, _u8p, _f64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_bg_get_policies", C.c_int64, vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_mm_extract_policies", C.c_int64, vp, _u64p, C.c_uint64, _u64p, _u8p, _f64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_mm_get_policies", C.c_int64, vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_extract_policies", C.c_int64, C.c_int, C.c_uint64, _f64p, _u32p, _f64p, C.c_uint32, C.c_uint32, _u32p, _u64p, _u32p, _f64p,
        _u64p, C.c_uint64, C.c_uint64, _u64p, _u8p, _f64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_policies_info", C.c_int, vp, C.POINTER(PoliciesInfo))
    for nm in ("porrt_bg_refine_policies", "porrt_mm_refine_policies"):
        sig(nm, C.c_int64, vp, C.c_uint64, _u64p, _u8p, _f64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_refine_policies", C.c_int64, vp, C.c_uint64, _u64p, _f64p, _i64p, _u64p, _u32p, _f64p, C.c_uint32, C.c_uint32, C.c_uint64,
        _u64p, _u8p, _f64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_refine_policies_info", C.c_int, vp, C.POINTER(RefinePoliciesInfo))
    sig("porrt_bg_reparent_policies", C.c_int64, vp, C.c_double, _u64p, _u8p, _f64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_bg_get_reparented_policies", C.c_int64, vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_bg_reparent_policy", C.c_int64, vp, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
    sig("porrt_reparent_policies", C.c_int64, vp, C.c_uint64, _f64p, _u32p, _f64p, C.c_uint32, C.c_uint32, _u64p, _u32p, C.c_uint64, _u64p, _u64p, _i64p,
        C.c_double, _u64p, _u8p, _f64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    sig("porrt_reparent_policies_info", C.c_int, vp, C.POINTER(ReparentPoliciesInfo))
    sig("porrt_plan_belief_space_batch", C.c_int64, vp, C.c_uint32, vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64)
    sig("porrt_plan_batch_get_policies", C.c_int64, vp, vp, vp, vp, vp, vp, C.c_uint64)
    sig("porrt_plan_batch_get_expected_costs", C.c_int, vp, C.c_uint32, vp)
    sig("porrt_plan_batch_info", C.c_int, vp, C.POINTER(PlanBatchInfo))
    sig("porrt_mm_plan_batch", C.c_int64, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, C.c_double, C.c_double, C.c_uint64, C.c_uint64,
        vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64)
    sig("porrt_mm_plan_batch_get_policies", C.c_int64, vp, vp, vp, vp, vp, vp, C.c_uint64)
    sig("porrt_mm_plan_batch_get_expected_costs", C.c_int, vp, C.c_uint32, vp)
    sig("porrt_mm_plan_batch_get_plan", C.c_int, vp, C.c_uint32, C.POINTER(MmBatchPlan))
    sig("porrt_mm_plan_batch_info", C.c_int, vp, C.POINTER(MmPlanBatchInfo))
    sig("porrt_canvas_create", vp, vp, C.c_uint32)
    sig("porrt_canvas_destroy", None, vp)
    sig("porrt_canvas_last_error", C.c_char_p, vp)
    sig("porrt_canvas_size", C.c_int, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
    sig("porrt_canvas_draw_lines", C.c_int, vp, _f64p, C.c_uint64, _u8p, C.c_float)
    sig("porrt_canvas_draw_path", C.c_int, vp, _f64p, C.c_uint64, _u8p)
    sig("porrt_canvas_draw_circles", C.c_int, vp, _f64p, C.c_uint64, C.c_double, _u8p)
    sig("porrt_canvas_draw_tree", C.c_int, vp, vp)
    sig("porrt_canvas_draw_full_graph", C.c_int, vp, vp)
    sig("porrt_canvas_draw_zones_observability", C.c_int, vp)
    sig("porrt_canvas_draw_policy", C.c_int, vp, _f64p, _i64p, C.c_uint64)
    sig("porrt_canvas_get_rgb", C.c_int, vp, _u8p)
    sig("porrt_canvas_save_png", C.c_int, vp, C.c_char_p)
    sig("porrt_write_png", C.c_int, C.c_char_p, _u8p, C.c_uint32, C.c_uint32)
    sig("porrt_canvas_get_info", C.c_int, vp, C.POINTER(DrawInfo))
    _LIB = L
    return L


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _policy_list(off, status, cost, oid, par, leaf, xy=None):
    """the answers of an extract_policies call as a list: ((oid, par, leaf[, xy]), cost) per query, None where its status is not 0"""
    out = []
    for q in range(len(status)):
        if status[q]:
            out.append(None)
            continue
        a, b = int(off[q]), int(off[q + 1])
        arrays = (oid[a:b], par[a:b], leaf[a:b]) + ((xy[a:b],) if xy is not None else ())
        out.append((arrays, float(cost[q])))
    return out


class Engine:
    """One porrt_ctx on one GPU (mirrors the `&mut self` RRT / PTO object of the reference)."""

    def __init__(self, device=0):
        self._l = load_library()
        self._c = self._l.porrt_create(device)
        if not self._c:
            raise PorrtError(-6, "porrt_create failed: no usable HIP device %d" % device)

    def close(self):
        if getattr(self, "_c", None):
            self._l.porrt_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise PorrtError(rc, self._l.porrt_last_error(self._c).decode())
        return rc

    def set_option(self, name, value):
        self._chk(self._l.porrt_set_option(self._c, name.encode(), int(value)))

    def set_grid(self, occ, low=(-1.0, -1.0), up=(1.0, 1.0), domain=DOMAIN_SHELF):
        occ = np.ascontiguousarray(occ, dtype=np.uint8)
        H, W = occ.shape
        self._chk(self._l.porrt_set_grid(self._c, occ, W, H, _f64(low), _f64(up), domain))

    def set_zones(self, zone_ids, visibility):
        self._chk(self._l.porrt_set_zones(self._c, np.ascontiguousarray(zone_ids, dtype=np.uint8), visibility))

    def set_sampler(self, low=(-1.0, -1.0), up=(1.0, 1.0), seed=0):
        self._chk(self._l.porrt_set_sampler(self._c, _f64(low), _f64(up), seed))

    def set_discrete_seed(self, seed):
        self._chk(self._l.porrt_set_discrete_seed(self._c, seed))

    def set_samples(self, xy):
        xy = _f64(xy).reshape(-1, 2)
        self._chk(self._l.porrt_set_samples(self._c, xy, xy.shape[0]))

    def set_worlds(self, worlds):
        w = np.ascontiguousarray(worlds, dtype=np.uint32)
        self._chk(self._l.porrt_set_worlds(self._c, w, w.size))

    def set_square_goal(self, centers, masks, l1_radius):
        centers = _f64(centers).reshape(-1, 2)
        masks = np.ascontiguousarray(masks, dtype=np.uint64)
        self._chk(self._l.porrt_set_square_goal(self._c, centers, masks, centers.shape[0], l1_radius))

    def set_observation_goal(self, zone_id):
        self._chk(self._l.porrt_set_observation_goal(self._c, zone_id))

    def n_worlds(self):
        return self._l.porrt_n_worlds(self._c)

    def validities(self):
        out = np.zeros(65, dtype=np.uint64)
        n = self._chk(self._l.porrt_get_validities(self._c, out))
        return out[:n].copy()

    def zone_positions(self):
        out = np.zeros((64, 2), dtype=np.float64)
        n = self._chk(self._l.porrt_get_zone_positions(self._c, out))
        return out[:n].copy()

    def grow(self, start, max_step, search_radius, n_iter_min, n_iter_max, batch_K=1024, mode=MODE_RRT):
        """RRT::grow_tree (rrt.rs:102-174) / PTO::grow_graph (pto.rs:55-139) on the GPU."""
        return self._chk(self._l.porrt_grow(self._c, _f64(start), max_step, search_radius, n_iter_min, n_iter_max,
                                            batch_K, mode))

    @staticmethod
    def grow_batch(engines, starts, max_step, search_radius, n_iter_min, batch_K=1024, mode=MODE_RRT, n_iter_max=None):
        """porrt_grow_batch / porrt_grow_batch_each: the same growth for several contexts of one GPU in one launch sequence, each
        running the reference's loop `while i < n_iter_min || (no solution && i < n_iter_max)`.  n_iter_min / n_iter_max: one
        number for all, or one per engine; n_iter_max = None: a fixed budget (= n_iter_min)."""
        engines = list(engines)
        arr = (C.c_void_p * len(engines))(*[e._c for e in engines])
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(len(engines), 2))
        if n_iter_max is None:
            n_iter_max = n_iter_min
        if np.ndim(n_iter_min) == 0 and np.ndim(n_iter_max) == 0:
            return engines[0]._chk(engines[0]._l.porrt_grow_batch(arr, len(engines), st.reshape(-1), max_step, search_radius,
                                                                   int(n_iter_min), int(n_iter_max), batch_K, mode))
        mn = np.ascontiguousarray(np.broadcast_to(np.asarray(n_iter_min, dtype=np.uint64), (len(engines),)))
        mx = np.ascontiguousarray(np.broadcast_to(np.asarray(n_iter_max, dtype=np.uint64), (len(engines),)))
        return engines[0]._chk(engines[0]._l.porrt_grow_batch_each(arr, len(engines), st.reshape(-1), max_step, search_radius, mn, mx, batch_K, mode))

    def num_nodes(self):
        return self._l.porrt_num_nodes(self._c)

    def num_iterations(self):
        return self._l.porrt_num_iterations(self._c)

    def num_final(self):
        return self._l.porrt_num_final(self._c)

    TAMP_SEARCH = {"branch_and_bound": 0, "astar": 1, "branch_and_bound_multiple_viewpoints": 2}

    def plan_tamp_rrt(self, start, belief, max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, goal_radius=0.05,
                      batch_K=128, search="branch_and_bound"):
        """MapShelfDomainTampRRT::plan(.., TampSearch) (porrt_tamp_rrt_plan): dict of the policy (xy, parents, is_leaf, beliefs,
        expected_cost) and the search's info.  Stream mode, wave width and pool size are the options tamp_streams / tamp_wave /
        tamp_pool.  This entry point runs branch_and_bound only and raises PorrtError (PORRT_ERR_INVALID) for the other two search
        kinds, which have methods of their own: plan_tamp_rrt_astar and plan_tamp_rrt_viewpoints."""
        if search not in self.TAMP_SEARCH:
            raise ValueError("search: one of %s" % sorted(self.TAMP_SEARCH))
        keep = self.get_option("tamp_search")
        self.set_option("tamp_search", self.TAMP_SEARCH[search])
        try:
            b = _f64(belief)
            n = self._chk(self._l.porrt_tamp_rrt_plan(self._c, _f64(start), b, b.size, max_step, search_radius, n_iter_min, n_iter_max,
                                                       goal_radius, batch_K))
        finally:
            self.set_option("tamp_search", keep)
        return self._tamp_policy(n, b.size)

    def _tamp_policy(self, n, nw):
        xy, par = np.zeros((n, 2)), np.zeros(n, dtype=np.int64)
        leaf, bel = np.zeros(n, dtype=np.uint8), np.zeros((n, nw))
        cost = C.c_double(0.0)
        self._chk(self._l.porrt_tamp_rrt_policy(self._c, xy.ctypes.data, par.ctypes.data, leaf.ctypes.data, bel.ctypes.data, n,
                                                C.byref(cost)))
        out = dict(xy=xy, parents=par, is_leaf=leaf, beliefs=bel, expected_cost=cost.value)
        out.update(self.tamp_info())
        return out

    def plan_tamp_rrt_viewpoints(self, start, belief, max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, goal_radius=0.05,
                                 batch_K=128, max_viewpoints=0):
        """MapShelfDomainTampRRT::plan(.., BranchAndBoundMultipleViewPoints) with the viewpoints of a query walked in ascending
        node id (porrt_tamp_rrt_plan_viewpoints): the dict of plan_tamp_rrt plus tamp_viewpoints_info().  max_viewpoints (ours, not
        the reference's): 0 = all, n = the n cheapest solutions per observation query."""
        b = _f64(belief)
        n = self._chk(self._l.porrt_tamp_rrt_plan_viewpoints(self._c, _f64(start), b, b.size, max_step, search_radius, n_iter_min, n_iter_max,
                                                              goal_radius, batch_K, max_viewpoints))
        out = self._tamp_policy(n, b.size)
        out.update(self.tamp_viewpoints_info())
        return out

    def plan_tamp_rrt_astar(self, start, belief, max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, goal_radius=0.05,
                            batch_K=128):
        """MapShelfDomainTampRRT::plan(.., AStar) with equal priorities popped in ascending search node id
        (porrt_tamp_rrt_plan_astar): the dict of plan_tamp_rrt plus tamp_astar_info().  tamp_streams / tamp_wave / tamp_pool as for
        plan_tamp_rrt (the wave width speculates; it never changes the result), tamp_arena_states = the path arena's first size."""
        b = _f64(belief)
        n = self._chk(self._l.porrt_tamp_rrt_plan_astar(self._c, _f64(start), b, b.size, max_step, search_radius, n_iter_min, n_iter_max,
                                                         goal_radius, batch_K))
        out = self._tamp_policy(n, b.size)
        out.update(self.tamp_astar_info())
        return out

    def tamp_astar_info(self):
        i = TampAstarInfo()
        self._chk(self._l.porrt_tamp_rrt_get_astar_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in TampAstarInfo._fields_}

    def tamp_astar_nodes(self):
        """the search nodes of the last plan_tamp_rrt_astar in id order (after a failed plan: those made so far):
        dict(parents, targets, ec, priority)"""
        n = self._chk(self._l.porrt_tamp_astar_nodes(self._c, None, None, None, None, 0))
        par, tgt = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        ec, pr = np.zeros(n), np.zeros(n)
        self._chk(self._l.porrt_tamp_astar_nodes(self._c, par.ctypes.data, tgt.ctypes.data, ec.ctypes.data, pr.ctypes.data, n))
        return dict(parents=par, targets=tgt, ec=ec, priority=pr)

    def plan_tamp_rrt_astar_batch(self, starts, priors, seeds=None, max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000,
                                  goal_radius=0.05, batch_K=128):
        """porrt_tamp_rrt_plan_astar_batch: many A* plans on this engine's map in one call, plan p from starts[p] with prior
        priors[p] and root stream seed seeds[p] (None: the engine's sampler seed for every plan).  Each plan is, bit for bit, what
        plan_tamp_rrt_astar gives alone on an engine whose sampler seed is seeds[p].  Returns one dict per plan with the keys of
        plan_tamp_rrt_astar's dict plus `status` (0, or -10 for a plan that found no path: it has no policy arrays, and fail_* say
        where it failed).  search_cost, expected_cost, search_nodes, queries, waves, speculated, zone_order and fail_* are the
        plan's own; the seconds, streams, wave, pool and the arena figures are the call's.  A failed plan does not raise; every
        other failure raises PorrtError for the whole call."""
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, 2))
        n = st.shape[0]
        pr = np.ascontiguousarray(np.asarray(priors, dtype=np.float64).reshape(n, -1) if n else np.zeros((0, 1)))
        nw = pr.shape[1]
        sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(n))
        self._chk(self._l.porrt_tamp_rrt_plan_astar_batch(self._c, n, st.ctypes.data, pr.ctypes.data, None if sd is None else sd.ctypes.data,
                                                           nw, max_step, search_radius, n_iter_min, n_iter_max, goal_radius, batch_K))
        return self._tamp_batch_plans(n, nw)

    def _tamp_batch_plans(self, n, nw, pruned=False):
        """the per-plan dicts of the last batch call of either search; pruned: the plan's own count replaces the call's"""
        call = self.tamp_info()
        call.update(self.tamp_astar_info())
        out = []
        for p in range(n):
            rec = TampBatchPlan()
            self._chk(self._l.porrt_tamp_batch_get_plan(self._c, p, C.byref(rec)))
            d = dict(call)
            d.update({k: getattr(rec, k) for k in ("status", "fail_node", "fail_zone", "fail_query", "search_cost", "expected_cost",
                                                   "search_nodes", "queries", "waves", "speculated")})
            d["zone_order"] = [int(rec.zone_order[k]) for k in range(rec.n_order)]
            if pruned:
                own = C.c_uint64(0)
                self._chk(self._l.porrt_tamp_batch_get_pruned(self._c, p, C.byref(own)))
                d["pruned"] = own.value
            if rec.status == 0:
                m = int(rec.policy_nodes)
                xy, par = np.zeros((m, 2)), np.zeros(m, dtype=np.int64)
                leaf, bel = np.zeros(m, dtype=np.uint8), np.zeros((m, nw))
                self._chk(self._l.porrt_tamp_batch_policy(self._c, p, xy.ctypes.data, par.ctypes.data, leaf.ctypes.data, bel.ctypes.data, m, None))
                d.update(xy=xy, parents=par, is_leaf=leaf, beliefs=bel)
            out.append(d)
        return out

    def tamp_batch_astar_nodes(self, plan):
        """the search nodes of plan `plan` of the last plan_tamp_rrt_astar_batch in id order (of a failed plan: those made so far):
        dict(parents, targets, ec, priority)"""
        n = self._chk(self._l.porrt_tamp_batch_astar_nodes(self._c, plan, None, None, None, None, 0))
        par, tgt = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        ec, pr = np.zeros(n), np.zeros(n)
        self._chk(self._l.porrt_tamp_batch_astar_nodes(self._c, plan, par.ctypes.data, tgt.ctypes.data, ec.ctypes.data, pr.ctypes.data, n))
        return dict(parents=par, targets=tgt, ec=ec, priority=pr)

    def plan_tamp_rrt_batch(self, starts, priors, seeds=None, discrete_seeds=None, max_step=0.1, search_radius=2.0, n_iter_min=2500,
                            n_iter_max=10000, goal_radius=0.05, batch_K=128):
        """porrt_tamp_rrt_plan_batch: many branch-and-bound plans on this engine's map in one call, plan p from starts[p] with prior
        priors[p], root stream seed seeds[p] (None: the engine's sampler seed for every plan) and a discrete sampler of its own
        seeded discrete_seeds[p] (None: seeds[p]).  Each plan is, bit for bit, what plan_tamp_rrt gives alone on a fresh engine
        seeded alike at the same tamp_wave.  Returns one dict per plan in the shape plan_tamp_rrt_astar_batch returns: `status` (0,
        or -10 for a plan that found no path: it has no policy arrays, and fail_* say where it failed), search_cost, expected_cost,
        search_nodes, queries, waves, pruned, zone_order and fail_* are the plan's own (speculated is 0); the seconds, streams, wave,
        pool and the arena figures are the call's.  The engine's own samplers are left alone.  A failed plan does not raise; every
        other failure raises PorrtError for the whole call."""
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, 2))
        n = st.shape[0]
        pr = np.ascontiguousarray(np.asarray(priors, dtype=np.float64).reshape(n, -1) if n else np.zeros((0, 1)))
        nw = pr.shape[1]
        sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(n))
        ds = None if discrete_seeds is None else np.ascontiguousarray(np.asarray(discrete_seeds, dtype=np.uint64).reshape(n))
        self._chk(self._l.porrt_tamp_rrt_plan_batch(self._c, n, st.ctypes.data, pr.ctypes.data, None if sd is None else sd.ctypes.data,
                                                     None if ds is None else ds.ctypes.data, nw, max_step, search_radius, n_iter_min,
                                                     n_iter_max, goal_radius, batch_K))
        return self._tamp_batch_plans(n, nw, pruned=True)

    def tamp_batch_bnb_nodes(self, plan):
        """the search nodes of plan `plan` of the last plan_tamp_rrt_batch in id order (of a failed plan: those made up to and
        including the failing wave): dict(parents, targets, ec, pushed)"""
        n = self._chk(self._l.porrt_tamp_batch_bnb_nodes(self._c, plan, None, None, None, None, 0))
        par, tgt = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        ec, pushed = np.zeros(n), np.zeros(n, dtype=np.uint8)
        self._chk(self._l.porrt_tamp_batch_bnb_nodes(self._c, plan, par.ctypes.data, tgt.ctypes.data, ec.ctypes.data, pushed.ctypes.data, n))
        return dict(parents=par, targets=tgt, ec=ec, pushed=pushed)

    def tamp_viewpoints_info(self):
        i = TampViewpointsInfo()
        self._chk(self._l.porrt_tamp_rrt_get_viewpoints_info(self._c, C.byref(i)))
        d = {k: getattr(i, k) for k, _ in TampViewpointsInfo._fields_ if k not in ("ranks", "n_ranks")}
        d["viewpoint_ranks"] = [int(i.ranks[k]) for k in range(i.n_ranks)]
        return d

    def solutions(self):
        """RRT::get_solutions (rrt.rs:195-246) of the last grow, on the device: [(id, path n x 2, cost)] in ascending node id"""
        return Engine.solutions_batch([self])[0]

    @staticmethod
    def solutions_batch(engines):
        """porrt_solutions: per engine [(id, path n x 2, cost)], all trees walked in one device call (no tree is downloaded)"""
        L, e0, n = engines[0]._l, engines[0], len(engines)
        arr = (C.c_void_p * n)(*[e._c for e in engines])
        ns, nst = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        e0._chk(L.porrt_solutions(arr, n, ns.ctypes.data, nst.ctypes.data, None, None, None, 0, None, 0))
        S, X = int(ns.sum()), int(nst.sum())
        ids, lens = np.zeros(max(S, 1), dtype=np.uint64), np.zeros(max(S, 1), dtype=np.uint64)
        costs, xy = np.zeros(max(S, 1)), np.zeros((max(X, 1), 2))
        e0._chk(L.porrt_solutions(arr, n, ns.ctypes.data, nst.ctypes.data, ids.ctypes.data, lens.ctypes.data, costs.ctypes.data, S,
                                  xy.ctypes.data, X))
        out, s, at = [], 0, 0
        for q in range(n):
            row = []
            for _ in range(int(ns[q])):
                k = int(lens[s])
                row.append((int(ids[s]), xy[at:at + k].copy(), float(costs[s])))
                s, at = s + 1, at + k
            out.append(row)
        return out

    def tamp_info(self):
        i = TampInfo()
        self._chk(self._l.porrt_tamp_rrt_get_info(self._c, C.byref(i)))
        d = {k: getattr(i, k) for k, _ in TampInfo._fields_ if k not in ("zone_order", "n_order", "pad")}
        d["zone_order"] = [int(i.zone_order[k]) for k in range(i.n_order)]
        return d

    @staticmethod
    def best_paths(engines):
        """porrt_best_paths: [(path n x 2, cost) or None] per engine of the last grow_batch, gathered on the device"""
        L = engines[0]._l
        arr = (C.c_void_p * len(engines))(*[e._c for e in engines])
        lens, costs = np.zeros(len(engines), dtype=np.uint64), np.zeros(len(engines))
        engines[0]._chk(L.porrt_best_paths(arr, len(engines), None, 0, lens, costs))
        xy = np.zeros((max(int(lens.sum()), 1), 2))
        engines[0]._chk(L.porrt_best_paths(arr, len(engines), xy.ctypes.data, int(lens.sum()), lens, costs))
        out, at = [], 0
        for n, c in zip(lens.tolist(), costs.tolist()):
            out.append((xy[at:at + n].copy(), c) if n else None)
            at += n
        return out

    def tamp_shortcut(self, paths, resident=False):
        """the planner's shortcut (map_shelves_tamp_rrt.rs:565-617) of each path (a list of n x 2 arrays), on the device.
        resident: through the device-resident input form the A* planner uses (the paths start in its arena)"""
        arrs = [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 2)) for p in paths]
        off = np.zeros(len(arrs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(a) for a in arrs]) if arrs else []
        xy = np.concatenate(arrs) if arrs and off[-1] else np.zeros((0, 2))
        out = np.zeros_like(xy)
        call = self._l.porrt_tamp_shortcut_paths_resident if resident else self._l.porrt_tamp_shortcut_paths
        self._chk(call(self._c, xy.ctypes.data, off, len(arrs), out.ctypes.data))
        return [out[int(off[k]):int(off[k + 1])].copy() for k in range(len(arrs))]

    def canvas(self, factor=1):
        """Map::open + resize(factor): the occupancy raster as an RGB canvas on this engine's device (porrt_canvas_create)"""
        return Canvas(self, factor)

    def get_option(self, name):
        v = C.c_int64(0)
        self._chk(self._l.porrt_get_option(self._c, name.encode(), C.byref(v)))
        return v.value

    def tree(self):
        n = self.num_nodes()
        xy = np.zeros((n, 2))
        parent = np.zeros(n, dtype=np.int64)
        dist = np.zeros(n)
        self._chk(self._l.porrt_get_tree(self._c, xy, parent, dist))
        return xy, parent, dist

    @staticmethod
    def trees(engines, buffers=None):
        """porrt_get_trees: the trees of several contexts of one device in one call -> [(xy, parent, dist_root), ...].
        buffers: per engine (xy [cap, 2] f64, parent [cap] i64, dist [cap] f64) to fill instead of new arrays (a caller that
        fetches trees again and again keeps its memory mapped: fresh pages cost more than the copies); views of them come back."""
        n = len(engines)
        sizes = [e.num_nodes() for e in engines]
        if buffers is None:
            out = [(np.empty((m, 2)), np.empty(m, dtype=np.int64), np.empty(m)) for m in sizes]
        else:
            out = []
            for m, (bxy, bp, bd) in zip(sizes, buffers):
                if len(bxy) < m or len(bp) < m or len(bd) < m or bxy.dtype != np.float64 or bp.dtype != np.int64 or bd.dtype != np.float64:
                    raise ValueError("trees: a buffer is too small or of the wrong type")
                out.append((bxy[:m], bp[:m], bd[:m]))
        arr = (C.c_void_p * n)(*[e._c for e in engines])
        ptrs = [(C.c_void_p * n)(*[o[k].ctypes.data for o in out]) for k in range(3)]
        rc = engines[0]._l.porrt_get_trees(arr, n, ptrs[0], ptrs[1], ptrs[2])
        engines[0]._chk(rc)
        return out

    @staticmethod
    def pin_buffers(buffers):
        """porrt_host_pin for the arrays of `buffers` (as Engine.trees takes them): a later trees(engines, buffers) lets one kernel write
        every tree straight into them.  The arrays must stay alive until unpin_buffers(buffers)."""
        L = load_library()
        for arrs in buffers:
            for a in arrs:
                rc = L.porrt_host_pin(a.ctypes.data, a.nbytes)
                if rc:
                    raise PorrtError(rc, "porrt_host_pin (%d bytes)" % a.nbytes)

    @staticmethod
    def unpin_buffers(buffers):
        L = load_library()
        for arrs in buffers:
            for a in arrs:
                L.porrt_host_unpin(a.ctypes.data)

    def final_ids(self):
        n = self._l.porrt_num_final(self._c)
        ids = np.zeros(n, dtype=np.uint64)
        if n:
            self._chk(self._l.porrt_get_final_ids(self._c, ids))
        return ids

    def final_masks(self):
        n = self._l.porrt_num_final(self._c)
        m = np.zeros(n, dtype=np.uint64)
        if n:
            self._chk(self._l.porrt_get_final_masks(self._c, m))
        return m

    def reach(self):
        m = np.zeros(self.num_nodes(), dtype=np.uint64)
        self._chk(self._l.porrt_get_reach(self._c, m))
        return m

    def node_validity(self):
        v = np.zeros(self.num_nodes(), dtype=np.uint32)
        self._chk(self._l.porrt_get_node_validity(self._c, v))
        return v

    def edges(self):
        n = self._l.porrt_num_edges(self._c)
        f = np.zeros(n, dtype=np.uint32)
        t = np.zeros(n, dtype=np.uint32)
        v = np.zeros(n, dtype=np.uint32)
        if n:
            self._chk(self._l.porrt_get_edges(self._c, f, t, v))
        return f, t, v

    def is_final_set_complete(self):
        return bool(self._l.porrt_is_final_set_complete(self._c))

    def best_solution(self):
        cost = C.c_double(0.0)
        n = self._l.porrt_best_solution(self._c, None, 0, C.byref(cost))
        if n == 0:
            return None
        path = np.zeros((n, 2))
        self._l.porrt_best_solution(self._c, path.ctypes.data_as(C.c_void_p), n, C.byref(cost))
        return path, cost.value

    def best_cost(self):
        """cost of best_solution()'s path, evaluated on the device (no tree download); None = no solution"""
        cost, fid = C.c_double(0.0), C.c_uint64(0)
        r = self._chk(self._l.porrt_best_cost(self._c, C.byref(cost), C.byref(fid)))
        return cost.value if r else None

    @staticmethod
    def best_cost_batch(engines):
        """best_cost() of every engine (inf = no solution); one launch when they are the last grow_batch's members"""
        n = len(engines)
        arr = (C.c_void_p * n)(*[e._c for e in engines])
        costs = np.zeros(n)
        rc = engines[0]._l.porrt_best_cost_batch(arr, n, costs.ctypes.data_as(C.POINTER(C.c_double)))
        if rc < 0:
            engines[0]._chk(rc)
        return costs

    def grow_prm(self, start, max_step, search_radius, n_iter):
        """PRM::init + PRM::grow_graph (prm.rs:33-109); nodes and edges through tree() / edges()"""
        return self._chk(self._l.porrt_grow_prm(self._c, np.ascontiguousarray(start, dtype=np.float64), max_step, search_radius, n_iter))

    def prm_plan_path(self, start, goal):
        """PRM::plan_path (prm.rs:111-123): array of states, empty when start and goal are not connected"""
        a, b = np.ascontiguousarray(start, dtype=np.float64), np.ascontiguousarray(goal, dtype=np.float64)
        n = self._l.porrt_prm_plan_path(self._c, a, b, None, 0)
        if n < 0:
            self._chk(int(n))
        out = np.zeros((n, 2))
        if n:
            self._l.porrt_prm_plan_path(self._c, a, b, out.ctypes.data_as(C.c_void_p), n)
        return out

    def prm_plan_paths(self, starts, goals):
        """porrt_prm_plan_paths: PRM::plan_path for every pair (starts[i], goals[i]) in one call -- a list of (k, 2) arrays, each
        equal to prm_plan_path(starts[i], goals[i]) (empty when start and goal are not connected)"""
        s, g = _f64(starts).reshape(-1, 2), _f64(goals).reshape(-1, 2)
        if len(s) != len(g):
            raise ValueError("prm_plan_paths: one goal per start")
        n = len(s)
        off = np.zeros(n + 1, dtype=np.uint64)
        total = self._chk(int(self._l.porrt_prm_plan_paths(self._c, s.reshape(-1), g.reshape(-1), n, off, None, 0)))
        xy = np.zeros((total, 2))
        if total:
            self._chk(int(self._l.porrt_prm_get_paths(self._c, xy.ctypes.data_as(C.c_void_p), total)))
        return [xy[int(off[i]):int(off[i + 1])] for i in range(n)]

    def prm_paths_info(self):
        """porrt_prm_paths_info of the last prm_plan_paths: queries, rows, sweeps, passes, ms_device, ms_wall, ms_nearest"""
        i = PrmPathsInfo()
        self._chk(self._l.porrt_prm_paths_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in PrmPathsInfo._fields_}

    # ---- QMdpPolicyExtractor (qmdp_policy_extractor.rs)
    def qmdp_plan(self):
        """plan_qmdp (:23-35) on the graph of the last PTO growth; the costs stay on the device"""
        self._chk(self._l.porrt_qmdp_plan(self._c))

    def qmdp_costs(self):
        """cost_to_goals as an (n_worlds, N) array"""
        out = np.zeros((self.n_worlds(), self.num_nodes()))
        self._chk(self._l.porrt_qmdp_get_costs(self._c, out.reshape(-1)))
        return out

    def qmdp_react(self, starts, beliefs, horizons, with_common_len=False):
        """react_qmdp (:38-49) for every (starts[i], beliefs[i], horizons[i]) in one call: a list with one entry per query, each a list
        of n_worlds (k, 2) arrays (paths[w]); with_common_len also returns the number of common-path states of every query"""
        s, b, h = _f64(starts).reshape(-1, 2), np.atleast_2d(_f64(beliefs)), _f64(horizons).reshape(-1)
        n, nw = len(s), b.shape[1]
        if len(b) != n or len(h) != n:
            raise ValueError("qmdp_react: one belief and one horizon per start")
        off, cl = np.zeros(n * nw + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        args = (self._c, s.reshape(-1), np.ascontiguousarray(b).reshape(-1), nw, h, n, off, cl)
        total = self._chk(int(self._l.porrt_qmdp_react(*args, None, 0)))
        xy = np.zeros((total, 2))
        if total:
            self._chk(int(self._l.porrt_qmdp_react(*args, xy.ctypes.data_as(C.c_void_p), total)))
        paths = [[xy[int(off[q * nw + w]):int(off[q * nw + w + 1])] for w in range(nw)] for q in range(n)]
        return (paths, cl[:n].copy()) if with_common_len else paths

    def qmdp_policy_graph(self):
        """get_policy_graph (pto_graph.rs:363-419) on the graph and costs of the last qmdp_plan; the result stays with the context"""
        self._chk(self._l.porrt_qmdp_policy_graph(self._c))

    def qmdp_policy_graph_get(self):
        """the last qmdp_policy_graph: dict of keep, how (one byte per adjacency entry in push order) and the pruned children and
        parents lists as CSR (child_off, child_ids, parent_off, parent_ids)"""
        i = self.qmdp_policy_graph_info()
        n = self.num_nodes()
        keep, how = np.zeros(i["entries"], dtype=np.uint8), np.zeros(i["entries"], dtype=np.uint8)
        co, po = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
        ci, pi = np.zeros(i["kept"], dtype=np.uint32), np.zeros(i["kept"], dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self._l.porrt_qmdp_policy_graph_get(self._c, p(keep), p(how), p(co), p(ci), p(po), p(pi)))
        return dict(keep=keep.astype(bool), how=how, child_off=co, child_ids=ci, parent_off=po, parent_ids=pi)

    def qmdp_policy_graph_info(self):
        """porrt_qmdp_policy_graph_info of the last qmdp_policy_graph"""
        i = PolicyGraphInfo()
        self._chk(self._l.porrt_qmdp_policy_graph_info(self._c, C.byref(i)))
        return i.as_dict()

    def qmdp_info(self):
        """porrt_qmdp_info of the last qmdp_plan / qmdp_react"""
        i = QmdpInfo()
        self._chk(self._l.porrt_qmdp_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in QmdpInfo._fields_}

    # ---- belief-space expansion (PTO::build_belief_graph, pto.rs:185-259)
    def build_belief_graph(self, start_belief):
        b = np.ascontiguousarray(start_belief, dtype=np.float64)
        self._chk(self._l.porrt_build_belief_graph(self._c, b, len(b)))

    def belief_graph(self, lists=True):
        """beliefs [B, n_worlds], node types [N*B], (child_off, child_ids), (parent_off, parent_ids)"""
        B, NB, E = (self._l.porrt_bg_num_beliefs(self._c), self._l.porrt_bg_num_nodes(self._c), self._l.porrt_bg_num_edges(self._c))
        beliefs = np.zeros((B, self.n_worlds()))
        types = np.zeros(NB, dtype=np.uint8)
        coff, poff = np.zeros(NB + 1, dtype=np.uint64), np.zeros(NB + 1, dtype=np.uint64)
        cid, pid = np.zeros(max(E, 1) if lists else 1, dtype=np.uint32), np.zeros(max(E, 1) if lists else 1, dtype=np.uint32)
        self._chk(self._l.porrt_bg_get_beliefs(self._c, beliefs))
        self._chk(self._l.porrt_bg_get_node_types(self._c, types))
        self._chk(self._l.porrt_bg_get_children(self._c, coff, cid.ctypes.data_as(C.c_void_p) if lists else None))
        self._chk(self._l.porrt_bg_get_parents(self._c, poff, pid.ctypes.data_as(C.c_void_p) if lists else None))
        return beliefs, types, (coff, cid[:E] if lists else None), (poff, pid[:E] if lists else None)

    def bg_num_edges(self):
        return self._l.porrt_bg_num_edges(self._c)

    def observable_zones(self):
        m = np.zeros(self.num_nodes(), dtype=np.uint64)
        self._chk(self._l.porrt_bg_get_observable_zones(self._c, m))
        return m

    def bg_seconds(self):
        v = np.zeros(8)
        self._chk(self._l.porrt_bg_get_seconds(self._c, v, 8))
        keys = ("total_s", "device_s", "host_tables_s", "reach_s", "fold_table_s", "adjacency_s", "alloc_upload_s", "edges_fetch_s")
        return dict(zip(keys, v.tolist()))

    def compute_expected_costs(self):
        """PTO::compute_expected_costs_to_goals on the device (pto.rs:261-275)"""
        self._chk(self._l.porrt_bg_compute_expected_costs(self._c))

    def expected_costs(self):
        d = np.zeros(self._l.porrt_bg_num_nodes(self._c))
        self._chk(self._l.porrt_bg_get_expected_costs(self._c, d))
        return d

    def expected_cost_of(self, belief_node=0):
        v = C.c_double(0.0)
        self._chk(self._l.porrt_bg_expected_cost_of(self._c, belief_node, C.byref(v)))
        return v.value

    def extract_policy(self):
        """PTO::extract_policy: (original belief node ids, parents (-1 = root), leaf flags), expected cost of the root"""
        cost = C.c_double(0.0)
        n = self._l.porrt_bg_extract_policy(self._c, None, None, None, 0, C.byref(cost))
        if n < 0:
            self._chk(int(n))
        oid, par, leaf = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint8)
        self._l.porrt_bg_extract_policy(self._c, oid.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p), leaf.ctypes.data_as(C.c_void_p), n, C.byref(cost))
        return (oid, par, leaf), cost.value

    def extract_policies_raw(self, starts):
        """porrt_bg_extract_policies as arrays: pol_off [n + 1], status [n], expected costs [n], original ids, parents, leaf flags"""
        st = np.ascontiguousarray(starts, dtype=np.uint64).reshape(-1)
        n = len(st)
        off, status, cost = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
        stp = st if n else np.zeros(1, dtype=np.uint64)
        total = self._chk(int(self._l.porrt_bg_extract_policies(self._c, stp, n, off, status, cost, None, None, None, 0)))
        self._n_pol = dict(getattr(self, "_n_pol", {}), bg=n)        # what refine_policies sizes its answer by
        oid, par, leaf = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8)
        if total:
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            self._chk(int(self._l.porrt_bg_get_policies(self._c, p(oid), p(par), p(leaf), total)))
        return off, status[:n], cost[:n], oid, par, leaf

    def extract_policies(self, starts):
        """extract_policy (belief_graph.rs:184-267) from every belief node of starts in one device call: a list with
        ((original belief node ids, parents (-1 = root), leaf flags), expected cost) per query -- None where the query has no policy --
        and the status array (0 OK, 1 no finite cost, 2 the walk returns onto its own path, 3 an assertion of the reference fails,
        4 more than option policy_max_nodes nodes)"""
        off, status, cost, oid, par, leaf = self.extract_policies_raw(starts)
        return _policy_list(off, status, cost, oid, par, leaf), status

    def mm_extract_policies(self, starts):
        """the same on the multi-modal belief graph: ((belief node ids, parents, leaf flags, states [k, 2]), expected cost) or None per
        query, and the status array"""
        st = np.ascontiguousarray(starts, dtype=np.uint64).reshape(-1)
        n = len(st)
        off, status, cost = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
        stp = st if n else np.zeros(1, dtype=np.uint64)
        total = self._chk(int(self._l.porrt_mm_extract_policies(self._c, stp, n, off, status, cost, None, None, None, None, 0)))
        self._n_pol = dict(getattr(self, "_n_pol", {}), mm=n)
        oid, par, leaf, xy = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8), np.zeros((total, 2))
        if total:
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            self._chk(int(self._l.porrt_mm_get_policies(self._c, p(oid), p(par), p(leaf), p(xy), total)))
        return _policy_list(off, status[:n], cost[:n], oid, par, leaf, xy), status[:n]

    def policies_info(self):
        """porrt_policies_info of the last extract_policies / mm_extract_policies: queries, ok, nodes, max_nodes, ms_device, ms_wall"""
        i = PoliciesInfo()
        self._chk(self._l.porrt_policies_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in PoliciesInfo._fields_}

    # ---- policy refinement (PTOPolicyRefiner::refine_solution(PartialShortCut(n)), pto_policy_refiner.rs:87-124)
    def _refined(self, call):
        cost = C.c_double(0.0)
        n = call(None, None, None, None, 0, None)
        if n < 0:
            self._chk(int(n))
        xy, oid, par, leaf = np.zeros((n, 2)), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint8)
        self._chk(int(call(xy.ctypes.data_as(C.c_void_p), oid.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p),
                           leaf.ctypes.data_as(C.c_void_p), n, C.byref(cost))))
        return (xy, oid, par, leaf), cost.value

    def refine_policy(self, n_iterations):
        """the policy of the last extract_policy, partially shortcut n_iterations times per piece:
        (states [n, 2], original belief node ids, parents (-1 = root or a piece left unconnected), leaf flags), expected cost"""
        return self._refined(lambda xy, oid, par, leaf, cap, cost: self._l.porrt_bg_refine_policy(self._c, int(n_iterations), xy, oid, par, leaf, cap, cost))

    def refine_policy_explicit(self, xy, parents, original_ids, belief_row, beliefs, n_iterations):
        """the same on a policy given as arrays (children in ascending id order), checked on this context's raster"""
        xy = _f64(xy).reshape(-1, 2)
        par = np.ascontiguousarray(parents, dtype=np.int64)
        oid = np.ascontiguousarray(original_ids, dtype=np.uint64)
        row = np.ascontiguousarray(belief_row, dtype=np.uint32)
        bel = _f64(beliefs).reshape(len(beliefs), -1)
        return self._refined(lambda oxy, ooid, opar, oleaf, cap, cost: self._l.porrt_refine_policy(
            self._c, len(par), xy, par, oid, row, bel, bel.shape[0], bel.shape[1], int(n_iterations), oxy, ooid, opar, oleaf, cap, cost))

    def _refined_many_raw(self, n, cap, call):
        """one batch call with room for cap nodes (never fewer than come back): ref_off [n + 1], status [n], expected costs [n],
        states [total, 2], original ids, parents, leaf flags"""
        off, status, cost = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
        cap = max(int(cap), 1)
        xy, oid, par, leaf = np.zeros((cap, 2)), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        total = self._chk(int(call(off, status, cost, p(xy), p(oid), p(par), p(leaf), cap)))
        assert total <= cap
        return off, status[:n], cost[:n], xy[:total], oid[:total], par[:total], leaf[:total]

    def _refined_many(self, n, cap, call):
        """the same as a list: ((states, original ids, parents, leaf flags), cost) per policy -- None where its status is not 0 --
        and the status array"""
        off, status, cost, xy, oid, par, leaf = self._refined_many_raw(n, cap, call)
        out = []
        for q in range(n):
            a, b = int(off[q]), int(off[q + 1])
            out.append(None if status[q] else ((xy[a:b], oid[a:b], par[a:b], leaf[a:b]), float(cost[q])))
        return out, status

    def refine_policies_raw(self, n_iterations):
        """porrt_bg_refine_policies as arrays: ref_off [n + 1], status [n], expected costs [n], states, original ids, parents, leaf flags"""
        n = max(int(self._l.porrt_bg_get_policies(self._c, None, None, None, 0)), 0)
        return self._refined_many_raw(self._n_policies("bg"), n, lambda off, st, cost, xy, oid, par, leaf, cap: self._l.porrt_bg_refine_policies(
            self._c, int(n_iterations), off, st, cost, xy, oid, par, leaf, cap))

    def refine_policies(self, n_iterations):
        """every policy of the last extract_policies, refined as refine_policy refines one, in one device call
        (porrt_bg_refine_policies): a list with ((states [k, 2], original belief node ids, parents, leaf flags), expected cost) per
        policy -- None where there is none -- and the status array (0 refined, 1 no policy to refine, 2 a shortcut met a raster
        fault, 3 a piece whose nodes carry different beliefs)"""
        n = int(self._l.porrt_bg_get_policies(self._c, None, None, None, 0))         # the nodes going in bound the nodes coming out
        if n < 0:                                                                    # none, or stale: the call says which
            n = 0
        return self._refined_many(self._n_policies("bg"), n, lambda off, st, cost, xy, oid, par, leaf, cap: self._l.porrt_bg_refine_policies(
            self._c, int(n_iterations), off, st, cost, xy, oid, par, leaf, cap))

    def mm_refine_policies(self, n_iterations):
        """the same for the policies of the last mm_extract_policies (porrt_mm_refine_policies)"""
        n = int(self._l.porrt_mm_get_policies(self._c, None, None, None, None, 0))
        if n < 0:
            n = 0
        return self._refined_many(self._n_policies("mm"), n, lambda off, st, cost, xy, oid, par, leaf, cap: self._l.porrt_mm_refine_policies(
            self._c, int(n_iterations), off, st, cost, xy, oid, par, leaf, cap))

    def _n_policies(self, which):
        """queries of the last extract_policies ("bg") / mm_extract_policies ("mm") of this engine; 0 before the first"""
        return getattr(self, "_n_pol", {}).get(which, 0)

    def refine_policies_explicit(self, policies, beliefs, n_iterations):
        """the same on policies given as arrays, checked on this context's raster (porrt_refine_policies): policies is a list of
        (xy [k, 2], parents (within the policy, -1 for its row 0), original ids, belief rows); an empty policy has status 1"""
        bel = _f64(beliefs).reshape(len(beliefs), -1)
        n = len(policies)
        off = np.zeros(n + 1, dtype=np.uint64)
        for q, pol in enumerate(policies):
            off[q + 1] = off[q] + np.uint64(len(pol[1]))
        total = int(off[n])
        cat = lambda i, dt, tail=(): (np.ascontiguousarray(np.concatenate([np.asarray(pol[i], dtype=dt).reshape((-1,) + tail) for pol in policies]))
                                      if total else np.zeros((1,) + tail, dtype=dt))
        xy, par, oid, row = cat(0, np.float64, (2,)), cat(1, np.int64), cat(2, np.uint64), cat(3, np.uint32)
        return self._refined_many(n, total, lambda roff, st, cost, oxy, ooid, opar, oleaf, cap: self._l.porrt_refine_policies(
            self._c, n, off, xy, par, oid, row, bel, bel.shape[0], bel.shape[1], int(n_iterations), roff, st, cost, oxy, ooid, opar, oleaf, cap))

    def refine_policies_info(self):
        """porrt_refine_policies_info of the last batch refinement: policies, ok, pieces, shortcut_pieces, nodes, distinct_lengths,
        ms_device (the shortcut launch), ms_wall"""
        i = RefinePoliciesInfo()
        self._chk(self._l.porrt_refine_policies_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in RefinePoliciesInfo._fields_}

    # ---- PTO::plan_belief_space for many grown engines in one device call (porrt_plan_belief_space_batch)
    @staticmethod
    def plan_belief_space_batch_raw(engines, start_belief, refine_iterations=0):
        """porrt_plan_belief_space_batch as arrays: pol_off [n + 1], status [n], expected costs [n], refine status [n], refined costs [n],
        states [total, 2], original ids (the member's own belief node ids), parents, leaf flags.  The call sizes (cap 0), the nodes come
        from porrt_plan_batch_get_policies."""
        engines = list(engines)
        n = len(engines)
        lead = engines[0]
        arr = (C.c_void_p * n)(*[e._c for e in engines])
        b = np.ascontiguousarray(start_belief, dtype=np.float64)
        off, status, cost = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros(n)
        rstatus, rcost = np.zeros(n, dtype=np.uint8), np.zeros(n)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        total = lead._chk(int(lead._l.porrt_plan_belief_space_batch(arr, n, p(b), len(b), int(refine_iterations), p(off), p(status), p(cost), p(rstatus),
                                                                    p(rcost), None, None, None, None, 0)))
        B = lead.plan_batch_info()["beliefs"]
        lead._plan_batch_sizes = [e.num_nodes() * B for e in engines]        # what plan_batch_expected_costs sizes its answer by
        xy, oid, par, leaf = np.zeros((total, 2)), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8)
        if total:
            lead._chk(int(lead._l.porrt_plan_batch_get_policies(lead._c, None, p(xy), p(oid), p(par), p(leaf), total)))
        return off, status, cost, rstatus, rcost, xy, oid, par, leaf

    @staticmethod
    def plan_belief_space_batch(engines, start_belief, refine_iterations=0):
        """PTO::plan_belief_space (pto.rs:152-182) for every engine of the list (grown in MODE_PTO on one map) in one device call: per
        member (status, expected cost of the root, refine status, refined cost, policy) with policy = (states [k, 2], the member's own
        belief node ids, parents, leaf flags) -- the refined policy when refine_iterations > 0, the extracted one otherwise -- or None
        where the member has none.  The answers live on engines[0] (plan_batch_info, plan_batch_expected_costs)."""
        off, status, cost, rstatus, rcost, xy, oid, par, leaf = Engine.plan_belief_space_batch_raw(engines, start_belief, refine_iterations)
        out = []
        for q in range(len(status)):
            a, b = int(off[q]), int(off[q + 1])
            gone = status[q] != 0 or (refine_iterations > 0 and rstatus[q] != 0)
            out.append((int(status[q]), float(cost[q]), int(rstatus[q]), float(rcost[q]), None if gone else (xy[a:b], oid[a:b], par[a:b], leaf[a:b])))
        return out

    def plan_batch_info(self):
        """porrt_plan_batch_info of the last plan_belief_space_batch this engine led: counts and milliseconds per stage"""
        i = PlanBatchInfo()
        self._chk(self._l.porrt_plan_batch_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in PlanBatchInfo._fields_}

    def plan_batch_expected_costs(self, member):
        """the expected costs of one member of the last pass of the last plan_belief_space_batch this engine led (the member's
        nodes x beliefs values, as expected_costs gives them for the engine alone), copied from the device"""
        sizes = getattr(self, "_plan_batch_sizes", [])
        if not 0 <= int(member) < len(sizes):
            raise PorrtError(-1, "plan_batch_expected_costs: no member %d in the last plan_belief_space_batch of this engine" % member)
        d = np.zeros(int(sizes[int(member)]))
        self._chk(self._l.porrt_plan_batch_get_expected_costs(self._c, int(member), d.ctypes.data_as(C.c_void_p)))
        return d

    # ---- the Reparent strategy (PTOPolicyRefiner::refine_solution(Reparent(radius)), pto_policy_refiner.rs:209-322)
    def reparent_policies_raw(self, radius):
        """porrt_bg_reparent_policies as arrays: ref_off [n + 1], status [n], expected costs [n], states, original ids, parents, leaf
        flags.  The call computes and keeps its answers; the node arrays come from porrt_bg_get_reparented_policies."""
        n = self._n_policies("bg")
        off, status, cost = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
        total = self._chk(int(self._l.porrt_bg_reparent_policies(self._c, float(radius), off, status, cost, None, None, None, None, 0)))
        xy, oid, par, leaf = np.zeros((total, 2)), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8)
        if total:
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            self._chk(int(self._l.porrt_bg_get_reparented_policies(self._c, None, None, None, p(xy), p(oid), p(par), p(leaf), total)))
        return off, status[:n], cost[:n], xy, oid, par, leaf

    @staticmethod
    def _reparented_list(off, status, cost, xy, oid, par, leaf):
        out = []
        for q in range(len(status)):
            a, b = int(off[q]), int(off[q + 1])
            out.append(None if status[q] else ((xy[a:b], oid[a:b], par[a:b], leaf[a:b]), float(cost[q])))
        return out, status

    def reparent_policies(self, radius):
        """every policy of the last extract_policies, refined with the Reparent strategy in one device call: a list with
        ((states [k, 2], belief node ids, parents, leaf flags), expected cost) per policy -- None where there is none -- and the status
        array (0 refined, 1 nothing to refine, 2 raster fault, 3 a piece with different beliefs, 4 a tree or a work area beyond
        option reparent_max_tree_nodes, 5 the pop cap).  Ties between equal priorities pop the lowest tree node id (ours)."""
        return self._reparented_list(*self.reparent_policies_raw(radius))

    def reparent_policy(self, radius):
        """the policy of the last extract_policy, refined with the Reparent strategy: (states, belief node ids, parents, leaf flags),
        expected cost"""
        return self._refined(lambda xy, oid, par, leaf, cap, cost: self._l.porrt_bg_reparent_policy(self._c, float(radius), xy, oid, par, leaf, cap, cost))

    def reparent_policies_explicit(self, xy, belief_row, beliefs, child_off, child_ids, policies, radius):
        """the same on a belief graph given as arrays (node g: state xy[g], belief vector beliefs[belief_row[g]], children
        child_ids[child_off[g]:child_off[g + 1]]) and policies given as a list of (belief-graph node ids, parents within the policy),
        checked on this context's raster (porrt_reparent_policies)"""
        xy = _f64(xy).reshape(-1, 2)
        row = np.ascontiguousarray(belief_row, dtype=np.uint32)
        bel = _f64(beliefs).reshape(len(beliefs), -1)
        coff = np.ascontiguousarray(child_off, dtype=np.uint64)
        cid = np.ascontiguousarray(child_ids, dtype=np.uint32)
        if len(cid) == 0:
            cid = np.zeros(1, dtype=np.uint32)
        n = len(policies)
        off = np.zeros(n + 1, dtype=np.uint64)
        for q, pol in enumerate(policies):
            off[q + 1] = off[q] + np.uint64(len(pol[0]))
        total = int(off[n])
        cat = lambda i, dt: (np.ascontiguousarray(np.concatenate([np.asarray(pol[i], dtype=dt).reshape(-1) for pol in policies])) if total else np.zeros(1, dtype=dt))
        oid, par = cat(0, np.uint64), cat(1, np.int64)
        cap = 2 * total + 1024
        while True:
            roff, status, cost = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
            oxy, ooid, opar, oleaf = np.zeros((cap, 2)), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.uint8)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            m = self._chk(int(self._l.porrt_reparent_policies(self._c, len(row), xy, row, bel, bel.shape[0], bel.shape[1], coff, cid, n, off, oid, par,
                                                              float(radius), roff, status, cost, p(oxy), p(ooid), p(opar), p(oleaf), cap)))
            if m <= cap:
                break
            cap = m                                                  # (the answers did not fit: once more with room for them)
        return self._reparented_list(roff, status[:n], cost[:n], oxy[:m], ooid[:m], opar[:m], oleaf[:m])

    def reparent_policies_info(self):
        """porrt_reparent_policies_info of the last batched Reparent call: policies, ok, pieces, tree_nodes, max_tree, pairs, pops,
        reparents, nodes, rounds, ms_tube, ms_neighbours, ms_pop, ms_recompose, ms_wall"""
        i = ReparentPoliciesInfo()
        self._chk(self._l.porrt_reparent_policies_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in ReparentPoliciesInfo._fields_}

    def refine_info(self):
        a, b = C.c_double(0), C.c_double(0)
        self._chk(self._l.porrt_bg_get_refine_info(self._c, C.byref(a), C.byref(b)))
        return dict(total_s=a.value, device_s=b.value)

    def dp_info(self):
        a, b, n = C.c_double(0), C.c_double(0), C.c_uint32(0)
        self._chk(self._l.porrt_bg_get_dp_info(self._c, C.byref(a), C.byref(b), C.byref(n)))
        return dict(total_s=a.value, device_s=b.value, sweeps=n.value, sweep_rows=int(self._l.porrt_bg_get_dp_sweep_rows(self._c)))

    def selftest(self, n=1 << 20):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._l.porrt_selftest(self._c, n, C.byref(a), C.byref(b)))
        return a.value, b.value

    def grow_mm_prm(self, start, belief, max_step, search_radius, n_iter_per_belief):
        """MapShelfDomainTampPRM::grow_mm_prm (map_shelves_tamp_prm.rs:328-393); same dict as the oracle's"""
        L = self._l
        b = _f64(belief)
        self._chk(L.porrt_grow_mm_prm(self._c, _f64(start), b, len(b), max_step, search_radius, n_iter_per_belief))
        nw = len(b)
        modes, trs = [], []
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        for m in range(L.porrt_mm_num_modes(self._c)):
            bb, rp = np.zeros(nw), C.c_double(0)
            nn, ne, nf = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            self._chk(L.porrt_mm_get_mode(self._c, m, bb, C.byref(rp), C.byref(nn), C.byref(ne), C.byref(nf)))
            xy = np.zeros((nn.value, 2))
            ef, et, fin = np.zeros(ne.value, dtype=np.uint32), np.zeros(ne.value, dtype=np.uint32), np.zeros(nf.value, dtype=np.uint64)
            self._chk(L.porrt_mm_get_mode_graph(self._c, m, p(xy), p(ef), p(et), p(fin)))
            modes.append(dict(belief=bb, reaching_probability=rp.value, xy=xy, edges=(ef.astype(np.uint64), et.astype(np.uint64)), finals=fin))
        for t in range(L.porrt_mm_num_transitions(self._c)):
            z, f, to, ob, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int(0), C.c_uint64(0)
            self._chk(L.porrt_mm_get_transition(self._c, t, C.byref(z), C.byref(f), C.byref(to), C.byref(ob), C.byref(n)))
            pairs = np.zeros((n.value, 2), dtype=np.uint64)
            self._chk(L.porrt_mm_get_transition_pairs(self._c, t, p(pairs)))
            trs.append(dict(zone=z.value, from_mode=f.value, to_mode=to.value, observation=ob.value, pairs=pairs))
        return dict(n_beliefs=L.porrt_mm_num_beliefs(self._c), modes=modes, transitions=trs)

    def mm_seconds(self):
        h, r, d = C.c_double(0), C.c_double(0), C.c_double(0)
        self._chk(self._l.porrt_mm_get_seconds(self._c, C.byref(h), C.byref(r), C.byref(d)))
        return dict(host_s=h.value, roadmap_s=r.value, device_s=d.value)

    # ---- the rest of MapShelfDomainTampPRM::plan (map_shelves_tamp_prm.rs:310-326) on the modes of the last grow_mm_prm
    def mm_build_belief_graph(self):
        """build_belief_graph (:395-473) on the device"""
        self._chk(self._l.porrt_mm_build_belief_graph(self._c))

    def mm_belief_graph(self):
        """dict(types, belief_ids, children=(off, ids), parents=(off, ids), mode_offsets, finals) of the last mm_build_belief_graph"""
        L = self._l
        N, E, F = L.porrt_mm_bg_num_nodes(self._c), L.porrt_mm_bg_num_edges(self._c), L.porrt_mm_bg_num_finals(self._c)
        M = L.porrt_mm_num_modes(self._c)
        coff, poff = np.zeros(N + 1, dtype=np.uint64), np.zeros(N + 1, dtype=np.uint64)
        cid, pid = np.zeros(max(E, 1), dtype=np.uint32), np.zeros(max(E, 1), dtype=np.uint32)
        types, bid = np.zeros(max(N, 1), dtype=np.uint8), np.zeros(max(N, 1), dtype=np.uint32)
        moff, fin = np.zeros(M + 1, dtype=np.uint64), np.zeros(max(F, 1), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(L.porrt_mm_bg_get_graph(self._c, p(coff), p(cid), p(poff), p(pid), p(types), p(bid), p(moff), p(fin)))
        return dict(types=types[:N], belief_ids=bid[:N], children=(coff, cid[:E]), parents=(poff, pid[:E]), mode_offsets=moff, finals=fin[:F])

    def mm_compute_expected_costs(self):
        self._chk(self._l.porrt_mm_compute_expected_costs(self._c))

    def mm_expected_costs(self, compute=True):
        """compute_expected_costs_to_goals (:475-477) on the device (unless compute=False: the last ones); dist per belief node"""
        if compute:
            self.mm_compute_expected_costs()
        d = np.zeros(self._l.porrt_mm_bg_num_nodes(self._c))
        self._chk(self._l.porrt_mm_get_expected_costs(self._c, d))
        return d

    def mm_extract_policy(self):
        """extract_policy (:479-485): (belief node ids, parents (-1 = root), leaf flags, states [n, 2]), expected cost of the root"""
        cost = C.c_double(0.0)
        n = self._l.porrt_mm_extract_policy(self._c, None, None, None, None, 0, C.byref(cost))
        if n < 0:
            self._chk(int(n))
        oid, par, leaf, xy = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint8), np.zeros((n, 2))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(int(self._l.porrt_mm_extract_policy(self._c, p(oid), p(par), p(leaf), p(xy), n, C.byref(cost))))
        return (oid, par, leaf, xy), cost.value

    def mm_refine_policy(self, n_iterations):
        """PartialShortCut(n_iterations) of the last mm_extract_policy: (states, belief node ids, parents, leaf flags), expected cost"""
        return self._refined(lambda xy, oid, par, leaf, cap, cost: self._l.porrt_mm_refine_policy(self._c, int(n_iterations), xy, oid, par, leaf, cap, cost))

    def plan_mm_prm(self, start, belief, max_step, search_radius, n_iter_per_belief, refine_iterations=0):
        """MapShelfDomainTampPRM::plan (:310-326), then PartialShortCut(refine_iterations) when > 0 (main.rs:546-575):
        ((belief node ids, parents, leaf flags, states), expected cost)"""
        b = _f64(belief)
        self._chk(int(self._l.porrt_mm_plan(self._c, _f64(start), b, len(b), max_step, search_radius, n_iter_per_belief)))
        if refine_iterations > 0:
            (xy, oid, par, leaf), cost = self.mm_refine_policy(refine_iterations)
            return (oid, par, leaf, xy), cost
        return self.mm_extract_policy()

    # ---- MapShelfDomainTampPRM::plan + PartialShortCut for many problems on this engine's map in one device call (porrt_mm_plan_batch)
    def plan_mm_prm_batch_raw(self, starts, priors, max_step, search_radius, n_iter_per_belief, refine_iterations=0, sampler_seeds=None,
                              discrete_seeds=None):
        """porrt_mm_plan_batch as arrays: pol_off [n + 1], status [n], expected costs [n], refine status [n], refined costs [n], and the
        policies' rows (states [total, 2], the plans' own belief node ids, parents, leaf flags) from porrt_mm_plan_batch_get_policies.
        sampler_seeds / discrete_seeds None: every plan clones the engine's current continuous / discrete sampler state."""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 2)
        n = starts.shape[0]
        priors = np.ascontiguousarray(priors, dtype=np.float64).reshape(n, -1) if n else np.zeros((0, 1))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        seeds = [None if v is None else np.ascontiguousarray(v, dtype=np.uint64) for v in (sampler_seeds, discrete_seeds)]
        for v in seeds:
            if v is not None and v.shape != (n,):
                raise PorrtError(-1, "plan_mm_prm_batch: one seed per plan")
        off, status, cost = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
        rstatus, rcost = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1))
        total = self._chk(int(self._l.porrt_mm_plan_batch(self._c, n, p(starts), p(priors), p(seeds[0]), p(seeds[1]), priors.shape[1], float(max_step),
                                                          float(search_radius), int(n_iter_per_belief), int(refine_iterations), p(off), p(status), p(cost),
                                                          p(rstatus), p(rcost), None, None, None, None, 0)))
        xy, oid, par, leaf = np.zeros((total, 2)), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8)
        if total:
            self._chk(int(self._l.porrt_mm_plan_batch_get_policies(self._c, None, p(xy), p(oid), p(par), p(leaf), total)))
        return off, status[:n], cost[:n], rstatus[:n], rcost[:n], xy, oid, par, leaf

    def plan_mm_prm_batch(self, starts, priors, max_step, search_radius, n_iter_per_belief, refine_iterations=0, sampler_seeds=None, discrete_seeds=None):
        """One dict per plan: status, cost (the root's expected cost), refine_status, refined_cost and policy = (belief node ids, parents,
        leaf flags, states), the refined policy when refine_iterations > 0; a plan with nonzero status has an empty policy."""
        off, status, cost, rstatus, rcost, xy, oid, par, leaf = self.plan_mm_prm_batch_raw(starts, priors, max_step, search_radius, n_iter_per_belief,
                                                                                           refine_iterations, sampler_seeds, discrete_seeds)
        out = []
        for q in range(len(status)):
            a, b = int(off[q]), int(off[q + 1])
            out.append(dict(status=int(status[q]), cost=float(cost[q]), refine_status=int(rstatus[q]), refined_cost=float(rcost[q]),
                            policy=(oid[a:b], par[a:b], leaf[a:b], xy[a:b])))
        return out

    def mm_plan_batch_info(self):
        """porrt_mm_plan_batch_info of the last plan_mm_prm_batch: counts summed over the passes and milliseconds per stage"""
        i = MmPlanBatchInfo()
        self._chk(self._l.porrt_mm_plan_batch_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in MmPlanBatchInfo._fields_}

    def mm_plan_batch_plan(self, plan):
        """porrt_mm_plan_batch_get_plan: modes, transitions, beliefs, nodes, forward_edges, belief_edges, finals and pass of one plan"""
        i = MmBatchPlan()
        self._chk(self._l.porrt_mm_plan_batch_get_plan(self._c, int(plan), C.byref(i)))
        return {k.rstrip("_"): getattr(i, k) for k, _ in MmBatchPlan._fields_}

    def mm_plan_batch_expected_costs(self, plan):
        """the expected costs of one plan of the last pass of the last plan_mm_prm_batch (what mm_expected_costs gives for the plan alone)"""
        d = np.zeros(self.mm_plan_batch_plan(plan)["nodes"])
        self._chk(self._l.porrt_mm_plan_batch_get_expected_costs(self._c, int(plan), d.ctypes.data_as(C.c_void_p)))
        return d

    def mm_plan_seconds(self):
        v = np.zeros(8)
        self._chk(self._l.porrt_mm_get_plan_seconds(self._c, v, 8))
        keys = ("grow_s", "build_s", "build_device_s", "costs_s", "costs_device_s", "extract_s", "refine_s", "refine_device_s")
        return dict(zip(keys, v.tolist()))

    def mm_dp_info(self):
        lv, la, sw, ls = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_int(0)
        self._chk(self._l.porrt_mm_get_dp_info(self._c, C.byref(lv), C.byref(la), C.byref(sw), C.byref(ls)))
        return dict(levels=lv.value, launches=la.value, sweeps=sw.value, level_schedule=bool(ls.value))

    def save_graph_json(self, path):
        """the PTO graph / PRM roadmap of the last grow as the reference's PTOGraph JSON (pto_graph.rs:22-118)"""
        self._chk(self._l.porrt_graph_save_json(self._c, os.fsencode(path)))

    def metrics(self):
        m = Metrics()
        self._chk(self._l.porrt_get_metrics(self._c, C.byref(m)))
        return {k: getattr(m, k) for k, _ in Metrics._fields_}


def _rgb(c):
    return np.ascontiguousarray(np.asarray(c, dtype=np.uint8).reshape(3))


class Canvas:
    """One porrt_canvas: the drawing half of MapShelfDomain / Map (map_shelves_io.rs:276-457) on the device.  Every method forwards to one
    exported symbol; the image is bit for bit the reference's sequential loop's."""

    def __init__(self, engine, factor=1):
        self._l = engine._l
        self._c = self._l.porrt_canvas_create(engine._c, int(factor))
        if not self._c:
            raise PorrtError(engine.get_option("draw_create_status"), self._l.porrt_last_error(engine._c).decode())

    def close(self):
        if getattr(self, "_c", None):
            self._l.porrt_canvas_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise PorrtError(rc, self._l.porrt_canvas_last_error(self._c).decode())
        return rc

    def size(self):
        """(W, H)"""
        w, h = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._l.porrt_canvas_size(self._c, C.byref(w), C.byref(h)))
        return w.value, h.value

    def draw_lines(self, ab, color, alpha=1.0):
        """draw_line(a, b, color, alpha) for every row (ax, ay, bx, by) of ab, in row order"""
        ab = _f64(ab).reshape(-1, 4)
        self._chk(self._l.porrt_canvas_draw_lines(self._c, ab, ab.shape[0], _rgb(color), float(alpha)))

    def draw_path(self, xy, color):
        xy = _f64(xy).reshape(-1, 2)
        self._chk(self._l.porrt_canvas_draw_path(self._c, xy, xy.shape[0], _rgb(color)))

    def draw_circles(self, xy, radius, color):
        xy = _f64(xy).reshape(-1, 2)
        self._chk(self._l.porrt_canvas_draw_circles(self._c, xy, xy.shape[0], float(radius), _rgb(color)))

    def draw_tree(self, engine):
        self._chk(self._l.porrt_canvas_draw_tree(self._c, engine._c))

    def draw_full_graph(self, engine):
        self._chk(self._l.porrt_canvas_draw_full_graph(self._c, engine._c))

    def draw_zones_observability(self):
        self._chk(self._l.porrt_canvas_draw_zones_observability(self._c))

    def draw_policy(self, xy, parent):
        xy = _f64(xy).reshape(-1, 2)
        parent = np.ascontiguousarray(parent, dtype=np.int64)
        self._chk(self._l.porrt_canvas_draw_policy(self._c, xy, parent, xy.shape[0]))

    def rgb(self):
        w, h = self.size()
        out = np.zeros((h, w, 3), dtype=np.uint8)
        self._chk(self._l.porrt_canvas_get_rgb(self._c, out))
        return out

    def save_png(self, path):
        self._chk(self._l.porrt_canvas_save_png(self._c, os.fsencode(path)))

    def info(self):
        """the last draw call: lines, fragments, passes, heaviest_pixel, heavy_pixels, wave_pixels, gradient_by_f64 and seconds per stage"""
        i = DrawInfo()
        self._chk(self._l.porrt_canvas_get_info(self._c, C.byref(i)))
        return {k: getattr(i, k) for k, _ in DrawInfo._fields_}


def write_png(path, rgb):
    """porrt_write_png: an H x W x 3 uint8 array as an 8-bit RGB PNG (host code, no device)"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, _ = rgb.shape
    rc = load_library().porrt_write_png(os.fsencode(path), rgb.reshape(-1), w, h)
    if rc < 0:
        raise PorrtError(rc, "porrt_write_png(%s)" % path)


def conditional_dijkstra(xy, belief_row, beliefs, types, children, parents, finals, device=0):
    """porrt_conditional_dijkstra: conditional_dijkstra (belief_graph.rs:89-175) of an explicit graph on the GPU;
    children / parents are lists of lists in add_edge order"""
    L = load_library()
    n = len(types)

    def csr(lists):
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in lists])
        return off, np.array([v for x in lists for v in x] + [0], dtype=np.uint32)
    coff, cid = csr(children)
    poff, pid = csr(parents)
    beliefs = np.ascontiguousarray(beliefs, dtype=np.float64)
    dist = np.zeros(n)
    rc = L.porrt_conditional_dijkstra(device, n, np.ascontiguousarray(xy, dtype=np.float64), np.ascontiguousarray(belief_row, dtype=np.uint32),
                                      beliefs, beliefs.shape[0], beliefs.shape[1], np.ascontiguousarray(types, dtype=np.uint8), coff, cid, poff, pid,
                                      np.ascontiguousarray(finals, dtype=np.uint64), len(finals), dist)
    if rc < 0:
        raise RuntimeError("porrt_conditional_dijkstra failed (%d)" % rc)
    return dist


def extract_policies_explicit(xy, belief_row, beliefs, belief_ids, children, dist, starts, policy_max_nodes=0, device=0):
    """porrt_extract_policies: extract_policy (belief_graph.rs:184-267) from every node of starts on an explicit graph, on the GPU.
    children: per-node lists in add_edge order (or a CSR pair (off, ids)); belief_row[i] = row of `beliefs` node i carries, belief_ids[i]
    its clustering key, dist[i] its expected cost.  Returns (list of ((oid, par, leaf), cost) or None per query, status array)."""
    L = load_library()
    n = len(dist)
    if isinstance(children, tuple):
        coff, cid = np.ascontiguousarray(children[0], dtype=np.uint64), np.ascontiguousarray(np.append(children[1], 0), dtype=np.uint32)
    else:
        coff = np.zeros(n + 1, dtype=np.uint64)
        coff[1:] = np.cumsum([len(x) for x in children])
        cid = np.array([v for x in children for v in x] + [0], dtype=np.uint32)
    beliefs = np.ascontiguousarray(beliefs, dtype=np.float64)
    st = np.ascontiguousarray(starts, dtype=np.uint64).reshape(-1)
    nq = len(st)
    off, status, cost = np.zeros(nq + 1, dtype=np.uint64), np.zeros(max(nq, 1), dtype=np.uint8), np.zeros(max(nq, 1))
    args = (device, n, np.ascontiguousarray(xy, dtype=np.float64).reshape(-1), np.ascontiguousarray(belief_row, dtype=np.uint32), beliefs,
            beliefs.shape[0], beliefs.shape[1], np.ascontiguousarray(belief_ids, dtype=np.uint32), coff, cid,
            np.ascontiguousarray(dist, dtype=np.float64), st if nq else np.zeros(1, dtype=np.uint64), nq, int(policy_max_nodes), off, status, cost)
    total = int(L.porrt_extract_policies(*args, None, None, None, 0))
    if total < 0:
        raise RuntimeError("porrt_extract_policies failed (%d)" % total)
    oid, par, leaf = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8)
    if total:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = int(L.porrt_extract_policies(*args, p(oid), p(par), p(leaf), total))
        if rc != total:
            raise RuntimeError("porrt_extract_policies failed (%d)" % rc)
    return _policy_list(off, status[:nq], cost[:nq], oid, par, leaf), status[:nq]


def qmdp_costs_explicit(xy, node_validity, validities, children, finals, device=0):
    """porrt_qmdp_costs: plan_qmdp's costs (one dijkstra per world over PTOGraphWorldView, pto_graph.rs:245-303) of an explicit graph
    on the GPU.  validities: one word of world bits per validity id; children: per-node lists in push order; finals: per-world lists
    of final node ids (an empty list: that world's costs are all +inf).  Returns an (n_worlds, n) array."""
    L = load_library()
    n, nw = len(children), len(finals)

    def csr(lists, dt):
        off = np.zeros(len(lists) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c) for c in lists])
        ids = np.array([i for c in lists for i in c], dtype=dt)
        return off, (ids if len(ids) else np.zeros(1, dtype=dt))

    co, ci = csr(children, np.uint32)
    fo, fi = csr(finals, np.uint64)
    val = np.ascontiguousarray(validities, dtype=np.uint64)
    out = np.zeros((nw, n))
    rc = L.porrt_qmdp_costs(device, n, _f64(xy).reshape(-1), np.ascontiguousarray(node_validity, dtype=np.uint32), val, len(val), nw,
                            co, ci, fo, fi, out.reshape(-1))
    if rc != 0:
        raise RuntimeError("porrt_qmdp_costs failed (%d)" % rc)
    return out


def policy_graph_explicit(children, costs, device=0):
    """porrt_policy_graph: get_policy_graph's decision (pto_graph.rs:363-419) for every adjacency entry of an explicit graph on the
    GPU.  children: per-node lists in push order; costs[w][id] (+inf allowed).  Returns (keep, how, info): one entry per adjacency
    entry in push order, and the counts and times as a dict."""
    L = load_library()
    n = len(children)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in children])
    ids = np.array([i for c in children for i in c], dtype=np.uint32)
    cost = _f64(costs)
    if cost.ndim != 2 or cost.shape[1] != n:
        raise ValueError("policy_graph_explicit: costs[w][id], one row per world")
    keep, how = np.zeros(max(len(ids), 1), dtype=np.uint8), np.zeros(max(len(ids), 1), dtype=np.uint8)
    info = PolicyGraphInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.porrt_policy_graph(device, n, cost.shape[0], off, ids if len(ids) else np.zeros(1, dtype=np.uint32), p(cost), p(keep), p(how),
                              C.byref(info))
    if rc != 0:
        raise RuntimeError("porrt_policy_graph failed (%d)" % rc)
    return keep[:len(ids)].astype(bool), how[:len(ids)], info.as_dict()


def exchange_decide(entries):
    """porrt_exchange_decide: entries[rank, map] (BEST_ENTRY) -> winning rank per map (-1 = nobody solved it); host code only"""
    L = load_library()
    e = np.ascontiguousarray(entries, dtype=BEST_ENTRY)
    world, n_maps = e.shape
    win = np.zeros(n_maps, dtype=np.int32)
    rc = L.porrt_exchange_decide(e.ctypes.data_as(C.c_void_p), world, n_maps, win.ctypes.data_as(C.c_void_p))
    if rc:
        raise PorrtError(rc, "porrt_exchange_decide")
    return win


def exchange_agree(words, my_rank):
    """porrt_exchange_agree: words[rank] = (status code, n_maps) -> (what rank my_rank must return, first failing rank or -1); host code only"""
    L = load_library()
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, 2)
    bad = C.c_int32(-1)
    rc = L.porrt_exchange_agree(w.ctypes.data_as(C.c_void_p), len(w), my_rank, C.byref(bad))
    return rc, bad.value


class Comm:
    """The one exchange of a query-sharded job (porrt_comm_*, porrt_exchange_*): RCCL over xGMI, device to device."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        rc = load_library().porrt_comm_unique_id(buf)
        if rc:
            raise PorrtError(rc, "porrt_comm_unique_id (RCCL)")
        return bytes(buf)

    def __init__(self, device, rank, world, unique_id):
        self._l = load_library()
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._c = self._l.porrt_comm_create(device, rank, world, buf)
        if not self._c:
            raise PorrtError(-4, "porrt_comm_create failed (device %d, rank %d of %d)" % (device, rank, world))
        self.rank, self.world = rank, world

    def close(self):
        if getattr(self, "_c", None):
            self._l.porrt_comm_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def usable(self):
        """False once a collective step failed on this rank (the communicator was aborted: make a new one)"""
        return bool(self._c) and bool(self._l.porrt_comm_usable(self._c))

    def set_timeout_ms(self, ms):
        rc = self._l.porrt_comm_set_timeout_ms(self._c, int(ms))
        if rc:
            raise PorrtError(rc, "porrt_comm_set_timeout_ms")

    def exchange_best(self, engines, map_ids, n_maps):
        """collective: winners[m] (BEST_ENTRY) identical on every rank; the winning trees stay on the device (tree(m))"""
        n = len(engines)
        arr = (C.c_void_p * max(n, 1))(*[e._c for e in engines])
        ids = np.ascontiguousarray(map_ids, dtype=np.uint32)
        win = np.zeros(n_maps, dtype=BEST_ENTRY)
        rc = self._l.porrt_exchange_best(self._c, arr, n, ids, n_maps, win.ctypes.data_as(C.c_void_p))
        if rc:
            raise PorrtError(rc, self._l.porrt_comm_last_error(self._c).decode())
        return win

    def tree(self, m):
        n = self._l.porrt_exchange_num_nodes(self._c, m)
        xy, parent, dist = np.zeros((n, 2)), np.zeros(n, dtype=np.int64), np.zeros(n)
        rc = self._l.porrt_exchange_get_tree(self._c, m, xy, parent, dist)
        if rc:
            raise PorrtError(rc, self._l.porrt_comm_last_error(self._c).decode())
        return xy, parent, dist


# ---- on-disk formats (host code of the library: no GPU needed)
def read_pgm(path=None, data=None):
    """porrt_read_pgm / porrt_read_pgm_mem: the gray raster the reference's domains open (uint8 [H, W])"""
    L = load_library()
    W, H = C.c_uint32(0), C.c_uint32(0)
    if data is not None:
        call = lambda out: L.porrt_read_pgm_mem(data, len(data), out, C.byref(W), C.byref(H))
    else:
        call = lambda out: L.porrt_read_pgm(os.fsencode(path), out, C.byref(W), C.byref(H))
    rc = call(None)
    if rc:
        raise PorrtError(rc, "porrt_read_pgm: %s" % ("cannot open the file" if rc == -7 else "not an 8-bit gray PNM (the reference: \"Wrong image format!\")"))
    out = np.zeros((H.value, W.value), dtype=np.uint8)
    rc = call(out.ctypes.data_as(C.c_void_p))
    if rc:
        raise PorrtError(rc, "porrt_read_pgm")
    return out


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def graph_write_json(path, xy, node_validity, children, parents, validities):
    """porrt_graph_write_json; children / parents = (offsets, ids, validity ids); validities = bool [n_validities, n_worlds]"""
    L = load_library()
    xy = _f64(xy).reshape(-1, 2)
    v = np.ascontiguousarray(np.asarray(validities, dtype=np.uint8).reshape(len(validities), -1))
    (co, ci, cv), (po, pi, pv) = children, parents
    rc = L.porrt_graph_write_json(os.fsencode(path), len(xy), xy, _u64(node_validity), _u64(co), _u64(ci), _u64(cv), _u64(po), _u64(pi), _u64(pv),
                                  v.shape[0], v.shape[1] if v.size else 0, v)
    if rc:
        raise PorrtError(rc, "porrt_graph_write_json")


def graph_load_json(path):
    """porrt_graph_load_json: dict(xy, node_validity, children=(off, ids, validity), parents=(...), validities bool [n, n_worlds])"""
    L = load_library()
    err = C.create_string_buffer(256)
    g = L.porrt_graph_load_json(os.fsencode(path), err, 256)
    if not g:
        raise PorrtError(-1, "porrt_graph_load_json: " + err.value.decode())
    try:
        n, nc, npar = L.porrt_graph_file_num_nodes(g), L.porrt_graph_file_num_children(g), L.porrt_graph_file_num_parents(g)
        nv, nw = L.porrt_graph_file_num_validities(g), L.porrt_graph_file_num_worlds(g)
        xy, val = np.zeros((n, 2)), np.zeros(n, dtype=np.uint64)
        co, ci, cv = np.zeros(n + 1, dtype=np.uint64), np.zeros(nc, dtype=np.uint64), np.zeros(nc, dtype=np.uint64)
        po, pi, pv = np.zeros(n + 1, dtype=np.uint64), np.zeros(npar, dtype=np.uint64), np.zeros(npar, dtype=np.uint64)
        vb = np.zeros((nv, nw), dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = L.porrt_graph_file_get(g, p(xy), p(val), p(co), p(ci), p(cv), p(po), p(pi), p(pv), p(vb))
        if rc:
            raise PorrtError(rc, "porrt_graph_file_get")
    finally:
        L.porrt_graph_file_free(g)
    return dict(xy=xy, node_validity=val, children=(co, ci, cv), parents=(po, pi, pv), validities=vb.astype(bool))
