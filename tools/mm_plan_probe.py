"""Times the multi-modal PRM planner after the growth (porrt_mm_*; map_shelves_tamp_prm.rs:310-326) and writes
profiles/<tag>mm_plan.json (PORRT_OUT or out/ with --out).

1. The config.mm_prm workload of bench.py --full (12 shelves, uniform prior, 100 samples per belief, max_step 0.1, radius 2): the
   belief-graph build and the expected costs, level schedule against the general sweeps (bits compared), levels and launches, and
   the C restatement's conditional_dijkstra (oracle) on the same graph.  Its root is +inf on the stand-in raster: no walk.
2. The reference driver's shape (main.rs:546-575): plan with 5000 samples per belief, then PartialShortCut(1500), for 2 goals
   (committed zones) and 4 / 6 / 8 goals (free-centroid zones), end to end."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--goals", default="2,4,6,8")
    ap.add_argument("--n-iter", type=int, default=5000)
    args = ap.parse_args()
    import cases
    import mm_plan_ref as ref
    import po_rrt_amd
    from oracle import orc
    res = {}
    # 1. the config.mm_prm workload
    case = cases.cfg4(1000, 1000)
    prior = [1.0 / 12] * 12
    e = cases.configure(po_rrt_amd.Engine(0), case)
    e.set_discrete_seed(0)
    g = e.grow_mm_prm(case.start, prior, 0.1, 2.0, 100)
    builds = []
    for _ in range(3):
        e.mm_build_belief_graph()
        builds.append(e.mm_plan_seconds())
    e.set_option("mm_levels", 1)
    d_lv, info_lv, secs_lv = None, None, []
    for _ in range(3):
        d_lv = e.mm_expected_costs()
        info_lv, secs_lv = e.mm_dp_info(), secs_lv + [e.mm_plan_seconds()]
    e.set_option("dp_sweeps", 1)
    secs_sw = []
    for _ in range(3):
        d_sw = e.mm_expected_costs()
        info_sw, secs_sw = e.mm_dp_info(), secs_sw + [e.mm_plan_seconds()]
    e.set_option("dp_sweeps", 0)
    o = cases.configure(orc.Oracle(), case)
    t0 = time.perf_counter()
    bg = ref.build_belief_graph(g, o.reachable_beliefs(prior), o.belief_hash)
    t_restate = time.perf_counter() - t0
    t0 = time.perf_counter()
    d_c = ref.expected_costs(bg)
    t_c = time.perf_counter() - t0
    med = lambda xs, k: float(np.median([x[k] for x in xs]))
    res["config_mm_prm"] = {
        "what": "12 shelves, uniform prior, 100 samples per belief: %d modes, %d belief nodes, %d edges" % (len(g["modes"]), len(d_lv), e._l.porrt_mm_bg_num_edges(e._c)),
        "ms_build": 1e3 * med(builds, "build_s"), "ms_build_device": 1e3 * med(builds, "build_device_s"),
        "ms_costs_levels": 1e3 * med(secs_lv, "costs_s"), "ms_costs_levels_device": 1e3 * med(secs_lv, "costs_device_s"),
        "levels": info_lv["levels"], "launches": info_lv["launches"], "mode_sweeps_summed": info_lv["sweeps"],
        "ms_costs_sweeps": 1e3 * med(secs_sw, "costs_s"), "ms_costs_sweeps_device": 1e3 * med(secs_sw, "costs_device_s"),
        "sweeps_general": info_sw["sweeps"],
        "levels_equal_sweeps_bitwise": bool(np.array_equal(d_lv.view(np.uint64), d_sw.view(np.uint64))),
        "equal_to_c_restatement_bitwise": bool(np.array_equal(d_lv.view(np.uint64), d_c.view(np.uint64))),
        "ms_c_restatement_dijkstra": 1e3 * t_c, "ms_numpy_graph_build": 1e3 * t_restate,
        "root_cost": float(d_lv[0])}
    print(json.dumps(res["config_mm_prm"]), flush=True)
    # 2. the reference driver's shape
    res["driver"] = []
    for n_goals in [int(x) for x in args.goals.split(",") if x]:
        zones = "map_benchmark_like_2_goals_zone_ids" if n_goals == 2 else "map_benchmark_like_%d_free_zone_ids" % n_goals
        c = cases.cfg2(10)
        c.update(zones=zones, visibility=0.5)
        p = cases.configure(po_rrt_amd.Engine(0), c)
        p.set_discrete_seed(0)
        t0 = time.perf_counter()
        try:
            (oid, par, leaf, xy), cost = p.plan_mm_prm(c.start, [1.0 / n_goals] * n_goals, 0.1, 2.0, args.n_iter, refine_iterations=1500)
            err = None
        except RuntimeError as ex:
            oid, cost, err = [], float("inf"), str(ex)
        wall = time.perf_counter() - t0
        lv_sw = {}
        if err is None:                                       # the same costs by level and by the general sweeps
            for name, sw in (("levels", 0), ("sweeps", 1)):
                p.set_option("mm_levels", 1 - sw)
                d = p.mm_expected_costs()
                lv_sw[name] = (d, p.mm_plan_seconds()["costs_device_s"], p.mm_dp_info())
            p.set_option("mm_levels", 0)
            lv_sw = {"ms_costs_levels_device": 1e3 * lv_sw["levels"][1], "ms_costs_sweeps_device": 1e3 * lv_sw["sweeps"][1],
                     "general_sweeps": lv_sw["sweeps"][2]["sweeps"], "mode_sweeps_summed": lv_sw["levels"][2]["sweeps"],
                     "levels_equal_sweeps_bitwise": bool(np.array_equal(lv_sw["levels"][0].view(np.uint64), lv_sw["sweeps"][0].view(np.uint64)))}
        row = dict(goals=n_goals, **lv_sw, zones=zones, n_iter_per_belief=args.n_iter, s_total=wall, expected_cost=cost, policy_nodes=len(oid), error=err,
                   **{k: v for k, v in p.mm_plan_seconds().items()})
        res["driver"].append(row)
        print(json.dumps(row), flush=True)
    res["reference_recorded_s"] = {"2": 0.209, "4": 1.188, "6": 6.12, "8": 33.4}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.tag + "mm_plan.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
