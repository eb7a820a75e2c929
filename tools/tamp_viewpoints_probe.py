"""Times the device gather of all RRT* solutions (porrt_solutions) and the multiple-viewpoints TAMP-RRT search
(porrt_tamp_rrt_plan_viewpoints; map_shelves_tamp_rrt.rs:293-430) and writes profiles/<tag>tamp_viewpoints.json
(or the file --out names).

  1. solutions gather: a 512-row TAMP-shaped batch (cases.tamp_queries) after one porrt_grow_batch; Engine.solutions_batch (size query
     + gather: two calls) and the gather call alone, median of --runs after a warm-up.  Baseline, the only way without the device
     path: porrt_get_trees of the same rows (timed alone: a lower bound of the baseline) plus the host walk (timed as the Python
     restatement tests/solutions_ref.py on the downloaded trees; the C++ walk of include/porrt.hpp is the same loop).
  2. plan wall time in the reference driver's shape (start (0, -1), uniform prior, 0.1 / 2.0 / 2500 / 10000, goal radius 0.05, K 128):
     2 goals with all viewpoints, 4 and 6 goals with max_viewpoints 2, at several wave widths: queries, queries/s, viewpoints, costs.
     The second run on a lead (its pool made) is the one recorded.  A shape is left out at a wave width once a wider wave of the same
     shape took longer than --budget seconds.
  3. the restatement (tests/tamp_viewpoints_ref.py) on the CPU oracle at 2 goals (all) and 4 goals (cap 2): seconds, queries."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

RASTERS = {2: "map_benchmark_like_2_goals_zone_ids", 4: "map_benchmark_like_4_free_zone_ids", 6: "map_benchmark_like_6_free_zone_ids"}
START = (0.0, -1.0)


def setup(eng, zones, seed):
    import cases
    eng.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    eng.set_zones(cases.load_map(zones), 0.5)
    eng.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return eng


def median_ms(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), ts


def gather(po, rows, runs):
    import cases
    import solutions_ref
    qs = cases.tamp_queries(rows)
    es = [cases.configure(po.Engine(0), q) for q in qs]
    po.Engine.grow_batch(es, [q.start for q in qs], qs[0].max_step, qs[0].search_radius, qs[0].n_iter_min, 128, n_iter_max=qs[0].n_iter_max)
    sols = po.Engine.solutions_batch(es)
    n_sol, n_states = sum(len(s) for s in sols), sum(len(p) for s in sols for _, p, _ in s)
    both, _ = median_ms(lambda: po.Engine.solutions_batch(es), runs)
    L = es[0]._l
    arr = (C.c_void_p * rows)(*[e._c for e in es])
    ids, lens, costs, xy = np.zeros(n_sol, dtype=np.uint64), np.zeros(n_sol, dtype=np.uint64), np.zeros(n_sol), np.zeros((n_states, 2))

    def one_call():
        rc = L.porrt_solutions(arr, rows, None, None, ids.ctypes.data, lens.ctypes.data, costs.ctypes.data, n_sol, xy.ctypes.data, n_states)
        assert rc == 0
    one, one_all = median_ms(one_call, runs)
    size, _ = median_ms(lambda: L.porrt_solutions(arr, rows, None, None, None, None, None, 0, None, 0), runs)
    trees_ms, trees_all = median_ms(lambda: po.Engine.trees(es), runs)
    trees = po.Engine.trees(es)
    finals = [e.final_ids() for e in es]
    t0 = time.perf_counter()
    walked = [solutions_ref.solutions(t[0], t[1], f) for t, f in zip(trees, finals)]
    walk_ms = 1e3 * (time.perf_counter() - t0)
    assert [[i for i, _, _ in w] for w in walked] == [[i for i, _, _ in s] for s in sols]
    return dict(rows=rows, nodes=int(sum(len(t[1]) for t in trees)), finals=int(sum(len(f) for f in finals)), solutions=n_sol, states=n_states,
                largest_set=max(len(s) for s in sols), runs=runs, device_gather_ms=one, device_gather_all_ms=one_all, size_query_ms=size,
                size_query_plus_gather_ms=both, baseline_get_trees_ms=trees_ms, baseline_get_trees_all_ms=trees_all,
                baseline_host_walk_python_ms=walk_ms)


def plan(po, n, cap, wave, seed=0, lead=None):
    e = lead or setup(po.Engine(0), RASTERS[n], seed)
    e.set_option("tamp_streams", 1)
    e.set_option("tamp_wave", wave)
    t0 = time.perf_counter()
    r = e.plan_tamp_rrt_viewpoints(START, [1.0 / n] * n, 0.1, 2.0, 2500, 10000, 0.05, 128, cap)
    wall = time.perf_counter() - t0
    return dict(goals=n, max_viewpoints=cap, seed=seed, wave=wave, wall_ms=1e3 * wall, grow_ms=1e3 * r["grow_s"], solutions_ms=1e3 * r["solutions_s"],
                path_ms=1e3 * r["path_s"], shortcut_ms=1e3 * r["shortcut_s"], search_ms=1e3 * r["search_s"], pool_ms=1e3 * r["pool_s"],
                goals_ms=1e3 * r["goals_s"], queries=r["queries"], observation_queries=r["observation_queries"],
                pickup_queries=r["pickup_queries"], queries_per_s=r["queries"] / wall, waves=r["waves"], search_nodes=r["search_nodes"],
                pruned=r["pruned"], viewpoints_found=r["viewpoints_found"], viewpoints_kept=r["viewpoints_kept"], largest_set=r["largest_set"],
                cost_before=r["search_cost"], cost_after=r["expected_cost"], zone_order=r["zone_order"], viewpoint_ranks=r["viewpoint_ranks"]), e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--waves", default="64,8,1")
    ap.add_argument("--shapes", default="2:0,4:2,6:2")
    ap.add_argument("--budget", type=float, default=30.0)
    args = ap.parse_args()
    import po_rrt_amd
    import tamp_viewpoints_ref as V
    from oracle import orc
    res = dict(shape=dict(start=START, prior="uniform", max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, goal_radius=0.05,
                          batch_K=128), gather=None, plans=[], skipped=[], restatement=[])
    res["gather"] = gather(po_rrt_amd, args.rows, args.runs)
    print(json.dumps(res["gather"]), flush=True)
    waves = sorted((int(w) for w in args.waves.split(",")), reverse=True)
    for shape in args.shapes.split(","):
        n, cap = (int(x) for x in shape.split(":"))
        slow = False
        for w in waves:
            if slow:
                res["skipped"].append(dict(goals=n, max_viewpoints=cap, wave=w, why="a wider wave took longer than %g s" % args.budget))
                continue
            first, e = plan(po_rrt_amd, n, cap, w)
            if first["wall_ms"] > 1e3 * args.budget:
                slow = True
                again = first
            else:
                e.set_sampler((-1.0, -1.0), (1.0, 1.0), 0)
                again, _ = plan(po_rrt_amd, n, cap, w, lead=e)
            again["first_call_pool_ms"] = first["pool_ms"]
            again["first_call_wall_ms"] = first["wall_ms"]
            res["plans"].append(again)
            print(json.dumps({k: again[k] for k in ("goals", "max_viewpoints", "wave", "wall_ms", "grow_ms", "solutions_ms", "queries",
                                                    "queries_per_s", "waves", "largest_set", "cost_before", "cost_after")}), flush=True)
            del e
    for n, cap in ((2, 0), (4, 2)):
        o = setup(orc.Oracle(), RASTERS[n], 0)
        t0 = time.perf_counter()
        r = V.Planner(o, 0).plan(START, [1.0 / n] * n, streams=1, max_viewpoints=cap)
        res["restatement"].append(dict(goals=n, max_viewpoints=cap, seconds=time.perf_counter() - t0, queries=r["queries"],
                                       cost_before=r["search_cost"], cost_after=r["expected_cost"]))
        print(json.dumps(res["restatement"][-1]), flush=True)
    out = args.out or os.path.join(os.environ.get("PORRT_OUT", os.path.join(ROOT, "profiles")), args.tag + "tamp_viewpoints.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
