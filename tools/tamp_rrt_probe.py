"""Times the TAMP-RRT branch-and-bound planner (porrt_tamp_rrt_plan; map_shelves_tamp_rrt.rs:159-291) and writes
profiles/<tag>tamp_rrt.json (or the file --out names).

The reference driver's shape (main.rs:523-545, 612-633): start (0, -1), uniform prior, max_step 0.1, search_radius 2, n_iter_min 2500,
n_iter_max 10000, goal radius 0.05, batch_K 128, on the benchmark map with the 2-goal raster and the 4 / 6 / 8 free-centroid rasters.
  1. one stream per edge (tamp_streams 1) at several wave widths and seeds: wall ms, growth ms, queries, queries/s, waves, search nodes,
     cost before and after the shortcut, worker creation and goal setting;
  2. the shared stream (tamp_streams 0, the reference's order) at 2 and 4 goals;
  3. the restatement (tests/tamp_rrt_ref.py) on the CPU oracle at 2 and 4 goals: its seconds and query counts;
  4. the multi-modal PRM planner (porrt_mm_plan, 5000 samples per belief, PartialShortCut 1500) on the same rasters: its cost beside."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

RASTERS = {2: "map_benchmark_like_2_goals_zone_ids", 4: "map_benchmark_like_4_free_zone_ids",
           6: "map_benchmark_like_6_free_zone_ids", 8: "map_benchmark_like_8_free_zone_ids"}
START = (0.0, -1.0)


def setup(eng, zones, seed):
    import cases
    eng.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    eng.set_zones(cases.load_map(zones), 0.5)
    eng.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return eng


def run(po, n, seed, streams, wave, lead=None):
    e = lead or setup(po.Engine(0), RASTERS[n], seed)
    e.set_option("tamp_streams", streams)
    e.set_option("tamp_wave", wave)
    t0 = time.perf_counter()
    r = e.plan_tamp_rrt(START, [1.0 / n] * n, 0.1, 2.0, 2500, 10000, 0.05, 128)
    wall = time.perf_counter() - t0
    out = dict(goals=n, seed=seed, streams=streams, wave=wave, wall_ms=1e3 * wall, grow_ms=1e3 * r["grow_s"], path_ms=1e3 * r["path_s"],
               shortcut_ms=1e3 * r["shortcut_s"], search_ms=1e3 * r["search_s"], pool_ms=1e3 * r["pool_s"], goals_ms=1e3 * r["goals_s"],
               queries=r["queries"], queries_per_s=r["queries"] / wall, waves=r["waves"], search_nodes=r["search_nodes"],
               pruned=r["pruned"], cost_before=r["search_cost"], cost_after=r["expected_cost"], zone_order=r["zone_order"],
               policy_nodes=len(r["parents"]))
    return out, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--goals", default="2,4,6,8")
    ap.add_argument("--waves", default="1,8,32,128")
    ap.add_argument("--seeds", default="0,1")
    args = ap.parse_args()
    import po_rrt_amd
    import tamp_rrt_ref as R
    from oracle import orc
    goals = [int(g) for g in args.goals.split(",")]
    waves = [int(w) for w in args.waves.split(",")]
    seeds = [int(s) for s in args.seeds.split(",")]
    res = dict(shape=dict(start=START, prior="uniform", max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, goal_radius=0.05,
                          batch_K=128), per_edge=[], shared=[], restatement=[], mm_prm=[])
    # 1. one stream per edge; the first run of a lead makes its worker pool (reported), a second run of the same shape on the same
    #    lead is the one timed for the table
    for n in goals:
        for seed in seeds:
            for w in waves:
                if n == 8 and w == 1 and seed != seeds[0]:
                    continue
                first, e = run(po_rrt_amd, n, seed, 1, w)
                e.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
                again, _ = run(po_rrt_amd, n, seed, 1, w, lead=e)
                again["first_call_pool_ms"] = first["pool_ms"]
                again["first_call_wall_ms"] = first["wall_ms"]
                res["per_edge"].append(again)
                print(json.dumps({k: again[k] for k in ("goals", "seed", "wave", "wall_ms", "grow_ms", "queries", "queries_per_s", "waves",
                                                        "cost_before", "cost_after", "first_call_pool_ms")}), flush=True)
                del e
    # 2. the shared stream
    for n in [g for g in goals if g <= 4]:
        r, _ = run(po_rrt_amd, n, 0, 0, 1)
        res["shared"].append(r)
        print(json.dumps({k: r[k] for k in ("goals", "streams", "wall_ms", "queries", "cost_before", "cost_after")}), flush=True)
    # 3. the restatement on the CPU oracle
    for n in [g for g in goals if g <= 4]:
        for streams in (0, 1):
            o = setup(orc.Oracle(), RASTERS[n], 0)
            t0 = time.perf_counter()
            r = R.Planner(o, 0).plan(START, [1.0 / n] * n, streams=streams)
            s = time.perf_counter() - t0
            res["restatement"].append(dict(goals=n, streams=streams, seconds=s, queries=r["queries"], cost_before=r["search_cost"],
                                           cost_after=r["expected_cost"]))
            print(json.dumps(res["restatement"][-1]), flush=True)
    # 4. the multi-modal PRM planner on the same rasters (the reference's own comparison, main.rs:100-200)
    for n in goals:
        e = setup(po_rrt_amd.Engine(0), RASTERS[n], 0)
        e.set_discrete_seed(0)
        t0 = time.perf_counter()
        try:
            _, cost = e.plan_mm_prm(START, [1.0 / n] * n, 0.1, 2.0, 5000, refine_iterations=1500)
        except po_rrt_amd.engine.PorrtError as ex:
            cost = "error %d" % ex.code
        res["mm_prm"].append(dict(goals=n, cost_after_refine=cost, wall_ms=1e3 * (time.perf_counter() - t0)))
        print(json.dumps(res["mm_prm"][-1]), flush=True)
    out = args.out or os.path.join(os.environ.get("PORRT_OUT", os.path.join(ROOT, "profiles")), args.tag + "tamp_rrt.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
