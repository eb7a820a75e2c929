"""Times many TAMP-RRT A* plans in one device call (porrt_tamp_rrt_plan_astar_batch) against the same plans one
by one (porrt_tamp_rrt_plan_astar at wave 8, section 23's best width), and writes profiles/<tag>tamp_astar_batch.json (or the file
--out names).

The workload is the reference's n_runs loop (main.rs:100-199): the free-centroid rasters at 2 / 4 / 6 / 8 goals, seeds 0 .. n - 1,
start (0, -1), uniform prior, 0.1 / 2.0 / 2500 / 10000, goal radius 0.05, batch_K 128.  Grid: n_plans x tamp_wave x tamp_pool.  Both
sides run in this process on leads of their own, alternating -- batch, one by one, batch, one by one -- and the second call of each
is the timed one (pool and arena warm).  The results of the timed calls are checked equal, plan by plan and bit for bit.  Recorded
beside the walls: rounds, rows per porrt_grow_batch (the mean rows of a round's observation or pickup stage, capped by the pool),
and the seconds split of porrt_tamp_info."""
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

RASTERS = {2: "map_benchmark_like_2_goals_zone_ids", 4: "map_benchmark_like_4_free_zone_ids", 6: "map_benchmark_like_6_free_zone_ids",
           8: "map_benchmark_like_8_free_zone_ids"}
START = (0.0, -1.0)
PARAMS = (0.1, 2.0, 2500, 10000, 0.05, 128)
SINGLE_WAVE = 8
SPLIT = ("total_s", "grow_s", "path_s", "shortcut_s", "search_s", "pool_s", "goals_s", "children_s", "chain_s")


def lead(po, zones, wave, pool):
    import cases
    e = po.Engine(0)
    e.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    e.set_zones(cases.load_map(zones), 0.5)
    e.set_sampler((-1.0, -1.0), (1.0, 1.0), 0)
    e.set_option("tamp_streams", 1)
    e.set_option("tamp_wave", wave)
    e.set_option("tamp_pool", pool)
    return e


def one_by_one(e, goals, n_plans):
    """the plans of seeds 0 .. n_plans - 1 through the single call: (seconds inside the calls, the plans, summed queries)"""
    prior = [1.0 / goals] * goals
    wall, out = 0.0, []
    for seed in range(n_plans):
        e.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
        t0 = time.perf_counter()
        try:
            r = e.plan_tamp_rrt_astar(START, prior, *PARAMS)
        except Exception:                          # a plan without a path: its time counts, it has no policy
            r = None
        wall += time.perf_counter() - t0
        out.append(r)
    return wall, out


def batch(e, goals, n_plans):
    prior = [[1.0 / goals] * goals] * n_plans
    t0 = time.perf_counter()
    out = e.plan_tamp_rrt_astar_batch([START] * n_plans, prior, list(range(n_plans)), *PARAMS)
    return time.perf_counter() - t0, out


def equal(b, s):
    if s is None:
        return b["status"] != 0
    return (b["status"] == 0 and b["zone_order"] == s["zone_order"] and b["search_cost"] == s["search_cost"] and
            b["expected_cost"] == s["expected_cost"] and b["search_nodes"] == s["search_nodes"] and
            np.array_equal(b["xy"].view(np.uint64), s["xy"].view(np.uint64)) and np.array_equal(b["parents"], s["parents"]) and
            np.array_equal(b["beliefs"].view(np.uint64), s["beliefs"].view(np.uint64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--goals", default="2,4,6,8")
    ap.add_argument("--plans", default="1,10,100")
    ap.add_argument("--waves", default="1,2,8")
    ap.add_argument("--pools", default="512,2048")
    args = ap.parse_args()
    import po_rrt_amd
    ints = lambda s: [int(x) for x in s.split(",")]
    res = dict(shape=dict(start=START, prior="uniform", max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, goal_radius=0.05,
                          batch_K=128, seeds="0 .. n_plans - 1", single_wave=SINGLE_WAVE, single_pool=512), rows=[])
    for goals in ints(args.goals):
        single = lead(po_rrt_amd, RASTERS[goals], SINGLE_WAVE, 512)
        for pool in ints(args.pools):
            for wave in ints(args.waves):
                b = lead(po_rrt_amd, RASTERS[goals], wave, pool)
                for n_plans in ints(args.plans):
                    batch(b, goals, n_plans)
                    one_by_one(single, goals, n_plans)
                    wall_b, got = batch(b, goals, n_plans)
                    info = {k: got[0][k] for k in SPLIT}
                    call_queries, rounds = b.tamp_info()["queries"], b.tamp_info()["waves"]
                    wall_s, ref = one_by_one(single, goals, n_plans)
                    # a round grows its rows in two stages (observation, pickup), each cut into chunks of `pool` rows: the mean rows
                    # of a stage, and that figure capped by the pool = the mean rows of one porrt_grow_batch while no stage is cut
                    per_stage = call_queries / (2.0 * max(rounds, 1))
                    row = dict(goals=goals, n_plans=n_plans, wave=wave, pool=pool, batch_ms=1e3 * wall_b, one_by_one_ms=1e3 * wall_s,
                               ratio=wall_s / wall_b, equal=all(equal(x, y) for x, y in zip(got, ref)), ok=sum(1 for x in got if x["status"] == 0),
                               rounds=rounds, queries=call_queries, one_by_one_queries=sum(r["queries"] for r in ref if r is not None),
                               rows_per_stage=per_stage, rows_per_grow_batch=min(per_stage, float(pool)), speculated=b.tamp_astar_info()["speculated"],
                               pool_contexts=got[0]["pool"], arena_used=got[0]["arena_used"], arena_grown=got[0]["arena_grown"], **info)
                    res["rows"].append(row)
                    print(json.dumps({k: row[k] for k in ("goals", "n_plans", "wave", "pool", "batch_ms", "one_by_one_ms", "ratio", "equal", "rounds",
                                                           "queries", "rows_per_grow_batch", "grow_s")}), flush=True)
    out = args.out or os.path.join(os.environ.get("PORRT_OUT", os.path.join(ROOT, "profiles")), args.tag + "tamp_astar_batch.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
