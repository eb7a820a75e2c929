"""Times the TAMP-RRT A* planner (porrt_tamp_rrt_plan_astar; plan_astar, map_shelves_tamp_rrt.rs:432-563) beside
the branch and bound (porrt_tamp_rrt_plan, section 17) in one run, and writes profiles/<tag>tamp_astar.json (or the file --out names).

The shape of tools/tamp_rrt_probe.py: start (0, -1), uniform prior, 0.1 / 2.0 / 2500 / 10000, goal radius 0.05, batch_K 128, seed 0, per-edge
streams, on the benchmark map with the 2 / 4 / 6 / 8 free-centroid rasters at several wave widths, then the 12-zone raster at the width
that was fastest at the largest of those.  Every result is the SECOND plan on a lead (the first makes its worker pool): wall ms,
queries, rounds (waves), speculated expansions, per-phase seconds, cost before and after the shortcut, and what the path arena held --
the bytes a search that fetched every child's paths would have moved, beside the record bytes that were moved."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

RASTERS = {2: "map_benchmark_like_2_goals_zone_ids", 4: "map_benchmark_like_4_free_zone_ids", 6: "map_benchmark_like_6_free_zone_ids",
           8: "map_benchmark_like_8_free_zone_ids", 12: "map_benchmark_like_12_free_zone_ids"}
START = (0.0, -1.0)
RECORD_BYTES, BEST_PATH_BYTES, STATE_BYTES = 64, 40, 16      # AstarChildOut, BestPath, double2


def setup(eng, zones, seed):
    import cases
    eng.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    eng.set_zones(cases.load_map(zones), 0.5)
    eng.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return eng


def second_plan(po, n, seed, wave, astar):
    e = setup(po.Engine(0), RASTERS[n], seed)
    e.set_option("tamp_streams", 1)
    e.set_option("tamp_wave", wave)
    plan = e.plan_tamp_rrt_astar if astar else e.plan_tamp_rrt
    first = plan(START, [1.0 / n] * n, 0.1, 2.0, 2500, 10000, 0.05, 128)
    e.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    t0 = time.perf_counter()
    r = plan(START, [1.0 / n] * n, 0.1, 2.0, 2500, 10000, 0.05, 128)
    wall = time.perf_counter() - t0
    out = dict(search="astar" if astar else "branch_and_bound", goals=n, seed=seed, wave=wave, wall_ms=1e3 * wall, queries=r["queries"],
               rounds=r["waves"], search_nodes=r["search_nodes"], grow_s=r["grow_s"], path_s=r["path_s"], shortcut_s=r["shortcut_s"],
               search_s=r["search_s"], goals_s=r["goals_s"], pool_s=r["pool_s"], cost_before=r["search_cost"], cost_after=r["expected_cost"],
               zone_order=r["zone_order"], first_call_wall_ms=1e3 * first["total_s"])
    if astar:
        out.update(speculated=r["speculated"], children_s=r["children_s"], chain_s=r["chain_s"], arena_states=r["arena_states"],
                   arena_used=r["arena_used"], arena_grown=r["arena_grown"])
        # every query with a path put it into the arena: fetching them all would have moved arena_used states; what was moved
        # instead is one record per child, one BestPath per observation query and the winning chain's states
        n_children = r["queries"] - r["queries"] // 2          # children expanded: one observation query each, at most one pickup
        out.update(all_paths_bytes=r["arena_used"] * STATE_BYTES, policy_states=len(r["parents"]),
                   moved_bytes=n_children * (RECORD_BYTES + BEST_PATH_BYTES) + len(r["parents"]) * STATE_BYTES)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--goals", default="2,4,6,8")
    ap.add_argument("--waves", default="1,8,32,128")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--twelve", type=int, default=1, help="also plan the 12-zone raster at the best width (0 = no)")
    ap.add_argument("--bb-wave", type=int, default=128, help="the branch and bound's width (its default)")
    args = ap.parse_args()
    import po_rrt_amd
    goals = [int(g) for g in args.goals.split(",")]
    waves = [int(w) for w in args.waves.split(",")]
    res = dict(shape=dict(start=START, prior="uniform", max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, goal_radius=0.05,
                          batch_K=128, seed=args.seed, streams=1), astar=[], branch_and_bound=[], twelve=[])
    show = ("search", "goals", "wave", "wall_ms", "queries", "rounds", "speculated", "cost_before", "cost_after")
    for n in goals:
        for w in waves:
            r = second_plan(po_rrt_amd, n, args.seed, w, True)
            res["astar"].append(r)
            print(json.dumps({k: r.get(k) for k in show}), flush=True)
        r = second_plan(po_rrt_amd, n, args.seed, args.bb_wave, False)
        res["branch_and_bound"].append(r)
        print(json.dumps({k: r.get(k) for k in show}), flush=True)
    if args.twelve:
        last = [r for r in res["astar"] if r["goals"] == goals[-1]]
        best = min(last, key=lambda r: r["wall_ms"])["wave"]
        r = second_plan(po_rrt_amd, 12, args.seed, best, True)
        res["twelve"].append(r)
        print(json.dumps({k: r.get(k) for k in show}), flush=True)
    out = args.out or os.path.join(os.environ.get("PORRT_OUT", os.path.join(ROOT, "profiles")), args.tag + "tamp_astar.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
