"""Times many TAMP-RRT branch-and-bound plans in one device call (porrt_tamp_rrt_plan_batch) against the sum
of the same plans one by one through the shipped single call (porrt_tamp_rrt_plan at its default tamp_wave 128 and tamp_pool 512),
and writes profiles/<tag>tamp_bnb_batch.json (or the file --out names).

The workload is the reference's n_runs loop (main.rs:100-199): the free-centroid rasters at 2 / 4 / 6 / 8 goals, seeds 0 .. n - 1,
start (0, -1), uniform prior, 0.1 / 2.0 / 2500 / 10000, goal radius 0.05, batch_K 128.  A cell is (goals, n_plans); it runs in a
process of its own under a time limit of its own (--cell-timeout); the rows a cell has finished are kept when it runs out of time,
and the probe ends there.  Within a cell every (tamp_pool, tamp_wave) of the grid gets a lead of its own, and so does the baseline.
Both sides run in the cell's process, alternating -- batch, one by one, batch, one by one -- on the first configuration of the
grid, and the second call of each is the timed one (pool and arena warm); the later configurations run their batch twice and time
the second, against the same baseline figure.
`equal`: every plan of the timed batch has the policy, both costs and the zone order of the baseline's plan (they do not depend on
the width), and the first --check plans also have search_nodes, queries, waves and pruned of plan_tamp_rrt alone at the batch's
own width on a fresh engine seeded alike."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
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
SINGLE_WAVE, SINGLE_POOL = 128, 512
SPLIT = ("total_s", "grow_s", "path_s", "shortcut_s", "search_s", "pool_s", "goals_s", "children_s", "chain_s")
CELLS = "2:10,2:100,4:10,4:100,6:10,6:100,8:10"


def lead(po, zones, wave, pool, seed=0):
    import cases
    e = po.Engine(0)
    e.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    e.set_zones(cases.load_map(zones), 0.5)
    e.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    e.set_option("tamp_streams", 1)
    e.set_option("tamp_wave", wave)
    e.set_option("tamp_pool", pool)
    return e


def one_by_one(e, goals, n_plans):
    """the plans of seeds 0 .. n_plans - 1 through the single call: (seconds inside the calls, the plans).  set_sampler seeds both of
    the lead's samplers, which is the fresh context of the batch's contract."""
    prior = [1.0 / goals] * goals
    wall, out = 0.0, []
    for seed in range(n_plans):
        e.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
        t0 = time.perf_counter()
        try:
            r = e.plan_tamp_rrt(START, prior, *PARAMS)
        except Exception:                          # a plan without a path: its time counts, it has no policy
            r = None
        wall += time.perf_counter() - t0
        out.append(r)
    return wall, out


def batch(e, goals, n_plans):
    prior = [[1.0 / goals] * goals] * n_plans
    t0 = time.perf_counter()
    out = e.plan_tamp_rrt_batch([START] * n_plans, prior, list(range(n_plans)), None, *PARAMS)
    return time.perf_counter() - t0, out


def same_policy(b, s):
    if s is None:
        return b["status"] != 0
    return (b["status"] == 0 and b["zone_order"] == s["zone_order"] and b["search_cost"] == s["search_cost"] and
            b["expected_cost"] == s["expected_cost"] and np.array_equal(b["xy"].view(np.uint64), s["xy"].view(np.uint64)) and
            np.array_equal(b["parents"], s["parents"]) and np.array_equal(b["beliefs"].view(np.uint64), s["beliefs"].view(np.uint64)))


def same_counts(b, s):
    return s is not None and all(b[k] == s[k] for k in ("search_nodes", "queries", "waves", "pruned"))


def run_cell(goals, n_plans, waves, pools, check, out_path):
    import po_rrt_amd
    rows = []
    single = lead(po_rrt_amd, RASTERS[goals], SINGLE_WAVE, SINGLE_POOL)
    wall_s = ref = None
    at_width = {}                                  # wave -> the first `check` plans alone at that width
    for pool in pools:
        for wave in waves:
            b = lead(po_rrt_amd, RASTERS[goals], wave, pool)
            batch(b, goals, n_plans)
            if ref is None:
                one_by_one(single, goals, n_plans)
            wall_b, got = batch(b, goals, n_plans)
            if ref is None:
                wall_s, ref = one_by_one(single, goals, n_plans)
            if wave not in at_width:
                at_width[wave] = one_by_one(lead(po_rrt_amd, RASTERS[goals], wave, SINGLE_POOL), goals, min(check, n_plans))[1]
            info = {k: got[0][k] for k in SPLIT}
            t = b.tamp_info()
            call_queries, rounds = t["queries"], t["waves"]
            equal = all(same_policy(x, y) for x, y in zip(got, ref)) and all(same_counts(x, y) for x, y in zip(got, at_width[wave]))
            row = dict(goals=goals, n_plans=n_plans, wave=wave, pool=pool, batch_ms=1e3 * wall_b, one_by_one_ms=1e3 * wall_s,
                       ratio=wall_s / wall_b, equal=equal, checked_at_width=len(at_width[wave]), ok=sum(1 for x in got if x["status"] == 0),
                       rounds=rounds, queries=call_queries, one_by_one_queries=sum(r["queries"] for r in ref if r is not None),
                       us_per_row=1e6 * wall_b / max(call_queries, 1), rows_per_stage=call_queries / (2.0 * max(rounds, 1)),
                       search_nodes=t["search_nodes"], pruned=t["pruned"], pool_contexts=got[0]["pool"], arena_states=got[0]["arena_states"],
                       arena_used=got[0]["arena_used"], arena_grown=got[0]["arena_grown"], **info)
            rows.append(row)
            print(json.dumps({k: row[k] for k in ("goals", "n_plans", "wave", "pool", "batch_ms", "one_by_one_ms", "ratio", "equal", "rounds",
                                                   "queries", "us_per_row", "arena_used", "arena_grown", "grow_s", "search_s")}), flush=True)
            with open(out_path, "w") as f:         # what is done so far survives the cell's time limit
                json.dump(rows, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--cells", default=CELLS, help="goals:n_plans, comma separated")
    ap.add_argument("--waves", default="1,2,8,128")
    ap.add_argument("--pools", default="512,2048")
    ap.add_argument("--check", type=int, default=10, help="plans per configuration also run alone at the batch's width")
    ap.add_argument("--cell-timeout", type=float, default=240.0, help="seconds per cell")
    ap.add_argument("--date", default=time.strftime("%Y-%m-%d"))
    ap.add_argument("--run-cell", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cell-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",")]
    if args.run_cell:
        goals, n_plans = (int(x) for x in args.run_cell.split(":"))
        run_cell(goals, n_plans, ints(args.waves), ints(args.pools), args.check, args.cell_out)
        return
    res = dict(date=args.date,
               shape=dict(start=START, prior="uniform", max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, goal_radius=0.05,
                          batch_K=128, seeds="0 .. n_plans - 1", single_wave=SINGLE_WAVE, single_pool=SINGLE_POOL, check=args.check,
                          cell_timeout_s=args.cell_timeout),
               rows=[], cells_cut_short=[])
    for cell in args.cells.split(","):
        with tempfile.TemporaryDirectory() as tmp:
            part = os.path.join(tmp, "cell.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--run-cell", cell, "--cell-out", part, "--waves", args.waves, "--pools", args.pools,
                   "--check", str(args.check)]
            try:
                rc = subprocess.run(cmd, timeout=args.cell_timeout).returncode
            except subprocess.TimeoutExpired:
                rc = "time limit"
            if os.path.exists(part):
                with open(part) as f:
                    res["rows"] += json.load(f)
            if rc != 0:
                res["cells_cut_short"].append(dict(cell=cell, why=rc))
                print("cell", cell, "ended with", rc, flush=True)
                break                              # nothing more is started on a device after a process that died or hung on it
    out = args.out or os.path.join(os.environ.get("PORRT_OUT", os.path.join(ROOT, "profiles")), args.tag + "tamp_bnb_batch.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
