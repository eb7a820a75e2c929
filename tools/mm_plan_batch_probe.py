"""porrt_mm_plan_batch (many multi-modal PRM plans on one map in one device call) beside what there was before it: porrt_mm_plan +
porrt_mm_refine_policy plan after plan on one context, in one process.  The reference driver's shape (main.rs:100-166, 546-575): 5000
samples per belief, PartialShortCut(1500), uniform prior, 2 goals (committed zones) and 4 / 6 / 8 goals (free-centroid zones), the
plans' seeds 0 .. n - 1 (sampler and discrete alike).  Per size and number of plans, after a warm-up of each form, --reps alternations
of the one-by-one loop and the one batch call, timed with a host clock around calls that end in a synchronise; the batch's statuses
and cost bits are compared with the singles' at every size timed.  Also a batch of one against the single sequence, and the batch
under several values of option mm_plan_batch_max_nodes (--limits, at --limit-plans plans of --limit-goals goals): the cut into passes.
Writes profiles/mm_plan_batch.json (or --out).
usage: python tools/mm_plan_batch_probe.py [--goals 2,4,6,8] [--plans 10,100] [--reps 3] [--limits a,b,..] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import cases  # noqa: E402
import po_rrt_amd  # noqa: E402

REFINE = 1500
STEP, RADIUS = 0.1, 2.0


def engine(n_goals):
    zones = "map_benchmark_like_2_goals_zone_ids" if n_goals == 2 else "map_benchmark_like_%d_free_zone_ids" % n_goals
    c = cases.cfg2(10)
    c.update(zones=zones, visibility=0.5)
    return cases.configure(po_rrt_amd.Engine(0), c), c


def one_by_one(e, c, prior, n_iter, seeds):
    """porrt_mm_plan + porrt_mm_refine_policy per seed on one context: (status, cost bits) per plan and the loop's wall time"""
    out = []
    b = np.ascontiguousarray(prior, dtype=np.float64)
    s = np.ascontiguousarray(c.start, dtype=np.float64)
    t = time.perf_counter()
    for seed in seeds:
        e.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
        e.set_discrete_seed(seed)
        n = int(e._l.porrt_mm_plan(e._c, s, b, len(b), STEP, RADIUS, n_iter))
        if n >= 0:
            _, cost = e.mm_refine_policy(REFINE)
            out.append((0, cost))
        else:
            out.append((1, float("inf")))
    return out, 1e3 * (time.perf_counter() - t)


def batch(e, c, prior, n_iter, seeds):
    n = len(seeds)
    t = time.perf_counter()
    raw = e.plan_mm_prm_batch_raw([c.start] * n, [prior] * n, STEP, RADIUS, n_iter, REFINE, sampler_seeds=seeds, discrete_seeds=seeds)
    wall = 1e3 * (time.perf_counter() - t)
    info = e.mm_plan_batch_info()
    info["ms_wall_python"] = wall
    return raw, info


def assert_same(raw, want):
    off, status, cost, rstatus, rcost = raw[:5]
    for q, (st, c) in enumerate(want):
        assert (status[q] == 0) == (st == 0), "plan %d: status %d" % (q, status[q])
        if st == 0:
            assert np.float64(rcost[q]).view(np.uint64) == np.float64(c).view(np.uint64), "plan %d: refined cost" % q


def spread(v):
    return {"runs": v, "median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


STAGES = ("ms_host", "ms_points", "ms_roadmaps", "ms_belief_graph", "ms_costs", "ms_policies", "ms_refine", "ms_device")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", default="2,4,6,8")
    ap.add_argument("--plans", default="10,100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--limits", default=",".join(str(1 << k) for k in (16, 18, 20, 21, 22, 23, 24)))
    ap.add_argument("--limit-goals", default="2,4")
    ap.add_argument("--limit-plans", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mm_plan_batch.json"))
    a = ap.parse_args()
    out = {"what": "n plans of the driver shape (%d per belief, PartialShortCut(%d), uniform prior, seeds 0 .. n - 1): porrt_mm_plan + porrt_mm_refine_policy "
                   "one by one on one context beside one porrt_mm_plan_batch call; milliseconds" % (a.iters, REFINE), "sizes": {}, "pass_limits": {}}
    limit_goals = [int(x) for x in a.limit_goals.split(",") if x]
    for n_goals in [int(x) for x in a.goals.split(",") if x]:
        prior = [1.0 / n_goals] * n_goals
        e1, c = engine(n_goals)                                 # the one-by-one context
        eb, _ = engine(n_goals)                                 # the batch's
        res = {}
        for n in [1] + [int(x) for x in a.plans.split(",") if x]:
            seeds = list(range(n))
            want, _ = one_by_one(e1, c, prior, a.iters, seeds)  # warm-up of each form, and the comparison
            raw, info = batch(eb, c, prior, a.iters, seeds)
            assert_same(raw, want)
            one, many, infos = [], [], []
            for _ in range(a.reps):
                one.append(one_by_one(e1, c, prior, a.iters, seeds)[1])
                raw, info = batch(eb, c, prior, a.iters, seeds)
                many.append(info["ms_wall_python"])
                infos.append(info)
            assert_same(raw, want)
            res[str(n)] = {"one_by_one_ms": spread(one), "batch_ms": spread(many), "batch_info": infos, "ratio_of_medians": spread(one)["median"] / spread(many)["median"],
                           "slowest_batch_below_fastest_one_by_one": max(many) < min(one)}
            i = sorted(infos, key=lambda x: x["ms_wall"])[len(infos) // 2]
            print("%d goals, %3d plans: one by one %.2f ms (%.2f .. %.2f) | batch %.2f ms (%.2f .. %.2f) | %s | passes %d nodes %d modes %d ok %d upload %d B" % (
                n_goals, n, spread(one)["median"], min(one), max(one), spread(many)["median"], min(many), max(many),
                " ".join("%s %.2f" % (k[3:], i[k]) for k in STAGES), i["passes"], i["nodes"], i["modes"], i["policies_ok"], i["upload_bytes"]), flush=True)
        out["sizes"][str(n_goals)] = res
        if n_goals in limit_goals:
            seeds = list(range(a.limit_plans))
            default = eb.get_option("mm_plan_batch_max_nodes")
            limits = [int(x) for x in a.limits.split(",")]
            cuts = {str(lim): [] for lim in limits}
            for rep in range(a.reps + 1):                       # (the first round warms up)
                for lim in limits:
                    eb.set_option("mm_plan_batch_max_nodes", lim)
                    _, info = batch(eb, c, prior, a.iters, seeds)
                    if rep:
                        cuts[str(lim)].append({k: info[k] for k in ("ms_wall_python", "passes") + STAGES})
            eb.set_option("mm_plan_batch_max_nodes", default)
            out["pass_limits"][str(n_goals)] = {"plans": a.limit_plans, "limits": cuts}
            for lim, runs in cuts.items():
                print("%d goals, %d plans, mm_plan_batch_max_nodes %s: %d passes, %s" % (
                    n_goals, a.limit_plans, lim, runs[0]["passes"], ", ".join("wall %.2f costs %.2f roadmaps %.2f" % (x["ms_wall_python"], x["ms_costs"], x["ms_roadmaps"]) for x in runs)),
                    flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
