"""Times the QMDP policy extractor (porrt_qmdp_plan / porrt_qmdp_react; qmdp_policy_extractor.rs) on a grown PTO graph and prints one
JSON line: the plan's device and wall milliseconds and sweep count (median of --repeat runs), 1024 react queries in one call, the
algorithmic bytes of one sweep, edges x (4 + 8 n_worlds), and -- labelled as what it is -- the single-thread time of n_worlds heap
Dijkstras in plain Python (tests/qmdp_ref.py) on the same graph, whose costs are compared bit for bit.

    python tools/qmdp_probe.py --case cfg4 --n-iter 20000
    python tools/qmdp_probe.py --case cfg_map4"""
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
    ap.add_argument("--case", default="cfg4", choices=["cfg3", "cfg4", "cfg_map4"])
    ap.add_argument("--n-iter", type=int, default=None, help="n_iter_min of the growth (the case's default otherwise)")
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import cases
    import po_rrt_amd
    import qmdp_ref as Q
    mk = getattr(cases, args.case)
    case = mk(args.n_iter) if args.n_iter else mk()
    e = cases.configure(po_rrt_amd.Engine(0), case)
    cases.grow(e, case, K=args.K)
    nw = e.n_worlds()
    plans = []
    for _ in range(args.repeat):
        e.qmdp_plan()
        plans.append(e.qmdp_info())
    rng = np.random.default_rng(0)
    low, up = case.get("low", (-1.0, -1.0)), case.get("up", (1.0, 1.0))
    starts = rng.uniform(low, up, (args.queries, 2))
    beliefs = rng.dirichlet(np.ones(nw), args.queries)
    horizons = rng.choice([0.0, 0.2, 1.0], args.queries)
    reacts, states = [], 0
    for _ in range(args.repeat):
        off = np.zeros(args.queries * nw + 1, dtype=np.uint64)
        cl = np.zeros(args.queries, dtype=np.uint64)
        t0 = time.perf_counter()
        paths = e.qmdp_react(starts, beliefs, horizons)
        wall2 = 1e3 * (time.perf_counter() - t0)
        reacts.append(dict(e.qmdp_info(), ms_two_calls=wall2))
        states = sum(len(p) for pw in paths for p in pw)
    med = lambda xs, k: float(np.median([x[k] for x in xs]))
    info = plans[-1]
    res = {"case": case.name, "n_iter": int(e.num_iterations()), "K": args.K, "nodes": int(info["nodes"]), "edges": int(info["edges"]),
           "worlds": nw, "sweeps": int(info["sweeps"]), "ms_plan_device": med(plans, "ms_plan_device"), "ms_plan_wall": med(plans, "ms_plan_wall"),
           "bytes_per_sweep_algorithmic": int(info["edges"]) * (4 + 8 * nw), "queries": args.queries, "react_states": int(states),
           "ms_react_device": med(reacts, "ms_react_device"), "ms_react_wall": med(reacts, "ms_react_wall"), "ms_react_nearest": med(reacts, "ms_nearest"),
           "ms_react_sizing_and_fetch_calls": med(reacts, "ms_two_calls")}
    if not args.no_baseline:
        q = Q.from_planner(e)
        t0 = time.perf_counter()
        q.plan_qmdp()
        res["ms_baseline_python_heap_dijkstras_single_thread"] = 1e3 * (time.perf_counter() - t0)
        res["equal_to_baseline_bitwise"] = bool(np.array_equal(e.qmdp_costs().view(np.uint64), np.array(q.cost_to_goals).view(np.uint64)))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
