"""Policy refinement on the device (porrt_bg_refine_policy: the batch refiner with one policy): one JSON line per case.

Cases: the reference's recorded problem (cfg_map4: main.rs:893-908, paper_map_4, uniform prior over 16 worlds, K = 256) for five
seeds at the drivers' 500 and 1500 iterations (main.rs:336,375,442,508,558,597,867,908), and the 12-shelf policy of bench.py's
belief_space row at 1500.  Per case: pieces, policy nodes, device ms (HIP events around the launch, after a warm-up call), wall ms
of Engine.refine_policy, expected cost before and after x 7.65 (the scale the reference reports).

Context, not a baseline: the reference records partial_shortcut at 2.95 +- 0.38 ms (map_4, 500 iterations, CPU not stated) and a
refined cost of 43.99 +- 1.25 (results/maps_paper/map_4/costs_and_timings_5000_20.txt).

    python tools/refine_probe.py [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
import po_rrt_amd  # noqa: E402

SCALE = 7.65


def pieces_of(parents):
    """Policy::decompose's piece count: the root, plus one piece per child of a branching node"""
    import numpy as np
    nc = np.bincount(parents[parents >= 0], minlength=len(parents))
    return 1 + int(nc[nc >= 2].sum())


def measure(e, name, n_iter, extra):
    (oid, par, leaf), cost0 = e.extract_policy()
    e.refine_policy(n_iter)                                   # warm-up: code object, scratch slots, the raster's upload
    t0 = time.perf_counter()
    (x, oid_r, par_r, leaf_r), cost = e.refine_policy(n_iter)
    wall = time.perf_counter() - t0
    info = e.refine_info()
    row = dict(case=name, n_iterations=n_iter, pieces=pieces_of(par), nodes=int(len(oid)), leafs=int(leaf.sum()),
               refined_nodes=int(len(oid_r)), device_ms=1e3 * info["device_s"], wall_ms=1e3 * wall,
               cost_before_x7_65=SCALE * cost0, cost_after_x7_65=SCALE * cost, **extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    rows = []
    e = po_rrt_amd.Engine(0)
    prior = [1.0 / 16] * 16
    for seed in range(5):
        case = cases.cfg_map4(5000, seed)
        cases.configure(e, case)
        cases.grow(e, case, K=256)
        e.build_belief_graph(prior)
        e.compute_expected_costs()
        for n in (500, 1500):
            try:
                rows.append(measure(e, "cfg_map4 seed %d" % seed, n, {"reference_partial_shortcut_ms": 2.95,
                                                                      "reference_refined_cost_x7_65": 43.99}))
            except po_rrt_amd.PorrtError as err:              # (extract_policy's walk of belief_graph.rs:193-213 does not end)
                rows.append({"case": "cfg_map4 seed %d" % seed, "n_iterations": n, "error": str(err)})
                print(json.dumps(rows[-1]), flush=True)
    # bench.py belief_space: the 12-shelf problem after its four growths (the policy it reports)
    case = cases.cfg4(20000, 20000)
    case.update(start=(0.0, -0.3))
    e2 = cases.configure(po_rrt_amd.Engine(0), case)
    for _ in range(4):
        cases.grow(e2, case, K=256)
    e2.build_belief_graph([1.0 / 12] * 12)
    e2.compute_expected_costs()
    rows.append(measure(e2, "belief_space 12 shelves (bench.py)", 1500, {}))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
