"""porrt_bg_extract_policies (the policy walk on the device, many starts per call) beside Engine.extract_policy (the single call: the same
walk as a batch of one with a result of its own) on the same graphs in the same process: the 12-shelf belief-space graph of bench.py
(cfg4, 20 000 iterations, 4095 beliefs, uniform prior) and cfg_map4 seed 1 (the reference's recorded problem, K = 1, 16 worlds).
Per graph: ms_device / ms_wall of the new call for n = 1 (start 0) and for n = 1024 starts drawn from a fixed seed, after a warm-up
call, and the wall time of extract_policy() right after a cost run (so that it walks).  Writes profiles/policies.json (or --out).
usage: python tools/policies_probe.py [--reps 5] [--out PATH]"""
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


def median(v):
    return sorted(v)[len(v) // 2]


def probe(e, reps, n_many=1024, seed=1024):
    n = len(e.expected_costs())
    starts = np.random.default_rng(seed).integers(0, n, size=n_many).astype(np.uint64)
    starts[0] = 0
    host = []
    for _ in range(reps):                                       # the single call (a cost run before it, or it hands out its copy)
        e.compute_expected_costs()
        t = time.perf_counter()
        (oid, par, leaf), _ = e.extract_policy()
        host.append(1e3 * (time.perf_counter() - t))
    e.extract_policies([0])                                     # warm-up: code object, pool
    e.extract_policies(starts)
    out = {"belief_nodes": n, "policy_nodes_from_0": len(oid), "single_call_ms_wall": median(host), "single_call_ms_wall_runs": host}
    for name, st in (("n1", starts[:1]), ("n%d" % n_many, starts)):
        runs = []
        for _ in range(reps):
            t = time.perf_counter()
            got, status = e.extract_policies(st)
            wall = 1e3 * (time.perf_counter() - t)
            info = e.policies_info()
            info["ms_wall_python"] = wall
            runs.append(info)
        assert status[0] == 0 and np.array_equal(got[0][0][0], oid) and np.array_equal(got[0][0][1], par) and np.array_equal(got[0][0][2], leaf)
        out[name] = {"median_by_wall": sorted(runs, key=lambda i: i["ms_wall"])[len(runs) // 2], "runs": runs}
    one, many = out["n1"]["median_by_wall"], out["n%d" % n_many]["median_by_wall"]
    out["single_call_over_n1_wall"] = out["single_call_ms_wall"] / one["ms_wall"]
    out["n%d_over_n1_wall" % n_many] = many["ms_wall"] / one["ms_wall"]
    out["us_per_policy_node_n1_device"] = 1e3 * one["ms_device"] / max(one["nodes"], 1)
    out["us_per_policy_node_n%d_device" % n_many] = 1e3 * many["ms_device"] / max(many["nodes"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policies.json"))
    a = ap.parse_args()
    out = {"what": "policies from n belief nodes in one device call (porrt_bg_extract_policies) beside the single call (porrt_bg_extract_policy)"}
    case = cases.cfg4(20000, 20000)
    case.update(start=(0.0, -0.3))
    e = cases.configure(po_rrt_amd.Engine(), case)
    cases.grow(e, case, K=256)
    e.build_belief_graph([1.0 / 12] * 12)
    e.compute_expected_costs()
    out["twelve_shelves"] = probe(e, a.reps)
    e.close()
    case = cases.cfg_map4(5000, 1)
    e = cases.configure(po_rrt_amd.Engine(), case)
    cases.grow(e, case, K=1)
    e.build_belief_graph([1.0 / 16] * 16)
    e.compute_expected_costs()
    out["map4_seed1"] = probe(e, a.reps)
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    brief = {k: {k2: v2 for k2, v2 in v.items() if not k2.endswith("runs") and not isinstance(v2, dict)} | {k2: v[k2]["median_by_wall"] for k2 in v if isinstance(v[k2], dict)}
             for k, v in out.items() if isinstance(v, dict)}
    print(json.dumps(brief, indent=1), flush=True)


if __name__ == "__main__":
    main()
