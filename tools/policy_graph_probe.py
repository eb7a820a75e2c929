"""Times get_policy_graph on the device (porrt_qmdp_policy_graph; pto_graph.rs:363-419) on a grown and QMDP-planned PTO graph and prints
one JSON line: device and wall milliseconds of the three passes (classify, simplex, compaction; median of --repeat runs), the share
of the adjacency entries per `how` value, the pivots, and -- labelled as what it is -- the single-thread Python time of the
restatement (tests/policy_graph_ref.py) on a seeded sample of entries, which is compared with the device entry for entry.

    python tools/policy_graph_probe.py --case cfg4 --n-iter 20000
    python tools/policy_graph_probe.py --case cfg_map4"""
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
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000, help="entries the restatement decides (0: none)")
    args = ap.parse_args()
    import cases
    import po_rrt_amd
    import policy_graph_ref as P
    import qmdp_ref as Q
    mk = getattr(cases, args.case)
    case = mk(args.n_iter) if args.n_iter else mk()
    e = cases.configure(po_rrt_amd.Engine(0), case)
    cases.grow(e, case, K=args.K)
    e.qmdp_plan()
    runs = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        e.qmdp_policy_graph()
        wall = 1e3 * (time.perf_counter() - t0)
        runs.append(dict(e.qmdp_policy_graph_info(), ms_call=wall))
    med = lambda k: float(np.median([r[k] for r in runs]))
    info = runs[-1]
    n = max(int(info["entries"]), 1)
    res = {"case": case.name, "n_iter": int(e.num_iterations()), "K": args.K, "nodes": int(e.num_nodes()), "worlds": int(e.n_worlds()),
           "entries": int(info["entries"]), "kept": int(info["kept"]), "how": [int(h) for h in info["how"]],
           "how_share": [round(int(h) / n, 4) for h in info["how"]], "residual": int(info["residual"]),
           "pivots_total": int(info["pivots_total"]), "pivots_max": int(info["pivots_max"]),
           "pivots_per_residual": round(int(info["pivots_total"]) / max(int(info["residual"]), 1), 2)}
    for k in ("ms_classify_device", "ms_classify_wall", "ms_simplex_device", "ms_simplex_wall", "ms_compact_device", "ms_compact_wall", "ms_call"):
        res[k] = med(k)
    if args.sample:
        got = e.qmdp_policy_graph_get()
        f, t, _ = e.edges()
        children = Q.children_from_edges(e.num_nodes(), f, t)
        costs = e.qmdp_costs()
        # whole nodes in a seeded order until they hold --sample entries; the other nodes' lists emptied (the restatement goes node by node)
        first = np.concatenate([[0], np.cumsum([len(c) for c in children])]).astype(np.int64)
        nodes, have = [], 0
        for u in np.random.default_rng(0).permutation(len(children)).tolist():
            if have >= args.sample:
                break
            nodes.append(u)
            have += len(children[u])
        chosen = set(nodes)
        sub = [c if u in chosen else [] for u, c in enumerate(children)]
        idx = np.concatenate([np.arange(first[u], first[u + 1]) for u in sorted(chosen)])
        t0 = time.perf_counter()
        keep, how, _ = P.policy_graph(sub, costs)
        res["ms_restatement_python_single_thread"] = 1e3 * (time.perf_counter() - t0)
        res["restatement_entries"] = int(len(how))
        res["restatement_residual"] = int((how >= 3).sum())
        res["equal_to_restatement"] = bool(np.array_equal(how, got["how"][idx]) and np.array_equal(keep, got["keep"][idx]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
