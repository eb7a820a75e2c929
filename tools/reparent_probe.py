"""The Reparent refinement on the device (porrt_bg_reparent_policies, porrt_reparent.hpp) measured: the root policy of cfg_map4 (the
reference's recorded problem, seeds 0-4) and of the 12-shelf belief-space graph of bench.py (cfg4, 20 000 iterations, uniform prior) at
Reparent(0.3), then 1024 policies from fixed-seed starts on map_4 seed 1 and on the 12-shelf graph.  Per case: trees, tree nodes, the
largest tree, valid-neighbour pairs, pops, reparents, milliseconds per stage (HIP events, the median call of --reps after a warm-up call)
and wall, statuses, expected cost before -> after, and beside it the same policies under PartialShortCut(500).  For context only: the
wall time of the Python restatement (tests/reparent_ref.py) on the first map_4 root policy there is -- it is Python and no baseline.
Writes profiles/reparent.json (or --out) after every case.
usage: python tools/reparent_probe.py [--reps 5] [--out PATH] [--many 1024] [--skip-restatement]"""
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

RADIUS = 0.3


def measure(e, starts, reps):
    pols, ext_status = e.extract_policies(starts)
    before = [None if p is None else p[1] for p in pols]
    e.reparent_policies(RADIUS)                                 # warm-up: code objects, scratch, the raster
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        got, status = e.reparent_policies(RADIUS)
        wall = 1e3 * (time.perf_counter() - t)
        runs.append(dict(e.reparent_policies_info(), ms_wall_python=wall))
    med = sorted(runs, key=lambda r: r["ms_wall"])[len(runs) // 2]
    e.refine_policies(500)
    t = time.perf_counter()
    short, sstatus = e.refine_policies(500)
    short_wall = 1e3 * (time.perf_counter() - t)
    ok = [q for q in range(len(pols)) if got[q] is not None and short[q] is not None]
    out = {"policies": len(starts), "extracted": int((np.asarray(ext_status) == 0).sum()),
           "status_counts": {str(s): int((np.asarray(status) == s).sum()) for s in sorted(set(np.asarray(status).tolist()))},
           "median_by_wall": med, "runs": runs,
           "nodes_in": int(sum(len(pols[q][0][0]) for q in ok)), "nodes_reparent": int(sum(len(got[q][0][0]) for q in ok)),
           "partial_shortcut_500": dict(e.refine_policies_info(), ms_wall_python=short_wall)}
    if ok:
        pick = ok[:8]
        out["expected_cost"] = [{"start": int(starts[q]), "before": before[q], "reparent": got[q][1], "partial_shortcut_500": short[q][1]} for q in pick]
        out["expected_cost_mean"] = {"before": float(np.mean([before[q] for q in ok])), "reparent": float(np.mean([got[q][1] for q in ok])),
                                     "partial_shortcut_500": float(np.mean([short[q][1] for q in ok]))}
    return out


def show(name, r):
    m = r["median_by_wall"]
    print("%s: policies %d status %s | pieces %d tree nodes %d largest %d pairs %d pops %d reparents %d rounds %d | ms tube %.3f neighbours %.3f pop %.3f "
          "recompose %.3f wall %.3f | cost %s | PartialShortCut(500) ms_wall %.3f" % (
              name, r["policies"], r["status_counts"], m["pieces"], m["tree_nodes"], m["max_tree"], m["pairs"], m["pops"], m["reparents"], m["rounds"],
              m["ms_tube"], m["ms_neighbours"], m["ms_pop"], m["ms_recompose"], m["ms_wall"], r.get("expected_cost_mean"), r["partial_shortcut_500"]["ms_wall"]), flush=True)


def grown(case, K, prior):
    e = cases.configure(po_rrt_amd.Engine(), case)
    cases.grow(e, case, K=K)
    e.build_belief_graph(prior)
    e.compute_expected_costs()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--many", type=int, default=1024)
    ap.add_argument("--skip-restatement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reparent.json"))
    a = ap.parse_args()
    out = {"what": "refine_solution(Reparent(0.3)) on the device (porrt_bg_reparent_policies); option reparent_max_tree_nodes at its default", "radius": RADIUS}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    def many_starts(e):
        n = len(e.expected_costs())
        starts = np.random.default_rng(1024).integers(0, n, size=a.many).astype(np.uint64)
        starts[0] = 0
        return starts

    restated = False
    for seed in range(5):
        e = grown(cases.cfg_map4(5000, seed), 1, [1.0 / 16] * 16)
        name = "map4_seed%d_root" % seed
        out[name] = measure(e, [0], a.reps)
        show(name, out[name])
        save()
        if "0" in out[name]["status_counts"] and not restated and not a.skip_restatement:      # (the walk from node 0 does not end on every seed)
            restated = True
            import reparent_ref as rr
            from oracle import orc
            o = cases.configure(orc.Oracle(), cases.cfg_map4(5000, seed))
            beliefs, _, (coff, cid), _ = e.belief_graph()
            G = rr.Graph.implicit(e.tree()[0], beliefs, coff, cid)
            (oid, par, leaf), _ = e.extract_policy()
            t = time.perf_counter()
            status, res = rr.refine(o, G, oid, par, RADIUS, queue="heap")
            out["restatement_python"] = {"case": name, "s_wall": time.perf_counter() - t, "status": status, "note": "context only: Python on the CPU, not a baseline"}
            print("restatement of %s (Python, context only): %.1f s, status %d" % (name, out["restatement_python"]["s_wall"], status), flush=True)
            save()
        if seed == 1:
            out["map4_seed1_many"] = measure(e, many_starts(e), max(1, a.reps // 2))
            show("map4_seed1_many", out["map4_seed1_many"])
            save()
        e.close()
    case = cases.cfg4(20000, 20000)
    case.update(start=(0.0, -0.3))
    e = grown(case, 256, [1.0 / 12] * 12)
    out["twelve_shelves_root"] = measure(e, [0], a.reps)
    show("twelve_shelves_root", out["twelve_shelves_root"])
    save()
    out["twelve_shelves_many"] = measure(e, many_starts(e), max(1, a.reps // 2))
    show("twelve_shelves_many", out["twelve_shelves_many"])
    save()
    e.close()


if __name__ == "__main__":
    main()
