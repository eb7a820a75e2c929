"""porrt_prm_plan_paths against porrt_prm_plan_path one query at a time, on the bench's roadmap (map_benchmark_like, start (0, -0.8),
max_step 0.1, search_radius 2.0, 200 000 samples, sampler seed 3): 1024 start/goal pairs drawn from a fixed seed inside the map bounds
as one batch (the XCD placement of the sweep rows on and off, alternated), the same pairs one after the other in the same process, and
1024 starts to one goal (one row).  Also the bytes a sweep must move (roofline block).  Writes profiles/prm_paths.json (or --out).
usage: python tools/prm_paths_probe.py [--reps 3] [--singles 1024] [--out PATH]"""
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

HBM_BPS = 6.29e12          # measured copy bandwidth of the MI355X's HBM (float4 copy)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def batch(e, S, G, xcd):
    e.set_option("prm_xcd_rows", xcd)
    t = time.perf_counter()
    paths = e.prm_plan_paths(S, G)
    wall = time.perf_counter() - t
    info = e.prm_paths_info()
    info["ms_wall_python"] = 1e3 * wall
    info["states"] = int(sum(len(p) for p in paths))
    return paths, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--singles", type=int, default=1024, help="how many of the pairs also go through porrt_prm_plan_path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prm_paths.json"))
    a = ap.parse_args()
    n = 200000
    e = po_rrt_amd.Engine()
    e.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    e.set_sampler((-1.0, -1.0), (1.0, 1.0), 3)
    e.grow_prm((0.0, -0.8), 0.1, 2.0, n)
    E = len(e.edges()[0])                                        # forward edges (and the adjacency order, made once)
    rng = np.random.default_rng(1024)
    S, G = rng.uniform(-1.0, 1.0, (a.pairs, 2)), rng.uniform(-1.0, 1.0, (a.pairs, 2))
    out = {"what": "PRM::plan_path for %d start/goal pairs on the bench's roadmap (%d samples, %d forward edges)" % (a.pairs, n, E),
           "pairs_seed": 1024, "N": n + 1, "forward_edges": E}
    batch(e, S[:8], G[:8], 1)                                    # warm-up: weights, code objects, buffers
    batch(e, S, G, 1)
    runs = {"xcd_rows_on": [], "xcd_rows_off": []}
    paths = None
    for rep in range(a.reps):
        for xcd in (1, 0) if rep % 2 == 0 else (0, 1):
            p, info = batch(e, S, G, xcd)
            runs["xcd_rows_on" if xcd else "xcd_rows_off"].append(info)
            if paths is None:
                paths = p
            else:
                assert all(same(x, y) for x, y in zip(paths, p)), "a batch differs from the first"
    e.set_option("prm_xcd_rows", 1)
    med = {k: sorted(v, key=lambda i: i["ms_wall"])[len(v) // 2] for k, v in runs.items()}
    out["batch"] = {"median_by_wall": med, "runs": runs}
    # the same pairs one after the other
    k = min(a.singles, a.pairs)
    if k:
        t = time.perf_counter()
        singles = [e.prm_plan_path(S[i], G[i]) for i in range(k)]
        dt = time.perf_counter() - t
        bad = [i for i in range(k) if not same(singles[i], paths[i])]
        best = min(med.values(), key=lambda i: i["ms_wall"])
        out["one_by_one"] = {"queries": k, "ms_wall_total": 1e3 * dt, "ms_per_query": 1e3 * dt / k, "mismatches": len(bad),
                             "ms_wall_total_scaled_to_pairs": 1e3 * dt * a.pairs / k,
                             "speedup_wall": (1e3 * dt * a.pairs / k) / best["ms_wall"]}
    # many starts, one goal: one row
    G1 = np.tile([0.9, 0.0], (a.pairs, 1))
    batch(e, S, G1, 1)
    one = [batch(e, S, G1, 1)[1] for _ in range(max(1, a.reps))]
    out["one_goal"] = sorted(one, key=lambda i: i["ms_wall"])[len(one) // 2]
    # roofline: what a sweep must move per row.  A node evaluated reads its dirty byte, its cost, two offsets and, per parent, the
    # id (4 B), the weight (8 B) and the parent's cost (8 B, a gather); a whole-row sweep in which every node is evaluated moves
    # full_row_sweep_bytes, a sweep that finds nothing still reads N dirty bytes per active row.
    N, E2 = n + 1, 2 * E
    full = N * (1 + 8 + 16) + E2 * (4 + 8 + 8)
    r = med["xcd_rows_on"]
    out["roofline"] = {"full_row_sweep_bytes": full, "idle_row_sweep_bytes": N,
                       "one_full_sweep_of_every_row_ms_at_hbm": 1e3 * r["rows"] * full / HBM_BPS,
                       "dirty_scans_upper_bound_bytes": r["sweeps"] * min(r["rows"], 256) * N,
                       "measured_ms_device": r["ms_device"],
                       "full_row_sweeps_equivalent": r["ms_device"] * 1e-3 * HBM_BPS / full,
                       "note": "the gathers of parents' costs hit L2 when a row's costs stay on one XCD; HBM rate: 6.29 TB/s copy"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k2: out[k2] for k2 in ("batch", "one_by_one", "one_goal", "roofline") if k2 in out and k2 != "batch"}, indent=1))
    print(json.dumps(med, indent=1), flush=True)


if __name__ == "__main__":
    main()
