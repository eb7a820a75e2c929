"""porrt_bg_refine_policies (decomposition, shortcuts, recomposition and costs of many policies in one device call) beside what there
was before it -- the same policies refined one by one through porrt_refine_policy -- on the same graphs in the same process: the
12-shelf belief-space graph of bench.py (cfg4, 20 000 iterations, 4095 beliefs, uniform prior) and cfg_map4 seed 1 (the reference's
recorded problem, K = 1, 16 worlds).  Per graph: 1024 policies from fixed-seed starts (extract_policies), then for 500 and 1500
iterations ms_device / ms_wall of the batch call after a warm-up call, with option "refine_short_lds" off (one launch, 16 KiB of LDS
per wave) and on (the pieces of <= 256 nodes in a launch of their own with 4 KiB), the one-by-one baseline's wall time, and n = 1
(start 0 alone) beside extract_policy() + refine_policy().  Every batch result is checked against the one-by-one results, bit for bit.
Writes profiles/refine_policies.json (or --out).
usage: python tools/refine_policies_probe.py [--reps 5] [--out PATH]"""
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


def median_by(runs, key):
    return sorted(runs, key=lambda i: i[key])[len(runs) // 2]


def same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a[0], b[0])) and \
        np.float64(a[1]).view(np.uint64) == np.float64(b[1]).view(np.uint64)


def batch_runs(e, n_iter, reps):
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        got, status = e.refine_policies(n_iter)
        wall = 1e3 * (time.perf_counter() - t)
        info = e.refine_policies_info()
        info["ms_wall_python"] = wall
        runs.append(info)
    return got, status, runs


def probe(e, reps, n_many=1024, seed=1024):
    n = len(e.expected_costs())
    starts = np.random.default_rng(seed).integers(0, n, size=n_many).astype(np.uint64)
    starts[0] = 0
    xy = e.tree()[0]
    beliefs = e.belief_graph(lists=False)[0]
    B = np.uint64(len(beliefs))
    out = {"belief_nodes": n}
    for n_iter in (500, 1500):
        res = {}
        pols, ext_status = e.extract_policies(starts)
        arrays = [None if p is None else (xy[(p[0][0] // B).astype(np.int64)], p[0][1], p[0][0], (p[0][0] % B).astype(np.uint32)) for p in pols]
        e.refine_policies(n_iter)                               # warm-up: code objects, scratch, the raster
        for name, opt in (("batch", 0), ("batch_short_lds", 1)):
            e.set_option("refine_short_lds", opt)
            e.refine_policies(n_iter)
            got, status, runs = batch_runs(e, n_iter, reps)
            res[name] = {"median_by_wall": median_by(runs, "ms_wall"), "median_by_device": median_by(runs, "ms_device"), "runs": runs}
            res[name + "_result"] = got
        e.set_option("refine_short_lds", 0)
        assert all((a is None) == (b is None) and (a is None or same(a, b)) for a, b in zip(res["batch_result"], res["batch_short_lds_result"]))
        got = res.pop("batch_result")
        res.pop("batch_short_lds_result")
        one_by_one = []
        for rep in range(max(1, reps // 2)):                    # the baseline: what the parent commit offers for these policies
            t = time.perf_counter()
            single = [None if a is None else e.refine_policy_explicit(*a, beliefs, n_iter) for a in arrays]
            one_by_one.append(1e3 * (time.perf_counter() - t))
        assert all((a is None) == (b is None) and (a is None or same(a, b)) for a, b in zip(got, single)), "batch and one-by-one differ"
        res["one_by_one_ms_wall_python"] = sorted(one_by_one)[len(one_by_one) // 2]
        res["one_by_one_ms_wall_python_runs"] = one_by_one
        res["one_by_one_over_batch_wall"] = res["one_by_one_ms_wall_python"] / res["batch"]["median_by_wall"]["ms_wall_python"]
        # n = 1: start 0 alone, beside the single pair on the context
        e.extract_policies(starts[:1])
        e.refine_policies(n_iter)
        got1, _, runs1 = batch_runs(e, n_iter, reps)
        e.extract_policy()
        e.refine_policy(n_iter)
        single_runs = []
        for _ in range(reps):
            t = time.perf_counter()
            s1 = e.refine_policy(n_iter)
            wall = 1e3 * (time.perf_counter() - t)
            single_runs.append(dict(e.refine_info(), ms_wall_python=wall))
        assert same(got1[0], s1)
        res["n1_batch"] = {"median_by_wall": median_by(runs1, "ms_wall"), "runs": runs1}
        res["n1_refine_policy"] = {"median_by_wall": median_by(single_runs, "ms_wall_python"), "runs": single_runs}
        out["iterations_%d" % n_iter] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_policies.json"))
    a = ap.parse_args()
    out = {"what": "1024 policies refined in one device call (porrt_bg_refine_policies) beside one porrt_refine_policy call per policy"}
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
    for g in ("twelve_shelves", "map4_seed1"):
        for it in ("iterations_500", "iterations_1500"):
            r = out[g][it]
            b, s = r["batch"]["median_by_wall"], r["batch_short_lds"]["median_by_wall"]
            print("%s %s: policies %d ok %d pieces %d shortcut %d lengths %d | batch ms_device %.3f ms_wall %.3f | short-LDS ms_device %.3f ms_wall %.3f | "
                  "one by one %.1f ms (x%.1f) | n=1 batch %.3f ms, refine_policy %.3f ms" % (
                      g, it, b["policies"], b["ok"], b["pieces"], b["shortcut_pieces"], b["distinct_lengths"], b["ms_device"], b["ms_wall"],
                      s["ms_device"], s["ms_wall"], r["one_by_one_ms_wall_python"], r["one_by_one_over_batch_wall"],
                      r["n1_batch"]["median_by_wall"]["ms_wall"], r["n1_refine_policy"]["median_by_wall"]["ms_wall_python"]), flush=True)


if __name__ == "__main__":
    main()
