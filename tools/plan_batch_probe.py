"""porrt_plan_belief_space_batch (belief graph, expected costs, policy and refinement of many grown contexts in one device call) beside
what there was before it -- the single sequence, context by context -- on the reference's recorded problem (cases.cfg_map4(5000):
map_4, 16 worlds, uniform prior) in one process.  100 members with seeds 0 .. 99 are grown by one porrt_grow_batch at K = 256; for
1, 8, 30 and 100 of them (seeds 0 .. n - 1), after a warm-up of each form, three alternations of
    the single sequence over all members (build_belief_graph, compute_expected_costs, extract_policies([0]) [, refine_policies(500)])
    the one batch call, with 0 and with 500 refinement iterations,
timed with a host clock around calls that end in a synchronise, with the phase times of porrt_plan_batch_info.  At 30 members the
batch call is also timed with the kd ranks made on the device (option plan_batch_host_ranks = 0) beside the default.  The batch's
answers are compared with the singles', bit for bit, at every size timed.  Writes profiles/plan_batch.json (or --out).
At 30 members it is timed, too, under several values of option plan_batch_max_belief_nodes (--limits): the cut into passes.
usage: python tools/plan_batch_probe.py [--sizes 1,8,30,100] [--reps 3] [--limits a,b,..] [--out PATH]"""
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

REFINE = 500


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def singles(es, prior, n_refine, fresh_order=False):
    """the single sequence over all members: per member (status, cost bits, policy arrays), and the wall time of the whole loop.
    A context keeps the adjacency order of its graph, so a second build on the same graph does not pay for it again; fresh_order
    drops it before every build (setting option host_ranks does), as on a graph that has just been grown -- the host kd-tree stays."""
    t = time.perf_counter()
    out = []
    for e in es:
        if fresh_order:
            e.set_option("host_ranks", 1)
        e.build_belief_graph(prior)
        e.compute_expected_costs()
        off, status, cost, oid, par, leaf = e.extract_policies_raw([0])
        if n_refine:
            roff, rst, rc, xy, oid, par, leaf = e.refine_policies_raw(n_refine)
            out.append((int(status[0]), cost[0], int(rst[0]), rc[0], xy, oid, par, leaf))
        else:
            out.append((int(status[0]), cost[0], 1, 0.0, None, oid, par, leaf))
    return out, 1e3 * (time.perf_counter() - t)


def batch(es, prior, n_refine):
    t = time.perf_counter()
    raw = po_rrt_amd.Engine.plan_belief_space_batch_raw(es, prior, n_refine)
    wall = 1e3 * (time.perf_counter() - t)
    info = es[0].plan_batch_info()
    info["ms_wall_python"] = wall
    return raw, info


def assert_same(raw, want):
    off, status, cost, rstatus, rcost, xy, oid, par, leaf = raw
    for q, (st, c, rst, rc, w_xy, w_oid, w_par, w_leaf) in enumerate(want):
        a, b = int(off[q]), int(off[q + 1])
        assert status[q] == st and rstatus[q] == rst, "member %d: status" % q
        assert np.array_equal(u8(np.float64([cost[q], rcost[q]])), u8(np.float64([c, rc]))), "member %d: costs" % q
        assert np.array_equal(oid[a:b], w_oid) and np.array_equal(par[a:b], w_par) and np.array_equal(leaf[a:b], w_leaf), "member %d: policy" % q
        if w_xy is not None:
            assert np.array_equal(u8(xy[a:b]), u8(w_xy)), "member %d: states" % q


def spread(v):
    return {"runs": v, "median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,30,100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--limits", default="%d,%d,%d,%d,%d,%d" % (1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 27),
                    help="option plan_batch_max_belief_nodes values timed at 30 members")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_batch.json"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    cs = [cases.cfg_map4(a.iters, seed=s) for s in range(max(sizes))]
    es = [cases.configure(po_rrt_amd.Engine(), c) for c in cs]
    t = time.perf_counter()
    po_rrt_amd.Engine.grow_batch(es, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, cs[0].n_iter_min, 256, cases.PTO, n_iter_max=cs[0].n_iter_max)
    prior = [1.0 / 16] * 16
    out = {"what": "plan_belief_space for n grown contexts of cfg_map4(%d), K = 256: the single sequence context by context beside one "
                   "porrt_plan_belief_space_batch call; milliseconds" % a.iters,
           "grow_batch_ms": 1e3 * (time.perf_counter() - t), "nodes": [e.num_nodes() for e in es], "sizes": {}}
    for n in sizes:
        sub = es[:n]
        res = {}
        for n_refine in (0, REFINE):
            want, _ = singles(sub, prior, n_refine)              # warm-up of each form, and the comparison
            raw, _ = batch(sub, prior, n_refine)
            assert_same(raw, want)
            one, fresh, many, infos = [], [], [], []
            for _ in range(a.reps):
                want, ms = singles(sub, prior, n_refine)
                one.append(ms)
                fresh.append(singles(sub, prior, n_refine, True)[1])
                raw, info = batch(sub, prior, n_refine)
                many.append(info["ms_wall_python"])
                infos.append(info)
                assert_same(raw, want)
            res["refine_%d" % n_refine] = {"one_by_one_ms": spread(one), "one_by_one_fresh_order_ms": spread(fresh), "batch_ms": spread(many), "batch_info": infos,
                                           "slowest_batch_below_fastest_one_by_one": max(many) < min(one)}
        if n == 30:
            ranks = {"host": [], "device": []}
            want0 = singles(sub, prior, 0)[0]
            for name, opt in (("host", 1), ("device", 0)):       # warm-up of each
                sub[0].set_option("plan_batch_host_ranks", opt)
                batch(sub, prior, 0)
            for _ in range(a.reps):
                for name, opt in (("host", 1), ("device", 0)):
                    sub[0].set_option("plan_batch_host_ranks", opt)
                    raw, info = batch(sub, prior, 0)
                    assert_same(raw, want0)
                    ranks[name].append({"ms_wall_python": info["ms_wall_python"], "ms_edge_order": info["ms_edge_order"]})
            sub[0].set_option("plan_batch_host_ranks", 1)
            res["ranks"] = ranks
            # the cut into passes: fewer members per union sweep fewer rows that have already settled (a union is swept until its
            # slowest member's costs stand), more passes pay the fixed costs of a pass more often
            limits = [int(x) for x in a.limits.split(",")]
            default = sub[0].get_option("plan_batch_max_belief_nodes")
            cuts = {str(lim): [] for lim in limits}
            for rep in range(a.reps + 1):                        # (the first round warms up)
                for lim in limits:
                    sub[0].set_option("plan_batch_max_belief_nodes", lim)
                    raw, info = batch(sub, prior, 0)
                    assert_same(raw, want0)
                    if rep:
                        cuts[str(lim)].append({k: info[k] for k in ("ms_wall_python", "passes", "ms_costs", "ms_belief_graph", "ms_edge_order", "ms_join")})
            sub[0].set_option("plan_batch_max_belief_nodes", default)
            res["pass_limits"] = cuts
        out["sizes"][str(n)] = res
        for k in ("refine_0", "refine_%d" % REFINE):
            r = res[k]
            i = sorted(r["batch_info"], key=lambda x: x["ms_wall"])[len(r["batch_info"]) // 2]
            print("n = %3d %s: one by one %.2f ms (%.2f .. %.2f), with the edge order rebuilt %.2f | batch %.2f ms (%.2f .. %.2f) | join %.2f order %.2f belief graph %.2f costs %.2f "
                  "policies %.2f refine %.2f device %.2f | passes %d belief nodes %d edges %d" % (
                      n, k, r["one_by_one_ms"]["median"], r["one_by_one_ms"]["min"], r["one_by_one_ms"]["max"], r["one_by_one_fresh_order_ms"]["median"], r["batch_ms"]["median"],
                      r["batch_ms"]["min"], r["batch_ms"]["max"], i["ms_join"], i["ms_edge_order"], i["ms_belief_graph"], i["ms_costs"],
                      i["ms_policies"], i["ms_refine"], i["ms_device"], i["passes"], i["belief_nodes"], i["belief_edges"]), flush=True)
        if "ranks" in res:
            for name in ("host", "device"):
                print("n = %3d ranks from the %s: %s" % (n, name, ", ".join("wall %.2f order %.2f" % (x["ms_wall_python"], x["ms_edge_order"]) for x in res["ranks"][name])), flush=True)
            for lim, runs in res["pass_limits"].items():
                print("n = %3d plan_batch_max_belief_nodes %s: %d passes, %s" % (n, lim, runs[0]["passes"], ", ".join("wall %.2f costs %.2f" % (x["ms_wall_python"], x["ms_costs"]) for x in runs)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
