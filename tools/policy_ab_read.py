"""One reading of the policy rows of a commit, for an A/B of two checkouts (profiles/policy_store_ab.json): one JSON line.
ROOT holds po_rrt_amd / tests / tools of the commit to read (built); run it once per reading in a process of its own, the two commits
alternated.  WHAT: shelves (the 12-shelf belief_space graph of bench.py: cfg4, 20 000 iterations, K = 256), map4 (cfg_map4 seed 1, K = 1),
mm (plan_mm_prm with 500 refine iterations on the two-goal benchmark map) or tamp (the TAMP planner's shortcut of the best paths of 64
tamp_queries).  The graph rows: extract_policy() and extract + refine_policy(500) right after a cost run, refine_policy(500 / 1500),
extract_policies n = 1 and n = 1024, refine_policies n = 1 and n = 1024.  Every row is the median of 7 timings after a warm-up.
usage: python tools/policy_ab_read.py ROOT WHAT"""
import json
import os
import sys
import time

ROOT, WHAT = os.path.abspath(sys.argv[1]), sys.argv[2]
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import cases  # noqa: E402
import po_rrt_amd  # noqa: E402

assert os.path.abspath(po_rrt_amd.__file__).startswith(ROOT), po_rrt_amd.__file__
REPS = 7


def med(v):
    return sorted(v)[len(v) // 2]


def timed(fn, before=None):
    out = []
    for _ in range(REPS):
        if before:
            before()
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return med(out)


def graph_rows(e):
    rows = {}
    n = len(e.expected_costs())
    starts = np.random.default_rng(1024).integers(0, n, size=1024).astype(np.uint64)
    starts[0] = 0
    e.extract_policy(); e.refine_policy(500); e.refine_policy(1500)          # warm-up: code objects, scratch, the raster
    rows["extract_policy_ms"] = timed(e.extract_policy, e.compute_expected_costs)
    rows["pair_extract_refine_500_ms"] = timed(lambda: (e.extract_policy(), e.refine_policy(500)), e.compute_expected_costs)
    e.extract_policy()
    rows["policy_nodes"] = int(len(e.extract_policy()[0][0]))
    for it in (500, 1500):
        rows["refine_policy_%d_ms" % it] = timed(lambda: e.refine_policy(it))
    e.extract_policies([0]); e.extract_policies(starts)
    rows["extract_policies_n1_ms"] = timed(lambda: e.extract_policies([0]))
    v = []
    for _ in range(REPS):
        e.extract_policies(starts)
        v.append(e.policies_info()["ms_wall"])
    rows["extract_policies_n1024_ms_wall"] = med(v)
    e.refine_policies(500)
    v = []
    for _ in range(REPS):
        e.refine_policies(500)
        v.append(e.refine_policies_info()["ms_wall"])
    rows["refine_policies_n1024_500_ms_wall"] = med(v)
    e.extract_policies([0])
    for it in (500, 1500):
        e.refine_policies(it)
        rows["refine_policies_n1_%d_ms" % it] = timed(lambda: e.refine_policies(it))
    single, batch = e.refine_policy(500), e.refine_policies(500)[0][0]
    rows["single_equals_batch_of_one_bits"] = bool(all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(single[0], batch[0])) and single[1] == batch[1])
    return rows


if WHAT == "shelves":
    case = cases.cfg4(20000, 20000)
    case.update(start=(0.0, -0.3))
    e = cases.configure(po_rrt_amd.Engine(), case)
    cases.grow(e, case, K=256)
    e.build_belief_graph([1.0 / 12] * 12)
    e.compute_expected_costs()
    rows = graph_rows(e)
elif WHAT == "map4":
    case = cases.cfg_map4(5000, 1)
    e = cases.configure(po_rrt_amd.Engine(), case)
    cases.grow(e, case, K=1)
    e.build_belief_graph([1.0 / 16] * 16)
    e.compute_expected_costs()
    rows = graph_rows(e)
elif WHAT == "mm":
    c = cases.cfg2(10)
    c.update(zones="map_benchmark_like_2_goals_zone_ids", visibility=0.5)
    case = cases.Case(c, seed=0)
    e = cases.configure(po_rrt_amd.Engine(), case)
    nodes = []

    def plan():
        (oid, par, leaf, xy), cost = e.plan_mm_prm(case.start, [0.5, 0.5], 0.1, 2.0, 1000, refine_iterations=500)
        nodes.append(int(len(oid)))

    def reseed():
        cases.configure(e, case)
        e.set_discrete_seed(0)
    reseed(); plan()
    rows = {"plan_mm_prm_refine_500_ms": timed(plan, reseed), "refined_nodes": nodes[-1], "refine_s_of_the_last": e.mm_plan_seconds()["refine_s"]}
elif WHAT == "tamp":
    cs = cases.tamp_queries(64)
    engs = [cases.configure(po_rrt_amd.Engine(), c) for c in cs]
    po_rrt_amd.Engine.grow_batch(engs, [c.start for c in cs], 0.1, 2.0, 2500, 128, n_iter_max=10000)
    paths = [p[0] for p in po_rrt_amd.Engine.best_paths(engs) if p is not None]
    e = engs[0]
    e.tamp_shortcut(paths)
    rows = {"tamp_shortcut_ms": timed(lambda: e.tamp_shortcut(paths)), "paths": len(paths), "states": int(sum(len(p) for p in paths))}
print(json.dumps({"root": os.path.basename(ROOT), "what": WHAT, "rows": rows}), flush=True)
