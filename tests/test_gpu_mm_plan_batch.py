"""porrt_mm_plan_batch: MapShelfDomainTampPRM::plan (+ PartialShortCut) for many (start, prior, sampler seed, discrete seed) on one map
in one device call, against fresh engines one by one -- bit for bit: statuses, cost bits, policies, refined policies, whole cost
vectors, per-plan counts -- and, for two plans, against the restatement (tests/mm_plan_ref.py, tests/refine_ref.py) on the oracle's
growth."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import mm_clamped_inputs as mc
import mm_plan_ref as ref
import refine_ref
from oracle import orc

pytestmark = pytest.mark.gpu

BITS = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bench_case(zones, seed):
    c = cases.cfg2(10)
    c.update(zones=zones, visibility=0.5)
    return cases.Case(c, seed=seed)


def fresh(case, discrete_seed, configure=cases.configure):
    import po_rrt_amd
    e = configure(po_rrt_amd.Engine(), case)
    e.set_discrete_seed(discrete_seed)
    return e


def single(e, start, prior, max_step, radius, n_per_belief, refine=()):
    """one plan on its own engine: the stages of porrt_mm_plan one by one (a root without finite cost ends porrt_mm_plan itself with an
    error, after the costs), the status from the batched walk of one start, the refinements of the root's policy"""
    g = e.grow_mm_prm(start, prior, max_step, radius, n_per_belief)
    e.mm_build_belief_graph()
    dist = e.mm_expected_costs()
    got, status = e.mm_extract_policies([0])
    out = dict(status=int(status[0]), cost=dist[0], dist=dist, grow=g, policy=None, refined={})
    bg = e.mm_belief_graph()
    out["counts"] = dict(modes=len(g["modes"]), transitions=len(g["transitions"]), beliefs=g["n_beliefs"], nodes=len(dist),
                         forward_edges=sum(len(m["edges"][0]) for m in g["modes"]), belief_edges=len(bg["children"][1]), finals=len(bg["finals"]))
    if out["status"] == 0:
        out["policy"] = e.mm_extract_policy()[0]                        # (ids, parents, leaf flags, states)
        for n in refine:
            out["refined"][n] = e.mm_refine_policy(n)                   # ((states, ids, parents, leaf flags), cost)
    return out


def assert_plan(b, s, refine_iterations, who=""):
    """a batch's plan (Engine.plan_mm_prm_batch's dict) against the single plan"""
    assert b["status"] == s["status"], who
    assert BITS([b["cost"]])[0] == BITS([s["cost"]])[0], who
    oid, par, leaf, xy = b["policy"]
    if s["status"] != 0:
        assert len(oid) == 0 and b["refine_status"] == 1, who
        return
    if refine_iterations == 0:
        oid2, par2, leaf2, xy2 = s["policy"]
        assert b["refine_status"] == 1 and b["refined_cost"] == 0.0, who
    else:
        (xy2, oid2, par2, leaf2), cost2 = s["refined"][refine_iterations]
        assert b["refine_status"] == 0 and BITS([b["refined_cost"]])[0] == BITS([cost2])[0], who
    assert np.array_equal(oid, oid2) and np.array_equal(par, par2) and np.array_equal(leaf, leaf2), who
    assert np.array_equal(BITS(xy), BITS(xy2)), who


def assert_counts(e, p, s):
    got = e.mm_plan_batch_plan(p)
    for k, v in s["counts"].items():
        assert got[k] == v, (p, k, got[k], v)


TWO_GOALS = ("map_benchmark_like_2_goals_zone_ids", [0.5, 0.5], 1000, 0.1, 2.0)
SEEDS = ((0, 0), (1, 1), (0, 1), (2, 0))                               # (sampler, discrete)


@functools.lru_cache(maxsize=None)
def two_goal_singles():
    zones, prior, n, step, radius = TWO_GOALS
    out = []
    for cs, ds in SEEDS:
        case = bench_case(zones, cs)
        out.append(single(fresh(case, ds), case.start, prior, step, radius, n, refine=(200,)))
    return out


def two_goal_batch(refine_iterations, max_nodes=None):
    zones, prior, n, step, radius = TWO_GOALS
    case = bench_case(zones, 77)                                        # the engine's own seeds are not the plans'
    e = fresh(case, 5)
    if max_nodes is not None:
        e.set_option("mm_plan_batch_max_nodes", max_nodes)
    plans = e.plan_mm_prm_batch([case.start] * len(SEEDS), [prior] * len(SEEDS), step, radius, n, refine_iterations,
                                sampler_seeds=[s[0] for s in SEEDS], discrete_seeds=[s[1] for s in SEEDS])
    return e, plans


def test_batch_equals_one_by_one_and_the_restatement():
    zones, prior, n, step, radius = TWO_GOALS
    singles = two_goal_singles()
    statuses = [s["status"] for s in singles]
    assert statuses[0] == 0 and statuses[1] == 1 and np.isfinite(singles[0]["cost"]) and not np.isfinite(singles[1]["cost"])
    for it in (0, 200):
        e, plans = two_goal_batch(it)
        assert [p["status"] for p in plans] == statuses and 0 in statuses and 1 in statuses
        for p, (b, s) in enumerate(zip(plans, singles)):
            assert_plan(b, s, it, "plan %d, %d iterations" % (p, it))
            assert_counts(e, p, s)
            assert np.array_equal(BITS(e.mm_plan_batch_expected_costs(p)), BITS(s["dist"])), p
        info = e.mm_plan_batch_info()
        assert info["plans"] == 4 and info["passes"] == 1 and info["policies_ok"] == statuses.count(0)
        assert info["nodes"] == sum(s["counts"]["nodes"] for s in singles) and info["modes"] == sum(s["counts"]["modes"] for s in singles)
        assert info["explicit_points"] * 4 < info["nodes"]              # most nodes are references into the plans' prefixes
        # the restatement on the oracle's growth, plans 0 and 1
        if it == 200:
            for p in (0, 1):
                case = bench_case(zones, SEEDS[p][0])
                o = cases.configure(orc.Oracle(), case)
                o.set_discrete_seed(SEEDS[p][1])
                _, bg, dist = ref.plan(o, case.start, prior, step, radius, n)
                assert np.array_equal(BITS(e.mm_plan_batch_expected_costs(p)), BITS(dist))
                if p == 1:
                    assert not np.isfinite(dist[0]) and plans[p]["status"] == 1
                    continue
                oid, par, leaf = ref.extract_policy(bg, dist)
                idx = oid.astype(np.int64)
                (x2, oid2, par2, leaf2), cost2 = refine_ref.refine(o, bg["xy"][idx], par, oid, bg["belief_vec"][idx], bg["beliefs"], 200)
                boid, bpar, bleaf, bxy = plans[p]["policy"]
                assert np.array_equal(boid, oid2) and np.array_equal(bpar, par2) and np.array_equal(bleaf, leaf2)
                assert np.array_equal(BITS(bxy), BITS(x2)) and BITS([plans[p]["refined_cost"]])[0] == BITS([cost2])[0]


def test_different_starts_and_priors_in_one_call():
    """Three priors and two starts in one call.  The prior [0.5, 0.5, 0, 0] cannot be planned from, alone or in a batch: the growth draws
    an observation of a zone without mass, whose "object there" mode has a belief that is no reachable belief state (where the
    reference panics, map_shelves_tamp_prm.rs:400) -- a single plan ends with that error after its growth, and a batch that holds
    such a plan is refused before any launch, the plan named.  The prior with fewer reachable beliefs that CAN be planned from is a
    certain one, [1, 0, 0, 0]: one belief, a tenth of the sample budget, a mode tree of one mode, no goal state, status 1."""
    zones, n, step, radius = "map_benchmark_like_4_free_zone_ids", 2000, 0.1, 2.0
    priors = [[0.25] * 4, [0.4, 0.3, 0.2, 0.1], [0.5, 0.5, 0.0, 0.0]]
    starts = [(0.0, -1.0), (0.0, -0.8), (0.0, -1.0)]
    seeds = ((0, 0), (1, 1), (2, 2))
    e = fresh(bench_case(zones, 9), 9)
    lone = fresh(bench_case(zones, 2), 2)
    lone.grow_mm_prm(starts[2], priors[2], step, radius, n)
    with pytest.raises(RuntimeError, match="not a reachable belief state"):
        lone.mm_build_belief_graph()
    with pytest.raises(RuntimeError, match="plan 2: .*not a reachable belief state"):
        e.plan_mm_prm_batch(starts, priors, step, radius, n, 200, sampler_seeds=[s[0] for s in seeds], discrete_seeds=[s[1] for s in seeds])
    with pytest.raises(RuntimeError):
        e.mm_plan_batch_info()
    priors[2] = [1.0, 0.0, 0.0, 0.0]
    singles = []
    for (cs, ds), st, pr in zip(seeds, starts, priors):
        singles.append(single(fresh(bench_case(zones, cs), ds), st, pr, step, radius, n, refine=(200,)))
    assert len({s["counts"]["modes"] for s in singles}) > 1              # the last prior reaches fewer beliefs: another budget, another mode tree
    assert singles[2]["counts"]["beliefs"] < singles[0]["counts"]["beliefs"] and singles[2]["counts"]["nodes"] < singles[0]["counts"]["nodes"]
    assert singles[0]["status"] == 0 and singles[2]["status"] == 1
    plans = e.plan_mm_prm_batch(starts, priors, step, radius, n, 200, sampler_seeds=[s[0] for s in seeds], discrete_seeds=[s[1] for s in seeds])
    for p, (b, s) in enumerate(zip(plans, singles)):
        assert_plan(b, s, 200, "plan %d" % p)
        assert_counts(e, p, s)
        assert np.array_equal(BITS(e.mm_plan_batch_expected_costs(p)), BITS(s["dist"])), p


def test_the_cut_does_not_matter():
    singles = two_goal_singles()
    nodes = [s["counts"]["nodes"] for s in singles]
    two = max(nodes[0] + nodes[1], nodes[2] + nodes[3])
    assert two < nodes[0] + nodes[1] + min(nodes[2:]) and two < (1 << 22)
    for max_nodes, passes in ((1, 4), (two, 2), (None, 1)):
        e, plans = two_goal_batch(200, max_nodes)
        assert e.mm_plan_batch_info()["passes"] == passes
        for p, (b, s) in enumerate(zip(plans, singles)):
            assert_plan(b, s, 200, "plan %d, %d passes" % (p, passes))
            assert_counts(e, p, s)
            per = 4 // passes
            assert e.mm_plan_batch_plan(p)["pass"] == p // per
            if p >= 4 - per:                                            # the last pass's costs are still on the device
                assert np.array_equal(BITS(e.mm_plan_batch_expected_costs(p)), BITS(s["dist"]))
            else:
                with pytest.raises(RuntimeError):
                    e.mm_plan_batch_expected_costs(p)


def test_many_small_modes_and_modes_of_explicit_points_only():
    case = cases.cfg4(1500, 1500)
    prior, n, step, radius = [1.0 / 12] * 12, 20, 0.05, 5.0
    singles = [single(fresh(case, ds), case.start, prior, step, radius, n) for ds in (0, 1)]
    for s in singles:
        sizes = [len(m["xy"]) for m in s["grow"]["modes"]]
        assert len(sizes) > 1000 and min(sizes) < 190                   # a mode that was never drawn holds no random point (they come 190 at a time)
        assert s["status"] == 1 and not np.isfinite(s["cost"])
    e = fresh(case, 3)
    plans = e.plan_mm_prm_batch([case.start] * 2, [prior] * 2, step, radius, n, 0, sampler_seeds=[case.seed] * 2, discrete_seeds=[0, 1])
    for p, (b, s) in enumerate(zip(plans, singles)):
        assert b["status"] == 1 and len(b["policy"][0]) == 0
        assert_counts(e, p, s)
        assert np.array_equal(BITS(e.mm_plan_batch_expected_costs(p)), BITS(s["dist"])), p


@pytest.mark.parametrize("name", ["A", "B"])
def test_clamped_samples(name):
    inp = mc.INPUTS[name]()
    args = (inp.start, inp.prior, inp.max_step, inp.search_radius, inp.n_per_belief)
    singles = [single(fresh(inp, ds, mc.configure), *args, refine=(1, 200)) for ds in (0, 1)]
    dup = [max(mc.place_counts(m["xy"]).max() for m in s["grow"]["modes"]) for s in singles]
    assert max(dup) > 1                                                  # the window clamps observation samples onto one another
    e = fresh(inp, 7, mc.configure)
    for it in (0, 1, 200):
        plans = e.plan_mm_prm_batch([inp.start] * 2, [inp.prior] * 2, inp.max_step, inp.search_radius, inp.n_per_belief, it,
                                    sampler_seeds=[inp.seed] * 2, discrete_seeds=[0, 1])
        for p, (b, s) in enumerate(zip(plans, singles)):
            assert_plan(b, s, it, "input %s, plan %d, %d iterations" % (name, p, it))
            assert_counts(e, p, s)
            assert np.array_equal(BITS(e.mm_plan_batch_expected_costs(p)), BITS(s["dist"])), p


def grow_bits(g):
    return [m["xy"].tobytes() for m in g["modes"]] + [t["pairs"].tobytes() for t in g["transitions"]] + [len(g["modes"]), len(g["transitions"])]


def test_the_context_is_left_alone():
    zones, prior, n, step, radius = TWO_GOALS
    case = bench_case(zones, 0)
    e, twin = fresh(case, 0), fresh(case, 0)
    first = e.plan_mm_prm(case.start, prior, step, radius, n)
    twin.plan_mm_prm(case.start, prior, step, radius, n)
    dist = e.mm_expected_costs(compute=False)
    # a batch with NULL seeds: every plan clones the engine's CURRENT samplers (the continuous one never moved, the discrete one did)
    plans = e.plan_mm_prm_batch([case.start] * 2, [prior] * 2, step, radius, n, 0)
    assert plans[0]["status"] == plans[1]["status"] and np.array_equal(plans[0]["policy"][0], plans[1]["policy"][0])
    again = e.mm_extract_policy()
    for a, b in zip(first[0], again[0]):
        assert np.array_equal(a, b)
    assert BITS([first[1]])[0] == BITS([again[1]])[0]
    assert np.array_equal(BITS(e.mm_expected_costs(compute=False)), BITS(dist))
    # the discrete sampler was not advanced: the next single growth is the twin's, which ran no batch
    assert grow_bits(e.grow_mm_prm(case.start, prior, step, radius, n)) == grow_bits(twin.grow_mm_prm(case.start, prior, step, radius, n))
    # a batch of one with NULL seeds is the single plan from the same samplers
    s = two_goal_singles()[0]
    x = fresh(case, 0)
    b = x.plan_mm_prm_batch([case.start], [prior], step, radius, n, 200)[0]
    assert_plan(b, s, 200)
    assert np.array_equal(BITS(x.mm_plan_batch_expected_costs(0)), BITS(s["dist"]))
    assert_counts(x, 0, s)


def test_refusals():
    import po_rrt_amd
    zones, prior, n, step, radius = TWO_GOALS
    case = bench_case(zones, 0)
    e = fresh(case, 0)
    for getter in (e.mm_plan_batch_info, lambda: e.mm_plan_batch_plan(0), lambda: e.mm_plan_batch_expected_costs(0)):
        with pytest.raises(RuntimeError):
            getter()
    off = np.zeros(2, dtype=np.uint64)
    assert e._l.porrt_mm_plan_batch_get_policies(e._c, off.ctypes.data_as(C.c_void_p), None, None, None, None, 0) < 0
    with pytest.raises(RuntimeError):
        e.plan_mm_prm_batch(np.zeros((0, 2)), np.zeros((0, 2)), step, radius, n)                       # n_plans = 0
    with pytest.raises(RuntimeError):
        e.plan_mm_prm_batch(np.tile(case.start, (65537, 1)), np.tile(prior, (65537, 1)), step, radius, n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st, pr = np.array([case.start], dtype=np.float64), np.array([prior], dtype=np.float64)
    o, s8, c = np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(1)

    def raw(starts, priors, pol_off=o, status=s8, cost=c):
        q = lambda a: None if a is None else p(a)
        return e._l.porrt_mm_plan_batch(e._c, 1, q(starts), q(priors), None, None, 2, step, radius, n, 0, q(pol_off), q(status), q(cost), None, None, None, None,
                                        None, None, 0)
    assert raw(None, pr) == -1 and raw(st, None) == -1 and raw(st, pr, pol_off=None) == -1 and raw(st, pr, status=None) == -1 and raw(st, pr, cost=None) == -1
    with pytest.raises(RuntimeError, match="plan 1"):
        e.plan_mm_prm_batch([case.start] * 2, [prior, [0.5, 0.4]], step, radius, n)                   # a prior summing to 0.9
    with pytest.raises(RuntimeError):
        e.plan_mm_prm_batch([case.start], [[0.5, 0.25, 0.25]], step, radius, n)                       # not the context's n_worlds
    with pytest.raises(RuntimeError):
        e.mm_plan_batch_info()                                                                         # none of these left answers
    nz = cases.configure(po_rrt_amd.Engine(), cases.cfg2(10))                                          # no zones
    with pytest.raises(RuntimeError):
        nz.plan_mm_prm_batch([case.start], [[1.0]], step, radius, n)
    door = cases.configure(po_rrt_amd.Engine(), cases.cfg_door(10, 10))
    with pytest.raises(RuntimeError):
        door.plan_mm_prm_batch([case.start], [[0.25] * 4], step, radius, n)
    # and after the refusals the engine still plans
    assert e.plan_mm_prm_batch([case.start], [prior], step, radius, n, sampler_seeds=[0], discrete_seeds=[0])[0]["status"] == 0
