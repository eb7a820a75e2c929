"""GPU parity of the policies from many belief nodes in one device call (porrt_bg_extract_policies, porrt_mm_extract_policies,
porrt_extract_policies; porrt_policy.hpp) against tests/policies_ref.py, the restatement of extract_policy
(belief_graph.rs:184-267) from any start.  Everything is compared exactly: ids, parents, leaf flags, statuses, cost bits."""
import time

import numpy as np
import pytest

import cases
import kat_graphs
import policies_ref as ref
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_answers(got, status, want, what=""):
    """got: the list an extract_policies call returns; want: policies_ref.extract_policies of the same starts"""
    assert len(got) == len(want) == len(status)
    for q, (st, pol, cost) in enumerate(want):
        assert status[q] == st, "%s query %d: status %d, the reference says %d" % (what, q, status[q], st)
        if st != ref.OK:
            assert got[q] is None
            continue
        (oid, par, leaf), c = got[q][0][:3], got[q][1]
        assert np.array_equal(oid, pol[0]) and np.array_equal(par, pol[1]) and np.array_equal(leaf, pol[2]), "%s query %d" % (what, q)
        assert bits([c])[0] == bits([cost])[0]
        assert oid.dtype == np.uint64 and par.dtype == np.int64 and par[0] == -1 and leaf[0] == 0


def context_ref(e):
    beliefs, types, (coff, cid), _ = e.belief_graph()
    d = e.expected_costs()
    return ref.context_graph(e.tree()[0], beliefs, coff, cid), d, types


# ---------------------------------------------------------------------------------------------- explicit graphs

@pytest.mark.parametrize("which", [1, 2])
def test_reference_graphs_every_start(eng_mod, which):
    """every node of the reference's known-answer graph as a start, one call; its own policy assertions (belief_graph.rs:531-543,
    563-566) on the device output for start 0"""
    g = kat_graphs.graph_1() if which == 1 else kat_graphs.graph_2()
    d = eng_mod.conditional_dijkstra(g["xy"], g["belief_vec"], g["beliefs"], g["types"], g["children"], g["parents"], g["finals"])
    starts = list(range(len(d)))
    got, status = eng_mod.extract_policies_explicit(g["xy"], g["belief_vec"], g["beliefs"], g["belief_id"], g["children"], d, starts)
    G = ref.graph_of_lists(g["xy"], g["belief_vec"], g["beliefs"], g["belief_id"], g["children"])
    assert_answers(got, status, ref.extract_policies(G, d, starts), "graph_%d" % which)
    assert status[0] == 0
    ref.check_reference_assertions(g, got[0][0], which)
    assert (status == 0).sum() >= len(d) // 2


def long_rows_graph():
    """Rows of 699 children (more than a wave's stride, more than 256, more than the kernel's LDS row cache of 512) over three belief ids
    -- 5, 9, 2, interleaved in children order -- below Action and Observation nodes (the walk does not read the type).  All parents sit
    at the origin; a child is a leaf (dist 0) at (2 + j / 1024, 0.5) except two per cluster at (1, 0.25) and (1, -0.25): two exactly
    equal minima, the earlier of which must win.  Cluster 5: positions 510 (lane 62, cached) and 576 (lane 0, not cached); cluster 2:
    191 (lane 63) and 194 (lane 2) -- a reduction on the cost alone, or one that prefers the lower lane, takes the later one.
    Nodes 0, 1: all clusters finite (status 0).  Nodes 2, 3: every child of cluster 9 has dist +inf -- its first child is kept and
    p * inf <= dist[node] fails (status 3).  Node 4: dist +inf (status 1).  Node 5: a root above nodes 0 and 1 (two levels, the LIFO)."""
    KEYS, ROW_OF = (5, 9, 2), {5: 1, 9: 2, 2: 0}
    beliefs = [[0.2, 0.3, 0.5], [0.4, 0.6, 0.0], [0.0, 0.0, 1.0]]
    xy, row, key, dist, children = [], [], [], [], []

    def node(x, y, k, dd):
        xy.append([x, y]); row.append(ROW_OF[k]); key.append(k); dist.append(dd); children.append([])
        return len(xy) - 1
    parents = [node(0.0, 0.0, 2, 1.0) for _ in range(4)]
    node(0.0, 0.0, 2, np.inf)                                   # 4
    top = node(0.0, 0.0, 2, 2.0)                                # 5
    key[1] = 5                                                  # nodes 0 and 1 in clusters of their own below node 5 (both carry belief row 0)
    children[top] = [0, 1]
    minima = {510: 0.25, 576: -0.25, 191: 0.25, 194: -0.25}
    for pi, parent in enumerate(parents):
        for j in range(699):
            k = KEYS[j % 3]
            dd = np.inf if (pi >= 2 and k == 9) else 0.0
            c = node(1.0, minima[j], k, dd) if j in minima else node(2.0 + j / 1024.0, 0.5, k, dd)
            children[parent].append(c)
    return dict(xy=xy, row=row, key=key, dist=np.array(dist), children=children, beliefs=beliefs)


def test_ties_and_long_rows(eng_mod):
    g = long_rows_graph()
    starts = [0, 1, 2, 3, 4, 5, 6]                              # 6: a leaf without children
    got, status = eng_mod.extract_policies_explicit(g["xy"], g["row"], g["beliefs"], g["key"], g["children"], g["dist"], starts)
    G = ref.graph_of_lists(g["xy"], g["row"], g["beliefs"], g["key"], g["children"])
    want = ref.extract_policies(G, g["dist"], starts)
    assert [w[0] for w in want] == [0, 0, 3, 3, 1, 0, 0]
    assert_answers(got, status, want, "long rows")
    # the earlier of the two equal minima, by position in the row: clusters in ascending id order 2, 5, 9
    for q in (0, 1):
        oid = got[q][0][0]
        row = g["children"][q]
        k2 = [j for j in range(699) if g["key"][row[j]] == 2]
        k5 = [j for j in range(699) if g["key"][row[j]] == 5]
        lo2 = [j for j in k2 if g["xy"][row[j]][0] == 1.0]
        lo5 = [j for j in k5 if g["xy"][row[j]][0] == 1.0]
        assert len(lo2) == 2 and len(lo5) == 2 and max(lo2 + lo5) >= 512 and min(lo2 + lo5) < 512
        assert oid.tolist() == [q, row[min(lo2)], row[min(lo5)], row[1]]
    (oid, par, leaf) = got[5][0]
    assert oid[:3].tolist() == [5, 0, 1] and par[:3].tolist() == [-1, 0, 0] and par[3:6].tolist() == [2, 2, 2] and par[6:].tolist() == [1, 1, 1]


# ---------------------------------------------------------------------------------------------- the context's graph

@pytest.fixture(scope="module")
def shelf(eng_mod):
    case = cases.cfg3_near(1500)
    e = cases.configure(eng_mod.Engine(), case)
    cases.grow(e, case, K=64)
    o = cases.configure(orc.Oracle(), case)
    cases.grow(o, case, K=64, algo=orc.ALGO_BATCHED_KD)
    e.build_belief_graph([0.5, 0.5])
    o.build_belief_graph([0.5, 0.5])
    e.compute_expected_costs()
    G, d, types = context_ref(e)
    return e, o, G, d, types


def test_context_graph(eng_mod, shelf):
    e, o, G, d, types = shelf
    single, cost0 = e.extract_policy()
    got, status = e.extract_policies([0])
    assert status[0] == 0 and all(np.array_equal(a, b) for a, b in zip(got[0][0], single)) and got[0][1] == cost0
    assert all(np.array_equal(a, b) for a, b in zip(got[0][0], o.extract_policy(o.expected_costs())))
    rng = np.random.default_rng(2024)
    drawn = rng.integers(0, len(d), size=200).tolist()
    by_hand = [int(np.flatnonzero(d == 0.0)[0]), int(np.flatnonzero((types == 2) & np.isfinite(d))[0])]
    if np.isinf(d).any():
        by_hand.append(int(np.flatnonzero(np.isinf(d))[0]))
    starts = [0] + drawn + by_hand
    got, status = e.extract_policies(starts)
    want = ref.extract_policies(G, d, starts)
    assert_answers(got, status, want, "cfg3_near")
    off, st2, cost, _, _, _ = e.extract_policies_raw(starts)
    assert np.array_equal(bits(cost), bits(d[starts])) and np.array_equal(st2, status)          # written for every query, whatever its status
    assert (status[1:201] == 0).sum() >= 100, "fewer than half of the drawn starts have a policy"
    assert d[by_hand[0]] == 0.0 and types[by_hand[1]] == 2 and np.isfinite(d[by_hand[1]])
    if len(by_hand) == 3:
        assert status[203] == 1
    info = e.policies_info()
    assert info["queries"] == len(starts) and info["ok"] == (status == 0).sum() and info["nodes"] == off[-1] and info["ms_device"] > 0.0
    assert info["max_nodes"] == max(len(g[0][0]) for g in got if g is not None)


def test_single_extraction_outgrows_its_first_slice(eng_mod):
    """The single call walks as a batch of one whose first slice holds kPolSingleSlice = 512 policy nodes; a longer policy is walked
    again with a slice 16 times as long.  cfg3_near with a step of 0.0018: the oracle's root policy has 546 nodes."""
    case = cases.cfg3_near(26000)
    case.update(max_step=0.0018)
    e = cases.configure(eng_mod.Engine(), case)
    cases.grow(e, case, K=64)
    o = cases.configure(orc.Oracle(), case)
    cases.grow(o, case, K=64, algo=orc.ALGO_BATCHED_KD)
    e.build_belief_graph([0.5, 0.5])
    o.build_belief_graph([0.5, 0.5])
    do = o.expected_costs()
    want = o.extract_policy(do)
    assert len(want[0]) > 512
    e.compute_expected_costs()
    got, cost = e.extract_policy()
    assert bits([cost])[0] == bits([do[0]])[0]
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_sixteen_worlds_branching(eng_mod):
    case = cases.cfg_door(paper=True)
    e = cases.configure(eng_mod.Engine(), case)
    cases.grow(e, case, K=256)
    e.build_belief_graph([1.0 / 16] * 16)
    e.compute_expected_costs()
    G, d, types = context_ref(e)
    (oid, par, leaf), cost0 = e.extract_policy()
    below_obs = [int(oid[k]) for k in range(1, len(oid)) if types[int(oid[par[k]])] == 2]
    assert len(below_obs) >= 2                                   # the policy branches
    rng = np.random.default_rng(16)
    finite = np.flatnonzero(np.isfinite(d))
    starts = [0] + below_obs[:12] + rng.choice(finite, size=30, replace=False).tolist() + rng.integers(0, len(d), size=8).tolist()
    got, status = e.extract_policies(starts)
    assert status[0] == 0 and all(np.array_equal(a, b) for a, b in zip(got[0][0], (oid, par, leaf))) and got[0][1] == cost0
    assert_answers(got, status, ref.extract_policies(G, d, starts), "door")
    assert (status == 0).sum() >= len(starts) // 2


def test_the_walk_that_does_not_end(eng_mod):
    """cfg_map4 grown by the reference's own loop (K = 1): with seed 0 the walk from node 0 returns onto its own path (status 2, at once);
    with seed 1 it ends and equals the oracle"""
    prior = [1.0 / 16] * 16
    for seed, want in ((0, 2), (1, 0)):
        case = cases.cfg_map4(5000, seed)
        e = cases.configure(eng_mod.Engine(), case)
        cases.grow(e, case, K=1)
        e.build_belief_graph(prior)
        e.compute_expected_costs()
        t0 = time.perf_counter()
        got, status = e.extract_policies([0])
        assert time.perf_counter() - t0 < 1.0
        assert status[0] == want
        if want == 0:
            o = cases.configure(orc.Oracle(), case)
            cases.grow(o, case, K=1, algo=orc.ALGO_SEQ)
            o.build_belief_graph(prior)
            assert all(np.array_equal(a, b) for a, b in zip(got[0][0], o.extract_policy(o.expected_costs())))
        else:
            assert got[0] is None
            with pytest.raises(eng_mod.PorrtError, match="returns to a belief node on its own path"):
                e.extract_policy()


# ---------------------------------------------------------------------------------------------- the multi-modal graph

def test_multi_modal(eng_mod):
    """The smallest case of test_gpu_mm_plan.py: test_benchmark_two_goals, seed 0 (3123 belief nodes, 3 modes, a finite root).  Its
    test_two_shelves is larger (6243) and its root has no finite cost, so there is no single extraction to compare start 0 with.
    The reference walks the ORACLE's growth (mm_plan_ref on oracle/mmprm.c), not the engine's own belief graph: a wrong roadmap is
    not walked consistently on both sides.  There policies_ref gives status 0 for 43 of the 50 drawn starts and status 1 for the
    other 7."""
    import mm_plan_ref
    c = cases.cfg2(10)
    c.update(zones="map_benchmark_like_2_goals_zone_ids", visibility=0.5)
    case = cases.Case(c, seed=0)
    e = cases.configure(eng_mod.Engine(), case)
    o = cases.configure(orc.Oracle(), case)
    e.set_discrete_seed(0)
    o.set_discrete_seed(0)
    e.grow_mm_prm(case.start, [0.5, 0.5], 0.1, 2.0, 1000)
    _, obg, odist = mm_plan_ref.plan(o, case.start, [0.5, 0.5], 0.1, 2.0, 1000)
    e.mm_build_belief_graph()
    d = e.mm_expected_costs()
    assert np.array_equal(bits(d), bits(odist))
    xy = obg["xy"]
    G = ref.graph_of_lists(xy, obg["belief_vec"], obg["beliefs"], obg["belief_ids"], obg["children"])
    (oid, par, leaf, pxy), cost0 = e.mm_extract_policy()
    rng = np.random.default_rng(5)
    starts = [0] + rng.integers(0, len(d), size=50).tolist()
    got, status = e.mm_extract_policies(starts)
    assert status[0] == 0 and got[0][1] == cost0
    for a, b in zip(got[0][0], (oid, par, leaf, pxy)):
        assert np.array_equal(a, b)
    assert_answers(got, status, ref.extract_policies(G, odist, starts), "multi-modal")
    for g in got:
        if g is not None:
            assert np.array_equal(bits(g[0][3]), bits(xy[g[0][0].astype(np.int64)]))
    assert (status[1:] == 0).sum() >= 25 and (status == 1).any()
    (oid2, par2, leaf2, pxy2), _ = e.mm_extract_policy()        # the single extraction is what it was
    assert np.array_equal(oid, oid2) and np.array_equal(par, par2)
    assert e.policies_info()["queries"] == len(starts)


# ---------------------------------------------------------------------------------------------- the interface

def test_interface(eng_mod, shelf):
    import ctypes as C
    _, _, G, d, _ = shelf
    case = cases.cfg3_near(1500)
    e = cases.configure(eng_mod.Engine(), case)
    cases.grow(e, case, K=64)
    with pytest.raises(eng_mod.PorrtError):
        e.extract_policies([0])                                 # no belief graph
    e.build_belief_graph([0.5, 0.5])
    with pytest.raises(eng_mod.PorrtError):
        e.extract_policies([0])                                 # no costs
    e.compute_expected_costs()
    single, cost0 = e.extract_policy()
    refined, rcost = e.refine_policy(50)
    L, c = e._l, e._c
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # n = 0
    off = np.full(1, 7, dtype=np.uint64)
    assert L.porrt_bg_extract_policies(c, np.zeros(1, dtype=np.uint64), 0, off, np.zeros(1, dtype=np.uint8), np.zeros(1), None, None, None, 0) == 0
    assert off[0] == 0
    got, status = e.extract_policies([])
    assert got == [] and len(status) == 0
    # cap too small: offsets, statuses and costs only; the total comes back; the getter hands out the same arrays
    rng = np.random.default_rng(3)
    starts = np.array([0] + rng.integers(0, len(d), size=20).tolist(), dtype=np.uint64)
    n = len(starts)
    off, st, cost = np.zeros(n + 1, dtype=np.uint64), np.full(n, 9, dtype=np.uint8), np.zeros(n)
    oid, par, leaf = np.full(4, 77, dtype=np.uint64), np.full(4, 77, dtype=np.int64), np.full(4, 77, dtype=np.uint8)
    total = L.porrt_bg_extract_policies(c, starts, n, off, st, cost, p(oid), p(par), p(leaf), 4)
    assert total > 4 and off[-1] == total and (oid == 77).all() and (par == 77).all() and (leaf == 77).all() and (st != 9).all()
    oid, par, leaf = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8)
    assert L.porrt_bg_extract_policies(c, starts, n, off, st, cost, p(oid), p(par), p(leaf), total) == total
    oid2, par2, leaf2 = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8)
    assert L.porrt_bg_get_policies(c, p(oid2), p(par2), p(leaf2), total) == total
    assert np.array_equal(oid, oid2) and np.array_equal(par, par2) and np.array_equal(leaf, leaf2)
    assert L.porrt_bg_get_policies(c, None, None, None, 0) == total
    want = ref.extract_policies(G, d, starts)
    assert np.array_equal(st, [w[0] for w in want])
    # one batch equals one-by-one calls
    for q in range(n):
        g1, s1 = e.extract_policies([starts[q]])
        assert s1[0] == st[q]
        if st[q] == 0:
            a, b = int(off[q]), int(off[q + 1])
            assert np.array_equal(g1[0][0][0], oid[a:b]) and np.array_equal(g1[0][0][1], par[a:b]) and np.array_equal(g1[0][0][2], leaf[a:b])
    # a start that is no belief node fails the call
    with pytest.raises(eng_mod.PorrtError) as ei:
        e.extract_policies([0, len(d)])
    assert ei.value.code == -1                                  # PORRT_ERR_INVALID
    # policy_max_nodes = 8: a longer policy is status 4, a short one in the same call stays 0
    near = [int(s) for s in np.argsort(d)[:400] if d[s] > 0.0][:60]                         # starts close to a goal: short policies
    short = [(s, len(pol[0])) for s, (status, pol, _) in zip(near, ref.extract_policies(G, d, near)) if status == 0 and len(pol[0]) <= 8]
    long_s, short_s = 0, short[0][0]
    lens = {long_s: len(single[0]), short_s: short[0][1]}
    assert lens[long_s] > 8 >= lens[short_s]
    assert e.get_option("policy_max_nodes") == 1 << 16
    e.set_option("policy_max_nodes", 8)
    got, status = e.extract_policies([long_s, short_s])
    assert status.tolist() == [4, 0] and got[0] is None and len(got[1][0][0]) == lens[short_s]
    assert [w[0] for w in ref.extract_policies(G, d, [long_s, short_s], max_nodes=8)] == [4, 0]
    assert "query 0" in L.porrt_last_error(c).decode()
    with pytest.raises(eng_mod.PorrtError):
        e.set_option("policy_max_nodes", 0)
    with pytest.raises(eng_mod.PorrtError):
        e.set_option("policy_max_nodes", (1 << 24) + 1)
    e.set_option("policy_max_nodes", 1 << 16)
    # the single extraction and its refinement are what they were
    single2, cost2 = e.extract_policy()
    refined2, rcost2 = e.refine_policy(50)
    assert all(np.array_equal(a, b) for a, b in zip(single, single2)) and cost0 == cost2
    assert all(np.array_equal(a, b) for a, b in zip(refined, refined2)) and rcost == rcost2
    # stale: a new belief graph without new costs, then a regrowth
    e.build_belief_graph([0.5, 0.5])
    with pytest.raises(eng_mod.PorrtError):
        e.extract_policies([0])
    assert L.porrt_bg_get_policies(c, None, None, None, 0) < 0
    e.compute_expected_costs()
    assert e.extract_policies([0])[1][0] == 0
    cases.grow(e, case, K=64)
    with pytest.raises(eng_mod.PorrtError):
        e.extract_policies([0])
    assert L.porrt_bg_get_policies(c, None, None, None, 0) < 0


# ---------------------------------------------------------------------------------------------- the single extraction's store

def test_single_extraction_refuses_costs_of_another_belief_graph(eng_mod):
    """a belief graph rebuilt without a new cost run: the single extraction refuses as the batched one does, whether a policy was
    walked on the old costs (it is not handed out again) or not (nothing is walked on the old costs)"""
    case = cases.cfg3_near(1500)
    e = cases.configure(eng_mod.Engine(), case)
    cases.grow(e, case, K=64)
    for walked_before in (True, False):
        e.build_belief_graph([0.5, 0.5])
        e.compute_expected_costs()
        if walked_before:
            e.extract_policy()
        e.build_belief_graph([0.9, 0.1])
        with pytest.raises(eng_mod.PorrtError) as ei:
            e.extract_policy()
        assert ei.value.code == -1 and "compute the expected costs first" in str(ei.value)
        with pytest.raises(eng_mod.PorrtError):
            e.extract_policies([0])
    e.compute_expected_costs()
    single, cost = e.extract_policy()
    got, status = e.extract_policies([0])
    assert status[0] == 0 and all(np.array_equal(a, b) for a, b in zip(got[0][0], single))
    assert bits([got[0][1]])[0] == bits([cost])[0]
    G, d, _ = context_ref(e)
    assert_answers(got, status, ref.extract_policies(G, d, [0]), "the rebuilt graph")


def test_single_and_batched_results_are_kept_apart(eng_mod, shelf):
    e, _, _, d, _ = shelf
    first, cost1 = e.extract_policy()
    again, cost2 = e.extract_policy()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)) and bits([cost1])[0] == bits([cost2])[0]
    starts = [5, 17, 0, 3]
    got, status = e.extract_policies(starts)
    info = e.policies_info()
    third, cost3 = e.extract_policy()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, third)) and bits([cost1])[0] == bits([cost3])[0]
    assert e.policies_info() == info and info["queries"] == len(starts) and info["ok"] == (status == 0).sum()
    assert info["nodes"] == sum(len(g[0][0]) for g in got if g is not None)
