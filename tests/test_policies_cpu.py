"""tests/policies_ref.py -- the Python restatement of extract_policy (belief_graph.rs:184-267) from any start, the reference of
the device's porrt_*_extract_policies -- pinned against the oracle's C restatement, which starts at node 0: at s = 0 directly, at
s != 0 on the same graph with nodes 0 and s swapped.  No GPU."""
import numpy as np
import pytest

import cases
import kat_graphs
import policies_ref as ref
from oracle import orc


def kat(which):
    g = kat_graphs.graph_1() if which == 1 else kat_graphs.graph_2()
    d, ccsr, _ = orc.conditional_dijkstra(g["xy"], g["belief_vec"], g["beliefs"], g["types"], g["children"], g["parents"], g["finals"])
    return g, d, ccsr


def swapped(s, xy, belief_id, belief_vec, children, dist):
    """the graph with the labels of nodes 0 and s exchanged; children lists keep their order"""
    n = len(dist)
    perm = np.arange(n)
    perm[0], perm[s] = s, 0                                  # its own inverse
    pick = lambda a: np.asarray(a)[perm]
    ch = [[int(perm[c]) for c in children[int(perm[i])]] for i in range(n)]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in ch])
    ids = np.array([v for c in ch for v in c] + [0], dtype=np.uint32)
    return perm, pick(xy), pick(belief_id), pick(belief_vec), (off, ids), pick(dist)


def oracle_from(s, xy, belief_id, belief_vec, beliefs, children, dist, cap=4096):
    """orc.extract_policy started at s by relabelling: the policy with the ids mapped back, or None where the oracle fails"""
    perm, xy2, bid2, bvec2, csr2, d2 = swapped(s, xy, belief_id, belief_vec, children, dist)
    try:
        oid, par, leaf = orc.extract_policy(xy2, bid2, bvec2, beliefs, csr2, d2, cap=cap)
    except RuntimeError:
        return None
    return perm[oid.astype(np.int64)].astype(np.uint64), par, leaf


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("which", [1, 2])
def test_restatement_equals_oracle_on_the_reference_graphs(which):
    g, d, ccsr = kat(which)
    G = ref.graph_of_lists(g["xy"], g["belief_vec"], g["beliefs"], g["belief_id"], g["children"])
    st, pol, cost = ref.extract_policy(G, d, 0)
    assert st == ref.OK and cost == d[0]
    assert same(pol, orc.extract_policy(g["xy"], g["belief_id"], g["belief_vec"], g["beliefs"], ccsr, d))
    ref.check_reference_assertions(g, pol, which)            # belief_graph.rs:531-543, 563-566
    n_ok = 0
    for s in range(len(d)):                                  # every start, against the oracle on the relabelled graph
        st, pol, cost = ref.extract_policy(G, d, s)
        want = oracle_from(s, g["xy"], g["belief_id"], g["belief_vec"], g["beliefs"], g["children"], d)
        assert cost == d[s]
        assert (st == ref.OK) == (want is not None), "start %d: status %d" % (s, st)
        if want is not None:
            assert same(pol, want), "start %d" % s
            n_ok += 1
    assert n_ok >= len(d) // 2


@pytest.fixture(scope="module")
def grown():
    case = cases.cfg3_near(1500)
    o = cases.configure(orc.Oracle(), case)
    cases.grow(o, case, K=64, algo=orc.ALGO_BATCHED_KD)
    o.build_belief_graph([0.5, 0.5])
    d = o.expected_costs()
    beliefs, types, (coff, cid), _ = o.belief_graph()
    return o, d, beliefs, coff, cid


def test_restatement_equals_oracle_on_a_grown_graph(grown):
    o, d, beliefs, coff, cid = grown
    G = ref.context_graph(o.tree()[0], beliefs, coff, cid)
    st, pol, cost = ref.extract_policy(G, d, 0)
    assert st == ref.OK and cost == d[0]
    assert same(pol, o.extract_policy(d))
    # a few dozen other starts: the oracle on the relabelled graph
    n, B = len(d), len(beliefs)
    xy = np.repeat(np.asarray(o.tree()[0]).reshape(-1, 2), B, axis=0)
    bid = (np.arange(n) % B).astype(np.uint32)
    children = [cid[int(coff[i]):int(coff[i + 1])].tolist() for i in range(n)]
    rng = np.random.default_rng(7)
    starts = rng.choice(np.arange(1, n), size=40, replace=False).tolist()
    starts += [int(np.flatnonzero(d == 0.0)[0])]                              # a final node
    if np.isinf(d).any():
        starts += [int(np.flatnonzero(np.isinf(d))[0])]                       # no policy from there
    statuses = []
    for s in starts:
        st, pol, cost = ref.extract_policy(G, d, s)
        statuses.append(st)
        assert cost == d[s] or (np.isnan(cost) and np.isnan(d[s]))
        if st in (ref.OK, ref.ASSERT, ref.NO_COST):
            want = oracle_from(s, xy, bid, bid, beliefs, children, d, cap=1 << 16)
            if st == ref.OK:
                assert want is not None and same(pol, want), "start %d" % s
            elif st == ref.ASSERT:
                assert want is None, "start %d: the oracle's assertion holds" % s
    assert statuses.count(ref.OK) >= 20


def test_statuses_of_the_restatement():
    g, d, _ = kat(1)
    G = ref.graph_of_lists(g["xy"], g["belief_vec"], g["beliefs"], g["belief_id"], g["children"])
    dinf = np.array(d)
    dinf[0] = np.inf
    assert ref.extract_policy(G, dinf, 0)[0] == ref.NO_COST
    assert ref.extract_policy(G, d, 0, max_nodes=4)[0] == ref.CAPACITY
    assert ref.extract_policy(G, d, 0, max_nodes=len(ref.extract_policy(G, d, 0)[1][0]))[0] == ref.OK
    # two nodes at one place, each the other's best child: the walk returns onto its own path
    G2 = ref.graph_of_lists([[0, 0], [0, 0]], [0, 0], [[1.0]], [0, 0], [[1], [0]])
    assert ref.extract_policy(G2, [1.0, 1.0], 0)[0] == ref.OWN_PATH
    # p * dist[best] <= dist[node] fails below a final start whose only child costs something
    G3 = ref.graph_of_lists([[0, 0], [1, 0]], [0, 0], [[1.0]], [0, 0], [[1], []])
    assert ref.extract_policy(G3, [0.0, 1.0], 0)[0] == ref.ASSERT
    st, pol, _ = ref.extract_policy(G3, [0.0, 0.0], 0)       # a final start above a final child: root (no leaf) and one leaf
    assert st == ref.OK and pol[2].tolist() == [0, 1]
    # a child whose belief has no world in common: p = 0
    G4 = ref.graph_of_lists([[0, 0], [1, 0]], [0, 1], [[1.0, 0.0], [0.0, 1.0]], [0, 1], [[1], []])
    assert ref.extract_policy(G4, [1.0, 0.0], 0)[0] == ref.ASSERT
