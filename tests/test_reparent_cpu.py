"""The restatement of refine_solution(Reparent(radius)) (tests/reparent_ref.py) on its own: hand-built graphs with their answers written
out, the queue against a second implementation, the tie rule reversed, the reference's leaf assertion on grown cases, the caps.
No GPU."""
import numpy as np
import pytest

import cases
import refine_policies_cases as rp
import reparent_cases as rc
import reparent_ref as rr
from oracle import orc

from reparent_cases import GROWN_SEEDS, door_case, shelf_case


@pytest.fixture(scope="module")
def o():
    o = orc.Oracle()
    o.set_grid(rp.wall_raster(), (-1.0, -1.0), (1.0, 1.0), orc.DOMAIN_SHELF)
    return o


def tree_of(o, case, piece=None):
    """build_tree, the valid neighbours and reparent of the case's first piece (or the piece given as policy node ids)"""
    ids = [case.ids[i] for i in (piece or rr.decompose(case.parents)[0][0])]
    t = rr.build_tree(case.G, ids, case.radius, 1 << 14)
    nbrs = rr.valid_neighbours(o, t, 0.5 * case.radius, [True], 1, 1 << 14)
    return t, nbrs


def test_grandchild_skip(o):
    t, _ = tree_of(o, rc.grandchild_skip())
    assert t.g == [0, 1, 3] and t.parent == [None, 0, 1]                 # cc (id 2) is not added; x hangs from c
    assert t.cost[2] == rr.norm2(t.state[0], t.state[2])                 # ... with the cost of A -> x


def test_push_time_visited_filter(o):
    t, _ = tree_of(o, rc.push_time_filter())
    assert t.g == [0, 1, 2, 4]                                           # A, v, c, z: y (id 3) is absent
    assert t.parent == [None, 0, 0, 1]                                   # z hangs from v's tree node alone


def test_offspring_edge_cost_decides_a_reparent(o):
    t, nbrs = tree_of(o, rc.offspring_edge_cost())
    assert t.cost[2] == 0.125 and t.dist_from_root(2) == 0.1875
    assert rr.norm2(t.state[1], t.state[2]) + t.cost[1] == 0.125         # what the sum would be with the distance to the tree parent
    st = {}
    rr.reparent(t, nbrs, stats=st)
    assert t.parent == [None, 0, 0] and st["reparents"] == 1


def test_upward_summation_order_decides(o):
    case = rc.summation_order()
    t, nbrs = tree_of(o, case)
    up = t.dist_from_root(3)
    down = (t.cost[1] + t.cost[2]) + t.cost[3]
    offer = t.dist_from_root(1) + rr.norm2(t.state[1], t.state[3])
    assert up == 0.864 and down == 0.8640000000000001 and offer == up and offer < down
    rr.reparent(t, nbrs)
    assert t.parent == [None, 0, 1, 2]
    status, ((xy, oid, par, leaf), cost) = rc.restate(o, case)
    assert status == 0 and list(oid) == [0, 1, 2, 3]


def test_stale_priority_is_popped(o):
    case = rc.stale_priority()
    t, nbrs = tree_of(o, case)
    assert t.g == [0, 1, 2, 3, 4, 6] and t.parent[5] == 4                # V is skipped, X hangs from W
    st = {}
    pops = rr.reparent(t, nbrs, stats=st)
    assert pops == 7 and st["stale_pops"] >= 1                           # c is popped under the sum it had before b moved
    assert t.parent[2] == 0 and t.parent[5] == 3                         # b under R; X under c, after X's own pop
    status, ((xy, oid, par, leaf), cost) = rc.restate(o, case)
    assert status == 0 and list(oid) == [0, 2, 3]                        # the detour over a is gone


def test_one_node_piece_that_branches(o):
    status, ((xy, oid, par, leaf), cost) = rc.restate(o, rc.one_node_piece_branches())
    assert status == 0 and list(oid) == [0, 1, 3, 2, 4] and list(par) == [-1, -1, 1, -1, 3] and list(leaf) == [1, 0, 1, 0, 1]
    assert cost == 0.0


def test_two_node_piece_grows_longer(o):
    status, ((xy, oid, par, leaf), cost) = rc.restate(o, rc.two_node_piece_grows())
    assert status == 0 and list(oid) == [0, 2, 1] and list(par) == [-1, 0, 1] and list(leaf) == [0, 0, 1]
    assert cost == 0.423


def test_wall_inside_the_radius(o):
    case = rc.wall_in_range()
    t, nbrs = tree_of(o, case)
    assert t.g == [0, 1, 2, 4, 3]
    assert 2 not in nbrs[0] and 0 not in nbrs[2] and 3 in nbrs[0]        # across the wall: in range (0.1 <= 0.15), refused


@pytest.mark.parametrize("make", rc.HAND, ids=lambda f: f.__name__)
def test_neighbours_literal_and_with_cached_state_validities(o, make):
    case = make()
    t, nbrs = tree_of(o, case)
    assert nbrs == rr.valid_neighbours(o, t, 0.5 * case.radius, [True], 1, 1 << 14, literal=True)


def same(a, b):
    if a[0] != b[0]:
        return False
    if a[0] != 0:
        return True
    (x, oid, par, leaf), cost = a[1]
    (x2, oid2, par2, leaf2), cost2 = b[1]
    return (x.shape == x2.shape and np.array_equal(x.view(np.uint64), x2.view(np.uint64)) and np.array_equal(oid, oid2) and np.array_equal(par, par2)
            and np.array_equal(leaf, leaf2) and np.float64(cost).view(np.uint64) == np.float64(cost2).view(np.uint64))


@pytest.mark.parametrize("make", rc.HAND, ids=lambda f: f.__name__)
def test_second_queue_implementation(o, make):
    case = make()
    s1, s2 = {}, {}
    assert same(rc.restate(o, case, stats=s1), rc.restate(o, case, queue="heap", stats=s2))
    assert (s1["pops"], s1["reparents"]) == (s2["pops"], s2["reparents"])


def test_lattice_has_ties_and_the_tie_rule_reversed(o):
    """ties occur on the lattice; popping the HIGHEST id among them gives the same refined policies on every hand case and on the grown
    ones below: no case was found where the outcome differs"""
    st = {}
    status, _ = rc.restate(o, rc.lattice(), stats=st)
    assert status == 0 and st["tied_pops"] > 0
    st = {}
    rc.restate(o, rc.copies(), stats=st)
    assert st["tied_pops"] > 0
    for make in rc.HAND:
        assert same(rc.restate(o, make()), rc.restate(o, make(), tie="high")), make.__name__


class GrownCpu:
    def __init__(self, case, prior):
        self.o = o = cases.configure(orc.Oracle(), case)
        cases.grow(o, case)
        o.build_belief_graph(prior)
        beliefs, _, (coff, cid), _ = o.belief_graph()
        d = o.expected_costs()
        assert np.isfinite(d[0])
        self.policy = o.extract_policy(d)
        self.G = rr.Graph.implicit(o.tree()[0], beliefs, coff, cid)


@pytest.mark.parametrize("domain,seed", [(d, s) for d in ("door", "shelf") for s in GROWN_SEEDS[d]])
def test_reference_assertion_on_grown_cases(domain, seed):
    """the reference's own assertion, policy.leafs.len() == refined.leafs.len(), at Reparent(0.3)"""
    g = GrownCpu(*(door_case if domain == "door" else shelf_case)(seed))
    oid, par, leaf = g.policy
    st = {}
    status, ((xy, roid, rpar, rleaf), cost) = rr.refine(g.o, g.G, oid, par, 0.3, stats=st)
    assert status == 0 and int(rleaf.sum()) == int(leaf.sum())
    assert st["reparents"] > 0 and st["max_tree"] > len(oid)
    assert same((status, ((xy, roid, rpar, rleaf), cost)), rr.refine(g.o, g.G, oid, par, 0.3, tie="high"))
    assert same((status, ((xy, roid, rpar, rleaf), cost)), rr.refine(g.o, g.G, oid, par, 0.3, queue="heap"))


def test_caps(o):
    case = rc.star(9)                                                    # a tree of 10 nodes
    assert rc.restate(o, case, max_tree_nodes=10)[0] == 0
    assert rc.restate(o, case, max_tree_nodes=9)[0] == 4
    case = rc.path_with_star(4, 0)                                       # the path alone counts
    assert rc.restate(o, case, max_tree_nodes=4)[0] == 0 and rc.restate(o, case, max_tree_nodes=3)[0] == 4
    # the pop cap: the stale-priority case makes 7 pops for 6 nodes
    assert rc.restate(o, rc.stale_priority(), pops_per_node=1)[0] == 5
    assert rc.restate(o, rc.stale_priority(), pops_per_node=2)[0] == 0
    assert rc.restate(o, rc.lattice(), pops_per_node=1)[0] == 0
    # the pairs in range: 301 nodes all within reach of each other are 90 601 pairs; 256 x max_tree_nodes pairs are allowed
    assert rc.restate(o, rc.star(300), max_tree_nodes=353)[0] == 4 and rc.restate(o, rc.star(300), max_tree_nodes=354)[0] == 0     # 256 * 353 = 90 368 < 90 601 <= 256 * 354


def test_status_of_faults_and_mixed_pieces(o):
    assert rc.restate(o, rc.leaves_raster())[0] == 2
    assert rc.restate(o, rc.mixed_piece())[0] == 3
    assert rr.refine(o, rc.star(3).G, [], [], 0.3)[0] == 1
