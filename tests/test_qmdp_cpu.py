"""CPU checks of the QMDP restatement (tests/qmdp_ref.py) against the vectors the reference itself asserts for dijkstra
(pto_graph.rs:626-678) and the 2-world diamond (:539-564) worked by hand, of its walks on graphs small enough to follow, and of the
interface's declarations.  No device is touched."""
import math
import os
import re

import pytest

import qmdp_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
QMDP_SYMBOLS = ["porrt_qmdp_plan", "porrt_qmdp_get_costs", "porrt_qmdp_info", "porrt_qmdp_react", "porrt_qmdp_costs"]


@pytest.mark.parametrize("name", sorted(Q.KATS))
def test_restatement_matches_the_asserted_vectors(name):
    make, finals, want = Q.KATS[name]
    assert Q.costs_explicit(make(), finals) == want


def test_plain_dijkstra_is_the_world_view_with_one_validity():
    g = Q.grid_graph()
    par = Q.weighted_parents(g["xy"], g["children"])
    assert Q.dijkstra_world(g["node_validity"], g["validities"], par, None, [8]) == Q.KATS["grid_to_8"][2][0]


def test_view_filters_the_parent_not_the_child():
    """node 1 of the diamond is not valid in world 0: it keeps inf although its child 3 is final, and node 0 is reached through 2"""
    c = Q.costs_explicit(Q.diamond_graph_2_worlds(), [[3], [3]])
    assert c[0][1] == INF and c[0][0] == c[0][2] + math.sqrt(2.0)
    # a final node that is not valid in the world still starts at 0 and relaxes its parents
    g = Q.diamond_graph_2_worlds()
    c = Q.costs_explicit(g, [[1], [2]])
    assert c[0][1] == 0.0 and c[0][0] == math.sqrt(2.0) and c[0][3] == math.sqrt(2.0) and c[0][2] == 2 * math.sqrt(2.0)


def diamond():
    g = Q.diamond_graph_2_worlds()
    return Q.Qmdp(g["xy"], g["node_validity"], g["validities"], g["children"], [3], [0b11], [0b11] * 4, 2)


def test_plan_needs_a_final_node_per_world():
    q = diamond()
    q.final_masks = [0b01]
    with pytest.raises(ValueError, match="We should have final node ids for each world"):
        q.plan_qmdp()
    q = diamond()
    q.reach[3] = 0b10                 # final for both worlds but reached in world 1 only
    with pytest.raises(ValueError, match="final node ids"):
        q.plan_qmdp()


def test_react_on_the_diamond():
    q = diamond()
    q.plan_qmdp()
    assert q.cost_to_goals == Q.KATS["diamond_2_worlds"][2]
    # certain of world 0: inf * 0.0 is NaN for child 2 ... no: child 1 has inf in world 0 -> E = inf; child 2: sqrt2 * 1 + inf * 0 = NaN.
    # Neither wins: the walk falls to node 0 with cost inf and goes on until the horizon is used up -- it never is (norm2(0, 0) = 0).
    q.max_states = 8
    with pytest.raises(Q.WalkTooLong):
        q.react_qmdp((0.1, 0.0), [1.0, 0.0], 0.5)
    # horizon 0: no common state; per world the greedy walk 0 -> 2 -> (3) and 0 -> 1 -> (3); the node of cost 0 is not pushed
    paths, ncommon = q.react_qmdp((0.1, 0.0), [0.5, 0.5], 0.0)
    assert ncommon == 0
    assert paths == [[(0.0, 0.0), (1.0, -1.0)], [(0.0, 0.0), (1.0, 1.0)]]
    # a start nearest to the goal node: every path is empty
    assert q.react_qmdp((2.1, 0.0), [0.5, 0.5], 0.0) == ([[], []], 0)
    with pytest.raises(ValueError, match="belief state size should match the number of worlds"):
        q.react_qmdp((0.0, 0.0), [1.0], 0.2)


def test_react_on_the_grid_follows_the_expected_cost():
    g = Q.grid_graph()
    q = Q.Qmdp(g["xy"], g["node_validity"], g["validities"], g["children"], [8], [1], [1] * 9, 1)
    q.plan_qmdp()
    # from node 0: children [1, 3] both cost 3: the first (1) wins; then 1's children [0, 2, 4]: 2 is the first of cost 2; ..
    paths, ncommon = q.react_qmdp((0.2, 0.1), [1.0], 1.5)
    assert ncommon == 2 and paths == [[(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (2.0, 1.0)]]
    # a horizon longer than the way: the common path stops when the expected cost reaches 0 and holds every node but the goal
    paths, ncommon = q.react_qmdp((0.2, 0.1), [1.0], 100.0)
    assert ncommon == 4 and paths == [[(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (2.0, 1.0)]]
    # the cap counts emitted states: exactly max_states is fine, one more is not
    q.max_states = 4
    assert q.react_qmdp((0.2, 0.1), [1.0], 100.0)[1] == 4
    q.max_states = 3
    with pytest.raises(Q.WalkTooLong):
        q.react_qmdp((0.2, 0.1), [1.0], 100.0)


def test_kd_nearest_is_the_nearest():
    import random
    rnd = random.Random(5)
    xy = [(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(400)]
    kd = Q.KdTree(xy)
    for _ in range(100):
        s = (rnd.uniform(-1.2, 1.2), rnd.uniform(-1.2, 1.2))
        assert Q.norm2(xy[kd.nearest(s)], s) == min(Q.norm2(p, s) for p in xy)


def test_children_from_edges_is_the_push_order():
    # node 2 is created with neighbours [1, 0] (kd order), node 3 with [2]: 0: [.., 2], 1: [.., 2], 2: [1, 0, 3], 3: [2]
    assert Q.children_from_edges(4, [0, 1, 0, 2], [1, 2, 2, 3]) == [[1, 2], [0, 2], [1, 0, 3], [2]]


def test_interface_is_declared():
    from po_rrt_amd import engine
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "porrt_hip.h")).read(), flags=re.S)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mirror = open(os.path.join(ROOT, "include", "porrt.hpp")).read()
    for s in QMDP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), "%s is not declared in porrt_hip.h" % s
        assert "pub fn %s(" % s in integ, "%s is not in INTEGRATION.md's Rust block" % s
        assert s in engine.SYMBOLS
        assert s in mirror, "%s is not used by include/porrt.hpp" % s
    full = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    for cite in ("qmdp_policy_extractor.rs:23-35", "qmdp_policy_extractor.rs:38-49", "pto_reachability.rs:58-63", "pto_graph.rs:245-271"):
        assert cite in full
    for m in ("qmdp_plan", "qmdp_costs", "qmdp_react", "qmdp_info"):
        assert hasattr(engine.Engine, m)
    assert hasattr(engine, "qmdp_costs_explicit")


def test_library_exports_the_entries_and_rejects_null():
    import ctypes as C
    import numpy as np
    from po_rrt_amd import build, engine
    build.build()
    L = engine.load_library()
    for s in QMDP_SYMBOLS:
        assert hasattr(L, s)
    assert L.porrt_qmdp_plan(None) < 0
    assert L.porrt_qmdp_get_costs(None, np.zeros(1)) < 0
    assert L.porrt_qmdp_info(None, C.byref(engine.QmdpInfo())) < 0
    z, u = np.zeros(2), np.zeros(2, dtype=np.uint64)
    assert L.porrt_qmdp_react(None, z, z, 1, z, 0, u, u, None, 0) < 0
    # the explicit entry validates its arrays before it looks for a device: n = 0, 65 worlds, a child id out of range
    one32 = np.zeros(1, dtype=np.uint32)
    val = np.ones(1, dtype=np.uint64)
    off = np.zeros(2, dtype=np.uint64)
    args = lambda n, nw, co, ci: (0, n, z, one32, val, 1, nw, co, ci, np.zeros(nw + 1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(max(n, 1) * nw))
    assert L.porrt_qmdp_costs(*args(0, 1, off, one32)) < 0
    assert L.porrt_qmdp_costs(*args(1, 65, off, one32)) < 0
    assert L.porrt_qmdp_costs(*args(1, 1, np.array([0, 1], dtype=np.uint64), np.array([7], dtype=np.uint32))) < 0
