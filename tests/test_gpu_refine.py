"""GPU parity of the policy refiner (porrt_bg_refine_policy / porrt_refine_policy: the batch refiner with one policy): PTOPolicyRefiner::
refine_solution(PartialShortCut(n)) (src/pto_policy_refiner.rs:87-124) on grown pipelines and on hand-built policies, every result
compared bit for bit (states, original ids, parents, leafs, expected cost) with the restatement tests/refine_ref.py."""
import ctypes as C

import numpy as np
import pytest

import cases
import refine_ref
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def assert_same(got, want):
    (x, oid, par, leaf), cost = got
    (x2, oid2, par2, leaf2), cost2 = want
    assert x.shape == x2.shape and np.array_equal(x.view(np.uint64), x2.view(np.uint64)), "refined states differ"
    assert np.array_equal(oid, oid2) and np.array_equal(par, par2) and np.array_equal(leaf, leaf2)
    assert np.float64(cost).view(np.uint64) == np.float64(cost2).view(np.uint64), (cost, cost2)


def pipeline(eng_mod, case, K, prior):
    e = cases.configure(eng_mod.Engine(), case)
    cases.grow(e, case, K=K)
    e.build_belief_graph(prior)
    e.compute_expected_costs()
    return e


def check_grown(e, case, ns=(0, 1, 500, 1500)):
    (oid, par, leaf), _ = e.extract_policy()
    xy = e.tree()[0]
    beliefs = e.belief_graph(lists=False)[0]
    B = len(beliefs)
    o = cases.configure(orc.Oracle(), case)
    x0 = e.refine_policy(0)[0][0]
    assert len(x0) == len(oid)
    for n in ns:
        got = e.refine_policy(n)
        want = refine_ref.refine_policy_of(o, xy, oid, par, B, beliefs, n)
        assert_same(got, want)
        (x, oid_r, par_r, leaf_r), cost = got
        # independent property check: every edge the shortcuts moved is a valid transition under its piece's belief (that of the node's id)
        moved = np.any(x != x0, axis=1)
        if n == 0:
            assert not moved.any()
        assert refine_ref.transitions_valid(o, x, par_r, lambda k: int(oid_r[k] % np.uint64(B)), beliefs, moved)
        info = e.refine_info()
        assert info["total_s"] > 0.0 and (info["device_s"] > 0.0) == (n > 0 and any(len(p) >= 3 for p in refine_ref.decompose(par)[0]))
    assert_same(e.refine_policy(500), e.refine_policy(500))          # repeated calls on one context


def door_goal_behind_door_1(n, seed=0):
    c = cases.cfg_door(n, n, seed=seed)
    c.update(goals=[(0.5, 0.3)])
    return c


def test_grown_shelf_two_worlds(eng_mod):
    case = cases.cfg3_near(1500)
    check_grown(pipeline(eng_mod, case, 64, [0.5, 0.5]), case)


def test_grown_door_four_worlds(eng_mod):
    case = door_goal_behind_door_1(5000)
    check_grown(pipeline(eng_mod, case, 256, [0.0, 0.0, 0.4, 0.6]), case)


def test_grown_map4_three_seeds(eng_mod):
    """the reference's recorded problem (main.rs:893-908): refined at the drivers' 500 and 1500 iterations"""
    done = 0
    for seed in range(8):
        case = cases.cfg_map4(5000, seed)
        e = pipeline(eng_mod, case, 256, [1.0 / 16] * 16)
        try:
            e.extract_policy()
        except eng_mod.PorrtError:            # (the walk of belief_graph.rs:193-213 does not end on this graph)
            continue
        check_grown(e, case)
        done += 1
        if done == 3:
            break
    assert done == 3


def explicit(eng_mod, case_or_occ, xy, par, row, beliefs, n, stats=None):
    e = eng_mod.Engine()
    if isinstance(case_or_occ, np.ndarray):
        e.set_grid(case_or_occ, (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
        o = orc.Oracle()
        o.set_grid(case_or_occ, (-1.0, -1.0), (1.0, 1.0), orc.DOMAIN_SHELF)
    else:
        e = cases.configure(e, case_or_occ)
        o = cases.configure(orc.Oracle(), case_or_occ)
    xy = np.asarray(xy, dtype=np.float64)
    oid = np.arange(7, 7 + len(par), dtype=np.uint64)
    got = e.refine_policy_explicit(xy, par, oid, row, beliefs, n)
    want = refine_ref.refine(o, xy, par, oid, row, beliefs, n, stats)
    assert_same(got, want)
    return got, e


def test_shelf_low_obstacle_rejects_a_shortcut(eng_mod):
    """a path round a low shelf (map1_2_goals_like): the straight shortcut crosses LowObstacle, which state_validity / transition_validator
    refuse in the shelf domain (map_shelves_io.rs:464-488)"""
    path = [(0.8, 0.6), (0.88, 0.52), (0.92, 0.4), (0.93, 0.3), (0.9, 0.2), (0.8, 0.1)]
    stats = {}
    for n in (1, 500, 1500):
        st = {} if n != 500 else stats
        explicit(eng_mod, cases.cfg3_near(), path, np.arange(-1, len(path) - 1), np.zeros(len(path), dtype=np.uint32), [[0.5, 0.5]], n, st)
    assert stats.get("low", 0) > 0 and stats.get("commits", 0) > 0


def test_door_the_belief_forbids(eng_mod):
    """door_map_like: the path goes through door 1 and over the inner wall; the straight shortcut would cross door 0.  Under a belief in
    which door 0 may be closed the refiner refuses it (compatibility, common.rs:266-276); with both doors known open it takes it"""
    path = [(-0.5, -0.4), (-0.1, -0.35), (0.3, -0.3), (0.47, -0.2), (0.47, 0.2), (0.45, 0.7), (0.1, 0.8), (-0.2, 0.75), (-0.45, 0.6), (-0.5, 0.3)]
    beliefs = [[0.0, 0.0, 0.5, 0.5], [0.0, 0.0, 0.0, 1.0]]
    par = np.arange(-1, len(path) - 1)
    res = []
    for b in (0, 1):
        stats = {}
        got, _ = explicit(eng_mod, cases.cfg_door(), path, par, np.full(len(path), b, dtype=np.uint32), beliefs, 500, stats)
        res.append(got)
        if b == 0:
            assert stats.get("belief", 0) > 0
    assert res[1][1] < res[0][1]                                   # the open door gives the shorter path


def zigzag(n, x0=-0.9, x1=0.9, y=-0.85, amp=0.02):
    xs = np.linspace(x0, x1, n)
    return np.stack([xs, y + amp * (np.arange(n) % 2)], axis=1)


def test_explicit_piece_longer_than_a_wave_and_the_lds_cap(eng_mod):
    """one piece of 100 nodes (more than 64: several passes of the lanes) and one of 1100 (more than kRefineLdsNodes: global memory)"""
    occ = np.full((100, 100), 255, dtype=np.uint8)
    occ[:70, 49:51] = 0
    for m, n in ((100, 300), (1100, 60)):
        xy = zigzag(m)
        got, e = explicit(eng_mod, occ, xy, np.arange(-1, m - 1), np.zeros(m, dtype=np.uint32), [[1.0]], n)
        assert e.refine_info()["device_s"] > 0.0
        assert not np.array_equal(got[0][0], xy)


def test_explicit_small_pieces_and_the_one_node_quirk(eng_mod):
    """pieces of 1, 2 and 3 nodes; a one-node piece that branches (its successors stay unconnected, it becomes a leaf); a root that
    branches at once; nodes the walk from the root does not reach are dropped"""
    occ = np.full((100, 100), 255, dtype=np.uint8)
    occ[:70, 49:51] = 0
    path = [(-0.6, 0.6), (-0.5, 0.2), (-0.3, -0.2), (-0.25, -0.6), (-0.1, -0.75), (0.0, -0.8), (0.1, -0.75), (0.25, -0.6),
            (0.3, -0.2), (0.45, 0.1), (0.5, 0.4), (0.6, 0.6)]
    xy = list(path) + [(0.6, 0.7), (0.7, 0.6), (0.75, 0.55), (0.7, 0.7), (0.72, 0.8), (0.74, 0.75), (0.76, 0.82), (0.65, 0.75)]
    par = np.array(list(range(-1, 11)) + [11, 11, 13, 11, 15, 16, 17, 15])
    for n in (0, 1, 500):
        (x, oid, p, leaf), cost = explicit(eng_mod, occ, xy, par, np.zeros(len(par), dtype=np.uint32), [[1.0]], n)[0]
        assert p[16] == -1 and p[19] == -1 and leaf[15] == 1
    root = [(0.0, 0.0), (0.1, 0.1), (0.2, 0.3), (0.3, 0.2), (-0.1, 0.1), (-0.2, 0.2), (0.5, 0.5)]
    (x, oid, p, leaf), cost = explicit(eng_mod, occ, root, np.array([-1, 0, 1, 2, 0, 4, 3]), np.zeros(7, dtype=np.uint32), [[1.0]], 50)[0]
    assert list(p) == [-1, -1, 1, 2, 3, -1, 5] and cost == 0.0
    # three beliefs: the root piece in one, the branches in the others (an observation's outcomes); nodes 5 and 6, parents of each
    # other and not reached from the root, are dropped
    b2 = [[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]]
    case = cases.cfg3_near()
    xyb = [(-0.5, -0.9), (-0.4, -0.8), (-0.3, -0.9), (-0.2, -0.8), (-0.1, -0.9), (0.0, -0.8), (0.1, -0.9), (0.2, -0.8)]
    parb = np.array([-1, 0, 1, 2, 2, 6, 5, 4])
    rows = np.array([0, 0, 0, 1, 2, 0, 0, 2], dtype=np.uint32)
    (x, oid, p, leaf), cost = explicit(eng_mod, case, xyb, parb, rows, b2, 200)[0]
    assert len(x) == 6 and 5 not in oid - 7 and 6 not in oid - 7


def test_stale_policy_is_an_error(eng_mod):
    case = cases.cfg3_near(1500)
    e = cases.configure(eng_mod.Engine(), case)
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policy(10)                                    # nothing grown
    cases.grow(e, case, K=64)
    e.build_belief_graph([0.5, 0.5])
    e.compute_expected_costs()
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policy(10)                                    # no policy extracted yet
    e.extract_policy()
    first = e.refine_policy(500)
    cases.grow(e, case, K=64)                                  # regrown: the policy is gone
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policy(500)
    e.build_belief_graph([0.5, 0.5])
    e.compute_expected_costs()
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policy(500)
    e.extract_policy()
    e.refine_policy(500)
    e.build_belief_graph([0.9, 0.1])                           # a new belief graph: stale until extract_policy runs again
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policy(500)
    e.compute_expected_costs()
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policy(500)
    (oid, par, leaf), _ = e.extract_policy()
    (x, oid_r, _, _), _ = e.refine_policy(500)
    assert np.array_equal(np.sort(oid_r), np.sort(oid))        # the new policy's nodes, not the old one's
    assert first[0][0].shape[1] == 2


def test_plan_refines_like_the_engine(eng_mod):
    """pto_c.rs:217-218: plan() with refine_iterations = 500 reports the refined paths and cost, and the time it took"""
    import test_pto_c_shim as shim_t
    L = shim_t.shim()
    case = cases.cfg3_near(1500)
    case.update(n_iter_max=60000)
    belief = [0.5, 0.5]
    p = shim_t.configure(L, case, belief, seed=0)
    assert L.set_refine_parameters(p, C.c_size_t(500)) == 0
    assert L.plan(p, shim_t.dbl(list(case.start)), C.c_size_t(2)) == 0, L.po_rrt_last_error(p)
    e = cases.configure(eng_mod.Engine(), case)
    e.set_discrete_seed(0)
    cases.grow(e, case, K=256)
    e.build_belief_graph(belief)
    e.compute_expected_costs()
    e.extract_policy()
    (x, oid, par, leaf), cost = e.refine_policy(500)
    n, lens, ecost = C.c_size_t(0), C.POINTER(C.c_size_t)(), C.c_double(0)
    assert L.get_paths_info(p, C.byref(n), C.byref(lens), C.byref(ecost)) == 0
    leaves = np.nonzero(leaf)[0]
    assert n.value == len(leaves) and ecost.value == cost
    for i, k in enumerate(leaves):
        path = []
        while k >= 0:
            path.append(x[k])
            k = par[k]
        path = path[::-1]
        assert lens[i] == len(path)
        for s, st in enumerate(path):
            ptr, size = C.POINTER(C.c_double)(), C.c_size_t(0)
            assert L.get_paths_variable(p, C.c_size_t(i), C.c_size_t(s), C.byref(ptr), C.byref(size)) == 0
            assert ptr[0] == st[0] and ptr[1] == st[1]
    it, g, b, d, r, t = C.c_size_t(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
    assert L.get_planning_metrics(p, C.byref(it), C.byref(g), C.byref(b), C.byref(d), C.byref(r), C.byref(t)) == 0
    assert r.value > 0.0 and t.value >= r.value
    L.delete_planning_problem(p)
