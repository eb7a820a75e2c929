"""GPU parity of the batch refiner (porrt_bg_refine_policies / porrt_mm_refine_policies / porrt_refine_policies,
porrt_refine_batch.hpp): every policy of a batch is compared bit for bit (states, original ids, parents, leafs, expected cost) with
the restatement tests/refine_ref.py applied to it alone, and with the single-policy calls on the same arrays."""
import numpy as np
import pytest

import cases
import refine_policies_cases as rp
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


def door_goal_behind_door_1(n, seed=0):
    c = cases.cfg_door(n, n, seed=seed)
    c.update(goals=[(0.5, 0.3)])
    return c


class Grown:
    """a grown pipeline, its policies from `starts` and the restatement of each (computed once per iteration count)"""

    def __init__(self, eng_mod, case, K, prior, n_random, seed, with_infinite):
        self.e = e = pipeline(eng_mod, case, K, prior)
        self.o = cases.configure(orc.Oracle(), case)
        d = e.expected_costs()
        finite = np.flatnonzero(np.isfinite(d) & (np.arange(len(d)) > 0))
        rng = np.random.default_rng(seed)
        self.starts = [0] + sorted(rng.choice(finite, size=n_random, replace=False).tolist())
        if with_infinite:
            assert not np.isfinite(d).all(), "the case was chosen for its belief nodes without a finite cost"
            self.starts.insert(5, int(np.flatnonzero(~np.isfinite(d))[0]))
        self.pols, self.ext_status = e.extract_policies(self.starts)
        self.xy = e.tree()[0]
        self.beliefs = e.belief_graph(lists=False)[0]
        self.B = len(self.beliefs)
        self._want = {}

    def arrays(self, q):
        (oid, par, leaf), _ = self.pols[q]
        return (self.xy[(oid // np.uint64(self.B)).astype(np.int64)], par, oid, (oid % np.uint64(self.B)).astype(np.uint32))

    def want(self, n):
        if n not in self._want:
            self._want[n] = [None if p is None else rp.restate(self.o, self.arrays(q), self.beliefs, n) for q, p in enumerate(self.pols)]
        return self._want[n]

    def check(self, n):
        e = self.e
        off, status, cost, xy, oid, par, leaf = e.refine_policies_raw(n)
        got, status2 = e.refine_policies(n)
        assert np.array_equal(status, status2) and len(got) == len(self.starts) and off[0] == 0 and off[-1] == len(xy)
        n_ok = 0
        for q, want in enumerate(self.want(n)):
            a, b = int(off[q]), int(off[q + 1])
            if want is None:                                   # the extraction gave no policy from there
                assert self.ext_status[q] != 0 and status[q] == 1 and got[q] is None and a == b and cost[q] == 0.0
                continue
            assert status[q] == 0 and b - a == len(want[0][0])
            assert_same(got[q], want)
            assert_same(((xy[a:b], oid[a:b], par[a:b], leaf[a:b]), cost[q]), want)
            assert_same(got[q], e.refine_policy_explicit(*self.arrays(q), self.beliefs, n))
            n_ok += 1
        e.extract_policy()
        assert_same(got[0], e.refine_policy(n))                # start 0: the single-policy pair on the context
        return n_ok, status


@pytest.fixture(scope="module")
def shelf(eng_mod):
    return Grown(eng_mod, cases.cfg3_near(1500), 64, [0.5, 0.5], 30, 7, True)


@pytest.mark.parametrize("n", [0, 1, 500])
def test_grown_shelf_two_worlds(shelf, n):
    n_ok, status = shelf.check(n)
    assert n_ok >= 20 and status[5] == 1                       # the start without a finite cost


def test_refine_policies_info(shelf):
    e = shelf.e
    got, status = e.refine_policies(500)
    info = e.refine_policies_info()
    pols = [rp.policy(np.zeros((0, 2)), []) if p is None else shelf.arrays(q) for q, p in enumerate(shelf.pols)]
    want = rp.info_of(pols, status)
    assert {k: info[k] for k in want} == want
    assert want["shortcut_pieces"] > 0 and info["ms_device"] > 0.0 and info["ms_wall"] >= info["ms_device"]
    e.refine_policies(0)                                       # nothing is shortcut without iterations
    info = e.refine_policies_info()
    assert info["ms_device"] == 0.0 and info["shortcut_pieces"] == 0 and info["pieces"] == want["pieces"] and info["nodes"] == want["nodes"]


def test_grown_door_four_worlds(eng_mod):
    g = Grown(eng_mod, door_goal_behind_door_1(5000), 256, [0.0, 0.0, 0.4, 0.6], 15, 11, False)
    assert len(g.starts) == 16
    n_ok, _ = g.check(500)
    assert n_ok >= 8
    compat = refine_ref.compatibility(np.asarray(g.beliefs), g.o.validities())
    roots = {tuple(compat[int(p[0][0][0] % np.uint64(g.B))]) for p in g.pols if p is not None}
    assert len(roots) >= 2, "the policies start under beliefs with the same compatibility bits"


def test_multi_modal(eng_mod):
    """every policy of the batch against the single-policy call on the same arrays AND against refine_ref on the policy that
    policies_ref walks on the ORACLE's growth from the same start"""
    import mm_plan_ref
    import policies_ref
    c = cases.cfg2(10)
    c.update(zones="map_benchmark_like_2_goals_zone_ids", visibility=0.5)
    case = cases.Case(c, seed=0)
    e = cases.configure(eng_mod.Engine(), case)
    o = cases.configure(orc.Oracle(), case)
    e.set_discrete_seed(0)
    o.set_discrete_seed(0)
    e.grow_mm_prm(case.start, [0.5, 0.5], 0.1, 2.0, 1000)
    _, bg, dist = mm_plan_ref.plan(o, case.start, [0.5, 0.5], 0.1, 2.0, 1000)
    e.mm_build_belief_graph()
    d = e.mm_expected_costs()
    assert np.array_equal(d.view(np.uint64), dist.view(np.uint64))
    finite = np.flatnonzero(np.isfinite(d) & (np.arange(len(d)) > 0))
    starts = [0] + sorted(np.random.default_rng(5).choice(finite, size=5, replace=False).tolist())
    G = policies_ref.graph_of_lists(bg["xy"], bg["belief_vec"], bg["beliefs"], bg["belief_ids"], bg["children"])
    walked = policies_ref.extract_policies(G, dist, starts)
    pols, ext_status = e.mm_extract_policies(starts)
    assert ext_status.tolist() == [w[0] for w in walked]
    got, status = e.mm_refine_policies(500)
    assert len(got) == len(starts) and status[0] == 0
    e.mm_extract_policy()
    assert_same(got[0], e.mm_refine_policy(500))
    n_ok = 0
    for q in range(len(starts)):
        if pols[q] is None:
            assert status[q] == 1 and got[q] is None
            continue
        (oid, par, leaf, xy), _ = pols[q]
        row = bg["belief_vec"][oid.astype(np.int64)]
        assert_same(got[q], e.refine_policy_explicit(xy, par, oid, row, bg["beliefs"], 500))
        oid_o, par_o, _ = walked[q][1]
        i = oid_o.astype(np.int64)
        assert_same(got[q], rp.restate(o, (bg["xy"][i], par_o, oid_o, bg["belief_vec"][i]), bg["beliefs"], 500))
        n_ok += 1
    assert n_ok >= 3


def batch_state(e, mm=False):
    """what the getters hand out of the last batched calls: the policies' node arrays, porrt_policies_info, porrt_refine_policies_info"""
    import ctypes as C
    get = (lambda *a: e._l.porrt_mm_get_policies(e._c, *a)) if mm else (lambda *a: e._l.porrt_bg_get_policies(e._c, *a))
    n = int(get(*([None] * (4 if mm else 3)), 0))
    assert n > 0
    arrays = [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint8)] + ([np.zeros((n, 2))] if mm else [])
    assert int(get(*[a.ctypes.data_as(C.c_void_p) for a in arrays], n)) == n
    return [a.tobytes() for a in arrays], e.policies_info(), e.refine_policies_info()


def test_single_calls_leave_the_batch_state_alone(shelf):
    """extract_policy() and refine_policy() are batches of one with results of their own: what the last batched calls left stays"""
    e = shelf.e
    try:
        pols, status = e.extract_policies([0] + [s for s, p in zip(shelf.starts[1:], shelf.pols[1:]) if p is not None][:2])
        refined, rstatus = e.refine_policies(50)
        assert list(status) == [0, 0, 0] and list(rstatus) == [0, 0, 0]
        before = batch_state(e)
        single, cost = e.extract_policy()
        single_refined = e.refine_policy(50)
        assert batch_state(e) == before
        assert all(np.array_equal(a, b) for a, b in zip(single, pols[0][0])) and cost == pols[0][1]
        assert_same(single_refined, refined[0])
    finally:
        e.extract_policies(shelf.starts)                       # what the other tests of this module refine


def test_multi_modal_single_calls_leave_the_batch_state_alone(eng_mod):
    """the same for mm_extract_policy() / mm_refine_policy() on the two-goal case of test_multi_modal"""
    c = cases.cfg2(10)
    c.update(zones="map_benchmark_like_2_goals_zone_ids", visibility=0.5)
    case = cases.Case(c, seed=0)
    e = cases.configure(eng_mod.Engine(), case)
    e.set_discrete_seed(0)
    e.grow_mm_prm(case.start, [0.5, 0.5], 0.1, 2.0, 1000)
    e.mm_build_belief_graph()
    d = e.mm_expected_costs()
    finite = np.flatnonzero(np.isfinite(d) & (np.arange(len(d)) > 0))
    pols, status = e.mm_extract_policies([0] + sorted(np.random.default_rng(5).choice(finite, size=2, replace=False).tolist()))
    refined, rstatus = e.mm_refine_policies(50)
    assert status[0] == 0 and rstatus[0] == 0
    before = batch_state(e, mm=True)
    single, cost = e.mm_extract_policy()
    single_refined = e.mm_refine_policy(50)
    assert batch_state(e, mm=True) == before
    assert all(np.array_equal(a, b) for a, b in zip(single, pols[0][0])) and cost == pols[0][1]
    assert_same(single_refined, refined[0])


def engine_and_oracle(eng_mod, case_or_occ):
    e, o = eng_mod.Engine(), orc.Oracle()
    if isinstance(case_or_occ, np.ndarray):
        e.set_grid(case_or_occ, (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
        o.set_grid(case_or_occ, (-1.0, -1.0), (1.0, 1.0), orc.DOMAIN_SHELF)
        return e, o
    return cases.configure(e, case_or_occ), cases.configure(o, case_or_occ)


def check_explicit(e, o, pols, beliefs, n):
    got, status = e.refine_policies_explicit(pols, beliefs, n)
    for q, pol in enumerate(pols):
        assert status[q] == 0, "policy %d: status %d" % (q, status[q])
        assert_same(got[q], rp.restate(o, pol, beliefs, n))
    return got


def test_explicit_shelf_raster_low_shelf_and_unreachable_nodes(eng_mod):
    e, o = engine_and_oracle(eng_mod, cases.cfg3_near())
    pols = [rp.policy(rp.LOW_SHELF_PATH, rp.chain(6)), rp.unreachable_nodes()]
    for n in (1, 500):
        got = check_explicit(e, o, pols, rp.SHELF_BELIEFS, n)
        assert len(got[1][0][0]) == 6 and 5 not in got[1][0][1] - 7 and 6 not in got[1][0][1] - 7
    assert_same(got[0], e.refine_policy_explicit(*pols[0], rp.SHELF_BELIEFS, 500))


def test_explicit_door_raster_one_path_under_two_beliefs(eng_mod):
    """the same states with different belief rows in one call: the belief that keeps door 0 shut refuses the shortcut through it"""
    e, o = engine_and_oracle(eng_mod, cases.cfg_door())
    k = len(rp.DOOR_PATH)
    pols = [rp.policy(rp.DOOR_PATH, rp.chain(k), np.full(k, b)) for b in (0, 1)]
    got = check_explicit(e, o, pols, rp.DOOR_BELIEFS, 500)
    assert got[1][1] < got[0][1] and not np.array_equal(got[0][0][0], got[1][0][0])


@pytest.fixture(scope="module")
def wall(eng_mod):
    return engine_and_oracle(eng_mod, rp.wall_raster())


def test_explicit_wall_raster_small_pieces_and_long_ones(wall):
    """pieces of 1, 2 and 3 nodes, the one-node quirk, a root that branches at once, policies of one and two nodes, a piece longer
    than a wave and one longer than the LDS array -- one batch"""
    e, o = wall
    pols = [rp.small_pieces(), rp.root_branches_at_once(), rp.policy([(0.1, -0.7)], [-1]), rp.policy([(0.1, -0.7), (0.2, -0.6)], [-1, 0]),
            rp.zigzag(100), rp.zigzag(1100)]
    for n in (0, 60):
        got = check_explicit(e, o, pols, [[1.0]], n)
        (x, oid, p, leaf), cost = got[0]
        assert p[16] == -1 and p[19] == -1 and leaf[15] == 1
        assert list(got[1][0][2]) == [-1, -1, 1, 2, 3, -1, 5] and got[1][1] == 0.0
        assert len(got[2][0][0]) == 1 and got[2][1] == 0.0 and len(got[3][0][0]) == 2
    assert not np.array_equal(got[4][0][0], pols[4][0]) and not np.array_equal(got[5][0][0], pols[5][0])
    assert e.refine_policies_info()["distinct_lengths"] == 5   # 12, 3, 4, 100, 1100


def test_lengths_at_the_lds_limits_in_both_launch_forms(wall):
    """pieces of exactly and one more than the short launch's LDS array (256) and the long launch's (1024): bit-equal with option
    refine_short_lds on (two launches by length class, the default) and off (one launch)"""
    e, o = wall
    pols = [rp.zigzag(m) for m in (256, 257, 1024, 1025)] + [rp.small_pieces()]
    want = [rp.restate(o, pol, [[1.0]], 40) for pol in pols]
    assert e.get_option("refine_short_lds") == 1
    try:
        for opt in (0, 1):
            e.set_option("refine_short_lds", opt)
            got, status = e.refine_policies_explicit(pols, [[1.0]], 40)
            assert not status.any()
            for g, w in zip(got, want):
                assert_same(g, w)
    finally:
        e.set_option("refine_short_lds", 1)
    assert not np.array_equal(want[0][0][0], pols[0][0]) and not np.array_equal(want[3][0][0], pols[3][0])


def test_explicit_repeats_and_order(wall):
    e, o = wall
    a, b, c = rp.small_pieces(), rp.zigzag(100), rp.bushy()
    got, status = e.refine_policies_explicit([a, b, a, c, a], [[1.0]], 300)
    assert not status.any()
    assert_same(got[0], rp.restate(o, a, [[1.0]], 300))
    assert_same(got[2], got[0])
    assert_same(got[4], got[0])
    rev, status = e.refine_policies_explicit([a, c, a, b, a], [[1.0]], 300)
    assert not status.any()
    for i, j in ((0, 4), (1, 3), (2, 2), (3, 1), (4, 0)):
        assert_same(rev[j], got[i])


def test_more_pieces_than_lanes_and_breadth_first_layout(wall):
    e, o = wall
    pols = [rp.comb(70), rp.bushy()]
    for n in (0, 200):
        got = check_explicit(e, o, pols, [[1.0]], n)
    assert len(got[0][0][0]) == 141 and got[0][0][3].all()
    assert list(got[1][0][1] - 7) == [0, 1, 2, 3, 4, 7, 10, 13, 5, 8, 11, 14, 16, 6, 9, 12, 15, 17, 19, 21, 18, 20, 22, 23, 24, 25]
    assert not np.array_equal(got[1][0][0], pols[1][0][(got[1][0][1] - 7).astype(np.int64)])


def test_a_fault_or_a_mixed_piece_stays_with_its_policy(eng_mod):
    e, o = engine_and_oracle(eng_mod, cases.cfg3_near())
    good1, good2 = rp.policy(rp.LOW_SHELF_PATH, rp.chain(6)), rp.unreachable_nodes()
    # a middle node left of and below the raster (a y above it would saturate to row 0, as in the reference: `high`): the first
    # iteration (s = 0, e = 2 is the only draw for three nodes) classifies a candidate that keeps one of its coordinates
    bad = rp.policy([(0.8, 0.6), (5.0, -5.0), (0.88, 0.52)], rp.chain(3))
    high = rp.policy([(0.8, 0.6), (5.0, 5.0), (0.88, 0.52)], rp.chain(3))
    mixed = rp.policy(rp.LOW_SHELF_PATH, rp.chain(6), [0, 0, 0, 1, 1, 1])       # one piece, two belief vectors
    got, status = e.refine_policies_explicit([good1, bad, good2, mixed, good1, high], rp.SHELF_BELIEFS, 500)
    assert list(status) == [0, 2, 0, 3, 0, 0] and got[1] is None and got[3] is None
    assert "policy 1" in e._l.porrt_last_error(e._c).decode()
    for q, pol in ((0, good1), (2, good2), (4, good1), (5, high)):
        assert_same(got[q], e.refine_policy_explicit(*pol, rp.SHELF_BELIEFS, 500))
        assert_same(got[q], rp.restate(o, pol, rp.SHELF_BELIEFS, 500))
    for pol in (bad, mixed):
        with pytest.raises(eng_mod.PorrtError):
            e.refine_policy_explicit(*pol, rp.SHELF_BELIEFS, 500)
    # two rows that hold the same vector are one belief, as in the single call (it compares the vectors)
    mixed2 = rp.policy(rp.LOW_SHELF_PATH, rp.chain(6), [0, 3, 0, 3, 0, 3])
    got, status = e.refine_policies_explicit([mixed2], rp.SHELF_BELIEFS + [[0.5, 0.5]], 500)
    assert status[0] == 0
    assert_same(got[0], rp.restate(o, good1, rp.SHELF_BELIEFS, 500))


def test_staleness_and_call_level_errors(eng_mod):
    case = cases.cfg3_near(1500)
    e = cases.configure(eng_mod.Engine(), case)
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies(10)                                  # nothing grown
    cases.grow(e, case, K=64)
    e.build_belief_graph([0.5, 0.5])
    e.compute_expected_costs()
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies(10)                                  # no extract_policies yet
    e.extract_policy()
    single = e.refine_policy(500)
    info = e.refine_info()
    starts = [0, 3, 17]
    e.extract_policies(starts)
    first, _ = e.refine_policies(500)
    assert e.refine_info() == info                             # the single pair's state is its own
    assert_same(e.refine_policy(500), single)
    assert_same(first[0], single)
    cases.grow(e, case, K=64)                                  # regrown
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies(500)
    e.build_belief_graph([0.5, 0.5])
    e.compute_expected_costs()
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies(500)
    e.extract_policies(starts)
    again, _ = e.refine_policies(500)
    e.extract_policy()
    assert_same(again[0], e.refine_policy(500))                # the regrown graph's policy (the samplers went on: not the first one's)
    e.build_belief_graph([0.9, 0.1])                           # a rebuilt belief graph
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies(500)
    e.compute_expected_costs()
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies(500)
    e.extract_policies(starts)
    e.compute_expected_costs()                                 # recomputed costs
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies(500)
    e.extract_policies(starts)
    e.refine_policies(500)
    # call-level errors of the explicit form: nothing is launched
    good = rp.policy(rp.LOW_SHELF_PATH, rp.chain(6))
    for par in ([-1, 0, 1, 2, 9, 4], [0, 0, 1, 2, 3, 4], [-1, 0, 1, -1, 3, 4], [-1, 0, 1, 3, 3, 4]):
        with pytest.raises(eng_mod.PorrtError):
            e.refine_policies_explicit([good, rp.policy(rp.LOW_SHELF_PATH, par)], rp.SHELF_BELIEFS, 10)
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies_explicit([rp.policy(rp.LOW_SHELF_PATH, rp.chain(6), np.full(6, 3))], rp.SHELF_BELIEFS, 10)
    with pytest.raises(eng_mod.PorrtError):
        e.refine_policies_explicit([good], rp.SHELF_BELIEFS, 1 << 31)
    got, status = e.refine_policies_explicit([], rp.SHELF_BELIEFS, 10)
    assert got == [] and len(status) == 0
    got, status = e.refine_policies_explicit([rp.policy(np.zeros((0, 2)), []), good, rp.policy(np.zeros((0, 2)), [])], rp.SHELF_BELIEFS, 10)
    assert list(status) == [1, 0, 1] and got[0] is None and got[2] is None
