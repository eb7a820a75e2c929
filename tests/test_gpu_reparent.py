"""GPU parity of the Reparent strategy (porrt_bg_reparent_policies / porrt_bg_reparent_policy / porrt_reparent_policies,
porrt_reparent.hpp): every policy is compared bit for bit (states as uint64, original ids, parents, leafs, status, expected cost) with
the restatement tests/reparent_ref.py applied to it alone."""
import numpy as np
import pytest

import cases
import refine_policies_cases as rp
import reparent_cases as rc
import reparent_ref as rr
from oracle import orc
from reparent_cases import GROWN_SEEDS, door_case, shelf_case

pytestmark = pytest.mark.gpu

BOTH = [[1.0], [0.0]]          # the belief rows of the one-world cases: row 1 only where a case asks for it


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def assert_same(got, want):
    (x, oid, par, leaf), cost = got
    (x2, oid2, par2, leaf2), cost2 = want
    assert x.shape == x2.shape and np.array_equal(x.view(np.uint64), x2.view(np.uint64)), "states differ"
    assert np.array_equal(oid, oid2) and np.array_equal(par, par2) and np.array_equal(leaf, leaf2)
    assert np.float64(cost).view(np.uint64) == np.float64(cost2).view(np.uint64), (cost, cost2)


def merged(case_list, beliefs=BOTH):
    """the graphs of the cases side by side as one graph, and their policies over it"""
    xy, row, children, pols, at = [], [], [], [], 0
    for c in case_list:
        n = len(c.G.xy)
        xy += c.G.xy.tolist()
        row += c.G.belief_row.tolist()
        children += [[at + k for k in c.G.children(g)] for g in range(n)]
        pols.append((np.asarray(c.ids, dtype=np.uint64) + np.uint64(at), np.asarray(c.parents, dtype=np.int64)))
        at += n
    return rr.Graph.of_lists(xy, np.asarray(row, dtype=np.uint32), beliefs, children), pols


def run(e, G, pols, radius):
    return e.reparent_policies_explicit(G.xy, G.belief_row, G.beliefs, G.child_off, G.child_ids, pols, radius)


def check(e, o, G, pols, radius, **caps):
    """the batch against the restatement of every policy, and against every policy run alone; returns the answers and the statuses"""
    got, status = run(e, G, pols, radius)
    info = e.reparent_policies_info()
    stats = {}
    for q, (ids, par) in enumerate(pols):
        st, want = rr.refine(o, G, ids, par, radius, stats=stats, **caps)
        assert status[q] == st, "policy %d: status %d, restated %d" % (q, status[q], st)
        if st == 0:
            assert_same(got[q], want)
        else:
            assert got[q] is None
    for q, pol in enumerate(pols):
        one, st1 = run(e, G, [pol], radius)
        assert st1[0] == status[q]
        if status[q] == 0:
            assert_same(one[0], got[q])
    return got, status, info, stats


@pytest.fixture(scope="module")
def wall(eng_mod):
    e, o = eng_mod.Engine(), orc.Oracle()
    e.set_grid(rp.wall_raster(), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    o.set_grid(rp.wall_raster(), (-1.0, -1.0), (1.0, 1.0), orc.DOMAIN_SHELF)
    return e, o


def test_hand_built_graphs_alone_and_in_one_batch(wall):
    e, o = wall
    cs = [make() for make in rc.HAND]
    G, pols = merged(cs)
    got, status, info, stats = check(e, o, G, pols, 0.3)       # one radius for the batch: the cases' geometry at 0.3
    assert not status.any()
    for c, make in zip(cs, rc.HAND):                           # and every case on its own graph with its own radius
        one, st = run(e, c.G, [(c.ids, c.parents)], c.radius)
        s1, want = rc.restate(o, c)
        assert st[0] == s1 == 0, make.__name__
        assert_same(one[0], want)
    c = rc.two_node_piece_grows()
    one, _ = run(e, c.G, [(c.ids, c.parents)], c.radius)
    assert list(one[0][0][1]) == [0, 2, 1]                     # the piece grew
    c = rc.one_node_piece_branches()
    one, _ = run(e, c.G, [(c.ids, c.parents)], c.radius)
    assert list(one[0][0][2]) == [-1, -1, 1, -1, 3]            # the quirk


def info_matches(info, stats, pols, status):
    assert info["policies"] == len(pols) and info["ok"] == int((np.asarray(status) == 0).sum())
    for k in ("tree_nodes", "max_tree", "pairs", "pops", "reparents"):
        assert info[k] == stats.get(k, 0), (k, info[k], stats.get(k, 0))


@pytest.mark.parametrize("n_tree", [1, 2, 63, 64, 65])
def test_tree_sizes_around_a_wave(wall, n_tree):
    e, o = wall
    c = rc.star(n_tree - 1)
    got, status, info, stats = check(e, o, c.G, [(c.ids, c.parents)], c.radius)
    assert status[0] == 0 and info["max_tree"] == n_tree and info["pieces"] == 1
    info_matches(info, stats, [0], status)
    assert info["pairs"] == n_tree * n_tree                    # all within each other's reach


def test_long_children_list_duplicate_child_and_many_neighbours(wall):
    e, o = wall
    cs = [rc.star(100), rc.star(10, dup=True), rc.path_with_star(70, 70)]
    G, pols = merged(cs)
    got, status, info, stats = check(e, o, G, pols, 0.3)
    assert not status.any() and info["max_tree"] == 140 and info["tree_nodes"] == 101 + 11 + 140
    info_matches(info, stats, pols, status)
    assert info["pairs"] >= 101 * 101                          # 101 valid neighbours per node of the first tree


def test_trees_on_both_sides_of_the_lds_limit(wall):
    """the pop loop keeps (parent, cost, priority) in LDS up to 1024 nodes and in global memory beyond; the tube has no such limit"""
    e, o = wall
    for n in (1024, 1025):
        c = rc.long_zigzag(n)
        got, status, info, stats = check(e, o, c.G, [(c.ids, c.parents)], c.radius)
        assert status[0] == 0 and info["max_tree"] == n and info["reparents"] > n // 2
        info_matches(info, stats, [0], status)
        assert len(got[0][0][1]) < n                           # the skips shortened it


def test_copies_and_radius_zero(wall):
    e, o = wall
    c = rc.copies(40)
    pol = [(c.ids, c.parents)]
    got, status, info, stats = check(e, o, c.G, pol, c.radius)
    assert status[0] == 0 and info["max_tree"] == 43 and stats["tied_pops"] > 30
    info_matches(info, stats, pol, status)
    got, status, info, stats = check(e, o, c.G, pol, 0.0)      # only zero-distance children and copies take part
    assert status[0] == 0 and info["max_tree"] == 43 and info["pairs"] == 2 + 41 * 41
    c = rc.lattice()
    got, status, info, stats = check(e, o, c.G, [(c.ids, c.parents)], 0.0)
    assert status[0] == 0 and info["max_tree"] == len(c.ids) and list(got[0][0][1]) == list(c.ids)


def test_wall_inside_the_radius(wall):
    e, o = wall
    c = rc.wall_in_range()
    got, status, info, stats = check(e, o, c.G, [(c.ids, c.parents)], c.radius)
    assert status[0] == 0 and info["max_tree"] == 5 and info["pairs"] < 25
    info_matches(info, stats, [0], status)


def test_every_status_beside_status_zero(wall):
    e, o = wall
    cs = [rc.grandchild_skip(), rc.leaves_raster(), rc.star(300), rc.mixed_piece(), rc.stale_priority(), rc.lattice()]
    G, pols = merged(cs)
    pols.insert(2, (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)))
    try:
        e.set_option("reparent_max_tree_nodes", 70)
        e.set_option("reparent_max_pops_per_node", 1)
        got, status, info, stats = check(e, o, G, pols, 0.4, max_tree_nodes=70, pops_per_node=1)
        assert list(status) == [0, 2, 1, 4, 3, 5, 0]
        run(e, G, pols, 0.4)
        assert "policy 1" in e._l.porrt_last_error(e._c).decode()
        z = rc.long_zigzag(100)                                # a tree of exactly the cap passes, one node more does not
        for cap, want in ((100, 0), (99, 4)):
            e.set_option("reparent_max_tree_nodes", cap)
            assert run(e, z.G, [(z.ids, z.parents)], z.radius)[1][0] == want == rc.restate(o, z, max_tree_nodes=cap)[0]
        e.set_option("reparent_max_tree_nodes", 353)           # 301 nodes fit, their 301 x 301 pairs in range do not (256 x 353 = 90 368)
        assert run(e, G, [pols[3]], 0.4)[1][0] == 4 == rr.refine(o, G, *pols[3], 0.4, max_tree_nodes=353)[0]
        e.set_option("reparent_max_tree_nodes", 354)           # 256 x 354 hold them
        assert run(e, G, [pols[3]], 0.4)[1][0] == 0 == rr.refine(o, G, *pols[3], 0.4, max_tree_nodes=354)[0]
        e.set_option("reparent_max_tree_nodes", 70)
        e.set_option("reparent_max_pops_per_node", 2)
        assert run(e, G, [pols[5]], 0.4)[1][0] == 0
    finally:
        e.set_option("reparent_max_tree_nodes", 16384)
        e.set_option("reparent_max_pops_per_node", 64)
    assert e.get_option("reparent_max_tree_nodes") == 16384 and e.get_option("reparent_max_pops_per_node") == 64


def test_more_pieces_than_a_round_and_an_output_longer_than_the_input(wall):
    """at the largest cap a round holds fewer than 80 pieces (1 GiB of slots of about 40 MiB), and every piece here comes out one node longer than it went in: the pool of
    recomposed rows is grown after the first round and again, with the earlier rounds' rows kept, after the later ones"""
    e, o = wall
    G, pols = merged([rc.two_node_piece_grows()] * 80)
    _, want = rr.refine(o, G, *pols[0], 0.8)
    try:
        e.set_option("reparent_max_tree_nodes", 1 << 15)
        got, status = run(e, G, pols, 0.8)
        info = e.reparent_policies_info()
    finally:
        e.set_option("reparent_max_tree_nodes", 16384)
    assert not status.any() and info["rounds"] >= 2 and info["nodes"] == 240 and info["pieces"] == 80
    for q, g in enumerate(got):
        (x, oid, par, leaf), cost = g
        assert_same(((x, oid - np.uint64(3 * q), par, leaf), cost), want)


def test_refused_inputs(wall, eng_mod):
    e, o = wall
    c = rc.grandchild_skip()
    G = c.G
    ok = [(c.ids, c.parents)]
    assert run(e, G, ok, 0.3)[1][0] == 0
    bad = eng_mod.PorrtError
    for radius in (-0.1, float("nan"), float("inf")):
        with pytest.raises(bad):
            run(e, G, ok, radius)
    with pytest.raises(bad):                                   # an id out of range
        run(e, G, [([4], [-1])], 0.3)
    for par in ([0], [-1, 2], [-1, 1]):                        # parents out of range, or a row 0 that is no root
        with pytest.raises(bad):
            run(e, G, [(list(range(len(par))), par)], 0.3)
    xy = G.xy.copy()
    xy[2, 0] = np.inf
    with pytest.raises(bad):                                   # a state that is not finite
        e.reparent_policies_explicit(xy, G.belief_row, G.beliefs, G.child_off, G.child_ids, ok, 0.3)
    with pytest.raises(bad):                                   # two worlds on a context of one
        e.reparent_policies_explicit(G.xy, G.belief_row, [[0.5, 0.5]], G.child_off, G.child_ids, ok, 0.3)
    with pytest.raises(bad):                                   # a child id out of range
        e.reparent_policies_explicit(G.xy, G.belief_row, G.beliefs, G.child_off, np.array([1, 2, 9], dtype=np.uint32), ok, 0.3)
    for name, value in (("reparent_max_tree_nodes", 0), ("reparent_max_tree_nodes", (1 << 15) + 1), ("reparent_max_pops_per_node", 65)):
        with pytest.raises(bad):
            e.set_option(name, value)
    got, status = run(e, G, [], 0.3)
    assert got == [] and len(status) == 0


def test_tube_crosses_into_other_beliefs(eng_mod):
    case = cases.cfg3_near()
    e, o = cases.configure(eng_mod.Engine(), case), cases.configure(orc.Oracle(), case)
    c = rc.crosses_beliefs()
    got, status, info, stats = check(e, o, c.G, [(c.ids, c.parents)], c.radius)
    assert status[0] == 0 and info["max_tree"] == 4
    (xy, oid, par, leaf), cost = got[0]
    assert list(oid) == [0, 2, 1]                              # through O, which carries belief [1, 0]
    assert cost == 0.5 * rr.norm2(xy[0], xy[1]) + 0.5 * rr.norm2(xy[1], xy[2])


def test_door_the_belief_is_not_compatible_with(eng_mod):
    case = cases.cfg_door()
    e, o = cases.configure(eng_mod.Engine(), case), cases.configure(orc.Oracle(), case)
    shut, open_ = rc.door_two_beliefs()
    pols = [(shut.ids, shut.parents), (open_.ids, open_.parents)]
    got, status, info, stats = check(e, o, shut.G, pols, shut.radius)
    assert not status.any() and got[1][1] < got[0][1]          # the belief that has door 0 open goes through it
    assert list(got[1][0][1]) == [10, 19]
    pairs = []
    for pol in pols:
        run(e, shut.G, [pol], shut.radius)
        pairs.append(e.reparent_policies_info()["pairs"])
    assert pairs[0] < pairs[1]                                 # the belief that has door 0 open may cross it


class Grown:
    """a grown pipeline, its policies from node 0 and drawn starts, and the restatement of each (computed once per radius; at 0.3 the 31
    restatements are nearly all of the test's 5-7 s: trees of hundreds of nodes in Python, the device call itself takes milliseconds)"""

    def __init__(self, eng_mod, case, prior, n_random=30, seed=7):
        self.e = e = cases.configure(eng_mod.Engine(), case)
        cases.grow(e, case, K=64)
        e.build_belief_graph(prior)
        e.compute_expected_costs()
        self.o = cases.configure(orc.Oracle(), case)
        d = e.expected_costs()
        finite = np.flatnonzero(np.isfinite(d) & (np.arange(len(d)) > 0))
        rng = np.random.default_rng(seed)
        self.starts = [0] + sorted(rng.choice(finite, size=n_random, replace=False).tolist())
        if not np.isfinite(d).all():                           # one start without a finite cost: no policy from there
            self.starts.insert(5, int(np.flatnonzero(~np.isfinite(d))[0]))
        self.pols, self.ext_status = e.extract_policies(self.starts)
        self.beliefs, _, (self.coff, self.cid), _ = e.belief_graph()
        self.G = rr.Graph.implicit(e.tree()[0], self.beliefs, self.coff, self.cid)
        self._want, self.cache = {}, {}                        # (the heap queue: the faster of the restatement's two, tests/test_reparent_cpu.py)

    def want(self, radius):
        if radius not in self._want:
            self._want[radius] = [None if p is None else rr.refine(self.o, self.G, p[0][0], p[0][1], radius, queue="heap", cache=self.cache) for p in self.pols]
        return self._want[radius]

    def check(self, radius):
        e = self.e
        off, status, cost, xy, oid, par, leaf = e.reparent_policies_raw(radius)
        got, status2 = e.reparent_policies(radius)             # a second call on the same context
        assert np.array_equal(status, status2) and len(got) == len(self.starts) and off[0] == 0 and off[-1] == len(xy)
        n_ok = 0
        for q, want in enumerate(self.want(radius)):
            a, b = int(off[q]), int(off[q + 1])
            if want is None:
                assert self.ext_status[q] != 0 and status[q] == 1 and got[q] is None and a == b and cost[q] == 0.0
                continue
            assert status[q] == want[0] == 0
            assert_same(got[q], want[1])
            assert_same(((xy[a:b], oid[a:b], par[a:b], leaf[a:b]), cost[q]), want[1])
            n_ok += 1
        return got, n_ok


@pytest.fixture(scope="module", params=[(d, s) for d in ("door", "shelf") for s in GROWN_SEEDS[d][:1]], ids=lambda p: "%s-%d" % p)
def grown(eng_mod, request):
    domain, seed = request.param
    return Grown(eng_mod, *(door_case if domain == "door" else shelf_case)(seed))


@pytest.mark.parametrize("radius", [0.3, 0.05])
def test_grown_pipeline(grown, radius):
    got, n_ok = grown.check(radius)
    assert n_ok >= 20
    e = grown.e
    info = e.reparent_policies_info()
    assert info["policies"] == len(grown.starts) and info["ok"] == n_ok and info["reparents"] > 0 and info["max_tree"] > 1
    assert info["ms_tube"] > 0.0 and info["ms_neighbours"] > 0.0 and info["ms_pop"] > 0.0 and info["ms_wall"] >= info["ms_pop"]
    e.extract_policy()
    assert_same(e.reparent_policy(radius), got[0])             # the single call: a batch of one
    assert e.reparent_policies_info() == info                  # ... that leaves the batch's info alone
    pols = [(p[0][0], p[0][1]) if p is not None else (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)) for p in grown.pols]
    G = grown.G
    exp, status = e.reparent_policies_explicit(G.xy, G.belief_row, G.beliefs, G.child_off, G.child_ids, pols, radius)
    for a, b in zip(exp, got):                                 # the explicit form fed with belief_graph()'s own arrays
        assert (a is None) == (b is None)
        if a is not None:
            assert_same(a, b)


def test_shortcut_refinement_is_not_disturbed(grown):
    e = grown.e
    before, st0 = e.refine_policies(100)
    e.reparent_policies(0.3)
    after, st1 = e.refine_policies(100)
    assert np.array_equal(st0, st1)
    for a, b in zip(before, after):
        assert (a is None) == (b is None)
        if a is not None:
            assert_same(a, b)


def test_kept_result_and_staleness(eng_mod):
    import ctypes as C
    case, prior = shelf_case(GROWN_SEEDS["shelf"][0], 1500)
    e = cases.configure(eng_mod.Engine(), case)
    with pytest.raises(eng_mod.PorrtError):
        e.reparent_policies(0.3)                               # nothing grown
    cases.grow(e, case, K=64)
    e.build_belief_graph(prior)
    e.compute_expected_costs()
    with pytest.raises(eng_mod.PorrtError):
        e.reparent_policies(0.3)                               # no extract_policies yet
    with pytest.raises(eng_mod.PorrtError):
        e.reparent_policy(0.3)                                 # no extract_policy yet
    starts = [0, 3, 17]
    e.extract_policies(starts)
    off, status, cost, xy, oid, par, leaf = e.reparent_policies_raw(0.3)
    n = len(oid)
    assert n > 0 and status[0] == 0

    def kept(cap):
        off2, st2, cost2 = np.zeros(len(starts) + 1, dtype=np.uint64), np.zeros(len(starts), dtype=np.uint8), np.zeros(len(starts))
        xy2, oid2, par2, leaf2 = np.zeros((n, 2)), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        m = int(e._l.porrt_bg_get_reparented_policies(e._c, p(off2), p(st2), p(cost2), p(xy2), p(oid2), p(par2), p(leaf2), cap))
        return m, (off2, st2, cost2, xy2, oid2, par2, leaf2)

    m, arrays = kept(n)
    assert m == n and all(np.array_equal(a, b) for a, b in zip(arrays, (off, status, cost, xy, oid, par, leaf)))
    m, arrays = kept(n - 1)                                    # too small: the total comes back, the node arrays stay untouched
    assert m == n and not arrays[4].any() and np.array_equal(arrays[0], off)

    def stale():
        assert kept(n)[0] < 0
        with pytest.raises(eng_mod.PorrtError):
            e.reparent_policies(0.3)

    cases.grow(e, case, K=64)                                  # regrown
    stale()
    e.build_belief_graph(prior)
    e.compute_expected_costs()
    stale()
    e.extract_policies(starts)
    e.reparent_policies(0.3)
    assert kept(1 << 20)[0] > 0
    e.build_belief_graph([0.9, 0.1])                           # a new belief graph
    stale()
    e.compute_expected_costs()
    stale()
    e.extract_policies(starts)
    e.reparent_policies(0.3)
    e.compute_expected_costs()                                 # new costs
    stale()
    with pytest.raises(eng_mod.PorrtError):
        e.reparent_policy(0.3)
