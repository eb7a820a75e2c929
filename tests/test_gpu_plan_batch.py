"""GPU parity of porrt_plan_belief_space_batch (porrt_plan_batch.hpp): PTO::plan_belief_space for many grown contexts in one call.
Every member's answer is compared exactly -- statuses, ids, parents, leaf flags, the bits of costs and states, the member's whole
cost vector -- with the single sequence on a FRESH context configured and grown alike: build_belief_graph, compute_expected_costs,
extract_policies([0]), refine_policies(n).  One scenario is also checked against the oracle and the restatements of the policy walk
and the refiner, so that the batch is not only compared with ourselves."""
import ctypes as C

import numpy as np
import pytest

import cases
import make_maps
import policies_ref
import refine_ref
from oracle import orc

pytestmark = pytest.mark.gpu

PRIOR4 = [0.1, 0.2, 0.3, 0.4]
PRIOR4_OPEN = [0.0, 0.0, 0.4, 0.6]                  # door 1 is open for sure: a goal just behind it has a finite expected cost
SIZES = (1500, 700, 1500, 300, 1100)                # node counts differ, so no offset is a round number


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def door_near(n, seed):
    """cfg_door with the goal just behind door 1: graphs of 1100 iterations and more reach it"""
    c = cases.cfg_door(n, n, seed=seed)
    c.update(goals=[(0.5, 0.15)])
    return c


def grown_batch(eng_mod, cs, K=64):
    es = [cases.configure(eng_mod.Engine(), c) for c in cs]
    eng_mod.Engine.grow_batch(es, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, [c.n_iter_min for c in cs], K, cases.PTO,
                              n_iter_max=[c.n_iter_max for c in cs])
    return es


def grown_single(eng_mod, c, K=64):
    e = cases.configure(eng_mod.Engine(), c)
    cases.grow(e, c, K=K)
    return e


def single_sequence(e, prior, n_refine=()):
    """what one context gives alone: the extraction from node 0, the whole cost vector, the belief edges, the refinements asked for"""
    e.build_belief_graph(prior)
    e.compute_expected_costs()
    off, status, cost, oid, par, leaf = e.extract_policies_raw([0])
    B = len(e.belief_graph(lists=False)[0])
    out = dict(status=int(status[0]), cost=cost[0], oid=oid, par=par, leaf=leaf, xy=e.tree()[0][(oid // np.uint64(B)).astype(np.int64)],
               dist=e.expected_costs(), edges=e.bg_num_edges(), B=B, nodes=e.num_nodes(), refined={})
    for n in n_refine:
        out["refined"][n] = e.refine_policies_raw(n)
    return out


def assert_member(raw, q, want, n_refine):
    """member q of a plan_belief_space_batch_raw answer against its single sequence"""
    off, status, cost, rstatus, rcost, xy, oid, par, leaf = raw
    a, b = int(off[q]), int(off[q + 1])
    assert status[q] == want["status"], "member %d: status %d, alone %d" % (q, status[q], want["status"])
    assert bits([cost[q]])[0] == bits([want["cost"]])[0], "member %d: root cost" % q
    if n_refine == 0:
        assert rstatus[q] == 1 and bits([rcost[q]])[0] == 0
        w_xy, w_oid, w_par, w_leaf = want["xy"], want["oid"], want["par"], want["leaf"]
    else:
        roff, rst, rc, w_xy, w_oid, w_par, w_leaf = want["refined"][n_refine]
        assert rstatus[q] == rst[0] and bits([rcost[q]])[0] == bits([rc[0]])[0], "member %d: refinement status / cost" % q
    assert b - a == len(w_oid), "member %d: %d policy nodes, alone %d" % (q, b - a, len(w_oid))
    assert np.array_equal(oid[a:b], w_oid) and np.array_equal(par[a:b], w_par) and np.array_equal(leaf[a:b], w_leaf), "member %d: policy" % q
    assert np.array_equal(bits(xy[a:b]), bits(w_xy)), "member %d: states" % q
    if status[q] != 0:
        assert a == b


class Scenario:
    """members grown by one grow_batch, and the single sequence of each on a fresh context grown by a single grow"""

    def __init__(self, eng_mod, cs, prior, n_refine=(200,), K=64):
        self.cs, self.prior = cs, prior
        self.es = grown_batch(eng_mod, cs, K)
        self.singles = [single_sequence(grown_single(eng_mod, c, K), prior, n_refine) for c in cs]
        for e, s in zip(self.es, self.singles):
            assert e.num_nodes() == s["nodes"]

    def check(self, eng_mod, n_refine, lead_options=()):
        for k, v in lead_options:
            self.es[0].set_option(k, v)
        raw = eng_mod.Engine.plan_belief_space_batch_raw(self.es, self.prior, n_refine)
        assert raw[0][0] == 0 and raw[0][-1] == len(raw[6])
        for q, want in enumerate(self.singles):
            assert_member(raw, q, want, n_refine)
        return raw


@pytest.fixture(scope="module")
def door5(eng_mod):
    """the five door contexts of different sizes (4 worlds); no graph reaches the far goal: every root cost is +inf"""
    return Scenario(eng_mod, [cases.cfg_door(n, n, seed=s) for s, n in enumerate(SIZES)], PRIOR4)


@pytest.fixture(scope="module")
def door5_near(eng_mod):
    """the same sizes with the goal just behind door 1 and a prior under which it is open: finite and infinite roots in one batch"""
    return Scenario(eng_mod, [door_near(n, s) for s, n in enumerate(SIZES)], PRIOR4_OPEN)


@pytest.mark.parametrize("n_refine", [0, 200])
@pytest.mark.parametrize("which", ["door5", "door5_near"])
def test_batch_equals_one_by_one(eng_mod, request, which, n_refine):
    sc = request.getfixturevalue(which)
    raw = sc.check(eng_mod, n_refine)
    lead = sc.es[0]
    info = lead.plan_batch_info()
    assert info["members"] == 5 and info["passes"] == 1 and info["beliefs"] == sc.singles[0]["B"]
    assert info["belief_edges"] == sum(s["edges"] for s in sc.singles)
    assert info["graph_nodes"] == sum(s["nodes"] for s in sc.singles) and info["belief_nodes"] == sum(s["nodes"] * s["B"] for s in sc.singles)
    assert info["policies_ok"] == int((raw[1] == 0).sum()) and info["policy_nodes"] == raw[0][-1]
    assert info["ms_wall"] > 0.0 and info["ms_wall"] >= info["ms_costs"] > 0.0
    for q, s in enumerate(sc.singles):                   # each member's whole cost vector
        assert np.array_equal(bits(lead.plan_batch_expected_costs(q)), bits(s["dist"])), "member %d: cost vector" % q
    ok = [s["status"] == 0 for s in sc.singles]
    if which == "door5_near":
        assert sum(ok) >= 2 and not all(ok), "the scenario was chosen for its mix of finite and infinite roots"
        assert all(len(s["oid"]) > 3 for s, k in zip(sc.singles, ok) if k)
    # the list form
    got = eng_mod.Engine.plan_belief_space_batch(sc.es, sc.prior, n_refine)
    for q, (st, cost, rst, rcost, pol) in enumerate(got):
        assert st == raw[1][q] and (pol is None) == (not ok[q])


def test_device_ranks_give_the_same_answers(eng_mod, door5_near):
    """option plan_batch_host_ranks = 0: the members' kd pre-order ranks from k_seg_kd_ranks, a workgroup per member"""
    try:
        door5_near.check(eng_mod, 200, [("plan_batch_host_ranks", 0)])
        assert door5_near.es[0].get_option("plan_batch_host_ranks") == 0
    finally:
        door5_near.es[0].set_option("plan_batch_host_ranks", 1)


def test_against_the_oracle(eng_mod):
    """two members on the shelf domain (2 worlds, finite root cost on a small graph): the oracle's growth, belief graph and expected
    costs, policies_ref.extract_policies from node 0 and refine_ref at 200 iterations"""
    cs = [cases.cfg3_near(1500, seed=s) for s in (0, 1)]
    prior = [0.5, 0.5]
    es = grown_batch(eng_mod, cs)
    raw0 = eng_mod.Engine.plan_belief_space_batch_raw(es, prior, 0)
    dists = [es[0].plan_batch_expected_costs(q) for q in range(2)]
    raw = eng_mod.Engine.plan_belief_space_batch_raw(es, prior, 200)
    off, status, cost, rstatus, rcost, xy, oid, par, leaf = raw
    for q, c in enumerate(cs):
        o = cases.configure(orc.Oracle(), c)
        cases.grow(o, c, K=64, algo=orc.ALGO_BATCHED_KD)
        o.build_belief_graph(prior)
        beliefs, types, (coff, cid), _ = o.belief_graph()
        d = o.expected_costs()
        assert np.array_equal(bits(dists[q]), bits(d)), "member %d: expected costs differ from the oracle's" % q
        G = policies_ref.context_graph(o.tree()[0], beliefs, coff, cid)
        (st, pol, c0), = policies_ref.extract_policies(G, d, [0])
        assert st == policies_ref.OK and np.isfinite(c0)
        assert status[q] == 0 and bits([cost[q]])[0] == bits([c0])[0]
        a, b = int(raw0[0][q]), int(raw0[0][q + 1])
        assert np.array_equal(raw0[6][a:b], pol[0]) and np.array_equal(raw0[7][a:b], pol[1]) and np.array_equal(raw0[8][a:b], pol[2])
        B = len(beliefs)
        p_oid, p_par = np.asarray(pol[0], dtype=np.uint64), np.asarray(pol[1], dtype=np.int64)
        p_xy = o.tree()[0][(p_oid // np.uint64(B)).astype(np.int64)]
        assert np.array_equal(bits(raw0[5][a:b]), bits(p_xy))
        (w_xy, w_oid, w_par, w_leaf), w_cost = refine_ref.refine(o, p_xy, p_par, p_oid, (p_oid % np.uint64(B)).astype(np.uint32), beliefs, 200)
        a, b = int(off[q]), int(off[q + 1])
        assert rstatus[q] == 0 and bits([rcost[q]])[0] == bits([w_cost])[0]
        assert np.array_equal(bits(xy[a:b]), bits(w_xy)) and np.array_equal(oid[a:b], w_oid) and np.array_equal(par[a:b], w_par)
        assert np.array_equal(leaf[a:b], w_leaf)


def test_degenerate_members_inside_a_batch(eng_mod):
    """between ordinary members: a context grown for one iteration (an all but empty segment in the middle of the union) and one whose
    goal lies behind the wall (incomplete final set, root cost +inf)"""
    one = cases.cfg_door(1, 1, seed=5)
    wall = cases.cfg_door(400, 400, seed=2)             # the far goal: no node reaches it in 400 iterations
    cs = [door_near(1500, 0), one, door_near(1100, 4), wall, door_near(1500, 2)]
    sc = Scenario(eng_mod, cs, PRIOR4_OPEN)
    for n in (0, 200):
        raw = sc.check(eng_mod, n)
        assert raw[1].tolist() == [0, 1, 0, 1, 0]
    e_one, e_wall = sc.es[1], sc.es[3]
    assert e_one.num_nodes() <= 2 and e_one.num_final() == 0 and len(e_one.edges()[0]) <= 1
    assert e_wall.num_nodes() > 300 and not e_wall.is_final_set_complete()
    assert np.isinf(sc.singles[3]["cost"]) and np.isinf(sc.singles[1]["cost"])
    assert all(np.isfinite(sc.singles[q]["cost"]) and len(sc.singles[q]["oid"]) > 3 for q in (0, 2, 4))


def own_state(e):
    n = int(e._l.porrt_bg_get_policies(e._c, None, None, None, 0))
    assert n > 0
    oid, par, leaf = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert e._l.porrt_bg_get_policies(e._c, p(oid), p(par), p(leaf), n) == n
    return oid, par, leaf, bits(e.expected_costs())


def kept_policies(lead, n_members):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    off = np.zeros(n_members + 1, dtype=np.uint64)
    total = int(lead._l.porrt_plan_batch_get_policies(lead._c, p(off), None, None, None, None, 0))
    assert total >= 0 and off[-1] == total
    xy, oid, par, leaf = np.zeros((total, 2)), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.uint8)
    assert lead._l.porrt_plan_batch_get_policies(lead._c, p(off), p(xy), p(oid), p(par), p(leaf), total) == total
    return off, xy, oid, par, leaf


def test_members_keep_their_own_state(eng_mod):
    cs = [door_near(1500, 0), door_near(1100, 4), door_near(1500, 2)]
    es = grown_batch(eng_mod, cs)
    m = es[1]
    m.build_belief_graph([0.0, 0.0, 0.5, 0.5])          # another prior than the batch's
    m.compute_expected_costs()
    rng = np.random.default_rng(5)
    starts = rng.integers(0, len(m.expected_costs()), size=50)
    _, st, _, _, _, _ = m.extract_policies_raw(starts)
    assert (st == 0).any()
    before = own_state(m)
    raw = eng_mod.Engine.plan_belief_space_batch_raw(es, PRIOR4_OPEN, 200)
    assert raw[1].tolist() == [0, 0, 0]
    after = own_state(m)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    kept = kept_policies(es[0], 3)
    cases.grow(m, cs[1], K=64)                           # the answers are snapshots: a regrowth of a member does not touch them
    again = kept_policies(es[0], 3)
    assert all(np.array_equal(a, b) for a, b in zip(kept, again))
    assert np.array_equal(kept[0], raw[0]) and np.array_equal(bits(kept[1]), bits(raw[5])) and np.array_equal(kept[2], raw[6])
    assert np.array_equal(kept[3], raw[7]) and np.array_equal(kept[4], raw[8])


def pass_count(sizes, limit):
    """the rule of join_pass_end: members in order while the sum stays at or below the limit, a member that alone exceeds it alone"""
    passes, acc = 0, None
    for s in sizes:
        if acc is None or acc + s > limit:
            passes, acc = passes + 1, s
        else:
            acc += s
    return passes


@pytest.mark.parametrize("n_refine", [0, 200])
def test_passes(eng_mod, door5_near, n_refine):
    sc = door5_near
    sizes = [s["nodes"] * s["B"] for s in sc.singles]
    three = [lim for lim in sorted({sum(sizes[i:j]) for i in range(5) for j in range(i + 1, 6)}) if pass_count(sizes, lim) == 3]
    assert three
    lead = sc.es[0]
    default = lead.get_option("plan_batch_max_belief_nodes")
    assert pass_count(sizes, default) == 1
    try:
        for limit, passes in ((three[0], 3), (1, 5)):
            sc.check(eng_mod, n_refine, [("plan_batch_max_belief_nodes", limit)])
            info = lead.plan_batch_info()
            assert info["passes"] == passes and info["belief_edges"] == sum(s["edges"] for s in sc.singles)
            with pytest.raises(eng_mod.engine.PorrtError):
                lead.plan_batch_expected_costs(0)                # its costs went with its pass
            assert np.array_equal(bits(lead.plan_batch_expected_costs(4)), bits(sc.singles[4]["dist"]))
    finally:
        lead.set_option("plan_batch_max_belief_nodes", default)


def six_door_map():
    """two rooms split by a wall with six doors: 64 worlds, some 700 reachable beliefs -- the tiled count kernels' path"""
    a = np.full((200, 200), 255, np.uint8)
    make_maps.rect(a, -1.0, 0.0, 1.0, 0.04, 0)
    for x in (-0.85, -0.55, -0.25, 0.05, 0.35, 0.65):
        make_maps.rect(a, x, 0.0, x + 0.12, 0.04, 128)
    z, k = make_maps.door_zone_ids(a)
    assert k == 6
    return a, z


def test_many_beliefs(eng_mod):
    occ, zones = six_door_map()
    prior = [1.0 / 64] * 64

    def make(seed):
        x = eng_mod.Engine()
        x.set_grid(occ, (-1.0, -1.0), (1.0, 1.0), cases.DOOR)
        x.set_zones(zones, 0.45)
        x.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
        x.set_square_goal(np.array([(-0.5, 0.6)]), np.array([(1 << 64) - 1], dtype=np.uint64), 0.05)
        return x
    es = [make(11), make(12)]
    eng_mod.Engine.grow_batch(es, [(0.5, -0.6)] * 2, 0.05, 5.0, [400, 250], 64, cases.PTO)
    singles = []
    for seed, n in ((11, 400), (12, 250)):
        x = make(seed)
        x.grow((0.5, -0.6), 0.05, 5.0, n, n, batch_K=64, mode=cases.PTO)
        singles.append(single_sequence(x, prior, (200,)))
    assert singles[0]["B"] >= 256 and singles[0]["nodes"] != singles[1]["nodes"]          # (the tiled kernels take 256 beliefs and more)
    for n in (0, 200):
        raw = eng_mod.Engine.plan_belief_space_batch_raw(es, prior, n)
        for q, want in enumerate(singles):
            assert_member(raw, q, want, n)
            assert np.array_equal(bits(es[0].plan_batch_expected_costs(q)), bits(want["dist"]))
    assert es[0].plan_batch_info()["belief_edges"] == sum(s["edges"] for s in singles)


def test_batch_of_one_and_members_grown_alone(eng_mod):
    """a batch of one, and contexts grown by single grow calls with different K in one batch"""
    cs = [door_near(1500, 0), door_near(1100, 4)]
    es = [grown_single(eng_mod, cs[0], 64), grown_single(eng_mod, cs[1], 1)]
    singles = [single_sequence(grown_single(eng_mod, cs[0], 64), PRIOR4_OPEN, (200,)), single_sequence(grown_single(eng_mod, cs[1], 1), PRIOR4_OPEN, (200,))]
    assert all(s["status"] == 0 for s in singles)
    for n in (0, 200):
        raw = eng_mod.Engine.plan_belief_space_batch_raw(es, PRIOR4_OPEN, n)
        for q, want in enumerate(singles):
            assert_member(raw, q, want, n)
        for q in (1, 0):                                        # either as a batch of one, led by itself
            one = eng_mod.Engine.plan_belief_space_batch_raw([es[q]], PRIOR4_OPEN, n)
            assert_member(one, 0, singles[q], n)
            assert es[q].plan_batch_info()["members"] == 1
            assert np.array_equal(bits(es[q].plan_batch_expected_costs(0)), bits(singles[q]["dist"]))


def test_refusals(eng_mod):
    E = eng_mod.Engine
    err = eng_mod.engine.PorrtError
    cs = [door_near(1500, 0), door_near(1100, 4)]
    es = grown_batch(eng_mod, cs)
    lead = es[0]

    def refused(engines, prior, text):
        with pytest.raises(err) as x:
            E.plan_belief_space_batch_raw(engines, prior, 0)
        assert x.value.code == -1 and text in str(x.value), str(x.value)
        with pytest.raises(err):
            engines[0].plan_batch_info()                         # refused before anything ran: no answers on the leader
    refused([lead, es[1], lead], PRIOR4_OPEN, "twice")
    rrt = cases.cfg2(500)
    e_rrt = cases.configure(E(), rrt)
    cases.grow(e_rrt, rrt, K=64)
    refused([lead, e_rrt], PRIOR4_OPEN, "PTO")
    shelf = cases.cfg3(300, 300)
    e_shelf = cases.configure(E(), shelf)
    cases.grow(e_shelf, shelf, K=64)
    refused([lead, e_shelf], PRIOR4_OPEN, "raster")
    other = door_near(300, 2)
    other.update(visibility=0.35)
    e_vis = cases.configure(E(), other)
    cases.grow(e_vis, other, K=64)
    refused([lead, e_vis], PRIOR4_OPEN, "visibility")
    refused(es, [0.5, 0.25, 0.25], "per world")
    refused(es, [0.0, 0.0, 0.4, 0.5], "sum to 1")
    L, p = lead._l, (lambda a: a.ctypes.data_as(C.c_void_p))
    arr = (C.c_void_p * 2)(es[0]._c, es[1]._c)
    b = np.array(PRIOR4_OPEN)
    off, st, cost = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.uint8), np.zeros(2)
    for outs in ((None, p(st), p(cost)), (p(off), None, p(cost)), (p(off), p(st), None)):
        assert L.porrt_plan_belief_space_batch(arr, 2, p(b), 4, 0, outs[0], outs[1], outs[2], None, None, None, None, None, None, 0) == -1
    assert L.porrt_plan_belief_space_batch(arr, 2, None, 4, 0, p(off), p(st), p(cost), None, None, None, None, None, None, 0) == -1
    with pytest.raises(err):
        lead.plan_batch_info()
    # no members: 0, pol_off[0] written
    off[0] = 7
    assert L.porrt_plan_belief_space_batch(arr, 0, p(b), 4, 0, p(off), None, None, None, None, None, None, None, None, 0) == 0 and off[0] == 0
    # the sizing call returns the total with pol_off filled; the getter with room fills the arrays; so does the call itself
    total = int(L.porrt_plan_belief_space_batch(arr, 2, p(b), 4, 0, p(off), p(st), p(cost), None, None, None, None, None, None, 0))
    assert total > 6 and off[0] == 0 and off[2] == total and st.tolist() == [0, 0]
    kept = kept_policies(lead, 2)
    assert np.array_equal(kept[0], off)
    cap = total + 3
    xy, oid, par, leaf = np.zeros((cap, 2)), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.uint8)
    rst, rc = np.zeros(2, dtype=np.uint8), np.ones(2)
    assert L.porrt_plan_belief_space_batch(arr, 2, p(b), 4, 0, p(off), p(st), p(cost), p(rst), p(rc), p(xy), p(oid), p(par), p(leaf), cap) == total
    assert np.array_equal(bits(xy[:total]), bits(kept[1])) and np.array_equal(oid[:total], kept[2]) and np.array_equal(par[:total], kept[3])
    assert rst.tolist() == [1, 1] and bits(rc).tolist() == [0, 0]
