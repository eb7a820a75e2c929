"""GPU tests of the QMDP policy extractor (porrt_qmdp_plan / porrt_qmdp_react / porrt_qmdp_costs, po_rrt_amd/csrc/porrt_qmdp.hpp)
against the literal restatement of src/qmdp_policy_extractor.rs in tests/qmdp_ref.py.  Bit equality throughout.

Iteration counts: the growth of a context case stops at the first check that finds the final set complete (n_iter_min small,
n_iter_max large) -- the smallest graph on which plan_qmdp succeeds; cfg4 runs the 5000 iterations its configuration names.  The
synthetic two-door map of cases.cfg_door() has a world in which the goal cannot be reached (its final set never completes, at any
iteration count): there plan_qmdp's error is what device and restatement must agree on, and it doubles as the reference's
test_when_grow_graph_doesnt_reach_goal (qmdp_policy_extractor.rs:214-238)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import qmdp_ref as Q
from oracle import orc

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. the reference's asserted vectors through porrt_qmdp_costs
@pytest.mark.parametrize("name", sorted(Q.KATS))
def test_kat_graphs(eng_mod, name):
    from po_rrt_amd import engine
    make, finals, want = Q.KATS[name]
    g = make()
    got = engine.qmdp_costs_explicit(g["xy"], g["node_validity"], g["validities"], g["children"], finals)
    assert same(got, want), (got, want)


# ---- 2. random explicit graphs at the widths where the lane grouping can go wrong
def random_graph(seed, n, nw):
    """directed edges from a seeded generator; node 1 without children, node 2 with 200 (n permitting), nodes 3, 4, 5 at one position
    and linked both ways (zero-length edges); up to 65 validity rows; random final sets, world nw - 1 (nw > 1) without any"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    children = [[] for _ in range(n)]
    if n >= 6:
        xy[4] = xy[3]
        xy[5] = xy[3]
        for u in range(n):
            if u != 1:
                children[u] = [int(v) for v in rng.integers(0, n, int(rng.integers(1, 9)))]
        children[2] = [int(v) for v in rng.integers(0, n, 200)]
        for a, b in ((3, 4), (4, 5), (3, 5)):
            children[a].append(b)
            children[b].append(a)
    elif n == 2:
        children = [[1], [0, 0]]
    n_val = min(65, max(1, n // 4 + 1))
    full = (1 << nw) - 1
    validities = [full] + [int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) & full for _ in range(n_val - 1)]
    node_validity = [int(v) for v in rng.integers(0, n_val, n)]
    finals = []
    for w in range(nw):
        if nw > 1 and w == nw - 1:
            finals.append([])
        else:
            finals.append(sorted({int(v) for v in rng.integers(0, n, int(rng.integers(1, 4)))}))
    return dict(xy=[tuple(p) for p in xy.tolist()], node_validity=node_validity, validities=validities, children=children), finals


@pytest.mark.parametrize("nw", [1, 2, 12, 16, 17, 33, 64])
@pytest.mark.parametrize("n", [1, 2, 300])
def test_random_explicit_graphs(eng_mod, n, nw):
    from po_rrt_amd import engine
    g, finals = random_graph(1000 * n + nw, n, nw)
    want = Q.costs_explicit(g, finals)
    got = engine.qmdp_costs_explicit(g["xy"], g["node_validity"], g["validities"], g["children"], finals)
    assert same(got, want)
    if n == 300:
        finite = np.isfinite(np.array(want))
        assert finite.any() and not finite.all()                 # the filter and the empty world leave +inf beside finite costs
        if nw > 1:
            assert not finite[nw - 1].any()


# ---- 3 / 4. the context path
def context_case(name):
    c = {"cfg3_k1": lambda: cases.cfg3(1, 100000), "cfg3_k256": lambda: cases.cfg3(1, 100000), "cfg4": lambda: cases.cfg4(n_iter_min=5000),
         "door": lambda: cases.cfg_door(300, 1000), "door_paper": lambda: cases.cfg_door(1, 100000, paper=True), "wide": cases.cfg_wide}[name]()
    if name == "wide":
        c.update(n_iter_min=1, n_iter_max=100000)
    return c, {"cfg3_k1": 1, "cfg3_k256": 256, "cfg4": 256, "door": 64, "door_paper": 64, "wide": 64}[name]


@functools.lru_cache(maxsize=None)
def grown(name):
    """engine with its graph grown, and the restatement fed from the engine's own getters (planned where the final set is complete)"""
    import po_rrt_amd
    case, K = context_case(name)
    e = cases.configure(po_rrt_amd.Engine(0), case)
    cases.grow(e, case, K=K)
    q = Q.from_planner(e)
    if e.is_final_set_complete():
        q.plan_qmdp()
        e.qmdp_plan()
    return e, q


@pytest.mark.parametrize("name", ["cfg3_k1", "cfg3_k256", "cfg4", "door_paper", "wide"])
def test_context_costs_equal_restatement(eng_mod, name):
    e, q = grown(name)
    assert e.is_final_set_complete()
    got = e.qmdp_costs()
    assert got.shape == (e.n_worlds(), e.num_nodes())
    assert same(got, q.cost_to_goals)
    info = e.qmdp_info()
    assert info["nodes"] == e.num_nodes() and info["worlds"] == e.n_worlds() and info["edges"] == sum(len(c) for c in q.children)
    assert info["sweeps"] >= 8 and info["sweeps"] % 8 == 0 and info["ms_plan_wall"] >= info["ms_plan_device"] > 0.0
    # every world has a final node of cost 0 and the root's cost is finite in the worlds that reach a goal
    assert all(min(row) == 0.0 for row in q.cost_to_goals)


def test_context_costs_from_the_oracles_arrays(eng_mod):
    """the same costs when the restatement is fed from the oracle's graph instead of the engine's getters"""
    e, _ = grown("door_paper")
    case, K = context_case("door_paper")
    o = cases.configure(orc.Oracle(), case)
    cases.grow(o, case, K=K, algo=orc.ALGO_BATCHED_KD)
    assert o.is_final_set_complete() and o.num_nodes() == e.num_nodes()
    q = Q.from_planner(o)
    q.plan_qmdp()
    assert same(e.qmdp_costs(), q.cost_to_goals)


def test_incomplete_final_set_is_the_references_error(eng_mod):
    """qmdp_policy_extractor.rs:214-238: a door map grown for 300 .. 1000 iterations; plan_qmdp().unwrap() panics"""
    e, q = grown("door")
    assert not e.is_final_set_complete() and 300 <= e.num_iterations() <= 1000
    with pytest.raises(ValueError, match="We should have final node ids for each world"):
        q.plan_qmdp()
    with pytest.raises(eng_mod.PorrtError, match="We should have final node ids for each world") as ei:
        e.qmdp_plan()
    assert ei.value.code == -1
    with pytest.raises(eng_mod.PorrtError):
        e.qmdp_costs()


# ---- 5. react
def make_queries(seed, nw, n=64, box=((-1.0, -1.0), (1.0, 1.0))):
    """random starts, Dirichlet beliefs of which a quarter have exact zeros (the NaN rule), horizons from {0, 0.2, 1, 10}"""
    rng = np.random.default_rng(seed)
    starts = rng.uniform(box[0], box[1], (n, 2))
    beliefs = rng.dirichlet(np.ones(nw), n)
    for k in range(0, n, 4):
        beliefs[k, rng.integers(0, nw, max(1, nw // 2))] = 0.0
        if beliefs[k].sum() == 0.0:
            beliefs[k, 0] = 1.0
        beliefs[k] /= beliefs[k].sum()
    horizons = rng.choice([0.0, 0.2, 1.0, 10.0], n)
    return starts, beliefs, horizons


def ref_answers(q, starts, beliefs, horizons):
    """per query: (paths, common_len), or the WalkTooLong the restatement raised"""
    out = []
    for s, b, h in zip(starts, beliefs, horizons):
        try:
            out.append(q.react_qmdp(s, b, h))
        except Q.WalkTooLong as err:
            out.append(err)
    return out


def check_react(eng_mod, e, q, starts, beliefs, horizons, min_share=0.75):
    want = ref_answers(q, starts, beliefs, horizons)
    good = [k for k, a in enumerate(want) if not isinstance(a, Q.WalkTooLong)]
    assert len(good) >= min_share * len(want), "only %d of %d queries are answered by the restatement" % (len(good), len(want))
    nw = e.n_worlds()
    # the answerable queries in one call
    paths, cl = e.qmdp_react(starts[good], beliefs[good], horizons[good], with_common_len=True)
    for k, pw, c in zip(good, paths, cl):
        ref_paths, ref_c = want[k]
        assert int(c) == ref_c, k
        for w in range(nw):
            assert same(pw[w].reshape(-1, 2), np.array(ref_paths[w], dtype=np.float64).reshape(-1, 2)), (k, w)
    # path_off through the C ABI
    off, cl2 = np.zeros(len(good) * nw + 1, dtype=np.uint64), np.zeros(len(good), dtype=np.uint64)
    s, b, h = (np.ascontiguousarray(a[good], dtype=np.float64) for a in (starts, beliefs, horizons))
    total = e._l.porrt_qmdp_react(e._c, s.reshape(-1), b.reshape(-1), nw, h, len(good), off, cl2, None, 0)
    assert off[0] == 0 and total == int(off[-1]) == sum(len(p) for pw in paths for p in pw) and np.array_equal(cl, cl2)
    # one by one: the same answers, and the device's error where the restatement raises
    for k, a in enumerate(want):
        if isinstance(a, Q.WalkTooLong):
            with pytest.raises(eng_mod.PorrtError, match="query 0") as ei:
                e.qmdp_react(starts[k:k + 1], beliefs[k:k + 1], horizons[k:k + 1])
            assert ei.value.code == -1 and ("common path" if a.world is None else "world %d" % a.world) in str(ei.value)
        elif k % 4 == 0:
            one, c1 = e.qmdp_react(starts[k:k + 1], beliefs[k:k + 1], horizons[k:k + 1], with_common_len=True)
            assert int(c1[0]) == a[1] and all(same(one[0][w].reshape(-1, 2), np.array(a[0][w], dtype=np.float64).reshape(-1, 2)) for w in range(nw))
    # all queries in one call: the first failing query is named
    bad = [k for k, a in enumerate(want) if isinstance(a, Q.WalkTooLong)]
    if bad:
        with pytest.raises(eng_mod.PorrtError, match="query %d[,:]" % bad[0]):
            e.qmdp_react(starts, beliefs, horizons)
    return want


REACT_SEEDS = {"cfg3_k256": 1, "door_paper": 1, "cfg4": 1}


def test_react_the_references_calls(eng_mod):
    """test_plan_on_map1_2_goals (:175-212): start (-0.8, -0.8), belief (0.5, 0.5), horizon 0.2; test_plan_on_map2_qmdp (:138-172):
    uniform belief, horizon 0.2, a start 0.2 above the root"""
    e, q = grown("cfg3_k256")
    want = check_react(eng_mod, e, q, np.array([[-0.8, -0.8]]), np.array([[0.5, 0.5]]), np.array([0.2]), 1.0)
    assert want[0][1] >= 1 and all(len(p) > want[0][1] for p in want[0][0])          # a common part, then a way of its own per world
    e, q = grown("door_paper")
    case, _ = context_case("door_paper")
    start = np.array([[case.start[0], case.start[1] + 0.2]])
    want = check_react(eng_mod, e, q, start, np.full((1, 16), 1.0 / 16.0), np.array([0.2]), 1.0)
    assert want[0][1] >= 1


@pytest.mark.parametrize("name", sorted(REACT_SEEDS))
def test_react_many_queries(eng_mod, name):
    e, q = grown(name)
    starts, beliefs, horizons = make_queries(REACT_SEEDS[name], e.n_worlds())
    want = check_react(eng_mod, e, q, starts, beliefs, horizons)
    assert any(not isinstance(a, Q.WalkTooLong) and a[1] > 1 for a in want)


# ---- 6. interface
def test_interface_rules(eng_mod):
    import po_rrt_amd
    case, K = context_case("cfg3_k1")
    e = cases.configure(po_rrt_amd.Engine(0), case)
    s, b, h = np.array([[-0.8, -0.8]]), np.array([[0.5, 0.5]]), np.array([0.2])
    with pytest.raises(eng_mod.PorrtError):
        e.qmdp_plan()                                            # no graph at all
    cases.grow(e, case, K=K)
    with pytest.raises(eng_mod.PorrtError, match="porrt_qmdp_plan"):
        e.qmdp_react(s, b, h)                                    # react before plan
    e.qmdp_plan()
    q = Q.from_planner(e)
    q.plan_qmdp()
    ref_paths, ref_c = q.react_qmdp(s[0], b[0], h[0])
    total_ref = sum(len(p) for p in ref_paths)
    # the cap = 0 sizing call writes offsets and common_len, no states; a cap that is too small writes none either
    off, cl = np.zeros(3, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    args = (e._c, s.reshape(-1), b.reshape(-1), 2, h, 1, off, cl)
    assert e._l.porrt_qmdp_react(*args, None, 0) == total_ref and list(off) == [0, len(ref_paths[0]), total_ref] and cl[0] == ref_c
    buf = np.full((total_ref + 1, 2), -7.0)
    assert e._l.porrt_qmdp_react(*args, buf.ctypes.data_as(C.c_void_p), total_ref - 1) == total_ref and np.all(buf == -7.0)
    assert e._l.porrt_qmdp_react(*args, buf.ctypes.data_as(C.c_void_p), total_ref) == total_ref
    assert same(buf[:total_ref], np.array(ref_paths[0] + ref_paths[1])) and np.all(buf[total_ref] == -7.0)
    # n = 0
    off0 = np.full(1, 9, dtype=np.uint64)
    assert e._l.porrt_qmdp_react(e._c, s.reshape(-1), b.reshape(-1), 2, h, 0, off0, cl, None, 0) == 0 and off0[0] == 0
    assert e.qmdp_react(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0)) == []
    # a wrong n_worlds: the reference's message
    with pytest.raises(eng_mod.PorrtError, match="belief state size should match the number of worlds"):
        e.qmdp_react(s, np.array([[0.5, 0.25, 0.25]]), h)
    # qmdp_max_states = 4 makes a long walk an error naming its query: the common path of 5 states, and with horizon 0 world 0's own walk
    assert ref_c > 4 and min(len(p) for p in ref_paths) - ref_c > 4
    e.set_option("qmdp_max_states", 4)
    assert e.get_option("qmdp_max_states") == 4
    q4 = Q.from_planner(e, max_states=4)
    q4.plan_qmdp()
    with pytest.raises(Q.WalkTooLong) as ri:
        q4.react_qmdp(s[0], b[0], h[0])
    assert ri.value.world is None
    with pytest.raises(eng_mod.PorrtError, match="query 0, common path"):
        e.qmdp_react(s, b, h)
    with pytest.raises(Q.WalkTooLong) as ri:
        q4.react_qmdp(s[0], b[0], 0.0)
    assert ri.value.world == 0
    with pytest.raises(eng_mod.PorrtError, match="query 0, world 0"):
        e.qmdp_react(s, b, np.array([0.0]))
    e.set_option("qmdp_max_states", 1 << 16)
    assert len(e.qmdp_react(s, b, h)[0][0]) == len(ref_paths[0])
    # plan, regrow, react: stale
    cases.grow(e, case, K=K)
    with pytest.raises(eng_mod.PorrtError, match="porrt_qmdp_plan"):
        e.qmdp_react(s, b, h)
    with pytest.raises(eng_mod.PorrtError):
        e.qmdp_costs()
    e.qmdp_plan()
    q2 = Q.from_planner(e)                                       # (the sampler went on: another graph)
    q2.plan_qmdp()
    assert same(e.qmdp_costs(), q2.cost_to_goals)
