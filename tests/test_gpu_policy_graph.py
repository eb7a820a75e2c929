"""GPU tests of get_policy_graph on the device (porrt_policy_graph / porrt_qmdp_policy_graph, po_rrt_amd/csrc/porrt_policy_graph.hpp)
against the restatement in tests/policy_graph_ref.py: keep and how equal entry for entry, pivots equal in total and in their maximum
(the interface reports pivots through its info), pruned children and parents lists equal to remove_edge applied in Python.

A context whose graph sends more than STEP3_SAMPLE entries to the simplex has steps 0-2 compared on all entries and step 3 on a
seeded sample of STEP3_SAMPLE residual entries (the restatement's simplex is a Python loop)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cases
import policy_graph_ref as P
import qmdp_ref as Q
from oracle import orc

pytestmark = pytest.mark.gpu
INF = float("inf")
STEP3_SAMPLE = 2000


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def check_explicit(children, costs):
    """device against restatement on an explicit graph: flags, classes, counts, pivots"""
    from po_rrt_amd import engine
    keep, how, info = engine.policy_graph_explicit(children, costs)
    rk, rh, rp = P.policy_graph(children, costs)
    assert np.array_equal(how, rh), np.nonzero(how != rh)[0][:10]
    assert np.array_equal(keep, rk)
    assert info["entries"] == len(rh) and info["kept"] == int(rk.sum())
    assert info["how"] == [int((rh == h).sum()) for h in range(6)]
    assert info["residual"] == int((rh >= 3).sum())
    assert info["pivots_total"] == int(rp.sum()) and info["pivots_max"] == (int(rp.max()) if len(rp) else 0)
    return how, info


# ---- 1. the reference's asserted answers through porrt_policy_graph
@pytest.mark.parametrize("name", sorted(P.KATS))
def test_kat_graphs(eng_mod, name):
    from po_rrt_amd import engine
    make, want = P.KATS[name]
    children, costs = make()
    keep, _, _ = engine.policy_graph_explicit(children, costs)
    got = P.pruned_children(children, keep)
    for node, cs in want.items():
        assert got[node] == cs, (node, got[node], cs)
    check_explicit(children, costs)


# ---- 2. random explicit graphs (the generator of test_gpu_qmdp.py::random_graph)
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
    g, finals = random_graph(1000 * n + nw, n, nw)
    check_explicit(g["children"], Q.costs_explicit(g, finals))


@pytest.mark.parametrize("nw", [1, 2, 12, 16, 17, 33, 64])
@pytest.mark.parametrize("n", [1, 2, 300])
def test_random_cost_tables(eng_mod, n, nw):
    """the same graphs over a random cost table with +inf entries.  Among node 2's 200 children no world is likely to have one child
    below all others and no child is above another in every world, so at 33 and 64 worlds most of its entries reach the simplex
    (the nodes with 1 to 8 children mostly end at the world shortcut)"""
    g, _ = random_graph(1000 * n + nw, n, nw)
    rng = np.random.default_rng(7000 * n + nw)
    costs = rng.uniform(0.0, 10.0, (nw, n))
    costs[rng.random((nw, n)) < 0.1] = INF
    how, _ = check_explicit(g["children"], costs)
    if n == 300 and nw >= 33:
        first = sum(len(c) for c in g["children"][:2])
        assert (how[first:first + 200] >= 3).sum() > 100


def test_copies_of_one_child(eng_mod):
    """a node whose children are all copies of one node has no rivals; one whose children are different nodes with identical cost rows
    has zero rows: every entry is kept by the world shortcut"""
    children = [[1] * 70, [], [], [2, 3] * 40, []]
    costs = [[5.0, 1.0, 2.0, 2.0, 0.0], [5.0, INF, 3.0, 3.0, 0.0]]
    how, _ = check_explicit(children, costs)
    assert (how == 1).all()


def test_empty_world_set(eng_mod):
    """an entry whose target is finite in no world is pruned by step 0, whatever its rivals are"""
    children = [[1, 2], [0], [0]]
    costs = [[1.0, INF, 2.0], [1.0, INF, INF]]
    how, _ = check_explicit(children, costs)
    assert how.tolist() == [0, 1, 1, 1]


# ---- 3. the context path
def context_case(name):
    c = {"cfg3_k256": lambda: cases.cfg3(1, 100000), "cfg4": lambda: cases.cfg4(n_iter_min=5000),
         "door_paper": lambda: cases.cfg_door(1, 100000, paper=True)}[name]()
    return c, {"cfg3_k256": 256, "cfg4": 256, "door_paper": 64}[name]


def grow_planned(name):
    import po_rrt_amd
    case, K = context_case(name)
    e = cases.configure(po_rrt_amd.Engine(0), case)
    cases.grow(e, case, K=K)
    assert e.is_final_set_complete()
    e.qmdp_plan()
    return e


def children_of(x):
    f, t, _ = x.edges()
    return Q.children_from_edges(x.num_nodes(), f, t)


def restated(children, costs, seed, max_pivots=P.MAX_PIVOTS):
    """the restatement with step 3 on all residual entries, or on a seeded sample of STEP3_SAMPLE of them (the others: how 255)"""
    keep, how, piv = P.policy_graph(children, costs, max_pivots=max_pivots, sample=(seed, STEP3_SAMPLE))
    return keep, how, piv, bool((how == 255).any())


@functools.lru_cache(maxsize=None)
def decided(name):
    e = grow_planned(name)
    e.qmdp_policy_graph()
    children = children_of(e)
    return e, children, e.qmdp_costs(), e.qmdp_policy_graph_get(), e.qmdp_policy_graph_info()


def compare(got, info, children, want):
    keep, how, piv, sampled = want
    done = how != 255
    assert np.array_equal(got["how"][done], how[done]), np.nonzero(done & (got["how"] != how))[0][:10]
    assert np.array_equal(got["keep"][done], keep[done])
    assert ((got["how"][~done] >= 3) & (got["how"][~done] <= 5)).all()
    assert info["entries"] == len(how) == sum(len(c) for c in children)
    assert info["how"][:3] == [int((how == h).sum()) for h in range(3)]
    assert info["residual"] == int((how >= 3).sum()) and info["kept"] == int(got["keep"].sum())
    assert sum(info["how"]) == info["entries"]
    if not sampled:
        assert info["how"] == [int((how == h).sum()) for h in range(6)]
        assert info["pivots_total"] == int(piv.sum()) and info["pivots_max"] == int(piv.max())
    return sampled


@pytest.mark.parametrize("name", ["cfg3_k256", "cfg4", "door_paper"])
def test_context_equals_restatement(eng_mod, name):
    e, children, costs, got, info = decided(name)
    sampled = compare(got, info, children, restated(children, costs, 5))
    print("%s: %d entries, how %s, residual %d (%s), pivots %d total, %d max" % (
        name, info["entries"], info["how"], info["residual"], "sample of %d" % STEP3_SAMPLE if sampled else "all restated",
        info["pivots_total"], info["pivots_max"]))
    assert info["ms_classify_wall"] >= info["ms_classify_device"] > 0.0 and info["ms_compact_device"] > 0.0


@pytest.mark.parametrize("name", ["cfg3_k256", "cfg4", "door_paper"])
def test_context_pruned_lists(eng_mod, name):
    """the pruned children and parents CSR against remove_edge (pto_graph.rs:214-217) applied in Python for the device's own flags;
    a PTO graph's parents[x] is its children[x] (every edge goes both ways and both entries are pushed together)"""
    e, children, _, got, _ = decided(name)
    ch, pa = P.remove_edges(children, children, got["keep"])
    for off, ids, want in ((got["child_off"], got["child_ids"], ch), (got["parent_off"], got["parent_ids"], pa)):
        assert off[0] == 0 and off[-1] == len(ids)
        assert [len(c) for c in want] == np.diff(off.astype(np.int64)).tolist()
        assert ids.tolist() == [i for c in want for i in c]
    assert ch == P.pruned_children(children, got["keep"])


def test_context_from_the_oracles_graph(eng_mod):
    """the same decisions when the restatement is fed from the oracle's graph and the restated dijkstras, not the engine's getters.
    The oracle lists the edges of one batch in another order than the engine, so the children lists are equal as multisets and the
    comparison is per edge (u, t): steps 0-2 do not depend on the order of the rivals, and the simplex's decision depends on it only
    through Bland's ties (its class, 3 or 4, is compared through keep)."""
    e, children, _, got, info = decided("door_paper")
    case, K = context_case("door_paper")
    o = cases.configure(orc.Oracle(), case)
    cases.grow(o, case, K=K, algo=orc.ALGO_BATCHED_KD)
    assert o.is_final_set_complete() and o.num_nodes() == e.num_nodes()
    q = Q.from_planner(o)
    q.plan_qmdp()
    assert [sorted(c) for c in q.children] == [sorted(c) for c in children]
    keep, how, _, _ = restated(q.children, q.cost_to_goals, 5)
    want, k = {}, 0
    for u, cs in enumerate(q.children):
        for t in cs:
            if how[k] != 255:
                want[(u, t)] = (int(how[k]), bool(keep[k]))
            k += 1
    k, seen = 0, 0
    for u, cs in enumerate(children):
        for t in cs:
            if (u, t) in want:
                h, kept = want[(u, t)]
                assert bool(got["keep"][k]) == kept and (h >= 3 or int(got["how"][k]) == h), (u, t, h, int(got["how"][k]))
                seen += 1
            k += 1
    assert seen >= len(want) >= info["how"][0] + info["how"][1] + info["how"][2] + STEP3_SAMPLE


# ---- 4. interface rules
def test_needs_a_plan_and_goes_stale(eng_mod):
    import po_rrt_amd
    case, K = context_case("cfg3_k256")
    e = cases.configure(po_rrt_amd.Engine(0), case)
    cases.grow(e, case, K=K)
    with pytest.raises(po_rrt_amd.engine.PorrtError):
        e.qmdp_policy_graph()                        # no porrt_qmdp_plan yet
    e.qmdp_plan()
    with pytest.raises(po_rrt_amd.engine.PorrtError):
        e.qmdp_policy_graph_info()                   # planned, not pruned yet
    e.qmdp_policy_graph()
    info = e.qmdp_policy_graph_info()
    assert info["entries"] == 2 * len(e.edges()[0])
    # every output of the getter may be NULL
    assert e._l.porrt_qmdp_policy_graph_get(e._c, None, None, None, None, None, None) == 0
    how = np.zeros(info["entries"], dtype=np.uint8)
    assert e._l.porrt_qmdp_policy_graph_get(e._c, None, how.ctypes.data_as(C.c_void_p), None, None, None, None) == 0
    assert np.array_equal(how, e.qmdp_policy_graph_get()["how"])
    cases.grow(e, case, K=K)                         # a new growth: plan and policy graph are stale
    for call in (e.qmdp_policy_graph, e.qmdp_policy_graph_get, e.qmdp_policy_graph_info):
        with pytest.raises(po_rrt_amd.engine.PorrtError):
            call()


def test_explicit_refusals_and_null_outputs(eng_mod):
    from po_rrt_amd import engine
    L = engine.load_library()
    off = np.array([0, 1, 2], dtype=np.uint64)
    ids = np.array([1, 0], dtype=np.uint32)

    def call(costs, nw, ids=ids):
        c = np.ascontiguousarray(costs, dtype=np.float64)
        return L.porrt_policy_graph(0, 2, nw, off, ids, c.ctypes.data_as(C.c_void_p), None, None, None)

    assert call([[1.0, 0.0]], 1) == 0                # keep, how and info NULL
    assert call([[float("nan"), 0.0]], 1) != 0
    assert call([[-INF, 0.0]], 1) != 0
    assert call([[1.0, 0.0]], 0) != 0
    assert call(np.zeros((65, 2)), 65) != 0
    assert call([[1.0, 0.0]], 1, ids=np.array([1, 2], dtype=np.uint32)) != 0
    with pytest.raises(RuntimeError):
        engine.policy_graph_explicit([[1], [0]], [[float("nan"), 0.0]])


def test_out_of_pivots_is_kept(eng_mod):
    """policy_graph_max_pivots = 1: an entry the simplex does not settle in one pivot is how 5, kept and counted, as in the
    restatement under the same cap"""
    e = grow_planned("cfg4")
    e.set_option("policy_graph_max_pivots", 1)
    assert e.get_option("policy_graph_max_pivots") == 1
    e.qmdp_policy_graph()
    got, info = e.qmdp_policy_graph_get(), e.qmdp_policy_graph_info()
    children = children_of(e)
    compare(got, info, children, restated(children, e.qmdp_costs(), 6, max_pivots=1))
    assert info["how"][5] > 0 and info["pivots_max"] == 1
    assert got["keep"][got["how"] == 5].all()


def test_cpp_mirror(eng_mod, tmp_path):
    """policy_graph() and PTO::get_policy_graph() of include/porrt.hpp, in a program of its own (tests/policy_graph_mirror.cpp)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "po_rrt_amd")
    exe = str(tmp_path / "policy_graph_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(root, "tests", "policy_graph_mirror.cpp"),
                    "-L" + lib, "-lporrt_hip", "-Wl,-rpath," + lib], check=True)
    case = cases.cfg3()
    out = subprocess.run([exe, os.path.join(cases.MAPS, case.grid + ".pgm"), os.path.join(cases.MAPS, case.zones + ".pgm")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "policy_graph_mirror ok" in out.stdout, out.stdout + out.stderr
