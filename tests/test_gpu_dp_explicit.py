"""GPU parity of the general expected-cost sweeps (dp_run, k_dp_sweep, k_dp_set_finals; porrt_dp.hpp) on explicit belief graphs:
porrt_conditional_dijkstra on every input of tests/dp_graphs.py against the oracle's queue-driven conditional_dijkstra, bit for bit,
+inf included, and error for error.  tests/test_dp_graphs_cpu.py shows on the CPU what each input makes a sweep solver do (a chain one
sweep longer than a group, a cycle through a sum that converges over hundreds of sweeps, rows of thousands of children or parents, node
counts beside a block's edge, nodes that must never be evaluated).  Then the same call twice, permuted children lists, the policies from
the device's costs, and the implicit layout (option dp_sweeps) on random shelf worlds.  No malformed graph is fed to the device: the
argument checks are CPU tests (tests/test_abi_cpu.py)."""
import numpy as np
import pytest

import cases
import dp_graphs
import policies_ref as ref
from oracle import orc
from test_gpu_policies import assert_answers
from test_gpu_random_worlds import configure_pair, random_shelf_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def args(g):
    return g["xy"], g["belief_vec"], g["beliefs"], g["types"], g["children"], g["parents"], g["finals"]


_graphs, _oracle, _device = {}, {}, {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = dp_graphs.INPUTS[name]()
    return _graphs[name]


def oracle_dist(name):
    """the oracle's answer, computed once per input and shared (never written to)"""
    if name not in _oracle:
        _oracle[name] = orc.conditional_dijkstra(*args(graph(name)))[0]
        _oracle[name].setflags(write=False)
    return _oracle[name]


def device_dist(eng_mod, name):
    if name not in _device:
        _device[name] = eng_mod.conditional_dijkstra(*args(graph(name)))
    return _device[name]


@pytest.mark.parametrize("name", sorted(dp_graphs.INPUTS))
def test_device_equals_oracle(eng_mod, name):
    want = oracle_dist(name)                                       # (no input of this list makes the oracle raise: neither may the device)
    got = device_dist(eng_mod, name)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), \
        "%s: %d of %d costs differ, first at node %d" % (name, (bits(got) != bits(want)).sum(), len(want), int(np.flatnonzero(bits(got) != bits(want))[0]))


@pytest.mark.parametrize("which", dp_graphs.NEVER_EVALUATED)
def test_errors_fire_only_for_evaluated_nodes(eng_mod, which):
    """a node of type 0, or an observation node with an impossible child: no error while nothing below it becomes finite (the
    parametrised test above has both graphs), the reference's panic once a child does"""
    quiet = dp_graphs.never_evaluated(which, False)
    d = eng_mod.conditional_dijkstra(*args(quiet))
    assert np.array_equal(bits(d), bits(orc.conditional_dijkstra(*args(quiet))[0])) and np.isinf(d[2:]).all()
    loud = dp_graphs.never_evaluated(which, True)
    with pytest.raises(RuntimeError):
        orc.conditional_dijkstra(*args(loud))
    with pytest.raises(RuntimeError):
        eng_mod.conditional_dijkstra(*args(loud))
    d = eng_mod.conditional_dijkstra(*args(quiet))                  # and the failed call leaves nothing behind
    assert np.array_equal(bits(d), bits(orc.conditional_dijkstra(*args(quiet))[0]))


def test_the_same_call_twice_and_two_graphs_in_turn(eng_mod):
    """the entry owns no state: a second call, and calls on two graphs of different sizes alternately, give the same bits"""
    for name in ("contraction-0.9", "chain-17-down", "cyclic-400-12", "shaped-60-12"):
        a = eng_mod.conditional_dijkstra(*args(graph(name)))
        b = eng_mod.conditional_dijkstra(*args(graph(name)))
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(oracle_dist(name))), name
    for _ in range(3):
        for name in ("arbitrary-3000-12", "cyclic-120-3", "wide_rows", "arbitrary-257-12"):
            assert np.array_equal(bits(eng_mod.conditional_dijkstra(*args(graph(name)))), bits(oracle_dist(name))), name


@pytest.mark.parametrize("name", ["shaped-20-12", "shaped-60-64", "shaped-150-12", "arbitrary-3000-12", "cyclic-400-2"])
def test_permuted_children(eng_mod, name):
    """every children list shuffled, parents rebuilt.  A min does not mind; for the sums the oracle decides, run on the permuted graph.
    A shaped graph's sums have two terms, and 0.0 + a + b commutes exactly: there nothing at all may change."""
    g = graph(name)
    rng = np.random.default_rng(11)
    h = dp_graphs.with_children(g, [[r[k] for k in rng.permutation(len(r))] for r in g["children"]])
    assert dp_graphs.is_transpose(h)
    moved = [u for u, t in enumerate(g["types"]) if t == dp_graphs.O and h["children"][u] != g["children"][u]]
    assert len(moved) >= 3                                          # sums whose terms come in another order
    want = orc.conditional_dijkstra(*args(h))[0]
    got = eng_mod.conditional_dijkstra(*args(h))
    assert np.array_equal(bits(got), bits(want))
    if name.startswith("shaped"):
        assert np.array_equal(bits(got), bits(oracle_dist(name)))


def policy_starts(n):
    return list(range(n)) if n <= 1500 else [0] + [int(s) for s in np.random.default_rng(n).choice(np.arange(1, n), 500, replace=False)]


def test_policies_from_the_device_costs(eng_mod):
    """porrt_extract_policies from the device's costs against the restatement: every node of a graph of up to 1 500 nodes as a start,
    else 500 seeded starts and node 0.  Walks that return to their own path (status 2) and failed asserts (3) occur, as the CPU test
    shows they do in the restatement's answers."""
    counts = np.zeros(5, dtype=np.int64)
    for name in sorted(dp_graphs.INPUTS):
        if not name.startswith(("shaped", "cyclic", "wide_rows")):
            continue
        g, d = graph(name), device_dist(eng_mod, name)
        starts = policy_starts(len(d))
        got, status = eng_mod.extract_policies_explicit(g["xy"], g["belief_vec"], g["beliefs"], g["belief_id"], g["children"], d, starts)
        G = ref.graph_of_lists(g["xy"], g["belief_vec"], g["beliefs"], g["belief_id"], g["children"])
        assert_answers(got, status, ref.extract_policies(G, oracle_dist(name), starts), name)
        counts += np.bincount(status, minlength=5)[:5]
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0 and counts[3] > 0, counts


@pytest.mark.parametrize("seed", [0, 1])
def test_general_sweeps_on_the_context_graph(eng_mod, seed):
    """k_dp_sweep<IMPLICIT = true>: the context's own belief graph of a random shelf world through option dp_sweeps, at a prior with
    one world at zero (beliefs the graph's nodes cannot all carry), against the oracle"""
    rng = np.random.default_rng(1000 + seed)
    a, z, goals = random_shelf_world(rng)
    assert len(goals) >= 3
    e, o = configure_pair(eng_mod, a, z, cases.SHELF, goals, 0.45, seed)
    start = (0.0, -0.9)
    re = e.grow(start, 0.05, 5.0, 1500, 1500, batch_K=64, mode=cases.PTO)
    ro = o.grow(start, 0.05, 5.0, 1500, 1500, batch_K=64, mode=cases.PTO, algo=orc.ALGO_BATCHED_KD)
    assert re == ro
    prior = rng.dirichlet(np.ones(len(goals)))
    prior[int(rng.integers(len(goals)))] = 0.0
    prior = list(prior / prior.sum())
    e.build_belief_graph(prior)
    o.build_belief_graph(prior)
    want = o.expected_costs()
    e.compute_expected_costs()
    layered, rows_layered = e.expected_costs(), e.dp_info()["sweep_rows"]
    e.set_option("dp_sweeps", 1)
    e.compute_expected_costs()
    got, info = e.expected_costs(), e.dp_info()
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(layered), bits(want))
    assert info["sweeps"] > 0 and info["sweep_rows"] == len(want) * info["sweeps"] and info["sweep_rows"] != rows_layered    # whole-graph sweeps ran
    assert np.isfinite(want).any() and (want > 0.0).any()
