"""porrt_solutions / Engine.solutions() (RRT::get_solutions, rrt.rs:195-246, on the device: DESIGN.md section 21) against the
restatement tests/solutions_ref.py on the oracle's tree, bit for bit: ids, path states, costs."""
import numpy as np
import pytest

import cases
import solutions_ref as S
from oracle import orc

pytestmark = pytest.mark.gpu

START = (0.0, -1.0)


@pytest.fixture(scope="module")
def po():
    import po_rrt_amd
    return po_rrt_amd


def _setup(eng, zones, seed=0):
    eng.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    eng.set_zones(cases.load_map(zones), 0.5)
    eng.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return eng


def _same(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(g[1]).view(np.uint64), np.ascontiguousarray(w[1]).view(np.uint64))
        assert np.float64(g[2]).view(np.uint64) == np.float64(w[2]).view(np.uint64)


def _grow_pair(po, zones, goal, start, n_iter_min, n_iter_max, K):
    e, o = _setup(po.Engine(0), zones), _setup(orc.Oracle(), zones)
    for x in (e, o):
        if goal[0] == "observation":
            x.set_observation_goal(goal[1])
        else:
            x.set_square_goal(np.array([o.zone_positions()[goal[1]]]), np.array([1], dtype=np.uint64), 0.05)
    e.grow(start, 0.1, 2.0, n_iter_min, n_iter_max, batch_K=K)
    o.grow(start, 0.1, 2.0, n_iter_min, n_iter_max, batch_K=K, algo=orc.ALGO_BATCHED_KD if K > 1 else orc.ALGO_SEQ)
    return e, o


@pytest.mark.parametrize("zones,zone", [("map_benchmark_like_2_goals_zone_ids", 1), ("map_benchmark_like_4_free_zone_ids", 2)])
@pytest.mark.parametrize("n_iter_min,K", [(300, 1), (2500, 128)])
def test_single_context_observation_goal(po, zones, zone, n_iter_min, K):
    e, o = _grow_pair(po, zones, ("observation", zone), START, n_iter_min, 10000, K)
    want = S.of_oracle(o)
    got = e.solutions()
    assert len(want) >= 1 and len(o.final_ids()) > len(want)       # final chains: more finals than solutions
    _same(got, want)


def test_square_goal(po):
    e, o = _grow_pair(po, "map_benchmark_like_4_free_zone_ids", ("square", 0), (0.0, -0.8), 2500, 10000, 128)
    want = S.of_oracle(o)
    assert want
    _same(e.solutions(), want)


def test_goal_not_reached_is_count_zero(po):
    e, o = _grow_pair(po, "map_benchmark_like_4_free_zone_ids", ("square", 2), START, 50, 50, 1)
    assert len(o.final_ids()) == 0 and S.of_oracle(o) == []
    assert e.solutions() == []
    assert po.Engine.solutions_batch([e, e]) == [[], []]


@pytest.fixture(scope="module")
def batch(po):
    """the 40 rows of cases.tamp_queries(40) after one grow_batch, and their oracle twins' solutions"""
    qs = cases.tamp_queries(40)
    es = [cases.configure(po.Engine(0), q) for q in qs]
    po.Engine.grow_batch(es, [q.start for q in qs], qs[0].max_step, qs[0].search_radius, qs[0].n_iter_min, 128, n_iter_max=qs[0].n_iter_max)
    want = []
    for q in qs:
        o = cases.configure(orc.Oracle(), q)
        cases.grow(o, q, K=128, algo=orc.ALGO_BATCHED_KD)
        want.append(S.of_oracle(o))
    return es, want


def test_batch_rows_against_their_oracle_twins_and_the_single_call(po, batch):
    es, want = batch
    got = po.Engine.solutions_batch(es)
    assert len(got) == 40 and max(len(w) for w in want) >= 2
    for e, g, w in zip(es, got, want):
        _same(g, w)
        _same(e.solutions(), w)


def test_batch_rows_in_another_order_go_one_by_one(po, batch):
    es, want = batch
    order = list(range(len(es)))[::-1]
    order[3], order[17] = order[17], order[3]
    got = po.Engine.solutions_batch([es[k] for k in order])
    for k, g in zip(order, got):
        _same(g, want[k])
    # a run in the middle of other contexts: rows 5 .. 1, then the whole batch, then row 7
    mixed = [es[k] for k in (5, 4, 3, 2, 1)] + es + [es[7]]
    got = po.Engine.solutions_batch(mixed)
    for k, g in zip([5, 4, 3, 2, 1] + list(range(40)) + [7], got):
        _same(g, want[k])


def test_first_minimum_has_the_best_cost(po, batch):
    es, want = batch
    best = po.Engine.best_cost_batch(es)
    for e, w, b in zip(es, want, best):
        if not w:
            assert np.isinf(b)
            continue
        assert min(c for _, _, c in w) == b          # a final node below a final node costs no less than its parent


def test_capacity_and_invalid(po, batch):
    import ctypes as C
    es, want = batch
    L = es[0]._l
    arr = (C.c_void_p * 2)(es[0]._c, es[1]._c)
    ns, nst = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    assert L.porrt_solutions(arr, 2, ns.ctypes.data, nst.ctypes.data, None, None, None, 0, None, 0) == 0
    assert ns.tolist() == [len(want[0]), len(want[1])]
    assert nst.tolist() == [sum(len(p) for _, p, _ in want[0]), sum(len(p) for _, p, _ in want[1])]
    S_, X = int(ns.sum()), int(nst.sum())
    ids, lens, costs, xy = np.zeros(S_, dtype=np.uint64), np.zeros(S_, dtype=np.uint64), np.zeros(S_), np.zeros((X, 2))
    a = (ids.ctypes.data, lens.ctypes.data, costs.ctypes.data)
    assert L.porrt_solutions(arr, 2, None, None, *a, S_ - 1, xy.ctypes.data, X) == -5
    assert L.porrt_solutions(arr, 2, None, None, *a, S_, xy.ctypes.data, X - 1) == -5
    assert L.porrt_solutions(arr, 2, None, None, *a, S_, xy.ctypes.data, X) == 0
    assert ids.tolist() == [i for i, _, _ in want[0]] + [i for i, _, _ in want[1]]
    fresh = po.Engine(0)
    with pytest.raises(po.engine.PorrtError) as ex:
        fresh.solutions()                            # no results
    assert ex.value.code == -1
    c = cases.cfg3(300, 300)
    pto = cases.configure(po.Engine(0), c)
    cases.grow(pto, c, K=64)
    with pytest.raises(po.engine.PorrtError) as ex:
        pto.solutions()                              # PTO-mode results
    assert ex.value.code == -1
