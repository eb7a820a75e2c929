"""The TAMP-RRT branch-and-bound planner on the device (porrt_tamp_rrt_plan) against its restatement on the
oracle (tests/tamp_rrt_ref.py), bit for bit: policy states, parents, leaves, beliefs, both expected costs, zone order, queries."""
import numpy as np
import pytest

import cases
import tamp_rrt_ref as R
from oracle import orc

pytestmark = pytest.mark.gpu

GRID = "map_benchmark_like"
START = (0.0, -1.0)


@pytest.fixture(scope="module")
def po():
    import po_rrt_amd
    return po_rrt_amd


def _setup(eng, zones, seed=0):
    eng.set_grid(cases.load_map(GRID), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    eng.set_zones(cases.load_map(zones), 0.5)
    eng.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return eng


def _engine(po, zones, seed=0, streams=1, wave=1):
    e = _setup(po.Engine(0), zones, seed)
    e.set_option("tamp_streams", streams)
    e.set_option("tamp_wave", wave)
    return e


def _ref(zones, seed=0):
    return R.Planner(_setup(orc.Oracle(), zones, seed), seed)


def _uniform(n):
    return [1.0 / n] * n


def _same(d, r, queries=True):
    assert d["zone_order"] == r["zone_order"]
    assert d["search_cost"] == r["search_cost"]
    assert d["expected_cost"] == r["expected_cost"]
    assert np.array_equal(d["xy"].view(np.uint64), r["xy"].view(np.uint64))
    assert np.array_equal(d["parents"], r["parents"])
    assert np.array_equal(d["is_leaf"], r["is_leaf"])
    assert np.array_equal(d["beliefs"].view(np.uint64), r["beliefs"].view(np.uint64))
    if queries:
        assert d["queries"] == r["queries"]
        assert d["search_nodes"] == r["search_nodes"]


@pytest.mark.parametrize("seed", [0, 1])
def test_shared_stream_2_goals(po, seed):
    z = "map_benchmark_like_2_goals_zone_ids"
    d = _engine(po, z, seed, streams=0).plan_tamp_rrt(START, _uniform(2))
    r = _ref(z, seed).plan(START, _uniform(2), streams=0)
    _same(d, r)


def test_shared_stream_4_goals_and_a_second_plan(po):
    z = "map_benchmark_like_4_free_zone_ids"
    e = _engine(po, z, 0, streams=0)
    ref = _ref(z, 0)
    for _ in range(2):           # the discrete stream runs on, the continuous one starts again
        d = e.plan_tamp_rrt(START, _uniform(4))
        r = ref.plan(START, _uniform(4), streams=0)
        _same(d, r)


@pytest.mark.parametrize("zones,n", [("map_benchmark_like_4_free_zone_ids", 4), ("map_benchmark_like_6_free_zone_ids", 6)])
def test_per_edge_streams_wave_widths(po, zones, n):
    r = _ref(zones, 0).plan(START, _uniform(n), streams=1, wave=1)
    for wave in (1, 7, 64):
        d = _engine(po, zones, 0, streams=1, wave=wave).plan_tamp_rrt(START, _uniform(n))
        _same(d, r, queries=(wave == 1))
        assert d["wave"] == wave and d["streams"] == 1


def test_best_path_equals_host_walk(po):
    """k_best_path on every row of a 40-query TAMP-shaped batch against porrt_best_solution (the host walk)"""
    qs = cases.tamp_queries(40)
    es = [cases.configure(po.Engine(0), q) for q in qs]
    po.Engine.grow_batch(es, [q.start for q in qs], qs[0].max_step, qs[0].search_radius, qs[0].n_iter_min, 128)
    got = po.Engine.best_paths(es)
    for e, g in zip(es, got):
        h = e.best_solution()
        if h is None:
            assert g is None
            continue
        assert g is not None
        assert np.array_equal(g[0].view(np.uint64), np.asarray(h[0]).view(np.uint64)) and g[1] == h[1]


def _shortcut_pair(po, paths):
    e = _setup(po.Engine(0), "map_benchmark_like_4_free_zone_ids")
    o = _setup(orc.Oracle(), "map_benchmark_like_4_free_zone_ids")
    got = e.tamp_shortcut(paths)
    want = [np.array(R.shortcut(o, p)).reshape(-1, 2) for p in paths]
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64))
    return got


def test_shortcut_short_and_long_paths(po):
    t = np.linspace(0.0, 1.0, 1500)
    long = np.stack([-0.9 + 1.8 * t, -0.95 + 0.02 * np.sin(40 * t)], axis=1)       # longer than the wave's LDS stage (1024)
    zig = [[-0.5, -0.9], [-0.3, -0.7], [-0.1, -0.9], [0.1, -0.7], [0.3, -0.9], [0.5, -0.7]]
    got = _shortcut_pair(po, [[[0.0, -1.0]], [[0.0, -1.0], [0.1, -0.9]], [[0.0, -1.0], [0.05, -0.8], [0.1, -0.95]], long, zig])
    assert np.array_equal(got[0], [[0.0, -1.0]]) and np.array_equal(got[1], [[0.0, -1.0], [0.1, -0.9]])


def test_shortcut_leaves_the_last_step_unchecked(po):
    o = _setup(orc.Oracle(), "map_benchmark_like_4_free_zone_ids")
    path = unchecked_last_step_path(o)
    got = _shortcut_pair(po, [path])
    assert not np.array_equal(got[0], np.asarray(path))


def unchecked_last_step_path(o):
    return R.find_unchecked_path(o)


def test_no_path_names_the_node(po):
    """zones 1 and 2 of the 4-goal raster have their centroids inside shelves: a pickup query to either finds no path"""
    z = "map_benchmark_like_4_goals_zone_ids"
    e = _engine(po, z, 0, streams=1, wave=1)
    with pytest.raises(po.engine.PorrtError) as ex:
        e.plan_tamp_rrt(START, _uniform(4), n_iter_max=2500)
    assert ex.value.code == -10
    i = e.tamp_info()
    assert i["fail_node"] > 0 and i["fail_zone"] in (1, 2)
    with pytest.raises(R.NoPath) as rx:
        _ref(z, 0).plan(START, _uniform(4), n_iter_max=2500, streams=1)
    assert (rx.value.node, rx.value.zone, rx.value.which) == (i["fail_node"], i["fail_zone"], ("observation", "pickup")[i["fail_query"]])


def test_invalid_prior_and_refused_searches(po):
    z = "map_benchmark_like_2_goals_zone_ids"
    e = _engine(po, z)
    for bad in ([0.5, 0.6], [1.0, 0.0, 0.0]):
        with pytest.raises(po.engine.PorrtError) as ex:
            e.plan_tamp_rrt(START, bad)
        assert ex.value.code == -1
    for kind in ("astar", "branch_and_bound_multiple_viewpoints"):
        with pytest.raises(po.engine.PorrtError) as ex:
            e.plan_tamp_rrt(START, _uniform(2), search=kind)
        assert ex.value.code == -1
    assert e.get_option("tamp_search") == 0
