"""The TAMP-RRT A* planner on the device (porrt_tamp_rrt_plan_astar) against its restatement on the oracle
(tests/tamp_astar_ref.py), bit for bit: policy states, parents, leaves, beliefs, both expected costs, zone order and every search
node (parent, zone, expected cost, priority) in id order."""
import numpy as np
import pytest

import cases
import tamp_astar_ref as A
import tamp_rrt_ref as R
from oracle import orc

pytestmark = pytest.mark.gpu

GRID = "map_benchmark_like"
START = (0.0, -1.0)
Z2 = "map_benchmark_like_2_goals_zone_ids"
Z4 = "map_benchmark_like_4_free_zone_ids"
Z6 = "map_benchmark_like_6_free_zone_ids"


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
    return A.Planner(_setup(orc.Oracle(), zones, seed), seed)


def _uniform(n):
    return [1.0 / n] * n


_REF = {}


def _ref_plan(zones, n, wave):
    """the restatement's plans with per-edge streams at seed 0, computed once and shared (never modified)"""
    if (zones, wave) not in _REF:
        _REF[(zones, wave)] = _ref(zones, 0).plan(START, _uniform(n), streams=1, wave=wave)
    return _REF[(zones, wave)]


def _same(e, d, r, queries=True):
    assert d["zone_order"] == r["zone_order"]
    assert d["search_cost"] == r["search_cost"]
    assert d["expected_cost"] == r["expected_cost"]
    assert np.array_equal(d["xy"].view(np.uint64), r["xy"].view(np.uint64))
    assert np.array_equal(d["parents"], r["parents"])
    assert np.array_equal(d["is_leaf"], r["is_leaf"])
    assert np.array_equal(d["beliefs"].view(np.uint64), r["beliefs"].view(np.uint64))
    assert d["search_nodes"] == r["search_nodes"]
    nd = e.tamp_astar_nodes()
    assert np.array_equal(nd["parents"], r["node_parents"]) and np.array_equal(nd["targets"], r["node_targets"])
    assert np.array_equal(nd["ec"].view(np.uint64), r["node_ec"].view(np.uint64))
    assert np.array_equal(nd["priority"].view(np.uint64), r["node_priority"].view(np.uint64))
    if queries:
        assert (d["queries"], d["waves"], d["speculated"]) == (r["queries"], r["waves"], r["speculated"])


@pytest.mark.parametrize("seed", [0, 1])
def test_shared_stream_2_goals(po, seed):
    e = _engine(po, Z2, seed, streams=0, wave=64)
    d = e.plan_tamp_rrt_astar(START, _uniform(2))
    r = _ref(Z2, seed).plan(START, _uniform(2), streams=0)
    _same(e, d, r)
    assert d["wave"] == 1 and d["streams"] == 0


def test_shared_stream_4_goals_twice_and_the_shuffles_are_untouched(po):
    e = _engine(po, Z4, 0, streams=0)
    r = _ref(Z4, 0).plan(START, _uniform(4), streams=0)
    for _ in range(2):           # the continuous stream is set back: the second plan repeats the first
        _same(e, e.plan_tamp_rrt_astar(START, _uniform(4)), r)
    # A* drew no shuffle: a branch and bound after it is that of a fresh engine
    after = e.plan_tamp_rrt(START, _uniform(4))
    fresh = _engine(po, Z4, 0, streams=0).plan_tamp_rrt(START, _uniform(4))
    assert after["zone_order"] == fresh["zone_order"] and after["search_cost"] == fresh["search_cost"]
    assert after["queries"] == fresh["queries"] and after["search_nodes"] == fresh["search_nodes"]
    assert np.array_equal(after["xy"].view(np.uint64), fresh["xy"].view(np.uint64)) and np.array_equal(after["parents"], fresh["parents"])
    assert e.tamp_astar_info()["speculated"] == 0


@pytest.mark.parametrize("zones,n", [(Z4, 4), (Z6, 6)])
@pytest.mark.parametrize("wave", [1, 7, 64])
def test_per_edge_streams_wave_widths(po, zones, n, wave):
    e = _engine(po, zones, 0, streams=1, wave=wave)
    d = e.plan_tamp_rrt_astar(START, _uniform(n))
    _same(e, d, _ref_plan(zones, n, 1), queries=False)              # the result is that of width 1
    rw = _ref_plan(zones, n, wave)
    assert (d["queries"], d["waves"], d["speculated"]) == (rw["queries"], rw["waves"], rw["speculated"])
    assert d["wave"] == wave and d["streams"] == 1 and d["pruned"] == 0


def test_the_arena_grows_and_the_plan_stays(po):
    e = _engine(po, Z4, 0, streams=1, wave=7)
    e.set_option("tamp_arena_states", 1024)
    d = e.plan_tamp_rrt_astar(START, _uniform(4))
    # room is made for 1024 states per row before a gather, whatever the paths then take
    assert d["arena_grown"] > 0 and d["arena_states"] > 1024 and d["arena_states"] >= d["arena_used"] > 0
    _same(e, d, _ref_plan(Z4, 4, 1), queries=False)
    assert d["queries"] == _ref_plan(Z4, 4, 7)["queries"]
    with pytest.raises(po.engine.PorrtError):
        e.set_option("tamp_arena_states", 1023)


def test_short_paths_through_the_device_resident_shortcut(po):
    """paths of 0, 1 and 2 states are copied, longer ones shortcut -- through k_astar_chain, as the winning chain of a plan is"""
    e = _setup(po.Engine(0), Z4)
    o = _setup(orc.Oracle(), Z4)
    t = np.linspace(0.0, 1.0, 1500)
    long = np.stack([-0.9 + 1.8 * t, -0.95 + 0.02 * np.sin(40 * t)], axis=1)       # longer than the wave's LDS stage (1024)
    zig = [[-0.5, -0.9], [-0.3, -0.7], [-0.1, -0.9], [0.1, -0.7], [0.3, -0.9], [0.5, -0.7]]
    paths = [[[0.0, -1.0]], [], [[0.0, -1.0], [0.1, -0.9]], [[0.0, -1.0], [0.05, -0.8], [0.1, -0.95]], long, zig, [[0.2, -0.9], [0.3, -0.9]]]
    got = e.tamp_shortcut(paths, resident=True)
    host = e.tamp_shortcut(paths)
    for g, h, p in zip(got, host, paths):
        w = np.array(R.shortcut(o, p)).reshape(-1, 2)
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)) and np.array_equal(g.view(np.uint64), h.view(np.uint64))
    assert np.array_equal(got[2], [[0.0, -1.0], [0.1, -0.9]]) and len(got[1]) == 0
    only_short = e.tamp_shortcut(paths[:3], resident=True)
    assert all(np.array_equal(a, np.asarray(b, dtype=np.float64).reshape(-1, 2)) for a, b in zip(only_short, paths[:3]))


@pytest.mark.parametrize("wave", [1, 64])
def test_no_path_at_the_roots_expansion(po, wave):
    """zones 1 and 2 of the 4-goal raster have their centroids inside shelves: a pickup query to either finds no path"""
    z = "map_benchmark_like_4_goals_zone_ids"
    e = _engine(po, z, 0, streams=1, wave=wave)
    with pytest.raises(po.engine.PorrtError) as ex:
        e.plan_tamp_rrt_astar(START, _uniform(4), n_iter_max=2500)
    assert ex.value.code == -10
    i = e.tamp_info()
    with pytest.raises(A.NoPath) as rx:
        _ref(z, 0).plan(START, _uniform(4), n_iter_max=2500, streams=1, wave=wave)
    assert (rx.value.node, rx.value.zone, rx.value.which) == (i["fail_node"], i["fail_zone"], ("observation", "pickup")[i["fail_query"]])
    assert i["fail_node"] == 1 + i["fail_zone"] and i["fail_zone"] in (1, 2)          # a child of the root
    assert len(e.tamp_astar_nodes()["parents"]) == i["fail_node"]                    # the nodes made before it


@pytest.mark.parametrize("wave", [1, 64])
def test_no_observation_path_below_the_root(po, wave):
    """2100 iterations leave an observation query under a popped child of the root without a path: the wave's other rows go on to
    their pickup queries without it, and the plan fails when that child is popped, with the id its child would have got"""
    e = _engine(po, Z6, 0, streams=1, wave=wave)
    with pytest.raises(po.engine.PorrtError) as ex:
        e.plan_tamp_rrt_astar(START, _uniform(6), n_iter_min=2100, n_iter_max=2100)
    assert ex.value.code == -10
    i = e.tamp_info()
    with pytest.raises(A.NoPath) as rx:
        _ref(Z6, 0).plan(START, _uniform(6), n_iter_min=2100, n_iter_max=2100, streams=1, wave=wave)
    assert (rx.value.node, rx.value.zone, rx.value.which) == (i["fail_node"], i["fail_zone"], ("observation", "pickup")[i["fail_query"]])
    assert i["fail_query"] == 0 and i["fail_node"] > 6
    assert len(e.tamp_astar_nodes()["parents"]) == i["fail_node"]                    # the nodes made before it


def test_refusals(po):
    e = _engine(po, Z2)
    for bad in ([1.0, 0.0], [0.5, 0.6], [1.0, 0.0, 0.0], [1.0 / 3] * 3, [1.5, -0.5]):
        with pytest.raises(po.engine.PorrtError) as ex:
            e.plan_tamp_rrt_astar(START, bad)
        assert ex.value.code == -1
    with pytest.raises(po.engine.PorrtError) as ex:
        e.plan_tamp_rrt(START, _uniform(2), search="astar")
    assert ex.value.code == -1
    assert e.get_option("tamp_search") == 0
