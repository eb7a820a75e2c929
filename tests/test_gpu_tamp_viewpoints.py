"""The multiple-viewpoints TAMP-RRT search on the device (porrt_tamp_rrt_plan_viewpoints) against its
restatement on the oracle (tests/tamp_viewpoints_ref.py), bit for bit: policy states, parents, leaves, beliefs, both expected costs,
zone order, viewpoint ranks, and at wave 1 the search nodes and queries."""
import numpy as np
import pytest

import cases
import tamp_rrt_ref as R
import tamp_viewpoints_ref as V
from oracle import orc

pytestmark = pytest.mark.gpu

GRID = "map_benchmark_like"
START = (0.0, -1.0)
Z2 = "map_benchmark_like_2_goals_zone_ids"
Z4 = "map_benchmark_like_4_free_zone_ids"
N_MIN = 1000


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
    e.set_option("tamp_pool", 64)
    return e


def _ref(zones, seed=0):
    return V.Planner(_setup(orc.Oracle(), zones, seed), seed)


def _uniform(n):
    return [1.0 / n] * n


def _same(d, r, queries=True):
    assert d["zone_order"] == r["zone_order"]
    assert d["viewpoint_ranks"] == r["viewpoint_ranks"]
    assert d["search_cost"] == r["search_cost"]
    assert d["expected_cost"] == r["expected_cost"]
    assert np.array_equal(d["xy"].view(np.uint64), r["xy"].view(np.uint64))
    assert np.array_equal(d["parents"], r["parents"])
    assert np.array_equal(d["is_leaf"], r["is_leaf"])
    assert np.array_equal(d["beliefs"].view(np.uint64), r["beliefs"].view(np.uint64))
    if queries:
        for k in ("queries", "search_nodes", "observation_queries", "pickup_queries", "viewpoints_found", "viewpoints_kept", "largest_set",
                  "pruned"):
            assert d[k] == r[k], k


@pytest.mark.parametrize("seed", [0, 1])
def test_shared_stream_2_goals_and_a_second_plan(po, seed):
    e, ref = _engine(po, Z2, seed, streams=0), _ref(Z2, seed)
    for _ in range(2):           # the discrete stream runs on, the continuous one starts again
        d = e.plan_tamp_rrt_viewpoints(START, _uniform(2), n_iter_min=N_MIN)
        r = ref.plan(START, _uniform(2), n_iter_min=N_MIN, streams=0)
        _same(d, r)
        assert d["largest_set"] >= 2


def test_per_query_streams_wave_widths_2_goals(po):
    r = _ref(Z2, 0).plan(START, _uniform(2), n_iter_min=N_MIN, streams=1, wave=1)
    assert r["largest_set"] >= 2 and r["pruned"] >= 1
    for wave in (1, 7, 64):
        d = _engine(po, Z2, 0, wave=wave).plan_tamp_rrt_viewpoints(START, _uniform(2), n_iter_min=N_MIN)
        _same(d, r, queries=(wave == 1))
        assert d["wave"] == wave and d["streams"] == 1 and d["max_viewpoints"] == 0


@pytest.fixture(scope="module")
def ref4():
    return _ref(Z4, 0).plan(START, _uniform(4), n_iter_min=N_MIN, streams=1, wave=1, max_viewpoints=2)


@pytest.mark.parametrize("wave", [1, 64])
def test_4_zones_two_viewpoints_per_query(po, ref4, wave):
    d = _engine(po, Z4, 0, wave=wave).plan_tamp_rrt_viewpoints(START, _uniform(4), n_iter_min=N_MIN, max_viewpoints=2)
    _same(d, ref4, queries=(wave == 1))
    assert d["max_viewpoints"] == 2 and all(k <= 1 for k in d["viewpoint_ranks"])
    if wave == 1:
        assert d["viewpoints_kept"] < d["viewpoints_found"]


def test_one_viewpoint_per_query(po):
    """max_viewpoints 1 keeps the cheapest observation path, as BranchAndBound does -- on other streams, so the two plans are not
    asserted equal: the pickup query here does not continue the observation stream"""
    d = _engine(po, Z2, 0).plan_tamp_rrt_viewpoints(START, _uniform(2), n_iter_min=N_MIN, max_viewpoints=1)
    r = _ref(Z2, 0).plan(START, _uniform(2), n_iter_min=N_MIN, streams=1, max_viewpoints=1)
    _same(d, r)
    assert d["viewpoint_ranks"] == [0, 0] and d["pickup_queries"] == d["observation_queries"]


def test_no_pickup_path_names_the_node(po):
    """zones 1 and 2 of the 4-goal raster have their centroids inside shelves: a pickup query to either finds no path"""
    z = "map_benchmark_like_4_goals_zone_ids"
    e = _engine(po, z)
    with pytest.raises(po.engine.PorrtError) as ex:
        e.plan_tamp_rrt_viewpoints(START, _uniform(4), n_iter_min=N_MIN, n_iter_max=2500)
    assert ex.value.code == -10
    i = e.tamp_info()
    with pytest.raises(R.NoPath) as rx:
        _ref(z).plan(START, _uniform(4), n_iter_min=N_MIN, n_iter_max=2500, streams=1)
    assert rx.value.which == "pickup" and rx.value.zone in (1, 2)
    assert (i["fail_node"], i["fail_zone"], i["fail_query"]) == (rx.value.node, rx.value.zone, 1)
    with pytest.raises(po.engine.PorrtError):
        e._tamp_policy(1, 4)                     # no policy after a failed plan


def test_a_plan_of_either_kind_replaces_the_other(po):
    e = _engine(po, Z2, 0, wave=64)
    a = e.plan_tamp_rrt_viewpoints(START, _uniform(2), n_iter_min=N_MIN)
    assert a["pickup_queries"] > a["observation_queries"] > 0
    b = e.plan_tamp_rrt(START, _uniform(2), n_iter_min=N_MIN)
    stored = e._tamp_policy(len(b["parents"]), 2)
    assert np.array_equal(stored["xy"], b["xy"]) and stored["search_cost"] == b["search_cost"]
    v = e.tamp_viewpoints_info()
    assert v["observation_queries"] == 0 and v["viewpoint_ranks"] == []
    c = e.plan_tamp_rrt_viewpoints(START, _uniform(2), n_iter_min=N_MIN)
    stored = e._tamp_policy(len(c["parents"]), 2)
    assert np.array_equal(stored["xy"], c["xy"]) and stored["search_cost"] == c["search_cost"] and e.tamp_info()["queries"] == c["queries"]


def test_the_enum_value_is_still_refused(po):
    e = _engine(po, Z2)
    with pytest.raises(po.engine.PorrtError) as ex:
        e.plan_tamp_rrt(START, _uniform(2), search="branch_and_bound_multiple_viewpoints")
    assert ex.value.code == -1
    for bad in ([0.5, 0.6], [1.0, 0.0, 0.0]):
        with pytest.raises(po.engine.PorrtError) as ex:
            e.plan_tamp_rrt_viewpoints(START, bad)
        assert ex.value.code == -1


def test_no_viewpoint_at_all_is_no_leaf(po):
    """observation queries that end before they see their zone make no children (no error of their own); the search then ends
    without a leaf: expect("No solution found!")"""
    e = _engine(po, Z2)
    with pytest.raises(po.engine.PorrtError) as ex:
        e.plan_tamp_rrt_viewpoints(START, _uniform(2), n_iter_min=20, n_iter_max=20)
    assert ex.value.code == -10
    i, v = e.tamp_info(), e.tamp_viewpoints_info()
    assert (i["fail_node"], i["fail_zone"], i["fail_query"]) == (-1, -1, -1)
    assert v["observation_queries"] == 2 and v["pickup_queries"] == 0 and v["viewpoints_found"] == 0
    with pytest.raises(V.NoLeaf):
        _ref(Z2).plan(START, _uniform(2), n_iter_min=20, n_iter_max=20, streams=1)
