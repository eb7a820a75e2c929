"""The restatement of BranchAndBoundMultipleViewPoints with ascending-id viewpoints (tests/tamp_viewpoints_ref.py) on the CPU oracle.

The device planner (porrt_tamp_rrt_plan_viewpoints) is checked against it in tests/test_gpu_tamp_viewpoints.py."""
import numpy as np
import pytest

import cases
import tamp_rrt_ref as R
import tamp_viewpoints_ref as V
from oracle import orc

START = (0.0, -1.0)
Z2 = "map_benchmark_like_2_goals_zone_ids"


def _oracle(zones, seed=0):
    o = orc.Oracle()
    o.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    o.set_zones(cases.load_map(zones), 0.5)
    o.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return o


@pytest.fixture(scope="module")
def plans():
    """2 goals, visibility 0.5, start (0, -1), uniform prior, 0.1 / 2.0 / 1000 / 10000, K 128, seed 0, one stream per query"""
    return {w: V.Planner(_oracle(Z2), 0).plan(START, [0.5, 0.5], 0.1, 2.0, 1000, 10000, K=128, streams=1, wave=w) for w in (1, 7, 64)}


def test_same_policy_and_cost_at_every_wave(plans):
    a = plans[1]
    for w in (7, 64):
        b = plans[w]
        assert b["search_cost"] == a["search_cost"] and b["expected_cost"] == a["expected_cost"]
        assert b["zone_order"] == a["zone_order"] and b["viewpoint_ranks"] == a["viewpoint_ranks"]
        assert np.array_equal(b["xy"].view(np.uint64), a["xy"].view(np.uint64))
        assert np.array_equal(b["parents"], a["parents"]) and np.array_equal(b["is_leaf"], a["is_leaf"])
        assert np.array_equal(b["beliefs"], a["beliefs"])
    assert plans[64]["waves"] < plans[1]["waves"]


def test_the_case_has_what_it_is_meant_to_test(plans):
    """floors from the restatement's own output: a case that misses one of them tests nothing"""
    a = plans[1]
    assert max(a["viewpoint_counts"]) >= 2                 # some observation query has several viewpoints
    assert a["pruned"] >= 1                                # a child is pruned at wave 1
    lc = a["leaf_costs"]
    assert lc[0] == a["search_cost"] and (len(lc) == 1 or lc[1] > lc[0])      # the lowest leaf cost is unique
    assert a["queries"] == a["observation_queries"] + a["pickup_queries"]
    assert a["pickup_queries"] == a["viewpoints_kept"] == a["viewpoints_found"] == a["search_nodes"] - 1


def test_seed_rule_and_the_cap():
    ho = R.splitmix64(5 ^ (2 + 1))
    assert R.splitmix64(ho ^ (1 << 32)) != R.splitmix64(ho ^ (2 << 32)) != ho
    sols = [(3, None, 2.0), (5, None, 1.0), (8, None, 1.0), (9, None, 3.0)]
    assert [s[0] for s in V.keep(sols, 0)] == [3, 5, 8, 9]
    assert [s[0] for s in V.keep(sols, 1)] == [5]                 # ties: the lower id
    assert [s[0] for s in V.keep(sols, 3)] == [3, 5, 8]           # kept ones stay in ascending id
    assert [s[0] for s in V.keep(sols, 7)] == [3, 5, 8, 9]


def test_the_cap_bounds_the_children_per_query():
    r = V.Planner(_oracle(Z2), 0).plan(START, [0.5, 0.5], 0.1, 2.0, 1000, 10000, K=128, streams=1, wave=1, max_viewpoints=2)
    assert r["viewpoints_kept"] < r["viewpoints_found"] and r["viewpoints_kept"] <= 2 * r["observation_queries"]
    assert all(k <= 1 for k in r["viewpoint_ranks"])


def test_invalid_prior():
    with pytest.raises(ValueError):
        V.Planner(_oracle(Z2), 0).plan(START, [0.5, 0.6])
