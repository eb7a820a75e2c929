"""Many TAMP-RRT A* plans in one device call (porrt_tamp_rrt_plan_astar_batch).  The reference for every plan
of a batch is plan_tamp_rrt_astar alone on a fresh engine whose sampler seed is the plan's, bit for bit: policy states, parents,
leaves, beliefs, both expected costs, zone order, every search node, and queries / waves / speculated at equal width.  One plan per
test is also compared with the restatement on the oracle (tests/tamp_astar_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import tamp_astar_ref as A
from oracle import orc

pytestmark = pytest.mark.gpu

GRID = "map_benchmark_like"
START = (0.0, -1.0)
Z2 = "map_benchmark_like_2_goals_zone_ids"
Z4 = "map_benchmark_like_4_free_zone_ids"
Z4_SHELVES = "map_benchmark_like_4_goals_zone_ids"          # zones 1 and 2 have their centroids inside shelves
Z6 = "map_benchmark_like_6_free_zone_ids"
U4 = (0.25, 0.25, 0.25, 0.25)
# (seed, start, prior): the mixed batch of the 4-free-goal raster; the last repeats the first
MIXED = [(0, START, U4), (1, (-0.6, -0.9), (0.4, 0.3, 0.2, 0.1)), (2, (0.6, -0.9), (0.1, 0.2, 0.3, 0.4)), (3, (0.0, 0.0), U4),
         (0, START, (0.97, 0.01, 0.01, 0.01)), (0, START, U4)]


@pytest.fixture(scope="module")
def po():
    import po_rrt_amd
    return po_rrt_amd


def _setup(eng, zones, seed=0):
    eng.set_grid(cases.load_map(GRID), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    eng.set_zones(cases.load_map(zones), 0.5)
    eng.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return eng


def _engine(po, zones, seed=0, wave=1, pool=None, streams=1):
    e = _setup(po.Engine(0), zones, seed)
    e.set_option("tamp_streams", streams)
    e.set_option("tamp_wave", wave)
    if pool is not None:
        e.set_option("tamp_pool", pool)
    return e


_SINGLE = {}


def _single(po, zones, plan, wave, **kw):
    """plan_tamp_rrt_astar alone on a fresh engine seeded with the plan's seed: (dict or None, PorrtError or None, info, nodes).
    Computed once per case and shared (never modified)."""
    key = (zones, plan, wave, tuple(sorted(kw.items())))
    if key not in _SINGLE:
        seed, start, prior = plan
        e = _engine(po, zones, seed, wave)
        d = err = None
        try:
            d = e.plan_tamp_rrt_astar(start, list(prior), **kw)
        except po.engine.PorrtError as ex:
            err = ex
        _SINGLE[key] = (d, err, e.tamp_info(), e.tamp_astar_nodes())
    return _SINGLE[key]


def _batch(e, plans, **kw):
    return e.plan_tamp_rrt_astar_batch([p[1] for p in plans], [p[2] for p in plans], [p[0] for p in plans], **kw)


def _same_nodes(nd, r):
    assert np.array_equal(nd["parents"], r["parents"]) and np.array_equal(nd["targets"], r["targets"])
    assert np.array_equal(nd["ec"].view(np.uint64), r["ec"].view(np.uint64))
    assert np.array_equal(nd["priority"].view(np.uint64), r["priority"].view(np.uint64))


def _same_policy(d, r):
    assert d["zone_order"] == r["zone_order"]
    assert d["search_cost"] == r["search_cost"]
    assert d["expected_cost"] == r["expected_cost"]
    assert np.array_equal(d["xy"].view(np.uint64), r["xy"].view(np.uint64))
    assert np.array_equal(d["parents"], r["parents"])
    assert np.array_equal(d["is_leaf"], r["is_leaf"])
    assert np.array_equal(d["beliefs"].view(np.uint64), r["beliefs"].view(np.uint64))
    assert d["search_nodes"] == r["search_nodes"]


def _same_as_single(po, e, p, d, zones, plan, wave, **kw):
    """plan p of the last batch on e against the single plan at the same width"""
    sd, err, info, nodes = _single(po, zones, plan, wave, **kw)
    _same_nodes(e.tamp_batch_astar_nodes(p), nodes)
    if err is not None:
        assert d["status"] == err.code == -10 and "xy" not in d
        assert (d["fail_node"], d["fail_zone"], d["fail_query"]) == (info["fail_node"], info["fail_zone"], info["fail_query"])
        assert d["search_nodes"] == info["search_nodes"] == d["fail_node"]
        assert (d["queries"], d["waves"]) == (info["queries"], info["waves"])
        return
    assert d["status"] == 0 and (d["fail_node"], d["fail_zone"], d["fail_query"]) == (-1, -1, -1)
    _same_policy(d, sd)
    assert (d["queries"], d["waves"], d["speculated"]) == (sd["queries"], sd["waves"], sd["speculated"])


def _same_as_restatement(e, p, d, zones, plan, wave, **kw):
    seed, start, prior = plan
    r = A.Planner(_setup(orc.Oracle(), zones, seed), seed).plan(start, list(prior), streams=1, wave=wave, **kw)
    _same_policy(d, r)
    _same_nodes(e.tamp_batch_astar_nodes(p), dict(parents=r["node_parents"], targets=r["node_targets"], ec=r["node_ec"], priority=r["node_priority"]))
    assert (d["queries"], d["waves"], d["speculated"]) == (r["queries"], r["waves"], r["speculated"])


def _raw_batch(e, plans, **kw):
    """the C call itself, for its return value"""
    st = np.ascontiguousarray([p[1] for p in plans], dtype=np.float64)
    pr = np.ascontiguousarray([p[2] for p in plans], dtype=np.float64)
    sd = np.ascontiguousarray([p[0] for p in plans], dtype=np.uint64)
    return e._l.porrt_tamp_rrt_plan_astar_batch(e._c, len(plans), st.ctypes.data, pr.ctypes.data, sd.ctypes.data, pr.shape[1], 0.1, 2.0,
                                                kw.get("n_iter_min", 2500), kw.get("n_iter_max", 10000), 0.05, 128)


@pytest.mark.parametrize("zones,n", [(Z2, 2), (Z4, 4)])
def test_a_batch_of_one_is_the_single_plan(po, zones, n):
    plan = (0, START, tuple([1.0 / n] * n))
    e = _engine(po, zones, 5, wave=7)            # the lead's own seed is not the plan's: the plan's stream is seeds[p]
    out = _batch(e, [plan])
    assert len(out) == 1
    _same_as_single(po, e, 0, out[0], zones, plan, 7)
    _same_as_restatement(e, 0, out[0], zones, plan, 7)
    assert out[0]["wave"] == 7 and out[0]["streams"] == 1
    # seeds = None: the lead's sampler seed for every plan
    e0 = _engine(po, zones, 0, wave=7)
    none = e0.plan_tamp_rrt_astar_batch([START], [plan[2]])
    _same_as_single(po, e0, 0, none[0], zones, plan, 7)


@pytest.mark.parametrize("pool", [5, 512])
@pytest.mark.parametrize("wave", [1, 7])
def test_a_mixed_batch(po, wave, pool):
    """pool 5 cuts inside a node's children and mixes plans in a chunk; on the restatement the plans take 9 / 4 / 4 / 10 / 4 rounds
    at width 1"""
    e = _engine(po, Z4, 9, wave=wave, pool=pool)
    out = _batch(e, MIXED)
    assert [d["status"] for d in out] == [0] * len(MIXED)
    for p, (d, plan) in enumerate(zip(out, MIXED)):
        _same_as_single(po, e, p, d, Z4, plan, wave)
    _same_as_restatement(e, 1, out[1], Z4, MIXED[1], wave)
    if wave == 1:                                               # the plans do not end in the same round
        assert [d["waves"] for d in out] == [9, 4, 4, 10, 4, 9]
    # (at width 7 every one of these plans takes 4 rounds, alone as in the batch: the speculation levels them)
    _same_policy(out[5], out[0])                                # the repeat is the first
    _same_nodes(e.tamp_batch_astar_nodes(5), e.tamp_batch_astar_nodes(0))
    i = e.tamp_info()
    assert i["waves"] == max(d["waves"] for d in out) and i["queries"] == sum(d["queries"] for d in out)
    assert i["search_nodes"] == sum(d["search_nodes"] for d in out)
    assert e.tamp_astar_info()["speculated"] == sum(d["speculated"] for d in out)
    assert i["pool"] >= min(pool, 4) and i["pool"] <= pool


_NO_PATH = {}


def _restated_failure(zones, seed, n, **kw):
    """the restatement's NoPath of the failing plan, computed once (it is the same at every width: the width-1 search fails there)"""
    key = (zones, seed, tuple(sorted(kw.items())))
    if key not in _NO_PATH:
        with pytest.raises(A.NoPath) as rx:
            A.Planner(_setup(orc.Oracle(), zones, seed), seed).plan(START, [1.0 / n] * n, streams=1, wave=1, **kw)
        _NO_PATH[key] = (rx.value.node, rx.value.zone, ("observation", "pickup").index(rx.value.which))
    return _NO_PATH[key]


@pytest.mark.parametrize("wave", [1, 8])
def test_a_failing_plan_does_not_stop_the_others(po, wave):
    kw = dict(n_iter_min=2300, n_iter_max=2300)
    u6 = tuple([1.0 / 6] * 6)
    plans = [(0, START, u6), (3, START, u6), (4, START, u6)]
    e = _engine(po, Z6, 0, wave=wave)
    out = _batch(e, plans, **kw)
    assert [d["status"] for d in out] == [0, -10, 0]
    for p, (d, plan) in enumerate(zip(out, plans)):
        _same_as_single(po, e, p, d, Z6, plan, wave, **kw)
    bad = out[1]
    assert (bad["fail_node"], bad["fail_zone"], bad["fail_query"]) == _restated_failure(Z6, 3, 6, **kw)
    assert len(e.tamp_batch_astar_nodes(1)["parents"]) == bad["fail_node"]
    with pytest.raises(po.engine.PorrtError):                    # a failed plan has no policy to read
        e._chk(e._l.porrt_tamp_batch_policy(e._c, 1, None, None, None, None, 0, None))
    assert _raw_batch(e, plans, **kw) == 2


def test_a_batch_in_which_every_plan_fails(po):
    u4 = tuple(U4)
    plans = [(0, START, u4), (1, START, u4)]
    e = _engine(po, Z4_SHELVES, 0, wave=8)
    out = _batch(e, plans, n_iter_max=2500)                      # no exception
    assert [d["status"] for d in out] == [-10, -10]
    for p, (d, plan) in enumerate(zip(out, plans)):
        _same_as_single(po, e, p, d, Z4_SHELVES, plan, 8, n_iter_max=2500)
        assert d["fail_zone"] in (1, 2) and d["fail_node"] == 1 + d["fail_zone"]
    assert _raw_batch(e, plans, n_iter_max=2500) == 0


def test_the_arena_grows_under_a_batch(po):
    e = _engine(po, Z4, 0, wave=7, pool=5)
    e.set_option("tamp_arena_states", 1024)
    out = _batch(e, MIXED[:3])
    a = e.tamp_astar_info()
    assert a["arena_grown"] > 0 and a["arena_states"] > 1024 and a["arena_states"] >= a["arena_used"] > 0
    assert out[0]["arena_grown"] == a["arena_grown"]
    for p, (d, plan) in enumerate(zip(out, MIXED[:3])):
        _same_as_single(po, e, p, d, Z4, plan, 7)


def test_the_same_batch_twice_and_the_lead_is_left_alone(po):
    e = _engine(po, Z4, 0, wave=7)
    before = e.plan_tamp_rrt_astar(START, list(U4))
    before_nodes = e.tamp_astar_nodes()
    first = _batch(e, MIXED[:4])
    first_nodes = [e.tamp_batch_astar_nodes(p) for p in range(4)]
    # the batch replaced the last single plan
    with pytest.raises(po.engine.PorrtError) as ex:
        e._tamp_policy(0, 4)
    assert ex.value.code == -1 and len(e.tamp_astar_nodes()["parents"]) == 0
    second = _batch(e, MIXED[:4])                                # pool and arena are reused
    for p in range(4):
        _same_policy(second[p], first[p])
        _same_nodes(e.tamp_batch_astar_nodes(p), first_nodes[p])
        assert (second[p]["queries"], second[p]["waves"], second[p]["speculated"]) == (first[p]["queries"], first[p]["waves"], first[p]["speculated"])
        _same_as_single(po, e, p, second[p], Z4, MIXED[p], 7)
    # streams and shuffles untouched: a branch and bound on the lead is that of a fresh engine
    after = e.plan_tamp_rrt(START, list(U4))
    fresh = _engine(po, Z4, 0, wave=7).plan_tamp_rrt(START, list(U4))
    assert after["zone_order"] == fresh["zone_order"] and after["search_cost"] == fresh["search_cost"]
    assert after["queries"] == fresh["queries"] and after["search_nodes"] == fresh["search_nodes"]
    assert np.array_equal(after["xy"].view(np.uint64), fresh["xy"].view(np.uint64)) and np.array_equal(after["parents"], fresh["parents"])
    again = e.plan_tamp_rrt_astar(START, list(U4))
    _same_policy(again, before)
    _same_nodes(e.tamp_astar_nodes(), before_nodes)
    assert (again["queries"], again["waves"], again["speculated"]) == (before["queries"], before["waves"], before["speculated"])


def test_refusals(po):
    good = [(0, START, U4), (1, START, U4), (2, START, U4)]

    def refused(e, plans, named=None, **kw):
        with pytest.raises(po.engine.PorrtError) as ex:
            _batch(e, plans, **kw)
        assert ex.value.code == -1
        if named is not None:
            assert "plan %d" % named in str(ex.value)
        assert e.tamp_info()["queries"] == 0                     # nothing was grown

    refused(_engine(po, Z4), [good[0], (1, START, (0.5, 0.0, 0.25, 0.25)), good[2]], named=1)       # a zero entry in the middle
    refused(_engine(po, Z4), [good[0], good[1], (2, START, (0.3, 0.3, 0.3, 0.3))], named=2)         # a wrong sum
    refused(_engine(po, Z4), [(0, START, (0.5, 0.25, 0.25))])                                       # n_worlds is not the zone count
    refused(_engine(po, Z4), [])                                                                    # n_plans 0
    refused(_engine(po, Z4, streams=0), good)                                                       # one continuous stream cannot be shared
    e = _engine(po, Z4)
    assert e._l.porrt_tamp_rrt_plan_astar_batch(e._c, 65537, None, None, None, 4, 0.1, 2.0, 2500, 10000, 0.05, 128) == -1
    st = np.zeros((1, 2))
    assert e._l.porrt_tamp_rrt_plan_astar_batch(e._c, 1, st.ctypes.data, None, None, 4, 0.1, 2.0, 2500, 10000, 0.05, 128) == -1
    rec = po.engine.TampBatchPlan()
    assert e._l.porrt_tamp_batch_get_plan(e._c, 0, C.byref(rec)) == -1                              # no batch has run


def test_cpp_mirror_batch_is_the_single_plans(po, tmp_path):
    """MapShelfDomainTampRRT::plan_astar_batch (include/porrt.hpp) against plan_astar alone, in a program of its own"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "po_rrt_amd")
    exe = str(tmp_path / "astar_batch_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(root, "tests", "astar_batch_mirror.cpp"),
                    "-L" + lib, "-lporrt_hip", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe, os.path.join(cases.MAPS, GRID + ".pgm"), os.path.join(cases.MAPS, Z4 + ".pgm"), "4"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "astar_batch_mirror ok" in out.stdout, out.stdout + out.stderr
