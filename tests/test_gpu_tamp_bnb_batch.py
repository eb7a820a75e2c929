"""Many TAMP-RRT branch-and-bound plans in one device call (porrt_tamp_rrt_plan_batch).  The reference for
every plan of a batch is plan_tamp_rrt alone on a fresh engine whose sampler seed and discrete seed are the plan's, at the same
tamp_wave with tamp_streams 1, bit for bit: policy states, parents, leaves, beliefs, both expected costs, zone order, and
search_nodes / queries / waves / pruned.  Some plans are also compared with the restatement on the oracle (tests/tamp_rrt_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import tamp_rrt_ref as R
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
TWO = [(0, START, (0.5, 0.5)), (1, (-0.6, -0.9), (0.7, 0.3)), (2, (0.6, -0.9), (0.2, 0.8)), (3, (0.0, 0.0), (0.5, 0.5)),
       (4, (0.3, -1.0), (0.999, 0.001))]
RECORD = ("status", "fail_node", "fail_zone", "fail_query", "search_cost", "expected_cost", "search_nodes", "queries", "waves", "pruned",
          "speculated", "zone_order")


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


def _single(po, zones, plan, wave, dseed=None, **kw):
    """plan_tamp_rrt alone on a fresh engine seeded with the plan's seed (and then its discrete seed): (dict or None, PorrtError or
    None, info).  Computed once per case and shared (never modified)."""
    key = (zones, plan, wave, dseed, tuple(sorted(kw.items())))
    if key not in _SINGLE:
        seed, start, prior = plan
        e = _engine(po, zones, seed, wave)
        if dseed is not None:
            e.set_discrete_seed(dseed)
        d = err = None
        try:
            d = e.plan_tamp_rrt(start, list(prior), **kw)
        except po.engine.PorrtError as ex:
            err = ex
        _SINGLE[key] = (d, err, e.tamp_info())
    return _SINGLE[key]


def _batch(e, plans, dseeds=None, **kw):
    return e.plan_tamp_rrt_batch([p[1] for p in plans], [p[2] for p in plans], [p[0] for p in plans], dseeds, **kw)


def _same_policy(d, r):
    assert d["zone_order"] == r["zone_order"]
    assert d["search_cost"] == r["search_cost"]
    assert d["expected_cost"] == r["expected_cost"]
    assert np.array_equal(d["xy"].view(np.uint64), r["xy"].view(np.uint64))
    assert np.array_equal(d["parents"], r["parents"])
    assert np.array_equal(d["is_leaf"], r["is_leaf"])
    assert np.array_equal(d["beliefs"].view(np.uint64), r["beliefs"].view(np.uint64))
    assert d["search_nodes"] == r["search_nodes"]


def _same_counts(d, r):
    assert (d["queries"], d["waves"], d["pruned"]) == (r["queries"], r["waves"], r["pruned"])


def _same_as_single(po, e, p, d, zones, plan, wave, dseed=None, **kw):
    """plan p of the last batch on e against the single plan at the same width"""
    sd, err, info = _single(po, zones, plan, wave, dseed, **kw)
    nodes = e.tamp_batch_bnb_nodes(p)
    assert len(nodes["parents"]) == d["search_nodes"] and nodes["parents"][0] == -1 and nodes["pushed"][0] == 1
    assert d["speculated"] == 0
    if err is not None:
        assert d["status"] == err.code == -10 and "xy" not in d
        assert (d["fail_node"], d["fail_zone"], d["fail_query"]) == (info["fail_node"], info["fail_zone"], info["fail_query"])
        assert d["search_nodes"] == info["search_nodes"] > d["fail_node"] > 0
        assert nodes["targets"][d["fail_node"]] == d["fail_zone"]
        return
    assert d["status"] == 0 and (d["fail_node"], d["fail_zone"], d["fail_query"]) == (-1, -1, -1)
    _same_policy(d, sd)
    _same_counts(d, sd)
    # the node table holds the policy's chain: the best leaf is a pushed node of that cost without remaining zones below it
    nz = len(plan[2])
    depth = np.zeros(len(nodes["parents"]), dtype=np.int64)
    for k in range(1, len(depth)):
        assert 0 <= nodes["parents"][k] < k
        depth[k] = depth[nodes["parents"][k]] + 1
    leaves = np.flatnonzero((depth == nz) & (nodes["pushed"] == 1))
    assert len(leaves) and nodes["ec"][leaves].min() == d["search_cost"]
    assert d["pruned"] == int((nodes["pushed"] == 0).sum())


def _same_as_restatement(d, zones, plan, wave, **kw):
    seed, start, prior = plan
    r = R.Planner(_setup(orc.Oracle(), zones, seed), seed).plan(start, list(prior), streams=1, wave=wave, **kw)
    _same_policy(d, r)
    _same_counts(d, r)


def _raw_batch(e, plans, **kw):
    """the C call itself, for its return value"""
    st = np.ascontiguousarray([p[1] for p in plans], dtype=np.float64)
    pr = np.ascontiguousarray([p[2] for p in plans], dtype=np.float64)
    sd = np.ascontiguousarray([p[0] for p in plans], dtype=np.uint64)
    return e._l.porrt_tamp_rrt_plan_batch(e._c, len(plans), st.ctypes.data, pr.ctypes.data, sd.ctypes.data, None, pr.shape[1], 0.1, 2.0,
                                          kw.get("n_iter_min", 2500), kw.get("n_iter_max", 10000), 0.05, 128)


@pytest.mark.parametrize("wave", [1, 8])
def test_two_goals_five_plans(po, wave):
    e = _engine(po, Z2, 9, wave=wave)
    out = _batch(e, TWO)
    assert [d["status"] for d in out] == [0] * len(TWO)
    for p, (d, plan) in enumerate(zip(out, TWO)):
        _same_as_single(po, e, p, d, Z2, plan, wave)
        assert d["wave"] == wave and d["streams"] == 1
    _same_as_restatement(out[1], Z2, TWO[1], wave)


@pytest.mark.parametrize("wave", [1, 7])
def test_a_mixed_batch(po, wave):
    e = _engine(po, Z4, 9, wave=wave)
    out = _batch(e, MIXED)
    assert [d["status"] for d in out] == [0] * len(MIXED)
    for p, (d, plan) in enumerate(zip(out, MIXED)):
        _same_as_single(po, e, p, d, Z4, plan, wave)
    if wave == 1:
        _same_as_restatement(out[1], Z4, MIXED[1], wave)
    _same_policy(out[5], out[0])                                # the repeat is the first
    assert all(out[5][k] == out[0][k] for k in RECORD)
    n0, n5 = e.tamp_batch_bnb_nodes(0), e.tamp_batch_bnb_nodes(5)
    assert all(np.array_equal(n0[k].view(np.uint8), n5[k].view(np.uint8)) for k in n0)
    i = e.tamp_info()
    assert i["queries"] == sum(d["queries"] for d in out) and i["search_nodes"] == sum(d["search_nodes"] for d in out)
    assert i["pruned"] == sum(d["pruned"] for d in out) and 0 < i["waves"] <= max(d["waves"] for d in out)
    a = e.tamp_astar_info()
    assert a["speculated"] == 0 and a["arena_states"] >= a["arena_used"] > 0


@pytest.mark.parametrize("wave", [1, 7])
def test_chunk_cuts_change_nothing(po, wave):
    """tamp_pool 5 cuts inside a node's children (the root has 4, a wave of 7 nodes up to 21) and between plans; a first arena of
    1024 states has to grow between gathers"""
    whole = _engine(po, Z4, 9, wave=wave)
    want = _batch(whole, MIXED)
    e = _engine(po, Z4, 9, wave=wave, pool=5)
    e.set_option("tamp_arena_states", 1024)
    out = _batch(e, MIXED)
    assert e.tamp_info()["pool"] == 5 and e.tamp_astar_info()["arena_grown"] > 0
    for p, (d, w) in enumerate(zip(out, want)):
        assert d["status"] == 0 and all(d[k] == w[k] for k in RECORD)
        _same_policy(d, w)
        n, m = e.tamp_batch_bnb_nodes(p), whole.tamp_batch_bnb_nodes(p)
        assert all(np.array_equal(n[k].view(np.uint8), m[k].view(np.uint8)) for k in n)
        _same_as_single(po, e, p, d, Z4, MIXED[p], wave)


def test_discrete_seeds(po):
    plan = MIXED[1]
    e = _engine(po, Z4, 9, wave=1)
    out = _batch(e, [plan, plan, MIXED[2]], dseeds=[11, plan[0], 12])
    nodes = [e.tamp_batch_bnb_nodes(p) for p in range(3)]
    _same_as_single(po, e, 0, out[0], Z4, plan, 1, dseed=11)
    _same_as_single(po, e, 1, out[1], Z4, plan, 1)               # discrete_seeds[p] == seeds[p]: what set_sampler alone leaves
    _same_as_single(po, e, 2, out[2], Z4, MIXED[2], 1, dseed=12)
    # the shuffles differ, so the searches do: other children in other orders
    assert not (np.array_equal(nodes[0]["targets"], nodes[1]["targets"]) and np.array_equal(nodes[0]["parents"], nodes[1]["parents"]))
    # the best order is the minimum over all orders of a cost that is a function of the zone prefix: the same whatever the shuffles
    assert out[0]["search_cost"] == out[1]["search_cost"] and out[0]["zone_order"] == out[1]["zone_order"]
    _same_policy(dict(out[0], search_nodes=0), dict(out[1], search_nodes=0))


def test_a_failing_plan_does_not_stop_the_others(po):
    """On the shelf raster every plan must fail (below), so the failing plan among good ones is made with a tight iteration budget
    on the 6-free-goal raster instead: with 2300 iterations the plan of seed 3 finds no observation path for a child of its second
    wave, the plans of seeds 0 and 4 find all theirs."""
    kw = dict(n_iter_min=2300, n_iter_max=2300)
    u6 = tuple([1.0 / 6] * 6)
    plans = [(0, START, u6), (3, START, u6), (4, START, u6)]
    e = _engine(po, Z6, 0, wave=8)
    out = _batch(e, plans, **kw)
    assert [d["status"] for d in out] == [0, -10, 0]
    for p, (d, plan) in enumerate(zip(out, plans)):
        _same_as_single(po, e, p, d, Z6, plan, 8, **kw)
    bad = out[1]
    assert bad["fail_query"] == 0 and bad["fail_node"] > 6       # not in the root's wave: nodes 1 .. 6 are the root's children
    assert len(e.tamp_batch_bnb_nodes(1)["parents"]) == bad["search_nodes"] > bad["fail_node"]
    with pytest.raises(po.engine.PorrtError):                    # a failed plan has no policy to read
        e._chk(e._l.porrt_tamp_batch_policy(e._c, 1, None, None, None, None, 0, None))
    assert _raw_batch(e, plans, **kw) == 2                       # the return value counts the good plans


def test_every_plan_of_the_shelf_raster_fails_as_its_single_plan(po):
    """Raster 4_goals_zone_ids: the centroids of zones 1 and 2 lie inside shelves and a branch and bound runs the pickup query of
    every zone below its root whatever the prior, so every plan on that raster must fail: the batch is of failing plans only."""
    plans = [(0, START, U4), (1, (-0.6, -0.9), (0.4, 0.3, 0.2, 0.1)), (2, START, (0.97, 0.01, 0.01, 0.01))]
    for wave in (1, 8):
        e = _engine(po, Z4_SHELVES, 0, wave=wave)
        out = _batch(e, plans, n_iter_max=2500)                  # no exception
        assert [d["status"] for d in out] == [-10, -10, -10]
        for p, (d, plan) in enumerate(zip(out, plans)):
            _same_as_single(po, e, p, d, Z4_SHELVES, plan, wave, n_iter_max=2500)
            assert 1 <= d["fail_node"] <= 4 and d["search_nodes"] == 5     # a child of the root: the first wave is the root alone
            assert len(e.tamp_batch_bnb_nodes(p)["parents"]) == 5      # the nodes of a failed plan are readable
            with pytest.raises(po.engine.PorrtError):                  # a failed plan has no policy to read
                e._chk(e._l.porrt_tamp_batch_policy(e._c, p, None, None, None, None, 0, None))
        assert _raw_batch(e, plans, n_iter_max=2500) == 0


def test_six_goals_two_plans(po):
    u6 = tuple([1.0 / 6] * 6)
    plans = [(0, START, u6), (1, (-0.6, -0.9), (0.3, 0.2, 0.2, 0.1, 0.1, 0.1))]
    e = _engine(po, Z6, 3, wave=8)
    out = _batch(e, plans)
    assert [d["status"] for d in out] == [0, 0]
    for p, (d, plan) in enumerate(zip(out, plans)):
        _same_as_single(po, e, p, d, Z6, plan, 8)
    assert _raw_batch(e, plans) == 2                             # the return value counts the plans with a policy


def test_a_batch_of_one_and_what_it_leaves(po):
    plan = MIXED[1]
    e = _engine(po, Z4, 5, wave=7)               # the lead's own seed is not the plan's: the plan's streams are seeds[p]'s
    out = _batch(e, [plan])
    assert len(out) == 1
    _same_as_single(po, e, 0, out[0], Z4, plan, 7)
    # the batch replaced the last single plan, and its nodes are not an A* batch's
    with pytest.raises(po.engine.PorrtError) as ex:
        e._tamp_policy(0, 4)
    assert ex.value.code == -1
    with pytest.raises(po.engine.PorrtError) as ex:
        e.tamp_batch_astar_nodes(0)
    assert ex.value.code == -1
    # seeds = None: the lead's sampler seed, for the streams and for the plan's discrete sampler
    e1 = _engine(po, Z4, plan[0], wave=7)
    none = e1.plan_tamp_rrt_batch([plan[1]], [plan[2]])
    _same_as_single(po, e1, 0, none[0], Z4, plan, 7)
    # continuous stream and discrete sampler untouched: a single plan on the lead is that of a fresh engine
    lead = (5, START, U4)
    after = e.plan_tamp_rrt(START, list(U4))
    fresh, _, _ = _single(po, Z4, lead, 7)
    _same_policy(after, fresh)
    _same_counts(after, fresh)
    # and the other way round: after an A* batch the branch-and-bound nodes are refused
    e.plan_tamp_rrt_astar_batch([START], [U4], [0])
    assert len(e.tamp_batch_astar_nodes(0)["parents"]) > 0
    with pytest.raises(po.engine.PorrtError) as ex:
        e.tamp_batch_bnb_nodes(0)
    assert ex.value.code == -1


def test_refusals(po):
    good = [(0, START, U4), (1, START, U4), (2, START, U4)]
    e = _engine(po, Z4, wave=7)
    first = _batch(e, good[:1])[0]

    def still_there():
        rec = po.engine.TampBatchPlan()
        assert e._l.porrt_tamp_batch_get_plan(e._c, 0, C.byref(rec)) == 0
        assert (rec.status, rec.search_nodes, rec.queries, rec.search_cost) == (0, first["search_nodes"], first["queries"], first["search_cost"])
        assert len(e.tamp_batch_bnb_nodes(0)["parents"]) == first["search_nodes"]

    def refused(plans, named=None, text=None):
        with pytest.raises(po.engine.PorrtError) as ex:
            _batch(e, plans)
        assert ex.value.code == -1
        if named is not None:
            assert "plan %d" % named in str(ex.value)
        if text is not None:
            assert text in str(ex.value)
        still_there()

    e.set_option("tamp_streams", 0)
    refused(good)                                                # one continuous stream cannot be shared
    e.set_option("tamp_streams", 1)
    e.set_option("tamp_search", 1)
    refused(good, text="porrt_tamp_rrt_plan_astar")             # porrt_tamp_rrt_plan's message
    e.set_option("tamp_search", 0)
    refused([good[0], good[1], (2, START, (0.3, 0.3, 0.3, 0.3))], named=2)         # a wrong sum
    refused([(0, START, (0.5, 0.25, 0.25))])                                        # n_worlds is not the zone count
    refused([])                                                                     # n_plans 0
    assert e._l.porrt_tamp_rrt_plan_batch(e._c, 65537, None, None, None, None, 4, 0.1, 2.0, 2500, 10000, 0.05, 128) == -1
    st = np.zeros((1, 2))
    assert e._l.porrt_tamp_rrt_plan_batch(e._c, 1, st.ctypes.data, None, None, None, 4, 0.1, 2.0, 2500, 10000, 0.05, 128) == -1      # NULL priors
    still_there()
    # a zero entry is allowed here (unlike in the A* batch)
    zero = _batch(e, [(1, START, (0.5, 0.0, 0.25, 0.25))])
    assert zero[0]["status"] == 0
    _same_as_single(po, e, 0, zero[0], Z4, (1, START, (0.5, 0.0, 0.25, 0.25)), 7)
    fresh = _engine(po, Z4)
    rec = po.engine.TampBatchPlan()
    assert fresh._l.porrt_tamp_batch_get_plan(fresh._c, 0, C.byref(rec)) == -1                        # no batch has run


def test_cpp_mirror_batch_is_the_single_plans(po, tmp_path):
    """MapShelfDomainTampRRT::plan_batch (include/porrt.hpp) against plan(.., BranchAndBound) alone, in a program of its own"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "po_rrt_amd")
    exe = str(tmp_path / "bnb_batch_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(root, "tests", "bnb_batch_mirror.cpp"),
                    "-L" + lib, "-lporrt_hip", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe, os.path.join(cases.MAPS, GRID + ".pgm"), os.path.join(cases.MAPS, Z4 + ".pgm"), "4"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "bnb_batch_mirror ok" in out.stdout, out.stdout + out.stderr
