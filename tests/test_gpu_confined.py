"""GPU parity of the growth in confined sampler windows and at other step geometries (tests/confined_inputs.py; the oracle's side, with
everything an input was built to produce asserted from the oracle's output, is tests/test_confined_inputs_cpu.py).

  one region      every node in one region of the page grid: page directories of 43 .. 65 levels (gscan_disc's level loop, gscan_region,
                  scan_disc, the clone workgroup), up to 16 new pages of one region in one step (insert_step_pages, file_step_fast),
                  every sample heavy, neighbour lists beyond the default cand_cap: the list replay at the defaults, its capacity
                  clamped to the tree's
  region corner   four such regions around one corner on the benchmark-like raster
  PTO windows     hundreds of edges per node: the edge-pool replay at the default edge_per_node
  PRM window      a roadmap of 2001 nodes and more than a million edges in one region
  geometries      max_step 0.5 (a disc meets 21 x 21 regions: the young tree's id-ordered streaming lasts until 7056 nodes; no LDS tile,
                  rays of 50 pixels), max_step 0.02, the radius equal to max_step or below it for a whole run, either side of the limit
                  of the LDS tile (TW = 63)

No option is set to reach any of this: the replays and capacities are the defaults', and what the options name here are the launch
forms that the other files enumerate.  Every comparison is assert_same of test_gpu_parity.py against the oracle, bit for bit."""
import numpy as np
import pytest

import cases
import confined_inputs as W
from test_gpu_parity import assert_same
from test_gpu_prm import assert_same_roadmap

pytestmark = pytest.mark.gpu

DEFAULT_CAND_CAP, DEFAULT_EDGE_PER_NODE = 2048, 256


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


_ORC = {}


def oracle(case, K, grows=1):
    """(the oracle grown `grows` times on the case, the last return code): made once per module, read only"""
    key = (case.name, case.seed, case.n_iter_min, case.n_iter_max, case.max_step, case.search_radius, K, grows)
    if key not in _ORC:
        _ORC[key] = W.oracle(case, K, grows=grows)
    return _ORC[key]


def engine(eng_mod, case, **opts):
    e = eng_mod.Engine()
    for k, v in opts.items():
        e.set_option(k, v)
    return W.configure(e, case)


def grown_cand_cap(case):
    """the default capacity after one list replay: four times as large, clamped to the tree's capacity (n_iter_max + 2)"""
    return min(4 * DEFAULT_CAND_CAP, case.n_iter_max + 2)


def grow_rows(eng_mod, cs, K, **opts):
    """the cases as the rows of one grow_batch through the group kernels"""
    opts.setdefault("group_lanes", 16)
    engs = [engine(eng_mod, c, **opts) for c in cs]
    c0 = cs[0]
    assert all(c.max_step == c0.max_step and c.search_radius == c0.search_radius for c in cs)
    eng_mod.Engine.grow_batch(engs, [c.start for c in cs], c0.max_step, c0.search_radius, [c.n_iter_min for c in cs], K)
    for k, v in opts.items():
        if k != "early_wave_steps":                               # (an option without a getter)
            assert engs[0].get_option(k) == v, "%s was not in force" % k
    return engs


# ---------------------------------------------------------------------------------------------------------------- single query
FORMS = [dict(), dict(pipeline=0), dict(pipeline=0, graph=0), dict(graph=0)]
form_id = lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults"


@pytest.mark.parametrize("K", [64, 256, 1024])
def test_one_region_single_query(eng_mod, K):
    """(1): the lists outgrow the default cand_cap, so the growth is replayed with 8192 clamped to n_iter_max + 2; the second grow on the
    same context starts with that capacity, its sampler moved on"""
    case = W.one_region(W.ONE_REGION_ITERS[K])
    e = engine(eng_mod, case)
    assert e.get_option("cand_cap") == DEFAULT_CAND_CAP
    for grows in (1, 2):
        cases.grow(e, case, K=K)
        assert_same(e, oracle(case, K, grows)[0])
        assert e.get_option("cand_cap") == grown_cand_cap(case) > DEFAULT_CAND_CAP


@pytest.mark.parametrize("opts", FORMS[1:], ids=form_id)
@pytest.mark.parametrize("make", [W.one_region, W.one_region_raster, W.corner_window], ids=lambda f: f.__name__)
def test_windows_single_query_forms(eng_mod, make, opts):
    case = make()
    e = engine(eng_mod, case, **opts)
    cases.grow(e, case, K=256)
    assert_same(e, oracle(case, 256)[0])
    assert e.get_option("cand_cap") == grown_cand_cap(case)


@pytest.mark.parametrize("make", [W.one_region_raster, W.corner_window], ids=lambda f: f.__name__)
def test_windows_single_query(eng_mod, make):
    """(2), (3) at the defaults, and a second grow"""
    case = make()
    e = engine(eng_mod, case)
    for grows in (1, 2):
        cases.grow(e, case, K=256)
        assert_same(e, oracle(case, 256, grows)[0])
        assert e.get_option("cand_cap") == grown_cand_cap(case)


@pytest.mark.parametrize("opts", FORMS[:2], ids=form_id)
@pytest.mark.parametrize("name", sorted(W.GEOMETRIES))
def test_geometries_single_query(eng_mod, name, opts):
    case = W.geometry(name)
    e = engine(eng_mod, case, **opts)
    cases.grow(e, case, K=W.GEOMETRY_K)
    assert_same(e, oracle(case, W.GEOMETRY_K)[0])


# ---------------------------------------------------------------------------------------------------------------- group kernels
ROW_FORMS = [dict(conn_wg_waves=4), dict(conn_wg_waves=1, commit_flat=0), dict(conn_wg_waves=1, commit_flat=1),
             dict(conn_wg_waves=1, riders_fast=0), dict(conn_wg_waves=1, riders_fast=1)]


def check_heavy_rows(engs, cs, K):
    """every row against its oracle; every row had samples with more hits than their LDS list holds; and the lists of the rows of one
    region overflowed at the default capacity (the corner's do for some seeds): the batch was replayed with larger ones for every row"""
    for e, c in zip(engs, cs):
        assert_same(e, oracle(c, K)[0])
        assert e.get_option("n_heavy") > 0
        if c.name.startswith("one_region"):
            assert e.get_option("cand_cap") == grown_cand_cap(c) > DEFAULT_CAND_CAP


@pytest.mark.parametrize("opts", ROW_FORMS, ids=form_id)
@pytest.mark.parametrize("rows", [8, 3])
@pytest.mark.parametrize("make", [W.one_region, W.corner_window], ids=lambda f: f.__name__)
def test_window_rows(eng_mod, make, rows, opts):
    """8 rows take the XCD dealing of the rows, 3 do not; every row a window of its own seed.  A row's overflow replays the batch."""
    cs = [make(seed=s) for s in W.SEEDS[:rows]]
    check_heavy_rows(grow_rows(eng_mod, cs, 256, **opts), cs, 256)


@pytest.mark.parametrize("opts", [dict(early_wave_steps=0), dict(group_lanes=64), dict(group_lanes=64, conn_wg_waves=1)], ids=form_id)
def test_one_region_rows_other_forms(eng_mod, opts):
    cs = [W.one_region(seed=s) for s in W.SEEDS[:3]]
    check_heavy_rows(grow_rows(eng_mod, cs, 256, **opts), cs, 256)


@pytest.mark.parametrize("waves", [1, 4])
def test_one_region_rows_sixteen_pages_a_step(eng_mod, waves):
    """K = 1024: all samples of a step in one region, need = 16 in file_step_fast"""
    cs = [W.one_region(W.ONE_REGION_ITERS[1024], seed=s) for s in W.SEEDS]
    check_heavy_rows(grow_rows(eng_mod, cs, 1024, conn_wg_waves=waves), cs, 1024)


@pytest.mark.parametrize("waves", [1, 4])
def test_one_region_rows_three_steps_of_2048(eng_mod, waves):
    """K = 2048 keeps insert_step_pages<1>: three steps, 32 new pages of one region in each"""
    cs = [W.one_region(3 * 2048, seed=s) for s in W.SEEDS[:3]]
    check_heavy_rows(grow_rows(eng_mod, cs, 2048, conn_wg_waves=waves), cs, 2048)


def ordinary(raster, seed):
    """a row on the whole map with the step lengths of the one-region rows beside it"""
    c = cases.cfg2(2000, seed=seed) if raster else cases.empty_space(2000, 2000, seed=seed)
    c.update(search_radius=W.one_region().search_radius)
    return c


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("raster", [True, False], ids=["raster", "no_raster"])
def test_heavy_and_ordinary_rows_side_by_side(eng_mod, raster, waves):
    """Rows of one region beside rows on the whole map: descriptors of different sizes in one launch.  The rows of a batch share their
    LDS tile (grow_batch refuses a row without raster beside one with), so cfg2(2000) runs beside the rows of (2), which have a
    raster, and the rows of (1) beside the empty map."""
    make = W.one_region_raster if raster else W.one_region
    cs = [make(seed=s) if s % 2 == 0 else ordinary(raster, s) for s in W.SEEDS]
    engs = grow_rows(eng_mod, cs, 256, conn_wg_waves=waves)
    for e, c in zip(engs, cs):
        assert_same(e, oracle(c, 256)[0])
    assert all(e.get_option("n_heavy") > 0 for e in engs[::2]) and engs[0].get_option("cand_cap") > DEFAULT_CAND_CAP


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("name", ["long_steps_fixed_radius", "long_steps_shrinking_radius"])
def test_long_step_rows(eng_mod, name, waves):
    """max_step 0.5 as eight rows: the r0 loop over 441 regions, the hand-over to the pages late in the run or never.  With the fixed
    radius one row runs 8500 iterations, to the hand-over and beyond, and seven end at 2500 (the oracle takes seconds for a long row;
    the single query runs the whole length)."""
    n_iter = [None if name != "long_steps_fixed_radius" else 8500 if s == 0 else 2500 for s in W.SEEDS]
    cs = [W.geometry(name, seed=s, n_iter=n) for s, n in zip(W.SEEDS, n_iter)]
    engs = grow_rows(eng_mod, cs, W.GEOMETRY_K, conn_wg_waves=waves)
    for e, c in zip(engs, cs):
        o = oracle(c, W.GEOMETRY_K)[0]
        assert_same(e, o)
    if name == "long_steps_fixed_radius":
        assert engs[0].num_nodes() > 16 * W.discs_regions(cs[0].max_step) > engs[1].num_nodes()


# ---------------------------------------------------------------------------------------------------------------- belief space
@pytest.mark.parametrize("make", [W.pto_shelf_window, W.pto_door_window], ids=lambda f: f.__name__)
def test_pto_window(eng_mod, make):
    """(4): more edges than the default pool of 256 per node holds, so the growth is replayed with 1024; then a second grow"""
    case = make()
    e = engine(eng_mod, case)
    assert e.get_option("edge_per_node") == DEFAULT_EDGE_PER_NODE
    for grows in (1, 2):
        o, rco = oracle(case, W.PTO_K, grows)
        assert cases.grow(e, case, K=W.PTO_K) == rco
        assert_same(e, o, pto=True)
        assert e.get_option("edge_per_node") == 4 * DEFAULT_EDGE_PER_NODE
    assert oracle(case, W.PTO_K)[1] == 1                          # "n_iter_max reached"


def test_pto_window_batch(eng_mod):
    """three members in windows of their own seeds.  A member of a batch is not replayed for its edge pool (the call fails and leaves no
    results, test_gpu_growth_replays.py), so every context first grows alone, which leaves it the capacity its window needs; the batch
    is then the contexts' second grow, against the oracles' second grow."""
    cs = [W.pto_shelf_window(seed=s) for s in (1, 2, 3)]
    engs = [engine(eng_mod, c) for c in cs]
    for e, c in zip(engs, cs):
        o, rco = oracle(c, W.PTO_K)
        assert len(o.edges()[0]) > DEFAULT_EDGE_PER_NODE * o.num_nodes()
        assert cases.grow(e, c, K=W.PTO_K) == rco
        assert e.get_option("edge_per_node") == 4 * DEFAULT_EDGE_PER_NODE
    eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, 1500, W.PTO_K, mode=cases.PTO)
    for e, c in zip(engs, cs):
        assert_same(e, oracle(c, W.PTO_K, grows=2)[0], pto=True)


@pytest.mark.parametrize("name", W.TILE_ROWS)
def test_pto_either_side_of_the_tile_limit(eng_mod, name):
    case = W.pto_tile(W.GEOMETRIES[name][0])
    e = engine(eng_mod, case)
    o, rco = oracle(case, W.PTO_K)
    assert cases.grow(e, case, K=W.PTO_K) == rco
    assert_same(e, o, pto=True)


# ---------------------------------------------------------------------------------------------------------------- roadmap
@pytest.mark.parametrize("host_ranks", [1, 0])
def test_prm_window(eng_mod, host_ranks):
    """(5): 2001 roadmap nodes in one region and 664 edges per node, more than the 256 the edge list starts with: porrt_grow_prm counts
    them and grows again from the sampler state it found.  The second roadmap on the same pair shows that state put back (its samples
    follow the first roadmap's), with the list now large enough.  Then paths inside the window and to a goal outside it."""
    e, o = W.prm_pair(eng_mod.Engine)
    e.set_option("host_ranks", host_ranks)
    for _ in range(2):
        for x in (e, o):
            x.grow_prm(W.PRM["start"], W.PRM["max_step"], W.PRM["search_radius"], W.PRM["n_iter"])
        assert len(o.edges()[0]) > 1000000
        assert_same_roadmap(e, o)
    for start, goal in W.PRM_QUERIES:
        pe, po = e.prm_plan_path(start, goal), o.prm_plan_path(start, goal)
        assert pe.shape == po.shape and np.array_equal(pe.view(np.uint64), po.view(np.uint64)) and len(po) >= 2
