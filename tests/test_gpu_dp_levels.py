"""The size-gated paths of the expected costs and of what feeds them, each compared with the oracle bit for bit and each with an
assertion that it actually ran:

* the layered conditional_dijkstra sweeps a level of N * W rows (N graph nodes, W beliefs of one number of possible worlds) with
  k_dp_level_sweep<1> ("wide": a workgroup = 256 beliefs of one node) when N * W >= option dp_wide_rows (default 2 << 20), with
  k_dp_level_sweep<4> ("split") otherwise; option "dp_wide_levels" says which levels of the last computation ran wide;
* the sweeps' item stamps repeat after 255 sweeps and outlive levels: computations of more than 510 sweeps;
* the policy walk (k_pol_walk) keeps the first kPolRowCache = 512 children of a policy node in LDS and reads the rest of a longer
  row again;
* k_eo_segsort sorts buckets of more than kSegLds = 512 entries from global memory (the PTO graph's adjacency, and the children /
  parents lists of the multi-modal belief graph)."""
import os

import numpy as np
import pytest

import cases
import make_golden_trees as mg
import make_maps
import test_gpu_dp as dp
import test_gpu_mm_plan as mm
import test_gpu_random_worlds as rw
from oracle import orc

pytestmark = pytest.mark.gpu

DEFAULT_WIDE_ROWS = 2 << 20
MODES = {"default": None, "wide": 0, "split": 1 << 62}


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def levels(e):
    """per level of the layered evaluation, fewest possible worlds first: (possible worlds, W beliefs, N * W rows)"""
    beliefs, types, _, _ = e.belief_graph(lists=False)
    N = len(types) // len(beliefs)
    support, W = np.unique((beliefs > 0).sum(axis=1), return_counts=True)
    return support, W, N * W.astype(np.int64)


def wide_mask(rows, threshold):
    return sum(1 << k for k, r in enumerate(rows) if r >= threshold)


def compare_modes(e, o, modes=MODES):
    """costs under each forced kernel (and the default) equal the oracle's, the policy too where the root is finite; returns
    {mode: dp_info()} and the oracle's costs"""
    do = o.expected_costs()
    pol = o.extract_policy(do) if np.isfinite(do[0]) else None
    support, W, rows = levels(e)
    out = {}
    for name, value in modes.items():
        e.set_option("dp_wide_rows", DEFAULT_WIDE_ROWS if value is None else value)
        assert e.get_option("dp_wide_rows") == (DEFAULT_WIDE_ROWS if value is None else value)
        e.compute_expected_costs()
        de = e.expected_costs()
        assert np.array_equal(de.view(np.uint64), do.view(np.uint64)), "%s: expected costs differ (%d of %d)" % (name, (de != do).sum(), len(de))
        assert e.get_option("dp_levels") == len(W)
        assert e.get_option("dp_wide_levels") == wide_mask(rows, DEFAULT_WIDE_ROWS if value is None else value), name
        if pol is not None:
            (oid, par, leaf), cost = e.extract_policy()
            assert cost == do[0] and np.array_equal(oid, pol[0]) and np.array_equal(par, pol[1]) and np.array_equal(leaf, pol[2]), name
        else:
            with pytest.raises(RuntimeError):
                e.extract_policy()
        out[name] = e.dp_info()
    e.set_option("dp_wide_rows", DEFAULT_WIDE_ROWS)
    return out, do, pol


def grown_pair(eng_mod, case, K, prior):
    e = cases.configure(eng_mod.Engine(), case)
    cases.grow(e, case, K=K)
    o = cases.configure(orc.Oracle(), case)
    cases.grow(o, case, K=K, algo=orc.ALGO_BATCHED_KD)
    e.build_belief_graph(prior)
    o.build_belief_graph(prior)
    return e, o


def twelve_worlds_case():
    case = cases.cfg4(700, 700)
    case.update(visibility=0.6, start=(0.0, -0.3))
    return case, 64, [1.0 / 12] * 12


CASES = dict(dp.GROWN, twelve_worlds=twelve_worlds_case)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forced_wide_split_and_default_equal_oracle(eng_mod, name):
    if name == "twelve_worlds":
        case, K, prior = twelve_worlds_case()
    else:
        mk, K, prior = dp.GROWN[name]
        case = mk()
    e, o = grown_pair(eng_mod, case, K, prior)
    infos, do, pol = compare_modes(e, o)
    support, W, rows = levels(e)
    assert all(r < DEFAULT_WIDE_ROWS for r in rows)            # these graphs are small: the default sweeps every level split
    if name == "twelve_worlds":
        assert sorted(set(W[W > 256].tolist())) == [495, 792, 924]     # several 256-belief chunks per node under the forced wide kernel
    if name == "shelf_2_worlds_until_complete":                # (e): a policy node with a long row (several passes of the walk's lanes)
        coff = e.belief_graph()[2][0]
        assert np.diff(coff.astype(np.int64))[pol[0].astype(np.int64)].max() > 255


def random_world_pair(eng_mod, seed):
    """the growth and prior of test_gpu_random_worlds.test_random_shelf_world_whole_chain (same draws)"""
    rng = np.random.default_rng(1000 + seed)
    a, z, goals = rw.random_shelf_world(rng)
    assert len(goals) >= 2
    e, o = rw.configure_pair(eng_mod, a, z, cases.SHELF, goals, float(rng.uniform(0.25, 0.6)), seed)
    n_iter, K = int(rng.integers(1500, 4000)), int(rng.choice([64, 256]))
    e.grow((0.0, -0.9), 0.05, 5.0, n_iter, n_iter, batch_K=K, mode=cases.PTO)
    o.grow((0.0, -0.9), 0.05, 5.0, n_iter, n_iter, batch_K=K, mode=cases.PTO, algo=orc.ALGO_BATCHED_KD)
    prior = rng.dirichlet(np.ones(len(goals)))
    if rng.random() < 0.5:
        prior[int(rng.integers(len(goals)))] = 0.0
        prior = prior / prior.sum()
    prior = list(prior / prior.sum())
    e.build_belief_graph(prior)
    o.build_belief_graph(prior)
    return e, o


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_worlds_forced_kernels(eng_mod, seed):
    e, o = random_world_pair(eng_mod, seed)
    compare_modes(e, o)


def test_frozen_255_beliefs_with_the_wide_kernel(eng_mod):
    """tests/golden/trees/pto_cfg4_20000_it_255_beliefs (the oracle's answers, frozen) with every level swept wide"""
    name = "pto_cfg4_20000_it_255_beliefs"
    case, K, _ = {n: (c, k, a) for n, c, k, a in mg.specs()}[name]
    gold = np.load(os.path.join(mg.OUT, name + ".npz"))
    e = cases.configure(eng_mod.Engine(), case)
    cases.grow(e, case, K=K)
    assert e.num_nodes() == int(gold["n_nodes"])
    e.build_belief_graph(mg.CFG4_PRIOR)
    support, W, rows = levels(e)
    for value in (0, 1 << 62):
        e.set_option("dp_wide_rows", value)
        e.compute_expected_costs()
        assert e.get_option("dp_wide_levels") == wide_mask(rows, value)
        d = e.expected_costs()
        assert mg.digest(d) == str(gold["cost_digest"]) and np.array_equal(d[:1].view(np.uint64), gold["root_cost_bits"])
        (oid, par, leaf), cost = e.extract_policy()
        assert np.array_equal(oid, gold["policy_ids"]) and np.array_equal(par, gold["policy_parents"]) and np.array_equal(leaf, gold["policy_leaf"])
        assert cost == d[0]
    assert e.get_option("dp_wide_levels") == 0 and wide_mask(rows, 0) == (1 << len(W)) - 1


def ring_world(n_goals=12, radius=0.6):
    """open floor, n_goals small shelves on a ring around the start, each a zone; goal k in front of shelf k"""
    a = np.full((200, 200), 255, np.uint8)
    z = np.full((200, 200), 255, np.uint8)
    goals = []
    for k in range(n_goals):
        t = 2.0 * np.pi * k / n_goals
        x, y = radius * np.cos(t), radius * np.sin(t)
        make_maps.rect(a, x - 0.06, y + 0.07, x + 0.06, y + 0.11, 200)
        make_maps.rect(z, x - 0.03, y + 0.08, x + 0.03, y + 0.10, k)
        goals.append((x, y))
    return a, z, goals


def test_wide_levels_at_the_real_threshold(eng_mod):
    """12 worlds, 4095 beliefs, ~2900 graph nodes: the levels of 5, 6 and 7 possible worlds (792, 924, 792 beliefs) pass 2 << 20 rows
    and run wide by default, the others split -- and nearly every row is finite, so the wide kernel's answers are not all +inf.  The
    oracle takes ~30 s here."""
    a, z, goals = ring_world()
    pair = []
    for mk in (eng_mod.Engine, orc.Oracle):
        x = mk()
        x.set_grid(a, (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
        x.set_zones(z, 0.6)
        x.set_sampler((-1.0, -1.0), (1.0, 1.0), 1)
        x.set_square_goal(np.array(goals, dtype=np.float64), np.array([1 << k for k in range(12)], dtype=np.uint64), 0.1)
        pair.append(x)
    e, o = pair
    e.grow((0.0, 0.0), 0.03, 5.0, 3000, 3000, batch_K=64, mode=cases.PTO)            # (a short step: many hops, many sweeps per level)
    o.grow((0.0, 0.0), 0.03, 5.0, 3000, 3000, batch_K=64, mode=cases.PTO, algo=orc.ALGO_BATCHED_KD)
    assert np.array_equal(e.tree()[1], o.tree()[1])
    e.build_belief_graph([1.0 / 12] * 12)
    o.build_belief_graph([1.0 / 12] * 12)
    infos, do, pol = compare_modes(e, o)
    support, W, rows = levels(e)
    N = len(do) // 4095
    wide = (rows >= DEFAULT_WIDE_ROWS) & (W > 256)
    assert wide.sum() >= 2 and (~wide).sum() >= 2                                      # mixed: both kernels in one computation
    sup = (o.belief_graph()[0] > 0).sum(axis=1)
    finite = np.isfinite(do.reshape(N, len(sup)))
    finite_wide = sum(int(finite[:, sup == s].sum()) for s in support[wide])
    assert finite_wide >= 3_000_000, finite_wide                                       # a real share of the ~7 M wide rows
    assert np.isfinite(do[0]) and pol is not None
    for name, info in infos.items():                                                   # (d) the item stamps wrap twice
        assert info["sweeps"] > 510, (name, info)


def test_dense_graph_long_buckets_and_policy_rows(eng_mod):
    """max_step 0.5, search radius 10: nodes found by more than 512 later ones (k_eo_segsort's global-memory branch) and policy
    nodes of more than 512 children (more than k_pol_walk's row cache; the oracle shows 595), both on lists equal to the oracle's"""
    case = cases.cfg3_near(3000)
    case.update(max_step=0.5, search_radius=10.0)
    e, o = grown_pair(eng_mod, case, 64, [0.5, 0.5])
    f, t, _ = o.edges()
    N = o.num_nodes()
    assert np.bincount(f, minlength=N).max() > 512 and np.bincount(t, minlength=N).max() > 512
    fe, te, _ = e.edges()
    assert np.array_equal(np.bincount(fe, minlength=N), np.bincount(f, minlength=N))
    be, ty, (ceo, ce), (peo, pe) = e.belief_graph()
    bo, to, (coo, co), (poo, po) = o.belief_graph()
    assert np.array_equal(ty, to) and np.array_equal(ceo, coo) and np.array_equal(ce, co) and np.array_equal(peo, poo) and np.array_equal(pe, po)
    infos, do, pol = compare_modes(e, o)
    assert pol is not None
    assert np.diff(coo.astype(np.int64))[pol[0].astype(np.int64)].max() > 512


@pytest.mark.parametrize("nw,n,max_step,search_radius,seed", [(6, 1100, 0.5, 10.0, 0), (12, 60, 0.5, 8.0, 0)])
def test_free_centroid_zones_dense(eng_mod, nw, n, max_step, search_radius, seed):
    """the 6- and 12-goal free-centroid rasters through porrt_mm_* against the numpy restatement, with long roadmap radii: policy rows
    of more than 512 children (more than k_pol_walk's row cache: 526 and 939 in the restatement), and (12 goals) belief graph rows of
    more than 512 sorted on the device"""
    case = mm.bench_case("map_benchmark_like_%d_free_zone_ids" % nw, seed)
    e, o, bg, dist = mm.both(case, [1.0 / nw] * nw, n, max_step, search_radius, seed)
    assert np.isfinite(dist[0])
    mm.assert_graph(e, bg)
    mm.assert_dist(e.mm_expected_costs(), dist)
    oid, par = mm.assert_policy(e, bg, dist)
    n_children = np.array([len(c) for c in bg["children"]])
    n_parents = np.array([len(c) for c in bg["parents"]])
    assert n_children[oid.astype(np.int64)].max() > 512
    if nw == 12:
        assert max(n_children.max(), n_parents.max()) > 512
