"""GPU parity of the multi-modal PRM planner after the growth (porrt_mm_*: build_belief_graph, expected costs, policy, refinement;
map_shelves_tamp_prm.rs:310-326, 395-485) against the restatement of tests/mm_plan_ref.py on the oracle's growth, bit for bit."""
import numpy as np
import pytest

import cases
import mm_plan_ref as ref
import refine_ref
from oracle import orc

pytestmark = pytest.mark.gpu


def bench_case(zones, seed):
    c = cases.cfg2(10)
    c.update(zones=zones, visibility=0.5)
    return cases.Case(c, seed=seed)


def both(case, belief, n_iter_per_belief, max_step, search_radius, seed):
    import po_rrt_amd
    e = cases.configure(po_rrt_amd.Engine(), case)
    o = cases.configure(orc.Oracle(), case)
    e.set_discrete_seed(seed)
    o.set_discrete_seed(seed)
    e.grow_mm_prm(case.start, belief, max_step, search_radius, n_iter_per_belief)
    _, bg, dist = ref.plan(o, case.start, belief, max_step, search_radius, n_iter_per_belief)
    e.mm_build_belief_graph()
    return e, o, bg, dist


def assert_graph(e, bg):
    got = e.mm_belief_graph()
    assert np.array_equal(got["types"], bg["types"])
    assert np.array_equal(got["belief_ids"], bg["belief_ids"])
    assert np.array_equal(got["mode_offsets"], bg["mode_offsets"])
    assert np.array_equal(got["finals"], bg["finals"])
    for k in ("children", "parents"):
        off, ids = ref.csr(bg[k])
        assert np.array_equal(got[k][0], off) and np.array_equal(got[k][1], ids), k


def assert_dist(d, want):
    assert np.array_equal(d.view(np.uint64), want.view(np.uint64)), "expected costs differ (%d of %d)" % ((d != want).sum(), len(d))


def assert_policy(e, bg, dist):
    (oid, par, leaf, xy), cost = e.mm_extract_policy()
    oid2, par2, leaf2 = ref.extract_policy(bg, dist)
    assert np.array_equal(oid, oid2) and np.array_equal(par, par2) and np.array_equal(leaf, leaf2)
    assert np.array_equal(xy.view(np.uint64), bg["xy"][oid.astype(np.int64)].view(np.uint64))
    assert np.float64(cost).view(np.uint64) == np.float64(dist[0]).view(np.uint64)
    return oid, par


def test_two_shelves():
    case = cases.cfg3(1500, 1500)
    e, o, bg, dist = both(case, [0.5, 0.5], 2000, 0.1, 2.0, 0)
    assert_graph(e, bg)
    assert_dist(e.mm_expected_costs(), dist)


def test_twelve_shelves():
    """the uniform 12-shelf prior: more than a thousand modes, a dozen levels; the root is +inf (centroids on shelves)"""
    case = cases.cfg4(1500, 1500)
    e, o, bg, dist = both(case, [1.0 / 12] * 12, 20, 0.05, 5.0, 0)
    assert len(bg["mode_offsets"]) > 1000
    assert_graph(e, bg)
    assert_dist(e.mm_expected_costs(), dist)
    assert not e.mm_dp_info()["level_schedule"]                            # the general sweeps by default
    e.set_option("mm_levels", 1)
    assert_dist(e.mm_expected_costs(), dist)
    info = e.mm_dp_info()
    assert info["level_schedule"] and info["launches"] == info["levels"] and info["levels"] >= 10
    with pytest.raises(RuntimeError):
        e.mm_extract_policy()                                              # no policy from an infinite root


@pytest.mark.parametrize("seed", [0])
def test_benchmark_two_goals(seed):
    case = bench_case("map_benchmark_like_2_goals_zone_ids", seed)
    e, o, bg, dist = both(case, [0.5, 0.5], 1000, 0.1, 2.0, seed)
    assert np.isfinite(dist[0])
    assert_graph(e, bg)
    assert_dist(e.mm_expected_costs(), dist)
    assert_policy(e, bg, dist)


def test_benchmark_two_goals_infinite_root():
    """seed 1 at 1000 samples per belief does not connect: the costs compute, the walk is refused"""
    case = bench_case("map_benchmark_like_2_goals_zone_ids", 1)
    e, o, bg, dist = both(case, [0.5, 0.5], 1000, 0.1, 2.0, 1)
    assert not np.isfinite(dist[0])
    assert_dist(e.mm_expected_costs(), dist)
    with pytest.raises(RuntimeError):
        e.mm_extract_policy()
    with pytest.raises(RuntimeError):
        e.mm_refine_policy(100)


@pytest.mark.parametrize("nw,n,seed", [(4, 2000, 0), (8, 1000, 1)])
def test_free_centroid_zones(nw, n, seed):
    case = bench_case("map_benchmark_like_%d_free_zone_ids" % nw, seed)
    e, o, bg, dist = both(case, [1.0 / nw] * nw, n, 0.1, 2.0, seed)
    assert np.isfinite(dist[0])
    assert_graph(e, bg)
    assert_dist(e.mm_expected_costs(), dist)
    assert_policy(e, bg, dist)


def test_level_schedule_equals_general_sweeps_and_lds_limit():
    case = bench_case("map_benchmark_like_4_free_zone_ids", 1)
    e, o, bg, dist = both(case, [0.25] * 4, 2000, 0.1, 2.0, 1)
    sizes = np.diff(bg["mode_offsets"].astype(np.int64))
    assert sizes.max() > 2000 and sizes.min() < 2000                      # "mixed": modes on both paths of the level kernel in one launch
    runs = {}
    e.set_option("mm_levels", 1)
    for name, opts in (("levels", {}), ("sweeps", {"dp_sweeps": 1}), ("global", {"mm_lds_nodes": 0}), ("mixed", {"mm_lds_nodes": 2000})):
        e.set_option("dp_sweeps", opts.get("dp_sweeps", 0))
        e.set_option("mm_lds_nodes", opts.get("mm_lds_nodes", 6400))
        runs[name] = (e.mm_expected_costs(), e.mm_dp_info())
    for name, (d, info) in runs.items():
        assert_dist(d, dist)
        assert info["level_schedule"] == (name != "sweeps"), name
    assert runs["levels"][1]["levels"] == 4 and runs["levels"][1]["launches"] == 4
    e.set_option("dp_sweeps", 0)
    e.set_option("mm_lds_nodes", 6400)


def test_refined_policy_and_plan():
    case = bench_case("map_benchmark_like_2_goals_zone_ids", 0)
    e, o, bg, dist = both(case, [0.5, 0.5], 1000, 0.1, 2.0, 0)
    e.mm_expected_costs()
    oid, par = assert_policy(e, bg, dist)
    got = e.mm_refine_policy(1500)
    want = refine_ref.refine(o, bg["xy"][oid.astype(np.int64)], par, oid, bg["belief_vec"][oid.astype(np.int64)], bg["beliefs"], 1500)
    (x, oid_r, par_r, leaf_r), cost = got
    (x2, oid2, par2, leaf2), cost2 = want
    assert np.array_equal(x.view(np.uint64), x2.view(np.uint64)) and np.array_equal(oid_r, oid2) and np.array_equal(par_r, par2)
    assert np.array_equal(leaf_r, leaf2) and np.float64(cost).view(np.uint64) == np.float64(cost2).view(np.uint64)
    assert cost <= dist[0]
    secs = e.mm_plan_seconds()
    assert secs["build_device_s"] > 0 and secs["costs_device_s"] > 0 and secs["refine_s"] > 0
    # plan(): the four steps in one call, from the same samplers' state
    import po_rrt_amd
    p = cases.configure(po_rrt_amd.Engine(), case)
    p.set_discrete_seed(0)
    (oid_p, par_p, leaf_p, xy_p), cost_p = p.plan_mm_prm(case.start, [0.5, 0.5], 0.1, 2.0, 1000)
    assert np.array_equal(oid_p, oid) and np.array_equal(par_p, par) and cost_p == dist[0]
    assert p.mm_plan_seconds()["grow_s"] > 0


def test_stale_and_missing_steps_are_errors():
    import po_rrt_amd
    case = bench_case("map_benchmark_like_2_goals_zone_ids", 0)
    e = cases.configure(po_rrt_amd.Engine(), case)
    with pytest.raises(RuntimeError):
        e.mm_build_belief_graph()                                          # no grow_mm_prm first
    with pytest.raises(RuntimeError):
        e.mm_expected_costs()
    e.set_discrete_seed(0)
    e.grow_mm_prm(case.start, [0.5, 0.5], 0.1, 2.0, 1000)
    with pytest.raises(RuntimeError):
        e.mm_expected_costs()                                              # no belief graph yet
    e.mm_build_belief_graph()
    d = e.mm_expected_costs()
    e.mm_extract_policy()
    e.grow_mm_prm(case.start, [0.5, 0.5], 0.1, 2.0, 300)                  # everything built on the old modes is stale now
    for call in (lambda: e.mm_expected_costs(compute=False), e.mm_compute_expected_costs, e.mm_extract_policy, lambda: e.mm_refine_policy(10),
                 e.mm_belief_graph):
        with pytest.raises(RuntimeError):
            call()
    e.mm_build_belief_graph()
    assert len(e.mm_expected_costs()) != len(d)


def test_single_and_batched_extraction_share_their_states():
    """mm_extract_policy() and mm_extract_policies([0])[0] hand out the same states, bit for bit.  On the two-shelf case the root's cost
    is +inf, so both refuse there and the states of whatever policies the finite starts have are checked against the graph's; the
    two-goal case has a policy from the root."""
    case = cases.cfg3(1500, 1500)
    e, o, bg, dist = both(case, [0.5, 0.5], 2000, 0.1, 2.0, 0)
    assert_dist(e.mm_expected_costs(), dist)
    assert not np.isfinite(dist[0])
    with pytest.raises(RuntimeError):
        e.mm_extract_policy()
    starts = [0] + np.flatnonzero(np.isfinite(dist))[:8].tolist()
    got, status = e.mm_extract_policies(starts)
    assert status[0] == 1 and got[0] is None
    for g in (g for g in got if g is not None):
        oid, xy = g[0][0], g[0][3]
        assert np.array_equal(xy.view(np.uint64), bg["xy"][oid.astype(np.int64)].view(np.uint64))
    case = bench_case("map_benchmark_like_2_goals_zone_ids", 0)
    e, o, bg, dist = both(case, [0.5, 0.5], 1000, 0.1, 2.0, 0)
    e.mm_expected_costs()
    (oid, par, leaf, xy), cost = e.mm_extract_policy()
    got, status = e.mm_extract_policies([0])
    assert status[0] == 0
    (oid_b, par_b, leaf_b, xy_b), cost_b = got[0]
    assert np.array_equal(oid, oid_b) and np.array_equal(par, par_b) and np.array_equal(leaf, leaf_b)
    assert xy.tobytes() == xy_b.tobytes() and np.float64(cost).view(np.uint64) == np.float64(cost_b).view(np.uint64)
    assert np.array_equal(xy.view(np.uint64), bg["xy"][oid.astype(np.int64)].view(np.uint64))
