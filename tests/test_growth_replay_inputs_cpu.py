"""The oracle's side of the inputs of tests/test_gpu_growth_replays.py (tests/growth_replay_inputs.py): which (box, seed) streams hold
a redraw and where, that the far-box cases grow the same with and without the kd-tree, and how many edges the graphs have against
the pool sizes that the device tests name.  If one of these drifts, a device test would pass without the replay it was built for."""
import numpy as np
import pytest

import cases
import exact_inputs as X
import growth_replay_inputs as R
from oracle import orc


def far_box(L):
    return (L, -1.0), (L + 2.0, 1.0)


@pytest.mark.parametrize("L,seed,calls", [(R.FAR36, 8, [3458]), (R.FAR36, 0, []), (R.FAR38, 44, [148]), (R.FAR38, 24, [475, 3148])],
                         ids=["2^36-seed8", "2^36-seed0", "2^38-seed44", "2^38-seed24"])
def test_redraws_of_the_far_boxes(oracle_lib, L, seed, calls):
    """gen_range draws again while low + v * scale >= high: the state after such a call is more than two steps on"""
    assert R.redraw_calls(*far_box(L), seed, 4000) == calls


def test_iteration_of_a_sampler_call():
    assert [R.iteration_of_call(k) for k in (0, 98, 99, 148, 3458)] == [1, 99, 101, 150, 3493]


def test_advance_is_the_stream_without_redraws(oracle_lib):
    """on the unit box nothing is ever redrawn: 2 steps per call, whatever the jump"""
    a = orc.Pcg64.seed_from_u64(5)
    b = a.copy()
    for _ in range(100):
        a.gen_range_f64(-1.0, 1.0)
        a.gen_range_f64(-1.0, 1.0)
    b.advance(200)
    assert (a.state() == b.state()).all()
    assert R.redraw_calls((-1.0, -1.0), (1.0, 1.0), 5, 2000) == []


def grown(case, K, algo):
    o = cases.configure(orc.Oracle(), case)
    rc = cases.grow(o, case, K=K, algo=algo)
    return o, rc


@pytest.mark.parametrize("name,K", [("far_rrt0", 256), ("far_rrt8", 256), ("far_tail", 64), ("far_pto8", 256)])
def test_far_cases_grow_the_same_with_and_without_the_kd_tree(oracle_lib, name, K):
    case = {"far_rrt0": R.far_rrt(0), "far_rrt8": R.far_rrt(8), "far_tail": R.far_tail(), "far_pto8": R.far_pto(8)}[name]
    (a, rca), (b, rcb) = grown(case, K, orc.ALGO_BATCHED_KD), grown(case, K, orc.ALGO_BATCHED)
    assert rca == rcb and a.num_iterations() == b.num_iterations()
    for u, v in zip(a.tree(), b.tree()):
        assert np.array_equal(u, v)
    assert np.array_equal(a.final_ids(), b.final_ids())
    x = a.tree()[0]
    assert (x[:, 0] >= case.low[0]).all() and (x[:, 0] < case.up[0]).all(), "the growth left the far box"
    if name == "far_rrt8":
        assert (a.num_nodes(), len(a.final_ids())) == (3762, 19)
    if name == "far_tail":
        assert 150 < a.num_iterations() < case.n_iter_max          # the run passes the redraw of iteration 150 and stops on its goal
    if name == "far_pto8":
        assert len(a.edges()[0]) == 148278 < R.edge_pool(case.n_iter_max, 256)[0]      # no edge replay beside the redraw


@pytest.mark.parametrize("name,K,n_edges,replays,per_node", [("pto_1500", 256, 68952, 3, 64), ("door_1500", 256, 50637, 3, 64),
                                                             ("pto_tail", 100, 55841, 2, 16), ("pto_tail", 256, 218373, 3, 64)])
def test_edge_counts_against_the_pools(oracle_lib, name, K, n_edges, replays, per_node):
    case = {"pto_1500": R.pto_1500(), "door_1500": R.door_1500(), "pto_tail": R.pto_tail()}[name]
    o, _ = grown(case, K, orc.ALGO_BATCHED_KD)
    assert len(o.edges()[0]) == n_edges
    assert R.edge_replays(n_edges, case.n_iter_max) == (replays, per_node)


def test_edge_pool_sizes():
    """the pools of a 1500-iteration graph at edge_per_node 1, 4, 16, 64: asked, and with the arena's eighth of headroom"""
    assert [R.edge_pool(1500, 4 ** k)[0] for k in range(4)] == [5598, 10104, 28128, 100224]
    assert [R.edge_pool(1500, 4 ** k)[1] for k in range(4)] == [6297, 11367, 31644, 112752]
    assert R.edge_pool(1500, 256)[0] == 1502 * 256 + 4096


def test_batch_members_overflow_the_first_pool(oracle_lib):
    for seed in (0, 1, 2):
        o, _ = grown(R.pto_1500(seed), 256, orc.ALGO_BATCHED_KD)
        assert R.edge_replays(len(o.edges()[0]), 1500) == (3, 64)


def test_the_lattice_stream_for_two_grows_starts_with_the_stream_for_one():
    one, two = X.lattice(1 / 16, X.SINGLE_SEED, X.RRT_ITERS), X.lattice(1 / 16, X.SINGLE_SEED, 2 * X.RRT_ITERS)
    assert np.array_equal(one, two[:X.RRT_ITERS]) and len(two) >= 2 * (X.RRT_ITERS - X.RRT_ITERS // 100)
