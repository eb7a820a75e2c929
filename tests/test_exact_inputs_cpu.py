"""CPU side of the exact-tie inputs (tests/exact_inputs.py): the streams are what they say, the oracle's kd-accelerated contract equals its
brute-force definition on every stream and case that tests/test_gpu_exact_ties.py compares the device against, and the statement
"batched(K = 1) is the reference loop" pinned both ways:

  * it holds on a stream in which no sample has two nodes at different places at one distance (test_k1_is_the_reference_loop_without_ties);
  * it does not on the plain lattice: the reference's nearest_neighbor keeps the first node its near-side-first walk visits
    (nearest_neighbor.rs:59-88), the contract the lowest id, and two nodes at different places and at bit-equal least distance steer
    the sample to different states (test_k1_differs_from_the_reference_loop_on_nearest_ties).
"""
import numpy as np
import pytest

import cases
import exact_inputs as X
from oracle import orc


def grow(case, xy, K, algo, **kw):
    c = cases.Case(case, **kw)
    o = cases.configure(orc.Oracle(), c)
    o.set_samples(xy)
    rc = cases.grow(o, c, K=K, algo=algo)
    return o, rc


def assert_same_tree(a, b):
    assert a.num_iterations() == b.num_iterations() and a.num_nodes() == b.num_nodes()
    for p, q in zip(a.tree(), b.tree()):
        assert np.array_equal(np.ascontiguousarray(p).view(np.uint64), np.ascontiguousarray(q).view(np.uint64))
    assert np.array_equal(a.final_ids(), b.final_ids()) and np.array_equal(a.final_masks(), b.final_masks())
    assert np.array_equal(a.nearest_ids(), b.nearest_ids())


def assert_same_graph(a, b):
    assert_same_tree(a, b)
    assert np.array_equal(a.reach(), b.reach()) and np.array_equal(a.node_validity(), b.node_validity())
    for x, y in zip(a.edges(), b.edges()):
        assert np.array_equal(x, y)
    assert a.is_final_set_complete() == b.is_final_set_complete()


# ---- the streams
def oracle_kd_depth(xy):
    """depth of the oracle's kd-tree (kdtree.c, pinned by the reference's own vectors) through its structure probe orc_kd_child"""
    lib = orc.lib()
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    kd = lib.orc_kd_new(xy[0], 0)
    for j in range(1, len(xy)):
        lib.orc_kd_add(kd, xy[j], j)
    deepest, level = 0, [0]
    while level:
        deepest += 1
        level = [c for n in level for c in (lib.orc_kd_child(kd, n, 0), lib.orc_kd_child(kd, n, 1)) if c >= 0]
    lib.orc_kd_free(kd)
    return deepest


def test_streams_are_what_they_say(oracle_lib):
    assert len(X.lattice_points(1 / 16)) == 961 and len(X.lattice_points(1 / 32)) == 3969
    a = X.lattice(1 / 16, 3, 2000)
    assert a.shape == (2000, 2) and np.array_equal(a[:961], X.lattice_once(1 / 16, 3, 961)) and np.array_equal(a[961:1922], a[:961])
    assert len(np.unique(a[:961], axis=0)) == 961 and np.abs(a).max() == 15 / 16
    assert np.array_equal(a * 16, np.round(a * 16)) and not np.array_equal(a, X.lattice(1 / 16, 4, 2000))
    with pytest.raises(ValueError):
        X.lattice_once(1 / 16, 0, 962)
    s = X.staircase(1500)
    assert (np.diff(s[:, 0]) >= 0).all() and np.array_equal(s[:, 0], s[:, 1]) and np.count_nonzero(np.diff(s[:, 0]) == 0) == 1500 // 4
    assert np.array_equal(s[:5, 0], -0.9 + np.array([0, 1, 2, 2, 3]) / 1024.0)
    assert X.kd_depth(s) == 1500                                  # a chain
    for pts in (X.lattice(1 / 16, 2, 1200), X.staircase(200), X.cluster(300, (0.0, -0.8), 0.03, 4)):
        assert X.kd_depth(pts) == oracle_kd_depth(pts)            # the plain insert against the oracle's kd-tree
    c = X.cluster(700, (0.0, -0.8), 0.03, 1)
    assert len(np.unique(c, axis=0)) == 700 and np.array_equal(c * 8192, np.round(c * 8192))
    assert np.abs(c - np.array([0.0, np.round(-0.8 * 8192) / 8192])).max() <= 0.03
    with pytest.raises(ValueError):
        X.cluster(492 * 492, (0.0, 0.0), 0.03, 0)
    d = X.decimal_grid(0, 40000)
    assert len(np.unique(d, axis=0)) == 191 * 191 and np.abs(d).max() == 0.95


def test_counting_helpers():
    xy = np.array([[0.0, 0.0], [0.125, 0.0], [0.0, 0.125], [0.0, 0.0], [0.25, 0.0]])
    assert X.count_pairs_at_distance(xy, 0.125) == 5 and X.count_pairs_at_distance(xy, 0.0) == 1
    assert X.count_shared_dist_root(xy, np.array([0.0, 1.0, 1.0, 0.0, 2.0])) == 2          # the copies of the root do not count
    assert X.count_nearest_ties(xy, [[0.0625, 0.0625], [0.0, 0.0], [0.3, 0.0]]) == 1
    assert X.count_nearest_ties(xy, [[0.0, 0.0]], different_places=False) == 1
    assert X.count_equidistant_places(xy, [[0.0625, 0.0625]]) == 3 and X.count_equidistant_places(xy[[0, 3, 4]], [[1.0, 0.0]]) == 0
    rows = [[3.0, 1.0, 2.0], [1.0, 2.0, 1.0], [5.0] + [9.0] * 63 + [5.0], [7.0] * 2 + [8.0] * 70 + [7.0], [float("inf")] * 3, []]
    assert X.walk_tie_counts(rows) == (3, 2, 2)                   # row 2: positions 0 and 64 are one lane of a striding wave


# ---- the kd-accelerated contract equals the brute-force definition on every input of the GPU file
@pytest.mark.parametrize("K", [1, 64, 128, 256])
def test_rrt_lattice_kd_equals_brute(oracle_lib, K):
    case = X.rrt_lattice_case()
    for seed in X.RRT_SEEDS if K >= 128 else (X.SINGLE_SEED,):   # the GPU file: one stream at K = 1, 64, 256; eight at 128 and 256
        xy = X.lattice(1 / 16, seed, X.RRT_ITERS)
        kw = dict(n_iter_min=X.ROW_MIN[seed], n_iter_max=X.ROW_MAX[seed]) if K == 128 else {}
        a, _ = grow(case, xy, K, orc.ALGO_BATCHED, **kw)
        b, _ = grow(case, xy, K, orc.ALGO_BATCHED_KD, **kw)
        assert a.num_nodes() > 500
        assert_same_tree(a, b)


def test_rrt_decimal_grid_kd_equals_brute(oracle_lib):
    case = X.rrt_decimal_case()
    for seed in X.RRT_SEEDS:
        xy = X.decimal_grid(seed, X.RRT_ITERS)
        a, _ = grow(case, xy, 64, orc.ALGO_BATCHED)
        b, _ = grow(case, xy, 64, orc.ALGO_BATCHED_KD)
        assert a.num_nodes() > 1000
        assert_same_tree(a, b)


PTO_CASES = {
    "cfg3_near_lattice32": (X.pto_lattice_case, lambda: X.pto_stream(0)),
    "cfg3": (lambda: cases.Case(cases.cfg3(1500, 1500), max_step=0.0625), lambda: X.lattice_once(1 / 32, 1, 1500)),
    "cfg_door": (lambda: cases.Case(cases.cfg_door(1500, 1500), max_step=0.0625), lambda: X.lattice_once(1 / 32, 2, 1500)),
}


@pytest.mark.parametrize("K", [1, 64])
@pytest.mark.parametrize("name", sorted(PTO_CASES))
def test_pto_lattice_kd_equals_brute(oracle_lib, name, K):
    mk, stream = PTO_CASES[name]
    case, xy = mk(), stream()
    a, rca = grow(case, xy, K, orc.ALGO_BATCHED)
    b, rcb = grow(case, xy, K, orc.ALGO_BATCHED_KD)
    assert rca == rcb and a.num_nodes() > 500
    assert_same_graph(a, b)


# ---- "K = 1 is the reference loop", both ways
def creating_iterations(o, samples, max_step):
    """the iteration (1-based) that made every node of a K = 1 growth: iteration i steers its sample from nearest_ids()[i - 1], and
    makes the next node iff the steered state is valid -- which it is iff it is that node's state (validity is a function of the state)"""
    xy, nn = o.tree()[0], o.nearest_ids()
    made, n = np.zeros(len(xy), dtype=np.int64), 1
    for i, (q, j) in enumerate(zip(samples, nn), 1):
        p = np.array(q, dtype=np.float64)
        orc.lib().orc_steer(np.ascontiguousarray(xy[int(j)]), p, max_step)
        if n < len(xy) and np.array_equal(p.view(np.uint64), xy[n].view(np.uint64)):
            made[n] = i
            n += 1
    assert n == len(xy), "the walk over the iterations did not account for every node"
    return made


def test_k1_is_the_reference_loop_without_ties(oracle_lib):
    """the lattice moved so that no sample has two places at one distance: ALGO_SEQ == ALGO_BATCHED(1), the nearest ids included"""
    case = X.rrt_lattice_case()
    xy = X.moved_lattice(1 / 16, 3, X.RRT_ITERS)
    a, _ = grow(case, xy, 1, orc.ALGO_SEQ)
    b, _ = grow(case, xy, 1, orc.ALGO_BATCHED)
    assert a.num_nodes() > 1500
    samples = X.rrt_iteration_samples(case, xy, X.RRT_ITERS)
    assert X.count_equidistant_places(a.tree()[0], samples) == 0
    assert X.count_pairs_at_distance(a.tree()[0], 0.0) > 0          # copies at one place there are: the stream cycles
    assert_same_tree(a, b)


def test_k1_differs_from_the_reference_loop_on_nearest_ties(oracle_lib):
    """the plain lattice: the two loops part at a sample with two nodes at different places at bit-equal least distance"""
    case = X.rrt_lattice_case()
    xy = X.lattice(1 / 16, 3, X.RRT_ITERS)
    a, _ = grow(case, xy, 1, orc.ALGO_SEQ)
    b, _ = grow(case, xy, 1, orc.ALGO_BATCHED)
    xa, xb = a.tree()[0], b.tree()[0]
    m = min(len(xa), len(xb))
    differ = np.flatnonzero((xa[:m].view(np.uint64) != xb[:m].view(np.uint64)).any(axis=1))
    assert differ.size > 0, "the two loops agree on this stream: it holds no nearest-neighbour tie that steers"
    j = int(differ[0])                                            # the first differing node differs in position
    samples = X.rrt_iteration_samples(case, xy, X.RRT_ITERS)
    ia, ib = creating_iterations(a, samples, case.max_step)[j], creating_iterations(b, samples, case.max_step)[j]
    assert ia == ib, "node %d was made by iterations %d and %d" % (j, ia, ib)
    q = samples[ia - 1]
    na, nb = int(a.nearest_ids()[ia - 1]), int(b.nearest_ids()[ib - 1])
    assert np.array_equal(a.nearest_ids()[:ia - 1], b.nearest_ids()[:ia - 1])
    snap = xa[:j]                                                 # K = 1: the snapshot is the tree so far, the same in both loops
    assert np.array_equal(snap.view(np.uint64), xb[:j].view(np.uint64))
    d = X.norm2(snap, q)
    least = np.flatnonzero(d == d.min())
    assert na != nb and na in least and nb in least and d[na].view(np.uint64) == d[nb].view(np.uint64)
    assert (snap[na] != snap[nb]).any(), "the two nearest nodes are copies at one place"
    assert nb == least[0], "the contract takes the lowest id"
    assert X.norm1_exceeds(snap[na], q, case.max_step) and X.norm1_exceeds(snap[nb], q, case.max_step)      # both steer
    print("first differing node %d, iteration %d, sample %s: ALGO_SEQ steers from %d at %s, ALGO_BATCHED(1) from %d at %s, both at %r"
          % (j, ia, q, na, snap[na], nb, snap[nb], d[na]))
