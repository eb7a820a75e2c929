"""GPU parity on inputs that make exact ties between DIFFERENT places (tests/exact_inputs.py): lattice samples end to end.

With a continuous sampler every exact comparison of the engine -- the nearest neighbour as the least (norm2, id), norm2 <= radius,
equal dist_root + cost parents in kd pre-order, rewires won by the least (candidate dist, new id), the first minimum in push order of
the path walks -- is decided by a strict inequality, and the suite's other ties are exact copies at one place.  Here samples sit on
a lattice whose pitch divides max_step: nodes at different places are at bit-equal distances, the radius is met exactly, and a wrong
choice between two nearest nodes steers to another state.  Every comparison is exact (bits); nothing has a tolerance.  Each test
asserts from the oracle's own output that its stream reached the comparison it was built for, and prints the counts.
The oracle's side of these inputs (kd-accelerated == brute force) is tests/test_exact_inputs_cpu.py."""
import numpy as np
import pytest

import cases
import exact_inputs as X
import qmdp_ref as Q
from oracle import orc
from test_gpu_parity import assert_same
from test_gpu_prm import assert_same_roadmap
from test_gpu_qmdp import check_react, same

pytestmark = pytest.mark.gpu

SINGLE_SEED = X.SINGLE_SEED


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


# ---------------------------------------------------------------------------------------------------------------- RRT* growth
def rrt_inputs(kind, seed):
    if kind == "lattice":
        return X.rrt_lattice_case(), X.lattice(1 / 16, seed, X.RRT_ITERS)
    return X.rrt_decimal_case(), X.decimal_grid(seed, X.RRT_ITERS)


@pytest.fixture(scope="module")
def rrt_oracle():
    """the oracle's tree of a stream, made once per module and dropped with it; read only"""
    made = {}

    def get(kind, seed, K, n_min=X.RRT_ITERS, n_max=X.RRT_ITERS):
        key = (kind, seed, K, n_min, n_max)
        if key not in made:
            case, xy = rrt_inputs(kind, seed)
            case.update(n_iter_min=n_min, n_iter_max=n_max)
            o = cases.configure(orc.Oracle(), case)
            o.set_samples(xy)
            cases.grow(o, case, K=K, algo=orc.ALGO_BATCHED_KD)
            made[key] = o
        return made[key]
    yield get
    made.clear()


def rrt_engine(eng_mod, kind, seed, **opts):
    case, xy = rrt_inputs(kind, seed)
    e = cases.configure(eng_mod.Engine(), case)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_samples(xy)
    return e, case


def report_rrt_ties(label, kind, seed, K, o, radius):
    """what the stream did, from the oracle's tree: pairs at exactly the radius, copies, shared dist_root, nearest ties"""
    case, xy = rrt_inputs(kind, seed)
    x, _, d = o.tree()
    n_it = o.num_iterations()
    at_radius, copies, shared = X.count_pairs_at_distance(x, radius), X.count_pairs_at_distance(x, 0.0), X.count_shared_dist_root(x, d)
    ties, steered = X.count_steering_ties(x, X.rrt_iteration_samples(case, xy, n_it), o.nearest_ids(), K, case.max_step)
    print("%s seed %d K %d: %d nodes, %d pairs at exactly %g, %d pairs at one place, %d nodes sharing dist_root with another place, "
          "%d nearest ties between places (%d steered)" % (label, seed, K, len(x), at_radius, radius, copies, shared, ties, steered))
    return at_radius, copies, shared, ties, steered


@pytest.mark.parametrize("K", [1, 64, 256])
def test_rrt_lattice_single_query(eng_mod, rrt_oracle, K):
    """form (a): the single-query step kernels.  The radius is max_step itself (two pitches exactly) until about 1900 nodes."""
    e, case = rrt_engine(eng_mod, "lattice", SINGLE_SEED)
    cases.grow(e, case, K=K)
    o = rrt_oracle("lattice", SINGLE_SEED, K)
    at_radius, copies, shared, ties, steered = report_rrt_ties("single", "lattice", SINGLE_SEED, K, o, case.max_step)
    assert at_radius > 0 and copies > 0 and shared > 0 and ties > 0 and steered > 0
    assert_same(e, o)                                            # n_tie_fallbacks == 0 is part of it


@pytest.mark.parametrize("conn_wg_waves", [1, 4])
@pytest.mark.parametrize("commit_flat", [0, 1])
def test_rrt_lattice_batch_of_eight(eng_mod, rrt_oracle, commit_flat, conn_wg_waves):
    """form (b): eight rows with eight seeds of the stream at K = 256 through the group kernels, both commit forms, both connect forms"""
    case = X.rrt_lattice_case()
    engs = [rrt_engine(eng_mod, "lattice", s, commit_flat=commit_flat, conn_wg_waves=conn_wg_waves)[0] for s in X.RRT_SEEDS]
    eng_mod.Engine.grow_batch(engs, [case.start] * 8, case.max_step, case.search_radius, X.RRT_ITERS, 256)
    assert engs[0].get_option("group_lanes") == 16 and engs[0].get_option("commit_flat") == commit_flat
    assert engs[0].get_option("conn_wg_waves") == conn_wg_waves
    assert engs[0].get_option("kd_built_after") == 1
    for s, e in zip(X.RRT_SEEDS, engs):
        o = rrt_oracle("lattice", s, 256)
        if commit_flat == 0 and conn_wg_waves == 1:
            at_radius, copies, shared, ties, steered = report_rrt_ties("batch", "lattice", s, 256, o, case.max_step)
            assert at_radius > 0 and shared > 0 and ties > 0
        assert_same(e, o)


def test_rrt_lattice_rows_with_loop_conditions_of_their_own(eng_mod, rrt_oracle):
    """form (c): the batch of (b) at K = 128 with n_iter_min spread over 600 .. 1800 and n_iter_max above it; every row against its
    single grow and against the oracle"""
    case = X.rrt_lattice_case()
    engs = [rrt_engine(eng_mod, "lattice", s)[0] for s in X.RRT_SEEDS]
    eng_mod.Engine.grow_batch(engs, [case.start] * 8, case.max_step, case.search_radius, X.ROW_MIN, 128, n_iter_max=X.ROW_MAX)
    assert engs[0].get_option("group_lanes") == 16 and engs[0].get_option("kd_built_after") == 1
    its = [e.num_iterations() for e in engs]
    assert len(set(its)) > 1 and all(a <= i <= b for i, a, b in zip(its, X.ROW_MIN, X.ROW_MAX))
    for s, e in zip(X.RRT_SEEDS, engs):
        single, c1 = rrt_engine(eng_mod, "lattice", s)
        c1.update(n_iter_min=X.ROW_MIN[s], n_iter_max=X.ROW_MAX[s])
        cases.grow(single, c1, K=128)
        assert_same(e, single)
        o = rrt_oracle("lattice", s, 128, X.ROW_MIN[s], X.ROW_MAX[s])
        at_radius, copies, shared, ties, steered = report_rrt_ties("rows", "lattice", s, 128, o, case.max_step)
        assert at_radius > 0 and shared > 0 and ties > 0
        assert_same(e, o)


def test_rrt_decimal_grid(eng_mod, rrt_oracle):
    """samples on the pixel corners k / 100 of the 200 x 200 raster (not exact in binary: to_pixel's floor sits on the rounding of every
    one of them), K = 64, single and a batch of eight"""
    case = X.rrt_decimal_case()
    e, _ = rrt_engine(eng_mod, "decimal", 0)
    cases.grow(e, case, K=64)
    o = rrt_oracle("decimal", 0, 64)
    x = o.tree()[0]
    on_corner = int(np.count_nonzero((x * 100 == np.round(x * 100)).all(axis=1)))
    print("decimal grid seed 0: %d nodes, %d on a pixel corner" % (len(x), on_corner))
    at_radius, copies, shared, ties, steered = report_rrt_ties("decimal single", "decimal", 0, 64, o, case.max_step)
    assert on_corner > 0 and at_radius > 0 and copies > 0 and ties > 0
    assert_same(e, o)
    engs = [rrt_engine(eng_mod, "decimal", s)[0] for s in X.RRT_SEEDS]
    eng_mod.Engine.grow_batch(engs, [case.start] * 8, case.max_step, case.search_radius, X.RRT_ITERS, 64)
    assert engs[0].get_option("group_lanes") == 16
    for s, e in zip(X.RRT_SEEDS, engs):
        o = rrt_oracle("decimal", s, 64)
        at_radius, copies, shared, ties, steered = report_rrt_ties("decimal batch", "decimal", s, 64, o, case.max_step)
        assert at_radius > 0 and copies > 0 and ties > 0
        assert_same(e, o)


# ---------------------------------------------------------------------------------------------------------------- PTO growth
@pytest.fixture(scope="module")
def pto_oracle():
    """the oracle's belief-space graph on lattice_once(1/32) and its return code, made once per module and dropped with it.  Tests read
    its graph; the one that builds a belief graph on it always builds the same one."""
    made = {}

    def get(K):
        if K not in made:
            case = X.pto_lattice_case()
            o = cases.configure(orc.Oracle(), case)
            o.set_samples(X.pto_stream(0))
            made[K] = (o, cases.grow(o, case, K=K, algo=orc.ALGO_BATCHED_KD))
        return made[K]
    yield get
    made.clear()


def pto_engine(eng_mod, K):
    """an engine of its own for every test (the tests go on to build different things on it), grown on the same stream"""
    case = X.pto_lattice_case()
    e = cases.configure(eng_mod.Engine(), case)
    e.set_samples(X.pto_stream(0))
    return e, cases.grow(e, case, K=K)


@pytest.mark.parametrize("K", [1, 64])
def test_pto_lattice_growth(eng_mod, pto_oracle, K):
    (e, rce), (o, rco) = pto_engine(eng_mod, K), pto_oracle(K)
    case = X.pto_lattice_case()
    x = o.tree()[0]
    f, t, _ = o.edges()
    deg = np.bincount(np.concatenate([f, t]))
    print("PTO lattice K %d: %d nodes, %d edges, %d pairs at exactly %g, most neighbours of a node %d, final set complete %s"
          % (K, len(x), len(f), X.count_pairs_at_distance(x, case.max_step), case.max_step, deg.max(), o.is_final_set_complete()))
    assert X.count_pairs_at_distance(x, case.max_step) > 0 and o.is_final_set_complete()
    assert rce == rco
    assert_same(e, o, pto=True)                                  # nodes, edges in order, reach, finals


@pytest.mark.parametrize("K", [1, 64])
def test_pto_lattice_belief_graph_costs_and_policy(eng_mod, pto_oracle, K):
    e, o = pto_engine(eng_mod, K)[0], pto_oracle(K)[0]
    e.build_belief_graph([0.5, 0.5])
    o.build_belief_graph([0.5, 0.5])
    ge, go = e.belief_graph(), o.belief_graph()
    assert np.array_equal(ge[0], go[0]) and np.array_equal(ge[1], go[1])
    for k in (2, 3):
        assert np.array_equal(ge[k][0], go[k][0]) and np.array_equal(ge[k][1], go[k][1])
    e.compute_expected_costs()
    de, do = e.expected_costs(), o.expected_costs()
    assert np.array_equal(de.view(np.uint64), do.view(np.uint64)), "expected costs differ"
    assert np.isfinite(do[0]) and do[0] > 0.0
    (oid, par, leaf), cost = e.extract_policy()
    oo, po, lo = o.extract_policy(do)
    assert cost == do[0] and np.array_equal(oid, oo) and np.array_equal(par, po) and np.array_equal(leaf, lo)


def qmdp_queries():
    """64 queries: starts on lattice points and on cell centres (equidistant from four lattice points) by turns, the three beliefs and
    the three horizons in every combination"""
    k = np.random.default_rng(11).integers(-30, 31, (64, 2)).astype(np.float64)
    starts = np.where((np.arange(64) % 2 == 0)[:, None], k / 32.0, (k + 0.5) / 32.0)
    beliefs = np.array([(0.5, 0.5), (1.0, 0.0), (0.25, 0.75)])[np.arange(64) % 3]
    horizons = np.array([0.0, 0.2, 1.0])[(np.arange(64) // 3) % 3]
    return starts, beliefs, horizons


def test_pto_lattice_qmdp(eng_mod, pto_oracle):
    """porrt_qmdp_plan / porrt_qmdp_react on the K = 64 graph against the restatement fed from the oracle's graph"""
    e, o = pto_engine(eng_mod, 64)[0], pto_oracle(64)[0]
    q = Q.from_planner(o)
    q.plan_qmdp()
    e.qmdp_plan()
    assert same(e.qmdp_costs(), q.cost_to_goals)
    starts, beliefs, horizons = qmdp_queries()
    want = check_react(eng_mod, e, q, starts, beliefs, horizons)
    steps, tied, lanes, late = 0, 0, 0, 0
    for s, b, h, a in zip(starts, beliefs, horizons, want):
        if not isinstance(a, Q.WalkTooLong):
            rows = X.qmdp_world_walk_rows(q, s, b, h)
            c = X.walk_tie_counts(rows)
            steps, tied, lanes, late = steps + len(rows), tied + c[0], lanes + c[1], late + c[2]
    print("QMDP per-world walks: %d steps, %d with a tied least cost, %d of them across lanes, %d with a tied entry at position >= 64"
          % (steps, tied, lanes, late))
    assert lanes > 0


# ---------------------------------------------------------------------------------------------------------------- PRM roadmap
PRM_START = (0.0, -0.875)


def prm_pair(eng_mod, xy, max_step, start=PRM_START, host_ranks=1, n_iter=None):
    """the benchmark map without zones; engine and oracle grown on the injected stream"""
    objs = []
    for mk in (eng_mod.Engine, orc.Oracle):
        x = mk()
        x.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
        x.set_sampler((-1.0, -1.0), (1.0, 1.0), 0)
        x.set_samples(xy)
        objs.append(x)
    e, o = objs
    e.set_option("host_ranks", host_ranks)
    n = len(xy) if n_iter is None else n_iter
    e.grow_prm(start, max_step, 5.0, n)
    o.grow_prm(start, max_step, 5.0, n)
    return e, o


def edge_lengths(o):
    x = o.tree()[0]
    f, t, _ = o.edges()
    return np.array([0.0]) if len(f) == 0 else np.sqrt(0.0 + (x[t, 0] - x[f, 0]) ** 2 + (x[t, 1] - x[f, 1]) ** 2)


@pytest.mark.parametrize("host_ranks", [1, 0])
def test_prm_window_and_cell_boundaries(eng_mod, host_ranks):
    """3000 samples of lattice(1/16) with max_step = 0.125: the extent is 1.875 = 15 radii, a cell of k_prm_connect's grid is exactly one
    radius wide and every node lies on a cell boundary"""
    e, o = prm_pair(eng_mod, X.lattice(1 / 16, 0, 3000), 0.125, host_ranks=host_ranks)
    d = edge_lengths(o)
    print("PRM window: %d edges, %d at exactly 0.125, %d of length 0" % (len(d), np.count_nonzero(d == 0.125), np.count_nonzero(d == 0.0)))
    assert np.count_nonzero(d == 0.125) > 0 and np.count_nonzero(d == 0.0) > 0
    assert_same_roadmap(e, o)


@pytest.mark.parametrize("host_ranks", [1, 0])
def test_prm_deep_kd_tree(eng_mod, host_ranks):
    """staircase(1500): a kd-tree as deep as it has nodes, coordinate ties going right at every level"""
    e, o = prm_pair(eng_mod, X.staircase(1500), 0.1, host_ranks=host_ranks)
    depth = X.kd_depth(o.tree()[0])
    print("PRM staircase: kd depth %d of %d nodes, %d edges" % (depth, o.num_nodes(), len(o.edges()[0])))
    assert depth >= 1000
    assert_same_roadmap(e, o)


def test_prm_long_buckets_and_paths_into_the_cluster(eng_mod):
    """2300 lattice points plus a cluster of 700 inside one radius: adjacency buckets longer than k_eo_segsort's LDS stage (512) and
    cell rows longer than a wave; then paths with an end inside the cluster, one by one and in one call"""
    pts = np.concatenate([X.lattice_once(1 / 32, 0, 2300), X.cluster(700, (0.0, -0.8), 0.03, 1)])
    pts = np.ascontiguousarray(pts[np.random.default_rng(5).permutation(len(pts))])
    e, o = prm_pair(eng_mod, pts, 0.1)
    f, t, _ = o.edges()
    made, found = int(np.bincount(t).max()), int(np.bincount(f).max())
    print("PRM long buckets: %d edges of %d capacity, largest creation bucket %d, largest later-finders bucket %d"
          % (len(f), (len(pts) + 1) * 256 + 4096, made, found))
    assert made > 512 and found > 512
    assert_same_roadmap(e, o)
    rng = np.random.default_rng(6)
    inside = X.cluster(16, (0.0, -0.8), 0.03, 9) + 1.0 / 16384                  # between the cluster's points
    far = X.lattice_once(1 / 32, 7, 16) + np.where(np.arange(16)[:, None] % 2 == 0, 0.0, 1.0 / 64)
    swap = rng.integers(0, 2, 16).astype(bool)[:, None]
    S, G = np.where(swap, inside, far), np.where(swap, far, inside)
    want = [o.prm_plan_path(s, g) for s, g in zip(S, G)]
    assert sum(len(p) > 1 for p in want) >= 8
    for s, g, p in zip(S, G, want):
        assert same(e.prm_plan_path(s, g), p), (s, g)
    for got, p in zip(e.prm_plan_paths(S, G), want):
        assert same(got, p)


PATH_PAIRS = [((-0.875, -0.875), (0.875, 0.875)), ((0.0, -0.875), (0.90625, 0.0)), ((-0.5, 0.75), (0.75, -0.75))]


def test_prm_path_ties(eng_mod):
    """all 3969 points of lattice_once(1/32) with max_step = 0.1875 = six pitches: adjacency lists longer than a wave, equal
    cost-to-goal + edge parents in different lanes and beyond position 64 (wave_first_min in k_prm_walk), query points equidistant from
    four nodes (HostKd::nearest's first-visited rule)"""
    e, o = prm_pair(eng_mod, X.lattice_once(1 / 32, 0, 3969), 0.1875)
    assert_same_roadmap(e, o)
    xy = o.tree()[0]
    f, t, _ = o.edges()
    deg = np.bincount(np.concatenate([f, t]))
    tied = lanes = late = steps = 0
    roadmap = X.Roadmap(xy, f, t)
    for s, g in PATH_PAIRS:                                      # the walk again in plain Python: it is the oracle's, and it meets ties
        p, rows = roadmap.walk(s, g)
        assert same(p, o.prm_plan_path(s, g))
        c = X.walk_tie_counts(rows)
        steps, tied, lanes, late = steps + len(rows), tied + c[0], lanes + c[1], late + c[2]
    print("PRM path ties: %d edges, median adjacency %d, %.0f %% of the nodes above 64; %d walk steps, %d with a tied minimum, %d across "
          "lanes, %d with a tied entry at position >= 64" % (len(f), np.median(deg), 100.0 * np.mean(deg > 64), steps, tied, lanes, late))
    assert tied > 0 and lanes > 0 and late > 0
    k = np.random.default_rng(12).integers(-30, 31, (29, 4)).astype(np.float64)
    S = np.where((np.arange(29) % 2 == 0)[:, None], k[:, :2] / 32.0, (k[:, :2] + 0.5) / 32.0)
    G = np.where((np.arange(29) % 3 == 0)[:, None], k[:, 2:] / 32.0, (k[:, 2:] + 0.5) / 32.0)
    S, G = np.concatenate([[p[0] for p in PATH_PAIRS], S]), np.concatenate([[p[1] for p in PATH_PAIRS], G])
    want = [o.prm_plan_path(s, g) for s, g in zip(S, G)]
    assert sum(len(p) > 1 for p in want) >= 24
    for s, g, p in zip(S, G, want):
        assert same(e.prm_plan_path(s, g), p), (s, g)
    for got, p in zip(e.prm_plan_paths(S, G), want):
        assert same(got, p)


@pytest.mark.parametrize("n_iter", [0, 1, 2, 3, 4, 5, 63, 64, 65])
def test_prm_sizes(eng_mod, n_iter):
    e, o = prm_pair(eng_mod, X.lattice(1 / 16, 0, 65), 0.125, n_iter=n_iter)
    assert e.num_nodes() == n_iter + 1
    assert_same_roadmap(e, o)


def test_prm_beyond_256_edges_per_node_then_reuse(eng_mod):
    """1200 points inside one radius make about 720 000 edges against a first edge list of N * 256 + 4096 = 311 552: grow_prm counts them
    before the fill and runs again with a list of that size (it used to end in a capacity error), and the context then grows a small
    roadmap as usual"""
    pts = X.cluster(1200, (0.0, -0.8), 0.03, 2)
    o = orc.Oracle()
    o.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    o.set_samples(pts)
    o.grow_prm((0.0, -0.8), 0.1, 5.0, len(pts))
    assert len(o.edges()[0]) > (len(pts) + 1) * 256 + 4096
    e = eng_mod.Engine()
    e.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    e.set_samples(pts)
    e.grow_prm((0.0, -0.8), 0.1, 5.0, len(pts))
    assert_same_roadmap(e, o)
    xy = X.lattice(1 / 16, 1, 300)
    e.set_samples(xy)
    o.set_samples(xy)
    e.grow_prm(PRM_START, 0.125, 5.0, 300)
    o.grow_prm(PRM_START, 0.125, 5.0, 300)
    assert_same_roadmap(e, o)
