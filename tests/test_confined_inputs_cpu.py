"""CPU side of the confined-window and step-geometry inputs (tests/confined_inputs.py): the oracle runs every input that
tests/test_gpu_confined.py compares the device against, and what each input was built to produce is asserted from the oracle's own
output -- an input that stops producing its condition fails here instead of passing there.  Every test prints one line of figures."""
import numpy as np
import pytest

import cases
import confined_inputs as W
from oracle import orc

RC_ITER_MAX = 1            # orc_grow / porrt_grow: the growth ended on n_iter_max ("n_iter_max reached")


def fills(x):
    return np.bincount(W.cell(x), minlength=W.GRID * W.GRID)


def levels(n):
    """page levels of a region that holds n nodes"""
    return (n + 63) // 64


# ---- the counters
def test_counters(oracle_lib):
    x = np.array([[0.025, 0.025], [0.03, 0.03], [0.03, 0.03], [-0.001, 0.049], [0.0499, -0.975]])
    assert list(W.cell(x)) == [W.REGION, W.REGION, W.REGION, W.REGION - 1, 20], W.cell(x)
    assert W.copies_of(x, (0.03, 0.03)) == 2 and W.most_added_to_a_region(x, [1, 3, 5]) == 2
    assert W.discs_regions(0.5) == 441 and W.discs_regions(0.02) == 1 and levels(64) == 1 and levels(65) == 2
    assert [W.tile_radius(m) for m in (0.05, 0.1, 0.2895, 0.29, 0.2901, 0.5)] == [7, 12, 31, 31, 0, 0]
    occ = W.window_raster()
    assert np.count_nonzero(occ == 0) == 1 and np.count_nonzero(occ == 200) == 1 and np.count_nonzero(occ == 255) == 200 * 200 - 2
    o = orc.Oracle()
    o.set_grid(occ, (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    lo, up, ij = W.pixel_box(o, W.OBSTACLE_AT)
    assert occ[ij] == 0 and np.allclose(lo, (0.03, 0.03)) and np.allclose(up, (0.04, 0.04))
    for p in (lo + 1e-6, up - 1e-6, (lo[0] + 1e-6, up[1] - 1e-6)):                     # the box is the pixel
        assert o.to_pixel(p) == ij
    for p in (lo - 1e-6, up + 1e-6):
        assert o.to_pixel(p) != ij
    # node 2 sees node 0 across the box, node 1 sees nothing across it
    y = np.array([[0.02, 0.035], [0.02, 0.02], [0.046, 0.035]])
    assert W.nodes_across_box(y, [1, 3], [0.1], lo, up) == 1
    assert W.nodes_across_box(y, [1, 3], [0.01], lo, up) == 0
    # the walk over the iterations counts a step's nodes as the shorter runs do
    c = cases.cfg2(1000, seed=7)
    g, _ = W.oracle(c, 256)
    assert W.n_at_all(c, g, 256) == W.n_at(c, 3, 256) + [g.num_nodes()]


# ---- (1), (2): one region
def report_one_region(case, K, o, at, hits):
    x = o.tree()[0]
    full = fills(x)
    print("%s K %d: %d nodes, %d in region %d (%d page levels), %d final, most hits %d, %d heavy (> 2048), %d copies of the goal point, "
          "most added to the region in a step %d" % (case.name, K, len(x), full[W.REGION], W.REGION, levels(full[W.REGION]), len(o.final_ids()),
                                                     hits.max(), np.count_nonzero(hits > 2048), W.copies_of(x, case.goals[0]),
                                                     W.most_added_to_a_region(x, at)))
    return full


@pytest.mark.parametrize("K", [256, 1024])
def test_one_region(oracle_lib, K):
    case = W.one_region(W.ONE_REGION_ITERS[K])
    o, _ = W.oracle(case, K)
    at = W.n_at_all(case, o, K)
    hits = W.hits_per_node(case, o, at)
    x = o.tree()[0]
    full = report_one_region(case, K, o, at, hits)
    assert full[W.REGION] == len(x) == case.n_iter_min + 1
    assert hits.max() > 2048
    assert W.copies_of(x, case.goals[0]) >= 20
    if K == 1024:
        assert W.most_added_to_a_region(x, at) > 512


def test_one_region_raster(oracle_lib):
    K = 256
    case = W.one_region_raster()
    o, _ = W.oracle(case, K)
    at = W.n_at_all(case, o, K)
    hits = W.hits_per_node(case, o, at)
    x = o.tree()[0]
    full = report_one_region(case, K, o, at, hits)
    lo, up, _ = W.pixel_box(o, W.OBSTACLE_AT)
    across = W.nodes_across_box(x, at, W.radii(case, at), lo, up)
    print("%s K %d: %d nodes with an earlier node of their radius across the obstacle pixel" % (case.name, K, across))
    assert full[W.REGION] == len(x)
    assert hits.max() > 2048
    assert across >= 100


# ---- (3): a region corner
def test_corner_window(oracle_lib):
    K = 256
    case = W.corner_window()
    o, _ = W.oracle(case, K)
    at = W.n_at_all(case, o, K)
    hits = W.hits_per_node(case, o, at)
    full = fills(o.tree()[0])
    print("%s K %d: %d nodes in %d regions, the fullest %d, %d regions above 320, most hits %d" % (
        case.name, K, o.num_nodes(), np.count_nonzero(full), full.max(), np.count_nonzero(full > 320), hits.max()))
    assert np.count_nonzero(full > 320) >= 4
    assert hits.max() > 320


# ---- (4): belief-space graphs in a window
@pytest.mark.parametrize("make", [W.pto_shelf_window, W.pto_door_window], ids=lambda f: f.__name__)
def test_pto_window(oracle_lib, make):
    case = make()
    o, rc = W.oracle(case, W.PTO_K)
    n, e = o.num_nodes(), len(o.edges()[0])
    print("%s K %d: %d nodes, %d edges (%.0f per node), return code %d" % (case.name, W.PTO_K, n, e, e / n, rc))
    assert rc == RC_ITER_MAX
    assert e > 256 * n


# ---- (5): a roadmap in the window
def test_prm_window(oracle_lib):
    a, o = W.prm_pair(orc.Oracle)
    for x in (a, o):
        x.grow_prm(W.PRM["start"], W.PRM["max_step"], W.PRM["search_radius"], W.PRM["n_iter"])
    e = len(o.edges()[0])
    paths = [o.prm_plan_path(s, g) for s, g in W.PRM_QUERIES]
    print("prm_window: %d nodes, %d edges, paths of %s states" % (o.num_nodes(), e, [len(p) for p in paths]))
    assert o.num_nodes() == W.PRM["n_iter"] + 1 and e > 1000000
    assert all(len(p) >= 2 for p in paths)
    assert all(np.array_equal(p, a.prm_plan_path(s, g)) for p, (s, g) in zip(paths, W.PRM_QUERIES))     # (the oracle is deterministic)
    xy = o.tree()[0]
    assert (W.cell(xy) == W.REGION).all()
    assert W.cell(np.array([W.PRM_QUERIES[2][1]]))[0] != W.REGION                                      # the third goal is outside the window


# ---- (6): step geometries
@pytest.fixture(scope="module")
def geometry_runs():
    made = {}

    def get(name):
        if name not in made:
            case = W.geometry(name)
            o, _ = W.oracle(case, W.GEOMETRY_K)
            at = W.n_at_all(case, o, W.GEOMETRY_K)
            made[name] = (case, o, at, W.radii(case, at))
        return made[name]
    yield get
    made.clear()


def longest_edge(o):
    x, parent, _ = o.tree()
    d = x[1:] - x[parent[1:]]
    return float(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).max())


def report_geometry(case, o, at, rad, more=""):
    full = fills(o.tree()[0])
    print("%s (max_step %g, search_radius %g) K %d: %d nodes in %d regions, the fullest %d, %d final, radius %.4g .. %.4g from step 1 on, "
          "tile %d pixels, longest edge %.1f pixels%s"
          % (case.name, case.max_step, case.search_radius, W.GEOMETRY_K, o.num_nodes(), np.count_nonzero(full), full.max(), len(o.final_ids()),
             rad[1:].max(), rad[1:].min(), W.tile_radius(case.max_step), longest_edge(o) * W.PPM, more))
    return full


def test_long_steps_fixed_radius(oracle_lib, geometry_runs):
    case, o, at, rad = geometry_runs("long_steps_fixed_radius")
    hits = W.hits_per_node(case, o, at)
    report_geometry(case, o, at, rad, ", most hits %d, hand-over at %d nodes" % (hits.max(), 16 * W.discs_regions(case.max_step)))
    assert (rad[1:] == case.max_step).all()                       # (step 0 searches the root alone: heuristic_radius(1) is 0)
    hand_over = 16 * W.discs_regions(case.max_step)
    assert at[1] < hand_over < at[-2], "no step on either side of the hand-over of the largest discs"
    assert hits.max() > 2048
    assert longest_edge(o) * W.PPM > 30.0                         # rays beyond any tile


def test_long_steps_shrinking_radius(oracle_lib, geometry_runs):
    """The tree never reaches the 16 * 441 nodes at which a disc of radius max_step would be handed over to the pages -- but no disc is
    that large here: the radius is below max_step from step 1 on (0.29 at 250 nodes) and shrinks below 0.1, so the hand-over moves
    with it and falls into the run, with steps on either side."""
    case, o, at, rad = geometry_runs("long_steps_shrinking_radius")
    streams = [16 * W.discs_regions(r) > n for r, n in zip(rad[1:], at[1:-1])]
    report_geometry(case, o, at, rad, ", streamed steps 1 .. %d of %d" % (sum(streams), len(streams)))
    assert o.num_nodes() < 16 * W.discs_regions(case.max_step)
    assert (rad[1:] < case.max_step).all() and rad[-1] < 0.1 and (np.diff(rad[1:]) < 0).all()
    assert streams[0] and not streams[-1] and streams == sorted(streams, reverse=True)


def test_short_steps(oracle_lib, geometry_runs):
    case, o, at, rad = geometry_runs("short_steps")
    x, parent, _ = o.tree()
    full = report_geometry(case, o, at, rad)
    assert full.max() > 256
    # a sample is steered to max_step (L1) from its nearest node (common.rs:215-225), so every node has a node of its step's snapshot
    # that close; the parent it hangs below in the end is a node of its radius, which is never above max_step (Euclidean)
    slack = case.max_step * (1.0 + 1e-12)
    for a, b in zip(at[:-1], at[1:]):
        l1 = np.abs(x[a:b, None, :] - x[None, :a, :]).sum(axis=2).min(axis=1)
        assert (l1 <= slack).all()
    d = x[1:] - x[parent[1:]]
    assert (np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) <= slack).all() and (rad <= case.max_step).all()


def test_radius_is_max_step(oracle_lib, geometry_runs):
    case, o, at, rad = geometry_runs("radius_is_max_step")
    report_geometry(case, o, at, rad)
    assert (rad[1:] == case.max_step).all() and len(rad) > 10


def test_radius_below_max_step(oracle_lib, geometry_runs):
    case, o, at, rad = geometry_runs("radius_below_max_step")
    report_geometry(case, o, at, rad)
    assert (rad < case.max_step).all() and (rad[1:] > 0.0).all() and len(rad) > 10


@pytest.mark.parametrize("name", W.TILE_ROWS)
def test_tile_limit(oracle_lib, geometry_runs, name):
    """either side of max_step * ppm = kTileRMax - 2 = 29 pixels.  0.29 itself is on the tile's side: 0.29 * 100 rounds to
    28.999999999999996, so the row that has no tile is 0.2901"""
    case, o, at, rad = geometry_runs(name)
    report_geometry(case, o, at, rad)
    ppm_step = case.max_step * W.PPM
    if name == "no_tile":
        assert ppm_step >= W.TILE_R_MAX - 2 and W.tile_radius(case.max_step) == 0
    else:
        assert ppm_step < W.TILE_R_MAX - 2 and 2 * W.tile_radius(case.max_step) + 1 == 63
    assert longest_edge(o) * W.PPM > 25.0
    p = W.pto_tile(case.max_step)
    g, rc = W.oracle(p, W.PTO_K)
    print("%s K %d: %d nodes, %d edges, return code %d" % (p.name, W.PTO_K, g.num_nodes(), len(g.edges()[0]), rc))
    assert g.num_nodes() > 1000 and len(g.edges()[0]) > 10 * g.num_nodes()
