"""Growths whose sampler window is smaller than the map (local replanning), growths at other step geometries than the workload's, and the
counters that state, from a finished oracle object, what such an input did.  Shared by tests/test_confined_inputs_cpu.py (the oracle
side: every condition an input was built for is asserted there) and tests/test_gpu_confined.py (the device against the oracle).

A window inside one region of the 40 x 40 page grid over [-1, 1)^2 sends every node into one page directory (a level per 64 nodes),
makes every sample's neighbour list as long as the tree, lets one step ask for many pages of one region at once, and gives a
belief-space graph hundreds of edges per node.  A large max_step makes a disc meet hundreds of regions (the id-ordered streaming of a
young tree lasts for thousands of nodes) and takes the LDS tile of the raster away; a search_radius far from the workload's keeps
heuristic_radius on one side of max_step for a whole run."""
import numpy as np

import cases
from oracle import orc

GRID = 40                                   # regions per axis over [-1, 1)^2 (rep_cell)
TILE_R_MAX = 31                             # kTileRMax: the tile covers max_step * ppm + 2 pixels around a workgroup's samples, at most this
PPM = 100.0                                 # pixels per unit of a 200 x 200 raster over [-1, 1)^2


# ---------------------------------------------------------------------------------------------------------------------- counters
def cell(x):
    """region of every row of x"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    return np.floor((x[:, 0] + 1.0) * 20.0).astype(int) + GRID * np.floor((x[:, 1] + 1.0) * 20.0).astype(int)


def configure(x, case):
    """cases.configure, then the case's own raster ("occ") and its sampler window ("window"), if it has them"""
    if case.get("occ") is not None:
        x.set_grid(case.occ, (-1.0, -1.0), (1.0, 1.0), case.domain)
    cases.configure(x, case)
    if case.get("window") is not None:
        x.set_sampler(case.window[0], case.window[1], case.seed)
    return x


def oracle(case, K, n_iter=None, samples=None, grows=1):
    """(the oracle grown on the case, the last return code)"""
    c = case if n_iter is None else cases.Case(case, n_iter_min=n_iter, n_iter_max=n_iter)
    o = configure(orc.Oracle(), c)
    if samples is not None:
        o.set_samples(samples)
    for _ in range(grows):
        rc = cases.grow(o, c, K=K, algo=orc.ALGO_BATCHED_KD)
    return o, rc


def n_at(case, steps, K):
    """nodes of the tree at the start of step 0 .. steps (a shorter run's tree is a prefix of a longer one's)"""
    return [1] + [oracle(case, K, n_iter=s * K)[0].num_nodes() for s in range(1, steps + 1)]


def creating_iterations(case, o):
    """the iteration (1-based) that made every node of the RRT* growth o, without growing again: iteration i steers its sample -- the
    next draw of the case's sampler, or the goal point in every hundredth iteration (rrt.rs:176-181) -- from nearest_ids()[i - 1], and
    makes the next node iff the steered state is valid, which it is iff it is that node's state (validity is a function of the state)"""
    x, nn = o.tree()[0], o.nearest_ids()
    s = configure(orc.Oracle(), case)
    made, n = np.zeros(len(x), dtype=np.int64), 1
    for i, j in enumerate(nn, 1):
        p = np.array(case.goals[0], dtype=np.float64) if i % 100 == 0 else s.sample()
        orc.lib().orc_steer(np.ascontiguousarray(x[int(j)]), p, case.max_step)
        if n < len(x) and p[0] == x[n, 0] and p[1] == x[n, 1]:
            made[n] = i
            n += 1
    assert n == len(x), "the walk over the iterations did not account for every node"
    return made


def n_at_all(case, o, K):
    """n_at for every step of the finished growth o, its end included"""
    steps = (o.num_iterations() + K - 1) // K
    made = creating_iterations(case, o)
    return [1] + [int(np.count_nonzero(made <= s * K)) for s in range(1, steps + 1)]


def radii(case, at):
    """heuristic_radius of every step (common.rs:357-369; the snapshot's size before insertion, rrt.rs:121)"""
    return np.array([orc.lib().orc_heuristic_radius(n0, case.max_step, case.search_radius, 2) for n0 in at[:-1]])


def hits_per_node(case, o, at):
    """radius-search hits of every new node of the oracle's tree: the nodes of its step's snapshot within heuristic_radius(n)
    (common.rs:357-369; the snapshot's size before insertion, rrt.rs:121)"""
    x = o.tree()[0]
    hits = np.zeros(len(x), dtype=int)
    for s in range(len(at) - 1):
        n0, n1 = at[s], at[s + 1]
        r = orc.lib().orc_heuristic_radius(n0, case.max_step, case.search_radius, 2)
        for i in range(n0, n1):
            dx, dy = x[i, 0] - x[:n0, 0], x[i, 1] - x[:n0, 1]
            hits[i] = np.count_nonzero(np.sqrt(dx * dx + dy * dy) <= r)
    return hits


def copies_of(x, p):
    return int(np.count_nonzero((x[:, 0] == p[0]) & (x[:, 1] == p[1])))


def most_added_to_a_region(x, at):
    """the most nodes that one step added to one region"""
    c = cell(x)
    return max(int(np.bincount(c[a:b], minlength=1).max()) if b > a else 0 for a, b in zip(at[:-1], at[1:]))


def discs_regions(max_step):
    """regions that the bounding box of a disc of radius max_step can meet"""
    side = int(np.floor(2.0 * max_step * (GRID / 2.0))) + 1           # GRID / 2 regions per unit of length
    return side * side


def pixel_box(o, p):
    """(low corner, up corner) in map coordinates of the pixel of a 200 x 200 raster over [-1, 1)^2 that holds p, and its (i, j)"""
    i, j = o.to_pixel(p)
    lo = np.floor((np.asarray(p, dtype=np.float64) + 1.0) * PPM) / PPM - 1.0
    return lo, lo + 1.0 / PPM, (i, j)


def nodes_across_box(x, at, rad, lo, up, chunk=128, points=32):
    """nodes whose straight segment to some node of their step's snapshot within the step's radius passes the box [lo, up): the
    middle third of the segment sampled finely (a proxy for the ray of map_shelves_io.rs:187-203, as _crosses of
    test_gpu_page_loads.py: whatever the half pixel the proxy may be off by at the rim, a middle third inside the box crosses it)"""
    t = (1.0 + np.linspace(0.0, 1.0, points)) / 3.0
    found = 0
    for s in range(len(at) - 1):
        n0, n1, r = at[s], at[s + 1], rad[s]
        for i in range(n0, n1):
            d = x[:n0] - x[i]
            near = np.flatnonzero(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) <= r)
            for a in range(0, len(near), chunk):
                q = x[near[a:a + chunk]]
                p = x[i][None, None, :] + (q - x[i])[:, None, :] * t[None, :, None]
                if ((p >= lo) & (p < up)).all(axis=2).any():
                    found += 1
                    break
    return found


def tile_radius(max_step):
    """pixels of raster that a workgroup's LDS tile holds around its samples, 0 when a step is too long for any tile"""
    return 0 if max_step * PPM >= TILE_R_MAX - 2 else int(np.ceil(max_step * PPM)) + 2


# ---------------------------------------------------------------------------------------------------------------------- the cases
WINDOW = ((0.002, 0.002), (0.048, 0.048))            # inside region (20, 20)
REGION = 20 + GRID * 20
SEEDS = tuple(range(8))


def one_region(n_iter=3000, seed=0):
    """(1): the empty map, every sample in one region; every hundredth iteration is the goal point itself, also in the window"""
    c = cases.empty_space(n_iter, n_iter, seed)
    c.update(name="one_region", window=WINDOW, start=(0.025, 0.025), goals=[(0.03, 0.03)], l1=0.005)
    return c


ONE_REGION_ITERS = {64: 3000, 256: 3000, 1024: 4100}


def window_raster():
    """all free but the pixel that holds (0.035, 0.035), an obstacle, and the one that holds (0.015, 0.035), low"""
    probe = orc.Oracle()
    occ = np.full((200, 200), 255, np.uint8)
    probe.set_grid(occ, (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    occ[probe.to_pixel((0.035, 0.035))] = 0
    occ[probe.to_pixel((0.015, 0.035))] = 200
    return occ


OBSTACLE_AT = (0.035, 0.035)


def one_region_raster(n_iter=3000, seed=0):
    """(2): the window of (1) on a raster with one obstacle pixel and one low pixel in it"""
    c = one_region(n_iter, seed)
    c.update(name="one_region_raster", occ=window_raster(), start=(0.01, 0.01))
    return c


def corner_window(n_iter=3000, seed=5):
    """(3): a window around a corner of four regions on the benchmark-like raster"""
    c = cases.cfg2(n_iter, seed=seed)
    c.update(name="corner_window", window=((-0.04, -0.84), (0.04, -0.76)), start=(0.0, -0.8))
    return c


PTO_K = 64


def pto_shelf_window(seed=1):
    c = cases.cfg3(1500, 1500, seed=seed)
    c.update(name="pto_shelf_window", window=((-0.84, -0.84), (-0.76, -0.76)))
    return c


def pto_door_window(seed=1):
    c = cases.cfg_door(1200, 1200, seed=seed)
    c.update(name="pto_door_window", window=((0.46, -0.64), (0.54, -0.56)))
    return c


PRM = dict(start=(0.025, 0.025), max_step=0.1, search_radius=5.0, n_iter=2000)
PRM_QUERIES = (((0.004, 0.004), (0.046, 0.046)), ((0.04, 0.01), (0.012, 0.044)), ((0.025, 0.025), (0.9, 0.9)))


def prm_pair(make_engine):
    """an engine (or a second oracle) and an oracle on the raster and in the window of (2)"""
    out = []
    for mk in (make_engine, orc.Oracle):
        x = mk()
        x.set_grid(window_raster(), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
        x.set_sampler(WINDOW[0], WINDOW[1], 0)
        out.append(x)
    return out


# (6) max_step, search_radius, iterations on cfg2(n, seed=3)
GEOMETRIES = {
    "long_steps_fixed_radius": (0.5, 50.0, 10500),           # (9000 iterations reach 1863 hits at the most)
    "long_steps_shrinking_radius": (0.5, 2.0, 4000),
    "short_steps": (0.02, 5.0, 4000),
    "radius_is_max_step": (0.1, 50.0, 4000),
    "radius_below_max_step": (0.1, 0.3, 4000),
    "largest_tile": (0.2895, 2.0, 4000),
    "largest_tile_by_rounding": (0.29, 2.0, 4000),           # 0.29 * 100 is 28.999999999999996 in f64: still below the limit of 29
    "no_tile": (0.2901, 2.0, 4000),
}
TILE_ROWS = ("largest_tile", "largest_tile_by_rounding", "no_tile")
GEOMETRY_K = 256


def geometry(name, seed=3, n_iter=None):
    max_step, search_radius, n = GEOMETRIES[name]
    c = cases.cfg2(n_iter or n, seed=seed)
    c.update(name=name, max_step=max_step, search_radius=search_radius)
    return c


def pto_tile(max_step):
    c = cases.cfg3(1500, 1500, seed=1)
    c.update(name="pto_step_%g" % max_step, max_step=max_step)
    return c
