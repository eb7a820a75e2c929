"""Inputs of tests/test_gpu_step_trips.py: the smallest batches at which the step kernels' set-up loads can go wrong (the valid-mask words
held by the lanes of a group, the class and the clearance byte of a pixel asked for whether or not the pixel exists, the loads issued
beside them), and what each of them has to produce, computed from the oracle alone (tests/test_step_trips_inputs_cpu.py asserts it).

Every input is a Batch: the rows' cases, their injected samples (or None: the row's own sampler), the step size K, the iterations --
one number, or (n_iter_min, n_iter_max) per row for rows with step plans of their own -- and the step geometry of the call.
"""
import numpy as np

import cases
from oracle import orc

W = 200                 # pixels per side of the rasters here, over [-1, 1)^2
PPM = 100.0


class Batch(dict):
    __getattr__ = dict.__getitem__


def batch(cs, K, n_iter, samples=None, n_iter_max=None, max_step=None, search_radius=None):
    return Batch(cases=cs, K=K, n_iter=n_iter, n_iter_max=n_iter_max, samples=samples or [None] * len(cs),
                 max_step=cs[0].max_step if max_step is None else max_step, search_radius=cs[0].search_radius if search_radius is None else search_radius)


# ---------------------------------------------------------------- the oracle's side
def configure(x, case, samples=None):
    if case.get("occ") is not None:
        x.set_grid(case.occ, (-1.0, -1.0), (1.0, 1.0), case.domain)
        x.set_sampler((-1.0, -1.0), (1.0, 1.0), case.seed)
        x.set_square_goal(np.array(case.goals, dtype=np.float64), np.array(case.masks, dtype=np.uint64), case.l1)
    else:
        cases.configure(x, case)
    if samples is not None:
        x.set_samples(samples)
    return x


def row_iters(bt, j):
    """(n_iter_min, n_iter_max) of row j"""
    mn = bt.n_iter[j] if isinstance(bt.n_iter, (list, tuple)) else bt.n_iter
    mx = mn if bt.n_iter_max is None else (bt.n_iter_max[j] if isinstance(bt.n_iter_max, (list, tuple)) else bt.n_iter_max)
    return mn, mx


def oracle_row(bt, j, n_iter=None):
    """the oracle grown on row j (n_iter: a fixed budget in place of the row's own)"""
    mn, mx = row_iters(bt, j) if n_iter is None else (n_iter, n_iter)
    c = bt.cases[j]
    o = configure(orc.Oracle(), c, bt.samples[j])
    o.grow(c.start, bt.max_step, bt.search_radius, mn, mx, batch_K=bt.K, mode=cases.RRT, algo=orc.ALGO_BATCHED_KD)
    return o


_GROWN = {}


def oracles(name):
    """the oracles of every row of the named batch, grown once and left unchanged"""
    if name not in _GROWN:
        bt = BATCHES[name]()
        _GROWN[name] = (bt, [oracle_row(bt, j) for j in range(len(bt.cases))])
    return _GROWN[name]


def sizes(bt, j, steps):
    """nodes of row j's tree at the start of step 0 .. steps (a shorter run's tree is a prefix of a longer one's)"""
    return [1] + [oracle_row(bt, j, n_iter=s * bt.K).num_nodes() for s in range(1, steps + 1)]


def pixel(p):
    """(i, j) of a state on the rasters here (map_shelves_io.rs:165-170: `as u32` truncates and sends a negative number to 0), without the
    range check"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    return (np.trunc(((W - 1) - (p[:, 1] + 1.0) * PPM).clip(0, 2 * W)).astype(int), np.trunc(((p[:, 0] + 1.0) * PPM).clip(0, 2 * W)).astype(int))


# ---------------------------------------------------------------- rasters
def mix_raster(seed=5):
    """free, strewn with small blocks of the three kinds of shelf pixel: 0 (high, the class with the early return: CLS_HIGH0), 60 (high)
    and 200 (low); the rim (three pixels) and the middle stay free"""
    rng = np.random.default_rng(seed)
    occ = np.full((W, W), 255, np.uint8)
    for n in range(240):
        i, j = rng.integers(4, W - 8, 2)
        h, w = rng.integers(1, 5, 2)
        occ[i:i + h, j:j + w] = (0, 60, 200)[n % 3]
    occ[92:108, 92:108] = 255
    return occ


def raster_case(n_iter, seed, start=(0.0, 0.0), goal=(0.7, 0.7)):
    return cases.Case(name="mix", grid=None, occ=mix_raster(), zones=None, visibility=0.0, domain=cases.SHELF, mode=cases.RRT, start=start,
                      goals=[goal], masks=[1], l1=0.05, obs_zone=None, max_step=0.1, search_radius=2.0, n_iter_min=n_iter, n_iter_max=n_iter,
                      seed=seed)


def border_samples(n, seed):
    """n samples over the whole raster [-1, 1)^2, every 16th inside the outermost pixels: row 0, row H - 1, column 0, column W - 1 in
    turn (the first four of them in the four corner pixels)"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-1.0, 1.0, (n, 2))
    edge = np.arange(0, n, 16)
    for t, a in enumerate(edge):
        u = rng.uniform(0.0, 0.0099)
        side = t % 4
        if side == 0: s[a, 1] = 0.99 + u                  # row 0
        elif side == 1: s[a, 1] = -1.0                    # row H - 1: i = (H - 1) - (y + 1) ppm truncated, so the box's low edge alone
        elif side == 2: s[a, 0] = -1.0 + u                # column 0
        else: s[a, 0] = 0.99 + u                          # column W - 1
    for t, (cx, cy) in enumerate([(-0.996, 0.994), (0.994, 0.994), (-0.996, -1.0), (0.994, -1.0)]):
        s[edge[t]] = (cx, cy)
    return np.minimum(s, np.nextafter(1.0, 0.0))


# ---------------------------------------------------------------- the batches
K_ITERS = {64: 640, 1024: 4096, 2048: 6000}


def mask_words(K, rows):
    """K = 64 / 1024 / 2048: one word of the step's valid mask, one per lane of a 16-lane group, two per lane (the last step of 2048 is a
    short one); 8 rows take the dealing of rows to XCDs, 3 do not"""
    return batch([cases.cfg2(K_ITERS[K], seed=500 + j) for j in range(rows)], K, K_ITERS[K])


def border(rows=8):
    """the raster of three kinds of shelf pixel, the sampler's box the raster's own: samples in the outermost pixels and on CLS_HIGH0
    pixels, ten steps of 256 from a tree of one node"""
    n = 2560
    cs = [raster_case(n, seed=600 + j) for j in range(rows)]
    return batch(cs, 256, n, samples=[border_samples(n, 700 + j) for j in range(rows)])


def outside():
    """three rows on the raster above, the start 0.03 from its right rim; row 1's stream holds a sample 0.005 beyond the rim, within
    max_step (L1) of the start: it is not steered, and its pixel does not exist (the reference panics, the oracle reports it)"""
    n = 128
    cs = [raster_case(n, seed=610 + j, start=(0.97, 0.0), goal=(0.5, 0.5)) for j in range(3)]
    sets = []
    for j in range(3):
        s = np.random.default_rng(710 + j).uniform((0.9, -0.1), (0.999, 0.1), (n, 2))
        if j == 1:
            s[70] = (1.005, 0.01)
        sets.append(s)
    return batch(cs, 64, n, samples=sets)


def no_raster(rows=8):
    """rows without a raster: no class, no clearance, nothing to ask for"""
    return batch([cases.empty_space(2560, 2560, seed=620 + j) for j in range(rows)], 256, 2560)


def short_steps(rows=8):
    """max_step 0.02: most samples are steered for many steps, and the class of the steered state is fetched again"""
    n = 2560
    cs = [raster_case(n, seed=630 + j) for j in range(rows)]
    return batch(cs, 256, n, samples=[border_samples(n, 730 + j) for j in range(rows)], max_step=0.02)


def long_steps(rows=8):
    """max_step 0.5: the radius search's disc meets so many regions that the young-tree streaming lasts"""
    n = 2560
    cs = [raster_case(n, seed=640 + j) for j in range(rows)]
    return batch(cs, 256, n, samples=[border_samples(n, 740 + j) for j in range(rows)], max_step=0.5)


def own_plans(rows=8):
    """rows with step plans of their own (n_iter_min differs): row 0 reaches its goal -- one step away from its start -- and ends at its
    n_iter_min of 300 while the others, whose goal is out of reach, go on to their n_iter_max"""
    mn = [300] + [600 + 100 * (j % 3) for j in range(1, rows)]
    mx = [1500] * rows
    cs = []
    for j in range(rows):
        c = cases.cfg2(mn[j], seed=650 + j)
        c.update(goals=[(0.05, -0.95)] if j == 0 else [(0.9, 0.0)], n_iter_max=mx[j])
        cs.append(c)
    return batch(cs, 128, mn, n_iter_max=mx)


def goal_reached(rows=8):
    """the goal one step from the start (the case of test_gpu_run_constants.py), 1100 iterations at K = 256: every row reaches it and
    re-adds the goal point every hundredth iteration -- slots with bq_k = 0xFFFF and the clone workgroup"""
    cs = []
    for j in range(rows):
        c = cases.cfg2(1100, seed=660 + j)
        c.update(goals=[(0.15, -0.85)])
        cs.append(c)
    return batch(cs, 256, 1100)


BATCHES = {
    "words64x8": lambda: mask_words(64, 8), "words64x3": lambda: mask_words(64, 3),
    "words1024x8": lambda: mask_words(1024, 8), "words1024x3": lambda: mask_words(1024, 3),
    "words2048x8": lambda: mask_words(2048, 8), "words2048x3": lambda: mask_words(2048, 3),
    "border": border, "border3": lambda: border(3), "no_raster": no_raster, "short_steps": short_steps, "long_steps": long_steps,
    "own_plans": own_plans, "goal_reached": goal_reached,
}
