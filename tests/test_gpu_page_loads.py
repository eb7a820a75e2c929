"""GPU parity of the step kernels' page loads (the buffer views of pg_xy / pg_id / pg_d, PageBuf in porrt_device.hpp): the cases at which
a load that takes its bound from a descriptor and its address from a 32-bit offset can go wrong.

  fill levels     regions that hold exactly 1 .. 129 nodes: the edge of every 16-lane row of a page, of a page, of the second and third
                  page (directory and pool pages) -- a lane past the fill must get nothing and count for nothing
  bound           a short run makes the page pool small; the dense start puts hundreds of nodes into a few regions, whose pool pages a
                  descriptor that is too short would drop
  young tree      the first steps stream the id-ordered arrays instead and hand over to the pages while the tree grows
  heavy samples   more hits than the LDS list holds, with the memory lists at their smallest capacity
  goal copies     the clone workgroup serves a list
  rows            every row of a batch has its own arrays: its own descriptors
  fallback        a sample without a connectable neighbour asks for its nearest node out of line (group_nn_call)

Everything runs the group kernels (group_lanes = 16) at K = 256, as one-wave workgroups with riders (conn_wg_waves = 1) and as four-wave
workgroups (4), and every tree must equal the oracle's bit for bit.  What a case needs of its input is asserted from the oracle's tree, so
that a set which stops producing it fails instead of passing.
"""
import numpy as np
import pytest

import cases
from confined_inputs import hits_per_node as _hits_per_node, n_at as _n_at
from oracle import orc
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

K = 256
WAVES = [1, 4]


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def _engine(eng_mod, case, waves, **opts):
    e = cases.configure(eng_mod.Engine(), case)
    e.set_option("group_lanes", 16)
    e.set_option("conn_wg_waves", waves)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def _oracle(case, samples=None, n_iter=None):
    c = case if n_iter is None else cases.Case(case, n_iter_min=n_iter, n_iter_max=n_iter)
    o = cases.configure(orc.Oracle(), c)
    if samples is not None:
        o.set_samples(samples)
    cases.grow(o, c, K=K, algo=orc.ALGO_BATCHED_KD)
    return o


def _grow_rows(eng_mod, cs, waves, sets=None, n_iter=None, **opts):
    engs = [_engine(eng_mod, c, waves, **opts) for c in cs]
    for e, s in zip(engs, sets or [None] * len(cs)):
        if s is not None:
            e.set_samples(s)
    c0 = cs[0]
    eng_mod.Engine.grow_batch(engs, [c.start for c in cs], c0.max_step, c0.search_radius, c0.n_iter_min if n_iter is None else n_iter, K)
    assert engs[0].get_option("group_lanes") == 16 and engs[0].get_option("conn_wg_waves") == waves
    return engs


def _cell(x):
    """region of a point: the 40 x 40 grid over [-1, 1)^2 (rep_cell)"""
    return np.floor((x[:, 0] + 1.0) * 20.0).astype(int) + 40 * np.floor((x[:, 1] + 1.0) * 20.0).astype(int)


# ---------------------------------------------------------------- fill levels
FILLS = [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 128, 129]
FILL_STEPS = 3                 # steps that build the fills; one more step searches them


def _fill_case():
    c = cases.empty_space(n_iter_min=(FILL_STEPS + 1) * K, n_iter_max=(FILL_STEPS + 1) * K)
    return c


def _fill_samples():
    """Injected samples on the empty map, start (0, 0), max_step 0.1: a sample within 0.09 (L1) of a node of the step's snapshot is not
    steered and becomes a node where it lies, so the tree is built by hand -- into 13 regions of the 4 x 4 block around the start exactly
    FILLS nodes (the start's own region takes the 129, the root included), everything else into regions outside the targets.  Every
    hundredth iteration is the goal point (0.9, 0.9), not an injected sample: it is steered up and to the right, into region (21, 21) or
    beyond, which is no target.  -> (samples, {region: nodes})"""
    rng = np.random.default_rng(11)
    block = [(cx, cy) for cy in range(18, 22) for cx in range(18, 22)]
    spare = [(21, 21), (18, 18), (18, 21)]
    cells = [c for c in block if c not in spare and c != (20, 20)]
    want = {(20, 20): 129}
    want.update(zip(cells, [f for f in FILLS if f != 129]))
    assert len(want) == len(FILLS)
    pending = dict(want)
    pending[(20, 20)] -= 1                                    # the root
    nodes = [np.zeros(2)]
    out = []

    def reach(pts, snap):
        return np.abs(pts[:, None, :] - snap[None, :, :]).sum(axis=2).min(axis=1) < 0.09

    def inside(cell, n):
        lo = np.array(cell) * 0.05 - 1.0
        return lo + rng.uniform(0.002, 0.048, (n, 2))
    for s in range(FILL_STEPS + 1):
        n_inj = K - len([i for i in range(s * K + 1, (s + 1) * K + 1) if i % 100 == 0])
        snap = np.array(nodes)
        batch = []
        for cell in sorted(pending, key=lambda c: -pending[c]):
            need = min(pending[cell], n_inj - len(batch))
            if need <= 0:
                continue
            pts = inside(cell, 8 * need + 64)
            pts = pts[reach(pts, snap)][:need]
            batch.extend(pts)
            pending[cell] -= len(pts)
        while len(batch) < n_inj:                             # the rest: anywhere near the tree outside the targets
            pts = rng.uniform(-0.3, 0.3, (4 * K, 2))
            cxy = np.floor((pts + 1.0) * 20.0).astype(int)
            free = np.array([(a, b) not in want for a, b in cxy])
            pts = pts[free & reach(pts, snap)][:n_inj - len(batch)]
            batch.extend(pts)
        if s == FILL_STEPS - 1:
            assert not any(pending.values()), "the fills are not complete after %d steps: %s" % (FILL_STEPS, pending)
        nodes.extend(batch)
        out.extend(batch)
    return np.array(out), {cx + 40 * cy: n for (cx, cy), n in want.items()}


@pytest.fixture(scope="module")
def fill_set():
    case = _fill_case()
    samples, want = _fill_samples()
    o = _oracle(case, samples)
    n_at = _oracle(case, samples, n_iter=FILL_STEPS * K).num_nodes()      # (a shorter run's tree is a prefix of a longer one's)
    return case, samples, want, o, n_at


def test_fill_levels_hold_in_the_oracle(fill_set):
    case, samples, want, o, n_at = fill_set
    x = o.tree()[0]
    assert n_at > 400 and len(x) > n_at, "the step after the fills does not walk the pages (a disc meets at most 25 regions: 25 * 16 nodes)"
    have = np.bincount(_cell(x[:n_at]), minlength=1600)
    for reg, n in want.items():
        assert have[reg] == n, "region %d holds %d nodes at the start of step %d, not %d" % (reg, have[reg], FILL_STEPS, n)
    assert sorted(want.values()) == FILLS                    # (the last step's samples lie in and around the block: they search these regions)


@pytest.mark.parametrize("waves", WAVES)
def test_fill_levels(eng_mod, fill_set, waves):
    case, samples, want, o, n_at = fill_set
    e, = _grow_rows(eng_mod, [case], waves, [samples])
    assert_same(e, o)


# ---------------------------------------------------------------- the dense start: bound of the arrays, heavy samples, list capacity
DENSE_ITER = 3000


@pytest.fixture(scope="module")
def dense_set():
    case = cases.cfg2(DENSE_ITER, seed=7)
    o = _oracle(case)
    steps = (DENSE_ITER + K - 1) // K
    n_at = _n_at(case, steps - 1, K) + [o.num_nodes()]
    return case, o, n_at, _hits_per_node(case, o, n_at)


def test_dense_start_in_the_oracle(dense_set):
    case, o, n_at, hits = dense_set
    x = o.tree()[0]
    assert (hits > 80).any() and (hits > 320).any(), "no sample beyond the LDS lists of 16 and of 64 lanes: most hits %d" % hits.max()
    fill = np.bincount(_cell(x[:n_at[-2]]), minlength=1600)
    assert np.count_nonzero(fill > 64) >= 4, "too few regions with pool pages (behind the 1600 static ones): fullest %d" % fill.max()


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("tight", [False, True])
def test_dense_start(eng_mod, dense_set, waves, tight):
    """tight: cand_cap at the most hits of any sample (at least the option's minimum of 64) -- the memory lists end where the last hit is
    written; a list that overflowed would have grown the option and replayed the call."""
    case, o, n_at, hits = dense_set
    opts = {"cand_cap": max(64, int(hits.max()))} if tight else {}
    e, = _grow_rows(eng_mod, [case], waves, **opts)
    assert e.get_option("n_heavy") > 0
    if tight:
        assert e.get_option("cand_cap") == opts["cand_cap"], "the lists overflowed at the oracle's own count of hits"
    assert_same(e, o)


# ---------------------------------------------------------------- young tree and its hand-over
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("early", [None, 0])
def test_young_tree_hand_over(eng_mod, waves, early):
    """Steps 0-12 of configs[1], nothing injected: the first steps stream nx / ny / distA (nreg * 16 > N), the later ones walk the pages,
    with one wave per sample in the first steps (early_wave_steps at its default) and with 16 lanes from the first step on (0)."""
    case = cases.cfg2(13 * K, seed=21)
    o = _oracle(case)
    e, = _grow_rows(eng_mod, [case], waves, **({} if early is None else {"early_wave_steps": early}))
    assert_same(e, o)


# ---------------------------------------------------------------- goal copies
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("waves", WAVES)
def test_goal_copies(eng_mod, waves, fast):
    """The start one step from the goal point (the case of test_gpu_riders_forms.py), 6000 iterations: sixty copies of the goal point, which
    the clone workgroup serves from a list in memory once the neighbourhood holds more nodes than its LDS."""
    case = cases.cfg2(6000, seed=161)
    case.update(start=(0.85, -0.03))
    o = _oracle(case)
    x = o.tree()[0]
    goal = np.array(case.goals[0])
    assert np.count_nonzero((x[:, 0] == goal[0]) & (x[:, 1] == goal[1])) >= 20
    e, = _grow_rows(eng_mod, [case], waves, riders_fast=fast)
    assert_same(e, o)


# ---------------------------------------------------------------- rows with their own bases
@pytest.mark.parametrize("rows", [8, 3])
@pytest.mark.parametrize("waves", WAVES)
def test_rows_with_their_own_arrays(eng_mod, waves, rows):
    """8 rows take the XCD dealing of the rows, 3 do not; seeds differ, and the rows run two different numbers of iterations, so their
    page pools differ in size: every row is searched through descriptors of its own."""
    n_iters = [2000 if j % 2 else 3500 for j in range(rows)]
    cs = [cases.cfg2(n, seed=300 + j) for j, n in enumerate(n_iters)]
    engs = [_engine(eng_mod, c, waves) for c in cs]
    eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, n_iters, K)
    for e, c in zip(engs, cs):
        assert_same(e, _oracle(c))


# ---------------------------------------------------------------- nearest-node fallback
def _blocks_raster():
    """the block-strewn raster of test_gpu_parity_r3.py::test_segments_around_many_corners"""
    W = 200
    rng = np.random.default_rng(5)
    occ = np.full((W, W), 255, np.uint8)
    for _ in range(260):
        i, j = rng.integers(4, W - 8, 2)
        h, w = rng.integers(1, 5, 2)
        occ[i:i + h, j:j + w] = 0 if rng.random() < 0.7 else 200
    occ[95:105, 95:105] = 255
    return occ


def _crosses(occ, a, b, only=None):
    """does the straight line a -> b pass a pixel that is not free (only: that has this value)?  (finely sampled: a proxy for the ray of
    map_shelves_io.rs:187-203, with the pixel transform of map_shelves_io.rs:165-170)"""
    t = np.linspace(0.0, 1.0, 64)[:, None]
    p = a[None, :] * (1.0 - t) + b[None, :] * t
    i = np.clip((199.0 - (p[:, 1] + 1.0) * 100.0).astype(int), 0, 199)
    j = np.clip(((p[:, 0] + 1.0) * 100.0).astype(int), 0, 199)
    return bool((occ[i, j] != 255).any() if only is None else (occ[i, j] == only).any())


@pytest.mark.parametrize("waves", WAVES)
def test_nearest_node_fallback(eng_mod, waves):
    """A sample none of whose neighbours is connectable hangs below its nearest node whatever lies between (rrt.rs:132-134): for a sample
    that was not steered the connect pass searches that node itself (group_nn_call).  Such nodes exist here: their edge crosses a block."""
    occ = _blocks_raster()

    def make(x, seed):
        x.set_grid(occ, (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
        x.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
        x.set_square_goal(np.array([(0.7, 0.7)]), np.array([1], dtype=np.uint64), 0.05)
        return x
    n_iter, rows = 6000, 3
    orcs = []
    for s in range(rows):
        o = make(orc.Oracle(), 70 + s)
        o.grow((0.0, 0.0), 0.1, 2.0, n_iter, n_iter, batch_K=K, mode=cases.RRT, algo=orc.ALGO_BATCHED_KD)
        orcs.append(o)
    x, parent, _ = orcs[0].tree()
    # ... of a sample that was not steered: its edge to the nearest node is shorter (L1) than max_step (common.rs:215-225), and the block it
    # crosses is an obstacle (0), whatever the half pixel the proxy may be off by at a block's rim: the segment's middle third is looked at
    blocked = [i for i in range(1, len(x)) if np.abs(x[i] - x[parent[i]]).sum() < 0.1 * (1.0 - 1e-9)
               and _crosses(occ, x[parent[i]] + (x[i] - x[parent[i]]) / 3.0, x[parent[i]] + 2.0 * (x[i] - x[parent[i]]) / 3.0, only=0)]
    assert len(blocked) >= 3, "no unsteered sample hangs below its nearest node across an obstacle"
    engs = [make(eng_mod.Engine(), 70 + s) for s in range(rows)]
    for e in engs:
        e.set_option("group_lanes", 16)
        e.set_option("conn_wg_waves", waves)
    eng_mod.Engine.grow_batch(engs, [(0.0, 0.0)] * rows, 0.1, 2.0, n_iter, K)
    for e, o in zip(engs, orcs):
        assert_same(e, o)
