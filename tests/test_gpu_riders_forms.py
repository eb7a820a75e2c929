"""GPU parity of the two forms of the riders' page filing and goal path (developer option riders_fast):

  1  file_step_fast<256> and g_track_step<2>: every load that depends on nothing in one round trip before the first barrier;
  0  insert_step_pages<1> and g_track_step<1>, the forms the riders had beside a connect pass several times their length.

Both in k_conn2_riders (conn_wg_waves = 1) and as the first workgroups of k_conn2_wg4 (conn_wg_waves = 4).  The forms file the same nodes
into the same pages (up to the order inside a region's pages, which no search depends on) and extend the goal path by the same nodes in the
same order, so every tree must equal the oracle's -- and hence each other's -- bit for bit.
"""
import numpy as np
import pytest

import cases
from oracle import orc
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

# (riders_fast, conn_wg_waves)
FORMS = [(0, 1), (1, 1), (0, 4), (1, 4)]


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def _engine(eng_mod, case, form, **opts):
    e = cases.configure(eng_mod.Engine(), case)
    e.set_option("group_lanes", 16)             # (the group kernels whatever the number of rows: fewer than 8 would take the single query's)
    e.set_option("riders_fast", form[0])
    e.set_option("conn_wg_waves", form[1])
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def _same_bits(a, b):
    xa, pa, da = a.tree()
    xb, pb, db = b.tree()
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)) and np.array_equal(pa, pb) and np.array_equal(da.view(np.uint64), db.view(np.uint64))


def _oracles(cs, K, sets=None):
    out = []
    for j, c in enumerate(cs):
        o = cases.configure(orc.Oracle(), c)
        if sets is not None and sets[j] is not None:
            o.set_samples(sets[j])
        cases.grow(o, c, K=K, algo=orc.ALGO_BATCHED_KD)
        out.append(o)
    return out


def _all_forms(eng_mod, cs, orcs, K, sets=None, check=None):
    """Grow the rows in every form; every tree against the oracle's, and bit-equal between the forms."""
    c0 = cs[0]
    first = None
    for form in FORMS:
        engs = [_engine(eng_mod, c, form) for c in cs]
        if sets is not None:
            for e, s in zip(engs, sets):
                if s is not None:
                    e.set_samples(s)
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], c0.max_step, c0.search_radius, c0.n_iter_min, K)
        assert engs[0].get_option("group_lanes") == 16 and engs[0].get_option("kd_lazy") == 1
        assert engs[0].get_option("riders_fast") == form[0] and engs[0].get_option("conn_wg_waves") == form[1]
        if check is not None:
            check(engs)
        for e, o in zip(engs, orcs):
            assert_same(e, o)
        if first is None:
            first = engs
        else:
            for e, f in zip(engs, first):
                _same_bits(e, f)


def test_option_values(eng_mod):
    e = eng_mod.Engine()
    assert e.get_option("riders_fast") == 1
    for v in (0, 1):
        e.set_option("riders_fast", v)
        assert e.get_option("riders_fast") == v
    for v in (-1, 2, 4):
        with pytest.raises(Exception):
            e.set_option("riders_fast", v)
    assert e.get_option("riders_fast") == 1


@pytest.mark.parametrize("rows", [8, 9])
def test_rows_and_a_short_last_step(eng_mod, rows):
    """`rows` configs[1] queries at K = 1024 (four samples in each of the 256 threads), ten full steps and an eleventh of 3 samples: fewer than
    one pass of the threads.  8 rows take the XCD dealing of the rows, 9 do not have one."""
    n_iter = 10 * 1024 + 3
    cs = [cases.cfg2(n_iter, seed=170 + j) for j in range(rows)]
    _all_forms(eng_mod, cs, _oracles(cs, 1024), 1024)


def test_k_that_does_not_divide_the_threads(eng_mod):
    """K = 320: the second sample slot of a thread is taken by 64 threads only, the third and fourth by none (the k < nb guards); a last
    step of 7."""
    n_iter = 4 * 320 + 7
    cs = [cases.cfg2(n_iter, seed=180 + j) for j in range(3)]
    _all_forms(eng_mod, cs, _oracles(cs, 320), 320)


def test_k_above_the_fast_filing(eng_mod):
    """K = 2048, 3 steps: more samples than file_step_fast<256> holds per thread -- the filing stays insert_step_pages<1> in both forms --
    and two passes of g_track_step<2>'s sample loop, the candidates' coordinates read back from memory."""
    n_iter = 3 * 2048
    cs = [cases.cfg2(n_iter, seed=190 + j) for j in range(2)]
    _all_forms(eng_mod, cs, _oracles(cs, 2048), 2048)


def _box_samples(n, seed):
    """samples inside ONE region of the 40 x 40 grid over [-1, 1]^2: the cell [0, 0.05) x [-0.95, -0.9), a step from the start (0, -1)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.005, 0.045, n), rng.uniform(-0.945, -0.905, n)], axis=1)


def test_several_new_pages_for_one_region_in_a_step(eng_mod):
    """Samples injected into one small box: one region gains hundreds of nodes in a step, so more than one new page (64 slots) at once --
    p_new - p_old >= 2 -- and every sample's neighbour list overflows LDS (n_heavy).  Two rows of four with injected samples."""
    n, K = 2000, 512
    case = cases.cfg2(n - n // 100 - 5)
    sets = [_box_samples(n, 30 + j) if j % 2 == 0 else None for j in range(4)]
    cs = [cases.Case(case, seed=150 + j) for j in range(4)]
    orcs = _oracles(cs, K, sets)
    steps = (case.n_iter_min + K - 1) // K
    for j in (0, 2):
        x = orcs[j].tree()[0]
        cell = np.floor((x[:, 0] + 1.0) * 20.0).astype(int) + 40 * np.floor((x[:, 1] + 1.0) * 20.0).astype(int)
        most = np.bincount(cell).max()
        # some step gives that region at least most / steps nodes: an old page's free slots take fewer than 64 of them, 128 more need two new pages
        assert most >= steps * 3 * 64, "the injected samples do not fill one region: %d nodes in %d steps" % (most, steps)

    def dense(engs):
        assert engs[0].get_option("n_heavy") > 0 and engs[2].get_option("n_heavy") > 0, "the cluster was not dense"
    _all_forms(eng_mod, cs, orcs, K, sets, dense)


def test_goal_copies_from_the_first_steps(eng_mod):
    """The start one step from the goal point: every hundredth sample is the goal point itself and is steered exactly onto it from the
    first step on, so the clone workgroup and the goal path's sequential wave serve several copies per step (five at K = 512).  The counts
    are read from the oracle: the tree of a shorter run is a prefix of a longer one's, so its size is the longer run's size at that step."""
    K, steps = 512, 5
    n_iter = steps * K + 37

    def near_goal(n, seed):
        c = cases.cfg2(n, seed=seed)
        c.update(start=(0.85, -0.03))
        return c
    cs = [near_goal(n_iter, 160 + j) for j in range(3)]
    orcs = _oracles(cs, K)
    goal = np.array(cs[0].goals[0])
    for j, o in enumerate(orcs):
        x = o.tree()[0]
        copies = np.flatnonzero((x[:, 0] == goal[0]) & (x[:, 1] == goal[1]))
        assert len(copies) >= 20, "too few copies of the goal point: %d" % len(copies)
        n_at = [1] + [_oracles([near_goal(s * K, 160 + j)], K)[0].num_nodes() for s in range(1, steps + 1)] + [len(x)]
        per_step = np.histogram(copies, bins=n_at)[0]
        assert per_step.sum() == len(copies) and per_step.max() >= 2, "no step with two copies of the goal point: %s" % per_step
    _all_forms(eng_mod, cs, orcs, K)
