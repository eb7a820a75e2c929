"""GPU parity of the two forms of the group kernels' connect pass (option conn_wg_waves):

  4  k_conn2_wg4: four waves per workgroup, the step's single workgroups (page filing, goal-point copies, goal path) in the same kernel;
  1  k_conn2 with one wave per workgroup + k_conn2_riders as a kernel of its own, before the samples (conn_riders_first = 1) or after.

Neither the size of a workgroup nor the place of the riders changes a load or an instruction of a sample, so every tree must equal the
oracle's -- and hence each other's -- bit for bit: positions, parents, dist_root, without a tie falling back to the host.
"""
import numpy as np
import pytest

import cases
from oracle import orc
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

# (conn_wg_waves, conn_riders_first)
FORMS = [(4, 1), (1, 1), (1, 0)]


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def _engine(eng_mod, case, form, **opts):
    e = cases.configure(eng_mod.Engine(), case)
    e.set_option("conn_wg_waves", form[0])
    e.set_option("conn_riders_first", form[1])
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def _same_bits(a, b):
    xa, pa, da = a.tree()
    xb, pb, db = b.tree()
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)) and np.array_equal(pa, pb) and np.array_equal(da.view(np.uint64), db.view(np.uint64))


def test_option_values(eng_mod):
    e = eng_mod.Engine()
    assert e.get_option("conn_wg_waves") in (1, 4)
    for v in (1, 4):
        e.set_option("conn_wg_waves", v)
        assert e.get_option("conn_wg_waves") == v
    for v in (0, 2, 3, 8):
        with pytest.raises(Exception):
            e.set_option("conn_wg_waves", v)
    assert e.get_option("n_heavy") == 0


@pytest.mark.parametrize("rows", [8, 9])
def test_bench_call_heavy_steps(eng_mod, rows):
    """The bench's call, shortened: `rows` configs[1] queries at K = 1024, ten full steps and an eleventh of 3 samples (fewer than one
    four-wave workgroup's 16, fewer than one wave's 4).  The first steps put most samples on the heavy path (more than 80 hits):
    n_heavy says that it ran.  8 rows take the XCD dealing of the rows, 9 do not have one.  Every row against the oracle."""
    n_iter = 10 * 1024 + 3
    cs = [cases.cfg2(n_iter, seed=70 + j) for j in range(rows)]
    orcs = []
    for c in cs:
        o = cases.configure(orc.Oracle(), c)
        cases.grow(o, c, K=1024, algo=orc.ALGO_BATCHED_KD)
        orcs.append(o)
    first = None
    for form in FORMS:
        engs = [_engine(eng_mod, c, form) for c in cs]
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, n_iter, 1024)
        assert engs[0].get_option("group_lanes") == 16 and engs[0].get_option("conn_wg_waves") == form[0]
        heavy = [e.get_option("n_heavy") for e in engs]
        print("form", form, "rows", rows, "n_heavy", heavy)
        assert all(h > 0 for h in heavy), "the heavy path did not run"
        for e, o in zip(engs, orcs):
            assert_same(e, o)
        if first is None:
            first = engs
        else:
            assert heavy == [e.get_option("n_heavy") for e in first]
            for e, f in zip(engs, first):
                _same_bits(e, f)


def test_one_wave_per_sample_in_the_first_steps(eng_mod):
    """early_wave_steps: the first steps' connect pass with 64 lanes per sample (one sample per wave, one per workgroup in the one-wave
    form), the rest with 16 -- both group sizes of both forms in one run, in two launch sequences side by side."""
    n_iter = 6 * 1024 + 1
    cs = [cases.cfg2(n_iter, seed=90 + j) for j in range(10)]
    for form in FORMS:
        engs = [_engine(eng_mod, c, form, early_wave_steps=3, batch_streams=2) for c in cs]
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, n_iter, 1024)
        for j in (0, 4, 5, 9):
            o = cases.configure(orc.Oracle(), cs[j])
            cases.grow(o, cs[j], K=1024, algo=orc.ALGO_BATCHED_KD)
            assert_same(engs[j], o)


def _dup_samples(n, seed):
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(-0.02, 0.02, n), rng.uniform(-0.92, -0.88, n)], axis=1)
    xy[::3] = xy[(np.arange(0, n, 3) // 7) * 2 + 1]          # exact duplicates of other samples: equal-cost parents off the goal path
    return xy


def test_injected_duplicates_force_the_build_after_the_steps(eng_mod):
    """Injected exact duplicates tie off the goal path: the whole kd structure is built after the steps (kd_built_after), from what the
    riders and the samples of every step left.  A batch of eight with duplicates in three rows, a dense cluster (every sample heavy)."""
    n = 4000
    case = cases.cfg2(n - n // 100 - 5)
    sets = [_dup_samples(n, 20 + j) if j % 3 == 0 else None for j in range(8)]
    cs = [cases.Case(case, seed=50 + j) for j in range(8)]
    orcs = []
    for j, c in enumerate(cs):
        o = cases.configure(orc.Oracle(), c)
        if sets[j] is not None:
            o.set_samples(sets[j])
        cases.grow(o, c, K=512, algo=orc.ALGO_BATCHED_KD)
        orcs.append(o)
    first = None
    for form in FORMS:
        engs = [_engine(eng_mod, c, form) for c in cs]
        for j, e in enumerate(engs):
            if sets[j] is not None:
                e.set_samples(sets[j])
        eng_mod.Engine.grow_batch(engs, [case.start] * 8, case.max_step, case.search_radius, case.n_iter_min, 512)
        assert engs[0].get_option("kd_lazy") == 1 and engs[0].get_option("kd_built_after") == 1
        assert engs[0].get_option("n_heavy") > 0
        for e, o in zip(engs, orcs):
            assert_same(e, o)
        if first is None:
            first = engs
        else:
            for e, f in zip(engs, first):
                _same_bits(e, f)
