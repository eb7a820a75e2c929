"""GPU parity of the forms of the group kernels' rewire commit (option commit_flat):

  0  a group of 16 lanes per sample (commit_rrt_sample in k_nn2's commit workgroups, k_commit2 after the last step);
  1  a workgroup per span of 128 samples, one lane per candidate record (commit_flat_span: k_nn2's commit workgroups, k_commit_flat).

The flat form makes the same stores with the same values -- the parent is a minimum over the new ids, all winners of a node carry the
same bits -- so every tree must equal the oracle's, and hence the other form's, bit for bit: positions, parents, dist_root, without a
tie falling back to the host.  References (oracle trees, single grows) are computed once per module and shared by the forms.
(The search with one lane per sample that the same work tried, option nn_pack_from, was bit-exact and slower and is not in the tree:
profiles/nn2_forms_experiments.txt.)
"""
import numpy as np
import pytest

import cases
from oracle import orc
from test_gpu_parity import assert_same, run_gpu

pytestmark = pytest.mark.gpu

FORMS = [0, 1]          # commit_flat


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


_ORC = {}


def _oracle(key, case, K, samples=None):
    if key not in _ORC:
        o = cases.configure(orc.Oracle(), case)
        if samples is not None:
            o.set_samples(samples)
        cases.grow(o, case, K=K, algo=orc.ALGO_BATCHED_KD)
        _ORC[key] = o
    return _ORC[key]


def _engine(eng_mod, case, form, **opts):
    e = cases.configure(eng_mod.Engine(), case)
    e.set_option("commit_flat", form)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def _same_bits(a, b):
    xa, pa, da = a.tree()
    xb, pb, db = b.tree()
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)) and np.array_equal(pa, pb) and np.array_equal(da.view(np.uint64), db.view(np.uint64))


def _forms_agree(runs):
    first = runs[0]
    for engs in runs[1:]:
        for e, f in zip(engs, first):
            _same_bits(e, f)


def test_option_values(eng_mod):
    e = eng_mod.Engine()
    assert e.get_option("commit_flat") in (0, 1)
    for v in (0, 1, 0):
        e.set_option("commit_flat", v)
        assert e.get_option("commit_flat") == v
    for v in (-1, 2, 16, 128):
        with pytest.raises(Exception):
            e.set_option("commit_flat", v)
        assert e.get_option("commit_flat") == 0


HEAVY_N = 10 * 1024 + 3


def _heavy_cases(rows):
    return [cases.cfg2(HEAVY_N, seed=70 + j) for j in range(rows)]


@pytest.mark.parametrize("rows", [8, 9])
def test_heavy_first_steps(eng_mod, rows):
    """The bench's call, shortened: ten full steps at K = 1024 and an eleventh of 3 samples (fewer than a span, fewer than a wave).  The
    first steps leave hundreds of records per sample (n_heavy > 0): a span makes many passes.  8 rows take the XCD dealing of the rows
    and replay a hipGraph, 9 have no dealing."""
    cs = _heavy_cases(rows)
    runs = []
    for form in FORMS:
        engs = [_engine(eng_mod, c, form) for c in cs]
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, HEAVY_N, 1024)
        assert engs[0].get_option("group_lanes") == 16 and engs[0].get_option("commit_flat") == form
        assert all(e.get_option("n_heavy") > 0 for e in engs), "the heavy path did not run"
        for j, (e, c) in enumerate(zip(engs, cs)):
            assert_same(e, _oracle(("heavy", j), c, 1024))
        if rows == 8:
            # the same engines again: the captured graph is replayed (the samplers have moved on: compare the forms with each other)
            eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, HEAVY_N, 1024)
            assert all(e.metrics()["n_tie_fallbacks"] == 0 for e in engs)
        runs.append(engs)
    _forms_agree(runs)


def _dup_samples(n, seed):
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(-0.02, 0.02, n), rng.uniform(-0.92, -0.88, n)], axis=1)
    xy[::3] = xy[(np.arange(0, n, 3) // 7) * 2 + 1]          # exact duplicates of other samples: equal-cost parents off the goal path
    return xy


def test_exact_duplicates_lowest_id_wins(eng_mod):
    """Injected exact duplicates in three rows of eight, K = 512, a dense cluster: equal candidates for one node from different new
    ids -- the lowest must win whichever lane gets there first -- and the kd structure built after the steps."""
    n = 4000
    case = cases.cfg2(n - n // 100 - 5)
    sets = [_dup_samples(n, 20 + j) if j % 3 == 0 else None for j in range(8)]
    cs = [cases.Case(case, seed=50 + j) for j in range(8)]
    runs = []
    for form in FORMS:
        engs = [_engine(eng_mod, c, form) for c in cs]
        for j, e in enumerate(engs):
            if sets[j] is not None:
                e.set_samples(sets[j])
        eng_mod.Engine.grow_batch(engs, [case.start] * 8, case.max_step, case.search_radius, case.n_iter_min, 512)
        assert engs[0].get_option("kd_lazy") == 1 and engs[0].get_option("kd_built_after") == 1
        assert engs[0].get_option("n_heavy") > 0
        for j, (e, c) in enumerate(zip(engs, cs)):
            assert_same(e, _oracle(("dup", j), c, 512, sets[j]))
        runs.append(engs)
    _forms_agree(runs)


@pytest.mark.parametrize("rows", [20, 96])
def test_rows_with_loop_conditions_of_their_own(eng_mod, rows):
    """Rows at K = 128 with n_iter_min spread over 300 .. 900 and n_iter_max above it: rows end early and spans lie beyond a row's own
    end of the step (row_nb).  96 rows (rows are gathered from 64 on) also launch later steps, and with them the commit of the step
    before, on compacted rows: the leader's count of compactions says that it happened.  Every row against a single grow."""
    cs0 = cases.tamp_queries(rows)
    mn = [300 + (600 * j) // (rows - 1) for j in range(rows)]
    mx = [a + 100 + 37 * (j % 5) for j, a in enumerate(mn)]
    cs = [cases.Case(c, n_iter_min=a, n_iter_max=b) for c, a, b in zip(cs0, mn, mx)]
    single = [run_gpu(eng_mod, c, 128)[0] for c in cs]
    runs = []
    for form in FORMS:
        engs = [_engine(eng_mod, c, form, batch_streams=1) for c in cs]
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, mn, 128, n_iter_max=mx)
        assert engs[0].get_option("group_lanes") == 16
        its = [e.num_iterations() for e in engs]
        assert len(set(its)) > 1 and min(its) >= 300 and max(its) <= max(mx)
        print("rows", rows, "form", form, "compactions", engs[0].get_option("compactions"), "steps", -(-max(its) // 128))
        if rows >= 64:
            assert engs[0].get_option("compactions") > 0, "no step was launched on compacted rows"
        for e, s in zip(engs, single):
            assert_same(e, s)
        runs.append(engs)
    _forms_agree(runs)


def test_list_capacity_overflow_replays(eng_mod):
    """cand_cap = 64 on the heavy case: the first attempt overflows its lists and the call replays with larger ones; the clamped counts
    must not read past a slice, and the result equals the oracle."""
    cs = _heavy_cases(8)
    runs = []
    for form in FORMS:
        engs = [_engine(eng_mod, c, form, cand_cap=64) for c in cs]
        assert engs[0].get_option("cand_cap") == 64
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, HEAVY_N, 1024)
        assert all(e.get_option("cand_cap") > 64 for e in engs), "the lists did not overflow: nothing was replayed"
        for j, (e, c) in enumerate(zip(engs, cs)):
            assert_same(e, _oracle(("heavy", j), c, 1024))
        runs.append(engs)
    _forms_agree(runs)


def test_two_sequences_side_by_side(eng_mod):
    """10 rows as two launch sequences (batch_streams = 2), rows 0, 4, 5 and 9 against the oracle"""
    n_iter = 6 * 1024 + 1
    cs = [cases.cfg2(n_iter, seed=90 + j) for j in range(10)]
    runs = []
    for form in FORMS:
        engs = [_engine(eng_mod, c, form, batch_streams=2) for c in cs]
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, n_iter, 1024)
        for j in (0, 4, 5, 9):
            assert_same(engs[j], _oracle(("two", j), cs[j], 1024))
        runs.append(engs)
    _forms_agree(runs)


def test_goal_reached_early(eng_mod):
    """A goal close to the start is hit within the first steps; from then on every 100th iteration re-adds the goal point, so a step of
    512 holds several copies of it, served together by their leader, whose uncompacted list -- with its negative entries -- goes through
    the commit.  The oracle's tree says that it happened: more than twice as many nodes exactly on the goal point as the run has steps,
    so some step holds at least three."""
    n_iter = 6 * 512 + 7
    steps = 7
    cs = []
    for j in range(8):
        c = cases.cfg2(n_iter, seed=30 + j)
        c.update(goals=[(0.15, -0.85)])
        cs.append(c)
    runs = []
    for form in FORMS:
        engs = [_engine(eng_mod, c, form) for c in cs]
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, n_iter, 512)
        for j, (e, c) in enumerate(zip(engs, cs)):
            o = _oracle(("goal", j), c, 512)
            xy = o.tree()[0]
            copies = int(np.sum((xy[:, 0] == c.goals[0][0]) & (xy[:, 1] == c.goals[0][1])))
            assert copies > 2 * steps, "the goal was meant to be reached in the first steps: %d copies of the goal point" % copies
            assert_same(e, o)
        runs.append(engs)
    _forms_agree(runs)
