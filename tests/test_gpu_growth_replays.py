"""The growth's replays and what a failed growth leaves, on the device.

porrt_grow runs a growth again when the device reports that a pool was too small or that the device sampler's stream left the
reference's ("Replays and what a failed growth leaves"):

  -100  a neighbour list overflowed        cand_cap * 4               (test_gpu_parity.py, test_gpu_nn2_forms.py)
  -101  a float draw would have been redrawn  the exact host stream   here: the far boxes of growth_replay_inputs.py
  -102  the PTO edge pool overflowed       edge_per_node * 4          here: option edge_per_node = 1
  -103  the deferred-tie pool overflowed   the pool in ids * 4        here: option tie_pool_ids = 1 on the lattice stream

A member of a porrt_grow_batch is never replayed for the last three: the call fails, and every context of it is left as the call found
it, without results.  Every comparison is bit for bit against the oracle (assert_same); nothing has a tolerance.  Each test asserts
that the path it was built for ran -- an option that grew, or the redraw pinned by tests/test_growth_replay_inputs_cpu.py -- and
prints the number of attempts.  No test reads anything of a failed run: the refusals are the getters' own."""
import numpy as np
import pytest

import cases
import exact_inputs as X
import growth_replay_inputs as R
from oracle import orc
from test_gpu_parity import assert_same, run_orc

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_CAPACITY = -1, -5


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


_ORC = {}


def oracle(key, case, K, grows=1, samples=None):
    """(the oracle grown `grows` times on the case, the last return code): made once per module, read only"""
    key = (key, K, grows)
    if key not in _ORC:
        o = cases.configure(orc.Oracle(), case)
        if samples is not None:
            o.set_samples(samples)
        for _ in range(grows):
            rc = cases.grow(o, case, K=K, algo=orc.ALGO_BATCHED_KD)
        _ORC[key] = (o, rc)
    return _ORC[key]


def engine(eng_mod, case, samples=None, **opts):
    e = cases.configure(eng_mod.Engine(), case)
    for k, v in opts.items():
        e.set_option(k, v)
    if samples is not None:
        e.set_samples(samples)
    return e


def assert_no_results(eng_mod, e):
    """as a context that never grew (test_gpu_parity.py::test_errors)"""
    with pytest.raises(eng_mod.PorrtError):
        e.tree()
    assert e.num_nodes() == 0 and e.num_iterations() == 0 and e._l.porrt_num_edges(e._c) == 0 and e._l.porrt_num_final(e._c) == 0
    assert all(len(a) == 0 for a in e.edges())
    assert e.best_solution() is None
    assert not e.is_final_set_complete()


def log4(v):
    k = 0
    while 4 ** k < v:
        k += 1
    assert 4 ** k == v, "%d is no power of 4" % v
    return k


def test_seam_option_values(eng_mod):
    e = eng_mod.Engine()
    assert e.get_option("edge_per_node") == 256 and e.get_option("tie_pool_ids") == 0
    assert e.get_option("tie_pooled_ids") == 0 and e.get_option("tie_records") == 0
    for name, good, bad in (("edge_per_node", (1, 65536, 256), (0, -1, 65537)), ("tie_pool_ids", (1, 1 << 30, 0), (-1, (1 << 30) + 1))):
        for v in good:
            e.set_option(name, v)
            assert e.get_option(name) == v
        for v in bad:
            with pytest.raises(eng_mod.PorrtError):
                e.set_option(name, v)
            assert e.get_option(name) == good[-1]
    for name in ("tie_pooled_ids", "tie_records"):                # views, not options
        with pytest.raises(eng_mod.PorrtError):
            e.set_option(name, 1)


# ---------------------------------------------------------------------------------------------------------------- edge pool (-102)
def check_edge_replays(eng_mod, name, case, K, min_replays):
    o, rco = oracle(name, case, K)
    n_edges = len(o.edges()[0])
    replays, per_node = R.edge_replays(n_edges, case.n_iter_max)
    assert n_edges > R.edge_pool(case.n_iter_max, 1)[1], "the first pool holds the oracle's graph: no replay"
    assert replays >= min_replays
    e = engine(eng_mod, case, edge_per_node=1)
    assert e.get_option("edge_per_node") == 1
    rce = cases.grow(e, case, K=K)
    print("%s K %d: %d edges, pools of %s slots, %d attempts, edge_per_node %d" % (name, K, n_edges,
          [R.edge_pool(case.n_iter_max, 4 ** k)[1] for k in range(replays + 1)], replays + 1, e.get_option("edge_per_node")))
    assert e.get_option("edge_per_node") == per_node
    assert rce == rco
    assert_same(e, o, pto=True)
    return e


def test_edge_pool_replays(eng_mod):
    """cfg3(1500, 1500): 68952 edges against pools of 6297, 11367 and 31644 slots (5598, 10104, 28128 asked, an eighth on top): three
    replays, the fourth attempt with 64 slots per node.  Then the same engine again against the oracle grown twice: both sampler
    streams (states, worlds) were put back before every replay."""
    case = R.pto_1500()
    e = check_edge_replays(eng_mod, "pto_1500", case, 256, 3)
    assert e.get_option("edge_per_node") == 64
    o2, rc2 = oracle("pto_1500", case, 256, grows=2)
    assert cases.grow(e, case, K=256) == rc2
    assert_same(e, o2, pto=True)


def test_edge_pool_overflow_in_the_steps_launched_one_by_one(eng_mod):
    """cfg3(40, 9000) at K = 100: one step of 40 iterations (at most 40 * 41 / 2 edges), everything else in the tail loop, where the
    overflow falls; then a second grow on the same engine"""
    case = R.pto_tail()
    assert 40 * 41 // 2 < R.edge_pool(case.n_iter_max, 1)[0]
    e = check_edge_replays(eng_mod, "pto_tail", case, 100, 1)
    assert e.num_iterations() > case.n_iter_min
    o2, rc2 = oracle("pto_tail", case, 100, grows=2)
    assert cases.grow(e, case, K=100) == rc2
    assert_same(e, o2, pto=True)


def test_edge_pool_replays_on_a_door_map(eng_mod):
    check_edge_replays(eng_mod, "door_1500", R.door_1500(), 256, 3)


# ---------------------------------------------------------------------------------------------------------------- tie pool (-103)
def lattice_inputs(seed=X.SINGLE_SEED, grows=1):
    """the lattice stream of test_gpu_exact_ties.py; lattice() cycles, so the stream for two grows starts with the stream for one"""
    return X.rrt_lattice_case(), X.lattice(1 / 16, seed, grows * X.RRT_ITERS)


@pytest.mark.parametrize("K", [64, 256])
def test_tie_pool_replays(eng_mod, K):
    case, xy = lattice_inputs(grows=2)
    o, _ = oracle("lattice2", case, K, samples=xy)
    # with the default pool: the stream defers ties between different places (kd_lazy: they wait for the structure built after the steps)
    e0 = engine(eng_mod, case, samples=xy)
    cases.grow(e0, case, K=K)
    pooled, records = e0.get_option("tie_pooled_ids"), e0.get_option("tie_records")
    print("lattice K %d, default pool: %d deferred-tie records over %d pooled ids" % (K, records, pooled))
    assert e0.get_option("tie_pool_ids") == 0 and e0.get_option("kd_lazy") == 1 and e0.get_option("kd_built_after") == 1
    assert pooled >= 2 and records >= 1
    assert_same(e0, o)
    # a pool of one id
    e = engine(eng_mod, case, samples=xy, tie_pool_ids=1)
    assert e.get_option("tie_pool_ids") == 1
    cases.grow(e, case, K=K)
    cap, used = e.get_option("tie_pool_ids"), e.get_option("tie_pooled_ids")
    print("lattice K %d, pool of 1 id: %d attempts, the last with %d ids for %d pooled" % (K, log4(cap) + 1, cap, used))
    assert cap > 1 and 2 <= used <= cap
    assert_same(e, o)                                            # n_tie_fallbacks == 0 is part of it
    # the same engine again: the injected stream stands where one grow leaves it
    o2, _ = oracle("lattice2", case, K, grows=2, samples=xy)
    cases.grow(e, case, K=K)
    assert_same(e, o2)


# ---------------------------------------------------------------------------------------------------------------- redraw (-101)
def box(case):
    return case.low, case.up


def sampler_calls(n_iter):
    return n_iter - n_iter // 100


def test_far_box_without_a_redraw(eng_mod):
    """x in [2^36, 2^36 + 2): an f32 of such a coordinate is worth nothing (its ulp is 4096).  Seed 0 draws 3960 times without a redraw,
    so this is the search kernels on the far box and nothing else: results do not depend on the box."""
    case = R.far_rrt(0)
    assert R.redraw_calls(*box(case), 0, sampler_calls(R.N_FAR)) == []
    o, _ = oracle("far_rrt0", case, 256)
    e = engine(eng_mod, case)
    cases.grow(e, case, K=256)
    assert o.num_nodes() > 3000 and len(o.final_ids()) > 0
    assert_same(e, o)


def test_redraw_in_the_samples_made_up_front(eng_mod):
    """seed 8 redraws once, in call 3458 (iteration 3493 of 4000): k_gen_samples flags it, the growth runs again on the host's stream.
    Three grows on one engine: the stream goes on from the host's state, not from 2 * calls steps past the old one."""
    case = R.far_rrt(8)
    calls = R.redraw_calls(*box(case), 8, sampler_calls(R.N_FAR))
    assert calls == [3458] and R.iteration_of_call(3458) == 3493
    print("far box seed 8: redraw in call %s: 2 attempts" % calls)
    e = engine(eng_mod, case)
    for grows in (1, 2, 3):
        o, _ = oracle("far_rrt8", case, 256, grows=grows)
        cases.grow(e, case, K=256)
        assert_same(e, o)


def test_redraw_in_the_steps_launched_one_by_one(eng_mod):
    """2^38, seed 44: the redraw of call 148 is iteration 150, past n_iter_min = 100, in a growth that goes on to iteration 676"""
    case = R.far_tail()
    calls = R.redraw_calls(*box(case), 44, 400)
    assert calls == [148] and R.iteration_of_call(148) == 150 > case.n_iter_min
    o, _ = oracle("far_tail", case, 64)
    assert 150 < o.num_iterations() < case.n_iter_max
    print("far box 2^38 seed 44: redraw in iteration 150 of %d: 2 attempts" % o.num_iterations())
    e = engine(eng_mod, case)
    cases.grow(e, case, K=64)
    assert_same(e, o)


def test_redraw_in_a_belief_space_growth(eng_mod):
    """cfg3 on the far box, seed 8: the replay draws the worlds again from the stream as it was"""
    case = R.far_pto(8)
    assert R.redraw_calls(*box(case), 8, sampler_calls(R.N_FAR)) == [3458]
    o, rco = oracle("far_pto8", case, 256)
    e = engine(eng_mod, case)
    assert cases.grow(e, case, K=256) == rco
    assert_same(e, o, pto=True)
    o2, rc2 = oracle("far_pto8", case, 256, grows=2)
    assert cases.grow(e, case, K=256) == rc2
    assert_same(e, o2, pto=True)


def test_injected_stream_one_sample_short(eng_mod):
    """not a replay: the error names the stream, the context has no results, and grows as usual once the stream is long enough"""
    case = cases.cfg1(2000)
    s = cases.configure(orc.Oracle(), case)
    xy = np.array([s.sample() for _ in range(sampler_calls(2000))])
    e = engine(eng_mod, case, samples=xy[:-1])
    with pytest.raises(eng_mod.PorrtError, match="injected sample stream exhausted") as ei:
        cases.grow(e, case, K=256)
    assert ei.value.code == ERR_INVALID
    assert_no_results(eng_mod, e)
    e.set_samples(xy)
    cases.grow(e, case, K=256)
    assert_same(e, oracle("cfg1_2000", case, 256)[0])
    # belief space: the failed call had drawn its 1500 worlds; they are drawn again, as by a fresh context
    case = R.pto_1500()
    s = cases.configure(orc.Oracle(), case)
    xy = np.array([s.sample() for _ in range(sampler_calls(1500))])
    e = engine(eng_mod, case, samples=xy[:-1])
    with pytest.raises(eng_mod.PorrtError, match="injected sample stream exhausted"):
        cases.grow(e, case, K=256)
    assert_no_results(eng_mod, e)
    e.set_samples(xy)
    o, rco = oracle("pto_1500", case, 256)
    assert cases.grow(e, case, K=256) == rco
    assert_same(e, o, pto=True)


# ---------------------------------------------------------------------------------------------------------------- members of a batch
def test_batch_member_edge_overflow_rolls_every_context_back(eng_mod):
    cs = [R.pto_1500(seed) for seed in (0, 1, 2)]
    engs = [engine(eng_mod, c) for c in cs]
    engs[1].set_option("edge_per_node", 1)
    with pytest.raises(eng_mod.PorrtError, match="edge pool overflow") as ei:
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, 1500, 256, mode=cases.PTO)
    assert ei.value.code == ERR_CAPACITY
    assert engs[1].get_option("edge_per_node") == 1             # a member is not replayed
    for e in engs:
        assert_no_results(eng_mod, e)
    # each on its own, as a fresh context would: the world streams (drawn from before the steps) were put back
    for j, (e, c) in enumerate(zip(engs, cs)):
        o, rco = oracle("pto_1500_s%d" % j, c, 256)
        assert cases.grow(e, c, K=256) == rco
        assert_same(e, o, pto=True)
    print("member 1 alone: %d attempts" % (log4(engs[1].get_option("edge_per_node")) + 1))
    assert [e.get_option("edge_per_node") for e in engs] == [256, 64, 256]


def test_batch_member_redraw_rolls_every_context_back(eng_mod):
    seeds = (0, 8, 0)
    cs = [R.far_rrt(s) for s in seeds]
    engs = [engine(eng_mod, c) for c in cs]
    with pytest.raises(eng_mod.PorrtError, match="grow this context on its own") as ei:
        eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, R.N_FAR, 256)
    assert ei.value.code == ERR_INVALID
    for e in engs:
        assert_no_results(eng_mod, e)
    for e, c, s in zip(engs, cs, seeds):
        cases.grow(e, c, K=256)
        assert_same(e, oracle("far_rrt%d" % s, c, 256)[0])


def test_batch_member_tie_overflow_rolls_every_context_back(eng_mod):
    """eight lattice rows through the group kernels, row 3 with a pool of one id: a capacity error and no results anywhere; with the
    default pool the same engines, their injected streams where they were, equal the oracles"""
    case = X.rrt_lattice_case()
    streams = [lattice_inputs(s)[1] for s in X.RRT_SEEDS]
    engs = [engine(eng_mod, case, samples=xy) for xy in streams]
    engs[3].set_option("tie_pool_ids", 1)
    with pytest.raises(eng_mod.PorrtError, match="deferred-tie pool") as ei:
        eng_mod.Engine.grow_batch(engs, [case.start] * 8, case.max_step, case.search_radius, X.RRT_ITERS, 256)
    assert ei.value.code == ERR_CAPACITY
    assert engs[3].get_option("tie_pool_ids") == 1
    for e in engs:
        assert_no_results(eng_mod, e)
    engs[3].set_option("tie_pool_ids", 0)
    eng_mod.Engine.grow_batch(engs, [case.start] * 8, case.max_step, case.search_radius, X.RRT_ITERS, 256)
    assert engs[0].get_option("group_lanes") == 16
    assert engs[3].get_option("tie_pooled_ids") >= 2, "row 3 never asked the pool for more than the one id it had"
    for s, e, xy in zip(X.RRT_SEEDS, engs, streams):
        assert_same(e, oracle("lattice_s%d" % s, case, 256, samples=xy)[0])
