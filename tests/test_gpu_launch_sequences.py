"""State carried from one launch sequence into the next on the same contexts.

The other GPU tests grow a fresh context (or the same form twice) per launch form.  Here nine contexts go through a chain of
growths that alternates batches and single grows and changes the form from one to the next -- group kernels, one kernel per step,
the goal path on the side stream, the kd chain beside the steps and on the main stream, pipelined pairs, rows with plans of
their own, the persistent step loop -- so that whatever one sequence leaves behind (a pending rewire commit, a kd group counter,
an event still marked pending, rows switched to a compacted array) would show in the trees of the next.  (What the kd chain leaves
behind shows only where two parents tie bit for bit, which these inputs never make: tests/test_gpu_kd_forms.py runs SEQUENCE on
lattice streams, where they do.)
"""
import numpy as np
import pytest

import cases
from oracle import orc
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

N_CTX, N_ITER, K = 9, 3000, 256
DEFAULTS = dict(gtrack_side=0, kd_lazy=1, kd_inline=0, pipeline=4)
# (batch?, options on top of the defaults, (n_iter_min, n_iter_max), what get_option shows afterwards on context 0)
SEQUENCE = [
    (True, {}, (N_ITER, N_ITER), dict(group_lanes=16, kd_lazy=1)),
    (False, {}, (N_ITER, N_ITER), dict(pipeline=4, kd_lazy=1)),
    (False, dict(gtrack_side=1), (N_ITER, N_ITER), dict(pipeline=4, kd_lazy=1)),
    (True, dict(kd_lazy=0), (N_ITER, N_ITER), dict(group_lanes=16, kd_lazy=0)),
    (False, dict(pipeline=1), (N_ITER, N_ITER), dict(pipeline=1)),
    (True, {}, (1000, N_ITER), dict(group_lanes=16, kd_lazy=1)),
    (True, dict(kd_lazy=0, kd_inline=1), (N_ITER, N_ITER), dict(group_lanes=16, kd_lazy=0)),
    (False, dict(pipeline=2), (N_ITER, N_ITER), dict(pipeline=1)),        # (the persistent loop reads as the pipelined layout it runs on)
    (True, {}, (N_ITER, N_ITER), dict(group_lanes=16, kd_lazy=1)),
]


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def _contexts(eng_mod):
    cs = [cases.cfg2(N_ITER, seed=90 + s) for s in range(N_CTX)]
    return cs, [cases.configure(eng_mod.Engine(), c) for c in cs]


def _grow_batch(eng_mod, cs, engs, budget=(N_ITER, N_ITER)):
    return eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, budget[0], K, n_iter_max=budget[1])


def test_forms_in_sequence_on_the_same_contexts(eng_mod):
    """nine steps on the same Engine objects; after each, contexts 0 and 4 against oracle objects grown as often with the same budgets"""
    cs, engs = _contexts(eng_mod)
    orcs = {j: cases.configure(orc.Oracle(), cs[j]) for j in (0, 4)}
    for step, (batch, opts, budget, shown) in enumerate(SEQUENCE):
        for e in engs:
            for k, v in dict(DEFAULTS, **opts).items():
                e.set_option(k, v)
        grown = (0, 4) if batch else (0,)
        if batch:
            assert _grow_batch(eng_mod, cs, engs, budget) == 0
        else:
            assert cases.grow(engs[0], cs[0], K=K) == 0
        for j in grown:
            cases.grow(orcs[j], cases.Case(cs[j], n_iter_min=budget[0], n_iter_max=budget[1]), K=K, algo=orc.ALGO_BATCHED_KD)
        for j in (0, 4):
            assert engs[j].num_iterations() == orcs[j].num_iterations(), "step %d, context %d" % (step, j)
            assert_same(engs[j], orcs[j])
        for name, want in shown.items():
            assert engs[0].get_option(name) == want, "step %d: %s" % (step, name)


def test_profiled_batch_same_trees_and_leader_metrics(eng_mod):
    """profile = 1 (events around the two phases of every step, no hipGraph): the same trees; the leader's metrics carry the batch's totals"""
    cs, plain = _contexts(eng_mod)
    assert _grow_batch(eng_mod, cs, plain) == 0
    _, prof = _contexts(eng_mod)
    for e in prof:
        e.set_option("profile", 1)
    assert _grow_batch(eng_mod, cs, prof) == 0
    for a, b in zip(prof, plain):
        assert_same(a, b)
    m = prof[0].metrics()
    assert m["scan_launches"] == -(-N_ITER // K)
    assert m["scan_s"] > 0 and m["connect_s"] > 0 and m["scan_pairs"] > 0
