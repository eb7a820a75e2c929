"""GPU parity of the group kernels with their run constants read through the scalar cache (rc_const, porrt_device.hpp).

Only the path of wave-uniform loads changes, so every tree must equal the oracle's bit for bit: positions, parents, dist_root, final
nodes, without a tie falling back to the host.  The base case is the smallest batch that takes the group kernels (8 contexts) at
K = 128 with the goal next to the start, and n_iter just large enough -- four steps and a fifth of 5 samples -- that the oracle's tree of
every row (checked below, on the CPU) holds

  * a new node with more than 80 nodes within its search radius: its sample takes the heavy path (heavy_sample_wave, which takes the
    helper again at its entry) -- the engine's counter n_heavy says that it ran;
  * copies of the goal point (clone_workgroup; the engine keeps no counter of it beyond the running step, Counters::clone_n is reset by
    the workgroup itself: the copies in the tree are the evidence, they are created nowhere else);
  * at least three copies, so that one of them chose between earlier copies at equal cost: a tie settled from the goal path
    (g_track_step).  No counter says so directly; kd_built_after == 0 says that no tie of the run took the whole kd structure and
    n_tie_fallbacks == 0 (assert_same) that none went to the host, so the goal path settled it.

The same case runs with conn_wg_waves = 4 (k_conn2_wg4), commit_flat = 0 (commit_rrt_sample in k_nn2, k_commit2) and kd_lazy = 0 (the
kd kernels read the same rows beside the steps).  The compaction case is the one place where the DEVICE writes an array of run constants
that later kernels read through the helper (k_rows_gather)."""
import math

import numpy as np
import pytest

import cases
from oracle import orc
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

K = 128
N_ITER = 4 * K + 5
GOAL = (0.15, -0.85)
ROWS = 8


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def _case(j, n_iter=N_ITER):
    c = cases.cfg2(n_iter, seed=30 + j)
    c.update(goals=[GOAL])
    return c


def _grown_oracle(case, k=K):
    o = cases.configure(orc.Oracle(), case)
    cases.grow(o, case, K=k, algo=orc.ALGO_BATCHED_KD)
    return o


_ORC = {}


def _oracles():
    """the base case's oracle trees, grown once and left unchanged"""
    if not _ORC:
        for j in range(ROWS):
            _ORC[j] = _grown_oracle(_case(j))
    return _ORC


def _max_hits(j):
    """most nodes of the step's snapshot within the search radius of one of the step's new nodes, over the steps of row j (rrt.rs:121:
    the radius of the size before the step)"""
    c = _case(j)
    sizes = [1] + [_grown_oracle(_case(j, b * K)).num_nodes() for b in range(1, N_ITER // K + 1)] + [_oracles()[j].num_nodes()]
    xy = _oracles()[j].tree()[0]
    best = 0
    for n0, n1 in zip(sizes[:-1], sizes[1:]):
        r = min(c.search_radius * math.sqrt(math.log(n0) / n0), c.max_step) if n0 > 1 else c.max_step
        d = np.hypot(xy[n0:n1, None, 0] - xy[None, :n0, 0], xy[n0:n1, None, 1] - xy[None, :n0, 1])
        best = max(best, int((d <= r).sum(axis=1).max()))
    return best


def _copies(o):
    xy = o.tree()[0]
    return int(np.sum((xy[:, 0] == GOAL[0]) & (xy[:, 1] == GOAL[1])))


def test_base_case_holds_what_it_is_for():
    """the oracle's trees alone (no engine): every row has a heavy sample and at least three copies of the goal point"""
    for j in range(ROWS):
        hits, copies = _max_hits(j), _copies(_oracles()[j])
        print("row", j, "most hits", hits, "copies of the goal point", copies)
        assert hits > 80, "row %d: no new node with more than 80 nodes within its radius" % j
        assert copies >= 3, "row %d: %d copies of the goal point" % (j, copies)


@pytest.mark.parametrize("opts", [{}, {"conn_wg_waves": 4}, {"commit_flat": 0}, {"kd_lazy": 0}], ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()) or "defaults")
def test_base_case(eng_mod, opts):
    cs = [_case(j) for j in range(ROWS)]
    engs = [cases.configure(eng_mod.Engine(), c) for c in cs]
    for e in engs:
        for k, v in opts.items():
            e.set_option(k, v)
    eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, N_ITER, K)
    lead = engs[0]
    assert lead.get_option("group_lanes") == 16, "the group kernels did not run"
    for k, v in opts.items():
        assert lead.get_option(k) == v
    print("n_heavy", [e.get_option("n_heavy") for e in engs], "kd_built_after", lead.get_option("kd_built_after"))
    assert all(e.get_option("n_heavy") > 0 for e in engs), "the heavy path did not run"
    if lead.get_option("kd_lazy") == 1:
        assert lead.get_option("kd_built_after") == 0, "a tie took the whole kd structure, not the goal path"
    for j, e in enumerate(engs):
        assert_same(e, _oracles()[j])


def test_compacted_rows(eng_mod):
    """One launch sequence of 64 rows (rows are gathered from 64 on) at K = 128 with loop conditions of their own, n_iter_min spread over
    300 .. 900: rows end step by step, and once a quarter of them has ended the steps are launched on the array k_rows_gather wrote."""
    rows = 64
    cs0 = cases.tamp_queries(rows)
    mn = [300 + (600 * j) // (rows - 1) for j in range(rows)]
    mx = [a + 100 + 37 * (j % 5) for j, a in enumerate(mn)]
    cs = [cases.Case(c, n_iter_min=a, n_iter_max=b) for c, a, b in zip(cs0, mn, mx)]
    engs = [cases.configure(eng_mod.Engine(), c) for c in cs]
    for e in engs:
        e.set_option("batch_streams", 1)
    eng_mod.Engine.grow_batch(engs, [c.start for c in cs], cs[0].max_step, cs[0].search_radius, mn, K, n_iter_max=mx)
    assert engs[0].get_option("group_lanes") == 16
    its = [e.num_iterations() for e in engs]
    print("compactions", engs[0].get_option("compactions"), "iterations", min(its), "..", max(its))
    assert engs[0].get_option("compactions") > 0, "no step was launched on compacted rows"
    assert len(set(its)) > 1
    for e, c in zip(engs, cs):
        assert_same(e, _grown_oracle(c))
