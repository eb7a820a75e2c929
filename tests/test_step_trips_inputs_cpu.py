"""The inputs of tests/test_gpu_step_trips.py produce what they are there for: asserted from the oracle alone (no GPU), so that an input
that stops producing its condition fails here instead of passing there."""
import numpy as np
import pytest

import step_trips_inputs as sti
from oracle import orc


def _copies(x, p):
    return int(np.count_nonzero((x[:, 0] == p[0]) & (x[:, 1] == p[1])))


def _steered_share(bt, j, o):
    """share of the row's new nodes that do not lie where a sample of its stream (or the goal point) lies: their sample was steered"""
    x = o.tree()[0]
    s = np.ascontiguousarray(np.vstack([bt.samples[j], np.array(bt.cases[j].goals, dtype=np.float64)]))
    keys = set(map(tuple, s.view(np.uint64).reshape(-1, 2).tolist()))
    mine = np.ascontiguousarray(x[1:]).view(np.uint64).reshape(-1, 2).tolist()
    return 1.0 - sum(tuple(v) in keys for v in mine) / max(1, len(mine))


@pytest.mark.parametrize("K,words", [(64, 1), (1024, 16), (2048, 32)])
@pytest.mark.parametrize("rows", [8, 3])
def test_mask_words(K, words, rows):
    bt, orcs = sti.oracles("words%dx%d" % (K, rows))
    assert bt.K // 64 == words and len(orcs) == rows
    steps = (bt.n_iter + K - 1) // K
    assert steps >= 3 and (K != 64 or steps == 10), "K = 64 runs the first ten steps of a run"
    if K == 2048:
        assert bt.n_iter % K != 0, "the last step is a short one"
    for o in orcs:
        assert o.num_nodes() > bt.n_iter // 4                 # (new nodes in every word of the later steps' masks)


def test_border_pixels_and_high0():
    for name in ("border", "border3", "short_steps", "long_steps"):
        bt, orcs = sti.oracles(name)
        occ = bt.cases[0].occ
        assert (occ == 0).any() and (occ == 60).any() and (occ == 200).any()
        assert bt.n_iter == 10 * bt.K, "ten steps from a tree of one node"
        for j, s in enumerate(bt.samples):
            i, jj = sti.pixel(s)
            assert i.min() == 0 and i.max() == sti.W - 1 and jj.min() == 0 and jj.max() == sti.W - 1, "row %d: a rim of the raster without a sample" % j
            assert i.min() >= 0 and jj.max() < sti.W, "a sample outside the raster"
            for ci, cj in ((0, 0), (0, sti.W - 1), (sti.W - 1, 0), (sti.W - 1, sti.W - 1)):
                assert ((i == ci) & (jj == cj)).any(), "row %d: no sample in corner pixel (%d, %d)" % (j, ci, cj)
            on_high0 = int(np.count_nonzero(occ[i, jj] == 0))
            assert on_high0 >= 10, "row %d: %d samples on CLS_HIGH0 pixels" % (j, on_high0)
            # the oracle's own transform agrees with the one used here
            o = orcs[j]
            for t in (0, 16, 32, 48):
                assert tuple(o.to_pixel(s[t])) == (i[t], jj[t])


def test_outside_row_panics_in_the_oracle():
    bt = sti.outside()
    i, j = sti.pixel(bt.samples[1][70])
    assert j[0] >= sti.W, "the sample's pixel exists"
    assert np.abs(bt.samples[1][70] - np.array(bt.cases[1].start)).sum() < bt.max_step, "the sample would be steered"
    with pytest.raises(RuntimeError, match="raster"):
        sti.oracle_row(bt, 1)
    for r in (0, 2):
        assert sti.oracle_row(bt, r).num_nodes() > 1


def test_no_raster_rows_grow():
    bt, orcs = sti.oracles("no_raster")
    assert all(c.grid is None and c.get("occ") is None for c in bt.cases)
    assert all(o.num_nodes() > 1000 for o in orcs)


def test_step_lengths():
    """0.02: most new nodes are steered states, in every row; 0.5: the discs of the radius search meet more than N / 16 regions for more
    steps than at the default step of 0.1, and for fewer than all: the hand-over to the pages happens inside the run"""
    bt, orcs = sti.oracles("short_steps")
    for j, o in enumerate(orcs):
        share = _steered_share(bt, j, o)
        print("short_steps row", j, "steered share %.2f" % share)
        assert share > 0.5

    def streaming_steps(name):
        bt, orcs = sti.oracles(name)
        at = sti.sizes(bt, 0, bt.n_iter // bt.K)
        c = bt.cases[0]
        rad = [orc.lib().orc_heuristic_radius(n0, bt.max_step, bt.search_radius, 2) for n0 in at[:-1]]
        # a disc inside the map meets at least floor(2 rho * 20)^2 regions of side 0.05
        return sum(16 * int(np.floor(2.0 * r * 20.0)) ** 2 > n0 for r, n0 in zip(rad, at[:-1])), len(rad), c
    long_n, steps, _ = streaming_steps("long_steps")
    base_n, _, _ = streaming_steps("border")
    print("streaming steps: max_step 0.5:", long_n, "0.1:", base_n, "of", steps)
    assert base_n < long_n < steps


def test_own_plans_one_row_ends_early():
    bt, orcs = sti.oracles("own_plans")
    its = [o.num_iterations() for o in orcs]
    print("iterations", its)
    assert its[0] == 300 and len(orcs[0].final_ids()) > 0, "row 0 does not end at its n_iter_min with its goal reached"
    assert all(i >= 600 for i in its[1:]), "the other rows do not go on"
    assert -(-its[0] // bt.K) < min(-(-i // bt.K) for i in its[1:]), "row 0 does not end steps before the others"


def test_goal_reached_leaves_copies():
    bt, orcs = sti.oracles("goal_reached")
    for j, o in enumerate(orcs):
        n = _copies(o.tree()[0], bt.cases[j].goals[0])
        assert len(o.final_ids()) > 0 and n >= 3, "row %d: %d copies of the goal point" % (j, n)
