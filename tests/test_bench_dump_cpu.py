"""bench.py --dump-outputs on the host: what last_step_outputs takes from the fetched trees -- float64 arrays, under 64 MB in all,
the same sample for the same arguments, and the sampled trees as the caller's arrays held them."""
import numpy as np
import pytest

import bench
from po_rrt_amd.engine import BEST_ENTRY


class FakeEngine:
    def __init__(self, n):
        self.n = n

    def num_nodes(self):
        return self.n


def fetched(n_iter, Q, seed=5):
    cap = n_iter + 2
    rng = np.random.default_rng(seed)
    engs = [FakeEngine(int(rng.integers(1, cap + 1))) for _ in range(Q)]
    bufs = [(rng.random((cap, 2)), rng.integers(-1, cap, size=cap), rng.random(cap)) for _ in range(Q)]
    win = np.zeros(2, dtype=BEST_ENTRY)
    win["cost"], win["rank"], win["n_nodes"] = (1.5, np.inf), (0, -1), (engs[0].n, 0)
    return engs, bufs, win


@pytest.mark.parametrize("n_iter,Q", [(2000, 5), (111500, 64), (3_000_000, 3)])
def test_dump_is_float64_bounded_and_repeatable(n_iter, Q):
    engs, bufs, win = fetched(n_iter, Q)
    d = bench.last_step_outputs(engs, bufs, win, n_iter)
    assert all(a.dtype == np.float64 for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    assert np.array_equal(d["num_nodes"], [e.n for e in engs]) and np.array_equal(d["winner_cost"], win["cost"])
    again = bench.last_step_outputs(engs, bufs, win, n_iter)
    assert sorted(d) == sorted(again) and all(np.array_equal(d[k], again[k]) for k in d)
    off = d["tree_offsets"].astype(np.int64)
    for i, q in enumerate(d["tree_query"].astype(np.int64)):
        node = d["tree_node"][off[i]:off[i + 1]].astype(np.int64)
        assert len(node) == min(engs[q].n, off[i + 1] - off[i]) and np.all(np.diff(node) > 0) and node[-1] < engs[q].n
        assert np.array_equal(d["tree_xy"][off[i]:off[i + 1]], bufs[q][0][node])
        assert np.array_equal(d["tree_parent"][off[i]:off[i + 1]], bufs[q][1][node].astype(np.float64))
        assert np.array_equal(d["tree_dist_root"][off[i]:off[i + 1]], bufs[q][2][node])
    if n_iter < 100000:
        assert len(d["tree_query"]) == Q and off[-1] == sum(e.n for e in engs)      # small trees: all of them, whole
