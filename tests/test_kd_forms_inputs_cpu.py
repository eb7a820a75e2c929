"""CPU side of tests/test_gpu_kd_forms.py, from the oracle alone: for every (stream, seed, K, n_iter) that file grows, the stream makes
the ties it is there for -- the kd structure that orders equal-cost parents only changes a tree when two candidate parents have
bit-equal cost -- and the oracle's kd-accelerated contract equals its brute-force definition there.

  lattice      nodes at different places share dist_root bit for bit
  chain        the kd-tree is at least half as deep as it has nodes (every group's new nodes bid for a few child slots), and there are
               more nodes than places (the ties are between copies at one place)
  duplicates   pairs of nodes at distance 0
"""
import numpy as np
import pytest

import cases
import exact_inputs as X
from oracle import orc
from test_exact_inputs_cpu import assert_same_tree

KEYS = X.kd_forms_keys()


def key_id(key):
    return "%s-seed%d-K%d-%d-%d" % key


def test_keys_cover_the_three_streams_and_the_group_sizes():
    assert len(KEYS) == len(set(KEYS)) and {k[0] for k in KEYS} == {"lattice", "chain", "duplicates"}
    for K, (g, n) in X.KDF_CLAIM.items():
        # two full kd groups and a short last one; a group within the claim kernel's 4096 nodes; the suite's limit of 9000 iterations
        assert g * K <= 4096 and n > 2 * g * K and n % (g * K) != 0 and n <= 9000
        assert {("lattice", s, K, n, n) for s in X.KDF_SEEDS} <= set(KEYS)
    K, seeds, n = X.KDF_LOCATE64
    assert 8 * K * len(seeds) < 4096                             # the one-wave-per-node locate kernel: fewer than 4096 nodes a group over all rows
    assert all(k[4] <= 9000 for k in KEYS)


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_stream_makes_ties_and_kd_equals_brute(oracle_lib, key):
    stream, seed, K, n_min, n_max = key
    case, xy = X.kd_forms_inputs(stream, seed, n_min, n_max)
    grown = []
    for algo in (orc.ALGO_BATCHED, orc.ALGO_BATCHED_KD):
        o = cases.configure(orc.Oracle(), case)
        o.set_samples(xy)
        cases.grow(o, case, K=K, algo=algo)
        grown.append(o)
    assert_same_tree(*grown)
    x, _, d = grown[1].tree()
    if stream == "lattice":
        shared = X.count_shared_dist_root(x, d)
        print("%s: %d nodes, %d sharing dist_root with another place" % (key_id(key), len(x), shared))
        assert shared > 0
    elif stream == "chain":
        depth, places = X.kd_depth(x), len(np.unique(x, axis=0))
        print("%s: %d nodes, %d places, kd depth %d" % (key_id(key), len(x), places, depth))
        assert 2 * depth >= len(x) and len(x) > places
    else:
        copies = X.count_pairs_at_distance(x, 0.0)
        print("%s: %d nodes, %d pairs at one place" % (key_id(key), len(x), copies))
        assert copies > 0
