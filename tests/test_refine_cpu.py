"""CPU checks of the policy refiner (PTOPolicyRefiner::refine_solution(PartialShortCut(n)), src/pto_policy_refiner.rs:87-124):
the library exports the three entry points the header and INTEGRATION.md declare, and the Python restatement (tests/refine_ref.py,
the yardstick of the GPU tests) keeps the reference's invariants on hand-built policies over a free raster and a raster with a wall."""
import os
import re

import numpy as np
import pytest

import refine_ref
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("porrt_bg_refine_policy", "porrt_refine_policy", "porrt_bg_get_refine_info")


def test_refine_symbols_exported_and_declared():
    from po_rrt_amd import build, engine
    build.build()
    L = engine.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "porrt_hip.h")).read(), flags=re.S)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rust = integ[integ.index("```rust"):]
    rust = rust[:rust.index("```", 7)]                         # the FFI block of section 1
    for s in NEW:
        assert hasattr(L, s), "libporrt_hip.so does not export %s" % s
        assert re.search(r"\b%s\s*\(" % s, hdr), "%s is not declared in porrt_hip.h" % s
        assert "pub fn %s(" % s in rust, "%s is not in INTEGRATION.md's Rust block" % s
        assert s in engine.SYMBOLS
    assert L.porrt_bg_refine_policy(None, 10, None, None, None, None, 0, None) < 0
    assert L.porrt_bg_get_refine_info(None, None, None) < 0


def oracle_on(occ):
    o = orc.Oracle()
    o.set_grid(occ, (-1.0, -1.0), (1.0, 1.0), orc.DOMAIN_SHELF)
    return o


def free_raster():
    return np.full((100, 100), 255, dtype=np.uint8)


def wall_raster():
    occ = free_raster()
    occ[:70, 49:51] = 0                     # a wall from the top edge down to y = -0.4, at x = 0
    return occ


# A policy with every kind of piece (children of a node in ascending id order):
#   piece 0: nodes 0..11, a zig-zag; node 11 branches into 12, 13, 15
#   piece 1: [12] one node, a leaf;  piece 2: [13, 14] two nodes;  piece 3: [15] one node that branches into 16 and 19
#   piece 4: [16, 17, 18] three nodes;  piece 5: [19] one node, a leaf
def zigzag_policy(path):
    xy = list(path) + [(0.6, 0.7), (0.7, 0.6), (0.75, 0.55), (0.7, 0.7), (0.72, 0.8), (0.74, 0.75), (0.76, 0.82), (0.65, 0.75)]
    par = list(range(-1, len(path) - 1)) + [11, 11, 13, 11, 15, 16, 17, 15]
    return np.array(xy, dtype=np.float64), np.array(par, dtype=np.int64)


FREE_PATH = [(-0.8, -0.8), (-0.6, -0.5), (-0.5, -0.75), (-0.3, -0.4), (-0.2, -0.7), (0.0, -0.3), (0.1, -0.6), (0.2, -0.1),
             (0.3, -0.4), (0.4, 0.2), (0.5, 0.1), (0.6, 0.6)]
WALL_PATH = [(-0.6, 0.6), (-0.5, 0.2), (-0.3, -0.2), (-0.25, -0.6), (-0.1, -0.75), (0.0, -0.8), (0.1, -0.75), (0.25, -0.6),
             (0.3, -0.2), (0.45, 0.1), (0.5, 0.4), (0.6, 0.6)]


@pytest.mark.parametrize("L", [3, 4, 5, 12, 65, 1500])
def test_draws_stay_in_range(L):
    d = refine_ref.draws(L, 1500)                              # the reference's asserts (:176-177) run inside
    assert {j for j, _, _ in d} == {0, 1}
    assert all(0 <= s < L - 2 and s + 2 <= e < L for _, s, e in d)
    assert d == refine_ref.draws(L, 1500)                      # a fresh seed-0 sampler per piece: the same sequence for one length


@pytest.mark.parametrize("raster,path", [(free_raster, FREE_PATH), (wall_raster, WALL_PATH)], ids=["free", "wall"])
def test_restatement_invariants(raster, path):
    o = oracle_on(raster())
    xy, par = zigzag_policy(path)
    n = len(par)
    oid = np.arange(100, 100 + n, dtype=np.uint64)
    row = np.zeros(n, dtype=np.uint32)
    beliefs = np.ones((1, 1))
    assert refine_ref.transitions_valid(o, xy, par, lambda k: 0, beliefs), "the hand-built policy itself must be valid"
    (x0, oid0, par0, leaf0), c0 = refine_ref.refine(o, xy, par, oid, row, beliefs, 0)
    stats = {}
    (x1, oid1, par1, leaf1), c1 = refine_ref.refine(o, xy, par, oid, row, beliefs, 500, stats)
    # recompose: pieces in order (0..11 | 12 | 13 14 | 15 | 16 17 18 | 19): the same order here, states untouched at n = 0
    assert np.array_equal(oid0, oid) and np.array_equal(oid1, oid)
    assert np.array_equal(x0, xy)
    # the one-node piece 15 branches: no skeleton edges from it -- 16 and 19 keep no parent, 15 becomes a leaf
    exp_par = par.copy()
    exp_par[16] = exp_par[19] = -1
    assert np.array_equal(par0, exp_par) and np.array_equal(par1, exp_par)
    assert leaf1[15] == 1 and leaf1[12] == 1 and leaf1[14] == 1 and leaf1[18] == 1 and leaf1[19] == 1 and leaf1.sum() == 5
    assert np.array_equal(leaf0, leaf1)
    # pieces of <= 2 nodes are untouched, piece ends never move
    for k in (12, 13, 14, 15, 19, 0, 11, 16, 18):
        assert tuple(x1[k]) == tuple(xy[k])
    assert stats.get("commits", 0) > 0 and not np.array_equal(x1, xy)
    # every committed transition is valid; the path got shorter
    assert refine_ref.transitions_valid(o, x1, par1, lambda k: 0, beliefs)
    length = lambda x: sum(refine_ref.norm2(x[k], x[k + 1]) for k in range(11))
    assert length(x1) < length(xy)
    assert c1 < c0 and c0 == refine_ref.expected_cost(xy, exp_par, [beliefs[0]] * n)
    if raster is wall_raster:
        assert stats.get("segment", 0) > 0                     # shortcuts through the wall were drawn and refused


def test_root_that_branches_at_once_leaves_everything_unconnected():
    """piece 0 = [0] alone: the quirk disconnects the whole policy below it, and the expected cost from the root is 0"""
    o = oracle_on(free_raster())
    xy = np.array([(0.0, 0.0), (0.1, 0.1), (0.2, 0.3), (0.3, 0.2), (-0.1, 0.1), (-0.2, 0.2)])
    par = np.array([-1, 0, 1, 2, 0, 4])
    (x, oid, p, leaf), cost = refine_ref.refine(o, xy, par, np.arange(6, dtype=np.uint64), np.zeros(6, dtype=np.uint32), np.ones((1, 1)), 100)
    assert list(p) == [-1, -1, 1, 2, -1, 4] and cost == 0.0
    assert list(leaf) == [1, 0, 0, 1, 0, 1]
