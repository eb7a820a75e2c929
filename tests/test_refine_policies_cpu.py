"""CPU checks of the batch refiner (porrt_bg_refine_policies / porrt_mm_refine_policies / porrt_refine_policies): the library
exports the entry points that the header and INTEGRATION.md declare, engine.py binds them with as many arguments as the header
gives them, and the restatement the GPU tests compare with -- tests/refine_ref.py applied policy by policy -- sees in the hand-built
batch policies (tests/refine_policies_cases.py) the shapes they were built for.  No GPU."""
import os
import re

import numpy as np

import refine_policies_cases as rp
import refine_ref
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("porrt_bg_refine_policies", "porrt_mm_refine_policies", "porrt_refine_policies", "porrt_refine_policies_info")


def test_batch_refine_symbols_exported_declared_and_bound():
    from po_rrt_amd import build, engine
    build.build()
    L = engine.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "porrt_hip.h")).read(), flags=re.S)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rust = integ[integ.index("```rust"):]
    rust = rust[:rust.index("```", 7)]
    for s in NEW:
        assert hasattr(L, s), "libporrt_hip.so does not export %s" % s
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, hdr)
        assert m, "%s is not declared in porrt_hip.h" % s
        assert len(getattr(L, s).argtypes) == len(m.group(1).split(",")), "%s: engine.py binds another number of arguments" % s
        assert "pub fn %s(" % s in rust, "%s is not in INTEGRATION.md's Rust block" % s
        assert s in engine.SYMBOLS
    assert re.search(r"struct\s+porrt_refine_policies_info\s*\{", hdr)
    assert [f for f, _ in engine.RefinePoliciesInfo._fields_] == ["policies", "ok", "pieces", "shortcut_pieces", "nodes", "distinct_lengths",
                                                                  "ms_device", "ms_wall"]
    off = np.zeros(1, dtype=np.uint64)
    st, cost = np.zeros(1, dtype=np.uint8), np.zeros(1)
    assert L.porrt_bg_refine_policies(None, 10, off, st, cost, None, None, None, None, 0) < 0
    assert L.porrt_mm_refine_policies(None, 10, off, st, cost, None, None, None, None, 0) < 0
    assert L.porrt_refine_policies_info(None, None) < 0
    for name in ("refine_policies", "mm_refine_policies", "refine_policies_explicit", "refine_policies_info"):
        assert callable(getattr(engine.Engine, name))


def oracle_on(occ):
    o = orc.Oracle()
    o.set_grid(occ, (-1.0, -1.0), (1.0, 1.0), orc.DOMAIN_SHELF)
    return o


def test_comb_has_more_pieces_than_a_wave_has_lanes():
    xy, par, oid, row = rp.comb(70)
    pieces, skeleton = refine_ref.decompose(par)
    assert len(pieces) == 70 + 71 and all(len(p) == 1 for p in pieces)
    (x, oid_r, p_r, leaf), cost = rp.restate(oracle_on(rp.wall_raster()), (xy, par, oid, row), [[1.0]], 20)
    # every branching piece has one node: the quirk leaves every piece unconnected, the cost from the root is 0
    assert (p_r >= 0).sum() == 0 and leaf.all() and cost == 0.0 and np.array_equal(x, xy[(oid_r - 7).astype(np.int64)])


def test_bushy_pieces_come_breadth_first_and_all_get_shortcut():
    pol = rp.bushy()
    pieces, skeleton = refine_ref.decompose(pol[1])
    assert pieces == [[0, 1, 2, 3], [4, 7, 10, 13], [5, 8, 11, 14, 16], [6, 9, 12, 15], [17, 19, 21], [18, 20, 22, 23, 24, 25]]
    assert skeleton == [[1, 2, 3], [], [4, 5], [], [], []]
    o = oracle_on(rp.wall_raster())
    (x0, oid0, par0, leaf0), c0 = rp.restate(o, pol, [[1.0]], 0)
    (x1, oid1, par1, leaf1), c1 = rp.restate(o, pol, [[1.0]], 200)
    assert list(oid0 - 7) == [k for p in pieces for k in p] and np.array_equal(oid0, oid1) and np.array_equal(par0, par1)
    assert list(par0) == [-1, 0, 1, 2, 3, 4, 5, 6, 3, 8, 9, 10, 11, 3, 13, 14, 15, 12, 17, 18, 12, 20, 21, 22, 23, 24]
    assert c1 < c0 and not np.array_equal(x0, x1)


def test_info_restatement_counts_the_hand_built_batch():
    pols = [rp.small_pieces(), rp.root_branches_at_once(), rp.policy([(0.0, 0.0)], [-1]), rp.policy(np.zeros((0, 2)), []), rp.zigzag(100)]
    want = rp.info_of(pols, [0, 0, 0, 1, 0])
    assert want == dict(policies=5, ok=4, pieces=6 + 3 + 1 + 1, shortcut_pieces=2 + 1 + 0 + 1, nodes=20 + 7 + 1 + 100, distinct_lengths=4)
