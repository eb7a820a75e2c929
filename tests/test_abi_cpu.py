"""CPU checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol
include/porrt_hip.h declares.  No compute call is made (there is no GPU here and no CPU fallback)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from po_rrt_amd import build, engine
    build.build()
    return engine.load_library()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(porrt_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_are_exported(lib):
    from po_rrt_amd import engine
    syms = declared_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), "libporrt_hip.so does not export %s" % s
    assert sorted(engine.SYMBOLS) == syms


def test_header_cites_reference_lines():
    text = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    for cite in ("rrt.rs:102-174", "pto.rs:55-139", "common.rs:310-333", "sample_space.rs", "pto_c.rs:63-270"):
        assert cite in text


def test_no_cpu_fallback(lib):
    """Without a HIP device the product path must fail loudly, never compute on the CPU."""
    import torch
    from po_rrt_amd import Engine, PorrtError
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(PorrtError):
        Engine()


def test_product_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    pat = re.compile(r"from\s+oracle|import\s+oracle|liboracle|porrt_oracle\.h|\borc_[a-z]|oracle/")
    for dirpath, _, files in os.walk(os.path.join(ROOT, "po_rrt_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not pat.search(src), "%s references the oracle" % f
    hdr = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    assert not pat.search(hdr)


def test_null_context_is_an_error_not_a_crash(lib):
    """Every entry point of the widened rows rejects a NULL context with a negative code (no device is touched)."""
    import ctypes as C
    import numpy as np
    z = np.zeros(4)
    assert lib.porrt_build_belief_graph(None, z, 4) < 0
    assert lib.porrt_bg_compute_expected_costs(None) < 0
    assert lib.porrt_bg_extract_policy(None, None, None, None, 0, None) < 0
    assert lib.porrt_grow_prm(None, z, 0.1, 2.0, 10) < 0
    assert lib.porrt_prm_plan_path(None, z, z, None, 0) < 0
    assert lib.porrt_bg_get_expected_costs(None, z) < 0
    assert lib.porrt_bg_num_edges(None) == 0 and lib.porrt_bg_num_nodes(None) == 0 and lib.porrt_bg_num_beliefs(None) == 0
    d = C.c_double(0.0)
    assert lib.porrt_best_cost(None, C.byref(d), None) < 0
    # the explicit-graph entry validates its arrays before looking for a device
    one = np.array([0.0, 0.0])
    assert lib.porrt_conditional_dijkstra(0, 0, one, np.zeros(1, dtype=np.uint32), np.ones((1, 1)), 1, 1, np.ones(1, dtype=np.uint8),
                                          np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=np.uint32), np.zeros(2, dtype=np.uint64),
                                          np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 0, np.zeros(1)) < 0      # n = 0


def test_conditional_dijkstra_rejects_bad_arguments_before_the_device(lib):
    """porrt_conditional_dijkstra with n = 0 or a NULL array is PORRT_ERR_INVALID (-1): the answer of the argument check, which comes
    before any device call (a machine without a GPU would answer PORRT_ERR_DEVICE from there on)"""
    import ctypes as C
    import numpy as np
    raw = C.CDLL(lib._name).porrt_conditional_dijkstra            # the same symbol with plain pointers, so that NULL can be passed
    vp = C.c_void_p
    raw.restype = C.c_int
    raw.argtypes = [C.c_int, C.c_uint64, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_uint64, vp]
    arrays = [np.zeros(2), np.zeros(1, dtype=np.uint32), np.ones((1, 1)), np.ones(1, dtype=np.uint8), np.zeros(2, dtype=np.uint64),
              np.zeros(1, dtype=np.uint32), np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.zeros(1)]

    def call(n, null=None, n_final=0):
        xy, brow, bel, types, coff, cid, poff, pid, fin, dist = [None if k == null else a.ctypes.data for k, a in enumerate(arrays)]
        return raw(0, n, xy, brow, bel, 1, 1, types, coff, cid, poff, pid, fin, n_final, dist)
    assert call(0) == -1
    for null in (0, 1, 2, 3, 4, 6, 9):                             # xy, belief_row, beliefs, types, child_off, parent_off, dist
        assert call(1, null) == -1, null
    assert call(1, 8, n_final=1) == -1                               # finals announced but not given
    assert call(0xFFFFFFFF) == -1                                    # more nodes than a 32-bit id holds: refused before any array is read

    # a well-formed graph of three nodes (0 -> 1 -> 2, final 2), then one thing wrong at a time: every check of the arrays is made on the
    # host, so each answer is -1 here, where any call that got as far as the device would answer PORRT_ERR_DEVICE (-4)
    u32, u64 = np.uint32, np.uint64
    good = dict(n=3, xy=np.zeros(6), brow=np.array([0, 1, 0], dtype=u32), bel=np.array([[0.5, 0.5], [1.0, 0.0]]), rows=2, nw=2,
                types=np.ones(3, dtype=np.uint8), coff=np.array([0, 1, 2, 2], dtype=u64), cid=np.array([1, 2], dtype=u32),
                poff=np.array([0, 0, 1, 2], dtype=u64), pid=np.array([0, 1], dtype=u32), fin=np.array([2], dtype=u64), n_final=1, dist=np.zeros(3))

    def graph_call(**changes):
        a = dict(good, **changes)
        p = lambda x: None if x is None else x.ctypes.data
        return raw(0, a["n"], p(a["xy"]), p(a["brow"]), p(a["bel"]), a["rows"], a["nw"], p(a["types"]), p(a["coff"]), p(a["cid"]), p(a["poff"]),
                   p(a["pid"]), p(a["fin"]), a["n_final"], p(a["dist"]))
    import torch
    if not torch.cuda.is_available():
        assert graph_call() == -4                                    # the well-formed graph passes every check and stops at the missing device
    bad = {
        "child_off[0] != 0": dict(coff=np.array([1, 1, 2, 2], dtype=u64)),
        "parent_off[0] != 0": dict(poff=np.array([1, 1, 1, 2], dtype=u64)),
        "child_off decreases": dict(coff=np.array([0, 2, 1, 2], dtype=u64)),
        "parent_off decreases": dict(poff=np.array([0, 2, 1, 2], dtype=u64)),
        "child_off decreases at its end": dict(coff=np.array([0, 1, 2, 1], dtype=u64)),
        "child_ids NULL with entries announced": dict(cid=None),
        "parent_ids NULL with entries announced": dict(pid=None),
        "n_worlds == 0": dict(nw=0),
        "n_belief_rows == 0": dict(rows=0),
        "belief_row out of range": dict(brow=np.array([0, 2, 0], dtype=u32)),
        "child id out of range": dict(cid=np.array([1, 3], dtype=u32)),
        "parent id out of range": dict(pid=np.array([3, 1], dtype=u32)),
        "final out of range": dict(fin=np.array([3], dtype=u64)),
    }
    for what, change in bad.items():
        assert graph_call(**change) == -1, what
    # NULL id arrays are fine while the offsets announce nothing
    if not torch.cuda.is_available():
        assert graph_call(coff=np.zeros(4, dtype=u64), cid=None, poff=np.zeros(4, dtype=u64), pid=None) == -4
