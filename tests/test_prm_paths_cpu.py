"""CPU checks of the batched PRM queries (porrt_prm_plan_paths, porrt_prm_get_paths, porrt_prm_paths_info): a NULL context is a
negative code, not a crash (no device is touched), and the header cites the reference lines the batched call restates."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from po_rrt_amd import build, engine
    build.build()
    return engine.load_library()


def test_null_context_is_an_error(lib):
    from po_rrt_amd import engine
    z = np.zeros(4)
    off = np.zeros(3, dtype=np.uint64)
    assert lib.porrt_prm_plan_paths(None, z, z, 2, off, None, 0) < 0
    assert lib.porrt_prm_get_paths(None, None, 0) < 0
    info = engine.PrmPathsInfo()
    assert lib.porrt_prm_paths_info(None, C.byref(info)) < 0
    assert C.sizeof(engine.PrmPathsInfo) == 56


def test_header_cites_reference_lines():
    text = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    a = text.index("porrt_prm_plan_path(porrt_ctx")
    b = text.index("porrt_prm_paths_info(const porrt_ctx")
    block = text[a:b]
    assert "porrt_prm_plan_paths(" in block and "porrt_prm_get_paths(" in block
    for cite in ("prm.rs:111-123", "pto_graph.rs:305-326"):
        assert cite in block
