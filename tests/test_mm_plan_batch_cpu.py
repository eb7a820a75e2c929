"""porrt_mm_plan_batch without a device: the recipe, the pass cuts and the id translation (csrc/porrt_mm_recipe.hpp) checked on the
host by tests/mm_recipe_check.cpp, a program of its own built with the address and undefined-behaviour sanitizers; the entry points'
declarations, bindings and answers to NULL arguments, which need no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["porrt_mm_plan_batch", "porrt_mm_plan_batch_get_policies", "porrt_mm_plan_batch_get_expected_costs", "porrt_mm_plan_batch_get_plan",
       "porrt_mm_plan_batch_info"]


def test_recipe_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "mm_recipe_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "mm_recipe_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mm_recipe_check ok" in out.stdout


@pytest.fixture(scope="module")
def lib():
    from po_rrt_amd import build
    build.build()
    from po_rrt_amd import engine
    return engine.load_library(), engine


def test_signatures(lib):
    L, engine = lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "porrt_hip.h")).read(), flags=re.S)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rust = integ[integ.index("```rust"):]
    rust = rust[:rust.index("```", 7)]
    mirror = open(os.path.join(ROOT, "include", "porrt.hpp")).read()
    for s in NEW:
        assert hasattr(L, s), "libporrt_hip.so does not export %s" % s
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, hdr)
        assert m, "%s is not declared in porrt_hip.h" % s
        assert len(getattr(L, s).argtypes) == len(m.group(1).split(",")), "%s: engine.py binds another number of arguments" % s
        assert "pub fn %s(" % s in rust, "%s is not in INTEGRATION.md's Rust block" % s
        assert s in engine.SYMBOLS
    for s in ("porrt_mm_plan_batch", "porrt_mm_plan_batch_get_policies", "porrt_mm_plan_batch_get_plan"):
        assert s in mirror, "%s is not used by include/porrt.hpp" % s
    assert L.porrt_mm_plan_batch.restype == C.c_int64 and L.porrt_mm_plan_batch_get_policies.restype == C.c_int64
    assert L.porrt_mm_plan_batch.argtypes[1] == C.c_uint32 and L.porrt_mm_plan_batch.argtypes[6] == C.c_uint32
    assert L.porrt_mm_plan_batch.argtypes[7:11] == [C.c_double, C.c_double, C.c_uint64, C.c_uint64] and L.porrt_mm_plan_batch.argtypes[-1] == C.c_uint64

    def fields(name):
        body = re.search(r"struct\s+%s\s*\{([^}]*)\}" % name, hdr).group(1)
        return [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(uint64_t|double)", "", decl.strip()).split(",") if f.strip()]
    assert [f.rstrip("_") for f, _ in engine.MmBatchPlan._fields_] == fields("porrt_mm_batch_plan")
    assert [f for f, _ in engine.MmPlanBatchInfo._fields_] == fields("porrt_mm_plan_batch_info")
    assert C.sizeof(engine.MmBatchPlan) == 8 * 8 and C.sizeof(engine.MmPlanBatchInfo) == 8 * 22
    for name in ("plan_mm_prm_batch", "plan_mm_prm_batch_raw", "mm_plan_batch_info", "mm_plan_batch_plan", "mm_plan_batch_expected_costs"):
        assert callable(getattr(engine.Engine, name))


def test_null_arguments_need_no_device(lib):
    L, engine = lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    one, prior = np.zeros(2), np.array([0.5, 0.5])
    off, st, cost = np.full(2, 7, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(1)
    assert L.porrt_mm_plan_batch(None, 1, p(one), p(prior), None, None, 2, 0.1, 2.0, 1000, 0, p(off), p(st), p(cost), None, None, None, None, None, None, 0) < 0
    assert off[0] == 7
    assert L.porrt_mm_plan_batch_get_policies(None, p(off), None, None, None, None, 0) < 0
    assert L.porrt_mm_plan_batch_get_expected_costs(None, 0, p(cost)) < 0
    assert L.porrt_mm_plan_batch_get_plan(None, 0, C.byref(engine.MmBatchPlan())) < 0
    assert L.porrt_mm_plan_batch_info(None, C.byref(engine.MmPlanBatchInfo())) < 0
