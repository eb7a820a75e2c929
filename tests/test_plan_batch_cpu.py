"""porrt_plan_belief_space_batch without a device: the index arithmetic of the union of PTO graphs (csrc/porrt_join.hpp: the pass
cuts, the member of a union index by a search of fixed length, belief node ids there and back) checked on the host by
tests/join_check.cpp, a program of its own built with the address and undefined-behaviour sanitizers; and the entry points' answers
to NULL arguments, which need no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "join_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "join_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "join_check ok" in out.stdout


@pytest.fixture(scope="module")
def lib():
    from po_rrt_amd import build
    build.build()
    from po_rrt_amd import engine
    return engine.load_library(), engine


def test_null_arguments_need_no_device(lib):
    L, engine = lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    prior = np.array([0.5, 0.5])
    off, st, cost = np.full(3, 7, dtype=np.uint64), np.zeros(2, dtype=np.uint8), np.zeros(2)

    def call(ctxs, n):
        return L.porrt_plan_belief_space_batch(ctxs, n, p(prior), 2, 0, p(off), p(st), p(cost), None, None, None, None, None, None, 0)
    assert call(None, 2) < 0                                     # a NULL context list
    assert call((C.c_void_p * 2)(None, None), 2) < 0             # NULL members
    assert off[0] == 7
    assert call(None, 0) == 0 and off[0] == 0                    # no members: nothing to plan
    assert L.porrt_plan_belief_space_batch(None, 0, p(prior), 2, 0, None, None, None, None, None, None, None, None, None, 0) < 0
    info = engine.PlanBatchInfo()
    assert L.porrt_plan_batch_info(None, C.byref(info)) < 0
    assert L.porrt_plan_batch_get_policies(None, p(off), None, None, None, None, 0) < 0
    assert L.porrt_plan_batch_get_expected_costs(None, 0, p(cost)) < 0
