"""Many TAMP-RRT branch-and-bound plans in one call (porrt_tamp_rrt_plan_batch), the parts that need no GPU:
the host-only search type (po_rrt_amd/csrc/porrt_bnb_search.hpp) and the driver as a template over the search type
(porrt_astar_search.hpp) under the sanitizers with a stub in place of the device, and the header against the Python binding.

The device call is checked against the single plan and the restatement in tests/test_gpu_tamp_bnb_batch.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("porrt_tamp_rrt_plan_batch", "porrt_tamp_batch_get_pruned", "porrt_tamp_batch_bnb_nodes")


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    return cxx


def test_search_and_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bnb_search_check")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "bnb_search_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bnb_search_check ok" in out.stdout


def test_the_search_header_is_host_only():
    """no HIP in it, directly or through what it includes: the stand-alone program above is built by the host compiler alone"""
    for name in ("porrt_bnb_search.hpp", "porrt_pcg64.hpp"):
        src = open(os.path.join(ROOT, "po_rrt_amd", "csrc", name)).read()
        assert "hip" not in src.replace("no HIP", "").lower(), name
        for inc in re.findall(r'#include "([^"]+)"', src):
            assert inc in ("porrt_astar_search.hpp", "porrt_pcg64.hpp"), inc
    planner = open(os.path.join(ROOT, "po_rrt_amd", "csrc", "porrt_tamp_bnb_batch.hpp")).read()
    assert '#include "porrt_bnb_search.hpp"' in planner and "porrt_astar::run" in planner and "SearchRun<BnbSearch>" in planner
    # the single plan draws its shuffles through the same statement
    assert "porrt_bnb::shuffled" in open(os.path.join(ROOT, "po_rrt_amd", "csrc", "porrt_tamp.hpp")).read()


def test_header_declares_the_batch_and_the_binding_matches_it(tmp_path):
    h = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    for s in SYMBOLS:
        assert s in h
    assert "plan_batch" in open(os.path.join(ROOT, "include", "porrt.hpp")).read()
    from po_rrt_amd import engine
    assert set(SYMBOLS) <= set(engine.SYMBOLS)
    # the header's declarations are the argument types this file states: a program that assigns the symbols to function pointers
    # of those types compiles only if they agree
    src = tmp_path / "types.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "porrt_hip.h"\n'
                   "int64_t (*plan)(porrt_ctx *, uint32_t, const double *, const double *, const uint64_t *, const uint64_t *, uint32_t, double, double,\n"
                   "                uint64_t, uint64_t, double, uint32_t) = porrt_tamp_rrt_plan_batch;\n"
                   "int (*pruned)(const porrt_ctx *, uint32_t, uint64_t *) = porrt_tamp_batch_get_pruned;\n"
                   "int64_t (*nodes)(const porrt_ctx *, uint32_t, int64_t *, int32_t *, double *, uint8_t *, uint64_t) = porrt_tamp_batch_bnb_nodes;\n"
                   "int main() {\n"
                   '    std::printf("%zu\\n", sizeof(porrt_tamp_batch_plan));\n' +
                   "".join('    std::printf("%%zu\\n", offsetof(porrt_tamp_batch_plan, %s));\n' % k for k, _ in engine.TampBatchPlan._fields_) +
                   "    return plan && pruned && nodes ? 0 : 1;\n}\n")
    lib = os.path.join(ROOT, "po_rrt_amd")
    exe = str(tmp_path / "types")
    subprocess.run([_cxx(), "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src), "-L" + lib, "-lporrt_hip",
                    "-Wl,-rpath," + lib], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    # a batch record's size and the offsets of its fields are what they were before this call existed
    assert got[0] == C.sizeof(engine.TampBatchPlan) == 344
    assert got[1:] == [getattr(engine.TampBatchPlan, k).offset for k, _ in engine.TampBatchPlan._fields_]
    assert got[1:] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88]


def test_the_built_library_has_the_symbols_with_the_binding_s_types():
    import po_rrt_amd
    L = po_rrt_amd.load_library()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    u32, u64, dbl, vp = C.c_uint32, C.c_uint64, C.c_double, C.c_void_p
    assert L.porrt_tamp_rrt_plan_batch.restype is C.c_int64
    assert list(L.porrt_tamp_rrt_plan_batch.argtypes) == [vp, u32, vp, vp, vp, vp, u32, dbl, dbl, u64, u64, dbl, u32]
    assert L.porrt_tamp_batch_get_pruned.restype is C.c_int and list(L.porrt_tamp_batch_get_pruned.argtypes) == [vp, u32, C.POINTER(u64)]
    assert L.porrt_tamp_batch_bnb_nodes.restype is C.c_int64 and list(L.porrt_tamp_batch_bnb_nodes.argtypes) == [vp, u32, vp, vp, vp, vp, u64]
    for m in ("plan_tamp_rrt_batch", "tamp_batch_bnb_nodes"):
        assert callable(getattr(po_rrt_amd.Engine, m))
