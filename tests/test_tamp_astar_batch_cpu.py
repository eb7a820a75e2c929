"""Many TAMP-RRT A* plans in one call (porrt_tamp_rrt_plan_astar_batch), the parts that need no GPU: the
host-only search type and driver (po_rrt_amd/csrc/porrt_astar_search.hpp) under the sanitizers with a stub in place of the device,
and the header against the Python binding.

The device call is checked against the single plan and the restatement in tests/test_gpu_tamp_astar_batch.py."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("porrt_tamp_rrt_plan_astar_batch", "porrt_tamp_batch_get_plan", "porrt_tamp_batch_policy", "porrt_tamp_batch_astar_nodes")


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    return cxx


def test_search_and_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "astar_search_check")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "astar_search_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "astar_search_check ok" in out.stdout


def test_the_search_header_is_host_only():
    """no HIP in it, directly or through what it includes: the stand-alone program above is built by the host compiler alone"""
    for name in ("porrt_astar_search.hpp", "porrt_astar_queue.hpp"):
        src = open(os.path.join(ROOT, "po_rrt_amd", "csrc", name)).read()
        assert "hip" not in src.replace("no HIP", "").replace("No HIP", "").lower(), name
    planner = open(os.path.join(ROOT, "po_rrt_amd", "csrc", "porrt_tamp_astar.hpp")).read()
    assert '#include "porrt_astar_search.hpp"' in planner and "porrt_astar::run" in planner


def test_header_declares_the_batch_and_the_binding_matches_it(tmp_path):
    h = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    for s in SYMBOLS + ("porrt_tamp_batch_plan",):
        assert s in h
    assert "plan_astar_batch" in open(os.path.join(ROOT, "include", "porrt.hpp")).read()
    from po_rrt_amd import engine
    assert set(SYMBOLS) <= set(engine.SYMBOLS)
    # size and offsets of porrt_tamp_batch_plan as the C compiler lays the header's struct out
    names = [k for k, _ in engine.TampBatchPlan._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "porrt_hip.h"\nint main() {\n'
                   '    std::printf("%zu\\n", sizeof(porrt_tamp_batch_plan));\n' +
                   "".join('    std::printf("%%zu\\n", offsetof(porrt_tamp_batch_plan, %s));\n' % k for k in names) +
                   "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([_cxx(), "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(engine.TampBatchPlan) == 344
    assert got[1:] == [getattr(engine.TampBatchPlan, k).offset for k in names]
    assert engine.TampBatchPlan.zone_order.size == 64 * 4
