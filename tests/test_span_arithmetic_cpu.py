"""The index arithmetic of the flat rewire commit (csrc/porrt_span.hpp: clamped counts, the prefix, the binary search of fixed length,
the rank from the valid words) on the host: tests/span_check.cpp, a program of its own built with the address and undefined-behaviour
sanitizers, checks it against plain loops over random counts -- zeros, counts at and beyond the list capacity, garbage, spans cut by the
row's own end of the step, K up to 4096."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_span_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "span_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "span_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "span_check ok" in out.stdout
