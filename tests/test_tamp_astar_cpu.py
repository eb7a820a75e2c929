"""The TAMP-RRT A* restatement (tests/tamp_astar_ref.py) on the CPU oracle, and the host queue of the device planner
(po_rrt_amd/csrc/porrt_astar_queue.hpp) under the sanitizers.

The device planner (porrt_tamp_rrt_plan_astar) is checked against the restatement in tests/test_gpu_tamp_astar.py."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import tamp_astar_ref as A
import tamp_rrt_ref as R
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START = (0.0, -1.0)
RASTERS = {2: "map_benchmark_like_2_goals_zone_ids", 4: "map_benchmark_like_4_free_zone_ids", 6: "map_benchmark_like_6_free_zone_ids"}


def _oracle(n, seed=0):
    o = orc.Oracle()
    o.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    o.set_zones(cases.load_map(RASTERS[n]), 0.5)
    o.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return o


def _uniform(n):
    return [1.0 / n] * n


def _same_plan(a, b):
    assert a["zone_order"] == b["zone_order"] and a["search_nodes"] == b["search_nodes"]
    for k in ("search_cost", "expected_cost"):
        assert a[k] == b[k]
    for k in ("xy", "beliefs", "node_ec", "node_priority"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    for k in ("parents", "is_leaf", "node_parents", "node_targets"):
        assert np.array_equal(a[k], b[k]), k


def _replay(r, n_zones):
    """the stated order, from the node table alone: pop the lowest (priority, id); the popped node's children must be exactly the
    next ids, in zone order; the first popped node of full depth is the solution"""
    par, tgt, pr = r["node_parents"], r["node_targets"], r["node_priority"]
    depth = [0] * len(par)
    for k in range(1, len(par)):
        assert par[k] < k
        depth[k] = depth[par[k]] + 1
    kids = {}
    for k in range(1, len(par)):
        kids.setdefault(int(par[k]), []).append(k)
    queue, next_id = [(0.0, 0)], 1
    while queue:
        queue.sort()
        _, u = queue.pop(0)
        mine = kids.get(u, [])
        assert mine == list(range(next_id, next_id + len(mine)))
        assert [int(tgt[k]) for k in mine] == sorted(int(tgt[k]) for k in mine)          # zone order
        next_id += len(mine)
        queue += [(float(pr[k]), k) for k in mine]
        if depth[u] == n_zones:
            order, k = [], u
            while k > 0:
                order.append(int(tgt[k]))
                k = int(par[k])
            assert order[::-1] == r["zone_order"] and r["node_ec"][u] == r["search_cost"]
            assert next_id == len(par)                 # nothing was given an id after the solution
            return
        assert len(mine) == n_zones - depth[u]         # a popped inner node has all its children
    raise AssertionError("the replay found no leaf")


def test_queue_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "astar_queue_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "astar_queue_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "astar_queue_check ok" in out.stdout


@pytest.mark.parametrize("n,queries", [(2, 6), (4, 46), (6, 122)])
def test_wave_widths_give_the_same_search(n, queries):
    out = {w: A.Planner(_oracle(n), 0).plan(START, _uniform(n), streams=1, wave=w) for w in (1, 8, 64)}
    for w in (1, 8, 64):
        _replay(out[w], n)
        _same_plan(out[w], out[1])
    # two queries per child of a popped node, and nothing else, at width 1: every node but the root is such a child
    assert out[1]["queries"] == 2 * (out[1]["search_nodes"] - 1) == queries
    assert out[1]["speculated"] == 0
    assert out[64]["waves"] <= out[8]["waves"] <= out[1]["waves"] and out[64]["queries"] >= out[8]["queries"] >= out[1]["queries"]
    if n > 2:
        assert out[64]["waves"] < out[1]["waves"] and out[64]["speculated"] > 0


def test_shared_stream_repeats_because_it_is_set_back():
    P = A.Planner(_oracle(2), 0)
    a = P.plan(START, _uniform(2), streams=0, wave=64)          # the width is forced to 1
    b = P.plan(START, _uniform(2), streams=0)
    _same_plan(a, b)
    assert a["queries"] == b["queries"] == 2 * (a["search_nodes"] - 1) and a["speculated"] == 0
    _replay(a, 2)


@pytest.mark.parametrize("n", [2, 4])
def test_cost_is_not_below_the_branch_and_bounds(n):
    """per-edge streams: both searches give a node the same cost, a function of its zone prefix; the branch and bound's leaf is the
    minimum over all orders.  (The heuristic measures to the zone position while the observation goal is met earlier, so the A*
    leaf is not claimed to be that minimum.)"""
    a = A.Planner(_oracle(n), 0).plan(START, _uniform(n), streams=1)
    b = R.Planner(_oracle(n), 0).plan(START, _uniform(n), streams=1)
    assert a["search_cost"] >= b["search_cost"]
    if a["zone_order"] == b["zone_order"]:
        assert a["search_cost"] == b["search_cost"]
    assert a["queries"] < b["queries"] or n == 2


class _Stub:
    """straight two-state paths instead of RRT* (the shortcut leaves them alone): a zone is seen 60 % of the way to its position"""

    def __init__(self, zone_pos, fail=()):
        self.zp, self.fail, self.expanded = zone_pos, set(fail), set()

    def __call__(self, start, which, zone, p, prefix):
        self.expanded.add(prefix[:-1])
        if (prefix, which) in self.fail:
            return None
        z = self.zp[zone]
        end = (start[0] + 0.6 * (z[0] - start[0]), start[1] + 0.6 * (z[1] - start[1])) if which == "observation" else (z[0], z[1])
        return [list(start), list(end)], math.hypot(end[0] - start[0], end[1] - start[1])


def _stub_plan(wave, fail=()):
    o = _oracle(4)
    stub = _Stub([tuple(map(float, z)) for z in o.zone_positions()], fail)
    prior = [0.4, 0.3, 0.2, 0.1]
    return A.Planner(o, 0).plan(START, prior, streams=1, wave=wave, query=stub), stub


def _prefixes(r):
    pre = [()]
    for k in range(1, len(r["node_parents"])):
        pre.append(pre[int(r["node_parents"][k])] + (int(r["node_targets"][k]),))
    return pre


def test_a_failure_counts_only_under_a_popped_node():
    base, s1 = _stub_plan(1)
    wide, s64 = _stub_plan(64)
    _same_plan(wide, base)
    _replay(base, 4)
    popped = s1.expanded                                  # width 1 expands exactly what it pops
    only_speculated = sorted(s64.expanded - popped)
    assert only_speculated and wide["speculated"] == len(only_speculated)
    # under a node that width 1 never pops: no error at width 64, the same plan
    sp = only_speculated[0]
    t = min(z for z in range(4) if z not in sp)
    for which in ("observation", "pickup"):
        r, _ = _stub_plan(64, fail={(sp + (t,), which)})
        _same_plan(r, base)
    # under a popped node: the id the child would have got, the first failing child in zone order, at every width
    pre = _prefixes(base)
    parent = max((p for p in popped if len(p) == 1), key=lambda p: pre.index(p))          # not the root: ids and pops came before it
    zones = [z for z in range(4) if z not in parent]
    first_child = min(k for k in range(len(pre)) if pre[k][:-1] == parent and len(pre[k]) == 2)
    fail = {(parent + (zones[1],), "pickup"), (parent + (zones[2],), "observation")}
    for w in (1, 8, 64):
        with pytest.raises(A.NoPath) as ex:
            _stub_plan(w, fail=fail)
        assert (ex.value.node, ex.value.zone, ex.value.which) == (first_child + 1, zones[1], "pickup")
    fail = {(parent + (zones[0],), "observation"), (parent + (zones[0],), "pickup")}
    for w in (1, 64):
        with pytest.raises(A.NoPath) as ex:
            _stub_plan(w, fail=fail)
        assert (ex.value.node, ex.value.zone, ex.value.which) == (first_child, zones[0], "observation")


def test_refusals():
    P = A.Planner(_oracle(2), 0)
    for bad in ([1.0, 0.0], [0.5, 0.6], [1.0], [0.3, 0.3, 0.4], [1.5, -0.5]):
        with pytest.raises(ValueError):
            P.plan(START, bad)


def test_header_declares_the_planner():
    h = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    for s in ("porrt_tamp_rrt_plan_astar", "porrt_tamp_rrt_get_astar_info", "porrt_tamp_astar_nodes", "porrt_tamp_astar_info",
              "porrt_tamp_shortcut_paths_resident"):
        assert s in h
    assert "plan_astar" in open(os.path.join(ROOT, "include", "porrt.hpp")).read()
    import po_rrt_amd
    assert {"porrt_tamp_rrt_plan_astar", "porrt_tamp_rrt_get_astar_info", "porrt_tamp_astar_nodes"} <= set(po_rrt_amd.engine.SYMBOLS)
