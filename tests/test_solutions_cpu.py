"""RRT::get_solutions (rrt.rs:195-246): the restatement tests/solutions_ref.py on the CPU oracle, and the interface of its device
path (porrt_solutions).  The device call is checked against the restatement in tests/test_gpu_solutions.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cases
import solutions_ref as S
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["porrt_solutions", "porrt_tamp_rrt_plan_viewpoints", "porrt_tamp_rrt_get_viewpoints_info"]
START = (0.0, -1.0)


def test_header_declares_library_exports_and_engine_binds():
    from po_rrt_amd import build, engine
    build.build()
    L = engine.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "porrt_hip.h")).read(), flags=re.S)
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, hdr)
        assert m, "%s is not declared in porrt_hip.h" % s
        assert hasattr(L, s), "libporrt_hip.so does not export %s" % s
        assert s in engine.SYMBOLS
        assert len(getattr(L, s).argtypes) == len(m.group(1).split(",")), "%s: engine.py binds another number of arguments" % s
    for m in ("solutions", "solutions_batch", "plan_tamp_rrt_viewpoints", "tamp_viewpoints_info"):
        assert hasattr(engine.Engine, m)
    mirror = open(os.path.join(ROOT, "include", "porrt.hpp")).read()
    assert "porrt_solutions" in mirror and "plan_multiple_viewpoints" in mirror


def test_null_and_empty_arguments_are_invalid():
    from po_rrt_amd import build, engine
    build.build()
    L = engine.load_library()
    n = np.zeros(1, dtype=np.uint64)
    assert L.porrt_solutions(None, 0, None, None, None, None, None, 0, None, 0) == -1
    assert L.porrt_solutions(None, 1, n.ctypes.data, n.ctypes.data, None, None, None, 0, None, 0) == -1
    arr = (C.c_void_p * 1)(None)
    assert L.porrt_solutions(arr, 0, n.ctypes.data, n.ctypes.data, None, None, None, 0, None, 0) == -1      # no contexts
    assert L.porrt_solutions(arr, 1, n.ctypes.data, n.ctypes.data, None, None, None, 0, None, 0) == -1      # a NULL context
    z = np.zeros(2)
    assert L.porrt_tamp_rrt_plan_viewpoints(None, z, z, 2, 0.1, 2.0, 10, 10, 0.05, 1, 0) == -1
    assert L.porrt_tamp_rrt_get_viewpoints_info(None, C.byref(engine.TampViewpointsInfo())) == -1
    assert L.porrt_tamp_rrt_get_viewpoints_info(None, None) == -1


def _oracle(zones, seed=0):
    o = orc.Oracle()
    o.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    o.set_zones(cases.load_map(zones), 0.5)
    o.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return o


def _check(o):
    xy, parent, _ = o.tree()
    finals = o.final_ids()
    got = S.of_oracle(o)
    ids = [i for i, _, _ in got]
    assert ids == [int(i) for i in o.firstly_final_ids()]
    fset = set(int(f) for f in finals)
    assert 0 not in fset                                       # only added nodes are pushed (rrt.rs:165-167)
    assert ids == sorted(f for f in fset if int(parent[f]) not in fset)
    for i, path, cost in got:
        assert np.array_equal(path[0], xy[0]) and np.array_equal(path[-1], xy[i])
        assert cost == S.path_cost(path)
    return len(ids), len(finals)


@pytest.mark.parametrize("zones,zone", [("map_benchmark_like_2_goals_zone_ids", 1), ("map_benchmark_like_4_free_zone_ids", 2)])
@pytest.mark.parametrize("n_iter_min,K", [(300, 1), (300, 128), (2500, 1), (2500, 128)])
def test_ids_are_the_finals_with_a_non_final_parent_observation_goal(zones, zone, n_iter_min, K):
    o = _oracle(zones)
    o.set_observation_goal(zone)
    o.grow(START, 0.1, 2.0, n_iter_min, 10000, batch_K=K, algo=orc.ALGO_BATCHED_KD if K > 1 else orc.ALGO_SEQ)
    n_sol, n_fin = _check(o)
    assert 1 <= n_sol <= n_fin


def test_ids_on_a_square_pickup_goal():
    o = _oracle("map_benchmark_like_4_free_zone_ids")
    zp = o.zone_positions()[0]
    o.set_square_goal(np.array([zp]), np.array([1], dtype=np.uint64), 0.05)
    o.grow((0.0, -0.8), 0.1, 2.0, 2500, 10000, batch_K=128, algo=orc.ALGO_BATCHED_KD)
    n_sol, n_fin = _check(o)
    assert n_sol >= 1


def test_hand_made_tree():
    #  0 root; 1 final child of the root; 2 -> 3 -> 4 -> 5: 3, 4, 5 a chain of three finals under the non-final 2;
    #  6 (non-final, under 1... no: under 0) -> 7 final -> 8 final: parent final, grandparent not; 9 a non-final leaf
    xy = np.array([[0, 0], [1, 0], [0, 1], [0, 2], [0, 3], [0, 4], [-1, 0], [-2, 0], [-2, 1], [3, 3]], dtype=np.float64)
    parent = np.array([-1, 0, 0, 2, 3, 4, 0, 6, 7, 1])
    finals = np.array([5, 1, 8, 3, 4, 7], dtype=np.uint64)       # any order: the set decides
    assert S.firstly_final_ids(parent, finals) == [1, 3, 7]
    got = S.solutions(xy, parent, finals)
    assert [i for i, _, _ in got] == [1, 3, 7]
    assert got[0][1].tolist() == [[0, 0], [1, 0]] and got[0][2] == 1.0
    assert got[1][1].tolist() == [[0, 0], [0, 1], [0, 2]] and got[1][2] == 2.0
    assert got[2][1].tolist() == [[0, 0], [-1, 0], [-2, 0]] and got[2][2] == 2.0
    assert S.firstly_final_ids(parent, np.array([8], dtype=np.uint64)) == [8]     # its parent 7 is no longer final
    assert S.solutions(xy, parent, np.zeros(0, dtype=np.uint64)) == []            # no finals at all
    # a final child of the root ends its walk there: unwrap_or(0) reads the root, which is never final
    assert S.firstly_final_ids(np.array([-1, 0, 1]), np.array([1, 2], dtype=np.uint64)) == [1]
