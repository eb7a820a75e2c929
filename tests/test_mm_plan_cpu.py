"""The multi-modal PRM planner after the growth (build_belief_graph, expected costs, policy; map_shelves_tamp_prm.rs:395-485): the numpy
restatement of tests/mm_plan_ref.py on a hand-built two-level mode tree, and the C ABI that exposes the device version."""
import os
import re

import numpy as np

import mm_plan_ref as ref
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MM_PLAN_SYMBOLS = ["porrt_mm_build_belief_graph", "porrt_mm_bg_num_nodes", "porrt_mm_bg_num_edges", "porrt_mm_bg_num_finals",
                   "porrt_mm_bg_get_graph", "porrt_mm_compute_expected_costs", "porrt_mm_get_expected_costs", "porrt_mm_extract_policy",
                   "porrt_mm_refine_policy", "porrt_mm_plan", "porrt_mm_get_plan_seconds", "porrt_mm_get_dp_info"]


def two_level_tree():
    """2 worlds, prior (0.5, 0.5): mode 0 = the prior (start 0, 1, observation point 2), modes 1 / 2 = object in shelf 0 / 1 (goal 0,
    arrival 1).  Mode 0's roadmap: 1 finds 0, 2 finds 0 and 1; modes 1 and 2: 1 finds 0."""
    modes = [dict(belief=np.array([0.5, 0.5]), xy=np.array([[0.0, 0.0], [0.0, 1.0], [0.0, 2.0]]),
                  edges=(np.array([0, 0, 1]), np.array([1, 2, 2])), finals=np.array([], dtype=np.uint64)),
             dict(belief=np.array([1.0, 0.0]), xy=np.array([[1.0, 2.0], [0.0, 2.0]]), edges=(np.array([0]), np.array([1])),
                  finals=np.array([0], dtype=np.uint64)),
             dict(belief=np.array([0.0, 1.0]), xy=np.array([[-2.0, 2.0], [0.0, 2.0]]), edges=(np.array([0]), np.array([1])),
                  finals=np.array([0], dtype=np.uint64))]
    trs = [dict(zone=0, from_mode=0, to_mode=1, observation=1, pairs=np.array([[2, 1]], dtype=np.uint64)),
           dict(zone=0, from_mode=0, to_mode=2, observation=1, pairs=np.array([[2, 1]], dtype=np.uint64))]
    return dict(n_beliefs=3, modes=modes, transitions=trs)


def hash_of(b):
    return orc.lib().orc_belief_hash(np.ascontiguousarray(b, dtype=np.float64), len(b))


def test_roadmap_children_order():
    # node 3 finds 1 and 0 (kd order), node 4 finds 3 and 0: children = creation neighbours, then the later nodes that found it
    ch = ref.roadmap_children(5, [1, 0, 2, 3, 0], [2, 2, 3, 4, 4])
    assert ch == [[2, 4], [2], [1, 0, 3], [2, 4], [3, 0]]


def test_restatement_on_a_hand_built_tree():
    g = two_level_tree()
    reachable = np.array([[0.5, 0.5], [0.0, 1.0], [1.0, 0.0]])      # belief id = the hash map's index, not the mode id
    bg = ref.build_belief_graph(g, reachable, hash_of)
    assert bg["mode_offsets"].tolist() == [0, 3, 5, 7]
    assert bg["types"].tolist() == [1, 1, 2, 1, 1, 1, 1]
    assert bg["belief_ids"].tolist() == [0, 0, 0, 2, 2, 1, 1]
    assert bg["children"] == [[1, 2], [0, 2], [4, 6], [4], [3], [6], [5]]
    # observation edges first (2 -> 4, 2 -> 6), then the action edges node by node
    assert bg["parents"] == [[1], [0], [0, 1], [4], [2, 3], [6], [2, 5]]
    assert bg["finals"].tolist() == [3, 5]
    dist = ref.expected_costs(bg)
    # 4 -> 3: 1, 6 -> 5: 2; the observation node: 0.5 (0 + 1) + 0.5 (0 + 2); 1: 1 + 1.5; 0: min(1 + 2.5, 2 + 1.5)
    assert dist.tolist() == [3.5, 2.5, 1.5, 0.0, 1.0, 0.0, 2.0]
    oid, par, leaf = ref.extract_policy(bg, dist)
    # clusters in ascending belief id: mode 2's arrival (id 1) before mode 1's (id 2)
    assert oid.tolist() == [0, 1, 2, 6, 4, 3, 5]
    assert par.tolist() == [-1, 0, 1, 2, 2, 4, 3]
    assert leaf.tolist() == [0, 0, 0, 0, 0, 1, 1]


def test_header_declares_and_library_exports_the_mm_plan():
    header = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    declared = set(re.findall(r"\b(porrt_\w+)\s*\(", header))
    missing = [s for s in MM_PLAN_SYMBOLS if s not in declared]
    assert not missing, "include/porrt_hip.h does not declare %s" % missing
    from po_rrt_amd import engine
    assert all(s in engine.SYMBOLS for s in MM_PLAN_SYMBOLS)
    lib = os.path.join(ROOT, "po_rrt_amd", "libporrt_hip.so")
    if os.path.exists(lib):
        import subprocess
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
        assert not [s for s in MM_PLAN_SYMBOLS if s not in exported]
    for m in ("mm_build_belief_graph", "mm_belief_graph", "mm_expected_costs", "mm_extract_policy", "mm_refine_policy", "plan_mm_prm"):
        assert hasattr(engine.Engine, m)


def test_cpp_header_has_the_planner():
    src = open(os.path.join(ROOT, "include", "porrt.hpp")).read()
    assert "class MapShelfDomainTampPRM" in src and "porrt_mm_plan" in src
    assert os.path.exists(os.path.join(ROOT, "examples", "plan_tamp_prm.cpp"))
