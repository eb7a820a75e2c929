"""The TAMP-RRT branch-and-bound restatement (tests/tamp_rrt_ref.py) on the CPU oracle, and the C++ mirror's build.

The device planner (porrt_tamp_rrt_plan) is checked against the restatement in tests/test_gpu_tamp_rrt.py."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import cases
import refine_ref
import tamp_rrt_ref as R
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(zone_ids, seed=0):
    o = orc.Oracle()
    o.set_grid(cases.load_map("map_benchmark_like"), (-1.0, -1.0), (1.0, 1.0), cases.SHELF)
    o.set_zones(zone_ids, 0.5)
    o.set_sampler((-1.0, -1.0), (1.0, 1.0), seed)
    return o


def _three_zones():
    z = cases.load_map("map_benchmark_like_4_free_zone_ids").copy()
    z[z == 3] = 255                     # zones 0, 1, 2 with their free centroids
    return z


def test_splitmix64_and_edge_seeds():
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF   # SplitMix64's first output from state 0
    assert R.edge_seed(5, ()) == 5
    assert R.edge_seed(5, (2, 0)) == R.splitmix64(R.splitmix64(5 ^ 3) ^ 1)


def test_shuffled_is_swap_remove():
    rng, ref = orc.Pcg64.seed_from_u64(3), orc.Pcg64.seed_from_u64(3)
    got = R.shuffled(range(5), rng)
    to, want = list(range(5)), []
    while to:                                    # Vec::swap_remove: the last element takes the drawn one's place
        i = ref.gen_range_usize(0, len(to))
        want.append(to[i])
        last = to.pop()
        if i < len(to):
            to[i] = last
    assert sorted(got) == list(range(5)) and got == want


def test_branch_and_bound_finds_the_brute_force_minimum():
    """3 zones, one stream per edge: every node's cost is a function of its zone prefix, so the minimum over all 6 orders is known"""
    o = _oracle(_three_zones())
    assert o.n_zones() == 3
    P = R.Planner(o, 0)
    r = P.plan((0.0, -1.0), [1 / 3] * 3, streams=1)
    p = dict(max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, K=128)
    memo = {}

    def node_cost(prefix):                       # the search's own arithmetic along one branch
        if prefix in memo:
            return memo[prefix]
        ec, rp, b, state = 0.0, 1.0, [1 / 3] * 3, (0.0, -1.0)
        for d in range(len(prefix)):
            t, u_target = prefix[d], prefix[d - 1] if d else None
            vb = list(b)
            if u_target is not None:
                vb[u_target] = 0.0
            vb = R.normalize(vb)
            rp = rp * R.transition_probability(b, vb)
            o.set_sampler((-1.0, -1.0), (1.0, 1.0), R.edge_seed(0, prefix[:d + 1]))
            path, oc = P._query(state, "observation", t, p)
            end = (float(path[-1][0]), float(path[-1][1]))
            _, pc = P._query(end, "pickup", t, p)
            ec = ec + rp * (oc + vb[t] * pc)
            b, state = vb, end
        memo[prefix] = ec
        return ec

    costs = {perm: node_cost(perm) for perm in itertools.permutations(range(3))}
    best = min(costs.values())
    assert r["search_cost"] == best
    assert costs[tuple(r["zone_order"])] == best
    assert r["queries"] <= 2 * 15                # at most the full tree's 15 edges


def test_wave_widths_give_the_same_best_leaf():
    z = _three_zones()
    out = [R.Planner(_oracle(z), 0).plan((0.0, -1.0), [1 / 3] * 3, streams=1, wave=w) for w in (1, 2, 64)]
    for r in out[1:]:
        assert r["zone_order"] == out[0]["zone_order"] and r["search_cost"] == out[0]["search_cost"]
        assert np.array_equal(r["xy"], out[0]["xy"]) and r["expected_cost"] == out[0]["expected_cost"]
    assert out[2]["waves"] < out[0]["waves"]


def test_shortcut_draws_are_partial_shortcuts_and_short_paths_stay():
    for n in (3, 7, 40):
        assert R.shortcut_draws(n) == refine_ref.draws(n, 100)
    o = _oracle(cases.load_map("map_benchmark_like_4_free_zone_ids"))
    for path in ([], [[0.0, -1.0]], [[0.0, -1.0], [0.3, 0.2]]):
        assert R.shortcut(o, path) == path


def test_shortcut_does_not_check_the_step_into_node_e():
    o = _oracle(cases.load_map("map_benchmark_like_4_free_zone_ids"))
    path = R.find_unchecked_path(o)
    got = R.shortcut(o, path)
    assert got[1] != path[1] and got[0] == path[0] and got[2] == path[2]
    assert o.traversed_class(got[1], got[2]) != orc.FREE          # committed across an obstacle
    # partial_shortcut (the policy refiner) checks that step and refuses the same candidate
    states = [list(s) for s in path]
    nv = len(o.validities())
    refine_ref.partial_shortcut(o, states, [True] * nv, nv, 100)
    assert states[1] != got[1]


def test_build_policy_on_a_hand_made_chain():
    """root -> zone 1 -> zone 0 on 2 worlds, two-state paths (the shortcut leaves them): costs worked out by hand"""
    o = _oracle(cases.load_map("map_benchmark_like_2_goals_zone_ids"))
    a, b, c, d, e = (0.0, -1.0), (0.0, -0.5), (0.3, -0.5), (0.0, 0.0), (-0.4, 0.0)
    chain = [dict(target=None, belief=[0.5, 0.5], path_obs=[], path_pick=[]),
             dict(target=1, belief=[0.5, 0.5], path_obs=[a, b], path_pick=[b, c]),
             dict(target=0, belief=[1.0, 0.0], path_obs=[b, d], path_pick=[d, e])]
    pol = R.build_policy(o, chain)
    # nodes: 0 a, 1 b, 2 b (pickup, belief [0 1]), 3 c (leaf), 4 b (belief [1 0]), 5 d, 6 d (pickup [1 0]), 7 e (leaf)
    assert pol["parents"].tolist() == [-1, 0, 1, 2, 1, 4, 5, 6]
    assert pol["is_leaf"].tolist() == [0, 0, 0, 1, 0, 0, 0, 1]
    assert pol["beliefs"].tolist() == [[0.5, 0.5], [0.5, 0.5], [0.0, 1.0], [0.0, 1.0], [1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [1.0, 0.0]]
    # a -> b with q 1 (0.5), b -> b' and b -> c with q 0.5, b -> b'' with q 0.5, then d and e with p 0.5: 0.5 + 0.5 * 0.3 + 0.5 * (0.5 + 0.4)
    want = 1.0 * 1.0 * 0.5 + (0.5 * 0.0 + 0.5 * 1.0 * 0.3) + (0.5 * 0.0 + 0.5 * 1.0 * 0.5 + 0.5 * 1.0 * 0.0 + 0.5 * 1.0 * 0.4)
    assert math.isclose(pol["expected_cost"], want, rel_tol=1e-12)
    assert math.isclose(pol["expected_cost"], 1.1, rel_tol=1e-12)


def test_header_declares_and_library_exports_the_planner():
    h = open(os.path.join(ROOT, "include", "porrt_hip.h")).read()
    for s in ("porrt_tamp_rrt_plan", "porrt_tamp_rrt_policy", "porrt_tamp_rrt_get_info", "porrt_tamp_shortcut_paths", "porrt_best_paths",
              "PORRT_ERR_NO_PATH = -10"):
        assert s in h
    assert "class MapShelfDomainTampRRT" in open(os.path.join(ROOT, "include", "porrt.hpp")).read()


def test_cpp_example_builds_and_needs_a_gpu(tmp_path):
    import torch
    from po_rrt_amd import build
    build.build()
    exe = str(tmp_path / "plan_tamp_rrt")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "examples", "plan_tamp_rrt.cpp"),
                    "-L" + os.path.join(ROOT, "po_rrt_amd"), "-lporrt_hip", "-Wl,-rpath," + os.path.join(ROOT, "po_rrt_amd")], check=True)
    if torch.cuda.is_available():
        return
    out = subprocess.run([exe, os.path.join(cases.MAPS, "map_benchmark_like.pgm"),
                          os.path.join(cases.MAPS, "map_benchmark_like_2_goals_zone_ids.pgm"), "2"], capture_output=True, text=True)
    assert out.returncode == 1 and "no usable HIP device" in out.stderr
