"""CPU side of the clamped-sample inputs (tests/mm_clamped_inputs.py): from the oracle (oracle/mmprm.c: literal kd-tree insertion) and
the restatements (mm_plan_ref, policies_ref, refine_ref) alone, the inputs are what tests/test_gpu_mm_clamped.py needs -- copies of
roadmap nodes, kd chains of equal keys, zero-length edges, walks that return onto their own path and walks that end, zero-length
steps in the policies handed to the refiner.  The floors sit under what the oracle gives:

  input   modes   nodes   duplicate nodes   largest multiplicity   equal x / y   zero-length child edges   duplicate starts: status 0 / 2
  A           3    3123                55                     14       40 / 40                       570                          31 / 24
  B          15   32205               109                     18     150 / 152                      2880                          51 / 58
  C        1364   89693               213                     72     145 / 206                      7880                 (the root is +inf)

With the sampler's window on the whole map the same cases have no duplicate at all."""
import numpy as np
import pytest

import cases
import mm_clamped_inputs as M
import mm_plan_ref
import policies_ref
import refine_policies_cases as rp


@pytest.fixture(scope="module")
def planned(oracle_lib):
    """the oracle's growth, belief graph and expected costs of an input, made once per module; read only"""
    made = {}

    def get(name):
        if name not in made:
            inp = M.INPUTS[name]()
            o = M.configure(oracle_lib.Oracle(), inp)
            made[name] = (inp, o) + M.plan(o, inp)
        return made[name]
    yield get
    made.clear()


def test_counters():
    """the counters on a hand-made growth: two modes, the second with three copies of one place and a pair at another"""
    m0 = dict(xy=np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.5]]))
    m1 = dict(xy=np.array([[0.5, 0.5], [0.25, 0.5], [0.5, 0.5], [0.25, 0.5], [0.5, 0.5], [0.5, 0.75], [-0.0, 0.0], [0.0, 0.0]]))
    g = dict(modes=[m0, m1, dict(xy=np.zeros((0, 2)))])
    assert M.duplicates_per_mode(g).tolist() == [0, 5, 0] and M.multiplicity_per_mode(g).tolist() == [1, 3, 0]       # -0.0 is another place
    assert M.largest_multiplicity(g) == 3 and M.mode_sizes(g).tolist() == [3, 8, 0]
    assert M.longest_equal_run(g, 0) == 4 and M.longest_equal_run(g, 1) == 5
    xy = np.concatenate([m0["xy"], m1["xy"]])
    bg = dict(xy=xy, belief_vec=np.repeat([0, 1], [3, 8]), mode_offsets=np.array([0, 3, 11, 11], dtype=np.uint64),
              children=[[3], [0], [], [5, 7, 4], [6], [3], [], [], [], [10], [9]])
    assert M.duplicate_nodes(bg) == [3, 4, 5, 6, 7]
    assert M.zero_length_child_edges(bg) == (4, 4)             # 3 -> 5, 3 -> 7, 4 -> 6, 5 -> 3; -0.0 and 0.0 are different bits
    bg["xy"][0] = (0.5, 0.5)
    assert M.zero_length_child_edges(bg) == (5, 4)             # 0 -> 3 crosses the modes


def test_the_window_stays_off_the_grid(oracle_lib):
    """the trap: cases.configure hands low / up to set_grid as well, and then the root of A has no finite cost"""
    inp = M.input_a()
    assert "low" not in inp and "up" not in inp
    with pytest.raises(AssertionError):
        M.configure(oracle_lib.Oracle(), cases.Case(inp, low=inp.window_low, up=inp.window_up))
    o = cases.configure(oracle_lib.Oracle(), cases.Case(inp, low=inp.window_low, up=inp.window_up))
    o.set_discrete_seed(inp.discrete_seed)
    _, _, dist = M.plan(o, inp)
    assert np.isinf(dist[0])
    o = cases.configure(oracle_lib.Oracle(), inp)              # the whole map as the window: no copies
    o.set_discrete_seed(inp.discrete_seed)
    g, bg, _ = M.plan(o, inp)
    assert M.duplicates_per_mode(g).sum() == 0 and M.longest_equal_run(g, 1) == 1


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_growth_and_belief_graph(planned, name):
    inp, o, g, bg, dist = planned(name)
    c = M.assert_ties(name, g, bg)
    print(name, c)
    assert np.isfinite(dist[0]) == (name != "C")
    assert c["zero_length_edges"] > 0 and c["modes_with_duplicates"] >= (2 if name != "C" else 30)
    if name == "A":
        assert c["zero_length_action_edges"] > 0               # copies joined by roadmap edges: zero-length cycles
    # a second growth on the same oracle: the discrete stream has moved on, the continuous sampler is cloned from the same state
    if name == "A":
        g2 = M.grow(o, inp, prior=[0.3, 0.7])
        assert M.duplicates_per_mode(g2).sum() >= M.FLOORS["A"]["duplicates"]
        assert not all(np.array_equal(a["xy"], b["xy"]) for a, b in zip(g["modes"], g2["modes"]))


@pytest.mark.parametrize("name", ["A", "B"])
def test_policy_starts(planned, name):
    inp, o, g, bg, dist = planned(name)
    st = M.Starts(bg, dist)
    assert st.dropped == [], "policies_ref answers status 3 or 4 for starts %s: they are left out of the list" % st.dropped
    assert not np.isin(st.status, (policies_ref.ASSERT, policies_ref.CAPACITY)).any()
    dup = M.duplicate_nodes(bg)
    assert st.starts[0] == 0 and st.starts[1:1 + st.n_duplicates] == dup and len(st.starts) == 1 + len(dup) + 50
    assert dup == sorted(dup) and len(dup) == M.duplicates_per_mode(g).sum()
    ok, own = M.assert_statuses(name, st)
    print(name, "duplicate starts: %d status 0, %d status 2; node 0: status %d" % (ok, own, st.status[0]))
    assert st.status[0] == policies_ref.OK
    # the policy from node 0 is the oracle's own extract_policy
    oid, par, leaf = mm_plan_ref.extract_policy(bg, dist)
    assert all(np.array_equal(a, b) for a, b in zip(st.want[0][1], (oid, par, leaf)))


@pytest.mark.parametrize("name,count,n", [("A", M.REFINED_A, 200), ("B", M.REFINED_B, 200)])
def test_refiner_policies(planned, name, count, n):
    inp, o, g, bg, dist = planned(name)
    st = M.Starts(bg, dist)
    pols = st.refiner_policies(bg, count)
    assert len(pols) == count
    zero = sum(M.zero_length_steps(bg, st.want[q][1]) for q, _ in pols)
    print(name, "%d policies, %d zero-length steps" % (len(pols), zero))
    if name == "A":
        assert zero >= M.FLOORS["A"]["refiner_zero_steps"]
    for q, pol in pols:                                         # the restatement runs on every one of them
        (x, oid, par, leaf), cost = rp.restate(o, pol, bg["beliefs"], n)
        assert len(x) == len(pol[1]) and np.isfinite(cost)
