"""GPU parity of the multi-modal PRM on clamped observation samples (tests/mm_clamped_inputs.py): copies of roadmap nodes, kd chains of
equal keys, zero-length edges and zero-length cycles, met through the public interface alone (a sampler window narrower than the map).

Every other multi-modal case of the suite has distinct nodes within a mode, no equal y and no zero-length edge, so k_seg_kd_ranks,
k_mm_connect, k_mm_order, the belief-graph build, k_mm_level, the general sweeps on the mode graph, the policy walks and the refiner
never met an exact tie there.  Here the engine is compared bit for bit with the oracle's literal loop (oracle/mmprm.c) and with the
restatements run on the ORACLE's growth (mm_plan_ref, policies_ref, refine_ref); nothing has a tolerance.  Every test asserts from
the oracle's side, with the floors of tests/test_mm_clamped_cpu.py, that the ties it is here for occurred."""
import numpy as np
import pytest

import mm_clamped_inputs as M
import policies_ref
import refine_policies_cases as rp
from oracle import orc
from test_gpu_mm_plan import assert_dist, assert_graph
from test_gpu_mmprm import assert_same
from test_gpu_policies import assert_answers, bits
from test_gpu_refine_policies import assert_same as assert_same_refined

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


class Side:
    """the oracle's side of an input, made once per module and read only: growth, belief graph, expected costs, the counters of the
    ties (their floors asserted when it is made), and -- for the inputs with a finite root -- the start list with the restatement's
    answers and the restated refinements"""

    def __init__(self, name):
        self.name, self.inp = name, M.INPUTS[name]()
        self.o = M.configure(orc.Oracle(), self.inp)
        self.g, self.bg, self.dist = M.plan(self.o, self.inp)
        self.ties = M.assert_ties(name, self.g, self.bg)
        print("input %s on the oracle: %s" % (name, self.ties))
        self._starts, self._refined = None, {}

    @property
    def starts(self):
        if self._starts is None:
            self._starts = M.Starts(self.bg, self.dist)
            assert self._starts.dropped == []
            print("input %s: duplicate starts with status 0 / 2: %s" % (self.name, M.assert_statuses(self.name, self._starts)))
        return self._starts

    def refined(self, q, n):
        """refine_ref.refine of the restatement's policy from starts[q], n iterations"""
        if (q, n) not in self._refined:
            self._refined[q, n] = rp.restate(self.o, M.policy_arrays(self.bg, self.starts.want[q][1]), self.bg["beliefs"], n)
        return self._refined[q, n]


@pytest.fixture(scope="module")
def side():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Side(name)
        return made[name]
    yield get
    made.clear()


@pytest.fixture(scope="module")
def planned(eng_mod, side):
    """an engine with the input grown and its belief graph built (the options at their defaults), once per module: (engine, growth)"""
    made = {}

    def get(name):
        if name not in made:
            e = M.configure(eng_mod.Engine(), side(name).inp)
            g = M.grow(e, side(name).inp)
            e.mm_build_belief_graph()
            made[name] = (e, g)
        return made[name]
    yield get
    made.clear()


DEFAULTS = dict(mm_levels=0, dp_sweeps=0, mm_lds_nodes=6400)


def costs_with(e, **opts):
    """the expected costs and mm_dp_info under the given options; the options are put back"""
    try:
        for k, v in dict(DEFAULTS, **opts).items():
            e.set_option(k, v)
        return e.mm_expected_costs(), e.mm_dp_info()
    finally:
        for k, v in DEFAULTS.items():
            e.set_option(k, v)


# ---------------------------------------------------------------------------------------------------------------- growth
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_growth(side, planned, name):
    """k_seg_kd_ranks on chains of equal keys (C: 72 copies of one place, a chain longer than a wave, and modes smaller than a wave
    that hold copies), k_mm_connect at distance 0, k_mm_order: nodes, edges in the reference's adjacency order, finals, transitions"""
    s = side(name)
    assert s.ties["duplicates"] > 0 and s.ties["equal_y"] >= s.ties["multiplicity"] >= 2
    if name == "C":
        assert s.ties["multiplicity"] > M.WAVE
    assert_same(planned(name)[1], s.g)


@pytest.mark.parametrize("name", ["A", "B"])
def test_growth_one_by_one(eng_mod, side, monkeypatch, name):
    """the grid-binned k_prm_connect with the host's kd ranks, one launch sequence per mode, against the oracle"""
    s = side(name)
    assert s.ties["duplicates"] >= M.FLOORS[name]["duplicates"]
    monkeypatch.setenv("PORRT_MM_ONE_BY_ONE", "1")
    e = M.configure(eng_mod.Engine(), s.inp)
    assert_same(M.grow(e, s.inp), s.g)


def test_second_growth_on_the_same_contexts(eng_mod):
    """the continuous sampler is cloned, not advanced; the discrete stream has moved on, the same on both sides"""
    inp = M.input_a()
    e, o = M.configure(eng_mod.Engine(), inp), M.configure(orc.Oracle(), inp)
    assert_same(M.grow(e, inp), M.grow(o, inp))
    ge, go = M.grow(e, inp, prior=[0.3, 0.7]), M.grow(o, inp, prior=[0.3, 0.7])
    assert M.duplicates_per_mode(go).sum() >= M.FLOORS["A"]["duplicates"] and M.largest_multiplicity(go) >= M.FLOORS["A"]["multiplicity"]
    assert_same(ge, go)


# ---------------------------------------------------------------------------------------------------------------- belief graph, costs
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_belief_graph_and_expected_costs(side, planned, name):
    """the build's count / scan / scatter / order on rows that hold copies, then the general sweeps over zero-length cycles"""
    s, (e, _) = side(name), planned(name)
    assert s.ties["zero_length_edges"] >= M.FLOORS["A"]["zero_length_edges"]
    assert_graph(e, s.bg)
    d, info = costs_with(e)
    assert not info["level_schedule"]
    assert_dist(d, s.dist)
    assert np.isfinite(s.dist[0]) == (name != "C")
    if name == "C":
        with pytest.raises(RuntimeError):
            e.mm_extract_policy()                                          # no policy from an infinite root


@pytest.mark.parametrize("name", ["B", "C"])
def test_level_schedule(side, planned, name):
    """k_mm_level: a mode's roadmap relaxed to its fixpoint by one workgroup, over zero-length edges between copies"""
    s, (e, _) = side(name), planned(name)
    assert s.ties["zero_length_edges"] > 0 and s.ties["duplicates"] > 0
    d, info = costs_with(e, mm_levels=1)
    assert info["level_schedule"] and info["launches"] == info["levels"]
    assert_dist(d, s.dist)


@pytest.mark.parametrize("opts", [dict(dp_sweeps=1), dict(mm_lds_nodes=0), dict(mm_lds_nodes=M.LDS_LIMIT)], ids=["sweeps", "global", "mixed"])
def test_level_schedule_paths_on_b(side, planned, opts):
    """with test_level_schedule[B] the four runs of test_level_schedule_equals_general_sweeps_and_lds_limit: the level kernel in LDS,
    on global memory, both in one launch (B has modes above and below 2000 nodes), and the general sweeps on request"""
    s, (e, _) = side("B"), planned("B")
    sizes = M.mode_sizes(s.g)
    assert sizes.max() > M.LDS_LIMIT and sizes.min() < M.LDS_LIMIT and s.ties["zero_length_action_edges"] > 0
    d, info = costs_with(e, mm_levels=1, **opts)
    assert info["level_schedule"] == ("dp_sweeps" not in opts)
    assert_dist(d, s.dist)


# ---------------------------------------------------------------------------------------------------------------- policies
def extracted(e, s):
    """mm_extract_policies of the input's start list on fresh default costs"""
    costs_with(e)
    return e.mm_extract_policies(s.starts.starts)


@pytest.mark.parametrize("name", ["A", "B"])
def test_policies(eng_mod, side, planned, name):
    """the walks from node 0, every copy and 50 drawn starts against policies_ref on the ORACLE's graph: status for status (the walk
    ends exactly where the restatement's does, and returns onto its own path exactly where the reference would not end), ids,
    parents, leaves, costs and states bit for bit"""
    s, (e, _) = side(name), planned(name)
    st = s.starts
    ok, own = M.assert_statuses(name, st)
    got, status = extracted(e, s)
    assert_answers(got, status, st.want, "input " + name)
    for g in got:
        if g is not None:
            assert np.array_equal(bits(g[0][3]), bits(s.bg["xy"][g[0][0].astype(np.int64)]))
    # one start whose walk returns onto its own path, in a call of its own
    q2 = int(np.flatnonzero(st.status == policies_ref.OWN_PATH)[0])
    alone, status_alone = e.mm_extract_policies([st.starts[q2]])
    assert status_alone.tolist() == [policies_ref.OWN_PATH] and alone[0] is None
    # node 0: the single call answers as the batch does; which of the two it is comes from the reference
    if st.status[0] == policies_ref.OWN_PATH:
        with pytest.raises(eng_mod.PorrtError, match="returns to a belief node on its own path"):
            e.mm_extract_policy()
    else:
        assert st.status[0] == policies_ref.OK
        (oid, par, leaf, xy), cost = e.mm_extract_policy()
        (oid_b, par_b, leaf_b, xy_b), cost_b = got[0]
        assert np.array_equal(oid, oid_b) and np.array_equal(par, par_b) and np.array_equal(leaf, leaf_b)
        assert xy.tobytes() == xy_b.tobytes() and bits([cost])[0] == bits([cost_b])[0] == bits([s.dist[0]])[0]


# ---------------------------------------------------------------------------------------------------------------- refinement
def check_refined(e, s, n, restated):
    """mm_refine_policies(n) of the start list's policies: the positions in `restated` against refine_ref on the oracle's policy,
    every start without a policy status 1 and None, start 0 equal to the single call"""
    st = s.starts
    got, status = e.mm_refine_policies(n)
    assert len(got) == len(st.starts) == len(status)
    for q, want_status in enumerate(st.status):
        if want_status != policies_ref.OK:
            assert status[q] == 1 and got[q] is None, q
        else:
            assert status[q] == 0 and got[q] is not None, q
    for q in restated:
        assert_same_refined(got[q], s.refined(q, n))
    e.mm_extract_policy()
    assert_same_refined(got[0], e.mm_refine_policy(n))


@pytest.mark.parametrize("n", [0, 1, 200])
def test_refined_policies_a(side, planned, n):
    """every status-0 policy of A's start list, zero-length steps among them (a shortcut between two copies divides nothing by their
    distance: lambda is a ratio of indices)"""
    s, (e, _) = side("A"), planned("A")
    st = s.starts
    handed = st.refiner_policies(s.bg, M.REFINED_A)
    assert len(handed) == M.REFINED_A
    assert sum(M.zero_length_steps(s.bg, st.want[q][1]) for q, _ in handed) >= M.FLOORS["A"]["refiner_zero_steps"]
    extracted(e, s)
    check_refined(e, s, n, [int(q) for q in np.flatnonzero(st.status == policies_ref.OK)])


def test_refined_policies_b(side, planned):
    """B at 200 iterations: node 0's policy and the first 16 status-0 policies from copies against the restatement"""
    s, (e, _) = side("B"), planned("B")
    st = s.starts
    handed = st.refiner_policies(s.bg, M.REFINED_B)
    assert len(handed) == M.REFINED_B and sum(M.zero_length_steps(s.bg, st.want[q][1]) for q, _ in handed) > 0
    extracted(e, s)
    check_refined(e, s, 200, [0] + [q for q, _ in handed])
