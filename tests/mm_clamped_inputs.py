"""Inputs on which the multi-modal PRM meets exact ties through its public interface alone, and the counters that show, on the
oracle's output, which ties an input made.  TEST INFRASTRUCTURE ONLY.  Plain numpy with fixed seeds.

grow_mm_prm accepts no injected samples: every mode draws from a clone of the sampler.  But sample_observation_of_zone
(map_shelves_tamp_prm.rs) clamps each observation sample to [low, up - 0.0001] of the SAMPLER's window, so a window narrower than the
map's box (set_sampler after set_grid with the map's own box) sends every sample clamped on both axes to one corner point: a
mode's roadmap then holds bit-identical nodes, runs of equal x and of equal y (a kd chain: strictly less goes left, equal goes
right), zero-length edges between the copies, and its belief graph equal-cost children and zero-length cycles -- on which the
reference's extract_policy does not end.

cases.configure hands a case's `low` / `up` to set_grid too; with the window on the grid the root of input A has no finite cost and
nothing is tested.  So the window is kept under other names (window_low / window_up) and applied by set_sampler alone."""
import numpy as np

import cases
import mm_plan_ref
import policies_ref


# ---------------------------------------------------------------------------------------------------------------------- the inputs
def _bench(zones, seed):
    c = cases.cfg2(10)
    c.update(zones=zones, visibility=0.5, seed=seed)
    return c


def input_a():
    """two goal zones on the benchmark map: 3 modes, 3123 nodes"""
    return cases.Case(_bench("map_benchmark_like_2_goals_zone_ids", 0), name="A", window_low=(-0.9, -1.0), window_up=(0.9, 0.2),
                      prior=[0.5, 0.5], max_step=0.1, search_radius=2.0, n_per_belief=1000, discrete_seed=0)


def input_b():
    """four free zones: 15 modes, 32 205 nodes, modes above and below the level kernel's LDS limit"""
    return cases.Case(_bench("map_benchmark_like_4_free_zone_ids", 1), name="B", window_low=(-0.9, -1.0), window_up=(0.9, 0.9),
                      prior=[0.25] * 4, max_step=0.1, search_radius=2.0, n_per_belief=2000, discrete_seed=1)


def input_c():
    """cases.cfg4, twelve shelves: 1364 modes, most of them smaller than a wave; the root has no finite cost"""
    return cases.Case(cases.cfg4(1500, 1500), name="C", window_low=(-0.85, -1.0), window_up=(0.85, 0.85),
                      prior=[1.0 / 12] * 12, max_step=0.05, search_radius=5.0, n_per_belief=20, discrete_seed=0)


INPUTS = {"A": input_a, "B": input_b, "C": input_c}


def configure(eng, inp):
    """an engine or an oracle (the method names are the same on both): the map's own box on the grid, the window on the sampler"""
    assert "low" not in inp and "up" not in inp, "cases.configure would put the window on the grid as well"
    cases.configure(eng, inp)
    eng.set_sampler(inp.window_low, inp.window_up, inp.seed)
    eng.set_discrete_seed(inp.discrete_seed)
    return eng


def grow(eng, inp, prior=None):
    return eng.grow_mm_prm(inp.start, inp.prior if prior is None else prior, inp.max_step, inp.search_radius, inp.n_per_belief)


def plan(oracle, inp):
    """mm_plan_ref.plan on a configured oracle: (grow dict, belief graph, expected costs)"""
    return mm_plan_ref.plan(oracle, inp.start, inp.prior, inp.max_step, inp.search_radius, inp.n_per_belief)


# ---------------------------------------------------------------------------------------------------------------------- counters
def place_counts(xy):
    """per node, the number of nodes of xy (itself included) at its place, bit for bit"""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    if len(xy) == 0:
        return np.zeros(0, dtype=np.int64)
    _, inverse, counts = np.unique(xy.view(np.uint64), axis=0, return_inverse=True, return_counts=True)
    return counts[inverse.reshape(-1)]


def duplicates_per_mode(g):
    """per mode, the nodes that share their place with another node of the mode"""
    return np.array([int(np.count_nonzero(place_counts(m["xy"]) > 1)) for m in g["modes"]], dtype=np.int64)


def multiplicity_per_mode(g):
    """per mode, the largest number of nodes at one place (0 for an empty mode)"""
    return np.array([int(place_counts(m["xy"]).max()) if len(m["xy"]) else 0 for m in g["modes"]], dtype=np.int64)


def largest_multiplicity(g):
    return int(multiplicity_per_mode(g).max())


def longest_equal_run(g, axis):
    """the most nodes of one mode with one value of coordinate `axis`: inserted in id order they hang below one another in the
    mode's kd-tree (equal goes right at the levels that split on this axis)"""
    best = 0
    for m in g["modes"]:
        if len(m["xy"]):
            best = max(best, int(np.unique(np.asarray(m["xy"])[:, axis].view(np.uint64), return_counts=True)[1].max()))
    return best


def mode_sizes(g):
    return np.array([len(m["xy"]) for m in g["modes"]], dtype=np.int64)


def zero_length_child_edges(bg):
    """edges of the belief graph, in children order, between two nodes at one place: (count of all of them, count of those inside a
    mode -- action edges between copies; the others are observation edges, which keep the state)"""
    xy = bg["xy"].view(np.uint64)
    total = inside = 0
    for u, row in enumerate(bg["children"]):
        if row:
            r = np.asarray(row, dtype=np.int64)
            same = (xy[r] == xy[u]).all(axis=1)
            total += int(same.sum())
            inside += int((same & (bg["belief_vec"][r] == bg["belief_vec"][u])).sum())
    return total, inside


def duplicate_nodes(bg):
    """belief nodes that share their place with another node of their mode, ascending"""
    off = bg["mode_offsets"].astype(np.int64)
    out = []
    for k in range(len(off) - 1):
        out.extend((off[k] + np.flatnonzero(place_counts(bg["xy"][off[k]:off[k + 1]]) > 1)).tolist())
    return out


def counters(g, bg):
    dup = duplicates_per_mode(g)
    zero, inside = zero_length_child_edges(bg)
    return dict(modes=len(g["modes"]), nodes=int(mode_sizes(g).sum()), duplicates=int(dup.sum()), modes_with_duplicates=int((dup > 0).sum()),
                multiplicity=largest_multiplicity(g), equal_x=longest_equal_run(g, 0), equal_y=longest_equal_run(g, 1),
                zero_length_edges=zero, zero_length_action_edges=inside)


# ---------------------------------------------------------------------------------------------------------------------- policies
def reference_graph(bg):
    """the policies_ref.Graph of the oracle's belief graph"""
    return policies_ref.graph_of_lists(bg["xy"], bg["belief_vec"], bg["beliefs"], bg["belief_ids"], bg["children"])


def candidate_starts(bg):
    """node 0, every duplicate node in ascending id, then 50 drawn starts"""
    return [0] + duplicate_nodes(bg) + np.random.default_rng(5).integers(0, len(bg["xy"]), size=50).tolist()


class Starts:
    """the start list of a policy test and what policies_ref.extract_policies answers for it on the oracle's graph.
    starts: node 0, the duplicate nodes in ascending id (starts[1 : 1 + n_duplicates]), then the drawn ones; want: (status, policy,
    cost) per start; dropped: the candidates left out.  A candidate for which the restatement answers status 3 (an assertion of the
    reference) or 4 (capacity) is dropped: those statuses have tests of their own, and a start is in this list for the walk it
    makes.  The rule is the status, never a position in the list; node 0 is never dropped."""

    def __init__(self, bg, dist):
        dup = duplicate_nodes(bg)
        cand = candidate_starts(bg)
        want = policies_ref.extract_policies(reference_graph(bg), dist, cand)
        keep = [q for q, w in enumerate(want) if q == 0 or w[0] not in (policies_ref.ASSERT, policies_ref.CAPACITY)]
        self.starts, self.want = [cand[q] for q in keep], [want[q] for q in keep]
        self.dropped = [cand[q] for q in range(len(cand)) if q not in set(keep)]
        self.n_duplicates = sum(1 for q in keep if 1 <= q <= len(dup))
        self.status = np.array([w[0] for w in self.want], dtype=np.uint8)

    def duplicate_statuses(self):
        return self.status[1:1 + self.n_duplicates]

    def refiner_policies(self, bg, count):
        """the first `count` status-0 policies from duplicate starts: [(position in starts, policy arrays)]"""
        qs = [q for q in range(1, 1 + self.n_duplicates) if self.status[q] == policies_ref.OK][:count]
        return [(q, policy_arrays(bg, self.want[q][1])) for q in qs]


def policy_arrays(bg, pol):
    """a policy of policies_ref as the refiner's restatement takes it: (states, parents, original ids, belief rows)"""
    oid, par, _ = pol
    i = oid.astype(np.int64)
    return bg["xy"][i], par, oid, bg["belief_vec"][i]


def zero_length_steps(bg, pol):
    """policy nodes at the place of their parent"""
    xy, par, _, _ = policy_arrays(bg, pol)
    k = np.flatnonzero(par >= 0)
    return int((xy[k].view(np.uint64) == xy[par[k]].view(np.uint64)).all(axis=1).sum())


# ---------------------------------------------------------------------------------------------------------------------- the floors
# Under what the oracle gives today (see the table in tests/test_mm_clamped_cpu.py), so that an unrelated change of a seed or of a
# map shows up as a failed floor and does not quietly empty the GPU tests.
FLOORS = {
    "A": dict(duplicates=40, multiplicity=8, zero_length_edges=200, status_ok=10, status_own_path=10, refiner_zero_steps=5),
    "B": dict(duplicates=60, status_ok=20, status_own_path=20),
    "C": dict(modes=1000, small_modes_with_duplicates=5, multiplicity=65),
}
REFINED_A = 12           # the first status-0 policies from duplicate starts handed to the refiner on A
REFINED_B = 16           # ... on B
LDS_LIMIT = 2000         # B has modes above and below: both paths of the level kernel in one launch
WAVE = 64


def assert_ties(name, g, bg):
    """the floors that need the growth and the belief graph alone; returns the counters"""
    c, f = counters(g, bg), FLOORS[name]
    sizes, dup = mode_sizes(g), duplicates_per_mode(g)
    if name in ("A", "B"):
        assert c["duplicates"] >= f["duplicates"], c
    if name == "A":
        assert c["multiplicity"] >= f["multiplicity"] and c["zero_length_edges"] >= f["zero_length_edges"], c
    if name == "B":
        assert sizes.max() > LDS_LIMIT and sizes.min() < LDS_LIMIT, sizes
    if name == "C":
        assert c["modes"] >= f["modes"] and c["multiplicity"] >= f["multiplicity"], c
        assert int(((sizes < WAVE) & (dup > 0)).sum()) >= f["small_modes_with_duplicates"]
        assert (sizes == 1).any()
    assert c["equal_x"] >= c["multiplicity"] and c["equal_y"] >= c["multiplicity"]
    return c


def assert_statuses(name, st):
    """the floors on the policies from the duplicate starts of a Starts; returns (status-0 count, status-2 count) among them"""
    d = st.duplicate_statuses().tolist()
    ok, own = d.count(policies_ref.OK), d.count(policies_ref.OWN_PATH)
    assert ok >= FLOORS[name]["status_ok"] and own >= FLOORS[name]["status_own_path"], (ok, own)
    return ok, own
