"""Python restatement of MapShelfDomainTampRRT::plan(.., TampSearch::BranchAndBound) (src/map_shelves_tamp_rrt.rs:159-291): the
yardstick of the device planner (porrt_tamp_rrt_plan, Engine.plan_tamp_rrt).

TEST INFRASTRUCTURE ONLY, built on the CPU oracle alone: every RRT query is Oracle.grow(.., algo=ALGO_BATCHED_KD) and
Oracle.best_solution (rrt.rs:88-193), the shuffles draw from an orc.Pcg64, the shortcut checks segments with
Oracle.traversed_class.  Never imported by the product package po_rrt_amd.

Two stream modes:
  streams = 0  one continuous stream across every query of the search, in the reference's order (its one RRT object, :196)
  streams = 1  one stream per search edge: an edge's two queries run on a stream seeded with edge_seed(h0, zone prefix)
and a wave width: up to `wave` nodes are popped from the top of the stack, their children made in the sequential order, all their
queries run, then the children are pushed and the leaves recorded in the sequential order.  wave = 1 is the reference's loop.
"""
import math

import numpy as np

from oracle import orc

M64 = (1 << 64) - 1
SHORTCUT_ITERATIONS = 100           # map_shelves_tamp_rrt.rs:581


class NoPath(RuntimeError):
    """a query without a solution: the reference panics (expect("no observation path found!") / "no pickup path found!")"""

    def __init__(self, node, zone, which):
        super().__init__("no %s path found (search node %d, zone %d)" % (which, node, zone))
        self.node, self.zone, self.which = node, zone, which


class RasterFault(RuntimeError):
    """a segment the traversed-space walk cannot classify: the reference panics"""


def splitmix64(x):
    """SplitMix64's output function on x + golden gamma"""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def edge_seed(h0, prefix):
    """h_0 = the planner's sampler seed, h_k = splitmix64(h_{k-1} ^ (z_k + 1)) along the zone prefix of a search edge"""
    h = h0 & M64
    for z in prefix:
        h = splitmix64(h ^ (int(z) + 1))
    return h


def shuffled(vector, rng):
    """:20-32: draw an index, push it, swap_remove it"""
    to = list(vector)
    out = []
    while to:
        i = rng.gen_range_usize(0, len(to))
        out.append(to[i])
        to[i] = to[-1]
        to.pop()
    return out


def normalize(b):
    s = 0.0
    for p in b:
        s = s + p
    return [p / s for p in b]


def transition_probability(parent, child):
    """common.rs:188-190"""
    s = 0.0
    for p, q in zip(child, parent):
        s = s + (q if p > 0.0 else 0.0)
    return s


def check_belief_state(b):
    """common.rs:390-392"""
    s = 0.0
    for p in b:
        s = s + p
    return abs(s - 1.0) < 0.001


def shortcut_draws(length, n_iterations=SHORTCUT_ITERATIONS):
    """the (joint, s, e) sequence of shortcut (:578-584): DiscreteSampler::new() is Pcg64 seed 0 -- partial_shortcut's sequence"""
    rng = orc.Pcg64.seed_from_u64(0)
    out = []
    for _ in range(n_iterations):
        joint = rng.gen_range_usize(0, 2)
        s = rng.gen_range_usize(0, length - 2)
        e = s + 2 + rng.gen_range_usize(0, length - s - 2)
        out.append((joint, s, e))
    return out


def free_segment(o, a, b):
    """RTTFuncs::transition_validator of the planner (:43-45): the traversed space is Free"""
    cls = o.traversed_class(a, b)
    if cls < 0:
        raise RasterFault("class %d" % cls)
    return cls == orc.FREE


def shortcut(o, path, n_iterations=SHORTCUT_ITERATIONS):
    """:565-617.  Only the transitions among the candidates are checked: the step from the last candidate into node e is not."""
    states = [list(map(float, s)) for s in path]
    if len(states) <= 2:
        return states
    for joint, s, e in shortcut_draws(len(states), n_iterations):
        a, b = states[s][joint], states[e][joint]
        cand = []
        for j in range(s, e):
            lam = float(j - s) / float(e - s)
            c = list(states[j])
            c[joint] = a * (1.0 - lam) + b * lam
            cand.append(c)
        ok = True
        for k in range(len(cand) - 1):                       # should_commit && ...: stops at the first rejection
            ok = ok and free_segment(o, cand[k], cand[k + 1])
        if ok:
            for j in range(s, e):
                states[j] = cand[j - s]
    return states


def find_unchecked_path(o, tries=20000, seed=7):
    """a 3-state path whose shortcut commits a candidate that reaches its last state across an obstacle: with 3 states every draw
    is s = 0, e = 2, so only the step from node 0 to the moved node 1 is checked.  Found by a seeded search over the map."""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        a = rng.uniform(-0.95, 0.95, 2)
        c = a + rng.uniform(-0.3, 0.3, 2)
        b = (a + c) / 2 + rng.uniform(-0.2, 0.2, 2)
        path = [a.tolist(), b.tolist(), c.tolist()]
        if np.any(np.abs(c) > 0.99) or o.state_class(a) != orc.FREE or o.state_class(c) != orc.FREE:
            continue
        try:
            out = shortcut(o, path)
        except RasterFault:
            continue
        if out[1] != path[1] and o.traversed_class(out[1], out[2]) not in (orc.FREE,) and o.traversed_class(out[1], out[2]) >= 0:
            return path
    raise RuntimeError("no such path found")


def policy_expected_cost(xy, parents, beliefs):
    """Policy::compute_expected_costs_to_goals (common.rs:131-154): children in ascending id order, cost = norm2"""
    n = len(parents)
    if n == 0:
        return 0.0
    children = [[] for _ in range(n)]
    for k in range(1, n):
        if parents[k] >= 0:
            children[int(parents[k])].append(k)

    def rec(p, u):
        acc = 0.0
        for c in children[u]:
            q = transition_probability(beliefs[u], beliefs[c])
            d2 = 0.0
            dx = xy[c][0] - xy[u][0]
            d2 += dx * dx
            dx = xy[c][1] - xy[u][1]
            d2 += dx * dx
            acc += p * q * math.sqrt(d2) + rec(p * q, c)
        return acc

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * n + 100))
    try:
        return rec(1.0, 0)
    finally:
        sys.setrecursionlimit(old)


def build_policy(o, chain, n_iterations=SHORTCUT_ITERATIONS):
    """:619-663 on the search nodes root .. best leaf.  A node is a dict with target, belief, path_obs, path_pick.
    Returns dict(xy [n,2], parents, is_leaf, beliefs [n, n_worlds], expected_cost)."""
    xy, parents, leaf, beliefs = [], [], [], []

    def add(state, belief, is_leaf):
        xy.append([float(state[0]), float(state[1])])
        parents.append(-1)
        leaf.append(1 if is_leaf else 0)
        beliefs.append(list(belief))
        return len(xy) - 1

    last_obs = 0
    for sn in chain:
        prev = last_obs
        for state in shortcut(o, sn["path_obs"], n_iterations):
            nid = add(state, sn["belief"], False)
            if nid != prev:
                parents[nid] = prev
            prev = nid
        last_obs = prev
        pick = shortcut(o, sn["path_pick"], n_iterations)
        if pick:
            b = [p if w == sn["target"] else 0.0 for w, p in enumerate(sn["belief"])]
            b = normalize(b)
        for i, state in enumerate(pick):
            nid = add(state, b, i == len(sn["path_pick"]) - 1)
            if nid != prev:
                parents[nid] = prev
            prev = nid
    xy = np.array(xy, dtype=np.float64).reshape(-1, 2)
    beliefs = np.array(beliefs, dtype=np.float64).reshape(len(parents), -1) if parents else np.zeros((0, 0))
    cost = policy_expected_cost(xy, parents, beliefs)
    return dict(xy=xy, parents=np.array(parents, dtype=np.int64), is_leaf=np.array(leaf, dtype=np.uint8), beliefs=beliefs,
                expected_cost=cost)


class Planner:
    """MapShelfDomainTampRRT on one oracle context `o` (grid, zones, sampler box already set).  seed = the planner's continuous
    sampler seed (h_0 of the per-edge streams); the discrete sampler (shuffles) is a Pcg64 of that seed that persists across plans,
    as the engine's porrt_set_sampler seeds both."""

    def __init__(self, o, seed, low=(-1.0, -1.0), up=(1.0, 1.0), goal_radius=0.05):
        self.o, self.seed, self.low, self.up, self.goal_radius = o, seed, low, up, goal_radius
        self.drng = orc.Pcg64.seed_from_u64(seed)

    def _query(self, start, goal, zone, p):
        o = self.o
        if goal == "observation":
            o.set_observation_goal(zone)
        else:
            zp = o.zone_positions()[zone]
            o.set_square_goal(np.array([zp]), np.array([1], dtype=np.uint64), self.goal_radius)
        o.grow(start, p["max_step"], p["search_radius"], p["n_iter_min"], p["n_iter_max"], batch_K=p["K"], algo=orc.ALGO_BATCHED_KD)
        return o.best_solution()

    def plan(self, start, belief, max_step=0.1, search_radius=2.0, n_iter_min=2500, n_iter_max=10000, K=128, streams=1, wave=1):
        o = self.o
        nz = o.n_zones()
        if len(belief) != nz or not check_belief_state(belief):
            raise ValueError("invalid prior")
        p = dict(max_step=max_step, search_radius=search_radius, n_iter_min=n_iter_min, n_iter_max=n_iter_max, K=K)
        if streams == 0:
            wave = 1
            o.set_sampler(self.low, self.up, self.seed)          # RRT::new(self.continuous_sampler.clone(), ..) (:196)
        start = (float(start[0]), float(start[1]))
        root = dict(id=0, target=None, parent=None, remaining=shuffled(range(nz), self.drng), obs_state=start, path_obs=[],
                    path_pick=[], rp=1.0, belief=[float(x) for x in belief], ec=0.0, prefix=())
        nodes = [root]
        stack = [0]
        best = math.inf
        best_leaf = None
        stats = dict(queries=0, waves=0, pruned=0)
        while stack:
            popped = [stack.pop() for _ in range(min(wave, len(stack)))]
            stats["waves"] += 1
            made = []                                        # (u, child) in the sequential order
            for uid in popped:
                u = nodes[uid]
                kids = []
                for t in u["remaining"]:
                    rem = [z for z in shuffled(u["remaining"], self.drng) if z != t]
                    vb = list(u["belief"])
                    if u["target"] is not None:
                        vb[u["target"]] = 0.0
                    vb = normalize(vb)
                    rp = u["rp"] * transition_probability(u["belief"], vb)
                    v = dict(id=len(nodes), target=t, parent=uid, remaining=rem, rp=rp, belief=vb, prefix=u["prefix"] + (t,))
                    nodes.append(v)
                    kids.append(v)
                made.append((u, kids))
            for u, kids in made:
                for v in kids:
                    if streams == 1:                         # the edge's two queries back to back on its own stream
                        o.set_sampler(self.low, self.up, edge_seed(self.seed, v["prefix"]))
                    for which in ("observation", "pickup"):
                        st = u["obs_state"] if which == "observation" else v["obs_state"]
                        r = self._query(st, which, v["target"], p)
                        stats["queries"] += 1
                        if r is None:
                            raise NoPath(v["id"], v["target"], which)
                        path, cost = r
                        if which == "observation":
                            v["path_obs"], v["obs_cost"] = path, cost
                            v["obs_state"] = (float(path[-1][0]), float(path[-1][1]))
                        else:
                            v["path_pick"], v["pick_cost"] = path, cost
            for u, kids in made:
                for v in kids:
                    v["ec"] = u["ec"] + v["rp"] * (v["obs_cost"] + v["belief"][v["target"]] * v["pick_cost"])
                    if v["ec"] < best:
                        stack.append(v["id"])
                    else:
                        stats["pruned"] += 1
                if not u["remaining"]:
                    if u["ec"] < best:
                        best = u["ec"]
                    if best_leaf is None or u["ec"] <= best_leaf["ec"]:     # BTreeMap insert: the last of equal keys stays
                        best_leaf = u
        if streams == 0:
            o.set_sampler(self.low, self.up, self.seed)
        chain = []
        n = best_leaf
        while n is not None:
            chain.append(n)
            n = nodes[n["parent"]] if n["parent"] is not None else None
        chain.reverse()
        pol = build_policy(o, chain)
        pol.update(search_cost=best_leaf["ec"], zone_order=list(best_leaf["prefix"]), search_nodes=len(nodes), **stats)
        return pol
