"""Crafted trees for the tree read-outs -- k_best_cost, k_best_path, k_solutions_select / k_solutions_write and the host code that hangs
on them -- and the counters that state, from a finished tree, what such a tree holds.  Shared by tests/test_readout_inputs_cpu.py (the
oracle's side: every condition a case was built for is asserted there) and tests/test_gpu_readouts.py (the device against the oracle).

Every case is an RRT* growth in empty space at batch_K = 1 fed an injected stream (set_samples).  Every sample lies within max_step
(L1) of its nearest node and nothing is invalid, so every iteration makes a node and the node of iteration i has id i.  Every 100th
iteration takes the goal point of world 0 and draws nothing (rrt.rs:176-181): its node is steered, and Stream leaves its id out.  The
cases with small goals list a decoy goal first (mask 1, so world 0's), behind the root and never reached: the steered nodes then form
a branch of their own from the root and touch nothing else.  The combs cannot (one L1 radius serves all goals of a context): their
steered nodes walk from the chain towards the goal's centre, inside the goal, and are counted with the rest.

All coordinates are multiples of S / 64 with S = 2^-10 = max_step, so differences, their squares and the sums of two squares are
exact, `norm2 <= radius` meets equality on a chain of pitch S, and mirror images have bit-equal costs.  heuristic_radius is max_step
itself from the second node on (search_radius 1 puts the uncapped radius above 0.05 up to several thousand nodes)."""
import numpy as np

import cases
import solutions_ref

S = 2.0 ** -10                              # max_step of every case (one porrt_grow_batch has one max_step), and the chains' pitch
SEARCH_RADIUS = 1.0
SLOT = 1024                                 # kTampPathSlot (porrt_tamp.hpp): states of one best path that porrt_best_paths hands out
BEST_COST_THREADS = 1024                    # k_best_cost: thread t folds the final nodes t, t + 1024, ...
SOLUTION_THREADS = 256                      # kSolThreads (porrt_solutions.hpp): solutions of a row per trip of both kernels


def scratch_bound(n_iter_max):
    """ints of k_best_cost's path scratch on a fresh context: porrt_ctx::grow_once's `d_bcscratch.reserve(8 * Nmax + 4096)` with
    Nmax = n_iter_max + 2 (porrt_engine.hip).  The final nodes' path lengths summed beyond it is BestCost::overflow."""
    return 8 * (n_iter_max + 2) + 4096


# ---------------------------------------------------------------------------------------------------------------------- streams
class Stream:
    """the injected samples of a growth in which every iteration makes a node: add() returns the id its point will have"""

    def __init__(self):
        self.points, self.iteration = [], 0

    def add(self, x, y):
        self.iteration += 1
        if self.iteration % 100 == 0:           # the goal point's iteration: it makes a node of its own
            self.iteration += 1
        self.points.append((float(x), float(y)))
        return self.iteration

    def fill_to(self, node_id, walker):
        """points of `walker` until the next id is node_id"""
        while self._next() < node_id:
            self.add(*next(walker))
        assert self._next() == node_id, "id %d is a goal point's" % node_id

    def _next(self):
        return self.iteration + (2 if (self.iteration + 1) % 100 == 0 else 1)

    def xy(self):
        return np.ascontiguousarray(np.array(self.points, dtype=np.float64).reshape(-1, 2))


def walk(x, y, dx, dy):
    """(x, y) + k * (dx, dy), k = 1, 2, ..."""
    k = 0
    while True:
        k += 1
        yield x + k * dx, y + k * dy


def _case(name, start, goals, masks, l1, stream, **marks):
    c = cases.empty_space(stream.iteration, stream.iteration)
    c.update(name=name, start=start, goals=goals, masks=masks, l1=l1, max_step=S, search_radius=SEARCH_RADIUS, samples=stream.xy(), **marks)
    return c


# ---------------------------------------------------------------------------------------------------------------------- the cases
COMB_L1 = 0.875


def comb(teeth, name=None):
    """Staircase comb: a chain that alternates (+S, 0) and (0, +S) just outside the edge x - y = 0.875 of the goal (an L1 ball at the
    origin), from the goal's lower corner on; a tooth (0, +S / 2) hangs off every second chain node, inside the goal.  A tooth has one
    node within the radius, its chain node, which is not final: every tooth is a solution.  The steered nodes of the goal point's
    iterations add a few more (those that leave from the chain)."""
    assert teeth <= 890
    st = Stream()
    x, y = 0.0, -COMB_L1 - S / 4
    start = (x, y)
    for _ in range(teeth):
        st.add(x, y + S / 2)
        x += S
        st.add(x, y)
        y += S
        st.add(x, y)
    return _case(name or "comb_%d" % teeth, start, [(0.0, 0.0)], [1], COMB_L1, st, teeth=teeth)


GOAL_L1 = S / 4                             # the small goals: a point S / 2 from a chain's tip is in, the tip is not
CORRIDOR_X0 = -0.75                         # the corridors' roots are (CORRIDOR_X0, 0)
DECOY_BEHIND = 0.25                         # the decoy goal lies this far behind the root (256 steps; a run has some 20 goal iterations)


def corridor(depth, finals, name):
    """A chain of `depth` nodes along y = 0 at pitch S from the root (x0, 0), then final nodes about its tip.  `finals`: (node id or
    None for the next, "up" | "down" | "up_copy" | "down_copy") -- the points tip + (S / 2, +-S / 2), each the centre of a goal of its
    own (a copy shares it), each with the tip as its only cheaper parent: mirror images at bit-equal cost.  Up to a wanted id the
    stream walks a side branch from the root along -y."""
    st, x0 = Stream(), CORRIDOR_X0
    for k in range(1, depth + 1):
        st.add(x0 + k * S, 0.0)
    tip = x0 + depth * S
    side = walk(x0, 0.0, 0.0, -S)
    at = {"up": (tip + S / 2, S / 2), "down": (tip + S / 2, -S / 2)}
    ids, goals, masks = [], [(x0 - DECOY_BEHIND, 0.0)], [1]
    for node_id, where in finals:
        if node_id is not None:
            st.fill_to(node_id, side)
        p = at[where.split("_")[0]]
        ids.append(st.add(*p))
        if p not in goals:
            goals.append(p)
            masks.append(1 << len(masks))
    return _case(name, (x0, 0.0), goals, masks, GOAL_L1, st, depth=depth, tied=ids)


def fan(depth, n_fan, name):
    """Corridor and fan: the chain of corridor(), then n_fan final nodes on a grid of pitch S / 64 about tip + (S / 2, 0), all inside
    the one goal there and all within the radius of the tip: n_fan final nodes of depth + 2 states or more."""
    st, x0 = Stream(), CORRIDOR_X0
    for k in range(1, depth + 1):
        st.add(x0 + k * S, 0.0)
    cx = x0 + depth * S + S / 2
    g = S / 64
    cells = sorted(((abs(i) + abs(j), i, j) for i in range(-15, 16) for j in range(-15, 16) if abs(i) + abs(j) < 16))
    assert n_fan <= len(cells)
    order = np.random.default_rng(7).permutation(n_fan)
    for k in order:
        _, i, j = cells[k]
        st.add(cx + i * g, j * g)
    return _case(name, (x0, 0.0), [(x0 - DECOY_BEHIND, 0.0), (cx, 0.0)], [1, 2], GOAL_L1, st, depth=depth, n_fan=n_fan)


def start_in_goal(n_ring=64, n_outer=30):
    """The root at the goal's centre: n_ring children on the L1 sphere of radius S about it (no two in line with the root, so the root
    is every one's parent), then n_outer points further out whose parents are ring nodes.  Every node is final but the root, which is
    never pushed (rrt.rs:165-167): the ring nodes are the solutions, of two states each.  Fewer than 100 iterations: no goal point."""
    assert n_ring % 4 == 0 and n_ring + n_outer < 100
    st, q = Stream(), n_ring // 4
    ring = []
    for k in range(n_ring):
        a, side = k % q, k // q
        u, v = a * S / q, S - a * S / q                  # u + v = S
        ring.append([(u, v), (v, -u), (-u, -v), (-v, u)][side])
    for k in np.random.default_rng(3).permutation(n_ring):
        st.add(*ring[k])
    for k in range(n_outer):
        u, v = ring[(k * 7) % n_ring]
        st.add(1.5 * u, 1.5 * v)
    return _case("start_in_goal", (0.0, 0.0), [(0.0, 0.0)], [1], 0.25, st, n_ring=n_ring)


def no_goal(n=150):
    """a chain that never comes near its goal: no final node"""
    st = Stream()
    side = walk(-0.75, 0.0, 0.0, -S)
    for _ in range(n):
        st.add(*next(side))
    return _case("no_goal", (-0.75, 0.0), [(0.5, 0.5)], [1], GOAL_L1, st)


# solution counts: a comb's solutions are its teeth and the steered nodes that leave from the chain (the CPU file pins the counts)
COMB_256, COMB_257, COMB_3_TRIPS = 249, 250, 530
CASES = {
    "comb_256": lambda: comb(COMB_256, "comb_256"),
    "comb_257": lambda: comb(COMB_257, "comb_257"),
    "comb_3_trips": lambda: comb(COMB_3_TRIPS, "comb_3_trips"),
    "start_in_goal": start_in_goal,
    "no_goal": no_goal,
    # k_best_cost's scratch: the fan beyond it, the small fan far below it
    "fan_overflow": lambda: fan(400, 120, "fan_overflow"),
    "fan_fits": lambda: fan(40, 24, "fan_fits"),
    # ties at the minimum: a < b with a % 1024 > b % 1024; b - a = 1024; three, of which two in one thread
    "tie_lower_thread": lambda: corridor(985, [(1001, "up"), (1030, "down")], "tie_lower_thread"),
    "tie_same_thread": lambda: corridor(40, [(50, "up"), (50 + 1024, "down")], "tie_same_thread"),
    "tie_three": lambda: corridor(30, [(40, "up"), (70, "down"), (40 + 1024, "down_copy")], "tie_three"),
    # the slot of a best path: exactly 1024 states and one more (root, the chain, the final node)
    "path_1024": lambda: corridor(SLOT - 2, [(None, "up"), (None, "down")], "path_1024"),
    "path_1025": lambda: corridor(SLOT - 1, [(None, "up"), (None, "down")], "path_1025"),
}
SOLUTION_CASES = ("comb_256", "comb_257", "comb_3_trips", "start_in_goal", "no_goal")
TIE_CASES = ("tie_lower_thread", "tie_same_thread", "tie_three")
BATCH_ROWS = ("comb_257", "no_goal", "tie_three", "fan_overflow", "comb_3_trips", "start_in_goal")


def case(name):
    return CASES[name]()


def grow_oracle(c):
    """the oracle's tree of a case (the contract at K = 1, kd-accelerated, as the GPU files compare against)"""
    from oracle import orc
    o = cases.configure(orc.Oracle(), c)
    o.set_samples(c.samples)
    cases.grow(o, c, K=1, algo=orc.ALGO_BATCHED_KD)
    return o


# ---------------------------------------------------------------------------------------------------------------------- counters
def depths(parent):
    """states of the path root .. node, for every node (a parent may have a higher id than its child: rewires)"""
    parent = np.asarray(parent).astype(np.int64)
    d = np.zeros(len(parent), dtype=np.int64)
    for i in range(len(parent)):
        chain, p = [], i
        while p >= 0 and d[p] == 0:
            chain.append(p)
            p = int(parent[p])
        base = d[p] if p >= 0 else 0
        for k, q in enumerate(reversed(chain), 1):
            d[q] = base + k
    return d


class Counters:
    """what the read-outs meet on a tree: (xy, parent) and its final ids in push order"""

    def __init__(self, xy, parent, final_ids):
        self.final_ids = [int(f) for f in final_ids]
        self.depth = depths(parent)
        self.firstly_final = solutions_ref.firstly_final_ids(parent, final_ids)
        self.n_solutions = len(self.firstly_final)
        self.final_states = int(sum(self.depth[f] for f in self.final_ids))               # what k_best_cost asks of its scratch
        self.solution_states = int(sum(self.depth[f] for f in self.firstly_final))
        costs = np.array([solutions_ref.path_cost(solutions_ref.path_to(xy, parent, f)) for f in self.final_ids], dtype=np.float64)
        self.costs = costs
        if len(costs):
            bits = costs.view(np.uint64)
            self.min_ids = [f for f, b in zip(self.final_ids, bits) if b == bits.min()]   # costs are >= 0: bits order like values
            self.best_cost = float(costs.min())
            self.best_len = int(self.depth[self.min_ids[0]])
        else:
            self.min_ids, self.best_cost, self.best_len = [], None, 0

    @classmethod
    def of(cls, o):
        xy, parent, _ = o.tree()
        return cls(xy, parent, o.final_ids())

    def line(self, c):
        return ("%s: %d iterations, %d final nodes, %d solutions of %d states, final paths of %d states against a scratch of %d, "
                "least cost at %s, best path of %d states"
                % (c.name, c.n_iter_min, len(self.final_ids), self.n_solutions, self.solution_states, self.final_states,
                   scratch_bound(c.n_iter_max), self.min_ids, self.best_len))


def is_clean(c, o):
    """nothing was refused and no injected sample was steered: node i is iteration i's sample, bit for bit, but in the goal point's
    iterations"""
    import exact_inputs
    x = o.tree()[0]
    if not (o.num_iterations() == c.n_iter_min and o.num_nodes() == o.num_iterations() + 1):
        return False
    want = exact_inputs.rrt_iteration_samples(c, c.samples, c.n_iter_min)
    own = np.arange(1, c.n_iter_min + 1) % 100 != 0
    return bool(np.array_equal(x[1:][own].view(np.uint64), np.ascontiguousarray(want[own]).view(np.uint64)))
