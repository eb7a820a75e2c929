"""A literal Python restatement of the reference's QMDP policy extractor (src/qmdp_policy_extractor.rs) and of what it stands on:
dijkstra over PTOGraphWorldView (src/pto_graph.rs:245-303), Reachability::get_final_nodes_for_world (src/pto_reachability.rs:58-63)
and KdTree::add / nearest_neighbor (src/nearest_neighbor.rs:29-92), over plain arrays.  Python floats and math.sqrt are IEEE f64, so
equality with the device is bit equality.

The reference does not terminate on some inputs (a walk parked on node 0 with nothing finite below it, a zero-length hop between
exact duplicates).  Here, as on the device, a walk that would emit more than max_states states raises WalkTooLong."""
import heapq
import math
import sys

INF = float("inf")
MAX_STATES = 1 << 16          # option "qmdp_max_states"


class WalkTooLong(Exception):
    def __init__(self, world):
        super().__init__("common path" if world is None else "world %d" % world)
        self.world = world


def norm2(a, b):
    """common.rs:203-213"""
    d2 = 0.0
    for xa, xb in zip(a, b):
        dx = xb - xa
        d2 += dx * dx
    return math.sqrt(d2)


def weighted_parents(xy, children):
    """graph.parents(v) with cost_evaluator(u.state, v.state) = norm2 beside each parent u: the weight of an edge is the same in every
    world, so it is computed once (PTOGraph::add_edge pushes the child and the parent entry together; the order of a parents list
    does not matter to the fixpoint)"""
    par = [[] for _ in children]
    for u, cs in enumerate(children):
        for v in cs:
            par[v].append((u, norm2(xy[u], xy[v])))
    return par


def dijkstra_world(node_validity, validities, wparents, world, finals):
    """dijkstra (pto_graph.rs:275-303) over PTOGraphWorldView{world} (:245-271): a queue, re-push on improvement; graph.parents(v)
    keeps the parents whose own node validity has the world.  world = None: the plain graph (no filter).  The reference's
    PriorityQueue holds a node once (a push of a queued node changes its priority): a heap entry that is out of date is skipped."""
    n = len(wparents)
    ok = [True] * n if world is None else [bool((validities[v] >> world) & 1) for v in node_validity]
    dist = [INF] * n
    q = []
    for i in finals:
        dist[i] = 0.0
        heapq.heappush(q, (0.0, i))
    while q:
        d, v = heapq.heappop(q)
        if d > dist[v]:
            continue
        for u, w in wparents[v]:
            if ok[u]:
                alt = d + w
                if alt < dist[u]:
                    dist[u] = alt
                    heapq.heappush(q, (alt, u))
    return dist


def finals_for_world(final_ids, final_masks, reach, world):
    """pto_reachability.rs:58-63"""
    return [i for i, m in zip(final_ids, final_masks) if (reach[i] >> world) & 1 and (m >> world) & 1]


class KdTree:
    """nearest_neighbor.rs: add in node-id order (:29-46), nearest_neighbor (:48-92)"""

    def __init__(self, xy):
        self.xy = xy
        self.left = [-1] * len(xy)
        self.right = [-1] * len(xy)
        for i in range(1, len(xy)):
            cur, axis = 0, 0
            while True:
                side = self.left if xy[i][axis] < xy[cur][axis] else self.right
                if side[cur] < 0:
                    side[cur] = i
                    break
                cur, axis = side[cur], (axis + 1) % 2

    def nearest(self, s):
        best = [INF, 0]
        xy, left, right = self.xy, self.left, self.right

        def inner(n, axis):
            d = norm2(xy[n], s)
            if d < best[0]:
                best[0], best[1] = d, n
            nxt = (axis + 1) % 2
            if s[axis] < xy[n][axis]:
                if s[axis] - best[0] < xy[n][axis] and left[n] >= 0:
                    inner(left[n], nxt)
                if s[axis] + best[0] >= xy[n][axis] and right[n] >= 0:
                    inner(right[n], nxt)
            else:
                if s[axis] + best[0] >= xy[n][axis] and right[n] >= 0:
                    inner(right[n], nxt)
                if s[axis] - best[0] < xy[n][axis] and left[n] >= 0:
                    inner(left[n], nxt)

        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, len(xy) + 100))
        try:
            inner(0, 0)
        finally:
            sys.setrecursionlimit(old)
        return best[1]


class Qmdp:
    """QMdpPolicyExtractor over plain arrays: xy[i] = (x, y); node_validity[i] indexes validities (ints of world bits); children[i] in
    push order; final_ids / final_masks as Reachability keeps them; reach[i] per node."""

    def __init__(self, xy, node_validity, validities, children, final_ids, final_masks, reach, n_worlds, max_states=MAX_STATES):
        self.xy = [tuple(float(c) for c in p) for p in xy]
        self.node_validity = [int(v) for v in node_validity]
        self.validities = [int(v) for v in validities]
        self.children = children
        self.final_ids = [int(i) for i in final_ids]
        self.final_masks = [int(m) for m in final_masks]
        self.reach = [int(r) for r in reach]
        self.n_worlds = n_worlds
        self.max_states = max_states
        self.cost_to_goals = []
        self._kd = None

    def plan_qmdp(self):
        """:23-35"""
        par = weighted_parents(self.xy, self.children)
        self.cost_to_goals = []
        for world in range(self.n_worlds):
            finals = finals_for_world(self.final_ids, self.final_masks, self.reach, world)
            if not finals:
                raise ValueError("We should have final node ids for each world")
            self.cost_to_goals.append(dijkstra_world(self.node_validity, self.validities, par, world, finals))

    def get_best_expected_child(self, node, belief):
        """:90-108"""
        best_child, smallest = 0, INF
        for c in self.children[node]:
            e = 0.0
            for world in range(self.n_worlds):
                e += self.cost_to_goals[world][c] * belief[world]
            if e < smallest:
                best_child, smallest = c, e
        return best_child, smallest

    def get_best_child(self, node, world):
        """:110-123"""
        best_child, smaller = 0, INF
        cost = self.cost_to_goals[world]
        for c in self.children[node]:
            if cost[c] < smaller:
                smaller, best_child = cost[c], c
        return best_child

    def get_common_path(self, start_id, belief, common_horizon):
        """:65-87"""
        if len(belief) != self.n_worlds:
            raise ValueError("belief state size should match the number of worlds")
        path, i, smallest, acc = [], start_id, INF, 0.0
        while acc < common_horizon and smallest > 0.0:
            if len(path) >= self.max_states:
                raise WalkTooLong(None)
            path.append(self.xy[i])
            c, e = self.get_best_expected_child(i, belief)
            acc += norm2(self.xy[i], self.xy[c])
            i, smallest = c, e
        return path, i

    def get_path(self, start_id, world):
        """:51-62"""
        path, i = [], start_id
        while self.cost_to_goals[world][i] > 0.0:
            if len(path) >= self.max_states:
                raise WalkTooLong(world)
            path.append(self.xy[i])
            i = self.get_best_child(i, world)
        return path

    def nearest(self, start):
        if self._kd is None:
            self._kd = KdTree(self.xy)
        return self._kd.nearest((float(start[0]), float(start[1])))

    def react_qmdp(self, start, belief, common_horizon):
        """:38-49; returns (paths, number of common states)"""
        belief = [float(b) for b in belief]
        common, i = self.get_common_path(self.nearest(start), belief, float(common_horizon))
        return [common + self.get_path(i, world) for world in range(self.n_worlds)], len(common)


def children_from_edges(n, efrom, eto):
    """PTOGraph.children in push order from the forward edges in creation order (pto.rs:110-120: for a new node first
    add_edge(neighbour, new) for all its neighbours, then add_edge(new, neighbour))"""
    adj = [[] for _ in range(n)]
    e = 0
    while e < len(eto):
        e1 = e
        while e1 < len(eto) and eto[e1] == eto[e]:
            e1 += 1
        for k in range(e, e1):
            adj[int(efrom[k])].append(int(eto[k]))
        for k in range(e, e1):
            adj[int(eto[k])].append(int(efrom[k]))
        e = e1
    return adj


def from_planner(x, max_states=MAX_STATES):
    """a Qmdp over the getters of an engine or oracle object holding a grown PTO graph"""
    xy, _, _ = x.tree()
    f, t, _ = x.edges()
    return Qmdp(xy.tolist(), x.node_validity().tolist(), [int(v) for v in x.validities()], children_from_edges(len(xy), f, t),
                x.final_ids().tolist(), x.final_masks().tolist(), x.reach().tolist(), x.n_worlds(), max_states)


# ---- the graphs of the reference's own tests (pto_graph.rs:434-564) as data: xy, node validity ids, validities, edges in add order
def _graph(xy, node_validity, validities, edges):
    children = [[] for _ in xy]
    for a, b in edges:
        children[a].append(b)
    return dict(xy=xy, node_validity=node_validity, validities=validities, children=children)


def _both(a, b):
    return [(a, b), (b, a)]          # add_bi_edge (:209-212)


def minimal_graph():
    return _graph([(0.0, 0.0), (1.0, 0.0)], [0, 0], [1], [(0, 1)])


def grid_graph():
    xy = [(float(x), float(y)) for y in range(3) for x in range(3)]
    e = _both(0, 1) + _both(1, 2) + _both(0, 3) + _both(1, 4) + _both(2, 5) + _both(3, 4) + _both(4, 5)
    e += _both(3, 6) + _both(4, 7) + _both(5, 8) + _both(6, 7) + _both(7, 8)
    return _graph(xy, [0] * 9, [1], e)


def oriented_grid_graph():
    return _graph([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)], [0] * 4, [1], [(0, 1), (0, 2), (1, 3), (3, 2)])


def diamond_graph_2_worlds():
    """:539-564: validities [1,0], [0,1], [1,1]; node 1 has validity id 1 (world 1 only), node 2 validity id 0 (world 0 only)"""
    e = _both(0, 1) + _both(0, 2) + _both(1, 3) + _both(2, 3)
    return _graph([(0.0, 0.0), (1.0, 1.0), (1.0, -1.0), (2.0, 0.0)], [2, 1, 0, 2], [0b01, 0b10, 0b11], e)


S2 = math.sqrt(2.0)
# (graph, per-world final lists, expected per-world costs): the vectors the reference asserts (pto_graph.rs:626-678) and the diamond by hand
KATS = {
    "minimal": (minimal_graph, [[1]], [[1.0, 0.0]]),
    "grid_to_8": (grid_graph, [[8]], [[4.0, 3.0, 2.0, 3.0, 2.0, 1.0, 2.0, 1.0, 0.0]]),
    "grid_to_7_5": (grid_graph, [[7, 5]], [[3.0, 2.0, 1.0, 2.0, 1.0, 0.0, 1.0, 0.0, 1.0]]),
    "grid_no_finals": (grid_graph, [[]], [[INF] * 9]),
    "oriented": (oriented_grid_graph, [[3]], [[2.0, 1.0, INF, 0.0]]),
    "diamond_2_worlds": (diamond_graph_2_worlds, [[3], [3]], [[S2 + S2, INF, S2, 0.0], [S2 + S2, S2, INF, 0.0]]),
}


def costs_explicit(g, finals):
    """per-world dijkstra over the world view of an explicit graph dict (a world without finals: all inf, pto_graph.rs:658-667)"""
    par = weighted_parents(g["xy"], g["children"])
    return [dijkstra_world(g["node_validity"], g["validities"], par, w, f) for w, f in enumerate(finals)]
