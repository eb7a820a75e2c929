"""Python restatement of PTOPolicyRefiner::refine_solution(RefinmentStrategy::Reparent(radius)) (src/pto_policy_refiner.rs:87-124, build_tree
:209-279, reparent :281-322, recompose :324-393): the yardstick of the device path (porrt_bg_reparent_policies / porrt_reparent_policies).

TEST INFRASTRUCTURE ONLY, built on the CPU oracle alone (tests/refine_ref.py for decompose, compatibility, is_transition_valid, norm2 and
expected_cost).  Never imported by the product package po_rrt_amd.

The text is restated line by line, with what looks like mistakes kept (an offspring is measured from the PATH node and its edge costs that
distance; a grandchild is never tested itself, its children are; the push-time visited filter; stale priorities; the upward summation).

Ours, not the reference's (the reference's queue orders bit-equal priorities by the internals of a crate):
  * among bit-equal priorities the node of the lowest tree id is popped (tie="high" pops the highest: a probe of the tests);
  * push on an item in the queue replaces its priority (higher or lower), on an item already popped inserts it again;
  * a piece's tree holds at most max_tree_nodes nodes, the FIFO of build_tree at most FIFO_PER_NODE x max_tree_nodes entries at a time,
    the tree nodes within 0.5 * radius of each other are at most PAIRS_PER_NODE x max_tree_nodes pairs (status 4);
  * a piece's loop makes at most POPS_PER_NODE x its tree's nodes pops (status 5).
A policy's status: 3 before anything else, then over its pieces 4, else 2 (raster fault in any node's neighbour check: every node is
popped at least once, so the checks are made for all nodes before the loop), else 5, else 0.
"""
import heapq
from collections import deque

import numpy as np

from refine_ref import RasterFault, _validity, compatibility, decompose, expected_cost, is_transition_valid, norm2

FIFO_PER_NODE = 16
PAIRS_PER_NODE = 256
POPS_PER_NODE = 64
DEFAULT_MAX_TREE_NODES = 16384


class Capacity(RuntimeError):
    pass


class PopCap(RuntimeError):
    pass


class Graph:
    """the belief graph as the reference reads it: node g has state xy[g], belief vector beliefs[belief_row[g]] and children
    child_ids[child_off[g]:child_off[g + 1]] in list order"""

    def __init__(self, xy, belief_row, beliefs, child_off, child_ids):
        self.xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self.belief_row = np.ascontiguousarray(belief_row, dtype=np.uint32)
        self.beliefs = np.ascontiguousarray(beliefs, dtype=np.float64)
        self.child_off = np.ascontiguousarray(child_off, dtype=np.uint64)
        self.child_ids = np.ascontiguousarray(child_ids, dtype=np.uint32)
        self._xy = self.xy.tolist()
        self._off = self.child_off.tolist()
        self._ids = self.child_ids.tolist()

    @classmethod
    def of_lists(cls, xy, belief_row, beliefs, children):
        off = np.zeros(len(children) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c) for c in children])
        ids = np.array([c for ch in children for c in ch], dtype=np.uint32)
        return cls(xy, belief_row, beliefs, off, ids)

    @classmethod
    def implicit(cls, xy_nodes, beliefs, child_off, child_ids):
        """the context's belief graph: belief node id = graph node * B + belief"""
        B = len(beliefs)
        n = len(child_off) - 1
        ids = np.arange(n)
        return cls(np.asarray(xy_nodes)[ids // B], (ids % B).astype(np.uint32), beliefs, child_off, child_ids)

    def state(self, g):
        return self._xy[g]

    def children(self, g):
        return self._ids[self._off[g]:self._off[g + 1]]


class Tree:
    def __init__(self):
        self.state, self.parent, self.cost, self.g = [], [], [], []
        self.leaf = 0

    def add(self, state, parent, cost, g):
        self.state.append(state); self.parent.append(parent); self.cost.append(cost); self.g.append(g)
        return len(self.g) - 1

    def dist_from_root(self, i):                             # :55-64: upward, cost += link.cost from 0.0
        cost = 0.0
        while self.parent[i] is not None:
            cost += self.cost[i]
            i = self.parent[i]
        return cost


def build_tree(G, path_g, radius, max_tree_nodes, stats=None):
    """:209-279 for a piece whose path has the belief-graph ids path_g"""
    t = Tree()
    visited = set()
    for k, g in enumerate(path_g):
        if len(t.g) >= max_tree_nodes:
            raise Capacity("tree")
        if k == 0:
            t.add(G.state(g), None, 0.0, g)
        else:
            t.add(G.state(g), k - 1, norm2(G.state(path_g[k - 1]), G.state(g)), g)
        visited.add(g)
    t.leaf = len(t.g) - 1
    n_path = len(t.g)
    fifo_max = 0
    for node_id in range(n_path):                            # nodes = tree.nodes.clone(): the path alone
        node_state = t.state[node_id]
        q = deque([(node_id, t.g[node_id])])
        while q:
            tree_id, g = q.popleft()
            for child in G.children(g):
                if child in visited:
                    continue
                d = norm2(node_state, G.state(child))       # from the PATH node, not from tree_id's state
                if d <= radius:
                    if len(t.g) >= max_tree_nodes:
                        raise Capacity("tree")
                    new_id = t.add(G.state(child), tree_id, d, child)
                    visited.add(child)
                    for cc in G.children(child):
                        if cc not in visited:               # at that moment
                            q.append((new_id, cc))
                    if len(q) > FIFO_PER_NODE * max_tree_nodes:
                        raise Capacity("fifo")
                    fifo_max = max(fifo_max, len(q))
    if stats is not None:
        stats["fifo_max"] = max(stats.get("fifo_max", 0), fifo_max)
    return t


class DirectQueue:
    """the queue as a table: pop scans for the least (priority, id)"""

    def __init__(self, tie):
        self.prio, self.sign = {}, 1 if tie == "low" else -1
        self.tied_pops = 0

    def push(self, i, p):
        self.prio[i] = p

    def pop(self):
        if not self.prio:
            return None
        i = min(self.prio, key=lambda k: (self.prio[k], self.sign * k))
        p = self.prio.pop(i)
        if any(v == p for v in self.prio.values()):
            self.tied_pops += 1
        return i, p


class HeapQueue:
    """a second implementation: heapq on (priority, id) with lazy deletion"""

    def __init__(self, tie):
        self.h, self.cur, self.sign = [], {}, 1 if tie == "low" else -1
        self.tied_pops = 0

    def push(self, i, p):
        self.cur[i] = p
        heapq.heappush(self.h, (p, self.sign * i))

    def pop(self):
        while self.h:
            p, si = heapq.heappop(self.h)
            i = self.sign * si
            if i in self.cur and self.cur[i] == p:
                del self.cur[i]
                while self.h and (self.sign * self.h[0][1] not in self.cur or self.cur[self.sign * self.h[0][1]] != self.h[0][0]):
                    heapq.heappop(self.h)                    # (stale entries off the top, so that the tie counter sees a live one)
                if self.h and self.h[0][0] == p:
                    self.tied_pops += 1
                return i, p
        return None


def valid_neighbours(o, t, half, compat_row, n_validities, max_tree_nodes, literal=False, cache=None):
    """per tree node: the tree nodes within `half` (itself and copies included) that is_transition_valid lets it reach, ascending.
    literal: is_transition_valid pair by pair, as the text has it.  Otherwise the same relation worked out once per pair of distinct
    STATES (a tree holds many copies of a state, one per belief): every node is in range of itself, so every state is classified (and
    may fault) in the literal form too, and a segment is looked at only where both its states have a validity.  cache (optional dict,
    shared by the policies of one graph): the class of a segment, a function of its two states alone."""
    xy = np.array(t.state, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    if literal:
        near = []
        for s in xy:                                         # norm2, vectorised: the same operations in the same order
            dx = xy[:, 0] - s[0]
            d2 = 0.0 + dx * dx
            dy = xy[:, 1] - s[1]
            d2 = d2 + dy * dy
            near.append(np.flatnonzero(np.sqrt(d2) <= half).tolist())
        if sum(len(v) for v in near) > PAIRS_PER_NODE * max_tree_nodes:
            raise Capacity("pairs")
        return [[j for j in near[i] if is_transition_valid(o, s, t.state[j], compat_row, n_validities)] for i, s in enumerate(t.state)]
    uniq, inv, mult = np.unique(xy, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    dx = uniq[None, :, 0] - uniq[:, None, 0]                 # [a, b]: b - a, as norm2(a, b) has it
    d2 = 0.0 + dx * dx
    dy = uniq[None, :, 1] - uniq[:, None, 1]
    d2 = d2 + dy * dy
    in_range = np.sqrt(d2) <= half
    if int((in_range * mult[:, None] * mult[None, :]).sum()) > PAIRS_PER_NODE * max_tree_nodes:
        raise Capacity("pairs")
    states = uniq.tolist()
    valid = [_validity(o.state_class(s), n_validities) is not None for s in states]
    ok = np.zeros(in_range.shape, dtype=bool)
    for a, b in zip(*np.nonzero(in_range)):
        if valid[a] and valid[b]:
            k = (states[a][0], states[a][1], states[b][0], states[b][1])
            cls = cache.get(k) if cache is not None else None
            if cls is None:
                cls = o.traversed_class(states[a], states[b])
                if cache is not None:
                    cache[k] = cls
            v = _validity(cls, n_validities)
            ok[a, b] = v is not None and compat_row[v]
    return [np.flatnonzero(ok[inv[i]][inv]).tolist() for i in range(n)]


def reparent(t, nbrs, queue="direct", tie="low", stats=None):
    """:281-322 on the valid neighbours computed above (states never move: the relation is a function of the tree)"""
    q = (DirectQueue if queue == "direct" else HeapQueue)(tie)
    xy = np.array(t.state, dtype=np.float64).reshape(-1, 2)
    for i in range(len(t.g)):
        q.push(i, t.dist_from_root(i))
    pops = reparents = stale = 0
    while True:
        top = q.pop()
        if top is None:
            break
        if pops == POPS_PER_NODE * len(t.g):
            raise PopCap()
        pops += 1
        i = top[0]
        d = t.dist_from_root(i)
        stale += d != top[1]
        nb = nbrs[i]
        snap = np.array([t.dist_from_root(j) for j in nb], dtype=np.float64)      # before any change
        dx = xy[nb, 0] - xy[i, 0]                            # norm2(node, neighbour) of all neighbours: the same operations in the same order
        d2 = 0.0 + dx * dx
        dy = xy[nb, 1] - xy[i, 1]
        cost = np.sqrt(d2 + dy * dy)
        for k in np.flatnonzero(d + cost < snap).tolist():
            j = nb[k]
            t.parent[j], t.cost[j] = i, float(cost[k])
            q.push(j, d + float(cost[k]))
            reparents += 1
    if stats is not None:
        stats["pops"] = stats.get("pops", 0) + pops
        stats["reparents"] = stats.get("reparents", 0) + reparents
        stats["tied_pops"] = stats.get("tied_pops", 0) + q.tied_pops
        stats["stale_pops"] = stats.get("stale_pops", 0) + stale
    return pops


def refine(o, G, original_ids, parents, radius, max_tree_nodes=DEFAULT_MAX_TREE_NODES, queue="direct", tie="low", stats=None, pops_per_node=None, cache=None):
    """refine_solution(Reparent(radius)) of the policy (belief-graph ids original_ids, parents within the policy) over graph G on oracle
    context `o`: status, ((xy, original ids, parents, is_leaf), expected cost) -- the latter None unless status is 0"""
    global POPS_PER_NODE
    if len(parents) == 0:
        return 1, None
    ids = [int(v) for v in original_ids]
    validities = o.validities()
    compat = compatibility(G.beliefs, validities)
    pieces, skeleton = decompose(parents)
    row = G.belief_row
    for p in pieces:                                         # decompose's assert_eq! on the beliefs along a piece
        for i in p:
            if not np.array_equal(G.beliefs[row[ids[i]]].view(np.uint64), G.beliefs[row[ids[p[0]]]].view(np.uint64)):
                return 3, None
    flags = set()
    trees = []
    old = POPS_PER_NODE
    if pops_per_node is not None:
        POPS_PER_NODE = pops_per_node
    try:
        for p in pieces:
            try:
                t = build_tree(G, [ids[i] for i in p], radius, max_tree_nodes, stats)
                nbrs = valid_neighbours(o, t, 0.5 * radius, compat[int(row[ids[p[0]]])], len(validities), max_tree_nodes, cache=cache)
                if stats is not None:
                    stats["tree_nodes"] = stats.get("tree_nodes", 0) + len(t.g)
                    stats["max_tree"] = max(stats.get("max_tree", 0), len(t.g))
                    stats["pairs"] = stats.get("pairs", 0) + sum(len(v) for v in nbrs)
                    stats.setdefault("trees", []).append(len(t.g))
                reparent(t, nbrs, queue, tie, stats)
                trees.append(t)
            except Capacity:
                flags.add(4)
            except RasterFault:
                flags.add(2)
            except PopCap:
                flags.add(5)
    finally:
        POPS_PER_NODE = old
    for s in (4, 2, 5):
        if s in flags:
            return s, None
    # recompose (:324-393): per piece the parent chain from tree.leaf up to the root, reversed
    out_xy, out_g, par = [], [], []
    start, end = [None] * len(pieces), [None] * len(pieces)
    for i, t in enumerate(trees):
        chain = [t.leaf]
        while t.parent[chain[-1]] is not None:
            chain.append(t.parent[chain[-1]])
        chain.reverse()
        for j, k in enumerate(chain):
            nid = len(out_g)
            out_xy.append(t.state[k]); out_g.append(t.g[k])
            par.append(-1 if j == 0 else nid - 1)
            if j == 0:                                       # if is_start ... else if is_end: a one-node chain has no end
                start[i] = nid
            elif j == len(chain) - 1:
                end[i] = nid
    for i, nxt in enumerate(skeleton):
        for k in nxt:
            if end[i] is not None and start[k] is not None:
                par[start[k]] = end[i]
    m = len(out_g)
    leaf = np.ones(m, dtype=np.uint8)
    for p in par:
        if p >= 0:
            leaf[p] = 0
    bel = [G.beliefs[row[g]] for g in out_g]
    cost = expected_cost(out_xy, par, bel)
    return 0, ((np.array(out_xy, dtype=np.float64).reshape(-1, 2), np.array(out_g, dtype=np.uint64), np.array(par, dtype=np.int64), leaf), cost)
