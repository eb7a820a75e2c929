"""extract_policy / get_best_expected_children (src/belief_graph.rs:184-267) restated in Python, started at any belief
node s of an explicit graph: the reference for porrt_bg_extract_policies, porrt_mm_extract_policies and
porrt_extract_policies (the oracle's orc_extract_policy starts at node 0).  Pinned against the oracle in
tests/test_policies_cpu.py.  Plain Python floats: IEEE doubles, no fused operations, math.sqrt correctly rounded.

Statuses, as include/porrt_hip.h lists them:
  0 OK
  1 dist[s] is not finite
  2 the walk returns to a belief node on its own path (the reference does not terminate)
  3 assert!(p > 0.0) (:250) or assert!(p * dist[best] <= dist[node]) (:261) fails
  4 the policy would exceed max_nodes, or a row has more than 65535 children
"""
import math

import numpy as np

OK, NO_COST, OWN_PATH, ASSERT, CAPACITY = 0, 1, 2, 3, 4
MAX_NODES = 1 << 16              # option "policy_max_nodes"
ROW_MAX = 65535


class Graph:
    """What the walk reads: per belief node its state, the row of `beliefs` it carries, its clustering key (belief id), its
    children in add_edge order (CSR).  Kept as arrays (a grown graph has millions of edges); a row is fetched when it is walked."""

    def __init__(self, xy, belief_row, beliefs, belief_ids, child_off, child_ids):
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        self.x, self.y = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
        self.row = np.asarray(belief_row).astype(np.int64)
        self.beliefs = np.asarray(beliefs, dtype=np.float64).tolist()
        self.key = np.asarray(belief_ids).astype(np.int64)
        self.off = np.asarray(child_off).astype(np.int64)
        self.ids = np.asarray(child_ids).astype(np.int64)
        self.n = len(self.x)


def graph_of_lists(xy, belief_row, beliefs, belief_ids, children):
    off = np.zeros(len(children) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in children])
    return Graph(xy, belief_row, beliefs, belief_ids, off, [v for c in children for v in c])


def context_graph(node_xy, beliefs, child_off, child_ids):
    """the belief graph of a context (Engine.belief_graph() / Oracle.belief_graph()): belief node i = graph node i // B with belief i % B"""
    B = len(beliefs)
    n = len(child_off) - 1
    xy = np.repeat(np.asarray(node_xy, dtype=np.float64).reshape(-1, 2), B, axis=0)[:n]
    b = np.arange(n) % B
    return Graph(xy, b, beliefs, b, child_off, child_ids)


def transition_probability(parent, child):
    """common.rs:187-190, summed in world order"""
    s = 0.0
    for pw, cw in zip(parent, child):
        s = s + (pw if cw > 0.0 else 0.0)
    return s


def extract_policy(g, dist, s, max_nodes=MAX_NODES):
    """(status, (original ids, parents, leaf flags) or None, dist[s])"""
    d = dist if isinstance(dist, np.ndarray) and dist.dtype == np.float64 else np.asarray(dist, dtype=np.float64)
    s = int(s)
    ds = float(d[s])
    if not math.isfinite(ds):
        return NO_COST, None, ds
    oid, par, leaf = [s], [-1], [0]                  # the root: no leaf, whatever its cost (:192)
    lifo = [0]
    while lifo:
        k = lifo.pop()
        bn = oid[k]
        up = par[k]
        while up >= 0:                               # the reference has no memory: here its endless walk ends
            if oid[up] == bn:
                return OWN_PATH, None, ds
            up = par[up]
        ids = g.ids[g.off[bn]:g.off[bn + 1]]
        if len(ids) > ROW_MAX:
            return CAPACITY, None, ds
        row, keys = ids.tolist(), g.key[ids].tolist()
        cx, cy, cd = g.x[ids].tolist(), g.y[ids].tolist(), d[ids].tolist()
        ux, uy, dn = float(g.x[bn]), float(g.y[bn]), float(d[bn])
        clusters = {}                                # BTreeMap<belief id, Vec<child>>: members in children order
        for j, key in enumerate(keys):
            clusters.setdefault(key, []).append(j)
        for key in sorted(clusters):
            members = clusters[key]
            p = transition_probability(g.beliefs[g.row[bn]], g.beliefs[g.row[row[members[0]]]])
            if not p > 0.0:
                return ASSERT, None, ds
            best_cost, best = math.inf, members[0]
            for j in members:
                dx, dy = ux - cx[j], uy - cy[j]
                cost = p * (math.sqrt(dx * dx + dy * dy) + cd[j])
                if cost < best_cost:
                    best_cost, best = cost, j
            if not p * cd[best] <= dn:
                return ASSERT, None, ds
            if len(oid) >= max_nodes:
                return CAPACITY, None, ds
            is_leaf = cd[best] == 0.0
            oid.append(row[best])
            par.append(k)
            leaf.append(1 if is_leaf else 0)
            if not is_leaf:
                lifo.append(len(oid) - 1)
    return OK, (np.array(oid, dtype=np.uint64), np.array(par, dtype=np.int64), np.array(leaf, dtype=np.uint8)), ds


def extract_policies(g, dist, starts, max_nodes=MAX_NODES):
    """one (status, policy or None, cost) per start"""
    d = np.ascontiguousarray(dist, dtype=np.float64)
    return [extract_policy(g, d, int(s), max_nodes) for s in starts]


def leaves_and_paths(policy):
    """Policy::leaves and Policy::path_to_leaf as the reference's tests use them (belief_graph.rs:531-543): ids of the leaf policy
    nodes, and per leaf the original ids from the root to it"""
    oid, par, leaf = policy
    leaves = [k for k in range(len(oid)) if leaf[k]]
    paths = []
    for k in leaves:
        p = []
        while k >= 0:
            p.append(int(oid[k]))
            k = int(par[k])
        paths.append(p[::-1])
    return leaves, paths


def check_reference_assertions(g, policy, which):
    """the policy assertions of the reference's own tests on its known-answer graphs (kat_graphs.graph_1 / graph_2), start 0:
    belief_graph.rs:531-543 (which = 1) and 563-566 (which = 2)"""
    oid, _, _ = policy
    leaves, paths = leaves_and_paths(policy)
    assert len(leaves) == 2
    state = lambda k: list(g["xy"][int(oid[k])])
    belief = lambda k: list(g["beliefs"][g["belief_vec"][int(oid[k])]])
    if which == 1:
        assert state(leaves[0]) == [0.0, 4.0] and state(leaves[1]) == [0.0, 4.0]             # the policy arrives at the goal
        assert belief(leaves[0]) == [0.0, 1.0] and belief(leaves[1]) == [1.0, 0.0]           # second belief first
        xy = lambda path: [list(g["xy"][i]) for i in path]
        assert xy(paths[0]) == [[0.0, 1.0], [0.0, 0.0], [0.0, 0.0], [0.0, 1.0], [1.0, 2.0], [10.0, 3.0], [0.0, 4.0]]     # on the right
        assert xy(paths[1]) == [[0.0, 1.0], [0.0, 0.0], [0.0, 0.0], [0.0, 1.0], [-1.0, 2.0], [-1.0, 3.0], [0.0, 4.0]]    # on the left
    else:
        assert state(leaves[0]) == [0.0, 3.0] and state(leaves[1]) == [0.0, 3.0]
