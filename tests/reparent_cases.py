"""Hand-built belief graphs and policies for the tests of the Reparent strategy (tests/test_reparent_cpu.py on the restatement alone,
tests/test_gpu_reparent.py on the device).  TEST INFRASTRUCTURE ONLY.

A case is a Case(G, ids, parents, radius): graph G (reparent_ref.Graph), the policy's belief-graph ids and its parents within the policy.
All states of the one-world cases lie in the free part of refine_policies_cases.wall_raster() (a wall at x = 0 from the top edge down to
y = -0.4) unless the case is about the wall."""
from collections import namedtuple

import numpy as np

import reparent_ref as rr

Case = namedtuple("Case", "G ids parents radius")
ONE = [[1.0]]


def graph(xy, children, belief_row=None, beliefs=ONE):
    row = np.zeros(len(xy), dtype=np.uint32) if belief_row is None else belief_row
    return rr.Graph.of_lists(xy, row, beliefs, children)


def chain(n):
    return np.arange(-1, n - 1)


def grandchild_skip():
    """A -> c -> cc -> x, all inside the radius: x is added and hangs from c; cc is not added"""
    xy = [(0.3, -0.7), (0.32, -0.7), (0.34, -0.7), (0.36, -0.7)]
    return Case(graph(xy, [[1], [2], [3], []]), [0], [-1], 0.3)


def push_time_filter():
    """A -> v and A -> c, both added; c -> v; v -> y; y -> z.  After both adds the FIFO holds only (tree(v), y): z hangs from v's tree
    node, not also from c's; y itself is absent.  ids: A 0, v 1, c 2, y 3, z 4"""
    xy = [(0.3, -0.7), (0.32, -0.7), (0.3, -0.72), (0.34, -0.7), (0.36, -0.7)]
    return Case(graph(xy, [[1, 2], [3], [1], [4], []]), [0], [-1], 0.3)


def offspring_edge_cost():
    """A -> c -> cc -> x on a line, pitch 1/16: x hangs from c with the cost of A -> x (0.125), so its upward sum is 0.1875 and A's pop
    reparents it (0 + 0.125 < 0.1875); with the distance c -> x as its cost the sum would be 0.125 exactly and nothing would move"""
    xy = [(0.25, -0.75), (0.3125, -0.75), (0.34375, -0.75), (0.375, -0.75)]
    return Case(graph(xy, [[1], [2], [3], []]), [0], [-1], 0.5)


def summation_order():
    """a path of four collinear nodes: the upward sum of node 3 (cost3 + cost2 + cost1 = 0.864) equals what node 1's pop offers it
    bit for bit, so it keeps its parent; summed from the root down it is 0.8640000000000001 and it would be reparented"""
    xy = [(-0.551, -0.5), (-0.53, -0.5), (-0.121, -0.5), (0.313, -0.5)]
    return Case(graph(xy, [[], [], [], []]), [0, 1, 2, 3], chain(4), 2.0)


def stale_priority():
    """path R -> a -> b -> c with a a detour; R's pop reparents b, c keeps its priority (1.04, its sum is now 0.35); X, an offspring
    that hangs from W with the cost of R -> X, is popped before c and reparented by c's pop after it: 7 pops for 6 nodes.
    ids: R 0, a 1, b 2, c 3, W 4, V 5, X 6"""
    xy = [(0.1, -0.9), (0.1, -0.51), (0.2, -0.9), (0.45, -0.9), (0.15, -0.6), (0.3, -0.7), (0.48, -0.85)]
    return Case(graph(xy, [[4], [], [], [], [5], [6], []]), [0, 1, 2, 3], chain(4), 0.4)


def one_node_piece_branches():
    """the root branches at once: its piece has one node, a start and no end, so the two pieces after it keep parent -1"""
    xy = [(0.3, -0.7), (0.4, -0.7), (0.3, -0.8), (0.5, -0.7), (0.3, -0.9)]
    return Case(graph(xy, [[], [], [], [], []]), [0, 1, 2, 3, 4], [-1, 0, 0, 1, 2], 0.1)


def two_node_piece_grows():
    """P0 -> P1 with an offspring O of P0 between them: (O - P0) + (P1 - O) = 0.423 < P1 - P0 = 0.42300000000000004, so P1 hangs under O
    and the piece comes out with three nodes.  ids: P0 0, P1 1, O 2"""
    xy = [(0.107, -0.6), (0.53, -0.6), (0.153, -0.6)]
    return Case(graph(xy, [[2], [], []]), [0, 1], chain(2), 0.8)


def lattice(n=6, pitch=1.0 / 32):
    """an n x n lattice right of the wall, every node the child of its 4-neighbours; the policy runs along the bottom row and up the
    last column: many bit-equal priorities"""
    xy = [(0.25 + pitch * i, -0.9 + pitch * j) for j in range(n) for i in range(n)]
    at = lambda i, j: j * n + i
    children = [[at(i + di, j + dj) for di, dj in ((1, 0), (0, 1), (-1, 0), (0, -1)) if 0 <= i + di < n and 0 <= j + dj < n]
                for j in range(n) for i in range(n)]
    ids = [at(i, 0) for i in range(n)] + [at(n - 1, j) for j in range(1, n)]
    return Case(graph(xy, children), ids, chain(len(ids)), 4 * pitch)


def star(n_children, radius=0.3, dup=False):
    """a root with n_children children on a circle of radius 0.05 around it (dup: the first child listed a second time at the end); the
    policy is the root alone: a tree of 1 + n_children nodes, all within each other's reach"""
    ang = np.linspace(0.0, 2.0 * np.pi, n_children, endpoint=False)
    xy = [(0.5, -0.7)] + [(0.5 + 0.05 * np.cos(a), -0.7 + 0.05 * np.sin(a)) for a in ang]
    kids = list(range(1, n_children + 1)) + ([1] if dup and n_children else [])
    return Case(graph(xy, [kids] + [[] for _ in range(n_children)]), [0], [-1], radius)


def path_with_star(n_path, n_children, radius=0.3):
    """a path of n_path nodes, pitch 0.01, whose first node has n_children children around it: a tree of n_path + n_children nodes"""
    ang = np.linspace(0.0, 2.0 * np.pi, max(n_children, 1), endpoint=False)[:n_children]
    xy = [(0.3 + 0.01 * k, -0.7) for k in range(n_path)] + [(0.3 + 0.05 * np.cos(a), -0.7 + 0.05 * np.sin(a)) for a in ang]
    children = [list(range(n_path, n_path + n_children))] + [[] for _ in range(n_path - 1 + n_children)]
    return Case(graph(xy, children), list(range(n_path)), chain(n_path), radius)


def copies(n_copies=40):
    """a path of three nodes whose middle node has n_copies children at its own state, each the child of the one before as well:
    zero-length edges and tied priorities"""
    xy = [(0.3, -0.7), (0.35, -0.7), (0.4, -0.7)] + [(0.35, -0.7)] * n_copies
    children = [[], list(range(3, 3 + n_copies)), []] + [[k + 1] if k + 1 < 3 + n_copies else [] for k in range(3, 3 + n_copies)]
    return Case(graph(xy, children), [0, 1, 2], chain(3), 0.2)


def wall_in_range():
    """two path nodes left of the wall (above its lower end) and offsprings right of it, 0.06 away: in range, transition refused"""
    xy = [(-0.05, -0.2), (-0.05, -0.1), (0.05, -0.2), (0.05, -0.1), (-0.08, -0.15)]
    return Case(graph(xy, [[2, 4], [3], [], [], []]), [0, 1], chain(2), 0.3)


def leaves_raster():
    """an offspring outside the raster: its transition check is the reference's panic"""
    xy = [(0.9, -0.9), (0.95, -0.9), (1.2, -0.9)]
    return Case(graph(xy, [[2], [], []]), [0, 1], chain(2), 0.8)


def mixed_piece():
    """a piece whose two input nodes carry different belief vectors (one world: 1.0 and 0.0)"""
    xy = [(0.3, -0.7), (0.35, -0.7)]
    return Case(graph(xy, [[], []], np.array([0, 1], dtype=np.uint32), [[1.0], [0.0]]), [0, 1], chain(2), 0.3)


def long_zigzag(n):
    """a path of n nodes, pitch 0.0003 in x, every other node 0.0002 up; radius 0.002 (a node reaches three on either side): the
    straight skips shorten it.  No offsprings: the tree has exactly n nodes"""
    xy = [(0.3 + 0.0003 * k, -0.7 + 0.0002 * (k % 2)) for k in range(n)]
    return Case(graph(xy, [[] for _ in range(n)]), list(range(n)), chain(n), 0.002)


SHELF_BELIEFS = [[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]]


def crosses_beliefs():
    """on the shelf raster, two worlds: P0 -> P1 under belief 0; P0's child O carries belief 1 ([1, 0], as the child of an observation
    would) and lies between them where (O - P0) + (P1 - O) < P1 - P0: the piece comes out as P0, O, P1 with O's own belief in it, and
    O's other child (same state, belief 2) is in the tree as well.  ids: P0 0, P1 1, O 2, O' 3"""
    xy = [(0.107, -0.9), (0.53, -0.9), (0.153, -0.9), (0.153, -0.9)]
    return Case(graph(xy, [[2, 3], [], [], []], np.array([0, 0, 1, 2], dtype=np.uint32), SHELF_BELIEFS), [0, 1], chain(2), 0.8)


def door_two_beliefs():
    """on the door raster: the path of refine_policies_cases.DOOR_PATH once under a belief that leaves door 0 possibly shut and once
    under one that has it open, as two policies over one graph (ids 0-9 and 10-19)"""
    import refine_policies_cases as rp
    k = len(rp.DOOR_PATH)
    G = graph(rp.DOOR_PATH + rp.DOOR_PATH, [[] for _ in range(2 * k)], np.repeat([0, 1], k).astype(np.uint32), rp.DOOR_BELIEFS)
    return [Case(G, list(range(b * k, (b + 1) * k)), chain(k), 1.5) for b in (0, 1)]     # door 0 lies between the path's ends, 0.7 apart


HAND = [grandchild_skip, push_time_filter, offspring_edge_cost, summation_order, stale_priority, one_node_piece_branches, two_node_piece_grows,
        lattice, copies, wall_in_range]


# the grown cases of both test files: the seeds tried (0 and 1 in both domains) all satisfy the reference's leaf-count assertion
GROWN_SEEDS = {"door": (0, 1), "shelf": (0, 1)}


def door_case(seed, n=2000):
    import cases
    c = cases.cfg_door(n, n, seed=seed)
    c.update(goals=[(0.5, 0.3)])                             # behind door 1
    return c, [0.0, 0.0, 0.4, 0.6]


def shelf_case(seed, n=2000):
    import cases
    return cases.cfg3_near(n, seed=seed), [0.5, 0.5]


def restate(o, case, **kw):
    return rr.refine(o, case.G, case.ids, case.parents, case.radius, **kw)
