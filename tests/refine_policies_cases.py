"""Hand-built policies for the batch refiner's tests (porrt_refine_policies): the policies of tests/test_gpu_refine.py and
tests/test_refine_cpu.py as arrays, plus the shapes only a batch meets.  TEST INFRASTRUCTURE ONLY.

A policy is (xy [k, 2], parents within the policy (-1 for row 0, children in ascending id order), original ids, belief rows)."""
import numpy as np

import refine_ref


def policy(xy, par, row=None, oid0=7):
    par = np.asarray(par, dtype=np.int64)
    row = np.zeros(len(par), dtype=np.uint32) if row is None else np.asarray(row, dtype=np.uint32)
    return (np.asarray(xy, dtype=np.float64).reshape(-1, 2), par, np.arange(oid0, oid0 + len(par), dtype=np.uint64), row)


def chain(n):
    return np.arange(-1, n - 1)


def wall_raster():
    occ = np.full((100, 100), 255, dtype=np.uint8)
    occ[:70, 49:51] = 0                     # a wall from the top edge down to y = -0.4, at x = 0
    return occ


LOW_SHELF_PATH = [(0.8, 0.6), (0.88, 0.52), (0.92, 0.4), (0.93, 0.3), (0.9, 0.2), (0.8, 0.1)]
DOOR_PATH = [(-0.5, -0.4), (-0.1, -0.35), (0.3, -0.3), (0.47, -0.2), (0.47, 0.2), (0.45, 0.7), (0.1, 0.8), (-0.2, 0.75), (-0.45, 0.6), (-0.5, 0.3)]
DOOR_BELIEFS = [[0.0, 0.0, 0.5, 0.5], [0.0, 0.0, 0.0, 1.0]]
WALL_PATH = [(-0.6, 0.6), (-0.5, 0.2), (-0.3, -0.2), (-0.25, -0.6), (-0.1, -0.75), (0.0, -0.8), (0.1, -0.75), (0.25, -0.6),
             (0.3, -0.2), (0.45, 0.1), (0.5, 0.4), (0.6, 0.6)]
SHELF_BELIEFS = [[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]]


def zigzag(n, x0=-0.9, x1=0.9, y=-0.85, amp=0.02):
    xs = np.linspace(x0, x1, n)
    return policy(np.stack([xs, y + amp * (np.arange(n) % 2)], axis=1), chain(n))


def small_pieces():
    """pieces of 12, 1, 2, 1 (branches: the quirk), 3 and 1 nodes"""
    xy = list(WALL_PATH) + [(0.6, 0.7), (0.7, 0.6), (0.75, 0.55), (0.7, 0.7), (0.72, 0.8), (0.74, 0.75), (0.76, 0.82), (0.65, 0.75)]
    return policy(xy, list(range(-1, 11)) + [11, 11, 13, 11, 15, 16, 17, 15])


def root_branches_at_once():
    return policy([(0.0, 0.0), (0.1, 0.1), (0.2, 0.3), (0.3, 0.2), (-0.1, 0.1), (-0.2, 0.2), (0.5, 0.5)], [-1, 0, 1, 2, 0, 4, 3])


def unreachable_nodes():
    """three beliefs (rows of SHELF_BELIEFS); nodes 5 and 6, parents of each other, are not reached from the root"""
    xy = [(-0.5, -0.9), (-0.4, -0.8), (-0.3, -0.9), (-0.2, -0.8), (-0.1, -0.9), (0.0, -0.8), (0.1, -0.9), (0.2, -0.8)]
    return policy(xy, [-1, 0, 1, 2, 2, 6, 5, 4], [0, 0, 0, 1, 2, 0, 0, 2])


def comb(n=70):
    """a spine of n nodes (ids 0 .. n - 1), every spine node with a leaf child too (ids n .. 2n - 1) and the last one with a second
    (id 2n): n one-node pieces that branch and n + 1 one-node leaves"""
    xs = np.linspace(-0.9, 0.9, n)
    xy = [(x, -0.9) for x in xs] + [(x, -0.85) for x in xs] + [(0.9, -0.95)]
    return policy(xy, [-1] + list(range(n - 1)) + list(range(n)) + [n - 1])


def bushy():
    """every piece has >= 3 nodes, and the ids are dealt so that the breadth-first piece order is not the id order:
    root piece 0-1-2-3; 3 branches into A (4, 7, 10, 13), B (5, 8, 11, 14, 16) and C (6, 9, 12, 15); B's end 16 branches into
    D (17, 19, 21) and E (18, 20, 22, 23, 24, 25)"""
    par = [-1, 0, 1, 2, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 16, 17, 18, 19, 20, 22, 23, 24]
    n = len(par)
    rng = np.random.default_rng(3)
    xy = np.zeros((n, 2))
    xy[0] = (-0.8, -0.8)
    for k in range(1, n):                                         # short steps below the wall's end, a zig-zag the shortcuts can straighten
        xy[k] = np.clip(xy[par[k]] + rng.uniform(-0.08, 0.12, size=2), -0.95, -0.45)
    return policy(xy, par)


def restate(o, pol, beliefs, n_iterations):
    """refine_ref.refine of one policy of a batch"""
    xy, par, oid, row = pol
    return refine_ref.refine(o, xy, par, oid, row, beliefs, n_iterations)


def info_of(policies, statuses):
    """what porrt_refine_policies_info counts, from refine_ref.decompose policy by policy"""
    pieces = longs = nodes = 0
    lengths = set()
    for pol, st in zip(policies, statuses):
        if st not in (0, 2) or len(pol[1]) == 0:
            continue
        pcs = refine_ref.decompose(pol[1])[0]
        pieces += len(pcs)
        longs += sum(len(p) >= 3 for p in pcs)
        lengths |= {len(p) for p in pcs if len(p) >= 3}
        if st == 0:
            nodes += sum(len(p) for p in pcs)
    return dict(policies=len(policies), ok=sum(int(s) == 0 for s in statuses), pieces=pieces, shortcut_pieces=longs, nodes=nodes,
                distinct_lengths=len(lengths))
