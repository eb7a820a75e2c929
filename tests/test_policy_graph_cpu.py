"""CPU tests of the policy-graph procedure as restated in tests/policy_graph_ref.py: the reference's asserted answers
(pto_graph.rs:574-623), and the f64 procedure against the exact rational oracle on every entry of small inputs.

Agreement is required wherever v* <= 0 (keep) or v* > 2 * TOL * scale (prune); an entry with 0 < v* <= 2 * TOL * scale may go
either way, and at most 2 % of an input's entries may be of that kind.  The f64 game value with early stopping off is within
ERR_BOUND * scale of v* (the measurement DESIGN.md section 26 reports; TOL = 1e-9 stands while it is at most 1e-12)."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import policy_graph_ref as P
import qmdp_ref as Q

INF = float("inf")
ERR_BOUND = 1e-12


# ---- the reference's three answers
@pytest.mark.parametrize("name", sorted(P.KATS))
def test_kat_restatement(name):
    make, want = P.KATS[name]
    children, costs = make()
    keep, how, _ = P.policy_graph(children, costs)
    got = P.pruned_children(children, keep)
    for node, cs in want.items():
        assert got[node] == cs, (node, got[node], cs)
    assert not (how == 5).any()


@pytest.mark.parametrize("name", sorted(P.KATS))
def test_kat_exact(name):
    make, want = P.KATS[name]
    children, costs = make()
    costs = np.asarray(costs)
    for node, cs in want.items():
        ids = np.asarray(children[node])
        C = P.node_costs(costs, ids)
        got = []
        for j in range(len(ids)):
            D, _, nv = P.entry_rows(ids, C, j)
            if P.exact_keep(D.tolist(), nv)[1]:
                got.append(int(ids[j]))
        assert got == cs, (node, got, cs)


# ---- inputs
def geometric(seed, n, nw, radius):
    """a seeded random geometric graph, edges both ways in creation order, one goal and a random set of blocked nodes per world"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 1.0, (n, 2))
    edges = []
    for i in range(n):
        for j in range(i):
            if np.hypot(*(xy[i] - xy[j])) < radius:
                edges += Q._both(j, i)
    validities = [(1 << nw) - 1] + [int(rng.integers(0, 1 << nw)) for _ in range(15)]
    node_validity = [int(v) if rng.random() < 0.3 else 0 for v in rng.integers(0, 16, n)]
    g = Q._graph([tuple(p) for p in xy.tolist()], node_validity, validities, edges)
    finals = [[int(rng.integers(0, n))] for _ in range(nw)]
    return g["children"], Q.costs_explicit(g, finals)


def random_table(seed, n, nw, deg, p_inf, lattice):
    """random children lists (duplicates included) over a random cost table with +inf entries; lattice: small integers, exact ties"""
    rng = np.random.default_rng(seed)
    children = [[int(v) for v in rng.integers(0, n, int(rng.integers(0, deg + 1)))] for _ in range(n)]
    if lattice:
        costs = rng.integers(0, 4, (nw, n)).astype(np.float64)
    else:
        costs = rng.uniform(0.0, 10.0, (nw, n))
    costs[rng.random((nw, n)) < p_inf] = INF
    return children, costs.tolist()


def tie_pair():
    """d = (1, -1), (-1, 1) for entry (0, 1): value exactly 0 at b = (.5, .5); and its mirror images"""
    children = [[1, 2, 3], [], [], []]
    costs = [[9.0, 2.0, 1.0, 3.0], [9.0, 2.0, 3.0, 1.0]]
    return children, costs


INPUTS = {
    "geo_w1": lambda: geometric(11, 120, 1, 0.17),
    "geo_w2": lambda: geometric(12, 120, 2, 0.17),
    "geo_w6": lambda: geometric(13, 110, 6, 0.17),
    "geo_w12": lambda: geometric(14, 100, 12, 0.17),
    "geo_w16": lambda: geometric(15, 100, 16, 0.17),
    "table_w2": lambda: random_table(21, 40, 2, 9, 0.15, False),
    "table_w6": lambda: random_table(22, 40, 6, 9, 0.15, False),
    "table_w16": lambda: random_table(23, 30, 16, 12, 0.1, False),
    "lattice_w2": lambda: random_table(31, 40, 2, 8, 0.1, True),
    "lattice_w6": lambda: random_table(32, 40, 6, 8, 0.1, True),
    "lattice_w12": lambda: random_table(33, 30, 12, 10, 0.05, True),
    "tie_pair": tie_pair,
}


@functools.lru_cache(maxsize=None)
def judged(name):
    """every entry of the input through the restatement, the exact oracle, and the f64 simplex with early stopping off"""
    children, costs = INPUTS[name]()
    costs = np.asarray(costs, dtype=np.float64)
    keep, how, piv = P.policy_graph(children, costs)
    rows = []
    e = 0
    for cs in children:
        ids = np.asarray(cs, dtype=np.int64)
        C = P.node_costs(costs, ids) if len(cs) else None
        for j in range(len(cs)):
            D, pos, nv = P.entry_rows(ids, C, j)
            v_exact, k_exact = P.exact_keep(D.tolist(), nv)
            err, scale = None, None
            if how[e] >= 3:
                _, _, v64, scale = P.simplex(D, pos, early_stop=False)
                err = abs(Fraction(v64) - v_exact) / Fraction(scale)
            elif len(D) and nv:
                scale = float(np.abs(D).max())
            rows.append((v_exact, k_exact, err, scale))
            e += 1
    return keep, how, piv, rows


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_restatement_against_exact(name):
    keep, how, piv, rows = judged(name)
    either = 0
    worst = Fraction(0)
    for e, (v, k, err, scale) in enumerate(rows):
        if v is None or v <= 0 or scale is None:
            assert bool(keep[e]) == k, (e, how[e], v)
        elif v > Fraction(2 * P.TOL) * Fraction(scale):
            assert not keep[e], (e, how[e], float(v), scale)
        else:
            either += 1
        if how[e] in (0, 2, 4):
            assert not k or (v is not None and v > 0)
        if err is not None:
            worst = max(worst, err)
    print("%s: %d entries, %d either way, %d at step 3, max pivots %d, worst |v64 - v*| / scale = %.3g"
          % (name, len(rows), either, int((how >= 3).sum()), int(piv.max()) if len(piv) else 0, float(worst)))
    assert either <= 0.02 * len(rows)
    assert not (how == 5).any()
    assert worst <= Fraction(ERR_BOUND)


def test_tie_pair_is_kept():
    """the pair (1,-1), (-1,1): no world and no rival decides, the simplex reaches value 0 exactly"""
    keep, how, _, rows = judged("tie_pair")
    assert rows[0][0] == 0 and how[0] == 3 and keep[0]


def test_every_class_occurs():
    seen = set()
    for name in INPUTS:
        seen |= set(int(h) for h in judged(name)[1])
    assert seen >= {0, 1, 2, 3, 4}, seen
