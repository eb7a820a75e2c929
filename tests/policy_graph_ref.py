"""get_policy_graph (src/pto_graph.rs:363-419) three ways.

(a) exact_keep(rows): the game value v* = min_b max_o d_o . b over the simplex, and the decision v* <= 0, in fractions.Fraction
    (an active-set simplex under Bland's rule on exact rationals; an f64 is a rational).
(b) policy_graph(children, costs): the device procedure restated, operation for operation: steps 0-2 with
    numpy, step 3 with elementwise numpy operations only and every sum over worlds a serial loop in world order (np.sum and np.dot
    are pairwise or BLAS: never used on the way to a decision).
(c) KATS: the three answers the reference's own tests assert (pto_graph.rs:574-623), as data.

The LP of an entry (u, t): unknowns x = (b_w for w in V, v).  Constraints, each with an id (Bland's order):
    id w' (0 .. |V|-1)   b_w' >= 0                 (w' counts the worlds of V in world order)
    id 64 + j            d_j . b - v <= 0          (j: position of the rival in u's children list)
    EQ                   sum b = 1                 (always active)
A vertex has |V| + 1 active constraints, one per slot; M = A^-1, where row s of A is the active constraint of slot s; column s of
M is the direction that moves constraint s alone, and the last row of M holds the multipliers."""
from fractions import Fraction

import numpy as np

import qmdp_ref as Q

TOL = 1e-9                    # PORRT_POLICY_GRAPH_TOL
EPS = 1e-13                   # PORRT_POLICY_GRAPH_EPS: multipliers, pivot elements and rates below it (relative) count as zero
MAX_PIVOTS = 4096             # option "policy_graph_max_pivots"
RIVAL0 = 64                   # id of the rival at list position 0
INF = float("inf")


# ---------------------------------------------------------------- (a) the exact oracle
def exact_value(rows):
    """v* = min over b >= 0, sum b = 1 of max over rows d of d . b, exactly.  rows: sequences of n finite numbers (n >= 1).
    No rows: the maximum over nothing is -inf; returns None."""
    D = [[Fraction(x) for x in r] for r in rows]
    if not D:
        return None
    m, n = len(D), len(D[0])
    k = n + 1
    one, zero = Fraction(1), Fraction(0)
    o0 = max(range(m), key=lambda o: (D[o][0], -o))
    b = [zero] * n
    b[0] = one
    v = D[o0][0]
    M = [[zero] * k for _ in range(k)]
    M[n][0] = -one
    for j in range(1, n):
        M[j][j] = one
        M[0][j] = -one
        M[n][j] = D[o0][j] - D[o0][0]
    M[0][n] = one
    M[n][n] = D[o0][0]
    act = [RIVAL0 + o0] + list(range(1, n))
    while True:
        lam = M[n]
        cand = [s for s in range(n) if (lam[s] > 0 if act[s] >= RIVAL0 else lam[s] < 0)]
        if not cand:
            return v
        i = min(cand, key=lambda s: act[s])
        sgn = -1 if act[i] >= RIVAL0 else 1
        p = [sgn * M[w][i] for w in range(k)]
        best = None
        for w in range(n):
            if p[w] < 0 and w not in act:
                t = b[w] / -p[w]
                if best is None or (t, w) < best:
                    best = (t, w)
        for o in range(m):
            if RIVAL0 + o in act:
                continue
            g = sum(D[o][w] * p[w] for w in range(n)) - p[n]
            if g > 0:
                r = sum(D[o][w] * b[w] for w in range(n)) - v
                t = -r / g
                if best is None or (t, RIVAL0 + o) < best:
                    best = (t, RIVAL0 + o)
        assert best is not None, "the game value is bounded below"
        t, e = best
        b = [b[w] + t * p[w] for w in range(n)]
        v = v + t * p[n]
        a = [one if w == e else zero for w in range(n)] + [zero] if e < RIVAL0 else D[e - RIVAL0] + [-one]
        u = [sum(a[w] * M[w][s] for w in range(k)) for s in range(k)]
        mi = [M[w][i] / u[i] for w in range(k)]
        for w in range(k):
            for s in range(k):
                M[w][s] = mi[w] if s == i else M[w][s] - mi[w] * u[s]
        act[i] = e


def exact_keep(rows, n_valid=None):
    """(v*, kept).  rows are the rival rows over V; n_valid = |V| when there are no rows.  V empty: pruned; no rivals: kept."""
    if n_valid is None:
        n_valid = len(rows[0]) if len(rows) else 0
    if n_valid == 0:
        return None, False
    if not len(rows):
        return None, True
    v = exact_value(rows)
    return v, v <= 0


# ---------------------------------------------------------------- (b) the device procedure
def entry_rows(ids, C, j):
    """rival rows of entry j of a node: ids[m] the children list, C[m, W] their cost rows.  Returns (D[rivals, |V|], list positions of
    the rivals, |V|).  d = c[t] - c[o] where c[o] is finite, 0 where it is +inf."""
    ct = C[j]
    V = np.isfinite(ct)
    riv = np.nonzero(ids != ids[j])[0]
    Cr = C[riv][:, V]
    with np.errstate(invalid="ignore"):
        D = np.where(np.isfinite(Cr), ct[V][None, :] - Cr, 0.0)
    return D, riv, int(V.sum())


def classify_node(ids, C):
    """steps 0-2 for every entry of one node at once: how 0 / 1 / 2, or 255 for step 3.  ids[m], C[m, W]."""
    fin = np.isfinite(C)                                             # [entry or rival, world]
    V = fin[:, None, :]                                              # the entry's worlds
    rival = (ids[:, None] != ids[None, :])[:, :, None]               # [entry, rival, 1]
    with np.errstate(invalid="ignore"):
        D = np.where(fin[None, :, :], C[:, None, :] - C[None, :, :], 0.0)
    world_ok = (V[:, 0, :] & (~rival | (D <= 0.0)).all(axis=1)).any(axis=1)
    dominated = (rival[:, :, 0] & (~V | (D > 0.0)).all(axis=2)).any(axis=1)      # d is 0 where the rival is +inf: such a rival is finite on V
    how = np.full(len(ids), 255, dtype=np.uint8)
    how[dominated] = 2
    how[world_ok] = 1
    how[~fin.any(axis=1)] = 0
    return how


def simplex(D, pos, max_pivots=MAX_PIVOTS, tol=TOL, early_stop=True):
    """step 3 on the rows D[m, n] whose list positions are pos[m].  Returns (how, pivots, v, scale)."""
    m, n = D.shape
    k = n + 1
    scale = float(np.abs(D).max())
    lim = tol * scale
    col0 = D[:, 0]
    o0 = int(np.argmax(col0))                      # the first maximum
    v = float(col0[o0])
    b = np.zeros(n)
    b[0] = 1.0
    M = np.zeros((k, k))
    M[n, 0] = -1.0
    for j in range(1, n):
        M[j, j] = 1.0
        M[0, j] = -1.0
        M[n, j] = D[o0, j] - D[o0, 0]
    M[0, n] = 1.0
    M[n, n] = D[o0, 0]
    act = np.empty(n, dtype=np.int64)
    act[0] = RIVAL0 + pos[o0]
    act[1:] = np.arange(1, n)
    ids = RIVAL0 + np.asarray(pos, dtype=np.int64)
    pivots = 0
    while True:
        if early_stop and v <= lim:
            return 3, pivots, v, scale
        lam = M[n, :n]
        is_riv = act >= RIVAL0
        cand = np.where(is_riv, lam > EPS, lam < -(EPS * scale))
        if not cand.any():
            return (3 if v <= lim else 4), pivots, v, scale
        if pivots >= max_pivots:
            return 5, pivots, v, scale
        i = int(np.argmin(np.where(cand, act, 1 << 62)))
        p = -M[:, i] if is_riv[i] else M[:, i].copy()
        pb1, pmax = 0.0, 0.0
        for w in range(n):
            a = abs(float(p[w]))
            pb1 = pb1 + a
            pmax = a if a > pmax else pmax
        g_lim = EPS * (scale * pb1 + abs(float(p[n])))
        r = np.zeros(m)
        g = np.zeros(m)
        for w in range(n):
            r = r + D[:, w] * b[w]
            g = g + D[:, w] * p[w]
        r = r - v
        g = g - p[n]
        ok = (g > g_lim) & ~np.isin(ids, act)
        best_t, best_id = INF, -1
        okb = (p[:n] < -(EPS * pmax)) & ~np.isin(np.arange(n), act)
        for w in np.nonzero(okb)[0]:                                  # ids ascending: the first minimum is the lowest id
            t = (b[w] if b[w] > 0.0 else 0.0) / -p[w]
            if t < best_t:
                best_t, best_id = float(t), int(w)
        if ok.any():
            num = np.where(-r > 0.0, -r, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(ok, num / g, INF)
            o = int(np.argmin(t))                                     # rivals after bounds, positions ascending
            if t[o] < best_t:
                best_t, best_id = float(t[o]), int(ids[o])
        if best_id < 0:
            return 5, pivots, v, scale                                # nothing blocks (rounding): undecided, kept
        b = b + best_t * p[:n]
        v = v + best_t * float(p[n])
        if best_id < RIVAL0:
            u = M[best_id, :].copy()
        else:
            d = D[int(np.nonzero(ids == best_id)[0][0])]
            u = np.zeros(k)
            for w in range(n):
                u = u + d[w] * M[w, :]
            u = u - M[n, :]
        mi = M[:, i] / u[i]
        M = M - mi[:, None] * u[None, :]
        M[:, i] = mi
        act[i] = best_id
        b[act[act < RIVAL0]] = 0.0                                    # an active bound holds exactly
        pivots += 1


def node_costs(costs, ids):
    """C[m, W] for the children list ids from world-major costs[W][n]"""
    return np.ascontiguousarray(np.asarray(costs, dtype=np.float64)[:, ids].T)


def policy_graph(children, costs, max_pivots=MAX_PIVOTS, tol=TOL, sample=None):
    """keep, how, pivots per adjacency entry in push order.  costs[w][id].  sample = (seed, count): when more than count entries
    reach step 3, it is run on a seeded choice of count of them and the others keep how 255."""
    costs = np.asarray(costs, dtype=np.float64)
    first = np.concatenate([[0], np.cumsum([len(c) for c in children])]).astype(np.int64)
    how = np.zeros(first[-1], dtype=np.uint8)
    piv = np.zeros(first[-1], dtype=np.uint32)
    for u, cs in enumerate(children):
        if len(cs):
            ids = np.asarray(cs, dtype=np.int64)
            how[first[u]:first[u + 1]] = classify_node(ids, node_costs(costs, ids))
    todo = np.nonzero(how == 255)[0]
    if sample is not None and len(todo) > sample[1]:
        todo = np.sort(np.random.default_rng(sample[0]).choice(todo, sample[1], replace=False))
    node, ids, C = -1, None, None
    for e in todo.tolist():
        u = int(np.searchsorted(first, e, side="right")) - 1
        if u != node:
            node, ids = u, np.asarray(children[u], dtype=np.int64)
            C = node_costs(costs, ids)
        D, pos, _ = entry_rows(ids, C, e - int(first[u]))
        how[e], piv[e], _, _ = simplex(D, pos, max_pivots, tol)
    return np.isin(how, (1, 3, 5)), how, piv


def pruned_children(children, keep):
    out, e = [], 0
    for cs in children:
        out.append([c for j, c in enumerate(cs) if keep[e + j]])
        e += len(cs)
    return out


def remove_edges(children, parents, keep):
    """PTOGraph::remove_edge (pto_graph.rs:214-217) for every pruned entry, on copies"""
    ch = [list(c) for c in children]
    pa = [list(p) for p in parents]
    e = 0
    for u, cs in enumerate(children):
        for j, t in enumerate(cs):
            if not keep[e + j]:
                ch[u] = [x for x in ch[u] if x != t]
                pa[t] = [x for x in pa[t] if x != u]
        e += len(cs)
    return ch, pa


# ---------------------------------------------------------------- (c) the reference's asserted answers
def _diamond_graph():
    """pto_graph.rs:512-537"""
    e = Q._both(0, 1) + Q._both(0, 3) + Q._both(0, 2) + Q._both(1, 3) + Q._both(2, 3)
    return Q._graph([(0.0, 0.0), (1.0, 1.0), (1.0, -1.0), (2.0, 0.0)], [0] * 4, [1], e)


def _kat_diamond():
    g = _diamond_graph()
    return g["children"], Q.costs_explicit(g, [[3]])                                  # :581


def _kat_diamond_2_worlds():
    g = Q.diamond_graph_2_worlds()
    return g["children"], Q.costs_explicit(g, [[3], [3]])                             # :597-598


def _kat_grid_2_goals():
    g = Q.grid_graph()
    return g["children"], Q.costs_explicit(g, [[2]]) + Q.costs_explicit(g, [[5]])     # :614-615: both over world view 0


# name -> (children and costs, {node: the children the reference asserts})
KATS = {
    "diamond": (_kat_diamond, {0: [3], 1: [3], 2: [3]}),
    "diamond_2_worlds": (_kat_diamond_2_worlds, {3: [1, 2], 1: [3], 2: [3]}),
    "grid_2_goals": (_kat_grid_2_goals, {3: [0, 4], 4: [1, 5], 8: [5]}),
}
