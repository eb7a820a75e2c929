"""Explicit belief graphs for conditional_dijkstra (src/belief_graph.rs:89-175): seeded random generators and crafted graphs, as data.
Plain Python and numpy; shared by tests/test_dp_graphs_cpu.py (the oracle against sweeps) and tests/test_gpu_dp_explicit.py (the device
against the oracle).  Every function returns the dictionary of tests/kat_graphs.py: xy, belief_vec, beliefs, belief_id (= belief_vec),
types, children, parents, finals.

The contract: `parents` is the transpose of `children`, in the order the edges are added (BeliefGraph::add_edge, belief_graph.rs:60-63,
pushes both).  The reference relaxes an action parent from the parents list of the popped node and the device pulls it from its own
children list, so a graph in which the two lists disagree is outside what either side promises; no generator here makes one."""
import numpy as np

A, O = 1, 2          # BeliefNodeType::Action / Observation (belief_graph.rs:13-17)


def _graph(xy, bvec, beliefs, types, edges, finals):
    n = len(types)
    children = [[] for _ in range(n)]
    parents = [[] for _ in range(n)]
    for a, b in edges:                       # BeliefGraph::add_edge
        children[a].append(int(b))
        parents[b].append(int(a))
    bvec = [int(b) for b in bvec]
    return dict(xy=[[float(x), float(y)] for x, y in xy], belief_vec=bvec, belief_id=list(bvec), beliefs=[[float(p) for p in r] for r in beliefs],
                types=[int(t) for t in types], children=children, parents=parents, finals=[int(f) for f in finals])


def is_transpose(g):
    """parents holds the edges of children, each as often as there (a parents row is in the order its edges were added, which the
    children rows alone do not tell: rows are compared as multisets)"""
    parents = [[] for _ in g["types"]]
    for u, row in enumerate(g["children"]):
        for v in row:
            parents[v].append(u)
    return len(parents) == len(g["parents"]) and all(sorted(a) == sorted(b) for a, b in zip(parents, g["parents"]))


def with_children(g, children):
    """the same graph with other children lists (a permutation of each row, say): parents rebuilt as their transpose"""
    parents = [[] for _ in g["types"]]
    for u, row in enumerate(children):
        for v in row:
            parents[v].append(u)
    return dict(g, children=[list(r) for r in children], parents=parents)


# ------------------------------------------------------------------------------------------------------ seeded generators

SHAPED_SIZES = [(3, 1), (3, 2), (3, 3), (20, 1), (20, 2), (20, 3), (20, 6), (20, 12), (60, 2), (60, 3), (60, 6), (60, 12), (60, 64),
                (150, 3), (150, 12), (150, 64)]


def shaped(seed, n_places, n_worlds):
    """Shaped like the planner's belief graph: nodes are (place, belief row) pairs; the rows come from repeated random two-way splits of
    a Dirichlet prior's support (at most 48 rows); action nodes keep the row and change the place (fan 0..4; a few places are copies of
    others, which gives zero-length edges); observation nodes keep the place and go to the two rows of their row's split; finals are
    most rows of a few goal places."""
    rng = np.random.default_rng([seed, n_places, n_worlds, 1])
    prior = rng.dirichlet(np.ones(n_worlds))
    supports, split = [list(range(n_worlds))], [None]
    k = 0
    while k < len(supports) and len(supports) + 2 <= 48:
        s = supports[k]
        if len(s) >= 2:
            s = [int(w) for w in rng.permutation(s)]
            cut = int(rng.integers(1, len(s)))
            split[k] = (len(supports), len(supports) + 1)
            supports += [sorted(s[:cut]), sorted(s[cut:])]
            split += [None, None]
        k += 1
    beliefs = np.zeros((len(supports), n_worlds))
    for r, s in enumerate(supports):
        beliefs[r, s] = prior[s] / prior[s].sum()
    place_xy = rng.uniform(-1.0, 1.0, (n_places, 2))
    copies = []
    for _ in range(1 + n_places // 10):                                   # copied places: edges of length zero
        a, b = (int(v) for v in rng.choice(n_places, 2, replace=False))
        place_xy[b] = place_xy[a]
        copies.append((a, b))
    R = len(supports)
    node_of = -np.ones((n_places, R), dtype=np.int64)
    xy, bvec = [], []
    for p in range(n_places):
        for r in range(R):
            if R == 1 or rng.random() < 0.75:
                node_of[p, r] = len(xy)
                xy.append(place_xy[p]); bvec.append(r)
    n = len(xy)
    types = [A] * n
    for p in range(n_places):
        for r in range(R):
            if node_of[p, r] >= 0 and split[r] and node_of[p, split[r][0]] >= 0 and node_of[p, split[r][1]] >= 0 and rng.random() < 0.25:
                types[node_of[p, r]] = O
    edges = []
    for p in range(n_places):
        for r in range(R):
            u = node_of[p, r]
            if u < 0:
                continue
            if types[u] == O:
                edges += [(u, node_of[p, split[r][0]]), (u, node_of[p, split[r][1]])]
                continue
            for q in rng.choice(n_places, int(rng.integers(0, 5))):
                v = node_of[int(q), r]
                if v < 0 or v == u:
                    continue
                edges.append((u, v))
                if types[v] == A and rng.random() < 0.6:
                    edges.append((v, u))
    for a, b in copies:                                                   # both ways between a place and its copy, in most rows
        for r in range(R):
            u, v = node_of[a, r], node_of[b, r]
            if u >= 0 and v >= 0 and types[u] == A and types[v] == A and rng.random() < 0.7:
                edges += [(u, v), (v, u)]
    finals = []
    for p in rng.choice(n_places, 1 + n_places // 20, replace=False):
        finals += [int(node_of[int(p), r]) for r in range(R) if node_of[int(p), r] >= 0 and rng.random() < 0.8]
    return _graph(xy, bvec, beliefs, types, edges, finals)


ARBITRARY_SIZES = [(1, 1), (2, 2), (17, 3), (64, 1), (64, 12), (255, 2), (256, 3), (257, 12), (600, 64), (600, 3), (3000, 12), (3000, 2)]


def arbitrary(seed, n, n_worlds):
    """Random types (about a quarter observation nodes); action children anywhere, 0..5 of them, duplicates allowed; observation nodes
    have 1..6 children among the nodes whose support is a strict subset of their own, so that p > 0; a few zero-length pairs linked
    both ways."""
    rng = np.random.default_rng([seed, n, n_worlds, 2])
    R = min(24, 1 << n_worlds) if n_worlds < 5 else 24
    masks = [np.ones(n_worlds, dtype=bool)]
    while len(masks) < R:
        m = rng.random(n_worlds) < rng.uniform(0.2, 0.9)
        if not m.any():
            m[int(rng.integers(n_worlds))] = True
        masks.append(m)
    beliefs = np.zeros((len(masks), n_worlds))
    for r, m in enumerate(masks):
        beliefs[r, m] = rng.dirichlet(np.ones(int(m.sum())))
    below = [[s for s in range(len(masks)) if not (masks[s] & ~masks[r]).any() and (masks[r] & ~masks[s]).any()] for r in range(len(masks))]
    bvec = rng.integers(0, len(masks), n)
    by_row = [np.flatnonzero(bvec == r) for r in range(len(masks))]
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    types, edges = [A] * n, []
    pairs = []
    for _ in range(min(n // 2, 1 + n // 40)):
        a, b = (int(v) for v in rng.choice(n, 2, replace=False))
        xy[b] = xy[a]
        pairs.append((a, b))
    paired = {v for p in pairs for v in p}
    cands = [np.concatenate([by_row[s] for s in b]) if b else np.zeros(0, dtype=np.int64) for b in below]
    for u in range(n):
        cand = cands[bvec[u]]
        if len(cand) and u not in paired and rng.random() < 0.25:
            types[u] = O
            edges += [(u, int(v)) for v in rng.choice(cand, int(rng.integers(1, 7)))]
        else:
            edges += [(u, int(v)) for v in rng.integers(0, n, int(rng.integers(0, 6)))]
    for a, b in pairs:
        edges += [(a, b), (b, a)]
    finals = rng.choice(n, max(1, n // 16), replace=False)
    return _graph(xy, bvec, beliefs, types, edges, finals)


CYCLIC_SIZES = [(8, 2), (30, 3), (120, 3), (120, 12), (400, 2), (400, 12)]


def cyclic(seed, n, n_worlds):
    """Every node has 1..4 children anywhere, observation nodes included: cycles run through the sums.  Rows of full support and copies
    of them with random zeros that keep world 0, so every transition probability is positive."""
    rng = np.random.default_rng([seed, n, n_worlds, 3])
    full = rng.dirichlet(np.ones(n_worlds), 4)
    rows = [r for r in full]
    for r in full:
        for _ in range(2):
            c = r.copy()
            c[1:][rng.random(n_worlds - 1) < 0.5] = 0.0
            rows.append(c)
    bvec = rng.integers(0, len(rows), n)
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    types = [O if rng.random() < 0.25 else A for _ in range(n)]
    edges = [(u, int(v)) for u in range(n) for v in rng.integers(0, n, int(rng.integers(1, 5)))]
    finals = rng.choice(n, max(1, n // 12), replace=False)
    return _graph(xy, bvec, rows, types, edges, finals)


# ------------------------------------------------------------------------------------------------------ crafted graphs

CHAIN_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 100]


def chain(L, ascending):
    """L action edges in a row to one final: the cost of the far end arrives after exactly L sweeps.  ascending: the final is node L and
    node k's child is k + 1; else the final is node 0 and node k's child is k - 1."""
    ids = list(range(L + 1)) if ascending else list(range(L, -1, -1))          # ids[k] = the node k edges away from the far end
    xy = [[0.0, 0.0]] * (L + 1)
    for k, i in enumerate(ids):
        xy[i] = [0.125 * k, 0.0]
    edges = [(ids[k], ids[k + 1]) for k in range(L)]
    return _graph(xy, [0] * (L + 1), [[1.0]], [A] * (L + 1), edges, [ids[L]])


def contraction(q):
    """A cycle through a sum: observation node 0 (row [q, 1 - q], at the origin) has children 1 and 2; action node 1 (row [1, 0], same
    place) has children 0 and final 3, at distance 10; node 2 is a final at distance 1 with row [0, 1].  d1 = min(d0, 10) and
    d0 = q * d1 + (1 - q) * 1 contract to d0 = d1 = 1 at the rate q per two sweeps."""
    xy = [[0.0, 0.0], [0.0, 0.0], [1.0, 0.0], [0.0, 10.0]]
    return _graph(xy, [0, 1, 2, 1], [[q, 1.0 - q], [1.0, 0.0], [0.0, 1.0]], [O, A, A, A], [(0, 1), (0, 2), (1, 0), (1, 3)], [2, 3])


def wide_rows():
    """Four degenerate rows: observation node 0 with 300 children (rows repeat among them), action node 1 with 2 000 children, final 2
    with 3 000 parents, node 3 listing one child three times."""
    rng = np.random.default_rng(77)
    beliefs = [[0.25, 0.25, 0.5], [0.5, 0.5, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]
    xy, bvec, types, edges = [[0.0, 0.0], [0.5, 0.5], [-1.0, 0.25], [0.25, -0.5]], [0, 1, 2, 1], [O, A, A, A], []
    for j in range(300):                                                   # node 0's children: rows 1..3, every one below row 0
        xy.append([float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1))]); bvec.append(1 + j % 3); types.append(A)
        edges.append((0, len(xy) - 1))
    for j in range(2000):
        xy.append([float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1))]); bvec.append(1); types.append(A)
        edges.append((1, len(xy) - 1))
    first = 4
    for v in range(first, first + 2300):                                   # every one of those, and 700 more, is a parent of final 2
        edges.append((v, 2))
    for j in range(700):
        xy.append([float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1))]); bvec.append(2); types.append(A)
        edges.append((len(xy) - 1, 2))
    edges += [(3, 1), (3, 1), (3, 1)]
    return _graph(xy, bvec, beliefs, types, edges, [2])


NEVER_EVALUATED = ["unknown_type", "zero_probability"]


def never_evaluated(which, evaluated):
    """Nodes the reference would fail on if it ever relaxed them: a node of type 0 (node 2; "node type should be know at this stage!",
    oracle code -1), an observation node whose child has a disjoint support (node 3; assert!(p > 0.0), code -2), an observation node
    without children (node 6).  All sit only above node 4, which stays at +inf, so they are never touched.  evaluated: the one named by
    `which` also gets child 1, which is finite, and the reference fails."""
    beliefs = [[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]]
    #      0 final    1 finite    2 type 0   3 obs       4 island   5 above 2, 3  6 obs, no children
    xy = [[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [2.0, 1.0], [3.0, 0.0], [2.0, 2.0], [0.0, 3.0]]
    bvec = [0, 0, 0, 1, 2, 0, 0]
    types = [A, A, 0, O, A, A, O]
    edges = [(1, 0), (2, 4), (3, 4), (5, 2), (5, 3), (5, 6)]
    if evaluated:
        edges.append(({"unknown_type": 2, "zero_probability": 3}[which], 1))
    return _graph(xy, bvec, beliefs, types, edges, [0])


def final_with_children():
    """A final observation node (1) and a final action node (2) whose children improve later: a final stays at 0 (no alternative is
    smaller).  Chain 5 -> 4 -> 3 -> 0 (final); 1 -> {3, 6}, 2 -> {5, 4}; 7 above both."""
    beliefs = [[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]]
    xy = [[0.0, 0.0], [1.0, 1.0], [2.0, 1.0], [0.5, 0.0], [1.0, 0.0], [1.5, 0.0], [1.0, 2.0], [3.0, 3.0]]
    bvec = [1, 0, 0, 1, 0, 0, 2, 0]
    types = [A, O, A, A, A, A, A, A]
    edges = [(3, 0), (4, 3), (5, 4), (1, 3), (1, 6), (6, 0), (2, 5), (2, 4), (7, 1), (7, 2)]
    return _graph(xy, bvec, beliefs, types, edges, [0, 1, 2])


def islands():
    """What stays at +inf: a component without a final (nodes 2, 3, 4), a two-node zero-length action cycle that no final reaches
    (5, 6), an observation node with one finite and one infinite child (7 -> {1, 5})."""
    beliefs = [[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]]
    xy = [[0.0, 0.0], [1.0, 0.0], [5.0, 5.0], [6.0, 5.0], [6.0, 6.0], [-3.0, 1.0], [-3.0, 1.0], [1.0, 1.0], [2.0, 2.0]]
    bvec = [1, 1, 0, 0, 0, 2, 2, 0, 0]
    types = [A, A, A, O, A, A, A, O, A]
    edges = [(1, 0), (2, 3), (3, 4), (4, 2), (5, 6), (6, 5), (7, 1), (7, 5), (8, 7)]
    return _graph(xy, bvec, beliefs, types, edges, [0])


# ------------------------------------------------------------------------------------------------------ the whole set

def all_inputs():
    """(name, graph-making function) of every input that has an answer (never_evaluated with evaluated = True has an error instead)"""
    out = []
    for k, (p, w) in enumerate(SHAPED_SIZES):
        out.append(("shaped-%d-%d" % (p, w), lambda k=k, p=p, w=w: shaped(k, p, w)))
    for k, (n, w) in enumerate(ARBITRARY_SIZES):
        out.append(("arbitrary-%d-%d" % (n, w), lambda k=k, n=n, w=w: arbitrary(k, n, w)))
    for k, (n, w) in enumerate(CYCLIC_SIZES):
        out.append(("cyclic-%d-%d" % (n, w), lambda k=k, n=n, w=w: cyclic(k, n, w)))
    for L in CHAIN_LENGTHS:
        out.append(("chain-%d-up" % L, lambda L=L: chain(L, True)))
        out.append(("chain-%d-down" % L, lambda L=L: chain(L, False)))
    out += [("contraction-0.5", lambda: contraction(0.5)), ("contraction-0.9", lambda: contraction(0.9)), ("wide_rows", wide_rows),
            ("final_with_children", final_with_children), ("islands", islands)]
    out += [("never_evaluated-" + w, lambda w=w: never_evaluated(w, False)) for w in NEVER_EVALUATED]
    return out


INPUTS = dict(all_inputs())
