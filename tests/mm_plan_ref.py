"""A numpy restatement of MapShelfDomainTampPRM::build_belief_graph (src/map_shelves_tamp_prm.rs:395-473) on the dict grow_mm_prm
returns (oracle or engine), then the oracle's conditional_dijkstra and extract_policy on the explicit graph (:475-485).

Belief node id = mode offset + roadmap node; every node carries its mode's belief vector (row = mode index) and the belief id of that
belief (its index in reachable_belief_states), which is what get_best_expected_children clusters by."""
import numpy as np

from oracle import orc

ACTION, OBSERVATION = 1, 2


def roadmap_children(n, efrom, eto):
    """PTONode::children of a PRM roadmap: for each new node in order, add_edge(nbr, new) for its neighbours, then add_edge(new, nbr)
    (prm.rs:96-103); the forward list holds the neighbour -> new edges grouped by new node"""
    ch = [[] for _ in range(n)]
    efrom, eto = np.asarray(efrom, dtype=np.int64), np.asarray(eto, dtype=np.int64)
    starts = np.flatnonzero(np.r_[True, eto[1:] != eto[:-1]]) if len(eto) else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], len(eto)]
    for a, b in zip(starts, ends):
        new = int(eto[a])
        nbrs = efrom[a:b].tolist()
        for f in nbrs:
            ch[f].append(new)
        ch[new].extend(nbrs)
    return ch


def build_belief_graph(g, reachable, belief_hash):
    """g: grow_mm_prm's dict; reachable: reachable_belief_states of the prior [n, n_worlds]; belief_hash: common.rs:352-355.
    Returns dict(xy, belief_vec, beliefs, belief_ids, types, children, parents, finals, mode_offsets)."""
    id_of = {belief_hash(b): k for k, b in enumerate(reachable)}
    modes = g["modes"]
    sizes = [len(m["xy"]) for m in modes]
    off = np.zeros(len(modes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(sizes)
    N = int(off[-1])
    xy = np.concatenate([np.asarray(m["xy"], dtype=np.float64).reshape(-1, 2) for m in modes]) if N else np.zeros((0, 2))
    beliefs = np.array([m["belief"] for m in modes], dtype=np.float64)
    belief_vec = np.repeat(np.arange(len(modes), dtype=np.uint32), sizes)
    mode_bid = np.array([id_of[belief_hash(m["belief"])] for m in modes], dtype=np.uint32)     # (a missing one: the reference panics)
    belief_ids = mode_bid[belief_vec]
    types = np.full(N, ACTION, dtype=np.uint8)
    children, parents = [[] for _ in range(N)], [[] for _ in range(N)]
    finals = [int(off[k]) + int(f) for k, m in enumerate(modes) for f in m["finals"]]
    for t in g["transitions"]:                                          # observation edges (:421-438)
        for a, b in np.asarray(t["pairs"], dtype=np.int64).reshape(-1, 2):
            assert a < sizes[t["from_mode"]] and b < sizes[t["to_mode"]], "a pair names a missing node (the reference panics)"
            u, v = int(off[t["from_mode"]]) + int(a), int(off[t["to_mode"]]) + int(b)
            children[u].append(v)
            parents[v].append(u)
            types[u] = OBSERVATION
    for k, m in enumerate(modes):                                       # action edges (:441-470)
        o = int(off[k])
        ch = roadmap_children(sizes[k], m["edges"][0], m["edges"][1])
        for node in range(sizes[k]):
            u = o + node
            if types[u] == OBSERVATION:
                continue
            for c in ch[node]:
                children[u].append(o + c)
                parents[o + c].append(u)
    return dict(xy=xy, belief_vec=belief_vec, beliefs=beliefs, belief_ids=belief_ids, types=types, children=children, parents=parents,
                finals=np.array(finals, dtype=np.uint64), mode_offsets=off)


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    ids = np.array([v for x in lists for v in x], dtype=np.uint32)
    return off, ids


def expected_costs(bg):
    """conditional_dijkstra (belief_graph.rs:89-175) on the oracle: dist per belief node"""
    dist, _, _ = orc.conditional_dijkstra(bg["xy"], bg["belief_vec"], bg["beliefs"], bg["types"], bg["children"], bg["parents"], bg["finals"])
    return dist


def extract_policy(bg, dist, cap=1 << 16):
    """extract_policy (belief_graph.rs:177-263) from belief node 0: (belief node ids, parents, leaf flags)"""
    return orc.extract_policy(bg["xy"], bg["belief_ids"], bg["belief_vec"], bg["beliefs"], csr(bg["children"]), dist, cap)


def plan(oracle, start, belief, max_step, search_radius, n_iter_per_belief):
    """MapShelfDomainTampPRM::plan up to the expected costs on the oracle: (grow dict, belief graph, dist)"""
    g = oracle.grow_mm_prm(start, belief, max_step, search_radius, n_iter_per_belief)
    bg = build_belief_graph(g, oracle.reachable_beliefs(belief), oracle.belief_hash)
    return g, bg, expected_costs(bg)
