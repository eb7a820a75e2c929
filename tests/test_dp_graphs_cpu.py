"""The reference side of tests/dp_graphs.py, CPU only: on every input the oracle's queue-driven conditional_dijkstra (oracle/dp.c)
equals, bit for bit, the Gauss-Seidel sweeps of tests/test_oracle_dp.py and Jacobi sweeps (every node evaluated from the previous
sweep's values: the extreme of the device's schedule) -- the order-independence DESIGN.md 10 rests on.  Then each input's teeth: that
it makes the sweeps do what it is there for, asserted from the oracle's output and the sweep counts alone."""
import numpy as np
import pytest

import dp_graphs
import policies_ref as ref
from oracle import orc
from test_oracle_dp import sweep_fixpoint

SWEEP_NODES = 1500             # the plain-Python Gauss-Seidel sweeps run on graphs up to this size
JACOBI_CAP = 4000              # sweeps; the slowest input (contraction(0.9)) needs about 700


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle(g):
    return orc.conditional_dijkstra(g["xy"], g["belief_vec"], g["beliefs"], g["types"], g["children"], g["parents"], g["finals"])


def jacobi(g, coff, cid, cap=JACOBI_CAP):
    """(dist, number of sweeps that changed something).  The operations of sweep_fixpoint, per edge and in children order, vectorised
    over the nodes; a node of type 0 or without children is skipped, as there."""
    n = len(g["types"])
    xy = np.asarray(g["xy"], dtype=np.float64).reshape(-1, 2)
    beliefs = np.asarray(g["beliefs"], dtype=np.float64)
    bvec = np.asarray(g["belief_vec"], dtype=np.int64)
    types = np.asarray(g["types"])
    coff = coff.astype(np.int64)
    deg = np.diff(coff)
    cid = cid[:coff[-1]].astype(np.int64)
    src = np.repeat(np.arange(n), deg)
    dx, dy = xy[cid, 0] - xy[src, 0], xy[cid, 1] - xy[src, 1]
    cost = np.sqrt(0.0 + dx * dx + dy * dy)
    p = np.zeros(len(cid))
    for w in range(beliefs.shape[1]):                            # transition_probability, summed in world order
        p = p + np.where(beliefs[bvec[cid], w] > 0.0, beliefs[bvec[src], w], 0.0)
    act = np.flatnonzero((types == 1) & (deg > 0))
    obs = np.flatnonzero((types == 2) & (deg > 0))                 # (a node without children is never relaxed: it has no child to be popped)
    act_edges = np.flatnonzero(types[src] == 1)
    d = np.full(n, np.inf)
    d[np.asarray(g["finals"], dtype=np.int64)] = 0.0
    sweeps = 0
    with np.errstate(invalid="ignore"):
        while True:
            alt = np.full(n, np.inf)                                 # (type 0, and an action node without children)
            term = 0.0 + (cost + d[cid])
            if len(act):                                             # an action node's edges are one run of act_edges
                alt[act] = np.minimum.reduceat(term[act_edges], np.searchsorted(act_edges, coff[act]))
            acc = np.zeros(len(obs))
            for k in range(int(deg[obs].max()) if len(obs) else 0):   # the sum, child after child
                has = deg[obs] > k
                e = coff[obs[has]] + k
                acc[has] = acc[has] + p[e] * (cost[e] + d[cid[e]])
            alt[obs] = acc
            better = alt < d
            if not better.any():
                return d, sweeps
            d = np.where(better, alt, d)
            sweeps += 1
            assert sweeps <= cap, "no fixpoint after %d Jacobi sweeps" % cap


@pytest.fixture(scope="module")
def solved():
    """name -> (graph, oracle dist, children CSR, Jacobi sweeps): computed once, read by every test below"""
    out = {}
    for name, mk in dp_graphs.INPUTS.items():
        g = mk()
        d, (coff, cid), _ = oracle(g)
        dj, sweeps = jacobi(g, coff, cid)
        assert np.array_equal(bits(d), bits(dj)), "%s: Jacobi sweeps and the queue disagree" % name
        out[name] = (g, d, (coff, cid), sweeps)
    return out


def test_every_parents_list_is_the_transpose(solved):
    for name, (g, _, _, _) in solved.items():
        assert dp_graphs.is_transpose(g), name
    for which in dp_graphs.NEVER_EVALUATED:
        assert dp_graphs.is_transpose(dp_graphs.never_evaluated(which, True))
    g = dp_graphs.INPUTS["shaped-20-3"]()
    assert dp_graphs.is_transpose(dp_graphs.with_children(g, [r[::-1] for r in g["children"]]))
    u = next(u for u, r in enumerate(g["parents"]) if r)              # and the check has teeth: one parent entry dropped, one doubled
    assert not dp_graphs.is_transpose(dict(g, parents=[r[1:] if v == u else r for v, r in enumerate(g["parents"])]))
    assert not dp_graphs.is_transpose(dict(g, parents=[r + r[:1] if v == u else r for v, r in enumerate(g["parents"])]))


def test_queue_equals_gauss_seidel_sweeps(solved):
    ran = 0
    for name, (g, d, (coff, cid), _) in solved.items():
        if len(d) > SWEEP_NODES:
            continue
        with np.errstate(invalid="ignore"):
            d2 = sweep_fixpoint(g["xy"], g["belief_vec"], g["beliefs"], g["types"], coff, cid, g["finals"])
        assert np.array_equal(bits(d), bits(d2)), name
        ran += 1
    assert ran >= 50


def test_set_sizes(solved):
    """the sizes the generators are there for: beside a 256-thread block's edge, several blocks, one node"""
    sizes = {name: len(d) for name, (_, d, _, _) in solved.items()}
    assert {sizes["arbitrary-%d-%d" % s] for s in dp_graphs.ARBITRARY_SIZES} == {1, 2, 17, 64, 255, 256, 257, 600, 3000}
    assert max(sizes.values()) == sizes["shaped-150-64"] and 4000 < sizes["shaped-150-64"] < 7000
    g = solved["shaped-150-64"][0]
    assert len(g["beliefs"]) <= 48 and len(g["beliefs"][0]) == 64
    w = solved["wide_rows"][0]
    assert len(w["children"][0]) == 300 and len(w["children"][1]) == 2000 and len(w["parents"][2]) == 3000 and w["children"][3] == [1, 1, 1]


@pytest.mark.parametrize("L", dp_graphs.CHAIN_LENGTHS)
def test_chain_needs_exactly_L_sweeps(solved, L):
    for way in ("up", "down"):
        g, d, _, sweeps = solved["chain-%d-%s" % (L, way)]
        assert sweeps == L
        far = 0 if way == "up" else L
        assert d[far] == 0.125 * L and np.isfinite(d).all() and (d == 0.0).sum() == 1


def test_contraction_converges_slowly(solved):
    for q in (0.5, 0.9):
        _, d, _, sweeps = solved["contraction-%s" % q]
        assert sweeps > 64
        assert d[1] == d[0] and d[2] == 0.0 and d[3] == 0.0
    assert solved["contraction-0.5"][1][0] == 1.0
    assert solved["contraction-0.9"][1][0] > 1.0                 # the limit in f64 is not the real one: the last bits are the schedule's to keep


def test_some_cyclic_graph_needs_more_than_a_group_of_sweeps(solved):
    sweeps = [s for name, (_, _, _, s) in solved.items() if name.startswith("cyclic")]
    assert max(sweeps) > 8
    n_obs_in_cycles = 0
    for name, (g, d, _, _) in solved.items():
        if name.startswith("cyclic"):
            t = np.asarray(g["types"])
            n_obs_in_cycles += int(((t == 2) & np.isfinite(d) & (d > 0.0)).sum())
    assert n_obs_in_cycles >= 20


def test_shaped_graphs_have_sums_and_policies(solved):
    """sums that matter, and policies (belief_id = belief_vec) of all four kinds: most finite starts have one (status 0), the zero-length
    pairs give walks that return to their own path (2), a row that sums to a little more than 1 over a zero-length edge fails
    assert!(p * dist[best] <= dist[node]) (3)"""
    counts, sums = np.zeros(5, dtype=np.int64), 0
    for name, (g, d, (coff, cid), _) in solved.items():
        if not name.startswith("shaped"):
            continue
        t = np.asarray(g["types"])
        here = int(((t == 2) & np.isfinite(d) & (d > 0.0)).sum())
        sums += here
        G = ref.Graph(g["xy"], g["belief_vec"], g["beliefs"], g["belief_vec"], coff, cid[:int(coff[-1])])
        status = np.array([w[0] for w in ref.extract_policies(G, d, range(len(d)))])
        assert np.array_equal(status == ref.NO_COST, np.isinf(d))
        if len(d) >= 100:                                          # (the three-place graphs have a handful of finite nodes)
            assert here >= 1, name
            assert (status == ref.OK).sum() * 2 >= np.isfinite(d).sum(), name
        counts += np.bincount(status, minlength=5)
    assert sums >= 200
    assert counts[0] * 2 >= counts[0] + counts[2] + counts[3] + counts[4]
    assert counts[0] > 1000 and counts[1] > 1000 and counts[2] > 50 and counts[3] > 50, counts


@pytest.mark.parametrize("which,code", [("unknown_type", -1), ("zero_probability", -2)])
def test_never_evaluated(solved, which, code):
    g, d, _, _ = solved["never_evaluated-" + which]
    assert np.isinf(d[2:]).all() and d[0] == 0.0 and d[1] == 1.0
    with pytest.raises(RuntimeError, match=r"\(%d\)" % code):
        oracle(dp_graphs.never_evaluated(which, True))


def test_finals_and_islands(solved):
    g, d, _, _ = solved["final_with_children"]
    assert d[1] == 0.0 and d[2] == 0.0 and d[5] == 1.5 and d[7] > 0.0 and np.isfinite(d).all()
    g, d, _, _ = solved["islands"]
    assert np.isinf(d[2:]).all() and d[1] == 1.0
