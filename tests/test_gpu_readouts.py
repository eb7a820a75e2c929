"""The tree read-outs on crafted trees (tests/readout_inputs.py): porrt_best_cost / porrt_best_cost_batch (k_best_cost and the host walk
behind it), porrt_best_paths (k_best_path, tamp_gather) and porrt_solutions (k_solutions_select / k_solutions_write) on trees that a
random stream never grows -- hundreds of solutions in a row, final paths beyond k_best_cost's scratch, bit-equal least costs within
one thread and across threads, best paths at the slot limit -- alone and as rows of one porrt_grow_batch_each.

Every comparison is by bit pattern against the oracle's tree, its best_solution and tests/solutions_ref.py on it; nothing has a
tolerance.  Each test first compares the device's tree with the oracle's, and asserts from the oracle's side that the tree holds what
the test is for (tests/test_readout_inputs_cpu.py shows the same conditions without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import cases
import readout_inputs as R
import solutions_ref
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

NOT_TRACKED = (1 << 64) - 1                 # porrt_best_cost's final_id after the host walk ("not tracked by the host fallback")
ERR_CAPACITY = -5


@pytest.fixture(scope="module")
def po():
    import po_rrt_amd
    return po_rrt_amd


class Twin:
    """the oracle's side of a case, made once and read only: its tree, counters, solutions, best path"""

    def __init__(self, name):
        self.case = R.case(name)
        self.o = R.grow_oracle(self.case)
        self.k = R.Counters.of(self.o)
        self.solutions = solutions_ref.of_oracle(self.o)
        self.best = self.o.best_solution()                       # (path, cost) or None
        assert R.is_clean(self.case, self.o)
        print(self.k.line(self.case))


@pytest.fixture(scope="module")
def twin():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Twin(name)
        return made[name]
    yield get
    made.clear()


def fresh(po, c):
    e = cases.configure(po.Engine(0), c)
    e.set_samples(c.samples)
    return e


def alone(po, t):
    """a fresh context grown alone on the twin's case, its tree compared with the oracle's"""
    e = fresh(po, t.case)
    cases.grow(e, t.case, K=1)
    assert_same(e, t.o)
    return e


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_solutions(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert np.array_equal(bits(g[1]), bits(w[1])), "states of solution %d" % w[0]
        assert bits(g[2]) == bits(w[2]), "cost of solution %d" % w[0]


def same_best_path(got, want):
    """an entry of Engine.best_paths against Oracle.best_solution"""
    if want is None:
        assert got is None
        return
    assert got is not None and np.array_equal(bits(got[0]), bits(want[0])) and bits(got[1]) == bits(want[1])


def best_cost(e):
    """porrt_best_cost through the C ABI: (return code, cost, final_id)"""
    cost, fid = C.c_double(-1.0), C.c_uint64(12345)
    r = e._l.porrt_best_cost(e._c, C.byref(cost), C.byref(fid))
    return r, cost.value, fid.value


def want_cost(t):
    return np.inf if t.best is None else t.best[1]


# ---------------------------------------------------------------------------------------------------------------- solutions
@pytest.mark.parametrize("name", R.SOLUTION_CASES + ("fan_overflow", "tie_three"))
def test_solutions(po, twin, name):
    """one, two and three trips of kSolThreads solutions through both kernels (exactly 256: no partial trip; 257: a last trip of one),
    a row of two-state solutions, none, and rows with fewer solutions than final nodes"""
    t = twin(name)
    T, n = R.SOLUTION_THREADS, t.k.n_solutions
    assert {"comb_256": n == T, "comb_257": n == T + 1, "comb_3_trips": n > 2 * T, "no_goal": n == 0, "fan_overflow": n == t.case.get("n_fan"),
            "start_in_goal": n == t.case.get("n_ring") and all(len(p) == 2 for _, p, _ in t.solutions),
            "tie_three": n < len(t.k.final_ids)}[name]
    assert len(t.solutions) == n
    e = alone(po, t)
    same_solutions(e.solutions(), t.solutions)
    same_solutions(e.solutions(), t.solutions)                   # again: the arena's cursor starts anew


def test_solutions_caps_one_short(po, twin):
    """porrt_solutions on the row with more than 512 solutions: the counts, PORRT_ERR_CAPACITY with either cap one short, then all"""
    t = twin("comb_3_trips")
    assert t.k.n_solutions > 2 * R.SOLUTION_THREADS
    e = alone(po, t)
    L, arr = e._l, (C.c_void_p * 1)(e._c)
    ns, nst = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    assert L.porrt_solutions(arr, 1, ns.ctypes.data, nst.ctypes.data, None, None, None, 0, None, 0) == 0
    assert ns.tolist() == [t.k.n_solutions] and nst.tolist() == [t.k.solution_states]
    n, X = int(ns[0]), int(nst[0])
    ids, lens, costs, xy = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n), np.zeros((X, 2))
    a = (ids.ctypes.data, lens.ctypes.data, costs.ctypes.data)
    assert L.porrt_solutions(arr, 1, None, None, *a, n - 1, xy.ctypes.data, X) == ERR_CAPACITY
    assert L.porrt_solutions(arr, 1, None, None, *a, n, xy.ctypes.data, X - 1) == ERR_CAPACITY
    assert not ids.any() and not lens.any() and not costs.any() and not xy.any()              # nothing was written short
    assert L.porrt_solutions(arr, 1, None, None, *a, n, xy.ctypes.data, X) == 0
    assert ids.tolist() == [i for i, _, _ in t.solutions] and lens.tolist() == [len(p) for _, p, _ in t.solutions]
    assert np.array_equal(bits(costs), bits([c for _, _, c in t.solutions]))
    assert np.array_equal(bits(xy), bits(np.concatenate([p for _, p, _ in t.solutions])))


# ---------------------------------------------------------------------------------------------------------------- best cost
@pytest.mark.parametrize("name", R.TIE_CASES + ("path_1024", "path_1025", "start_in_goal"))
def test_best_cost_device_path_keeps_the_lowest_tied_id(po, twin, name):
    """k_best_cost under bit-equal least costs: a thread's strict `<` over t, t + 1024, ..., the reduction's lower id across threads"""
    t = twin(name)
    m, W = t.k.min_ids, R.BEST_COST_THREADS
    assert len(m) >= 2 and t.k.final_states <= R.scratch_bound(t.case.n_iter_max)
    assert {"tie_lower_thread": m[0] % W > m[1] % W, "tie_same_thread": (m[1] - m[0]) % W == 0,
            "tie_three": len(m) == 3 and (m[2] - m[0]) % W == 0 and m[1] % W != m[0] % W}.get(name, True)
    assert np.array_equal(t.best[0][-1], t.o.tree()[0][m[0]])    # the oracle's first minimum is the lowest id
    e = alone(po, t)
    r, cost, fid = best_cost(e)
    assert r == 1 and bits(cost) == bits(t.best[1])
    assert fid == m[0], "k_best_cost chose %d of the tied %s" % (fid, m)
    assert bits(po.Engine.best_cost_batch([e])[0]) == bits(t.best[1])
    if t.k.best_len <= R.SLOT:
        same_best_path(po.Engine.best_paths([e])[0], t.best)     # k_best_path walks from the id that k_best_cost chose


@pytest.mark.parametrize("name", ["fan_overflow", "comb_257", "fan_fits", "no_goal"])
def test_best_cost_beyond_the_scratch_walks_on_the_host(po, twin, name):
    """final paths of twice the scratch and more: BestCost::overflow, read_best_cost's -1 and the host walk, whose mark is final_id = ~0;
    far below the bound the device answers with the id"""
    t = twin(name)
    over = t.k.final_states > R.scratch_bound(t.case.n_iter_max)
    if name in ("fan_overflow", "comb_257"):
        assert t.k.final_states >= 2 * R.scratch_bound(t.case.n_iter_max)
    else:
        assert 2 * t.k.final_states <= R.scratch_bound(t.case.n_iter_max)
    e = alone(po, t)
    r, cost, fid = best_cost(e)
    if t.best is None:
        assert r == 0 and e.best_cost() is None and np.isinf(po.Engine.best_cost_batch([e])[0])
        assert po.Engine.best_paths([e]) == [None]
        return
    assert r == 1 and bits(cost) == bits(t.best[1])
    assert fid == (NOT_TRACKED if over else t.k.min_ids[0])
    assert bits(e.best_cost()) == bits(t.best[1])
    assert bits(po.Engine.best_cost_batch([e])[0]) == bits(t.best[1])            # a context outside a run: porrt_best_cost again
    same_best_path(po.Engine.best_paths([e])[0], t.best)                          # tamp_gather's status 2: porrt_best_solution's path
    assert best_cost(e) == (r, cost, fid)


# ---------------------------------------------------------------------------------------------------------------- best paths
def test_best_paths_at_the_slot_limit(po, twin):
    """kTampPathSlot = 1024 states: a best path of exactly that comes back whole; one state more is PORRT_ERR_CAPACITY with the slot's
    message, and nothing is written -- not for the row before it either"""
    t0, t1 = twin("path_1024"), twin("path_1025")
    assert t0.k.best_len == R.SLOT == len(t0.best[0]) and t1.k.best_len == R.SLOT + 1 == len(t1.best[0])
    e0, e1 = alone(po, t0), alone(po, t1)
    got = po.Engine.best_paths([e0])[0]
    assert len(got[0]) == R.SLOT
    same_best_path(got, t0.best)
    with pytest.raises(po.engine.PorrtError) as ex:
        po.Engine.best_paths([e1])
    assert ex.value.code == ERR_CAPACITY and "slot of %d states" % R.SLOT in str(ex.value)
    L = e0._l
    for engs in ([e1], [e0, e1], [e1, e0]):
        arr = (C.c_void_p * len(engs))(*[e._c for e in engs])
        lens, costs, xy = np.full(len(engs), 77, dtype=np.uint64), np.full(len(engs), -3.0), np.full((3 * R.SLOT, 2), -7.0)
        assert L.porrt_best_paths(arr, len(engs), xy.ctypes.data, len(xy), lens, costs) == ERR_CAPACITY
        assert (lens == 77).all() and (costs == -3.0).all() and (xy == -7.0).all()
    same_best_path(po.Engine.best_paths([e0])[0], t0.best)       # the context is as good as before
    r, cost, fid = best_cost(e1)                                 # the cost has no slot
    assert r == 1 and bits(cost) == bits(t1.best[1]) and fid == t1.k.min_ids[0]


# ---------------------------------------------------------------------------------------------------------------- batches
@pytest.fixture(scope="module")
def batch(po, twin):
    """one porrt_grow_batch_each at K = 1: a stream and an iteration count per row; and the same cases grown alone"""
    ts = [twin(n) for n in R.BATCH_ROWS]
    es = [fresh(po, t.case) for t in ts]
    its = [t.case.n_iter_min for t in ts]
    po.Engine.grow_batch(es, [t.case.start for t in ts], R.S, R.SEARCH_RADIUS, its, 1, n_iter_max=[t.case.n_iter_max for t in ts])
    singles = [alone(po, t) for t in ts]
    return ts, es, singles


def check_readouts(po, engs, ts):
    """the three batch calls on engs against the twins ts, row by row"""
    for got, t in zip(po.Engine.solutions_batch(engs), ts):
        same_solutions(got, t.solutions)
    for got, t in zip(po.Engine.best_cost_batch(engs), ts):
        assert bits(got) == bits(want_cost(t)), t.case.name
    for got, t in zip(po.Engine.best_paths(engs), ts):
        same_best_path(got, t.best)


def test_batch_rows_match_their_twins_and_their_single_grows(po, batch):
    ts, es, singles = batch
    counts = [t.k.n_solutions for t in ts]
    over = [t.k.final_states > R.scratch_bound(t.case.n_iter_max) for t in ts]
    assert counts[1] == 0 and counts[0] > R.SOLUTION_THREADS and counts[2] > 0 and counts[4] > 2 * R.SOLUTION_THREADS
    assert over[3] and not over[2] and not over[5] and len(ts[2].k.min_ids) == 3
    its = [e.num_iterations() for e in es]
    assert len(set(its)) == len(es)
    # (a row that has ended is carried along to the last step of the longest row: its per-step arrays must hold the batch's steps.
    # Sized by its own budget they were overrun by some 1500 entries here, and the growth ended in PORRT_ERR_DEVICE.)
    assert max(its) - min(its) > 1500
    for e, t in zip(es, ts):
        assert_same(e, t.o)
    check_readouts(po, es, ts)
    sol_b, sol_s = po.Engine.solutions_batch(es), po.Engine.solutions_batch(singles)
    for b, s in zip(sol_b, sol_s):
        same_solutions(b, s)
    assert np.array_equal(bits(po.Engine.best_cost_batch(es)), bits(po.Engine.best_cost_batch(singles)))
    for b, s in zip(po.Engine.best_paths(es), po.Engine.best_paths(singles)):
        same_best_path(b, s)
    for e, s, t in zip(es, singles, ts):                         # and every member through the single calls
        same_solutions(e.solutions(), t.solutions)
        assert best_cost(e) == best_cost(s)
        r, cost, fid = best_cost(e)
        if t.best is None:
            assert r == 0
        else:
            over_t = t.k.final_states > R.scratch_bound(t.case.n_iter_max)
            assert r == 1 and bits(cost) == bits(t.best[1]) and fid == (NOT_TRACKED if over_t else t.k.min_ids[0])


def test_batch_rows_in_another_order_and_among_other_contexts(po, batch):
    ts, es, singles = batch
    n = len(es)
    order = list(range(n))[::-1]
    check_readouts(po, [es[k] for k in order], [ts[k] for k in order])
    order[1], order[4] = order[4], order[1]
    check_readouts(po, [es[k] for k in order], [ts[k] for k in order])
    # the run in the middle of singly grown contexts and of members out of their places
    mixed = [singles[3], es[4], singles[0]] + es + [es[2], singles[1]]
    check_readouts(po, mixed, [ts[3], ts[4], ts[0]] + ts + [ts[2], ts[1]])
    check_readouts(po, es + es, ts + ts)                         # the run twice in one call


def test_repeated_and_interleaved_calls_give_the_same(po, batch):
    """best_cost, solutions, best_paths, best_cost again: the cursors (bc_cursor, the arenas') are reset by every call"""
    ts, es, singles = batch
    for engs in (es, singles, [es[3], singles[3], es[0]]):
        tw = ts if len(engs) == len(ts) else [ts[3], ts[3], ts[0]]
        first = po.Engine.best_cost_batch(engs)
        singly = [best_cost(e) for e in engs]
        check_readouts(po, engs, tw)
        check_readouts(po, engs, tw)
        assert np.array_equal(bits(po.Engine.best_cost_batch(engs)), bits(first))
        assert [best_cost(e) for e in engs] == singly
        for got, t in zip(first, tw):
            assert bits(got) == bits(want_cost(t))
