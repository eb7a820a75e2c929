"""CPU side of the read-out inputs (tests/readout_inputs.py): every crafted tree reaches what it was built for, shown from the oracle's
tree alone.  These are conditions, not measurements: tests/test_gpu_readouts.py relies on them (and asserts them again on the trees it
compares), so that a read-out kernel's second trip, the scratch overflow, the tie rules and the slot limit are met and not assumed.
Each test prints the case's counters."""
import numpy as np
import pytest

import readout_inputs as R
import solutions_ref


@pytest.fixture(scope="module")
def grown(oracle_lib):
    """(case, oracle, counters) of a name, grown once per module; read only"""
    made = {}

    def get(name):
        if name not in made:
            c = R.case(name)
            o = R.grow_oracle(c)
            made[name] = (c, o, R.Counters.of(o))
            print(made[name][2].line(c))
        return made[name]
    yield get
    made.clear()


def test_counters_on_a_small_tree():
    """a tree written out by hand: 0 - 1 - 2 - 3, 1 - 4, 0 - 5; final 2, 3, 4, 5 (3 below 2); node 1 was rewired under node 5"""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [1.0, 1.0], [0.5, 0.0]])
    parent = np.array([-1, 5, 1, 2, 1, 0])
    k = R.Counters(xy, parent, [2, 3, 4, 5])
    assert k.depth.tolist() == [1, 3, 4, 5, 4, 2]
    assert k.firstly_final == [2, 4, 5] and k.n_solutions == 3 and k.solution_states == 4 + 4 + 2
    assert k.final_states == 4 + 5 + 4 + 2
    assert k.min_ids == [5] and k.best_cost == 0.5 and k.best_len == 2
    assert k.costs.tolist() == [2.0, 3.0, 2.0, 0.5]
    tied = R.Counters(xy, parent, [2, 4])
    assert tied.min_ids == [2, 4] and tied.best_len == 4
    none = R.Counters(xy, parent, [])
    assert none.n_solutions == 0 and none.final_states == 0 and none.min_ids == [] and none.best_cost is None
    assert R.scratch_bound(1000) == 8 * 1002 + 4096


def test_stream_ids_skip_the_goal_iterations():
    st = R.Stream()
    ids = [st.add(k, 0) for k in range(250)]
    assert ids[:3] == [1, 2, 3] and ids[98:101] == [99, 101, 102] and 100 not in ids and 200 not in ids and ids[-1] == 252
    st.fill_to(299, R.walk(0.0, 0.0, 0.0, -1.0))
    assert st.add(0, 0) == 299 and st.add(0, 0) == 301
    with pytest.raises(AssertionError):
        st.fill_to(400, R.walk(0.0, 0.0, 0.0, -1.0))
    assert len(st.xy()) == st.iteration - st.iteration // 100


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_streams_are_clean_and_fit_one_batch(grown, name):
    """nothing steered, nothing refused: ids are stream positions; one max_step and one search_radius (a batch has one of each); at
    most about 2000 steps"""
    c, o, k = grown(name)
    assert R.is_clean(c, o)
    assert len(c.samples) == c.n_iter_min - c.n_iter_min // 100
    assert c.max_step == R.S and c.search_radius == R.SEARCH_RADIUS and c.n_iter_min <= 2000
    assert o.final_ids().tolist() == sorted(o.final_ids().tolist())          # push order is id order: "first minimum" is the lowest id
    assert np.array_equal(o.firstly_final_ids(), np.array(k.firstly_final, dtype=np.uint64))


def test_solution_counts(grown):
    """exactly 256 and 257 solutions (one trip of kSolThreads and one more), more than 512 (a third trip, with a running base twice),
    none"""
    T = R.SOLUTION_THREADS
    assert grown("comb_256")[2].n_solutions == T and grown("comb_257")[2].n_solutions == T + 1
    assert grown("comb_3_trips")[2].n_solutions > 2 * T
    for name in ("comb_256", "comb_257", "comb_3_trips"):
        c, o, k = grown(name)
        assert k.n_solutions >= c.teeth and len(k.final_ids) >= k.n_solutions
        assert len(set(int(k.depth[f]) for f in k.firstly_final)) > T // 2                   # lengths of every size: the scan's offsets matter
    c, o, k = grown("no_goal")
    assert len(k.final_ids) == 0 and k.n_solutions == 0


def test_start_in_goal(grown):
    """every node but the root is final, the root is not; every child of the root is a solution of two states"""
    c, o, k = grown("start_in_goal")
    parent = o.tree()[1]
    assert k.final_ids == list(range(1, o.num_nodes()))
    children = np.flatnonzero(parent == 0).tolist()
    assert k.firstly_final == children and len(children) == c.n_ring and len(k.final_ids) > len(children)
    assert all(k.depth[f] == 2 for f in children)
    assert [len(p) for _, p, _ in solutions_ref.of_oracle(o)] == [2] * c.n_ring


def test_scratch_overflow_and_its_opposite(grown):
    """the final paths of one fan are twice the scratch bound and more, those of the other half of it and less"""
    c, o, k = grown("fan_overflow")
    assert k.final_states >= 2 * R.scratch_bound(c.n_iter_max) and len(k.final_ids) == c.n_fan
    assert k.best_len <= R.SLOT                                                              # (the host walk's path is handed out whole)
    c, o, k = grown("fan_fits")
    assert 2 * k.final_states <= R.scratch_bound(c.n_iter_max) and len(k.final_ids) == c.n_fan
    for name in ("comb_256", "comb_257", "comb_3_trips"):                                    # the combs overflow it as well
        c, o, k = grown(name)
        assert k.final_states >= 2 * R.scratch_bound(c.n_iter_max)
    for name in ("start_in_goal",) + R.TIE_CASES + ("path_1024", "path_1025"):
        c, o, k = grown(name)
        assert 2 * k.final_states <= R.scratch_bound(c.n_iter_max)


@pytest.mark.parametrize("name", R.TIE_CASES)
def test_ties_at_the_minimum(grown, name):
    c, o, k = grown(name)
    W = R.BEST_COST_THREADS
    assert k.min_ids == c.tied and len(set(k.costs.view(np.uint64).tolist())) == 1
    a, b = k.min_ids[0], k.min_ids[-1]
    if name == "tie_lower_thread":
        assert len(k.min_ids) == 2 and a < b and a % W > b % W                               # a reduction that prefers the lower thread picks b
    elif name == "tie_same_thread":
        assert len(k.min_ids) == 2 and (b - a) % W == 0 and b > a                            # one thread folds both: its strict `<` keeps a
    else:
        m = k.min_ids
        assert len(m) == 3 and (m[2] - m[0]) % W == 0 and m[0] % W != m[1] % W
    x = o.tree()[0]
    path, cost = o.best_solution()
    assert cost == k.best_cost and len(path) == k.best_len
    assert np.array_equal(path[-1], x[a])
    others = [f for f in k.min_ids[1:] if not np.array_equal(x[f], x[a])]
    assert others, "every tied final node sits where the lowest does: the path's end does not tell them apart"
    assert 2 * k.final_states <= R.scratch_bound(c.n_iter_max)                               # the device answers


def test_best_paths_at_the_slot_limit(grown):
    for name, want in (("path_1024", R.SLOT), ("path_1025", R.SLOT + 1)):
        c, o, k = grown(name)
        assert k.best_len == want and len(o.best_solution()[0]) == want
        assert len(k.min_ids) == 2                                                           # the mirror pair again: the winner is the lower id


def test_batch_rows(grown):
    """the batch of the GPU file: a row without solutions between rows with hundreds, an overflowed row beside rows that fit, iteration
    counts of their own"""
    rows = [grown(n) for n in R.BATCH_ROWS]
    counts = [k.n_solutions for _, _, k in rows]
    over = [k.final_states > R.scratch_bound(c.n_iter_max) for c, _, k in rows]
    assert counts[1] == 0 and counts[0] > R.SOLUTION_THREADS and counts[4] > 2 * R.SOLUTION_THREADS
    assert True in over and False in over and over[3] and not over[2]
    assert len(set(c.n_iter_min for c, _, _ in rows)) == len(rows)
