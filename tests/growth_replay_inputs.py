"""Inputs that drive the growth into its replays (tests/test_gpu_growth_replays.py) and the facts about them that the oracle can
state on the CPU (tests/test_growth_replay_inputs_cpu.py).

A growth is replayed when a neighbour list overflowed (-100, covered elsewhere), when a float draw of the device sampler would have
been redrawn (-101: again with the exact host stream), when the PTO edge pool overflowed (-102: option edge_per_node * 4) and when the
deferred-tie pool overflowed (-103: option tie_pool_ids, or the default pool, * 4).  Edge and tie pools are reached through the two
options; a redraw needs a sampling box whose upper bound is a rounding away from its samples, which is what the far boxes are."""
import cases
from oracle import orc

FAR36, FAR38 = float(2 ** 36), float(2 ** 38)      # an ulp there is 2^-16 / 2^-14 of a box 2 wide
N_FAR = 4000                                       # iterations of the far-box growths


def shifted(case, L):
    """the case on the box x in [L, L + 2), y in [-1, 1): raster, sampler, start and goals moved by L + 1 in x"""
    c = cases.Case(case)
    c.update(name="%s_at_%g" % (case.name, L), low=(L, -1.0), up=(L + 2.0, 1.0), start=(case.start[0] + L + 1.0, case.start[1]),
             goals=[(x + L + 1.0, y) for x, y in case.goals])
    return c


def redraw_calls(low, up, seed, n_calls):
    """the sampler calls (0-based, one call = x then y) of the first n_calls during which gen_range draws again: the stream's state
    after the call is not the state two steps on (orc_pcg64_advance), which is where the device sampler would look for the next call"""
    rng = orc.Pcg64.seed_from_u64(seed)
    out = []
    for k in range(n_calls):
        ahead = rng.copy()
        ahead.advance(2)
        rng.gen_range_f64(low[0], up[0])
        rng.gen_range_f64(low[1], up[1])
        if (rng.state() != ahead.state()).any():
            out.append(k)
    return out


def iteration_of_call(k):
    """the 1-based iteration of a grow that makes sampler call k (0-based): every 100th iteration takes the goal point and draws nothing"""
    it, calls = 0, -1
    while calls < k:
        it += 1
        if it % 100:
            calls += 1
    return it


def edge_pool(n_iter_max, per_node):
    """slots of the PTO edge pool of a fresh context: (n_iter_max + 2) * edge_per_node + 4096 asked, an eighth of headroom on top"""
    want = (n_iter_max + 2) * per_node + 4096
    return want, want + want // 8


def edge_replays(n_edges, n_iter_max, per_node=1):
    """(attempts that overflow, edge_per_node of the attempt that holds n_edges) from the pool's first size on, * 4 per replay"""
    replays = 0
    while edge_pool(n_iter_max, per_node)[1] < n_edges:
        per_node *= 4
        replays += 1
    return replays, per_node


# ---- the cases of the device tests, by name
def pto_1500(seed=0):
    return cases.cfg3(1500, 1500, seed=seed)


def pto_tail():
    return cases.cfg3(40, 9000)


def door_1500():
    return cases.cfg_door(1500, 1500)


def far_rrt(seed, L=FAR36):
    return shifted(cases.cfg1(N_FAR, seed=seed), L)


def far_pto(seed, L=FAR36):
    return shifted(cases.cfg3(N_FAR, N_FAR, seed=seed), L)


def far_tail(seed=44, L=FAR38):
    """n_iter_min 100, n_iter_max 4000 on the 2^38 box: the redraw of call 148 falls into the steps launched one by one.  The goal is
    cfg1's, far from the start: the growth is still looking for it at iteration 150"""
    c = shifted(cases.cfg1(N_FAR, seed=seed), L)
    c.update(n_iter_min=100, n_iter_max=N_FAR)
    return c
