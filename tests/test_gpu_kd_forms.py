"""The kd tie-order side chain in every form, on streams that make the ties it is there for.

The RRT* growth orders equal-cost parents by the reference's kd pre-order; the device keeps that order in a structure built beside the
steps (k_kd_locate, k_kd_link, k_kd_claim, k_kd_hint, k_kd_hint_fix, k_tie_fix).  A dozen options choose how it is built and launched
-- kd_lazy, kd_after, kd_ride, kd_inline, kd_group, kd_claim_threads, pipeline, batch_streams, graph -- and the structure only changes a
tree when two candidate parents have bit-equal cost.  The inputs here (tests/exact_inputs.py, "kd forms") make such ties in every
step: lattice samples (different places at one cost), a staircase whose kd-tree is one chain (every new node of a group bids for the
same child slot; copies at one place) and exact duplicates.  tests/test_kd_forms_inputs_cpu.py shows from the oracle alone that they
do, and that the oracle's kd-accelerated contract equals its brute-force definition on them.

Every comparison is with the oracle through assert_same: bits, and n_tie_fallbacks == 0.  Nothing has a tolerance.  Which form a run
launched is read from the view "kd_forms_run" (include/porrt_hip.h; the bits below are the header's): every case asserts the bits its
form must set and that no bit of another form is set, and the last test asserts that the module reached every bit.  "tie_records" and
"tie_pooled_ids" are printed for every case; they are asserted only where the code makes them certain (kd_after: every tie waits for
the structure) -- elsewhere they depend on how far the side stream got.
"""
import numpy as np
import pytest

import cases
import exact_inputs as X
from oracle import orc
from test_gpu_launch_sequences import DEFAULTS, SEQUENCE
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

# the bits of "kd_forms_run"
BITS = ["claim_one_2048", "claim_one_max", "claim_rows_1024x256", "claim_rows_1024x512", "claim_rows_1024x1024", "claim_rows_2048x256",
        "claim_rows_2048x512", "claim_rows_2048x1024", "claim_rows_maxx512", "claim_rows_maxx1024", "claim_single_side", "locate_1",
        "locate_64", "hints_ride", "hint", "hint_fix", "tie_fix_beside", "built_after"]
BIT = {name: 1 << k for k, name in enumerate(BITS)}
ALL = (1 << len(BITS)) - 1
CLAIM_ROWS = sum(v for k, v in BIT.items() if k.startswith("claim_rows"))
LOCATE = BIT["locate_1"] | BIT["locate_64"]
SEEN = {}            # case label -> the masks it read: the last test takes their union


def names(mask):
    return "+".join(n for n in BITS if mask & BIT[n]) or "none"


def claim_rows(nodes, threads=0):
    """the instantiation k_kd_claim<CAP, false, TPB> for a group of `nodes` nodes per row: the smallest CAP that holds them, the option's
    workgroup size (0: 256), 512 at the least for the largest CAP"""
    cap = "1024" if nodes <= 1024 else "2048" if nodes <= 2048 else "max"
    tpb = max(threads or 256, 512 if cap == "max" else 256)
    return BIT["claim_rows_%sx%d" % (cap, tpb)]


def locate(nodes_all_rows):
    return BIT["locate_1"] if nodes_all_rows >= 4096 else BIT["locate_64"]


def check_mask(label, e, required, allowed):
    """the leader's view: every required bit, nothing outside required | allowed"""
    mask = e.get_option("kd_forms_run")
    SEEN.setdefault(label, []).append(mask)
    print("%s: kd_forms_run %s" % (label, names(mask)))
    assert mask & required == required, "%s: %s not launched (ran %s)" % (label, names(required & ~mask), names(mask))
    assert mask & ~(required | allowed) == 0, "%s: %s launched as well" % (label, names(mask & ~(required | allowed)))
    return mask


def report_ties(label, engs):
    rec, ids = [e.get_option("tie_records") for e in engs], [e.get_option("tie_pooled_ids") for e in engs]
    print("%s: tie_records %s, tie_pooled_ids %s" % (label, rec, ids))
    return rec


def beside(e):
    """the whole structure beside the steps was in force, and no build after them"""
    assert e.get_option("kd_lazy") == 0 and e.get_option("kd_built_after") == 0


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


@pytest.fixture(scope="module")
def oracle():
    """the oracle's tree of a key (stream, seed, K, n_iter_min, n_iter_max), made once per module and dropped with it; read only"""
    made = {}

    def get(stream, seed, K, n_min, n_max=None):
        key = (stream, seed, K, n_min, n_min if n_max is None else n_max)
        if key not in made:
            case, xy = X.kd_forms_inputs(stream, seed, key[3], key[4])
            o = cases.configure(orc.Oracle(), case)
            o.set_samples(xy)
            cases.grow(o, case, K=K, algo=orc.ALGO_BATCHED_KD)
            made[key] = o
        return made[key]
    yield get
    made.clear()


def engine(eng_mod, stream, seed, n_min, n_max=None, **opts):
    case, xy = X.kd_forms_inputs(stream, seed, n_min, n_min if n_max is None else n_max)
    e = cases.configure(eng_mod.Engine(), case)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_samples(xy)
    return e, case


def grow_batch(eng_mod, engs, case, K, n_min=None, n_max=None):
    n_min = case.n_iter_min if n_min is None else n_min
    assert eng_mod.Engine.grow_batch(engs, [case.start] * len(engs), case.max_step, case.search_radius, n_min, K, n_iter_max=n_max) == 0


# ---------------------------------------------------------------------------------------------------------------- claim and locate forms
@pytest.mark.parametrize("threads", [0, 256, 512, 1024])
@pytest.mark.parametrize("K", sorted(X.KDF_CLAIM))
def test_claim_forms_batch_of_eight(eng_mod, oracle, K, threads):
    """eight rows, kd_lazy = 0: (K, kd_group) sets a group's nodes (128, 1024, 2048, 4096), kd_claim_threads the workgroup -- the eight
    instantiations k_kd_claim<CAP, false, TPB>; two full groups and a short last one at least"""
    g, n = X.KDF_CLAIM[K]
    engs = [engine(eng_mod, "lattice", s, n, kd_lazy=0, kd_group=g, kd_claim_threads=threads)[0] for s in X.KDF_SEEDS]
    case = X.kd_forms_inputs("lattice", 0, n, n)[0]
    grow_batch(eng_mod, engs, case, K)
    label = "claim K %d group %d threads %d" % (K, g, threads)
    assert engs[0].get_option("group_lanes") == 16
    beside(engs[0])
    check_mask(label, engs[0], claim_rows(g * K, threads) | locate(g * K * 8) | BIT["hint"] | BIT["tie_fix_beside"], CLAIM_ROWS | LOCATE)
    report_ties(label, engs)
    for s, e in zip(X.KDF_SEEDS, engs):
        assert_same(e, oracle("lattice", s, K, n))


def test_locate_one_wave_per_node_two_rows(eng_mod, oracle):
    """k_kd_locate<64> runs when a group has fewer than 4096 nodes over all rows: two rows at K = 64 through the group kernels"""
    K, seeds, n = X.KDF_LOCATE64
    engs = [engine(eng_mod, "lattice", s, n, kd_lazy=0, group_lanes=16)[0] for s in seeds]
    case = X.kd_forms_inputs("lattice", 0, n, n)[0]
    grow_batch(eng_mod, engs, case, K)
    assert engs[0].get_option("group_lanes") == 16
    beside(engs[0])
    check_mask("locate<64> two rows", engs[0], BIT["locate_64"] | claim_rows(8 * K) | BIT["hint"] | BIT["tie_fix_beside"], CLAIM_ROWS)
    report_ties("locate<64> two rows", engs)
    for s, e in zip(seeds, engs):
        assert_same(e, oracle("lattice", s, K, n))


# ---------------------------------------------------------------------------------------------------------------- chain variants
# options, beside the steps?, bits required, bits allowed beside them (Q = 9, K = 256: groups of 8 steps = 2048 nodes a row)
VARIANTS = {
    "kd_lazy=0": (dict(kd_lazy=0), True, claim_rows(2048) | BIT["locate_1"] | BIT["hint"] | BIT["tie_fix_beside"], CLAIM_ROWS | LOCATE),
    "kd_ride": (dict(kd_lazy=0, kd_ride=1), True, claim_rows(2048) | BIT["locate_1"] | BIT["hints_ride"], CLAIM_ROWS | LOCATE),
    "kd_inline": (dict(kd_lazy=0, kd_inline=1), True, claim_rows(2048) | BIT["locate_1"] | BIT["hint_fix"], CLAIM_ROWS | LOCATE),
    "kd_after": (dict(kd_after=1), True, claim_rows(2048) | BIT["locate_1"] | BIT["hint"] | BIT["built_after"], CLAIM_ROWS | LOCATE),
    "kd_lazy=1": (dict(kd_lazy=1, kd_claim_threads=512), False, 0, BIT["claim_rows_1024x512"] | BIT["claim_rows_2048x512"] | LOCATE | BIT["hint"] | BIT["built_after"]),
}


def check_variant(label, variant, lead, engs, must_build):
    opts, is_beside, required, allowed = VARIANTS[variant]
    rec = report_ties(label, engs)
    if is_beside:
        beside(lead)
        check_mask(label, lead, required, allowed)
        if variant == "kd_after":
            assert all(r > 0 for r in rec), "kd_after: every tie waits for the structure"
    else:
        # the goal path beside the steps; the structure after them if a tie off the goal path asked, for the steps up to the last such tie
        mask = check_mask(label, lead, 0, allowed)
        assert lead.get_option("kd_lazy") == 1
        built = lead.get_option("kd_built_after")
        print("%s: kd_built_after %d" % (label, built))
        assert built == (1 if mask & BIT["built_after"] else 0)
        if must_build:
            assert built == 1 and mask & BIT["hint"] and mask & LOCATE and mask & (BIT["claim_rows_1024x512"] | BIT["claim_rows_2048x512"])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_chain_variants_lattice_batch_of_nine(eng_mod, oracle, variant):
    K, n = X.KDF_VARIANT_K, X.KDF_VARIANT_ITERS
    engs = [engine(eng_mod, "lattice", s, n, **VARIANTS[variant][0])[0] for s in X.KDF_VARIANT_SEEDS]
    grow_batch(eng_mod, engs, X.kd_forms_inputs("lattice", 0, n, n)[0], K)
    assert engs[0].get_option("group_lanes") == 16
    check_variant("lattice nine rows, " + variant, variant, engs[0], engs, must_build=True)
    for s, e in zip(X.KDF_VARIANT_SEEDS, engs):
        assert_same(e, oracle("lattice", s, K, n))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_chain_variants_staircase_batch_of_nine(eng_mod, oracle, variant):
    """nine rows fed the same staircase: a kd-tree of one chain as deep as the tree has nodes, so that nearly every new node of a group
    bids for the same child slot -- the claim kernel's rounds and its same-point tail.  Rows 0 and 8 against the oracle."""
    K, n = X.KDF_CHAIN_K, X.KDF_CHAIN_ITERS
    engs = [engine(eng_mod, "chain", 0, n, **VARIANTS[variant][0])[0] for _ in range(9)]
    grow_batch(eng_mod, engs, X.kd_forms_inputs("chain", 0, n, n)[0], K)
    assert engs[0].get_option("group_lanes") == 16
    check_variant("staircase nine rows, " + variant, variant, engs[0], engs, must_build=False)
    o = oracle("chain", 0, K, n)
    for j in (0, 8):
        assert_same(engs[j], o)


# ---------------------------------------------------------------------------------------------------------------- single query
SINGLE_FORMS = {
    "pipeline=0": dict(pipeline=0),
    "pipeline=1": dict(pipeline=1),
    "pipeline=2": dict(pipeline=2),
    "pipeline=4": dict(pipeline=4, kd_lazy=0),
    "group_lanes=16": dict(group_lanes=16, kd_lazy=0),
}


@pytest.mark.parametrize("key", X.KDF_SINGLE, ids=lambda k: "%s-K%d" % (k[0], k[2]))
@pytest.mark.parametrize("form", sorted(SINGLE_FORMS))
def test_single_query_forms(eng_mod, oracle, form, key):
    """one query, the whole structure beside the steps: the side stream's claim with the new nodes' coordinates in LDS (pipeline 0, 1, 4,
    the group kernels), the persistent loop's chain with the two plain claims (pipeline 2).  Twice on one context -- the second grow
    replays the captured sequence and reports the capture's forms -- and once more launch by launch (graph = 0)."""
    stream, seed, K, n = key
    e, case = engine(eng_mod, stream, seed, n, **SINGLE_FORMS[form])
    xy = X.kd_forms_inputs(stream, seed, n, n)[1]
    o = oracle(stream, seed, K, n)
    group = min(8, 4096 // K) * K                                  # a single query's group: as many steps as the claim kernel holds
    assert n > group, "two groups at least: the first one's hints ride in the second one's locate kernel"
    if form == "pipeline=2":
        required = (BIT["claim_one_2048"] if group <= 2048 else BIT["claim_one_max"]) | BIT["hint"] | locate(group)
        allowed = BIT["claim_one_2048"] | BIT["claim_one_max"] | LOCATE
    else:
        required = BIT["claim_single_side"] | BIT["hints_ride"] | locate(group)
        allowed = LOCATE
    masks = []
    for run in ("captured", "replayed", "graph=0"):
        if run == "graph=0":
            e.set_option("graph", 0)
        e.set_samples(xy)
        assert cases.grow(e, case, K=K) == 0
        label = "single %s K %d, %s, %s" % (stream, K, form, run)
        beside(e)
        masks.append(check_mask(label, e, required, allowed))
        report_ties(label, [e])
        assert_same(e, o)
    assert masks[0] == masks[1] == masks[2]
    assert e.get_option("group_lanes") == (16 if form == "group_lanes=16" else 0)


# ---------------------------------------------------------------------------------------------------------------- sub-batches, rows of their own
@pytest.mark.parametrize("group_lanes", [-1, 16])
def test_sub_batches_with_a_side_chain_each(eng_mod, oracle, group_lanes):
    """batch_streams = 2 on nine rows: two launch sequences of four and five rows side by side, each with a kd chain of its own on a
    side stream of its own (group_lanes = -1: rows of fewer than eight take the one-wave-per-sample kernels)"""
    K, n = X.KDF_VARIANT_K, X.KDF_VARIANT_ITERS
    engs = [engine(eng_mod, "lattice", s, n, kd_lazy=0, group_lanes=group_lanes)[0] for s in X.KDF_VARIANT_SEEDS]
    engs[0].set_option("batch_streams", 2)
    grow_batch(eng_mod, engs, X.kd_forms_inputs("lattice", 0, n, n)[0], K)
    assert engs[0].get_option("launch_mode") in (2, -2)
    for lead in (engs[0], engs[4]):                               # the sub-batches' first contexts
        label = "sub-batch led by row %d, group_lanes %d" % (engs.index(lead), group_lanes)
        assert lead.get_option("group_lanes") == (16 if group_lanes == 16 else 0)
        beside(lead)
        check_mask(label, lead, claim_rows(2048) | BIT["locate_1"] | BIT["hint"] | BIT["tie_fix_beside"], CLAIM_ROWS | LOCATE)
    report_ties("sub-batches, group_lanes %d" % group_lanes, engs)
    for s, e in zip(X.KDF_VARIANT_SEEDS, engs):
        assert_same(e, oracle("lattice", s, K, n))


@pytest.mark.parametrize("compact_rows", [1, 0])
def test_rows_with_loop_conditions_of_their_own(eng_mod, oracle, compact_rows):
    """the row plans of exact_inputs.ROW_MIN / ROW_MAX at K = 128 with the whole structure beside the steps: rows end at different steps
    while the side chain goes on inserting every row's nodes"""
    K = X.KDF_ROWS_K
    engs = [engine(eng_mod, "lattice", s, X.ROW_MIN[s], X.ROW_MAX[s], kd_lazy=0, compact_rows=compact_rows)[0] for s in X.KDF_SEEDS]
    case = X.kd_forms_inputs("lattice", 0, X.ROW_MIN[0], X.ROW_MAX[0])[0]
    grow_batch(eng_mod, engs, case, K, n_min=X.ROW_MIN, n_max=X.ROW_MAX)
    label = "rows of their own, compact_rows %d" % compact_rows
    assert engs[0].get_option("group_lanes") == 16
    beside(engs[0])
    check_mask(label, engs[0], claim_rows(8 * K) | BIT["locate_1"] | BIT["hint"] | BIT["tie_fix_beside"], CLAIM_ROWS | LOCATE)
    report_ties(label, engs)
    its = [e.num_iterations() for e in engs]
    assert len(set(its)) > 1 and all(a <= i <= b for i, a, b in zip(its, X.ROW_MIN, X.ROW_MAX))
    for s, e in zip(X.KDF_SEEDS, engs):
        assert_same(e, oracle("lattice", s, K, X.ROW_MIN[s], X.ROW_MAX[s]))


# ---------------------------------------------------------------------------------------------------------------- state carried between forms
def test_forms_in_sequence_on_lattice_streams(eng_mod):
    """SEQUENCE of tests/test_gpu_launch_sequences.py on nine contexts fed lattice streams (set again before every grow): what one form
    leaves behind -- a kd group counter, hints still to ride, a pending event -- would show in the next form's tied parents.  Contexts
    0 and 4 against oracles grown as often with the same budgets."""
    n, K = X.KDF_SEQ_ITERS, X.KDF_SEQ_K
    inputs = [X.kd_forms_inputs("lattice", s, n, n) for s in range(9)]
    case = inputs[0][0]
    engs = [cases.configure(eng_mod.Engine(), c) for c, _ in inputs]
    orcs = {j: cases.configure(orc.Oracle(), inputs[j][0]) for j in X.KDF_SEQ_CHECKED}
    for step, (batch, opts, budget, shown) in enumerate(SEQUENCE):
        assert budget[1] == n
        for e in engs:
            for k, v in dict(DEFAULTS, **opts).items():
                e.set_option(k, v)
        grown = range(9) if batch else (0,)
        for j in grown:
            engs[j].set_samples(inputs[j][1])
        if batch:
            grow_batch(eng_mod, engs, case, K, n_min=budget[0], n_max=budget[1])
        else:
            assert cases.grow(engs[0], case, K=K) == 0
        for j in X.KDF_SEQ_CHECKED:
            if j in grown:
                orcs[j].set_samples(inputs[j][1])
                cases.grow(orcs[j], cases.Case(case, n_iter_min=budget[0], n_iter_max=budget[1]), K=K, algo=orc.ALGO_BATCHED_KD)
        label = "sequence step %d (%s %s)" % (step, "batch" if batch else "single", opts)
        check_mask(label, engs[0], 0, ALL)
        report_ties(label, [engs[j] for j in X.KDF_SEQ_CHECKED])
        for j in X.KDF_SEQ_CHECKED:
            assert engs[j].num_iterations() == orcs[j].num_iterations(), "step %d, context %d" % (step, j)
            assert_same(engs[j], orcs[j])
        for name, want in shown.items():
            assert engs[0].get_option(name) == want, "step %d: %s" % (step, name)


# ---------------------------------------------------------------------------------------------------------------- nn_wg_waves = 1
def test_nn_wg_waves_accepts_one_and_four(eng_mod):
    e = eng_mod.Engine()
    assert e.get_option("nn_wg_waves") == 4
    for bad in (0, 2, 3, 8):
        with pytest.raises(Exception):
            e.set_option("nn_wg_waves", bad)
    e.set_option("nn_wg_waves", 1)
    assert e.get_option("nn_wg_waves") == 1


@pytest.mark.parametrize("commit_flat", [0, 1])
@pytest.mark.parametrize("group_lanes", [16, 32, 64])
def test_nn_wg_waves_one_lattice_batch_of_eight(eng_mod, oracle, group_lanes, commit_flat):
    """k_nn2<GL, 1>: the search and the rewire commit in 64-thread workgroups (commit_flat = 1: commit_flat_span<64>)"""
    K, n = X.KDF_VARIANT_K, X.KDF_VARIANT_ITERS
    engs = [engine(eng_mod, "lattice", s, n, nn_wg_waves=1, group_lanes=group_lanes, commit_flat=commit_flat)[0] for s in X.KDF_SEEDS]
    grow_batch(eng_mod, engs, X.kd_forms_inputs("lattice", 0, n, n)[0], K)
    lead = engs[0]
    assert lead.get_option("nn_wg_waves") == 1 and lead.get_option("group_lanes") == group_lanes and lead.get_option("commit_flat") == commit_flat
    assert lead.get_option("kd_lazy") == 1 and lead.get_option("kd_built_after") == 1
    label = "nn_wg_waves 1, group_lanes %d, commit_flat %d" % (group_lanes, commit_flat)
    check_mask(label, lead, BIT["built_after"], ALL)
    report_ties(label, engs)
    for s, e in zip(X.KDF_SEEDS, engs):
        assert_same(e, oracle("lattice", s, K, n))


def test_nn_wg_waves_one_duplicates_batch_of_eight(eng_mod, oracle):
    K, n = X.KDF_DUP_K, X.KDF_DUP_ITERS
    engs = [engine(eng_mod, "duplicates", s, n, nn_wg_waves=1)[0] for s in X.KDF_SEEDS]
    grow_batch(eng_mod, engs, X.kd_forms_inputs("duplicates", 0, n, n)[0], K)
    lead = engs[0]
    assert lead.get_option("nn_wg_waves") == 1 and lead.get_option("group_lanes") == 16
    assert lead.get_option("kd_lazy") == 1 and lead.get_option("kd_built_after") == 1
    check_mask("nn_wg_waves 1, duplicates", lead, BIT["built_after"], ALL)
    report_ties("nn_wg_waves 1, duplicates", engs)
    for s, e in zip(X.KDF_SEEDS, engs):
        assert_same(e, oracle("duplicates", s, K, n))


# ---------------------------------------------------------------------------------------------------------------- the last test of the file
def test_every_form_ran():
    """the union of kd_forms_run over the module is every bit: the matrix above still reaches each instantiation and each launch form
    (it needs the whole module to have run)"""
    union = 0
    for masks in SEEN.values():
        for m in masks:
            union |= m
    print("kd_forms_run over the module: %s" % names(union))
    assert union == ALL, "never launched: %s" % names(ALL & ~union)
