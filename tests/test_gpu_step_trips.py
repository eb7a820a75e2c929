"""GPU parity of the step kernels' set-up loads (PORRT_STEP_TRIPS in porrt_device.hpp: the run constants' hot block and RC_HOLD, the class
byte beside the finest cells in k_nn2, the valid-mask words and the clearance byte beside the first region counts in the connect pass,
the prefix wave's counts in the flat commit): the cases at which loads that are asked for early, unconditionally in form, or from words
held by the lanes can go wrong.  The inputs are tests/step_trips_inputs.py; what each has to produce is asserted from the oracle alone in
tests/test_step_trips_inputs_cpu.py.

  words          K = 64 / 1024 / 2048: one word of the step's valid mask, one per lane of a 16-lane group, two per lane (32- and 64-lane
                 groups hold one); 8 rows take the dealing of rows to XCDs, 3 do not; K = 64 runs ten steps
  border         samples in pixel row 0, row H - 1, column 0 and column W - 1 of a raster with CLS_HIGH0 pixels; the first ten steps
                 of a run, where level 1 of the pyramid and the nearest-node search decide
  outside        a sample whose pixel does not exist: the error the oracle reports
  no_raster      rows without a raster
  short / long   max_step 0.02 (most samples steered, the steered state's class fetched again) and 0.5 (the young-tree streaming lasts)
  own_plans      rows with step plans of their own, one of which ends early
  goal_reached   slots with bq_k = 0xFFFF and the clone workgroup

Every batch runs under group_lanes 16 / 32 / 64, conn_wg_waves 1 / 4, nn_wg_waves 1 / 4 and commit_flat 0 / 1, and every tree must
equal the oracle's bit for bit.
"""
import itertools

import pytest

import step_trips_inputs as sti
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

FORMS = [dict(group_lanes=g, conn_wg_waves=c, nn_wg_waves=n, commit_flat=f) for g, c, n, f in itertools.product((16, 32, 64), (1, 4), (1, 4), (0, 1))]


def _form_id(f):
    return "g%d-c%d-n%d-f%d" % (f["group_lanes"], f["conn_wg_waves"], f["nn_wg_waves"], f["commit_flat"])


@pytest.fixture(scope="module")
def eng_mod():
    from po_rrt_amd import build
    build.build()
    import po_rrt_amd
    return po_rrt_amd


def _engines(eng_mod, bt, form):
    engs = []
    for c, s in zip(bt.cases, bt.samples):
        e = sti.configure(eng_mod.Engine(), c, s)
        for k, v in form.items():
            e.set_option(k, v)
        engs.append(e)
    return engs


def _grow(eng_mod, bt, form):
    engs = _engines(eng_mod, bt, form)
    eng_mod.Engine.grow_batch(engs, [c.start for c in bt.cases], bt.max_step, bt.search_radius, bt.n_iter, bt.K, n_iter_max=bt.n_iter_max)
    for k, v in form.items():
        assert engs[0].get_option(k) == v, "the run did not take %s = %d" % (k, v)
    return engs


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("name", sorted(sti.BATCHES))
def test_batch(eng_mod, name, form):
    bt, orcs = sti.oracles(name)
    for e, o in zip(_grow(eng_mod, bt, form), orcs):
        assert_same(e, o)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_sample_outside_the_raster(eng_mod, form):
    """the row whose unsteered sample has no pixel: the oracle reports the reference's panic, and so does the batch"""
    from po_rrt_amd import PorrtError
    bt = sti.outside()
    with pytest.raises(RuntimeError, match="raster"):
        sti.oracle_row(bt, 1)
    engs = _engines(eng_mod, bt, form)
    with pytest.raises(PorrtError, match="raster"):
        eng_mod.Engine.grow_batch(engs, [c.start for c in bt.cases], bt.max_step, bt.search_radius, bt.n_iter, bt.K)
