"""The packed sim3 kernel's FIXD form takes the plan's dimensions (nv, nq, n', nelim, p_keep) as compile-time constants where the handle holds one
model whose plan has the a1_wx200 sim3 dimensions and the call passes no model_id array; the lane guards that compare with them
fold. The operands, the operations and their order are what they were, so every result is bit for bit what it was. The batches here are those in
which a guarded lane is inactive in ways the older fixtures do not hold together; their expected outputs were recorded from the build before the
change (tests/golden/sim3p_guards.npz, made by tools/make_guards_golden.py):
  * b5: a stress-recipe batch of B = 5 — one full wave, and a wave with one valid row and three rows that shadow instance B - 1;
  * mixed: B = 67 of a1_wx200 and a1_px100 through model_id — n' = 11 and 10 in the same wave; the form that reads the plan must have run;
  * single: B = 67 of a1_wx200 — the FIXD form must have run; the same batch with option "sim3p_fixd" 0 runs the other form: the two are compared
    with each other as well as with the recording;
  * nan: B = 67 with a NaN in the q row of instance 13: it reports WBC_QP_NUMERICAL and zeros, its three wave-mates the recorded bits;
  * warm (seeded with the cold run's working sets; `working_set` is compared too), trunk, tp, qcon: B = 67 each of the kernel's other variants.
Each with the wave order off and over three ticks on one handle with wave_order 2, on both forms where the row has both."""
import os

import numpy as np
import pytest

import common
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3p_guards.npz")
OUT = ("qdot", "status", "iters", "q_next")
NAN_ROW = 13
# case -> (batch size, configuration of tests/common.py, the case whose inputs it runs on, has a FIXD form)
CASES = {"b5": (5, "c3", "b5", True), "mixed": (67, "c3", "mixed", False), "single": (67, "c3", "single", True), "nan": (67, "c3", "nan", True),
         "warm": (67, "c3", "single", True), "trunk": (67, "c3_trunk_task", "trunk", True), "tp": (67, "c3", "tp", True),
         "qcon": (67, "c3_mani", "qcon", False)}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _bits_equal(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs in %d instances" % (
            what, k, int((x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1).sum()))


@pytest.mark.parametrize("case", list(CASES))
def test_bit_identical_to_the_build_before(golden, case):
    z = golden
    B, cfg_name, src, has_fixd = CASES[case]
    pre = src + "_in_"
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    kw = {"want_q_next": True}
    keys = OUT
    if case == "tp":
        kw["task_params"] = np.ascontiguousarray(d.pop("task_params"))
    if case == "warm":
        d["working_set"] = z["warm_in_working_set"]
        kw["want_working_set"] = True
        keys = OUT + ("working_set",)
    want = {k: z["%s_out_%s" % (case, k)] for k in keys}
    assert len(d["q"]) == B
    if case == "nan":                                   # what the recording says about the NaN row, before it is compared
        assert np.isnan(d["q"][NAN_ROW]).sum() == 1 and np.isnan(d["q"]).sum() == 1
        assert want["status"][NAN_ROW] == capi.QP_NUMERICAL and (want["qdot"][NAN_ROW] == 0.0).all()
        mates = [b for b in range(NAN_ROW & ~3, (NAN_ROW & ~3) + 4) if b != NAN_ROW]
        assert (want["status"][mates] == 0).all() and (want["qdot"][mates] != 0.0).any(axis=1).all()
    models = [wbc_model.load_model("a1_wx200")]
    if case == "mixed":
        models.append(wbc_model.load_model("a1_px100_pin_ver"))
        assert set(np.unique(d["model_id"][:4])) == {0, 1}                      # (both models in the first wave already)
    cfgs = [common.config(cfg_name, m) for m in models]
    first = None
    for fixd in ((1, 0) if has_fixd else (1,)):         # option "sim3p_fixd": 1 is the default
        for wave_order, ticks in ((0, 1), (2, 3)):
            bt = WbcBatch(models, B)
            for i, c in enumerate(cfgs):
                bt.configure(c, i)
            bt.set_option("wave_order", wave_order)
            bt.set_option("sim3p_fixd", fixd)
            for tick in range(1, ticks + 1):
                got = bt.tick(d, DT, **kw)
                what = "%s, sim3p_fixd %d, wave_order %d, tick %d" % (case, fixd, wave_order, tick)
                assert bt.stat("last_path") == 2, what                         # the packed sim3 kernel
                assert bt.stat("last_tick_fixd") == (1 if has_fixd and fixd else 0), what
                _bits_equal(got, want, keys, what)
                if first is None:
                    first = {k: np.asarray(got[k]).copy() for k in keys}
                _bits_equal(got, first, keys, what + " against the first run")
            bt.close()
