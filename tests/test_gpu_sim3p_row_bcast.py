"""The packed sim3 kernel's Cholesky sweep takes its columns by DPP row broadcast (one v_mov_b64_dpp row_newbcast per entry) instead of through LDS
(DESIGN.md §3.26). The operands, the operations and their order are what they were, so every result is bit for bit what it was. The batches here
are the ones tests/golden/sim3p_hot_path.npz does not hold; their expected outputs were recorded from the build before the change
(tests/golden/sim3p_row_bcast.npz, made by tools/make_row_bcast_golden.py):
  * laikago: B = 67 of the Laikago + ViperX-300 model (on the kernel path the recording build took);
  * rot: B = 67 of a1_wx200 with the ViperX-300's rotated placements (the ROT variants of the packed kernel);
  * tp: B = 67 through wbc_tick_tp with per-instance weights and gains (the TP variants);
  * b5: a stress-recipe batch of B = 5 — one full wave, and a wave with one valid row and three rows that shadow instance B - 1: the smallest
    shape at which a broadcast that reads a wrong or an inactive row shows;
  * nan: B = 67 with a NaN in the q row of instance 13: it reports WBC_QP_NUMERICAL and zeros, its three wave-mates the recorded bits — a
    broadcast must not carry one row's values into another.
Each with the wave order off and over three ticks on one handle with wave_order 2."""
import copy
import json
import os

import numpy as np
import pytest

import common
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3p_row_bcast.npz")
OUT = ("qdot", "status", "iters", "q_next")
NAN_ROW = 13


def _rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
            [-sp, cp * sr, cp * cr]]


def _rotated_wx200():
    """the rotated-placement a1_wx200 of test_gpu_rotated_placement.py"""
    with open(os.path.join(wbc_model.MODELS_DIR, "a1_wx200.json")) as f:
        data = copy.deepcopy(json.load(f))
    for name, rpy in (("elbow", (3.14, 0, 0)), ("wrist_rotate", (-3.14, 0, 0)), ("left_finger", (0.3, -0.2, 0.1))):
        next(j for j in data["joints"] if j["name"] == name)["placement_R"] = _rpy(*rpy)
    data["name"] = "a1_wx200_rotated"
    return wbc_model.Model(data, dict(wbc_model.A1_ROLES))


MODEL = {"laikago": lambda: wbc_model.load_model("laikago_vx300"), "rot": _rotated_wx200}
SIZE = {"laikago": 67, "rot": 67, "tp": 67, "b5": 5, "nan": 67}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _bits_equal(a, b, what):
    for k in OUT:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs in %d instances" % (
            what, k, int((x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1).sum()))


@pytest.mark.parametrize("case", list(SIZE))
def test_bit_identical_to_the_build_before(golden, case):
    z = golden
    pre = case + "_in_"
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    kw = {"want_q_next": True}
    if case == "tp":
        kw["task_params"] = np.ascontiguousarray(d.pop("task_params"))
    else:
        assert "task_params" not in d
    want = {k: z["%s_out_%s" % (case, k)] for k in OUT}
    path = int(z[case + "_path"])
    B = len(d["q"])
    assert B == SIZE[case]
    if case != "laikago":
        assert path == 2                                # the packed sim3 kernel
    if case == "nan":                                   # what the recording says about the NaN row, before it is compared
        assert np.isnan(d["q"][NAN_ROW]).sum() == 1 and np.isnan(d["q"]).sum() == 1
        assert want["status"][NAN_ROW] == capi.QP_NUMERICAL and (want["qdot"][NAN_ROW] == 0.0).all()
        mates = [b for b in range(NAN_ROW & ~3, (NAN_ROW & ~3) + 4) if b != NAN_ROW]
        assert (want["status"][mates] == 0).all() and (want["qdot"][mates] != 0.0).any(axis=1).all()
    model = MODEL.get(case, lambda: wbc_model.load_model("a1_wx200"))()
    cfg = common.config("c3", model)
    for wave_order, ticks in ((0, 1), (2, 3)):
        bt = WbcBatch(model, B)
        bt.configure(cfg)
        bt.set_option("wave_order", wave_order)
        for tick in range(1, ticks + 1):
            got = bt.tick(d, DT, **kw)
            assert bt.stat("last_path") == path
            _bits_equal(got, want, "%s, wave_order %d, tick %d" % (case, wave_order, tick))
        bt.close()
