#!/usr/bin/env python3
"""Writes tests/golden/sim3p_row_bcast.npz: the batches of the packed sim3 tick that tests/golden/sim3p_hot_path.npz does not hold, with the outputs
of the library it is run against. tests/test_gpu_sim3p_row_bcast.py expects those bits back from every later build, with the wave order off and
over three ticks with wave_order 2. The committed file was made with the library built from the commit BEFORE the sweep took its columns by DPP
row broadcast, on an MI355X:

    make -C mech5845m-wbc-for-legged-manipulator_amd/csrc SUF=_parent        # in a checkout of that commit; copy the library over
    WBC_HIP_LIB=.../libwbc_hip_parent.so python tools/make_row_bcast_golden.py [output.npz]

The cases:
  laikago   B = 67 of the Laikago + ViperX-300 model, C3 (the kernel path it runs on is recorded and expected back);
  rot       B = 67 of a1_wx200 with the ViperX-300's rotated placements (tests/test_gpu_rotated_placement.py): the packed kernel's ROT variants;
  tp        B = 67 of a1_wx200 through wbc_tick_tp with per-instance weights and gains (the TP variants);
  b5        a stress-recipe C3 batch of B = 5: one full wave and a wave with one valid row and three rows that shadow instance B - 1 — the five
            instances of a B = 67 batch that ran the most dual iterations;
  nan       B = 67 with a NaN in one instance's q row: that instance reports WBC_QP_NUMERICAL with zero qdot, its three wave-mates and everyone
            else what they report without it (asserted here against the same batch without the NaN).
Each case is run once with the wave order off — that result is recorded — and three times on one handle with wave_order 2, which must give the same
bits on the recording build too. Inputs are stored with the outputs (they come from the CPU oracle's FK, whose last bit may depend on the host's
libm)."""
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mech5845m-wbc-for-legged-manipulator_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import common  # noqa: E402
import wbc_capi as capi  # noqa: E402
import wbc_model  # noqa: E402
from wbc_batch import WbcBatch  # noqa: E402

DT = 0.002
OUT = ("qdot", "status", "iters", "q_next")
NAN_AT = (13, 10)      # instance 13 = row 1 of wave 3; q[10]: a leg angle
S = wbc_model.TASK_PARAMS_SLICES


def rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
            [-sp, cp * sr, cp * cr]]


def rotated_wx200():
    """a1_wx200 with the ViperX-300's rotated placements (tests/test_gpu_rotated_placement.py)"""
    with open(os.path.join(wbc_model.MODELS_DIR, "a1_wx200.json")) as f:
        data = copy.deepcopy(json.load(f))
    for name, a in (("elbow", (3.14, 0, 0)), ("wrist_rotate", (-3.14, 0, 0)), ("left_finger", (0.3, -0.2, 0.1))):
        next(j for j in data["joints"] if j["name"] == name)["placement_R"] = rpy(*a)
    data["name"] = "a1_wx200_rotated"
    return wbc_model.Model(data, dict(wbc_model.A1_ROLES))


def random_rows(cfg, B, seed):
    """the configuration's row with weights x log-uniform [0.1, 10], gains and joint_w x log-uniform [0.25, 4] (tests/test_gpu_task_params.py)"""
    rng = np.random.default_rng(seed)
    out = np.repeat(wbc_model.task_params(cfg, 1), B, axis=0).copy()
    for fields, (lo, hi) in ((("ee_W", "ee_w", "trunk_W", "trunk_w", "com_W"), (0.1, 10.0)), (("ee_gain", "trunk_gain", "com_gain", "joint_w"), (0.25, 4.0))):
        for f in fields:
            out[:, S[f]] *= np.exp(rng.uniform(np.log(lo), np.log(hi), (B, S[f].stop - S[f].start)))
    return out


def run(model, cfg, d, rows):
    """-> (outputs with the wave order off, kernel path); the same bits over three ticks with wave_order 2 are asserted"""
    B = len(d["q"])
    kw = {"want_q_next": True}
    if rows is not None:
        kw["task_params"] = rows
    res = []
    for wave_order, ticks in ((0, 1), (2, 3)):
        bt = WbcBatch(model, B)
        bt.configure(cfg)
        bt.set_option("wave_order", wave_order)
        for _ in range(ticks):
            got = bt.tick(d, DT, **kw)
            res.append(({k: np.asarray(got[k]).copy() for k in OUT}, bt.stat("last_path")))
        bt.close()
    for got, path in res[1:]:
        assert path == res[0][1]
        for k in OUT:
            assert np.array_equal(got[k].view(np.uint8), res[0][0][k].view(np.uint8)), k
    return res[0]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sim3p_row_bcast.npz")
    wx200 = wbc_model.load_model("a1_wx200")
    z = {}

    def record(case, model, d, rows=None):
        cfg = common.config("c3", model)
        got, path = run(model, cfg, d, rows)
        for k, v in d.items():
            z["%s_in_%s" % (case, k)] = np.asarray(v)
        if rows is not None:
            z[case + "_in_task_params"] = rows
        for k in OUT:
            z["%s_out_%s" % (case, k)] = got[k]
        z[case + "_path"] = np.int32(path)
        st, it = got["status"], got["iters"]
        print("%s: B = %d, path %d, %d optimal, iters %d..%d" % (case, len(st), path, int((st == 0).sum()), it.min(), it.max()))
        return got, path

    lk = wbc_model.load_model("laikago_vx300")
    record("laikago", lk, common.tick_inputs(lk, common.config("c3", lk), 67, seed=23))
    rot = rotated_wx200()
    _, path = record("rot", rot, common.tick_inputs(rot, common.config("c3", rot), 67, seed=21))
    assert path == 2, "not the packed sim3 kernel"
    cfg = common.config("c3", wx200)
    _, path = record("tp", wx200, common.tick_inputs(wx200, cfg, 67, seed=31), random_rows(cfg, 67, seed=5))
    assert path == 2
    d67 = common.tick_inputs(wx200, cfg, 67, seed=6)
    clean, path = run(wx200, cfg, d67, None)
    assert path == 2
    top = np.sort(np.argsort(-clean["iters"], kind="stable")[:5])
    got, path = record("b5", wx200, {k: np.ascontiguousarray(np.asarray(v)[top]) for k, v in d67.items()})
    assert path == 2
    print("b5: instances %s of the B = 67 batch (iters %d..%d there); same bits as in that batch: %s" % (
        top.tolist(), clean["iters"].min(), clean["iters"].max(), all(np.array_equal(got[k].view(np.uint8), clean[k][top].view(np.uint8)) for k in OUT)))
    dn = dict(d67, q=np.array(d67["q"], copy=True))
    dn["q"][NAN_AT] = np.nan
    got, path = record("nan", wx200, dn)
    assert path == 2
    b = NAN_AT[0]
    assert got["status"][b] == capi.QP_NUMERICAL and (got["qdot"][b] == 0.0).all(), "the NaN row does not report WBC_QP_NUMERICAL with zero qdot"
    mates = [i for i in range(b & ~3, (b & ~3) + 4) if i != b]
    assert (got["status"][mates] == 0).all(), "a wave-mate of the NaN row is not optimal: choose another row"
    others = np.arange(67) != b
    for k in OUT:
        assert np.array_equal(got[k][others].view(np.uint8), clean[k][others].view(np.uint8)), "the NaN row changed another instance's %s" % k
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **z)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
