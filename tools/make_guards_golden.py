#!/usr/bin/env python3
"""Writes tests/golden/sim3p_guards.npz: the batches of the packed sim3 tick in which a lane that a plan dimension switches off (s >= n', s >= nl,
s >= p_keep) is inactive in ways the older fixtures do not hold together, with the outputs of the library it is run against.
tests/test_gpu_sim3p_guards.py expects those bits back from every later build — from the kernel's FIXD form and from the form that reads the
dimensions from the plan — with the wave order off and over three ticks with wave_order 2. The committed file was made with the library built from
the commit BEFORE the FIXD form existed, on an MI355X:

    make -C mech5845m-wbc-for-legged-manipulator_amd/csrc SUF=_parent        # in a checkout of that commit; copy the library over
    WBC_HIP_LIB=.../libwbc_hip_parent.so python tools/make_guards_golden.py [output.npz]

The cases (C3 unless said otherwise; tests/common.py's configurations and stress recipe):
  b5      B = 5: one full wave and a wave with one valid row and three rows that shadow instance B - 1 — the five instances of a B = 67 batch
          (seed 12) that ran the most dual iterations;
  mixed   B = 67 of a1_wx200 and a1_px100 alternating through model_id: n' = 11 and n' = 10 in the same wave;
  single  B = 67 of a1_wx200 alone (seed 14);
  nan     the single batch with a NaN in instance 13's q row: it reports WBC_QP_NUMERICAL and zeros, everyone else what they report without it
          (asserted here);
  warm    the single batch seeded with its own cold run's working sets (the WARM variant; `working_set` is recorded too);
  trunk   B = 67 of c3_trunk_task with moving orientation references (the TRUNK variant);
  tp      B = 67 through wbc_tick_tp with per-instance weights and gains (the TP variant);
  qcon    B = 67 of c3_mani (the QCON variant: it has no FIXD form).
Each case is run once with the wave order off — that result is recorded — and three times on one handle with wave_order 2, which must give the same
bits on the recording build too. Inputs are stored with the outputs (they come from the CPU oracle's FK, whose last bit may depend on the host's
libm). Uses no option or statistic that the recording build does not have."""
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

B, DT = 67, 0.002
OUT = ("qdot", "status", "iters", "q_next")
NAN_AT = (13, 10)      # instance 13 = row 1 of wave 3; q[10]: a leg angle
S = wbc_model.TASK_PARAMS_SLICES


def random_rows(cfg, n, seed):
    """the configuration's row with weights x log-uniform [0.1, 10], gains and joint_w x log-uniform [0.25, 4] (tests/test_gpu_task_params.py)"""
    rng = np.random.default_rng(seed)
    out = np.repeat(wbc_model.task_params(cfg, 1), n, axis=0).copy()
    for fields, (lo, hi) in ((("ee_W", "ee_w", "trunk_W", "trunk_w", "com_W"), (0.1, 10.0)), (("ee_gain", "trunk_gain", "com_gain", "joint_w"), (0.25, 4.0))):
        for f in fields:
            out[:, S[f]] *= np.exp(rng.uniform(np.log(lo), np.log(hi), (n, S[f].stop - S[f].start)))
    return out


def run(models, cfgs, d, **kw):
    """-> outputs with the wave order off; the same bits over three ticks with wave_order 2 are asserted, and the packed sim3 kernel"""
    keys = OUT + (("working_set",) if kw.get("want_working_set") else ())
    res = []
    for wave_order, ticks in ((0, 1), (2, 3)):
        bt = WbcBatch(models, len(d["q"]))
        for i, c in enumerate(cfgs):
            bt.configure(c, i)
        bt.set_option("wave_order", wave_order)
        for _ in range(ticks):
            got = bt.tick(d, DT, want_q_next=True, **kw)
            assert bt.stat("last_path") == 2, "not the packed sim3 kernel"
            res.append({k: np.asarray(got[k]).copy() for k in keys})
        bt.close()
    for got in res[1:]:
        for k in keys:
            assert np.array_equal(got[k].view(np.uint8), res[0][k].view(np.uint8)), k
    return res[0]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sim3p_guards.npz")
    wx, px = wbc_model.load_model("a1_wx200"), wbc_model.load_model("a1_px100_pin_ver")
    z = {}

    def record(case, models, cfgs, d, store_inputs=True, **kw):
        got = run(models, cfgs, d, **kw)
        if store_inputs:
            for k, v in d.items():
                z["%s_in_%s" % (case, k)] = np.asarray(v)
        for k, v in got.items():
            z["%s_out_%s" % (case, k)] = v
        st, it = got["status"], got["iters"]
        print("%s: B = %d, %d optimal, iters %d..%d" % (case, len(st), int((st == 0).sum()), it.min(), it.max()))
        return got

    cfg = common.config("c3", wx)
    # b5: the five heaviest instances of a stress batch
    d12 = common.tick_inputs(wx, cfg, B, seed=12)
    full = run([wx], [cfg], d12)
    top = np.sort(np.argsort(-full["iters"], kind="stable")[:5])
    got = record("b5", [wx], [cfg], {k: np.ascontiguousarray(np.asarray(v)[top]) for k, v in d12.items()})
    print("b5: instances %s of the B = 67 batch; same bits as in that batch: %s" % (
        top.tolist(), all(np.array_equal(got[k].view(np.uint8), full[k][top].view(np.uint8)) for k in OUT)))
    # mixed: the two models alternate, so every wave holds n' = 11 and n' = 10
    cfgs = [cfg, common.config("c3", px)]
    mid = (np.arange(B) % 2).astype(np.int32)
    parts = [common.tick_inputs(m, c, B, seed=41 + i) for i, (m, c) in enumerate(zip((wx, px), cfgs))]
    dm = {}
    for k in parts[0]:
        v = parts[0][k].copy()
        v[mid == 1] = parts[1][k][mid == 1]
        dm[k] = v
    dm["model_id"] = mid
    record("mixed", [wx, px], cfgs, dm)
    # single, nan, warm: one batch
    d14 = common.tick_inputs(wx, cfg, B, seed=14)
    clean = record("single", [wx], [cfg], d14)
    dn = dict(d14, q=np.array(d14["q"], copy=True))
    dn["q"][NAN_AT] = np.nan
    got = record("nan", [wx], [cfg], dn)
    b = NAN_AT[0]
    assert got["status"][b] == capi.QP_NUMERICAL and (got["qdot"][b] == 0.0).all(), "the NaN row does not report WBC_QP_NUMERICAL with zero qdot"
    mates = [i for i in range(b & ~3, (b & ~3) + 4) if i != b]
    assert (got["status"][mates] == 0).all(), "a wave-mate of the NaN row is not optimal: choose another row"
    others = np.arange(B) != b
    for k in OUT:
        assert np.array_equal(got[k][others].view(np.uint8), clean[k][others].view(np.uint8)), "the NaN row changed another instance's %s" % k
    ws = run([wx], [cfg], d14, want_working_set=True)["working_set"]
    z["warm_in_working_set"] = ws
    record("warm", [wx], [cfg], dict(d14, working_set=ws), store_inputs=False, want_working_set=True)
    # trunk, tp, qcon
    ct = common.config("c3_trunk_task", wx)
    record("trunk", [wx], [ct], common.tick_inputs(wx, ct, B, seed=27, stress=False, with_rot=True))
    rows = random_rows(cfg, B, seed=8)
    z["tp_in_task_params"] = rows
    record("tp", [wx], [cfg], common.tick_inputs(wx, cfg, B, seed=35), task_params=rows)
    cq = common.config("c3_mani", wx)
    record("qcon", [wx], [cq], common.tick_inputs(wx, cq, B, seed=29, stress=False))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **z)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
