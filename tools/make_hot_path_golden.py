#!/usr/bin/env python3
"""Writes tests/golden/sim3p_hot_path.npz: four B = 67 batches of the packed sim3 tick (16 full waves and one wave with a single invalid row) —
cold C3 on a stress-recipe seed whose oracle answer shows drops, WARM seeded with that cold run's working sets, TRUNK (c3_trunk_task with
moving orientation references) and QCON (c3_mani) — with the outputs of the library it is run against. tests/test_gpu_sim3p_hot_path.py
expects those bits back from every later build, with the wave order off and on. The committed file was made with the library built from the
commit BEFORE the hot-path change, on an MI355X:

    make -C mech5845m-wbc-for-legged-manipulator_amd/csrc SUF=_parent        # in a checkout of that commit; copy the library over
    WBC_HIP_LIB=.../libwbc_hip_parent.so python tools/make_hot_path_golden.py [output.npz]

Each case is run once with the wave order off — that result is recorded — and three times on one handle with wave_order 2 (ticks 2 and 3 in the
order the tick before recorded), which must give the same bits on the recording build too. Inputs are stored with the outputs (they come from
the CPU oracle's FK, whose last bit may depend on the host's libm)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mech5845m-wbc-for-legged-manipulator_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import common  # noqa: E402
import oracle  # noqa: E402
import wbc_model  # noqa: E402
from wbc_batch import WbcBatch  # noqa: E402

B, DT = 67, 0.002
OUT = ("qdot", "status", "iters", "q_next")
# case -> (configuration of tests/common.py, seed, stress recipe, moving orientation references)
CASES = (("cold", "c3", 6, True, False), ("warm", "c3", 6, True, False), ("trunk", "c3_trunk_task", 23, False, True),
         ("qcon", "c3_mani", 23, False, False))


def drops(model, cfg, d, ref):
    """working-set changes of the oracle's answer beyond the equalities and the inequalities active at the optimum, halved: one drop and its add
    each (tests/test_gpu_sim3p_cold_paths.py)"""
    a = oracle.assemble([model], [cfg], d, DT, B)
    lo, hi = np.concatenate([a["lb"], a["Clb"]], axis=1), np.concatenate([a["ub"], a["Cub"]], axis=1)
    v = np.concatenate([ref["qdot"], np.einsum("bij,bj->bi", a["C"], ref["qdot"])], axis=1)
    ineq = lo != hi
    active = ineq & ((np.abs(v - lo) < 1e-7 * np.maximum(1, np.abs(lo))) | (np.abs(v - hi) < 1e-7 * np.maximum(1, np.abs(hi))))
    return (ref["iters"] - (~ineq).sum(axis=1) - active.sum(axis=1)) // 2


def handle(model, cfg, wave_order):
    bt = WbcBatch(model, B)
    bt.configure(cfg)
    bt.set_option("wave_order", wave_order)
    return bt


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sim3p_hot_path.npz")
    model = wbc_model.load_model("a1_wx200")
    z, ws = {}, None
    for case, cfg_name, seed, stress, with_rot in CASES:
        cfg = common.config(cfg_name, model)
        d = common.tick_inputs(model, cfg, B, seed=seed, stress=stress, with_rot=with_rot)
        if case == "cold":
            ref = oracle.tick([model], [cfg], d, DT, B, nthreads=8)
            nd = drops(model, cfg, d, ref)
            assert (nd[ref["status"] == 0] >= 1).sum() >= 1, "no instance of this seed drops a constraint: choose another"
            print("cold: %d instances with drops (oracle)" % int((nd >= 1).sum()))
        kw = {"want_q_next": True}
        if case == "warm":
            d = dict(d, working_set=ws)
            kw["want_working_set"] = True
        off = handle(model, cfg, 0)
        got = off.tick(d, DT, **kw)
        assert off.stat("last_path") == 2, "not the packed sim3 kernel"
        if case == "cold":     # the WARM case's seeds: the cold inputs' final working sets (asking for them runs the WARM variant unseeded)
            ws = np.asarray(off.tick(d, DT, want_working_set=True)["working_set"]).copy()
        off.close()
        on = handle(model, cfg, 2)
        for tick in (1, 2, 3):
            again = on.tick(d, DT, **kw)
            assert on.stat("wave_order_slices") == 1
            for k in OUT:
                assert np.array_equal(np.asarray(again[k]).view(np.uint8), np.asarray(got[k]).view(np.uint8)), (case, tick, k)
        on.close()
        if case != "warm":     # (the WARM case runs on the cold case's inputs plus its working sets)
            for k, v in d.items():
                z["%s_in_%s" % (case, k)] = np.asarray(v)
        else:
            z["warm_in_working_set"] = ws
        for k in OUT:
            z["%s_out_%s" % (case, k)] = np.asarray(got[k])
        st, it = z[case + "_out_status"], z[case + "_out_iters"]
        print("%s: %d of %d optimal, iters %d..%d" % (case, int((st == 0).sum()), B, it.min(), it.max()))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **z)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
