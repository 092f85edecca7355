#!/usr/bin/env python3
"""Writes tests/golden/sim3p_issue_order.npz: two B = 64 batches of the packed sim3 tick (the benchmark's switch set, cold; and sim3.py's own
"HYBRID" posture mode, whose post_static block perturbs the state the bounds see) with the outputs of the library it is run against.
tests/test_gpu_sim3p_issue_order.py expects those bits back from every later build. The committed file was made with the library built from
the commit BEFORE the issue-order change, on an MI355X:

    make -C mech5845m-wbc-for-legged-manipulator_amd/csrc SUF=_parent        # in a checkout of that commit; copy the library over
    WBC_HIP_LIB=.../libwbc_hip_parent.so python tools/make_issue_order_golden.py [output.npz]

Inputs are stored with the outputs (they come from the CPU oracle's FK, whose last bit may depend on the host's libm)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mech5845m-wbc-for-legged-manipulator_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import common  # noqa: E402
import wbc_model  # noqa: E402
from wbc_batch import WbcBatch  # noqa: E402

B, DT = 64, 0.002


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sim3p_issue_order.npz")
    model = wbc_model.load_model("a1_wx200")
    z = {}
    for case, cfg_name, seed in (("cold", "c3", 6), ("static_hybrid", "c3_hybrid", 23)):
        cfg = common.config(cfg_name, model)
        d = common.tick_inputs(model, cfg, B, seed=seed, stress=True)
        bt = WbcBatch(model, B)
        bt.configure(cfg)
        got = bt.tick(d, DT, want_q_next=True)
        assert bt.stat("last_path") == 2, "not the packed sim3 kernel"
        bt.close()
        for k, v in d.items():
            z["%s_in_%s" % (case, k)] = np.asarray(v)
        for k in ("qdot", "status", "iters", "q_next"):
            z["%s_out_%s" % (case, k)] = np.asarray(got[k])
        print("%s: %d of %d optimal, iters %d..%d" % (case, int((z[case + "_out_status"] == 0).sum()), B, z[case + "_out_iters"].min(), z[case + "_out_iters"].max()))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **z)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
