#!/usr/bin/env python3
"""Writes tests/golden/sim3p_entry.npz: the outputs of the batches of tests/sim3p_entry_cases.py from the library it is run against.
tests/test_gpu_sim3p_entry.py expects those bits back from every later build (the packed sim3 kernel's entry issues its loads in
another order; operands and operations are what they were). The committed file was made on an MI355X with the library built from the commit BEFORE
that change:

    make -C mech5845m-wbc-for-legged-manipulator_amd/csrc SUF=_parent        # in a checkout of that commit; copy the library over
    WBC_HIP_LIB=.../libwbc_hip_parent.so python tools/make_entry_golden.py [output.npz]

Stored: the orientation references of the small batch (the other inputs are tests/golden/sim3p_guards.npz's), and per case either every tick's
outputs (`<case>_t<tick>_<output>`), the statistic wave_order_slices (`<case>_slices`) and last_tick_fixd, or `<case>_refused` = 1 where the
library's argument check turns the call down (an optional input the configuration needs). Uses no option or statistic that the recording build does not
have."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mech5845m-wbc-for-legged-manipulator_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import common  # noqa: E402
import sim3p_entry_cases as ec  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sim3p_entry.npz")
    zg = np.load(os.path.join(ROOT, "tests", "golden", "sim3p_guards.npz"))
    rot = common.add_rot_references({"trunk_ref_euler": np.zeros((5, 3))}, 5, seed=61)
    small_rot = {k: np.ascontiguousarray(rot[k]) for k in ("ee_ref_rot", "ee_prev_rot")}
    z = {"small_in_" + k: v for k, v in small_rot.items()}
    for name, case in ec.cases(zg, small_rot).items():
        r = ec.run(case)
        if r[0] == "refused":
            z[name + "_refused"] = np.int32(1)
            print("%s: refused (%s)" % (name, r[1]))
            continue
        _, res, stats = r
        for t, got in enumerate(res, 1):
            for k in ec.keys_of(case):
                z["%s_t%d_%s" % (name, t, k)] = np.asarray(got[k]).copy()
        z[name + "_slices"] = np.array([s["wave_order_slices"] for s in stats], np.int64)
        z[name + "_fixd"] = np.array([s.get("last_tick_fixd", -1) for s in stats], np.int64)
        assert all(s["last_path"] == 2 for s in stats) or case["kind"] == "rollout", "%s: not the packed sim3 kernel" % name
        if case["fixd"] is not None:
            assert all(s["last_tick_fixd"] == case["fixd"] for s in stats), "%s: last_tick_fixd %s" % (name, stats)
        st, it = np.asarray(res[-1]["status"]), np.asarray(res[-1]["iters"])
        print("%s: B = %d, %d tick(s), %d optimal, iters %d..%d, slices %s" % (name, len(st), len(res), int((st == 0).sum()), it.min(), it.max(),
                                                                          z[name + "_slices"].tolist()))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **z)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
