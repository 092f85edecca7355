#!/usr/bin/env python3
"""Writes tests/golden/rollout_recorded.npz: what every roll-out entry point (rollout, rollout_traj, rollout_tracks, rollout_watch) gave BEFORE
the host code that sequences them was reorganised, with the inputs of the calls and the statistics after each. The calls and
their order are tests/rollout_recorded_cases.py's; tests/test_gpu_rollout_recorded.py expects those bits back from every later build, from host
arrays and from device tensors. The committed file was made on an MI355X in a checkout of the commit before the change (library AND Python
wrapper of that commit), with this tool and tests/rollout_recorded_cases.py copied in:

    python __graft_entry__.py build && python tools/make_rollout_golden.py [output.npz]

    python tools/make_rollout_golden.py --b5 [file.npz]: adds the "b5__*" arrays of rollout_recorded_cases.run_b5 (wbc_state_slack with
    rotated placements, B = 5) to an existing file and leaves every other array as it is. The committed ones were made that way with the
    library of the commit before the whole-tree kernels' shared header.

Asserted while recording, so that the cases exercise what they claim to: the bad row is counted; an instance of the trajectory call passes a
milestone inside its ticks; a watched family goes negative or has its minimum after tick 0; the calls without a watch and the repeated plain
call give the bits of the calls they repeat; the file stays far below tests/golden/packed_qp_shared.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mech5845m-wbc-for-legged-manipulator_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

import rollout_recorded_cases as rc  # noqa: E402
import wbc_workload  # noqa: E402


def record_b5():
    inputs = rc.b5_inputs()
    o = rc.run_b5(inputs)
    assert np.isfinite(o["slack"]).all() and o["slack"].shape == (rc.B5, 4) and o["components"].shape == (rc.B5, 12), o
    assert all(rc.run_b5(inputs)[k].tobytes() == v.tobytes() for k, v in o.items()), "two runs differ"
    z = {"b5__in__" + k: v for k, v in inputs.items()}
    z.update({"b5__out__" + k: v for k, v in o.items()})
    return z


def main():
    args = [a for a in sys.argv[1:] if a != "--b5"]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "rollout_recorded.npz")
    if "--b5" in sys.argv[1:]:
        old = np.load(out)
        z = {k: old[k] for k in old.files if not k.startswith("b5__")}
        z.update(record_b5())
        np.savez_compressed(out, **z)
        print("added %s to %s" % (sorted(k for k in z if k.startswith("b5__")), out))
        return
    inputs = rc.make_inputs()
    z = {"in__" + k: v for k, v in inputs.items()}
    # the trajectory call's milestone: the segment of tick K_TRAJ - 1 is not the first one
    n, du = inputs["traj_n"], inputs["traj_du"]
    passed = (np.floor((rc.K_TRAJ - 1) * du) >= 1) & (n >= 3)
    assert passed.any(), "no instance passes a milestone within %d ticks" % rc.K_TRAJ
    last = wbc_workload.traj_targets(inputs["traj_points"], n, du, rc.K_TRAJ - 1)
    assert np.isfinite(last[np.arange(rc.B) != rc.BAD]).all()
    bt = rc.handle()
    got = {}
    for case, o, stats in rc.run_cases(bt, inputs):
        got[case] = o
        print("%-18s stats %s  status %s  keys %s" % (case, stats.tolist(), o["status"].tolist(), " ".join(sorted(o))))
        z["stats__" + case] = stats
        want = rc.CASES[case]
        if want != case:          # a repeat: the bits of the case it repeats, nothing of its own in the file
            assert set(o) == set(got[want]), (case, sorted(o), sorted(got[want]))
            for k in o:
                assert o[k].tobytes() == got[want][k].tobytes(), (case, k)
            continue
        for k, v in o.items():
            z["out__%s__%s" % (case, k)] = v
        if case.startswith(("traj", "tracks", "watch_tracks")):
            assert stats[0] == 1, "%s: the bad row is not counted (last_traj_bad_rows = %d)" % (case, stats[0])
            assert o["bad_ticks"][rc.BAD] == rc.K_TRAJ and o["first_bad_tick"][rc.BAD] == 0, (o["bad_ticks"], o["first_bad_tick"])
        if case.startswith("watch"):
            moved = (o["neg_ticks"] > 0).any() or (o["slack_min_tick"] > 0).any()
            assert moved, "%s: no watched family goes negative or has its minimum after tick 0" % case
            print("%-18s neg_ticks\n%s\nslack_min_tick\n%s" % (case, o["neg_ticks"], o["slack_min_tick"]))
    bt.close()
    z.update(record_b5())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **z)
    size = os.path.getsize(out)
    assert 4 * size < os.path.getsize(os.path.join(ROOT, "tests", "golden", "packed_qp_shared.npz")), size
    print("wrote %s (%d bytes)" % (out, size))


if __name__ == "__main__":
    main()
