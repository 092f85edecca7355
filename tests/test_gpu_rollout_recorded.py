"""The roll-out entry points give, bit for bit, what they gave before their host code was reorganised into one pipeline with typed workspaces
(DESIGN.md §3.35): tests/golden/rollout_recorded.npz, recorded by tools/make_rollout_golden.py from the library and the wrapper of the commit
before. The calls and their order are rollout_recorded_cases.py's — a1_wx200 under c3, max_batch = 12 and B = 9, twelve calls on one handle:
the plain call (a step, hold ticks, a trace), with warm starts, with per-instance task rows; the trajectory call with and without a trace (a
milestone passed, a NaN row, groups of three); three tracks with three scored frames, then two tracks and a constant trunk step; the watch
over the tracks call and over the plain call; both again with an empty watch, and the plain call once more — the last three must give the
bits recorded for the calls they repeat. Every output's key set, dtype, shape and bits are held, and the statistics last_traj_bad_rows,
last_path and last_update_packed after every call; once from numpy arrays (the library stages them) and once from torch device tensors (the
pointers pass through), each on a handle of its own."""
import os

import numpy as np
import pytest
import torch

import rollout_recorded_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_recorded.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def test_the_record_holds_what_the_cases_claim(golden):
    z = golden
    assert z["in__d_q"].shape == (rc.B, 27) and rc.B < rc.MAX_BATCH
    assert np.isnan(z["in__traj_points"][rc.BAD]).any() and np.isnan(z["in__grip_points"][rc.BAD]).any()
    assert ((np.floor((rc.K_TRAJ - 1) * z["in__traj_du"]) >= 1) & (z["in__traj_n"] >= 3)).any()           # a milestone is passed
    for case in ("traj_trace", "traj", "tracks", "tracks_trunk_step", "watch_tracks"):
        assert z["stats__" + case][0] == 1 and z["out__%s__bad_ticks" % case][rc.BAD] == rc.K_TRAJ, case
    assert "out__traj__grip_trace" not in z and "out__traj_trace__grip_trace" in z
    for case in ("watch_tracks", "watch_plain"):
        assert (z["out__%s__neg_ticks" % case] > 0).any() or (z["out__%s__slack_min_tick" % case] > 0).any(), case
    assert z["out__watch_plain__slack_trace"].shape == (rc.K + rc.HOLD, 4, rc.B) and z["out__watch_tracks__slack_group_min"].shape == (4, rc.B // rc.GROUP)
    assert z["out__tracks__trace"].shape == (rc.K_TRAJ, 3, rc.B, 3) and z["out__plain__grip_trace"].shape == (rc.K + rc.HOLD, rc.B, 3)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_every_rollout_gives_the_recorded_bits(golden, mem):
    z = golden
    inputs = {k[4:]: v for k, v in z.items() if k.startswith("in__")}      # (the "b5__*" arrays are the test's below)
    conv = (lambda a: a) if mem == "host" else (lambda a: torch.from_numpy(a).cuda())
    bt = rc.handle()
    wrong = []
    for case, got, stats in rc.run_cases(bt, inputs, conv):
        rec = rc.CASES[case]
        want = {k[len("out__%s__" % rec):]: v for k, v in z.items() if k.startswith("out__%s__" % rec)}
        if set(got) != set(want):
            wrong.append((case, "keys", sorted(set(got) ^ set(want))))
            continue
        for k, v in got.items():
            if v.dtype != want[k].dtype or v.shape != want[k].shape:
                wrong.append((case, k, str(v.dtype), v.shape))
            elif v.tobytes() != want[k].tobytes():
                wrong.append((case, k))
        if stats.tolist() != z["stats__" + case].tolist():
            wrong.append((case, "stats", stats.tolist(), z["stats__" + case].tolist()))
    bt.close()
    print("%s: differing from the record: %s" % (mem, wrong or "nothing"))
    assert not wrong, wrong


@pytest.mark.parametrize("mem", ["host", "device"])
def test_state_slack_with_rotated_placements_gives_the_recorded_bits(golden, mem):
    """wbc_slack_kernel<ROT>, which no roll-out case launches: laikago_vx300 at B = 5 (a full wave and one with three padding rows), held to the
    bits recorded from the library before the whole-tree kernels shared a header"""
    z = golden
    inputs = {k[len("b5__in__"):]: v for k, v in z.items() if k.startswith("b5__in__")}
    want = {k[len("b5__out__"):]: v for k, v in z.items() if k.startswith("b5__out__")}
    assert inputs["q"].shape == (rc.B5, 27) and set(want) == {"slack", "which", "components"} and np.isfinite(want["slack"]).all()
    conv = (lambda a: a) if mem == "host" else (lambda a: torch.from_numpy(a).cuda())
    got = rc.run_b5(inputs, conv)
    wrong = [k for k in want if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes()]
    assert set(got) == set(want) and not wrong, wrong
