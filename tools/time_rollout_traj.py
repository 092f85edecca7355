#!/usr/bin/env python3
"""Closed-loop ticks/s of wbc_rollout_traj (two milestones = one segment, summary on, no trace) and of wbc_rollout_tracks with two tracks
(the trunk on a four-milestone HERMITE spline, the gripper on the same LINEAR segment, both scored, no trace) against wbc_rollout on the
same inputs: what the per-tick trajectory kernel costs; and of wbc_rollout_watch, the same two-track call with all four slack families watched
(no trace): what the per-tick slack kernel costs. Same process, same handle, interleaved rounds, HIP events around each call.
    python3 tools/time_rollout_traj.py [B] [ticks] [rounds] [only]      only: run the calls whose label contains one of these comma-separated
                                                                        words (e.g. tracks, for a profiler run of that leg alone)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd"))
import numpy as np
import torch

import wbc_capi as capi
import wbc_model
import wbc_workload
from wbc_batch import WbcBatch

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 500
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ONLY = sys.argv[4] if len(sys.argv) > 4 else ""
DT = 0.002

model = wbc_model.load_model("a1_wx200")
cfg = wbc_model.sim3_config(model)
bt = WbcBatch(model, B)
bt.configure(cfg)
fk = lambda q: bt.fk(q, want=("oMf",))["oMf"]   # noqa: E731
d = wbc_workload.make_tick_inputs(model, cfg, B, 0, fk)
grip0 = fk(d["q"])[:, capi.FR_EE0 + 4, 9:]
d["ee_target"][:, 4] = grip0
d["prev_ee_target"][:, 4] = grip0
seg = np.array([0.0, 0.25, 0.0])                          # sim3.py's first segment: 0.25 m in 500 ticks
points = np.stack([grip0, grip0 + seg * (TICKS / 500.0)], axis=1)
step = np.zeros((B, 5, 3))
step[:, 4] = (points[:, 1] - points[:, 0]) / TICKS
dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
imu = dev["q"][:, 3:7].contiguous()
step_d, pts_d = torch.from_numpy(step).cuda(), torch.from_numpy(points).cuda()
# the trunk's track: four milestones within a centimetre of its target, crossed in the call's ticks (three knots between ticks)
trunk_pts = d["trunk_target"][:, None, :] + np.random.default_rng(1).normal(0, 0.003, (B, 4, 3))
trunk_pts[:, 0] = d["trunk_target"]
trunk_d = torch.from_numpy(trunk_pts).cuda()
two_tracks = [dict(target="trunk", points=trunk_d, kind="hermite", du=3.0 / TICKS), dict(target=4, points=pts_d, du=1.0 / TICKS)]

calls = {
    "wbc_rollout (no trace)": lambda: bt.rollout(dev, DT, TICKS, ee_target_step=step_d, imu=imu, want_trace=False),
    "wbc_rollout_traj (summary, no trace)": lambda: bt.rollout_traj(dev, DT, TICKS, pts_d, du=1.0 / TICKS, imu=imu),
    "wbc_rollout_tracks (trunk HERMITE + gripper LINEAR, both scored, no trace)":
        lambda: bt.rollout_tracks(dev, DT, TICKS, two_tracks, score=("trunk", 4), imu=imu),
    "wbc_rollout_watch (the two-track call, four slack families watched, no trace)":
        lambda: bt.rollout_watch(dev, DT, TICKS, tracks=two_tracks, score=("trunk", 4), imu=imu),
}
calls = {k: v for k, v in calls.items() if any(w in k for w in ONLY.split(","))}
ms = {k: [] for k in calls}
last = {}
for rnd in range(ROUNDS + 1):                             # (the first round settles clocks, caches and the lazy workspaces: not counted)
    for label, call in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        last[label] = call()
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            ms[label].append(e0.elapsed_time(e1))
for label, t in ms.items():
    med = float(np.median(t))
    print(json.dumps({"call": label, "B": B, "ticks": TICKS, "rounds": ROUNDS, "ms_median": round(med, 3), "ms_min": round(min(t), 3),
                      "ms_max": round(max(t), 3), "M_closed_loop_ticks_per_s": round(B * TICKS / med / 1e3, 2),
                      "last_path": bt.stat("last_path")}))
if len(calls) == 4:
    a, b, c, w = (float(np.median(ms[k])) for k in calls)
    print("# wbc_rollout_traj takes %+.2f %% against wbc_rollout (%.1f us per tick more)" % (100.0 * (b / a - 1.0), 1e3 * (b - a) / TICKS))
    print("# wbc_rollout_tracks (two tracks) takes %+.2f %% against wbc_rollout (%.1f us per tick more)" % (100.0 * (c / a - 1.0), 1e3 * (c - a) / TICKS))
    print("# wbc_rollout_watch (two tracks, four families) takes %+.2f %% against wbc_rollout_tracks (%.1f us per tick more)" % (100.0 * (w / c - 1.0), 1e3 * (w - c) / TICKS))
    old, new, tr, wa = (last[k] for k in calls)
    print("# watched against unwatched: q identical %s; slack minima %s, instances with a negative tick %s" % (
        bool((tr["q"] == wa["q"]).all().item()), [round(float(v), 4) for v in wa["slack_min"].min(dim=1).values.tolist()],
        (wa["neg_ticks"] > 0).sum(dim=1).tolist()))
    same = bool((old["status"] == new["status"]).all().item())
    print("# same inputs: status identical %s, q max-abs difference %.3e" % (same, float((old["q"] - new["q"]).abs().max().item())))
bt.close()
