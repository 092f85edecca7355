#!/usr/bin/env python3
"""What a roll-out gradient along tracks costs against the calls it extends (recorded, not gated): on the benchmark's c3 inputs, K = 16 ticks,
B = 256, 4096 and 65536 (or the batches of argv[3]) in one process, device tensors in place, three tracks (the gripper on a HERMITE track
with default tangents, foot 0 on a LINEAR track, the trunk on a HERMITE track with the caller's tangents; S = 4),
    record_tracks  WbcBatch.rollout_record(tracks=...) alone     tracks  WbcBatch.rollout_tracks alone (what the record adds to the forward)
    vjp_tracks     WbcBatch.rollout_vjp over that tape alone     tick    wbc_tick alone (the unit the per-reverse-tick cost is stated in)
    record, vjp    the plain pair on the same inputs (tools/time_rollout_vjp.py's), for the difference the track adjoint makes per reverse tick
tools/time_rollout_vjp.py's protocol: warm-up, then ROUNDS rounds that alternate the runs, each REPS repeats between two device events; the
median over rounds and the spread (min .. max). Writes profiles/r26_track_vjp.txt (or argv[1]).
    python3 tools/time_track_vjp.py [out.txt] [K] [B,B,...]"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r26_track_vjp.txt")
K = int(sys.argv[2]) if len(sys.argv) > 2 else 16
BATCHES = tuple(int(x) for x in sys.argv[3].split(",")) if len(sys.argv) > 3 else (256, 4096, 65536)
DT, ROUNDS, REPS, WARM, S = 0.002, 5, 3, 2, 4

assert torch.cuda.is_available(), "time_track_vjp.py measures on the GPU; there is nothing to report without one"
model = wbc_model.load_model("a1_wx200")
cfg = wbc_model.sim3_config(model)
lines = ["# tools/time_track_vjp.py: a1_wx200, c3 (sim3 switch set), benchmark inputs (seed 0), K = %d ticks, seed g_q_final, three tracks (S = %d)" % (K, S),
         "# device tensors in place; %d rounds alternating the runs, %d calls between two device events each, %d warm-up calls; ms per call"
         % (ROUNDS, REPS, WARM),
         "# tape: %d bytes per instance + %d bytes per instance and tick" % (capi.TAPE_HEAD_BYTES, capi.TAPE_TICK_BYTES)]
for B in BATCHES:
    bt = WbcBatch(model, B)
    bt.configure(cfg)
    d = wbc_workload.make_tick_inputs(model, cfg, B, 0, lambda q: bt.fk(q, want=("oMf",))["oMf"])
    rng = np.random.default_rng(2)
    tracks = []
    for target, kind in ((4, "hermite"), (0, "linear"), ("trunk", "hermite")):
        base = d["trunk_target"] if target == "trunk" else d["ee_target"][:, target]
        t = dict(target=target, kind=kind, points=base[:, None, :] + rng.uniform(-0.01, 0.01, (B, S, 3)),
                 du=rng.uniform(0.05, 0.25, B))            # K du crosses a knot or two and some tracks reach their end
        if target == "trunk":
            t["tangents"] = rng.uniform(-0.01, 0.01, (B, S, 3))
        tracks.append({k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in t.items()})
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    rho = torch.from_numpy(np.random.default_rng(1).normal(0, 1.0, (B, 27))).cuda()
    rows = torch.from_numpy(wbc_model.task_params(cfg, B)).cuda()
    g_final = wbc_workload.raw_to_tangent(dev["q"], rho).contiguous()
    state = {}

    def run_record_tracks():
        state["rec_t"], state["tape_t"] = bt.rollout_record(dev, DT, K, task_params=rows, tape=state.get("tape_t"), tracks=tracks)

    def run_record():
        state["rec"], state["tape"] = bt.rollout_record(dev, DT, K, task_params=rows, tape=state.get("tape"))

    run_record_tracks()
    run_record()
    out_t = bt.rollout_vjp(state["tape_t"], g_q_final=g_final)
    out_p = bt.rollout_vjp(state["tape"], g_q_final=g_final)
    runs = dict(record_tracks=run_record_tracks, tracks=lambda: bt.rollout_tracks(dev, DT, K, tracks, task_params=rows),
                vjp_tracks=lambda: bt.rollout_vjp(state["tape_t"], g_q_final=g_final, out=out_t), record=run_record,
                vjp=lambda: bt.rollout_vjp(state["tape"], g_q_final=g_final, out=out_p), tick=lambda: bt.tick(dev, DT, task_params=rows))
    for fn in runs.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    dropped = int((out_t["ticks_dropped"] > 0).sum())
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / REPS)
    lines.append("# B = %d: %d instances with a dropped tick, %d with a grad_status" % (B, dropped, int((out_t["grad_status"] != 0).sum())))
    for k in runs:
        a = np.array(ms[k])
        lines.append(json.dumps(dict(B=B, what=k, median_ms=round(float(np.median(a)), 4), min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4))))
    med = {k: float(np.median(ms[k])) for k in runs}
    lines.append("# B = %d: record_tracks / tracks = %.3f; one reverse tick along tracks = vjp_tracks / K = %.4f ms = %.2f ticks (the plain sweep: %.2f ticks)" % (
        B, med["record_tracks"] / med["tracks"], med["vjp_tracks"] / K, med["vjp_tracks"] / K / med["tick"], med["vjp"] / K / med["tick"]))
    bt.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
