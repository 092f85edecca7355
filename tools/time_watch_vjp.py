#!/usr/bin/env python3
"""What the slack cotangent costs (recorded, not gated): on the benchmark's c3 inputs, K = 16 ticks, B = 256, 4096 and 65536 (or the batches
of argv[3]) in one process on one handle, device tensors in place, the box centre displaced (at the stock inputs the angle components tie),
    vjp            WbcBatch.rollout_vjp over a recorded roll-out, seed g_q_final (wbc_rollout_vjp)
    vjp_watched    the same call with watch_seed = a cotangent on every tick's slack of the four families as well (wbc_rollout_vjp_watched: one
                   more launch per reverse tick)
    vjp_watch_only the watch seed alone
    vjp_trace      the call the watch seed replaces: wbc_rollout_vjp with a [K][B][26] g_q_trace (the trace already on the device)
    slack          wbc_state_slack (the forward at one state)    slack_vjp   wbc_state_slack_vjp (its cotangent)    tick   wbc_tick
tools/time_rollout_vjp.py's protocol: warm-up, then ROUNDS rounds that alternate the runs, each REPS repeats between two device events; the
median over rounds and the spread (min .. max). The seed's share is (vjp_watched - vjp) / vjp_watched per reverse tick; the layer's cost is
given in ticks. Writes profiles/r30_watch_vjp.txt (or argv[1]).
    python3 tools/time_watch_vjp.py [out.txt] [K] [B,B,...]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd"))
import numpy as np
import torch

import wbc_model
import wbc_workload
from wbc_batch import WbcBatch

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r30_watch_vjp.txt")
K = int(sys.argv[2]) if len(sys.argv) > 2 else 16
BATCHES = tuple(int(x) for x in sys.argv[3].split(",")) if len(sys.argv) > 3 else (256, 4096, 65536)
DT, ROUNDS, REPS, WARM = 0.002, 5, 3, 2
WATCH = ("com", "trunk_z", "trunk_ang", "joint")

assert torch.cuda.is_available(), "time_watch_vjp.py measures on the GPU; there is nothing to report without one"
model = wbc_model.load_model("a1_wx200")
cfg = wbc_model.sim3_config(model)
lines = ["# tools/time_watch_vjp.py: a1_wx200, c3 (sim3 switch set), benchmark inputs (seed 0), K = %d ticks, the four slack families watched" % K,
         "# device tensors in place; %d rounds alternating the runs, %d calls between two device events each, %d warm-up calls; ms per call"
         % (ROUNDS, REPS, WARM)]
for B in BATCHES:
    bt = WbcBatch(model, B)
    bt.configure(cfg)
    d = wbc_workload.make_tick_inputs(model, cfg, B, 0, lambda q: bt.fk(q, want=("oMf",))["oMf"])
    rng = np.random.default_rng(11)
    d["trunk_box_center"] = d["trunk_box_center"] * np.concatenate([1.0 + rng.uniform(-0.15, 0.15, (B, 1)), np.ones((B, 3))], axis=1)
    d["trunk_box_center"][:, 1:] += rng.uniform(-0.1, 0.1, (B, 3))
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    rho = torch.from_numpy(np.random.default_rng(1).normal(0, 1.0, (B, 27))).cuda()
    rows = torch.from_numpy(wbc_model.task_params(cfg, B)).cuda()
    g_final = wbc_workload.raw_to_tangent(dev["q"], rho).contiguous()
    g_trace = torch.from_numpy(np.random.default_rng(3).normal(0, 1.0, (K, B, 26))).cuda()
    g_slack = torch.ones((B, 4), dtype=torch.float64, device="cuda")
    rec, tape = bt.rollout_record(dev, DT, K, task_params=rows, watch=WATCH, want_trace=False)
    seed = dict(mask=WATCH, q_final=rec["q"], g_trace=torch.ones((K, 4, B), dtype=torch.float64, device="cuda"))
    out_p = bt.rollout_vjp(tape, g_q_final=g_final)
    out_w = bt.rollout_vjp(tape, g_q_final=g_final, watch_seed=seed)
    runs = dict(vjp=lambda: bt.rollout_vjp(tape, g_q_final=g_final, out=out_p),
                vjp_watched=lambda: bt.rollout_vjp(tape, g_q_final=g_final, out=out_w, watch_seed=seed),
                vjp_watch_only=lambda: bt.rollout_vjp(tape, out=out_w, watch_seed=seed),
                vjp_trace=lambda: bt.rollout_vjp(tape, g_q_final=g_final, g_q_trace=g_trace, out=out_p),
                slack=lambda: bt.state_slack(dev["q"], dev["trunk_box_center"]),
                slack_vjp=lambda: bt.state_slack_grad(dev["q"], dev["trunk_box_center"], g_slack=g_slack),
                tick=lambda: bt.tick(dev, DT, task_params=rows))
    for fn in runs.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
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
    lines.append("# B = %d: %d instances with a dropped tick, %d with a grad_status" % (
        B, int((out_w["ticks_dropped"] > 0).sum()), int((out_w["grad_status"] != 0).sum())))
    for k in runs:
        a = np.array(ms[k])
        lines.append(json.dumps(dict(B=B, what=k, median_ms=round(float(np.median(a)), 4), min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4))))
    med = {k: float(np.median(ms[k])) for k in runs}
    extra = (med["vjp_watched"] - med["vjp"]) / K
    lines.append("# B = %d: the watch seed = (vjp_watched - vjp) / K = %.4f ms per reverse tick = %.1f %% of a watched reverse tick (%.4f ms) = %.2f ticks; "
                 "wbc_state_slack_vjp %.4f ms = %.2f ticks against wbc_state_slack %.4f ms = %.2f ticks (both with their output allocations)" % (
                     B, extra, 100.0 * extra / (med["vjp_watched"] / K), med["vjp_watched"] / K, extra / med["tick"], med["slack_vjp"],
                     med["slack_vjp"] / med["tick"], med["slack"], med["slack"] / med["tick"]))
    bt.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
