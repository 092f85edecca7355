#!/usr/bin/env python3
"""What the gradient of the state step costs (recorded, not gated): at B = 65536 on the benchmark's c3 inputs, in one process, device tensors
in place,
    step_vjp         wbc_step_vjp alone, mode RUNNING without an IMU quaternion (one launch of wbc_stepvjp_kernel)
    step_vjp_warmup  the same in mode WARMUP (no kinematics: the integrate part alone)
    step_forward     what it differentiates: wbc_integrate, then wbc_update_state
    tick             wbc_tick alone
tools/time_tick_grad_q.py's protocol: warm-up, then ROUNDS rounds that alternate the four, each REPS repeats between two device events; the
median over rounds and the spread (min .. max). Writes profiles/r23_step_vjp.txt (or argv[1]).
    python3 tools/time_step_vjp.py [out.txt] [B]"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23_step_vjp.txt")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
DT, ROUNDS, REPS, WARM = 0.002, 9, 10, 5

assert torch.cuda.is_available(), "time_step_vjp.py measures on the GPU; there is nothing to report without one"
model = wbc_model.load_model("a1_wx200")
cfg = wbc_model.sim3_config(model)
bt = WbcBatch(model, B)
bt.configure(cfg)
d = wbc_workload.make_tick_inputs(model, cfg, B, 0, lambda q: bt.fk(q, want=("oMf",))["oMf"])
dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
rng = np.random.default_rng(1)
g = torch.from_numpy(rng.normal(0, 1.0, (B, 26))).cuda()
g[:, model.nv:] = 0.0
t = bt.tick(dev, DT)
x, q, ft = t["qdot"], dev["q"], dev["ee_target"]
out = bt.step_vjp(q, x, ft, g, DT)
outw = bt.step_vjp(q, x, ft, g, DT, mode=capi.ROLLOUT_WARMUP)
torch.cuda.synchronize()
ok = int((out["grad_status"] == 0).sum())
out_bytes = sum(v.numel() * v.element_size() for v in out.values())


def run_step_vjp():
    bt.step_vjp(q, x, ft, g, DT, out=out)


def run_step_vjp_warmup():
    bt.step_vjp(q, x, ft, g, DT, mode=capi.ROLLOUT_WARMUP, out=outw)


def run_step_forward():
    bt.update_state(q, bt.integrate(q, x, DT), ft)


def run_tick():
    bt.tick(dev, DT)


runs = dict(step_vjp=run_step_vjp, step_vjp_warmup=run_step_vjp_warmup, step_forward=run_step_forward, tick=run_tick)
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
lines = ["# tools/time_step_vjp.py: B = %d, a1_wx200, c3 (sim3 switch set), benchmark inputs (seed 0), qdot of the tick itself, g ~ N(0, 1); %d of %d"
         " instances with grad_status 0" % (B, ok, B),
         "# device tensors in place; %d rounds alternating the four, %d calls between two device events each, %d warm-up calls; ms per call"
         % (ROUNDS, REPS, WARM),
         "# step_vjp writes %.0f bytes per instance; step_forward allocates its two outputs per call" % (out_bytes / B)]
for k in runs:
    a = np.array(ms[k])
    rec = dict(what=k, median_ms=round(float(np.median(a)), 4), min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4),
               M_instances_per_s=round(B / float(np.median(a)) / 1e3, 1))
    lines.append(json.dumps(rec))
lines.append("# step_vjp / tick = %.3f; step_vjp_warmup / tick = %.3f; step_vjp / step_forward = %.2f" % (
    np.median(ms["step_vjp"]) / np.median(ms["tick"]), np.median(ms["step_vjp_warmup"]) / np.median(ms["tick"]),
    np.median(ms["step_vjp"]) / np.median(ms["step_forward"])))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
bt.close()
