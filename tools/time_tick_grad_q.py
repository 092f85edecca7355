#!/usr/bin/env python3
"""What the state gradient of the tick costs (recorded, not gated): at B = 65536 on the benchmark's c3 inputs, in one process, device tensors
in place,
    vjp_state    wbc_tick_vjp_state alone (one launch of wbc_gradq_kernel)
    vjp          wbc_tick_vjp alone (one launch of wbc_grad_kernel)
    tick         wbc_tick_tp alone
    tick_grad_q  the whole WbcBatch.tick_grad_q: assemble, tick with the working set out, certificate, vjp_state
tools/time_tick_grad.py's protocol: warm-up, then ROUNDS rounds that alternate the four, each REPS repeats between two device events; the median
over rounds and the spread (min .. max). Writes profiles/r21_tick_grad_q.txt (or argv[1]).
    python3 tools/time_tick_grad_q.py [out.txt] [B]"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_tick_grad_q.txt")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
DT, ROUNDS, REPS, WARM = 0.002, 9, 10, 5

assert torch.cuda.is_available(), "time_tick_grad_q.py measures on the GPU; there is nothing to report without one"
model = wbc_model.load_model("a1_wx200")
cfg = wbc_model.sim3_config(model)
bt = WbcBatch(model, B)
bt.configure(cfg)
d = wbc_workload.make_tick_inputs(model, cfg, B, 0, lambda q: bt.fk(q, want=("oMf",))["oMf"])
dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
rng = np.random.default_rng(1)
tp = wbc_model.task_params(cfg, B)
tp *= np.exp(rng.uniform(np.log(0.5), np.log(2.0), tp.shape))
tpd = torch.from_numpy(tp).cuda()
v = torch.from_numpy(rng.normal(0, 1.0, (B, 26))).cuda()
v[:, model.nv:] = 0.0

c = bt.tick_certificate(dev, DT, task_params=tpd, v=v)
sens = dict(sens_bounds=c["sens_bounds"], sens_rows=c["sens_rows"], y_rows=c["y_rows"], status=c["status"], cert_status=c["cert_status"],
            working_set=c["working_set"], task_params=tpd)
gq = bt.tick_vjp_state(dev, DT, c["qdot"], c["sens_x"], **sens)
grads = bt.tick_vjp(dev, DT, c["qdot"], c["sens_x"], status=c["status"], cert_status=c["cert_status"], task_params=tpd)
torch.cuda.synchronize()
ok = int((gq["grad_status"] == 0).sum())
out_bytes = sum(t.numel() * t.element_size() for t in gq.values())
x, u = c["qdot"], c["sens_x"]


def run_vjp_state():
    bt.tick_vjp_state(dev, DT, x, u, out=gq, **sens)


def run_vjp():
    bt.tick_vjp(dev, DT, x, u, status=c["status"], cert_status=c["cert_status"], task_params=tpd, out=grads)


def run_tick():
    bt.tick(dev, DT, task_params=tpd)


def run_tick_grad_q():
    bt.tick_grad_q(dev, DT, v, task_params=tpd)


runs = dict(vjp_state=run_vjp_state, vjp=run_vjp, tick=run_tick, tick_grad_q=run_tick_grad_q)
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
lines = ["# tools/time_tick_grad_q.py: B = %d, a1_wx200, c3 (sim3 switch set), benchmark inputs (seed 0), rows x log-uniform [0.5, 2]; %d of %d instances"
         " solved and certified" % (B, ok, B),
         "# device tensors in place; %d rounds alternating the four, %d calls between two device events each, %d warm-up calls; ms per call"
         % (ROUNDS, REPS, WARM),
         "# vjp_state writes %.0f bytes per instance" % (out_bytes / B)]
for k in runs:
    t = np.array(ms[k])
    rec = dict(what=k, median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4),
               M_instances_per_s=round(B / float(np.median(t)) / 1e3, 1))
    lines.append(json.dumps(rec))
lines.append("# vjp_state / tick = %.3f; vjp_state / vjp = %.2f; tick_grad_q / tick = %.2f" % (
    np.median(ms["vjp_state"]) / np.median(ms["tick"]), np.median(ms["vjp_state"]) / np.median(ms["vjp"]),
    np.median(ms["tick_grad_q"]) / np.median(ms["tick"])))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
bt.close()
