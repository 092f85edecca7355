#!/usr/bin/env python3
"""Small batches of the benchmark configuration (C3: the sim3 switch set) on each kernel that can take them — the packed kernel (four
instances per wavefront, refined), the general kernel with the structural presolve (one instance per wavefront, refined) and the compact
one-instance kernel (not refined: option refine = 0) — device-resident inputs, HIP events over 200 steps. The table behind the batch-size
policy of the sim3 family (csrc/wbc_api.hip WBC_SIM3P_MIN_BATCH) and the B = 1 latency.
    python tools/small_batch.py [cfg] [wave_order] [packed]
wave_order: the option's value (2: the packed kernel's wave order at every batch size — against the default this is what the order's entry loads and
its atomic cost a launch); packed: the packed kernel's column alone."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd")]
import numpy as np, torch, common
from wbc_batch import WbcBatch
wx, px = common.models()
name = sys.argv[1] if len(sys.argv) > 1 else "c3"
cfg = common.config(name, wx)
wave_order = int(sys.argv[2]) if len(sys.argv) > 2 else None
kernels = ({"packed_kernel": 1, "refine": 1}, {"packed_kernel": 0, "refine": 1}, {"packed_kernel": 0, "refine": 0})[:1 if "packed" in sys.argv[3:] else 3]
print("%-6s %6s | %-28s | %-28s | %-28s" % ("config", "B", "packed (refined)", "general + presolve (refined)", "compact one-instance (refine 0)"))
for B in (1, 4, 16, 64, 256, 512, 1024, 2048, 4096, 8192, 16384):
    bt = WbcBatch(wx, B); bt.configure(cfg)
    bt.set_option("packed_min_batch", 1)
    if wave_order is not None:
        bt.set_option("wave_order", wave_order)
    d = common.tick_inputs(wx, cfg, B, 5)
    dd = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    out = dict(qdot=torch.zeros((B, 26), dtype=torch.float64, device="cuda"), status=torch.zeros(B, dtype=torch.int32, device="cuda"), iters=torch.zeros(B, dtype=torch.int32, device="cuda"))
    cells = []
    for opts in kernels:
        for k, v in opts.items():
            bt.set_option(k, v)
        step = bt.make_tick_call(dd, out, 0.002)
        for _ in range(10): step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200): step()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 200 * 1e3
        cells.append("path %d %7.1f us %6.1f M/s" % (bt.stat("last_path"), us, B / us))
    print(" | ".join(["%-6s %6d" % (name, B)] + ["%-28s" % c for c in cells]), flush=True)
    bt.close()
