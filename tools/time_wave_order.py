#!/usr/bin/env python3
"""The packed sim3 kernel's wave order (option "wave_order") on and off, in one process, rounds interleaved, HIP events:
    same       open-loop ticks on the same inputs every call (bench.py's case: the recorded order is an exact prediction)
    permuted   every call gets the inputs under another random permutation (the recorded order predicts nothing: its pure cost)
    rollout    wbc_rollout closed loop, the state moves every tick (stressed and un-stressed inputs)
ms per tick and M ticks/s for each; the outputs of the two settings are compared bit for bit. Last, the pass model: the sum over waves of
the largest dual-iteration count of a wave's four rows, for the identity grouping and for the exact and the useless order.
    python3 tools/time_wave_order.py [B] [K] [rounds]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd"))
import numpy as np, torch
import wbc_model, wbc_workload
from wbc_batch import WbcBatch

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
K = int(sys.argv[2]) if len(sys.argv) > 2 else 20
R = int(sys.argv[3]) if len(sys.argv) > 3 else 3
DT = 0.002
model = wbc_model.load_model("a1_wx200")
cfg = wbc_model.sim3_config(model)
bt = WbcBatch(model, B)
bt.configure(cfg)
fk = lambda q: bt.fk(q, want=("oMf",))["oMf"]


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


res = {}
for stress in (True, False):
    d = wbc_workload.make_tick_inputs(model, cfg, B, 0, fk, stress=stress)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    rng = np.random.default_rng(1)
    perms = [torch.from_numpy(rng.permutation(B)).cuda() for _ in range(2)]
    devp = [{k: v[p].contiguous() for k, v in dev.items()} for p in perms]
    out = dict(qdot=torch.empty((B, 26), dtype=torch.float64, device="cuda"), status=torch.empty(B, dtype=torch.int32, device="cuda"),
               iters=torch.empty(B, dtype=torch.int32, device="cuda"))
    same = bt.make_tick_call(dev, out, DT)
    pc = [bt.make_tick_call(x, out, DT) for x in devp]
    flip = [0]

    def permuted():
        pc[flip[0]]()
        flip[0] ^= 1
    step = torch.zeros((B, 5, 3), dtype=torch.float64, device="cuda")
    step[:, 4, 0] = 1e-4
    roll_out = {}

    def rollout(wo):
        roll_out[wo] = bt.rollout(dev, DT, K, ee_target_step=step, want_trace=False)
    tag = "stressed" if stress else "unstressed"
    for r in range(R):
        for wo in (1, 0):
            bt.set_option("wave_order", wo)
            for name, fn, n in (("same", same, K), ("permuted", permuted, K), ("rollout", lambda: rollout(wo), 1)):
                ms = timed(fn, n) / (K if name == "rollout" else 1)
                res.setdefault((tag, name, wo), []).append(ms)
    # bit-identical outputs: the last call of each setting on the same inputs, and the two roll-outs
    outs = {}
    for wo in (1, 0):
        bt.set_option("wave_order", wo)
        for _ in range(3):
            same()
        torch.cuda.synchronize()
        outs[wo] = {k: v.clone() for k, v in out.items()}
    ident = all(torch.equal(outs[1][k], outs[0][k]) for k in out) and \
        all(torch.equal(roll_out[1][k], roll_out[0][k]) for k in roll_out[0] if torch.is_tensor(roll_out[0][k]))
    print(json.dumps({"inputs": tag, "B": B, "bit_identical": bool(ident)}), flush=True)
    for name in ("same", "permuted", "rollout"):
        on, off = res[(tag, name, 1)], res[(tag, name, 0)]
        print(json.dumps({"inputs": tag, "case": name, "ms_per_tick_on": [round(x, 5) for x in on], "ms_per_tick_off": [round(x, 5) for x in off],
                          "M_ticks_per_s_on": round(B / np.median(on) / 1e3, 2), "M_ticks_per_s_off": round(B / np.median(off) / 1e3, 2),
                          "gain_pct": round(100.0 * (np.median(off) / np.median(on) - 1.0), 2)}), flush=True)
    # the passes a wave's QP loops run are set by the slowest of its four rows: sum over waves of the largest dual iteration count, for the
    # identity grouping and for the grouping the order gives (each slice's instances sorted by class: by their own class, the exact
    # prediction; by the class the other permutation had at the same index, the useless one)
    bt.set_option("wave_order", 0)
    its = []
    for x in [dev] + devp:
        o = bt.tick(x, DT)
        its.append(o["iters"].cpu().numpy().astype(np.int64) - int(o["iters"].min().item()))
    G = (B + 3) // 4
    ns = (G + 126) // 127
    grp = np.arange(G)
    members = [(4 * grp[grp % ns == g][:, None] + np.arange(4)).ravel() for g in range(ns)]
    cls = lambda it: np.where(it >= 10, 0, np.where(it >= 6, 1, np.where(it >= 3, 2, 5 - np.minimum(it, 2))))

    def wave_max(it, key):
        tot = 0
        for m in members:
            m = m[m < B]
            srt = m[np.argsort(key[m], kind="stable")]
            v = it[srt]
            v = np.concatenate([v, np.zeros((-len(v)) % 4, np.int64)])
            tot += int(v.reshape(-1, 4).max(axis=1).sum())
        return tot
    ident = int(np.concatenate([its[0], np.zeros(4 * G - B, np.int64)]).reshape(-1, 4).max(axis=1).sum())
    print(json.dumps({"inputs": tag, "sum_wave_max_iters": {"identity": ident, "exact": wave_max(its[0], cls(its[0])),
                                                           "useless": wave_max(its[1], cls(its[2])), "sum_iters": int(its[0].sum())}}), flush=True)
bt.close()
