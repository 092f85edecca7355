#!/usr/bin/env python3
"""What wbc_qp_certificate costs next to the solve it certifies: milliseconds of the cold solve and of the certificate launch (working set
given / read off x, without and with the sensitivities' right-hand side v), same process, warmed, HIP events — on tools/time_qp.py's
(m, n, p) = (32, 26, 16) recipe and on the c3 tick's own data (tools/time_qp_tick.py), B = 32768.
python tools/time_certify.py [B] > profiles/time_qp_certificate.txt"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd")]
import numpy as np, torch, common
from wbc_batch import WbcBatch
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32768


def timeit(f, n=10):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): r = f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, r


def report(what, bt, P):
    """P: A, b, C, lb, ub, Clb, Cub on the device"""
    args = (P["A"], P["b"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"])
    for _ in range(30): bt.qp_solve_ls(*args)                      # (also warms the clocks up)
    ms_solve, _ = timeit(lambda: bt.qp_solve_ls(*args))
    x, st, it, ws = bt.qp_solve_ls(*args, want_working_set=True)
    v = torch.randn_like(x)
    kw = dict(A=P["A"], b=P["b"], C_=P["C"], lb=P["lb"], ub=P["ub"], Clb=P["Clb"], Cub=P["Cub"], status=st)
    print("%s B = %d: cold solve (wbc_qp_solve_ls, path %d) %.3f ms  optimal %.3f  iters %.2f" % (
        what, B, bt.stat("last_qp_path"), ms_solve, (st == 0).double().mean().item(), it.double().mean().item()), flush=True)
    for label, extra in (("working set given", dict(working_set=ws)), ("active set read off x", dict()),
                         ("working set given, with v (sensitivities)", dict(working_set=ws, v=v))):
        ms, c = timeit(lambda: bt.qp_certificate(x, **kw, **extra))
        ok = c["cert_status"] == 0
        print("%s B = %d: certificate, %-42s %.3f ms = %.2f x the solve  OK %.3f  mean k %.1f  worst |grad f - N'y| %.1e  wrong-signed > 1e-9: %d" % (
            what, B, label + ":", ms, ms / ms_solve, ok.double().mean().item(), c["n_active"].double().mean().item(),
            c["kkt"][ok, 0].max().item(), int((c["kkt"][ok, 2] > 1e-9).sum().item())), flush=True)


rng = np.random.default_rng(0)
m, n, p = 32, 26, 16
P = dict(A=rng.normal(size=(B, m, n)), b=rng.normal(size=(B, m)), C=rng.normal(size=(B, p, n)), lb=-np.ones((B, n)) * 0.5, ub=np.ones((B, n)) * 0.5,
         Clb=-np.ones((B, p)), Cub=np.ones((B, p)))
bt = WbcBatch([], B)
report("random (32, 26, 16)", bt, {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in P.items()})
bt.close()

wx, _ = common.models()
cfg = common.config("c3", wx)
bt = WbcBatch(wx, B); bt.configure(cfg)
d = common.tick_inputs(wx, cfg, B, 5)
dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in d.items()}
a = bt.assemble(dev, 0.002)
report("c3 tick's own data (%d, 26, %d)" % (a["A"].shape[1], a["C"].shape[1]), bt, a)
ms, _ = timeit(lambda: bt.tick(dev, 0.002))
print("c3 the fused wbc_tick on the same instances: %.3f ms" % ms)
bt.close()
