#!/usr/bin/env python3
"""bench.py — WBC control ticks per second on MI355X (BASELINE.json metric), one JSON line on rank 0.

A "step" is ONE pass of the fused hot path (wbc_tick: FK -> Jacobians -> task stack -> H, g, C, bounds -> QP -> q̇)
over one batch of synthetic robot states already resident in HBM. Workload (config.workload): BASELINE configs[2],
"Batch=65536 A1+wx200 with 4-foot contact + ... inequalities, 1 MI355X" = SURVEY.md §8(d) C3: the reference's sim3
switch set (Grip task + posture; 12 contact equalities, 4 trunk-box rows, 26 velocity-damper bounds, 3 locked DoF).
With --gpus N every rank runs its own 65536-instance shard on its own GPU — no data-path collective —
and the job value is the sum: scaling "weak". Ranks: either torch.distributed.run starts them (RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* in the environment), or — a plain `python bench.py --gpus N` — this process starts N fresh child
interpreters itself (`launch_ranks`: the parent never imports torch or touches a GPU, no exec), forwards rank 0's JSON
line and returns the worst child's exit code.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--repeats R] [--batch B] [--no-cpu-baseline] [--dump-outputs DIR]

Timing: after at least W warm-up steps (the GPU engine warms up for SETTLE_S at least: from idle the tick needs ~100 steps
before its time per step settles), EXACTLY K timed steps, split into R blocks (default 1) whose sizes add up to K, each
block bracketed by barrier + device synchronise on both sides and reduced with MAX over the ranks; `value` / `ms_per_step`
come from the MEDIAN block (per step), every block is listed under "repeats". --dump-outputs DIR writes what the last timed step
returned on rank 0 (qdot, status, iters) as DIR/<name>.npy in float64; the inputs depend only on the arguments.
Extra objects on the line: "roofline" (algorithmic HBM bytes/tick x ticks / kernel time from HIP events on the launch stream
against 8 TB/s — reported because the contract asks for it; what bounds this kernel is issue/latency, see
"issue") and "cpu_baseline" (the CPU oracle, oracle/wbc_oracle.c, timed on this host's cores on a bounded sample of the
same inputs — the oracle is only the yardstick/checker here, never the thing measured). The run FAILS (exit code 1, line
still printed) if the q̇ error against the oracle exceeds the tolerance or any solver status differs.

The per-rank body is `run_rank(args, comm, engine)`: `comm` wraps torch.distributed (RCCL on the GPUs; tests/ drive the same
function over gloo on CPU ranks with an engine whose tick is the oracle), `engine` is the thing that ticks.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd"))

import numpy as np  # noqa: E402

# q 27*8 + targets 18*8 in, q̇ 26*8 + status 4 out
ALGO_BYTES_PER_TICK = 572
# what wbc_tick really streams per instance (adds prev targets 144 B, box centre 32 B, trunk refs 96 B, iters 4 B)
ACTUAL_BYTES_PER_TICK = 216 + 120 + 120 + 32 + 208 + 4 + 4
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_PEAK_TFLOPS = 78.6        # MI355X FP64 vector = matrix peak
ALGO_FLOP_PER_TICK = 5.5e4     # dense count of the n = 26 problem (+ ~1e4 per working-set change)
REDUCED_FLOP_PER_TICK = 1.1e4  # the problem the sim3 kernels actually solve (n' = 11, no equalities): DESIGN.md §4
PMC_PROFILE = "r04_pmc_summary_packed.txt"   # committed rocprofv3 PMC passes the static roofline.issue fields come from (tools/gpu_profile.sh)
TRAFFIC_PROFILE = "r04_traffic_calibration.txt"   # FETCH_SIZE / WRITE_SIZE of the tick kernel, calibrated against known-byte-count kernels in the
                                                  # tick's own access pattern (tools/calib_traffic.sh): roofline.traffic
DT = 0.002
QDOT_TOL = 1e-5
SETTLE_S = 0.1                 # minimum warm-up time of the GPU engine (clocks ramp for ~20 ms after idle)


def _pmc_lines(kernels):
    path = os.path.join(ROOT, "profiles", os.environ.get("WBC_PMC_PROFILE", PMC_PROFILE))
    out = {}
    try:
        for line in open(path):
            for kn in kernels:
                if kn in line:
                    parts = line.split()
                    for i, tok in enumerate(parts):
                        if tok.startswith("per_dispatch="):
                            out.setdefault(kn, {})[parts[i - 3]] = float(tok.split("=")[1])
    except Exception:
        return {}, path
    return out, path


def pmc_static():
    """roofline.traffic and roofline.issue from the COMMITTED rocprofv3 PMC passes of this same command (separate --pmc runs,
    tools/gpu_profile.sh): constants of that profile, not measurements of this run — marked "static_from_profile"."""
    v, path = _pmc_lines(("wbc_tick_sim3p_kernel", "wbc_tick_deferred_kernel"))
    s = v.get("wbc_tick_sim3p_kernel")
    if not s:
        return None, None
    traffic = 0.0
    try:     # bytes per 65536-tick dispatch: counters x the factors measured on tools/calib_traffic's tick-pattern kernel (FETCH_SIZE reads ~1/2 on gfx950)
        for line in open(os.path.join(ROOT, "profiles", TRAFFIC_PROFILE)):
            if line.startswith("CALIBRATED_TRAFFIC_BYTES_PER_DISPATCH"):
                traffic = float(line.split()[1]) / 1024.0
    except Exception:
        traffic = 0.0
    try:
        cu_cycles = 256.0 * s["GRBM_GUI_ACTIVE"] / 8.0
        ticks = 65536.0                      # the profile was taken at the bench batch; the packed kernel runs four ticks per wave
        issue = {"valu_busy": s["SQ_ACTIVE_INST_VALU"] / cu_cycles, "lds_busy": s["SQ_LDS_IDX_ACTIVE"] / cu_cycles,
                 "valu_insts_per_tick": s["SQ_INSTS_VALU"] / ticks, "lds_insts_per_tick": s["SQ_INSTS_LDS"] / ticks,
                 "salu_insts_per_tick": s["SQ_INSTS_SALU"] / ticks, "ticks_per_wave": ticks / s["SQ_WAVES"],
                 "lds_bank_conflict_rate": s["SQ_LDS_BANK_CONFLICT"] / s["SQ_LDS_IDX_ACTIVE"],
                 "static_from_profile": os.path.relpath(path, ROOT)}
    except KeyError:
        issue = None
    return (traffic * 1024.0 if traffic else None), issue


# ------------------------------------------------------------------------------------------------ communication
class Comm:
    """torch.distributed as the benchmark uses it: a barrier and a MAX all-reduce — nothing on the data path."""

    def __init__(self, backend, rank, world, device=None, force=False):
        """force: create the process group at world size 1 too (tests: the RCCL barrier / all-reduce on one GPU)"""
        self.rank, self.world, self.device = rank, world, device
        self.dist = None
        if world > 1 or force:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if not dist.is_initialized():
                kw = {"device_id": device} if (backend == "nccl" and device is not None) else {}
                dist.init_process_group(backend, rank=rank, world_size=world, **kw)
            self.dist = dist

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()

    def max(self, values):
        """element-wise max over the ranks of a list of floats"""
        if self.dist is None:
            return [float(v) for v in values]
        import torch
        t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=self.device if self.device is not None else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return [float(v) for v in t.cpu()]

    def close(self):
        if self.dist is not None:
            self.dist.barrier()
            self.dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ the GPU engine
class GpuEngine:
    """wbc_tick on one MI355X through the C-ABI (WbcBatch); inputs generated with the product's own FK, resident in HBM."""
    name = "hip"
    settle_s = SETTLE_S

    def __init__(self, args, local):
        import torch
        import wbc_model
        from wbc_batch import WbcBatch
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the product path)")
        torch.cuda.set_device(local)
        self.torch, self.dev, self.args = torch, torch.device("cuda", local), args
        self.model = wbc_model.load_model("a1_wx200")
        self.cfg = wbc_model.sim3_config(self.model, Joint=args.posture)
        self.bt = WbcBatch(self.model, args.batch, device_id=local)
        self.bt.configure(self.cfg)
        self.options = {"jtj_mfma": int(args.jtj_mfma), "presolve": 1, "presolve_orth": 1, "sim3_kernel": 1, "packed_kernel": 1, "packed_update": 1,
                        "dbg_alias_inputs": 0, "refine": 1}
        for env, opt in (("WBC_PRESOLVE", "presolve"), ("WBC_PRESOLVE_ORTH", "presolve_orth"), ("WBC_SIM3_KERNEL", "sim3_kernel"),
                         ("WBC_PACKED_KERNEL", "packed_kernel"), ("WBC_PACKED_UPDATE", "packed_update"), ("WBC_DBG_ALIAS", "dbg_alias_inputs"),
                         ("WBC_REFINE", "refine")):
            if os.environ.get(env) not in (None, ""):       # diagnostic A/B switches: they change WHAT is measured, so they are reported
                self.options[opt] = int(os.environ[env])
        for k, v in self.options.items():
            self.bt.set_option(k, v)

    def fk(self, q):
        return self.bt.fk(q, want=("oMf",))["oMf"]

    def load(self, host_in):
        t = self.torch
        B = host_in["q"].shape[0]
        self.dev_in = {k: t.from_numpy(np.ascontiguousarray(v)).to(self.dev) for k, v in host_in.items()}
        self.dev_out = dict(qdot=t.zeros((B, 26), dtype=t.float64, device=self.dev), status=t.zeros(B, dtype=t.int32, device=self.dev),
                            iters=t.zeros(B, dtype=t.int32, device=self.dev))
        self.step = self.bt.make_tick_call(self.dev_in, self.dev_out, DT)

    def sync(self):
        self.torch.cuda.synchronize()

    def timed_block(self, steps):
        """-> kernel milliseconds of the block from HIP events on the launch stream (the C-ABI launches on torch's current one)"""
        ev0, ev1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(steps):
            self.step()
        ev1.record()
        return lambda: ev0.elapsed_time(ev1)

    def results(self):
        return {k: v.cpu().numpy() for k, v in self.dev_out.items()}

    def path(self):
        return {2: "wbc_tick_sim3p_kernel (packed: four instances per wavefront; one kernel per tick, what it cannot reduce is redone in its own tail)",
                1: "wbc_tick_sim3_kernel (+ wbc_tick_deferred_kernel)"}.get(self.bt.stat("last_path"), "wbc_tick_kernel<MODE_TICK>")

    def closed_loop(self, host_in, ticks):
        t = self.torch
        B = host_in["q"].shape[0]
        dev_in = {k: t.from_numpy(np.ascontiguousarray(v)).to(self.dev) for k, v in host_in.items()}
        step_t = t.zeros((B, 5, 3), dtype=t.float64, device=self.dev)
        step_t[:, 4, 0] = 1e-4
        self.bt.rollout(dev_in, DT, 2, ee_target_step=step_t, want_trace=False)
        self.sync()
        t1 = time.perf_counter()
        ro = self.bt.rollout(dev_in, DT, ticks, ee_target_step=step_t, want_trace=False)
        self.sync()
        t_roll = time.perf_counter() - t1
        st = ro["status"].cpu().numpy()
        return {"value": float(B) * ticks / t_roll, "ms_per_tick": 1e3 * t_roll / ticks,
                "worst_status_histogram": {name: int((st == code).sum()) for code, name in enumerate(("optimal", "max_iter", "infeasible", "numerical"))},
                "optimal_frac": float((st == 0).mean()), "iters_per_tick": float(ro["iters"].double().mean().item()) / ticks}

    def other_configs(self, check=True):
        """Context for the headline (not bench lines): BASELINE configs[1] (five EE tasks + CoM task, contact equalities, no
        velocity box) at its own batch 1024 and at 65536, the warm-up problem and the tests' all-tasks / all-constraints stack at 65536 —
        each on the kernel the library picks."""
        import wbc_model
        import wbc_workload
        from wbc_batch import WbcBatch
        t = self.torch
        out = {}
        # (name, configuration, batch sizes): BASELINE configs[1], and the warm-up problem of setInitialState (Robot_Wrapper4.py:196-351, SURVEY §8 f4:
        #  six Cartesian tasks + Tikhonov, velocity box only — 2000 of these per robot)
        cases = (("c2", wbc_model.equality_only_config(self.model), (1024, 65536)),
                 ("warmup", wbc_model.make_config(self.model, Trunk=True, FR=True, FL=True, RR=True, RL=True, Grip=True, Joint=True), (65536,)),
                 # every task and every constraint type at once (tests/common.py "everything": coverage, not a reference preset)
                 ("everything", wbc_model.make_config(self.model, Trunk=True, FR=True, FL=True, RR=True, RL=True, Grip=True, Joint="PREV", task_com=True, cCoM=True,
                                                      cTrunk=True, cFR=True, cFL=True, cRR=True, cRL=True, mode="static_reach"), (65536,)))
        for name, cfg, B in ((n_, c_, b_) for n_, c_, bs in cases for b_ in bs):
            bt = WbcBatch(self.model, B, device_id=self.dev.index)
            bt.configure(cfg)

            class FK:
                def __call__(_, q):
                    return bt.fk(q, want=("oMf",))["oMf"]

                def com(_, q):
                    return bt.fk(q, want=("com",))["com"]
            d = wbc_workload.make_tick_inputs(self.model, cfg, B, 5, FK())
            dev_in = {k: t.from_numpy(np.ascontiguousarray(v)).to(self.dev) for k, v in d.items()}
            dev_out = dict(qdot=t.zeros((B, 26), dtype=t.float64, device=self.dev), status=t.zeros(B, dtype=t.int32, device=self.dev),
                           iters=t.zeros(B, dtype=t.int32, device=self.dev))
            step = bt.make_tick_call(dev_in, dev_out, DT)
            for _ in range(3):
                step()
            self.sync()
            ev0, ev1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(10):
                step()
            ev1.record()
            self.sync()
            ms = ev0.elapsed_time(ev1) / 10
            path = bt.stat("last_path")
            acc = {"gated": False}
            if check:       # the same run's answers against the oracle on a sub-sample (the checker, after the timed region): these numbers are quoted too
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import oracle
                nchk = min(B, 2048)
                ref = oracle.tick([self.model], [cfg], {k: v[:nchk] for k, v in d.items()}, DT, nchk, nthreads=min(32, len(os.sched_getaffinity(0))), want_q_next=False)
                gq, gs = dev_out["qdot"][:nchk].cpu().numpy(), dev_out["status"][:nchk].cpu().numpy()
                okc = (ref["status"] == 0) & (gs == 0)
                acc = {"gated": True, "instances_checked": int(nchk), "status_agree_frac": float((ref["status"] == gs).mean()),
                       "qdot_max_abs_err_vs_cpu": float(np.abs(gq - ref["qdot"])[okc].max()) if okc.any() else None}
            out["%s_B%d" % (name, B)] = {"ticks_per_s": B / ms * 1e3, "ms_per_step": ms, "task_rows": bt.task_rows, "constraint_rows": bt.constraint_rows,
                                         "optimal_frac": float((dev_out["status"] == 0).double().mean().item()), "accuracy": acc,
                                         "kernel_path": ("wbc_tick_orthp_kernel<INEQ> (packed: four instances per wavefront)" if bt.constraint_rows > 12 else
                                                         "wbc_tick_orthp_kernel (packed: four instances per wavefront)") if path == 3 else
                                                        "wbc_tick_boxp_kernel (packed: four instances per wavefront)" if path == 4 else
                                                        ("wbc_tick_kernel<MODE_TICK, ORTH>" if bt.stat("last_orth") else "wbc_tick_kernel<MODE_TICK>")}
            bt.close()
        # the reference's own plug-in boundary, QP(A, b, C, lb, ub, Clb, Cub).solveQP() = wbc_qp_solve_ls (QP_Wrapper.py:10-53), on the headline
        # workload's OWN problems (the first 32768 instances' A, b, C, bounds as wbc_assemble forms them on the device) — the packed QP kernel
        Bq = min(32768, int(self.dev_in["q"].shape[0]))
        bq = WbcBatch(self.model, Bq, device_id=self.dev.index)
        bq.configure(self.cfg)
        sub = {k: v[:Bq] for k, v in self.dev_in.items()}
        asm = bq.assemble(sub, DT)
        qp_in = [asm[k] if t.is_tensor(asm[k]) else t.from_numpy(np.ascontiguousarray(asm[k])).to(self.dev) for k in ("A", "b", "C", "lb", "ub", "Clb", "Cub")]
        for _ in range(3):
            res = bq.qp_solve_ls(*qp_in)
        self.sync()
        ev0, ev1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(10):
            res = bq.qp_solve_ls(*qp_in)
        ev1.record()
        self.sync()
        ms = ev0.elapsed_time(ev1) / 10
        acc = {"gated": False}
        xq, sq = (res[0].cpu().numpy(), res[1].cpu().numpy()) if t.is_tensor(res[0]) else (res[0], res[1])
        if check:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import oracle
            nchk = min(Bq, 2048)
            hst = [v[:nchk].cpu().numpy() for v in qp_in]
            xr, sr, _ = oracle.qp_solve_ls(*hst, nthreads=min(32, len(os.sched_getaffinity(0))))
            okc = (sr == 0) & (sq[:nchk] == 0)
            acc = {"gated": True, "instances_checked": int(nchk), "status_agree_frac": float((sr == sq[:nchk]).mean()),
                   "qdot_max_abs_err_vs_cpu": float(np.abs(xq[:nchk] - xr)[okc].max()) if okc.any() else None}
        out["qp_boundary_B%d" % Bq] = {"qps_per_s": Bq / ms * 1e3, "ms_per_step": ms, "m_n_p": [int(qp_in[0].shape[1]), int(qp_in[0].shape[2]), int(qp_in[2].shape[1])],
                                       "optimal_frac": float((sq == 0).mean()), "accuracy": acc, "problems_per_wavefront": bq.stat("last_qp_path"),
                                       "kernel_path": "wbc_qp_packed_kernel (stand-alone QP: wbc_qp_solve_ls on the headline workload's own A, b, C, bounds)"}
        bq.close()
        return out

    def close(self):
        self.bt.close()


# ------------------------------------------------------------------------------------------------ the per-rank body
def run_rank(args, comm, engine, make_inputs):
    """What every rank does: seed-by-rank inputs -> warm-up -> R bracketed blocks of K steps -> MAX over ranks ->
    rank 0 assembles the JSON line. Returns (line or None, results dict)."""
    rank, world = comm.rank, comm.world
    B, K = args.batch, args.steps
    if K < 1:
        raise SystemExit("--steps must be at least 1")
    R = min(max(1, args.repeats), K)
    sizes = [K // R + (1 if i < K % R else 0) for i in range(R)]    # the blocks' steps: K in all
    host_in = make_inputs(engine, B, seed=rank, stress=True)
    engine.host_in = host_in
    engine.load(host_in)

    def barrier():
        engine.sync()
        comm.barrier()
        engine.sync()

    for _ in range(args.warmup):
        engine.step()
    warm = args.warmup
    settle = getattr(engine, "settle_s", 0.0)
    if settle > 0:                                  # the W steps and then more, in tens, until the warm-up has lasted settle_s
        engine.sync()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < settle:
            for _ in range(10):
                engine.step()
            engine.sync()
            warm += 10
    elapsed, kernel_ms = [], []
    for k in sizes:
        barrier()
        t0 = time.perf_counter()
        km = engine.timed_block(k)
        barrier()
        elapsed.append(time.perf_counter() - t0)
        kernel_ms.append(km() / k)
    elapsed = comm.max(elapsed)                     # the job is as slow as its slowest rank, block by block
    res = engine.results()
    if rank != 0:
        return None, res
    per_step = [e / k for e, k in zip(elapsed, sizes)]
    order = np.argsort(per_step)
    med = int(order[len(order) // 2])
    t_med, k_med = per_step[med], kernel_ms[med]    # seconds / milliseconds of ONE step
    ticks = float(B) * world
    ach = ALGO_BYTES_PER_TICK * B / (k_med * 1e-3) / 1e9
    traffic, issue = pmc_static()
    status, iters = res["status"], res["iters"]
    line = {
        "metric": "wbc_qp_solves_per_sec", "value": ticks / t_med, "unit": "ticks/s", "n_gpus": world,
        "steps": K, "warmup": args.warmup, "warmup_steps_run": warm, "ms_per_step": 1e3 * t_med,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "BASELINE configs[2] / SURVEY C3: A1+wx200 (nq 27, nv 26), sim3 switch set: Grip task + " + args.posture + " posture, "
                               "12 contact equalities + 4 trunk-box rows + 26 damper bounds (3 locked), m=32 p=16 n=26",
                   "batch_per_gpu": B, "global_batch": B * world, "dt": DT, "parallelism": "shard%d (no collective)" % world,
                   "engine": engine.name, "backend": getattr(engine, "backend", None), "kernel_path": engine.path(), "options": getattr(engine, "options", {}),
                   "jtj": "mfma_f64" if getattr(engine, "options", {}).get("jtj_mfma", -1) > 0 else "valu_f64"},
        "repeats": {"n": R, "steps_per_block": sizes, "ms_per_step": [1e3 * e for e in per_step], "kernel_ms_per_step": kernel_ms,
                    "spread": (max(per_step) - min(per_step)) / t_med, "reported": "median block"},
        "roofline": {"bound": "valu_lds_issue_latency", "contract_bound": "hbm",
                     "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                     "traffic": traffic, "traffic_unit": "bytes/launch (PMC FETCH_SIZE + WRITE_SIZE at batch 65536, calibrated on a known-byte-count kernel "
                                                         "with the tick's own access pattern: x1.905 / x0.964)",
                     "traffic_static_from_profile": "profiles/" + TRAFFIC_PROFILE,
                     "kernel": engine.path(), "kernel_ms": k_med, "kernel_ms_mean_all_blocks": float(np.mean(kernel_ms)),
                     "algorithmic_bytes_per_tick": ALGO_BYTES_PER_TICK, "streamed_bytes_per_tick": ACTUAL_BYTES_PER_TICK,
                     "issue_frac": None if not issue else max(issue["valu_busy"], issue["lds_busy"]),
                     "fp64_tflops_nominal_n26": ALGO_FLOP_PER_TICK * B / (k_med * 1e-3) / 1e12,
                     "fp64_frac_nominal_n26": ALGO_FLOP_PER_TICK * B / (k_med * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                     "fp64_frac_solved_problem": REDUCED_FLOP_PER_TICK * B / (k_med * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                     "issue": issue,
                     "note": "tiny-dense LDS-resident fp64 work: bound by VALU/LDS issue and dependent-chain latency at 2 waves/SIMD (four instances per wave); neither HBM "
                             "nor MFMA is approachable (SURVEY.md §8d). achieved/peak/frac are the HBM figures the contract asks for; "
                             "issue_frac = max(VALU busy, LDS busy) of the committed PMC profile"},
        "solver": {"optimal_frac": float((status == 0).mean()), "iters_mean": float(iters.mean()),
                   "iters_p95": float(np.percentile(iters, 95)), "iters_max": int(iters.max())},
    }
    return line, res


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, res):
    """--dump-outputs: the arrays a caller of the timed path receives from its last step, as <out_dir>/<name>.npy in float64. If they
    would exceed DUMP_MAX_BYTES, the same fixed, seeded sample of instances is taken from every array and its indices go to sample_index.npy."""
    os.makedirs(out_dir, exist_ok=True)
    arrs = {k: np.asarray(v, dtype=np.float64) for k, v in sorted(res.items())}
    B = next(iter(arrs.values())).shape[0]
    per_inst = sum(a[:1].nbytes for a in arrs.values())
    n = B if per_inst * B <= DUMP_MAX_BYTES else DUMP_MAX_BYTES // (per_inst + 8)    # + 8: the sample's index
    if n < B:
        idx = np.sort(np.random.default_rng(0).choice(B, size=n, replace=False))
        arrs = {k: a[idx] for k, a in arrs.items()}
        arrs["sample_index"] = idx.astype(np.float64)
    for k, a in arrs.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.ascontiguousarray(a))


def make_inputs(engine, B, seed, stress):
    import wbc_workload

    class FK:   # inputs are placed on the robot with the engine's own FK
        def __call__(self, q):
            return engine.fk(q)
    return wbc_workload.make_tick_inputs(engine.model, engine.cfg, B, seed=seed, fk=FK(), stress=stress)


def cpu_baseline_and_accuracy(line, engine, host_in, res, args):
    """rank 0, N = 1 only: the oracle on this host's cores over rank 0's WHOLE batch (repeated for ~10 s), its single-thread rate on a
    sample, and the accuracy / status gate over every instance of the batch."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle   # checker / yardstick only
    model, cfg, B = engine.model, engine.cfg, host_in["q"].shape[0]
    cores = len(os.sched_getaffinity(0))
    n = min(B, args.cpu_sample) if args.cpu_sample else B
    sub = {k: v[:n] for k, v in host_in.items()}
    oracle.tick([model], [cfg], {k: v[:4096] for k, v in host_in.items()}, DT, min(4096, B), nthreads=cores, want_q_next=False)   # thread pool up
    # the box may expose more hardware threads than the job's CPU share: one pass per candidate thread count, the fastest one is timed
    sweep = {}
    for nt in sorted({cores, max(1, cores // 2), max(1, cores // 4), max(1, cores // 8), min(cores, 16)}):
        t1 = time.perf_counter()
        oracle.tick([model], [cfg], sub, DT, n, nthreads=nt, want_q_next=False)
        sweep[nt] = n / (time.perf_counter() - t1)
    visible, cores = cores, max(sweep, key=sweep.get)
    reps, t_cpu, ref, best = 0, 0.0, None, 0.0
    while t_cpu < 10.0 and reps < 256:
        t1 = time.perf_counter()
        ref = oracle.tick([model], [cfg], sub, DT, n, nthreads=cores, want_q_next=False)
        dt_ = time.perf_counter() - t1
        t_cpu += dt_
        best = max(best, n / dt_)
        reps += 1
    n1 = min(4096, B)
    t1 = time.perf_counter()
    oracle.tick([model], [cfg], {k: v[:n1] for k, v in host_in.items()}, DT, n1, nthreads=1, want_q_next=False)
    one = n1 / (time.perf_counter() - t1)
    rate = n * reps / t_cpu
    line["cpu_baseline"] = {"value": rate, "unit": "ticks/s", "cores": cores, "kind": "port",
                            "sample": "rank 0's first %d of %d instances x %d passes (%.1f s), OpenMP over %d threads (one oracle call per pass, "
                                      "no per-instance heap traffic); single-thread rate %.0f ticks/s on %d instances; reference design rate "
                                      "500 ticks/s (paced, not measured)" % (n, B, reps, t_cpu, cores, one, n1),
                            "single_thread": one, "best_pass": best, "parallel_efficiency": rate / (one * cores),
                            "threads_visible": visible, "thread_sweep_ticks_per_s": {str(k): v for k, v in sweep.items()}}
    got_q, got_s = res["qdot"][:n], res["status"][:n]
    ok = (ref["status"] == 0) & (got_s == 0)
    e_inst = np.abs(ref["qdot"] - got_q).max(axis=1)[ok] if ok.any() else np.array([float("nan")])
    err = float(e_inst.max())
    agree = float((ref["status"] == got_s).mean())
    pct = {name: float(np.percentile(e_inst, q)) for name, q in (("p50", 50), ("p99", 99), ("p99_9", 99.9))}
    line["accuracy"] = {"qdot_max_abs_err_vs_cpu": err, "qdot_err_percentiles": dict(pct, max=err), "status_agree_frac": agree,
                        "tolerance": QDOT_TOL, "instances": int(n), "instances_compared": int(ok.sum()),
                        "refine_steps": getattr(engine, "options", {}).get("refine"),
                        "pass": bool(err < QDOT_TOL and agree == 1.0)}
    return line["accuracy"]["pass"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps in all")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=1, help="timed blocks the --steps steps are split into; the median block is reported")
    ap.add_argument("--batch", type=int, default=65536, help="instances per GPU")
    ap.add_argument("--cpu-sample", type=int, default=0, help="instances for the CPU baseline and the accuracy gate (0 = the whole batch)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--jtj-mfma", type=int, default=-1, help="-1 auto (library default), 0 vector units, 1 matrix cores (general kernel)")
    ap.add_argument("--rollout-ticks", type=int, default=10, help="closed-loop ticks of the extra wbc_rollout measurement (0 = skip)")
    ap.add_argument("--posture", default="PREV", choices=["PREV", "HYBRID", "MANI"],
                    help="posture mode of the tick (default PREV = the BASELINE workload; HYBRID is what sim3.py:145 sets)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (rank 0) as DIR/<name>.npy in float64")
    args = ap.parse_args(argv)

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:     # plain `python bench.py --gpus N`: be the launcher
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:] if argv is None else list(argv)))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: the launcher's world size and --gpus must agree" % (args.gpus, world))
    stub = os.environ.get("WBC_BENCH_ENGINE_STUB")           # tests only ("file.py:Class"): CPU ranks over gloo, the line says so in config.engine
    if stub:
        import importlib.util
        path, cls = stub.rsplit(":", 1)
        spec = importlib.util.spec_from_file_location("bench_engine_stub", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        engine = getattr(mod, cls)(args, local)
        comm = Comm("gloo", rank, world, None)
    else:
        # one rank per GPU. WBC_BENCH_SHARE_GPU=1 (rehearsals on a box with fewer GPUs than ranks): rank r uses device r mod the device count and
        # the collectives run over gloo — RCCL refuses two ranks on one device; the line then says "backend": "gloo"
        share = os.environ.get("WBC_BENCH_SHARE_GPU") == "1"
        if share:
            import torch
            local = local % max(1, torch.cuda.device_count())
        engine = GpuEngine(args, local)
        comm = Comm("gloo" if share else "nccl", rank, world, None if share else engine.dev)
        engine.backend = "gloo (ranks share GPUs: rehearsal)" if share else "nccl (RCCL)"
    line, res = run_rank(args, comm, engine, make_inputs)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, res)
    ok = True
    if rank == 0:
        if args.rollout_ticks > 0 and world == 1:     # closed loop, extra leg of single-GPU runs
            what = "wbc_rollout: wbc_tick + wbc_update_state (FK + trunkWorldPos) + prev-target state advance, targets moving 0.1 mm/tick"
            line["closed_loop"] = dict(engine.closed_loop(make_inputs(engine, args.batch, seed=rank, stress=True), args.rollout_ticks),
                                       unit="closed-loop ticks/s per GPU", ticks=args.rollout_ticks, what=what,
                                       inputs="C3 stress recipe (25 % of the trunks start at / just outside their box edge: those QPs turn "
                                              "infeasible within a few ticks and the instance holds still — see worst_status_histogram)")
            line["closed_loop_unstressed"] = dict(engine.closed_loop(make_inputs(engine, args.batch, seed=rank, stress=False), args.rollout_ticks),
                                                  unit="closed-loop ticks/s per GPU", ticks=args.rollout_ticks,
                                                  inputs="same distribution without the stress recipe")
        if args.rollout_ticks > 0 and world == 1:
            line["configs"] = engine.other_configs(check=not args.no_cpu_baseline)
        if not args.no_cpu_baseline and world == 1:   # reported baseline: rank 0 at N = 1 only
            ok = cpu_baseline_and_accuracy(line, engine, engine.host_in, res, args)
        print(json.dumps(line), flush=True)
    comm.close()
    engine.close()
    if not ok:
        raise SystemExit("bench.py: accuracy gate failed (see \"accuracy\" in the line above)")
    if rank == 0 and line is not None:
        for name, c in (line.get("configs") or {}).items():      # the context configurations' own gate (their numbers are quoted too)
            a = c.get("accuracy", {})
            if a.get("gated") and (a["status_agree_frac"] != 1.0 or (a["qdot_max_abs_err_vs_cpu"] is not None and not a["qdot_max_abs_err_vs_cpu"] < QDOT_TOL)):
                raise SystemExit("bench.py: context configuration %s fails its accuracy gate: %s" % (name, a))


def launch_ranks(n, argv, timeout_s=None):
    """`python bench.py --gpus N` without a launcher: start N fresh interpreters of this file, one per GPU, with the
    environment torch.distributed.run would give them (RANK, LOCAL_RANK, WORLD_SIZE, MASTER_ADDR = 127.0.0.1, a free
    MASTER_PORT), wait for all of them, and return the worst exit code. Rank 0's JSON line is forwarded to stdout (the job's
    line); everything else the ranks print goes to stderr. This process never imports torch nor touches a GPU and never execs: the
    children are ordinary child processes. If one rank dies the others (who would wait at the next barrier for ever) are
    terminated by their exact PIDs."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0)))
    # rank 0's stdout is filtered: only its JSON line reaches ours (communication libraries print banners there), the rest goes to stderr
    import threading

    def pump(p):
        for ln in p.stdout:
            (sys.stdout if ln.lstrip().startswith("{") else sys.stderr).write(ln)
            sys.stdout.flush()
    th = threading.Thread(target=pump, args=(procs[0],), daemon=True)
    th.start()
    t0, worst = time.time(), 0
    alive = list(procs)
    while alive:
        time.sleep(0.2)
        for p in list(alive):
            rc = p.poll()
            if rc is None:
                continue
            alive.remove(p)
            if rc != 0:
                worst = worst or (rc if rc > 0 else 1)
        failed = worst != 0 or (timeout_s is not None and time.time() - t0 > timeout_s)
        if failed and alive:
            time.sleep(5.0)                                  # let the others fail by themselves first (their own message is better)
            for p in alive:
                if p.poll() is None:
                    p.terminate()
            for p in alive:
                try:
                    p.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
            worst = worst or 1
            alive = []
    th.join(timeout=10)
    return worst


if __name__ == "__main__":
    main()
