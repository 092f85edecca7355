"""CPU: roll-out gradients in two calls. wbc_rollout_record / wbc_rollout_vjp at the boundary (header, exports, struct sizes, variant count,
tape size) and the sweep's host restatement wbc_workload.rollout_gradients:
  same sweep    on the existing chain cases it equals step_common.reverse_sweep: the same float operations in the same order, so the two are
                held to 1e-13 max(1, max|ref|) of each other
  new parts     a loss over the whole roll-out, sum_k rho_k . raw q_(k+1), with a non-zero ee_target_step: dL/d(q_0, ee_target_step,
                prev_ee_target, ee_target) against central differences of the oracle's chain at steps h and h / 2 with
                test_step_grad_host.chain_directional's tolerance (4 |FD(h) - FD(h/2)| + cond(H) eps |terms| + the loss's rounding floor) and
                its cap of at most B // 4 instances left out

Measured (this file, CPU): same sweep — worst |rollout_gradients - reverse_sweep| / max(1, max|ref|) 2.4e-16, 2.5e-16 (full, seeds 3, 4) and
4.1e-16 (everything). New parts, `full` / seed 3: 16, 14, 16 and 16 of 16 instances kept (d_q0, d_ee_target_step, d_prev_ee_target,
d_ee_target), worst |analytic - FD(h/2)| / tolerance 0.077, 0.039, 0.076, 0.049 at |analytic - FD(h/2)| <= 3.6e-9 against |FD(h) - FD(h/2)|
<= 7.5e-9; `everything` / seed 4: 16 of 16 kept in all four, |analytic - FD(h/2)| <= 2.4e-8 against |FD(h) - FD(h/2)| <= 2.2e-8 (cond(H) puts that
case's tolerance floor at order 1, as in test_step_grad_host.py: `full` is the case that bites)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gradq_common as gq
import oracle
import step_common as sc
import test_step_grad_host as th
import test_tick_grad_q_host as tq
import wbc_capi as capi
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
K = th.K_TICKS
B = tq.E2E_B
SAME_BOUND = 1e-13


def test_header_declares_and_library_exports_the_rollout_gradient():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert re.search(r"int\s+wbc_rollout_record\s*\(\s*WbcBatch\s*\*", header) and re.search(r"int\s+wbc_rollout_vjp\s*\(\s*WbcBatch\s*\*", header)
    assert re.search(r"size_t\s+wbc_rollout_tape_bytes\s*\(", header) and re.search(r"int\s+wbc_rollout_grad_sizes\s*\(", header)
    for word in ("WbcRolloutSeed", "WbcRolloutGrad", "g_q_final", "g_qdot_last", "g_q_trace", "d_q0", "d_ee_target_step", "d_trunk_target_step",
                 "ticks_dropped", "grad_status", "last_rollvjp_variant", "TARGET BOOKKEEPING", "UNSOLVED TICKS", "HELD CONSTANT", "736", "432",
                 "hold_ticks", "q_con", "posture_u", "tape_bytes"):
        assert word in header, word
    assert "a fused reverse sweep is not" not in header
    lib = capi.load_library()
    for name in ("wbc_rollout_record", "wbc_rollout_vjp", "wbc_rollout_tape_bytes", "wbc_rollout_grad_sizes"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    s, g = C.c_int32(), C.c_int32()
    assert lib.wbc_rollout_grad_sizes(C.byref(s), C.byref(g)) == 0
    assert s.value == C.sizeof(capi.WbcRolloutSeed) == 3 * C.sizeof(C.c_void_p)
    assert g.value == C.sizeof(capi.WbcRolloutGrad) == (len(capi.ROLLOUT_GRAD_FIELDS) + 2) * C.sizeof(C.c_void_p)
    assert lib.wbc_variant_count(b"rollvjp") == 3                        # the stages BEGIN, ADDV, LINK
    assert "rollvjp" not in capi.VARIANT_FAMILIES
    for b, k in ((1, 1), (7, 3), (65536, 16)):
        assert lib.wbc_rollout_tape_bytes(b, k) == b * (capi.TAPE_HEAD_BYTES + k * capi.TAPE_TICK_BYTES)
    assert lib.wbc_rollout_tape_bytes(0, 3) == 0 and lib.wbc_rollout_tape_bytes(3, 0) == 0
    assert (capi.TAPE_HEAD_BYTES, capi.TAPE_TICK_BYTES) == (8 * (45 + 9), 8 * (27 + 26 + 15 + 15 + 3 + 3) + 8 + 16)


def restate(m, cfg, states, ticks, **seeds):
    """wbc_workload.rollout_gradients over an oracle chain (step_common.chain's states and ticks)"""
    n = len(ticks)
    x = np.stack([t["qdot"] for t in ticks])
    return wbc_workload.rollout_gradients(m, cfg, states[:n], x, tq.DT, gq.StateFK([m]), lambda d: oracle.assemble([m], [cfg], d, tq.DT, len(x[0])),
                                          **seeds)


@pytest.mark.parametrize("cfg_name,seed", [("full", 3), ("full", 4), ("everything", 4)])
def test_rollout_gradients_is_the_reverse_sweep(cfg_name, seed):
    m, cfg, d, rho, direc = th.sweep_setup(cfg_name, seed)
    states, ticks, sides0, status = sc.chain(m, cfg, d, K, tq.DT)
    assert all((s == 0).all() for s in status)
    sw = sc.reverse_sweep(m, cfg, states, rho, tq.DT)
    r = restate(m, cfg, states, ticks, g_q_final=sc.pull_back([m], None, states[K]["q"], rho))
    assert (r["ticks_dropped"] == 0).all()
    worst = 0.0
    for mine, theirs in (("d_q0", "d_q0"), ("d_ee_target", "d_ee_target"), ("d_prev_ee_target", "d_prev_ee_target0"), ("d_task_params", "d_task_params")):
        ratio = np.abs(r[mine] - sw[theirs]).max() / max(1.0, np.abs(sw[theirs]).max())
        worst = max(worst, ratio)
        assert ratio <= SAME_BOUND, "%s / seed %d: %s differs from reverse_sweep's by %.3e x max(1, max|ref| = %.3e)" % (
            cfg_name, seed, mine, ratio, np.abs(sw[theirs]).max())
        assert np.abs(sw[theirs]).max() > 0
    # constant targets: a step would have moved every tick's target by k steps
    assert (r["d_trunk_target_step"] == 0).all() == (not cfg.task_trunk)
    print("%s / seed %d, K = %d: worst |rollout_gradients - reverse_sweep| / max(1, max|ref|) %.2e" % (cfg_name, seed, K, worst))


# ---- the new parts: a loss over the whole roll-out, target steps, prev_ee_target
def _trace_loss(states, rhos):
    return sum((rhos[k] * states[k + 1]["q"]).sum(axis=1) for k in range(K))


def _directional(m, cfg, d, step, rhos, vary, sides0, margin, kappa, ana, scale_terms, what):
    """test_step_grad_host.chain_directional for the loss sum_k rho_k . raw q_(k+1) and a chain with a target step: vary(s) -> (inputs of
    tick 0, ee_target_step). The same rule for leaving an instance out, the same tolerance with the loss's own rounding floor."""
    H = tq.H_E2E
    vals = {}
    same = np.ones(B, dtype=bool)
    for s in (H, -H, H / 2, -H / 2):
        dv, sv = vary(s)
        states, _, sides, status = sc.chain(m, cfg, dv, K, tq.DT, ee_target_step=sv)
        vals[s] = _trace_loss(states, rhos)
        for k in range(K):
            same &= (sides[k] == sides0[k]).all(axis=1) & (status[k] == 0)
    fd1 = (vals[H] - vals[-H]) / (2 * H)
    fd2 = (vals[H / 2] - vals[-H / 2]) / H
    keep = same & (margin >= 1e-6)
    base = sc.chain(m, cfg, d, K, tq.DT, ee_target_step=step)[0]
    floor = kappa * EPS * scale_terms + EPS * sum(np.abs(rhos[k] * base[k + 1]["q"]).sum(axis=1) for k in range(K)) / (H / 2)
    tol = 4.0 * np.abs(fd1 - fd2) + floor
    err = np.abs(ana - fd2)
    line = "%s: %d of %d kept; worst |analytic - FD(h/2)| / tolerance %.3f; |analytic - FD(h/2)| up to %.3e against |FD(h) - FD(h/2)| up to %.3e, floor up to %.3e, |grad| up to %.1f" % (
        what, keep.sum(), B, (err / tol)[keep].max(), err[keep].max(), np.abs(fd1 - fd2)[keep].max(), floor[keep].max(), np.abs(fd2[keep]).max())
    return keep, (err[keep] <= tol[keep]).all(), line


@pytest.mark.parametrize("cfg_name,seed", [("full", 3), ("everything", 4)])
def test_new_parts_against_central_differences_of_the_oracle_chain(cfg_name, seed):
    m, cfg, d, rho, direc = th.sweep_setup(cfg_name, seed)
    rng = np.random.default_rng(seed + 311)
    step = rng.normal(0, 2e-4, (B, 5, 3))
    rhos = np.zeros((K, B, capi.Q_STRIDE))
    rhos[:, :, :m.nq] = rng.normal(0, 1.0, (K, B, m.nq))
    states, ticks, sides0, status = sc.chain(m, cfg, d, K, tq.DT, ee_target_step=step)
    assert all((s == 0).all() for s in status)
    sw = sc.reverse_sweep(m, cfg, states, rho, tq.DT)                    # (its margin and cond(H): properties of the ticks, not of the loss)
    trace = np.stack([sc.pull_back([m], None, states[k + 1]["q"], rhos[k]) for k in range(K)])
    r = restate(m, cfg, states, ticks, g_q_trace=trace)
    assert (r["ticks_dropped"] == 0).all()
    what = "%s / seed %d, K = %d, loss over the trace, stepped" % (cfg_name, seed, K)
    dE = rng.choice([-1.0, 1.0], (B, 5, 3)) * rng.uniform(0.5, 1.0, (B, 5, 3))
    checks = (
        ("d_q0", (r["d_q0"] * direc).sum(axis=1), np.abs(r["d_q0"] * direc).sum(axis=1), lambda s: (dict(d, q=gq.step([m], d["q"], s * direc)), step)),
        ("d_ee_target_step", (r["d_ee_target_step"] * dE).sum(axis=(1, 2)), np.abs(r["d_ee_target_step"] * dE).sum(axis=(1, 2)),
         lambda s: (d, step + s * dE)),
        ("d_prev_ee_target", (r["d_prev_ee_target"] * dE).sum(axis=(1, 2)), np.abs(r["d_prev_ee_target"] * dE).sum(axis=(1, 2)),
         lambda s: (dict(d, prev_ee_target=d["prev_ee_target"] + s * dE), step)),
        ("d_ee_target", (r["d_ee_target"] * dE).sum(axis=(1, 2)), np.abs(r["d_ee_target"] * dE).sum(axis=(1, 2)),
         lambda s: (dict(d, ee_target=d["ee_target"] + s * dE), step)),
    )
    for name, ana, scale, vary in checks:
        keep, ok, line = _directional(m, cfg, d, step, rhos, vary, sides0, sw["margin"], sw["kappa"], ana, scale, what + ", " + name)
        print(line)
        assert (~keep).sum() <= B // 4 and ok, line
        assert np.abs(ana).max() > 0, name
