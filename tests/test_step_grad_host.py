"""CPU: the state step between two ticks as a layer. wbc_step_vjp at the boundary (header, exports, struct size, variant count) and its host
restatement wbc_workload.step_gradients, held to the oracle alone:
  formulas       the directional derivative of a random linear functional of raw q_new along random directions in q, qdot and the foot targets
                 at once, from central differences of oracle.integrate o oracle.update_state at steps h and h / 2: the oracle calibrates its
                 own truncation error
  exact zeros    the columns the header says are exactly zero
  reverse sweep  K = 3 ticks chained: step_gradients and tick_state_gradients / tick_gradients (fed wbc_workload.qp_certificate), tick by tick
                 from the last, against central differences in q_0, ee_target and the task rows of the oracle's chain

Measured (this file, CPU): formulas — |analytic - FD(h/2)| is one third of |FD(h) - FD(h/2)| in all 126 cases (the truncation error of the
difference itself), worst ratio to the tolerance 0.083. Reverse sweep, 16 of 16 kept in every case: d_q0 |analytic - FD| 2.6e-9 and 3.4e-9 on full
(seeds 3, 4; |grad| 15), 1.9e-5 and 2.0e-7 on c2 (|grad| 150, inside 4 |FD(h) - FD(h/2)|), 5.5e-9 on everything; worst ratio to the tolerance
0.14 (d_q0), 0.10 (d_ee_target), 0.34 (d_task_params). The sim3 switch set is not among the chain cases: a cotangent from the next tick's state
is no task-space direction there (grad_common.task_space_v), sens_x reaches 1e6 and the chain's gradient holds about 7 digits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gradq_common as gq
import step_common as sc
import test_gpu_task_params as tgp
import test_tick_grad_q_host as tq
import wbc_capi as capi
import wbc_model
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def test_header_declares_and_library_exports_the_step_gradient():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert re.search(r"int\s+wbc_step_vjp\s*\(\s*WbcBatch\s*\*", header) and re.search(r"int\s+wbc_step_grad_sizes\s*\(", header)
    for word in ("WbcStepGrad", "d_q", "d_qdot", "d_foot_targets", "grad_status", "last_stepvjp_variant", "HELD CONSTANT", "EXACT ZEROS",
                 "right Jacobian", "fused reverse sweep"):
        assert word in header, word
    lib = capi.load_library()
    for name in ("wbc_step_vjp", "wbc_step_grad_sizes"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    s = C.c_int32()
    assert lib.wbc_step_grad_sizes(C.byref(s)) == 0
    assert s.value == C.sizeof(capi.WbcStepGrad)
    assert lib.wbc_variant_count(b"stepvjp") == 2                        # ROT off / on
    assert "stepvjp" not in capi.VARIANT_FAMILIES


# ---- formulas
# The rounding floor: test_tick_grad_q_host.py's kinematics constant. An entry of q_new comes through the exponential (a 3 x 3 product with
# the base rotation and the quaternion from it: under 20 roundings), a chain of at most 7 placements of 5 roundings each and the estimator's
# two means and one rotation (under 10): inside K_KIN = 64 roundings of max(1, |entry|), at q (+) h and q (-) h, over 2 h.
H_STEP = 2.0 ** -12
B_STEP = 8


def _directions(models, p, seed):
    rng = np.random.default_rng(seed + 99)
    B = len(p["q"])
    dq, dx = np.zeros((B, capi.V_STRIDE)), np.zeros((B, capi.V_STRIDE))
    nv = models[0].nv
    dq[:, :nv] = rng.choice([-1.0, 1.0], (B, nv)) * rng.uniform(0.5, 1.0, (B, nv))
    dx[:, :nv] = rng.choice([-1.0, 1.0], (B, nv)) * rng.uniform(0.5, 1.0, (B, nv))
    df = rng.choice([-1.0, 1.0], (B, 5, 3)) * rng.uniform(0.5, 1.0, (B, 5, 3))
    return dq, dx, df


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("model_name", sc.MODELS)
def test_formulas_against_central_differences_of_the_oracle_step(model_name, variant):
    m = tgp._model(model_name)
    mode = sc.mode_of(variant)
    worst, lines = 0.0, []
    for dt in (0.002, 0.02):
        for it, t in enumerate(sc.LADDER):
            p = sc.step_problem([m], None, B_STEP, 100 * it + 7, dt, t, variant)
            q_new = sc.step_forward([m], None, p["q"], p["qdot"], p["foot_targets"], p["imu"], dt, mode)
            g = sc.pull_back([m], None, q_new, p["rho"])
            res = wbc_workload.step_gradients(m, p["q"], p["qdot"], p["foot_targets"], dt, g, gq.StateFK([m]), imu=p["imu"], mode=mode)
            dq, dx, df = _directions([m], p, it)
            ana = (res["d_q"] * dq).sum(axis=1) + (res["d_qdot"] * dx).sum(axis=1) + (res["d_foot_targets"] * df).sum(axis=(1, 2))

            def L(s):
                qn = sc.step_forward([m], None, gq.step([m], p["q"], s * dq), p["qdot"] + s * dx, p["foot_targets"] + s * df, p["imu"], dt, mode)
                return (p["rho"] * qn).sum(axis=1)
            fd1 = (L(H_STEP) - L(-H_STEP)) / (2 * H_STEP)
            fd2 = (L(H_STEP / 2) - L(-H_STEP / 2)) / H_STEP
            floor = tq.K_KIN * EPS * (np.abs(p["rho"]) * np.maximum(1.0, np.abs(q_new))).sum(axis=1) / (H_STEP / 2)
            tol = 4.0 * np.abs(fd1 - fd2) + floor
            err = np.abs(ana - fd2)
            worst = max(worst, (err / tol).max())
            lines.append("dt %.3g |w| dt %.0e: |analytic - FD(h/2)| up to %.2e, |FD(h) - FD(h/2)| up to %.2e, floor %.2e, |grad| %.1f" % (
                dt, t, err.max(), np.abs(fd1 - fd2).max(), floor.max(), np.abs(fd2).max()))
            assert (err <= tol).all(), "%s / %s: %s; analytic %s, FD %s, tolerance %s" % (model_name, variant, lines[-1], ana, fd2, tol)
            assert np.abs(ana).min() > 0
    print("%s / %s: %d cases x %d instances, worst |analytic - FD(h/2)| / tolerance %.3f" % (model_name, variant, len(lines), B_STEP, worst))
    print("\n".join("  " + ln for ln in lines))


@pytest.mark.parametrize("model_name", sc.MODELS)
def test_exact_zeros(model_name):
    m = tgp._model(model_name)
    for variant in sc.VARIANTS:
        mode = sc.mode_of(variant)
        p = sc.step_problem([m], None, B_STEP, 5, 0.002, 3e-2, variant)
        g = np.random.default_rng(3).normal(0, 1.0, (B_STEP, capi.V_STRIDE))                 # columns >= nv of g are ignored
        r = wbc_workload.step_gradients(m, p["q"], p["qdot"], p["foot_targets"], 0.002, g, gq.StateFK([m]), imu=p["imu"], mode=mode)
        assert (r["d_q"][:, m.nv:] == 0).all() and (r["d_qdot"][:, m.nv:] == 0).all()
        assert (r["d_foot_targets"][:, 4] == 0).all()
        if mode == sc.RUNNING:
            assert (r["d_q"][:, 0:3] == 0).all() and (r["d_qdot"][:, 0:3] == 0).all()
            assert np.abs(r["d_foot_targets"][:, 0:4]).min() > 0
            if variant == "running_imu":
                assert (r["d_q"][:, 3:6] == 0).all() and (r["d_qdot"][:, 3:6] == 0).all()
            else:
                assert np.abs(r["d_q"][:, 3:6]).min() > 0 and np.abs(r["d_qdot"][:, 3:6]).min() > 0
        else:
            assert (r["d_foot_targets"] == 0).all()
            assert np.abs(r["d_q"][:, 0:6]).min() > 0 and np.abs(r["d_qdot"][:, 0:6]).min() > 0
        assert np.abs(r["d_q"][:, 6:m.nv]).min() > 0 and np.abs(r["d_qdot"][:, 6:m.nv]).min() > 0


def test_raw_to_tangent_is_the_transposed_tangent_map():
    m = tgp._model("a1_wx200")
    rng = np.random.default_rng(2)
    q = wbc_workload.sample_q(m, 5, rng)
    q[:, 3:7] *= rng.uniform(0.9, 1.1, (5, 1))                           # the map is taken at q as it stands
    c = rng.normal(0, 1.0, (5, capi.Q_STRIDE))
    ref = np.einsum("bqk,bq->bk", wbc_workload.raw_tangent_map(m, q), c)
    got = wbc_workload.raw_to_tangent(q, c)
    assert np.abs(got - ref).max() <= 16 * EPS * np.abs(c).max()
    import torch
    assert np.array_equal(wbc_workload.raw_to_tangent(torch.from_numpy(q), torch.from_numpy(c)).numpy(), got)


# ---- the reverse sweep through K ticks
K_TICKS = 3
SWEEP_CASES = [("full", 3), ("full", 4), ("c2", 3), ("c2", 4), ("everything", 4)]


def sweep_setup(cfg_name, seed):
    m, cfg, d, rng, _ = tq._e2e_setup(cfg_name, "near", seed)
    rho = np.zeros((tq.E2E_B, capi.Q_STRIDE))
    rho[:, :m.nq] = rng.normal(0, 1.0, (tq.E2E_B, m.nq))
    direc = np.zeros((tq.E2E_B, capi.V_STRIDE))
    direc[:, :m.nv] = rng.choice([-1.0, 1.0], (tq.E2E_B, m.nv)) * rng.uniform(0.5, 1.0, (tq.E2E_B, m.nv))
    return m, cfg, d, rho, direc


def chain_directional(m, cfg, d, rho, K, vary, sides0, margin, kappa, ana, scale_terms, what):
    """test_tick_grad_q_host._directional for the chain: FD of rho . raw q_K along vary(step) -> inputs of tick 0 (a key "task_params" in
    them: per-instance rows of every tick), at h and h / 2. Left out
    by the existing rule applied at every tick: the active set differs at any of the four steps, or margin < 1e-6. The same tolerance, with the
    largest cond(H) over the ticks. -> (keep, ok, line)"""
    B, H = tq.E2E_B, tq.H_E2E
    vals = {}
    same = np.ones(B, dtype=bool)
    for s in (H, -H, H / 2, -H / 2):
        dv = dict(vary(s))
        states, _, sides, status = sc.chain(m, cfg, dv, K, tq.DT, rows=dv.pop("task_params", None))
        vals[s] = (rho * states[K]["q"]).sum(axis=1)
        for k in range(K):
            same &= (sides[k] == sides0[k]).all(axis=1) & (status[k] == 0)
    fd1 = (vals[H] - vals[-H]) / (2 * H)
    fd2 = (vals[H / 2] - vals[-H / 2]) / H
    keep = same & (margin >= 1e-6)
    floor = kappa * EPS * scale_terms + EPS * np.abs(rho * sc.chain(m, cfg, d, K, tq.DT)[0][K]["q"]).sum(axis=1) / (H / 2)
    tol = 4.0 * np.abs(fd1 - fd2) + floor
    err = np.abs(ana - fd2)
    line = "%s: %d of %d kept; worst |analytic - FD(h/2)| / tolerance %.3f; |analytic - FD(h/2)| up to %.3e against |FD(h) - FD(h/2)| up to %.3e, floor up to %.3e, |grad| up to %.1f" % (
        what, keep.sum(), B, (err / tol)[keep].max(), err[keep].max(), np.abs(fd1 - fd2)[keep].max(), floor[keep].max(), np.abs(fd2[keep]).max())
    return keep, (err[keep] <= tol[keep]).all(), line, err


@pytest.mark.parametrize("cfg_name,seed", SWEEP_CASES)
def test_reverse_sweep_against_central_differences_of_the_oracle_chain(cfg_name, seed):
    m, cfg, d, rho, direc = sweep_setup(cfg_name, seed)
    states, ticks, sides0, status = sc.chain(m, cfg, d, K_TICKS, tq.DT)
    assert all((s == 0).all() for s in status)                           # every tick solved
    sw = sc.reverse_sweep(m, cfg, states, rho, tq.DT)
    ana = (sw["d_q0"] * direc).sum(axis=1)
    keep, ok, line, _ = chain_directional(m, cfg, d, rho, K_TICKS, lambda s: dict(d, q=gq.step([m], d["q"], s * direc)), sides0, sw["margin"],
                                          sw["kappa"], ana, np.abs(sw["d_q0"] * direc).sum(axis=1), "%s / seed %d, K = %d, d_q0" % (cfg_name, seed, K_TICKS))
    print(line)
    assert (~keep).sum() <= tq.E2E_B // 4
    assert ok, line
    # the same sweep's gradients with respect to what the ticks' caller owns: ee_target (the estimator's d_foot_targets, the task rows, and
    # prev_ee_target from the second tick on) and the weights and gains
    B = tq.E2E_B
    rng = np.random.default_rng(seed + 77)
    dE = rng.choice([-1.0, 1.0], (B, 5, 3)) * rng.uniform(0.5, 1.0, (B, 5, 3))
    g = sw["d_ee_target"]
    keep, ok, line, _ = chain_directional(m, cfg, d, rho, K_TICKS, lambda s: dict(d, ee_target=d["ee_target"] + s * dE), sides0, sw["margin"], sw["kappa"],
                                          (g * dE).sum(axis=(1, 2)), np.abs(g * dE).sum(axis=(1, 2)), "%s / seed %d, d_ee_target" % (cfg_name, seed))
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line
    rows = wbc_model.task_params(cfg, B)
    dT = rows * rng.choice([-1.0, 1.0], rows.shape) * rng.uniform(0.5, 1.0, rows.shape)
    g = sw["d_task_params"]
    keep, ok, line, _ = chain_directional(m, cfg, d, rho, K_TICKS, lambda s: dict(d, task_params=rows + s * dT), sides0, sw["margin"], sw["kappa"],
                                          (g * dT).sum(axis=1), np.abs(g * dT).sum(axis=1), "%s / seed %d, d_task_params" % (cfg_name, seed))
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line


def test_the_switch_set_chain_is_printed_not_held_to_the_bounds_above():
    """c3, K = 1 (from the second tick on a stress instance near seed 3 goes unsolved): the cotangent from the next state is no task-space
    direction, sens_x reaches 1e6, and the gradient holds about 7 digits — 6.1e-8 at |grad| 8.9 against |FD(h) - FD(h/2)| 2.3e-9 (measured). It
    is inside `_directional`'s tolerance only because cond(H) puts that tolerance's floor at 1e-5, so nothing is asserted of it."""
    m, cfg, d, rho, direc = sweep_setup("c3", 3)
    states, ticks, sides0, status = sc.chain(m, cfg, d, 1, tq.DT)
    sw = sc.reverse_sweep(m, cfg, states, rho, tq.DT)
    ana = (sw["d_q0"] * direc).sum(axis=1)
    keep, ok, line, _ = chain_directional(m, cfg, d, rho, 1, lambda s: dict(d, q=gq.step([m], d["q"], s * direc)), sides0, sw["margin"], sw["kappa"], ana,
                                          np.abs(sw["d_q0"] * direc).sum(axis=1), "c3 / seed 3, K = 1, d_q0 (printed, not asserted)")
    print(line)
    assert np.isfinite(sw["d_q0"]).all()
