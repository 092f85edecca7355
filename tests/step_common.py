"""Shared by test_step_grad_host.py and test_gpu_step_grad.py: problems of the state step (integrate, then the estimator), the per-model
restatement of a mixed batch, the oracle's chain of K ticks with its per-tick states, and the host reverse sweep through it."""
import numpy as np

import common
import gradq_common as gq
import oracle
import test_tick_grad_q_host as tq
import wbc_capi as capi
import wbc_workload

MODELS = ["a1_wx200", "a1_px100_pin_ver", "laikago_vx300"]
LADDER = (0.0, 1e-9, 1e-5, 1e-3, 3e-2, 0.6, 3.0)         # |omega| dt of the base
VARIANTS = ("running", "running_imu", "warmup")
RUNNING, WARMUP = capi.ROLLOUT_RUNNING, capi.ROLLOUT_WARMUP


def mode_of(variant):
    return WARMUP if variant == "warmup" else RUNNING


def step_problem(models, mid, B, seed, dt, t, variant):
    """-> dict(q, qdot, foot_targets, imu (None unless variant running_imu), rho [B, 27]): states near the stance, base angular rate of
    magnitude t / dt in a random direction, a random linear functional rho of raw q_new"""
    rng = np.random.default_rng(seed)
    q, x, rho = np.zeros((B, capi.Q_STRIDE)), np.zeros((B, capi.V_STRIDE)), np.zeros((B, capi.Q_STRIDE))
    for i, m in enumerate(models):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        n = int(sel.sum())
        q[sel] = wbc_workload.sample_q(m, n, rng)
        x[sel, :m.nv] = rng.normal(0, 0.5, (n, m.nv))
        rho[sel, :m.nq] = rng.normal(0, 1.0, (n, m.nq))
    w = rng.normal(0, 1.0, (B, 3))
    x[:, 3:6] = w / np.linalg.norm(w, axis=1, keepdims=True) * (t / dt)
    ft = oracle.fk(models, q, mid, want_com=False)["oMf"][:, capi.FR_EE0:capi.FR_EE0 + 5, 9:12] + rng.normal(0, 0.02, (B, 5, 3))
    imu = None
    if variant == "running_imu":
        imu = q[:, 3:7] + rng.normal(0, 0.05, (B, 4))
        imu /= np.linalg.norm(imu, axis=1, keepdims=True)
    return dict(q=q, qdot=x, foot_targets=np.ascontiguousarray(ft), imu=imu, rho=rho)


def step_forward(models, mid, q, qdot, foot_targets, imu, dt, mode):
    """the oracle's state step: integrate, then update_state (RUNNING)"""
    qn = oracle.integrate(models, q, qdot, dt, mid)
    return oracle.update_state(models, q, qn, foot_targets, imu, mid) if mode == RUNNING else qn


def pull_back(models, mid, q_new, rho):
    """g = raw_tangent_map(q_new)' rho [B, 26]"""
    g = np.zeros((len(q_new), capi.V_STRIDE))
    for i, m in enumerate(models):
        sel = np.ones(len(q_new), dtype=bool) if mid is None else (mid == i)
        if sel.any():
            g[sel] = np.einsum("bqk,bq->bk", wbc_workload.raw_tangent_map(m, q_new[sel]), rho[sel])
    return g


def restate_step(models, mid, p, g, dt, mode):
    """wbc_workload.step_gradients for a batch of several models interleaved by model_id"""
    B = len(p["q"])
    out = {k: np.zeros((B,) + shape) for k, shape in capi.STEP_GRAD_FIELDS.items()}
    for i, m in enumerate(models):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        if not sel.any():
            continue
        r = wbc_workload.step_gradients(m, p["q"][sel], p["qdot"][sel], p["foot_targets"][sel], dt, g[sel], gq.StateFK([m]),
                                        imu=None if p["imu"] is None else p["imu"][sel], mode=mode)
        for k in out:
            out[k][sel] = r[k]
    return out


# ---- K ticks chained: tick -> integrate -> update_state -> the reference-state side effects (oracle.rollout's loop, with the per-tick states kept)
def advance(cfg, d, q_new, ee_target_step=None):
    """the inputs of the next tick"""
    from scipy.spatial.transform import Rotation as R
    n = {k: np.array(v, copy=True) for k, v in d.items()}
    n["q"] = q_new
    for e in range(capi.NEE):
        if cfg.task_ee[e]:
            n["prev_ee_target"][:, e] = d["ee_target"][:, e]
            if d.get("ee_ref_rot") is not None:
                n["ee_prev_rot"][:, e] = d["ee_ref_rot"][:, e]
    if cfg.task_trunk:
        n["prev_trunk_target"] = d["trunk_target"].copy()
        n["trunk_prev_rot"] = R.from_euler("xyz", d["trunk_ref_euler"]).as_matrix().reshape(-1, 9)
    if ee_target_step is not None:
        n["ee_target"] = d["ee_target"] + ee_target_step
    return n


def chain(m, cfg, d0, K, dt, ee_target_step=None, rows=None):
    """-> (states [K + 1] (inputs dicts; the last one's q is q_K), ticks [K] (oracle.tick's outputs), sides [K], status [K]); rows [B, 85]:
    per-instance weights and gains on every tick (the oracle's form: one (model, configuration) pair per instance)"""
    B = len(d0["q"])
    ms, cs, pid = ([m], [cfg], None) if rows is None else common.per_instance_configs([m], [cfg], None, rows)
    states, ticks, sides, status = [d0], [], [], []
    for _ in range(K):
        d = states[-1]
        di = d if pid is None else dict(d, model_id=pid)
        t = oracle.tick(ms, cs, di, dt, B, nthreads=8)
        a = oracle.assemble(ms, cs, di, dt, B)
        ticks.append(t)
        sides.append(tq._sides(a, t["qdot"]))
        status.append(t["status"])
        states.append(advance(cfg, d, oracle.update_state([m], d["q"], t["q_next"], d["ee_target"], None, None), ee_target_step))
    return states, ticks, sides, status


def reverse_sweep(m, cfg, states, rho, dt):
    """dL/d(q_0 (tangent), ee_target, task_params) of L = rho . raw q_K through the K ticks of `states` (constant targets), from the numpy
    restatements alone: step_gradients, then tick_state_gradients / tick_gradients fed wbc_workload.qp_certificate, tick by tick from the
    last. -> dict(d_q0 [B, 26], d_ee_target [B, 5, 3], d_task_params [B, 85], margin [B] (the smallest over the ticks), kappa [B] (the
    largest cond(H))). test_tick_grad_q_host._certified asserts that every tick is solved and certified."""
    K = len(states) - 1
    B = len(rho)
    g = pull_back([m], None, states[K]["q"], rho)
    d_ee, d_tp = np.zeros((B, 5, 3)), np.zeros((B, capi.TASK_PARAMS_DOUBLES))
    margin, kappa = np.full(B, np.inf), np.zeros(B)
    d_prev_next = np.zeros((B, 5, 3))                                    # dL/d prev_ee_target of the tick after this one (= this tick's ee_target)
    for k in range(K - 1, -1, -1):
        d = states[k]
        x = oracle.tick([m], [cfg], d, dt, B, nthreads=8)["qdot"]
        sg = wbc_workload.step_gradients(m, d["q"], x, d["ee_target"], dt, g, gq.StateFK([m]))
        t0, a0, cert, res, side0, mg = tq._certified(m, cfg, d, sg["d_qdot"])
        assert np.array_equal(t0["qdot"], x)
        u = np.stack([c["sens_x"] for c in cert])
        tg = wbc_workload.tick_gradients(m, cfg, d, x, u, dt, gq.StateFK([m]))
        g = sg["d_q"] + res["d_q"]
        on = np.array([bool(cfg.task_ee[e]) for e in range(capi.NEE)])[None, :, None]
        d_ee += sg["d_foot_targets"] + tg["d_ee_target"] + np.where(on, d_prev_next, 0.0)
        d_prev_next = tg["d_prev_ee_target"]
        d_tp += tg["d_task_params"]
        margin = np.minimum(margin, mg)
        kappa = np.maximum(kappa, np.linalg.cond(a0["H"][:, :m.nv, :m.nv]))
    return dict(d_q0=g, d_ee_target=d_ee, d_prev_ee_target0=d_prev_next, d_task_params=d_tp, margin=margin, kappa=kappa)
