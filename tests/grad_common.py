"""Shared by test_tick_grad_host.py and test_gpu_tick_grad.py: the oracle-backed fk callable of wbc_workload.tick_gradients, problems, and the
per-model restatement of a mixed batch."""
import numpy as np

import common
import oracle
import wbc_capi as capi
import wbc_workload

DT = 0.002
FIELDS = ("ee_target", "prev_ee_target", "trunk_target", "prev_trunk_target", "com_target", "com_target_vel", "posture_u")
OUTPUTS = tuple(capi.TICK_GRAD_FIELDS)


class GradFK(common.OracleFK):
    """state_slack's fk convention plus jacobians(q) -> (J [B, 6, 26] WORLD joint Jacobians, Jcom [B, 3, 26]), from the CPU oracle"""

    def jacobians(self, q):
        f = oracle.fk(self.models, q, self.model_id)
        return f["J"], f["Jcom"]


def fields_read(cfg):
    """the target arrays the configuration's task rows read"""
    out = []
    if any(cfg.task_ee[e] for e in range(capi.NEE)):
        out += ["ee_target", "prev_ee_target"]
    if cfg.task_trunk:
        out += ["trunk_target", "prev_trunk_target"]
    if cfg.task_com:
        out += ["com_target", "com_target_vel"]
    if cfg.task_joint >= capi.JOINT_MANI:
        out += ["posture_u"]
    return out


def restate(models, cfgs, mid, d, x, u, rows=None, dt=DT):
    """wbc_workload.tick_gradients for a batch of several models interleaved by model_id: each model's instances through the one-model
    restatement, scattered back. -> dict of the eight output arrays [B, ...]"""
    B = len(d["q"])
    out = {k: np.zeros((B,) + shape) for k, shape in capi.TICK_GRAD_FIELDS.items()}
    for i, (m, c) in enumerate(zip(models, cfgs)):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        if not sel.any():
            continue
        di = {k: v[sel] for k, v in d.items() if k != "model_id"}
        r = wbc_workload.tick_gradients(m, c, di, x[sel], u[sel], dt, GradFK([m]), None if rows is None else rows[sel])
        for k in out:
            out[k][sel] = r[k]
    return out


def task_space_v(models, cfgs, mid, d, rng):
    """v = dL/dqdot [B, 26] of a loss on TASK-SPACE velocities: sum over the configuration's Cartesian blocks of J_block' e with e ~ N(0, 1)
    per row (unweighted rows, from the oracle's kinematics). Why not a random v: on the sim3 switch set the posture rows (d = joint_w / nv ~
    4e-5) are all that holds most of the 26 directions, so a v with a component there gives |u| ~ |v| / d^2 ~ 1e10 while J_r u stays O(1): the
    26-term products J_r . u then cancel ten digits, and the RESTATEMENT ITSELF moves by 1.3e-8 max|ref| under one ulp of noise in J (measured,
    c3, B = 7; 1.5e-7 between the device and the oracle's kinematics) — no reference there can hold anything to 1e-11. A loss that sees qdot
    through the task frames, which is what a tracking loss is, keeps u in the directions the tasks hold."""
    B = len(d["q"])
    v = np.zeros((B, capi.V_STRIDE))
    for i, (m, c) in enumerate(zip(models, cfgs)):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        if not sel.any():
            continue
        fk = GradFK([m])
        q = d["q"][sel]
        oMf = fk(q)
        J, Jcom = fk.jacobians(q)
        blocks = [wbc_workload.frame_rows(m, J, oMf, capi.FR_EE0 + e, world=False) for e in range(capi.NEE) if c.task_ee[e]]
        if c.task_trunk:
            blocks.append(wbc_workload.frame_rows(m, J, oMf, capi.FR_TRUNK, world=True))
        if c.task_com:
            blocks.append(Jcom)
        rows = np.concatenate(blocks, axis=1)
        v[sel] = np.einsum("brk,br->bk", rows, rng.normal(0, 1.0, rows.shape[:2]))
    return v
