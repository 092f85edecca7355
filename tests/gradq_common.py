"""Shared by test_tick_grad_q_host.py and test_gpu_tick_grad_q.py: the oracle-backed fk callable of wbc_workload.tick_state_gradients, the
tangent step, and the per-model restatement of a mixed batch."""
import numpy as np

import grad_common as gc
import oracle
import wbc_capi as capi
import wbc_workload

DT = gc.DT


class StateFK(gc.GradFK):
    """GradFK plus joints(q) -> oMi [B, njoints, 12], the joint placements, from the CPU oracle"""

    def joints(self, q):
        return oracle.fk(self.models, q, self.model_id, want_com=False)["oMi"]


def step(models, q, delta, mid=None):
    """q (+) delta = pin.integrate(q, delta): oracle.integrate with dt = 1"""
    return oracle.integrate(models, q, delta, 1.0, mid)


def restate(models, cfgs, mid, d, cert, rows=None, working_set=None, dt=DT):
    """wbc_workload.tick_state_gradients for a batch of several models interleaved by model_id -> dict(d_q [B, 26], d_trunk_box_center [B, 4]);
    cert: dict(qdot, sens_x, sens_bounds, sens_rows, y_rows)"""
    B = len(d["q"])
    out = dict(d_q=np.zeros((B, capi.V_STRIDE)), d_trunk_box_center=np.zeros((B, 4)))
    for i, (m, c) in enumerate(zip(models, cfgs)):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        if not sel.any():
            continue
        di = {k: v[sel] for k, v in d.items() if k != "model_id"}
        r = wbc_workload.tick_state_gradients(m, c, di, cert["qdot"][sel], cert["sens_x"][sel], dt, StateFK([m]),
                                              sens_bounds=cert["sens_bounds"][sel], sens_rows=cert["sens_rows"][sel], y_rows=cert["y_rows"][sel],
                                              task_params=None if rows is None else rows[sel],
                                              working_set=None if working_set is None else working_set[sel])
        for k in out:
            out[k][sel] = r[k]
    return out
