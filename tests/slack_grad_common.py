"""Shared by test_slack_grad_host.py and test_gpu_slack_grad.py: the displaced box (the stock inputs put trunk_box_center at the pose itself, so
all six angle components tie at trunk_box_ang), the per-model restatement of the slack cotangents on a mixed batch, the watch seeds, and the
condition under which a comparison that depends on the selected component means something (slack_common.TIE)."""
import numpy as np

import gradq_common as gq
import slack_common as sl
import wbc_capi as capi
import wbc_workload

BLOCKS = ((0, 4), (4, 6), (6, 12))      # the components of families 0..2
FULL_MASK = (1 << capi.N_SLACK) - 1


def displace_box(d, seed=11):
    """z centre x (1 +- 0.15), angles +- 0.1: families 0..2 then have their two smallest components well apart (>= 1.3e-4 on the shapes used)"""
    rng = np.random.default_rng(seed)
    B = len(d["q"])
    box = d["trunk_box_center"].copy()
    box[:, 0] *= 1.0 + rng.uniform(-0.15, 0.15, B)
    box[:, 1:] += rng.uniform(-0.1, 0.1, (B, 3))
    return dict(d, trunk_box_center=box)


def per_model(models, mid, B):
    for i, m in enumerate(models):
        sel = np.ones(B, dtype=bool) if mid is None else (np.asarray(mid) == i)
        if sel.any():
            yield i, m, sel


def restate_layer(models, cfgs, mid, q, box, g_slack=None, g_components=None):
    """wbc_workload.slack_gradients for a batch of several models interleaved by model_id -> dict(d_q, d_trunk_box_center, which, grad_status)"""
    B = len(q)
    out = dict(d_q=np.zeros((B, capi.V_STRIDE)), d_trunk_box_center=np.zeros((B, 4)), which=np.zeros((B, 4), np.int32), grad_status=np.zeros(B, np.int32))
    for i, m, sel in per_model(models, mid, B):
        r = wbc_workload.slack_gradients(m, cfgs[i], q[sel], None if box is None else box[sel], gq.StateFK([m]),
                                         None if g_slack is None else g_slack[sel], None if g_components is None else g_components[sel])
        for k in out:
            out[k][sel] = r[k]
    return out


def selection_ok(models, cfgs, mid, q, box):
    """[B, 4]: the restatement's two smallest components of the family are more than TIE apart, or exactly equal (slack_common.comparable's rule)"""
    g = sl.reference_slack(models, cfgs, q, box, mid)["gap"]
    return (g > sl.TIE) | (g == 0.0)


def watch_rows(models, cfgs, mid, q_after, box, seed):
    """wbc_workload.watch_seed_gradients on given states, per model -> (g_q_trace [K, B, 26], box term [B, 4])"""
    K, B = q_after.shape[:2]
    g, db = np.zeros((K, B, capi.V_STRIDE)), np.zeros((B, 4))
    for i, m, sel in per_model(models, mid, B):
        sub = lambda a: None if a is None else np.asarray(a)[..., sel]      # noqa: E731
        r = wbc_workload.watch_seed_gradients(m, cfgs[i], q_after[:, sel], box[sel], gq.StateFK([m]), seed["mask"], sub(seed.get("g_slack_min")),
                                              sub(seed.get("g_slack_final")), sub(seed.get("g_trace")), sub(seed.get("slack_min_tick")))
        g[:, sel], db[sel] = r["g_q_trace"], r["d_trunk_box_center"]
    return g, db


def watch_gammas(B, K, seed, n=capi.N_SLACK):
    rng = np.random.default_rng(seed)
    return dict(g_slack_min=rng.normal(0, 1.0, (n, B)), g_slack_final=rng.normal(0, 1.0, (n, B)), g_trace=rng.normal(0, 1.0, (K, n, B)))


def watch_seed_of(rec, gam, which=("g_slack_min", "g_slack_final", "g_trace"), mask=FULL_MASK):
    """the seed of a record's results (rec: rollout_record(..., watch=...)'s dict, or anything with q and slack_min_tick)"""
    s = dict(mask=mask, q_final=rec["q"], slack_min_tick=rec["slack_min_tick"] if "g_slack_min" in which else None)
    s.update({k: (gam[k] if k in which else None) for k in ("g_slack_min", "g_slack_final", "g_trace")})
    return s
