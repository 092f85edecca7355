"""Rotated joint placements on the packed kernels. Laikago + ViperX-300 (test_gpu_laikago.py) is declined by the packed plans for reasons
unrelated to its rotations, so this file puts the ViperX-300's rotations on a1_wx200: the elbow and wrist_rotate placed with
rpy "3.14 0 0" / "-3.14 0 0", plus an arbitrary rotation on the (prismatic) left finger. The oracle composes any placement, and the plans
see the same structure as a1_wx200's, so every packed kernel's ROT instantiation runs: sim3 (cold, warm, TRUNK, QCON), orth (equality-only and
INEQ), box, the packed state update and all three posture kernels."""
import copy
import json
import os

import numpy as np
import pytest

import common
import oracle
import wbc_model
import wbc_workload
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu
DT = 0.002
QDOT_TOL = 1e-5


def _rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
            [-sp, cp * sr, cp * cr]]


@pytest.fixture(scope="module")
def rot():
    with open(os.path.join(wbc_model.MODELS_DIR, "a1_wx200.json")) as f:
        data = copy.deepcopy(json.load(f))
    for name, rpy in (("elbow", (3.14, 0, 0)), ("wrist_rotate", (-3.14, 0, 0)), ("left_finger", (0.3, -0.2, 0.1))):
        next(j for j in data["joints"] if j["name"] == name)["placement_R"] = _rpy(*rpy)
    data["name"] = "a1_wx200_rotated"
    return wbc_model.Model(data, dict(wbc_model.A1_ROLES))


@pytest.fixture(scope="module")
def wx200():
    return wbc_model.load_model("a1_wx200")


def test_fk_parity_alone_and_mixed(rot, wx200):
    rng = np.random.default_rng(4)
    q = wbc_workload.sample_q(rot, 256, rng)
    q[:, 20:27] += rng.uniform(-0.02, 0.02, (256, 7))      # the fingers off their mocap values: the rotated prismatic joint moves
    for models, mid in (([rot], None), ([wx200, rot], (np.arange(256) % 2).astype(np.int32))):
        ref = oracle.fk(models, q, mid)
        bt = WbcBatch(models, 256)
        got = bt.fk(q) if mid is None else bt.fk(q, mid)
        for k in ("oMi", "oMf", "J", "com", "Jcom"):
            assert np.abs(got[k] - ref[k]).max() < 1e-12, k
        bt.close()


@pytest.mark.parametrize("cfg_name,B,path", [("c3", 4096, 2), ("c3_hybrid", 1024, 2), ("c3_mani", 512, 2), ("c3_trunk_task", 1024, 2),
                                             ("c2", 4096, 3), ("everything", 1024, 3), ("full", 1024, 4)])
def test_tick_parity_on_the_packed_kernels(rot, cfg_name, B, path):
    cfg = common.config(cfg_name, rot)
    d = common.tick_inputs(rot, cfg, B, seed=21, with_rot=cfg_name in ("everything", "full", "c3_trunk_task"))
    ref = oracle.tick([rot], [cfg], d, DT, B, nthreads=8)
    bt = WbcBatch(rot, B)
    bt.configure(cfg)
    bt.set_option("packed_orth", 2)
    got = bt.tick(d, DT, want_q_next=True)
    assert bt.stat("last_path") == path
    assert (got["status"] == ref["status"]).all()
    ok = ref["status"] == 0
    assert ok.mean() > 0.9
    err = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    print("rotated %s B=%d: path %d, qdot max-abs err %.3e" % (cfg_name, B, path, err))
    assert err < QDOT_TOL
    assert np.abs(got["q_next"] - ref["q_next"])[ok].max() < 1e-7
    a, ar = bt.assemble(d, DT), oracle.assemble([rot], [cfg], d, DT, B)
    for k in ("A", "b", "H", "g", "C", "Clb", "Cub", "lb", "ub"):
        assert a[k].shape == ar[k].shape, k
        if ar[k].size:                              # ("full" has no constraint rows)
            assert np.abs(a[k] - ar[k]).max() / max(1.0, np.abs(ar[k]).max()) < 1e-11, k
    bt.close()


def test_mixed_batch_on_the_packed_kernel(rot, wx200):
    B = 2048
    models = [wx200, rot]
    cfgs = [common.config("c3", m) for m in models]
    mid = (np.arange(B) % 2).astype(np.int32)
    parts = [common.tick_inputs(m, c, B, 5 + k) for k, (m, c) in enumerate(zip(models, cfgs))]
    d = {k: np.where(mid.reshape((B,) + (1,) * (parts[0][k].ndim - 1)) == 0, parts[0][k], parts[1][k]) for k in parts[0]}
    d["model_id"] = mid
    ref = oracle.tick(models, cfgs, d, DT, B, nthreads=8)
    bt = WbcBatch(models, B)
    for i, c in enumerate(cfgs):
        bt.configure(c, i)
    got = bt.tick(d, DT)
    assert bt.stat("last_path") == 2 and (got["status"] == ref["status"]).all()
    ok = ref["status"] == 0
    assert np.abs(got["qdot"] - ref["qdot"])[ok].max() < QDOT_TOL
    bt.close()


@pytest.mark.parametrize("literal", [True, False])
def test_posture_target_on_all_three_kernels(rot, literal):
    B = 255
    cfg = wbc_model.sim3_config(rot, Joint="MANI", posture_literal=literal)
    q = wbc_workload.sample_q(rot, B, np.random.default_rng(17))
    ur, qar = oracle.posture_target([rot], [cfg], q, None, nthreads=8)
    bt = WbcBatch(rot, B)
    bt.configure(cfg)
    for opt, stat in ((1, 2), (3, 1), (0, 0)):     # three instances per wavefront / a lane per point / the sequential whole-tree kernel
        bt.set_option("posture_par", opt)
        u, qa = bt.posture_target(q)
        assert bt.stat("last_posture_par") == stat
        assert np.abs(u - ur).max() < 1e-9 and (qa == qar).all(), opt
    assert np.abs(ur).max() > 1e-3
    bt.close()


def test_update_state_on_the_packed_kernel(rot, wx200):
    B = 510
    rng = np.random.default_rng(13)
    models = [wx200, rot]
    mid = (np.arange(B) % 2).astype(np.int32)
    qa = [wbc_workload.sample_q(m, B, rng) for m in models]
    qb = [wbc_workload.sample_q(m, B, rng) for m in models]
    q_cur = np.where(mid[:, None] == 0, qa[0], qa[1])
    q_next = np.where(mid[:, None] == 0, qb[0], qb[1])
    imu = rng.normal(size=(B, 4))
    imu /= np.linalg.norm(imu, axis=1, keepdims=True)
    targets = rng.normal(size=(B, 5, 3))
    bt = WbcBatch(models, B)
    for i, m in enumerate(models):
        bt.configure(common.config("c3", m), i)
    ref = oracle.update_state(models, q_cur, q_next, targets, imu, mid)
    for packed in (1, 0):
        bt.set_option("packed_update", packed)
        got = bt.update_state(q_cur, q_next, targets, imu, mid)
        assert bt.stat("last_update_packed") == packed
        assert np.abs(got - ref).max() < 1e-13
    bt.close()


@pytest.mark.parametrize("cfg_name,path", [("c3", 2), ("c3_mani", 2), ("full", 4)])
def test_rollout_warm_and_cold(rot, cfg_name, path):
    B, K = 192, 8
    cfg = common.config(cfg_name, rot)
    d = common.tick_inputs(rot, cfg, B, seed=37, with_rot=cfg_name == "full")
    rng = np.random.default_rng(2)
    step = np.zeros((B, 5, 3))
    step[:, 4] = rng.normal(0, 1e-4, (B, 3))
    imu = d["q"][:, 3:7].copy()
    ref = oracle.rollout([rot], [cfg], d, DT, B, K, ee_target_step=step, imu=imu, nthreads=8)
    ok = ref["status"] == 0
    assert ok.mean() > 0.8
    bt = WbcBatch(rot, B)
    bt.configure(cfg)
    for warm in (1, 0):                                  # WARM instantiations (hot-started working sets) and cold ones
        bt.set_option("warm_start", warm)
        got = bt.rollout(d, DT, K, ee_target_step=step, imu=imu)
        assert bt.stat("last_path") == path and bt.stat("last_update_packed") == 1, warm
        assert (got["status"] == ref["status"]).all(), warm
        assert np.abs(got["q"] - ref["q"])[ok].max() < 1e-6, warm
        assert np.abs(got["qdot"] - ref["qdot"])[ok].max() < 10 * QDOT_TOL, warm
    bt.close()


def test_warmup_on_the_packed_box_kernel(rot, wx200):
    B = 8
    models = [wx200, rot]
    mid = (np.arange(B) % 2).astype(np.int32)
    q0 = np.zeros((B, 27))
    for b in range(B):
        q0[b] = models[mid[b]].neutral()
    q0[:, 2] = 0.4
    ref = oracle.warmup(models, q0, DT, 50, foot_radius=0.02, model_id=mid, nthreads=8)
    bt = WbcBatch(models, B)
    bt.set_option("packed_box", 2)
    got = bt.warm_up(q0, mid, DT, 50, foot_radius=0.02)
    assert bt.stat("last_path") == 4 and bt.stat("last_update_packed") == 1
    assert (got["status"] == ref["status"]).all()
    assert np.abs(got["q"] - ref["q"]).max() < 1e-6
    bt.close()
