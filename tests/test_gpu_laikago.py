"""The Laikago + ViperX-300 robot (sim3.py robot_index 2) on the device, against the CPU oracle: its ViperX-300 elbow and wrist_rotate are
placed with rpy = "+-3.14 0 0", so every FK site runs its rotated-placement composition (fk_place_rot). Tolerances as test_gpu_parity.py."""
import importlib.util
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
HERE = os.path.dirname(os.path.abspath(__file__))


def relerr(a, b):
    return 0.0 if a.size == 0 else np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.fixture(scope="module")
def lk():
    return wbc_model.load_model("laikago_vx300")


@pytest.fixture(scope="module")
def wx200():
    return wbc_model.load_model("a1_wx200")


def test_fk_jacobians_com_parity(lk, wx200):
    rng = np.random.default_rng(3)
    q = wbc_workload.sample_q(lk, 300, rng)
    q[0] = lk.neutral()
    ref = oracle.fk([lk], q)
    bt = WbcBatch(lk, 512)
    got = bt.fk(q)
    for k in ("oMi", "oMf", "J", "com", "Jcom"):
        assert np.abs(got[k] - ref[k]).max() < 1e-12, k
    bt.close()
    # a mixed handle: the a1 instances and the Laikago instances side by side
    B = 64
    mid = (np.arange(B) % 2).astype(np.int32)
    qs = [wbc_workload.sample_q(m, B, rng) for m in (wx200, lk)]
    q = np.where(mid[:, None] == 0, qs[0], qs[1])
    ref = oracle.fk([wx200, lk], q, mid)
    bt = WbcBatch([wx200, lk], B)
    got = bt.fk(q, mid)
    for k in ("oMi", "oMf", "J", "com", "Jcom"):
        assert np.abs(got[k] - ref[k]).max() < 1e-12, k
    bt.close()


@pytest.mark.parametrize("cfg_name,with_rot", [("c3", False), ("c3_hybrid", False), ("c2", False), ("everything", False), ("everything", True),
                                               ("c3", True)])
def test_assemble_parity(lk, cfg_name, with_rot):
    cfg = common.config(cfg_name, lk)
    B = 200
    d = common.tick_inputs(lk, cfg, B, seed=11, with_rot=with_rot)
    ref = oracle.assemble([lk], [cfg], d, DT, B)
    bt = WbcBatch(lk, B)
    bt.configure(cfg)
    got = bt.assemble(d, DT)
    for k in ("A", "b", "H", "g", "C", "Clb", "Cub", "lb", "ub"):
        assert got[k].shape == ref[k].shape, k
        assert relerr(got[k], ref[k]) < 1e-11, (k, relerr(got[k], ref[k]))
    bt.close()


# Where the Laikago ticks run. The packed kernels' plan builders decline this model for structural reasons that have nothing to do with its
# rotated placements: with its fixed "gripper" no DoF is locked (lock_from = nv), so the reduced problem is n' = 13 (the
# packed sim3 kernel and the packed orth kernel's INEQ variant hold n' <= 12) and the two free fingers sit at tree depth 7 (the packed FK
# schedule reaches depth 6); the warm-up problem has 19 free limb DoF (the packed box kernel keeps 16 and eliminates at most 2 beyond the
# base). Those ticks run on the general kernel's ROT instantiation (path 0). The equality-only family (c2) fits the packed orth kernel.
PATHS = {"c3": 0, "c3_hybrid": 0, "c2": 3, "everything": 0, "full": 0}


def _tick(lk, cfg_name, B, seed=21, with_rot=False):
    cfg = common.config(cfg_name, lk)
    d = common.tick_inputs(lk, cfg, B, seed=seed, with_rot=with_rot)
    ref = oracle.tick([lk], [cfg], d, DT, B, nthreads=8)
    bt = WbcBatch(lk, B)
    bt.configure(cfg)
    bt.set_option("packed_orth", 2)                 # (the packed orth kernel at every batch size, not only from its default minimum)
    got = bt.tick(d, DT, want_q_next=True)
    path = bt.stat("last_path")
    assert (got["status"] == ref["status"]).all()
    ok = ref["status"] == 0
    assert ok.mean() > 0.9
    err = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    print("laikago %s B=%d: path %d, qdot max-abs err %.3e" % (cfg_name, B, path, err))
    assert err < QDOT_TOL
    assert np.abs(got["q_next"] - ref["q_next"])[ok].max() < 1e-7
    bt.close()
    return path


@pytest.mark.parametrize("B", [1, 1024, 65536])
def test_sim3_tick_parity(lk, B):
    path = _tick(lk, "c3", B)
    if B >= 1024:
        assert path == PATHS["c3"]


@pytest.mark.parametrize("cfg_name", ["c3_hybrid", "c2", "everything", "full"])
def test_tick_parity_other_paths(lk, cfg_name):
    assert _tick(lk, cfg_name, 1024, with_rot=cfg_name in ("everything", "full")) == PATHS[cfg_name]


@pytest.mark.parametrize("literal", [True, False])
def test_posture_target_parity(lk, wx200, literal):
    B = 256
    models = [wx200, lk]
    cfgs = [wbc_model.sim3_config(m, Joint="HYBRID", posture_literal=literal) for m in models]
    rng = np.random.default_rng(17)
    mid = (np.arange(B) % 2).astype(np.int32)
    qs = [wbc_workload.sample_q(m, B, rng) for m in models]
    q = np.where(mid[:, None] == 0, qs[0], qs[1])
    ur, qar = oracle.posture_target(models, cfgs, q, mid, nthreads=8)
    bt = WbcBatch(models, B)
    for i, c in enumerate(cfgs):
        bt.configure(c, i)
    for opt in (1, 3, 0):                 # default (posture_par kernels) / a lane per point / the sequential whole-tree kernel
        bt.set_option("posture_par", opt)
        u, qa = bt.posture_target(q, mid)
        assert (bt.stat("last_posture_par") >= 1) if opt else (bt.stat("last_posture_par") == 0)
        assert np.abs(u - ur).max() < 1e-9
        assert (qa == qar).all()
    bt.close()


def test_update_state_parity(lk, wx200):
    B = 510
    rng = np.random.default_rng(13)
    models = [wx200, lk]
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
    got = bt.update_state(q_cur, q_next, targets, imu, mid)
    assert bt.stat("last_update_packed") == 0       # (the packed update follows the packed sim3 plan, which declines Laikago: see PATHS)
    assert np.abs(got - ref).max() < 1e-13
    bt.set_option("packed_update", 0)
    assert (bt.update_state(q_cur, q_next, targets, imu, mid) == got).all()
    bt.close()


def test_rollout_parity(lk):
    B, K = 192, 10
    cfg = common.config("c3", lk)
    d = common.tick_inputs(lk, cfg, B, seed=37)
    rng = np.random.default_rng(2)
    step = np.zeros((B, 5, 3))
    step[:, 4] = rng.normal(0, 1e-4, (B, 3))
    imu = d["q"][:, 3:7].copy()
    ref = oracle.rollout([lk], [cfg], d, DT, B, K, ee_target_step=step, imu=imu, nthreads=8)
    bt = WbcBatch(lk, B)
    bt.configure(cfg)
    got = bt.rollout(d, DT, K, ee_target_step=step, imu=imu)
    assert bt.stat("last_path") == PATHS["c3"] and bt.stat("last_update_packed") == 0
    ok = ref["status"] == 0
    assert ok.mean() > 0.8 and (got["status"] == ref["status"]).all()
    assert np.abs(got["q"] - ref["q"])[ok].max() < 1e-6
    assert np.abs(got["qdot"] - ref["qdot"])[ok].max() < 10 * QDOT_TOL
    bt.close()


def test_warmup_alone_and_mixed(lk, wx200):
    for models in ([lk], [wx200, lk]):
        B = 8
        mid = (np.arange(B) % len(models)).astype(np.int32)
        q0 = np.zeros((B, 27))
        for b in range(B):
            q0[b] = models[mid[b]].neutral()
        q0[:, 2] = 0.4
        ref = oracle.warmup(models, q0, DT, 50, foot_radius=0.0, model_id=mid, nthreads=8)
        bt = WbcBatch(models, B)
        bt.set_option("packed_box", 2)
        got = bt.warm_up(q0, mid, DT, 50, foot_radius=0.0)
        assert bt.stat("last_path") == PATHS["full"] and bt.stat("last_update_packed") == 0
        assert (got["status"] == ref["status"]).all()
        assert np.abs(got["q"] - ref["q"]).max() < 1e-6
        bt.close()


def test_exact_rational_optimum(lk):
    cfg = common.config("c3", lk)
    B = 4
    d = common.tick_inputs(lk, cfg, B, seed=5)
    a = oracle.assemble([lk], [cfg], d, DT, B)
    bt = WbcBatch(lk, B)
    bt.configure(cfg)
    got = bt.tick(d, DT)
    for b in range(B):
        if got["status"][b] != 0:
            continue
        n = lk.nv
        x = got["qdot"][b, :n]
        xe = common.exact_ls_optimum(a["A"][b][:, :n], a["b"][b], a["C"][b][:, :n], a["lb"][b][:n], a["ub"][b][:n], a["Clb"][b], a["Cub"][b], x)
        assert np.abs(x - np.asarray(xe, dtype=float)).max() < QDOT_TOL
    bt.close()


def test_robot_model_runs_sim3_laikago():
    """RobotModel for laikago_vx300.urdf as sim3.py builds it for robot_index 2 (foot_offset False, HYBRID posture), 50 runWBC ticks along
    its first milestone segment (shifted 2 cm sideways, as in test_gpu_mirrors: the exactly symmetric stance is unstable in the waist). Every
    tick's q̇ is held to the oracle's closed-loop roll-out of the same ticks from the same state (oracle.rollout, ticks 1..k)."""
    spec = importlib.util.spec_from_file_location("replay_sim3", os.path.join(os.path.dirname(HERE), "tools", "replay_sim3.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    K = 50
    rm = rp.build_robot("laikago_vx300", "HYBRID")
    assert rm.end_effector_index_list_joint[4] == 21 and rm.arm_base_id == 14 and rm.foot_radius == 0
    nv = rm._model.nv
    off = np.array([0.0, 0.02, 0.0])
    start = np.asarray(rm.prev_EE_pos[4], dtype=float).reshape(3)
    step = (np.array(rp.MILESTONES["laikago_vx300"][0]) - start) / K
    EE_target = [np.asarray(rm.prev_EE_pos[i], dtype=float).reshape(3, 1).copy() for i in range(5)]
    EE_target[4] = (start + off).reshape(3, 1)
    cfg = rm._config()
    d0 = rm._tick_inputs(EE_target, None)             # the state and reference state the first tick starts from
    imu = np.array([0.0, 0.0, 0.0, 1.0])
    qd = []
    for k in range(K):
        EE_target[4] = (start + off + k * step).reshape(3, 1)
        rm.runWBC(imu, target_cartesian_pos_EE=EE_target, target_cartesian_pos_trunk=None)
        assert rm.solver_status == 0
        qd.append(np.array(rm.q_vel[:nv], dtype=float))

    def target_at(k):
        t = d0["ee_target"].copy()
        t[0, 4] = start + off + k * step
        return t
    worst = 0.0
    for k in range(K):
        ref = oracle.rollout([rm._model], [cfg], d0, rm.step_time, 1, k + 1, imu=imu[None], ee_target_at=target_at)
        assert ref["status"][0] == 0
        worst = max(worst, float(np.abs(qd[k] - ref["qdot"][0, :nv]).max()))
    print("laikago mirror: 50 runWBC ticks, q̇ max-abs err vs the oracle roll-out %.3e" % worst)
    assert worst < QDOT_TOL
