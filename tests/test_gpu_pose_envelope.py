"""Ticks far from the nominal stance with the trunk box's angle rows active.

wbc_workload.sample_q keeps the base within 5 cm and 0.1 rad of the origin and every tick batch centres the trunk box on the robot's own
angles: no q̇ comparison could see the Euler angles a tick kernel computes, and no kernel ever left the first quadrant of an atan2, the trace
branch of the quaternion read-out or a 0.1 rad rotation of a leg block. Here the base is +-3 m out at attitudes up to pi - 0.2 rad with both
quaternion signs (common.far_q) and each trunk angle sits at the edge of its box (common.edge_trunk_box), where a 1e-6 rad error moves q̇ past
QDOT_TOL on the oracle (test_pose_envelope_host.py holds that condition without a GPU). FK is held to the 50-digit reference
(tests/kin_reference.py), everything else to the oracle at the tolerances of the existing parity tests — none is new."""
import functools

import numpy as np
import pytest

import common
import oracle
import pose_cases as pc
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT, QDOT_TOL, B0 = pc.DT, pc.QDOT_TOL, pc.B0
BAR_EXP = 3              # test_gpu_sim3p_cold_paths.py: option presolve_tol_exp of the tail recipe


def relerr(a, b):
    if a.size == 0:
        return 0.0
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def stops_at_a_device_fault(test):
    """a failed HIP call is a device fault: the session ends there, nothing more is started on that device (test_gpu_device_inplace.run_modes)"""
    @functools.wraps(test)
    def run(*args, **kw):
        try:
            return test(*args, **kw)
        except RuntimeError as e:
            hip = getattr(e, "code", None) == capi.E_HIP if isinstance(e, capi.WbcError) else ("HIP error" in str(e) or "illegal memory access" in str(e))
            if hip:
                pytest.exit("device fault in %s: %s" % (test.__name__, e), returncode=3)
            raise
    return run


def _handle(models, cfgs, B, opts=None):
    bt = WbcBatch(list(models), B)
    for i, c in enumerate(cfgs or ()):
        bt.configure(c, i)
    for k, v in (opts or {}).items():
        bt.set_option(k, v)
    return bt


def _assert_row(bt, case, flags=None):
    """the statistics name the kernel family and the row of its variant table the case is meant for"""
    if case["row"] is None:
        assert bt.stat("last_path") == case["path"], bt.stat("last_path")
        return
    family, row = case["row"]
    row = row if flags is None else flags
    assert bt.stat("last_path") == pc.LAST_PATH[family], (family, bt.stat("last_path"))
    got = bt.stat("last_tick_variant")
    assert got == pc.key_of(row), "%s: last_tick_variant = %s, want %s" % (family, capi.variant_args(got), row)


def _check(got, p, tol, what):
    """status on every instance; q̇ on the instances the oracle solves; q_next twice: against the oracle's, and against oracle.integrate fed the
    device's own q̇ (that one separates the integrate branch from the solver's error: 1e-13, test_integrate_parity)"""
    ref = p["ref"]
    ok = ref["status"] == 0
    assert (got["status"] == ref["status"]).all(), (what, np.flatnonzero(got["status"] != ref["status"]))
    err = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    e_next = np.abs(got["q_next"] - ref["q_next"])[ok].max()
    own = oracle.integrate(p["models"], p["q_int"], got["qdot"], DT, p["mid"])
    e_own = np.abs(got["q_next"] - own).max()
    print("%s: qdot max-abs err vs oracle %.3e (tolerance %.0e), q_next %.3e, q_next vs integrate(own qdot) %.3e, optimal %d/%d" % (
        what, err, tol, e_next, e_own, int(ok.sum()), len(ok)))
    assert err < tol, (what, err)
    assert e_next < 1e-7, (what, e_next)
    assert e_own < 1e-13, (what, e_own)
    assert (got["qdot"][~ok] == 0).all(), what
    return ok


# ------------------------------------------------------------------------------------------------ 1. FK against the 50-digit reference
@pytest.mark.parametrize("name", pc.FK_MODELS + ("mixed",))
@stops_at_a_device_fault
def test_fk_on_full_range_far_poses_against_the_50_digit_reference(name):
    """wbc_fk_jacobians on far_fk_q poses, every model alone and wx200 + px100 mixed, against tests/kin_reference.py (not the oracle)"""
    if name == "mixed":
        parts = [pc.fk_problem(n) for n in ("wx200", "px100")]
        models = [x[0] for x in parts]
        mid = (np.arange(pc.FK_POSES) % 2).astype(np.int32)
        q = np.where(mid[:, None] == 0, parts[0][1], parts[1][1])
        nj, nf = max(m.njoints for m in models), max(m.blob.nframes for m in models)
        ref = {}
        for k in pc.KIN_KEYS:
            a, b = (pc.pad(x[2][k], nj if k == "oMi" else nf) if k in ("oMi", "oMf") else x[2][k] for x in parts)
            ref[k] = np.where(mid.reshape((-1,) + (1,) * (a.ndim - 1)) == 0, a, b)
    else:
        m, q, ref = pc.fk_problem(name)
        models, mid = [m], None
    bt = _handle(models, None, pc.FK_POSES)
    try:
        got = bt.fk(q, mid)
        for k in pc.KIN_KEYS:
            assert got[k].shape == ref[k].shape, (name, k)
            e = np.abs(got[k] - ref[k]).max()
            print("%s: %s worst error against the reference %.2e" % (name, k, e))
            assert e < pc.kin_tol(ref[k]), (name, k, e)
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 2. assemble
@pytest.mark.parametrize("cfg_name,with_rot", [("c3", False), ("everything", True), ("full", True)])
@stops_at_a_device_fault
def test_assemble_on_far_poses_with_edge_angles(cfg_name, with_rot):
    """the general kernel's own Euler extraction, visible in Clb / Cub; `everything` on the full attitudes (nothing is solved here)"""
    m = pc.model("wx200")
    cfg = common.config(cfg_name, m)
    d = common.far_tick_inputs(m, cfg, B0, pc.SEED, with_rot=with_rot)
    ref = oracle.assemble([m], [cfg], d, DT, B0)
    bt = _handle([m], [cfg], B0)
    try:
        got = bt.assemble(d, DT)
        for k in ("A", "b", "H", "g", "C", "Clb", "Cub", "lb", "ub"):
            assert got[k].shape == ref[k].shape, k
            assert relerr(got[k], ref[k]) < 1e-11, (k, relerr(got[k], ref[k]))
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 3. ticks, one per code path
def _tick(bt, p, d=None, **kw):
    return bt.tick(p["d"] if d is None else d, DT, want_q_next=True, task_params=p["rows"], **kw)


@pytest.mark.parametrize("name", list(pc.TICK_CASES))
@stops_at_a_device_fault
def test_tick_on_far_poses_with_edge_angles(name):
    case = pc.TICK_CASES[name]
    p = pc.tick_problem(name)
    bt = _handle(p["models"], p["cfgs"], B0, case["opts"])
    try:
        got = _tick(bt, p)
        _assert_row(bt, case)
        ok = _check(got, p, case["tol"], name)
        assert ok.mean() >= 0.9
        if p["mid"] is not None:
            assert (got["qdot"][p["mid"] == 1, 25] == 0).all()       # px100: the padded DoF
    finally:
        bt.close()


def _seeds(bt, p):
    """working sets of a perturbed solve (test_warm_started_tick_reaches_the_cold_optimum: the same robots a moment earlier, targets 0.3 mm back)"""
    prev = dict(p["d"], ee_target=p["d"]["ee_target"] - 3e-4)
    return bt.tick(prev, DT, want_working_set=True, task_params=p["rows"])["working_set"]


@pytest.mark.parametrize("name,flags", [("c3", (1, 0, 0, 0, 0)), ("everything_orthp", (1, 1, 0, 0))])
@stops_at_a_device_fault
def test_warm_tick_on_far_poses_reaches_the_cold_answer(name, flags):
    """the WARM row of the packed sim3 kernel and of the packed orth kernel's INEQ variant on the same inputs, held to the cold oracle answer"""
    case = pc.TICK_CASES[name]
    p = pc.tick_problem(name)
    bt = _handle(p["models"], p["cfgs"], B0, case["opts"])
    try:
        seeds = _seeds(bt, p)
        got = _tick(bt, p, dict(p["d"], working_set=seeds), want_working_set=True)
        _assert_row(bt, case, flags)
        ok = _check(got, p, QDOT_TOL, name + " WARM")
        assert (got["working_set"][~ok] == 0).all()
    finally:
        bt.close()


@stops_at_a_device_fault
def test_sim3p_tail_on_far_poses():
    """presolve_tol_exp = 3 with dbg_force_defer (test_forced_defer_takes_the_tail_and_counts): the world-frame contact rows of a base 3 m out
    have nearly parallel thigh and calf columns, so most stance-leg blocks are flagged and their waves' tails redo them on the general path"""
    case = pc.TICK_CASES["c3"]
    p = pc.tick_problem("c3")
    ratio = pc.leg_block_ratio(oracle.assemble(p["models"], p["cfgs"], p["d"], DT, B0))
    bar = 10.0 ** -BAR_EXP
    bt = _handle(p["models"], p["cfgs"], B0, {"presolve_tol_exp": BAR_EXP, "dbg_force_defer": 1})
    try:
        got = _tick(bt, p)
        _assert_row(bt, case)
        deferred = bt.stat("deferred_last")
        print("tail: %d instances deferred, %d flagged clear of the bar, %d near it" % (deferred, (ratio < 0.5 * bar).sum(), (ratio < 2 * bar).sum()))
        assert 1 <= (ratio < 0.5 * bar).sum() <= deferred <= (ratio < 2.0 * bar).sum()
        _check(got, p, QDOT_TOL, "c3 tail")
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 4. the CoM box at full attitudes
@stops_at_a_device_fault
def test_infeasible_com_box_at_full_attitudes():
    """`everything` on the full far_q attitudes: lower > upper in the CoM box under yaw or tilt. Status identical on every instance, q̇ = 0 and an
    empty working set wherever the status is not 0."""
    case = pc.INFEASIBLE_CASE
    p = pc.tick_problem("everything_far")
    bad = p["ref"]["status"] != 0
    assert bad.mean() > 0.5
    bt = _handle(p["models"], p["cfgs"], B0, case["opts"])
    try:
        got = _tick(bt, p, want_working_set=True)
        assert bt.stat("last_path") == pc.LAST_PATH["orthp"]
        assert (got["status"] == p["ref"]["status"]).all(), np.flatnonzero(got["status"] != p["ref"]["status"])
        assert (got["qdot"][bad] == 0).all() and (got["working_set"][bad] == 0).all()
        if (~bad).any():
            assert np.abs(got["qdot"] - p["ref"]["qdot"])[~bad].max() < QDOT_TOL
        own = oracle.integrate(p["models"], p["q_int"], got["qdot"], DT)
        assert np.abs(got["q_next"] - own).max() < 1e-13
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 5. closed loop
@functools.lru_cache(maxsize=None)
def _rollout_problem(name, narrow):
    return pc.build_problem(dict(pc.TICK_CASES[name], narrow=narrow))


# The reference's base estimator (trunkWorldPos, Robot_Wrapper4.py:1297-1327) rotates the mean foot offset by the trunk's attitude once more than
# the geometry asks for. Near the nominal stance that is a few millimetres; at the full far_q attitudes the first state update moves the base by up
# to 0.64 m, out of the trunk's z box, and from the second tick on the oracle finds two thirds of the instances infeasible (edge angles or not,
# IMU or not: checked on the CPU). So the run that must stay solved draws its attitudes from common.NARROW — translation, quaternion flips and
# edge angles as everywhere — and the full attitudes run as a batch of mixed fates: every tolerance on the third that stays solved.
@pytest.mark.parametrize("name,narrow,solved", [("c3", True, 0.8), ("c3", False, 0.25), ("everything_orthp", True, 0.8)])
@stops_at_a_device_fault
def test_rollout_from_far_poses(name, narrow, solved):
    """wbc_rollout, 6 ticks with the IMU on, held to oracle.rollout as test_rollout_parity does"""
    K = 6
    case = pc.TICK_CASES[name]
    p = _rollout_problem(name, narrow)
    m, cfg, d = p["models"][0], p["cfgs"][0], p["d"]
    rng = np.random.default_rng(2)
    step = np.zeros((B0, 5, 3))
    step[:, 4] = rng.normal(0, 1e-4, (B0, 3))
    tstep = rng.normal(0, 5e-5, (B0, 3))
    imu = d["q"][:, 3:7].copy()
    ref = oracle.rollout([m], [cfg], d, DT, B0, K, ee_target_step=step, trunk_target_step=tstep, imu=imu, nthreads=8)
    ok = ref["status"] == 0
    assert ok.mean() > solved and (narrow or (~ok).mean() > 0.25)
    bt = _handle([m], [cfg], B0, case["opts"])
    try:
        got = bt.rollout(d, DT, K, ee_target_step=step, trunk_target_step=tstep, imu=imu)
        assert bt.stat("last_path") == pc.LAST_PATH[case["row"][0]]
        if name == "c3":
            assert bt.stat("last_update_packed") == 1                 # (test_rollout_parity: the packed state update beside the packed sim3 kernel)
        assert (got["status"] == ref["status"]).all()
        eq, ev = np.abs(got["q"] - ref["q"])[ok].max(), np.abs(got["qdot"] - ref["qdot"])[ok].max()
        print("%s roll-out (%s attitudes): q max-abs err %.3e, qdot %.3e, optimal %d/%d" % (name, "narrowed" if narrow else "full", eq, ev, int(ok.sum()), B0))
        assert eq < 1e-6
        assert ev < 10 * QDOT_TOL
        assert np.abs(got["ee_target"] - ref["ee_target"]).max() < 1e-15
        assert np.abs(got["grip_trace"] - ref["grip_trace"])[:, ok].max() < 1e-6
        assert (got["q"][:, 3:7] == imu).all()
        assert (got["iters"][ok] - ref["iters"][ok]).__abs__().max() <= 2 * K
    finally:
        bt.close()


@stops_at_a_device_fault
def test_update_state_on_far_pose_pairs():
    """wbc_update_state between two far_q draws, both kernels, at test_update_state_parity's tolerances"""
    models = [pc.model("wx200"), pc.model("px100")]
    rng = np.random.default_rng(13)
    mid = (np.arange(B0) % 2).astype(np.int32)
    qa, qb = ([common.far_q(m, B0, rng) for m in models] for _ in range(2))
    q_cur = np.where(mid[:, None] == 0, qa[0], qa[1])
    q_next = np.where(mid[:, None] == 0, qb[0], qb[1])
    imu = common.far_q(models[0], B0, rng)[:, 3:7]
    targets = q_cur[:, None, 0:3] + rng.normal(size=(B0, 5, 3)) * 0.3
    bt = _handle(models, [common.config("c3", m) for m in models], B0)
    try:
        for packed in (1, 0):
            bt.set_option("packed_update", packed)
            for im in (imu, None):
                ref = oracle.update_state(models, q_cur, q_next, targets, im, mid)
                got = bt.update_state(q_cur, q_next, targets, im, mid)
                assert bt.stat("last_update_packed") == packed
                assert np.abs(got - ref).max() < 1e-13
                assert (got[:, 3:] == ref[:, 3:]).all()
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 6. posture target
@pytest.mark.parametrize("mode", ["HYBRID", "MANI"])
@stops_at_a_device_fault
def test_posture_target_on_far_poses(mode):
    """qpJointb MANI / HYBRID to the letter on far_q, the three posture kernels, at test_posture_target_parity's tolerances"""
    models = [pc.model("wx200"), pc.model("px100")]
    cfgs = [wbc_model.sim3_config(m, Joint=mode, posture_literal=True) for m in models]
    rng = np.random.default_rng(17)
    mid = (np.arange(B0) % 2).astype(np.int32)
    qs = [common.far_q(m, B0, rng) for m in models]
    q = np.where(mid[:, None] == 0, qs[0], qs[1])
    ur, qar = oracle.posture_target(models, cfgs, q, mid, nthreads=8)
    assert np.abs(ur).max() > 1e-3
    bt = _handle(models, cfgs, B0)
    try:
        for option, kernel in ((None, 2), (3, 1), (0, 0)):       # three instances per wavefront; one, every point on a lane; the sequential kernel
            if option is not None:
                bt.set_option("posture_par", option)
            u, qa = bt.posture_target(q, mid)
            assert bt.stat("last_posture_par") == kernel
            print("%s, posture kernel %d: u max-abs err vs oracle %.3e" % (mode, kernel, np.abs(u - ur).max()))
            assert np.abs(u - ur).max() < 1e-9
            assert (qa == qar).all()
    finally:
        bt.close()
