"""Poses far from the nominal stance, on the CPU: the oracle's kinematics and integrate against the 50-digit reference
(tests/kin_reference.py) on full-range poses; the condition on the inputs that keeps test_gpu_pose_envelope.py honest (the oracle solves them, and
its q̇ answers to a 1e-6 rad change of a trunk angle); and the finding that made the new inputs necessary, pinned on the old ones."""
import numpy as np
import pytest

import common
import kin_reference
import oracle
import pose_cases as pc
import wbc_workload


# ------------------------------------------------------------------------------------------------ 1. the oracle against the reference
@pytest.mark.parametrize("name", pc.FK_MODELS)
def test_oracle_kinematics_match_the_50_digit_reference_on_full_range_poses(name):
    """24 far_fk_q poses (every 1-DoF joint over its whole range, all lower / all upper limits, base +-3 m at large attitudes, both quaternion
    signs): oMi, oMf, data.J, com, Jcom and the LOCAL_WORLD_ALIGNED Jacobian of every frame within 1e-12 max(1, |ref|max); trunk angles 1e-12."""
    m, q, ref = pc.fk_problem(name)
    got = oracle.fk([m], q)
    worst = {}
    for k in pc.KIN_KEYS:
        assert got[k].shape == ref[k].shape, k
        worst[k] = np.abs(got[k] - ref[k]).max()
        assert worst[k] < pc.kin_tol(ref[k]), (name, k, worst[k])
    Jf = np.array([[oracle.frame_jacobian(m, q[b], frame=f, rf=2) for f in range(m.blob.nframes)] for b in range(len(q))])
    worst["Jf"] = np.abs(Jf - ref["Jf"]).max()
    assert worst["Jf"] < pc.kin_tol(ref["Jf"]), (name, worst["Jf"])
    R_to_euler = oracle.rot_helpers()[1]
    eul = np.array([R_to_euler(got["oMf"][b, kin_reference.TRUNK, :9]) for b in range(len(q))])
    worst["euler"] = np.abs(eul - ref["euler"]).max()
    assert worst["euler"] < 1e-12, (name, worst["euler"])
    assert np.abs(ref["euler"][:, 0]).max() > np.pi / 2 and np.abs(ref["euler"][:, 2]).max() > np.pi / 2      # (the poses leave the first quadrant)
    print("%s: worst error of the oracle against the reference: %s" % (name, ", ".join("%s %.2e" % kv for kv in worst.items())))


STEPS = (1e-9, 1e-5, 1e-4 - 1e-7, 1e-4 + 1e-7, 0.6, 2.5)     # rad: either side of the oracle's series switch at 1e-4, and large steps


@pytest.mark.parametrize("name", ["wx200", "laikago"])
def test_oracle_integrate_matches_the_50_digit_reference(name):
    """M exp6(v) from far_q attitudes (tr R <= 0 in most, every non-trace quaternion branch, w < 0 in half): within 1e-13 at every step size"""
    m = pc.model(name)
    rng = np.random.default_rng(51)
    n = 16
    q = common.far_q(m, n * len(STEPS), rng)
    v = rng.normal(size=(len(q), 26)) * 0.05
    w = rng.normal(size=(len(q), 3))
    v[:, 3:6] = w / np.linalg.norm(w, axis=1, keepdims=True) * np.repeat(STEPS, n)[:, None]
    v[:, m.nv:] = 0.0
    got = oracle.integrate([m], q, v, 1.0)                      # (dt = 1: v is the tangent step itself)
    ref = np.array([kin_reference.integrate(m.data, q[b], v[b]) for b in range(len(q))])
    tr = np.array([np.trace(kin_reference.fk(m.data, x)["oMi"][1, :9].reshape(3, 3)) for x in ref[::4]])
    assert (tr <= 0).mean() > 0.5                               # the integrated attitudes take the non-trace branches
    for i, s in enumerate(STEPS):
        err = np.abs(got - ref)[i * n:(i + 1) * n].max()
        print("%s: integrate, step %.7g rad: worst error of the oracle against the reference %.2e" % (name, s, err))
        assert err < 1e-13, (name, s, err)


def test_far_q_reaches_what_sample_q_never_does():
    """the recipe's own statistics (the numbers of the issue, loosely): tr R <= 0 in most draws, the three non-trace branches about a third each,
    |yaw| and |roll| beyond pi / 2 in about half, w < 0 in half; sample_q has none of it"""
    m = pc.model("wx200")
    q = common.far_q(m, 400, np.random.default_rng(3))
    R = oracle.fk([m], q, want_com=False)["oMi"][:, 1, :9].reshape(-1, 3, 3)
    tr = np.trace(R, axis1=1, axis2=2)
    branch = np.argmax(np.diagonal(R, axis1=1, axis2=2), axis=1)[tr <= 0]
    e = wbc_workload.R_to_euler_xyz(R.reshape(-1, 9))
    assert (tr <= 0).mean() > 0.7 and all((branch == k).mean() > 0.25 for k in range(3))
    assert (np.abs(e[:, 2]) > np.pi / 2).mean() > 0.4 and (np.abs(e[:, 0]) > np.pi / 2).mean() > 0.4 and np.abs(e[:, 1]).max() <= 1.3
    assert (q[:, 6] < 0).mean() > 0.4 and np.abs(q[:, 0:2]).max() > 2.5
    assert np.abs(np.linalg.norm(q[:, 3:7], axis=1) - 1).max() < 1e-15
    qs = wbc_workload.sample_q(m, 400, np.random.default_rng(3))
    Rs = oracle.fk([m], qs, want_com=False)["oMi"][:, 1, :9].reshape(-1, 3, 3)
    assert (np.trace(Rs, axis1=1, axis2=2) > 2.9).all() and (Rs[:, 0, 0] > 0).all() and (qs[:, 6] > 0).all()


# ------------------------------------------------------------------------------------------------ 2. observability: a condition on the inputs
@pytest.mark.parametrize("name", list(pc.TICK_CASES))
def test_the_oracle_solves_the_far_cases_and_its_answer_sees_a_microradian(name):
    """For every tick case of test_gpu_pose_envelope.py, on the oracle alone: status 0 on at least 90 % of the instances, and — where the
    configuration has a trunk box — moving the three angle centres by 1e-6 rad (what an error of 1e-6 rad in a kernel's Euler angles does to the
    rows' bounds) moves q̇ by more than 1e-5 = QDOT_TOL on at least 40 % of the solved instances. A case that misses this gets another recipe
    (the range of f, the seed), never another threshold."""
    p = pc.tick_problem(name)
    solved, moved = pc.observability(p)
    print("%s: the oracle solves %.3f of the instances (working-set changes: mean %.1f, max %d); a 1e-6 rad shift moves qdot by > 1e-5 on %s" % (
        name, solved, p["ref"]["iters"].mean(), p["ref"]["iters"].max(), "n/a (no trunk box)" if moved is None else "%.3f of the solved" % moved))
    assert solved >= 0.9, (name, solved)
    if moved is not None:
        assert moved >= 0.4, (name, moved)
    q = p["d"]["q"]
    assert np.abs(q[:, 0:2]).max() > 2.0 and (q[:, 6] < 0).any() and (q[:, 6] > 0).any()


def test_the_com_box_is_infeasible_at_full_attitudes():
    """`everything` on the full far_q attitudes: the CoM box's bounds are foot positions on world axes, lower > upper under yaw or tilt — the case
    test_gpu_pose_envelope.py holds to the oracle's statuses, with q̇ = 0"""
    p = pc.tick_problem("everything_far")
    bad = p["ref"]["status"] != 0
    assert bad.mean() > 0.5 and (p["ref"]["qdot"][bad] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the gap itself, on the old inputs
def test_the_nominal_inputs_cannot_see_a_tenth_of_a_radian():
    """A property of test_tick_parity's `c3` INPUTS (seed 21, B = 4096), not of the product: every batch sets the trunk box's angle centres to the
    robot's own angles, the bounds sit at +-37 rad/s, and shifting the three centres by 0.1 rad — an error of 0.1 rad in roll, pitch or yaw —
    changes no q̇ of the oracle, bit for bit. This is why those inputs cannot stand in for the ones above."""
    m = pc.model("wx200")
    cfg = common.config("c3", m)
    d = common.tick_inputs(m, cfg, 4096, seed=21)
    ref = oracle.tick([m], [cfg], d, pc.DT, 4096, nthreads=8)
    for shift in (0.05, 0.1):
        box = d["trunk_box_center"].copy()
        box[:, 1:] += shift
        sh = oracle.tick([m], [cfg], dict(d, trunk_box_center=box), pc.DT, 4096, nthreads=8)
        assert np.array_equal(sh["qdot"], ref["qdot"]) and np.array_equal(sh["status"], ref["status"]), shift
