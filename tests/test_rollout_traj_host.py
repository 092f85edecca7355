"""Roll-outs along per-instance milestone trajectories (wbc_rollout_traj) on the host: the C-ABI binding, the numpy restatement of
the target evaluation against klampt's piecewise-linear Trajectory.eval (Robot_Wrapper4._LinearTrajectory), and the front end's
shape checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wbc_batch
import wbc_capi as capi
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_ctypes_binds_the_entry_point():
    lib = capi.load_library()
    assert "wbc_rollout_traj" in capi.SIGNATURES and hasattr(lib, "wbc_rollout_traj")
    assert lib.wbc_rollout_traj.argtypes == capi.SIGNATURES["wbc_rollout_traj"][1]
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert re.search(r"\bwbc_rollout_traj\s*\(", header)
    assert int(re.search(r"#define WBC_MAX_TRAJ_POINTS (\d+)", header).group(1)) == capi.MAX_TRAJ_POINTS


def test_struct_layouts_follow_the_header():
    """field order of the two structs as the header declares them; LP64 offsets"""
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    for name, cls in (("WbcTrajectory", capi.WbcTrajectory), ("WbcRolloutSummary", capi.WbcRolloutSummary)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)\s*;", body)
        assert names == [f for f, _ in cls._fields_], name
    assert C.sizeof(capi.WbcTrajectory) == 40 and capi.WbcTrajectory.du_all.offset == 32
    assert C.sizeof(capi.WbcRolloutSummary) == 6 * 8 + 8 + 4 * 8 and capi.WbcRolloutSummary.group_rms.offset == 56


def _klampt(points, n_points, du, k):
    from Robot_Wrapper4 import _LinearTrajectory
    return np.array([_LinearTrajectory(points[b, :n_points[b]]).eval(k * du[b]) for b in range(len(points))])


def test_traj_targets_is_klampt_piecewise_linear_bit_for_bit():
    rng = np.random.default_rng(11)
    B, S = 64, 6
    points = rng.normal(0, 0.3, (B, S, 3))
    n = rng.integers(2, S + 1, B).astype(np.int32)
    du = rng.choice([0.002, 1 / 8, 1 / 5, 0.3, 1.0, 2.5], B)       # 0.3: knots fall between ticks; 1.0: on them; 2.5: over them
    for b in range(B):
        points[b, n[b]:] = np.nan                                   # rows beyond an instance's own milestones are never read
    seen_inner = seen_last = False
    for k in list(range(0, 30)) + [499, 10 ** 6]:
        got = wbc_workload.traj_targets(points, n, du, k)
        ref = _klampt(points, n, du, k)
        assert got.shape == (B, 3) and np.isfinite(got).all()
        assert (got == ref).all(), k
        t = k * du
        seen_inner |= bool(((t > 0) & (t < n - 1) & (t != np.floor(t))).any())
        seen_last |= bool((t >= n - 1).any())
    assert seen_inner and seen_last
    assert (wbc_workload.traj_targets(points, n, du, 0) == points[:, 0]).all()                       # clamped ends
    assert (wbc_workload.traj_targets(points, n, du, 10 ** 6) == points[np.arange(B), n - 1]).all()
    # n_points None = every row full; du a single number
    full = rng.normal(0, 0.3, (5, 3, 3))
    for k in (0, 1, 7, 400, 999, 1000, 1001):
        assert (wbc_workload.traj_targets(full, None, 0.002, k) == _klampt(full, [3] * 5, [0.002] * 5, k)).all()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the host checks" % name)


def _front_end(max_batch=8):
    bt = object.__new__(wbc_batch.WbcBatch)           # no handle: the checks under test run before any library call
    bt.lib, bt.max_batch, bt.device_id, bt._h, bt._mh = _NoLibrary(), max_batch, 0, None, []
    return bt


def test_rollout_traj_checks_shapes_before_any_library_call():
    bt = _front_end()
    B = 4
    d = dict(q=np.zeros((B, 27)), ee_target=np.zeros((B, 5, 3)), prev_ee_target=np.zeros((B, 5, 3)))
    pts = np.zeros((B, 3, 3))
    bad_calls = [
        dict(points=np.zeros((B, 3, 2))), dict(points=np.zeros((B + 1, 3, 3))), dict(points=np.zeros((B, 9))),
        dict(points=np.zeros((B, 1, 3))), dict(points=np.zeros((B, capi.MAX_TRAJ_POINTS + 1, 3))),
        dict(points=pts, n_points=np.zeros(B + 1, np.int32)), dict(points=pts, n_points=np.zeros((B, 2), np.int32)),
        dict(points=pts, du=np.full(B - 1, 0.002)), dict(points=pts, du=np.full((B, 2), 0.002)),
        dict(points=pts, ee_index=5), dict(points=pts, ee_index=-1),
        dict(points=pts, group_size=3), dict(points=pts, group_size=-1),
        dict(points=pts, trunk_target_step=np.zeros((B, 4))), dict(points=pts, imu=np.zeros((B, 3))),
        dict(points=pts, task_params=np.zeros((B, 84))),
    ]
    for kw in bad_calls:
        with pytest.raises(capi.WbcError):
            bt.rollout_traj(d, 0.002, 5, **kw)
    with pytest.raises(capi.WbcError):
        bt.rollout_traj(d, 0.002, 0, points=pts)
    with pytest.raises(capi.WbcError):
        bt.rollout_traj(dict(d, q=np.zeros((B, 26))), 0.002, 5, points=pts)
    with pytest.raises(AssertionError, match="wbc_rollout_traj"):     # a well-formed call is the first to reach the library
        bt.rollout_traj(d, 0.002, 5, points=pts, n_points=np.full(B, 3, np.int32), du=np.full(B, 0.002), group_size=2)
