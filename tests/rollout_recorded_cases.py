"""Shared by tools/make_rollout_golden.py and test_gpu_rollout_recorded.py: the inputs and the sequence of roll-out calls whose outputs
tests/golden/rollout_recorded.npz holds. a1_wx200 under c3, max_batch = 12 and B = 9 (workspace strides differ from output
strides; two full packed waves and a short one), every case on ONE handle in the order of CASES, so that what an earlier case left in the
handle's workspaces is part of what is held. Only WbcBatch's public methods are used."""
import numpy as np

import common
import wbc_model
from wbc_batch import WbcBatch

MODEL, CONFIG, MAX_BATCH, B, DT = "a1_wx200", "c3", 12, 9, 0.002
K, HOLD, K_TRAJ, GROUP, BAD = 3, 2, 4, 3, 4            # ticks + hold ticks of the plain call, ticks of the trajectory calls, group size, the bad row
STATS = ("last_traj_bad_rows", "last_path", "last_update_packed")
# case -> the recorded case whose bits it must give (itself: recorded under its own name)
CASES = {"plain": "plain", "warm": "warm", "task_params": "task_params", "traj_trace": "traj_trace", "traj": "traj", "tracks": "tracks",
         "tracks_trunk_step": "tracks_trunk_step", "watch_tracks": "watch_tracks", "watch_plain": "watch_plain",
         "nowatch_plain": "plain", "nowatch_tracks": "tracks", "plain_again": "plain"}
FOOT, OTHER_FOOT = 0, 1                                  # the followed foot, the scored one that nothing follows


def make_inputs():
    """-> dict of numpy arrays: the tick inputs ("d_*"), the same with prev_* of the followed targets at the first milestones ("t_*"), and
    every other argument of the calls. Made once by the tool and stored with the outputs: the oracle FK's last bit depends on the host libm."""
    model = wbc_model.load_model(MODEL)
    cfg = common.config(CONFIG, model)
    d = common.tick_inputs(model, cfg, B, seed=5, stress=True)
    rng = np.random.default_rng(19)
    z = {"d_" + k: np.asarray(v) for k, v in d.items()}
    step = np.zeros((B, 5, 3))
    step[:, common.GRIP] = (0.003, 0.0, -0.001)
    z["ee_step"], z["trunk_step"], z["imu"] = step, np.tile((0.0005, 0.0, -0.0005), (B, 1)), d["q"][:, 3:7].copy()
    gain = np.tile(np.ctypeslib.as_array(cfg.ee_gain).reshape(1, 5, 6), (B, 1, 1)) * rng.uniform(0.5, 1.5, (B, 1, 1))
    z["task_params"] = wbc_model.task_params(cfg, B, ee_gain=gain, joint_w=cfg.joint_w * rng.uniform(0.5, 2.0, B))
    pos = common.track_frames([model], d["q"], None)
    # wbc_rollout_traj: S = 3, du >= 0.4 so that tick 3 is past the second milestone wherever an instance has three; row BAD holds a NaN
    pts = pos[:, None, common.GRIP] + rng.normal(0, 0.01, (B, 3, 3))
    pts[:, 0] = pos[:, common.GRIP]
    pts[BAD, 1, 0] = np.nan
    z["traj_points"], z["traj_n"], z["traj_du"] = pts, np.array([3, 2, 3, 3, 3, 2, 3, 3, 2], np.int32), rng.choice([0.4, 0.5, 0.7], B)
    # wbc_rollout_tracks: common.base_tracks' trunk (HERMITE) and gripper (LINEAR, the same bad row) tracks and a foot track with per-instance du
    dt = {k: v.copy() for k, v in d.items()}
    trunk, grip = common.base_tracks(dt, pos[:, common.GRIP], 5)
    grip["points"][BAD, 1, 0] = np.nan
    fp = pos[:, None, FOOT] + rng.normal(0, 0.002, (B, 3, 3))
    fp[:, 0] = pos[:, FOOT]
    foot = dict(target=FOOT, points=fp, kind="linear", n_points=np.full(B, 3, np.int32), du=rng.choice([1 / 8, 0.3, 0.6], B))
    common.start_previous_targets(dt, [trunk, grip, foot])
    z.update({"t_" + k: np.asarray(v) for k, v in dt.items()})
    for name, t in (("grip", grip), ("trunk", trunk), ("foot", foot)):
        for k in ("points", "n_points", "du"):
            z["%s_%s" % (name, k)] = np.asarray(t[k])
    return z


def handle():
    model = wbc_model.load_model(MODEL)
    bt = WbcBatch(model, MAX_BATCH)
    bt.configure(common.config(CONFIG, model))
    return bt


def run_cases(bt, z, conv=lambda a: a):
    """Yields (case, outputs as numpy arrays, the STATS after the call) in the order of CASES. conv: what every input array goes through (the
    identity: numpy, the library stages them; to a torch device tensor: the pointers pass through)."""
    a = {k: conv(np.ascontiguousarray(z[k])) for k in z}
    d = {k[2:]: v for k, v in a.items() if k.startswith("d_")}
    dt = {k[2:]: v for k, v in a.items() if k.startswith("t_")}
    track = lambda name, target, kind: dict(target=target, kind=kind, **{k: a["%s_%s" % (name, k)] for k in ("points", "n_points", "du")})  # noqa: E731
    grip, trunk, foot = track("grip", common.GRIP, "linear"), track("trunk", "trunk", "hermite"), track("foot", FOOT, "linear")
    score = (common.GRIP, "trunk", OTHER_FOOT)
    plain = dict(ee_target_step=a["ee_step"], trunk_target_step=a["trunk_step"], imu=a["imu"], want_trace=True, hold_ticks=HOLD)
    traj = dict(points=a["traj_points"], n_points=a["traj_n"], du=a["traj_du"], group_size=GROUP, imu=a["imu"])
    tracks = dict(score=score, group_size=GROUP, want_trace=True, imu=a["imu"])

    def warm():
        bt.set_option("warm_start", 1)
        try:
            return bt.rollout(d, DT, K, **plain)
        finally:
            bt.set_option("warm_start", 0)
    calls = {
        "plain": lambda: bt.rollout(d, DT, K, **plain),
        "warm": warm,
        "task_params": lambda: bt.rollout(d, DT, K, task_params=a["task_params"], **plain),
        "traj_trace": lambda: bt.rollout_traj(d, DT, K_TRAJ, want_trace=True, **traj),
        "traj": lambda: bt.rollout_traj(d, DT, K_TRAJ, want_trace=False, **traj),          # the gripper row comes from the workspace
        "tracks": lambda: bt.rollout_tracks(dt, DT, K_TRAJ, [grip, trunk, foot], **tracks),
        "tracks_trunk_step": lambda: bt.rollout_tracks(dt, DT, K_TRAJ, [grip, foot], trunk_target_step=a["trunk_step"], **tracks),
        "watch_tracks": lambda: bt.rollout_watch(dt, DT, K_TRAJ, tracks=[grip, trunk, foot], **tracks),
        "watch_plain": lambda: bt.rollout_watch(d, DT, K, tracks=None, group_size=GROUP, **plain),
        "nowatch_plain": lambda: bt.rollout_watch(d, DT, K, watch=(), tracks=None, **plain),
        "nowatch_tracks": lambda: bt.rollout_watch(dt, DT, K_TRAJ, watch=(), tracks=[grip, trunk, foot], **tracks),
        "plain_again": lambda: bt.rollout(d, DT, K, **plain),
    }
    assert list(calls) == list(CASES)
    for case, call in calls.items():
        got = call()
        stats = np.array([bt.stat(s) for s in STATS], np.int64)
        yield case, {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in got.items()}, stats


# ---------------------------------------------------------------------------------------------- wbc_state_slack, rotated placements
# No case above launches wbc_slack_kernel<ROT> (a1_wx200 has no rotated joint placement). One stand-alone wbc_state_slack on laikago_vx300 at
# B = 5: one full four-instance wave and one with three padding rows. Its arrays are "b5__*" in the same file.
B5, B5_MODEL, B5_CONFIG = 5, "laikago_vx300", "everything"


def b5_inputs():
    """-> dict(q [5, 27], box [5, 4]); made once by the tool and stored with the outputs, as make_inputs'"""
    model = wbc_model.load_model(B5_MODEL)
    d = common.tick_inputs(model, common.config(B5_CONFIG, model), B5, seed=11)
    return dict(q=np.ascontiguousarray(d["q"]), box=np.ascontiguousarray(d["trunk_box_center"]))


def run_b5(z, conv=lambda a: a):
    """-> wbc_state_slack's outputs (slack, which, components) as numpy arrays, on a handle of its own"""
    model = wbc_model.load_model(B5_MODEL)
    bt = WbcBatch(model, MAX_BATCH)
    bt.configure(common.config(B5_CONFIG, model))
    try:
        o = bt.state_slack(conv(np.ascontiguousarray(z["q"])), conv(np.ascontiguousarray(z["box"])), want_components=True)
        return {k: (v.detach().cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in o.items()}
    finally:
        bt.close()
