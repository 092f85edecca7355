"""Shared by test_slack_host.py and test_gpu_slack.py: the slack restatement scattered over a mixed batch, the oracle's closed loop with the
configuration kept per tick (common.tracks_reference's loop written afresh, with or without tracks, RUNNING or WARMUP), the watch recipes
and the conditions under which tick and code comparisons mean something."""
import functools

import numpy as np

import common
import oracle
import wbc_capi as capi
import wbc_model
import wbc_workload

DT = 0.002
TIE = 1e-9           # two values closer than this (and not equal) may legitimately be ordered either way by two roundings of the same loop
NEAR_ZERO = 1e-6     # the trace tolerance: a per-tick slack closer to zero than this may change sign between the two loops
FAMILIES = ("com", "trunk_z", "trunk_ang", "joint")
NCODE = 2 * capi.MAX_NV


@functools.lru_cache(maxsize=None)
def model(name):
    return wbc_model.load_model(name)


def two_smallest_gap(v, axis):
    """difference of the two smallest entries along `axis` (inf with fewer than two)"""
    v = np.moveaxis(np.asarray(v, dtype=np.float64), axis, -1)
    if v.shape[-1] < 2:
        return np.full(v.shape[:-1], np.inf)
    s = np.sort(v, axis=-1)
    with np.errstate(invalid="ignore"):
        return np.where(s[..., 1] == s[..., 0], 0.0, s[..., 1] - s[..., 0])


def reference_slack(models, cfgs, q, box, mid):
    """wbc_workload.state_slack per model on the oracle's FK, scattered by model_id: dict(slack [B, 4], which [B, 4], components [B, 12],
    gap [B, 4]: the distance between the family's two smallest components, bycode [B, 4, NCODE]: the component of each code, +inf where the
    family has none of that code)"""
    q = np.asarray(q)
    B = q.shape[0]
    out = dict(slack=np.zeros((B, 4)), which=np.zeros((B, 4), np.int32), components=np.zeros((B, 12)), gap=np.zeros((B, 4)),
               bycode=np.full((B, 4, NCODE), np.inf))
    for i, (m, c) in enumerate(zip(models, cfgs)):
        sel = np.ones(B, bool) if mid is None else (np.asarray(mid) == i)
        if not sel.any():
            continue
        r = wbc_workload.state_slack(m, c, q[sel], None if box is None else box[sel], common.OracleFK([m]))
        for k in ("slack", "which", "components"):
            out[k][sel] = r[k]
        comp = r["components"]
        rows = np.nonzero(sel)[0]
        for f, (lo, hi) in enumerate(((0, 4), (4, 6), (6, 12))):
            out["bycode"][rows, f, :hi - lo] = comp[:, lo:hi]
        out["bycode"][rows[:, None], 3, r["joint_codes"][None, :]] = r["joint_components"]
        out["gap"][sel] = np.stack([two_smallest_gap(comp[:, 0:4], 1), two_smallest_gap(comp[:, 4:6], 1), two_smallest_gap(comp[:, 6:12], 1),
                                    two_smallest_gap(r["joint_components"], 1)], axis=1)
    return out


def mixed_inputs(names, cfg_name, B, seeds, stress=True):
    """tick inputs of a batch whose instance b is model b % len(names): model i's rows drawn with seeds[i]"""
    models = [model(n) for n in names]
    cfgs = [common.config(cfg_name, m) for m in models]
    parts = [common.tick_inputs(m, c, B, seed=s, stress=stress) for m, c, s in zip(models, cfgs, seeds)]
    d = {k: v.copy() for k, v in parts[0].items()}
    mid = None
    if len(models) > 1:
        mid = (np.arange(B) % len(models)).astype(np.int32)
        for i in range(1, len(parts)):
            for k in d:
                d[k][mid == i] = parts[i][k][mid == i]
        d["model_id"] = mid
    return models, cfgs, d, mid


# ---- the watch recipes (GPU test 3): mixed a1_wx200 + a1_px100, stressed inputs of seeds 5 / 6, the gripper target stepping (3, 0, -1) mm per
# tick where no track moves it. name -> (configuration, tracks: None / "grip" / "base", running)
GRIP_STEP = (0.003, 0.0, -0.001)
WATCH_CASES = {
    "sim3": ("c3", None, True),
    "sim3_grip_track_warmup": ("c3", "grip", False),
    "trunk_task_tracks": ("c3_trunk_task", "base", True),
    "trunk_task_warmup": ("c3_trunk_task", None, False),
    "everything": ("everything", None, True),
    "everything_tracks_warmup": ("everything", "base", False),
}


@functools.lru_cache(maxsize=None)
def watch_problem(name, B=67, K=12):
    cfg_name, kind, running = WATCH_CASES[name]
    models, cfgs, d, mid = mixed_inputs(("a1_wx200", "a1_px100_pin_ver"), cfg_name, B, (5, 6), stress=True)
    tracks, step = None, None
    if kind is None:
        step = np.zeros((B, 5, 3))
        step[:, common.GRIP] = GRIP_STEP
    else:
        pos = common.track_frames(models, d["q"], mid)
        tracks = common.base_tracks(d, pos[:, common.GRIP], 5)
        if kind == "grip":
            tracks = tracks[1:]
        common.start_previous_targets(d, tracks)
    imu = d["q"][:, 3:7].copy() if running else None
    return dict(models=models, cfgs=cfgs, d=d, mid=mid, tracks=tracks, step=step, B=B, K=K, imu=imu, running=running)


@functools.lru_cache(maxsize=None)
def watch_reference(name, B=67, K=12, dt=DT):
    """The oracle's closed loop of the named recipe with the configuration kept per tick: dict(q [K, B, 27] after each tick's update,
    tick_status [K, B], status, trace [K, 4, B] and which [K, 4, B] (the restatement at q[k]), gap [K, 4, B] (two smallest components), bycode
    [K, 4, B, NCODE] (every component by its code)).
    Computed once, read-only."""
    from scipy.spatial.transform import Rotation as R
    p = watch_problem(name, B, K)
    models, cfgs, mid = p["models"], p["cfgs"], p["mid"]
    d = {k: np.array(v, copy=True) for k, v in p["d"].items()}
    assert "ee_ref_rot" not in d
    qs, tick_status = np.zeros((K, B, capi.Q_STRIDE)), np.zeros((K, B), np.int32)
    trace, which, gap = np.zeros((K, 4, B)), np.zeros((K, 4, B), np.int32), np.zeros((K, 4, B))
    bycode = np.zeros((K, 4, B, NCODE))
    for k in range(K):
        for t in p["tracks"] or ():
            if common.track_index(t["target"]) == common.TRUNK:
                d["trunk_target"] = common.track_at(t, k)
            else:
                d["ee_target"][:, common.track_index(t["target"])] = common.track_at(t, k)
        out = oracle.tick(models, cfgs, d, dt, B, nthreads=8, want_q_next=True)
        tick_status[k] = out["status"]
        d["q"] = oracle.update_state(models, d["q"], out["q_next"], d["ee_target"], p["imu"], mid) if p["running"] else out["q_next"]
        qs[k] = d["q"]
        r = reference_slack(models, cfgs, d["q"], d["trunk_box_center"], mid)
        trace[k], which[k], gap[k] = r["slack"].T, r["which"].T, r["gap"].T
        bycode[k] = np.swapaxes(r["bycode"], 0, 1)
        for i, c in enumerate(cfgs):                                    # the reference-state side effects of qpb()
            sel = slice(None) if mid is None else (mid == i)
            for e in range(capi.NEE):
                if c.task_ee[e]:
                    d["prev_ee_target"][sel, e] = d["ee_target"][sel, e]
            if c.task_trunk:
                d["prev_trunk_target"][sel] = d["trunk_target"][sel]
                d["trunk_prev_rot"][sel] = R.from_euler("xyz", d["trunk_ref_euler"][sel]).as_matrix().reshape(-1, 9)
        if p["step"] is not None:
            d["ee_target"] = d["ee_target"] + p["step"]
    ref = dict(q=qs, tick_status=tick_status, status=tick_status.max(axis=0), trace=trace, which=which, gap=gap, bycode=bycode)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def comparable(ref):
    """Where the device's tick, code and counts must equal the oracle's, [4, B] each. tick and which: the oracle's two smallest per-tick values
    are more than TIE apart or exactly equal; counts: no per-tick |slack| below NEAR_ZERO."""
    tr = ref["trace"]
    g = two_smallest_gap(tr, 0)
    tick_ok = (g > TIE) | (g == 0.0)
    counts_ok = (np.abs(tr) >= NEAR_ZERO).all(axis=0)
    return dict(tick=tick_ok, which=tick_ok, counts=counts_ok, near_tie=(g > 0.0) & (g <= TIE), exact_tie=g == 0.0)
