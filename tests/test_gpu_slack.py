"""Constraint slack on the device: wbc_state_slack and wbc_rollout_watch (csrc/wbc_k_slack.hip).

The row call is held to wbc_workload.state_slack fed by the oracle's FK at 1e-12 (the project's FK parity tolerance). The watch is held to the
oracle's closed loop (slack_common.watch_reference: tick, update_state and the restatement at every tick's configuration) at 1e-6,
test_rollout_parity's trace tolerance — the closed loop is compared there, not the kernel — and, without tolerance, to the reduction of its OWN
trace (wbc_workload.watch_summary). Ticks, codes and counts are compared where the oracle's own values leave no doubt (slack_common.comparable)."""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import common
import devguard
import slack_common as sc
import wbc_capi as capi
import wbc_model
import wbc_workload
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = sc.DT
ROWS = ("slack_min", "slack_final", "slack_min_tick", "slack_min_which", "neg_ticks", "first_neg_tick")
COMMON = ("q", "qdot", "status", "iters", "ee_target")
SLACK_TOL = 1e-12        # wbc_state_slack against the numpy restatement: slack and components


@functools.lru_cache(maxsize=None)
def _rotated():
    """test_gpu_rotated_placement.py's recipe: the ViperX-300's rotations on a1_wx200"""
    def _rpy(r, p, y):
        cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
        return [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                [-sp, cp * sr, cp * cr]]
    with open(os.path.join(wbc_model.MODELS_DIR, "a1_wx200.json")) as f:
        data = copy.deepcopy(json.load(f))
    for name, rpy in (("elbow", (3.14, 0, 0)), ("wrist_rotate", (-3.14, 0, 0)), ("left_finger", (0.3, -0.2, 0.1))):
        next(j for j in data["joints"] if j["name"] == name)["placement_R"] = _rpy(*rpy)
    data["name"] = "a1_wx200_rotated"
    return wbc_model.Model(data, dict(wbc_model.A1_ROLES))


def _models(case):
    if case == "rotated":
        return [_rotated()]
    return [sc.model(n) for n in {"wx_px": ("a1_wx200", "a1_px100_pin_ver"), "laikago": ("laikago_vx300",),
                                  "laikago_wx": ("laikago_vx300", "a1_wx200")}[case]]


@functools.lru_cache(maxsize=None)
def _state_problem(case, B):
    """q: sample_q poses on even rows, far_q poses on odd rows, the arm joints moved by up to 5 mrad / mm; box centres off the pose by N(0, 0.02) so that no family is a tie by design"""
    models = _models(case)
    cfgs = [wbc_model.sim3_config(m) for m in models]
    rng = np.random.default_rng(100 + B)
    mid = (np.arange(B) % len(models)).astype(np.int32) if len(models) > 1 else None
    q = np.zeros((B, capi.Q_STRIDE))
    for i, m in enumerate(models):
        near, far = wbc_workload.sample_q(m, B, rng), common.far_q(m, B, rng)
        qm = np.where((np.arange(B) % 2 == 1)[:, None], far, near)
        qm[:, 19:m.nq] += rng.uniform(-0.005, 0.005, (B, m.nq - 19))   # the arm and the fingers off their nominal values (the fingers sit symmetric: a tie)
        sel = np.ones(B, bool) if mid is None else mid == i
        q[sel] = qm[sel]
    import oracle
    oMf = oracle.fk(models, q, mid, want_com=False)["oMf"]
    box = np.concatenate([oMf[:, capi.FR_TRUNK, 11:12], wbc_workload.R_to_euler_xyz(oMf[:, capi.FR_TRUNK, 0:9])], axis=1) + rng.normal(0, 0.02, (B, 4))
    ref = sc.reference_slack(models, cfgs, q, box, mid)
    return dict(models=models, cfgs=cfgs, q=q, box=box, mid=mid, ref=ref, B=B)


def _handle(models, cfgs, max_batch):
    bt = WbcBatch(models, max_batch)
    for i, c in enumerate(cfgs):
        bt.configure(c, i)
    return bt


def _guarded_state(bt, p, q=None, box="given"):
    """wbc_state_slack on device arrays between guard rows, on a side stream: inputs untouched, guards intact"""
    sess = devguard.Session("nan", torch.cuda.Stream())
    B = p["B"]
    q_d = sess.put("q", p["q"] if q is None else q, None)
    box_d = sess.put("box", p["box"], None) if box == "given" else None
    mid_d = sess.put("model_id", p["mid"], np.zeros(2 * devguard.G, np.int32)) if p["mid"] is not None else None
    bt.allocator = sess.alloc
    try:
        got = devguard.to_host(sess.run(lambda: bt.state_slack(q_d, box_d, mid_d, want_components=True)))
    finally:
        bt.allocator = None
    sess.check("state_slack B=%d" % B)
    return got


@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("case", ["wx_px", "laikago", "laikago_wx", "rotated"])
def test_state_slack_matches_the_restatement(case, B):
    p = _state_problem(case, B)
    bt = _handle(p["models"], p["cfgs"], B)
    got = _guarded_state(bt, p)
    ref = p["ref"]
    e_s, e_c = np.abs(got["slack"] - ref["slack"]).max(), np.abs(got["components"] - ref["components"]).max()
    clear = ref["gap"] > sc.TIE
    print("%s B=%d: slack %.3e components %.3e, codes compared on %s of %d rows" % (case, B, e_s, e_c, clear.sum(axis=0), B))
    assert e_s < SLACK_TOL and e_c < SLACK_TOL
    assert (clear.mean(axis=0) >= 0.75).all()
    assert (got["which"] == ref["which"])[clear].all()
    assert got["which"].dtype == np.int32 and (got["which"][:, 3] >= 12).all()
    if B == 67:
        # one NaN row: its four families NaN / -1, every other row bit-equal to the run without it (rows 64..66 sit in the partial wave 16)
        q = p["q"].copy()
        q[33, 12] = np.nan
        bad = _guarded_state(bt, p, q=q)
        assert np.isnan(bad["slack"][33]).all() and (bad["which"][33] == -1).all() and np.isnan(bad["components"][33]).all()
        keep = np.arange(B) != 33
        for k in ("slack", "which", "components"):
            assert devguard.same_bytes(bad[k][keep], got[k][keep]), k
        # no box: families 0 and 3 unchanged, 1 and 2 NaN / -1
        nb = _guarded_state(bt, p, box=None)
        assert devguard.same_bytes(nb["slack"][:, [0, 3]], got["slack"][:, [0, 3]]) and devguard.same_bytes(nb["which"][:, [0, 3]], got["which"][:, [0, 3]])
        assert np.isnan(nb["slack"][:, 1:3]).all() and (nb["which"][:, 1:3] == -1).all() and np.isnan(nb["components"][:, 4:]).all()
        assert devguard.same_bytes(nb["components"][:, :4], got["components"][:, :4])
        # a non-finite box entry takes its own family alone
        box = p["box"].copy()
        box[5, 0], box[6, 3] = np.inf, np.nan
        pb = dict(p, box=box)
        gb = _guarded_state(bt, pb)
        assert np.isnan(gb["slack"][5, 1]) and gb["which"][5, 1] == -1 and np.isnan(gb["slack"][6, 2]) and gb["which"][6, 2] == -1
        assert devguard.same_bytes(gb["slack"][5, [0, 2, 3]], got["slack"][5, [0, 2, 3]]) and devguard.same_bytes(gb["slack"][6, [0, 1, 3]], got["slack"][6, [0, 1, 3]])
    bt.close()


# ---- the watch
def _watch(bt, p, **kw):
    args = dict(imu=p["imu"], mode=capi.ROLLOUT_RUNNING if p["running"] else capi.ROLLOUT_WARMUP, want_trace=True, tracks=p["tracks"],
                ee_target_step=p["step"])
    if p["tracks"] is not None and len(p["tracks"]) == 2:
        args["score"] = ("trunk", common.GRIP)
    args.update(kw)
    return bt.rollout_watch(p["d"], DT, p["K"], **args)


def _small_two_track_problem():
    p = sc.watch_problem("trunk_task_tracks", 29, 8)
    return p


def test_no_watch_is_the_unwatched_call_and_a_watch_only_reads():
    # the two-track call
    p = _small_two_track_problem()
    bt = _handle(p["models"], p["cfgs"], p["B"])
    args = dict(score=("trunk", common.GRIP), group_size=0, want_trace=True, mode=capi.ROLLOUT_RUNNING, imu=p["imu"])
    plain = bt.rollout_tracks(p["d"], DT, p["K"], p["tracks"], **args)
    nowatch = bt.rollout_watch(p["d"], DT, p["K"], watch=(), tracks=p["tracks"], **args)
    assert devguard.same_bytes(plain, nowatch)
    watched = bt.rollout_watch(p["d"], DT, p["K"], tracks=p["tracks"], **args)
    assert set(plain) < set(watched)
    for k in plain:
        assert devguard.same_bytes(plain[k], watched[k]), k
    bt.close()
    # the plain call: a constant step and three hold ticks
    p = sc.watch_problem("sim3", 29, 8)
    bt = _handle(p["models"], p["cfgs"], p["B"])
    plain = bt.rollout(p["d"], DT, p["K"], ee_target_step=p["step"], imu=p["imu"], hold_ticks=3, want_trace=True)
    nowatch = bt.rollout_watch(p["d"], DT, p["K"], watch=(), ee_target_step=p["step"], imu=p["imu"], hold_ticks=3, want_trace=True)
    assert devguard.same_bytes(plain, nowatch)
    watched = bt.rollout_watch(p["d"], DT, p["K"], ee_target_step=p["step"], imu=p["imu"], hold_ticks=3, want_trace=True)
    for k in plain:
        assert devguard.same_bytes(plain[k], watched[k]), k
    assert watched["slack_trace"].shape == (p["K"] + 3, 4, p["B"]) and plain["grip_trace"].shape == (p["K"] + 3, p["B"], 3)
    own = wbc_workload.watch_summary(watched["slack_trace"])
    for k in own:
        assert devguard.same_bytes(own[k], watched[k]), k
    bt.close()


@pytest.mark.parametrize("name", list(sc.WATCH_CASES))
def test_watch_matches_the_oracle_loop(name):
    """trace, slack_min and slack_final within 1e-6 of the oracle's loop (ok instances); tick, code and counts where slack_common.comparable says the
    oracle's own values leave no doubt, each on at least 3/4 of the instances; the summary against the reduction of the device's OWN trace bit
    for bit. The code is held to "a component the oracle has within 1e-9 of its minimum at that tick", which is the minimum's own code wherever
    the components are further apart: with the IMU fed back unchanged all six trunk-angle components tie to an ulp on both sides. The trace holds
    no codes, so of the own-trace comparison the code keeps only: -1 exactly where the minimum is NaN.
    Measured on MI355X (profiles/r14_rollout_watch.txt): trace 5.3e-15 .. 4.6e-13, slack_min 3.3e-15 .. 1.3e-13, slack_final 5.3e-15 .. 4.6e-13 over
    the six recipes; 57 to 67 of 67 instances compared per family, all equal."""
    p, ref = sc.watch_problem(name), sc.watch_reference(name)
    B, K = p["B"], p["K"]
    bt = _handle(p["models"], p["cfgs"], B)
    if name.startswith("everything"):
        bt.set_option("packed_orth", 2)                            # the packed orth kernel at every batch size (by default from 4608 instances on)
    got = _watch(bt, p)
    path = bt.stat("last_path")
    bt.close()
    assert path == {"sim3": 2, "everything": 3, "everything_tracks_warmup": 3}.get(name, path)
    assert (got["status"] == ref["status"]).all()
    ok = ref["status"] == 0
    tr = ref["trace"]
    own = wbc_workload.watch_summary(got["slack_trace"])
    want = wbc_workload.watch_summary(tr)
    e_t = np.abs(got["slack_trace"] - tr)[:, :, ok].max()
    e_m = np.abs(got["slack_min"] - want["slack_min"])[:, ok].max()
    e_f = np.abs(got["slack_final"] - want["slack_final"])[:, ok].max()
    c = sc.comparable(ref)
    print("%s: path %d, optimal %d/%d, trace %.3e  slack_min %.3e  slack_final %.3e; compared tick %s which %s counts %s of %d" % (
        name, path, int(ok.sum()), B, e_t, e_m, e_f, (c["tick"] & ok).sum(axis=1), (c["which"] & ok).sum(axis=1), (c["counts"] & ok).sum(axis=1), B))
    assert ok.mean() >= 0.75
    assert e_t < 1e-6 and e_m < 1e-6 and e_f < 1e-6
    for k in ("tick", "which", "counts"):
        assert ((c[k] & ok).mean(axis=1) >= 0.75).all(), k
    m = c["tick"] & ok
    assert (got["slack_min_tick"] == want["slack_min_tick"])[m].all()
    # the code: a component the oracle has within TIE of its minimum at that tick (the minimum's own code wherever the components are not tied)
    m = c["which"] & ok
    f_i, b_i = np.nonzero(m)
    k_i, w_i = want["slack_min_tick"][f_i, b_i], got["slack_min_which"][f_i, b_i]
    assert (w_i >= 0).all()
    assert (ref["bycode"][k_i, f_i, b_i, w_i] <= tr[k_i, f_i, b_i] + sc.TIE).all()
    clear = np.take_along_axis(ref["gap"], want["slack_min_tick"][None].astype(np.int64), axis=0)[0] > sc.TIE
    wref = np.take_along_axis(ref["which"], want["slack_min_tick"][None].astype(np.int64), axis=0)[0]
    assert (got["slack_min_which"] == wref)[m & clear].all()
    m = c["counts"] & ok
    assert (got["neg_ticks"] == want["neg_ticks"])[m].all() and (got["first_neg_tick"] == want["first_neg_tick"])[m].all()
    # without conditions: the summary is the reduction of the device's OWN trace, bit for bit
    for k in own:
        assert devguard.same_bytes(own[k], got[k]), k
    assert ((got["slack_min_which"] == -1) == np.isnan(got["slack_min"])).all()


def test_groups_and_repeatability():
    p = sc.watch_problem("sim3", 66, 6)
    B = p["B"]
    bt = _handle(p["models"], p["cfgs"], B)
    runs = {M: _watch(bt, p, group_size=M) for M in (1, 6, B)}
    again = _watch(bt, p, group_size=6)
    assert devguard.same_bytes(runs[6], again)
    bt.close()
    bt2 = _handle(p["models"], p["cfgs"], B + 61)
    wide = _watch(bt2, p, group_size=6)
    bt2.close()
    assert devguard.same_bytes(runs[6], wide)
    for M, got in runs.items():
        for k in ROWS + COMMON + ("slack_trace",):
            assert devguard.same_bytes(got[k], runs[1][k]), (M, k)
        gmin = got["slack_min"].reshape(4, B // M, M).min(axis=2)
        gneg = (got["neg_ticks"] > 0).reshape(4, B // M, M).sum(axis=2).astype(np.int32)
        assert devguard.same_bytes(got["slack_group_min"], gmin) and devguard.same_bytes(got["slack_group_neg_instances"], gneg), M
    assert (runs[1]["neg_ticks"] > 0).any()


def test_refusals_name_the_field_and_write_nothing():
    p = sc.watch_problem("trunk_task_tracks", 12, 2)
    B = p["B"]
    bt = _handle(p["models"], p["cfgs"], B)
    lib = bt.lib
    keep = []
    d = dict(p["d"])
    tin = bt._tick_in(d, keep, B)
    pattern = -12345.5
    outs = {k: np.full((4, B), pattern) for k in ("slack_min", "slack_final")}
    q_final = np.full((B, 27), pattern)

    def rollout(ticks=2, hold=0):
        r = capi.WbcRollout()
        r.ticks, r.mode, r.hold_ticks = ticks, capi.ROLLOUT_RUNNING, hold
        r.q_final = q_final.ctypes.data
        return r

    def watch(mask=15, group_size=0):
        w = capi.WbcSlackWatch()
        w.mask, w.group_size = mask, group_size
        w.slack_min, w.slack_final = outs["slack_min"].ctypes.data, outs["slack_final"].ctypes.data
        return w

    def tracks():
        tk = capi.WbcTracks()
        tk.n_tracks = 1
        t = tk.track[0]
        pts = np.ascontiguousarray(p["tracks"][1]["points"])
        keep.append(pts)
        t.target, t.kind, t.max_points, t.points, t.du_all = common.GRIP, capi.TRACK_LINEAR, pts.shape[1], pts.ctypes.data, 0.2
        return tk

    def refused(word, tin_=tin, r=None, tk=None, sc_=None, w=None, code=capi.E_ARG):
        r = r or rollout()
        rc = lib.wbc_rollout_watch(bt._h, B, C.byref(tin_), None, DT, C.byref(r), C.byref(tk) if tk else None, C.byref(sc_) if sc_ else None,
                                   C.byref(w) if w else None, capi.MEM_HOST, None)
        msg = (lib.wbc_last_error() or b"").decode()
        assert rc == code and word in msg, (word, rc, msg)

    refused("mask", w=watch(mask=0))
    refused("mask", w=watch(mask=16))
    refused("mask", w=watch(mask=-1))
    refused("scores", sc_=capi.WbcTrackScores(), w=watch())
    refused("group_size", w=watch(group_size=5))
    nobox = bt._tick_in({k: v for k, v in d.items() if k != "trunk_box_center"}, keep, B)
    refused("trunk_box_center", tin_=nobox, w=watch(mask=2))
    refused("trunk_box_center", tin_=nobox, w=watch(mask=4))
    refused("hold_ticks", r=rollout(hold=1), tk=tracks(), w=watch())             # with tracks, the tracks call's own refusals
    o = capi.WbcSlackOut()
    sl = np.full((B, 4), pattern)
    o.slack = sl.ctypes.data
    q = np.ascontiguousarray(d["q"])
    mid = np.ascontiguousarray(p["mid"])
    for args, word in (((None, None, mid.ctypes.data, capi.MEM_HOST, C.byref(o), None), "q"),
                       ((q.ctypes.data, None, mid.ctypes.data, capi.MEM_HOST, None, None), "out"),
                       ((q.ctypes.data, None, None, capi.MEM_HOST, C.byref(o), None), "model_id")):
        rc = lib.wbc_state_slack(bt._h, B, *args)
        msg = (lib.wbc_last_error() or b"").decode()
        assert rc == capi.E_ARG and (" %s " % word) in msg, (word, rc, msg)
    bt.synchronize()
    assert (sl == pattern).all() and (q_final == pattern).all() and all((v == pattern).all() for v in outs.values())
    # ... and the same arguments without the fault are taken
    ok = bt.rollout_watch(d, DT, 2, watch=("joint",), tracks=None)
    assert np.isfinite(ok["slack_min"]).all() and ok["slack_min"].shape == (1, B)
    # the Python front end's own checks
    with pytest.raises(capi.WbcError, match="twice"):
        bt.rollout_watch(d, DT, 2, watch=("com", 0))
    with pytest.raises(capi.WbcError, match="watch"):
        bt.rollout_watch(d, DT, 2, watch=("centre of mass",))
    with pytest.raises(capi.WbcError, match="score"):
        bt.rollout_watch(d, DT, 2, score=(4,))
    bt.close()
