"""Closed loops of K = 300 ticks on the device, every tick held one step ahead to the oracle.

End-to-end parity after hundreds of ticks is ill-posed (a 1e-9 change of q_0 grows a million-fold: test_long_horizon_host.py prints the
table), one-step parity is not: the device runs its OWN closed loop, wbc_rollout_record tapes the state, the targets, q̇, the status and
(warm_start 1) the working set of every tick, and the K x B taped states go through the oracle as one batch. The cases, their conditions and
the references are long_horizon_cases.py's; every tolerance is an existing one, named where it is used:
  status equal; q̇ within the path's parity tolerance (pose_cases.REFINED_TOL on the packed sim3 kernel under c3, QDOT_TOL elsewhere);
  iterations within 2 per tick (test_rollout_parity's rule per tick; cold ticks — the oracle has no hot start — read from the one-tick
  chain, which is the long call byte for byte); the state after the tick within pose_cases.kin_tol of the oracle's step from the device's
  own q̇; the targets bit-equal to numpy's running sums; the taped working set equal to the exact active-side rule on the oracle's q̇
  (ticks with a side near the rule's threshold left out, at most 5 %).
An instance is compared up to its first unsolved tick, and its status is compared there."""
import functools

import numpy as np
import pytest

import common
import long_horizon_cases as lh
import oracle
import pose_cases as pc
import step_common as sc
import test_gpu_task_params as tgp
import wbc_capi as capi
from wbc_batch import RolloutTape

pytestmark = pytest.mark.gpu

DT, K = lh.DT, lh.K
OUT = ("q", "qdot", "ee_target", "status", "iters")
TAPED = ("q", "qdot", "ee_target", "prev_ee_target", "trunk_target", "prev_trunk_target", "status", "working_set")


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _handle(p, warm=0, **more):
    return tgp._handle(p["models"], p["cfgs"], p["B"], dict(p["case"]["opts"], warm_start=warm, **more))


def _assert_row(bt, case, warm):
    """the statistics name the kernel family and the row of its variant table the case is meant for (test_gpu_pose_envelope._assert_row)"""
    if case["row"] is None:
        assert bt.stat("last_path") == case["path"], bt.stat("last_path")
        return
    family, row = case["row"](warm)
    assert bt.stat("last_path") == pc.LAST_PATH[family], (family, bt.stat("last_path"))
    got = bt.stat("last_tick_variant")
    assert got == pc.key_of(row), "%s: last_tick_variant = %s, want %s" % (family, capi.variant_args(got), row)


def _tape_arrays(p, tape, warm):
    """the blocks a record writes, [K, B, ...] on the host (cold, the working sets are never written)"""
    host = RolloutTape(tape.buf.cpu(), tape.B, tape.ticks)               # (one copy; the views are RolloutTape.tick's)
    ticks = [{k: v.numpy() for k, v in host.tick(k).items()} for k in range(tape.ticks)]
    t = {k: np.stack([x[k] for x in ticks]) for k in TAPED if warm or k != "working_set"}
    t["ee_target"], t["prev_ee_target"] = t["ee_target"].reshape(-1, p["B"], 5, 3), t["prev_ee_target"].reshape(-1, p["B"], 5, 3)
    # the head: the previous rotations every tick after the first read (include/wbc.h: ee_prev_rot [B][5][9], then trunk_prev_rot [B][9])
    head = host.buf[:tape.B * capi.TAPE_HEAD_BYTES].numpy().view(np.float64)
    if "ee_prev_rot" in p["d"]:
        t["ee_prev_rot"] = head[:45 * tape.B].reshape(tape.B, 5, 9).copy()
    t["trunk_prev_rot"] = head[45 * tape.B:].reshape(tape.B, 9).copy()
    return t


def _record(bt, p, **more):
    return bt.rollout_record(p["d"], DT, p["K"], ee_target_step=p["step"], imu=p["imu"], task_params=p["rows"], **more)


@functools.lru_cache(maxsize=None)
def _recorded(name, warm):
    """-> (rec: rollout_record's outputs, tape: its blocks [K, B, ...]) of the case under option warm_start = warm; the kernel row is
    confirmed, and a second identical call on the same handle gives identical bytes"""
    p = lh.problem(name)
    bt = _handle(p, warm)
    try:
        rec, tape = _record(bt, p)
        _assert_row(bt, p["case"], warm)
        t = _tape_arrays(p, tape, warm)
        rec2, tape2 = _record(bt, p)
        t2 = _tape_arrays(p, tape2, warm)
        assert all(_same(rec[k], rec2[k]) for k in rec) and all(_same(t[k], t2[k]) for k in t), "%s: two identical calls differ" % name
    finally:
        bt.close()
    for v in list(rec.values()) + list(t.values()):
        v.setflags(write=False)
    return rec, t


@functools.lru_cache(maxsize=None)
def _one_step(name, warm):
    """the oracle at every taped state: (its tick's outputs [K, B, ...], the assembled bounds and rows of those states)"""
    p = lh.problem(name)
    _, t = _recorded(name, warm)
    n = p["K"]
    d = lh.stacked(p, t["q"], t["ee_target"], t["prev_ee_target"], t["trunk_target"], t["prev_trunk_target"], head=t)
    o = lh.oracle_tick(p, d, n)
    ref = {k: v.reshape((n, p["B"]) + v.shape[1:]) for k, v in o.items()}
    return ref, d


def _check_status_and_qdot(name, what, status, qdot, ref, tol):
    """status on every compared instance-tick, q̇ on those both solve; -> the compared ticks [K, B]"""
    live = lh.compared(ref["status"])
    wrong = np.argwhere((status != ref["status"]) & live)
    assert not len(wrong), "%s: status differs from the oracle's at (tick, instance) %s" % (what, wrong[:8].tolist())
    ok = live & (ref["status"] == 0)
    err = np.abs(qdot - ref["qdot"]).max(axis=2) * ok
    k, b = np.unravel_index(np.argmax(err), err.shape)
    print("%s: %d of %d instance-ticks compared, %d solved; worst |qdot - oracle| / tol = %.3e (%.3e against %.0e) at tick %d, instance %d, "
          "where max|qdot| = %.3g" % (what, int(live.sum()), live.size, int(ok.sum()), err[k, b] / tol, err[k, b], tol, k, b, np.abs(ref["qdot"][k, b]).max()))
    assert ok.mean() >= 0.9
    assert err.max() <= tol, "%s: q̇ misses the path's tolerance at (tick, instance) %s" % (what, np.argwhere(err > tol)[:8].tolist())
    return live, ok


# ---- 2. one step ahead along the device's own trajectory
@pytest.mark.parametrize("name,warm", [(n, w) for n in lh.RECORDED for w in lh.CASES[n]["warm"]])
def test_every_tick_of_the_tape_one_step_ahead(name, warm):
    p = lh.problem(name)
    B, n, case = p["B"], p["K"], p["case"]
    rec, t = _recorded(name, warm)
    ref, d = _one_step(name, warm)
    what = "%s / warm_start %d" % (name, warm)
    live, ok = _check_status_and_qdot(name, what, t["status"], t["qdot"], ref, case["tol"])
    assert np.array_equal(rec["status"], t["status"].max(axis=0))

    # the state after the tick: the oracle's step from the device's own q̇ (the solver's tolerance does not enter)
    q_after = np.concatenate([t["q"][1:], rec["q"][None]])
    assert _same(q_after, rec["q_trace"])
    qk, vk = t["q"].reshape(n * B, 27), t["qdot"].reshape(n * B, 26)
    mid = None if p["mid"] is None else np.tile(p["mid"], n)
    step = oracle.update_state(p["models"], qk, oracle.integrate(p["models"], qk, vk, DT, mid), t["ee_target"].reshape(n * B, 15), np.tile(p["imu"], (n, 1)), mid)
    es = np.abs(q_after.reshape(n * B, 27) - step).max(axis=1).reshape(n, B) * live
    tol = pc.kin_tol(step)
    print("%s: worst |state after the tick - oracle's step of the device's qdot| = %.3e (kin_tol %.3e) at tick %d" % (what, es.max(), tol, np.argmax(es.max(axis=1))))
    assert es.max() <= tol

    # target bookkeeping: running sums in numpy, in the same order
    sums = lh.target_sums(p, n)
    assert _same(t["ee_target"], sums[:n]) and _same(rec["ee_target"], sums[n])
    cur = {k: np.array(v, copy=True) for k, v in p["d"].items()}
    for k in range(n):
        assert _same(t["prev_ee_target"][k], cur["prev_ee_target"]), (what, k)
        assert _same(t["trunk_target"][k], cur["trunk_target"]) and _same(t["prev_trunk_target"][k], cur["prev_trunk_target"]), (what, k)
        cur = sc.advance(p["cfgs"][0], cur, cur["q"], p["step"])

    if not warm:
        return
    # the carried working set: the exact active-side rule on the oracle's q̇ at that state
    a = lh.oracle_assemble(p, d, n)
    rule, near = lh.active_sides(a, ref["qdot"].reshape(n * B, 26))
    taped = lh.taped_sides(t["working_set"].reshape(n * B, 2), a["C"].shape[1])
    ineq = rule != 3
    use = (ok & ~near.reshape(n, B)).reshape(n * B)
    left_out = float((near.reshape(n, B) & ok).sum()) / max(1, int(ok.sum()))
    differs = ((taped != rule) & ineq).any(axis=1) & use
    sides = ((rule == 1) | (rule == 2)).reshape(n, B, -1)
    added, dropped = lh.set_events(taped.reshape(n, B, -1) * ineq.reshape(n, B, -1), ok)
    print("%s: taped working sets: %d of %d compared sets differ from the exact rule's, left out %.4f; active inequalities per tick %d..%d; "
          "a constraint added in %d / %d instances, dropped in %d / %d" % (what, int(differs.sum()), int(use.sum()), left_out, sides.sum(axis=2).min(),
                                                                       sides.sum(axis=2).max(), added.sum(), B, dropped.sum(), B))
    assert left_out <= lh.LEFT_OUT_CAP
    assert not differs.any(), "%s: (tick, instance) %s" % (what, [divmod(int(i), B) for i in np.flatnonzero(differs)[:8]])
    assert 2 * added.sum() >= B and 2 * dropped.sum() >= B           # condition (c) of test_long_horizon_host.py, on the tape itself
    assert not (t["working_set"][t["status"] != 0] != 0).any()       # (include/wbc.h: zeros for an instance whose QP was not solved)


# ---- 3. the long call is its own pieces, byte for byte
@pytest.mark.parametrize("name,warm", [(n, w) for n in lh.RECORDED for w in lh.CASES[n]["warm"]])
def test_the_recorded_call_is_the_plain_rollout(name, warm):
    p = lh.problem(name)
    rec, _ = _recorded(name, warm)
    bt = _handle(p, warm)
    try:
        plain = bt.rollout(p["d"], DT, p["K"], ee_target_step=p["step"], imu=p["imu"], task_params=p["rows"], want_trace=False)
        _assert_row(bt, p["case"], warm)
    finally:
        bt.close()
    for k in OUT:
        assert _same(rec[k], plain[k]), "%s / warm_start %d: %s of the record differs from wbc_rollout_tp's" % (name, warm, k)


@functools.lru_cache(maxsize=None)
def _chained(name):
    """K one-tick roll-outs chained by hand (warm_start 0): -> dict(q [K + 1, B, 27], qdot, ee_target [K + 1], prev_ee_target, status, iters [K, B])"""
    p = lh.problem(name)
    B, n, cfg = p["B"], p["K"], p["cfgs"][0]
    r = dict(q=np.zeros((n + 1, B, 27)), qdot=np.zeros((n, B, 26)), status=np.zeros((n, B), np.int32), iters=np.zeros((n, B), np.int32),
             ee_target=np.zeros((n + 1, B, 5, 3)), prev_ee_target=np.zeros((n, B, 5, 3)), trunk_target=np.zeros((n, B, 3)), prev_trunk_target=np.zeros((n, B, 3)))
    d = {k: np.array(v, copy=True) for k, v in p["d"].items()}
    head = {f: v for f, v in _recorded(name, 0)[1].items() if f in ("ee_prev_rot", "trunk_prev_rot")} if p["case"].get("tape", True) else {}
    bt = _handle(p, 0)
    try:
        for k in range(n):
            r["q"][k] = d["q"]
            for f in ("ee_target", "prev_ee_target", "trunk_target", "prev_trunk_target"):
                r[f][k] = d[f]
            o = bt.rollout(d, DT, 1, ee_target_step=p["step"], imu=p["imu"], task_params=p["rows"], want_trace=False)
            r["qdot"][k], r["status"][k], r["iters"][k] = o["qdot"], o["status"], o["iters"]
            d = sc.advance(cfg, d, o["q"], p["step"])
            assert _same(o["ee_target"], d["ee_target"])
            for f in head:                                   # the previous rotations as the device formed them (its own sines, not scipy's)
                assert np.abs(head[f] - d[f].reshape(head[f].shape)).max() < 1e-15, (f, k)
                d[f] = head[f].reshape(d[f].shape).copy()
        _assert_row(bt, p["case"], 0)
    finally:
        bt.close()
    r["q"][n], r["ee_target"][n] = d["q"], d["ee_target"]
    return r


@pytest.mark.parametrize("name", list(lh.CASES))
def test_the_long_call_is_300_one_tick_calls(name):
    """warm_start 0: one K = 300 call equals 300 one-tick calls chained by hand on a second handle (test_rollout_equals_tick_plus_update_state's
    pattern), `c3_hybrid` included; the chain's per-tick iteration counts are held to the oracle's within 2, and for `c3_hybrid`, which has
    no tape, the chain supplies the states for the one-step status and q̇"""
    p = lh.problem(name)
    B, n, case = p["B"], p["K"], p["case"]
    c = _chained(name)
    bt = _handle(p, 0)
    try:
        whole = bt.rollout(p["d"], DT, n, ee_target_step=p["step"], imu=p["imu"], task_params=p["rows"], want_trace=False)
    finally:
        bt.close()
    assert _same(whole["q"], c["q"][n]) and _same(whole["qdot"], c["qdot"][n - 1]) and _same(whole["ee_target"], c["ee_target"][n])
    assert np.array_equal(whole["status"], c["status"].max(axis=0)) and np.array_equal(whole["iters"], c["iters"].sum(axis=0))
    if case.get("tape", True):
        _, t = _recorded(name, 0)
        for k in ("q", "qdot", "status", "ee_target", "prev_ee_target"):
            assert _same(t[k], c[k][:n]), "%s: %s of the tape differs from the chain's" % (name, k)
        ref, _ = _one_step(name, 0)
    else:
        o = lh.oracle_tick(p, lh.stacked(p, c["q"][:n], c["ee_target"][:n], c["prev_ee_target"], c["trunk_target"], c["prev_trunk_target"]), n)
        ref = {k: v.reshape((n, B) + v.shape[1:]) for k, v in o.items()}
        _check_status_and_qdot(name, "%s (chain)" % name, c["status"], c["qdot"], ref, case["tol"])
    ok = lh.compared(ref["status"]) & (ref["status"] == 0)
    di = np.abs(c["iters"].astype(np.int64) - ref["iters"]) * ok
    print("%s: iterations per tick, device %d..%d, oracle %d..%d; worst |device - oracle| = %d at tick %d; equal on %.4f of the ticks" % (
        name, c["iters"].min(), c["iters"].max(), ref["iters"].min(), ref["iters"].max(), di.max(), np.argmax(di.max(axis=1)), (di == 0).mean()))
    assert di.max() <= 2


def _tape_of(p, warm, **opts):
    bt = _handle(p, warm, **opts)
    try:
        rec, tape = _record(bt, p)
        return rec, _tape_arrays(p, tape, warm)
    finally:
        bt.close()


@pytest.mark.parametrize("name,warm,option,values", [("c3", 1, "wave_order", (0, 2)), ("c3_trunk_task", 0, "wave_order", (0, 2)),
                                                     ("c3_general", 1, "grid", (1, 3)), ("mixed", 0, "grid", (1, 3))])
def test_wave_order_and_grid_do_not_change_a_bit(name, warm, option, values):
    """include/wbc.h and DESIGN.md §3.19 (wave_order: "results are bit-identical either way") and §3.32 (grid: byte-identical outputs at every
    grid): the same tape and outputs as the default handle's, over 300 ticks of carried wave order"""
    p = lh.problem(name)
    rec, t = _recorded(name, warm)
    for v in values:
        rec2, t2 = _tape_of(p, warm, **{option: v})
        for k in OUT:
            assert _same(rec[k], rec2[k]), "%s: %s = %d changes %s" % (name, option, v, k)
        for k in t:
            assert _same(t[k], t2[k]), "%s: %s = %d changes the tape's %s" % (name, option, v, k)


# ---- 4. device-side reductions over many ticks: scores and the slack watch along two tracks
FLOAT_SCORES, INT_SCORES = ("err_sq_sum", "err_max", "err_final"), ("first_bad_tick", "bad_ticks")
SCORE_FRAMES = [common.GRIP, 5]                     # rows of common.track_frames: the scored frames in increasing index order, the trunk last
WATCH_ROWS = ("slack_min", "slack_final", "slack_min_tick", "slack_min_which", "neg_ticks", "first_neg_tick")


@functools.lru_cache(maxsize=None)
def _tracked(name):
    """-> (the recorded tracks call's outputs, its tape, rollout_tracks' outputs, rollout_watch's outputs with all four families) on one handle"""
    p = lh.tracks_problem(name)
    bt = _handle(p, 0)
    try:
        kw = dict(score=lh.SCORE, group_size=lh.GROUP)
        rec, tape = bt.rollout_record(p["d"], DT, p["K"], tracks=p["tracks"], task_params=p["rows"], **kw)
        _assert_row(bt, p["case"], 0)
        t = _tape_arrays(p, tape, 0)
        plain = bt.rollout_tracks(p["d"], DT, p["K"], p["tracks"], task_params=p["rows"], **kw)
        watched = bt.rollout_watch(p["d"], DT, p["K"], tracks=p["tracks"], task_params=p["rows"], want_trace=True, **kw)
    finally:
        bt.close()
    return rec, t, plain, watched


def _score_bound(ref, ticks):
    return 4 * ticks * np.finfo(np.float64).eps * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name", lh.TRACK_CASES)
def test_scores_over_300_ticks_against_the_host_reduction(name):
    """err_sq_sum, err_max, err_final and the group outputs within 4 K eps max(1, |ref|) of numpy's reduction over oracle.fk at the taped
    states and wbc_workload.track_targets at each tick; the integers exact (err_max_tick: instances whose two largest errors are within
    1e-12 of each other left out, at most 5 %); the recorded call's scores are rollout_tracks' byte for byte"""
    p = lh.tracks_problem(name)
    B, n, M = p["B"], p["K"], lh.GROUP
    rec, t, plain, _ = _tracked(name)
    for k in plain:
        assert _same(rec[k], plain[k]), "%s: %s of the recorded call differs from wbc_rollout_tracks'" % (name, k)
    targets = lh.track_targets_all(p, n)
    assert _same(t["ee_target"][:, :, common.GRIP], targets[:, common.GRIP]) and _same(t["trunk_target"], targets[:, 5])       # what the ticks saw
    assert _same(rec["ee_target"][:, common.GRIP], lh.follow(p, p["d"], n)["ee_target"][:, common.GRIP])
    mid = None if p["mid"] is None else np.tile(p["mid"], n)
    frames = common.track_frames(p["models"], rec["q_trace"].reshape(n * B, 27), mid).reshape(n, B, 6, 3)
    trace = np.swapaxes(frames[:, :, SCORE_FRAMES], 1, 2)
    ref = common.numpy_scores(trace, targets[:, SCORE_FRAMES], t["status"])
    assert (t["status"] == 0).mean() >= 0.9
    for k in FLOAT_SCORES:
        err, bound = np.abs(rec[k] - ref[k]).max(), _score_bound(ref[k], n)
        print("%s: %s max|device - host| = %.3e (bound 4 K eps max(1, |ref|) = %.3e, max|ref| = %.3e)" % (name, k, err, bound, np.abs(ref[k]).max()))
        assert err <= bound, k
    for k in INT_SCORES:
        assert np.array_equal(rec[k], ref[k]), k
    e = np.sort(np.linalg.norm(trace - targets[:, SCORE_FRAMES], axis=-1), axis=0)
    clear = (e[-1] - e[-2]) > lh.TIE
    print("%s: err_max_tick compared on %d of %d (frame, instance) pairs; ticks %d..%d" % (name, clear.sum(), clear.size, ref["err_max_tick"].min(), ref["err_max_tick"].max()))
    assert (~clear).mean() <= lh.LEFT_OUT_CAP
    assert np.array_equal(rec["err_max_tick"][clear], ref["err_max_tick"][clear])
    G = B // M
    rms = np.sqrt(ref["err_sq_sum"].reshape(2, G, M).sum(axis=2) / (M * n))
    gmax = ref["err_max"].reshape(2, G, M).max(axis=2)
    assert np.abs(rec["group_rms"] - rms).max() <= _score_bound(rms, n) and np.abs(rec["group_err_max"] - gmax).max() <= _score_bound(gmax, n)
    assert np.array_equal(rec["group_worst_status"], t["status"].max(axis=0).reshape(G, M).max(axis=1))
    assert np.array_equal(rec["group_bad_instances"], (ref["bad_ticks"].reshape(G, M) > 0).sum(axis=1))
    # the segment switches happened on the device: the gripper's target of the last tick is the last milestone wherever the track ended
    held = lh.segment_passes(p, n)[0][1]
    assert 4 * held.sum() >= B and _same(t["ee_target"][n - 1][held, common.GRIP], p["tracks"][0]["points"][held, -1])


@pytest.mark.parametrize("name", lh.TRACK_CASES)
def test_watch_over_300_ticks_against_the_host_restatement(name):
    """rollout_watch with all four families on the same inputs: the same states as the recorded run byte for byte; every output recomputed
    from slack_common's restatement at the taped states — minimum and last value within pose_cases.kin_tol, first tick, component and ticks
    outside exact (instances with two candidates within 1e-12 left out, at most 5 %; the ticks outside of an instance that rests on an
    enforced face — a quarter of `everything`'s trunk-angle family, whatever the seed: DESIGN.md §3.46 — are held tick by tick instead);
    instances leave their box and come back"""
    import wbc_workload
    p = lh.tracks_problem(name)
    B, n, M = p["B"], p["K"], lh.GROUP
    rec, t, plain, got = _tracked(name)
    for k in plain:
        assert _same(got[k], plain[k]), "%s: %s of the watched call differs from the unwatched call's" % (name, k)
    assert _same(got["q"], rec["q"])
    trace, which, gap = lh.slack_at(p, rec["q_trace"])
    want = wbc_workload.watch_summary(trace, which)
    tol = pc.kin_tol(trace)
    e_t, e_m, e_f = np.abs(got["slack_trace"] - trace).max(), np.abs(got["slack_min"] - want["slack_min"]).max(), np.abs(got["slack_final"] - want["slack_final"]).max()
    print("%s: slack trace %.3e, minimum %.3e, last value %.3e against the restatement at the taped states (kin_tol %.3e)" % (name, e_t, e_m, e_f, tol))
    assert e_t <= tol and e_m <= tol and e_f <= tol
    s = np.sort(trace, axis=0)
    tick_ok = (s[1] - s[0]) > lh.TIE                                                   # the two smallest per-tick values of an instance
    gap_at = np.take_along_axis(gap, want["slack_min_tick"][None].astype(np.int64), axis=0)[0]
    which_ok = tick_ok & (gap_at > lh.TIE)                                             # ... and the two smallest components at that tick
    # a slack within TIE of zero has no sign two roundings must agree on (an instance at rest on an enforced face: its slack halves every
    # tick until it is rounding). The first tick outside is exact unless such a tick comes before it; the ticks outside are exact where
    # there is none and otherwise lie between the clearly negative ticks and those plus the undecided ones — nothing is left out of that
    clear = np.abs(trace) > lh.TIE
    neg = (trace < 0) & clear
    first = np.where(neg.any(axis=0), neg.argmax(axis=0), -1).astype(np.int32)
    before = np.arange(n)[:, None, None] < np.where(first < 0, n, first)[None]
    first_ok = ~(~clear & before).any(axis=0)
    lo = neg.sum(axis=0)
    hi = lo + (~clear).sum(axis=0)
    out, leaves = lh.crossings(trace)
    some = (out > 0) & (out < n)
    for f, fam in enumerate(lh.FAMILIES):
        print("%s: %s: compared of %d instances: tick %d, component %d, first tick outside %d, ticks outside exactly %d (the others within their %d..%d "
              "undecided ticks); outside on some ticks %d instances (ticks outside %d..%d, first tick %d..%d), most inside-to-outside transitions %d" % (
                  name, fam, B, tick_ok[f].sum(), which_ok[f].sum(), first_ok[f].sum(), (hi[f] == lo[f]).sum(), (hi - lo)[f].min(), (hi - lo)[f].max(),
                  some[f].sum(), out[f].min(), out[f].max(), first[f].min(), first[f].max(), leaves[f].max()))
    for ok in (tick_ok, which_ok, first_ok):
        assert (~ok).mean() <= lh.LEFT_OUT_CAP
    assert np.array_equal(got["slack_min_tick"][tick_ok], want["slack_min_tick"][tick_ok])
    assert np.array_equal(got["slack_min_which"][which_ok], want["slack_min_which"][which_ok])
    assert np.array_equal(got["first_neg_tick"][first_ok], first[first_ok])
    assert ((got["neg_ticks"] >= lo) & (got["neg_ticks"] <= hi)).all() and (hi == lo).mean() >= 0.75
    assert np.array_equal((got["slack_trace"] < 0)[clear], (trace < 0)[clear])          # every decided tick, one by one
    own = wbc_workload.watch_summary(got["slack_trace"])                                # ... and the counters are the reduction of that trace
    for k in own:
        assert _same(own[k], got[k]), k
    G = B // M
    gmin = want["slack_min"].reshape(4, G, M).min(axis=2)
    assert np.abs(got["slack_group_min"] - gmin).max() <= tol
    g_ok = ((lo > 0) | (hi == 0)).reshape(4, G, M).all(axis=2)
    assert g_ok.mean() >= 0.75 and np.array_equal(got["slack_group_neg_instances"][g_ok], (lo > 0).reshape(4, G, M).sum(axis=2)[g_ok])
    # the crossing condition of test_long_horizon_host.py on the device's own trajectory
    assert any(4 * some[f].sum() >= B and (leaves[f][some[f]] >= 2).any() for f in range(4))


# ---- 5. the reverse sweep over a tape whose working set changes
# The smallest K at which half of the instances' sets differ between the first and the last tick is 2 on these inputs (measured on the oracle,
# the first tick's transient drops a bound at once), so the length is set by what the restatement costs on the CPU: 64 ticks,
# 32 where two runs of it would take more than ten seconds.
SWEEP_CASES = [("b5", "full", 64), ("b5", "everything", 64), ("mixed7", "full", 64), ("mixed7", "everything", 32)]
PARITY_BOUND = 1e-11      # the per-layer device bound (test_gpu_tick_grad / test_gpu_step_grad): the size of the perturbation below
MEANINGLESS = 1e-3


@pytest.mark.parametrize("shape,cfg_name,ticks", SWEEP_CASES)
def test_sweep_over_a_long_tape_against_the_restatement(shape, cfg_name, ticks):
    """rollout_vjp under warm_start 1 against wbc_workload.rollout_gradients fed the tape (test_gpu_rollout_vjp's _ticks_seen / _restate), seeds
    at q_K, at the last q̇ and at every traced state. The bound is measured on the REFERENCE, never on the device: the restatement runs twice on
    the same tape, once with q̇ and the states perturbed by a relative 1e-11; per block, ten times the largest difference relative to
    max(1, |block|) — one factor of ten for the K layers each adding its own error and for the perturbation being one sample."""
    import test_gpu_rollout_vjp as rv
    names, B = rv.SHAPES[shape]
    models, cfgs, d, mid = tgp._problem(names, cfg_name, B, seed=7, with_rot=True)
    step = rv._step(B, 4)
    rows = tgp._random_rows(tgp._rows_of(cfgs, mid, B), 12, w=(0.8, 1.25), g=(0.8, 1.25))
    nvs = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
    seeds = rv._seeds(B, ticks, 21, nvs)
    bt = tgp._handle(models, cfgs, B, {"warm_start": 1})
    try:
        rec, tape = bt.rollout_record(d, DT, ticks, ee_target_step=step, task_params=rows)
        got = bt.rollout_vjp(tape, **seeds)
        names_out = bt.default_rollout_grad_wants()
        seen = rv._ticks_seen(cfgs, d, tape, ticks, step)
    finally:
        bt.close()
    ws = np.stack([t["working_set"] for _, t in seen])
    solved = np.stack([t["status"] for _, t in seen]) == 0
    moved = (ws[0] != ws[-1]).any(axis=1) & solved[0] & solved[-1]
    distinct = [len({tuple(w) for w in ws[:, b]}) for b in range(B)]
    print("%s / %s, K = %d: the taped working set differs between the first and the last tick in %d / %d instances; distinct sets per instance %s" % (
        shape, cfg_name, ticks, moved.sum(), B, distinct))
    assert 2 * moved.sum() >= B
    ref = rv._restate(models, cfgs, mid, seen, seeds, rows=rows, warm=1)
    rng = np.random.default_rng(5)
    nudged = [(dict(cur, q=cur["q"] * (1 + PARITY_BOUND * rng.uniform(-1, 1, cur["q"].shape))),
               dict(t, qdot=t["qdot"] * (1 + PARITY_BOUND * rng.uniform(-1, 1, t["qdot"].shape)))) for cur, t in seen]
    ref2 = rv._restate(models, cfgs, mid, nudged, seeds, rows=rows, warm=1)
    assert np.array_equal(got["ticks_dropped"], ref["ticks_dropped"]), (got["ticks_dropped"], ref["ticks_dropped"])
    assert (got["ticks_dropped"] == 0).sum() >= B - B // 4
    failed = []
    for k in names_out:
        scale = max(1.0, np.abs(ref[k]).max())
        response, ratio = np.abs(ref2[k] - ref[k]).max() / scale, np.abs(got[k] - ref[k]).max() / scale
        print("%s / %s, K = %d: %-20s perturbation response %.3e, device %.3e (bound %.3e, margin x%.1f), max|ref| %.3e" % (
            shape, cfg_name, ticks, k, response, ratio, 10 * response, 10 * response / ratio if ratio > 0 else np.inf, np.abs(ref[k]).max()))
        assert response <= MEANINGLESS, "%s: the restatement's own response says the gradient means nothing at this length" % k
        if ratio > 10 * response:
            failed.append(k)
    assert not failed, failed
    assert np.abs(got["d_q0"]).max() > 0 and np.abs(got["d_ee_target_step"]).max() > 0
