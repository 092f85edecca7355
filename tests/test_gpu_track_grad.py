"""wbc_rollout_record_tracks / wbc_rollout_vjp_tracks on the device: the recorded forward against wbc_rollout_tracks (and wbc_rollout_traj) byte
for byte, the reverse sweep against the numpy restatement wbc_workload.rollout_gradients(tracks=...) fed the device's own taped states, qdot,
status and working sets, exact zeros and repeatable bits, bad rows among good ones under guarded device buffers, refusals, graph capture, the
torch layer wbc_rollout_tracks_fused, and the handle's state after tracks calls.

Three tracks everywhere (track_grad_common.three_tracks, S = 4): the gripper on a HERMITE track with default tangents, foot 0 on a LINEAR
track, the trunk on a HERMITE track with the caller's tangents; n_points 2..4 across the instances; du mixes interior ticks, exact knots,
tracks that clamp within the K ticks and one instance whose every tick is clamped.

The sweep is held by test_gpu_rollout_vjp.SWEEP_BOUND unchanged (1e-11 on `full`, 1e-8 on `everything`, every block relative to max(1,
max|ref block|)): the new blocks are combinations of the same cotangents with coefficients bounded by 3. Measured on MI355X (worst ratio per
case): b1 / full 2.5e-14, b5 / full (warm_start 1) 2.9e-14, b5 / everything 8.0e-11, mixed7 / everything 4.6e-11 (warm_start 0) and 3.7e-11
(warm_start 1): none above a thirtieth of its bound.

A tape is compared by the blocks a record writes (the padding word, the blocks of inputs the call did not have and, cold, the working sets
are never written, so two tapes of two allocations differ there)."""
import ctypes as C

import numpy as np
import pytest

import common
import gradq_common as gq
import oracle
import test_gpu_rollout_vjp as rv
import test_gpu_task_params as tgp
import test_step_grad_host as th
import test_tick_grad_q_host as tq
import track_grad_common as tg
import wbc_capi as capi
import wbc_workload

pytestmark = pytest.mark.gpu

DT = tq.DT
_same, _host, _dev = rv._same, rv._host, rv._dev
TRACK_NAMES = ("d_points", "d_tangents", "d_du")


def _setup(shape, cfg_name, K, seed=7):
    names, B = rv.SHAPES[shape]
    models, cfgs, d, mid = tgp._problem(names, cfg_name, B, seed=seed, with_rot=True)
    return models, cfgs, d, mid, B, tg.three_tracks(d, K, seed + 50)


def _taped(tape, warm=0):
    """what a record writes of every tick, on the host (the padding word, the blocks of inputs the call did not have and, cold, the working
    sets are never written: two tapes differ there)"""
    return [{k: _host(v) for k, v in tape.tick(k).items() if warm or k != "working_set"} for k in range(tape.ticks)]


def _same_tapes(a, b, warm=0):
    return all(set(x) == set(y) and all(_same(x[k], y[k]) for k in x) for x, y in zip(_taped(a, warm), _taped(b, warm)))


def _live(t):
    return (np.arange(tg.S)[None, :] < t["n_points"][:, None])[:, :, None]


# ---- 1. the forward
@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("shape,cfg_name,K", [("b1", "full", 3), ("b5", "everything", 4), ("mixed7", "everything", 3)])
def test_recorded_forward_is_the_tracks_rollout_byte_for_byte(shape, cfg_name, K, warm):
    models, cfgs, d, mid, B, tracks = _setup(shape, cfg_name, K)
    score = (4, "trunk")
    bt = tgp._handle(models, cfgs, B, {"warm_start": warm})
    plain = bt.rollout_tracks(d, DT, K, tracks, score=score)
    path = bt.stat("last_path")
    bt.close()
    bt = tgp._handle(models, cfgs, B, {"warm_start": warm})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=score)
    assert bt.stat("last_path") == path
    assert set(plain) <= set(rec) and set(rec) - set(plain) == {"q_trace"}
    for k in plain:
        assert _same(rec[k], plain[k]), "%s / %s / warm_start %d: %s differs from wbc_rollout_tracks'" % (shape, cfg_name, warm, k)
    assert _same(rec["q_trace"][K - 1], rec["q"]) and tape.buf.numel() == B * (capi.TAPE_HEAD_BYTES + K * capi.TAPE_TICK_BYTES)
    for k in range(K):                                                   # the tape holds the followed targets the tick saw
        seen = tg.follow(d, tracks, k)
        t = tape.tick(k)
        for tr in tracks:
            f = tg.target_index(tr)
            if f == tg.TRUNK:
                assert _same(_host(t["trunk_target"]), seen["trunk_target"])
            else:
                assert _same(_host(t["ee_target"]).reshape(B, 5, 3)[:, f], seen["ee_target"][:, f])
    bt.close()


def test_one_linear_track_is_the_trajectory_rollout():
    models, cfgs, d, mid, B, tracks = _setup("b5", "full", 4)
    t = dict(tracks[1], target=4)
    bt = tgp._handle(models, cfgs, B, {})
    plain = bt.rollout_traj(d, DT, 4, t["points"], n_points=t["n_points"], du=t["du"], ee_index=4)
    rec, tape = bt.rollout_record(d, DT, 4, tracks=[t], score=(4,))
    for k in ("q", "qdot", "ee_target", "status", "iters", "first_bad_tick", "bad_ticks"):
        assert _same(rec[k], plain[k]), k
    for k in ("err_sq_sum", "err_max", "err_final", "err_max_tick"):
        assert _same(rec[k].reshape(B), plain[k]), k
    bt.close()


# ---- 2. the sweep against the restatement
def _seen(cfgs, d, tape, K):
    return rv._ticks_seen(cfgs, d, tape, K, None)


def _restate(models, cfgs, mid, seen, seeds, tracks, rows=None, warm=0):
    """test_gpu_rollout_vjp._restate with tracks: per model, the tracks' rows of that model's instances"""
    K, B = len(seen), len(seen[0][0]["q"])
    out = None
    for i, (m, c) in enumerate(zip(models, cfgs)):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        if not sel.any():
            continue
        n = int(sel.sum())
        ins = [{k: v[sel] for k, v in cur.items() if k != "model_id"} for cur, _ in seen]
        sub = [{k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in tracks]
        ms, cs, pid = ([m], [c], None) if rows is None else common.per_instance_configs([m], [c], None, rows[sel])
        r = wbc_workload.rollout_gradients(
            m, c, ins, np.stack([t["qdot"][sel] for _, t in seen]), DT, gq.StateFK([m]),
            lambda dd, ms=ms, cs=cs, pid=pid, n=n: oracle.assemble(ms, cs, dd if pid is None else dict(dd, model_id=pid), DT, n),
            g_q_final=seeds["g_q_final"][sel], g_qdot_last=seeds["g_qdot_last"][sel], g_q_trace=seeds["g_q_trace"][:, sel],
            task_params=None if rows is None else rows[sel], status=np.stack([t["status"][sel] for _, t in seen]),
            working_set=np.stack([t["working_set"][sel] for _, t in seen]) if warm else None, tracks=sub)
        rt = r.pop("tracks")
        if out is None:
            out = {k: np.zeros((B,) + v.shape[1:], dtype=v.dtype) for k, v in r.items()}
            out["tracks"] = [{k: (None if v is None else np.zeros((B,) + v.shape[1:])) for k, v in t.items()} for t in rt]
        for k in r:
            out[k][sel] = r[k]
        for j, t in enumerate(rt):
            for k, v in t.items():
                if v is not None:
                    out["tracks"][j][k][sel] = v
    return out


def _main_names(bt, tracks):
    no = {"d_ee_target_step", "d_trunk_target_step"}
    return tuple(k for k in bt.default_rollout_grad_wants() if k not in no)


@pytest.mark.parametrize("shape,cfg_name,K,warm", [("b1", "full", 3, 0), ("b5", "full", 4, 1), ("b5", "everything", 4, 0), ("mixed7", "everything", 3, 0),
                                                   ("mixed7", "everything", 3, 1)])
def test_sweep_against_the_restatement(shape, cfg_name, K, warm):
    models, cfgs, d, mid, B, tracks = _setup(shape, cfg_name, K)
    rows = tgp._random_rows(tgp._rows_of(cfgs, mid, B), 12, w=(0.8, 1.25), g=(0.8, 1.25))
    nvs = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
    seeds = rv._seeds(B, K, 21, nvs)
    bt = tgp._handle(models, cfgs, B, {"warm_start": warm})
    rec, tape = bt.rollout_record(d, DT, K, task_params=rows, tracks=tracks)
    got = bt.rollout_vjp(tape, **seeds)
    assert bt.stat("last_trackvjp_variant") == 1 << 32 and bt.stat("last_rollvjp_variant") == 2 << 32     # variant_key(TICK), variant_key(LINK)
    names = _main_names(bt, tracks)
    assert set(got) == set(names) | {"grad_status", "ticks_dropped", "tracks"}
    assert [set(t) for t in got["tracks"]] == [{"d_points", "d_du"}, {"d_points", "d_du"}, set(TRACK_NAMES)]
    ref = _restate(models, cfgs, mid, _seen(cfgs, d, tape, K), seeds, tracks, rows=rows, warm=warm)
    assert np.array_equal(got["ticks_dropped"], ref["ticks_dropped"]) and (got["grad_status"] != capi.GRAD_NONFINITE).all()
    assert (got["ticks_dropped"] == 0).sum() >= B - B // 4
    worst = 0.0
    blocks = [(k, got[k], ref[k]) for k in names] + [("tracks[%d].%s" % (j, k), v, ref["tracks"][j][k]) for j, t in enumerate(got["tracks"]) for k, v in t.items()]
    for name, a, b in blocks:
        ratio = np.abs(a - b).max() / max(1.0, np.abs(b).max())
        worst = max(worst, ratio)
        print("%s / %s, K = %d: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e)" % (shape, cfg_name, K, name, ratio, np.abs(b).max()))
    print("%s / %s, K = %d, warm_start %d: worst ratio %.3e (bound %.0e), max|sens_x| over the ticks %.3e" % (
        shape, cfg_name, K, warm, worst, rv.SWEEP_BOUND[cfg_name], ref["sens_max"].max()))
    assert worst <= rv.SWEEP_BOUND[cfg_name]
    for j, t in enumerate(got["tracks"]):
        assert np.abs(t["d_points"]).max() > 0 and np.abs(t["d_du"]).max() > 0
    assert np.abs(got["tracks"][2]["d_tangents"]).max() > 0
    # the du of a track given as one number: the same bits per instance (the caller sums)
    if shape == "b1":
        one = [dict(t, du=float(t["du"][0])) for t in tracks]
        _, tape1 = bt.rollout_record(d, DT, K, task_params=rows, tracks=one)
        got1 = bt.rollout_vjp(tape1, **seeds)
        for j in range(3):
            assert _same(got1["tracks"][j]["d_du"], got["tracks"][j]["d_du"]) and _same(got1["tracks"][j]["d_points"], got["tracks"][j]["d_points"])
    bt.close()


# ---- 3. bits
def test_bits_and_exact_zeros():
    K = 4
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    nvs = np.array([m.nv for m in models])[mid]
    seeds = rv._seeds(B, K, 21, nvs)
    bt = tgp._handle(models, cfgs, B, {})
    _, tape = bt.rollout_record(d, DT, K, tracks=tracks)
    a = bt.rollout_vjp(tape, **seeds)
    _, tape2 = bt.rollout_record(d, DT, K, tracks=tracks)
    b = bt.rollout_vjp(tape2, **seeds)
    assert _same_tapes(tape, tape2)
    for k in a:
        if k != "tracks":
            assert _same(a[k], b[k]), k
    for j, t in enumerate(tracks):
        for k, v in a["tracks"][j].items():
            assert _same(v, b["tracks"][j][k]), (j, k)
        f = tg.target_index(t)
        followed = a["d_trunk_target"] if f == tg.TRUNK else a["d_ee_target"][:, f]
        assert not followed.view(np.uint64).any()                        # exactly 0, not -0
        dead = np.broadcast_to(~_live(t), (B, tg.S, 3))
        assert not a["tracks"][j]["d_points"][dead].view(np.uint64).any()
        if "d_tangents" in a["tracks"][j]:
            assert not a["tracks"][j]["d_tangents"][dead].view(np.uint64).any()
    assert np.abs(a["d_ee_target"][:, 1:4]).max() > 0                     # the rows no track follows keep their gradient
    assert tracks[0]["du"][1] * 1 >= tracks[0]["n_points"][1] - 1 and a["ticks_dropped"][1] == 0      # the gripper track of instance 1: every tick clamped
    assert a["tracks"][0]["d_du"].view(np.uint64)[1] == 0 and np.abs(a["tracks"][0]["d_points"][1]).max() > 0
    # only some outputs: the same bits
    only = bt.rollout_vjp(tape, want=("d_q0", "d_du"), **seeds)
    assert set(only) == {"d_q0", "grad_status", "ticks_dropped", "tracks"} and all(set(t) == {"d_du"} for t in only["tracks"])
    assert _same(only["d_q0"], a["d_q0"]) and all(_same(only["tracks"][j]["d_du"], a["tracks"][j]["d_du"]) for j in range(3))
    bt.close()


# ---- 4. bad rows among good ones, guarded device buffers in place
def test_bad_rows_among_good_ones_under_guards():
    """B = 7 over the three models: instance 1 has a NaN milestone (gripper track), instance 3 du <= 0 (foot track), instance 5 n_points = 1
    (trunk track). Device pointers in place, pattern guard rows around every output, NaN guard rows around every float input. The guards
    come back intact, the inputs byte for byte; the bad instances get all-zero rows in every output and WBC_GRAD_NONFINITE; the others are
    bit-identical to the call without bad rows"""
    import torch
    import devguard as dg
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    names, _ = rv.SHAPES["mixed7"]
    _, _, o, _ = tgp._problem(names, "everything", 2 * dg.G, seed=9, with_rot=True)
    o["model_id"] = np.zeros(2 * dg.G, np.int32)
    nvs = np.array([m.nv for m in models])[mid]
    seeds = rv._seeds(B, K, 21, nvs)
    bt = tgp._handle(models, cfgs, B, {})
    _, tape = bt.rollout_record(d, DT, K, tracks=tracks)
    good = bt.rollout_vjp(tape, **seeds)
    bad_rows, ok = [1, 3, 5], np.array([0, 2, 4, 6])                    # (instance 2 of this batch goes unsolved: dropped ticks, the same bits)
    assert (good["grad_status"] != capi.GRAD_NONFINITE).all() and (good["ticks_dropped"][[0, 4, 6]] == 0).all()
    bad = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in tracks]
    bad[0]["points"][1, 1, 2] = np.nan
    bad[1]["du"][3] = -0.25
    bad[2]["n_points"][5] = 1
    stream = torch.cuda.Stream()
    sess = dg.Session("nan", stream)
    dev = sess.put_all(d, o)
    g_final = sess.put("g_q_final", seeds["g_q_final"], o["q"][:, :26])
    g_last = sess.put("g_qdot_last", seeds["g_qdot_last"], o["q"][:, :26])
    g_trace = torch.from_numpy(seeds["g_q_trace"]).cuda()
    dev_tracks = []
    for j, t in enumerate(bad):
        dt_ = dict(t, points=sess.put("points%d" % j, t["points"], None), du=sess.put("du%d" % j, t["du"], None),
                   n_points=sess.put("n_points%d" % j, t["n_points"], np.full(2 * dg.G, 4, np.int32)))
        if "tangents" in t:
            dt_["tangents"] = sess.put("tangents%d" % j, t["tangents"], None)
        dev_tracks.append(dt_)
    main = _main_names(bt, tracks)
    out = {k: sess.out((B,) + capi.ROLLOUT_GRAD_FIELDS[k]) for k in main}
    out["grad_status"], out["ticks_dropped"] = sess.out((B,), np.int32), sess.out((B,), np.int32)
    out["tracks"] = [{k: sess.out((B, tg.S, 3) if k != "d_du" else (B,)) for k in good["tracks"][j]} for j in range(3)]
    bt.allocator = sess.alloc

    def call():
        r, tp = bt.rollout_record(dev, DT, K, want_trace=False, tracks=dev_tracks)
        bt.rollout_vjp(tp, g_q_final=g_final, g_qdot_last=g_last, g_q_trace=g_trace, out=out)
        return r
    sess.run(call)
    bt.allocator = None
    sess.check("rollout_record + rollout_vjp along tracks")
    res = dg.to_host({k: v for k, v in out.items() if k != "tracks"})
    res_tracks = [dg.to_host(t) for t in out["tracks"]]
    expect = good["grad_status"].copy()
    expect[bad_rows] = capi.GRAD_NONFINITE
    assert np.array_equal(res["grad_status"], expect), res["grad_status"]
    for k in main:
        assert not res[k][bad_rows].view(np.uint64).any(), k
        assert _same(res[k][ok], good[k][ok]), k
    for j in range(3):
        for k, v in res_tracks[j].items():
            assert not v[bad_rows].view(np.uint64).any(), (j, k)
            assert _same(v[ok], good["tracks"][j][k][ok]), (j, k)
    bt.close()


# ---- 5. refusals
def test_refusals_name_their_field_and_come_before_any_launch():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("b5", "full", K)
    bt = tgp._handle(models, cfgs, B, {})
    _, tape = bt.rollout_record(d, DT, K, tracks=tracks)
    g = np.ones((B, 26))
    before = _host(tape.buf)

    def refused(fn, word, code=capi.E_ARG):
        with pytest.raises(capi.WbcError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), (word, str(e.value))

    def outs(**more):
        return dict(dict(d_q0=np.full((B, 26), 7.0), grad_status=np.full(B, 7, np.int32), tracks=[dict(d_du=np.full(B, 7.0)), {}, {}]), **more)

    def untouched(o):
        assert (o["d_q0"] == 7.0).all() and (o["grad_status"] == 7).all() and (o["tracks"][0]["d_du"] == 7.0).all()
    o = outs(d_ee_target_step=np.zeros((B, 5, 3)))
    refused(lambda: bt.rollout_vjp(tape, g_q_final=g, out=o), "d_ee_target_step")
    untouched(o)
    o = outs(d_trunk_target_step=np.zeros((B, 3)))
    refused(lambda: bt.rollout_vjp(tape, g_q_final=g, out=o), "d_trunk_target_step")
    untouched(o)
    for j in (0, 1):                                                     # HERMITE with default tangents; LINEAR
        o = outs()
        o["tracks"][j] = dict(o["tracks"][j], d_tangents=np.zeros((B, tg.S, 3)))
        refused(lambda: bt.rollout_vjp(tape, g_q_final=g, out=o), "d_tangents")
        untouched(o)
    refused(lambda: bt.rollout_vjp(tape, out=outs()), "seed")
    # the C ABI itself: tracks_out NULL, tracks NULL, a member set beyond n_tracks
    keep = []
    tin = bt._tick_in(d, keep, B)
    tk, _ = bt._tracks_struct(tracks, B, keep)
    r = capi.WbcRollout()
    r.ticks, r.mode, r.hold_ticks = K, capi.ROLLOUT_RUNNING, 0
    sd, og, tgr = capi.WbcRolloutSeed(), capi.WbcRolloutGrad(), capi.WbcTracksGrad()
    sd.g_q_final = g.ctypes.data
    dq0 = np.full((B, 26), 7.0)
    og.d_q0 = dq0.ctypes.data

    def vjp(tracks_p=C.byref(tk), out_p=C.byref(tgr), rr=r):
        capi.check(bt.lib.wbc_rollout_vjp_tracks(bt._h, B, C.byref(tin), None, DT, C.byref(rr), tracks_p, tape.buf.data_ptr(), tape.buf.numel(),
                                                 C.byref(sd), capi.MEM_HOST, C.byref(og), out_p, None), bt.lib)
    refused(lambda: vjp(out_p=None), "tracks_out")
    refused(lambda: vjp(tracks_p=None), "tracks")
    stray = np.full(B, 7.0)
    tgr.track[4].d_du = stray.ctypes.data
    refused(vjp, "track[4]")
    tgr.track[4].d_du = None
    two = capi.WbcTracks()
    C.memmove(C.byref(two), C.byref(tk), C.sizeof(tk))
    two.track[1].target = two.track[0].target
    refused(lambda: vjp(tracks_p=C.byref(two)), "repeated")              # the tracks call's own
    held = capi.WbcRollout()
    held.ticks, held.mode, held.hold_ticks = K, capi.ROLLOUT_RUNNING, 2
    refused(lambda: vjp(rr=held), "hold_ticks")
    assert (dq0 == 7.0).all() and (stray == 7.0).all()

    def record(tracks_p=C.byref(tk), ptr=tape.buf.data_ptr(), n=tape.buf.numel(), rr=r):
        capi.check(bt.lib.wbc_rollout_record_tracks(bt._h, B, C.byref(tin), None, DT, C.byref(rr), tracks_p, None, ptr, n, None, capi.MEM_HOST, None), bt.lib)
    refused(lambda: record(tracks_p=None), "tracks")
    refused(lambda: record(ptr=None), "tape")
    refused(lambda: record(n=tape.buf.numel() - 1), "tape_bytes")
    refused(lambda: record(rr=held), "hold_ticks")
    refused(lambda: bt.rollout_record(d, DT, K, tracks=tracks, ee_target_step=np.zeros((B, 5, 3))), "ee_target_step")
    refused(lambda: bt.rollout_record(dict(d, q_con=d["q"]), DT, K, tracks=tracks), "q_con")
    refused(lambda: bt.rollout_record(d, DT, K, tracks=[dict(tracks[2])], trunk_target_step=np.zeros((B, 3))), "trunk_target_step")
    bt.synchronize()
    assert _same(_host(tape.buf), before)                                # nothing was launched
    # trunk_target_step without a trunk track stays allowed, and d_trunk_target_step is then the plain sweep's
    step = np.random.default_rng(3).normal(0, 2e-4, (B, 3))
    _, tp2 = bt.rollout_record(d, DT, K, tracks=tracks[:2], trunk_target_step=step)
    got = bt.rollout_vjp(tp2, g_q_final=g)
    assert "d_trunk_target_step" in got and np.abs(got["d_trunk_target_step"]).max() > 0 and np.abs(got["d_trunk_target"]).max() > 0
    assert bt.lib.wbc_variant_count(b"trackvjp") == 2 and bt.lib.wbc_variant_count(b"rollvjp") == 3
    bt.close()


# ---- 6. capture and replay
def test_capture_and_replay_give_the_same_bits():
    import torch
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    nvs = np.array([m.nv for m in models])[mid]
    seeds = rv._seeds(B, K, 21, nvs)
    bt = tgp._handle(models, cfgs, B, {})
    rec0, tape0 = bt.rollout_record(d, DT, K, tracks=tracks)
    host = bt.rollout_vjp(tape0, **seeds)
    dev, sd = _dev(d), _dev(seeds)
    dev_tracks = [{k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in tracks]
    out = {k: torch.empty((B,) + capi.ROLLOUT_GRAD_FIELDS[k], dtype=torch.float64, device="cuda") for k in _main_names(bt, tracks)}
    out["grad_status"], out["ticks_dropped"] = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    out["tracks"] = [{k: torch.empty(v.shape, dtype=torch.float64, device="cuda") for k, v in t.items()} for t in host["tracks"]]
    flat = [(k, v) for k, v in out.items() if k != "tracks"] + [("tracks[%d].%s" % (j, k), v) for j, t in enumerate(out["tracks"]) for k, v in t.items()]
    ref = dict([(k, v) for k, v in host.items() if k != "tracks"] + [("tracks[%d].%s" % (j, k), v) for j, t in enumerate(host["tracks"]) for k, v in t.items()])
    state = {}

    def call():
        state["rec"], state["tape"] = bt.rollout_record(dev, DT, K, tape=state.get("tape"), tracks=dev_tracks)
        bt.rollout_vjp(state["tape"], out=out, **sd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                           # (warm-up outside the capture: the workspaces get their size)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first = {k: _host(v) for k, v in flat}
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        call()
    for _, v in flat:
        v.fill_(3)
    state["tape"].buf.fill_(0)
    gr.replay()
    torch.cuda.synchronize()
    for k, v in flat:
        assert _same(_host(v), first[k]) and _same(first[k], ref[k]), k
    assert _same(_host(state["rec"]["q"]), rec0["q"]) and np.abs(first["tracks[0].d_points"]).max() > 0
    bt.close()


# ---- 7. the torch layer
def _dev_tracks(tracks):
    import torch
    return [{k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in tracks]


def _fused(bt, dev, dev_tracks, K, rho):
    """-> (q_K, status, d_q0 raw, per track dict(points, tangents, du) gradients) of the loss rho . q_K through wbc_rollout_tracks_fused"""
    import torch
    import wbc_torch
    q0 = dev["q"].clone().requires_grad_(True)
    tt = [{k: (v.clone().requires_grad_(True) if k in ("points", "tangents", "du") else v) for k, v in t.items()} for t in dev_tracks]
    q, qdot, st, trace = wbc_torch.wbc_rollout_tracks_fused(q0, None, tt, {k: v for k, v in dev.items() if k != "q"}, DT, K, bt)
    (q * torch.from_numpy(rho).cuda()).sum().backward()
    grads = [{k: _host(n[k].grad) for k in ("points", "tangents", "du") if k in n} for n in tt]
    return _host(q.detach()), _host(st), _host(q0.grad), grads


def test_fused_backward_is_the_sweep_bit_for_bit():
    import torch
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("b5", "everything", K)
    rho = np.random.default_rng(33).normal(0, 1.0, (B, 27))
    bt = tgp._handle(models, cfgs, B, {})
    dev, dev_tracks = _dev(d), _dev_tracks(tracks)
    q, st, g_q0, grads = _fused(bt, dev, dev_tracks, K, rho)
    rec, tape = bt.rollout_record(dev, DT, K, tracks=dev_tracks)
    assert _same(q, _host(rec["q"]))
    seed = wbc_workload.raw_to_tangent(rec["q"], torch.from_numpy(rho).cuda()).contiguous()      # what the layer's backward does
    ref = bt.rollout_vjp(tape, g_q_final=seed, want=("d_q0",) + TRACK_NAMES)
    assert _same(g_q0, _host(wbc_workload.tangent_to_raw(dev["q"], ref["d_q0"])))
    for j in range(3):
        assert set(grads[j]) == {"points", "du"} | ({"tangents"} if "tangents" in tracks[j] else set())
        for k, v in grads[j].items():
            assert _same(v, _host(ref["tracks"][j]["d_" + k])), (j, k)
            assert np.abs(v).max() > 0
    bt.close()


@pytest.mark.parametrize("cfg_name,seed", [("full", 3)])
def test_fused_backward_against_central_differences_of_the_oracle_chain(cfg_name, seed):
    """the host test's item 4 with the device's gradients: the same inputs, tracks, directions, rule and cap"""
    m, cfg, d, rho, _ = th.sweep_setup(cfg_name, seed)
    K, B = th.K_TICKS, len(rho)
    tracks = tg.three_tracks(d, K, seed + 50, generic=True)
    states, ticks, sides0, status = tg.track_chain(m, cfg, d, K, DT, tracks)
    assert all((s == 0).all() for s in status)
    margin, kappa = tg.margins(m, cfg, states, ticks, K)
    bt = tgp._handle([m], [cfg], B, {})
    q, st, g_q0, g = _fused(bt, _dev(d), _dev_tracks(tracks), K, rho)
    bt.close()
    assert (st == 0).all()
    dP, dV, dU = tg.directions(tracks, seed + 9)
    zero, zu = [np.zeros_like(x) for x in dP], [np.zeros(B) for _ in dU]
    cases = (("d_points", dP, zero, zu, sum((g[j]["points"] * dP[j]).sum(axis=(1, 2)) for j in range(3)),
              sum(np.abs(g[j]["points"] * dP[j]).sum(axis=(1, 2)) for j in range(3))),
             ("d_tangents", zero, dV, zu, (g[2]["tangents"] * dV[2]).sum(axis=(1, 2)), np.abs(g[2]["tangents"] * dV[2]).sum(axis=(1, 2))),
             ("d_du", zero, zero, dU, sum(g[j]["du"] * dU[j] for j in range(3)), sum(np.abs(g[j]["du"] * dU[j]) for j in range(3))))
    for name, p_, v_, u_, ana, terms in cases:
        keep, ok, line = tg.track_chain_directional(m, cfg, d, rho, K, DT, lambda s: tg.perturbed(tracks, s, p_, v_, u_), sides0, margin, kappa,
                                                    ana, terms, "%s / seed %d, K = %d, fused, %s" % (cfg_name, seed, K, name))
        print(line)
        assert (~keep).sum() <= B // 4 and ok, line


# ---- 8. handle state
def test_a_plain_pair_after_tracks_calls_gives_the_bits_of_a_fresh_handle():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    nvs = np.array([m.nv for m in models])[mid]
    seeds = rv._seeds(B, K, 21, nvs)
    step = rv._step(B, 4)
    bt = tgp._handle(models, cfgs, B, {})
    rec0, tape0 = bt.rollout_record(d, DT, K, ee_target_step=step)
    fresh = bt.rollout_vjp(tape0, **seeds)
    bt.close()
    bt = tgp._handle(models, cfgs, B, {})
    _, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=(4,))
    bt.rollout_vjp(tape, **seeds)
    rec1, tape1 = bt.rollout_record(d, DT, K, ee_target_step=step)
    after = bt.rollout_vjp(tape1, **seeds)
    assert _same_tapes(tape1, tape0)
    for k in rec0:
        assert _same(rec1[k], rec0[k]), k
    assert set(after) == set(fresh)
    for k in fresh:
        assert _same(after[k], fresh[k]), k
    bt.close()
