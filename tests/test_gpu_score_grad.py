"""wbc_rollout_vjp_scored on the device: the track scores err_sq_sum / err_final / err_max as a loss, their cotangents formed where the sweep
runs (wbc_scorevjp_kernel). Three tracks everywhere (track_grad_common.three_tracks: gripper, foot 0, trunk); scored: foot 1 (constant
target), the gripper (followed) and the trunk (followed, or stepped where the test says so). Shapes: test_gpu_rollout_vjp.SHAPES' b1, b5 and
mixed7 (three models, the Laikago + ViperX-300 among them: the ROT row) and laikago5 (that robot alone, B = 5: a wave of one instance).

  1. the cross-check      the scored call with a score seed alone against wbc_rollout_vjp_tracks with a HOST-BUILT g_q_trace (the rows J_f' c
                          of wbc_workload.score_seed_gradients at the taped states): the blocks no target cotangent reaches agree within
                          SWEEP_BOUND, the target blocks differ by the closed forms of include/wbc.h (- sum c_k, - sum k c_k, the track adjoint of -c_k)
  2. the restatement      every block against rollout_gradients(score_seed=...); each score alone, all together, with and without a state
                          seed; both seeds = the sum of each
  3. bits                 identical calls, capture and replay
  4. exact zeros          a mask with one bit is that frame alone; all-zero cotangents with a state seed give wbc_rollout_vjp_tracks' bits
  5. bad rows             non-finite cotangent, non-finite q_final, err_max_tick out of range, under guarded device buffers
  6. refusals             each names its field and comes before any launch
  7. the handle           a plain wbc_rollout_vjp_tracks call after scored calls gives the bits of a fresh handle
  8. torch                wbc_rollout_tracks_scored: the scores byte for byte, the backward bit for bit, err_sq_sum.sum() against central
                          differences of the oracle chain (test_score_grad_host's item 3 with the device's gradients)

SWEEP_BOUND is test_gpu_rollout_vjp's, unchanged (1e-11 `full`, 1e-8 `everything`, relative to max(1, max|block|)): the score stage adds
J' c with |J| <= 1 m and |c| <= 5 |gamma| e to the same cotangents. Measured on MI355X (worst ratio per case). Cross-check: b1 / full
4.4e-15, b5 / everything 3.8e-15, mixed7 / everything 2.4e-14, laikago5 / full 4.1e-15; the stepped trunk target 4.9e-15. Restatement,
all three scores, without / with a state seed: b1 / full 2.8e-14 / 3.2e-14, b5 / everything 4.7e-14 / 5.2e-11, mixed7 / everything
1.7e-13 / 4.9e-11, laikago5 / full 2.4e-14 / 2.3e-14; on b5 / full err_sq_sum alone 3.8e-15, err_final alone 2.0e-14, err_max alone 2.0e-14:
none above a hundredth of its bound (the state seed's own error on `everything` is the largest term, as in test_gpu_track_grad)."""
import ctypes as C

import numpy as np
import pytest

import common
import gradq_common as gq
import oracle
import test_gpu_rollout_vjp as rv
import test_gpu_task_params as tgp
import test_gpu_track_grad as tt
import test_score_grad_host as sh
import test_tick_grad_q_host as tq
import track_grad_common as tg
import wbc_capi as capi
import wbc_workload

pytestmark = pytest.mark.gpu

DT = tq.DT
_same, _host, _dev = rv._same, rv._host, rv._dev
SHAPES = dict(rv.SHAPES, laikago5=(["laikago_vx300"], 5))
SCORE = (1, 4, "trunk")
FRAMES = (1, 4, capi.TARGET_TRUNK)
MASK = sum(1 << f for f in FRAMES)
KEY_SEED = {False: 0, True: 1 << 24}                                      # variant_key(SCOREVJP_SEED, ROT): the row a batch without / with a rotated placement runs
ROTATED = {"b1": False, "b5": False, "mixed7": True, "laikago5": True}
STATE_BLOCKS = ("d_q0", "d_task_params", "d_com_target", "d_com_target_vel", "d_posture_u", "d_trunk_box_center")


def _setup(shape, cfg_name, K, seed=7):
    names, B = SHAPES[shape]
    models, cfgs, d, mid = tgp._problem(names, cfg_name, B, seed=seed, with_rot=True)
    return models, cfgs, d, mid, B, tg.three_tracks(d, K, seed + 50)


def _gammas(B, seed, n=len(FRAMES)):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 1.0, (n, B)) for _ in range(3)]


def _seed_of(rec, gam, which=(0, 1, 2)):
    names = ("g_err_sq_sum", "g_err_final", "g_err_max")
    s = dict(mask=MASK, q_final=rec["q"], err_max_tick=rec["err_max_tick"] if 2 in which else None)
    s.update({n: (gam[i] if i in which else None) for i, n in enumerate(names)})
    return s


def _score_rows(models, mid, seen, q_final, seed):
    """wbc_workload.score_seed_gradients on the device's own states, per model -> (g_q_trace [K, B, 26], c [K, B, 6, 3])"""
    K, B = len(seen), len(q_final)
    g, c = np.zeros((K, B, 26)), np.zeros((K, B, 6, 3))
    q_after = np.stack([seen[k + 1][0]["q"] for k in range(K - 1)] + [q_final])
    for i, m in enumerate(models):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        if not sel.any():
            continue
        sub = lambda a: None if a is None else np.asarray(a)[:, sel]      # noqa: E731
        r = wbc_workload.score_seed_gradients(m, q_after[:, sel], [s[0]["ee_target"][sel] for s in seen], [s[0]["trunk_target"][sel] for s in seen],
                                              gq.StateFK([m]), seed["mask"], sub(seed["g_err_sq_sum"]), sub(seed["g_err_final"]),
                                              sub(seed["g_err_max"]), sub(seed["err_max_tick"]))
        g[:, sel], c[:, sel] = r["g_q_trace"], r["c"]
    return g, c


def _restate(models, cfgs, mid, seen, seeds, tracks, seed, warm=0):
    """test_gpu_track_grad._restate with a score seed (and state seeds or none): per model, the rows of that model's instances"""
    K, B = len(seen), len(seen[0][0]["q"])
    out = None
    for i, (m, c) in enumerate(zip(models, cfgs)):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        if not sel.any():
            continue
        n = int(sel.sum())
        ins = [{k: v[sel] for k, v in cur.items() if k != "model_id"} for cur, _ in seen]
        sub = [{k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in tracks]
        sd = {k: (None if v is None else v if k == "mask" else v[sel] if k == "q_final" else np.asarray(v)[:, sel]) for k, v in seed.items()}
        st = {} if seeds is None else dict(g_q_final=seeds["g_q_final"][sel], g_qdot_last=seeds["g_qdot_last"][sel], g_q_trace=seeds["g_q_trace"][:, sel])
        r = wbc_workload.rollout_gradients(m, c, ins, np.stack([t["qdot"][sel] for _, t in seen]), DT, gq.StateFK([m]),
                                           lambda dd, m=m, c=c, n=n: oracle.assemble([m], [c], dd, DT, n),
                                           status=np.stack([t["status"][sel] for _, t in seen]),
                                           working_set=np.stack([t["working_set"][sel] for _, t in seen]) if warm else None, tracks=sub,
                                           score_seed=sd, **st)
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


def _blocks(got, ref, names):
    return [(k, got[k], ref[k]) for k in names] + [("tracks[%d].%s" % (j, k), v, ref["tracks"][j][k]) for j, t in enumerate(got["tracks"]) for k, v in t.items()]


def _worst(blocks, what):
    worst = 0.0
    for name, a, b in blocks:
        ratio = np.abs(a - b).max() / max(1.0, np.abs(b).max())
        worst = max(worst, ratio)
        print("%s: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e)" % (what, name, ratio, np.abs(b).max()))
    return worst


CASES = [("b1", "full", 3), ("b5", "everything", 4), ("mixed7", "everything", 3), ("laikago5", "full", 3)]


# ---- 1. the cross-check against the existing sweep
@pytest.mark.parametrize("shape,cfg_name,K", CASES)
def test_score_seed_alone_is_the_tracks_sweep_with_a_host_built_trace(shape, cfg_name, K):
    models, cfgs, d, mid, B, tracks = _setup(shape, cfg_name, K)
    gam = _gammas(B, 31)
    bt = tgp._handle(models, cfgs, B, {})
    assert bt.stat("last_scorevjp_variant") == -1
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    seed = _seed_of(rec, gam)
    got = bt.rollout_vjp(tape, score_seed=seed)
    assert bt.stat("last_scorevjp_variant") == KEY_SEED[ROTATED[shape]] and bt.stat("last_trackvjp_variant") == 1 << 32
    seen = tt._seen(cfgs, d, tape, K)
    g_trace, c = _score_rows(models, mid, seen, rec["q"], seed)
    assert np.abs(g_trace).max() > 0 and np.abs(c[:, :, FRAMES]).min() > 0 and not np.delete(c, FRAMES, axis=2).any()
    plain = bt.rollout_vjp(tape, g_q_trace=g_trace)
    assert set(got) == set(plain) and np.array_equal(got["ticks_dropped"], plain["ticks_dropped"]) and np.array_equal(got["grad_status"], plain["grad_status"])
    what = "%s / %s, K = %d, cross-check" % (shape, cfg_name, K)
    names = tt._main_names(bt, tracks)
    blocks = [(k, got[k], plain[k]) for k in names if k in STATE_BLOCKS or k.startswith("d_prev")]
    assert {"d_q0", "d_task_params"} <= {b[0] for b in blocks}
    # the target blocks: the plain sweep's plus the closed forms
    ee = plain["d_ee_target"].copy()
    ee[:, 1] -= c[:, :, 1].sum(axis=0)                                   # foot 1: a constant target no track follows
    blocks.append(("d_ee_target", got["d_ee_target"], ee))
    for j, t in enumerate(tracks):
        f = tg.target_index(t)
        adj = wbc_workload.track_target_gradients(t["points"], t.get("n_points"), t["du"], K, t.get("kind", "linear"), t.get("tangents"), -c[:, :, f])
        for name, a in zip(tt.TRACK_NAMES, adj):
            if name in got["tracks"][j]:
                blocks.append(("tracks[%d].%s" % (j, name), got["tracks"][j][name], plain["tracks"][j][name] + a))
    worst = _worst(blocks, what)
    print("%s: worst ratio %.3e (bound %.0e)" % (what, worst, rv.SWEEP_BOUND[cfg_name]))
    assert worst <= rv.SWEEP_BOUND[cfg_name]
    assert not got["d_ee_target"][:, [0, 4]].view(np.uint64).any() and not got["d_trunk_target"].view(np.uint64).any()      # the followed rows carry nothing
    assert np.abs(got["tracks"][0]["d_points"] - plain["tracks"][0]["d_points"]).max() > 0
    bt.close()


def test_a_stepped_trunk_target_takes_the_sums_of_c():
    """no trunk track, trunk_target_step, the trunk scored: d_trunk_target takes - sum_k c_k and d_trunk_target_step - sum_k k c_k"""
    K = 4
    models, cfgs, d, mid, B, tracks = _setup("b5", "everything", K)
    step = np.random.default_rng(3).normal(0, 2e-4, (B, 3))
    gam = _gammas(B, 32)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks[:2], score=SCORE, trunk_target_step=step)
    seed = _seed_of(rec, gam)
    got = bt.rollout_vjp(tape, score_seed=seed)
    seen = tt._seen(cfgs, d, tape, K)
    for k in range(K):                                                   # the tape holds the stepped target the tick saw
        assert np.abs(seen[k][0]["trunk_target"] - (d["trunk_target"] + k * step)).max() <= 4 * np.finfo(float).eps
    g_trace, c = _score_rows(models, mid, seen, rec["q"], seed)
    plain = bt.rollout_vjp(tape, g_q_trace=g_trace)
    assert "d_trunk_target_step" in got and "d_trunk_target" in got
    ct = c[:, :, capi.TARGET_TRUNK]
    blocks = [("d_trunk_target", got["d_trunk_target"], plain["d_trunk_target"] - ct.sum(axis=0)),
              ("d_trunk_target_step", got["d_trunk_target_step"], plain["d_trunk_target_step"] - (np.arange(K)[:, None, None] * ct).sum(axis=0)),
              ("d_q0", got["d_q0"], plain["d_q0"])]
    worst = _worst(blocks, "b5 / everything, K = 4, stepped trunk target")
    assert worst <= rv.SWEEP_BOUND["everything"] and np.abs(ct[1:]).min() > 0
    bt.close()


# ---- 2. the sweep against the full restatement
@pytest.mark.parametrize("shape,cfg_name,K", CASES)
def test_scored_sweep_against_the_restatement(shape, cfg_name, K):
    models, cfgs, d, mid, B, tracks = _setup(shape, cfg_name, K)
    nvs = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
    seeds, gam = rv._seeds(B, K, 21, nvs), _gammas(B, 31)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    seed = _seed_of(rec, gam)
    seen = tt._seen(cfgs, d, tape, K)
    names = tt._main_names(bt, tracks)
    for state in (None, seeds):
        got = bt.rollout_vjp(tape, score_seed=seed, **(state or {}))
        ref = _restate(models, cfgs, mid, seen, state, tracks, seed)
        assert np.array_equal(got["ticks_dropped"], ref["ticks_dropped"]) and (got["grad_status"] != capi.GRAD_NONFINITE).all()
        what = "%s / %s, K = %d, all three scores%s" % (shape, cfg_name, K, " + state seed" if state else "")
        worst = _worst(_blocks(got, ref, names), what)
        print("%s: worst ratio %.3e (bound %.0e)" % (what, worst, rv.SWEEP_BOUND[cfg_name]))
        assert worst <= rv.SWEEP_BOUND[cfg_name]
        assert all(np.abs(t["d_points"]).max() > 0 for t in got["tracks"])
    bt.close()


def test_each_score_alone_and_the_sum_of_the_seeds():
    K, shape, cfg_name = 3, "b5", "full"
    models, cfgs, d, mid, B, tracks = _setup(shape, cfg_name, K)
    seeds, gam = rv._seeds(B, K, 21, np.full(B, models[0].nv)), _gammas(B, 31)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    seen = tt._seen(cfgs, d, tape, K)
    names = tt._main_names(bt, tracks)
    alone = []
    for i, label in enumerate(("err_sq_sum", "err_final", "err_max")):
        seed = _seed_of(rec, gam, which=(i,))
        got = bt.rollout_vjp(tape, score_seed=seed)
        ref = _restate(models, cfgs, mid, seen, None, tracks, seed)
        worst = _worst(_blocks(got, ref, names), "%s / %s, K = %d, %s alone" % (shape, cfg_name, K, label))
        print("%s alone: worst ratio %.3e (bound %.0e)" % (label, worst, rv.SWEEP_BOUND[cfg_name]))
        assert worst <= rv.SWEEP_BOUND[cfg_name] and np.abs(got["d_q0"]).max() > 0
        alone.append(got)
    # linearity: the three together = their sum; both seeds = the sum of each
    allg = bt.rollout_vjp(tape, score_seed=_seed_of(rec, gam))
    state = bt.rollout_vjp(tape, **seeds)
    both = bt.rollout_vjp(tape, score_seed=_seed_of(rec, gam), **seeds)
    add = lambda rs: dict({k: sum(r[k] for r in rs) for k in names},      # noqa: E731
                          tracks=[{k: sum(r["tracks"][j][k] for r in rs) for k in rs[0]["tracks"][j]} for j in range(3)])
    for what, got, ref in (("three scores = the sum of each", allg, add(alone)), ("both seeds = the sum of each", both, add([allg, state]))):
        worst = _worst(_blocks(got, ref, names), what)
        assert worst <= rv.SWEEP_BOUND[cfg_name], what
    bt.close()


# ---- 3. bits
def test_identical_calls_give_identical_bits():
    K = 4
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    seeds, gam = rv._seeds(B, K, 21, np.array([m.nv for m in models])[mid]), _gammas(B, 31)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    a = bt.rollout_vjp(tape, score_seed=_seed_of(rec, gam), **seeds)
    rec2, tape2 = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    b = bt.rollout_vjp(tape2, score_seed=_seed_of(rec2, gam), **seeds)
    for name, x, y in _blocks(a, b, [k for k in a if k != "tracks"]):
        assert _same(x, y), name
    only = bt.rollout_vjp(tape, score_seed=_seed_of(rec, gam), want=("d_q0", "d_du"), **seeds)      # only some outputs: the same bits
    assert _same(only["d_q0"], a["d_q0"]) and all(_same(only["tracks"][j]["d_du"], a["tracks"][j]["d_du"]) for j in range(3))
    bt.close()


def test_capture_and_replay_give_the_same_bits():
    import torch
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    gam = _gammas(B, 31)
    bt = tgp._handle(models, cfgs, B, {})
    rec0, tape0 = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    host = bt.rollout_vjp(tape0, score_seed=_seed_of(rec0, gam))
    dev, dev_tracks = _dev(d), tt._dev_tracks(tracks)
    dgam = [torch.from_numpy(g).cuda() for g in gam]
    out = {k: torch.empty((B,) + capi.ROLLOUT_GRAD_FIELDS[k], dtype=torch.float64, device="cuda") for k in tt._main_names(bt, tracks)}
    out["grad_status"], out["ticks_dropped"] = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    out["tracks"] = [{k: torch.empty(v.shape, dtype=torch.float64, device="cuda") for k, v in t.items()} for t in host["tracks"]]
    flat = [(k, v) for k, v in out.items() if k != "tracks"] + [("tracks[%d].%s" % (j, k), v) for j, t in enumerate(out["tracks"]) for k, v in t.items()]
    ref = dict([(k, v) for k, v in host.items() if k != "tracks"] + [("tracks[%d].%s" % (j, k), v) for j, t in enumerate(host["tracks"]) for k, v in t.items()])
    state = {}

    def call():
        state["rec"], state["tape"] = bt.rollout_record(dev, DT, K, tape=state.get("tape"), tracks=dev_tracks, score=SCORE, want_trace=False)
        r = state["rec"]
        bt.rollout_vjp(state["tape"], out=out, score_seed=dict(mask=MASK, q_final=r["q"], err_max_tick=r["err_max_tick"], g_err_sq_sum=dgam[0],
                                                               g_err_final=dgam[1], g_err_max=dgam[2]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                           # (warm-up outside the capture: the workspaces get their size)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first = {k: _host(v) for k, v in flat}
    keep_rec = state["rec"]                                              # (the captured call's buffers stay alive)
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
    assert np.abs(first["tracks[0].d_points"]).max() > 0 and keep_rec is not None
    bt.close()


# ---- 4. exact zeros
def test_one_bit_is_that_frame_alone_and_zero_cotangents_change_no_bit():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    seeds, gam = rv._seeds(B, K, 21, np.array([m.nv for m in models])[mid]), _gammas(B, 31)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    # the gripper alone (row 1 of the three scored frames): mask bit 4 with its rows == all three frames with zero rows for the others
    row = lambda a: np.ascontiguousarray(a[1:2])      # noqa: E731
    one = bt.rollout_vjp(tape, score_seed=dict(mask=1 << 4, q_final=rec["q"], err_max_tick=row(rec["err_max_tick"]), g_err_sq_sum=row(gam[0]),
                                               g_err_final=row(gam[1]), g_err_max=row(gam[2])), **seeds)
    zg = [np.where(np.arange(3)[:, None] == 1, g, 0.0) for g in gam]
    three = bt.rollout_vjp(tape, score_seed=_seed_of(rec, zg), **seeds)
    for name, x, y in _blocks(one, three, [k for k in one if k != "tracks"]):
        assert _same(x, y), name
    # all-zero cotangents with a state seed: wbc_rollout_vjp_tracks' bits
    plain = bt.rollout_vjp(tape, **seeds)
    assert bt.stat("last_trackvjp_variant") == 1 << 32
    zero = bt.rollout_vjp(tape, score_seed=_seed_of(rec, [np.zeros_like(g) for g in gam]), **seeds)
    for name, x, y in _blocks(zero, plain, [k for k in plain if k != "tracks"]):
        assert _same(x, y), name
    assert not _same(one["d_q0"], plain["d_q0"])
    bt.close()


# ---- 5. bad rows among good ones, guarded device buffers in place
def test_bad_rows_among_good_ones_under_guards():
    """B = 7 over the three models: instance 1 has a NaN g_err_sq_sum (the gripper's row), instance 3 an infinite q_final entry, instance 5
    err_max_tick = K under a non-zero g_err_max; instance 4's err_max_tick is out of range too, but its g_err_max is 0: it stays good.
    Device pointers in place, pattern guard rows around every output, NaN guard rows around every float input. The guards come back intact,
    the inputs byte for byte; the bad instances get all-zero rows in every output and WBC_GRAD_NONFINITE; the others keep their bits"""
    import torch
    import devguard as dg
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    names_, _ = SHAPES["mixed7"]
    _, _, o, _ = tgp._problem(names_, "everything", 2 * dg.G, seed=9, with_rot=True)
    seeds, gam = rv._seeds(B, K, 21, np.array([m.nv for m in models])[mid]), _gammas(B, 31)
    gam[2][:, 4] = 0.0
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    good = bt.rollout_vjp(tape, score_seed=_seed_of(rec, gam), **seeds)
    bad_rows, ok = [1, 3, 5], np.array([0, 2, 4, 6])
    assert (good["grad_status"] != capi.GRAD_NONFINITE).all()
    bgam = [g.copy() for g in gam]
    bgam[0][1, 1] = np.nan
    q_final, tick = rec["q"].copy(), rec["err_max_tick"].copy()
    q_final[3, 5] = np.inf
    tick[0, 5], tick[2, 4] = K, -7
    stream = torch.cuda.Stream()
    sess = dg.Session("nan", stream)
    main = tt._main_names(bt, tracks)
    ss = dict(mask=MASK, q_final=sess.put("q_final", q_final, o["q"]), err_max_tick=sess.put("err_max_tick", tick, np.zeros((2 * dg.G, B), np.int32)),
              g_err_sq_sum=sess.put("g_sq", bgam[0], None), g_err_final=sess.put("g_fin", bgam[1], None), g_err_max=sess.put("g_max", bgam[2], None))
    g_final = sess.put("g_q_final", seeds["g_q_final"], o["q"][:, :26])
    g_last = sess.put("g_qdot_last", seeds["g_qdot_last"], o["q"][:, :26])
    g_trace = torch.from_numpy(seeds["g_q_trace"]).cuda()
    out = {k: sess.out((B,) + capi.ROLLOUT_GRAD_FIELDS[k]) for k in main}
    out["grad_status"], out["ticks_dropped"] = sess.out((B,), np.int32), sess.out((B,), np.int32)
    out["tracks"] = [{k: sess.out((B, tg.S, 3) if k != "d_du" else (B,)) for k in good["tracks"][j]} for j in range(3)]
    dev_tape = tape                                                      # (the record ran on host arrays; its tape is device memory already)
    dev_tape.call = dict(tape.call, inputs=_dev(d), tracks=tt._dev_tracks(tracks))
    sess.run(lambda: bt.rollout_vjp(dev_tape, g_q_final=g_final, g_qdot_last=g_last, g_q_trace=g_trace, out=out, score_seed=ss))
    sess.check("rollout_vjp with a score seed")
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


# ---- 6. refusals
def test_refusals_name_their_field_and_come_before_any_launch():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("b5", "full", K)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    gam = _gammas(B, 31)
    bt.rollout_vjp(tape, g_q_final=np.ones((B, 26)))                     # (a plain call first: the workspace has its size, the statistic its -1)
    assert bt.stat("last_scorevjp_variant") == -1

    def refused(fn, word, code=capi.E_ARG):
        with pytest.raises(capi.WbcError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), (word, str(e.value))
        assert bt.stat("last_scorevjp_variant") == -1 and (dq0 == 7.0).all()

    keep = []
    tin = bt._tick_in(d, keep, B)
    tk, _ = bt._tracks_struct(tracks, B, keep)
    r = capi.WbcRollout()
    r.ticks, r.mode, r.hold_ticks = K, capi.ROLLOUT_RUNNING, 0
    og, tgr = capi.WbcRolloutGrad(), capi.WbcTracksGrad()
    dq0 = np.full((B, 26), 7.0)
    og.d_q0 = dq0.ctypes.data
    tick = np.ascontiguousarray(rec["err_max_tick"])
    q_final = np.ascontiguousarray(rec["q"])

    def seed(**kw):
        s = capi.WbcScoreSeed()
        s.score_mask = kw.pop("mask", MASK)
        vals = dict(g_err_sq_sum=gam[0], g_err_final=gam[1], g_err_max=gam[2], err_max_tick=tick, q_final=q_final)
        vals.update(kw)
        for k, v in vals.items():
            setattr(s, k, None if v is None else v.ctypes.data)
        return s

    def call(ss, rr=r, tin_=tin, tracks_p=C.byref(tk), out_p=C.byref(tgr)):
        capi.check(bt.lib.wbc_rollout_vjp_scored(bt._h, B, C.byref(tin_), None, DT, C.byref(rr), tracks_p, tape.buf.data_ptr(), tape.buf.numel(), None,
                                                 None if ss is None else C.byref(ss), capi.MEM_HOST, C.byref(og), out_p, None), bt.lib)
    refused(lambda: call(None), "score")
    refused(lambda: call(seed(g_err_sq_sum=None, g_err_final=None, g_err_max=None)), "g_err_sq_sum")
    refused(lambda: call(seed(err_max_tick=None)), "err_max_tick")
    refused(lambda: call(seed(q_final=None)), "q_final")
    refused(lambda: call(seed(mask=0)), "score_mask")
    refused(lambda: call(seed(mask=1 << 6)), "score_mask")
    refused(lambda: call(seed(mask=-1)), "score_mask")
    no_trunk = bt._tick_in({k: v for k, v in d.items() if k not in ("trunk_target", "prev_trunk_target")}, keep, B)
    two = capi.WbcTracks()
    C.memmove(C.byref(two), C.byref(tk), C.sizeof(tk))
    two.n_tracks = 2                                                     # (without the trunk track the tracks call itself asks for no trunk target)
    refused(lambda: call(seed(), tin_=no_trunk, tracks_p=C.byref(two)), "trunk_target")
    imu = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1))
    with_imu = capi.WbcRollout()
    with_imu.ticks, with_imu.mode, with_imu.hold_ticks, with_imu.imu = K, capi.ROLLOUT_RUNNING, 0, imu.ctypes.data
    refused(lambda: call(seed(), rr=with_imu), "imu")
    # what wbc_rollout_vjp_tracks refuses
    refused(lambda: call(seed(), out_p=None), "tracks_out")
    refused(lambda: call(seed(), tracks_p=None), "tracks")
    held = capi.WbcRollout()
    held.ticks, held.mode, held.hold_ticks = K, capi.ROLLOUT_RUNNING, 2
    refused(lambda: call(seed(), rr=held), "hold_ticks")
    refused(lambda: bt.rollout_vjp(tape, score_seed=dict(_seed_of(rec, gam)), out=dict(d_q0=dq0, grad_status=np.zeros(B, np.int32), d_ee_target_step=np.zeros((B, 5, 3)))),
            "d_ee_target_step")
    # the wrapper: a tape without tracks has no scores
    _, plain_tape = bt.rollout_record(d, DT, K)
    with pytest.raises(capi.WbcError):
        bt.rollout_vjp(plain_tape, score_seed=_seed_of(rec, gam))
    # and with everything in place the call runs: a state seed is not required
    call(seed())
    assert bt.stat("last_scorevjp_variant") == KEY_SEED[False] and not (dq0 == 7.0).any()
    assert bt.lib.wbc_variant_count(b"scorevjp") == 3
    bt.close()


# ---- 7. the handle
def test_a_plain_tracks_sweep_after_scored_calls_gives_the_bits_of_a_fresh_handle():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    seeds, gam = rv._seeds(B, K, 21, np.array([m.nv for m in models])[mid]), _gammas(B, 31)
    bt = tgp._handle(models, cfgs, B, {})
    _, tape0 = bt.rollout_record(d, DT, K, tracks=tracks)
    fresh = bt.rollout_vjp(tape0, **seeds)
    bt.close()
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=SCORE)
    bt.rollout_vjp(tape, score_seed=_seed_of(rec, gam), **seeds)
    bt.rollout_vjp(tape, score_seed=_seed_of(rec, gam))
    _, tape1 = bt.rollout_record(d, DT, K, tracks=tracks)
    after = bt.rollout_vjp(tape1, **seeds)
    assert tt._same_tapes(tape1, tape0)
    for name, x, y in _blocks(after, fresh, [k for k in fresh if k != "tracks"]):
        assert _same(x, y), name
    bt.close()


# ---- 8. the torch layer
def _scored(bt, dev, dev_tracks, K, gam, rho=None):
    """-> (outputs on the host, d_q0 raw, per track dict(points, tangents, du) gradients) of sum gamma . scores (+ rho . q_K)"""
    import torch
    import wbc_torch
    q0 = dev["q"].clone().requires_grad_(True)
    trk = [{k: (v.clone().requires_grad_(True) if k in ("points", "tangents", "du") else v) for k, v in t.items()} for t in dev_tracks]
    res = wbc_torch.wbc_rollout_tracks_scored(q0, None, trk, {k: v for k, v in dev.items() if k != "q"}, DT, K, bt, score=SCORE)
    q, qdot, st, trace, sq, fin, mx, tick = res
    assert sq.requires_grad and fin.requires_grad and mx.requires_grad and not tick.requires_grad and not st.requires_grad
    loss = sum((torch.from_numpy(g).cuda() * s).sum() for g, s in zip(gam, (sq, fin, mx)) if g is not None)
    if rho is not None:
        loss = loss + (q * torch.from_numpy(rho).cuda()).sum()
    loss.backward()
    grads = [{k: _host(n[k].grad) for k in ("points", "tangents", "du") if k in n} for n in trk]
    return [_host(t.detach()) for t in res], _host(q0.grad), grads


def test_scored_layer_is_the_record_and_the_sweep_bit_for_bit():
    import torch
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("b5", "everything", K)
    rho, gam = np.random.default_rng(33).normal(0, 1.0, (B, 27)), _gammas(B, 31)
    bt = tgp._handle(models, cfgs, B, {})
    dev, dev_tracks = _dev(d), tt._dev_tracks(tracks)
    res, g_q0, grads = _scored(bt, dev, dev_tracks, K, gam, rho)
    plain = bt.rollout_tracks(d, DT, K, tracks, score=SCORE)
    for i, k in enumerate(("q", "qdot", "status")):
        assert _same(res[i], plain[k]), k
    for i, k in zip(range(4, 8), ("err_sq_sum", "err_final", "err_max", "err_max_tick")):
        assert _same(res[i], plain[k]), k
    rec, tape = bt.rollout_record(dev, DT, K, tracks=dev_tracks, score=SCORE)
    seed = wbc_workload.raw_to_tangent(rec["q"], torch.from_numpy(rho).cuda()).contiguous()      # what the layer's backward does
    ref = bt.rollout_vjp(tape, g_q_final=seed, want=("d_q0",) + tt.TRACK_NAMES,
                         score_seed=dict(mask=SCORE, q_final=rec["q"], err_max_tick=rec["err_max_tick"], g_err_sq_sum=torch.from_numpy(gam[0]).cuda(),
                                         g_err_final=torch.from_numpy(gam[1]).cuda(), g_err_max=torch.from_numpy(gam[2]).cuda()))
    assert _same(g_q0, _host(wbc_workload.tangent_to_raw(dev["q"], ref["d_q0"])))
    for j in range(3):
        assert set(grads[j]) == {"points", "du"} | ({"tangents"} if "tangents" in tracks[j] else set())
        for k, v in grads[j].items():
            assert _same(v, _host(ref["tracks"][j]["d_" + k])), (j, k)
            assert np.abs(v).max() > 0
    # a loss on one score alone: the other cotangents are left out of the call, not passed as zeros
    res1, g1, _ = _scored(bt, dev, dev_tracks, K, [gam[0], None, None])
    ref1 = bt.rollout_vjp(tape, want=("d_q0",), score_seed=dict(mask=SCORE, q_final=rec["q"], g_err_sq_sum=torch.from_numpy(gam[0]).cuda()))
    assert _same(g1, _host(wbc_workload.tangent_to_raw(dev["q"], ref1["d_q0"])))
    bt.close()


@pytest.mark.parametrize("cfg_name,seed", [("full", 3)])
def test_backward_of_err_sq_sum_against_central_differences_of_the_oracle_chain(cfg_name, seed, monkeypatch):
    """test_score_grad_host's item 3 with the device's gradients of err_sq_sum.sum(): the same inputs, tracks, directions, rule and cap"""
    p = sh.score_problem(cfg_name, seed, only_sq=True)
    m, cfg, d, K, B, tracks = p["m"], p["cfg"], p["d"], p["K"], p["B"], p["tracks"]
    assert all((s == 0).all() for s in p["status"]) and sh.SCORED == FRAMES
    margin, kappa = tg.margins(m, cfg, p["states"], p["ticks"], K)
    bt = tgp._handle([m], [cfg], B, {})
    res, _, g = _scored(bt, _dev(d), tt._dev_tracks(tracks), K, [np.ones((3, B)), None, None])
    bt.close()
    assert (res[2] == 0).all()
    g = [{"d_" + k: v for k, v in t.items()} for t in g]
    rho = np.zeros((B, capi.Q_STRIDE))
    rho[:, :3] = sh.RHO
    monkeypatch.setattr(tg, "track_chain", sh.loss_in_q(p["loss"]))
    for name, p_, v_, u_, ana, terms in sh.directional_cases(p, g, seed):
        keep, ok, line = tg.track_chain_directional(m, cfg, d, rho, K, DT, lambda s: tg.perturbed(tracks, s, p_, v_, u_), p["sides0"], margin, kappa,
                                                    ana, terms, "%s / seed %d, K = %d, scored layer, %s" % (cfg_name, seed, K, name))
        print(line)
        assert (~keep).sum() <= B // 4 and ok, line
