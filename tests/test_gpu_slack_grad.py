"""wbc_state_slack_vjp / wbc_rollout_record_watch / wbc_rollout_vjp_watched on the device: the constraint slacks as a loss, their cotangents
formed by wbc_slackvjp_kernel at a state (STATE) and where the sweep runs (SEED). Shapes: test_gpu_score_grad.SHAPES' b1, b5, mixed7 (three
models, the Laikago + ViperX-300 among them: the ROT rows) and laikago5 (one instance in its last wave); configurations `full` and `everything`,
K = 3 or 4. The box is displaced everywhere (slack_grad_common.displace_box: at the stock inputs all six angle components tie); the sweep runs
without an IMU but for one case that is a pure bits / refusal check. A comparison that depends on the selected component is made where the
restatement's two smallest components are more than slack_common.TIE apart or exactly equal; at most B // 4 instances may fall out.

  1. the layer         against wbc_workload.slack_gradients within PARITY_BOUND (1e-11 x max(1, max|ref|), the project's per-layer bound);
                       `which` is wbc_state_slack's bit for bit; g_components alone, g_slack alone, both = the sum
  2. the cross-check   rollout_vjp(watch_seed) alone against rollout_vjp(g_q_trace = the host-built rows at the taped states), every block
                       within SWEEP_BOUND, d_trunk_box_center offset by the closed-form box term; the record's watch outputs are
                       rollout_watch's byte for byte, its tape rollout_record's
  3. the restatement   against rollout_gradients(watch_seed=...): each g array alone and all together, with a state seed, a score seed, both
                       (= the sum), with and without tracks
  4. bits              identical calls; capture and replay; all-zero cotangents beside a state seed = wbc_rollout_vjp[_tracks]' bits; a one-bit
                       mask = the full mask with zero rows; with an IMU the call runs and repeats its bits
  5. bad rows          a NaN cotangent on one tick of g_trace, an infinite q_final entry, slack_min_tick = K under a non-zero g_slack_min (and
                       under a zero one: good), a NaN box entry, under guarded device buffers
  6. refusals          each names its field and comes before any launch
  7. the handle        a plain sweep after watched calls gives a fresh handle's bits
  8. torch             wbc_state_slack / wbc_rollout_watched: outputs byte for byte, backward bit for bit, a squared hinge on trace against
                       central differences of the oracle chain (track_chain_directional's rule, the B // 4 cap)

Measured on MI355X (worst max|dev - ref| / max(1, max|ref|) per case; no instance fell out of any comparison). The layer (bound 1e-11): b1
3.5e-16, b5 4.0e-16, mixed7 3.9e-16, laikago5 2.0e-16. Cross-check: b1 / full 8.9e-16, b5 / everything 3.0e-15, mixed7 / everything 1.9e-14,
laikago5 / full 9.2e-16. Restatement, all three arrays / with a state seed / with a score seed: b1 / full 4.1e-14 / 2.6e-14 / -, b5 / everything
2.4e-13 / 4.1e-11 / 2.5e-13, mixed7 / everything 3.5e-11 / 3.9e-11 / 6.2e-11, laikago5 / full 1.4e-14 / 3.7e-14 / -; on b5 / full g_slack_min alone
1.9e-14, g_slack_final alone 4.3e-14, g_trace alone 2.4e-14: on `full` none above a hundredth of its bound, on `everything` the state layers' own
error is the largest term (as in test_gpu_score_grad). The hinge against the oracle chain: 16 of 16 instances kept in points, tangents and du."""
import ctypes as C

import numpy as np
import pytest

import gradq_common as gq
import oracle
import slack_common as sl
import slack_grad_common as sgc
import test_gpu_rollout_vjp as rv
import test_gpu_score_grad as sg
import test_gpu_task_params as tgp
import test_gpu_tick_grad_q as tgq
import test_gpu_track_grad as tt
import test_score_grad_host as sh
import test_step_grad_host as th
import test_tick_grad_q_host as tq
import track_grad_common as tg
import wbc_capi as capi
import wbc_workload

pytestmark = pytest.mark.gpu

DT = tq.DT
_same, _host, _dev = rv._same, rv._host, rv._dev
SHAPES = sg.SHAPES
PARITY_BOUND = tgq.PARITY_BOUND
WATCH = sl.FAMILIES
MASK = sgc.FULL_MASK
KEY = {("state", False): 0, ("state", True): 1 << 24, ("seed", False): 1 << 32, ("seed", True): (1 << 32) | (1 << 24)}      # variant_key(STAGE, ROT)
ROTATED = sg.ROTATED
CASES = sg.CASES


def _setup(shape, cfg_name, K, seed=7):
    models, cfgs, d, mid, B, tracks = sg._setup(shape, cfg_name, K, seed)
    return models, cfgs, sgc.displace_box(d), mid, B, tracks


def _flat(res):
    return [(k, v) for k, v in res.items() if k != "tracks"] + [("tracks[%d].%s" % (j, k), v) for j, t in enumerate(res.get("tracks", ())) for k, v in t.items()]


def _worst(got, ref, what, rows=None, offset=None):
    """the worst max|dev - ref| / max(1, max|ref|) over the float blocks of `got` (ref: a dict that holds at least those; rows: the instances
    compared; offset: block name -> what is added to the reference)"""
    worst, refs = 0.0, dict(_flat(ref))
    for name, a in _flat(got):
        if name in ("grad_status", "ticks_dropped"):
            continue
        b = refs[name] + (offset or {}).get(name, 0.0)
        if rows is not None:
            a, b = a[rows], b[rows]
        ratio = np.abs(a - b).max() / max(1.0, np.abs(b).max())
        worst = max(worst, ratio)
        print("%s: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e)" % (what, name, ratio, np.abs(b).max()))
    return worst


def _q_after(seen, q_final):
    return np.stack([seen[k + 1][0]["q"] for k in range(len(seen) - 1)] + [q_final])


def _kept(models, cfgs, mid, q_after, box):
    """[B]: every tick's selection of every family is comparable; the cap"""
    ok = np.ones(q_after.shape[1], dtype=bool)
    for k in range(len(q_after)):
        ok &= sgc.selection_ok(models, cfgs, mid, q_after[k], box).all(axis=1)
    assert (~ok).sum() <= len(ok) // 4, "too many near-ties: %d of %d" % ((~ok).sum(), len(ok))
    return ok


# ---- 1. the layer
@pytest.mark.parametrize("shape", ["b1", "b5", "mixed7", "laikago5"])
def test_layer_against_the_restatement(shape):
    models, cfgs, d, mid, B, _ = _setup(shape, "everything", 3)
    q, box = d["q"], d["trunk_box_center"]
    rng = np.random.default_rng(17)
    gs, gc_ = rng.normal(0, 1.0, (B, 4)), rng.normal(0, 1.0, (B, 12))
    bt = tgp._handle(models, cfgs, B, {})
    assert bt.stat("last_slackvjp_variant") == -1
    fwd = bt.state_slack(q, box, model_id=mid, want_components=True)
    keep = sgc.selection_ok(models, cfgs, mid, q, box).all(axis=1)
    assert (~keep).sum() <= B // 4
    worst, res = 0.0, {}
    for what, a, b in (("g_components alone", None, gc_), ("g_slack alone", gs, None), ("both", gs, gc_)):
        got = bt.state_slack_grad(q, box, g_slack=a, g_components=b, model_id=mid)
        assert bt.stat("last_slackvjp_variant") == KEY[("state", ROTATED[shape])]
        assert _same(got["which"], fwd["which"]) and (got["grad_status"] == capi.GRAD_OK).all()
        ref = sgc.restate_layer(models, cfgs, mid, q, box, a, b)
        rows = np.ones(B, dtype=bool) if a is None else keep
        assert np.array_equal(got["which"][rows], ref["which"][rows])
        w = _worst({k: got[k] for k in ("d_q", "d_trunk_box_center")}, ref, "%s, %s" % (shape, what), rows=rows)
        worst = max(worst, w)
        assert np.abs(got["d_q"]).max() > 0
        res[what] = got
    for k in ("d_q", "d_trunk_box_center"):
        s = res["g_components alone"][k] + res["g_slack alone"][k]
        assert np.abs(res["both"][k] - s).max() <= PARITY_BOUND * max(1.0, np.abs(s).max()), k
    nvs = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
    assert not res["both"]["d_q"][np.arange(26)[None, :] >= nvs[:, None]].view(np.uint64).any()
    print("%s: worst ratio %.3e (bound %.0e), %d of %d instances left out of the g_slack comparisons" % (shape, worst, PARITY_BOUND, (~keep).sum(), B))
    assert worst <= PARITY_BOUND
    bt.close()


# ---- 2. the cross-check, and the forward
@pytest.mark.parametrize("shape,cfg_name,K", CASES)
def test_watch_seed_alone_is_the_sweep_with_a_host_built_trace(shape, cfg_name, K):
    models, cfgs, d, mid, B, tracks = _setup(shape, cfg_name, K)
    tracks = tracks if shape in ("b5", "mixed7") else None              # with and without tracks
    gam = sgc.watch_gammas(B, K, 31)
    bt = tgp._handle(models, cfgs, B, {})
    plain_w = {k: v for k, v in bt.rollout_watch(d, DT, K, watch=WATCH, tracks=tracks, want_trace=True).items() if k != "grip_trace"}
    assert {"slack_min", "slack_final", "slack_min_tick", "slack_min_which", "neg_ticks", "first_neg_tick", "slack_trace"} <= set(plain_w)
    _, tape0 = bt.rollout_record(d, DT, K, tracks=tracks)
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, watch=WATCH, watch_trace=True)
    for k in plain_w:
        assert _same(rec[k], plain_w[k]), "%s differs from wbc_rollout_watch's" % k
    assert tt._same_tapes(tape, tape0)
    assert bt.stat("last_slackvjp_variant") == -1
    seed = sgc.watch_seed_of(rec, gam)
    got = bt.rollout_vjp(tape, watch_seed=seed)
    assert bt.stat("last_slackvjp_variant") == KEY[("seed", ROTATED[shape])]
    seen = tt._seen(cfgs, d, tape, K)
    q_after = _q_after(seen, rec["q"])
    keep = _kept(models, cfgs, mid, q_after, d["trunk_box_center"])
    g_trace, dbox = sgc.watch_rows(models, cfgs, mid, q_after, d["trunk_box_center"], seed)
    assert np.abs(g_trace).max() > 0
    plain = bt.rollout_vjp(tape, g_q_trace=g_trace)
    assert set(got) == set(plain) and np.array_equal(got["ticks_dropped"], plain["ticks_dropped"]) and np.array_equal(got["grad_status"], plain["grad_status"])
    what = "%s / %s, K = %d, cross-check" % (shape, cfg_name, K)
    worst = _worst(got, plain, what, rows=keep, offset=dict(d_trunk_box_center=dbox))
    print("%s: worst ratio %.3e (bound %.0e), %d of %d instances kept" % (what, worst, rv.SWEEP_BOUND[cfg_name], keep.sum(), B))
    assert worst <= rv.SWEEP_BOUND[cfg_name]
    if "d_trunk_box_center" in got:
        assert np.abs(got["d_trunk_box_center"] - plain["d_trunk_box_center"]).max() > 0
    bt.close()


# ---- 3. the restatement
def _restate(models, cfgs, mid, seen, state, tracks, score_seed, watch_seed):
    K, B = len(seen), len(seen[0][0]["q"])
    out = None
    for i, m, sel in sgc.per_model(models, mid, B):
        c, n = cfgs[i], int(sel.sum())
        ins = [{k: v[sel] for k, v in cur.items() if k != "model_id"} for cur, _ in seen]
        sub = None if tracks is None else [{k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in tracks]
        cut = lambda s_: None if s_ is None else {k: (None if v is None else v if k == "mask" else v[sel] if k == "q_final" else np.asarray(v)[..., sel])      # noqa: E731
                                                  for k, v in s_.items()}
        st = {} if state is None else dict(g_q_final=state["g_q_final"][sel], g_qdot_last=state["g_qdot_last"][sel], g_q_trace=state["g_q_trace"][:, sel])
        r = wbc_workload.rollout_gradients(m, c, ins, np.stack([t["qdot"][sel] for _, t in seen]), DT, gq.StateFK([m]),
                                           lambda dd, m=m, c=c, n=n: oracle.assemble([m], [c], dd, DT, n),
                                           status=np.stack([t["status"][sel] for _, t in seen]), tracks=sub, score_seed=cut(score_seed),
                                           watch_seed=cut(watch_seed), **st)
        rt = r.pop("tracks", [])
        if out is None:
            out = {k: np.zeros((B,) + v.shape[1:], dtype=v.dtype) for k, v in r.items()}
            if tracks is not None:
                out["tracks"] = [{k: (None if v is None else np.zeros((B,) + v.shape[1:])) for k, v in t.items()} for t in rt]
        for k in r:
            out[k][sel] = r[k]
        for j, t in enumerate(rt):
            for k, v in t.items():
                if v is not None:
                    out["tracks"][j][k][sel] = v
    return out


def _compare(got, ref, keep, what, bound):
    worst = _worst(got, ref, what, rows=keep)
    print("%s: worst ratio %.3e (bound %.0e)" % (what, worst, bound))
    assert worst <= bound, what
    return worst


@pytest.mark.parametrize("shape,cfg_name,K", CASES)
def test_watched_sweep_against_the_restatement(shape, cfg_name, K):
    models, cfgs, d, mid, B, tracks = _setup(shape, cfg_name, K)
    with_tracks = shape in ("b5", "mixed7")
    tracks = tracks if with_tracks else None
    nvs = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
    state, gam = rv._seeds(B, K, 21, nvs), sgc.watch_gammas(B, K, 31)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=sg.SCORE if with_tracks else (), watch=WATCH)
    seen = tt._seen(cfgs, d, tape, K)
    keep = _kept(models, cfgs, mid, _q_after(seen, rec["q"]), d["trunk_box_center"])
    wseed = sgc.watch_seed_of(rec, gam)
    bound = rv.SWEEP_BOUND[cfg_name]
    what = "%s / %s, K = %d" % (shape, cfg_name, K)
    got = bt.rollout_vjp(tape, watch_seed=wseed)
    ref = _restate(models, cfgs, mid, seen, None, tracks, None, wseed)
    assert np.array_equal(got["ticks_dropped"], ref["ticks_dropped"]) and (got["grad_status"] != capi.GRAD_NONFINITE).all()
    _compare(got, ref, keep, what + ", all three arrays", bound)
    assert np.abs(got["d_q0"]).max() > 0
    both = bt.rollout_vjp(tape, watch_seed=wseed, **state)
    _compare(both, _restate(models, cfgs, mid, seen, state, tracks, None, wseed), keep, what + ", + state seed", bound)
    if with_tracks:
        sseed = sg._seed_of(rec, sg._gammas(B, 32))
        sc_w = bt.rollout_vjp(tape, watch_seed=wseed, score_seed=sseed)
        _compare(sc_w, _restate(models, cfgs, mid, seen, None, tracks, sseed, wseed), keep, what + ", + score seed", bound)
        sc_only = bt.rollout_vjp(tape, score_seed=sseed)
        total = {k: got[k] + sc_only[k] for k in got if k not in ("grad_status", "ticks_dropped", "tracks")}
        total["tracks"] = [{k: got["tracks"][j][k] + sc_only["tracks"][j][k] for k in t} for j, t in enumerate(got["tracks"])]
        _compare(sc_w, total, None, what + ", watch + score = the sum of each", bound)
        assert all(np.abs(t["d_points"]).max() > 0 for t in got["tracks"])
    bt.close()


def test_each_array_alone_and_the_sum_of_the_seeds():
    K, shape, cfg_name = 3, "b5", "full"
    models, cfgs, d, mid, B, _ = _setup(shape, cfg_name, K)
    state, gam = rv._seeds(B, K, 21, np.full(B, models[0].nv)), sgc.watch_gammas(B, K, 31)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, watch=WATCH)
    seen = tt._seen(cfgs, d, tape, K)
    keep = _kept(models, cfgs, mid, _q_after(seen, rec["q"]), d["trunk_box_center"])
    bound = rv.SWEEP_BOUND[cfg_name]
    alone = []
    for name in ("g_slack_min", "g_slack_final", "g_trace"):
        seed = sgc.watch_seed_of(rec, gam, which=(name,))
        got = bt.rollout_vjp(tape, watch_seed=seed)
        _compare(got, _restate(models, cfgs, mid, seen, None, None, None, seed), keep, "%s / %s, %s alone" % (shape, cfg_name, name), bound)
        assert np.abs(got["d_q0"]).max() > 0
        alone.append(got)
    allg = bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam))
    st = bt.rollout_vjp(tape, **state)
    both = bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam), **state)
    names = [k for k in allg if k not in ("grad_status", "ticks_dropped")]
    add = lambda rs: {k: sum(r[k] for r in rs) for k in names}      # noqa: E731
    _compare(allg, add(alone), None, "three arrays = the sum of each", bound)
    _compare(both, add([allg, st]), None, "both seeds = the sum of each", bound)
    bt.close()


# ---- 4. bits
def test_identical_calls_zero_cotangents_and_a_one_bit_mask():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    state, gam = rv._seeds(B, K, 21, np.array([m.nv for m in models])[mid]), sgc.watch_gammas(B, K, 31)
    bt = tgp._handle(models, cfgs, B, {})
    for trk in (None, tracks):
        rec, tape = bt.rollout_record(d, DT, K, tracks=trk, watch=WATCH)
        a = bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam), **state)
        rec2, tape2 = bt.rollout_record(d, DT, K, tracks=trk, watch=WATCH)
        b = bt.rollout_vjp(tape2, watch_seed=sgc.watch_seed_of(rec2, gam), **state)
        for (name, x), (_, y) in zip(_flat(a), _flat(b)):
            assert _same(x, y), name
        # all-zero cotangents beside a state seed: wbc_rollout_vjp's / _tracks' bits
        plain = bt.rollout_vjp(tape, **state)
        zero = bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, {k: np.zeros_like(v) for k, v in gam.items()}), **state)
        for (name, x), (_, y) in zip(_flat(zero), _flat(plain)):
            assert _same(x, y), name
        assert not _same(a["d_q0"], plain["d_q0"])
        # the CoM family alone (row 0): mask bit 0 with its rows == the full mask with zero rows for the others
        row = lambda v: np.ascontiguousarray(v[..., 0:1, :])      # noqa: E731
        one = bt.rollout_vjp(tape, watch_seed=dict(mask=1, q_final=rec["q"], slack_min_tick=row(rec["slack_min_tick"]),
                                                   **{k: row(v) for k, v in gam.items()}), **state)
        zg = {k: np.where((np.arange(4) == 0)[:, None], v, 0.0) for k, v in gam.items()}
        four = bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, zg), **state)
        for (name, x), (_, y) in zip(_flat(one), _flat(four)):
            assert _same(x, y), name
    bt.close()


def test_an_imu_quaternion_is_allowed_and_a_score_seed_beside_it_is_refused():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("b5", "everything", K)
    gam = sgc.watch_gammas(B, K, 31)
    imu = d["q"][:, 3:7].copy()
    bt = tgp._handle(models, cfgs, B, {})
    plain_w = bt.rollout_watch(d, DT, K, watch=WATCH, tracks=tracks, imu=imu)
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=sg.SCORE, watch=WATCH, imu=imu)
    for k in plain_w:
        assert _same(rec[k], plain_w[k]), k
    a = bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam))
    b = bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam))
    for (name, x), (_, y) in zip(_flat(a), _flat(b)):
        assert _same(x, y), name
    assert np.abs(a["d_q0"]).max() > 0 and (a["grad_status"] != capi.GRAD_NONFINITE).all()
    with pytest.raises(capi.WbcError) as e:
        bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam), score_seed=sg._seed_of(rec, sg._gammas(B, 32)))
    assert e.value.code == capi.E_ARG and "imu" in str(e.value)
    bt.close()


def test_capture_and_replay_give_the_same_bits():
    import torch
    K = 3
    models, cfgs, d, mid, B, _ = _setup("mixed7", "everything", K)
    gam = sgc.watch_gammas(B, K, 31)
    bt = tgp._handle(models, cfgs, B, {})
    rec0, tape0 = bt.rollout_record(d, DT, K, watch=WATCH)
    host = bt.rollout_vjp(tape0, watch_seed=sgc.watch_seed_of(rec0, gam))
    layer0 = bt.state_slack_grad(d["q"], d["trunk_box_center"], g_slack=gam["g_slack_final"].T.copy(), model_id=mid)
    dev = _dev(d)
    dgam = {k: torch.from_numpy(v).cuda() for k, v in gam.items()}
    gsl = torch.from_numpy(gam["g_slack_final"].T.copy()).cuda()
    names = [k for k in host if k not in ("grad_status", "ticks_dropped")]
    out = {k: torch.empty((B,) + capi.ROLLOUT_GRAD_FIELDS[k], dtype=torch.float64, device="cuda") for k in names}
    out["grad_status"], out["ticks_dropped"] = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    state = {}

    def call():
        state["rec"], state["tape"] = bt.rollout_record(dev, DT, K, tape=state.get("tape"), watch=WATCH, want_trace=False)
        r = state["rec"]
        bt.rollout_vjp(state["tape"], out=out, watch_seed=dict(mask=MASK, q_final=r["q"], slack_min_tick=r["slack_min_tick"], **dgam))
        state["layer"] = bt.state_slack_grad(dev["q"], dev["trunk_box_center"], g_slack=gsl, model_id=dev["model_id"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                           # (warm-up outside the capture: the workspaces get their size)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first = {k: _host(v) for k, v in out.items()}
    keep_alive = [state["rec"], state["layer"]]
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        call()
    for v in out.values():
        v.fill_(3)
    state["tape"].buf.fill_(0)
    gr.replay()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert _same(_host(v), first[k]) and _same(first[k], host[k]), k
    for k, v in state["layer"].items():
        assert _same(_host(v), layer0[k]), k
    assert np.abs(first["d_q0"]).max() > 0 and keep_alive
    bt.close()


# ---- 5. bad rows among good ones, guarded device buffers in place
def test_bad_rows_among_good_ones_under_guards():
    """B = 7 over the three models: instance 1 has a NaN g_trace entry on tick 1 (family 0), instance 3 an infinite q_final entry, instance 5
    slack_min_tick = K under a non-zero g_slack_min, instance 2 a NaN box entry (the z centre; family 1 is seeded); instance 4's
    slack_min_tick is out of range too, but its g_slack_min is 0: it stays good. Device pointers in place, pattern guard rows around every
    output, NaN guard rows around every float input. The guards come back intact, the inputs byte for byte; the bad instances get all-zero
    rows in every output and WBC_GRAD_NONFINITE; the others keep their bits."""
    import torch
    import devguard as dg
    K = 3
    models, cfgs, d, mid, B, _ = _setup("mixed7", "everything", K)
    names_, _ = SHAPES["mixed7"]
    _, _, o, _ = tgp._problem(names_, "everything", 2 * dg.G, seed=9, with_rot=True)
    state, gam = rv._seeds(B, K, 21, np.array([m.nv for m in models])[mid]), sgc.watch_gammas(B, K, 31)
    gam["g_slack_min"][:, 4] = 0.0
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, watch=WATCH)
    good = bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam), **state)
    assert (good["grad_status"] != capi.GRAD_NONFINITE).all()
    # the NaN box entry: the forward must not see it (the tick reads the box), so the sweep alone gets the other box
    box = d["trunk_box_center"].copy()
    box[2, 0] = np.nan
    bad_rows, ok = [1, 2, 3, 5], np.array([0, 4, 6])
    bg = {k: v.copy() for k, v in gam.items()}
    bg["g_trace"][1, 0, 1] = np.nan
    q_final, tick = rec["q"].copy(), rec["slack_min_tick"].copy()
    q_final[3, 5] = np.inf
    tick[0, 5], tick[2, 4] = K, -7
    stream = torch.cuda.Stream()
    sess = dg.Session("nan", stream)
    main = [k for k in good if k not in ("grad_status", "ticks_dropped")]
    ws = dict(mask=MASK, q_final=sess.put("q_final", q_final, o["q"]), slack_min_tick=sess.put("slack_min_tick", tick, np.zeros((2 * dg.G, B), np.int32)),
              g_slack_min=sess.put("g_min", bg["g_slack_min"], None), g_slack_final=sess.put("g_fin", bg["g_slack_final"], None),
              g_trace=sess.put("g_trace", bg["g_trace"], None))
    g_final = sess.put("g_q_final", state["g_q_final"], o["q"][:, :26])
    g_last = sess.put("g_qdot_last", state["g_qdot_last"], o["q"][:, :26])
    g_trace = torch.from_numpy(state["g_q_trace"]).cuda()
    out = {k: sess.out((B,) + capi.ROLLOUT_GRAD_FIELDS[k]) for k in main}
    out["grad_status"], out["ticks_dropped"] = sess.out((B,), np.int32), sess.out((B,), np.int32)
    dev_in = _dev(d)
    dev_in["trunk_box_center"] = sess.put("trunk_box_center", box, o["trunk_box_center"])
    tape.call = dict(tape.call, inputs=dev_in)
    sess.run(lambda: bt.rollout_vjp(tape, g_q_final=g_final, g_qdot_last=g_last, g_q_trace=g_trace, out=out, watch_seed=ws))
    sess.check("rollout_vjp with a watch seed")
    res = dg.to_host(out)
    expect = good["grad_status"].copy()
    expect[bad_rows] = capi.GRAD_NONFINITE
    assert np.array_equal(res["grad_status"], expect), res["grad_status"]
    for k in main:
        assert not res[k][bad_rows].view(np.uint64).any(), k
        assert _same(res[k][ok], good[k][ok]), k
    # the layer: the same kinds of bad rows in the single call
    gs = gam["g_slack_final"].T.copy()
    q2, gs2 = d["q"].copy(), gs.copy()
    q2[3, 9], gs2[1, 2] = np.inf, np.nan
    gs2[4, 1] = 0.0
    box2 = box.copy()
    box2[4, 0] = np.nan                                                  # under a zero cotangent of its family: good
    lg = bt.state_slack_grad(d["q"], d["trunk_box_center"], g_slack=gs, model_id=mid)
    sess2 = dg.Session("nan", stream)
    lr = sess2.run(lambda: bt.state_slack_grad(sess2.put("q", q2, o["q"]), sess2.put("box", box2, o["trunk_box_center"]),
                                               g_slack=sess2.put("g_slack", gs2, None), model_id=dev_in["model_id"]))
    sess2.check("state_slack_grad")
    lr = dg.to_host(lr)
    assert np.array_equal(lr["grad_status"], np.where(np.isin(np.arange(B), [1, 2, 3]), capi.GRAD_NONFINITE, capi.GRAD_OK))
    for k in ("d_q", "d_trunk_box_center"):
        assert not lr[k][[1, 2, 3]].view(np.uint64).any() and _same(lr[k][[0, 5, 6]], lg[k][[0, 5, 6]]), k
    assert np.isfinite(lr["d_q"][4]).all() and _same(lr["which"][[0, 1, 5, 6]], lg["which"][[0, 1, 5, 6]]) and (lr["which"][3] == -1).all()
    bt.close()


# ---- 6. refusals
def test_refusals_name_their_field_and_come_before_any_launch():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("b5", "full", K)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, score=sg.SCORE, watch=WATCH, watch_trace=True)
    gam = sgc.watch_gammas(B, K, 31)
    bt.rollout_vjp(tape, g_q_final=np.ones((B, 26)))                     # (a plain call first: the workspace has its size, the statistic its -1)
    assert bt.stat("last_slackvjp_variant") == -1

    def refused(fn, word, code=capi.E_ARG):
        with pytest.raises(capi.WbcError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), (word, str(e.value))
        assert bt.stat("last_slackvjp_variant") == -1 and (dq0 == 7.0).all()

    keep = []
    tin = bt._tick_in(d, keep, B)
    tk, _ = bt._tracks_struct(tracks, B, keep)
    r = capi.WbcRollout()
    r.ticks, r.mode, r.hold_ticks = K, capi.ROLLOUT_RUNNING, 0
    og, tgr = capi.WbcRolloutGrad(), capi.WbcTracksGrad()
    dq0 = np.full((B, 26), 7.0)
    og.d_q0 = dq0.ctypes.data
    tick, q_final = np.ascontiguousarray(rec["slack_min_tick"]), np.ascontiguousarray(rec["q"])

    def seed(**kw):
        s = capi.WbcWatchSeed()
        s.mask = kw.pop("mask", MASK)
        vals = dict(g_slack_min=gam["g_slack_min"], g_slack_final=gam["g_slack_final"], g_trace=gam["g_trace"], slack_min_tick=tick, q_final=q_final)
        vals.update(kw)
        for k, v in vals.items():
            setattr(s, k, None if v is None else v.ctypes.data)
        return s

    def call(ws, rr=r, tin_=tin, tracks_p=C.byref(tk), out_p=C.byref(tgr), score=None):
        capi.check(bt.lib.wbc_rollout_vjp_watched(bt._h, B, C.byref(tin_), None, DT, C.byref(rr), tracks_p, tape.buf.data_ptr(), tape.buf.numel(), None,
                                                  score, None if ws is None else C.byref(ws), capi.MEM_HOST, C.byref(og), out_p, None), bt.lib)
    refused(lambda: call(None), "watch")
    refused(lambda: call(seed(g_slack_min=None, g_slack_final=None, g_trace=None)), "g_slack_min")
    refused(lambda: call(seed(slack_min_tick=None)), "slack_min_tick")
    refused(lambda: call(seed(q_final=None)), "q_final")
    for m_ in (0, 1 << 4, -1):
        refused(lambda: call(seed(mask=m_)), "mask")
    no_box = bt._tick_in({k: v for k, v in d.items() if k != "trunk_box_center"}, keep, B)
    refused(lambda: call(seed(), tin_=no_box), "trunk_box_center")
    refused(lambda: call(seed(), out_p=None), "tracks_out")
    refused(lambda: call(seed(), tracks_p=None), "tracks_out")
    ss = capi.WbcScoreSeed()
    refused(lambda: call(seed(), tracks_p=None, out_p=None, score=C.byref(ss)), "score")
    held = capi.WbcRollout()
    held.ticks, held.mode, held.hold_ticks = K, capi.ROLLOUT_RUNNING, 2
    refused(lambda: call(seed(), rr=held), "hold_ticks")
    # the record call: watch required, hold ticks refused, what wbc_rollout_watch refuses
    wt = capi.WbcSlackWatch()
    wt.mask = MASK

    def record(wp, rr=r, tin_=tin):
        capi.check(bt.lib.wbc_rollout_record_watch(bt._h, B, C.byref(tin_), None, DT, C.byref(rr), C.byref(tk), None, wp, tape.buf.data_ptr(),
                                                   tape.buf.numel(), None, capi.MEM_HOST, None), bt.lib)
    refused(lambda: record(None), "watch")
    refused(lambda: record(C.byref(wt), rr=held), "hold_ticks")
    refused(lambda: record(C.byref(wt), tin_=no_box), "trunk_box_center")
    bad = capi.WbcSlackWatch()
    refused(lambda: record(C.byref(bad)), "mask")
    # the layer
    q, box = np.ascontiguousarray(d["q"]), np.ascontiguousarray(d["trunk_box_center"])
    gs = np.ascontiguousarray(gam["g_slack_final"].T)
    lo = capi.WbcSlackGrad()
    ldq = np.full((B, 26), 7.0)
    lo.d_q = ldq.ctypes.data

    def layer(q_=q, box_=box, gs_=gs, gc_=None, out_=lo):
        p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        capi.check(bt.lib.wbc_state_slack_vjp(bt._h, B, p(q_), p(box_), None, p(gs_), p(gc_), capi.MEM_HOST, None if out_ is None else C.byref(out_), None), bt.lib)
    refused(lambda: layer(q_=None), "q")
    refused(lambda: layer(out_=None), "out")
    refused(lambda: layer(gs_=None), "g_slack")
    refused(lambda: layer(box_=None), "trunk_box_center")
    assert (ldq == 7.0).all()
    only = gs.copy()
    only[:, 1:3] = 0.0
    layer(box_=None, gs_=only)                                           # without a box and without a cotangent on the trunk families: runs
    assert bt.stat("last_slackvjp_variant") == KEY[("state", False)] and not (ldq == 7.0).any()
    # and with everything in place the sweep runs: a state seed is not required
    call(seed())
    assert bt.stat("last_slackvjp_variant") == KEY[("seed", False)] and not (dq0 == 7.0).any()
    assert bt.lib.wbc_variant_count(b"slackvjp") == 4
    mixed = tgp._handle(*_setup("mixed7", "full", K)[:2], 7, {})
    with pytest.raises(capi.WbcError) as e:
        mixed.state_slack_grad(np.zeros((7, 27)), np.zeros((7, 4)), g_slack=np.zeros((7, 4)))
    assert e.value.code == capi.E_ARG and "model_id" in str(e.value)
    mixed.close()
    bt.close()


# ---- 7. the handle
def test_a_plain_sweep_after_watched_calls_gives_the_bits_of_a_fresh_handle():
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("mixed7", "everything", K)
    state, gam = rv._seeds(B, K, 21, np.array([m.nv for m in models])[mid]), sgc.watch_gammas(B, K, 31)
    bt = tgp._handle(models, cfgs, B, {})
    _, tape0 = bt.rollout_record(d, DT, K, tracks=tracks)
    fresh = bt.rollout_vjp(tape0, **state)
    bt.close()
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K, tracks=tracks, watch=WATCH)
    bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam), **state)
    bt.rollout_vjp(tape, watch_seed=sgc.watch_seed_of(rec, gam))
    bt.state_slack_grad(d["q"], d["trunk_box_center"], g_slack=np.ones((B, 4)), model_id=mid)
    _, tape1 = bt.rollout_record(d, DT, K, tracks=tracks)
    after = bt.rollout_vjp(tape1, **state)
    assert tt._same_tapes(tape1, tape0)
    for (name, x), (_, y) in zip(_flat(after), _flat(fresh)):
        assert _same(x, y), name
    bt.close()


# ---- 8. the torch layer
def test_state_slack_layer_is_the_two_calls_bit_for_bit():
    import torch
    import wbc_torch
    models, cfgs, d, mid, B, _ = _setup("mixed7", "everything", 3)
    rng = np.random.default_rng(19)
    gs, gc_ = rng.normal(0, 1.0, (B, 4)), rng.normal(0, 1.0, (B, 12))
    bt = tgp._handle(models, cfgs, B, {})
    dev = _dev(d)
    q, box = dev["q"].clone().requires_grad_(True), dev["trunk_box_center"].clone().requires_grad_(True)
    slack, comp, which = wbc_torch.wbc_state_slack(q, box, bt, model_id=dev["model_id"])
    fwd = bt.state_slack(d["q"], d["trunk_box_center"], model_id=mid, want_components=True)
    assert _same(_host(slack.detach()), fwd["slack"]) and _same(_host(comp.detach()), fwd["components"]) and _same(_host(which), fwd["which"])
    assert slack.requires_grad and comp.requires_grad and not which.requires_grad
    ((slack * torch.from_numpy(gs).cuda()).sum() + (comp * torch.from_numpy(gc_).cuda()).sum()).backward()
    ref = bt.state_slack_grad(d["q"], d["trunk_box_center"], g_slack=gs, g_components=gc_, model_id=mid)
    assert _same(_host(q.grad), wbc_workload.tangent_to_raw(d["q"], ref["d_q"])) and _same(_host(box.grad), ref["d_trunk_box_center"])
    # a loss on the slack alone: the components' cotangent is left out of the call
    q2 = dev["q"].clone().requires_grad_(True)
    s2, _, _ = wbc_torch.wbc_state_slack(q2, dev["trunk_box_center"], bt, model_id=dev["model_id"])
    (s2 * torch.from_numpy(gs).cuda()).sum().backward()
    ref2 = bt.state_slack_grad(d["q"], d["trunk_box_center"], g_slack=gs, model_id=mid)
    assert _same(_host(q2.grad), wbc_workload.tangent_to_raw(d["q"], ref2["d_q"]))
    bt.close()


def _watched(bt, dev, dev_tracks, K, loss_of, rho=None):
    """-> (outputs on the host, d_q0 raw, per track dict(points, tangents, du) gradients)"""
    import torch
    import wbc_torch
    q0 = dev["q"].clone().requires_grad_(True)
    trk = None if dev_tracks is None else [{k: (v.clone().requires_grad_(True) if k in ("points", "tangents", "du") else v) for k, v in t.items()} for t in dev_tracks]
    res = wbc_torch.wbc_rollout_watched(q0, None, {k: v for k, v in dev.items() if k != "q"}, DT, K, bt, watch=WATCH, tracks=trk)
    q, qdot, st, q_trace, smin, sfin, trace, tick, wh = res
    assert smin.requires_grad and sfin.requires_grad and trace.requires_grad and not tick.requires_grad and not wh.requires_grad and not st.requires_grad
    loss = loss_of(smin, sfin, trace)
    if rho is not None:
        loss = loss + (q * torch.from_numpy(rho).cuda()).sum()
    loss.backward()
    grads = [] if trk is None else [{k: _host(n[k].grad) for k in ("points", "tangents", "du") if k in n} for n in trk]
    return [_host(t.detach()) for t in res], _host(q0.grad), grads


def test_watched_layer_is_the_record_and_the_sweep_bit_for_bit():
    import torch
    K = 3
    models, cfgs, d, mid, B, tracks = _setup("b5", "everything", K)
    rho, gam = np.random.default_rng(33).normal(0, 1.0, (B, 27)), sgc.watch_gammas(B, K, 31)
    dg_ = {k: torch.from_numpy(v).cuda() for k, v in gam.items()}
    bt = tgp._handle(models, cfgs, B, {})
    dev, dev_tracks = _dev(d), tt._dev_tracks(tracks)
    loss = lambda a, b, c: (a * dg_["g_slack_min"]).sum() + (b * dg_["g_slack_final"]).sum() + (c * dg_["g_trace"]).sum()      # noqa: E731
    res, g_q0, grads = _watched(bt, dev, dev_tracks, K, loss, rho)
    rec, tape = bt.rollout_record(dev, DT, K, tracks=dev_tracks, watch=WATCH, watch_trace=True)
    for i, k in enumerate(("q", "qdot", "status", "q_trace", "slack_min", "slack_final", "slack_trace", "slack_min_tick", "slack_min_which")):
        assert _same(res[i], _host(rec[k])), k
    seed = wbc_workload.raw_to_tangent(rec["q"], torch.from_numpy(rho).cuda()).contiguous()      # what the layer's backward does
    ref = bt.rollout_vjp(tape, g_q_final=seed, want=("d_q0",) + tt.TRACK_NAMES,
                         watch_seed=dict(mask=WATCH, q_final=rec["q"], slack_min_tick=rec["slack_min_tick"], **dg_))
    assert _same(g_q0, _host(wbc_workload.tangent_to_raw(dev["q"], ref["d_q0"])))
    for j in range(3):
        for k, v in grads[j].items():
            assert _same(v, _host(ref["tracks"][j]["d_" + k])), (j, k)
            assert np.abs(v).max() > 0
    # without tracks, and a loss on the trace alone: the other cotangents are left out of the call
    res1, g1, _ = _watched(bt, dev, None, K, lambda a, b, c: (c * dg_["g_trace"]).sum())
    rec1, tape1 = bt.rollout_record(dev, DT, K, watch=WATCH)
    ref1 = bt.rollout_vjp(tape1, want=("d_q0",), watch_seed=dict(mask=WATCH, q_final=rec1["q"], g_trace=dg_["g_trace"]))
    assert _same(g1, _host(wbc_workload.tangent_to_raw(dev["q"], ref1["d_q0"])))
    bt.close()


MAG = 4.0      # a slack is a difference of numbers below this: positions below 1 m, angles and joint limits below pi + trunk_box_ang


def _hinge_problem(cfg_name, seed):
    """the oracle chain along three generic tracks with the box displaced; margins at the upper quartile of each family's trace, so the squared hinge
    max(0, margin - slack)^2 is active on about three quarters of the (tick, instance) pairs and on every instance; smooth where it switches"""
    m, cfg, d, _, _ = th.sweep_setup(cfg_name, seed)
    d = sgc.displace_box(d)
    K, B = th.K_TICKS, len(d["q"])
    tracks = tg.three_tracks(d, K, seed + 50, generic=True)
    states, ticks, sides0, status = tg.track_chain(m, cfg, d, K, tq.DT, tracks)

    def trace_of(st):
        return np.stack([wbc_workload.state_slack(m, cfg, st[k + 1]["q"], d["trunk_box_center"], gq.StateFK([m]))["slack"].T for k in range(K)])
    margin = np.quantile(trace_of(states), 0.75, axis=(0, 2))

    def loss(st, tk):
        hinge = np.maximum(0.0, margin[None, :, None] - trace_of(st))
        return (hinge * hinge).sum(axis=(0, 1)), (2.0 * hinge * MAG).sum(axis=(0, 1))
    return dict(m=m, cfg=cfg, d=d, K=K, B=B, tracks=tracks, states=states, ticks=ticks, sides0=sides0, status=status, margin=margin, loss=loss)


@pytest.mark.parametrize("cfg_name,seed", [("full", 3)])
def test_backward_of_a_hinge_on_trace_against_central_differences_of_the_oracle_chain(cfg_name, seed, monkeypatch):
    """test_score_grad_host's item 3 with the device's gradients of sum max(0, margin - trace)^2: the same tracks, directions, rule and cap"""
    import torch
    p = _hinge_problem(cfg_name, seed)
    m, cfg, d, K, B, tracks = p["m"], p["cfg"], p["d"], p["K"], p["B"], p["tracks"]
    assert all((s == 0).all() for s in p["status"]) and (p["loss"](p["states"], p["ticks"])[0] > 0).all()
    margin, kappa = tg.margins(m, cfg, p["states"], p["ticks"], K)
    mg = torch.from_numpy(p["margin"]).cuda()[None, :, None]
    bt = tgp._handle([m], [cfg], B, {})
    res, _, g = _watched(bt, _dev(d), tt._dev_tracks(tracks), K, lambda a, b, c: (torch.clamp(mg - c, min=0.0) ** 2).sum())
    bt.close()
    assert (res[2] == 0).all()
    g = [{"d_" + k: v for k, v in t.items()} for t in g]
    rho = np.zeros((B, capi.Q_STRIDE))
    rho[:, :3] = sh.RHO
    monkeypatch.setattr(tg, "track_chain", sh.loss_in_q(p["loss"]))
    for name, p_, v_, u_, ana, terms in sh.directional_cases(p, g, seed):
        keep, ok, line = tg.track_chain_directional(m, cfg, d, rho, K, DT, lambda s: tg.perturbed(tracks, s, p_, v_, u_), p["sides0"], margin, kappa,
                                                    ana, terms, "%s / seed %d, K = %d, watched layer, %s" % (cfg_name, seed, K, name))
        print(line)
        assert (~keep).sum() <= B // 4 and ok, line
        assert np.abs(ana).max() > 0
