"""Shared by tools/make_sweep_golden.py and test_gpu_sweep_recorded.py: the inputs, the sequence of recorded roll-outs along tracks with their
reverse sweeps (track adjoint, score seed) and the list of refused calls whose results tests/golden/sweep_recorded.npz holds (DESIGN.md
§3.47). grad_recorded_cases.py's shapes: max_batch = 12 and B = 9 (two full four-instance waves and a short one; workspace strides differ from
output strides), K = 4, ONE long-lived handle per configuration (`rows` and `norows` of grad_recorded_cases.CONFIGS) with the calls in the
order of CALLS, so that what a call leaves in the handle's workspaces is part of what is held. Row BAD holds a NaN in one track: a tangent in
`six`, a milestone in `two`.

  six   all six targets followed (the adjoint kernel's second pass runs): LINEAR, HERMITE with default tangents and HERMITE with the
        caller's tangents mixed, max_points = 5, n_points of {2, 3, 5} and du per instance so that within the K ticks an instance stays in
        its first segment, one passes an interior milestone and one reaches t >= n - 1; the four default-tangent cases are built in
  two   the gripper and the trunk, one du_all for all instances, n_points = NULL

Only WbcBatch's and wbc_torch's public entry points are used (and the wrappers' struct builders for the refusals they cannot reach)."""
import ctypes as C
import hashlib

import numpy as np

import grad_recorded_cases as gr
import track_grad_common as tg
import wbc_capi as capi
import wbc_workload

MAX_BATCH, B, DT, K, BAD, S = gr.MAX_BATCH, gr.B, gr.DT, 4, gr.BAD, 5
CONFIGS = {k: gr.CONFIGS[k] for k in ("rows", "norows")}
STATS = ("last_rollvjp_variant", "last_trackvjp_variant", "last_scorevjp_variant")
SENTINEL = gr.SENTINEL
SIX = ((0, "linear", False), (1, "hermite", False), (2, "hermite", True), (3, "linear", False), (4, "hermite", False), ("trunk", "hermite", True))
SIX_SCORE, TWO_SCORE = (0, 4, "trunk"), (4,)
DU = (0.2, 0.45, 0.3, 0.4, 0.25, 0.7, 0.15, 0.9, 0.55)
DU_ALL, S_TWO = 0.35, 3
TRACK_KEYS = ("points", "tangents", "n_points", "du")
CALLS = ("rec_six_cold", "six_final", "six_qdot", "six_trace", "six_all", "six_subset", "six_out", "six_score_sq", "six_score_fin", "six_score_max",
         "six_score_state", "six_score_zero", "rec_six_warm", "six_warm_all", "six_warm_score", "rec_two_cold", "two_all", "two_score", "plain",
         "torch_fused", "torch_scored_scores", "torch_scored_q", "torch_scored_mixed")
FULL = {"rows": ("rec_six_cold", "six_score_state", "torch_scored_mixed")}
same = gr.same


def pack(name, call, v):
    """grad_recorded_cases.pack with this file's FULL"""
    if v.dtype.kind == "i" or call in FULL.get(name, ()):
        return v
    return np.array("%s|%s|%s" % (v.dtype.str, v.shape, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()))


def make_tracks(d, seed):
    """-> (six, two): lists of track dicts of numpy arrays around the targets of the inputs d"""
    rng = np.random.default_rng(seed + 60)
    rows = np.arange(B)
    six = []
    for j, (target, kind, own) in enumerate(SIX):
        base = d["trunk_target"] if target == "trunk" else d["ee_target"].reshape(B, 5, 3)[:, target]
        pts = base[:, None, :] + rng.uniform(-0.01, 0.01, (B, S, 3))
        n = np.array([2, 3, 5], np.int32)[(rows + j) % 3]
        du = np.array(DU)[(rows + 2 * j) % len(DU)]
        if kind == "hermite" and not own:      # the default-tangent cases at milestone 1, built in (track_grad_common.CASE, a centimetre wide)
            first = [b for b in rows if b != BAD and n[b] >= 3 and du[b] < 1.0 / (K - 1)][:2]      # (every tick in segment 0: it reads milestone 1's tangent)
            for b, cs in zip(first, ((1, 2, 3), (4, -2, -3))):
                for c, case in enumerate(cs):
                    pts[b, 0:3, c] = base[b, c] + (0.01 / 3.0) * np.array(tg.CASE[case])
        t = dict(target=target, kind=kind, points=np.ascontiguousarray(pts), n_points=n, du=np.ascontiguousarray(du))
        if own:
            t["tangents"] = rng.uniform(-0.01, 0.01, (B, S, 3))
        six.append(t)
    six[2]["tangents"][BAD, 1, 0] = np.nan      # (a tangent: the row is bad only to a test that reads the tangents; `two` has the bad milestone)
    two = []
    for target, kind in ((4, "linear"), ("trunk", "hermite")):
        base = d["trunk_target"] if target == "trunk" else d["ee_target"].reshape(B, 5, 3)[:, target]
        two.append(dict(target=target, kind=kind, points=np.ascontiguousarray(base[:, None, :] + rng.uniform(-0.01, 0.01, (B, S_TWO, 3))), du=DU_ALL))
    two[1]["points"][BAD, 0, 1] = np.nan
    return six, two


def coverage(tracks, ticks=K):
    """-> (the clamp branches, the default-tangent cases) that the ticks 0 .. ticks - 1 evaluate on the rows other than BAD"""
    branches, cases = set(), set()
    for t in tracks:
        p = t["points"]
        n = np.full(B, p.shape[1]) if t.get("n_points") is None else t["n_points"]
        du = np.broadcast_to(np.asarray(t["du"], dtype=np.float64), (B,))
        for b in range(B):
            if b == BAD:
                continue
            for k in range(ticks):
                x = float(k) * float(du[b])
                if x <= 0.0 or x >= float(n[b] - 1):
                    branches.add("first" if x <= 0.0 else "last")
                    continue
                branches.add("inside")
                i = int(np.floor(x))
                if t["kind"] == "hermite" and t.get("tangents") is None and n[b] >= 3:
                    for mi in (i, i + 1):
                        if 0 < mi < n[b] - 1:
                            cases |= {wbc_workload._tangent_case(p[b, mi - 1, c], p[b, mi, c], p[b, mi + 1, c]) for c in range(3)}
    return branches, cases


def make_inputs(seed=7):
    """-> dict of numpy arrays "<configuration>__<name>" ("both__<name>" where the configurations share the bits): the tick inputs ("d_*"), the
    tracks ("six<j>_*", "two<j>_*") and every other argument of the calls. Made once by the tool and stored with the outputs: the oracle FK's
    last bit depends on the host libm."""
    per = {}
    for name in CONFIGS:
        models, cfgs, d, mid = gr.problem(name, seed)
        assert "trunk_target" in d and "prev_trunk_target" in d, "the trunk track needs a trunk target among the inputs"
        rng = np.random.default_rng(seed + 41)
        nvs = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
        beyond = np.arange(26)[None, :] >= nvs[:, None]
        x = {"d_" + k: np.asarray(v).copy() for k, v in d.items()}
        x["task_params"] = gr.tgp._random_rows(gr.tgp._rows_of(cfgs, mid, B), 12, w=(0.8, 1.25), g=(0.8, 1.25))
        for k, scale, shape in (("g_q_final", 1.0, (B, 26)), ("g_qdot_last", 1e-3, (B, 26)), ("g_q_trace", 1.0, (K, B, 26))):
            x[k] = rng.normal(0, scale, shape)
            x[k][..., beyond] = 0.0
        for k in ("g_sq", "g_fin", "g_max"):
            x[k] = rng.normal(0, 1.0, (len(SIX_SCORE), B))
        x["ee_step"], x["trunk_step"] = rng.normal(0, 2e-4, (B, 5, 3)), np.tile((0.0005, 0.0, -0.0005), (B, 1))
        x["rho_qdot"], x["rho_q"], x["rho_trace"] = rng.normal(0, 1.0, (B, 26)), rng.normal(0, 1.0, (B, 27)), rng.normal(0, 1.0, (K, B, 27))
        x["nvs"] = nvs
        for tag, tracks in zip(("six", "two"), make_tracks(d, seed)):
            for j, t in enumerate(tracks):
                x.update({"%s%d_%s" % (tag, j, k): np.asarray(t[k]) for k in TRACK_KEYS if t.get(k) is not None})
        per[name] = x
    z = {}
    for name, x in per.items():
        for k, v in x.items():
            shared = all(k in o and same(np.asarray(o[k]), np.asarray(v)) for o in per.values())
            z["%s__%s" % ("both" if shared else name, k)] = v
    return z


def inputs_of(z, name):
    """the arrays of configuration `name` from make_inputs' dict, under their names without the configuration"""
    return {k.split("__", 1)[1]: np.ascontiguousarray(v) for k, v in z.items() if k.split("__", 1)[0] in (name, "both")}


def tracks_of(a, tag, conv=lambda v: v):
    """the track dicts of set `tag` from the arrays a of one configuration (make_inputs' names without the configuration)"""
    spec = SIX if tag == "six" else ((4, "linear", False), ("trunk", "hermite", False))
    out = []
    for j, (target, kind, _) in enumerate(spec):
        t = dict(target=target, kind=kind)
        for k in TRACK_KEYS:
            v = a.get("%s%d_%s" % (tag, j, k))
            if v is not None:
                t[k] = float(np.reshape(v, ())) if np.size(v) == 1 else conv(np.ascontiguousarray(v))      # (one number: du_all)
        out.append(t)
    return out


handle = gr.handle
_np = gr._np


def _tape_hash(tape, warm):
    """SHA-256 over the blocks a record writes of every tick (the padding word and, cold, the working sets are never written)"""
    h = hashlib.sha256()
    for k in range(tape.ticks):
        for key, v in sorted(tape.tick(k).items()):
            if warm or key != "working_set":
                h.update(np.ascontiguousarray(_np(v)).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def _flat(r):
    """rollout_vjp's dict with the per-track dicts under "t<j>_<name>" """
    out = {k: v for k, v in r.items() if k != "tracks"}
    for j, t in enumerate(r.get("tracks", ())):
        out.update({"t%d_%s" % (j, k): v for k, v in t.items()})
    return out


def run_cases(bt, name, z, conv=lambda a: a):
    """Yields (call, outputs as numpy arrays, the STATS after the call) in the order of CALLS for configuration `name` on its handle bt. conv:
    what every input array goes through (the identity: numpy, the library stages them; to a torch device tensor: the pointers pass through).
    The torch layers always run on device tensors."""
    import torch
    import wbc_torch
    raw = inputs_of(z, name)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()      # noqa: E731
    a = {k: conv(v) for k, v in raw.items()}
    t = {k: dev(v) for k, v in raw.items()}
    d = {k[2:]: v for k, v in a.items() if k.startswith("d_")}
    td = {k[2:]: v for k, v in t.items() if k.startswith("d_")}
    tp = a["task_params"]
    seeds = dict(g_q_final=a["g_q_final"], g_qdot_last=a["g_qdot_last"], g_q_trace=a["g_q_trace"])
    sets = dict(six=(tracks_of(raw, "six", conv), SIX_SCORE), two=(tracks_of(raw, "two", conv), TWO_SCORE))
    state = {}

    def record(tag, warm):
        tracks, score = sets[tag]
        bt.set_option("warm_start", warm)
        try:
            rec, tape = bt.rollout_record(d, DT, K, task_params=tp, tracks=tracks, score=score)
            state.update(rec=rec, tape=tape, warm=warm, ns=len(score), score=score)
            return dict({"rec_" + k: v for k, v in rec.items()}, tape=_tape_hash(tape, warm))
        finally:
            bt.set_option("warm_start", 0)

    def score_seed(*which, zero=False):
        ns, rec = state["ns"], state["rec"]
        sd = dict(mask=state["score"], q_final=rec["q"])
        for k in which:
            g = np.ascontiguousarray(raw[k][:ns])
            sd["g_err_" + dict(g_sq="sq_sum", g_fin="final", g_max="max")[k]] = conv(np.zeros_like(g) if zero else g)
        if "g_max" in which:
            sd["err_max_tick"] = rec["err_max_tick"]
        return sd

    def vjp(**kw):
        bt.set_option("warm_start", state["warm"])
        try:
            return _flat(bt.rollout_vjp(state["tape"], **kw))
        finally:
            bt.set_option("warm_start", 0)

    def vjp_out():
        """the call of six_all into the caller's arrays, the tracks' among them"""
        r = bt.rollout_vjp(state["tape"], **seeds)
        fill = lambda v: torch.full_like(v, int(SENTINEL)) if hasattr(v, "cpu") else np.full_like(v, int(SENTINEL))      # noqa: E731
        out = {k: fill(v) for k, v in r.items() if k != "tracks"}
        out["tracks"] = [{k: fill(v) for k, v in tr.items()} for tr in r["tracks"]]
        bt.rollout_vjp(state["tape"], out=out, **seeds)
        return _flat(out)      # (the caller's own arrays)

    def plain():
        rec, tape = bt.rollout_record(d, DT, K, ee_target_step=a["ee_step"], trunk_target_step=a["trunk_step"], task_params=tp)
        return dict({"rec_" + k: v for k, v in rec.items()}, tape=_tape_hash(tape, 0), **bt.rollout_vjp(tape, **seeds))

    def leaf(x):
        return x.clone().requires_grad_(True)

    def torch_layer(scored, loss):
        q0, tpl = leaf(td["q"]), leaf(t["task_params"])
        tracks = [{k: (leaf(v) if torch.is_tensor(v) and v.dtype == torch.float64 else v) for k, v in tr.items()} for tr in tracks_of(raw, "six", dev)]
        rest = {k: v for k, v in td.items() if k != "q"}
        if scored:
            out = wbc_torch.wbc_rollout_tracks_scored(q0, tpl, tracks, rest, DT, K, bt, score=SIX_SCORE)
        else:
            out = wbc_torch.wbc_rollout_tracks_fused(q0, tpl, tracks, rest, DT, K, bt)
        names = ("q", "qdot", "status", "q_trace", "err_sq_sum", "err_final", "err_max", "err_max_tick")[:len(out)]
        o = dict(zip(names, out))
        total = 0.0
        if "state" in loss:
            total = total + (o["q"] * t["rho_q"]).sum()
        if "trace" in loss:
            total = total + (o["qdot"] * t["rho_qdot"]).sum() + (o["q_trace"] * t["rho_trace"]).sum()
        if "scores" in loss:
            total = total + (o["err_sq_sum"] * t["g_sq"]).sum() + (o["err_final"] * t["g_fin"]).sum() + (o["err_max"] * t["g_max"]).sum()
        total.backward()
        o.update(g_q0=q0.grad, g_task_params=tpl.grad)
        for j, tr in enumerate(tracks):
            o.update({"g_t%d_%s" % (j, k): v.grad for k, v in tr.items() if torch.is_tensor(v) and v.requires_grad})
        return o

    both = ("g_sq", "g_fin", "g_max")
    calls = {
        "rec_six_cold": lambda: record("six", 0),
        "six_final": lambda: vjp(g_q_final=seeds["g_q_final"]),
        "six_qdot": lambda: vjp(g_qdot_last=seeds["g_qdot_last"]),
        "six_trace": lambda: vjp(g_q_trace=seeds["g_q_trace"]),
        "six_all": lambda: vjp(**seeds),
        "six_subset": lambda: vjp(want=("d_q0", "d_ee_target", "d_points"), **seeds),
        "six_out": vjp_out,
        "six_score_sq": lambda: vjp(score_seed=score_seed("g_sq")),
        "six_score_fin": lambda: vjp(score_seed=score_seed("g_fin")),
        "six_score_max": lambda: vjp(score_seed=score_seed("g_max")),
        "six_score_state": lambda: vjp(score_seed=score_seed(*both), **seeds),
        "six_score_zero": lambda: vjp(score_seed=score_seed(*both, zero=True), **seeds),      # the bits of six_all
        "rec_six_warm": lambda: record("six", 1),
        "six_warm_all": lambda: vjp(**seeds),
        "six_warm_score": lambda: vjp(score_seed=score_seed(*both), g_q_final=seeds["g_q_final"]),
        "rec_two_cold": lambda: record("two", 0),
        "two_all": lambda: vjp(**seeds),
        "two_score": lambda: vjp(score_seed=score_seed(*both), g_qdot_last=seeds["g_qdot_last"]),
        "plain": plain,      # after the track calls: the sweep without extensions on the workspace they left
        "torch_fused": lambda: torch_layer(False, ("state", "trace")),
        "torch_scored_scores": lambda: torch_layer(True, ("scores",)),
        "torch_scored_q": lambda: torch_layer(True, ("state",)),
        "torch_scored_mixed": lambda: torch_layer(True, ("state", "trace", "scores")),
    }
    assert tuple(calls) == CALLS
    for call, fn in calls.items():
        got = fn()
        stats = np.array([bt.stat(s) for s in STATS], np.int64)
        yield call, {k: _np(x) for k, x in got.items() if x is not None}, stats


# ---------------------------------------------------------------------------------------------- the score seed without rotated placements
# Both configurations hold laikago_vx300, so every call above launches wbc_scorevjp_kernel<SEED, ROT>. One record and one scored sweep on
# a1_wx200 alone at B = 5 (one full four-instance wave and one with three padding rows) launch <SEED, no ROT>. The inputs are `rows`' own: its
# a1_wx200 instances (model_id 0), repeated to five rows; nothing new is stored for them. The outputs are "b5__*" in the same file.
B5 = 5


def b5_rows(raw):
    """-> the five rows of configuration `rows` (inputs_of's dict) the case runs on"""
    own = np.flatnonzero(raw["d_model_id"] == 0)
    assert len(own) >= 2 and BAD not in own
    return own[np.arange(B5) % len(own)]


def run_b5(z, conv=lambda a: a):
    """-> (outputs of the record and of the scored sweep as numpy arrays, last_scorevjp_variant) on a handle of its own"""
    raw = inputs_of(z, "rows")
    idx = b5_rows(raw)
    cut = lambda v: conv(np.ascontiguousarray(v[idx]))      # noqa: E731
    d = {k[2:]: cut(v) for k, v in raw.items() if k.startswith("d_") and k != "d_model_id"}
    tracks = []
    for t in tracks_of(raw, "six"):
        tracks.append({k: (cut(v) if isinstance(v, np.ndarray) else v) for k, v in t.items()})
    ns = len(SIX_SCORE)
    m = gr.tgp._model("a1_wx200")
    bt = gr.tgp._handle([m], [gr.common.config(CONFIGS["rows"][0], m)], MAX_BATCH, {})
    try:
        rec, tape = bt.rollout_record(d, DT, K, task_params=cut(raw["task_params"]), tracks=tracks, score=SIX_SCORE)
        sd = dict(mask=SIX_SCORE, q_final=rec["q"], err_max_tick=rec["err_max_tick"])
        for k, name in (("g_sq", "sq_sum"), ("g_fin", "final"), ("g_max", "max")):
            sd["g_err_" + name] = conv(np.ascontiguousarray(raw[k][:ns][:, idx]))
        g = _flat(bt.rollout_vjp(tape, score_seed=sd, g_q_final=cut(raw["g_q_final"])))
        out = dict({"rec_" + k: v for k, v in rec.items()}, **g)
        return {k: _np(v) for k, v in out.items() if v is not None}, int(bt.stat("last_scorevjp_variant"))
    finally:
        bt.close()


# ---------------------------------------------------------------------------------------------- refusals
def run_refusals(bt, z):
    """Yields (name, code, message, ok) of every refused call of the sweep's own checks, on the `rows` handle bt: the tracks call's checks as
    the sweep reaches them (tracks == NULL first), the track outputs' (TrackAdjExt::check), the score seed's (ScoreSeedExt::check) and "score is
    required". ok: every output the call was given still holds SENTINEL and the tape its bytes. No call launches a kernel."""
    import torch
    raw = inputs_of(z, "rows")
    d = {k[2:]: v for k, v in raw.items() if k.startswith("d_")}
    six = tracks_of(raw, "six")
    six[2]["tangents"] = np.where(np.isnan(six[2]["tangents"]), 0.0, six[2]["tangents"])
    tape = torch.full((B * (capi.TAPE_HEAD_BYTES + K * capi.TAPE_TICK_BYTES),), 5, dtype=torch.uint8, device="cuda")
    f, alive = np.float64, []
    P = bt._p
    g = np.ones((B, 26))
    ns = len(SIX_SCORE)
    mask = sum(1 << (capi.TARGET_TRUNK if s == "trunk" else s) for s in SIX_SCORE)

    def call(scored, tracks=six, tracks_null=False, tg_null=False, track_outs=(), outs=("d_q0",), state_seed=True, score_null=False, score=None,
             imu=None, inputs=d, edit=None, out_null=False):
        """one raw call of wbc_rollout_vjp_tracks (scored False) or wbc_rollout_vjp_scored -> (return code, the caller-owned outputs)"""
        keep, owned = [], []

        def mine(shape, dtype=f):
            owned.append(np.full(shape, int(SENTINEL), dtype))
            return P(owned[-1], dtype, keep)
        tin = bt._tick_in(inputs, keep, B)
        r = capi.WbcRollout()
        r.ticks, r.mode, r.hold_ticks = K, capi.ROLLOUT_RUNNING, 0
        r.imu = P(imu, f, keep)
        tk, _ = bt._tracks_struct(tracks, B, keep)
        if edit is not None:
            edit(tk, r)
        sd = capi.WbcRolloutSeed()
        if state_seed:
            sd.g_q_final = P(g, f, keep)
        o = capi.WbcRolloutGrad()
        for n in outs:
            setattr(o, n, mine((B,) + capi.ROLLOUT_GRAD_FIELDS[n]))
        o.grad_status, o.ticks_dropped = mine(B, np.int32), mine(B, np.int32)
        tgr = capi.WbcTracksGrad()
        for j, n in track_outs:
            setattr(tgr.track[j], n, mine((B,) if n == "d_du" else (B, S, 3)))
        ss = capi.WbcScoreSeed()
        sc = dict(score_mask=mask, g_err_sq_sum=np.ones((ns, B)), q_final=d["q"])
        sc.update(score or {})
        ss.score_mask = sc["score_mask"]
        for n in capi.SCORE_SEED_FIELDS:
            setattr(ss, n, P(sc.get(n), np.int32 if n == "err_max_tick" else f, keep))
        head = (bt._h, B, C.byref(tin), None, DT, C.byref(r), None if tracks_null else C.byref(tk), tape.data_ptr(), tape.numel(), C.byref(sd))
        tail = (capi.MEM_HOST, None if out_null else C.byref(o), None if tg_null else C.byref(tgr), None)
        if scored:
            rc = bt.lib.wbc_rollout_vjp_scored(*head, None if score_null else C.byref(ss), *tail)
        else:
            rc = bt.lib.wbc_rollout_vjp_tracks(*head, *tail)
        return rc, owned

    def two_of_a_target(tk, r):
        tk.track[1].target = tk.track[0].target

    def set_field(**kw):
        def edit(tk, r):
            for k, v in kw.items():
                setattr(tk.track[0] if hasattr(tk.track[0], k) else (tk if hasattr(tk, k) else r), k, v)
        return edit
    no_trunk = {k: v for k, v in d.items() if k not in ("trunk_target", "prev_trunk_target")}
    ee_only = [t for t in six if t["target"] != "trunk"]
    cases = []
    add = lambda name, **kw: cases.append((name, kw))      # noqa: E731
    # "score is required", then the tracks call's checks as the sweep reaches them
    add("scored/score_null", scored=True, score_null=True, tracks_null=True)
    add("tracks/tracks_null", scored=False, tracks_null=True, tg_null=True)
    add("scored/tracks_null", scored=True, tracks_null=True)
    add("tracks/ee_target_step", scored=False, edit=set_field(ee_target_step=P(np.zeros((B, 15)), f, alive)))
    add("tracks/hold_ticks", scored=False, edit=set_field(hold_ticks=1))
    add("tracks/n_tracks", scored=False, edit=set_field(n_tracks=capi.MAX_TRACKS + 1))
    add("tracks/target_range", scored=False, edit=set_field(target=capi.TARGET_TRUNK + 1))
    add("tracks/target_repeated", scored=False, edit=two_of_a_target)
    add("tracks/kind", scored=False, edit=set_field(kind=7))
    add("tracks/max_points", scored=False, edit=set_field(max_points=1))
    add("tracks/points", scored=False, edit=set_field(points=None))
    add("tracks/linear_tangents", scored=False, edit=set_field(tangents=P(np.zeros((B, S, 3)), f, alive)))
    add("tracks/du_all", scored=False, edit=set_field(du=None, du_all=0.0))
    add("tracks/trunk_target_step", scored=False, edit=set_field(trunk_target_step=P(np.zeros((B, 3)), f, alive)))
    add("tracks/trunk_target", scored=False, inputs=no_trunk)
    add("tracks/out_null", scored=False, outs=(), out_null=True)
    # the track outputs
    add("grad/tracks_out_null", scored=False, tg_null=True)
    add("grad/d_ee_target_step", scored=False, outs=("d_q0", "d_ee_target_step"), track_outs=((0, "d_points"),))
    add("grad/beyond_n_tracks", scored=False, tracks=ee_only, track_outs=((0, "d_points"), (5, "d_du")))
    add("grad/d_trunk_target_step", scored=False, outs=("d_q0", "d_trunk_target_step"), track_outs=((5, "d_points"),))
    add("grad/d_tangents_linear", scored=False, track_outs=((0, "d_tangents"),))
    add("grad/d_tangents_default", scored=False, track_outs=((1, "d_tangents"),))
    add("scored/d_tangents_default", scored=True, track_outs=((4, "d_tangents"),))
    add("tracks/no_seed", scored=False, state_seed=False, track_outs=((0, "d_points"),))
    # the score seed
    add("score/no_cotangent", scored=True, state_seed=False, score=dict(g_err_sq_sum=None), track_outs=((0, "d_points"),))
    add("score/err_max_tick", scored=True, score=dict(g_err_max=np.ones((ns, B))), track_outs=((0, "d_points"),))
    add("score/q_final", scored=True, score=dict(q_final=None), track_outs=((0, "d_points"),))
    add("score/mask_zero", scored=True, score=dict(score_mask=0), track_outs=((0, "d_points"),))
    add("score/mask_beyond", scored=True, score=dict(score_mask=1 << capi.MAX_TRACKS), track_outs=((0, "d_points"),))
    add("score/trunk_target", scored=True, tracks=ee_only, inputs=no_trunk, track_outs=((0, "d_points"),))
    add("score/imu", scored=True, imu=d["q"][:, 3:7].copy(), track_outs=((0, "d_points"),))
    for name, kw in cases:
        rc, owned = call(**kw)
        msg = bt.lib.wbc_last_error().decode() if rc != 0 else "not refused"
        bt.synchronize()
        ok = all((v == int(SENTINEL)).all() for v in owned) and bool((tape == 5).all())
        yield name, rc, msg, ok

