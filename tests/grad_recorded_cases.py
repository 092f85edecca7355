"""Shared by tools/make_grad_golden.py and test_gpu_grad_recorded.py: the inputs, the sequence of gradient calls and the list of refused calls
whose results tests/golden/grad_recorded.npz holds. Three configurations, each on ONE long-lived handle of max_batch = 12
with B = 9 (two full packed waves and a short one; workspace strides differ from output strides), in the order of CONFIGS and CALLS, so that
what an earlier call left in the handle's workspaces is part of what is held:

  rows    `everything` over a1_wx200, a1_px100_pin_ver (nv < 26: padding rows) and laikago_vx300 (rotated placements), interleaved by model_id
  norows  `full` over the same models: no constraint rows, the p == 0 branch
  c3s3    c3 over a1_wx200, the first nine instances of test_step_grad_host.sweep_setup("c3", 3): instances that go unsolved after tick 0

Row BAD of q holds a NaN in every call. Only WbcBatch's and wbc_torch's public entry points are used (and _tick_in for the refusals that the
wrappers cannot reach)."""
import ctypes as C
import hashlib

import numpy as np

import common
import step_common as sc
import test_gpu_step_grad as tsg
import test_gpu_task_params as tgp
import test_step_grad_host as th
import wbc_capi as capi
import wbc_model
from wbc_batch import RolloutTape, WbcBatch

MAX_BATCH, B, DT, K, BAD = 12, 9, 0.002, 3, 4
CONFIGS = {"rows": ("everything", sc.MODELS), "norows": ("full", sc.MODELS), "c3s3": ("c3", ["a1_wx200"])}
STATS = ("last_grad_variant", "last_gradq_variant", "last_stepvjp_variant", "last_rollvjp_variant")
RUNNING, WARMUP = capi.ROLLOUT_RUNNING, capi.ROLLOUT_WARMUP
CALLS = ("rollout_q0_only", "certificate", "tick_vjp", "tick_vjp_subset", "tick_vjp_q_con", "tick_vjp_state", "tick_grad", "tick_grad_q", "step_vjp_running",
         "step_vjp_warmup", "rollout_cold", "rollout_warm", "rollout_final", "rollout_qdot", "rollout_trace", "rollout_warmup",
         "torch_tick", "torch_tick_state", "torch_step", "torch_fused")
SENTINEL = 7.0
FULL = {"rows": ("certificate", "tick_vjp", "tick_vjp_state", "step_vjp_running", "rollout_cold", "torch_fused")}


def pack(name, call, v):
    """What the fixture holds of one output: the array itself for the integer outputs and for the calls of FULL, else its dtype, shape and the
    SHA-256 of its bytes (the file stays small; a difference still names the output)."""
    if v.dtype.kind == "i" or call in FULL.get(name, ()):
        return v
    return np.array("%s|%s|%s" % (v.dtype.str, v.shape, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()))


def same(got, want):
    """pack()'s results compared: dtype, shape and bits"""
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def problem(name, seed=7):
    """-> (models, cfgs, tick inputs, model_id or None) of a configuration, without the bad row"""
    cfg_name, names = CONFIGS[name]
    if name == "c3s3":
        m, cfg, d, _, _ = th.sweep_setup("c3", 3)
        return [m], [cfg], {k: np.ascontiguousarray(v[:B]) for k, v in d.items()}, None
    return tgp._problem(names, cfg_name, B, seed=seed, with_rot=True)


def make_inputs(seed=7):
    """-> dict of numpy arrays "<configuration>__<name>": the tick inputs ("d_*") and every other argument of the calls. Made once by the tool
    and stored with the outputs: the oracle FK's last bit depends on the host libm."""
    z = {}
    for name in CONFIGS:
        models, cfgs, d, mid = problem(name, seed)
        rng = np.random.default_rng(seed + 40)
        nvs = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
        beyond = np.arange(26)[None, :] >= nvs[:, None]
        x = {"d_" + k: np.asarray(v).copy() for k, v in d.items()}
        x["d_q"][BAD, 9] = np.nan
        x["task_params"] = tgp._random_rows(tgp._rows_of(cfgs, mid, B), 12, w=(0.8, 1.25), g=(0.8, 1.25))
        for k, scale, shape in (("v", 1.0, (B, 26)), ("g_q_final", 1.0, (B, 26)), ("g_qdot_last", 1e-3, (B, 26)), ("g_q_trace", 1.0, (K, B, 26))):
            x[k] = rng.normal(0, scale, shape)
            x[k][..., beyond] = 0.0
        x["ee_step"], x["trunk_step"] = rng.normal(0, 2e-4, (B, 5, 3)), np.tile((0.0005, 0.0, -0.0005), (B, 1))
        x["imu"] = d["q"][:, 3:7].copy()
        x["rho_qdot"], x["rho_q"], x["rho_trace"] = rng.normal(0, 1.0, (B, 26)), rng.normal(0, 1.0, (B, 27)), rng.normal(0, 1.0, (K, B, 27))
        x["nvs"] = nvs
        z.update({"%s__%s" % (name, k): v for k, v in x.items()})
    return z


def handle(name, options=None):
    cfg_name, names = CONFIGS[name]
    models = [tgp._model(n) for n in names]
    bt = WbcBatch(models, MAX_BATCH)
    for i, m in enumerate(models):
        bt.configure(common.config(cfg_name, m), i)
    for k, v in (options or {}).items():
        bt.set_option(k, v)
    return bt


def _np(v):
    return v.detach().cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def run_cases(bt, name, z, conv=lambda a: a):
    """Yields (call, outputs as numpy arrays, the STATS after the call, the constraint rows) in the order of CALLS for configuration `name` on its handle bt. conv:
    what every input array goes through (the identity: numpy, the library stages them; to a torch device tensor: the pointers pass through).
    The torch layers always run on device tensors."""
    import torch
    import wbc_torch
    pre = name + "__"
    a = {k[len(pre):]: conv(np.ascontiguousarray(v)) for k, v in z.items() if k.startswith(pre)}
    t = {k[len(pre):]: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in z.items() if k.startswith(pre)}
    d = {k[2:]: v for k, v in a.items() if k.startswith("d_")}
    td = {k[2:]: v for k, v in t.items() if k.startswith("d_")}
    tp, v = a["task_params"], a["v"]
    seeds = dict(g_q_final=a["g_q_final"], g_qdot_last=a["g_qdot_last"], g_q_trace=a["g_q_trace"])
    p = bt.constraint_rows
    state = {}

    def certificate():
        state["c"] = bt.tick_certificate(d, DT, task_params=tp, v=v)
        return state["c"]

    def vjp(**kw):
        c = state["c"]
        return bt.tick_vjp(kw.pop("inputs", d), DT, c["qdot"], c["sens_x"], status=c["status"], cert_status=c["cert_status"], task_params=tp, **kw)

    def vjp_state():
        c = state["c"]
        return bt.tick_vjp_state(d, DT, c["qdot"], c["sens_x"], sens_bounds=c["sens_bounds"], sens_rows=c["sens_rows"], y_rows=c["y_rows"],
                                 status=c["status"], cert_status=c["cert_status"], working_set=c["working_set"], task_params=tp)

    def step(mode, imu):
        return bt.step_vjp(d["q"], state["c"]["qdot"], d["ee_target"], a["g_q_final"], DT, imu=imu, model_id=d.get("model_id"), mode=mode)

    def rollout(warm, mode=RUNNING, steps=True, want=None, **sd):
        bt.set_option("warm_start", warm)
        try:
            rec, tape = bt.rollout_record(d, DT, K, ee_target_step=a["ee_step"] if steps else None,
                                          trunk_target_step=a["trunk_step"] if steps and "trunk_target" in d else None,
                                          imu=a["imu"] if mode == RUNNING else None, mode=mode, task_params=tp)
            g = bt.rollout_vjp(tape, want=want, **sd)
        finally:
            bt.set_option("warm_start", 0)
        return dict({"rec_" + k: x for k, x in rec.items()}, **g)

    def leaf(x):
        return x.clone().requires_grad_(True)

    def torch_tick(with_q):
        reads = set(bt.default_grad_wants())
        args = [leaf(t["task_params"])] + [leaf(td[n]) if ("d_" + n) in reads and n in td else None for n in wbc_torch._TICK_ARGS[1:]]
        rest = {k: x for k, x in td.items() if k not in wbc_torch._TICK_ARGS and k != "q"}
        if with_q:
            q = leaf(td["q"])
            qdot, st = wbc_torch.wbc_tick_state(q, *args, rest, DT, bt)
        else:
            qdot, st = wbc_torch.wbc_tick(*args, dict(rest, q=td["q"]), DT, bt)
        (qdot * t["rho_qdot"]).sum().backward()
        out = dict(qdot=qdot, status=st, **{"g_" + n: x.grad for n, x in zip(wbc_torch._TICK_ARGS, args) if x is not None})
        if with_q:
            out["g_q"] = q.grad
        return out

    def torch_step():
        q, qd, ft = leaf(td["q"]), leaf(state["c_dev"]), leaf(td["ee_target"])
        q_new = wbc_torch.wbc_step(q, qd, ft, t["imu"], DT, bt, RUNNING, td.get("model_id"))
        (q_new * t["rho_q"]).sum().backward()
        return dict(q_new=q_new, g_q=q.grad, g_qdot=qd.grad, g_foot_targets=ft.grad)

    def torch_fused():
        q0, ee, tpl, es = leaf(td["q"]), leaf(td["ee_target"]), leaf(t["task_params"]), leaf(t["ee_step"])
        rest = {k: x for k, x in td.items() if k not in ("q", "ee_target")}
        q, qdot, st, trace = wbc_torch.wbc_rollout_fused(q0, tpl, ee, None, None, None, None, None, None, rest, DT, K, bt, ee_target_step=es, imu=t["imu"])
        ((q * t["rho_q"]).sum() + (qdot * t["rho_qdot"]).sum() + (trace * t["rho_trace"]).sum()).backward()
        return dict(q=q, qdot=qdot, status=st, q_trace=trace, g_q0=q0.grad, g_ee_target=ee.grad, g_task_params=tpl.grad, g_ee_step=es.grad)

    subset = ("d_task_params", "d_ee_target")
    calls = {
        "rollout_q0_only": lambda: rollout(0, want=("d_q0",), **seeds),      # first: no tick kernel in the sweep, last_grad_variant stays -1
        "certificate": certificate,
        "tick_vjp": vjp,
        "tick_vjp_subset": lambda: vjp(want=subset),
        "tick_vjp_q_con": lambda: vjp(inputs=dict(d, q_con=d["q"]), want=subset),      # (the tick layer clears q_con: the bits of the call before)
        "tick_vjp_state": vjp_state,
        "tick_grad": lambda: bt.tick_grad(d, DT, v, task_params=tp),
        "tick_grad_q": lambda: bt.tick_grad_q(d, DT, v, task_params=tp),
        "step_vjp_running": lambda: step(RUNNING, a["imu"]),
        "step_vjp_warmup": lambda: step(WARMUP, None),
        "rollout_cold": lambda: rollout(0, **seeds),
        "rollout_warm": lambda: rollout(1, **seeds),
        "rollout_final": lambda: rollout(0, g_q_final=seeds["g_q_final"]),
        "rollout_qdot": lambda: rollout(0, g_qdot_last=seeds["g_qdot_last"]),
        "rollout_trace": lambda: rollout(0, g_q_trace=seeds["g_q_trace"]),
        "rollout_warmup": lambda: rollout(0, mode=WARMUP, steps=False, **seeds),
        "torch_tick": lambda: torch_tick(False),
        "torch_tick_state": lambda: torch_tick(True),
        "torch_step": torch_step,
        "torch_fused": torch_fused,
    }
    assert tuple(calls) == CALLS
    for call, fn in calls.items():
        got = fn()
        if call == "certificate":
            qd = got["qdot"]
            state["c_dev"] = qd if hasattr(qd, "cpu") else torch.from_numpy(qd).cuda()
        stats = np.array([bt.stat(s) for s in STATS], np.int64)
        yield call, {k: _np(x) for k, x in got.items() if x is not None}, stats, p


# ---------------------------------------------------------------------------------------------- refusals
def refusal_handles():
    """-> dict of the handles the refused calls go to (the caller closes them)"""
    m = tgp._model("a1_wx200")
    deep = tsg._deep_wx200()
    one = lambda cfg: tgp._handle([m], [cfg], MAX_BATCH, {})      # noqa: E731
    return dict(rows=handle("rows"), norows=handle("norows"), c3=one(common.config("c3", m)), hybrid=one(common.config("c3_hybrid", m)),
                trunk=one(wbc_model.make_config(m, Trunk=True, Joint=True)), deep=tgp._handle([deep], [common.config("c3", deep)], MAX_BATCH, {}))


def run_refusals(hs, z):
    """Yields (name, code or None, message, ok) of every refused call: code None is a refusal of the Python wrapper; ok: the caller-owned outputs
    the call was given still hold SENTINEL and the tape, where there is one, its bytes. No call launches a kernel."""
    import torch
    d = {k[len("rows__d_"):]: np.ascontiguousarray(v) for k, v in z.items() if k.startswith("rows__d_")}
    d["q"] = np.where(np.isnan(d["q"]), 0.0, d["q"])
    one = {k: v for k, v in d.items() if k != "model_id"}
    g = np.ones((B, 26))
    rows_p = hs["rows"].constraint_rows
    pr = np.ones((B, rows_p))
    tapes = {}

    def tape_of(key, warm=0):
        """a tape that no call wrote: the refusals come before any launch (its bytes are compared afterwards)"""
        if key not in tapes:
            bt = hs[key]
            tp = RolloutTape(torch.full((B * (capi.TAPE_HEAD_BYTES + K * capi.TAPE_TICK_BYTES),), 5, dtype=torch.uint8, device="cuda"), B, K)
            tp.call = dict(inputs=dict(d if key in ("rows", "norows") else one), dt=DT, imu=None, mode=RUNNING, task_params=None, warm_start=warm)
            tapes[key] = tp
        return tapes[key]

    def fresh(fields, *names):
        o = {n: np.full((B,) + fields[n], SENTINEL) for n in names}
        o["grad_status"] = np.full(B, int(SENTINEL), np.int32)
        return o

    def tv(key, out=None, inputs=None, qdot=g, sens_x=g, dt=DT, **kw):
        return lambda: hs[key].tick_vjp(d if inputs is None else inputs, dt, qdot, sens_x, out=out, **kw)

    def ts(key, out=None, inputs=None, qdot=g, sens_x=g, dt=DT, **kw):
        for k in ("sens_rows", "y_rows"):                        # (as many rows as the handle's configuration has)
            if k in kw:
                kw[k] = np.ones((B, hs[key].constraint_rows))
        return lambda: hs[key].tick_vjp_state(d if inputs is None else inputs, dt, qdot, sens_x, out=out, **kw)

    def sv(key, out=None, q=d["q"], qdot=g, ft=d["ee_target"], gg=g, dt=DT, mid=d["model_id"], mode=RUNNING, **kw):
        return lambda: hs[key].step_vjp(q, qdot, ft, gg, dt, model_id=mid, mode=mode, out=out, **kw)

    def rv(key, out=None, call=None, buf=None, **kw):
        def fn():
            tp = tape_of(key)
            if call is not None or buf is not None:
                tp = RolloutTape(tp.buf if buf is None else buf(tp.buf), B, K)
                tp.call = dict(tapes[key].call, **(call or {}))
            return hs[key].rollout_vjp(tp, out=out, **kw)
        return fn

    def record_raw(key, hold=0, ptr=True, short=0, inputs=None):
        def fn():
            bt, tp = hs[key], tape_of(key)
            r = capi.WbcRollout()
            r.ticks, r.mode, r.hold_ticks = K, RUNNING, hold
            keep = []
            tin = bt._tick_in(d if inputs is None else inputs, keep, B)
            capi.check(bt.lib.wbc_rollout_record(bt._h, B, C.byref(tin), None, DT, C.byref(r), tp.buf.data_ptr() if ptr else None,
                                                 tp.buf.numel() - short, None, capi.MEM_HOST, None), bt.lib)
        return fn

    TG, SG, PG, RG = capi.TICK_GRAD_FIELDS, capi.TICK_STATE_GRAD_FIELDS, capi.STEP_GRAD_FIELDS, capi.ROLLOUT_GRAD_FIELDS
    sens = dict(sens_bounds=g, sens_rows=pr, y_rows=pr)
    x = np.ones((B, 26))
    H = np.tile(np.eye(26), (B, 1, 1))
    cases = []                                                   # (name, the call, its caller-owned outputs or None, the tape's handle or None)
    add = lambda name, fn, out=None, tape=None: cases.append((name, fn, out, tape))      # noqa: E731
    # wbc_qp_certificate
    bt = hs["rows"]
    add("cert/both_pairs", lambda: bt.qp_certificate(x, H=H, g=x, A=H, b=x))
    add("cert/no_pair", lambda: bt.qp_certificate(x))
    add("cert/H_alone", lambda: bt.qp_certificate(x, H=H))
    add("cert/A_alone", lambda: bt.qp_certificate(x, A=H))
    add("cert/lb_alone", lambda: bt.qp_certificate(x, H=H, g=x, lb=x))
    add("cert/C_without_sides", lambda: bt.qp_certificate(x, H=H, g=x, C_=H[:, :2]))
    # wbc_tick_vjp
    add("tick_vjp/qdot", tv("rows", qdot=None, sens_x=g, out=fresh(TG, "d_task_params")))
    add("tick_vjp/sens_x", tv("rows", sens_x=None))
    for bad_dt in (0.0, -0.002, float("inf"), float("nan")):
        add("tick_vjp/dt=%r" % bad_dt, tv("rows", dt=bad_dt))
    add("tick_vjp/model_id", tv("rows", inputs=one))
    add("tick_vjp/ee_target", tv("rows", inputs={k: v for k, v in d.items() if k != "ee_target"}))
    for n in ("d_trunk_target", "d_prev_trunk_target", "d_com_target", "d_com_target_vel", "d_posture_u"):
        o = fresh(TG, "d_task_params", n)
        add("tick_vjp/%s_requested" % n, tv("c3", inputs=one, out=o), o)
    for n in ("d_ee_target", "d_prev_ee_target"):
        o = fresh(TG, "d_task_params", n)
        add("tick_vjp/%s_requested" % n, tv("trunk", inputs=one, out=o), o)
    o = fresh(TG, "d_task_params", "d_posture_u")
    add("tick_vjp/d_posture_u_of_model", tv("norows", out=o), o)
    add("tick_vjp/two_wrong", tv("c3", inputs=one, dt=0.0, out=fresh(TG, "d_com_target", "d_posture_u")))
    add("tick_vjp/two_requested", tv("c3", inputs=one, out=fresh(TG, "d_com_target", "d_posture_u")))
    add("tick_vjp/schedule", tv("deep", inputs=one))
    add("tick_vjp/unknown_want", tv("rows", want=("d_q",)))
    add("tick_vjp/unknown_out", tv("rows", out=dict(d_q=g)))
    # wbc_tick_vjp_state
    add("tick_vjp_state/qdot", ts("rows", qdot=None, **sens))
    add("tick_vjp_state/sens_x", ts("rows", sens_x=None, **sens))
    add("tick_vjp_state/dt", ts("rows", dt=0.0, **sens))
    add("tick_vjp_state/q_con", ts("rows", inputs=dict(d, q_con=d["q"]), **sens))
    add("tick_vjp_state/posture_u", ts("hybrid", inputs=one, **sens))
    add("tick_vjp_state/sens_bounds", ts("rows", sens_rows=pr, y_rows=pr))
    add("tick_vjp_state/sens_rows", ts("rows", sens_bounds=g, y_rows=pr))
    add("tick_vjp_state/y_rows", ts("rows", sens_bounds=g, sens_rows=pr))
    o = fresh(SG, "d_q", "d_trunk_box_center")
    add("tick_vjp_state/d_trunk_box_center_requested", ts("norows", sens_bounds=g, out=o), o)
    add("tick_vjp_state/model_id", ts("rows", inputs=one, **sens))
    add("tick_vjp_state/schedule", ts("deep", inputs=one, **sens))
    add("tick_vjp_state/unknown_want", ts("rows", want=("d_task_params",), **sens))
    add("tick_vjp_state/unknown_out", ts("rows", out=dict(d_task_params=g), **sens))
    # wbc_step_vjp
    add("step_vjp/qdot", sv("rows", qdot=None))
    add("step_vjp/foot_targets", sv("rows", ft=None))
    add("step_vjp/g", sv("rows", gg=None))
    o = fresh(PG, "d_q")
    add("step_vjp/mode", sv("rows", mode=2, out=o), o)
    add("step_vjp/dt", sv("rows", dt=-0.002))
    add("step_vjp/model_id", sv("rows", mid=None))
    add("step_vjp/schedule", sv("deep", mid=None))
    add("step_vjp/unknown_want", sv("rows", want=("d_imu",)))
    add("step_vjp/unknown_out", sv("rows", out=dict(d_imu=g)))
    # wbc_rollout_record
    add("record/hold_ticks", record_raw("rows", hold=2), None, "rows")
    add("record/tape", record_raw("rows", ptr=False), None, "rows")
    add("record/tape_bytes", record_raw("rows", short=1), None, "rows")
    add("record/q_con", lambda: hs["rows"].rollout_record(dict(d, q_con=d["q"]), DT, K))
    add("record/ticks", lambda: hs["rows"].rollout_record(d, DT, 0))
    add("record/model_id", lambda: hs["rows"].rollout_record(one, DT, K))
    add("record/posture_u", lambda: hs["hybrid"].rollout_record(one, DT, K))
    add("record/schedule", lambda: hs["deep"].rollout_record(one, DT, K))
    # wbc_rollout_vjp
    o = fresh(RG, "d_q0")
    add("rollout_vjp/no_seed", rv("rows", out=o), o, "rows")
    for n in ("d_trunk_target", "d_prev_trunk_target", "d_trunk_target_step", "d_com_target", "d_com_target_vel", "d_posture_u"):
        o = fresh(RG, "d_q0", n)
        add("rollout_vjp/%s_requested" % n, rv("c3", out=o, g_q_final=g), o, "c3")
    for n in ("d_ee_target", "d_ee_target_step", "d_prev_ee_target"):
        o = fresh(RG, "d_q0", n)
        add("rollout_vjp/%s_requested_warmup" % n, rv("trunk", out=o, call=dict(mode=WARMUP), g_q_final=g), o, "trunk")
    o = fresh(RG, "d_q0", "d_prev_ee_target")
    add("rollout_vjp/d_prev_ee_target_requested_running", rv("trunk", out=o, g_q_final=g), o, "trunk")
    o = fresh(RG, "d_q0", "d_trunk_box_center")
    add("rollout_vjp/d_trunk_box_center_requested", rv("norows", out=o, g_q_final=g), o, "norows")
    add("rollout_vjp/tape_bytes", rv("rows", buf=lambda b: b[:-8], g_q_final=g), None, "rows")
    add("rollout_vjp/q_con", rv("rows", call=dict(inputs=dict(d, q_con=d["q"])), g_q_final=g), None, "rows")
    for bad_dt in (0.0, float("nan")):
        add("rollout_vjp/dt=%r" % bad_dt, rv("rows", call=dict(dt=bad_dt), g_q_final=g), None, "rows")
    add("rollout_vjp/mode", rv("rows", call=dict(mode=2), g_q_final=g), None, "rows")
    add("rollout_vjp/ee_target", rv("trunk", call=dict(inputs={k: v for k, v in one.items() if k not in ("ee_target", "prev_ee_target")}), g_q_final=g),
        None, "trunk")
    add("rollout_vjp/model_id", rv("rows", call=dict(inputs=one), g_q_final=g), None, "rows")
    add("rollout_vjp/posture_u", rv("hybrid", g_q_final=g), None, "hybrid")
    add("rollout_vjp/schedule", rv("deep", g_q_final=g), None, "deep")
    add("rollout_vjp/two_wrong", rv("c3", out=fresh(RG, "d_com_target", "d_posture_u"), call=dict(dt=0.0)), None, "c3")
    add("rollout_vjp/two_requested", rv("c3", out=fresh(RG, "d_com_target", "d_posture_u"), g_q_final=g), None, "c3")
    add("rollout_vjp/warm_start_changed", rv("rows", call=dict(warm_start=1), g_q_final=g), None, "rows")
    add("rollout_vjp/g_q_trace_shape", rv("rows", g_q_trace=np.ones((K + 1, B, 26))), None, "rows")
    add("rollout_vjp/unknown_want", rv("rows", want=("d_q",), g_q_final=g), None, "rows")
    add("rollout_vjp/unknown_out", rv("rows", out=dict(d_q=g), g_q_final=g), None, "rows")
    for name, fn, out, tape in cases:
        try:
            fn()
        except capi.WbcError as e:
            code, msg = e.code, str(e)
        else:
            code, msg = 0, "not refused"
        ok = True
        if out is not None:
            ok = all((v == (int(SENTINEL) if v.dtype == np.int32 else SENTINEL)).all() for v in out.values())
        if tape is not None:
            hs[tape].synchronize()
            ok = ok and bool((tapes[tape].buf == 5).all())
        yield name, code, msg, ok
