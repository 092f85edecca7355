"""Differentiable batched QP for torch: ``x, status = qp_solve(H, g, C, lb, ub, Clb, Cub, batch)``.

Forward is ``wbc_qp_solve`` with the working set out; backward is ONE ``wbc_qp_certificate`` call with v = grad_output (include/wbc.h:
K (u; w) = (v; 0) on the factors of the certificate) plus torch outer products:

    dL/dg = -u      dL/dH = -1/2 (u x' + x u')      dL/dC_j = -w_j x' + y_j u'      dL/de_i = w_i

where e_i is the bound value active constraint i sits at: the gradient goes to lb / Clb at a lower side, to ub / Cub at an upper side and
is split half and half on an equality (lb == ub, Clb == Cub). Instances whose QP was not solved, or whose certificate does not come back
WBC_CERT_OK (dependent active normals, non-finite data), get zero gradients. All tensors are contiguous float64 on the handle's device;
C, Clb, Cub (no rows) and lb, ub (no box) may be None. There is no CPU fallback.

``qdot, status = wbc_tick(task_params, ee_target, ..., inputs, dt, batch)`` is the same one level up: the whole control tick as a layer over
what its caller owns — the 85 per-instance weights and gains and the task targets. Forward is ``wbc_tick_tp`` with the working set out;
backward is one certificate of the tick's own problem with v = grad_output followed by ``wbc_tick_vjp`` (include/wbc.h), all on the device.

``qdot, status = wbc_tick_state(q, task_params, ee_target, ..., inputs, dt, batch)`` adds the state: the same forward with q a tensor argument;
backward is one certificate, ``wbc_tick_vjp`` when a gradient other than q's is wanted, and ``wbc_tick_vjp_state``, whose tangent-coordinate
d_q goes to raw coordinates through ``wbc_workload.tangent_to_raw``.

``q_new = wbc_step(q, qdot, foot_targets, imu, dt, batch, mode)`` is the state step between two ticks (integrate, then the estimator) with
``wbc_step_vjp`` behind it, and ``wbc_rollout(q0, task_params, ee_target, ..., inputs, dt, ticks, batch)`` chains K ticks out of the two layers.
``wbc_rollout_fused`` takes the same arguments and is one layer: forward ``wbc_rollout_record``, backward ``wbc_rollout_vjp``.

``slack, components, which = wbc_state_slack(q, trunk_box_center, batch)`` is the constraint slack at a state with ``wbc_state_slack_vjp``
behind it, and ``wbc_rollout_watched`` a recorded roll-out whose watched slacks (minimum, final, per-tick trace) are differentiable outputs.
"""
import torch

import wbc_capi as capi


def _c(t):
    return None if t is None else t.detach().contiguous()


class _QpSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, g, C, lb, ub, Clb, Cub, batch):
        args = [_c(t) for t in (H, g, C, lb, ub, Clb, Cub)]
        x, st, _, ws = batch.qp_solve(*args, want_working_set=True)
        ctx.batch = batch
        ctx.present = [a is not None for a in args]
        # through save_for_backward: an in-place change of an input between forward and backward is an autograd error, not a certificate of other data
        ctx.save_for_backward(x, st, ws, *[a for a in args if a is not None])
        ctx.mark_non_differentiable(st)
        return x, st

    @staticmethod
    def backward(ctx, gx, _gst):
        x, st, ws, *given = ctx.saved_tensors
        it = iter(given)
        H, g, C, lb, ub, Clb, Cub = [next(it) if have else None for have in ctx.present]
        if gx is None:              # x took no part in the loss
            return (None,) * 8
        B, n = x.shape
        c = ctx.batch.qp_certificate(x, H=H, g=g, C_=C, lb=lb, ub=ub, Clb=Clb, Cub=Cub, status=st, working_set=ws, v=gx.contiguous())
        ok = (c["cert_status"] == capi.CERT_OK).to(x.dtype)[:, None]
        u, wb = c["sens_x"] * ok, c["sens_bounds"] * ok
        need = ctx.needs_input_grad

        def sides(w, lo, hi, word):
            """dL/de -> (its lower bound's, its upper bound's) share"""
            k = w.shape[1]
            low = ((word[:, None] >> torch.arange(k, device=w.device)) & 1).bool()
            eq = lo == hi
            zero = torch.zeros_like(w)
            return torch.where(eq, 0.5 * w, torch.where(low, w, zero)), torch.where(eq, 0.5 * w, torch.where(low, zero, w))
        gH = -0.5 * (u[:, :, None] * x[:, None, :] + x[:, :, None] * u[:, None, :]) if need[0] else None
        gg = -u if need[1] else None
        gC = glb = gub = gcl = gcu = None
        if lb is not None and (need[3] or need[4]):
            glb, gub = sides(wb, lb, ub, ws[:, 0])
        if C is not None:
            wr, yr = c["sens_rows"] * ok, c["y_rows"] * ok
            if need[2]:
                gC = -wr[:, :, None] * x[:, None, :] + yr[:, :, None] * u[:, None, :]
            if need[5] or need[6]:
                gcl, gcu = sides(wr, Clb, Cub, ws[:, 1])
        return (gH, gg, gC, glb if need[3] else None, gub if need[4] else None, gcl if need[5] else None, gcu if need[6] else None, None)


def qp_solve(H, g, C, lb, ub, Clb, Cub, batch):
    """argmin 1/2 x'Hx + g'x s.t. lb <= x <= ub, Clb <= C x <= Cub for a batch (H [B,n,n], C [B,p,n]) on `batch` (a WbcBatch), differentiable
    with respect to every tensor argument. Returns (x [B,n], status [B] int32)."""
    return _QpSolve.apply(H, g, C, lb, ub, Clb, Cub, batch)


_TICK_ARGS = ("task_params", "ee_target", "prev_ee_target", "trunk_target", "prev_trunk_target", "com_target", "com_target_vel", "posture_u")
_STATE_ARGS = ("q",) + _TICK_ARGS
_FUSED_ARGS = ("q0",) + _TICK_ARGS + ("ee_target_step", "trunk_target_step")
_IN_NAME = dict({n: n for n in _TICK_ARGS[1:]}, q="q", q0="q")      # tensor argument -> the WbcTickIn field it stands for (the others are none)


# ---- the bookkeeping the layers over a tick share: tensor arguments that may be None, merged into `inputs`, saved, and asked for by name
def _merged(inputs, names, args):
    """-> dict(inputs) with every tensor argument that is given in under its WbcTickIn name"""
    d = dict(inputs)
    d.update({_IN_NAME[n]: a for n, a in zip(names, args) if a is not None and n in _IN_NAME})
    return d


def _save(ctx, head, args):
    """through save_for_backward: an in-place change of an argument between forward and backward is an autograd error, not a gradient of other data"""
    ctx.present = [a is not None for a in args]
    ctx.save_for_backward(*head, *[a for a in args if a is not None])


def _saved(ctx, n_head):
    """-> (the head tensors, the arguments with None where none was given)"""
    t = ctx.saved_tensors
    it = iter(t[n_head:])
    return t[:n_head], [next(it) if have else None for have in ctx.present]


def _wanted(names, args, need, offered=None):
    """the gradient names ("d_" + argument) that are needed, of arguments that were given (and that the configuration offers)"""
    return tuple("d_" + n for k, n in enumerate(names) if need[k] and args[k] is not None and (offered is None or "d_" + n in offered))


def _state_seeds(g_q, g_qdot, g_trace, q_final, q_trace):
    """the state seeds of WbcBatch.rollout_vjp from the raw gradients of a recorded roll-out's outputs (each may be None): q_K's and the
    trace's from raw to tangent coordinates in ONE wbc_workload.raw_to_tangent call -> dict(g_q_final, g_qdot_last, g_q_trace)"""
    import wbc_workload
    K, B = q_trace.shape[0], q_trace.shape[1]
    raw, at = [], []
    if g_q is not None:
        raw.append(g_q.reshape(B, -1))
        at.append(q_final)
    if g_trace is not None:
        raw.append(g_trace.reshape(K * B, -1))
        at.append(q_trace.reshape(K * B, -1))
    gq_f = gq_t = None
    if raw:
        tang = wbc_workload.raw_to_tangent(torch.cat(at), torch.cat(raw).contiguous())
        if g_q is not None:
            gq_f = tang[:B].contiguous()
        if g_trace is not None:
            gq_t = tang[-K * B:].reshape(K, B, -1).contiguous()
    return dict(g_q_final=gq_f, g_qdot_last=None if g_qdot is None else g_qdot.contiguous(), g_q_trace=gq_t)


class _WbcTick(torch.autograd.Function):
    """wbc_tick (q None: the state is inputs["q"] and gets no gradient) and wbc_tick_state"""
    @staticmethod
    def forward(ctx, q, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u, inputs, dt,
                batch):
        args = [_c(t) for t in (q, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u)]
        d = _merged(inputs, _STATE_ARGS, args)
        t = batch.tick(d, dt, want_working_set=True, task_params=args[1])
        ctx.batch, ctx.dt = batch, dt
        given = {_IN_NAME[n] for n, a in zip(_STATE_ARGS, args) if a is not None and n in _IN_NAME}
        ctx.rest = {k: v for k, v in d.items() if k not in given}          # (what came in `inputs`: not ours to version-check)
        _save(ctx, (t["qdot"], t["status"], t["working_set"]), args)
        ctx.mark_non_differentiable(t["status"])
        return t["qdot"], t["status"]

    @staticmethod
    def backward(ctx, gq, _gst):
        import wbc_workload
        (qdot, st, ws), args = _saved(ctx, 3)
        n_out = len(_STATE_ARGS) + 3
        want = _wanted(_STATE_ARGS, args, ctx.needs_input_grad)
        need_q, want = "d_q" in want, tuple(n for n in want if n != "d_q")
        if gq is None or not (want or need_q):              # qdot took no part in the loss, or nothing is asked for
            return (None,) * n_out
        bt, tp = ctx.batch, args[1]
        d = _merged(ctx.rest, _STATE_ARGS, args)
        c = bt.tick_certificate(d, ctx.dt, task_params=tp, v=gq.contiguous(), tick=dict(qdot=qdot, status=st, working_set=ws))
        # one launch per layer that is asked for: no wbc_tick_vjp without one of its gradients, no wbc_tick_vjp_state without q's
        g = bt.tick_vjp(d, ctx.dt, qdot, c["sens_x"], status=st, cert_status=c["cert_status"], task_params=tp, want=want) if want else {}
        if need_q:
            s = bt.tick_vjp_state(d, ctx.dt, qdot, c["sens_x"], sens_bounds=c["sens_bounds"], sens_rows=c["sens_rows"], y_rows=c["y_rows"], status=st,
                                  cert_status=c["cert_status"], working_set=ws, task_params=tp, want=("d_q",))
            g["d_q"] = wbc_workload.tangent_to_raw(args[0], s["d_q"])
        return tuple(g.get("d_" + n) for n in _STATE_ARGS) + (None, None, None)


def wbc_tick(task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u, inputs, dt, batch):
    """One control tick per instance as a differentiable layer on `batch` (a configured WbcBatch): returns (qdot [B,26], status [B] int32).
    The eight tensor arguments (contiguous float64 on the handle's device; task_params [B,85], the rest shaped as in WbcTickIn) are what
    gradients flow to; any of them may be None — task_params None is the configuration's block, a target None is taken from `inputs` (a dict
    keyed like WbcTickIn that holds everything else: q, trunk_box_center, the orientation references, model_id ...) and gets no gradient. An
    argument the configuration does not read (trunk_target without the trunk task ...) must be None or not require a gradient. Instances
    whose QP was not solved or whose certificate is not WBC_CERT_OK get zero gradients. No gradient flows to q or anything else in `inputs`."""
    return _WbcTick.apply(None, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u, inputs,
                          dt, batch)


def wbc_tick_state(q, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u, inputs, dt,
                   batch):
    """wbc_tick with the state as a differentiable argument: q [B,27] (contiguous float64 on the handle's device) replaces inputs["q"], and its
    gradient is that of the tick composed with the normalisation of q's quaternion, in raw coordinates (wbc_workload.tangent_to_raw of
    wbc_tick_vjp_state's d_q). The other eight arguments and their gradients are wbc_tick's. posture_u (MANI / HYBRID / CUSTOM: it must be
    given) and the orientation references are held constant; inputs must not hold q_con. No gradient flows to anything else in `inputs`."""
    return _WbcTick.apply(q, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u,
                          inputs, dt, batch)


class _WbcStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, qdot, foot_targets, imu, dt, batch, mode, model_id):
        q, qdot, ft, imu = _c(q), _c(qdot), _c(foot_targets), _c(imu)
        q_new = batch.integrate(q, qdot, dt, model_id=model_id)
        if mode == capi.ROLLOUT_RUNNING:
            q_new = batch.update_state(q, q_new, ft, imu=imu, model_id=model_id)
        ctx.batch, ctx.dt, ctx.mode, ctx.model_id, ctx.have_imu = batch, dt, mode, model_id, imu is not None
        ctx.save_for_backward(q, qdot, ft, q_new, *([imu] if imu is not None else []))
        return q_new

    @staticmethod
    def backward(ctx, g_raw):
        import wbc_workload
        q, qdot, ft, q_new, *rest = ctx.saved_tensors
        if g_raw is None:
            return (None,) * 8
        g = wbc_workload.raw_to_tangent(q_new, g_raw.contiguous())
        s = ctx.batch.step_vjp(q, qdot, ft, g, ctx.dt, imu=rest[0] if ctx.have_imu else None, model_id=ctx.model_id, mode=ctx.mode)
        need = ctx.needs_input_grad
        return (wbc_workload.tangent_to_raw(q, s["d_q"]) if need[0] else None, s["d_qdot"] if need[1] else None,
                s["d_foot_targets"].reshape(ft.shape) if need[2] else None, None, None, None, None, None)


def wbc_step(q, qdot, foot_targets, imu, dt, batch, mode=capi.ROLLOUT_RUNNING, model_id=None):
    """The state step between two ticks as a differentiable layer on `batch`: q_new [B,27] = update_state(q, integrate(q, qdot, dt), foot_targets,
    imu) (mode ROLLOUT_WARMUP: integrate alone). Gradients flow to q (raw coordinates: the step composed with the normalisation of q's
    quaternion), qdot and foot_targets [B,5,3]; backward is wbc_workload.raw_to_tangent at q_new, ONE wbc_step_vjp (include/wbc.h) and
    wbc_workload.tangent_to_raw at q. imu ([B,4] or None) is held constant. Contiguous float64 tensors on the handle's device."""
    return _WbcStep.apply(q, qdot, foot_targets, imu, dt, batch, mode, model_id)


def _euler_xyz_to_R(e):
    """[B, 9] row-major Rz(c) Ry(b) Rx(a) (wbc_workload._euler_xyz_to_R)"""
    sa, ca, sb, cb, sc, cc = torch.sin(e[:, 0]), torch.cos(e[:, 0]), torch.sin(e[:, 1]), torch.cos(e[:, 1]), torch.sin(e[:, 2]), torch.cos(e[:, 2])
    return torch.stack([cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa,
                        -sb, cb * sa, cb * ca], dim=1)


def wbc_rollout(q0, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u, inputs, dt,
                ticks, batch, ee_target_step=None, trunk_target_step=None, mode=capi.ROLLOUT_RUNNING, imu=None):
    """`ticks` closed-loop ticks as chained differentiable layers, written in torch operations: per tick wbc_tick_state -> wbc_step, then the
    reference-state side effects of the update kernel (prev_ee_target <- ee_target and ee_prev_rot <- ee_ref_rot for the end effectors whose
    task is on; prev_trunk_target <- trunk_target and trunk_prev_rot <- R(trunk_ref_euler) with the trunk task on), then the targets advance
    by their steps as a running sum, as the kernel does. The arguments are wbc_tick_state's (q0 for q; a target None is taken from `inputs` and
    gets no gradient) plus the steps ([B,5,3] / [B,3] or None), the mode and the IMU quaternion ([B,4] or None, held constant). Gradients flow
    to q0 and to whichever of the eight tensor arguments the configuration reads; ee_target also receives the estimator's d_foot_targets.
    Returns (q_final [B,27], qdot of the last tick [B,26], status [B] int32 the worst over the ticks, states: per tick dict(q, qdot, status)).
    An instance with an unsolved or uncertified tick gets zero gradient from that tick's layer on (wbc_tick_state's rule): what reaches q0
    and the arguments from such an instance is what flows around that tick, through the step alone. This is the forward of WbcBatch.rollout
    (no hold ticks) as separate launches; wbc_rollout_fused below is the same layer over the recorded roll-out and the device's reverse sweep.
    On the sim3 switch set (c3) the cotangent that arrives from the next tick's state is no task-space direction (grad_common.task_space_v in
    the tests says why): sens_x reaches 1e6, the chain's gradient is right to about 7 digits and cannot be held to tighter bounds."""
    cfg = batch.cfgs[0]
    on = [bool(cfg.task_ee[e]) for e in range(capi.NEE)]
    d = dict(inputs)
    pick = lambda t, name: d.get(name) if t is None else t      # noqa: E731
    ee, pee = pick(ee_target, "ee_target"), pick(prev_ee_target, "prev_ee_target")
    tt, ptt = pick(trunk_target, "trunk_target"), pick(prev_trunk_target, "prev_trunk_target")
    for name in ("ee_target", "prev_ee_target", "trunk_target", "prev_trunk_target"):
        d.pop(name, None)
    read = lambda t, yes: t if (yes or t is None) else t.detach()      # noqa: E731  (an argument the configuration does not read gets no gradient)
    on_t = torch.tensor(on, device=q0.device)[None, :, None]
    mid = d.get("model_id")
    q, status, states, qdot = q0, None, [], None
    for _ in range(int(ticks)):
        qdot, st = wbc_tick_state(q, task_params, read(ee, any(on)), read(pee, any(on)), read(tt, cfg.task_trunk), read(ptt, cfg.task_trunk),
                                  com_target, com_target_vel, posture_u, d, dt, batch)
        states.append(dict(q=q, qdot=qdot, status=st))
        status = st if status is None else torch.maximum(status, st)
        q = wbc_step(q, qdot, ee, imu, dt, batch, mode, mid)
        if any(on):
            pee = torch.where(on_t, ee.reshape(-1, capi.NEE, 3), pee.reshape(-1, capi.NEE, 3)).reshape(pee.shape) if pee is not None else None
            if d.get("ee_ref_rot") is not None and d.get("ee_prev_rot") is not None:
                d["ee_prev_rot"] = torch.where(on_t, d["ee_ref_rot"].reshape(-1, capi.NEE, 9), d["ee_prev_rot"].reshape(-1, capi.NEE, 9)).reshape(
                    d["ee_prev_rot"].shape).contiguous()
        if cfg.task_trunk:
            ptt = tt if ptt is not None else None
            if d.get("trunk_ref_euler") is not None and d.get("trunk_prev_rot") is not None:
                d["trunk_prev_rot"] = _euler_xyz_to_R(d["trunk_ref_euler"].reshape(-1, 3)).reshape(d["trunk_prev_rot"].shape).contiguous()
        if ee_target_step is not None:
            ee = ee + ee_target_step.reshape(ee.shape)
        if trunk_target_step is not None and tt is not None:
            tt = tt + trunk_target_step.reshape(tt.shape)
    return q, qdot, status, states


class _WbcRolloutFused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q0, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u,
                ee_target_step, trunk_target_step, inputs, dt, ticks, batch, mode, imu):
        args = [_c(t) for t in (q0, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u,
                                ee_target_step, trunk_target_step)]
        d = _merged(inputs, _FUSED_ARGS, args)
        es = None if args[9] is None else args[9].reshape(-1, capi.NEE, 3)
        out, tape = batch.rollout_record(d, dt, ticks, ee_target_step=es, trunk_target_step=args[10], imu=_c(imu), mode=mode, task_params=args[1])
        ctx.batch, ctx.tape = batch, tape
        _save(ctx, (out["q"], out["q_trace"]), args)
        ctx.mark_non_differentiable(out["status"])
        return out["q"], out["qdot"], out["status"], out["q_trace"]

    @staticmethod
    def backward(ctx, g_q, g_qdot, _gst, g_trace):
        import wbc_workload
        (q_final, q_trace), args = _saved(ctx, 2)
        n_out = len(_FUSED_ARGS) + 6
        bt, tape = ctx.batch, ctx.tape
        want = _wanted(_FUSED_ARGS, args, ctx.needs_input_grad, set(bt.default_rollout_grad_wants(tape.call["mode"])))
        if (g_q is None and g_qdot is None and g_trace is None) or not want:
            return (None,) * n_out
        r = bt.rollout_vjp(tape, want=want, **_state_seeds(g_q, g_qdot, g_trace, q_final, q_trace))
        res = [None if "d_" + n not in want else r["d_" + n].reshape(a.shape) if n != "q0" else wbc_workload.tangent_to_raw(a, r["d_q0"])
               for n, a in zip(_FUSED_ARGS, args)]
        return tuple(res) + (None,) * 6


def wbc_rollout_fused(q0, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel, posture_u, inputs, dt,
                      ticks, batch, ee_target_step=None, trunk_target_step=None, mode=capi.ROLLOUT_RUNNING, imu=None):
    """wbc_rollout as ONE layer: the arguments of wbc_rollout; the forward is one WbcBatch.rollout_record (the forward users run, with a tape),
    the backward converts the seeds with wbc_workload.raw_to_tangent once, makes one WbcBatch.rollout_vjp call (include/wbc.h: the reverse
    sweep on the device) and runs wbc_workload.tangent_to_raw on d_q0 once. Gradients flow to q0, to whichever of the eight tensor arguments
    the configuration reads, and to ee_target_step / trunk_target_step. Returns (q_final [B,27], qdot of the last tick [B,26], status [B]
    int32 the worst over the ticks, q_trace [ticks,B,27]: the state after every tick); a loss may use q_final, qdot and q_trace.
    Unsolved ticks: wbc_rollout's rule. inputs must not hold q_con; posture modes MANI / HYBRID need posture_u."""
    return _WbcRolloutFused.apply(q0, task_params, ee_target, prev_ee_target, trunk_target, prev_trunk_target, com_target, com_target_vel,
                                  posture_u, ee_target_step, trunk_target_step, inputs, dt, ticks, batch, mode, imu)


# ---- the two layers over a recorded roll-out along tracks: their arguments are (q0, task_params, eight that get no gradient, *flat)
_TRACK_GRADS = ("d_points", "d_tangents", "d_du")


def _flat_tracks(tracks):
    """rollout_tracks' list of dicts -> (specs, flat): flat holds (points, tangents, du) per track, None where there is none; what is no
    tensor (target, kind, n_points, a du given as a number) stays in the track's spec"""
    specs, flat = [], []
    for t in tracks:
        du = t.get("du", 0.002)
        specs.append({k: v for k, v in t.items() if k not in ("points", "tangents", "du")})
        if not torch.is_tensor(du):
            specs[-1]["du"] = du
        flat += [t["points"], t.get("tangents"), du if torch.is_tensor(du) else None]
    return specs, flat


def _tracks_of(specs, flat):
    """_flat_tracks undone"""
    tracks = []
    for j, spec in enumerate(specs):
        t = dict(spec, points=flat[3 * j])
        if flat[3 * j + 1] is not None:
            t["tangents"] = flat[3 * j + 1]
        if flat[3 * j + 2] is not None:
            t["du"] = flat[3 * j + 2]
        tracks.append(t)
    return tracks


def _tracks_record(ctx, q0, task_params, inputs, dt, ticks, batch, specs, flat, **kw):
    """the forward of both layers: one WbcBatch.rollout_record along the tracks -> (its dict, the arguments as saved)"""
    args = [_c(q0), _c(task_params)] + [_c(t) for t in flat]
    out, tape = batch.rollout_record(dict(inputs, q=args[0]), dt, ticks, task_params=args[1], tracks=_tracks_of(specs, args[2:]), **kw)
    ctx.batch, ctx.tape = batch, tape
    return out, args


def _tracks_sweep(ctx, args, g_q, g_qdot, g_trace, q_final, q_trace, **score):
    """the backward of both layers: one WbcBatch.rollout_vjp for what needs a gradient, seeded with the raw gradients of q_final, qdot and
    q_trace (each may be None) and, where the loss uses a score, score = dict(score_seed=...) -> the gradients of every forward argument"""
    import wbc_workload
    n_flat = len(args) - 2
    need = ctx.needs_input_grad
    want = [n for n, k in (("d_q0", 0), ("d_task_params", 1)) if need[k] and args[k] is not None]
    need_flat = [bool(need[10 + i]) and args[2 + i] is not None for i in range(n_flat)]
    want += [n for c, n in enumerate(_TRACK_GRADS) if any(need_flat[c::3])]
    if (not score and g_q is None and g_qdot is None and g_trace is None) or not want:
        return (None,) * (10 + n_flat)
    r = ctx.batch.rollout_vjp(ctx.tape, want=want, **_state_seeds(g_q, g_qdot, g_trace, q_final, q_trace), **score)
    res = [wbc_workload.tangent_to_raw(args[0], r["d_q0"]) if "d_q0" in want else None,
           r["d_task_params"].reshape(args[1].shape) if "d_task_params" in want else None] + [None] * 8
    for i in range(n_flat):
        got = r["tracks"][i // 3].get(_TRACK_GRADS[i % 3]) if need_flat[i] else None
        res.append(None if got is None else got.reshape(args[2 + i].shape))
    return tuple(res)


class _WbcRolloutTracksFused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q0, task_params, inputs, dt, ticks, batch, mode, imu, trunk_target_step, specs, *flat):
        out, args = _tracks_record(ctx, q0, task_params, inputs, dt, ticks, batch, specs, flat, trunk_target_step=_c(trunk_target_step),
                                   imu=_c(imu), mode=mode)
        _save(ctx, (out["q"], out["q_trace"]), args)
        ctx.mark_non_differentiable(out["status"])
        return out["q"], out["qdot"], out["status"], out["q_trace"]

    @staticmethod
    def backward(ctx, g_q, g_qdot, _gst, g_trace):
        (q_final, q_trace), args = _saved(ctx, 2)
        return _tracks_sweep(ctx, args, g_q, g_qdot, g_trace, q_final, q_trace)


def wbc_rollout_tracks_fused(q0, task_params, tracks, inputs, dt, ticks, batch, mode=capi.ROLLOUT_RUNNING, imu=None, trunk_target_step=None):
    """WbcBatch.rollout_tracks as ONE differentiable layer (trajectory optimisation through the controller): the forward is one
    WbcBatch.rollout_record(..., tracks=tracks) (wbc_rollout_record_tracks, include/wbc.h), the backward one WbcBatch.rollout_vjp
    (wbc_rollout_vjp_tracks: the reverse sweep and the adjoint of the track evaluation on the device). tracks: rollout_tracks' list of dicts;
    each track's points [B,S,3], tangents [B,S,3] (hermite with caller tangents) and du [B] may be tensors that require a gradient (a du
    given as a number is shared by the instances and gets none; n_points gets none). Gradients also flow to q0 (raw coordinates) and
    task_params; the constant targets come from `inputs` and get none here (wbc_rollout_fused is the layer for those). Returns what
    wbc_rollout_fused returns: (q_final [B,27], qdot of the last tick [B,26], status [B] int32, q_trace [ticks,B,27]). A bad row (include/wbc.h)
    gets zero gradients everywhere. Contiguous float64 tensors on the handle's device."""
    specs, flat = _flat_tracks(tracks)
    return _WbcRolloutTracksFused.apply(q0, task_params, inputs, dt, ticks, batch, mode, imu, trunk_target_step, specs, *flat)


class _WbcRolloutTracksScored(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q0, task_params, inputs, dt, ticks, batch, mode, trunk_target_step, score, specs, *flat):
        out, args = _tracks_record(ctx, q0, task_params, inputs, dt, ticks, batch, specs, flat, trunk_target_step=_c(trunk_target_step),
                                   mode=mode, score=score)
        ctx.score = tuple(score)
        ctx.set_materialize_grads(False)     # an output the loss does not use gives None, not zeros: its seed is left out of the call
        _save(ctx, (out["q"], out["q_trace"], out["err_max_tick"]), args)
        ctx.mark_non_differentiable(out["status"], out["err_max_tick"])
        return out["q"], out["qdot"], out["status"], out["q_trace"], out["err_sq_sum"], out["err_final"], out["err_max"], out["err_max_tick"]

    @staticmethod
    def backward(ctx, g_q, g_qdot, _gst, g_trace, g_sq, g_fin, g_max, _gtick):
        (q_final, q_trace, err_max_tick), args = _saved(ctx, 3)
        score = {}
        if not (g_sq is None and g_fin is None and g_max is None):
            cg = lambda t: None if t is None else t.contiguous()      # noqa: E731
            score["score_seed"] = dict(mask=ctx.score, g_err_sq_sum=cg(g_sq), g_err_final=cg(g_fin), g_err_max=cg(g_max),
                                       err_max_tick=None if g_max is None else err_max_tick, q_final=q_final)
        return _tracks_sweep(ctx, args, g_q, g_qdot, g_trace, q_final, q_trace, **score)


def wbc_rollout_tracks_scored(q0, task_params, tracks, inputs, dt, ticks, batch, score=(4,), mode=capi.ROLLOUT_RUNNING, trunk_target_step=None):
    """wbc_rollout_tracks_fused with the tracking scores as differentiable outputs (the loss the roll-out computes on the device): the forward
    is one WbcBatch.rollout_record(..., tracks=tracks, score=score), the backward one WbcBatch.rollout_vjp(..., score_seed=...)
    (wbc_rollout_vjp_scored, include/wbc.h: the scores' cotangents are formed where the sweep runs, nothing crosses to the host). score: the
    scored frames, end effector indices 0..4 and / or "trunk". Returns wbc_rollout_tracks_fused's (q_final, qdot, status, q_trace) and then
    err_sq_sum, err_final, err_max [n_scored,B] (rows in increasing frame order; differentiable) and err_max_tick [n_scored,B] int32 (not
    differentiable). A loss may mix the scores with q_final, qdot and q_trace: the gradients are those of the sum. The group RMS is
    torch.sqrt(err_sq_sum.reshape(n, G, M).sum(-1) / (M * ticks)). No IMU quaternion is fed back under a score (include/wbc.h)."""
    specs, flat = _flat_tracks(tracks)
    return _WbcRolloutTracksScored.apply(q0, task_params, inputs, dt, ticks, batch, mode, trunk_target_step, tuple(score), specs, *flat)


# ---- the constraint slack as a loss (wbc_state_slack_vjp / wbc_rollout_vjp_watched, include/wbc.h)
class _WbcStateSlack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, trunk_box_center, batch, model_id):
        q, box = _c(q), _c(trunk_box_center)
        out = batch.state_slack(q, box, model_id=model_id, want_components=True)
        ctx.batch, ctx.model_id, ctx.have_box = batch, model_id, box is not None
        ctx.set_materialize_grads(False)     # an output the loss does not use gives None: its cotangent is left out of the call
        ctx.save_for_backward(q, *([box] if box is not None else []))
        ctx.mark_non_differentiable(out["which"])
        return out["slack"], out["components"], out["which"]

    @staticmethod
    def backward(ctx, g_slack, g_comp, _gw):
        import wbc_workload
        q, *rest = ctx.saved_tensors
        if g_slack is None and g_comp is None:
            return None, None, None, None
        cg = lambda t: None if t is None else t.contiguous()      # noqa: E731
        r = ctx.batch.state_slack_grad(q, rest[0] if ctx.have_box else None, g_slack=cg(g_slack), g_components=cg(g_comp), model_id=ctx.model_id)
        need = ctx.needs_input_grad
        return (wbc_workload.tangent_to_raw(q, r["d_q"]) if need[0] else None,
                r["d_trunk_box_center"] if (need[1] and ctx.have_box) else None, None, None)


def wbc_state_slack(q, trunk_box_center, batch, model_id=None):
    """WbcBatch.state_slack as a differentiable layer: returns (slack [B,4], components [B,12], which [B,4] int32). slack and components are
    differentiable with respect to q [B,27] (raw coordinates: wbc_workload.tangent_to_raw of wbc_state_slack_vjp's d_q) and trunk_box_center
    [B,4]; a family's gradient is that of the component `which` names (at a tie: the lowest code, a subgradient). backward is ONE
    wbc_state_slack_vjp launch. A loss that puts a non-zero gradient on a trunk family needs trunk_box_center; a bad row (include/wbc.h) gets
    zero gradients. Contiguous float64 tensors on the handle's device."""
    return _WbcStateSlack.apply(q, trunk_box_center, batch, model_id)


class _WbcRolloutWatched(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q0, task_params, inputs, dt, ticks, batch, mode, held, watch, specs, *flat):      # (ten arguments, then the tracks': _tracks_sweep's layout)
        args = [_c(q0), _c(task_params)] + [_c(t) for t in flat]
        score = tuple(held.get("score", ()))
        out, tape = batch.rollout_record(dict(inputs, q=args[0]), dt, ticks, task_params=args[1], tracks=_tracks_of(specs, args[2:]) if specs else None,
                                         mode=mode, watch=watch, watch_trace=True, score=score, **{k: _c(v) for k, v in held.items() if k != "score"})
        ctx.batch, ctx.tape, ctx.watch, ctx.score = batch, tape, tuple(watch), score
        ctx.set_materialize_grads(False)     # an output the loss does not use gives None, not zeros: its seed is left out of the call
        _save(ctx, (out["q"], out["q_trace"], out["slack_min_tick"]) + ((out["err_max_tick"],) if score else ()), args)
        ctx.mark_non_differentiable(out["status"], out["slack_min_tick"], out["slack_min_which"], *((out["err_max_tick"],) if score else ()))
        res = (out["q"], out["qdot"], out["status"], out["q_trace"], out["slack_min"], out["slack_final"], out["slack_trace"], out["slack_min_tick"],
               out["slack_min_which"])
        return res + ((out["err_sq_sum"], out["err_final"], out["err_max"], out["err_max_tick"]) if score else ())

    @staticmethod
    def backward(ctx, g_q, g_qdot, _gst, g_trace, g_min, g_fin, g_str, _gt, _gw, g_sq=None, g_efin=None, g_max=None, _gtick=None):
        head, args = _saved(ctx, 4 if ctx.score else 3)
        q_final, q_trace, min_tick = head[:3]
        cg = lambda t: None if t is None else t.contiguous()      # noqa: E731
        seed = {}
        if not (g_min is None and g_fin is None and g_str is None):
            seed["watch_seed"] = dict(mask=ctx.watch, g_slack_min=cg(g_min), g_slack_final=cg(g_fin), g_trace=cg(g_str),
                                      slack_min_tick=None if g_min is None else min_tick, q_final=q_final)
        if not (g_sq is None and g_efin is None and g_max is None):
            seed["score_seed"] = dict(mask=ctx.score, g_err_sq_sum=cg(g_sq), g_err_final=cg(g_efin), g_err_max=cg(g_max),
                                      err_max_tick=None if g_max is None else head[3], q_final=q_final)
        return _tracks_sweep(ctx, args, g_q, g_qdot, g_trace, q_final, q_trace, **seed)


def wbc_rollout_watched(q0, task_params, inputs, dt, ticks, batch, watch=("com", "trunk_z", "trunk_ang", "joint"), tracks=None,
                        mode=capi.ROLLOUT_RUNNING, imu=None, trunk_target_step=None, ee_target_step=None, score=()):
    """A recorded roll-out with the slack families in `watch` as differentiable outputs ("and stay legal" as a loss): the forward is one
    WbcBatch.rollout_record(..., watch=watch, watch_trace=True) (wbc_rollout_record_watch, include/wbc.h), the backward one
    WbcBatch.rollout_vjp(..., watch_seed=...) (wbc_rollout_vjp_watched: the slacks' cotangents are formed where the sweep runs). tracks:
    None, or wbc_rollout_tracks_fused's list of dicts (points, tangents and du may require a gradient); without tracks ee_target_step is
    allowed (held constant). Returns wbc_rollout_tracks_fused's (q_final, qdot, status, q_trace) and then slack_min, slack_final [n_w,B],
    trace [ticks,n_w,B] (rows in increasing family order; differentiable: a hinge or barrier on trace is any per-tick penalty) and
    slack_min_tick, slack_min_which [n_w,B] int32 (not differentiable). score (with tracks; no IMU then): the scored frames as
    wbc_rollout_tracks_scored takes them — the tuple then ends with that layer's err_sq_sum, err_final, err_max (differentiable) and
    err_max_tick. Gradients flow to q0 (raw coordinates), task_params and the tracks; a loss may mix the slacks with the scores, q_final,
    qdot and q_trace: the gradients are those of the sum. An IMU quaternion may be fed back. Contiguous float64 tensors on the handle's
    device."""
    specs, flat = _flat_tracks(tracks) if tracks else ([], [])
    held = dict(imu=imu, trunk_target_step=trunk_target_step, ee_target_step=ee_target_step, score=tuple(score))
    return _WbcRolloutWatched.apply(q0, task_params, inputs, dt, ticks, batch, mode, held, tuple(watch), specs, *flat)
