"""Shared by test_gpu_handle_lifetime.py: the problems, the calls, the fresh-handle references and what holds those to the
oracle. A call on a long-lived handle must return, byte for byte, what the same call returns on a handle that was created, configured, given
the same options, called once and closed (`fresh`); every fresh reference is held to the CPU oracle, or to the numpy restatement for
tick_grad / state_slack, at the bound of the existing test that makes that call (`hold`, bounds imported, none written here).

Nothing here needs a GPU to import: `oracle_reference` and the conditions (`solved_by_the_oracle`, `certified_on_the_host`) run on the CPU."""
import functools

import numpy as np

import common
import grad_common as gc
import oracle
import slack_common as sc
import test_gpu_parity as par
import test_gpu_rollout_tracks as trk
import test_gpu_slack as tsl
import test_gpu_task_params as tgp
import test_gpu_tick_grad as tgg
import wbc_capi as capi
import wbc_workload
from wbc_batch import WbcBatch

DT = 0.002
MAX_BATCH = 70
BATCHES = (67, 5, 66, 1, 67)          # partial last waves, a smaller B with stale rows behind it, B < max_batch throughout
K = 3                                 # ticks of every roll-out
SEED = 11
SHIFT = 6                             # the "other inputs" of a call are rows SHIFT .. of the same 70 (a multiple of every mix's model count)
# (A): nv 26 / 25 / 25 interleaved by model_id, the ROT variants. The packed sim3, INEQ-orth and box plans decline the Laikago model
# (test_gpu_laikago.PATHS), and a batch takes a packed path only if every model's plan does: (A) runs on the general kernel except under c2.
# (B): one model, no model_id: the FIXD form. (C): (A) without the Laikago — the packed kernels with model_id, which the route is about.
MIXES = {"A": ("a1_wx200", "a1_px100_pin_ver", "laikago_vx300"), "B": ("a1_wx200",), "C": ("a1_wx200", "a1_px100_pin_ver")}
PACKED = {"A": False, "B": True, "C": True}
DEFAULTS = dict(packed_orth=1, packed_kernel=1, refine=1, presolve=1, presolve_tol_exp=7, dbg_force_defer=0, wave_order=1, warm_start=0)
POSTURE_CONFIGS = ("c3_hybrid", "c3_mani", "hybrid_grip_com")      # (their assembled arrays go through the posture kernel: ASSEMBLE_POSTURE_TOL)
FOOT = 0
# the switch sets of test_gpu_handle_lifetime._route, and those on which it makes the tick_grad call (test_handle_walk_host.py checks the
# conditions of their steps on the CPU)
ROUTE_CONFIGS = ("full", "c3", "c3+w", "c3_trunk_task", "everything", "c2", "c3_mani", "c3_hybrid", "hybrid_grip_com", "c3_two_feet")
GRAD_CONFIGS = ("c3", "c3+w", "c3_trunk_task", "everything", "c3_mani", "c3_hybrid")


# ------------------------------------------------------------------------------------------------ problems
@functools.lru_cache(maxsize=None)
def problem(mix, cfg_name):
    """every array has MAX_BATCH rows; a call at B takes the first B (or rows SHIFT .. SHIFT + B). Read-only."""
    names = list(MIXES[mix])
    base, _, other = cfg_name.partition("+")                   # "c3+w": the c3 switch set with other weights and gains on every model
    models, cfgs, d, mid = tgp._problem(names, base, MAX_BATCH, seed=SEED)
    if other:
        cfgs = [other_weights(c, seed=i) for i, c in enumerate(cfgs)]
    n = MAX_BATCH
    rng = np.random.default_rng(SEED + 3)
    rows = tgp._random_rows(tgp._rows_of(cfgs, mid, n), SEED + 5, w=(0.5, 2.0), g=(0.5, 2.0))
    v = gc.task_space_v(models, cfgs, mid, d, rng)
    step = np.zeros((n, 5, 3))
    step[:, common.GRIP] = (0.003, 0.0, -0.001)
    p = dict(models=models, cfgs=cfgs, d=d, mid=mid, rows=rows, v=v, ee_step=step, trunk_step=np.tile((0.0005, 0.0, -0.0005), (n, 1)),
             imu=d["q"][:, 3:7].copy(), vel=2.0 * rng.normal(size=(n, capi.V_STRIDE)), cfg_name=cfg_name)
    p["d_rot"] = common.add_rot_references({k: x.copy() for k, x in d.items()}, n, SEED)
    # the tracks / traj calls, rollout_recorded_cases' style: a gripper trajectory of three milestones; trunk (HERMITE), gripper and foot tracks
    pos = common.track_frames(models, d["q"], mid)
    pts = pos[:, None, common.GRIP] + rng.normal(0, 0.01, (n, 3, 3))
    pts[:, 0] = pos[:, common.GRIP]
    p["traj"] = dict(points=pts, n_points=rng.choice([2, 3], n).astype(np.int32), du=rng.choice([0.4, 0.5, 0.7], n))
    dt_ = {k: x.copy() for k, x in d.items()}
    trunk, grip = common.base_tracks(dt_, pos[:, common.GRIP], 5)
    fp = pos[:, None, FOOT] + rng.normal(0, 0.002, (n, 3, 3))
    fp[:, 0] = pos[:, FOOT]
    foot = dict(target=FOOT, points=fp, kind="linear", n_points=np.full(n, 3, np.int32), du=rng.choice([1 / 8, 0.3, 0.6], n))
    common.start_previous_targets(dt_, [trunk, grip, foot])
    p["d_tracks"], p["tracks"] = dt_, [grip, trunk, foot]
    for a in list(p.values()) + list(d.values()) + list(dt_.values()) + list(p["d_rot"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p


def other_weights(cfg, seed=0, fill_zeros=False):
    """the same switches, sizes and plan; every non-zero weight and gain of the 85 scaled by U(1.2, 1.8) (fill_zeros: the zeros set to that too)"""
    import ctypes
    import wbc_model
    c = capi.WbcConfig.from_buffer_copy(cfg)
    rows = wbc_model.task_params(cfg, 1)
    scale = np.random.default_rng(50 + seed).uniform(1.2, 1.8, rows.shape)
    rows = np.ascontiguousarray(np.where(rows != 0, rows * scale, scale if fill_zeros else 0.0))
    ctypes.memmove(ctypes.addressof(c) + capi.WbcConfig.ee_W.offset, rows.ctypes.data, capi.TASK_PARAMS_DOUBLES * 8)
    return c


@functools.lru_cache(maxsize=None)
def qp_problem(m, n, p):
    """test_qp_ls_packed_refined_matches_oracle's data: posture-like rows of 3e-5 under O(1) rows, one fixed variable, one equality row"""
    B = MAX_BATCH
    rng = np.random.default_rng(40 + n + p)
    A = np.concatenate([rng.normal(size=(B, m - n, n)), np.broadcast_to(3e-5 * np.eye(n), (B, n, n))], axis=1)
    b = np.concatenate([rng.normal(size=(B, m - n)), 3e-5 * rng.normal(size=(B, n))], axis=1)
    Cm = rng.normal(size=(B, p, n))
    lb, ub = -rng.uniform(0.5, 2.0, (B, n)), rng.uniform(0.5, 2.0, (B, n))
    lb[:, -1] = ub[:, -1] = 0.03
    cl, cu = -rng.uniform(0.1, 1.0, (B, p)), rng.uniform(0.1, 1.0, (B, p))
    cl[:, 0] = cu[:, 0] = 0.05
    return dict(A=A, b=b, C=Cm, lb=lb, ub=ub, Clb=cl, Cub=cu)


QP_SHAPES = {"qp32": (32, 26, 16), "qp12": (12, 8, 4)}


@functools.lru_cache(maxsize=None)
def warm_up_q0(mix):
    """each model's neutral configuration 0.4 m up (as test_gpu_laikago.py), the base moved in x, y per instance"""
    models = problem(mix, "c3")["models"]
    mid = problem(mix, "c3")["mid"]
    q0 = np.zeros((MAX_BATCH, capi.Q_STRIDE))
    for b in range(MAX_BATCH):
        q0[b] = models[0 if mid is None else mid[b]].neutral()
    q0[:, 2] = 0.4
    q0[:, 0:2] = np.random.default_rng(SEED + 9).uniform(-0.5, 0.5, (MAX_BATCH, 2))
    return q0


WARM_UP_TICKS = 20


def _rows(a, B, shift=0):
    return None if a is None else np.ascontiguousarray(a[shift:shift + B])


def _inputs(d, B, shift=0):
    return {k: _rows(v, B, shift) for k, v in d.items()}


def _track(t, B):
    return dict(t, points=_rows(t["points"], B), n_points=_rows(t["n_points"], B), du=_rows(t["du"], B))


# ------------------------------------------------------------------------------------------------ the calls
# name -> f(bt, p, B, cv): cv takes every input array to where the call reads it (numpy: as it is; device: a torch tensor). -> dict of outputs
def _dict(cv, d):
    return {k: cv(v) for k, v in d.items()}


def _tick(bt, p, B, cv):
    return bt.tick(_dict(cv, _inputs(p["d"], B)), DT, want_q_next=True, want_working_set=True)


def _tick_qdot_only(bt, p, B, cv):
    """no status buffer from the caller: the tick kernels of paths 1-4 write the handle's own"""
    d = _dict(cv, _inputs(p["d"], B))
    return bt.tick(d, DT, out=dict(qdot=bt._alloc(d["q"], (B, capi.V_STRIDE))))


def _tick_tp(bt, p, B, cv):
    return bt.tick(_dict(cv, _inputs(p["d"], B)), DT, want_q_next=True, task_params=cv(_rows(p["rows"], B)))


def _assemble(bt, p, B, cv):
    return bt.assemble(_dict(cv, _inputs(p["d"], B)), DT)


def _tick_grad(bt, p, B, cv):
    return bt.tick_grad(_dict(cv, _inputs(p["d"], B)), DT, cv(_rows(p["v"], B)), task_params=cv(_rows(p["rows"], B)))


def _rollout(bt, p, B, cv, shift=0):
    return bt.rollout(_dict(cv, _inputs(p["d"], B, shift)), DT, K, ee_target_step=cv(_rows(p["ee_step"], B, shift)),
                      trunk_target_step=cv(_rows(p["trunk_step"], B, shift)), imu=cv(_rows(p["imu"], B, shift)), want_trace=True)


def _rollout_shift(bt, p, B, cv):
    return _rollout(bt, p, min(B, MAX_BATCH - SHIFT), cv, SHIFT)


def _rollout_warmup_rot(bt, p, B, cv):
    """WARMUP mode with orientation references: the optional blocks ee_prev_rot / trunk_prev_rot of the roll-out workspace are in use"""
    return bt.rollout(_dict(cv, _inputs(p["d_rot"], B)), DT, K, ee_target_step=cv(_rows(p["ee_step"], B)), want_trace=True, mode=capi.ROLLOUT_WARMUP)


def _rollout_traj(bt, p, B, cv):
    t = p["traj"]
    return bt.rollout_traj(_dict(cv, _inputs(p["d"], B)), DT, K, cv(_rows(t["points"], B)), n_points=cv(_rows(t["n_points"], B)), du=cv(_rows(t["du"], B)),
                           want_trace=True, imu=cv(_rows(p["imu"], B)))


def _tracks_of(p, B, cv):
    return [dict(t, points=cv(t["points"]), n_points=cv(t["n_points"]), du=cv(t["du"])) for t in (_track(t, B) for t in p["tracks"])]


def _rollout_tracks(bt, p, B, cv):
    return bt.rollout_tracks(_dict(cv, _inputs(p["d_tracks"], B)), DT, K, _tracks_of(p, B, cv), score=(common.GRIP, "trunk", FOOT), want_trace=True,
                             imu=cv(_rows(p["imu"], B)))


def _rollout_watch(bt, p, B, cv):
    return bt.rollout_watch(_dict(cv, _inputs(p["d"], B)), DT, K, tracks=None, ee_target_step=cv(_rows(p["ee_step"], B)), imu=cv(_rows(p["imu"], B)),
                            want_trace=True, hold_ticks=1)


def _warm_up(bt, p, B, cv):
    """setInitialState for the batch, host arrays only: puts the warm-up switch set on the handle and leaves it there"""
    return bt.warm_up(_rows(warm_up_q0(bt.walk_mix), B), _rows(p["mid"], B), DT, WARM_UP_TICKS, configure=True)


def _mid(p, B, cv):
    return None if p["mid"] is None else cv(_rows(p["mid"], B))


def _update_state(bt, p, B, cv):
    d = p["d"]
    n = min(B, MAX_BATCH - SHIFT)
    return dict(q_new=bt.update_state(cv(_rows(d["q"], n)), cv(_rows(d["q"], n, SHIFT)), cv(_rows(d["ee_target"], n)), cv(_rows(p["imu"], n)), _mid(p, n, cv)))


def _posture_target(bt, p, B, cv):
    u, qa = bt.posture_target(cv(_rows(p["d"]["q"], B)), _mid(p, B, cv))
    return dict(u=u, q_after=qa)


def _state_slack(bt, p, B, cv):
    return bt.state_slack(cv(_rows(p["d"]["q"], B)), cv(_rows(p["d"]["trunk_box_center"], B)), _mid(p, B, cv), want_components=True)


def _fk(bt, p, B, cv):
    return bt.fk(cv(_rows(p["d"]["q"], B)), _mid(p, B, cv))


def _integrate(bt, p, B, cv):
    return dict(q_next=bt.integrate(cv(_rows(p["d"]["q"], B)), cv(_rows(p["vel"], B)), DT, _mid(p, B, cv)))


def _qp(name):
    def call(bt, p, B, cv):
        z = {k: cv(_rows(v, B)) for k, v in qp_problem(*QP_SHAPES[name]).items()}
        x, st, it, ws = bt.qp_solve_ls(z["A"], z["b"], z["C"], z["lb"], z["ub"], z["Clb"], z["Cub"], want_working_set=True)
        return dict(x=x, status=st, iters=it, working_set=ws)
    return call


CALLS = {"tick": _tick, "tick_qdot_only": _tick_qdot_only, "tick_tp": _tick_tp, "assemble": _assemble, "tick_grad": _tick_grad, "rollout": _rollout,
         "rollout_shift": _rollout_shift, "rollout_warmup_rot": _rollout_warmup_rot, "rollout_traj": _rollout_traj, "rollout_tracks": _rollout_tracks,
         "rollout_watch": _rollout_watch, "update_state": _update_state, "posture_target": _posture_target, "state_slack": _state_slack, "fk": _fk,
         "integrate": _integrate, "warm_up": _warm_up, "qp32": _qp("qp32"), "qp12": _qp("qp12")}

# the statistics that apply to a call: what the call itself sets (a statistic another family's call left behind is not this call's to define)
_TICK = ("last_path", "last_tick_variant", "last_tick_fixd", "deferred_last")
_ROLL = _TICK + ("last_update_packed",)
STATS = {"tick": _TICK, "tick_qdot_only": _TICK, "tick_tp": _TICK, "assemble": ("last_tick_variant",), "tick_grad": _TICK + ("last_grad_variant",),
         "rollout": _ROLL, "rollout_shift": _ROLL, "rollout_warmup_rot": _ROLL, "rollout_traj": _ROLL + ("last_traj_bad_rows",),
         "rollout_tracks": _ROLL + ("last_traj_bad_rows",), "rollout_watch": _ROLL, "warm_up": _ROLL, "update_state": ("last_update_packed",),
         "posture_target": ("last_posture_par",), "state_slack": (), "fk": ("last_tick_variant",), "integrate": (),
         "qp32": ("last_qp_path", "last_qp_variant"), "qp12": ("last_qp_path", "last_qp_variant")}
WAITING_STATS = ("deferred_last", "last_traj_bad_rows")     # these read device memory: wbc_batch_get_stat waits for the stream it is given
TICK_CALLS = tuple(k for k, v in STATS.items() if "last_path" in v)


def stats_of(cfg_name, call):
    extra = ("last_posture_par",) if cfg_name == "c3_mani" and (call in TICK_CALLS or call == "assemble") else ()    # MANI: the posture kernel runs ahead of the tick
    return STATS[call] + extra


# ------------------------------------------------------------------------------------------------ running a call in either memory kind
class Device:
    """torch device tensors on a side stream (non-blocking, as torch's are), outputs prefilled with NaN / -1 through the allocator hook"""

    def __init__(self):
        import torch
        self.torch = torch
        self.stream = torch.cuda.Stream()

    def cv(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def alloc(self, like, shape, dtype):
        t = self.torch
        td = {np.float64: t.float64, np.int32: t.int32, np.int64: t.int64}[dtype]
        return t.full(tuple(shape), float("nan") if dtype is np.float64 else -1, dtype=td, device="cuda")

    def launch(self, bt, cfg_name, call, B):
        """enqueue only -> the outputs as device tensors, the statistics that need no wait"""
        p = problem(bt.walk_mix, cfg_name)
        self.stream.wait_stream(self.torch.cuda.current_stream())
        bt.allocator = self.alloc
        try:
            with self.torch.cuda.stream(self.stream):
                out = CALLS[call](bt, p, B, self.cv)
        finally:
            bt.allocator = None
        return out, {s: bt.stat(s) for s in stats_of(cfg_name, call) if s not in WAITING_STATS}

    def finish(self, bt, cfg_name, call, out, stats, waiting=True):
        self.stream.synchronize()
        if waiting:
            stats = dict(stats, **{s: bt.stat(s, self.stream.cuda_stream) for s in stats_of(cfg_name, call) if s in WAITING_STATS})
        return {k: v.cpu().numpy() for k, v in out.items()}, stats

    def run(self, bt, cfg_name, call, B):
        out, stats = self.launch(bt, cfg_name, call, B)
        return self.finish(bt, cfg_name, call, out, stats)


class Host:
    """numpy arrays: the library stages them through its own workspace `ws` on the null stream; outputs prefilled likewise"""

    @staticmethod
    def cv(a):
        return a

    @staticmethod
    def alloc(like, shape, dtype):
        return np.full(tuple(shape), np.nan if dtype is np.float64 else -1, dtype=dtype)

    def run(self, bt, cfg_name, call, B):
        p = problem(bt.walk_mix, cfg_name)
        bt.allocator = self.alloc
        try:
            out = CALLS[call](bt, p, B, self.cv)
        finally:
            bt.allocator = None
        return {k: np.asarray(v) for k, v in out.items()}, {s: bt.stat(s) for s in stats_of(cfg_name, call)}


def new_handle(mix, cfg_name=None, options=()):
    """a handle of `mix`; with cfg_name: configured with it, model by model, then given `options` ((name, value) pairs) in order"""
    p = problem(mix, cfg_name or "c3")
    bt = WbcBatch(p["models"], MAX_BATCH)
    bt.walk_mix = mix
    if cfg_name is not None:
        for i, c in enumerate(p["cfgs"]):
            bt.configure(c, i)
    for k, v in options:
        bt.set_option(k, v)
    return bt


def option_key(options):
    """the options that differ from the defaults, sorted: what a fresh handle is given"""
    return tuple(sorted((k, v) for k, v in options.items() if DEFAULTS[k] != v))


_FRESH = {}


def fresh(mix, cfg_name, options, call, B, mem):
    """(outputs, statistics) of the call on a handle created, configured, given the options, called once and closed; held to the oracle before
    it is returned the first time. options: option_key(...). mem: a Host or a Device."""
    key = (mix, cfg_name, options, call, B, type(mem).__name__)
    if key not in _FRESH:
        bt = new_handle(mix, cfg_name, options)
        try:
            got = mem.run(bt, cfg_name, call, B)
        finally:
            bt.close()
        hold(mix, cfg_name, options, call, B, got[0])
        for a in got[0].values():
            a.setflags(write=False)
        _FRESH[key] = got
    return _FRESH[key]


def differences(got, want):
    """key set, dtype, shape, bytes of every output and the statistics -> list of what differs (empty: the call equals fresh)"""
    (out, stats), (wout, wstats) = got, want
    bad = []
    if set(out) != set(wout):
        return ["keys %s" % sorted(set(out) ^ set(wout))]
    for k, v in out.items():
        w = wout[k]
        if v.dtype != w.dtype or v.shape != w.shape:
            bad.append("%s: %s %s, fresh %s %s" % (k, v.dtype, v.shape, w.dtype, w.shape))
        elif v.tobytes() != w.tobytes():
            rows = v.reshape(len(v), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8) if v.ndim and len(v) else np.ones((1, 1), bool)
            bad.append("%s: bytes differ in %d of %d leading rows" % (k, int(rows.any(axis=1).sum()), len(rows)))
    if stats != wstats:
        bad.append("statistics %s, fresh %s" % (stats, wstats))
    return bad


# ------------------------------------------------------------------------------------------------ the oracle and the conditions
NTHREADS = 8                          # of the oracle's batch calls


@functools.lru_cache(maxsize=None)
def oracle_reference(mix, cfg_name, call, B):
    """what the CPU oracle gives for the call's inputs (the calls held to a restatement of the device's own outputs are not here)"""
    p = problem(mix, cfg_name)
    models, cfgs, mid = p["models"], p["cfgs"], _rows(p["mid"], B)
    d = _inputs(p["d"], B)
    if call in ("tick", "tick_qdot_only"):
        return oracle.tick(models, cfgs, d, DT, B, nthreads=NTHREADS)
    if call == "tick_tp":
        ms, cs, pid = tgp._per_instance(models, cfgs, mid, _rows(p["rows"], B))
        ref = oracle.tick(ms, cs, dict(d, model_id=pid), DT, B, nthreads=NTHREADS)
        tol, ratio = tgp._qdot_tol(models, cfgs, mid, d, ms, cs, pid, B)
        return dict(ref, tol=tol, ratio=ratio)
    if call == "assemble":
        return oracle.assemble(models, cfgs, d, DT, B)
    if call in ("rollout", "rollout_shift", "rollout_watch"):
        n, sh = (min(B, MAX_BATCH - SHIFT), SHIFT) if call == "rollout_shift" else (B, 0)
        # the watch call holds one tick more: tick K runs on the targets the K steps left, which is what a (K + 1)-th stepping tick runs on (only the
        # targets handed back differ, and they are not compared); the trunk step is the plain calls' alone
        ticks, tstep = (K + 1, None) if call == "rollout_watch" else (K, _rows(p["trunk_step"], n, sh))
        return oracle.rollout(models, cfgs, _inputs(p["d"], n, sh), DT, n, ticks, ee_target_step=_rows(p["ee_step"], n, sh), trunk_target_step=tstep,
                              imu=_rows(p["imu"], n, sh), nthreads=NTHREADS)
    if call == "warm_up":
        return oracle.warmup(models, _rows(warm_up_q0(mix), B), DT, WARM_UP_TICKS, model_id=mid, nthreads=NTHREADS)
    if call == "rollout_warmup_rot":
        return oracle.rollout(models, cfgs, _inputs(p["d_rot"], B), DT, B, K, ee_target_step=_rows(p["ee_step"], B), nthreads=NTHREADS, running=False)
    if call in ("rollout_traj", "rollout_tracks"):
        if call == "rollout_traj":
            tracks, dd = [dict(_track(p["traj"], B), target=common.GRIP, kind="linear")], d
        else:
            tracks, dd = [_track(t, B) for t in p["tracks"]], _inputs(p["d_tracks"], B)
        return common.tracks_reference(dict(models=models, cfgs=cfgs, mid=mid, B=B, K=K, d=dd, rows=None, tracks=tracks, imu=_rows(p["imu"], B), running=True))
    if call == "update_state":
        n = min(B, MAX_BATCH - SHIFT)
        return oracle.update_state(models, _rows(p["d"]["q"], n), _rows(p["d"]["q"], n, SHIFT), _rows(p["d"]["ee_target"], n), _rows(p["imu"], n), _rows(p["mid"], n))
    if call == "posture_target":
        return oracle.posture_target(models, cfgs, d["q"], mid, nthreads=NTHREADS)
    if call == "state_slack":
        return sc.reference_slack(models, cfgs, d["q"], d["trunk_box_center"], mid)
    if call == "fk":
        return oracle.fk(models, d["q"], mid)
    if call == "integrate":
        return oracle.integrate(models, d["q"], _rows(p["vel"], B), DT, mid)
    if call in QP_SHAPES:
        z = {k: _rows(v, B) for k, v in qp_problem(*QP_SHAPES[call]).items()}
        return oracle.qp_solve_ls(z["A"], z["b"], z["C"], z["lb"], z["ub"], z["Clb"], z["Cub"])
    raise KeyError(call)


def solved_by_the_oracle(mix, cfg_name, B):
    """instances of the (switch set, model mix, B) tick that the oracle alone solves"""
    return int((oracle_reference(mix, cfg_name, "tick", B)["status"] == 0).sum())


@functools.lru_cache(maxsize=None)
def certified_on_the_host(mix, cfg_name, B):
    """instances of the tick_grad step that the oracle solves and wbc_workload.qp_certificate certifies (the (A, b) form, unit rows on a smaller
    model's padded columns as WbcBatch.tick_certificate adds them)"""
    p = problem(mix, cfg_name)
    mid = _rows(p["mid"], B)
    ms, cs, pid = tgp._per_instance(p["models"], p["cfgs"], mid, _rows(p["rows"], B))
    d = dict(_inputs(p["d"], B), model_id=pid)
    t, a = oracle.tick(ms, cs, d, DT, B, nthreads=NTHREADS), oracle.assemble(ms, cs, d, DT, B)
    has = a["C"].shape[1] > 0
    n_ok = 0
    for i in range(B):
        if t["status"][i] != 0:
            continue
        nv = ms[i].nv
        A = np.concatenate([a["A"][i], np.eye(capi.V_STRIDE)[nv:]], axis=0)
        b = np.concatenate([a["b"][i], np.zeros(capi.V_STRIDE - nv)])
        c = wbc_workload.qp_certificate(t["qdot"][i], A=A, b=b, C_=a["C"][i] if has else None, lb=a["lb"][i], ub=a["ub"][i],
                                        Clb=a["Clb"][i] if has else None, Cub=a["Cub"][i] if has else None, v=_rows(p["v"], B)[i])
        n_ok += int(c["cert_status"] == capi.CERT_OK)
    return n_ok


def _enough(ok, B, what):
    if B >= 5:
        assert int(ok.sum()) >= B // 2, "%s: the oracle solves %d of %d instances — the step would pass nearly empty" % (what, int(ok.sum()), B)


def hold(mix, cfg_name, options, call, B, got):
    """the fresh reference `got` against the oracle / the restatement at the bound of the test that already makes the call; the
    non-emptiness conditions of the step"""
    what = "%s / %s / %s B=%d %s" % (mix, cfg_name, call, B, dict(options))
    p = problem(mix, cfg_name)
    models, cfgs, mid = p["models"], p["cfgs"], _rows(p["mid"], B)
    opts = dict(DEFAULTS, **dict(options))
    if call == "tick_grad":
        d, rows = _inputs(p["d"], B), _rows(p["rows"], B)
        ref, bad = tgg._reference(models, cfgs, mid, d, rows, got)
        if B >= 5:
            assert B - int(bad.sum()) >= B // 2 and certified_on_the_host(mix, cfg_name, B) >= B // 2, what
        for k in (k for k in got if k.startswith("d_")):
            ratio = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
            assert ratio <= tgg.PARITY_BOUND, (what, k, ratio)
        return
    ref = oracle_reference(mix, cfg_name, call, B)
    if call == "warm_up":
        assert (got["status"] == ref["status"]).all() and np.abs(got["q"] - ref["q"]).max() < par.ROLLOUT_Q_TOL, what
    elif call in ("tick", "tick_qdot_only", "tick_tp"):
        ok = ref["status"] == 0
        _enough(ok, B, what)
        if "status" in got:
            assert (got["status"] == ref["status"]).all(), what
        if call == "tick_tp":
            if ok.any():
                tgp._check_qdot(got, ref, ref["tol"], ref["ratio"], what)
        elif ok.any():
            assert np.abs(got["qdot"] - ref["qdot"])[ok].max() < par.QDOT_TOL, what
    elif call == "assemble":
        bound = par.ASSEMBLE_POSTURE_TOL if cfg_name in POSTURE_CONFIGS else par.ASSEMBLE_TOL
        for k, v in ref.items():
            assert got[k].shape == v.shape and par.relerr(got[k], v) < bound, (what, k, par.relerr(got[k], v))
    elif call.startswith("rollout"):
        ok = ref["status"] == 0
        _enough(ok, B, what)
        assert (got["status"] == ref["status"]).all(), what
        if ok.any():
            assert np.abs(got["q"] - ref["q"])[ok].max() < par.ROLLOUT_Q_TOL, what
            assert np.abs(got["qdot"] - ref["qdot"])[ok].max() < 10 * par.QDOT_TOL, what
            reached = ref["frames"][:, :, common.GRIP] if "frames" in ref else ref["grip_trace"]
            assert np.abs(got["grip_trace"] - reached)[:, ok].max() < par.ROLLOUT_Q_TOL, what
            if call == "rollout_tracks":                           # the scored frames in increasing index order: FOOT, GRIP, the trunk
                for j, f in enumerate((FOOT, common.GRIP, common.TRUNK)):
                    assert np.abs(got["trace"][:, j] - ref["frames"][:, :, f])[:, ok].max() < trk.TAU, (what, f)
        if call == "rollout_watch":                                # the watch's last row is the restatement at the state the call returns
            n = len(got["q"])
            own = sc.reference_slack(models, cfgs, got["q"], _rows(p["d"]["trunk_box_center"], n), mid)
            fin = np.isfinite(own["slack"].T)
            assert fin.any() and np.abs(got["slack_final"] - own["slack"].T)[fin].max() < tsl.SLACK_TOL, what
            assert wbc_workload.watch_summary(got["slack_trace"])["slack_final"].tobytes() == got["slack_final"].tobytes(), what
        if opts["warm_start"] and B >= 66 and cfg_name != "c2":       # (c2 has no inequality: its working sets are empty by definition)
            # a warm-started roll-out seeds tick 1 with tick 0's working set: the tick's own, on the same inputs
            ws = fresh(mix, cfg_name, options, "tick", B, Host())[0]["working_set"]
            assert ws[SHIFT if call == "rollout_shift" else 0:].any(), "%s: no instance has a working set to carry" % what
    elif call == "update_state":
        assert np.abs(got["q_new"] - ref).max() < par.UPDATE_TOL, what
    elif call == "posture_target":
        assert np.abs(got["u"] - ref[0]).max() < par.POSTURE_TOL and (got["q_after"] == ref[1]).all(), what
    elif call == "state_slack":
        assert np.abs(got["slack"] - ref["slack"]).max() < tsl.SLACK_TOL and np.abs(got["components"] - ref["components"]).max() < tsl.SLACK_TOL, what
    elif call == "fk":
        for k, v in ref.items():
            assert np.abs(got[k] - v).max() < par.FK_TOL, (what, k)
    elif call == "integrate":
        assert np.abs(got["q_next"] - ref).max() < par.INTEGRATE_TOL, what
    elif call in QP_SHAPES:
        xr, sr, _ = ref
        ok = sr == 0
        _enough(ok, B, what)
        assert (got["status"] == sr).all(), what
        if ok.any():
            assert np.abs(got["x"] - xr)[ok].max() < par.QP_LS_TOL, what
    else:
        raise KeyError(call)
