"""The long-horizon cases shared by test_long_horizon_host.py (the oracle alone, no GPU) and test_gpu_long_horizon.py.

Every case is a closed loop of K = 300 ticks of 2 ms on 16 (mixed: 19) instances, the gripper target stepping by N(0, 2e-4) m per tick and
instance. A problem, the oracle's own roll-out of it and the quantities derived from that roll-out are built once and handed out read-only.

The one-step reference: K x B taped states stacked into one batch of K * B instances and handed to the oracle once (stacked / oracle_tick /
oracle_assemble). The active-side rule is common.exact_optimum's (wbc_workload.qp_active_sides without a working set), vectorised."""
import functools

import numpy as np

import common
import oracle
import pose_cases as pc
import step_common as sc
import test_gpu_task_params as tgp
import wbc_workload

K, DT = 300, 0.002
STEP_SIGMA, STEP_SEED, INPUT_SEED = 2e-4, 1, 5
T = pc.T
WX, PX, LK = "a1_wx200", "a1_px100_pin_ver", "laikago_vx300"
ACT_TOL = 1e-7             # common.exact_optimum / wbc_workload.qp_active_sides: active within 1e-7 x max(1, |bound|)
FEAS_TOL = 1e-9            # the solvers' violation tolerance: an active row is met at least this well
LEFT_OUT_CAP = 0.05
QP_INF = wbc_workload.QP_INF

# case -> models, configuration, batch, handle options, the path's existing tolerance against the oracle (pose_cases / test_gpu_parity), the
# settings of option warm_start the case runs under (1 only where the path has a WARM variant), row(warm) -> (family, flags) as
# "last_tick_variant" reports it after the roll-out (None: the compact kernel, which has no variant table: path alone), with_rot as
# test_rollout_parity has it, tape: rollout_record takes the configuration
CASES = {
    "c3": dict(models=(WX,), cfg="c3", B=16, opts={}, tol=pc.REFINED_TOL, warm=(0, 1), row=lambda w: ("sim3p", (w, 0, 0, 0, 0))),
    "c3_general": dict(models=(WX,), cfg="c3", B=16, opts=pc.GEN, tol=pc.QDOT_TOL, warm=(0, 1), row=lambda w: ("general", (T, w, 0, 0, 0))),
    "c3_compact": dict(models=(WX,), cfg="c3", B=16, opts={"packed_kernel": 0, "refine": 0}, tol=pc.QDOT_TOL, warm=(0,), row=None, path=1),
    "c3_trunk_task": dict(models=(WX,), cfg="c3_trunk_task", B=16, opts={}, tol=pc.QDOT_TOL, warm=(0, 1), row=lambda w: ("sim3p", (w, 1, 0, 0, 0)),
                          with_rot=True),
    "c3_tp": dict(models=(WX,), cfg="c3", B=16, opts={}, tol=pc.QDOT_TOL, warm=(0, 1), row=lambda w: ("sim3p", (w, 0, 0, 0, 1)), tp=True),
    "everything": dict(models=(WX,), cfg="everything", B=16, opts=pc.PO, tol=pc.QDOT_TOL, warm=(0, 1), row=lambda w: ("orthp", (1, w, 0, 0)),
                       with_rot=True),
    "c2": dict(models=(WX,), cfg="c2", B=16, opts=pc.PO, tol=pc.QDOT_TOL, warm=(0,), row=lambda w: ("orthp", (0, 0, 0, 0))),
    "full": dict(models=(WX,), cfg="full", B=16, opts={}, tol=pc.QDOT_TOL, warm=(0, 1), row=lambda w: ("boxp", (w, 0, 0)), with_rot=True),
    "mixed": dict(models=(WX, PX, LK), cfg="c3", B=19, opts={}, tol=pc.QDOT_TOL, warm=(0, 1), row=lambda w: ("general", (T, w, 0, 1, 0))),
    # HYBRID as sim3.py sets it: the packed kernel forms the static posture target itself (test_tick_parity_posture_modes: no QCON row,
    # REFINED_TOL); rollout_record refuses the mode without posture_u, so the one-tick chain supplies its states
    "c3_hybrid": dict(models=(WX,), cfg="c3_hybrid", B=16, opts={}, tol=pc.REFINED_TOL, warm=(0,), row=lambda w: ("sim3p", (w, 0, 0, 0, 0)),
                      tape=False),
}
RECORDED = tuple(n for n, c in CASES.items() if c.get("tape", True))
WARM_CASES = tuple(n for n in RECORDED if 1 in CASES[n]["warm"])
AMPLIFICATION_TICKS = (10, 100, 300)


def _freeze(*dicts):
    for d in dicts:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> dict(models, cfgs, d, mid, rows, step [B, 5, 3], imu, B, ms / cs / pid: the oracle's form of the per-instance rows)"""
    case = CASES[name]
    B = case["B"]
    # test_gpu_task_params._problem's interleaving of several models, on the nominal inputs (stress=False: nothing starts at a bound or a box
    # edge; what becomes active does so because the loop went there)
    models = [tgp._model(n) for n in case["models"]]
    cfgs = [common.config(case["cfg"], m) for m in models]
    seed, rot = case.get("seed", INPUT_SEED), case.get("with_rot", False)
    mid = None
    if len(models) == 1:
        d = common.tick_inputs(models[0], cfgs[0], B, seed=seed, stress=False, with_rot=rot)
    else:
        mid = (np.arange(B) % len(models)).astype(np.int32)
        d = pc.merge([common.tick_inputs(m, c, B, seed=seed + i, stress=False, with_rot=rot) for i, (m, c) in enumerate(zip(models, cfgs))], mid)
    step = np.zeros((B, 5, 3))
    step[:, common.GRIP] = np.random.default_rng(STEP_SEED).normal(0, case.get("sigma", STEP_SIGMA), (B, 3))
    rows = pc.gain_rows(cfgs[0], B, INPUT_SEED + 7) if case.get("tp") else None
    ms, cs, pid = models, cfgs, mid
    if rows is not None:
        ms, cs, pid = common.per_instance_configs(models, cfgs, mid, rows)
    imu = d["q"][:, 3:7].copy()
    p = dict(name=name, case=case, models=models, cfgs=cfgs, d=d, mid=mid, rows=rows, step=step, imu=imu, B=B, K=case.get("K", K), ms=ms, cs=cs, pid=pid)
    _freeze(d, p)
    return p


def _oracle_inputs(p, d, reps=1):
    """the oracle's form of inputs for `reps` stacked copies of the batch"""
    dd = {k: v for k, v in d.items() if k != "model_id"}
    if p["pid"] is not None:
        dd["model_id"] = np.tile(p["pid"], reps)
    return dd


def oracle_tick(p, d, reps=1):
    return oracle.tick(p["ms"], p["cs"], _oracle_inputs(p, d, reps), DT, reps * p["B"], nthreads=8)


def oracle_assemble(p, d, reps=1):
    return oracle.assemble(p["ms"], p["cs"], _oracle_inputs(p, d, reps), DT, reps * p["B"])


def target_sums(p, ticks):
    """ee_target [ticks + 1, B, 5, 3]: the running sums in the roll-out's order, e_{k+1} = e_k + step"""
    e = np.empty((ticks + 1,) + p["d"]["ee_target"].shape)
    e[0] = p["d"]["ee_target"]
    for k in range(ticks):
        e[k + 1] = e[k] + p["step"]
    return e


def stacked(p, q, ee_target, prev_ee_target, trunk_target=None, prev_trunk_target=None, head=None):
    """the inputs of len(q) ticks as ONE batch of len(q) * B instances, tick-major: tick 0 reads the call's inputs, every later tick the
    previous rotations that step_common.advance leaves (they no longer change after the first tick) or, with `head`, the ones the tape's
    head holds (ee_prev_rot, trunk_prev_rot: what the device's ticks read); q [n, B, 27] and the targets as taped"""
    n, B = len(q), p["B"]
    d0 = {k: np.array(v, copy=True) for k, v in p["d"].items()}
    d1 = sc.advance(p["cfgs"][0], d0, d0["q"], None)
    for k in ("ee_prev_rot", "trunk_prev_rot"):
        if head is not None and k in head and k in d1:
            d1[k] = np.asarray(head[k]).reshape(d1[k].shape)
    out = {}
    for k in d0:
        out[k] = np.concatenate([d0[k][None]] + [d1[k][None]] * (n - 1)).reshape((n * B,) + d0[k].shape[1:])
    out["q"] = np.ascontiguousarray(q).reshape(n * B, 27)
    out["ee_target"] = np.ascontiguousarray(ee_target).reshape(n * B, 5, 3)
    out["prev_ee_target"] = np.ascontiguousarray(prev_ee_target).reshape(n * B, 5, 3)
    if trunk_target is not None:
        out["trunk_target"] = np.ascontiguousarray(trunk_target).reshape(n * B, 3)
        out["prev_trunk_target"] = np.ascontiguousarray(prev_trunk_target).reshape(n * B, 3)
    return out


def closed_loop(p, q0=None, ticks=None):
    """the oracle's own roll-out with every tick kept: q [K + 1, B, 27] (q[k]: the state tick k reads), qdot [K, B, 26], status, iters [K, B],
    ee_target, prev_ee_target [K, B, 5, 3], trunk_target, prev_trunk_target [K, B, 3] as tick k read them"""
    B, n = p["B"], p["K"] if ticks is None else ticks
    cfg = p["cfgs"][0]
    d = {k: np.array(v, copy=True) for k, v in p["d"].items()}
    if q0 is not None:
        d["q"] = np.array(q0, copy=True)
    r = dict(q=np.zeros((n + 1, B, 27)), qdot=np.zeros((n, B, 26)), status=np.zeros((n, B), np.int32), iters=np.zeros((n, B), np.int32),
             ee_target=np.zeros((n, B, 5, 3)), prev_ee_target=np.zeros((n, B, 5, 3)), trunk_target=np.zeros((n, B, 3)), prev_trunk_target=np.zeros((n, B, 3)))
    for k in range(n):
        r["q"][k] = d["q"]
        for f in ("ee_target", "prev_ee_target", "trunk_target", "prev_trunk_target"):
            r[f][k] = d[f]
        o = oracle_tick(p, d)
        r["qdot"][k], r["status"][k], r["iters"][k] = o["qdot"], o["status"], o["iters"]
        q_new = oracle.update_state(p["models"], d["q"], o["q_next"], d["ee_target"], p["imu"], p["mid"])
        d = sc.advance(cfg, d, q_new, p["step"])
    r["q"][n] = d["q"]
    _freeze(r)
    return r


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    return closed_loop(problem(name))


def compared(status):
    """[K, B] bool: an instance is compared up to and including its first unsolved tick"""
    bad = status != 0
    before = np.cumsum(bad, axis=0) - bad
    return before == 0


# ---- the active sides of K * B answers at once
def active_sides(a, x):
    """wbc_workload.qp_active_sides (no working set) for a batch -> (side [N, 26 + p] int32: 0 inactive, 1 lower, 2 upper, 3 equality;
    near [N] bool: some inequality side lies between the solvers' feasibility tolerance and twice the rule's threshold from its bound — a
    rounding-sized change of the answer, or the solver's own tolerance, decides which side of the rule it falls on)"""
    lo = np.concatenate([a["lb"], a["Clb"]], axis=1)
    hi = np.concatenate([a["ub"], a["Cub"]], axis=1)
    val = np.concatenate([x, np.einsum("bpn,bn->bp", a["C"], x)], axis=1)
    flo, fhi = np.abs(lo) < QP_INF, np.abs(hi) < QP_INF
    slo, shi = np.maximum(1.0, np.abs(lo)), np.maximum(1.0, np.abs(hi))
    dlo, dhi = np.abs(val - lo), np.abs(val - hi)
    eq = (lo == hi) & flo
    at_lo = flo & (dlo < ACT_TOL * slo)
    at_hi = fhi & (dhi < ACT_TOL * shi) & ~at_lo
    side = np.where(eq, 3, np.where(at_lo, 1, np.where(at_hi, 2, 0))).astype(np.int32)
    near = (~eq & ((flo & (dlo > FEAS_TOL * slo) & (dlo < 2 * ACT_TOL * slo)) | (fhi & (dhi > FEAS_TOL * shi) & (dhi < 2 * ACT_TOL * shi)))).any(axis=1)
    return side, near


def taped_sides(ws, p_rows):
    """[N, 2] int64 working sets (include/wbc.h: word 0 the velocity bounds, word 1 the rows; bit i the lower side, bit 32 + i the upper)
    -> side [N, 26 + p] with 0 / 1 / 2"""
    u = np.ascontiguousarray(ws).view(np.uint64).reshape(-1, 2)
    out = np.zeros((len(u), 26 + p_rows), np.int32)
    for word, n, off in ((0, 26, 0), (1, p_rows, 26)):
        for i in range(n):
            lo = (u[:, word] >> np.uint64(i)) & np.uint64(1)
            hi = (u[:, word] >> np.uint64(32 + i)) & np.uint64(1)
            out[:, off + i] = np.where(lo == 1, 1, np.where(hi == 1, 2, 0))
    return out


@functools.lru_cache(maxsize=None)
def oracle_sets(name):
    """the exact active sides along the oracle's own roll-out: (side [K, B, 26 + p], near [K, B])"""
    p, r = problem(name), oracle_run(name)
    n = p["K"]
    a = oracle_assemble(p, stacked(p, r["q"][:n], r["ee_target"], r["prev_ee_target"], r["trunk_target"], r["prev_trunk_target"]), n)
    side, near = active_sides(a, r["qdot"].reshape(n * p["B"], 26))
    side, near = side.reshape(n, p["B"], -1), near.reshape(n, p["B"])
    side.setflags(write=False)
    near.setflags(write=False)
    return side, near


def set_events(side, live):
    """per instance: (a constraint absent at tick 0 is present later, a constraint present at some tick is absent later), inequalities only,
    over the ticks `live` [K, B]"""
    act = ((side == 1) | (side == 2)) & live[:, :, None]
    added = (act[1:] & ~act[0][None]).any(axis=(0, 2))
    seen = np.maximum.accumulate(act, axis=0)
    dropped = (seen[:-1] & ~act[1:] & live[1:, :, None]).any(axis=(0, 2))
    return added, dropped


def iteration_change(iters, live):
    """[B] bool: the iteration count of a tick changes by 3 or more between the first tick and a later one within the compared ticks (the last
    compared tick included)"""
    d = np.abs(iters.astype(np.int64) - iters[0][None]) * live
    return d.max(axis=0) >= 3


@functools.lru_cache(maxsize=None)
def amplification(name):
    """max|q_k' - q_k| / 1e-9 at ticks 10, 100, 300 of the oracle's roll-out from q_0 + 1e-9 x N(0, 1) on the joint coordinates (recorded, not
    bounded: DESIGN.md §3.46), and the largest |qdot' - qdot| of the last tick"""
    p, r = problem(name), oracle_run(name)
    q0 = p["d"]["q"].copy()
    q0[:, 7:] += 1e-9 * np.random.default_rng(3).normal(0, 1, q0[:, 7:].shape) * (np.abs(q0[:, 7:]) > 0)
    e0 = np.abs(q0 - p["d"]["q"]).max()
    r2 = closed_loop(p, q0)
    both = (compared(r["status"]) & compared(r2["status"]))
    out = []
    for k in AMPLIFICATION_TICKS:
        k = min(k, p["K"])
        ok = both[k - 1]
        out.append(float(np.abs(r2["q"][k] - r["q"][k])[ok].max() / e0) if ok.any() else float("nan"))
    ok = both[-1]
    return tuple(out), float(np.abs(r2["qdot"][-1] - r["qdot"][-1])[ok].max()) if ok.any() else float("nan")


# ---- device-side reductions over many ticks: two tracks, every score and all four watch families (item 4 of DESIGN.md §3.46)
TRACK_CASES = ("c3", "everything")
TRACK_DU = (1 / 40, 1 / 55, 1 / 70)
TRACK_RADIUS = 0.03
GROUP = 4
SCORE = (common.GRIP, "trunk")
TIE = 1e-12                # two values closer than this may be ordered either way by two correct roundings: such instances are left out
FAMILIES = ("com", "trunk_z", "trunk_ang", "joint")


def _in_ball(rng, shape, radius):
    v = rng.normal(size=shape)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return v * (radius * rng.uniform(0.2, 1.0, shape[:-1] + (1,)) ** (1 / 3))


@functools.lru_cache(maxsize=None)
def tracks_problem(name):
    """the case's inputs with the gripper on a LINEAR track of S = 7 milestones and the trunk on a HERMITE track of S = 5 with tangents of
    its own, every milestone within 3 cm of the start, du per instance out of {1/40, 1/55, 1/70}; no IMU fed back (the trunk angles move)"""
    p = dict(problem(name))
    B = p["B"]
    rng = np.random.default_rng(23)
    d = {k: np.array(v, copy=True) for k, v in p["d"].items()}
    pos = common.track_frames(p["models"], d["q"], p["mid"])
    gp = pos[:, None, common.GRIP] + _in_ball(rng, (B, 7, 3), TRACK_RADIUS)
    gp[:, 0] = pos[:, common.GRIP]
    tp = d["trunk_target"][:, None, :] + _in_ball(rng, (B, 5, 3), TRACK_RADIUS)
    tp[:, 0] = d["trunk_target"]
    grip = dict(target=common.GRIP, points=gp, kind="linear", n_points=np.full(B, 7, np.int32), du=rng.choice(TRACK_DU, B))
    trunk = dict(target="trunk", points=tp, kind="hermite", tangents=rng.normal(0, 0.01, (B, 5, 3)), n_points=np.full(B, 5, np.int32),
                 du=rng.choice(TRACK_DU, B))
    tracks = [grip, trunk]
    common.start_previous_targets(d, tracks)
    _freeze(d, grip, trunk)
    p.update(d=d, tracks=tracks, imu=None, step=None)
    return p


def follow(p, d, k):
    """d with the followed targets of tick k"""
    n = dict(d)
    n["ee_target"] = np.array(d["ee_target"], copy=True)
    for t in p["tracks"]:
        if common.track_index(t["target"]) == common.TRUNK:
            n["trunk_target"] = common.track_at(t, k)
        else:
            n["ee_target"][:, common.track_index(t["target"])] = common.track_at(t, k)
    return n


def track_targets_all(p, ticks):
    """targets [ticks, 6, B, 3] of every tick (rows 0..4 the end effectors, 5 the trunk): followed rows from wbc_workload.track_targets, the
    others constant"""
    B = p["B"]
    out = np.zeros((ticks, 6, B, 3))
    for k in range(ticks):
        n = follow(p, p["d"], k)
        out[k, :5] = np.swapaxes(n["ee_target"], 0, 1)
        out[k, 5] = n["trunk_target"]
    return out


def segment_passes(p, ticks):
    """per track: (milestones passed within `ticks` ticks [B], the track's end reached and held [B])"""
    out = []
    for t in p["tracks"]:
        tmax = (ticks - 1) * np.asarray(t["du"])
        out.append((np.minimum(np.floor(tmax), t["n_points"] - 1).astype(int), tmax >= t["n_points"] - 1))
    return out


def slack_at(p, q):
    """slack_common.reference_slack at q [n, B, 27] -> trace [n, 4, B], which [n, 4, B], gap [n, 4, B] (between the two smallest components)"""
    import slack_common
    n, B = q.shape[:2]
    mid = None if p["mid"] is None else np.tile(p["mid"], n)
    r = slack_common.reference_slack(p["models"], p["cfgs"], q.reshape(n * B, 27), np.tile(p["d"]["trunk_box_center"], (n, 1)), mid)
    f = lambda a: np.swapaxes(a.reshape(n, B, 4), 1, 2)      # noqa: E731
    return f(r["slack"]), f(r["which"]), f(r["gap"])


@functools.lru_cache(maxsize=None)
def tracks_oracle_run(name):
    """the oracle's own closed loop along the tracks: q [K + 1, B, 27], status [K, B], slack trace [K, 4, B] of the state after every tick"""
    p = tracks_problem(name)
    B, n, cfg = p["B"], p["K"], p["cfgs"][0]
    d = {k: np.array(v, copy=True) for k, v in p["d"].items()}
    q, status = np.zeros((n + 1, B, 27)), np.zeros((n, B), np.int32)
    for k in range(n):
        q[k] = d["q"]
        d = follow(p, d, k)
        o = oracle_tick(p, d)
        status[k] = o["status"]
        d = sc.advance(cfg, d, oracle.update_state(p["models"], d["q"], o["q_next"], d["ee_target"], None, p["mid"]), None)
    q[n] = d["q"]
    trace, _, _ = slack_at(p, q[1:])
    r = dict(q=q, status=status, trace=trace)
    _freeze(r)
    return r


def crossings(trace, live=None):
    """per family and instance: ticks outside [4, B], and how often the instance goes from inside to outside [4, B]"""
    neg = trace < 0
    if live is not None:
        neg = neg & live[:, None, :]
    out = neg.sum(axis=0)
    leaves = (neg[1:] & ~neg[:-1]).sum(axis=0) + neg[0]
    return out, leaves
