"""Roll-outs along per-instance milestone trajectories, scored on the device (wbc_rollout_traj).

Every expected value comes from the CPU oracle: oracle.rollout(..., ee_target_at=...) fed with wbc_workload.traj_targets (itself held to
klampt's Trajectory.eval in test_rollout_traj_host.py), or the same loop restated here with the per-tick status kept. Tolerances are
test_gpu_parity.test_rollout_parity's: status exact, q 1e-6, qdot 10 x 1e-5, grip_trace TAU = 1e-6, ee_target 1e-15, iterations 2 per tick."""
import ctypes as C
import functools

import numpy as np
import pytest

import common
import oracle
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch
from wbc_workload import traj_targets

pytestmark = pytest.mark.gpu

DT = 0.002
QDOT_TOL = 1e-5
TAU = 1e-6           # grip_trace tolerance of test_rollout_parity
GRIP = 4
SUMMARY = ("err_sq_sum", "err_max", "err_max_tick", "err_final", "first_bad_tick", "bad_ticks")
GROUPS = ("group_rms", "group_err_max", "group_worst_status", "group_bad_instances")


@functools.lru_cache(maxsize=None)
def _model(name):
    return wbc_model.load_model(name)


def _grip_pos(models, q, mid):
    return oracle.fk(models, q, mid, want_com=False)["oMf"][:, capi.FR_EE0 + GRIP, 9:].copy()


def _trajectories(start, seed, S=4, sigma=0.01):
    """per instance: 2..S milestones, the first its own gripper position, the others within a few centimetres of it; a speed out of three"""
    rng = np.random.default_rng(seed)
    B = len(start)
    points = start[:, None, :] + rng.normal(0, sigma, (B, S, 3))
    points[:, 0] = start
    n = rng.choice([2, 3, 4], B).astype(np.int32)
    du = rng.choice([1 / 8, 1 / 5, 0.3], B)
    return points, n, du


def _inputs(names, cfg_name, B, seed, stress):
    models = [_model(n) for n in names]
    cfgs = [common.config(cfg_name, m) for m in models]
    mid = None
    parts = [common.tick_inputs(m, c, B, seed=seed + i, stress=stress) for i, (m, c) in enumerate(zip(models, cfgs))]
    d = {k: v.copy() for k, v in parts[0].items()}
    if len(models) > 1:
        mid = (np.arange(B) % len(models)).astype(np.int32)
        for i in range(1, len(parts)):
            for k in d:
                d[k][mid == i] = parts[i][k][mid == i]
        d["model_id"] = mid
    return models, cfgs, d, mid


def _target_at(d, points, n, du, ee=GRIP):
    base = d["ee_target"].copy()

    def at(k):
        t = base.copy()
        t[:, ee] = traj_targets(points, n, du, k)
        return t
    return at


def _per_instance(models, cfgs, mid, rows):
    """the oracle's form of per-instance task rows: B (model, configuration) pairs, model_id = arange(B)"""
    off = capi.WbcConfig.ee_W.offset
    ms, cs = [], []
    for b in range(len(rows)):
        i = 0 if mid is None else int(mid[b])
        c = capi.WbcConfig.from_buffer_copy(cfgs[i])
        C.memmove(C.addressof(c) + off, rows[b].ctypes.data, 85 * 8)
        ms.append(models[i])
        cs.append(c)
    return ms, cs, np.arange(len(rows), dtype=np.int32)


def _task_rows(cfg, B, seed):
    """gains and weights within a factor of two of the preset's (as test_rollout_with_rows_matches_the_oracle)"""
    rng = np.random.default_rng(seed)
    rows = wbc_model.task_params(cfg, B)
    sl = wbc_model.TASK_PARAMS_SLICES
    for f in ("ee_W", "ee_w", "ee_gain", "joint_w"):
        rows[:, sl[f]] *= np.exp(rng.uniform(np.log(0.5), np.log(2.0), (B, sl[f].stop - sl[f].start)))
    return rows


# problem -> (models, configuration, B, ticks, input seed, trajectory seed, stress recipe, running)
PROBLEMS = {
    "c3": (("a1_wx200",), "c3", 61, 24, 37, 5, False, True),          # ragged: 61 is no multiple of the four-instance packing
    "c3_tp": (("a1_wx200",), "c3", 61, 24, 37, 5, False, True),
    "mixed": (("a1_wx200", "laikago_vx300"), "c3", 32, 24, 43, 6, False, True),
    "warmup": (("a1_wx200",), "full", 61, 24, 47, 7, False, False),
    "stress": (("a1_wx200",), "c3", 64, 24, 37, 8, True, True),        # some trunks at / outside their box: non-optimal ticks
}


@functools.lru_cache(maxsize=None)
def _problem(name):
    names, cfg_name, B, K, seed, tseed, stress, running = PROBLEMS[name]
    models, cfgs, d, mid = _inputs(list(names), cfg_name, B, seed, stress)
    points, n, du = _trajectories(_grip_pos(models, d["q"], mid), tseed)
    d["prev_ee_target"][:, GRIP] = points[:, 0]       # (ee_target's gripper row keeps the generator's noise: the call must not read it)
    imu = d["q"][:, 3:7].copy() if running else None
    rows = _task_rows(cfgs[0], B, 9) if name == "c3_tp" else None
    return dict(models=models, cfgs=cfgs, d=d, mid=mid, points=points, n=n, du=du, B=B, K=K, imu=imu, running=running, rows=rows)


def _oracle_form(p):
    """(models, cfgs, inputs) the oracle takes for problem p: per-instance task rows become per-instance configurations"""
    if p["rows"] is None:
        return p["models"], p["cfgs"], p["d"]
    ms, cs, pid = _per_instance(p["models"], p["cfgs"], p["mid"], p["rows"])
    return ms, cs, dict(p["d"], model_id=pid)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """oracle.rollout along the trajectories (computed once per problem, never modified)"""
    p = _problem(name)
    ms, cs, d = _oracle_form(p)
    ref = oracle.rollout(ms, cs, d, DT, p["B"], p["K"], imu=p["imu"], nthreads=8, running=p["running"],
                         ee_target_at=_target_at(p["d"], p["points"], p["n"], p["du"]))
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _oracle_ticks(name):
    """oracle.rollout's loop restated with the per-tick status kept: -> (status [K, B], grip_trace [K, B, 3])"""
    p = _problem(name)
    models, cfgs, B, K = p["models"], p["cfgs"], p["B"], p["K"]
    assert not cfgs[0].task_trunk and "ee_ref_rot" not in p["d"]     # (no trunk / orientation reference state to carry in this restatement)
    at = _target_at(p["d"], p["points"], p["n"], p["du"])
    d = {k: np.array(v, copy=True) for k, v in p["d"].items()}
    status = np.zeros((K, B), np.int32)
    trace = np.zeros((K, B, 3))
    for k in range(K):
        d["ee_target"] = at(k)
        out = oracle.tick(models, cfgs, d, DT, B, nthreads=8, want_q_next=True)
        status[k] = out["status"]
        d["q"] = oracle.update_state(models, d["q"], out["q_next"], d["ee_target"], p["imu"], p["mid"])
        trace[k] = _grip_pos(models, d["q"], p["mid"])
        for e in range(capi.NEE):
            if cfgs[0].task_ee[e]:
                d["prev_ee_target"][:, e] = d["ee_target"][:, e]
    status.setflags(write=False)
    trace.setflags(write=False)
    return status, trace


def _handle(p, options=None, max_batch=None):
    bt = WbcBatch(p["models"], max_batch or p["B"])
    for i, c in enumerate(p["cfgs"]):
        bt.configure(c, i)
    for k, v in (options or {}).items():
        bt.set_option(k, v)
    return bt


def _run(bt, p, **kw):
    args = dict(points=p["points"], n_points=p["n"], du=p["du"], imu=p["imu"], task_params=p["rows"],
                mode=capi.ROLLOUT_RUNNING if p["running"] else capi.ROLLOUT_WARMUP, want_trace=True)
    args.update(kw)
    return bt.rollout_traj(p["d"], DT, p["K"], **args)


def _check_parity(got, p, ref, cold):
    K, B = p["K"], p["B"]
    ok = ref["status"] == 0
    assert ok.mean() >= 0.9                                        # the oracle alone solves the trajectories (every tick: status is the worst)
    t = (K - 1) * p["du"]                                          # the last tick's parameter
    assert (t > p["n"] - 1).any() and (t < p["n"] - 1).any()       # some instances run past their last milestone, some are still under way
    assert (p["du"] == 0.3).any()                                  # ... and some cross knots between ticks
    assert (got["status"] == ref["status"]).all()
    e_q = np.abs(got["q"] - ref["q"])[ok].max()
    e_v = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    e_t = np.abs(got["grip_trace"] - ref["grip_trace"])[:, ok].max()
    final = p["d"]["ee_target"].copy()
    final[:, GRIP] = traj_targets(p["points"], p["n"], p["du"], K)
    e_f = np.abs(got["ee_target"] - final).max()
    print("q %.3e  qdot %.3e  grip_trace %.3e  ee_target_final %.3e  optimal %d/%d" % (e_q, e_v, e_t, e_f, int(ok.sum()), B))
    assert e_q < 1e-6 and e_v < 10 * QDOT_TOL and e_t < TAU and e_f < 1e-15
    if cold:
        assert np.abs(got["iters"][ok] - ref["iters"][ok]).max() <= 2 * K


# ------------------------------------------------------------------------------------------------ 1. parity with the oracle
CASES = {   # case -> (problem, options, expected (last_path, last_update_packed) or None)
    "packed": ("c3", {}, (2, 1)),
    "unpacked": ("c3", {"packed_kernel": 0}, None),
    "warm": ("c3", {"warm_start": 1}, (2, 1)),
    "task_params": ("c3_tp", {}, (2, 1)),
    "mixed_laikago": ("mixed", {}, None),
    "warmup_mode": ("warmup", {}, None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_oracle(case):
    name, options, paths = CASES[case]
    p, ref = _problem(name), _reference(name)
    before = {k: v.copy() for k, v in p["d"].items()}
    bt = _handle(p, options)
    got = _run(bt, p)
    if paths:
        assert (bt.stat("last_path"), bt.stat("last_update_packed")) == paths
    if case == "unpacked":
        assert bt.stat("last_path") != 2
    assert bt.stat("last_traj_bad_rows") == 0
    assert all((p["d"][k] == before[k]).all() for k in before)     # in0 is only read
    _check_parity(got, p, ref, cold=case != "warm")
    if p["imu"] is not None:
        assert (got["q"][:, 3:7] == p["imu"]).all()
    bt.close()


# ------------------------------------------------------------------------------------------------ 2. one segment is the existing roll-out
def test_one_segment_is_the_existing_rollout():
    p = _problem("c3")
    B, K = p["B"], 16
    p0, p1 = p["points"][:, 0], p["points"][:, 1]
    d = {k: v.copy() for k, v in p["d"].items()}
    d["ee_target"][:, GRIP] = p0
    step = np.zeros((B, 5, 3))
    step[:, GRIP] = (p1 - p0) / K
    bt = _handle(p)
    old = bt.rollout(d, DT, K, ee_target_step=step, imu=p["imu"])
    new = bt.rollout_traj(d, DT, K, points=np.stack([p0, p1], axis=1), du=1.0 / K, imu=p["imu"], want_trace=True)
    assert (new["status"] == old["status"]).all() and (new["iters"] == old["iters"]).all()
    e_q = np.abs(new["q"] - old["q"]).max()
    e_f = np.abs(new["ee_target"] - old["ee_target"]).max()
    print("one segment against wbc_rollout: q %.3e, final target %.3e" % (e_q, e_f))
    assert e_q < 1e-6                                             # the targets differ by rounding only (K additions against one product)
    assert e_f < 1e-14 and np.abs(new["grip_trace"] - old["grip_trace"]).max() < TAU
    bt.close()


# ------------------------------------------------------------------------------------------------ 3. summaries
def _numpy_summary(trace, targets, status):
    """the summary of a [K, B, 3] trace against [K, B, 3] targets and [K, B] statuses, summed in tick order"""
    K, B = status.shape
    d = trace - targets
    e2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    err = np.sqrt(e2)
    ssum = np.zeros(B)
    for k in range(K):
        ssum = ssum + e2[k]
    bad = status != 0
    return dict(err_sq_sum=ssum, err_max=err.max(axis=0), err_max_tick=err.argmax(axis=0).astype(np.int32), err_final=err[-1],
                first_bad_tick=np.where(bad.any(axis=0), bad.argmax(axis=0), -1).astype(np.int32), bad_ticks=bad.sum(axis=0).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _stress_runs():
    """the stress problem with trace + summary, and with the summary alone"""
    p = _problem("stress")
    bt = _handle(p)
    both = _run(bt, p)
    alone = _run(bt, p, want_trace=False)
    bt.close()
    return both, alone


def _targets(p):
    return np.stack([traj_targets(p["points"], p["n"], p["du"], k) for k in range(p["K"])])


def test_summary_is_the_reduction_of_the_calls_own_trace():
    p = _problem("stress")
    K = p["K"]
    status, _ = _oracle_ticks("stress")
    got, _ = _stress_runs()
    want = _numpy_summary(got["grip_trace"], _targets(p), status)
    ulp = np.finfo(float).eps
    for k in ("err_sq_sum", "err_max", "err_final"):
        rel = np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), 1e-300)
        print("%s: worst relative difference %.2e" % (k, rel.max()))
        assert rel.max() <= 4 * K * ulp, k                         # (the kernel sums over k in order, as the loop above)
    for k in ("err_max_tick", "first_bad_tick", "bad_ticks"):
        assert (got[k] == want[k]).all(), k


def test_summary_against_the_oracle():
    p = _problem("stress")
    K = p["K"]
    status, trace = _oracle_ticks("stress")
    want = _numpy_summary(trace, _targets(p), status)
    assert (want["bad_ticks"] > 0).any() and (want["bad_ticks"] == 0).any()     # by the oracle: some instances with a non-optimal tick, some without
    got, _ = _stress_runs()
    assert (got["first_bad_tick"] == want["first_bad_tick"]).all() and (got["bad_ticks"] == want["bad_ticks"]).all()
    assert (got["status"] == status.max(axis=0)).all()
    ok = want["bad_ticks"] == 0                                                 # (TAU holds where every tick was solved, as in test 1)
    e_max = np.abs(got["err_max"] - want["err_max"])[ok].max()
    bound = 2 * K * want["err_max"] * TAU + K * TAU ** 2                        # |sum (e + d)^2 - sum e^2| <= 2 K e_max tau + K tau^2 for |d| <= tau
    e_sum = (np.abs(got["err_sq_sum"] - want["err_sq_sum"]) / bound)[ok].max()
    print("against the oracle: err_max differs by %.3e (tau %.0e), err_sq_sum by %.3e of its bound; %d of %d instances with a bad tick" % (
        e_max, TAU, e_sum, int((~ok).sum()), p["B"]))
    assert e_max <= TAU and e_sum <= 1.0
    assert np.abs(got["err_final"] - want["err_final"])[ok].max() <= TAU


def test_summary_without_the_trace_is_the_same_bits():
    both, alone = _stress_runs()
    assert "grip_trace" not in alone
    for k in SUMMARY + ("q", "qdot", "status", "iters", "ee_target"):
        assert both[k].tobytes() == alone[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 4. groups
@functools.lru_cache(maxsize=None)
def _group_problem():
    m = _model("a1_wx200")
    cfg = common.config("c3", m)
    B = 130
    d = common.tick_inputs(m, cfg, B, seed=53)
    points, n, du = _trajectories(_grip_pos([m], d["q"], None), 12)
    return dict(models=[m], cfgs=[cfg], d=d, points=points, n=n, du=du, B=B)


@pytest.mark.parametrize("M,B", [(16, 64), (5, 60), (130, 130)])    # 5: less than a wave, no power of two; 130: more than 64 lanes (the stride loop)
def test_group_summaries(M, B):
    g = _group_problem()
    K = 6
    d = {k: v[:B] for k, v in g["d"].items()}
    bt = _handle(g, max_batch=130)
    runs = [bt.rollout_traj(d, DT, K, points=g["points"][:B], n_points=g["n"][:B], du=g["du"][:B], group_size=M) for _ in range(2)]
    bt.close()
    got = runs[0]
    G = B // M
    assert all(got[k].shape == (G,) for k in GROUPS)
    rms = np.sqrt(got["err_sq_sum"].reshape(G, M).sum(axis=1) / (M * K))
    assert np.abs(got["group_rms"] - rms).max() <= 1e-12 * rms.max()
    assert (got["group_err_max"] == got["err_max"].reshape(G, M).max(axis=1)).all()
    assert (got["group_worst_status"] == got["status"].reshape(G, M).max(axis=1)).all()
    assert (got["group_bad_instances"] == (got["bad_ticks"].reshape(G, M) > 0).sum(axis=1)).all()
    assert got["err_sq_sum"].min() > 0
    for k in got:                                                   # two identical calls: identical bits
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 5. bad rows
@pytest.mark.parametrize("what", ["nan_point", "du_zero", "one_point"])
def test_bad_rows_fail_alone(what):
    g = _group_problem()
    B, K = 8, 6
    d = {k: v[:B] for k, v in g["d"].items()}
    points, n, du = g["points"][:B].copy(), g["n"][:B].copy(), g["du"][:B].copy()
    n[1] = 3
    for b in range(B):
        points[b, n[b]:] = np.nan                                   # beyond an instance's own milestones: never read, no bad row
    bt = _handle(g, max_batch=B)
    clean = bt.rollout_traj(d, DT, K, points=points, n_points=n, du=du, want_trace=True, group_size=4)
    assert bt.stat("last_traj_bad_rows") == 0 and np.isfinite(clean["q"]).all()
    if what == "nan_point":
        points[1, 2, 1] = np.nan
    elif what == "du_zero":
        du[1] = 0.0
    else:
        n[1] = 1
    got = bt.rollout_traj(d, DT, K, points=points, n_points=n, du=du, want_trace=True, group_size=4)
    assert bt.stat("last_traj_bad_rows") == 1
    assert got["status"][1] == capi.QP_NUMERICAL and got["first_bad_tick"][1] == 0 and got["bad_ticks"][1] == K
    assert (got["ee_target"][1] == d["ee_target"][1]).all()         # its target stayed where in0 put it
    assert np.isfinite(got["q"]).all() and np.isfinite(got["grip_trace"]).all()
    assert got["group_worst_status"][0] == capi.QP_NUMERICAL and got["group_bad_instances"][0] >= 1
    others = np.arange(B) != 1
    for k in SUMMARY + ("q", "qdot", "status", "iters", "ee_target"):
        assert got[k][others].tobytes() == clean[k][others].tobytes(), k
    assert got["grip_trace"][:, others].tobytes() == clean["grip_trace"][:, others].tobytes()
    for k in GROUPS:
        assert got[k][1:].tobytes() == clean[k][1:].tobytes(), k
    bt.close()


# ------------------------------------------------------------------------------------------------ 6. misuse
def _raw_call(bt, d, B, K, points, tweak):
    """wbc_rollout_traj through ctypes with well-formed host arrays, then `tweak(r, t, s)` -> (return code, wbc_last_error())"""
    keep = []
    f = np.float64
    out_q, out_st = np.zeros((B, 27)), np.zeros(B, np.int32)
    sq = np.zeros(B)
    zeros15 = np.zeros((B, 15))
    r, t, s = capi.WbcRollout(), capi.WbcTrajectory(), capi.WbcRolloutSummary()
    r.ticks, r.mode = K, capi.ROLLOUT_RUNNING
    r.q_final, r.status_max = bt._p(out_q, f, keep), bt._p(out_st, np.int32, keep)
    t.max_points, t.ee_index, t.du_all = points.shape[1], GRIP, 0.002
    t.points = bt._p(points, f, keep)
    s.err_sq_sum = bt._p(sq, f, keep)
    tweak(r, t, s, bt._p(zeros15, f, keep))
    tin = bt._tick_in(d, keep, B)
    rc = bt.lib.wbc_rollout_traj(bt._h, B, C.byref(tin), None, DT, C.byref(r), C.byref(t), C.byref(s), capi.MEM_HOST, None)
    return rc, (bt.lib.wbc_last_error() or b"").decode()


def test_misuse_is_refused_with_the_fields_name():
    g = _group_problem()
    B, K = 8, 3
    d = {k: v[:B] for k, v in g["d"].items()}
    points = g["points"][:B].copy()
    bt = _handle(g, max_batch=B)

    def setter(struct, field, value):
        def tweak(r, t, s, spare):
            setattr({"r": r, "t": t, "s": s}[struct], field, spare if value == "ptr" else value)
        return tweak
    refused = [("r", "ee_target_step", "ptr", "ee_target_step"), ("r", "hold_ticks", 1, "hold_ticks"),
               ("t", "max_points", 1, "max_points"), ("t", "max_points", capi.MAX_TRAJ_POINTS + 1, "max_points"),
               ("t", "ee_index", 5, "ee_index"), ("t", "ee_index", -1, "ee_index"), ("t", "points", None, "points"),
               ("t", "du_all", 0.0, "du_all"), ("t", "du_all", float("nan"), "du_all"), ("t", "du_all", float("inf"), "du_all"),
               ("t", "du_all", -0.002, "du_all"), ("s", "group_size", 3, "group_size")]
    for struct, field, value, word in refused:
        rc, msg = _raw_call(bt, d, B, K, points, setter(struct, field, value))
        assert rc == -1 and word in msg, (field, value, rc, msg)       # WBC_E_ARG
    rc, msg = _raw_call(bt, d, B, K, points, lambda r, t, s, spare: None)
    assert rc == 0, msg
    rc, msg = _raw_call(bt, d, B, K, points, setter("s", "group_size", 4))
    assert rc == 0, msg
    bt.close()


# ------------------------------------------------------------------------------------------------ 7. device pointers
def test_device_tensors_give_the_host_calls_bits():
    import torch
    p = _problem("c3")
    bt = _handle(p)
    host = _run(bt, p, group_size=0)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d = {k: dev(v) for k, v in p["d"].items()}
    got = bt.rollout_traj(d, DT, p["K"], points=dev(p["points"]), n_points=dev(p["n"]), du=dev(p["du"]), imu=dev(p["imu"]), want_trace=True)
    torch.cuda.synchronize()
    assert set(got) == set(host)
    for k in host:
        assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    _check_parity({k: v.cpu().numpy() for k, v in got.items()}, p, _reference("c3"), cold=True)
    bt.close()
