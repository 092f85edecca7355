"""Roll-outs with trunk and multi-target tracks, linear or Hermite spline, any frame scored (wbc_rollout_tracks).

Every expected value comes from the CPU oracle: oracle.rollout's loop (oracle.py, with the trunk side effects) restated here with an
ee_target_at(k) and a trunk_target_at(k) hook, the per-tick status and the positions of all six frames kept — built from oracle.tick,
oracle.update_state and oracle.fk, fed with wbc_workload.track_targets (itself held to the scalar Hermite trajectory in
test_rollout_tracks_host.py). Tolerances are test_gpu_parity.test_rollout_parity's: status exact, q 1e-6, qdot 1e-4, traces 1e-6, final
targets 1e-15 against the host restatement, iterations 2 per tick on cold runs."""
import ctypes as C
import functools

import numpy as np
import pytest

import common
import oracle
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch
from wbc_workload import spline_tangents, track_targets

pytestmark = pytest.mark.gpu

DT = 0.002
TAU = 1e-6           # trace tolerance of test_rollout_parity
GRIP, TRUNK = 4, capi.TARGET_TRUNK
FRAME_SCORES = ("err_sq_sum", "err_max", "err_final", "err_max_tick")
SCORES = FRAME_SCORES + ("first_bad_tick", "bad_ticks")
GROUPS = ("group_rms", "group_err_max", "group_worst_status", "group_bad_instances")
COMMON = ("q", "qdot", "status", "iters", "ee_target")


@functools.lru_cache(maxsize=None)
def _model(name):
    return wbc_model.load_model(name)


# the track recipe, the oracle loop and the scores' numpy restatement live in tests/common.py (test_gpu_device_inplace.py runs them too)
_frames, _base_tracks, _index, _at = common.track_frames, common.base_tracks, common.track_index, common.track_at
_start_previous_targets, _per_instance, _numpy_scores = common.start_previous_targets, common.per_instance_configs, common.numpy_scores


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


def _six_linear_tracks(d, pos, seed):
    """all six targets on LINEAR tracks from where the frames are"""
    rng = np.random.default_rng(seed)
    B = len(pos)
    tracks = []
    for f in range(6):
        start = d["trunk_target"] if f == TRUNK else pos[:, f]
        p = start[:, None, :] + rng.normal(0, 0.01 if f >= GRIP else 0.003, (B, 4, 3))
        p[:, 0] = start
        tracks.append(dict(target="trunk" if f == TRUNK else f, points=p, kind="linear", n_points=rng.choice([2, 3, 4], B).astype(np.int32),
                           du=rng.choice([1 / 8, 1 / 5, 0.3], B)))
    return tracks


def _task_rows(cfg, B, seed):
    """gains and weights within a factor of two of the preset's (as test_rollout_with_rows_matches_the_oracle)"""
    rng = np.random.default_rng(seed)
    rows = wbc_model.task_params(cfg, B)
    sl = wbc_model.TASK_PARAMS_SLICES
    for f in ("ee_W", "ee_w", "ee_gain", "trunk_W", "trunk_w", "trunk_gain", "joint_w"):
        rows[:, sl[f]] *= np.exp(rng.uniform(np.log(0.5), np.log(2.0), (B, sl[f].stop - sl[f].start)))
    return rows


# problem -> (models, configuration, B, ticks, input seed, track seed, stress recipe, running, tracks)
PROBLEMS = {
    "base": (("a1_wx200",), "c3_trunk_task", 61, 24, 37, 5, False, True, "base"),      # ragged: 61 is no multiple of the four-instance packing
    "base_tp": (("a1_wx200",), "c3_trunk_task", 61, 24, 37, 5, False, True, "base"),
    "half": (("a1_wx200",), "c3_trunk_task", 61, 24, 37, 5, False, True, "half"),      # the base recipe with the default tangents halved, passed by the caller
    "mixed": (("a1_wx200", "laikago_vx300"), "c3_trunk_task", 32, 24, 43, 6, False, True, "base"),
    "six": (("a1_wx200",), "full", 61, 24, 47, 7, False, False, "six"),                # WARMUP mode, n_tracks = 6
    "chicken": (("a1_wx200",), "c3_trunk_task", 64, 24, 37, 5, True, True, "trunk"),   # stress recipe: non-optimal ticks; the trunk alone is followed
}


@functools.lru_cache(maxsize=None)
def _problem(name):
    names, cfg_name, B, K, seed, tseed, stress, running, kind = PROBLEMS[name]
    models, cfgs, d, mid = _inputs(list(names), cfg_name, B, seed, stress)
    pos = _frames(models, d["q"], mid)
    if kind == "six":
        tracks = _six_linear_tracks(d, pos, tseed)
    else:
        tracks = _base_tracks(d, pos[:, GRIP], tseed)
        if kind == "half":
            tracks[0]["tangents"] = 0.5 * spline_tangents(tracks[0]["points"], tracks[0]["n_points"])
        if kind == "trunk":
            tracks = tracks[:1]
    _start_previous_targets(d, tracks)
    imu = d["q"][:, 3:7].copy() if running else None
    rows = _task_rows(cfgs[0], B, 9) if name == "base_tp" else None
    return dict(models=models, cfgs=cfgs, d=d, mid=mid, tracks=tracks, B=B, K=K, imu=imu, running=running, rows=rows)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """common.tracks_reference of the named problem. Computed once, never modified."""
    return common.tracks_reference(_problem(name))


def _handle(p, options=None, max_batch=None):
    bt = WbcBatch(p["models"], max_batch or p["B"])
    for i, c in enumerate(p["cfgs"]):
        bt.configure(c, i)
    for k, v in (options or {}).items():
        bt.set_option(k, v)
    return bt


def _run(bt, p, **kw):
    args = dict(score=("trunk", GRIP), imu=p["imu"], task_params=p["rows"],
                mode=capi.ROLLOUT_RUNNING if p["running"] else capi.ROLLOUT_WARMUP, want_trace=True)
    args.update(kw)
    tracks = args.pop("tracks", p["tracks"])
    return bt.rollout_tracks(p["d"], DT, p["K"], tracks, **args)


def _check_parity(got, p, ref, cold, scored=(GRIP, TRUNK)):
    K, B = p["K"], p["B"]
    ok = ref["status"] == 0
    assert ok.mean() >= 0.9                                        # the oracle alone solves the tracks (every tick: status is the worst)
    for t in p["tracks"]:
        last = (K - 1) * t["du"]                                   # the last tick's parameter
        assert (last > t["n_points"] - 1).any() and (last < t["n_points"] - 1).any()   # some past their last milestone, some under way
        assert (t["du"] == 0.3).any()                              # ... and some cross knots between ticks
    assert (got["status"] == ref["status"]).all()
    e_q = np.abs(got["q"] - ref["q"])[ok].max()
    e_v = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    e_g = np.abs(got["grip_trace"] - ref["frames"][:, :, GRIP])[:, ok].max()
    e_t = max(np.abs(got["trace"][:, j] - ref["frames"][:, :, f])[:, ok].max() for j, f in enumerate(sorted(scored)))
    e_f = max(np.abs(got["ee_target"] - ref["ee_target"]).max(), np.abs(got["trunk_target"] - ref["trunk_target"]).max())
    print("q %.3e  qdot %.3e  grip_trace %.3e  trace %.3e  final targets %.3e  optimal %d/%d" % (e_q, e_v, e_g, e_t, e_f, int(ok.sum()), B))
    assert e_q < 1e-6 and e_v < 1e-4 and e_g < TAU and e_t < TAU and e_f < 1e-15
    if cold:
        assert np.abs(got["iters"][ok] - ref["iters"][ok]).max() <= 2 * K


# ------------------------------------------------------------------------------------------------ 1. parity with the oracle
CASES = {   # case -> (problem, options, expected (last_path, last_update_packed) or None)
    "packed": ("base", {}, (2, 1)),
    "unpacked": ("base", {"packed_kernel": 0}, None),
    "warm": ("base", {"warm_start": 1}, (2, 1)),
    "task_params": ("base_tp", {}, (2, 1)),
    "mixed_laikago": ("mixed", {}, None),
    "six_tracks_warmup_mode": ("six", {}, None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_oracle(case):
    name, options, paths = CASES[case]
    p, ref = _problem(name), _reference(name)
    before = {k: v.copy() for k, v in p["d"].items()}
    bt = _handle(p, options)
    scored = tuple(range(6)) if name == "six" else (GRIP, TRUNK)
    got = _run(bt, p, score=tuple("trunk" if f == TRUNK else f for f in scored))
    if paths:
        assert (bt.stat("last_path"), bt.stat("last_update_packed")) == paths
    if case == "unpacked":
        assert bt.stat("last_path") != 2
    assert bt.stat("last_traj_bad_rows") == 0
    assert all((p["d"][k] == before[k]).all() for k in before)     # in0 is only read
    if name != "six":                                              # HERMITE is not LINEAR here: a kernel that ignored `kind` would fail
        t = p["tracks"][0]
        gap = max(np.abs(_at(t, k) - _at(dict(t, kind="linear"), k)).max() for k in range(p["K"]))
        v = spline_tangents(t["points"], t["n_points"])
        assert gap > 1e-3 and (np.abs(v) > 0).any(axis=(1, 2)).mean() > 0.8
    _check_parity(got, p, ref, cold=case != "warm", scored=scored)
    if p["imu"] is not None:
        assert (got["q"][:, 3:7] == p["imu"]).all()
    bt.close()


# ------------------------------------------------------------------------------------------------ 2. one LINEAR gripper track is wbc_rollout_traj
def test_one_linear_gripper_track_is_rollout_traj_bit_for_bit():
    p = _problem("base")
    g = p["tracks"][1]
    B, K, M = 60, 16, 5
    d = {k: v[:B] for k, v in p["d"].items()}
    bt = _handle(p)
    old = bt.rollout_traj(d, DT, K, points=g["points"][:B], n_points=g["n_points"][:B], du=g["du"][:B], ee_index=GRIP, group_size=M,
                          want_trace=True, imu=p["imu"][:B])
    new = bt.rollout_tracks(d, DT, K, [dict(target=GRIP, points=g["points"][:B], n_points=g["n_points"][:B], du=g["du"][:B])],
                            score=(GRIP,), group_size=M, want_trace=True, imu=p["imu"][:B])
    bt.close()
    for k in COMMON + ("grip_trace", "first_bad_tick", "bad_ticks", "group_worst_status", "group_bad_instances"):
        assert new[k].tobytes() == old[k].tobytes(), k
    for k in FRAME_SCORES:
        assert new[k].shape == (1, B) and new[k].tobytes() == old[k].tobytes(), k
    for k in ("group_rms", "group_err_max"):
        assert new[k].shape == (1, B // M) and new[k].tobytes() == old[k].tobytes(), k
    assert new["trace"][:, 0].tobytes() == old["grip_trace"].tobytes() and old["err_sq_sum"].min() > 0


# ------------------------------------------------------------------------------------------------ 3. caller tangents
def test_caller_tangents():
    p = _problem("base")
    bt = _handle(p)
    default = _run(bt, p)
    t = p["tracks"][0]
    given = _run(bt, p, tracks=[dict(t, tangents=spline_tangents(t["points"], t["n_points"])), p["tracks"][1]])
    assert set(given) == set(default)
    for k in default:                                               # the default rule passed by the caller: the bits of NULL
        assert given[k].tobytes() == default[k].tobytes(), k
    h = _problem("half")                                            # halved tangents: the oracle loop along THOSE targets
    got = _run(bt, h)
    bt.close()
    assert np.abs(got["trunk_target"] - default["trunk_target"]).max() > 1e-4 or np.abs(got["q"] - default["q"]).max() > 1e-6
    _check_parity(got, h, _reference("half"), cold=True)


# ------------------------------------------------------------------------------------------------ 4. chicken head: scores
@functools.lru_cache(maxsize=None)
def _chicken_runs():
    """the chicken-head problem (only the trunk followed; gripper and trunk scored) with trace + scores, and with the scores alone"""
    p = _problem("chicken")
    bt = _handle(p)
    both = _run(bt, p)
    alone = _run(bt, p, want_trace=False)
    bt.close()
    return both, alone


def _scored_targets(ref):
    return np.stack([ref["targets"][:, :, GRIP], ref["targets"][:, :, TRUNK]], axis=1)       # [K, 2, B, 3], frames in increasing order


def test_scores_are_the_reduction_of_the_calls_own_trace():
    p, ref = _problem("chicken"), _reference("chicken")
    K = p["K"]
    got, _ = _chicken_runs()
    assert (ref["targets"][:, :, GRIP] == p["d"]["ee_target"][:, GRIP]).all()                 # the gripper's target is constant
    want = _numpy_scores(got["trace"], _scored_targets(ref), ref["tick_status"])
    ulp = np.finfo(float).eps
    for k in ("err_sq_sum", "err_max", "err_final"):
        rel = np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), 1e-300)
        print("%s: worst relative difference %.2e" % (k, rel.max()))
        assert got[k].shape == (2, p["B"]) and rel.max() <= 4 * K * ulp, k        # (the kernel sums over k in order, as the loop above)
    for k in ("err_max_tick", "first_bad_tick", "bad_ticks"):
        assert (got[k] == want[k]).all(), k
    assert (got["trace"][:, 0] == got["grip_trace"]).all()


def test_scores_against_the_oracle():
    p, ref = _problem("chicken"), _reference("chicken")
    K = p["K"]
    trace = np.stack([ref["frames"][:, :, GRIP], ref["frames"][:, :, TRUNK]], axis=1)
    want = _numpy_scores(trace, _scored_targets(ref), ref["tick_status"])
    assert (want["bad_ticks"] > 0).any() and (want["bad_ticks"] == 0).any()     # by the oracle: some instances with a non-optimal tick, some without
    got, _ = _chicken_runs()
    assert (got["first_bad_tick"] == want["first_bad_tick"]).all() and (got["bad_ticks"] == want["bad_ticks"]).all()
    assert (got["status"] == ref["tick_status"].max(axis=0)).all()
    ok = want["bad_ticks"] == 0                                                 # (TAU holds where every tick was solved, as in test 1)
    e_max = np.abs(got["err_max"] - want["err_max"])[:, ok].max()
    bound = 2 * K * want["err_max"] * TAU + K * TAU ** 2                        # |sum (e + d)^2 - sum e^2| <= 2 K e_max tau + K tau^2 for |d| <= tau
    e_sum = (np.abs(got["err_sq_sum"] - want["err_sq_sum"]) / bound)[:, ok].max()
    print("against the oracle: err_max differs by %.3e (tau %.0e), err_sq_sum by %.3e of its bound; %d of %d instances with a bad tick" % (
        e_max, TAU, e_sum, int((~ok).sum()), p["B"]))
    assert e_max <= TAU and e_sum <= 1.0
    assert np.abs(got["err_final"] - want["err_final"])[:, ok].max() <= TAU
    final = _at(p["tracks"][0], K)
    assert np.abs(got["trunk_target"] - final).max() < 1e-15 and (got["ee_target"] == p["d"]["ee_target"]).all()


def test_scores_without_the_trace_are_the_same_bits():
    both, alone = _chicken_runs()
    assert "trace" not in alone and "grip_trace" not in alone
    for k in SCORES + COMMON + ("trunk_target",):
        assert both[k].tobytes() == alone[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 5. groups
@functools.lru_cache(maxsize=None)
def _group_problem():
    m = _model("a1_wx200")
    cfg = common.config("c3_trunk_task", m)
    B = 130
    d = common.tick_inputs(m, cfg, B, seed=53)
    tracks = _base_tracks(d, _frames([m], d["q"], None)[:, GRIP], 12)
    _start_previous_targets(d, tracks)
    return dict(models=[m], cfgs=[cfg], d=d, tracks=tracks, B=B)


def _cut(tracks, B):
    return [{k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in tracks]


@pytest.mark.parametrize("M,B", [(16, 64), (5, 60), (130, 130)])    # 5: less than a wave, no power of two; 130: more than 64 lanes (the stride loop)
def test_group_scores(M, B):
    g = _group_problem()
    K = 6
    d = {k: v[:B] for k, v in g["d"].items()}
    bt = _handle(g, max_batch=130)
    runs = [bt.rollout_tracks(d, DT, K, _cut(g["tracks"], B), score=("trunk", GRIP), group_size=M) for _ in range(2)]
    bt.close()
    got = runs[0]
    G = B // M
    assert all(got[k].shape == (2, G) for k in GROUPS[:2]) and all(got[k].shape == (G,) for k in GROUPS[2:])
    rms = np.sqrt(got["err_sq_sum"].reshape(2, G, M).sum(axis=2) / (M * K))
    assert np.abs(got["group_rms"] - rms).max() <= 1e-12 * rms.max()
    assert (got["group_err_max"] == got["err_max"].reshape(2, G, M).max(axis=2)).all()
    assert (got["group_worst_status"] == got["status"].reshape(G, M).max(axis=1)).all()
    assert (got["group_bad_instances"] == (got["bad_ticks"].reshape(G, M) > 0).sum(axis=1)).all()
    assert got["err_sq_sum"].min() > 0 and (got["group_rms"][0] != got["group_rms"][1]).all()
    for k in got:                                                   # two identical calls: identical bits
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 6. bad rows
@pytest.mark.parametrize("what", ["nan_tangent", "nan_trunk_point", "du_zero_on_one_track"])
def test_bad_rows_fail_alone(what):
    g = _group_problem()
    B, K = 8, 6
    d = {k: v[:B] for k, v in g["d"].items()}
    tracks = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in _cut(g["tracks"], B)]
    trunk, grip = tracks
    trunk["n_points"][1] = 3
    trunk["tangents"] = spline_tangents(trunk["points"], trunk["n_points"])
    for t in tracks:
        for b in range(B):
            t["points"][b, t["n_points"][b]:] = np.nan               # beyond an instance's own milestones: never read, no bad row
    for b in range(B):
        trunk["tangents"][b, trunk["n_points"][b]:] = np.nan
    bt = _handle(g, max_batch=B)
    kw = dict(score=("trunk", GRIP), want_trace=True, group_size=4)
    clean = bt.rollout_tracks(d, DT, K, tracks, **kw)
    assert bt.stat("last_traj_bad_rows") == 0 and np.isfinite(clean["q"]).all()
    if what == "nan_tangent":
        trunk["tangents"][1, 1, 2] = np.nan
    elif what == "nan_trunk_point":
        trunk["points"][1, 2, 1] = np.nan
    else:
        grip["du"][1] = 0.0
    got = bt.rollout_tracks(d, DT, K, tracks, **kw)
    assert bt.stat("last_traj_bad_rows") == 1
    assert got["status"][1] == capi.QP_NUMERICAL and got["first_bad_tick"][1] == 0 and got["bad_ticks"][1] == K
    assert (got["ee_target"][1] == d["ee_target"][1]).all() and (got["trunk_target"][1] == d["trunk_target"][1]).all()   # ALL its followed targets stayed
    assert np.isfinite(got["q"]).all() and np.isfinite(got["trace"]).all()
    assert got["group_worst_status"][0] == capi.QP_NUMERICAL and got["group_bad_instances"][0] >= 1
    others = np.arange(B) != 1
    for k in COMMON + ("trunk_target", "first_bad_tick", "bad_ticks"):
        assert got[k][others].tobytes() == clean[k][others].tobytes(), k
    for k in FRAME_SCORES:
        assert got[k][:, others].tobytes() == clean[k][:, others].tobytes(), k
    assert got["trace"][:, :, others].tobytes() == clean["trace"][:, :, others].tobytes()
    for k in GROUPS[:2]:
        assert got[k][:, 1:].tobytes() == clean[k][:, 1:].tobytes(), k
    for k in GROUPS[2:]:
        assert got[k][1:].tobytes() == clean[k][1:].tobytes(), k
    bt.close()


# ------------------------------------------------------------------------------------------------ 7. misuse
def _raw_call(bt, d, B, K, points, tweak):
    """wbc_rollout_tracks through ctypes with well-formed host arrays (a trunk HERMITE and a gripper LINEAR track, both scored), then
    `tweak(r, t, s, tin, spare)` -> (return code, wbc_last_error())"""
    keep = []
    f = np.float64
    out_q, out_st = np.zeros((B, 27)), np.zeros(B, np.int32)
    sq = np.zeros((2, B))
    spare = np.zeros((B, points.shape[1] * 3))
    r, t, s = capi.WbcRollout(), capi.WbcTracks(), capi.WbcTrackScores()
    r.ticks, r.mode = K, capi.ROLLOUT_RUNNING
    r.q_final, r.status_max = bt._p(out_q, f, keep), bt._p(out_st, np.int32, keep)
    t.n_tracks = 2
    for j, (target, kind) in enumerate(((TRUNK, capi.TRACK_HERMITE), (GRIP, capi.TRACK_LINEAR))):
        c = t.track[j]
        c.target, c.kind, c.max_points, c.du_all = target, kind, points.shape[1], 0.002
        c.points = bt._p(points, f, keep)
    s.score_mask = (1 << TRUNK) | (1 << GRIP)
    s.err_sq_sum = bt._p(sq, f, keep)
    tin = bt._tick_in(d, keep, B)
    tweak(r, t, s, tin, bt._p(spare, f, keep))
    rc = bt.lib.wbc_rollout_tracks(bt._h, B, C.byref(tin), None, DT, C.byref(r), C.byref(t), C.byref(s), capi.MEM_HOST, None)
    return rc, (bt.lib.wbc_last_error() or b"").decode()


def test_misuse_is_refused_with_the_fields_name():
    g = _group_problem()
    B, K = 8, 3
    d = {k: v[:B] for k, v in g["d"].items()}
    points = g["tracks"][0]["points"][:B].copy()
    bt = _handle(g, max_batch=B)

    def on(what, field, value):
        def tweak(r, t, s, tin, spare):
            obj = {"r": r, "t": t, "s": s, "in": tin, "t0": t.track[0], "t1": t.track[1]}[what]
            setattr(obj, field, spare if value == "ptr" else value)
        return tweak

    def trunk_unfollowed(field, value):
        def tweak(r, t, s, tin, spare):
            t.n_tracks = 1
            t.track[0].target, t.track[0].kind = GRIP, capi.TRACK_LINEAR
            setattr(tin, field, value)
        return tweak
    refused = [(on("r", "ee_target_step", "ptr"), "ee_target_step"), (on("r", "hold_ticks", 1), "hold_ticks"),
               (on("r", "trunk_target_step", "ptr"), "trunk_target_step"),
               (on("t", "n_tracks", 0), "n_tracks"), (on("t", "n_tracks", 7), "n_tracks"),
               (on("t1", "target", TRUNK), "target"), (on("t1", "target", 6), "target"), (on("t0", "target", -1), "target"),
               (on("t0", "kind", 2), "kind"), (on("t1", "kind", -1), "kind"),
               (on("t0", "max_points", 1), "max_points"), (on("t1", "max_points", capi.MAX_TRAJ_POINTS + 1), "max_points"),
               (on("t0", "points", None), "points"), (on("t1", "tangents", "ptr"), "tangents"),
               (on("t0", "du_all", 0.0), "du_all"), (on("t1", "du_all", float("nan")), "du_all"), (on("t0", "du_all", float("inf")), "du_all"),
               (on("t1", "du_all", -0.002), "du_all"),
               (on("in", "trunk_target", None), "trunk_target"), (on("in", "prev_trunk_target", None), "trunk_target"),
               (trunk_unfollowed("prev_trunk_target", None), "trunk_target"),             # score bit 5 alone needs them too
               (on("s", "score_mask", 1 << 6), "score_mask"), (on("s", "score_mask", -1), "score_mask"), (on("s", "group_size", 3), "group_size")]
    for tweak, word in refused:
        rc, msg = _raw_call(bt, d, B, K, points, tweak)
        assert rc == -1 and word in msg, (word, rc, msg)             # WBC_E_ARG
    rc, msg = _raw_call(bt, d, B, K, points, lambda *a: None)
    assert rc == 0, msg
    rc, msg = _raw_call(bt, d, B, K, points, on("s", "group_size", 4))
    assert rc == 0, msg
    rc, msg = _raw_call(bt, d, B, K, points, on("t0", "tangents", "ptr"))     # tangents on the HERMITE track
    assert rc == 0, msg

    def step_without_trunk_track(r, t, s, tin, spare):                        # trunk_target_step stays allowed without a trunk track
        t.n_tracks = 1
        t.track[0].target, t.track[0].kind = GRIP, capi.TRACK_LINEAR
        r.trunk_target_step = spare
    rc, msg = _raw_call(bt, d, B, K, points, step_without_trunk_track)
    assert rc == 0, msg
    bt.close()


def test_trunk_step_without_a_trunk_track_is_rollouts():
    """a constant trunk step beside a gripper track, the trunk scored against the target of the tick: the targets are wbc_rollout's sums"""
    g = _group_problem()
    B, K = 8, 5
    d = {k: v[:B] for k, v in g["d"].items()}
    step = np.full((B, 3), 1e-4) * np.arange(1, B + 1)[:, None]
    bt = _handle(g, max_batch=B)
    got = bt.rollout_tracks(d, DT, K, _cut(g["tracks"], B)[1:], score=("trunk",), trunk_target_step=step, want_trace=True)
    bt.close()
    tt = d["trunk_target"].copy()
    e2 = np.zeros(B)
    for k in range(K):
        dd = got["trace"][k, 0] - tt
        e2 = e2 + ((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
        tt = tt + step
    assert (got["trunk_target"] == tt).all()
    assert np.abs(got["err_sq_sum"][0] - e2).max() <= 4 * K * np.finfo(float).eps * e2.max()


# ------------------------------------------------------------------------------------------------ 8. device pointers
def test_device_tensors_give_the_host_calls_bits():
    import torch
    p = _problem("base")
    bt = _handle(p)
    host = _run(bt, p, group_size=0)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d = {k: dev(v) for k, v in p["d"].items()}
    tracks = [{k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in p["tracks"]]
    got = bt.rollout_tracks(d, DT, p["K"], tracks, score=("trunk", GRIP), imu=dev(p["imu"]), want_trace=True)
    torch.cuda.synchronize()
    assert set(got) == set(host)
    for k in host:
        assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    _check_parity({k: v.cpu().numpy() for k, v in got.items()}, p, _reference("base"), cold=True)
    bt.close()
