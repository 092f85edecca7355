"""Every kernel that reads dt, at time steps other than 2 ms (the steps, the bounds' scaling rule and the problems: dt_cases.py).

Assemble, tick on every path, the exact optimum through the device's own assembly, one handle at alternating steps, integrate, roll-outs and
the two gradient kernels, each against the CPU oracle or the host restatement at that step; and the steps that are not numbers to run at."""
import numpy as np
import pytest

import common
import devguard as dg
import dt_cases as dc
import grad_common as gc
import gradq_common as gq
import oracle
import slack_common as sc
import test_gpu_task_params as tgp
import test_gpu_tick_grad as tgg
import test_gpu_tick_grad_q as tggq
import wbc_capi as capi
import wbc_workload
from test_gpu_parity import ASSEMBLE_TOL, INTEGRATE_TOL, QDOT_TOL, relerr
from test_gpu_tick_grad import PARITY_BOUND

pytestmark = pytest.mark.gpu

DT0, DTS, B0 = dc.DT0, dc.DTS, dc.B0
# one: a1_wx200 alone, no model_id (the packed sim3 kernel's FIXD form); two: a1_wx200 / a1_px100 interleaved (the packed kernels' general
# forms); three: with the Laikago (the general kernel and the compact one: its tree fits no packed kernel)
KINDS = {"one": dc.ONE, "two": dc.TWO, "three": dc.THREE}
# (presolve, presolve_orth, sim3_kernel, packed_kernel) of test_gpu_solution_against_the_exact_optimum
KEYS = ((1, 1, 1, 1), (1, 1, 1, 0), (1, 1, 0, 0), (1, 0, 0, 0), (0, 0, 0, 0))


def _set_key(bt, key):
    """-> the refine option the key runs with"""
    for name, v in zip(("presolve", "presolve_orth", "sim3_kernel", "packed_kernel"), key):
        bt.set_option(name, v)
    refine = 0 if key == (1, 1, 1, 0) else 1     # (the one-instance compact kernel: chosen with the refinement off only)
    bt.set_option("refine", refine)
    bt.set_option("packed_orth", 2)              # (small batch: 1 would keep config 2 on the one-instance kernel)
    bt.set_option("packed_box", 2 if key[3] else 0)
    return refine


def _expected_paths(cfg_name):
    """the (last_path, last_orth) pairs test_gpu_solution_against_the_exact_optimum asks of a one-model a1_wx200 batch"""
    if cfg_name == "c3":
        return {(2, 0), (1, 0), (0, 0)}                    # packed, one-instance compact, general
    if cfg_name in ("c2", "everything"):
        return {(0, 1), (0, 0), (3, 1)}                    # orthonormal presolve, full size, the packed orth kernel
    if cfg_name == "full":
        return {(4, 0), (0, 0)}                            # the packed box kernel, full size
    return set()


# ------------------------------------------------------------------------------------------------ 5. assemble
@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("cfg_name", ["everything", "c3_trunk_task"])
def test_assemble_against_the_oracle_and_the_doubling_law(cfg_name, mfma):
    models, cfgs, d, mid = dc.problem(dc.THREE, cfg_name)
    bt = tgp._handle(models, cfgs, B0, {"jtj_mfma": mfma})
    for dt in DTS:
        got, ref = bt.assemble(d, dt), dc.assembled(dc.THREE, cfg_name, dt)
        worst = 0.0
        for k in ("A", "b", "H", "g", "C", "Clb", "Cub", "lb", "ub"):
            assert got[k].shape == ref[k].shape, k
            e = relerr(got[k], ref[k])
            worst = max(worst, e)
            assert e < ASSEMBLE_TOL, (cfg_name, dt, k, e)
        dc.report("assemble (relerr), jtj_mfma %d" % mfma, cfg_name, dt, worst, ASSEMBLE_TOL)
    for dt in dc.LAW_DTS:
        live = dc.check_doubling_law(bt.assemble(d, dt), bt.assemble(d, 2 * dt), cfg_name, "%s, dt %.7g, jtj_mfma %d" % (cfg_name, dt, mfma))
        assert live >= 2 * 4 + 6                           # the trunk-box rows of Clb and Cub and the gripper's rows of b at the least
    bt.close()


# ------------------------------------------------------------------------------------------------ 6. tick, every path
def _check_tick(got, ref, models, d, mid, dt, tol, test, cfg_name, what):
    assert (got["status"] == ref["status"]).all(), (what, np.flatnonzero(got["status"] != ref["status"]))
    ok = ref["status"] == 0
    err = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    own = oracle.integrate(models, d["q"], got["qdot"], dt, mid)
    e_own = np.abs(got["q_next"] - own).max()
    dc.report(test, cfg_name, dt, err, tol)
    print("%s: qdot max-abs err vs oracle %.3e (bound %.1e), q_next vs integrate(own qdot) %.3e, max|qdot| %.3g" % (
        what, err, tol, e_own, np.abs(ref["qdot"][ok]).max()))
    assert err < tol, (what, err, tol)
    assert e_own < 1e-13, (what, e_own)
    assert (got["qdot"][~ok] == 0).all(), what


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cfg_name", dc.TICK_CONFIGS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_tick_on_every_path(kind, cfg_name, dt):
    names = KINDS[kind]
    models, cfgs, d, mid = dc.problem(names, cfg_name)
    ref = dc.reference(names, cfg_name, dt)
    assert (ref["status"] == 0).sum() >= B0 - 4            # the oracle alone solves the step (measured: 67 of 67 everywhere)
    bt = tgp._handle(models, cfgs, B0, {})
    paths, status0 = set(), None
    for key in KEYS:
        refine = _set_key(bt, key)
        got = bt.tick(d, dt, want_q_next=True)
        path = (bt.stat("last_path"), bt.stat("last_orth"))
        paths.add(path)
        if path[0] == 2:     # the packed sim3 kernel: its FIXD form on one model without model_id (the rows without QCON: a posture target
            #                      passed by the caller, as under HYBRID here, is a QCON row), its general form on a mixed batch
            assert bt.stat("last_tick_fixd") == (1 if kind == "one" and cfg_name != "c3_hybrid" else 0), (key, path)
        else:
            assert bt.stat("last_tick_fixd") == 0, (key, path)
        if status0 is None:
            status0 = got["status"].copy()
        assert (got["status"] == status0).all(), "status differs between kernel paths %s" % (key,)
        tol = dc.path_tol(cfgs[0], path[0], path[1], refine, dt)
        held = "REFINED_TOL" if dc.path_refines(cfgs[0], path[0], path[1], refine) else "QDOT_TOL"
        _check_tick(got, ref, models, d, mid, dt, tol, "tick %s, path %s, %s" % (kind, path, held), cfg_name,
                    "%s / %s / dt %.7g / key %s / path %s" % (kind, cfg_name, dt, key, path))
    print("%s / %s / dt %.7g: paths %s" % (kind, cfg_name, dt, sorted(paths)))
    if kind != "three":      # (the Laikago's tree fits no packed kernel: the three-model batch runs the general kernel and the compact one)
        assert _expected_paths(cfg_name) <= paths, paths
        if cfg_name in ("c3_trunk_task", "c3_hybrid"):
            assert (2, 0) in paths                         # the packed sim3 kernel's TRUNK / QCON variants
    bt.close()


@pytest.mark.parametrize("dt", DTS)
def test_tick_with_per_instance_task_rows(dt):
    models, cfgs, d, mid = dc.problem(dc.TWO, "everything")
    rows = tgp._random_rows(tgp._rows_of(cfgs, mid, B0), seed=5)
    ms, cs, pid = tgp._per_instance(models, cfgs, mid, rows)
    ref = oracle.tick(ms, cs, dict(d, model_id=pid), dt, B0, nthreads=8)
    ok = ref["status"] == 0
    assert ok.sum() >= B0 - 4
    tol, ratio = tgp._qdot_tol(models, cfgs, mid, d, ms, cs, pid, B0)     # (per instance; H, and so the widening, does not depend on dt)
    bt = tgp._handle(models, cfgs, B0, {})
    for opts in ({}, {"packed_orth": 2}):
        for k, v in opts.items():
            bt.set_option(k, v)
        got = bt.tick(d, dt, want_q_next=True, task_params=rows)
        assert (got["status"] == ref["status"]).all()
        err = np.abs(got["qdot"] - ref["qdot"]).max(axis=1)
        plain = ok & (ratio <= 1.0)
        dc.report("tick, task rows, path %d (err / per-instance bound)" % bt.stat("last_path"), "everything", dt, (err / (tol * dc.qdot_scale(dt)))[ok].max(), 1.0)
        assert (err[ok] <= tol[ok] * dc.qdot_scale(dt)).all()
        assert err[plain].max(initial=0.0) < dc.qdot_bound(QDOT_TOL, dt)
        own = oracle.integrate(models, d["q"], got["qdot"], dt, mid)
        assert np.abs(got["q_next"] - own).max() < 1e-13
    bt.close()


# ------------------------------------------------------------------------------------------------ 7. the exact optimum
@pytest.mark.parametrize("dt", dc.GRAD_DTS)
@pytest.mark.parametrize("cfg_name", ["c3", "full"])
def test_exact_optimum_through_the_devices_own_assembly(cfg_name, dt):
    """test_gpu_solution_against_the_exact_optimum at another step: the bounds of its paths times max(1, 0.002 / dt)"""
    B = 8
    models, cfgs, d, mid = dc.problem(dc.ONE, cfg_name, B, 71)
    nv = models[0].nv
    bt = tgp._handle(models, cfgs, B, {})
    a = bt.assemble(d, dt)
    exact, worst, status0 = {}, {}, None
    for key in KEYS:
        _set_key(bt, key)
        got = bt.tick(d, dt)
        path = (bt.stat("last_path"), bt.stat("last_orth"))
        if status0 is None:
            status0 = got["status"].copy()
        assert (got["status"] == status0).all(), "status differs between kernel paths %s" % (key,)
        for b in range(B):
            if got["status"][b] != 0:
                continue
            if b not in exact:
                exact[b] = common.exact_ls_optimum(a["A"][b][:, :nv], a["b"][b], a["C"][b][:, :nv], a["lb"][b][:nv], a["ub"][b][:nv],
                                                   a["Clb"][b], a["Cub"][b], got["qdot"][b][:nv])
            worst[(key, path)] = max(worst.get((key, path), 0.0), np.abs(got["qdot"][b][:nv] - exact[b]).max())
    bt.close()
    assert len(exact) >= B - 4
    s = dc.qdot_scale(dt)
    for (key, path), w in worst.items():
        bound = (2e-6 if path == (1, 0) else 1e-7) * s
        dc.report("exact optimum, path %s" % (path,), cfg_name, dt, w, bound)
        assert w < bound, (key, path, w)
    paths = {k[1] for k in worst}
    assert _expected_paths(cfg_name) <= paths, paths
    if cfg_name == "full":
        assert worst[((1, 1, 1, 1), (4, 0))] < 1e-9 * s


# ------------------------------------------------------------------------------------------------ 8. one handle, alternating steps
@pytest.mark.parametrize("cfg_name,kind", [("c3", "one"), ("c3_trunk_task", "two"), ("everything", "two"), ("full", "one")])
def test_one_handle_at_alternating_steps(cfg_name, kind):
    """a handle carries nothing of the last call's dt into the next: 0.002, 0.0005, 0.002, 1 / 240, 0.002 on one handle, each byte for byte
    what a fresh handle gives at that step alone; wave_order 1, then 2"""
    names = KINDS[kind]
    models, cfgs, d, mid = dc.problem(names, cfg_name)
    opts = {"packed_orth": 2}
    steps = (DT0, 0.0005, DT0, 1 / 240, DT0)
    fresh = {}
    for dt in set(steps):
        bt = tgp._handle(models, cfgs, B0, opts)
        fresh[dt] = bt.tick(d, dt, want_q_next=True, want_working_set=True)
        bt.close()
    assert not dg.same_bytes(fresh[DT0]["qdot"], fresh[0.0005]["qdot"]) and not dg.same_bytes(fresh[DT0]["qdot"], fresh[1 / 240]["qdot"])
    bt = tgp._handle(models, cfgs, B0, opts)
    for wo in (1, 2):
        bt.set_option("wave_order", wo)
        for i, dt in enumerate(steps):
            got = bt.tick(d, dt, want_q_next=True, want_working_set=True)
            for k in got:
                assert dg.same_bytes(got[k], fresh[dt][k]), (cfg_name, "wave_order %d" % wo, "call %d at dt %.7g" % (i, dt), k)
    bt.close()


# ------------------------------------------------------------------------------------------------ 9. integrate
@pytest.mark.parametrize("dt", DTS)
def test_integrate(dt):
    """test_integrate_parity's two velocity sets at another step, the x 300 set rescaled by 0.002 / dt so the rotation per step stays what it is
    at 2 ms. That set turns the base by 0.6 rad x chi_3 per step: measured on the oracle's output, 1 attitude of 256 ends with tr R <= 0 (at
    every step, 2 ms included), so it does NOT reach the branches of the quaternion it is there for. A third set, x 1000 (2 rad x chi_3), does:
    more than a quarter of its attitudes have tr R <= 0 (measured: 151 of 256), asserted on the oracle's output. It is held to the x 300 set's
    1e-12: a unit quaternion's components come from sin and cos of |w| dt / 2 <= 6, a handful of roundings of values <= 1 each."""
    wx200 = tgp._model("a1_wx200")
    rng = np.random.default_rng(9)
    B = 256
    q = wbc_workload.sample_q(wx200, B, rng)
    v = rng.normal(size=(B, 26)) * 2
    v[:8, 3:6] = 0                       # the small-angle branch
    ref = oracle.integrate([wx200], q, v, dt)
    bt = tgp._handle([wx200], [common.config("c3", wx200)], B, {})
    e = np.abs(bt.integrate(q, v, dt) - ref).max()
    dc.report("integrate", "-", dt, e, INTEGRATE_TOL)
    assert e < INTEGRATE_TOL
    unit = rng.normal(size=(B, 26))
    for scale in (300, 1000):
        big = unit * scale * (DT0 / dt)
        rb = oracle.integrate([wx200], q, big, dt)
        x, y, z, w = rb[:, 3], rb[:, 4], rb[:, 5], rb[:, 6]
        trace = 3.0 - 4.0 * (x * x + y * y + z * z) / (x * x + y * y + z * z + w * w)          # tr R of the quaternion (x, y, z, w)
        print("integrate x %d at dt %.7g: %d of %d attitudes with tr R <= 0" % (scale, dt, (trace <= 0).sum(), B))
        if scale == 1000:
            assert (trace <= 0).mean() > 0.25, (trace <= 0).mean()
        e = np.abs(bt.integrate(q, big, dt) - rb).max()
        dc.report("integrate, x %d rotations" % scale, "-", dt, e, 1e-12)
        assert e < 1e-12
    bt.close()


def test_integrate_forward_and_back():
    """dt < 0 is a step back: q (+) v dt (+) v (-dt) on the device against the oracle's round trip"""
    wx200 = tgp._model("a1_wx200")
    rng = np.random.default_rng(10)
    B = 67
    q = wbc_workload.sample_q(wx200, B, rng)
    v = rng.normal(size=(B, 26)) * 2
    bt = tgp._handle([wx200], [common.config("c3", wx200)], B, {})
    for dt in (1 / 240, 0.02):
        fwd = bt.integrate(q, v, dt)
        back = bt.integrate(fwd, v, -dt)
        rf = oracle.integrate([wx200], q, v, dt)
        rb = oracle.integrate([wx200], rf, v, -dt)
        assert np.abs(fwd - rf).max() < INTEGRATE_TOL and np.abs(back - rb).max() < INTEGRATE_TOL
        assert np.abs(back - q).max() < 1e-12 and np.abs(fwd - q).max() > 1e-4
    bt.close()


# ------------------------------------------------------------------------------------------------ 10. roll-outs
RB, RK = 16, 6
ROLL_DTS = (0.0005, 0.02)


def _roll_problem(cfg_name):
    models, cfgs, d, mid = dc.problem(dc.ONE, cfg_name, RB, 37)
    rng = np.random.default_rng(2)
    step = np.zeros((RB, 5, 3))
    step[:, 4] = rng.normal(0, 1e-4, (RB, 3))
    tstep = rng.normal(0, 5e-5, (RB, 3))
    return models, cfgs, d, step, tstep, d["q"][:, 3:7].copy()


@pytest.mark.parametrize("dt", ROLL_DTS)
@pytest.mark.parametrize("cfg_name", ["c3", "everything"])
def test_rollout_against_the_oracle(cfg_name, dt):
    models, cfgs, d, step, tstep, imu = _roll_problem(cfg_name)
    ref = oracle.rollout(models, cfgs, d, dt, RB, RK, ee_target_step=step, trunk_target_step=tstep, imu=imu, nthreads=8)
    ok = ref["status"] == 0
    print("%s dt %.7g: the oracle solves every tick of %d of %d instances" % (cfg_name, dt, ok.sum(), RB))
    assert ok.sum() >= RB // 2
    bt = tgp._handle(models, cfgs, RB, {"packed_orth": 2})
    bound = dc.state_bound(dt)
    for warm in ((1, 0) if cfg_name == "c3" else (0,)):
        bt.set_option("warm_start", warm)
        got = bt.rollout(d, dt, RK, ee_target_step=step, trunk_target_step=tstep, imu=imu)
        assert (got["status"] == ref["status"]).all(), warm
        e_q = np.abs(got["q"] - ref["q"])[ok].max()
        e_t = np.abs(got["grip_trace"] - ref["grip_trace"])[:, ok].max()
        e_v = np.abs(got["qdot"] - ref["qdot"])[ok].max()
        dc.report("rollout state, warm_start %d" % warm, cfg_name, dt, max(e_q, e_t), bound)
        dc.report("rollout final qdot, warm_start %d" % warm, cfg_name, dt, e_v, dc.qdot_bound(10 * QDOT_TOL, dt))
        assert e_q < bound and e_t < bound, (warm, e_q, e_t)
        assert e_v < dc.qdot_bound(10 * QDOT_TOL, dt), (warm, e_v)
        assert np.abs(got["ee_target"] - ref["ee_target"]).max() < 1e-15
    bt.close()


@pytest.mark.parametrize("dt", ROLL_DTS)
def test_rollout_equals_tick_plus_update_state(dt):
    """test_rollout_equals_tick_plus_update_state at another step: bitwise, warm-started and cold"""
    wx200 = tgp._model("a1_wx200")
    B, K = 64, 4
    cfg = common.config("c3", wx200)
    d = common.tick_inputs(wx200, cfg, B, seed=39)
    step = np.zeros((B, 5, 3))
    step[:, 4] = [1e-4, -5e-5, 2e-5]
    bt = tgp._handle([wx200], [cfg], B, {})
    for warm in (1, 0):
        bt.set_option("warm_start", warm)
        got = bt.rollout(d, dt, K, ee_target_step=step)
        s = {k: v.copy() for k, v in d.items()}
        for _ in range(K):
            o = bt.tick(s, dt, want_q_next=True, want_working_set=bool(warm))
            s["q"] = bt.update_state(s["q"], o["q_next"], s["ee_target"])
            s["prev_ee_target"][:, 4] = s["ee_target"][:, 4]
            s["ee_target"] = s["ee_target"] + step
            if warm:
                s["working_set"] = o["working_set"]
        assert (got["q"] == s["q"]).all() and (got["qdot"] == o["qdot"]).all() and (got["ee_target"] == s["ee_target"]).all(), warm
    bt.close()


@pytest.mark.parametrize("dt", ROLL_DTS)
def test_rollout_tracks_against_the_oracle_loop(dt):
    """the base recipe of test_gpu_rollout_tracks.py (a Hermite trunk track, a linear gripper track) through common.tracks_reference at dt"""
    models, mid = [tgp._model("a1_wx200")], None
    cfgs = [common.config("c3_trunk_task", models[0])]
    d = common.tick_inputs(models[0], cfgs[0], RB, seed=37, stress=False)          # (no orientation references: tracks_reference carries none)
    pos = common.track_frames(models, d["q"], mid)
    tracks = common.base_tracks(d, pos[:, common.GRIP], 5)
    common.start_previous_targets(d, tracks)
    p = dict(models=models, cfgs=cfgs, d=d, mid=mid, tracks=tracks, B=RB, K=RK, imu=d["q"][:, 3:7].copy(), running=True, rows=None)
    ref = common.tracks_reference(p, dt)
    ok = ref["status"] == 0
    assert ok.sum() >= RB // 2
    bt = tgp._handle(models, cfgs, RB, {})
    got = bt.rollout_tracks(d, dt, RK, tracks, score=("trunk", common.GRIP), imu=p["imu"], want_trace=True)
    assert bt.stat("last_path") == 2
    bt.close()
    assert (got["status"] == ref["status"]).all()
    bound = dc.state_bound(dt)
    e_q = np.abs(got["q"] - ref["q"])[ok].max()
    e_g = np.abs(got["grip_trace"] - ref["frames"][:, :, common.GRIP])[:, ok].max()
    e_t = max(np.abs(got["trace"][:, j] - ref["frames"][:, :, f])[:, ok].max() for j, f in enumerate((common.GRIP, common.TRUNK)))
    e_v = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    e_f = max(np.abs(got["ee_target"] - ref["ee_target"]).max(), np.abs(got["trunk_target"] - ref["trunk_target"]).max())
    dc.report("rollout_tracks state and traces", "c3_trunk_task", dt, max(e_q, e_g, e_t), bound)
    assert e_q < bound and e_g < bound and e_t < bound and e_f < 1e-15
    assert e_v < dc.qdot_bound(10 * QDOT_TOL, dt)
    # the scores are those of the device's own trace against the oracle loop's targets of the tick
    targets = np.stack([ref["targets"][:, :, common.GRIP], ref["targets"][:, :, common.TRUNK]], axis=1)
    scores = common.numpy_scores(got["trace"], targets, ref["tick_status"])
    assert np.abs(got["err_final"] - scores["err_final"]).max() < 1e-12 and np.abs(got["err_max"] - scores["err_max"]).max() < 1e-12


@pytest.mark.parametrize("dt", ROLL_DTS)
def test_rollout_watch_against_the_oracle_loop(dt):
    """the sim3 recipe of test_gpu_slack.py at another step: trace, slack_min and slack_final at that test's 1e-6, the summary the reduction of
    the device's own trace bit for bit"""
    p, ref = sc.watch_problem("sim3", RB, RK), sc.watch_reference("sim3", RB, RK, dt)
    bt = tgp._handle(p["models"], p["cfgs"], RB, {})
    got = bt.rollout_watch(p["d"], dt, RK, imu=p["imu"], want_trace=True, ee_target_step=p["step"])
    assert bt.stat("last_path") == 2
    bt.close()
    assert (got["status"] == ref["status"]).all()
    ok = ref["status"] == 0
    assert ok.sum() >= RB // 2
    want, own = wbc_workload.watch_summary(ref["trace"]), wbc_workload.watch_summary(got["slack_trace"])
    e_t = np.abs(got["slack_trace"] - ref["trace"])[:, :, ok].max()
    e_m = np.abs(got["slack_min"] - want["slack_min"])[:, ok].max()
    e_f = np.abs(got["slack_final"] - want["slack_final"])[:, ok].max()
    dc.report("rollout_watch slack trace, min, final", "c3", dt, max(e_t, e_m, e_f), 1e-6)
    assert e_t < 1e-6 and e_m < 1e-6 and e_f < 1e-6
    for k in own:
        assert dg.same_bytes(own[k], got[k]), k


# ------------------------------------------------------------------------------------------------ 11. gradients
@pytest.mark.parametrize("dt", dc.GRAD_DTS)
@pytest.mark.parametrize("cfg_name", ["everything", "c3", "c3_trunk_task"])
def test_gradients_against_the_restatements(cfg_name, dt):
    """wbc_tick_vjp against wbc_workload.tick_gradients and wbc_tick_vjp_state against tick_state_gradients, both fed the device's own qdot
    and certificate, on the three-model batch at PARITY_BOUND max(1, max|ref|)"""
    models, cfgs, d, mid, rows, v = tgg._problem("mixed67", cfg_name)
    B = len(rows)
    bt = tgp._handle(models, cfgs, B, {})
    got = bt.tick_grad(d, dt, v, task_params=rows)
    ref = gc.restate(models, cfgs, mid, d, got["qdot"], got["sens_x"], rows, dt=dt)
    bad = (got["status"] != 0) | (got["cert_status"] != capi.CERT_OK)
    assert bad.sum() <= B // 2, "too few solved and certified instances: %d of %d" % (B - bad.sum(), B)
    worst = 0.0
    for k in bt.default_grad_wants():
        ref[k][bad] = 0.0
        ratio = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
        worst = max(worst, ratio)
        assert ratio <= PARITY_BOUND, (k, ratio)
        assert (got[k][bad] == 0).all()
    dc.report("tick_grad, worst ratio to max(1, max abs ref)", cfg_name, dt, worst, PARITY_BOUND)
    gotq = bt.tick_grad_q(d, dt, v, task_params=rows)
    refq = gq.restate(models, cfgs, mid, d, {k: gotq[k] for k in tggq.CERT_KEYS}, rows, gotq["working_set"], dt=dt)
    badq = (gotq["status"] != 0) | (gotq["cert_status"] != capi.CERT_OK)
    assert badq.sum() <= B // 2
    worst = 0.0
    for k in ["d_q"] + (["d_trunk_box_center"] if cfgs[0].con_trunk else []):
        refq[k][badq] = 0.0
        ratio = np.abs(gotq[k] - refq[k]).max() / max(1.0, np.abs(refq[k]).max())
        worst = max(worst, ratio)
        assert ratio <= PARITY_BOUND, (k, ratio)
        assert (gotq[k][badq] == 0).all()
    assert np.abs(gotq["d_q"][~badq]).max() > 0
    dc.report("tick_grad_q, worst ratio to max(1, max abs ref)", cfg_name, dt, worst, PARITY_BOUND)
    bt.close()


@pytest.mark.parametrize("dt", dc.GRAD_DTS)
def test_state_gradient_on_arbitrary_sensitivities(dt):
    """test_gpu_tick_grad_q.test_parity_on_arbitrary_sensitivities at another step: x, u, w, y drawn at random in every column and row, every
    bound and row marked at a random side. A tick's own certificate leaves w = 0 on every inactive row — on this batch the CoM box's rows — so
    only this weighs the 1 / dt of d Clb / d q and d Cub / d q of ALL box rows (a constant 500.0 in the CoM-box factor passes the test above)."""
    models, cfgs, d, mid, rows, _ = tggq._problem("mixed67", "everything", seed=37)
    B = len(rows)
    bt = tgp._handle(models, cfgs, B, {})
    p = bt.constraint_rows
    rng = np.random.default_rng(41)
    cert = dict(qdot=rng.normal(0, 0.5, (B, 26)), sens_x=rng.normal(0, 0.5, (B, 26)), sens_bounds=rng.normal(0, 1.0, (B, 26)),
                sens_rows=rng.normal(0, 1.0, (B, p)), y_rows=rng.normal(0, 1.0, (B, p)))
    ws = np.zeros((B, 2), dtype=np.int64)
    for word, n in ((0, 26), (1, p)):
        up = rng.integers(0, 2, (B, n))
        ws[:, word] = ((1 << (np.arange(n)[None, :] + 32 * up)).sum(axis=1)).astype(np.int64)
    got = bt.tick_vjp_state(d, dt, cert["qdot"], cert["sens_x"], sens_bounds=cert["sens_bounds"], sens_rows=cert["sens_rows"], y_rows=cert["y_rows"],
                            working_set=ws, task_params=rows)
    bt.close()
    assert (got["grad_status"] == 0).all()
    ref = gq.restate(models, cfgs, mid, d, cert, rows, ws, dt=dt)
    at_2ms = gq.restate(models, cfgs, mid, d, cert, rows, ws)
    worst = 0.0
    for k in ("d_q", "d_trunk_box_center"):
        scale = max(1.0, np.abs(ref[k]).max())
        ratio = np.abs(got[k] - ref[k]).max() / scale
        worst = max(worst, ratio)
        assert ratio <= PARITY_BOUND, (k, ratio)
        assert np.abs(ref[k] - at_2ms[k]).max() / scale > 1e-3, k             # (the step does reach the reference)
    dc.report("tick_vjp_state, arbitrary sensitivities, worst ratio to max(1, max abs ref)", "everything", dt, worst, PARITY_BOUND)


def test_torch_state_layer_backward_at_another_step():
    """wbc_torch.wbc_tick_state's backward at dt = 1 / 240 is tick_grad_q + tangent_to_raw at that step, bit for bit"""
    import torch
    import wbc_torch
    dt = 1 / 240
    models, cfgs, d, mid, rows, v, bt = tggq._clean("mixed67", "c3_trunk_task", seed=29)
    ref = bt.tick_grad_q(d, dt, v, task_params=rows)
    at_2ms = bt.tick_grad_q(d, DT0, v, task_params=rows)
    assert np.abs(ref["d_q"] - at_2ms["d_q"]).max() > 1e-6                 # (the step does reach the gradient)
    raw = wbc_workload.tangent_to_raw(d["q"], ref["d_q"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(x)).cuda() for k, x in d.items()}
    q = dev["q"].clone().requires_grad_(True)
    qdot, st = wbc_torch.wbc_tick_state(q, torch.from_numpy(rows).cuda(), None, None, None, None, None, None, None, dev, dt, bt)
    assert tggq._same(qdot.detach().cpu().numpy(), ref["qdot"])
    (qdot * torch.from_numpy(v).cuda()).sum().backward()
    assert tggq._same(q.grad.cpu().numpy(), raw)
    bt.close()


# ------------------------------------------------------------------------------------------------ 12. steps that are not numbers to run at
BAD_DTS = (float("nan"), 0.0, -0.002, float("inf"), 5e-324)


def test_bad_steps_are_refused_before_any_launch():
    """NaN, 0, a negative step, +inf (1 / dt = 0) and a subnormal (1 / dt = inf): every dt-taking entry point answers WBC_E_ARG with a message
    naming dt, writes nothing, and the valid call after it is byte for byte the valid call before. wbc_integrate takes a negative step."""
    B, K = 16, 3
    models, cfgs, d0, mid = dc.problem(dc.ONE, "c3_trunk_task", B, 37)
    d = {k: x.copy() for k, x in d0.items()}
    rng = np.random.default_rng(3)
    v = gc.task_space_v(models, cfgs, mid, d, rng)
    pos = common.track_frames(models, d["q"], mid)
    tracks = common.base_tracks(d, pos[:, common.GRIP], 5)
    common.start_previous_targets(d, tracks)
    imu = d["q"][:, 3:7].copy()
    grip = tracks[1]
    bt = tgp._handle(models, cfgs, B, {})
    c = bt.tick_certificate(d, DT0, v=v)
    vel = rng.normal(size=(B, 26))
    calls = {
        "tick": lambda dt: bt.tick(d, dt, want_q_next=True),
        "assemble": lambda dt: bt.assemble(d, dt),
        "rollout": lambda dt: bt.rollout(d, dt, K, imu=imu),
        "rollout_traj": lambda dt: bt.rollout_traj(d, dt, K, points=grip["points"], n_points=grip["n_points"], du=grip["du"], imu=imu),
        "rollout_tracks": lambda dt: bt.rollout_tracks(d, dt, K, tracks, score=("trunk",), imu=imu),
        "rollout_watch": lambda dt: bt.rollout_watch(d, dt, K, imu=imu),
        "tick_vjp": lambda dt: bt.tick_vjp(d, dt, c["qdot"], c["sens_x"], status=c["status"], cert_status=c["cert_status"]),
        "tick_vjp_state": lambda dt: bt.tick_vjp_state(d, dt, c["qdot"], c["sens_x"], sens_bounds=c["sens_bounds"], sens_rows=c["sens_rows"],
                                                       y_rows=c["y_rows"], status=c["status"], cert_status=c["cert_status"],
                                                       working_set=c["working_set"]),
        "integrate": lambda dt: dict(q_next=bt.integrate(d["q"], vel, dt)),
    }
    before = {name: call(DT0) for name, call in calls.items()}
    for bad in BAD_DTS:
        for name, call in calls.items():
            if name == "integrate" and bad < 0:
                continue
            with pytest.raises(capi.WbcError) as e:
                call(bad)
            assert e.value.code == capi.E_ARG and "dt" in str(e.value), (name, bad, str(e.value))
        # nothing is written: caller's outputs keep their fill
        out = dict(qdot=np.full((B, 26), np.nan), status=np.full(B, -77, np.int32), iters=np.full(B, -77, np.int32), q_next=np.full((B, 27), np.nan))
        with pytest.raises(capi.WbcError):
            bt.tick(d, bad, out=out)
        assert np.isnan(out["qdot"]).all() and np.isnan(out["q_next"]).all() and (out["status"] == -77).all() and (out["iters"] == -77).all()
    for name, call in calls.items():
        after = call(DT0)
        assert set(after) == set(before[name])
        for k in after:
            assert dg.same_bytes(after[k], before[name][k]), (name, k)
    back = bt.integrate(d["q"], vel, -0.002)
    assert np.abs(back - oracle.integrate(models, d["q"], vel, -0.002)).max() < INTEGRATE_TOL
    bt.close()
