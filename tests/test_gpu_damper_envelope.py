"""The velocity damper in every zone, DoF class and tick path.

The damper is written out on the device four times (damper_bounds of wbc_common.h for the packed kernels' kept and eliminated lanes, the same
statements in process_instance and in wbc_k_sim3.hip, gq_damper with the derivative) and the packed kernels show their copy through q̇ alone,
where a q-dependent bound is active. sample_q and the stress recipe reach one arm DoF in the band 0 <= d < qs and nothing else. Here
common.damper_tick_inputs puts 1 - 5 DoF of every instance (base, stance legs, arm) into the regular zone, the flipped band, beyond the limit,
exactly on the zone edge and exactly at d = qs, under the reference's index map and under the corrected one; test_damper_envelope_host.py holds
the conditions on these inputs without a GPU (every class and zone active in the oracle's solutions, q̇ answering to a 1e-4 change of qs).
Everything is held to the oracle at the tolerances of the existing parity tests — none is new."""
import functools

import numpy as np
import pytest

import common
import damper_cases as dc
import grad_common as gc
import oracle
import pose_cases as pc
import test_gpu_pose_envelope as pe
import test_gpu_task_params as tgp
import test_gpu_tick_grad_q as tgq
import wbc_capi as capi

pytestmark = pytest.mark.gpu

DT, QDOT_TOL, B0 = dc.DT, dc.QDOT_TOL, dc.B0
REG, FLIP, BEYOND, EDGE, AT_QS = range(5)      # common.DAMPER_KINDS
MAP_NAME = {True: "reference map", False: "corrected map"}
CASES = [(n, c) for n in dc.TICK_CASES for c in dc.MAPS]


def _report_row(bt, what):
    print("%s: ran on path %d, variant %s" % (what, bt.stat("last_path"), capi.variant_args(bt.stat("last_tick_variant"))))


# ------------------------------------------------------------------------------------------------ 1. assemble: lb / ub themselves
def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


@pytest.mark.parametrize("compat", dc.MAPS)
@pytest.mark.parametrize("cfg_name", ["c3", "everything", "full"])
@pe.stops_at_a_device_fault
def test_assembled_bounds_are_the_literal_transcription(cfg_name, compat):
    """wbc_assemble's lb / ub (process_instance's statements) on the full recipe against test_oracle_assembly._damper_literal: within 4 ulp, the
    "exactly" instances included; a bound that is exactly 0 in the transcription is exactly 0 on the device"""
    p = dc.build_problem(dict(dc.TICK_CASES["c3"], cfg=cfg_name, with_rot=cfg_name != "c3"), compat)
    lb, ub = dc.literal_bounds(p)
    bt = pe._handle(p["models"], p["cfgs"], B0)
    try:
        got = bt.assemble(p["d"], DT)
        worst = 0.0
        for k, want in (("lb", lb), ("ub", ub)):
            zero = want == 0
            assert (got[k][zero] == 0).all(), k
            u = _ulps(got[k][~zero], want[~zero])
            worst = max(worst, u.max())
            assert u.max() <= 4, (k, u.max())
            at = p["zone"][:, :, 0 if k == "lb" else 1]
            assert (at == EDGE).any() and (at == AT_QS).any()
            assert np.array_equal(got[k][(at == EDGE) | (at == AT_QS)], p["asm"][k][(at == EDGE) | (at == AT_QS)])     # the oracle's bits at the kinks
        print("%s, %s: lb, ub worst distance from the literal transcription %.1f ulp" % (cfg_name, MAP_NAME[compat], worst))
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 2. ticks, one per code path and index map
@pytest.mark.parametrize("name,compat", CASES)
@pe.stops_at_a_device_fault
def test_tick_with_bounds_in_every_zone(name, compat):
    case = dc.TICK_CASES[name]
    p = dc.tick_problem(name, compat)
    what = "%s, %s" % (name, MAP_NAME[compat])
    bt = pe._handle(p["models"], p["cfgs"], B0, case["opts"])
    try:
        got = pe._tick(bt, p)
        pe._assert_row(bt, case)
        _report_row(bt, what)
        ok = pe._check(got, p, case["tol"], what)
        if case.get("fates") != "mixed":
            assert ok.mean() >= 0.9
        if name == "c3_tail":
            deferred = bt.stat("deferred_last")
            ratio = pc.leg_block_ratio(p["asm"])
            bar = 10.0 ** -case["opts"]["presolve_tol_exp"]
            print("%s: %d instances deferred to their wave's tail, %d flagged clear of the bar, %d near it" % (
                what, deferred, (ratio < 0.5 * bar).sum(), (ratio < 2 * bar).sum()))
            assert 1 <= (ratio < 0.5 * bar).sum() <= deferred <= (ratio < 2.0 * bar).sum()
        if p["mid"] is not None:
            assert (got["qdot"][p["mid"] == 1, 25] == 0).all()       # px100: the padded DoF
    finally:
        bt.close()


@pytest.mark.parametrize("compat", dc.MAPS)
@pytest.mark.parametrize("name,flags", [("c3", (1, 0, 0, 0, 0)), ("everything_orthp", (1, 1, 0, 0)), ("full", (1, 0, 0))])
@pe.stops_at_a_device_fault
def test_warm_tick_with_bounds_in_every_zone_reaches_the_cold_answer(name, flags, compat):
    """the WARM rows of the packed sim3 kernel, of the packed orth kernel's INEQ variant and of the packed box kernel, seeded with the working
    sets of a perturbed solve, held to the cold oracle answer"""
    case = dc.TICK_CASES[name]
    p = dc.tick_problem(name, compat)
    what = "%s WARM, %s" % (name, MAP_NAME[compat])
    bt = pe._handle(p["models"], p["cfgs"], B0, case["opts"])
    try:
        seeds = pe._seeds(bt, p)
        got = pe._tick(bt, p, dict(p["d"], working_set=seeds), want_working_set=True)
        pe._assert_row(bt, case, flags)
        _report_row(bt, what)
        ok = pe._check(got, p, QDOT_TOL, what)
        assert (got["working_set"][~ok] == 0).all()
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 3. closed loop
@pytest.mark.parametrize("compat", dc.MAPS)
@pytest.mark.parametrize("name", ["c3", "everything_orthp", "full"])
@pe.stops_at_a_device_fault
def test_rollout_from_damper_poses(name, compat):
    """wbc_rollout, 6 ticks with the IMU on, warm start on and off, held to oracle.rollout at test_rollout_parity's tolerances; `everything`
    on the recipe of its must-solve case (base and arm: a stance leg at its limit leaves the CoM box infeasible)"""
    K = 6
    case = dc.TICK_CASES[name]
    p = dc.tick_problem(name, compat)
    m, cfg, d = p["models"][0], p["cfgs"][0], p["d"]
    rng = np.random.default_rng(2)
    step = np.zeros((B0, 5, 3))
    step[:, 4] = rng.normal(0, 1e-4, (B0, 3))
    tstep = rng.normal(0, 5e-5, (B0, 3))
    imu = d["q"][:, 3:7].copy()
    ref = oracle.rollout([m], [cfg], d, DT, B0, K, ee_target_step=step, trunk_target_step=tstep, imu=imu, nthreads=8)
    ok = ref["status"] == 0
    assert ok.mean() > 0.8
    bt = pe._handle([m], [cfg], B0, case["opts"])
    try:
        for warm in (1, 0):
            bt.set_option("warm_start", warm)
            got = bt.rollout(d, DT, K, ee_target_step=step, trunk_target_step=tstep, imu=imu)
            assert bt.stat("last_path") == pc.LAST_PATH[case["row"][0]], warm
            assert bt.stat("last_update_packed") == 1
            assert (got["status"] == ref["status"]).all(), warm
            eq, ev = np.abs(got["q"] - ref["q"])[ok].max(), np.abs(got["qdot"] - ref["qdot"])[ok].max()
            print("%s roll-out, %s, warm start %d: path %d, q max-abs err %.3e, qdot %.3e, optimal %d/%d" % (
                name, MAP_NAME[compat], warm, bt.stat("last_path"), eq, ev, int(ok.sum()), B0))
            assert eq < 1e-6, warm                                    # test_gpu_parity.ROLLOUT_Q_TOL
            assert ev < 10 * QDOT_TOL, warm
            assert np.abs(got["ee_target"] - ref["ee_target"]).max() < 1e-15
            assert np.abs(got["grip_trace"] - ref["grip_trace"])[:, ok].max() < 1e-6, warm
            assert (got["q"][:, 3:7] == imu).all()
            if not warm:
                assert (got["iters"][ok] - ref["iters"][ok]).__abs__().max() <= 2 * K
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 4. the state gradient
GRAD_SEED = 26           # 7 instances are few: of the seeds 11 .. 26 the first at which every batch below holds at least 2 active bounds of the regular
                         # and of the flipped zone in the oracle's solutions (3 and more at this one; measured with the oracle alone)


@functools.lru_cache(maxsize=None)
def _grad_problem(shape, cfg_name, compat, seed=GRAD_SEED):
    names, B = tgq.SHAPES[shape]
    models = [tgp._model(n) for n in names]
    cfgs = [dc.config(cfg_name, m, compat) for m in models]
    mid = None if len(models) == 1 else (np.arange(B) % len(models)).astype(np.int32)
    parts = [common.damper_tick_inputs(m, c, B, seed + i, with_rot=True) for i, (m, c) in enumerate(zip(models, cfgs))]
    d = parts[0] if mid is None else pc.merge(parts, mid)
    rng = np.random.default_rng(seed + 3)
    rows = tgp._random_rows(tgp._rows_of(cfgs, mid, B), seed + 5)
    v = gc.task_space_v(models, cfgs, mid, d, rng)
    return models, cfgs, d, mid, rows, v


@pytest.mark.parametrize("compat", dc.MAPS)
@pytest.mark.parametrize("cfg_name", ["c3", "full"])
@pytest.mark.parametrize("shape", list(tgq.SHAPES))
@pe.stops_at_a_device_fault
def test_state_gradient_parity_with_bounds_in_every_zone(shape, cfg_name, compat):
    """wbc_tick_vjp_state (gq_damper: the derivative branch by branch) on damper_tick_inputs, both gradq variants, against
    gradq_common.restate at test_gpu_tick_grad_q's PARITY_BOUND; the sensitivities come from the device's certificate of its own tick, and
    the batch holds active regular-zone and flipped-zone bounds (the un-flipped and the flipped derivative) and clamped ones (derivative 0)"""
    models, cfgs, d, mid, rows, v = _grad_problem(shape, cfg_name, compat)
    B = len(rows)
    bt = tgp._handle(models, cfgs, B, {})
    try:
        got = bt.tick_grad_q(d, DT, v, task_params=rows)
        assert bt.stat("last_gradq_variant") == (0 if shape == "b7" else 1 << 32)
        ref, bad = tgq._reference(models, cfgs, mid, d, rows, got)
        assert bad.sum() <= B // 2, "too few solved and certified instances to call this a parity test: %d of %d" % (B - bad.sum(), B)
        ms, cs, pid = common.per_instance_configs(models, cfgs, mid, rows)
        asm = oracle.assemble(ms, cs, dict(d, model_id=pid), DT, B)
        zone, active = dc.zones_and_active(models, cfgs, mid, d["q"], asm, dict(qdot=got["qdot"], status=np.where(bad, 1, 0)))
        weighed = active & (got["sens_bounds"] != 0)[:, :, None]
        n_reg, n_flip = int((weighed & (zone == REG)).sum()), int((weighed & (zone == FLIP)).sum())
        vm = np.stack([np.array([c.damper_vmax[i] for i in range(26)]) for c in cfgs])[np.zeros(B, int) if mid is None else mid]
        clamped = int(((zone[~bad] == BEYOND) & (np.stack([asm["lb"] == -vm, asm["ub"] == vm], axis=2))[~bad]).sum())
        names = ["d_q"] + (["d_trunk_box_center"] if cfgs[0].con_trunk else [])
        for k in names:
            ratio = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
            print("%s / %s / %s: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e); weighed active bounds: %d regular, %d flipped; clamped in a zone: %d; "
                  "%d of %d solved and certified" % (shape, cfg_name, MAP_NAME[compat], k, ratio, np.abs(ref[k]).max(), n_reg, n_flip, clamped, B - bad.sum(), B))
            assert ratio <= tgq.PARITY_BOUND, (k, ratio)
            assert (got[k][bad] == 0).all()
        assert n_reg >= 1 and n_flip >= 1 and clamped >= 1
    finally:
        bt.close()
