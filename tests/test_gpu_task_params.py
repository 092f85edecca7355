"""Per-instance task weights and gains (wbc_tick_tp / wbc_assemble_tp / wbc_rollout_tp) on the device.

The per-instance reference is the oracle called with B (model, configuration) pairs and model_id = arange(B), each configuration carrying
that instance's row. Rows copied from the handle's configuration must give what the call without rows gives, on every kernel path."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import common
import oracle
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
QDOT_TOL = 1e-5
S = wbc_model.TASK_PARAMS_SLICES


def _rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
            [-sp, cp * sr, cp * cr]]


def _rotated_wx200():
    """the rotated-placement a1_wx200 variant of test_gpu_rotated_placement.py (the packed kernels' ROT instantiations)"""
    with open(os.path.join(wbc_model.MODELS_DIR, "a1_wx200.json")) as f:
        data = copy.deepcopy(json.load(f))
    for name, rpy in (("elbow", (3.14, 0, 0)), ("wrist_rotate", (-3.14, 0, 0)), ("left_finger", (0.3, -0.2, 0.1))):
        next(j for j in data["joints"] if j["name"] == name)["placement_R"] = _rpy(*rpy)
    data["name"] = "a1_wx200_rotated"
    return wbc_model.Model(data, dict(wbc_model.A1_ROLES))


_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = _rotated_wx200() if name == "rot" else wbc_model.load_model(name)
    return _MODELS[name]


def _problem(model_names, cfg_name, B, seed, with_rot=False):
    """-> (models, cfgs, inputs, model_id or None): one model, or several interleaved instance by instance"""
    models = [_model(n) for n in model_names]
    cfgs = [common.config(cfg_name, m) for m in models]
    if len(models) == 1:
        return models, cfgs, common.tick_inputs(models[0], cfgs[0], B, seed=seed, with_rot=with_rot), None
    mid = (np.arange(B) % len(models)).astype(np.int32)
    parts = [common.tick_inputs(m, c, B, seed=seed + i, with_rot=with_rot) for i, (m, c) in enumerate(zip(models, cfgs))]
    d = {}
    for k in parts[0]:
        v = parts[0][k].copy()
        for i in range(1, len(parts)):
            v[mid == i] = parts[i][k][mid == i]
        d[k] = v
    d["model_id"] = mid
    return models, cfgs, d, mid


def _rows_of(cfgs, mid, B):
    """rows copied from each instance's own model's configuration"""
    rows = np.stack([wbc_model.task_params(c, 1)[0] for c in cfgs])
    return rows[np.zeros(B, int) if mid is None else mid].copy()


def _random_rows(rows, seed, w=(0.1, 10.0), g=(0.25, 4.0)):
    """weight diagonals and scalar weights x log-uniform [0.1, 10], gains and joint_w x log-uniform [0.25, 4] (by default)"""
    rng = np.random.default_rng(seed)
    out = rows.copy()
    B = len(rows)
    for f in ("ee_W", "ee_w", "trunk_W", "trunk_w", "com_W"):
        n = S[f].stop - S[f].start
        out[:, S[f]] *= np.exp(rng.uniform(np.log(w[0]), np.log(w[1]), (B, n)))
    for f in ("ee_gain", "trunk_gain", "com_gain", "joint_w"):
        n = S[f].stop - S[f].start
        out[:, S[f]] *= np.exp(rng.uniform(np.log(g[0]), np.log(g[1]), (B, n)))
    return out


def _kappa(H):
    ev = np.linalg.eigvalsh(H)
    return ev[:, -1] / np.maximum(ev[:, 0], 1e-300)


def _qdot_tol(models, cfgs, mid, d, ms, cs, pid, B):
    """Per instance: the parity tests' q̇ tolerance at the configuration's conditioning, widened by how much worse the instance's rows
    condition H = A'A. (Random weights in [0.1, 10] and joint_w down to a quarter move cond(H) from the presets' ~3e9 up to ~1e14 on the
    sim3 switch set, whose only task is the Grip: two correct fp64 solvers then agree to ~cond x eps, not to 1e-5.)"""
    k0 = _kappa(oracle.assemble(models, cfgs, d, DT, B)["H"])
    k1 = _kappa(oracle.assemble(ms, cs, dict(d, model_id=pid), DT, B)["H"])
    ratio = np.maximum(1.0, k1 / k0)
    return QDOT_TOL * ratio, ratio


def _check_qdot(got, ref, tol, ratio, what):
    ok = ref["status"] == 0
    err = np.abs(got["qdot"] - ref["qdot"]).max(axis=1)
    plain = ok & (ratio <= 1.0)
    print("%s: qdot max-abs err vs oracle %.3e (%.3e where the rows do not worsen cond(H): %d instances); widest widening x%.1e, worst err / tol %.3f" % (
        what, err[ok].max(), err[plain].max(initial=0.0), int(plain.sum()), ratio[ok].max(), (err / tol)[ok].max()))
    assert (err[ok] <= tol[ok]).all() and err[ok].max() < 1e-2
    assert err[plain].max(initial=0.0) < QDOT_TOL


def _per_instance(models, cfgs, mid, rows):
    """the oracle's form of per-instance rows: B (model, configuration) pairs, model_id = arange(B)"""
    B = len(rows)
    off = capi.WbcConfig.ee_W.offset
    ms, cs = [], []
    for b in range(B):
        i = 0 if mid is None else int(mid[b])
        c = capi.WbcConfig.from_buffer_copy(cfgs[i])
        C.memmove(C.addressof(c) + off, rows[b].ctypes.data, 85 * 8)
        ms.append(models[i])
        cs.append(c)
    return ms, cs, np.arange(B, dtype=np.int32)


def _handle(models, cfgs, B, options):
    bt = WbcBatch(models, B)
    for i, c in enumerate(cfgs):
        bt.configure(c, i)
    for k, v in options.items():
        bt.set_option(k, v)
    return bt


# (models, configuration, B, options, orientation references, last_path of the call without rows)
CASES = {
    "c1": (["a1_wx200"], "c1", 1, {}, False, 2),
    "c3": (["a1_wx200"], "c3", 4096, {}, False, 2),
    "c3_trunk": (["a1_wx200"], "c3_trunk_task", 1024, {}, True, 2),
    "c3_mani": (["a1_wx200"], "c3_mani", 512, {}, False, 2),
    "c3_hybrid": (["a1_wx200"], "c3_hybrid", 1024, {}, False, 2),
    "c2": (["a1_wx200"], "c2", 4096, {"packed_orth": 2}, False, 3),
    "everything_orthp": (["a1_wx200"], "everything", 1024, {"packed_orth": 2}, True, 3),
    "everything": (["a1_wx200"], "everything", 1024, {}, True, 0),
    "full": (["a1_wx200"], "full", 1024, {}, True, 4),
    "rot_c3": (["rot"], "c3", 4096, {}, False, 2),
    "rot_c2": (["rot"], "c2", 1024, {"packed_orth": 2}, False, 3),
    "rot_full": (["rot"], "full", 1024, {}, True, 4),
    "laikago_c3": (["laikago_vx300"], "c3", 4096, {}, False, None),
    "mixed_c3": (["a1_wx200", "a1_px100_pin_ver"], "c3", 4096, {}, False, 2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_rows_of_the_configuration_change_nothing(case):
    """Rows copied from the handle's configuration: the same status, iteration count, qdot and working set as the call without rows, on the same path."""
    names, cfg_name, B, opts, with_rot, path = CASES[case]
    models, cfgs, d, mid = _problem(names, cfg_name, B, seed=21, with_rot=with_rot)
    bt = _handle(models, cfgs, B, opts)
    plain = bt.tick(d, DT, want_q_next=True, want_working_set=True)
    p0 = bt.stat("last_path")
    if path is not None:
        assert p0 == path
    rows = _rows_of(cfgs, mid, B)
    got = bt.tick(d, DT, want_q_next=True, want_working_set=True, task_params=rows)
    assert bt.stat("last_path") == p0
    assert (got["status"] == plain["status"]).all() and (got["iters"] == plain["iters"]).all()
    assert (got["working_set"] == plain["working_set"]).all()
    err = np.abs(got["qdot"] - plain["qdot"]).max()
    print("%s: path %d, rows = configuration: qdot max-abs diff %.3e (bit-identical: %s)" % (
        case, p0, err, bool((got["qdot"] == plain["qdot"]).all() and (got["q_next"] == plain["q_next"]).all())))
    assert err <= 1e-12 and np.abs(got["q_next"] - plain["q_next"]).max() <= 1e-12
    # warm start (the WARM instantiations): seeded with the set just returned
    d2 = dict(d, working_set=plain["working_set"])
    pw = bt.tick(d2, DT, want_working_set=True)
    gw = bt.tick(d2, DT, want_working_set=True, task_params=rows)
    assert (gw["status"] == pw["status"]).all() and (gw["iters"] == pw["iters"]).all() and (gw["working_set"] == pw["working_set"]).all()
    assert np.abs(gw["qdot"] - pw["qdot"]).max() <= 1e-12
    bt.close()


@pytest.mark.parametrize("case", ["c3", "c3_trunk", "c3_hybrid", "c2", "everything_orthp", "everything", "full", "rot_c3", "laikago_c3",
                                  "mixed_c3"])
def test_random_rows_match_the_oracle(case):
    names, cfg_name, _, opts, with_rot, path = CASES[case]
    B = 4096
    models, cfgs, d, mid = _problem(names, cfg_name, B, seed=31, with_rot=with_rot)
    rows = _random_rows(_rows_of(cfgs, mid, B), seed=5)
    ms, cs, pid = _per_instance(models, cfgs, mid, rows)
    ref = oracle.tick(ms, cs, dict(d, model_id=pid), DT, B, nthreads=8)
    bt = _handle(models, cfgs, B, opts)
    bt.tick(d, DT)
    p0 = bt.stat("last_path")
    got = bt.tick(d, DT, want_q_next=True, task_params=rows)
    assert bt.stat("last_path") == p0
    assert (got["status"] == ref["status"]).mean() == 1.0
    ok = ref["status"] == 0
    assert ok.mean() > 0.8
    tol, ratio = _qdot_tol(models, cfgs, mid, d, ms, cs, pid, B)
    _check_qdot(got, ref, tol, ratio, "%s: path %d, random rows" % (case, p0))
    assert (np.abs(got["q_next"] - ref["q_next"]).max(axis=1) <= tol * DT + 1e-9)[ok].all()
    assert np.abs(got["qdot"][~ok]).max(initial=0.0) == 0.0
    if case in ("c3", "everything", "mixed_c3"):     # wbc_assemble_tp: the general kernel's task stack with the rows
        a = bt.assemble(d, DT, task_params=rows)
        ar = oracle.assemble(ms, cs, dict(d, model_id=pid), DT, B)
        for k in ("A", "b", "H", "g"):
            e = np.abs(a[k] - ar[k]).max()
            assert e < 1e-11 * max(1.0, np.abs(ar[k]).max()), (k, e)
    bt.close()


def test_the_compact_kernel_hands_rows_to_the_general_kernel():
    """With refine = 0 and packed_kernel = 0 the sim3 family runs on the one-instance compact kernel (path 1), which has no TP variant:
    a call with rows runs on the general kernel and says so."""
    m = _model("a1_wx200")
    cfg = common.config("c3", m)
    B = 1024
    d = common.tick_inputs(m, cfg, B, seed=41)
    bt = _handle([m], [cfg], B, {"refine": 0, "packed_kernel": 0})
    bt.tick(d, DT)
    assert bt.stat("last_path") == 1
    rows = _random_rows(_rows_of([cfg], None, B), seed=6)
    got = bt.tick(d, DT, task_params=rows)
    assert bt.stat("last_path") == 0
    ms, cs, pid = _per_instance([m], [cfg], None, rows)
    ref = oracle.tick(ms, cs, dict(d, model_id=pid), DT, B, nthreads=8)
    assert (got["status"] == ref["status"]).all()
    tol, ratio = _qdot_tol([m], [cfg], None, d, ms, cs, pid, B)
    _check_qdot(got, ref, tol, ratio, "compact kernel's call with rows on the general kernel")
    bt.close()


@pytest.mark.parametrize("kernel", ["sim3p", "orthp"])
def test_the_tail_uses_each_instances_own_row(kernel):
    """Instances the packed kernels redo on the general path inside the same launch (the tail) are computed with their own rows."""
    names = ["a1_wx200", "a1_px100_pin_ver"]
    B = 3000
    if kernel == "sim3p":
        models, cfgs, d, mid = _problem(names, "c3", B, seed=83)
        opts = {"presolve_tol_exp": 3, "dbg_force_defer": 1}
    else:
        models, cfgs, d, mid = _problem(names, "c2", B, seed=81)
        opts = {"packed_orth": 2, "orth_qr": 1}
    rows = _random_rows(_rows_of(cfgs, mid, B), seed=7)
    ms, cs, pid = _per_instance(models, cfgs, mid, rows)
    ref = oracle.tick(ms, cs, dict(d, model_id=pid), DT, B, nthreads=8)
    bt = _handle(models, cfgs, B, opts)
    got = bt.tick(d, DT, want_q_next=True, task_params=rows)
    n_def = bt.stat("deferred_last")
    assert bt.stat("last_path") == (2 if kernel == "sim3p" else 3)
    print("%s: %d of %d instances redone in the tail" % (kernel, n_def, B))
    assert n_def > 0 if kernel == "sim3p" else n_def == B
    assert (got["status"] == ref["status"]).all()
    tol, ratio = _qdot_tol(models, cfgs, mid, d, ms, cs, pid, B)
    _check_qdot(got, ref, tol, ratio, "%s tail" % kernel)
    bt.close()


@pytest.mark.parametrize("case", ["c3", "c3_trunk", "c3_hybrid", "c2", "everything", "full", "mixed_c3"])
def test_bad_rows_fail_alone(case):
    """A NaN in one row, joint_w = 0 in another: those instances report WBC_QP_NUMERICAL with zero qdot; every other instance — the
    wavefront neighbours of a packed group included — is what the clean run gives."""
    names, cfg_name, _, opts, with_rot, _ = CASES[case]
    B = 64
    models, cfgs, d, mid = _problem(names, cfg_name, B, seed=51, with_rot=with_rot)
    rows = _random_rows(_rows_of(cfgs, mid, B), seed=8)
    bt = _handle(models, cfgs, B, opts)
    clean = bt.tick(d, DT, want_q_next=True, task_params=rows)
    bad = rows.copy()
    bad[5, S["ee_gain"].start + 25] = np.nan
    bad[9, S["joint_w"]] = 0.0
    bad[22, S["trunk_W"].start] = np.inf
    got = bt.tick(d, DT, want_q_next=True, task_params=bad)
    hit = np.zeros(B, bool)
    hit[[5, 9, 22]] = True
    assert (got["status"][hit] == capi.QP_NUMERICAL).all()
    assert (got["qdot"][hit] == 0.0).all()
    assert (got["status"][~hit] == clean["status"][~hit]).all() and (got["iters"][~hit] == clean["iters"][~hit]).all()
    assert np.abs(got["qdot"][~hit] - clean["qdot"][~hit]).max() <= 1e-12
    assert np.abs(got["q_next"][~hit] - clean["q_next"][~hit]).max() <= 1e-12
    bt.close()


@pytest.mark.parametrize("mode", ["running", "warmup"])
def test_rollout_with_rows_matches_the_oracle(mode):
    m = _model("a1_wx200")
    B, K = 512, 50
    cfg = common.config("c3" if mode == "running" else "full", m)
    d = common.tick_inputs(m, cfg, B, seed=61, stress=False)
    rng = np.random.default_rng(3)
    step = np.zeros((B, 5, 3))
    step[:, 4] = rng.normal(0, 1e-4, (B, 3))
    imu = d["q"][:, 3:7].copy() if mode == "running" else None
    rows = _random_rows(_rows_of([cfg], None, B), seed=9, w=(0.5, 2.0), g=(0.5, 2.0))   # (50 closed-loop ticks: settings near the preset's)
    ms, cs, pid = _per_instance([m], [cfg], None, rows)
    ref = oracle.rollout(ms, cs, dict(d, model_id=pid), DT, B, K, ee_target_step=step, imu=imu, nthreads=8, running=mode == "running")
    ok = ref["status"] == 0
    assert ok.mean() > 0.8
    bt = _handle([m], [cfg], B, {})
    got = bt.rollout(d, DT, K, ee_target_step=step, imu=imu, mode=capi.ROLLOUT_RUNNING if mode == "running" else capi.ROLLOUT_WARMUP,
                     task_params=rows)
    assert (got["status"] == ref["status"]).all()
    e_q = np.abs(got["q"] - ref["q"])[ok].max()
    e_t = np.abs(got["grip_trace"] - ref["grip_trace"])[:, ok].max()
    print("rollout %s: q max-abs err %.3e, grip_trace %.3e" % (mode, e_q, e_t))
    assert e_q < 1e-6 and e_t < 1e-6
    assert np.abs(got["qdot"] - ref["qdot"])[ok].max() < 10 * QDOT_TOL
    # the rows do change the answer
    plain = bt.rollout(d, DT, K, ee_target_step=step, imu=imu, mode=capi.ROLLOUT_RUNNING if mode == "running" else capi.ROLLOUT_WARMUP)
    assert np.abs(plain["grip_trace"] - got["grip_trace"]).max() > 1e-6
    bt.close()


def test_a_sweep_equals_separate_handles():
    """K settings spread over one batch give what K handles, each configured with one setting, give."""
    m = _model("a1_wx200")
    cfg = common.config("c3", m)
    B, K = 256, 4
    d = common.tick_inputs(m, cfg, B, seed=71)
    gains = np.array([0.2, 0.5, 1.0, 2.0])
    wgrip = np.array([0.5, 1.0, 4.0, 10.0])
    setting = np.arange(B) % K
    eg = np.tile(np.ctypeslib.as_array(cfg.ee_gain).copy(), (B, 1, 1))
    eg[:, 4, :] *= gains[setting][:, None]
    ew = np.tile(np.ctypeslib.as_array(cfg.ee_w).copy(), (B, 1))
    ew[:, 4] *= wgrip[setting]
    rows = wbc_model.task_params(cfg, B, ee_gain=eg, ee_w=ew)
    bt = _handle([m], [cfg], B, {})
    got = bt.tick(d, DT, want_q_next=True, task_params=rows)
    bt.close()
    for k in range(K):
        sel = setting == k
        c = capi.WbcConfig.from_buffer_copy(cfg)
        for r in range(6):
            c.ee_gain[4][r] = cfg.ee_gain[4][r] * gains[k]
        c.ee_w[4] = cfg.ee_w[4] * wgrip[k]
        one = _handle([m], [c], int(sel.sum()), {})
        ref = one.tick({n: v[sel] for n, v in d.items()}, DT, want_q_next=True)
        one.close()
        assert (ref["status"] == got["status"][sel]).all() and (ref["iters"] == got["iters"][sel]).all()
        assert np.abs(ref["qdot"] - got["qdot"][sel]).max() <= 1e-12
        assert np.abs(ref["q_next"] - got["q_next"][sel]).max() <= 1e-12


def test_device_rows_and_graph_capture():
    """Rows in device memory are read by every call: a captured tick replays with whatever the row buffer holds at replay."""
    import torch
    m = _model("a1_wx200")
    cfg = common.config("c3", m)
    B = 1024
    d = common.tick_inputs(m, cfg, B, seed=91)
    rows0 = _rows_of([cfg], None, B)
    rows1 = _random_rows(rows0, seed=10)
    bt = _handle([m], [cfg], B, {})
    ref1 = bt.tick(d, DT, task_params=rows1)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    tpd = torch.from_numpy(rows0.copy()).cuda()
    out = dict(qdot=torch.empty((B, 26), dtype=torch.float64, device="cuda"), status=torch.empty(B, dtype=torch.int32, device="cuda"),
               iters=torch.empty(B, dtype=torch.int32, device="cuda"))
    call = bt.make_tick_call(dev, out, DT, task_params=tpd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                        # (warm-up outside the capture: lazy workspaces)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    tpd.copy_(torch.from_numpy(rows1))
    g.replay()
    torch.cuda.synchronize()
    assert (out["status"].cpu().numpy() == ref1["status"]).all()
    assert np.abs(out["qdot"].cpu().numpy() - ref1["qdot"]).max() <= 1e-12
    with pytest.raises(capi.WbcError):
        bt.tick(d, DT, task_params=tpd)               # host inputs with device rows: refused
    bt.close()
