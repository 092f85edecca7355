"""wbc_step_vjp on the device: dL/d(q, qdot, foot targets) of the state step between two ticks (csrc/wbc_k_stepvjp.hip), held to the numpy
restatement wbc_workload.step_gradients, and its behaviour at the boundary: bad rows among good ones, guarded device buffers in place,
refusals, graph capture, the torch layers wbc_step / wbc_rollout on top of it, and K ticks end to end against central differences of the
oracle's chain.

Parity bound: every output within PARITY_BOUND x max(1, max|ref|) of the restatement, the project's 1e-11 for the two other VJP kernels."""
import copy
import json
import os

import numpy as np
import pytest

import common
import gradq_common as gq
import oracle
import step_common as sc
import test_gpu_task_params as tgp
import test_step_grad_host as th
import test_tick_grad_q_host as tq
import wbc_capi as capi
import wbc_model
import wbc_workload
from test_gpu_parity import ROLLOUT_Q_TOL

pytestmark = pytest.mark.gpu

PARITY_BOUND = 1e-11
SHAPES = {"b1": (["a1_wx200"], 1), "b5": (["a1_wx200"], 5), "mixed67": (sc.MODELS, 67)}
DTS = (0.0005, 0.002, 0.02)
OUTS = tuple(capi.STEP_GRAD_FIELDS)


def _handle(names, B, cfg_name="c3"):
    models = [tgp._model(n) for n in names]
    cfgs = [common.config(cfg_name, m) for m in models]
    mid = None if len(models) == 1 else (np.arange(B) % len(models)).astype(np.int32)
    return models, mid, tgp._handle(models, cfgs, B, {})


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _call(bt, p, g, dt, mid, mode, **kw):
    return bt.step_vjp(p["q"], p["qdot"], p["foot_targets"], g, dt, imu=p["imu"], model_id=mid, mode=mode, **kw)


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_with_the_restatement(shape, variant):
    names, B = SHAPES[shape]
    models, mid, bt = _handle(names, B)
    mode = sc.mode_of(variant)
    nv = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
    beyond = np.arange(26)[None, :] >= nv[:, None]
    worst = {k: 0.0 for k in OUTS}
    for dt in DTS:
        for it, t in enumerate(sc.LADDER):
            p = sc.step_problem(models, mid, B, 100 * it + 11, dt, t, variant)
            g = np.random.default_rng(it + 5).normal(0, 1.0, (B, 26))    # (columns >= nv carry values the kernel must not read)
            got = _call(bt, p, g, dt, mid, mode)
            assert bt.stat("last_stepvjp_variant") == (0 if len(models) == 1 else 1 << 32)     # variant_key(ROT)
            assert (got["grad_status"] == 0).all()
            ref = sc.restate_step(models, mid, p, g, dt, mode)
            for k in OUTS:
                ratio = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
                worst[k] = max(worst[k], ratio)
                assert ratio <= PARITY_BOUND, "%s / %s / dt %g / |w| dt %g: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e)" % (
                    shape, variant, dt, t, k, ratio, np.abs(ref[k]).max())
            # the exact zeros
            assert not got["d_q"][beyond].view(np.uint64).any() and not got["d_qdot"][beyond].view(np.uint64).any()
            assert (got["d_foot_targets"][:, 4] == 0).all()
            if mode == sc.RUNNING:
                assert (got["d_q"][:, 0:3] == 0).all() and (got["d_qdot"][:, 0:3] == 0).all()
                if variant == "running_imu":
                    assert (got["d_q"][:, 3:6] == 0).all() and (got["d_qdot"][:, 3:6] == 0).all()
            else:
                assert (got["d_foot_targets"] == 0).all()
            assert np.abs(got["d_q"]).max() > 0 and np.abs(got["d_qdot"]).max() > 0
    print("%s / %s: %d calls; worst max|dev - ref| / max(1, max|ref|): %s" % (
        shape, variant, len(DTS) * len(sc.LADDER), ", ".join("%s %.2e" % (k, v) for k, v in worst.items())))
    bt.close()


def test_bad_rows_among_good_ones():
    """a non-finite value in q, qdot, g, a foot target that is read and the IMU row each give all-zero rows and WBC_GRAD_NONFINITE; every
    other instance is bitwise unchanged; a non-finite gripper target (row 4: not read) changes nothing"""
    B = 7
    models, mid, bt = _handle(["a1_wx200"], B)
    p = sc.step_problem(models, None, B, 17, 0.002, 3e-2, "running_imu")
    g = np.random.default_rng(1).normal(0, 1.0, (B, 26))
    good = _call(bt, p, g, 0.002, None, sc.RUNNING)
    assert (good["grad_status"] == 0).all()
    bad = {k: (None if v is None else v.copy()) for k, v in p.items()}
    g2 = g.copy()
    bad["q"][1, 9] = np.nan
    bad["qdot"][2, 4] = np.inf
    g2[3, 20] = np.nan
    bad["foot_targets"][4, 1, 2] = -np.inf
    bad["imu"][5, 0] = np.nan
    bad["foot_targets"][6, 4, 0] = np.nan
    got = _call(bt, bad, g2, 0.002, None, sc.RUNNING)
    expect = np.zeros(B, np.int32)
    expect[1:6] = capi.GRAD_NONFINITE
    assert np.array_equal(got["grad_status"], expect)
    for k in OUTS:
        assert not got[k][1:6].view(np.uint64).any(), k
        assert _same(got[k][[0, 6]], good[k][[0, 6]]), k
    bt.close()


def test_device_buffers_in_place_under_guards():
    """device pointers in place at B not a multiple of 4: pattern guard rows around the outputs, NaN guard rows around every float input; the
    guards come back intact, the inputs byte for byte, the results are the host call's; all outputs together and each alone"""
    import torch
    import devguard as dg
    B = 7
    models, mid, bt = _handle(sc.MODELS, B)
    p = sc.step_problem(models, mid, B, 19, 0.002, 1e-3, "running_imu")
    o = sc.step_problem(models, (np.arange(2 * dg.G) % len(models)).astype(np.int32), 2 * dg.G, 23, 0.002, 1e-3, "running_imu")   # guard rows: another valid batch
    g = np.random.default_rng(2).normal(0, 1.0, (B, 26))
    host = _call(bt, p, g, 0.002, mid, sc.RUNNING)
    ins = dict(q=p["q"], qdot=p["qdot"], foot_targets=p["foot_targets"], imu=p["imu"], g=g, model_id=mid)
    oth = dict(q=o["q"], qdot=o["qdot"], foot_targets=o["foot_targets"], imu=o["imu"], g=o["qdot"], model_id=np.zeros(2 * dg.G, np.int32))
    stream = torch.cuda.Stream()
    for subset in (OUTS + ("grad_status",), ("d_q",), ("d_qdot",), ("d_foot_targets",)):
        sess = dg.Session("nan", stream)
        dev = sess.put_all(ins, oth)
        out = {k: (sess.out((B,), np.int32) if k == "grad_status" else sess.out((B,) + capi.STEP_GRAD_FIELDS[k])) for k in subset}
        sess.run(lambda: bt.step_vjp(dev["q"], dev["qdot"], dev["foot_targets"], dev["g"], 0.002, imu=dev["imu"], model_id=dev["model_id"],
                                     mode=sc.RUNNING, out=out))
        sess.check("step_vjp %s" % (subset,))
        res = dg.to_host(out)
        for k in res:
            assert dg.same_bytes(res[k], host[k]), (subset, k)
    bt.close()


def _deep_wx200():
    """a1_wx200 with the arm hung off a calf: tree depth 9, past the packed whole-tree schedule's 7"""
    with open(os.path.join(wbc_model.MODELS_DIR, "a1_wx200.json")) as f:
        data = copy.deepcopy(json.load(f))
    names = [j["name"] for j in data["joints"]]
    data["joints"][names.index("waist")]["parent"] = names.index("FL_calf_joint")
    data["name"] = "a1_wx200_deep"
    return wbc_model.Model(data, dict(wbc_model.A1_ROLES))


def test_refusals():
    B = 7
    models, mid, bt = _handle(["a1_wx200"], B)
    p = sc.step_problem(models, None, B, 17, 0.002, 3e-2, "running")
    g = np.ones((B, 26))

    def outs():
        return dict(d_q=np.full((B, 26), 7.0), grad_status=np.full(B, 7, np.int32))
    for kw, word in ((dict(qdot=None), "qdot"), (dict(foot_targets=None), "foot_targets"), (dict(g=None), "g_q_new"), (dict(mode=2), "mode"),
                     (dict(mode=-1), "mode")):
        a = dict(qdot=p["qdot"], foot_targets=p["foot_targets"], g=g, mode=sc.RUNNING)
        a.update(kw)
        o = outs()
        with pytest.raises(capi.WbcError) as e:
            bt.step_vjp(p["q"], a["qdot"], a["foot_targets"], a["g"], 0.002, mode=a["mode"], out=o)
        assert e.value.code == capi.E_ARG and word in str(e.value), (word, str(e.value))
        assert (o["d_q"] == 7.0).all() and (o["grad_status"] == 7).all()
    # q_cur and out NULL: below the wrapper
    rc = bt.lib.wbc_step_vjp(bt._h, B, None, p["qdot"].ctypes.data, p["foot_targets"].ctypes.data, None, None, 0.002, 0, g.ctypes.data,
                             capi.MEM_HOST, None, None)
    assert rc == capi.E_ARG and "out" in bt.lib.wbc_last_error().decode()
    og = capi.WbcStepGrad()
    import ctypes as C
    rc = bt.lib.wbc_step_vjp(bt._h, B, None, p["qdot"].ctypes.data, p["foot_targets"].ctypes.data, None, None, 0.002, 0, g.ctypes.data,
                             capi.MEM_HOST, C.byref(og), None)
    assert rc == capi.E_ARG and "q_cur" in bt.lib.wbc_last_error().decode()
    # dt: the rule of a forward step, before any launch
    for dt in (0.0, -0.002, np.inf, np.nan, 5e-324):
        o = outs()
        with pytest.raises(capi.WbcError) as e:
            bt.step_vjp(p["q"], p["qdot"], p["foot_targets"], g, dt, out=o)
        assert e.value.code == capi.E_ARG and "dt" in str(e.value), (dt, str(e.value))
        assert (o["d_q"] == 7.0).all() and (o["grad_status"] == 7).all()
    bt.close()
    # model_id missing with several models
    models, mid, bt = _handle(["a1_wx200", "a1_px100_pin_ver"], B)
    with pytest.raises(capi.WbcError) as e:
        bt.step_vjp(p["q"], p["qdot"], p["foot_targets"], g, 0.002)
    assert e.value.code == capi.E_ARG and "model_id" in str(e.value)
    bt.close()
    # a model that does not fit the packed whole-tree schedule
    deep = _deep_wx200()
    bt = tgp._handle([deep], [common.config("c3", deep)], B, {})
    with pytest.raises(capi.WbcError) as e:
        bt.step_vjp(p["q"], p["qdot"], p["foot_targets"], g, 0.002)
    assert e.value.code == capi.E_UNSUPPORTED and "whole-tree" in str(e.value), str(e.value)
    bt.close()


def test_capture_and_replay_give_the_same_bits():
    import torch
    B = 67
    models, mid, bt = _handle(sc.MODELS, B)
    p = sc.step_problem(models, mid, B, 29, 0.002, 1e-3, "running")
    g = np.random.default_rng(3).normal(0, 1.0, (B, 26))
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(q=p["q"], qdot=p["qdot"], ft=p["foot_targets"], g=g, mid=mid).items()}
    out = {k: torch.empty((B,) + s, dtype=torch.float64, device="cuda") for k, s in capi.STEP_GRAD_FIELDS.items()}
    out["grad_status"] = torch.empty(B, dtype=torch.int32, device="cuda")

    def call():
        bt.step_vjp(dev["q"], dev["qdot"], dev["ft"], dev["g"], 0.002, model_id=dev["mid"], out=out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                           # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first = {k: v.cpu().numpy().copy() for k, v in out.items()}
    host = _call(bt, p, g, 0.002, mid, sc.RUNNING)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        call()
    for v in out.values():
        v.fill_(3)
    gr.replay()
    torch.cuda.synchronize()
    for k in out:
        assert _same(out[k].cpu().numpy(), first[k]) and _same(first[k], host[k]), k
    assert np.abs(first["d_q"]).max() > 0
    bt.close()


# ---- the torch layers
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_torch_step_backward_is_the_calls_by_hand(variant):
    import torch
    import wbc_torch
    B = 67
    models, mid, bt = _handle(sc.MODELS, B)
    mode = sc.mode_of(variant)
    p = sc.step_problem(models, mid, B, 31, 0.002, 1e-3, variant)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    q, x, ft = T(p["q"]).requires_grad_(True), T(p["qdot"]).requires_grad_(True), T(p["foot_targets"]).requires_grad_(True)
    imu, midd, rho = T(p["imu"]), T(mid), T(p["rho"])
    q_new = wbc_torch.wbc_step(q, x, ft, imu, 0.002, bt, mode, midd)
    hand = bt.integrate(p["q"], p["qdot"], 0.002, model_id=mid)
    if mode == sc.RUNNING:
        hand = bt.update_state(p["q"], hand, p["foot_targets"], imu=p["imu"], model_id=mid)
    assert _same(q_new.detach().cpu().numpy(), hand)
    (q_new * rho).sum().backward()
    g = wbc_workload.raw_to_tangent(hand, p["rho"])
    s = _call(bt, p, g, 0.002, mid, mode)
    assert _same(q.grad.cpu().numpy(), wbc_workload.tangent_to_raw(p["q"], s["d_q"]))
    assert _same(x.grad.cpu().numpy(), s["d_qdot"]) and _same(ft.grad.cpu().numpy(), s["d_foot_targets"])
    assert np.abs(s["d_q"]).max() > 0
    bt.close()


def _dev(d):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


@pytest.mark.parametrize("cfg_name,K,stepped", [("c3", 3, False), ("everything", 5, True)])
def test_torch_rollout_forward_is_the_rollout(cfg_name, K, stepped):
    import torch
    import wbc_torch
    B = 16
    m = tgp._model("a1_wx200")
    cfg = common.config(cfg_name, m)
    d = common.tick_inputs(m, cfg, B, seed=7, with_rot=True)
    step = np.random.default_rng(4).normal(0, 2e-4, (B, 5, 3)) if stepped else None
    bt = tgp._handle([m], [cfg], B, {})
    ref = oracle.rollout([m], [cfg], d, tq.DT, B, K, ee_target_step=step, nthreads=8)
    fused = bt.rollout(d, tq.DT, K, ee_target_step=step, want_trace=False)
    dev = _dev(d)
    q, qdot, st, states = wbc_torch.wbc_rollout(dev["q"], None, None, None, None, None, None, None, None, dev, tq.DT, K, bt,
                                                ee_target_step=None if step is None else torch.from_numpy(step).cuda())
    q, st = q.cpu().numpy(), st.cpu().numpy()
    assert len(states) == K and np.array_equal(st, fused["status"]) and np.array_equal(st, ref["status"])
    ok = st == 0
    assert ok.sum() >= B - B // 4
    print("%s, K = %d: max|q - fused| %.2e, max|q - oracle| %.2e" % (cfg_name, K, np.abs(q - fused["q"])[ok].max(), np.abs(q - ref["q"])[ok].max()))
    assert np.abs(q - fused["q"])[ok].max() < ROLLOUT_Q_TOL and np.abs(q - ref["q"])[ok].max() < ROLLOUT_Q_TOL
    assert np.abs(qdot.cpu().numpy() - fused["qdot"])[ok].max() < tgp.QDOT_TOL
    bt.close()


# ---- end to end: K ticks through wbc_rollout against central differences of the oracle's chain (test_step_grad_host.py's tolerance and cap)
_SWEEPS = {}


def _sweep(cfg_name, seed):
    """the oracle chain and the host reverse sweep of a case, computed once and shared"""
    if (cfg_name, seed) not in _SWEEPS:
        m, cfg, d, rho, direc = th.sweep_setup(cfg_name, seed)
        states, ticks, sides0, status = sc.chain(m, cfg, d, th.K_TICKS, tq.DT)
        assert all((s == 0).all() for s in status)
        _SWEEPS[cfg_name, seed] = (m, cfg, d, rho, direc, sides0, sc.reverse_sweep(m, cfg, states, rho, tq.DT))
    return _SWEEPS[cfg_name, seed]


def _device_gradients(m, cfg, d, rho):
    """wbc_rollout(...).backward() of rho . raw q_K -> (dL/dq0 raw, dL/d ee_target, dL/d task_params), numpy"""
    import torch
    import wbc_torch
    B = len(rho)
    bt = tgp._handle([m], [cfg], B, {})
    dev = _dev(d)
    rest = {k: v for k, v in dev.items() if k not in ("q", "ee_target")}
    q0 = dev["q"].clone().requires_grad_(True)
    ee = dev["ee_target"].clone().requires_grad_(True)
    tp = torch.from_numpy(wbc_model.task_params(cfg, B)).cuda().requires_grad_(True)
    q, _, st, _ = wbc_torch.wbc_rollout(q0, tp, ee, None, None, None, None, None, None, rest, tq.DT, th.K_TICKS, bt)
    assert (st == 0).all()
    (q * torch.from_numpy(rho).cuda()).sum().backward()
    res = q0.grad.cpu().numpy(), ee.grad.cpu().numpy(), tp.grad.cpu().numpy()
    bt.close()
    return res


@pytest.mark.parametrize("cfg_name,seed", [("full", 3), ("full", 4), ("everything", 4)])
def test_rollout_backward_against_central_differences_of_the_oracle_chain(cfg_name, seed):
    m, cfg, d, rho, direc, sides0, sw = _sweep(cfg_name, seed)
    B = len(rho)
    g_q0, g_ee, g_tp = _device_gradients(m, cfg, d, rho)
    what = "%s / seed %d, K = %d" % (cfg_name, seed, th.K_TICKS)
    # ---- dL/dq0
    tang = wbc_workload.raw_to_tangent(d["q"], g_q0)
    print("%s: max|device d_q0 - host sweep| %.3e at max|d_q0| %.3e" % (what, np.abs(tang - sw["d_q0"]).max(), np.abs(sw["d_q0"]).max()))
    keep, ok, line, _ = th.chain_directional(m, cfg, d, rho, th.K_TICKS, lambda s: dict(d, q=gq.step([m], d["q"], s * direc)), sides0, sw["margin"],
                                             sw["kappa"], (tang * direc).sum(axis=1), np.abs(tang * direc).sum(axis=1), what + ", d_q0")
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line
    # ---- dL/d ee_target (the estimator's d_foot_targets, the task rows, and prev_ee_target across ticks) and dL/d task_params
    rng = np.random.default_rng(seed + 77)
    dE = rng.choice([-1.0, 1.0], (B, 5, 3)) * rng.uniform(0.5, 1.0, (B, 5, 3))
    print("%s: max|device d_ee_target - host sweep| %.3e at max %.3e" % (what, np.abs(g_ee - sw["d_ee_target"]).max(), np.abs(sw["d_ee_target"]).max()))
    keep, ok, line, _ = th.chain_directional(m, cfg, d, rho, th.K_TICKS, lambda s: dict(d, ee_target=d["ee_target"] + s * dE), sides0, sw["margin"],
                                             sw["kappa"], (g_ee * dE).sum(axis=(1, 2)), np.abs(g_ee * dE).sum(axis=(1, 2)), what + ", d_ee_target")
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line
    rows = wbc_model.task_params(cfg, B)
    dT = rows * rng.choice([-1.0, 1.0], rows.shape) * rng.uniform(0.5, 1.0, rows.shape)
    print("%s: max|device d_task_params - host sweep| %.3e at max %.3e" % (what, np.abs(g_tp - sw["d_task_params"]).max(), np.abs(sw["d_task_params"]).max()))
    keep, ok, line, _ = th.chain_directional(m, cfg, d, rho, th.K_TICKS, lambda s: dict(d, task_params=rows + s * dT), sides0, sw["margin"],
                                             sw["kappa"], (g_tp * dT).sum(axis=1), np.abs(g_tp * dT).sum(axis=1), what + ", d_task_params")
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line
