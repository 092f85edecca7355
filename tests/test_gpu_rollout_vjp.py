"""wbc_rollout_record / wbc_rollout_vjp on the device: the recorded forward against wbc_rollout_tp byte for byte, the reverse sweep against the
numpy restatement wbc_workload.rollout_gradients fed the device's own taped states and qdot, the torch layer wbc_rollout_fused against the
chained layers wbc_rollout, K ticks end to end against central differences of the oracle's chain, bad rows among good ones under guarded
device buffers, refusals, layout, graph capture.

SWEEP_BOUND: every output block of the sweep within SWEEP_BOUND[configuration] x max(1, max|ref block|) of the restatement. Per layer the
project's device bound is 1e-11 (PARITY_BOUND); over K ticks the error passes through the same sens_x amplification as the reference, so the
K-tick bound is measured, not guessed: about 30 x the worst ratio measured (printed by the parity test), rounded to a power of ten. Measured
on MI355X: `full` 1.95e-13 (b1, K = 3) and 1.53e-13 (b16, K = 5, stepped) -> 1e-11; `everything` 3.4e-11 (b5), 3.7e-10 / 3.2e-10 (b16, stepped,
warm_start 0 / 1) and 2.3e-10 (mixed7, stepped) -> 1e-8. The same bounds hold the torch layer to the chained layers (measured 3.5e-15 on
`full`, 6.3e-11 on `everything`). c3 is in neither parity set (sens_x reaches 1e6 there, §3.40); the fused layer and the chain run the same kernels on the same
inputs and differ by the chain's forward (its ticks return working sets: other kernel variants, qdot within 1e-14) and its tangent -> raw ->
tangent round trips alone, a few eps that sens_x <= 1e6 then amplifies over three ticks: held to `everything`'s 1e-8 (measured 1.4e-9).

The record launches its ticks exactly as wbc_rollout_tp does, so the forward is the roll-out byte for byte with option warm_start 0 and 1;
the tape holds working sets under warm_start alone (a first version that asked every tick for one measured max|recorded - rollout| qdot
6.3e-15 on the packed sim3 path and 1.8e-12 on the general path with warm_start 0: other kernel variants)."""
import ctypes as C

import numpy as np
import pytest

import common
import gradq_common as gq
import oracle
import step_common as sc
import test_gpu_step_grad as tsg
import test_gpu_task_params as tgp
import test_step_grad_host as th
import test_tick_grad_q_host as tq
import wbc_capi as capi
import wbc_model
import wbc_workload
from test_gpu_parity import ROLLOUT_Q_TOL

pytestmark = pytest.mark.gpu

DT = tq.DT
SWEEP_BOUND = {"full": 1e-11, "everything": 1e-8, "c3": 1e-8}
SHAPES = {"b1": (["a1_wx200"], 1), "b5": (["a1_wx200"], 5), "b16": (["a1_wx200"], 16), "mixed7": (sc.MODELS, 7)}


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _step(B, seed):
    return np.random.default_rng(seed).normal(0, 2e-4, (B, 5, 3))


def _host(t):
    return t.cpu().numpy().copy()


# ---- 1. the forward
@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("shape,cfg_name,K,stepped", [("b1", "c3", 3, False), ("b5", "full", 3, False), ("b16", "everything", 5, True),
                                                      ("mixed7", "c3", 3, True)])
def test_recorded_forward_is_the_rollout_byte_for_byte(shape, cfg_name, K, stepped, warm):
    names, B = SHAPES[shape]
    models, cfgs, d, mid = tgp._problem(names, cfg_name, B, seed=7, with_rot=True)
    step = _step(B, 4) if stepped else None
    bt = tgp._handle(models, cfgs, B, {"warm_start": warm})
    plain = bt.rollout(d, DT, K, ee_target_step=step, want_trace=False)
    path = bt.stat("last_path")
    bt.close()
    bt = tgp._handle(models, cfgs, B, {"warm_start": warm})
    rec, tape = bt.rollout_record(d, DT, K, ee_target_step=step)
    assert bt.stat("last_path") == path
    print("%s / %s / warm_start %d (tick path %d): max|recorded - rollout| q %.3e, qdot %.3e, ee_target %.3e" % (
        shape, cfg_name, warm, path, np.abs(rec["q"] - plain["q"]).max(), np.abs(rec["qdot"] - plain["qdot"]).max(),
        np.abs(rec["ee_target"] - plain["ee_target"]).max()))
    for k in ("q", "qdot", "ee_target", "status", "iters"):
        assert _same(rec[k], plain[k]), "%s / %s / warm_start %d: %s differs from wbc_rollout_tp's" % (shape, cfg_name, warm, k)
    assert rec["q_trace"].shape == (K, B, 27) and _same(rec["q_trace"][K - 1], rec["q"])
    assert tape.buf.numel() == B * (capi.TAPE_HEAD_BYTES + K * capi.TAPE_TICK_BYTES)
    # the tape: tick 0 saw the call's inputs, tick k the state after tick k - 1; the last tick's answer is the call's
    t0, tl = tape.tick(0), tape.tick(K - 1)
    assert _same(_host(t0["q"]), d["q"]) and _same(_host(t0["ee_target"]).reshape(B, 5, 3), d["ee_target"])
    assert _same(_host(tl["qdot"]), rec["qdot"])
    for k in range(1, K):
        assert _same(_host(tape.tick(k)["q"]), rec["q_trace"][k - 1])
    if stepped:                                                          # the targets are running sums
        e = d["ee_target"].copy()
        for k in range(K):
            assert _same(_host(tape.tick(k)["ee_target"]).reshape(B, 5, 3), e)
            e = e + step
        assert _same(rec["ee_target"], e)
    assert np.array_equal(np.maximum.reduce([_host(tape.tick(k)["status"]) for k in range(K)]), rec["status"])
    bt.close()


# ---- 2. the sweep against the restatement
def _ticks_seen(cfgs, d, tape, K, step):
    """the inputs every tick saw: the tape's state and targets, the previous rotations of step_common.advance"""
    seen, cur = [], {k: v for k, v in d.items()}
    for k in range(K):
        t = {name: _host(v) for name, v in tape.tick(k).items()}
        cur = dict(cur, q=t["q"], ee_target=t["ee_target"].reshape(-1, 5, 3), prev_ee_target=t["prev_ee_target"].reshape(-1, 5, 3))
        if "trunk_target" in d:
            cur["trunk_target"], cur["prev_trunk_target"] = t["trunk_target"], t["prev_trunk_target"]
        seen.append((cur, t))
        cur = sc.advance(cfgs[0], cur, t["q"], None)
    return seen


def _restate(models, cfgs, mid, seen, seeds, imu=None, mode=capi.ROLLOUT_RUNNING, rows=None, warm=0):
    """wbc_workload.rollout_gradients for a batch of several models interleaved by model_id, on the device's own states, qdot, status and
    (warm: option warm_start, under which the tape holds them) working sets"""
    K, B = len(seen), len(seen[0][0]["q"])
    out = None
    for i, (m, c) in enumerate(zip(models, cfgs)):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        if not sel.any():
            continue
        n = int(sel.sum())
        ins = [{k: v[sel] for k, v in cur.items() if k != "model_id"} for cur, _ in seen]
        ms, cs, pid = ([m], [c], None) if rows is None else common.per_instance_configs([m], [c], None, rows[sel])   # (the oracle's form of per-instance rows)
        r = wbc_workload.rollout_gradients(
            m, c, ins, np.stack([t["qdot"][sel] for _, t in seen]), DT, gq.StateFK([m]),
            lambda dd, ms=ms, cs=cs, pid=pid, n=n: oracle.assemble(ms, cs, dd if pid is None else dict(dd, model_id=pid), DT, n),
            g_q_final=None if seeds.get("g_q_final") is None else seeds["g_q_final"][sel],
            g_qdot_last=None if seeds.get("g_qdot_last") is None else seeds["g_qdot_last"][sel],
            g_q_trace=None if seeds.get("g_q_trace") is None else seeds["g_q_trace"][:, sel], task_params=None if rows is None else rows[sel],
            imu=None if imu is None else imu[sel], mode=mode, status=np.stack([t["status"][sel] for _, t in seen]),
            working_set=np.stack([t["working_set"][sel] for _, t in seen]) if warm else None)
        if out is None:
            out = {k: np.zeros((B,) + v.shape[1:], dtype=v.dtype) for k, v in r.items()}
        for k in r:
            out[k][sel] = r[k]
    return out


def _seeds(B, K, seed, nvs):
    rng = np.random.default_rng(seed)
    s = dict(g_q_final=rng.normal(0, 1.0, (B, 26)), g_qdot_last=rng.normal(0, 1e-3, (B, 26)), g_q_trace=rng.normal(0, 1.0, (K, B, 26)))
    beyond = np.arange(26)[None, :] >= nvs[:, None]
    for k in ("g_q_final", "g_qdot_last"):
        s[k][beyond] = 0.0
    s["g_q_trace"][:, beyond] = 0.0
    return s


@pytest.mark.parametrize("shape,cfg_name,K,stepped,warm", [("b1", "full", 3, False, 0), ("b5", "everything", 3, False, 0), ("b16", "full", 5, True, 1),
                                                           ("b16", "everything", 3, True, 0), ("b16", "everything", 3, True, 1),
                                                           ("mixed7", "everything", 3, True, 0), ("mixed7", "everything", 3, True, 1)])
def test_sweep_against_the_restatement(shape, cfg_name, K, stepped, warm):
    names, B = SHAPES[shape]
    models, cfgs, d, mid = tgp._problem(names, cfg_name, B, seed=7, with_rot=True)
    step = _step(B, 4) if stepped else None
    rows = tgp._random_rows(tgp._rows_of(cfgs, mid, B), 12, w=(0.8, 1.25), g=(0.8, 1.25))
    nvs = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
    seeds = _seeds(B, K, 21, nvs)
    bt = tgp._handle(models, cfgs, B, {"warm_start": warm})
    rec, tape = bt.rollout_record(d, DT, K, ee_target_step=step, task_params=rows)
    got = bt.rollout_vjp(tape, **seeds)
    assert bt.stat("last_rollvjp_variant") == 2 << 32                   # variant_key(stage LINK)
    assert set(got) == set(bt.default_rollout_grad_wants()) | {"grad_status", "ticks_dropped"}
    ref = _restate(models, cfgs, mid, _ticks_seen(cfgs, d, tape, K, step), seeds, rows=rows, warm=warm)
    assert np.array_equal(got["ticks_dropped"], ref["ticks_dropped"]), (got["ticks_dropped"], ref["ticks_dropped"])
    assert (got["ticks_dropped"] == 0).sum() >= B - B // 4
    worst = 0.0
    for k in bt.default_rollout_grad_wants():
        ratio = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
        worst = max(worst, ratio)
        print("%s / %s, K = %d: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e)" % (shape, cfg_name, K, k, ratio, np.abs(ref[k]).max()))
    print("%s / %s, K = %d, warm_start %d: worst ratio %.3e (bound %.0e), max|sens_x| over the ticks %.3e" % (shape, cfg_name, K, warm, worst, SWEEP_BOUND[cfg_name], ref["sens_max"].max()))
    assert worst <= SWEEP_BOUND[cfg_name]
    assert np.abs(got["d_q0"]).max() > 0 and np.abs(got["d_ee_target_step"]).max() > 0
    beyond = np.arange(26)[None, :] >= nvs[:, None]
    assert not got["d_q0"][beyond].view(np.uint64).any()
    # one seed at a time, and only some outputs: the same bits as their part of the full call would have with that seed alone
    only = bt.rollout_vjp(tape, g_q_final=seeds["g_q_final"], want=("d_q0",))
    full = bt.rollout_vjp(tape, g_q_final=seeds["g_q_final"])
    assert set(only) == {"d_q0", "grad_status", "ticks_dropped"} and _same(only["d_q0"], full["d_q0"])
    bt.close()


# ---- 3. the torch layer against the chained layers
def _dev(d):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _both_backwards(m, cfg, d, K, rho_final, rho_trace, step=None):
    """-> (fused, chain): each dict(q, qdot, status, g_q0, g_ee, g_tp[, g_step]) of the loss rho_final . q_K + sum_k rho_trace[k] . q_(k+1)"""
    import torch
    import wbc_torch
    B = len(d["q"])
    bt = tgp._handle([m], [cfg], B, {})
    res = []
    for fused in (True, False):
        dev = _dev(d)
        rest = {k: v for k, v in dev.items() if k not in ("q", "ee_target")}
        q0 = dev["q"].clone().requires_grad_(True)
        ee = dev["ee_target"].clone().requires_grad_(True)
        tp = torch.from_numpy(wbc_model.task_params(cfg, B)).cuda().requires_grad_(True)
        st = None if step is None else torch.from_numpy(step).cuda().requires_grad_(True)
        fn = wbc_torch.wbc_rollout_fused if fused else wbc_torch.wbc_rollout
        q, qdot, status, states = fn(q0, tp, ee, None, None, None, None, None, None, rest, DT, K, bt, ee_target_step=st)
        after = states if fused else torch.stack([s["q"] for s in states[1:]] + [q])
        loss = (q * torch.from_numpy(rho_final).cuda()).sum() + (after * torch.from_numpy(rho_trace).cuda()).sum()
        loss.backward()
        res.append(dict(q=_host(q.detach()), qdot=_host(qdot.detach()), status=_host(status), g_q0=_host(q0.grad), g_ee=_host(ee.grad), g_tp=_host(tp.grad),
                        g_step=None if st is None else _host(st.grad)))
    bt.close()
    return res


@pytest.mark.parametrize("cfg_name,K,stepped", [("full", 3, False), ("everything", 5, True)])
def test_fused_backward_against_the_chained_layers(cfg_name, K, stepped):
    B = 16
    m = tgp._model("a1_wx200")
    cfg = common.config(cfg_name, m)
    d = common.tick_inputs(m, cfg, B, seed=7, with_rot=True)
    rng = np.random.default_rng(33)
    rho_final, rho_trace = rng.normal(0, 1.0, (B, 27)), rng.normal(0, 1.0, (K, B, 27))
    fused, chain = _both_backwards(m, cfg, d, K, rho_final, rho_trace, _step(B, 4) if stepped else None)
    ok = fused["status"] == 0
    assert np.array_equal(fused["status"], chain["status"]) and ok.sum() >= B - B // 4
    assert np.abs(fused["q"] - chain["q"])[ok].max() < ROLLOUT_Q_TOL and np.abs(fused["qdot"] - chain["qdot"])[ok].max() < tgp.QDOT_TOL
    for k in ("g_q0", "g_ee", "g_tp") + (("g_step",) if stepped else ()):
        ratio = np.abs(fused[k] - chain[k])[ok].max() / max(1.0, np.abs(chain[k][ok]).max())
        print("%s, K = %d: %s max|fused - chain| = %.3e x max(1, max|chain| = %.3e)" % (cfg_name, K, k, ratio, np.abs(chain[k][ok]).max()))
        assert ratio <= SWEEP_BOUND[cfg_name], (k, ratio)
        assert np.abs(fused[k]).max() > 0


def test_an_instance_that_goes_unsolved_is_dropped_as_the_chain_drops_it():
    """c3 / seed 3 (test_step_grad_host.py): from the second tick on a stress instance goes unsolved; the sweep and the chain agree on every
    instance, that one included"""
    m, cfg, d, rho, direc = th.sweep_setup("c3", 3)
    K, B = 3, len(rho)
    fused, chain = _both_backwards(m, cfg, d, K, rho, np.zeros((K, B, 27)))
    assert np.array_equal(fused["status"], chain["status"]) and (fused["status"] != 0).any() and (fused["status"] == 0).any()
    for k in ("g_q0", "g_ee", "g_tp"):
        ratio = np.abs(fused[k] - chain[k]).max() / max(1.0, np.abs(chain[k]).max())
        print("c3 / seed 3, K = %d: %s max|fused - chain| = %.3e x max(1, max|chain| = %.3e)" % (K, k, ratio, np.abs(chain[k]).max()))
        assert ratio <= SWEEP_BOUND["c3"], (k, ratio)


# ---- 4. end to end: test_gpu_step_grad's three cases through the new calls, its tolerance and cap unchanged
def _fused_gradients(m, cfg, d, rho):
    import torch
    import wbc_torch
    B = len(rho)
    bt = tgp._handle([m], [cfg], B, {})
    dev = _dev(d)
    rest = {k: v for k, v in dev.items() if k not in ("q", "ee_target")}
    q0 = dev["q"].clone().requires_grad_(True)
    ee = dev["ee_target"].clone().requires_grad_(True)
    tp = torch.from_numpy(wbc_model.task_params(cfg, B)).cuda().requires_grad_(True)
    q, _, st, _ = wbc_torch.wbc_rollout_fused(q0, tp, ee, None, None, None, None, None, None, rest, DT, th.K_TICKS, bt)
    assert (st == 0).all()
    (q * torch.from_numpy(rho).cuda()).sum().backward()
    res = _host(q0.grad), _host(ee.grad), _host(tp.grad)
    bt.close()
    return res


@pytest.mark.parametrize("cfg_name,seed", [("full", 3), ("full", 4), ("everything", 4)])
def test_fused_backward_against_central_differences_of_the_oracle_chain(cfg_name, seed):
    m, cfg, d, rho, direc, sides0, sw = tsg._sweep(cfg_name, seed)
    B = len(rho)
    g_q0, g_ee, g_tp = _fused_gradients(m, cfg, d, rho)
    what = "%s / seed %d, K = %d, fused" % (cfg_name, seed, th.K_TICKS)
    tang = wbc_workload.raw_to_tangent(d["q"], g_q0)
    print("%s: max|device d_q0 - host sweep| %.3e at max|d_q0| %.3e" % (what, np.abs(tang - sw["d_q0"]).max(), np.abs(sw["d_q0"]).max()))
    keep, ok, line, _ = th.chain_directional(m, cfg, d, rho, th.K_TICKS, lambda s: dict(d, q=gq.step([m], d["q"], s * direc)), sides0, sw["margin"],
                                             sw["kappa"], (tang * direc).sum(axis=1), np.abs(tang * direc).sum(axis=1), what + ", d_q0")
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line
    rng = np.random.default_rng(seed + 77)
    dE = rng.choice([-1.0, 1.0], (B, 5, 3)) * rng.uniform(0.5, 1.0, (B, 5, 3))
    keep, ok, line, _ = th.chain_directional(m, cfg, d, rho, th.K_TICKS, lambda s: dict(d, ee_target=d["ee_target"] + s * dE), sides0, sw["margin"],
                                             sw["kappa"], (g_ee * dE).sum(axis=(1, 2)), np.abs(g_ee * dE).sum(axis=(1, 2)), what + ", d_ee_target")
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line
    rows = wbc_model.task_params(cfg, B)
    dT = rows * rng.choice([-1.0, 1.0], rows.shape) * rng.uniform(0.5, 1.0, rows.shape)
    keep, ok, line, _ = th.chain_directional(m, cfg, d, rho, th.K_TICKS, lambda s: dict(d, task_params=rows + s * dT), sides0, sw["margin"],
                                             sw["kappa"], (g_tp * dT).sum(axis=1), np.abs(g_tp * dT).sum(axis=1), what + ", d_task_params")
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line


# ---- 5. bad rows among good ones, guarded device buffers in place
def test_bad_rows_among_good_ones_under_guards():
    """NaN in one instance's q0 row and in another's g_q_trace row at k = 1, B = 7 over the three models (not a multiple of 4): device pointers
    in place, pattern guard rows around every output, NaN guard rows around every float input. The guards come back intact, the inputs byte
    for byte; the neighbours are bit-identical to a run without the bad rows; the bad instances get all-zero rows and WBC_GRAD_NONFINITE"""
    import torch
    import devguard as dg
    names, B = SHAPES["mixed7"]
    K = 3
    models, cfgs, d, mid = tgp._problem(names, "everything", B, seed=7, with_rot=True)
    _, _, o, _ = tgp._problem(names, "everything", 2 * dg.G, seed=9, with_rot=True)
    o["model_id"] = np.zeros(2 * dg.G, np.int32)
    nvs = np.array([m.nv for m in models])[mid]
    seeds = _seeds(B, K, 21, nvs)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K)
    good = bt.rollout_vjp(tape, **seeds)
    ok = np.array([0, 1, 3, 5, 6])
    assert (good["grad_status"][ok] == 0).all() and (good["ticks_dropped"][ok] == 0).all()
    bad_d, bad_s = {k: v.copy() for k, v in d.items()}, {k: v.copy() for k, v in seeds.items()}
    bad_d["q"][2, 9] = np.nan
    bad_s["g_q_trace"][1, 4, 3] = np.nan
    stream = torch.cuda.Stream()
    sess = dg.Session("nan", stream)
    dev = sess.put_all(bad_d, o)
    g_final = sess.put("g_q_final", bad_s["g_q_final"], o["q"][:, :26])
    g_last = sess.put("g_qdot_last", bad_s["g_qdot_last"], o["q"][:, :26])
    g_trace = torch.from_numpy(bad_s["g_q_trace"]).cuda()              # ([K][B][26]: its leading dimension is not the batch)
    names_out = bt.default_rollout_grad_wants()
    out = {k: sess.out((B,) + capi.ROLLOUT_GRAD_FIELDS[k]) for k in names_out}
    out["grad_status"], out["ticks_dropped"] = sess.out((B,), np.int32), sess.out((B,), np.int32)
    bt.allocator = sess.alloc                                           # (what rollout_record allocates itself is guarded too)

    def call():
        r, tp = bt.rollout_record(dev, DT, K, want_trace=False)
        bt.rollout_vjp(tp, g_q_final=g_final, g_qdot_last=g_last, g_q_trace=g_trace, out=out)
        return r
    sess.run(call)
    bt.allocator = None
    sess.check("rollout_record + rollout_vjp")
    res = dg.to_host(out)
    expect = np.zeros(B, np.int32)
    expect[[2, 4]] = capi.GRAD_NONFINITE
    assert np.array_equal(res["grad_status"], expect), res["grad_status"]
    assert res["ticks_dropped"][2] == K and (res["ticks_dropped"][ok] == 0).all()
    for k in names_out:
        assert not res[k][[2, 4]].view(np.uint64).any(), k
        assert _same(res[k][ok], good[k][ok]), k
    bt.close()


# ---- 6. refusals, layout, capture
def test_refusals_name_their_field_and_come_before_any_launch():
    B, K = 5, 3
    models, cfgs, d, mid = tgp._problem(["a1_wx200"], "c3", B, seed=7, with_rot=True)
    bt = tgp._handle(models, cfgs, B, {})
    rec, tape = bt.rollout_record(d, DT, K)
    g = np.ones((B, 26))
    before = _host(tape.buf)

    def outs():
        return dict(d_q0=np.full((B, 26), 7.0), grad_status=np.full(B, 7, np.int32))

    def refused(fn, code, word):
        with pytest.raises(capi.WbcError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), (word, str(e.value))
    # record
    r = capi.WbcRollout()
    r.ticks, r.mode, r.hold_ticks = K, capi.ROLLOUT_RUNNING, 2
    keep = []
    tin = bt._tick_in(d, keep, B)
    nbytes = tape.buf.numel()

    def record(rr=r, tn=tin, ptr=tape.buf.data_ptr(), n=nbytes):
        capi.check(bt.lib.wbc_rollout_record(bt._h, B, C.byref(tn), None, DT, C.byref(rr), ptr, n, None, capi.MEM_HOST, None), bt.lib)
    refused(record, capi.E_ARG, "hold_ticks")
    r.hold_ticks = 0
    refused(lambda: record(ptr=None), capi.E_ARG, "tape")
    refused(lambda: record(n=nbytes - 1), capi.E_ARG, "tape_bytes")
    refused(lambda: bt.rollout_record(dict(d, q_con=d["q"]), DT, K), capi.E_ARG, "q_con")
    bt.synchronize()
    assert _same(_host(tape.buf), before)                                # nothing was launched
    # vjp
    refused(lambda: bt.rollout_vjp(tape, out=outs()), capi.E_ARG, "seed")
    for name, word in (("d_trunk_target", "d_trunk_target"), ("d_prev_trunk_target", "d_prev_trunk_target"), ("d_trunk_target_step", "d_trunk_target_step"),
                       ("d_com_target", "d_com_target"), ("d_com_target_vel", "d_com_target_vel"), ("d_posture_u", "d_posture_u")):
        o = outs()
        refused(lambda: bt.rollout_vjp(tape, g_q_final=g, out=dict(o, **{name: np.zeros((B,) + capi.ROLLOUT_GRAD_FIELDS[name])})), capi.E_ARG, word)
        assert (o["d_q0"] == 7.0).all() and (o["grad_status"] == 7).all()
    short = type(tape)(tape.buf[:nbytes - 8], B, K)
    short.call = tape.call
    refused(lambda: bt.rollout_vjp(short, g_q_final=g), capi.E_ARG, "tape_bytes")
    held = type(tape)(tape.buf, B, K)
    held.call = dict(tape.call, inputs=dict(d, q_con=d["q"]))
    refused(lambda: bt.rollout_vjp(held, g_q_final=g), capi.E_ARG, "q_con")
    for dt in (0.0, -0.002, np.inf, np.nan):
        held.call = dict(tape.call, dt=dt)
        refused(lambda: bt.rollout_vjp(held, g_q_final=g), capi.E_ARG, "dt")
    assert bt.lib.wbc_variant_count(b"rollvjp") == 3
    s, gsz = C.c_int32(), C.c_int32()
    assert bt.lib.wbc_rollout_grad_sizes(C.byref(s), C.byref(gsz)) == 0
    assert (s.value, gsz.value) == (C.sizeof(capi.WbcRolloutSeed), C.sizeof(capi.WbcRolloutGrad))
    bt.close()
    # MANI / HYBRID without posture_u; a model that does not fit the packed whole-tree schedule
    m = models[0]
    bt = tgp._handle([m], [common.config("c3_hybrid", m)], B, {})
    refused(lambda: bt.rollout_record(d, DT, K), capi.E_ARG, "posture_u")
    bt.close()
    deep = tsg._deep_wx200()
    bt = tgp._handle([deep], [common.config("c3", deep)], B, {})
    refused(lambda: bt.rollout_record(d, DT, K), capi.E_UNSUPPORTED, "whole-tree")
    bt.close()


def test_capture_and_replay_give_the_same_bits():
    import torch
    names, B = SHAPES["mixed7"]
    K = 3
    models, cfgs, d, mid = tgp._problem(names, "everything", B, seed=7, with_rot=True)
    nvs = np.array([m.nv for m in models])[mid]
    seeds = _seeds(B, K, 21, nvs)
    bt = tgp._handle(models, cfgs, B, {})
    rec0, tape0 = bt.rollout_record(d, DT, K)
    host = bt.rollout_vjp(tape0, **seeds)
    dev, sd = _dev(d), _dev(seeds)
    out = {k: torch.empty((B,) + s, dtype=torch.float64, device="cuda") for k, s in capi.ROLLOUT_GRAD_FIELDS.items() if k in bt.default_rollout_grad_wants()}
    out["grad_status"], out["ticks_dropped"] = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    state = {}

    def call():
        state["rec"], state["tape"] = bt.rollout_record(dev, DT, K, tape=state.get("tape"))
        bt.rollout_vjp(state["tape"], out=out, **sd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                           # (warm-up outside the capture: the workspaces get their size)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first = {k: _host(v) for k, v in out.items()}
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        call()
    for v in out.values():
        v.fill_(3)
    state["tape"].buf.fill_(0)
    gr.replay()
    torch.cuda.synchronize()
    for k in out:
        assert _same(_host(out[k]), first[k]) and _same(first[k], host[k]), k
    assert _same(_host(state["rec"]["q"]), rec0["q"]) and np.abs(first["d_q0"]).max() > 0
    bt.close()
