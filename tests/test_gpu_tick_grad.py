"""wbc_tick_vjp on the device: dL/d(task weights, gains, targets) of solved ticks (csrc/wbc_k_grad.hip), held to the numpy restatement
wbc_workload.tick_gradients fed the device's own qdot and sens_x, and its behaviour at the boundary: rows of the configuration, bad rows
among good ones, guarded device buffers in place, the WbcBatch and torch layers on top of it.

Parity bound: every output array within 1e-11 max(1, max|ref|) — what test_gpu_task_params.py holds the assembled arrays to. Measured on
MI355X over the fifteen parity cases: at most 5.4e-13 max(1, max|ref|) (mixed67 / everything; 3.8e-14 and less elsewhere). That is with
v = dL/dqdot of a loss on task-space velocities (grad_common.task_space_v). With a random v the c3 case measured 1.5e-7: the sim3 switch
set holds most directions by the posture rows alone, |u| reaches 1.6e10, J_r . u cancels ten digits and the restatement itself moves by
1.3e-8 under one ulp of noise in J — the reference's own error, not the kernel's."""
import numpy as np
import pytest

import grad_common as gc
import oracle
import test_gpu_task_params as tgp
import wbc_capi as capi
import wbc_model

pytestmark = pytest.mark.gpu

DT = gc.DT
S = wbc_model.TASK_PARAMS_SLICES
SHAPES = {"b7": (["a1_wx200"], 7), "mixed67": (["a1_wx200", "a1_px100_pin_ver", "laikago_vx300"], 67), "rot7": (["rot"], 7)}
CONFIGS = ["everything", "c3", "c3_trunk_task", "c3_hybrid", "c3_custom"]
PARITY_BOUND = 1e-11     # every output array within this x max(1, max|ref|) of the restatement (the docstring above says where it comes from)


def _problem(shape, cfg_name, seed=11):
    names, B = SHAPES[shape]
    models, cfgs, d, mid = tgp._problem(names, cfg_name, B, seed=seed, with_rot=True)
    rng = np.random.default_rng(seed + 3)
    if cfgs[0].task_joint == capi.JOINT_CUSTOM:
        d["posture_u"] = rng.normal(0, 0.3, (B, capi.V_STRIDE))
    rows = tgp._random_rows(tgp._rows_of(cfgs, mid, B), seed + 5)
    v = gc.task_space_v(models, cfgs, mid, d, rng)                        # (a loss on task-space velocities: grad_common.task_space_v says why)
    return models, cfgs, d, mid, rows, v


def _reference(models, cfgs, mid, d, rows, got):
    """the restatement on the device's own qdot and sens_x; zero rows where the device reports a status"""
    dd = dict(d)
    if cfgs[0].task_joint in (capi.JOINT_MANI, capi.JOINT_HYBRID) and "posture_u" not in dd:
        dd["posture_u"] = oracle.posture_target(models, cfgs, d["q"], mid, nthreads=8)[0]
    ref = gc.restate(models, cfgs, mid, dd, got["qdot"], got["sens_x"], rows)
    bad = (got["status"] != 0) | (got["cert_status"] != capi.CERT_OK)
    for k in ref:
        ref[k][bad] = 0.0
    return ref, bad


@pytest.mark.parametrize("cfg_name", CONFIGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_with_the_restatement(shape, cfg_name):
    models, cfgs, d, mid, rows, v = _problem(shape, cfg_name)
    B = len(rows)
    bt = tgp._handle(models, cfgs, B, {})
    got = bt.tick_grad(d, DT, v, task_params=rows)
    assert bt.stat("last_grad_variant") == (0 if shape == "b7" else 1 << 32)      # variant_key(ROT): the Laikago model has rotated joint placements too
    ref, bad = _reference(models, cfgs, mid, d, rows, got)
    want = bt.default_grad_wants()
    assert set(want) == {"d_task_params"} | {"d_" + f for f in gc.fields_read(cfgs[0])}
    assert (got["grad_status"] == np.where(got["status"] != 0, capi.GRAD_UNSOLVED, np.where(got["cert_status"] != 0, capi.GRAD_CERT, 0))).all()
    assert bad.sum() <= B // 2, "too few solved and certified instances to call this a parity test: %d of %d" % (B - bad.sum(), B)
    worst = 0.0
    for k in want:
        scale = max(1.0, np.abs(ref[k]).max())
        ratio = np.abs(got[k] - ref[k]).max() / scale
        worst = max(worst, ratio)
        print("%s / %s: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e)" % (shape, cfg_name, k, ratio, np.abs(ref[k]).max()))
        assert ratio <= PARITY_BOUND, (k, ratio)
        assert (got[k][bad] == 0).all()
    print("%s / %s: %d of %d instances solved and certified; worst ratio %.3e (bound 1e-11)" % (shape, cfg_name, B - bad.sum(), B, worst))
    g = got["d_task_params"]
    assert (g[:, S["ee_gain"]].reshape(B, 5, 6)[:, :, 3:] == 0).all()
    if cfg_name in ("c3", "c3_hybrid", "c3_custom"):         # Grip and posture only: every other entry is bitwise +0
        other = np.ones(capi.TASK_PARAMS_DOUBLES, dtype=bool)
        other[S["ee_W"].start + 24:S["ee_W"].start + 30] = False
        other[S["ee_w"].start + 4] = False
        other[S["ee_gain"].start + 24:S["ee_gain"].start + 27] = False
        other[S["joint_w"]] = False
        assert not g[:, other].view(np.uint64).any()
        assert not got["d_ee_target"][:, :4].view(np.uint64).any() and not got["d_prev_ee_target"][:, :4].view(np.uint64).any()
        assert np.abs(g[~bad][:, ~other]).min() > 0             # ... and the Grip and posture entries are not
    bt.close()


def test_task_rows_see_q_not_q_con():
    """a caller's q_con moves the constraints and the bounds of the tick (and so qdot and sens_x), never the task rows: the gradient is the
    restatement's at q"""
    models, cfgs, d, mid, rows, v = _problem("b7", "c3")
    B = len(rows)
    rng = np.random.default_rng(41)
    d["q_con"] = d["q"].copy()
    d["q_con"][:, 19:24] += rng.normal(0, 0.05, (B, 5))                   # the arm, which the Grip rows depend on
    bt = tgp._handle(models, cfgs, B, {})
    got = bt.tick_grad(d, DT, v, task_params=rows)
    plain = bt.tick_grad({k: x for k, x in d.items() if k != "q_con"}, DT, v, task_params=rows)
    assert np.abs(got["qdot"] - plain["qdot"]).max() > 1e-6                # (q_con did reach the tick)
    ref, bad = _reference(models, cfgs, mid, {k: x for k, x in d.items() if k != "q_con"}, rows, got)
    assert bad.sum() <= 1
    for k in bt.default_grad_wants():
        ratio = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
        print("q_con given: %s max|dev - ref| = %.3e x max(1, max|ref|)" % (k, ratio))
        assert ratio <= PARITY_BOUND, (k, ratio)
    bt.close()


def _clean(shape="mixed67", cfg_name="everything", seed=13):
    """a problem, its handle and one certified tick on host arrays"""
    models, cfgs, d, mid, rows, v = _problem(shape, cfg_name, seed)
    bt = tgp._handle(models, cfgs, len(rows), {})
    return models, cfgs, d, mid, rows, v, bt


def test_null_rows_equal_rows_copied_from_the_configuration():
    models, cfgs, d, mid, _, v, bt = _clean()
    B = len(v)
    c = bt.tick_certificate(d, DT, v=v)
    args = dict(status=c["status"], cert_status=c["cert_status"])
    a = bt.tick_vjp(d, DT, c["qdot"], c["sens_x"], **args)
    b = bt.tick_vjp(d, DT, c["qdot"], c["sens_x"], task_params=tgp._rows_of(cfgs, mid, B), **args)
    assert (a["grad_status"] == 0).sum() >= B // 2 and np.abs(a["d_task_params"]).max() > 0
    for k in a:
        assert np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k], b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k]), k
    bt.close()


def test_bad_rows_among_good_ones():
    """joint_w = 0 and a NaN weight: the tick refuses the rows (status != 0) and their gradient rows are zero, grad_status UNSOLVED; a
    certificate that is not OK and a NaN in sens_x likewise (CERT, NONFINITE); every other instance's rows are bitwise what they are without."""
    models, cfgs, d, mid, rows, v, bt = _clean("b7", "c3", seed=17)
    B = len(rows)
    good = bt.tick_grad(d, DT, v, task_params=rows)
    assert (good["grad_status"] == 0).sum() >= B - 1
    r2 = rows.copy()
    r2[2, S["joint_w"]] = 0.0
    r2[5, S["ee_W"].start + 25] = np.nan
    got = bt.tick_grad(d, DT, v, task_params=r2)
    keys = [k for k in got if k.startswith("d_")]
    expect = good["grad_status"].copy()
    expect[[2, 5]] = capi.GRAD_UNSOLVED
    assert (got["status"][[2, 5]] != 0).all() and np.array_equal(got["grad_status"], expect)
    rest = np.array([0, 1, 3, 4, 6])
    for k in keys:
        assert not got[k][[2, 5]].view(np.uint64).any(), k
        assert np.array_equal(got[k][rest].view(np.uint64), good[k][rest].view(np.uint64)), k
    # by hand: every instance solved, a certificate not OK, NaN / inf in sens_x and qdot
    st, cs = np.zeros(B, np.int32), np.zeros(B, np.int32)
    cs[1] = capi.CERT_DEPENDENT
    u, x = good["sens_x"].copy(), good["qdot"].copy()
    u[3, 7] = np.nan
    x[6, 0] = np.inf
    hand = bt.tick_vjp(d, DT, x, u, status=st, cert_status=cs, task_params=rows)
    assert list(hand["grad_status"]) == [0, capi.GRAD_CERT, 0, capi.GRAD_NONFINITE, 0, 0, capi.GRAD_NONFINITE]
    rest = np.array([i for i in (0, 2, 4, 5) if good["grad_status"][i] == 0])
    for k in keys:
        assert not hand[k][[1, 3, 6]].view(np.uint64).any(), k
        assert np.array_equal(hand[k][rest].view(np.uint64), good[k][rest].view(np.uint64)), k
    # status and cert_status NULL: every instance counts as solved and certified
    free = bt.tick_vjp(d, DT, good["qdot"], good["sens_x"], task_params=rows)
    ok = good["grad_status"] == 0
    for k in keys:
        assert np.array_equal(free[k][ok].view(np.uint64), good[k][ok].view(np.uint64)), k
    bt.close()


def test_argument_errors_name_the_field():
    models, cfgs, d, mid, rows, v, bt = _clean("b7", "c3", seed=17)
    c = bt.tick_certificate(d, DT, v=v)
    for kw, word in ((dict(want=("d_trunk_target",)), "d_trunk_target"), (dict(want=("d_com_target_vel",)), "d_com_target_vel"),
                     (dict(want=("d_posture_u",)), "d_posture_u")):
        with pytest.raises(capi.WbcError) as e:
            bt.tick_vjp(d, DT, c["qdot"], c["sens_x"], **kw)
        assert e.value.code == capi.E_ARG and word in str(e.value)
    for q, u, word in ((None, c["sens_x"], "qdot"), (c["qdot"], None, "sens_x")):
        with pytest.raises(capi.WbcError) as e:
            bt.tick_vjp(d, DT, q, u, out=dict(grad_status=np.zeros(len(v), np.int32)))
        assert e.value.code == capi.E_ARG and word in str(e.value)
    bt.close()


@pytest.mark.parametrize("cfg_name", ["everything", "c3_hybrid"])
def test_device_buffers_in_place_under_guards(cfg_name):
    """device pointers in place: NaN-filled outputs with guard rows around them, NaN guard rows around every float input; the guards come back
    intact, the inputs byte for byte, the results are the host call's, and a call that leaves outputs NULL gives the same bytes in the rest"""
    import torch
    import devguard as dg
    models, cfgs, d, mid, rows, v, bt = _clean("mixed67", cfg_name, seed=19)
    B = len(rows)
    _, _, other, _, orows, ov = _problem("mixed67", cfg_name, seed=23)
    host = bt.tick_grad(d, DT, v, task_params=rows)
    want = bt.default_grad_wants()
    ins = dict(d, qdot=host["qdot"], sens_x=host["sens_x"], status=host["status"], cert_status=host["cert_status"], task_params=rows)
    oth = dict(other, qdot=ov, sens_x=ov, status=np.zeros(B, np.int32), cert_status=np.zeros(B, np.int32), task_params=orows)
    stream = torch.cuda.Stream()
    for subset in (want, ("d_task_params",), want[1:]):
        sess = dg.Session("nan", stream)
        dev = sess.put_all(ins, oth)
        out = {k: sess.out((B,) + capi.TICK_GRAD_FIELDS[k]) for k in subset}
        if subset is want:
            out["grad_status"] = sess.out((B,), np.int32)
        tick_in = {k: dev[k] for k in d}
        sess.run(lambda: bt.tick_vjp(tick_in, DT, dev["qdot"], dev["sens_x"], status=dev["status"], cert_status=dev["cert_status"],
                                     task_params=dev["task_params"], out=out))
        sess.check("tick_vjp %s" % (subset,))
        res = dg.to_host(out)
        for k in res:
            assert dg.same_bytes(res[k], host[k]), (subset, k)
    bt.close()


def test_tick_grad_is_the_three_calls_by_hand():
    models, cfgs, d, mid, rows, v, bt = _clean("mixed67", "c3_trunk_task", seed=29)
    got = bt.tick_grad(d, DT, v, task_params=rows)
    a = bt.assemble(d, DT, want=("A", "b", "C", "Clb", "Cub", "lb", "ub"), task_params=rows)
    t = bt.tick(d, DT, want_working_set=True, task_params=rows)
    # (models with fewer than 26 velocity columns: a unit row on each padded column, H_dd = 1 as in the (H, g) form of the tick's problem)
    nv = np.array([m.nv for m in models])[mid]
    k = 26 - nv.min()
    pad = (np.arange(26)[None, None, :] == (nv[:, None] + np.arange(k)[None, :])[:, :, None]).astype(np.float64)
    assert k == 1 and pad.sum() == (nv < 26).sum() > 0
    A, b = np.concatenate([a["A"], pad], axis=1), np.concatenate([a["b"], np.zeros((len(v), k))], axis=1)
    c = bt.qp_certificate(t["qdot"], A=A, b=b, C_=a["C"], lb=a["lb"], ub=a["ub"], Clb=a["Clb"], Cub=a["Cub"], status=t["status"],
                          working_set=t["working_set"], v=v)
    assert (c["cert_status"][t["status"] == 0] == capi.CERT_OK).all()
    g = bt.tick_vjp(d, DT, t["qdot"], c["sens_x"], status=t["status"], cert_status=c["cert_status"], task_params=rows)
    import devguard as dg
    hand = dict(t, **dict(c, **g))
    assert set(hand) == set(got)
    for k in hand:
        assert dg.same_bytes(hand[k], got[k]), k
    bt.close()


def test_torch_layer_backward_is_tick_grad():
    import torch
    import wbc_torch
    models, cfgs, d, mid, rows, v, bt = _clean("mixed67", "c3_trunk_task", seed=29)
    ref = bt.tick_grad(d, DT, v, task_params=rows)
    dev = {k: torch.from_numpy(np.ascontiguousarray(x)).cuda() for k, x in d.items()}
    rest = {k: x for k, x in dev.items() if k not in ("ee_target", "prev_ee_target", "trunk_target", "prev_trunk_target")}
    tp = torch.from_numpy(rows).cuda().requires_grad_(True)
    ee = dev["ee_target"].clone().requires_grad_(True)
    eep = dev["prev_ee_target"].clone()                                   # requires_grad = False: no gradient
    tt = dev["trunk_target"].clone().requires_grad_(True)
    ttp = dev["prev_trunk_target"].clone().requires_grad_(True)
    qdot, st = wbc_torch.wbc_tick(tp, ee, eep, tt, ttp, None, None, None, rest, DT, bt)
    assert np.array_equal(qdot.detach().cpu().numpy().view(np.uint64), ref["qdot"].view(np.uint64)) and not st.requires_grad
    (qdot * torch.from_numpy(v).cuda()).sum().backward()
    for t, k in ((tp, "d_task_params"), (ee, "d_ee_target"), (tt, "d_trunk_target"), (ttp, "d_prev_trunk_target")):
        assert np.array_equal(t.grad.cpu().numpy().reshape(ref[k].shape).view(np.uint64), ref[k].view(np.uint64)), k
    assert eep.grad is None
    # the autograd function itself: None for arguments given as None and for those that need no gradient
    ctx_in = (tp.detach().requires_grad_(True), ee.detach(), None, tt.detach(), ttp.detach().requires_grad_(True), None, None, None)
    q2, _ = wbc_torch.wbc_tick(*ctx_in, dict(rest, prev_ee_target=dev["prev_ee_target"]), DT, bt)
    grads = torch.autograd.grad((q2 * torch.from_numpy(v).cuda()).sum(), [ctx_in[0], ctx_in[4]], allow_unused=True, retain_graph=True)
    assert np.array_equal(grads[0].cpu().numpy().view(np.uint64), ref["d_task_params"].view(np.uint64))
    assert np.array_equal(grads[1].cpu().numpy().view(np.uint64), ref["d_prev_trunk_target"].view(np.uint64))
    # ... seen at the function's own boundary: a stand-in context with the same saved tensors
    node = q2.grad_fn

    class Ctx:
        saved_tensors, batch, dt, rest, present = node.saved_tensors, node.batch, node.dt, node.rest, node.present
        needs_input_grad = (False, True, False, False, False, True, False, False, False, False, False, False)      # (q, which wbc_tick leaves None, first)
    out = wbc_torch._WbcTick.backward(Ctx, torch.from_numpy(v).cuda(), None)
    assert len(out) == 12 and [o is not None for o in out] == [False, True, False, False, False, True] + [False] * 6
    bt.close()
