"""wbc_tick_vjp_state on the device: dL/dq (tangent coordinates) and dL/d trunk_box_center of solved ticks (csrc/wbc_k_gradq.hip), held to the
numpy restatement wbc_workload.tick_state_gradients fed the device's own qdot and certificate outputs, and its behaviour at the boundary:
working set given or not, bad rows among good ones, guarded device buffers in place, refusals, the WbcBatch and torch layers on top of it.

Parity bound: both outputs within PARITY_BOUND x max(1, max|ref|) of the restatement, the project's 1e-11 (wbc_tick_vjp measured 5.4e-13 at
worst). v = dL/dqdot of a loss on task-space velocities (grad_common.task_space_v says why). Measured on MI355X over the 21 parity cases:
d_q at most 5.7e-13 max(1, max|ref|) (mixed67 / everything; 1.0e-13 and less elsewhere), d_trunk_box_center bitwise equal — every case holds
1e-11 as it stands, so none needed a bound from the restatement's own movement under one ulp of noise in J."""
import numpy as np
import pytest

import common
import grad_common as gc
import gradq_common as gq
import oracle
import test_gpu_task_params as tgp
import wbc_capi as capi
import wbc_workload

pytestmark = pytest.mark.gpu

DT = gc.DT
SHAPES = {"b7": (["a1_wx200"], 7), "mixed67": (["a1_wx200", "a1_px100_pin_ver", "laikago_vx300"], 67), "rot7": (["rot"], 7)}
CONFIGS = ["everything", "c3", "c3_far", "c3_trunk_task", "c2", "c3_custom", "c3_hybrid"]
PARITY_BOUND = 1e-11
CERT_KEYS = ("qdot", "sens_x", "sens_bounds", "sens_rows", "y_rows")


def _problem(shape, cfg_name, seed=11):
    names, B = SHAPES[shape]
    if cfg_name == "c3_far":                                             # poses far from the nominal stance: trunk-angle box rows active
        models = [tgp._model(n) for n in names]
        cfgs = [common.config("c3", m) for m in models]
        mid = None if len(models) == 1 else (np.arange(B) % len(models)).astype(np.int32)
        parts = [common.far_tick_inputs(m, c, B, seed + i, with_rot=True) for i, (m, c) in enumerate(zip(models, cfgs))]
        d = {k: parts[0][k].copy() for k in parts[0]}
        for i in range(1, len(parts)):
            for k in d:
                d[k][mid == i] = parts[i][k][mid == i]
        if mid is not None:
            d["model_id"] = mid
    else:
        models, cfgs, d, mid = tgp._problem(names, cfg_name, B, seed=seed, with_rot=True)
    rng = np.random.default_rng(seed + 3)
    if cfgs[0].task_joint == capi.JOINT_CUSTOM:
        d["posture_u"] = rng.normal(0, 0.3, (B, capi.V_STRIDE))
    elif cfgs[0].task_joint >= capi.JOINT_MANI:                          # MANI / HYBRID: posture_u given (held constant)
        d["posture_u"] = oracle.posture_target(models, cfgs, d["q"], mid, nthreads=8)[0]
    rows = tgp._random_rows(tgp._rows_of(cfgs, mid, B), seed + 5)
    v = gc.task_space_v(models, cfgs, mid, d, rng)
    return models, cfgs, d, mid, rows, v


def _reference(models, cfgs, mid, d, rows, got, working_set=True):
    """the restatement on the device's own qdot and certificate; zero rows where the device reports a status"""
    ref = gq.restate(models, cfgs, mid, d, {k: got[k] for k in CERT_KEYS}, rows, got["working_set"] if working_set else None)
    bad = (got["status"] != 0) | (got["cert_status"] != capi.CERT_OK)
    for k in ref:
        ref[k][bad] = 0.0
    return ref, bad


def _same(a, b):
    return np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)


@pytest.mark.parametrize("cfg_name", CONFIGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_with_the_restatement(shape, cfg_name):
    models, cfgs, d, mid, rows, v = _problem(shape, cfg_name)
    B = len(rows)
    bt = tgp._handle(models, cfgs, B, {})
    got = bt.tick_grad_q(d, DT, v, task_params=rows)
    assert bt.stat("last_gradq_variant") == (0 if shape == "b7" else 1 << 32)     # variant_key(ROT)
    ref, bad = _reference(models, cfgs, mid, d, rows, got)
    names = ["d_q"] + (["d_trunk_box_center"] if cfgs[0].con_trunk else [])
    assert set(names) | {"grad_status"} <= set(got)
    assert (got["grad_status"] == np.where(got["status"] != 0, capi.GRAD_UNSOLVED, np.where(got["cert_status"] != 0, capi.GRAD_CERT, 0))).all()
    assert bad.sum() <= B // 2, "too few solved and certified instances to call this a parity test: %d of %d" % (B - bad.sum(), B)
    nv = np.array([m.nv for m in models])[np.zeros(B, int) if mid is None else mid]
    assert not got["d_q"][np.arange(26)[None, :] >= nv[:, None]].view(np.uint64).any()       # columns >= the model's nv are 0
    for k in names:
        scale = max(1.0, np.abs(ref[k]).max())
        ratio = np.abs(got[k] - ref[k]).max() / scale
        print("%s / %s: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e)" % (shape, cfg_name, k, ratio, np.abs(ref[k]).max()))
        assert ratio <= PARITY_BOUND, (k, ratio)
        assert (got[k][bad] == 0).all()
    assert np.abs(got["d_q"][~bad]).max() > 0
    if cfg_name == "c3_far":
        act = (got["sens_rows"][:, 1:4] != 0).any(axis=1) & ~bad
        print("%s / %s: %d instances with an active trunk-angle row" % (shape, cfg_name, act.sum()))
        assert act.any() and np.abs(got["d_trunk_box_center"][act, 1:]).max() > 0
    bt.close()


@pytest.mark.parametrize("cfg_name", ["everything", "c3"])
def test_parity_on_arbitrary_sensitivities(cfg_name):
    """every term at once, whatever a certificate would leave at zero: x, u, w, y drawn at random in all 26 columns and all p rows, every
    bound and row marked at a random side. (A certificate gives w = 0 at an inactive bound, so a tick's own sensitivities never weigh the
    constant branches of the damper; columns >= nv of the px100 carry values here that the kernel must not read.)"""
    models, cfgs, d, mid, rows, _ = _problem("mixed67", cfg_name, seed=37)
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
    got = bt.tick_vjp_state(d, DT, cert["qdot"], cert["sens_x"], sens_bounds=cert["sens_bounds"], sens_rows=cert["sens_rows"], y_rows=cert["y_rows"],
                            working_set=ws, task_params=rows)
    assert (got["grad_status"] == 0).all()
    ref = gq.restate(models, cfgs, mid, d, cert, rows, ws)
    for k in ("d_q", "d_trunk_box_center"):
        ratio = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
        print("mixed67 / %s, arbitrary sensitivities: %s max|dev - ref| = %.3e x max(1, max|ref| = %.3e)" % (cfg_name, k, ratio, np.abs(ref[k]).max()))
        assert ratio <= PARITY_BOUND, (k, ratio)
    bt.close()


def _clean(shape="mixed67", cfg_name="everything", seed=13):
    models, cfgs, d, mid, rows, v = _problem(shape, cfg_name, seed)
    bt = tgp._handle(models, cfgs, len(rows), {})
    return models, cfgs, d, mid, rows, v, bt


def _by_hand(bt, d, c, rows, **over):
    kw = dict(sens_bounds=c["sens_bounds"], sens_rows=c["sens_rows"], y_rows=c["y_rows"], status=c["status"], cert_status=c["cert_status"],
              working_set=c["working_set"], task_params=rows)
    kw.update(over)
    qdot, sens_x = kw.pop("qdot", c["qdot"]), kw.pop("sens_x", c["sens_x"])
    return bt.tick_vjp_state(kw.pop("inputs", d), DT, qdot, sens_x, **kw)


@pytest.mark.parametrize("cfg_name", ["everything", "c3"])
def test_working_set_given_or_not_gives_the_same_bits(cfg_name):
    models, cfgs, d, mid, rows, v, bt = _clean("mixed67", cfg_name)
    c = bt.tick_certificate(d, DT, task_params=rows, v=v)
    a, b = _by_hand(bt, d, c, rows), _by_hand(bt, d, c, rows, working_set=None)
    assert (a["grad_status"] == 0).sum() >= len(v) // 2 and np.abs(a["d_q"]).max() > 0
    for k in a:
        assert _same(a[k], b[k]), k
    bt.close()


def test_tick_grad_q_is_the_calls_by_hand():
    models, cfgs, d, mid, rows, v, bt = _clean("mixed67", "c3_trunk_task", seed=29)
    got = bt.tick_grad_q(d, DT, v, task_params=rows)
    c = bt.tick_certificate(d, DT, task_params=rows, v=v)
    hand = dict(c, **_by_hand(bt, d, c, rows))
    assert set(hand) == set(got)
    for k in hand:
        assert _same(hand[k], got[k]), k
    bt.close()


def test_bad_rows_among_good_ones():
    """a NaN in q, an unsolved row, a certificate that is not OK and a NaN in sens_rows each give all-zero rows and their grad_status; every
    other instance is bitwise unchanged"""
    models, cfgs, d, mid, rows, v, bt = _clean("b7", "c3", seed=17)
    B = len(rows)
    c = bt.tick_certificate(d, DT, task_params=rows, v=v)
    good = _by_hand(bt, d, c, rows)
    assert (good["grad_status"] == 0).sum() >= B - 1
    q2, st, cs, wr = d["q"].copy(), c["status"].copy(), c["cert_status"].copy(), c["sens_rows"].copy()
    q2[2, 9] = np.nan
    st[1] = capi.QP_MAX_ITER
    cs[3] = capi.CERT_DEPENDENT
    wr[5, 0] = np.nan
    got = _by_hand(bt, d, c, rows, inputs=dict(d, q=q2), status=st, cert_status=cs, sens_rows=wr)
    expect = good["grad_status"].copy()
    expect[[1, 2, 3, 5]] = [capi.GRAD_UNSOLVED, capi.GRAD_NONFINITE, capi.GRAD_CERT, capi.GRAD_NONFINITE]
    assert np.array_equal(got["grad_status"], expect)
    rest = np.array([0, 4, 6])
    for k in ("d_q", "d_trunk_box_center"):
        assert not got[k][[1, 2, 3, 5]].view(np.uint64).any(), k
        assert np.array_equal(got[k][rest].view(np.uint64), good[k][rest].view(np.uint64)), k
    # status and cert_status NULL: every instance counts as solved and certified
    free = _by_hand(bt, d, c, rows, status=None, cert_status=None)
    ok = good["grad_status"] == 0
    for k in ("d_q", "d_trunk_box_center"):
        assert np.array_equal(free[k][ok].view(np.uint64), good[k][ok].view(np.uint64)), k
    bt.close()


def test_argument_errors_name_the_field():
    models, cfgs, d, mid, rows, v, bt = _clean("b7", "c3", seed=17)
    B = len(v)
    c = bt.tick_certificate(d, DT, task_params=rows, v=v)
    gs = lambda: dict(grad_status=np.zeros(B, np.int32))      # noqa: E731
    cases = [(dict(inputs=dict(d, q_con=d["q"].copy())), "q_con"), (dict(qdot=None, out=gs()), "qdot"), (dict(sens_x=None, out=gs()), "sens_x"),
             (dict(sens_rows=None), "sens_rows"), (dict(y_rows=None), "y_rows"), (dict(sens_bounds=None), "sens_bounds"),
             (dict(inputs={k: x for k, x in d.items() if k != "trunk_box_center"}), "trunk_box_center")]
    for kw, word in cases:
        with pytest.raises(capi.WbcError) as e:
            _by_hand(bt, d, c, rows, **kw)
        assert e.value.code == capi.E_ARG and word in str(e.value), (word, str(e.value))
    bt.close()
    # d_trunk_box_center without the trunk constraint
    models, cfgs, d, mid, rows, v, bt = _clean("b7", "full", seed=17)
    z = np.zeros((B, 26))
    with pytest.raises(capi.WbcError) as e:
        bt.tick_vjp_state(d, DT, z, z, sens_bounds=z, want=("d_trunk_box_center",))
    assert e.value.code == capi.E_ARG and "d_trunk_box_center" in str(e.value)
    bt.close()
    # MANI / HYBRID with posture_u NULL
    models, cfgs, d, mid, rows, v, bt = _clean("b7", "c3_hybrid", seed=17)
    p = bt.constraint_rows
    with pytest.raises(capi.WbcError) as e:
        bt.tick_vjp_state({k: x for k, x in d.items() if k != "posture_u"}, DT, z, z, sens_bounds=z, sens_rows=np.zeros((B, p)), y_rows=np.zeros((B, p)))
    assert e.value.code == capi.E_ARG and "posture_u" in str(e.value)
    bt.close()


@pytest.mark.parametrize("cfg_name", ["everything", "c3_hybrid"])
def test_device_buffers_in_place_under_guards(cfg_name):
    """device pointers in place: NaN-filled outputs with guard rows around them, NaN guard rows around every float input; the guards come back
    intact, the inputs byte for byte, the results are the host call's; each output alone and both together"""
    import torch
    import devguard as dg
    models, cfgs, d, mid, rows, v, bt = _clean("mixed67", cfg_name, seed=19)
    B = len(rows)
    _, _, other, _, orows, ov = _problem("mixed67", cfg_name, seed=23)
    c = bt.tick_certificate(d, DT, task_params=rows, v=v)
    host = _by_hand(bt, d, c, rows)
    sens = {k: c[k] for k in CERT_KEYS + ("status", "cert_status", "working_set")}
    ins = dict(d, task_params=rows, **sens)
    p = c["sens_rows"].shape[1]
    oth = dict(other, task_params=orows, qdot=ov, sens_x=ov, sens_bounds=ov, sens_rows=np.ones((B, p)), y_rows=np.ones((B, p)),
               status=np.zeros(B, np.int32), cert_status=np.zeros(B, np.int32), working_set=np.zeros((B, 2), np.int64))
    stream = torch.cuda.Stream()
    for subset in (("d_q", "d_trunk_box_center", "grad_status"), ("d_q",), ("d_trunk_box_center",)):
        sess = dg.Session("nan", stream)
        dev = sess.put_all(ins, oth)
        out = {k: (sess.out((B,), np.int32) if k == "grad_status" else sess.out((B,) + capi.TICK_STATE_GRAD_FIELDS[k])) for k in subset}
        tick_in = {k: dev[k] for k in d}
        sess.run(lambda: bt.tick_vjp_state(tick_in, DT, dev["qdot"], dev["sens_x"], sens_bounds=dev["sens_bounds"], sens_rows=dev["sens_rows"],
                                           y_rows=dev["y_rows"], status=dev["status"], cert_status=dev["cert_status"],
                                           working_set=dev["working_set"], task_params=dev["task_params"], out=out))
        sess.check("tick_vjp_state %s" % (subset,))
        res = dg.to_host(out)
        for k in res:
            assert dg.same_bytes(res[k], host[k]), (subset, k)
    bt.close()


def test_torch_layer_backward_is_tick_grad_q():
    import torch
    import wbc_torch
    models, cfgs, d, mid, rows, v, bt = _clean("mixed67", "c3_trunk_task", seed=29)
    ref = bt.tick_grad_q(d, DT, v, task_params=rows)
    refg = bt.tick_grad(d, DT, v, task_params=rows)
    raw = wbc_workload.tangent_to_raw(d["q"], ref["d_q"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(x)).cuda() for k, x in d.items()}
    rest = {k: x for k, x in dev.items() if k not in ("q", "ee_target", "trunk_target")}
    q = dev["q"].clone().requires_grad_(True)
    tp = torch.from_numpy(rows).cuda().requires_grad_(True)
    ee = dev["ee_target"].clone().requires_grad_(True)
    tt = dev["trunk_target"].clone().requires_grad_(True)
    qdot, st = wbc_torch.wbc_tick_state(q, tp, ee, None, tt, None, None, None, None, rest, DT, bt)
    assert _same(qdot.detach().cpu().numpy(), ref["qdot"]) and not st.requires_grad
    (qdot * torch.from_numpy(v).cuda()).sum().backward()
    assert _same(q.grad.cpu().numpy(), raw)
    for t, k in ((tp, "d_task_params"), (ee, "d_ee_target"), (tt, "d_trunk_target")):
        assert _same(t.grad.cpu().numpy().reshape(refg[k].shape), refg[k]), k
    # q alone: no wbc_tick_vjp call is needed, the gradient is the same
    q2 = dev["q"].clone().requires_grad_(True)
    qd2, _ = wbc_torch.wbc_tick_state(q2, tp.detach(), None, None, None, None, None, None, None, dev, DT, bt)
    g2, = torch.autograd.grad((qd2 * torch.from_numpy(v).cuda()).sum(), [q2])
    assert _same(g2.cpu().numpy(), raw)
    bt.close()
