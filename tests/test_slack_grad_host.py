"""CPU: the constraint slack as a loss. wbc_state_slack_vjp / wbc_rollout_record_watch / wbc_rollout_vjp_watched at the boundary (header,
exports, struct sizes, variant count) and the host restatement wbc_workload.slack_gradients / watch_seed_gradients /
rollout_gradients(watch_seed=...), held to the oracle alone:
  the layer        slack_gradients against central differences of wbc_workload.state_slack on the oracle's FK, along random tangent directions
                   in q (gradq_common.step, pin.integrate's (+)) and in the box centre, one output at a time: each of the 12 components, each of
                   the 4 families, and a random mix of all. q's joint entries are displaced so that no two joint components tie and the box is
                   displaced (slack_grad_common.displace_box) so that the angle components do not; an instance whose selected component changes
                   at one of the four steps is left out of that family's comparison (at most B // 4). test_score_grad_host's rule: 4 |FD(h) -
                   FD(h/2)| plus the rounding of the difference, K_ROUND eps |gamma| (the magnitudes the output is formed from) / (h / 2).
  the seed         rollout_gradients(watch_seed=g_trace alone) equals rollout_gradients(g_q_trace=the host-built rows) to LIN_BOUND, the box term
                   added in closed form; slack_min's and slack_final's cotangents are the corresponding rows of the trace, bit for bit.
Measured here (CPU): worst |analytic - FD(h/2)| / tolerance 0.113 (a1_wx200), 0.110 (a1_px100_pin_ver), 0.085 (laikago_vx300); 0 instances
left out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
import gradq_common as gq
import oracle
import slack_common as sl
import slack_grad_common as sgc
import step_common as sc
import test_score_grad_host as sh
import test_step_grad_host as th
import test_tick_grad_q_host as tq
import wbc_capi as capi
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
K_ROUND = sh.K_ROUND
LIN_BOUND = sh.LIN_BOUND
NEW_SYMBOLS = ("wbc_state_slack_vjp", "wbc_slack_grad_sizes", "wbc_rollout_record_watch", "wbc_rollout_vjp_watched", "wbc_rollout_watched_sizes")


# ---- 1., 2. the boundary
def test_header_declares_and_library_exports_the_five_symbols():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"int\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    for word in ("WbcSlackGrad", "WbcWatchSeed", "g_slack_min", "g_slack_final", "g_trace", "slack_min_tick", "last_slackvjp_variant", "subgradient"):
        assert word.lower() in header.lower(), word
    # struck from both lists of what is not offered
    for section in ("roll-out scores as a loss", "wbc_rollout_vjp_tracks is"):
        part = header[header.index(section):]
        part = part[part.index("Not offered"):]
        part = part[:part.index("*/")]
        assert "watch as a loss" not in part.split("(")[0] and "the watch," not in part, section


def test_struct_sizes_match_ctypes_and_the_variant_table_has_four_rows():
    lib = capi.load_library()
    a = C.c_int32()
    assert lib.wbc_slack_grad_sizes(C.byref(a)) == 0 and a.value == C.sizeof(capi.WbcSlackGrad) == 32
    assert lib.wbc_rollout_watched_sizes(C.byref(a)) == 0 and a.value == C.sizeof(capi.WbcWatchSeed) == 48
    assert lib.wbc_variant_count(b"slackvjp") == 4 and lib.wbc_variant_count(b"scorevjp") == 3
    assert "slackvjp" not in capi.VARIANT_FAMILIES


# ---- 3. the layer against central differences
B_FD = 8
H_FD = 2.0 ** -16


def _layer_problem(name, seed):
    m = sl.model(name)
    cfg = common.config("everything", m)
    d = sgc.displace_box(common.tick_inputs(m, cfg, B_FD, seed=seed, stress=True), seed=11)
    rng = np.random.default_rng(seed + 300)
    q = d["q"].copy()
    for _, i in wbc_workload.slack_joint_dofs(m, cfg):                     # no two joint components tie
        q[:, i] += rng.uniform(-0.02, 0.02, B_FD)
    return m, cfg, q, d["trunk_box_center"], rng


def _outputs(m, cfg, q, box):
    """-> (components [B, 12] + slack [B, 4] side by side, which [B, 4], mags [B, 16]: what each output is formed from)"""
    fk = gq.StateFK([m])
    r = wbc_workload.state_slack(m, cfg, q, box, fk)
    pos, com = fk(q)[:, :, 9:12], fk.com(q)
    pFL, pRR, pT = pos[:, capi.FR_EE0 + 1], pos[:, capi.FR_EE0 + 2], pos[:, capi.FR_TRUNK]
    mags = np.zeros((len(q), 16))
    for r_ in range(2):
        mags[:, 2 * r_], mags[:, 2 * r_ + 1] = np.abs(pRR[:, r_]) + np.abs(com[:, r_]), np.abs(pFL[:, r_]) + np.abs(com[:, r_])
    mags[:, 4:6] = (np.abs(box[:, 0]) * (1 + cfg.trunk_box_z_frac) + np.abs(pT[:, 2]))[:, None]
    mags[:, 6:12] = np.repeat(np.abs(box[:, 1:]) + cfg.trunk_box_ang + np.pi, 2, axis=1)
    mags[:, 12], mags[:, 13], mags[:, 14] = mags[:, 0:4].max(axis=1), mags[:, 4], mags[:, 6:12].max(axis=1)
    mags[:, 15] = np.abs(q[:, 7:]).max(axis=1) + max(np.abs(m.q_lo[7:m.nq]).max(), np.abs(m.q_hi[7:m.nq]).max())
    return np.concatenate([r["components"], r["slack"]], axis=1), r["which"], mags


@pytest.mark.parametrize("name,seed", [("a1_wx200", 3), ("a1_px100_pin_ver", 4), ("laikago_vx300", 5)])
def test_slack_gradients_against_central_differences(name, seed):
    m, cfg, q, box, rng = _layer_problem(name, seed)
    B, h = B_FD, H_FD
    fk = gq.StateFK([m])
    base, which0, mags = _outputs(m, cfg, q, box)
    assert (which0 >= 0).all() and (sl.two_smallest_gap(wbc_workload.state_slack(m, cfg, q, box, fk)["joint_components"], 1) > 0).all()
    worst, dropped = 0.0, 0
    for trial in range(3):
        dq = np.zeros((B, capi.V_STRIDE))
        dq[:, :m.nv] = rng.choice([-1.0, 1.0], (B, m.nv)) * rng.uniform(0.5, 1.0, (B, m.nv))
        db = rng.normal(0, 1.0, (B, 4))
        if trial == 1:
            db[:] = 0.0                                                   # the state alone
        if trial == 2:
            dq[:] = 0.0                                                   # the box centre alone
        vals, same = {}, np.ones((B, 4), dtype=bool)
        for s in (h, -h, h / 2, -h / 2):
            vals[s], w, _ = _outputs(m, cfg, gq.step([m], q, s * dq), box + s * db)
            same &= w == which0
        fd1, fd2 = (vals[h] - vals[-h]) / (2 * h), (vals[h / 2] - vals[-h / 2]) / h
        tol = 4.0 * np.abs(fd1 - fd2) + K_ROUND * EPS * mags / (h / 2)
        keep = np.concatenate([np.ones((B, 12), dtype=bool), same], axis=1)
        dropped = max(dropped, int((~same).any(axis=1).sum()))
        assert (~same).any(axis=1).sum() <= B // 4
        ana = np.zeros((B, 16))
        for j in range(16):                                               # one output at a time: a one-hot cotangent
            gs, gc_ = np.zeros((B, 4)), np.zeros((B, 12))
            (gc_ if j < 12 else gs)[:, j if j < 12 else j - 12] = 1.0
            r = wbc_workload.slack_gradients(m, cfg, q, box, fk, g_slack=gs if j >= 12 else None, g_components=gc_ if j < 12 else None)
            assert np.array_equal(r["which"], which0) and (r["grad_status"] == capi.GRAD_OK).all() and not r["d_q"][:, m.nv:].any()
            ana[:, j] = (r["d_q"] * dq).sum(axis=1) + (r["d_trunk_box_center"] * db).sum(axis=1)
        err = np.abs(ana - fd2)
        ratio = np.where(keep, err / tol, 0.0)
        worst = max(worst, ratio.max())
        print("%s, trial %d: worst |analytic - FD(h/2)| / tolerance %.3f (output %d); |analytic - FD(h/2)| up to %.3e, |FD(h) - FD(h/2)| up to %.3e, |grad| up to %.3g; %d instances left out" % (
            name, trial, ratio.max(), int(ratio.max(axis=0).argmax()), err[keep].max(), np.abs(fd1 - fd2)[keep].max(), np.abs(fd2).max(), int((~same).any(axis=1).sum())))
        assert (err[keep] <= tol[keep]).all(), (trial, np.argwhere(keep & (err > tol)))
        if trial != 2:
            assert (np.abs(ana).max(axis=0) > 0).all()                   # every output moves with the state
        # all cotangents together: the sum of the one-hot answers
        gs, gc_ = rng.normal(0, 1.0, (B, 4)), rng.normal(0, 1.0, (B, 12))
        r = wbc_workload.slack_gradients(m, cfg, q, box, fk, g_slack=gs, g_components=gc_)
        mix = (r["d_q"] * dq).sum(axis=1) + (r["d_trunk_box_center"] * db).sum(axis=1)
        ref = (ana[:, :12] * gc_).sum(axis=1) + (ana[:, 12:] * gs).sum(axis=1)
        assert np.abs(mix - ref).max() <= 64 * EPS * (np.abs(ana[:, :12] * gc_).sum(axis=1) + np.abs(ana[:, 12:] * gs).sum(axis=1)).max()
    print("%s: worst ratio %.3f, at most %d of %d instances left out" % (name, worst, dropped, B))


def test_exact_zeros_bad_rows_and_what_the_restatement_refuses():
    m, cfg, q, box, rng = _layer_problem("a1_wx200", 3)
    B, fk = B_FD, gq.StateFK([m])
    gs, gc_ = rng.normal(0, 1.0, (B, 4)), rng.normal(0, 1.0, (B, 12))
    good = wbc_workload.slack_gradients(m, cfg, q, box, fk, gs, gc_)
    zero = wbc_workload.slack_gradients(m, cfg, q, box, fk, np.zeros((B, 4)), np.zeros((B, 12)))
    assert not zero["d_q"].any() and not zero["d_trunk_box_center"].any() and (zero["grad_status"] == 0).all()
    # the joint family alone: one entry of d_q per instance, +gamma on the lower side and -gamma on the upper
    g3 = np.zeros((B, 4))
    g3[:, 3] = gs[:, 3]
    r = wbc_workload.slack_gradients(m, cfg, q, box, fk, g3)
    code = r["which"][:, 3]
    assert ((r["d_q"] != 0).sum(axis=1) == 1).all() and not r["d_trunk_box_center"].any()
    assert np.array_equal(r["d_q"][np.arange(B), code >> 1], np.where(code & 1, -gs[:, 3], gs[:, 3]))
    # bad rows: a NaN q entry, an infinite cotangent, a NaN box entry under a non-zero cotangent of its family (and under a zero one: good)
    q2, gs2, gc2, box2 = q.copy(), gs.copy(), gc_.copy(), box.copy()
    q2[1, 9], gs2[2, 0], box2[3, 2], box2[4, 0] = np.nan, np.inf, np.nan, np.nan
    gs2[4, 1], gc2[4, 4:6] = 0.0, 0.0
    r = wbc_workload.slack_gradients(m, cfg, q2, box2, fk, gs2, gc2)
    bad = np.array([1, 2, 3])
    assert np.array_equal(r["grad_status"], np.where(np.isin(np.arange(B), bad), capi.GRAD_NONFINITE, capi.GRAD_OK))
    assert not r["d_q"][bad].any() and not r["d_trunk_box_center"][bad].any()
    ok = np.array([0, 5, 6, 7])
    assert np.array_equal(r["d_q"][ok], good["d_q"][ok]) and np.array_equal(r["d_trunk_box_center"][ok], good["d_trunk_box_center"][ok])
    assert np.isfinite(r["d_q"][4]).all() and r["d_trunk_box_center"][4, 0] == 0.0 and r["which"][4, 1] == -1
    with pytest.raises(ValueError):
        wbc_workload.slack_gradients(m, cfg, q, box, fk)
    with pytest.raises(ValueError):
        wbc_workload.slack_gradients(m, cfg, q, None, fk, gs)
    only0 = np.zeros((B, 4))
    only0[:, [0, 3]] = gs[:, [0, 3]]
    r = wbc_workload.slack_gradients(m, cfg, q, None, fk, only0)        # without a box the trunk families have no component, the others work
    assert (r["which"][:, 1:3] == -1).all() and np.abs(r["d_q"]).max() > 0 and not r["d_trunk_box_center"].any()


# ---- 4., 5. the seed in the restated sweep
def _sweep_problem(cfg_name="everything", seed=4, K=3):
    m, cfg, d, _, _ = th.sweep_setup(cfg_name, seed)
    d = sgc.displace_box(d)
    states, ticks, _, status = sc.chain(m, cfg, d, K, tq.DT)
    B = len(d["q"])
    run = lambda **kw: wbc_workload.rollout_gradients(      # noqa: E731
        m, cfg, [dict(s) for s in states[:K]], np.stack([t["qdot"] for t in ticks]), tq.DT, gq.StateFK([m]),
        lambda dd: oracle.assemble([m], [cfg], dd, tq.DT, B), status=np.stack(status), **kw)
    q_after = np.stack([s["q"] for s in states[1:]])
    return m, cfg, d, K, B, q_after, run


def test_a_trace_seed_alone_is_the_sweep_with_the_host_built_rows():
    m, cfg, d, K, B, q_after, run = _sweep_problem()
    gam = sgc.watch_gammas(B, K, 41)
    seed = dict(mask=sgc.FULL_MASK, q_final=q_after[K - 1], g_trace=gam["g_trace"])
    rows = wbc_workload.watch_seed_gradients(m, cfg, q_after, d["trunk_box_center"], gq.StateFK([m]), sgc.FULL_MASK, g_trace=gam["g_trace"])
    db = rows["d_trunk_box_center"]
    assert np.abs(rows["g_q_trace"]).max() > 0 and np.abs(db[:, 0]).min() > 0 and np.abs(db[:, 1:]).sum(axis=1).min() > 0
    a, b = run(watch_seed=seed), run(g_q_trace=rows["g_q_trace"])
    assert np.array_equal(a["ticks_dropped"], b["ticks_dropped"])
    for k in b:
        if k in ("ticks_dropped", "sens_max"):
            continue
        ref = b[k] + (rows["d_trunk_box_center"] if k == "d_trunk_box_center" else 0.0)
        assert np.abs(a[k] - ref).max() <= LIN_BOUND * max(1.0, np.abs(ref).max()), k
    # with a state seed beside it: the sum of each
    g = np.random.default_rng(5).normal(0, 1.0, (B, capi.V_STRIDE))
    g[:, m.nv:] = 0.0
    c, both = run(g_q_final=g), run(g_q_final=g, watch_seed=seed)
    for k in ("d_q0", "d_task_params", "d_ee_target", "d_trunk_box_center"):
        s = a[k] + c[k]
        assert np.abs(both[k] - s).max() <= LIN_BOUND * max(1.0, np.abs(s).max()), k


def test_slack_min_and_slack_final_are_rows_of_the_trace():
    m, cfg, d, K, B, q_after, _ = _sweep_problem()
    fk, box = gq.StateFK([m]), d["trunk_box_center"]
    gam = sgc.watch_gammas(B, K, 42)
    tick = np.random.default_rng(6).integers(0, K, (4, B)).astype(np.int32)
    fin = wbc_workload.watch_seed_gradients(m, cfg, q_after, box, fk, sgc.FULL_MASK, g_slack_final=gam["g_slack_final"])
    tr = np.zeros((K, 4, B))
    tr[K - 1] = gam["g_slack_final"]
    ref = wbc_workload.watch_seed_gradients(m, cfg, q_after, box, fk, sgc.FULL_MASK, g_trace=tr)
    assert np.array_equal(fin["g_q_trace"], ref["g_q_trace"]) and np.array_equal(fin["d_trunk_box_center"], ref["d_trunk_box_center"])
    assert not fin["g_q_trace"][:K - 1].any() and np.abs(fin["g_q_trace"][K - 1]).max() > 0
    mn = wbc_workload.watch_seed_gradients(m, cfg, q_after, box, fk, sgc.FULL_MASK, g_slack_min=gam["g_slack_min"], slack_min_tick=tick)
    tr = np.where(np.arange(K)[:, None, None] == tick[None], gam["g_slack_min"][None], 0.0)
    ref = wbc_workload.watch_seed_gradients(m, cfg, q_after, box, fk, sgc.FULL_MASK, g_trace=tr)
    assert np.array_equal(mn["g_q_trace"], ref["g_q_trace"]) and np.array_equal(mn["d_trunk_box_center"], ref["d_trunk_box_center"])
    # a mask with two bits: the rows of those families alone, in increasing family order
    two = wbc_workload.watch_seed_gradients(m, cfg, q_after, box, fk, (1 << 0) | (1 << 3), g_slack_final=gam["g_slack_final"][[0, 3]])
    z = gam["g_slack_final"].copy()
    z[1:3] = 0.0
    ref = wbc_workload.watch_seed_gradients(m, cfg, q_after, box, fk, sgc.FULL_MASK, g_slack_final=z)
    assert np.array_equal(two["g_q_trace"], ref["g_q_trace"]) and not two["d_trunk_box_center"].any()
    with pytest.raises(ValueError):
        wbc_workload.watch_seed_gradients(m, cfg, q_after, box, fk, sgc.FULL_MASK, g_slack_min=gam["g_slack_min"])
