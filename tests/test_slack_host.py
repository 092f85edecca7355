"""Constraint slack on the host: wbc_workload.state_slack against quantities derived independently through the oracle's
assembly, wbc_workload.watch_summary against a hand-made trace, and the conditions the GPU watch test relies on, checked on the oracle alone."""
import numpy as np
import pytest

import common
import oracle
import slack_common as sc
import wbc_capi as capi
import wbc_model
import wbc_workload

DT = 0.002


@pytest.mark.parametrize("name", ["a1_wx200", "a1_px100_pin_ver", "laikago_vx300"])
@pytest.mark.parametrize("far", [False, True])
def test_restatement_against_the_oracle_assembly(name, far):
    """The CoM components are -Clb[0:2] dt / com_box_scale and Cub[0:2] dt / com_box_scale of the oracle's CoM rows, the trunk components the
    same from rows 2..5 with trunk_box_scale (probe configuration: both boxes on). The two routes share the FK alone. 1e-12: the FK parity
    tolerance; undoing the 1 / dt scaling costs a few ulp of a quantity below 1."""
    m = sc.model(name)
    cfg = wbc_model.make_config(m, Grip=True, Joint="PREV", cCoM=True, cTrunk=True, cFR=True, cFL=True, cRR=True, cRL=True, mode="static_reach")
    B = 48
    d = common.far_tick_inputs(m, cfg, B, 11, edge=True) if far else common.tick_inputs(m, cfg, B, 11)
    d["trunk_box_center"] = d["trunk_box_center"] + np.random.default_rng(12).normal(0, 0.02, (B, 4))   # (off the centre: no six-way tie of the angle rows)
    a = oracle.assemble([m], [cfg], d, DT, B)
    got = wbc_workload.state_slack(m, cfg, d["q"], d["trunk_box_center"], common.OracleFK([m]))
    want = np.zeros((B, 12))
    for r in range(2):
        want[:, 2 * r] = -a["Clb"][:, r] * DT / cfg.com_box_scale
        want[:, 2 * r + 1] = a["Cub"][:, r] * DT / cfg.com_box_scale
    for r in range(4):
        want[:, 4 + 2 * r] = -a["Clb"][:, 2 + r] * DT / cfg.trunk_box_scale
        want[:, 5 + 2 * r] = a["Cub"][:, 2 + r] * DT / cfg.trunk_box_scale
    err = np.abs(got["components"] - want).max()
    print("%s far=%s: components vs assembly %.3e" % (name, far, err))
    assert err < 1e-12
    for f, (lo, hi) in enumerate(((0, 4), (4, 6), (6, 12))):
        assert np.abs(got["slack"][:, f] - want[:, lo:hi].min(axis=1)).max() < 1e-12
        clear = sc.two_smallest_gap(want[:, lo:hi], 1) > sc.TIE
        assert clear.mean() >= 0.75
        assert (got["which"][:, f] == want[:, lo:hi].argmin(axis=1))[clear].all()
    # the joint family against the baked limits themselves
    data = m.data
    lo_best = np.full(B, np.inf)
    code = np.full(B, -1)
    n = 0
    for j in data["joints"][2:]:
        dof, i = j["idx_v"], j["idx_q"]
        if not 6 <= dof < cfg.lock_from:
            continue
        n += 1
        for c, v in ((2 * dof, d["q"][:, i] - wbc_model._num(data["q_lo"][i])), (2 * dof + 1, wbc_model._num(data["q_hi"][i]) - d["q"][:, i])):
            better = (v < lo_best) | ((v == lo_best) & (c < code))
            lo_best, code = np.where(better, v, lo_best), np.where(better, c, code)
    assert n == min(cfg.lock_from, m.nv) - 6 and n >= 12
    assert np.array_equal(got["slack"][:, 3], lo_best) and np.array_equal(got["which"][:, 3], code)


def test_restatement_bad_rows_and_missing_box():
    m = sc.model("a1_wx200")
    cfg = common.config("c3", m)
    d = common.tick_inputs(m, cfg, 6, 3)
    fk = common.OracleFK([m])
    base = wbc_workload.state_slack(m, cfg, d["q"], d["trunk_box_center"], fk)
    q = d["q"].copy()
    q[2, 9] = np.nan
    box = d["trunk_box_center"].copy()
    box[4, 0], box[5, 2] = np.inf, np.nan
    got = wbc_workload.state_slack(m, cfg, q, box, fk)
    assert np.isnan(got["slack"][2]).all() and (got["which"][2] == -1).all() and np.isnan(got["components"][2]).all()
    assert np.isnan(got["slack"][4, 1]) and got["which"][4, 1] == -1 and np.array_equal(got["slack"][4, [0, 2, 3]], base["slack"][4, [0, 2, 3]])
    assert np.isnan(got["slack"][5, 2]) and got["which"][5, 2] == -1 and np.array_equal(got["slack"][5, [0, 1, 3]], base["slack"][5, [0, 1, 3]])
    for b in (0, 1, 3):
        assert np.array_equal(got["slack"][b], base["slack"][b]) and np.array_equal(got["which"][b], base["which"][b])
    nobox = wbc_workload.state_slack(m, cfg, d["q"], None, fk)
    assert np.isnan(nobox["slack"][:, 1:3]).all() and (nobox["which"][:, 1:3] == -1).all()
    assert np.array_equal(nobox["slack"][:, [0, 3]], base["slack"][:, [0, 3]])
    nolock = capi.WbcConfig.from_buffer_copy(cfg)
    nolock.lock_from = 6                                              # no free DoF: +inf, code -1
    e = wbc_workload.state_slack(m, nolock, d["q"], None, fk)
    assert np.isposinf(e["slack"][:, 3]).all() and (e["which"][:, 3] == -1).all()


def test_watch_summary_on_a_hand_made_trace():
    nan = np.nan
    #                 tie (first wins)  NaN tick        all negative    never negative
    trace = np.array([[0.5,             0.2,            -0.1,           1.0],
                      [0.1,             nan,            -0.3,           2.0],
                      [0.1,             -1.0,           -0.3,           1.0],
                      [0.3,             -2.0,           -0.2,           3.0]])
    which = np.array([[1, 2, 3, 4], [5, -1, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]])
    s = wbc_workload.watch_summary(trace, which)
    assert np.array_equal(s["slack_min"], [0.1, nan, -0.3, 1.0], equal_nan=True)
    assert np.array_equal(s["slack_min_tick"], [1, 1, 1, 0])
    assert np.array_equal(s["slack_min_which"], [5, -1, 7, 4])
    assert np.array_equal(s["slack_final"], [0.3, -2.0, -0.2, 3.0])
    assert np.array_equal(s["neg_ticks"], [0, 2, 4, 0])
    assert np.array_equal(s["first_neg_tick"], [-1, 2, 0, -1])
    assert s["slack_min_tick"].dtype == np.int32 and s["neg_ticks"].dtype == np.int32
    s3 = wbc_workload.watch_summary(trace.reshape(4, 2, 2))
    assert s3["slack_min"].shape == (2, 2) and np.array_equal(s3["slack_min_tick"].ravel(), [1, 1, 1, 0])


def test_the_gpu_watch_tests_conditions_hold_on_the_oracle_alone():
    """The recipe of test_gpu_slack.py's watch test (sim3 switch set, mixed a1_wx200 + a1_px100, stressed seeds 5 / 6, the gripper target stepping
    (3, 0, -1) mm per tick) through the oracle's loop: no per-tick |slack| below 1e-6, at most a quarter of the instances per family with their
    two smallest per-tick values closer than 1e-9 without being equal, and a sign change in some family for at least one instance per model."""
    ref = sc.watch_reference("sim3")
    p = sc.watch_problem("sim3")
    tr = ref["trace"]
    B = tr.shape[2]
    c = sc.comparable(ref)
    near_zero = (np.abs(tr) < sc.NEAR_ZERO).any(axis=0)
    flips = ((tr < 0).any(axis=0) & (tr >= 0).any(axis=0))
    print("near zero %s  near ties %s  exact ties %s  sign changes %s  family minima %s .. %s" % (
        near_zero.sum(axis=1), c["near_tie"].sum(axis=1), c["exact_tie"].sum(axis=1), flips.sum(axis=1), tr.min(axis=(0, 2)), tr.max(axis=(0, 2))))
    assert not near_zero.any()
    assert (c["near_tie"].sum(axis=1) <= B // 4).all()
    for i in range(len(p["models"])):
        assert flips[:, p["mid"] == i].any(), "no sign change for model %d" % i
    for k in ("tick", "which", "counts"):
        assert (c[k].mean(axis=1) >= 0.75).all(), k
