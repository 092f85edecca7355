"""CPU: the tick as a layer. wbc_tick_vjp at the boundary (header, export, struct size) and its host restatement
wbc_workload.tick_gradients, held to the oracle alone:
  algebra     every coordinate of the 85 weights / gains and of every target array: the central difference of oracle.assemble's (A, b),
              contracted with the restatement's (dL/dA, dL/db), against its dL/dtheta. A and b are linear in each single coordinate, so
              the difference is exact up to rounding and the bound is computed, not chosen.
  end to end  the directional derivative of v . qdot from oracle.tick at steps h and h / 2 against the restatement fed
              wbc_workload.qp_certificate's u: the oracle calibrates its own error."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
import grad_common as gc
import oracle
import test_gpu_task_params as tgp
import wbc_capi as capi
import wbc_model
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
DT = gc.DT


def test_header_declares_and_library_exports_the_tick_gradient():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert re.search(r"int\s+wbc_tick_vjp\s*\(\s*WbcBatch\s*\*", header) and re.search(r"int\s+wbc_tick_grad_sizes\s*\(", header)
    for word in ("WbcTickGrad", "d_task_params", "d_prev_trunk_target", "d_posture_u", "grad_status", "WBC_GRAD_NONFINITE", "kinematic Hessians",
                 "ee_ref_rot", "trunk_box_center", "roll-outs"):
        assert word in header, word
    lib = capi.load_library()
    for name in ("wbc_tick_vjp", "wbc_tick_grad_sizes"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    s = C.c_int32()
    assert lib.wbc_tick_grad_sizes(C.byref(s)) == 0 and s.value == C.sizeof(capi.WbcTickGrad)
    assert lib.wbc_variant_count(b"grad") == 2                           # ROT off / on


def _problem(cfg_name, model_name, B, seed):
    m = tgp._model(model_name)
    cfg = common.config(cfg_name, m)
    d = common.tick_inputs(m, cfg, B, seed=seed, with_rot=True)
    rng = np.random.default_rng(seed + 17)
    if cfg.task_joint >= capi.JOINT_MANI:
        d["posture_u"] = rng.normal(0, 0.3, (B, capi.V_STRIDE))
    rows = tgp._random_rows(tgp._rows_of([cfg], None, B), seed + 5)
    return m, cfg, d, rows, rng


def _assemble(m, cfg, d, rows, dt=DT):
    ms, cs, pid = common.per_instance_configs([m], [cfg], None, rows)
    a = oracle.assemble(ms, cs, dict(d, model_id=pid), dt, len(rows))
    return a["A"], a["b"]


# the bound's constant. An entry of A carries two roundings (W (J w)) and an entry of b at most six (the target velocity's difference, quotient,
# gain product and sum, then w): at most 6 eps of the largest entry each, twice (theta + h and theta - h), over 2 h -> 6. The restatement's own
# dL/dtheta is a handful of products of the same quantities (<= 4 eps of the same scale) and the contraction's sum rounds once more per term
# (<= 2): 12. 16 leaves the power of two above it; a test that needs more than 16 is wrong.
K_BOUND = 16.0


@pytest.mark.parametrize("model_name", ["a1_wx200", "a1_px100_pin_ver", "laikago_vx300"])
@pytest.mark.parametrize("cfg_name", ["everything", "c3_trunk_task", "c2", "c3_custom"])
def test_algebra_against_central_differences_of_the_assembly(cfg_name, model_name):
    algebra_check(cfg_name, model_name)


def algebra_check(cfg_name, model_name, dt=DT):
    """the check at step dt (test_dt_host.py runs it at steps other than 2 ms)"""
    B = 4
    m, cfg, d, rows, rng = _problem(cfg_name, model_name, B, seed=31)
    x, u = np.zeros((B, 26)), np.zeros((B, 26))
    x[:, :m.nv], u[:, :m.nv] = rng.normal(0, 0.5, (B, m.nv)), rng.normal(0, 0.5, (B, m.nv))
    res = wbc_workload.tick_gradients(m, cfg, d, x, u, dt, gc.GradFK([m]), rows)
    A0, b0 = _assemble(m, cfg, d, rows, dt)
    # the restatement's rows ARE the oracle's task stack
    scale = max(np.abs(A0).max(), np.abs(b0).max())
    assert res["A"].shape == A0.shape and np.abs(res["A"] - A0).max() <= 1e-12 * scale and np.abs(res["b"] - b0).max() <= 1e-12 * scale
    dA, db = res["dA"], res["db"]
    size = np.abs(A0).max(axis=(1, 2)) + np.abs(b0).max(axis=1)
    l1 = np.abs(dA).sum(axis=(1, 2)) + np.abs(db).sum(axis=1)
    worst = 0.0
    n_coord = 0

    def check(theta, name, i, fd_of):
        nonlocal worst, n_coord
        h = 2.0 ** -10 * np.maximum(1.0, np.abs(theta))
        Ap, bp = fd_of(theta + h)
        Am, bm = fd_of(theta - h)
        step = (theta + h) - (theta - h)
        fd = (np.einsum("bmk,bmk->b", dA, Ap - Am) + np.einsum("bm,bm->b", db, bp - bm)) / step
        bound = K_BOUND * EPS * size * l1 / h
        got = res[name].reshape(B, -1)[:, i]
        ratio = np.abs(got - fd) / bound
        worst = max(worst, ratio.max() * K_BOUND)
        n_coord += 1
        assert (ratio <= 1.0).all(), "%s[%d]: analytic %s, central difference %s, bound %s" % (name, i, got, fd, bound)

    for i in range(capi.TASK_PARAMS_DOUBLES):
        def fd_of(t, i=i):
            r2 = rows.copy()
            r2[:, i] = t
            return _assemble(m, cfg, d, r2, dt)
        check(rows[:, i].copy(), "d_task_params", i, fd_of)
    for f in gc.FIELDS:
        if f not in d:
            continue
        flat = np.asarray(d[f], dtype=np.float64).reshape(B, -1)
        for i in range(flat.shape[1]):
            def fd_of(t, f=f, i=i, flat=flat):
                a2 = flat.copy()
                a2[:, i] = t
                return _assemble(m, cfg, dict(d, **{f: a2.reshape(d[f].shape)}), rows, dt)
            check(flat[:, i].copy(), "d_" + f, i, fd_of)
    print("%s / %s / dt %.7g: %d coordinates x %d instances, worst |analytic - central difference| = %.2f eps (max|A| + max|b|) (|dL/dA|_1 + |dL/db|_1) / h  (bound %g)" % (
        cfg_name, model_name, dt, n_coord, B, worst, K_BOUND))
    # what never reaches b is exactly 0; a switched-off task's entries are exactly 0
    S = wbc_model.TASK_PARAMS_SLICES
    g = res["d_task_params"]
    assert (g[:, S["ee_gain"]].reshape(B, 5, 6)[:, :, 3:] == 0).all()
    for e in range(5):
        if not cfg.task_ee[e]:
            assert (g[:, S["ee_W"]].reshape(B, 5, 6)[:, e] == 0).all() and (g[:, S["ee_w"]][:, e] == 0).all() and (res["d_ee_target"][:, e] == 0).all()
    if not cfg.task_trunk:
        assert (g[:, S["trunk_W"]] == 0).all() and (g[:, S["trunk_gain"]] == 0).all() and (res["d_trunk_target"] == 0).all()
    if not cfg.task_com:
        assert (g[:, S["com_W"]] == 0).all() and (g[:, S["com_gain"]] == 0).all() and (res["d_com_target"] == 0).all()


# ---- end to end
E2E_B = 16
E2E_SEED = {"c2": 3, "full": 3}       # chosen on the CPU: the oracle alone leaves out 0 of 16 instances at both (the count is printed)
H_E2E = 2.0 ** -17      # small enough that the bounds-only configuration keeps its active set across the step (at 2^-10 14 of 16 change it)


def _tick(m, cfg, d, rows):
    ms, cs, pid = common.per_instance_configs([m], [cfg], None, rows)
    dd = dict(d, model_id=pid)
    t = oracle.tick(ms, cs, dd, DT, len(rows), nthreads=8)
    return t, ms, cs, dd


def _sides(a, x):
    p = a["C"].shape[1] > 0
    return np.array([wbc_workload.qp_active_sides(x[i], a["C"][i] if p else None, a["lb"][i], a["ub"][i], a["Clb"][i] if p else None,
                                                  a["Cub"][i] if p else None)[0] for i in range(len(x))])


@pytest.mark.parametrize("cfg_name", ["c2", "full"])
def test_end_to_end_against_directional_differences_of_the_oracle_tick(cfg_name):
    B = E2E_B
    m = tgp._model("a1_wx200")
    cfg = common.config(cfg_name, m)
    seed = E2E_SEED[cfg_name]
    d = common.tick_inputs(m, cfg, B, seed=seed, with_rot=True)
    rows = tgp._random_rows(tgp._rows_of([cfg], None, B), seed + 5, w=(0.5, 2.0), g=(0.5, 2.0))
    rng = np.random.default_rng(seed + 23)
    v = np.zeros((B, 26))
    v[:, :m.nv] = rng.normal(0, 1.0, (B, m.nv))
    t0, ms, cs, dd = _tick(m, cfg, d, rows)
    a0 = oracle.assemble(ms, cs, dd, DT, B)
    assert (t0["status"] == 0).all()
    p = a0["C"].shape[1] > 0
    cert = [wbc_workload.qp_certificate(t0["qdot"][i], A=a0["A"][i], b=a0["b"][i], C_=a0["C"][i] if p else None, lb=a0["lb"][i], ub=a0["ub"][i],
                                        Clb=a0["Clb"][i] if p else None, Cub=a0["Cub"][i] if p else None, v=v[i]) for i in range(B)]
    assert all(c["cert_status"] == capi.CERT_OK for c in cert)
    u = np.stack([c["sens_x"] for c in cert])
    res = wbc_workload.tick_gradients(m, cfg, d, t0["qdot"], u, DT, gc.GradFK([m]), rows)
    # an instance is left out only when a multiplier or a slack is too small to trust the active set across the step
    side0 = _sides(a0, t0["qdot"])
    margin = np.full(B, np.inf)
    for i, c in enumerate(cert):
        y = np.concatenate([c["y_bounds"], c["y_rows"]])
        s, lo, hi, val = wbc_workload.qp_active_sides(t0["qdot"][i], a0["C"][i] if p else None, a0["lb"][i], a0["ub"][i],
                                                      a0["Clb"][i] if p else None, a0["Cub"][i] if p else None)
        ineq = (s == 1) | (s == 2)
        if ineq.any():
            margin[i] = min(margin[i], np.abs(y[ineq]).min())
        free = s == 0
        fin = free & (np.abs(lo) < 1e20)
        if fin.any():
            margin[i] = min(margin[i], (val - lo)[fin].min())
        fin = free & (np.abs(hi) < 1e20)
        if fin.any():
            margin[i] = min(margin[i], (hi - val)[fin].min())
    kappa = np.linalg.cond(a0["H"][:, :m.nv, :m.nv])
    lsum = np.abs(v * t0["qdot"]).sum(axis=1)
    worst = {}
    fields = [("d_task_params", None)] + [("d_" + f, f) for f in gc.fields_read(cfg)]
    left_out = np.zeros(B, dtype=bool)
    report = []
    for name, f in fields:
        theta = rows if f is None else np.asarray(d[f], dtype=np.float64).reshape(B, -1)
        direc = rng.choice([-1.0, 1.0], theta.shape) * rng.uniform(0.5, 1.0, theta.shape) * np.maximum(1.0, np.abs(theta))

        def L(step):
            th = theta + step * direc
            if f is None:
                t, ms2, cs2, dd2 = _tick(m, cfg, d, th)
            else:
                t, ms2, cs2, dd2 = _tick(m, cfg, dict(d, **{f: th.reshape(d[f].shape)}), rows)
            a = oracle.assemble(ms2, cs2, dd2, DT, B)
            return (v * t["qdot"]).sum(axis=1), _sides(a, t["qdot"]), t["status"]
        vals = {s: L(s) for s in (H_E2E, -H_E2E, H_E2E / 2, -H_E2E / 2)}
        fd1 = (vals[H_E2E][0] - vals[-H_E2E][0]) / (2 * H_E2E)
        fd2 = (vals[H_E2E / 2][0] - vals[-H_E2E / 2][0]) / H_E2E
        same = np.ones(B, dtype=bool)
        for s in vals:
            same &= (vals[s][1] == side0).all(axis=1) & (vals[s][2] == 0)
        keep = same & (margin >= 1e-6)
        left_out |= ~keep
        ana = (res[name].reshape(B, -1) * direc).sum(axis=1)
        # rounding floor. The restatement: u solves a linear system in H, so it — and every gradient entry, linear in u — carries a relative
        # error of up to cond(H) eps. The difference quotient: v . qdot is a sum that rounds at eps sum |v_i qdot_i|, over h / 2 (its
        # solver noise is the same at both steps up to sign and already sits in |FD(h) - FD(h/2)|).
        floor = kappa * EPS * (np.abs(res[name].reshape(B, -1) * direc)).sum(axis=1) + EPS * lsum / (H_E2E / 2)
        tol = 4.0 * np.abs(fd1 - fd2) + floor
        err = np.abs(ana - fd2)
        report.append("%s: worst |analytic - FD(h/2)| / tolerance %.3f; |analytic - FD(h/2)| up to %.3e against |FD(h) - FD(h/2)| up to %.3e, floor up to %.3e, |dL| up to %.3e" % (
            name, (err / tol)[keep].max(), err[keep].max(), np.abs(fd1 - fd2)[keep].max(), floor[keep].max(), np.abs(ana)[keep].max()))
        worst[name] = (err[keep] <= tol[keep]).all()
    print("%s: %d of %d instances left out (active set changes across the step, or a multiplier / slack under 1e-6)" % (cfg_name, int(left_out.sum()), B))
    for line in report:
        print("  " + line)
    assert left_out.sum() <= B // 4
    assert all(worst.values()), worst
