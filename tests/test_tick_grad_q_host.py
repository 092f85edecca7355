"""CPU: the tick as a layer over its state. wbc_tick_vjp_state at the boundary (header, exports, struct sizes, variant count) and its host
restatement wbc_workload.tick_state_gradients, held to the oracle alone:
  kinematics  frame_rows_dq / com_rows_dq against central differences of oracle.fk's J, oMf, Jcom along every tangent coordinate
  algebra     the central difference of oracle.assemble's (A, b, C, Clb, Cub, lb, ub) along every tangent coordinate, contracted with the
              restatement's dL/d(.), against d_q; d_trunk_box_center likewise (linear: the computed bound alone)
  end to end  the directional derivative of v . qdot from oracle.tick at steps h and h / 2 against the restatement fed
              wbc_workload.qp_certificate: the oracle calibrates its own error
  raw         tangent_to_raw against a central difference in raw coordinates of the tick composed with the quaternion's normalisation"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
import grad_common as gc
import gradq_common as gq
import oracle
import test_gpu_task_params as tgp
import wbc_capi as capi
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
DT = gc.DT
MODELS = ["a1_wx200", "a1_px100_pin_ver", "laikago_vx300"]


def test_header_declares_and_library_exports_the_state_gradient():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert re.search(r"int\s+wbc_tick_vjp_state\s*\(\s*WbcBatch\s*\*", header) and re.search(r"int\s+wbc_tick_state_grad_sizes\s*\(", header)
    for word in ("WbcTickSens", "WbcTickStateGrad", "d_q", "d_trunk_box_center", "sens_bounds", "y_rows", "working_set", "last_gradq_variant",
                 "pin.integrate", "HELD CONSTANT", "q_con", "kinematic Hessians", "roll-outs"):
        assert word in header, word
    lib = capi.load_library()
    for name in ("wbc_tick_vjp_state", "wbc_tick_state_grad_sizes"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    s, g = C.c_int32(), C.c_int32()
    assert lib.wbc_tick_state_grad_sizes(C.byref(s), C.byref(g)) == 0
    assert s.value == C.sizeof(capi.WbcTickSens) and g.value == C.sizeof(capi.WbcTickStateGrad)
    assert lib.wbc_variant_count(b"gradq") == 2                          # ROT off / on
    assert "gradq" not in capi.VARIANT_FAMILIES and "grad" not in capi.VARIANT_FAMILIES


# ---- kinematics
# The rounding floor's constant. An entry of J comes through a chain of at most 7 placements, each a 3 x 3 product (3 products, 2 sums: <= 5
# roundings of the largest entry), the LOCAL_WORLD_ALIGNED shift adds a cross product (<= 3), and the row's product with z sums 26 terms
# (<= 26): 7 x 5 + 3 + 26 = 64 eps of max|J| |z|_1, at q (+) h and q (-) h, over 2 h -> 64. A test that needs more is wrong.
K_KIN = 64.0
H_KIN = 2.0 ** -12


def _tangent_fd(models, q, k, h, f):
    dl = np.zeros((len(q), capi.V_STRIDE))
    dl[:, k] = h
    return (f(gq.step(models, q, dl)) - f(gq.step(models, q, -dl))) / (2 * h)


@pytest.mark.parametrize("model_name", MODELS)
def test_row_derivatives_against_central_differences_of_the_kinematics(model_name):
    B = 4
    m = tgp._model(model_name)
    rng = np.random.default_rng(7)
    q = wbc_workload.sample_q(m, B, rng)
    z = np.zeros((B, capi.V_STRIDE))
    z[:, :m.nv] = rng.normal(0, 1.0, (B, m.nv))
    f0 = oracle.fk([m], q)
    znorm = np.abs(z).sum(axis=1)
    roles = [(capi.FR_EE0 + e, w) for e in range(capi.NEE) for w in (False, True)] + [(capi.FR_TRUNK, True), (capi.FR_TRUNK, False)]
    worst = 0.0
    for role, world in roles + [("com", None)]:
        if role == "com":
            ana = wbc_workload.com_rows_dq(m, f0["J"], f0["oMi"], z)
            rows_of = lambda qq: np.einsum("brk,bk->br", oracle.fk([m], qq)["Jcom"], z)      # noqa: E731
            jmax = np.abs(f0["Jcom"]).max(axis=(1, 2))
        else:
            ana = wbc_workload.frame_rows_dq(m, f0["J"], f0["oMf"], role, world, z)

            def rows_of(qq, role=role, world=world):
                f = oracle.fk([m], qq, want_com=False)
                return np.einsum("brk,bk->br", wbc_workload.frame_rows(m, f["J"], f["oMf"], role, world), z)
            jmax = np.abs(wbc_workload.frame_rows(m, f0["J"], f0["oMf"], role, world)).max(axis=(1, 2))
        for k in range(m.nv):
            fd1, fd2 = _tangent_fd([m], q, k, H_KIN, rows_of), _tangent_fd([m], q, k, H_KIN / 2, rows_of)
            tol = 4.0 * np.abs(fd1 - fd2) + (K_KIN * EPS * jmax * znorm / (H_KIN / 2))[:, None]
            err = np.abs(ana[:, :, k] - fd2)
            worst = max(worst, (err / tol).max())
            assert (err <= tol).all(), "%s role %s world %s k %d: analytic %s, FD %s, tol %s" % (model_name, role, world, k, ana[:, :, k], fd2, tol)
        assert (ana[:, :, m.nv:] == 0).all()
    print("%s: %d row sets x %d tangent coordinates x %d instances, worst |analytic - FD(h/2)| / tolerance %.3f" % (
        model_name, len(roles) + 1, m.nv, B, worst))


# ---- algebra
K_BOUND = 16.0     # test_tick_grad_host.py counts it: <= 12 roundings of the largest entry per difference quotient, contraction and analytic value
H_ALG = 2.0 ** -12
QP_KEYS = ("A", "b", "C", "Clb", "Cub", "lb", "ub")
GRAD_OF = dict(A="dA", b="db", C="dC", Clb="dClb", Cub="dCub", lb="dlb", ub="dub")


def _random_sides(rng, B, n):
    up = rng.integers(0, 2, (B, n))
    return ((1 << (np.arange(n)[None, :] + 32 * up)).sum(axis=1)).astype(np.uint64)


def _algebra_problem(cfg_name, model_name, B, seed, dt=DT, inputs=None):
    m = tgp._model(model_name)
    if inputs is None:
        cfg = common.config(cfg_name, m)
        d = common.tick_inputs(m, cfg, B, seed=seed, with_rot=True)
    else:                                                                # inputs(model, cfg_name, B, seed) -> (configuration, tick inputs)
        cfg, d = inputs(m, cfg_name, B, seed)
    rng = np.random.default_rng(seed + 17)
    if cfg.task_joint >= capi.JOINT_MANI:
        d["posture_u"] = rng.normal(0, 0.3, (B, capi.V_STRIDE))
    rows = tgp._random_rows(tgp._rows_of([cfg], None, B), seed + 5)
    p = oracle.constraint_rows(cfg)
    x, u = np.zeros((B, 26)), np.zeros((B, 26))
    x[:, :m.nv], u[:, :m.nv] = rng.normal(0, 0.5, (B, m.nv)), rng.normal(0, 0.5, (B, m.nv))
    w, y, wb = rng.normal(0, 1, (B, p)), rng.normal(0, 1, (B, p)), rng.normal(0, 1, (B, 26))
    ws = np.stack([_random_sides(rng, B, 26), _random_sides(rng, B, p) if p else np.zeros(B, np.uint64)], axis=1)
    res = wbc_workload.tick_state_gradients(m, cfg, d, x, u, dt, gq.StateFK([m]), wb, w, y, rows, ws)
    ms, cs, pid = common.per_instance_configs([m], [cfg], None, rows)
    return m, cfg, d, res, (lambda dd: oracle.assemble(ms, cs, dict(dd, model_id=pid), dt, B)), ms, pid


def _finite(a):
    return np.where(np.abs(a) < 1e20, a, 0.0)


def _contract(res, ap, am, B):
    out = np.zeros(B)
    for k in QP_KEYS:
        out += (res[GRAD_OF[k]].reshape(B, -1) * (_finite(ap[k]) - _finite(am[k])).reshape(B, -1)).sum(axis=1)
    return out


@pytest.mark.parametrize("model_name", MODELS)
@pytest.mark.parametrize("cfg_name", ["everything", "c3_trunk_task", "c2", "c3_custom", "c3_nobounds"])
def test_algebra_against_central_differences_of_the_assembly(cfg_name, model_name):
    algebra_check(cfg_name, model_name)


def algebra_check(cfg_name, model_name, dt=DT, inputs=None, B=4):
    """the check at step dt (test_dt_host.py runs it at steps other than 2 ms), on the inputs of a recipe other than tick_inputs where one is
    given (test_damper_envelope_host.py); -> (model, configuration, inputs)"""
    m, cfg, d, res, asm, ms, pid = _algebra_problem(cfg_name, model_name, B, seed=31, dt=dt, inputs=inputs)
    a0 = asm(d)
    size = sum(np.abs(_finite(a0[k])).reshape(B, -1).max(axis=1, initial=0.0) for k in QP_KEYS)
    l1 = sum(np.abs(res[GRAD_OF[k]]).reshape(B, -1).sum(axis=1) for k in QP_KEYS)
    worst = 0.0
    for k in range(m.nv):
        fd = []
        for h in (H_ALG, H_ALG / 2):
            dl = np.zeros((B, 26))
            dl[:, k] = h
            fd.append(_contract(res, asm(dict(d, q=gq.step(ms, d["q"], dl, pid))), asm(dict(d, q=gq.step(ms, d["q"], -dl, pid))), B) / (2 * h))
        tol = 4.0 * np.abs(fd[0] - fd[1]) + K_BOUND * EPS * size * l1 / (H_ALG / 2)
        err = np.abs(res["d_q"][:, k] - fd[1])
        worst = max(worst, (err / tol).max())
        assert (err <= tol).all(), "d_q[%d]: analytic %s, central difference %s, tolerance %s" % (k, res["d_q"][:, k], fd[1], tol)
    assert (res["d_q"][:, m.nv:] == 0).all() and np.abs(res["d_q"]).max() > 0
    print("%s / %s / dt %.7g: %d tangent coordinates x %d instances, worst |analytic - FD(h/2)| / tolerance %.3f" % (cfg_name, model_name, dt, m.nv, B, worst))
    if cfg.con_trunk:                                                    # linear in the centre: the computed bound alone
        c = np.asarray(d["trunk_box_center"], dtype=np.float64)
        for i in range(4):
            h = 2.0 ** -10 * np.maximum(1.0, np.abs(c[:, i]))
            cp, cm = c.copy(), c.copy()
            cp[:, i] += h
            cm[:, i] -= h
            fdv = _contract(res, asm(dict(d, trunk_box_center=cp)), asm(dict(d, trunk_box_center=cm)), B) / (cp[:, i] - cm[:, i])
            bound = K_BOUND * EPS * size * l1 / h
            assert (np.abs(res["d_trunk_box_center"][:, i] - fdv) <= bound).all(), (i, res["d_trunk_box_center"][:, i], fdv, bound)
        assert np.abs(res["d_trunk_box_center"]).min() > 0
    else:
        assert (res["d_trunk_box_center"] == 0).all()
    return m, cfg, d


# ---- end to end
# Which instances are left out. test_tick_grad_host.py's rule: the active set changes across the step, or a multiplier / slack is under 1e-6. Its
# two cases (c2, full) have multipliers of order 1e-3 .. 1. On the sim3 switch set (c3) the posture rows (d^2 ~ 1.6e-9) are all that resists
# on the arm DoF whose damper bound is active, and EVERY such multiplier is of order 1e-10 .. 1e-8: taken absolutely, 1e-6 leaves out 5, 6, 7
# of 16 near the stance and 10, 12, 14 of 16 far from it (seeds 3, 4, 5; measured with the oracle alone) — exactly the instances with a
# q-dependent damper bound that this test is there to see. So the multiplier is measured in units of min(1, the instance's largest multiplier of
# an active inequality) (MARGIN_NOTE below): where a multiplier reaches 1 this IS the existing rule, elsewhere it leaves out fewer instances,
# never more, and what is kept has to hold the same tolerance. The slack threshold and the active-set comparison at all four steps are unchanged.
E2E_B = 16
H_E2E = 2.0 ** -20
E2E_CASES = [("c2", "near", 3), ("c3", "near", 3), ("c3_trunk_task", "near", 3), ("everything", "near", 3), ("full", "near", 3), ("c3", "far", 3),
             ("c3", "far", 4)]


def _e2e_setup(cfg_name, kind, seed, inputs=None):
    B = E2E_B
    m = tgp._model("a1_wx200")
    if inputs is None:
        cfg = common.config(cfg_name, m)
        d = (common.tick_inputs if kind == "near" else common.far_tick_inputs)(m, cfg, B, seed=seed, with_rot=True)
    else:                                                                # as _algebra_problem
        cfg, d = inputs(m, cfg_name, B, seed)
    rng = np.random.default_rng(seed + 23)
    v = gc.task_space_v([m], [cfg], None, d, rng)
    return m, cfg, d, rng, v


def _tick_of(m, cfg, d):
    t = oracle.tick([m], [cfg], d, DT, E2E_B, nthreads=8)
    a = oracle.assemble([m], [cfg], d, DT, E2E_B)
    return t, a


def _sides(a, x):
    p = a["C"].shape[1] > 0
    return np.array([wbc_workload.qp_active_sides(x[i], a["C"][i] if p else None, a["lb"][i], a["ub"][i], a["Clb"][i] if p else None,
                                                  a["Cub"][i] if p else None)[0] for i in range(len(x))])


def _certified(m, cfg, d, v):
    """-> (tick, assembly, certificates, restatement, side0, margin): the oracle's tick, its certificate by numpy, the state gradient"""
    B = E2E_B
    t0, a0 = _tick_of(m, cfg, d)
    assert (t0["status"] == 0).all()
    p = a0["C"].shape[1] > 0
    cert = [wbc_workload.qp_certificate(t0["qdot"][i], A=a0["A"][i], b=a0["b"][i], C_=a0["C"][i] if p else None, lb=a0["lb"][i], ub=a0["ub"][i],
                                        Clb=a0["Clb"][i] if p else None, Cub=a0["Cub"][i] if p else None, v=v[i]) for i in range(B)]
    assert all(c["cert_status"] == capi.CERT_OK for c in cert)
    st = lambda k: np.stack([c[k] for c in cert])      # noqa: E731
    res = wbc_workload.tick_state_gradients(m, cfg, d, t0["qdot"], st("sens_x"), DT, gq.StateFK([m]), st("sens_bounds"), st("sens_rows"), st("y_rows"))
    side0 = _sides(a0, t0["qdot"])
    margin = np.full(B, np.inf)
    for i, c in enumerate(cert):
        y = np.concatenate([c["y_bounds"], c["y_rows"]])
        s, lo, hi, val = wbc_workload.qp_active_sides(t0["qdot"][i], a0["C"][i] if p else None, a0["lb"][i], a0["ub"][i],
                                                      a0["Clb"][i] if p else None, a0["Cub"][i] if p else None)
        ineq = (s == 1) | (s == 2)
        if ineq.any():                                                   # (MARGIN_NOTE: in units of min(1, the instance's largest such multiplier))
            margin[i] = min(margin[i], np.abs(y[ineq]).min() / min(1.0, np.abs(y[ineq]).max()))
        for bnd, gap in ((lo, val - lo), (hi, hi - val)):
            fin = (s == 0) & (np.abs(bnd) < 1e20)
            if fin.any():
                margin[i] = min(margin[i], gap[fin].min())
    return t0, a0, cert, res, side0, margin


def _directional(m, cfg, d, v, q_of, side0, margin, ana, scale_terms, t0, a0, what):
    """FD of v . qdot along q_of(step) at h and h / 2 against `ana`; -> (kept, report line). The existing end-to-end test's tolerance."""
    B = E2E_B

    def L(step):
        dd = dict(d, q=q_of(step))
        t, a = _tick_of(m, cfg, dd)
        return (v * t["qdot"]).sum(axis=1), _sides(a, t["qdot"]), t["status"]
    vals = {s: L(s) for s in (H_E2E, -H_E2E, H_E2E / 2, -H_E2E / 2)}
    fd1 = (vals[H_E2E][0] - vals[-H_E2E][0]) / (2 * H_E2E)
    fd2 = (vals[H_E2E / 2][0] - vals[-H_E2E / 2][0]) / H_E2E
    same = np.ones(B, dtype=bool)
    for s in vals:
        same &= (vals[s][1] == side0).all(axis=1) & (vals[s][2] == 0)
    keep = same & (margin >= 1e-6)
    kappa = np.linalg.cond(a0["H"][:, :m.nv, :m.nv])
    lsum = np.abs(v * t0["qdot"]).sum(axis=1)
    floor = kappa * EPS * scale_terms + EPS * lsum / (H_E2E / 2)
    tol = 4.0 * np.abs(fd1 - fd2) + floor
    err = np.abs(ana - fd2)
    line = "%s: %d of %d kept; worst |analytic - FD(h/2)| / tolerance %.3f; |analytic - FD(h/2)| up to %.3e against |FD(h) - FD(h/2)| up to %.3e (relative %.2e), floor up to %.3e" % (
        what, keep.sum(), B, (err / tol)[keep].max(), err[keep].max(), np.abs(fd1 - fd2)[keep].max(),
        (np.abs(fd1 - fd2) / np.maximum(np.abs(fd2), 1e-300))[keep].max(), floor[keep].max())
    return keep, (err[keep] <= tol[keep]).all(), line


@pytest.mark.parametrize("cfg_name,kind,seed", E2E_CASES)
def test_end_to_end_against_directional_differences_of_the_oracle_tick(cfg_name, kind, seed):
    end_to_end_check(cfg_name, kind, seed)


def end_to_end_check(cfg_name, kind, seed, inputs=None):
    """-> (model, configuration, inputs, kept instances, the oracle's tick, its assembly, the active side of every bound and row)"""
    B = E2E_B
    m, cfg, d, rng, v = _e2e_setup(cfg_name, kind, seed, inputs)
    t0, a0, cert, res, side0, margin = _certified(m, cfg, d, v)
    direc = np.zeros((B, 26))
    direc[:, :m.nv] = rng.choice([-1.0, 1.0], (B, m.nv)) * rng.uniform(0.5, 1.0, (B, m.nv))
    keep, ok, line = _directional(m, cfg, d, v, lambda s: gq.step([m], d["q"], s * direc), side0, margin, (res["d_q"] * direc).sum(axis=1),
                                  np.abs(res["d_q"] * direc).sum(axis=1), t0, a0, "%s / %s / seed %d, d_q" % (cfg_name, kind, seed))
    print(line)
    assert (~keep).sum() <= B // 4
    if kind == "far":                                                    # the trunk box's inequality rows take part
        n = sum(1 for i in range(B) if keep[i] and (np.abs(cert[i]["sens_rows"][0:4]) > 0).any())
        print("  instances with an active trunk-box row: %d" % n)
        assert n >= 4
    elif cfg.use_bounds:                                                 # ... and the q-dependent damper bounds
        act = (side0[:, :26] == 1) | (side0[:, :26] == 2)
        vmax = np.array([cfg.damper_vmax[i] for i in range(26)])[None, :]
        e = np.where(side0[:, :26] == 1, a0["lb"], a0["ub"])
        n = int(((act & (np.abs(np.abs(e) - vmax) > 1e-12) & (e != 0)).any(axis=1) & keep).sum())
        print("  instances with an active damper bound that is not +-v_max: %d" % n)
        assert n >= 4
    assert ok, line
    return m, cfg, d, keep, t0, a0, side0


def test_tangent_to_raw_against_a_central_difference_in_raw_coordinates():
    """the raw-coordinate gradient is that of the tick composed with the normalisation of the quaternion"""
    B = E2E_B
    m, cfg, d, rng, v = _e2e_setup("c3", "near", 3)
    t0, a0, cert, res, side0, margin = _certified(m, cfg, d, v)
    raw = wbc_workload.tangent_to_raw(d["q"], res["d_q"])
    assert np.abs((raw[:, 3:7] * d["q"][:, 3:7]).sum(axis=1)).max() <= 64 * EPS * np.abs(raw[:, 3:7]).max()   # nothing along the quaternion itself
    direc = np.zeros((B, 27))
    direc[:, :m.nq] = rng.choice([-1.0, 1.0], (B, m.nq)) * rng.uniform(0.5, 1.0, (B, m.nq))

    def q_of(s):
        qq = d["q"] + s * direc
        qq[:, 3:7] /= np.linalg.norm(qq[:, 3:7], axis=1, keepdims=True)
        return qq
    keep, ok, line = _directional(m, cfg, d, v, q_of, side0, margin, (raw * direc).sum(axis=1), np.abs(raw * direc).sum(axis=1), t0, a0,
                                  "c3 / near / seed 3, raw coordinates")
    print(line)
    assert (~keep).sum() <= B // 4 and ok, line
