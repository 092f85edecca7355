"""The SE(3) terms of the state step's VJP on the host (no GPU): the 50-digit reference held to the definitions it restates, the numpy
restatement wbc_workload.step_gradients held to the reference over the whole ladder of step_se3_cases.py, and a float64 transcription of the
kernel's coefficient routine sv_coef held to mpmath's coefficients.

Bounds. BASE_BOUND = 1e-13 x max(1, max|ref block|) per row and block for the base blocks of WARMUP: plain float64 evaluation of the
documented closed forms errs at most 3.5e-15 against a 60-digit series on this ladder; thirty times that is allowed for contraction into fused
multiply-adds, the device's sine and cosine and its reciprocal sequences (the restatement: for the roundings of up to seven doublings), and it
is still nineteen times under the 1.9e-12 of a build whose coefficients switch to their closed forms at 1e-4. RUNNING: pose_cases.kin_tol's
1e-12 x max(1, |ref|), because 24-joint forward kinematics is in the path.

Measured: the reference against the definitions 8.0e-25 (quotients of the group operations, their own O(h)) and 1.2e-35 (the whole VJP);
step_gradients 1.0e-14 at worst in WARMUP (d_q ang), 6.3e-15 in RUNNING — before it halved its arguments, 5.8e-13 at |omega| dt = 10 and
4.0e-4 at 30; sv_coef 0.79 eps at worst below t = 1, 45 eps in c3 at the seam."""
import math

import mpmath as mp
import numpy as np
import pytest

import gradq_common as gq
import kin_reference as kr
import se3_reference as s3
import step_se3_cases as cases
import wbc_capi as capi
import wbc_workload

BASE_BOUND = 1e-13
KIN_BOUND = 1e-12                                                        # pose_cases.kin_tol
EPS = 2.0 ** -52
U = 2.0 ** -53                                                           # one rounding


def test_capi_modes_are_the_references():
    assert (s3.RUNNING, s3.WARMUP) == (capi.ROLLOUT_RUNNING, capi.ROLLOUT_WARMUP) and s3.NV == capi.V_STRIDE


def test_the_off_axis_seam_pair_lands_on_opposite_sides():
    """w . w summed the kernel's way (w0 w0 + w1 w1 + w2 w2, left to right), with and without every contraction into fused multiply-adds"""
    rows = cases.seam_rows()
    assert all(x < 1.0 for x in cases.norm2_all_ways(rows[0])) and all(x == 1.0 for x in cases.norm2_all_ways(rows[1]))
    assert all(x > 1.0 for x in cases.norm2_all_ways(rows[2])) and all(x == 1.0 for x in cases.norm2_all_ways(rows[5]))
    lo, hi = rows[3], rows[4]
    assert all(x < 1.0 for x in cases.norm2_all_ways(lo)) and all(x >= 1.0 for x in cases.norm2_all_ways(hi))
    assert np.array_equal(lo[0:2], hi[0:2]) and 0 < hi[2] - lo[2] <= 4 * np.spacing(lo[2]) and np.count_nonzero(lo) == 3
    w = lo
    assert (w[0] * w[0] + w[1] * w[1] + w[2] * w[2] < 1.0) and (hi[0] * hi[0] + hi[1] * hi[1] + hi[2] * hi[2] >= 1.0)


# ---- the reference against the definitions
TWISTS = [(0.0, 0.0), (0.0, 1.0), (1e-3, 1e-3), (1.0, 1.0), (math.pi, 30.0), (10.0, 1.0), (30.0, 30.0)]     # (|omega|, |v|)


def _hat6(x):
    return s3.twist4(x)


@pytest.mark.parametrize("t,vm", TWISTS)
def test_jr_and_ad_are_the_derivatives_of_the_group_operations(t, vm):
    """exp6(xi)^-1 exp6(xi + h e_i) = I + h hat(Jr e_i) + O(h^2) and exp6(xi)^-1 exp6(h e_i) exp6(xi) = I + h hat(Ad_{exp(-xi)} e_i) + O(h^2),
    at 60 digits with h = 1e-25: the quotient's rounding is 1e-60 / h = 1e-35 and its O(h) remainder about 1e-25 |xi|^2"""
    rng = np.random.default_rng(int(1000 * t) + int(vm))
    xi = np.concatenate([vm * cases._unit(rng), t * cases._unit(rng)])
    worst = mp.mpf(0)
    with mp.workdps(60):
        h = mp.mpf(10) ** -25
        x = [mp.mpf(float(v)) for v in xi]
        E = s3.exp6(x)
        Ei = s3.inv4(E)
        assert max(abs(v) for v in Ei * E - mp.eye(4)) < mp.mpf(10) ** -55
        J, A = s3.Jr(x), s3.Ad6(s3.exp6([-v for v in x]))
        for i in range(6):
            e = [mp.mpf(int(k == i)) for k in range(6)]
            D = (Ei * s3.exp6([a + h * b for a, b in zip(x, e)]) - mp.eye(4)) / h
            worst = max(worst, max(abs(v) for v in D - _hat6(J * mp.matrix(e))))
            D = (Ei * s3.exp6([h * b for b in e]) * E - mp.eye(4)) / h
            worst = max(worst, max(abs(v) for v in D - _hat6(A * mp.matrix(e))))
    print("|omega| %g, |v| %g: worst |quotient - hat(J e_i)| %.2e" % (t, vm, float(worst)))
    assert worst < mp.mpf(10) ** -20


def _perturbed(data, p, R, th, d, s):
    """(p, R, th) (+) s d"""
    E = s3.exp6([s * v for v in d[0:6]])
    pn = mp.matrix(p) + R * mp.matrix([E[0, 3], E[1, 3], E[2, 3]])
    return [pn[i] for i in range(3)], R * E[0:3, 0:3], {iq: th[iq] + s * d[iv] for iq, iv in s3._joint_cols(data)}


@pytest.mark.parametrize("name,variant,t", [("a1_wx200", "running", 2.0), ("laikago_vx300", "running_imu", 0.3), ("a1_px100_pin_ver", "warmup", 7.0)])
def test_the_reference_vjp_against_differences_of_the_50_digit_forward(name, variant, t):
    """the whole reference VJP against central differences of se3_reference._forward_state (exp6 from its series, then the estimator's formula
    as DESIGN.md §3.40 states it) along random directions in (q tangent, qdot, foot targets) jointly, at 60 digits with h = 1e-25: rounding
    1e-35, truncation 1e-50. The loss is a random linear functional of (R_new, p_new, joints), whose cotangent in the tangent coordinates at
    q_new is g_p = R_new' a, g_phi[k] = <A, R_new hat(e_k)>, g_theta = c."""
    m = cases.model(name)
    data, nv = m.data, m.nv
    rng = np.random.default_rng(len(name))
    mode = s3.WARMUP if variant == "warmup" else s3.RUNNING
    q = wbc_workload.sample_q(m, 1, rng)[0]
    xd = np.zeros(26)
    xd[6:nv] = rng.normal(0, 0.5, nv - 6)
    dt = 0.02
    xd[0:3], xd[3:6] = 1.0 / dt * cases._unit(rng), t / dt * cases._unit(rng)
    ft = rng.normal(0, 0.3, (5, 3))
    imu = None
    if variant == "running_imu":
        imu = q[3:7] + rng.normal(0, 0.05, 4)
        imu /= np.linalg.norm(imu)
    worst = 0.0
    with mp.workdps(60):
        f = lambda a: [mp.mpf(float(v)) for v in a]                                  # noqa: E731
        unit = lambda v: [u / mp.sqrt(sum(w * w for w in v)) for u in v]             # noqa: E731
        p, _, th = s3._state_of(data, q)
        R = mp.matrix(kr._quat_matrix(*unit(f(q[3:7]))))                             # (exactly a rotation: §3.40's forms assume one; a float
        R_imu = None if imu is None else mp.matrix(kr._quat_matrix(*unit(f(imu))))   # quaternion is one to 1e-16, which would show at 1e-20)
        x, fts, dtm = f(xd), [f(r) for r in ft], mp.mpf(dt)
        A, a, c = mp.matrix(3, 3), f(rng.normal(0, 1.0, 3)), f(rng.normal(0, 1.0, 26))
        for i in range(3):
            for j in range(3):
                A[i, j] = mp.mpf(float(rng.normal()))

        def loss(state):
            pn, Rn, thn = state
            return sum(A[i, j] * Rn[i, j] for i in range(3) for j in range(3)) + sum(x * y for x, y in zip(a, pn)) + \
                sum(c[iv] * thn[iq] for iq, iv in s3._joint_cols(data))
        pn, Rn, thn = s3._forward_state(data, p, R, th, x, fts, R_imu, dtm, mode)
        # the forward is kin_reference.integrate's where that applies
        if mode == s3.WARMUP:
            qn = kr.integrate(data, q, dt * xd)
            assert max(abs(float(u) - v) for u, v in zip(pn, qn[0:3])) < 1e-14 * max(1.0, np.abs(qn[0:3]).max())
            Rk = mp.matrix(kr._quat_matrix(*f(qn[3:7])))
            assert max(abs(v) for v in Rk - Rn) < 1e-14
            assert max(abs(float(thn[iq]) - qn[iq]) for iq, _ in s3._joint_cols(data)) < 1e-15
        g = [mp.mpf(0)] * 26
        gp = Rn.T * mp.matrix(a)
        for k in range(3):
            g[k] = gp[k]
            e = [mp.mpf(int(i == k)) for i in range(3)]
            RH = Rn * s3.hat(e)
            g[3 + k] = sum(A[i, j] * RH[i, j] for i in range(3) for j in range(3))
        for iq, iv in s3._joint_cols(data):
            g[iv] = c[iv]
        d_q, d_x, d_ft = s3._vjp_state(data, p, R, th, x, fts, R_imu, dtm, g, mode)
        h = mp.mpf(10) ** -25
        for trial in range(3):
            dq, dx, dft = f(rng.normal(0, 1.0, 26)), f(rng.normal(0, 1.0, 26)), [f(r) for r in rng.normal(0, 1.0, (5, 3))]
            for k in range(nv, 26):
                dq[k] = dx[k] = mp.mpf(0)
            L = []
            for s in (h, -h):
                ps, Rs, ths = _perturbed(data, p, R, th, dq, s)
                L.append(loss(s3._forward_state(data, ps, Rs, ths, [u + s * v for u, v in zip(x, dx)],
                                                [[u + s * v for u, v in zip(r, dr)] for r, dr in zip(fts, dft)], R_imu, dtm, mode)))
            fd = (L[0] - L[1]) / (2 * h)
            an = sum(u * v for u, v in zip(d_q, dq)) + sum(u * v for u, v in zip(d_x, dx)) + \
                sum(u * v for r, dr in zip(d_ft, dft) for u, v in zip(r, dr))
            worst = max(worst, float(abs(fd - an)))
            assert abs(an) > mp.mpf(10) ** -3
    print("%s / %s, |omega| dt %g: worst |analytic - difference| %.2e" % (name, variant, t, worst))
    assert worst < 1e-20


def test_the_trunk_frame_carries_the_base_rotation():
    """§3.40 writes the estimator with R_b, the free-flyer's rotation; the forward rotates by the trunk frame's: the same on every baked model"""
    for n in cases.MODELS:
        data = cases.model(n).data
        f = data["frames"][kr.role_frame_ids(data)[kr.TRUNK]]
        j = data["joints"][f["parent_joint"]]
        assert j["type"] == "FF" and np.array_equal(np.asarray(f["R"]), np.eye(3)) and np.array_equal(np.asarray(j["placement_R"]), np.eye(3))


# ---- the restatement against the reference
def restate(p, dt, mode):
    """wbc_workload.step_gradients over a case of step_se3_cases, model by model"""
    B = len(p["q"])
    out = {k: np.zeros((B,) + shape) for k, shape in capi.STEP_GRAD_FIELDS.items()}
    for i, n in enumerate(p["names"]):
        m = cases.model(n)
        sel = np.ones(B, dtype=bool) if p["mid"] is None else (p["mid"] == i)
        r = wbc_workload.step_gradients(m, p["q"][sel], p["qdot"][sel], p["foot_targets"][sel], dt, p["g"][sel], gq.StateFK([m]),
                                        imu=None if p["imu"] is None else p["imu"][sel], mode=mode)
        for k in out:
            out[k][sel] = r[k]
    return out


def hold(got, p, bounds, what):
    """every block of every row within its bound; -> {block: worst}"""
    errs = cases.block_errors(got, p["ref"])
    worst = {k: float(v.max()) for k, v in errs.items()}
    print("%s, %d rows: worst |got - ref| / max(1, max|ref block|): %s" % (what, len(p["q"]), ", ".join("%s %.2e" % kv for kv in worst.items())))
    for k, v in errs.items():
        b = int(v.argmax())
        assert v[b] <= bounds[k], "%s: %s of row %d (%s): %.3e > %.1e" % (what, k, b, p["labels"][b], v[b], bounds[k])
    return worst


WARMUP_BOUNDS = {k: (BASE_BOUND if k.split()[-1] in ("lin", "ang") else 0.0) for k in cases.BLOCKS}        # joints and foot targets: exact
RUNNING_BOUNDS = {k: KIN_BOUND for k in cases.BLOCKS}


@pytest.mark.parametrize("dt", cases.DTS)
def test_the_restatement_holds_the_device_bound_in_warmup(dt):
    p = cases.warmup_case("mixed", dt)
    hold(restate(p, dt, s3.WARMUP), p, WARMUP_BOUNDS, "step_gradients / warmup / dt %g" % dt)


@pytest.mark.parametrize("imu", [False, True])
@pytest.mark.parametrize("dt", cases.DTS)
def test_the_restatement_holds_the_kinematic_bound_in_running(dt, imu):
    p = cases.running_case("mixed", dt, imu)
    hold(restate(p, dt, s3.RUNNING), p, RUNNING_BOUNDS, "step_gradients / running%s / dt %g" % (" with IMU" if imu else "", dt))


# ---- the kernel's coefficients
SV_TERMS = 10


def _fma(a, b, c):
    return cases._fma(a, b, c)


def _sv_series(off, c3, t2):
    z = -t2
    s = 1.0
    for k in range(SV_TERMS, 0, -1):
        ratio = ((k + 1) / k if c3 else 1.0) / float((2 * k + off - 1) * (2 * k + off))
        s = _fma(z * s, ratio, 1.0)
    return s


def sv_coef(t2):
    """csrc/wbc_k_stepvjp.hip's sv_coef, operation by operation in float64 (the fused multiply-add rounded once)"""
    if t2 < 1.0:
        return (_sv_series(1, False, t2), _sv_series(2, False, t2) * 0.5, _sv_series(3, False, t2) * (1.0 / 6),
                _sv_series(4, False, t2) * (1.0 / 24), _sv_series(5, True, t2) * (1.0 / 120))
    t = math.sqrt(t2)
    s, c = math.sin(t), math.cos(t)
    a = s / t
    b = (1 - c) / t2
    c1 = (1 - a) / t2
    c2 = (0.5 - b) / t2
    c3 = (3 * c1 - b) / (2 * t2)
    return a, b, c1, c2, c3


def _closed_form_bounds(t2, ref):
    """first-order propagation of every rounding of the closed forms, from t2 >= 1 (exact) and the exact coefficients `ref`: each of + - x /
    and the square root errs by U relative, sine and cosine by one ulp = 2 U; -> the absolute bounds of (a, b, c1, c2, c3)"""
    a, b, c1, c2, c3 = (abs(float(v)) for v in ref)
    t = math.sqrt(t2)
    s, c = abs(math.sin(t)), abs(math.cos(t))
    dt_ = U * t
    ds, dc = 2 * U * s + c * dt_, 2 * U * c + s * dt_
    da = ds / t + a * (dt_ / t + U)
    one_c = abs(1 - math.cos(t))
    db = (dc + U * one_c) / t2 + U * b
    dc1 = (da + U * abs(1 - float(ref[0]))) / t2 + U * c1
    dc2 = (db + U * abs(0.5 - float(ref[1]))) / t2 + U * c2
    dc3 = (3 * dc1 + 3 * U * c1 + db + U * abs(3 * float(ref[2]) - float(ref[1]))) / (2 * t2) + U * c3
    return da, db, dc1, dc2, dc3


def test_sv_coef_against_mpmath():
    """a, b, c1, c2, c3 of the kernel's scheme against 110-digit closed forms at 2000 log-spaced t in [1e-9, 30] and the neighbours of the
    seam, t2 = t t being the routine's argument and sqrt(t2) the reference's t.

    Below t = 1 DESIGN.md §3.40 claims that nothing cancels: every partial sum of the nested series lies in [5/6, 1]. Per level the product
    z sum is rounded once (U), the ratio once or, for c3, twice (2 U), the fused multiply-add once (U of a sum <= 1), and the term is at most
    1/6 of the sum: the absolute error e of a level obeys e <= U + (e + 3 U) / 6 (c3: 4 U), so e <= 1.8 U (2 U), 2.2 U (2.4 U) relative to a
    sum >= 5/6; the constant factor adds two roundings (none for a, b), the truncation 1 / 23!. Bound: 4.4 U = 2.2 eps; asserted: 2.5 eps.

    From t = 1 up the closed forms' roundings are propagated to first order (_closed_form_bounds) and doubled for the second order; on top
    of that DESIGN's own figure is held where it is claimed: the worst cancellation is c3's at t = 1, 0.016 from terms of 0.46 — thirty times
    the relative error of those terms, which carry four roundings each (c1: sine, quotient, difference, quotient): 30 x 4 U = 60 eps."""
    ts = list(np.exp(np.linspace(math.log(1e-9), math.log(30.0), 2000)))
    t2s = [t * t for t in ts] + [np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)] + [float(x) for w in cases.seam_rows() for x in cases.norm2_all_ways(w)]
    names = ("a", "b", "c1", "c2", "c3")
    worst_lo, worst_hi, worst_seam = np.zeros(5), np.zeros(5), 0.0
    for t2 in t2s:
        t2 = float(t2)
        got = sv_coef(t2)
        with mp.workdps(s3.DPS + 60):
            ref = s3.coefficients(mp.sqrt(mp.mpf(t2)))
            err = [float(abs(mp.mpf(gv) - r)) for gv, r in zip(got, ref)]
            rel = np.array([e / float(abs(r)) for e, r in zip(err, ref)])
        if t2 < 1.0:
            worst_lo = np.maximum(worst_lo, rel)
            assert (rel <= 2.5 * EPS).all(), "t2 = %r: %s" % (t2, dict(zip(names, rel / EPS)))
        else:
            bound = _closed_form_bounds(t2, ref)
            ratio = np.array([e / (2 * b) for e, b in zip(err, bound)])
            worst_hi = np.maximum(worst_hi, ratio)
            assert (ratio <= 1.0).all(), "t2 = %r: error over the propagated bound: %s" % (t2, dict(zip(names, ratio)))
            if t2 <= 1.0 + 1e-9:
                worst_seam = max(worst_seam, rel[4])
                assert rel[4] <= 60 * EPS, "c3 at t2 = %r: %.1f eps" % (t2, rel[4] / EPS)
    print("sv_coef, t < 1: worst relative error in eps: %s" % ", ".join("%s %.2f" % kv for kv in zip(names, worst_lo / EPS)))
    print("sv_coef, t >= 1: worst error over twice the propagated bound: %s; c3 at the seam %.1f eps" % (
        ", ".join("%s %.3f" % kv for kv in zip(names, worst_hi)), worst_seam / EPS))
