"""A 50-digit reference for the SE(3) terms of the state step's VJP (wbc_step_vjp): plain mpmath, from the float64 inputs
exactly as given and the baked model JSON (Model.data) alone.

It imports neither wbc_workload, the oracle nor the library and shares no code with them; the tree walk is kin_reference's. exp6 and the right
Jacobian Jr(xi) = sum_k (-ad_xi)^k / (k + 1)! come from their defining power series (no closed coefficient, no switch), run until a term is
below 10^-(dps + 10), with GUARD further digits underneath: at |omega| dt = 30 and |v| = 30 the terms of the series reach e^60 = 1e26 before
they fall, and the guard digits carry that. The functions whose names begin with an underscore work on mpmath values at the ambient precision
(the host test runs them at 60 digits for its difference quotients); the two public entry points take and return float arrays at DPS.

Conventions are the product's (include/wbc.h): a twist is (linear, angular) in the body frame, q (+) delta = (M exp6(delta_base), joints +
delta_joints), a cotangent g = dL/d delta. The state of a free-flyer is carried as (p, R, joints) with R a matrix, so nothing is rounded
through a quaternion on the way: R(q) is the homogeneous quaternion form of the input as given (kin_reference._quat_matrix), the base
rotation of q_next is R(q) Re as a matrix, and kin_reference._tree is fed that matrix.
"""
import mpmath as mp
import numpy as np

import kin_reference as kr

DPS = 50
GUARD = 40                       # digits under the working precision inside the series
NV = 26
RUNNING, WARMUP = 0, 1           # WBC_ROLLOUT_RUNNING, WBC_ROLLOUT_WARMUP (include/wbc.h)


def _m(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def _vec(v):
    return [_m(x) for x in v]


def hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def twist4(xi):
    """the 4 x 4 matrix of the twist (v, w)"""
    X = mp.zeros(4)
    X[0:3, 0:3] = hat(xi[3:6])
    for i in range(3):
        X[i, 3] = xi[i]
    return X


def ad6(xi):
    """ad of the twist (v, w), linear rows first: [[W, V], [0, W]]"""
    A = mp.zeros(6)
    W, V = hat(xi[3:6]), hat(xi[0:3])
    A[0:3, 0:3] = W
    A[3:6, 3:6] = W
    A[0:3, 3:6] = V
    return A


def Ad6(E):
    """Ad of the 4 x 4 placement (R, p): [[R, [p]x R], [0, R]]"""
    R = E[0:3, 0:3]
    A = mp.zeros(6)
    A[0:3, 0:3] = R
    A[3:6, 3:6] = R
    A[0:3, 3:6] = hat([E[0, 3], E[1, 3], E[2, 3]]) * R
    return A


def _series(X, first_div):
    """I + X / first_div + X^2 / (first_div (first_div + 1)) + ... until a term is below 10^-(dps + 10); GUARD digits underneath"""
    dps = mp.mp.dps
    n = X.rows
    with mp.workdps(dps + GUARD):
        stop = mp.mpf(10) ** -(dps + 10)
        term = mp.eye(n)
        total = mp.eye(n)
        for k in range(1, 4000):
            term = term * X / (k + first_div - 1)
            total += term
            if max(abs(v) for v in term) < stop:
                break
        else:
            raise ArithmeticError("series did not converge")
        return total


def exp6(xi):
    """exp of the twist (v, w) as a 4 x 4 matrix"""
    return _series(twist4(_vec(xi)), 1)


def Jr(xi):
    """the right Jacobian of SE(3): sum_k (-ad_xi)^k / (k + 1)!"""
    return _series(-ad6(_vec(xi)), 2)


def inv4(E):
    R = E[0:3, 0:3].T
    o = mp.eye(4)
    o[0:3, 0:3] = R
    p = -(R * mp.matrix([E[0, 3], E[1, 3], E[2, 3]]))
    for i in range(3):
        o[i, 3] = p[i]
    return o


def _rows(M):
    return [[M[i, j] for j in range(3)] for i in range(3)]


def _estimator(data, p, R_b, joints):
    """the estimator's kinematics at [p, R_b, joints] (joints: idx_q -> value for the 1-DoF joints): the four foot origins, the trunk frame's
    origin, and per velocity column >= 6 the mean over the four feet of the LOCAL_WORLD_ALIGNED linear column (axis x (p_e - o) for a
    revolute joint on the foot's chain, the axis for a prismatic one, 0 off the chain)"""
    q = [mp.mpf(0)] * kr.NQS
    for i in range(3):
        q[i] = p[i]
    for iq, v in joints.items():
        q[iq] = v
    R, o, cols = kr._tree(data, q, base_R=_rows(R_b))
    ids = kr.role_frame_ids(data)
    pos, parent = [], []
    for fid in ids[0:4] + [ids[kr.TRUNK]]:
        f = data["frames"][fid]
        pj = f["parent_joint"]
        pos.append(kr._add(o[pj], kr._mv(R[pj], [_m(v) for v in f["p"]])))
        parent.append(pj)
    Jbar = [[mp.mpf(0)] * 3 for _ in range(NV)]
    for e in range(4):
        for a in kr._chain(data, parent[e]):
            for col, kind, axis in cols[a]:
                lin = kr._cross(axis, kr._sub(pos[e], o[a])) if kind == "rev" else axis
                Jbar[col] = [x + y / 4 for x, y in zip(Jbar[col], lin)]
    return pos[0:4], pos[4], Jbar


def _joint_cols(data):
    """(idx_q, idx_v) of the 1-DoF joints"""
    return [(j["idx_q"], j["idx_v"]) for j in data["joints"][1:] if j["type"] != "FF"]


def _forward_state(data, p, R, th, xd, ft, R_imu, dt, mode):
    """the state step on (p [3], R 3 x 3, th: idx_q -> joint), rates xd [26], foot targets ft [5][3], R_imu (None: no IMU) -> (p_new, R_new,
    th_new): q_next = q (+) dt xd; WARMUP returns it; RUNNING returns the estimator's (mean(ft[0..3]) - R_b BPA, R_b, joints of q_next) with
    R_b the IMU's rotation if given, else q_next's, and BPA the mean of foot minus trunk origins at [p, R_b, joints of q_next] (§3.40)"""
    E = exp6([dt * x for x in xd[0:6]])
    Rn = R * E[0:3, 0:3]
    pn = mp.matrix(p) + R * mp.matrix([E[0, 3], E[1, 3], E[2, 3]])
    thn = {iq: th[iq] + dt * xd[iv] for iq, iv in _joint_cols(data)}
    if mode == WARMUP:
        return [pn[i] for i in range(3)], Rn, thn
    R_b = Rn if R_imu is None else R_imu
    feet, trunk, _ = _estimator(data, p, R_b, thn)
    BPA = mp.matrix([sum(feet[e][i] - trunk[i] for e in range(4)) / 4 for i in range(3)])
    base = mp.matrix([sum(ft[e][i] for e in range(4)) / 4 for i in range(3)]) - R_b * BPA
    return [base[i] for i in range(3)], R_b, thn


def _vjp_state(data, p, R, th, xd, ft, R_imu, dt, g, mode):
    """the VJP of _forward_state: g [26] = dL/d delta_new -> (d_q [26] in the tangent coordinates at (p, R, th), d_qdot [26], d_ft [5][3])"""
    nv = max(iv for _, iv in _joint_cols(data)) + 1
    z = mp.mpf(0)
    xi = [dt * x for x in xd[0:6]]
    gp = mp.matrix(g[0:3])
    c = list(g[0:nv]) + [z] * (NV - nv)
    d_ft = [[z] * 3 for _ in range(5)]
    if mode == RUNNING:
        R_b = R * exp6(xi)[0:3, 0:3] if R_imu is None else R_imu
        thn = {iq: th[iq] + dt * xd[iv] for iq, iv in _joint_cols(data)}
        feet, trunk, Jbar = _estimator(data, p, R_b, thn)
        BPA = [sum(feet[e][i] - trunk[i] for e in range(4)) / 4 for i in range(3)]
        Rg, Rtg = R_b * gp, R_b.T * gp
        rbar = R_b.T * mp.matrix(BPA)
        for e in range(4):
            d_ft[e] = [Rg[i] / 4 for i in range(3)]
        for col in range(6, nv):
            c[col] = g[col] - sum(Jbar[col][i] * gp[i] for i in range(3))
        if R_imu is None:
            t1, t2 = kr._cross(BPA, list(gp)), kr._cross(list(rbar), list(Rtg))
            for i in range(3):
                c[3 + i] = g[3 + i] - t1[i] - t2[i]
        else:
            c[3:6] = [z] * 3
        c[0:3] = [z] * 3
    c6 = mp.matrix(c[0:6])
    d_q, d_x = list(c), [dt * v for v in c]
    if any(v != 0 for v in c6):
        a = Ad6(exp6([-x for x in xi])).T * c6
        j = Jr(xi).T * c6
        for i in range(6):
            d_q[i], d_x[i] = a[i], dt * j[i]
    return d_q, d_x, d_ft


def _state_of(data, q):
    """float q [27] -> (p, R, th) in mpmath"""
    qb = _vec(q[3:7])
    return _vec(q[0:3]), mp.matrix(kr._quat_matrix(*qb)), {iq: _m(q[iq]) for iq, _ in _joint_cols(data)}


def step_vjp(data, q, qdot, foot_targets, dt, g, imu=None, mode=RUNNING):
    """one instance, float inputs as given -> dict(d_q [26], d_qdot [26], d_foot_targets [5, 3]) rounded from DPS digits"""
    with mp.workdps(DPS):
        p, R, th = _state_of(data, np.asarray(q, dtype=np.float64).reshape(-1))
        R_imu = None if imu is None else mp.matrix(kr._quat_matrix(*_vec(imu)))
        ft = [_vec(r) for r in np.asarray(foot_targets, dtype=np.float64).reshape(5, 3)]
        d_q, d_x, d_ft = _vjp_state(data, p, R, th, _vec(qdot), ft, R_imu, _m(dt), _vec(g), mode)
        return dict(d_q=np.array([float(v) for v in d_q]), d_qdot=np.array([float(v) for v in d_x]),
                    d_foot_targets=np.array([[float(v) for v in r] for r in d_ft]))


def base_vjp(xi_rate, dt, c6):
    """the integrate part alone on the base block: (Ad_{exp(-xi)}' c6, dt Jr(xi)' c6) with xi = dt xi_rate formed in mpmath -> two float [6]"""
    with mp.workdps(DPS):
        xi = [_m(dt) * x for x in _vec(xi_rate)]
        c = mp.matrix(_vec(c6))
        a = Ad6(exp6([-x for x in xi])).T * c
        j = Jr(xi).T * c
        return np.array([float(v) for v in a]), np.array([float(_m(dt) * v) for v in j])


def coefficients(t):
    """a = sin t / t, b = (1 - cos t) / t^2, c1 = (t - sin t) / t^3, c2 = (t^2 + 2 cos t - 2) / (2 t^4), c3 = (2 t - 3 sin t + t cos t) /
    (2 t^5) of a float t > 0, from the closed forms with enough digits for their cancellation (t^-5 at t = 1e-9: 45 digits, so DPS + 60)"""
    with mp.workdps(DPS + 60):
        t = _m(t)
        s, c = mp.sin(t), mp.cos(t)
        return (s / t, (1 - c) / t ** 2, (t - s) / t ** 3, (t ** 2 + 2 * c - 2) / (2 * t ** 4), (2 * t - 3 * s + t * c) / (2 * t ** 5))
