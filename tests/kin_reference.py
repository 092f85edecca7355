"""A high-precision kinematics reference for the tests: plain mpmath at 50 digits, from the baked model JSON (Model.data) alone.

It imports neither the oracle nor the library and shares no code with either (nor with test_laikago_host._fk_numpy): textbook forms only.
A Jacobian column is axis x (p - p_joint) stacked on axis; the centre of mass is the mass-weighted sum of the bodies' centres and its
Jacobian the subtree form of the same sum; rotations come from the Rodrigues formula with no small-angle series (50 digits carry the
cancellation); a quaternion is read off a matrix by whichever of the four branches is largest. Conventions are the product's
(include/wbc.h): q = (x, y, z, quaternion (x, y, z, w), 1-DoF joints), v = (body-frame linear, body-frame angular, 1-DoF rates), a placement
is 9 row-major rotation entries then 3 of position, Jacobians are [6][26] with the linear rows first.
"""
import mpmath as mp
import numpy as np

DPS = 50
NV, NQS = 26, 27

# the controller's frames in the order of WbcFkOut.oMf (include/wbc.h, WBC_FR_*): (name, kind of frame)
ROLE_FRAMES = ([(n, "FIXED_JOINT") for n in ("FR_foot_fixed", "FL_foot_fixed", "RR_foot_fixed", "RL_foot_fixed", "gripper_bar", "imu_joint")] +
               [(n, "JOINT") for n in ("FR_hip_joint", "FL_hip_joint", "RR_hip_joint", "RL_hip_joint", "waist", "waist")])
TRUNK = 5


def _f(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))      # (se3_reference.py feeds _tree values that are mpmath's already)


def _mat(rows):
    return [[_f(v) for v in r] for r in rows]


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _mv(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _add(a, b):
    return [x + y for x, y in zip(a, b)]


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _eye():
    return [[mp.mpf(int(i == j)) for j in range(3)] for i in range(3)]


def _hat(w):
    z = mp.mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def _rodrigues(axis, angle):
    """rotation by `angle` about the UNIT vector `axis`: I + sin(angle) K + (1 - cos(angle)) K^2"""
    K = _hat(axis)
    K2 = _mm(K, K)
    s, c = mp.sin(angle), 1 - mp.cos(angle)
    I = _eye()
    return [[I[i][j] + s * K[i][j] + c * K2[i][j] for j in range(3)] for i in range(3)]


def _quat_matrix(qx, qy, qz, qw):
    """the matrix of the quaternion AS GIVEN (not normalised first): the homogeneous form 2 (v v' + w [v]x) + (1 - 2 v.v) I that equals the
    rotation for a unit quaternion — the product's definition of the free-flyer's attitude"""
    v = [qx, qy, qz]
    K = _hat(v)
    vv = qx * qx + qy * qy + qz * qz
    I = _eye()
    return [[2 * (v[i] * v[j] + qw * K[i][j]) + (1 - 2 * vv) * I[i][j] for j in range(3)] for i in range(3)]


def _euler_xyz(M):
    """(a, b, c) with M = Rz(c) Ry(b) Rx(a)"""
    return [mp.atan2(M[2][1], M[2][2]), mp.atan2(-M[2][0], mp.sqrt(M[2][1] ** 2 + M[2][2] ** 2)), mp.atan2(M[1][0], M[0][0])]


def _matrix_quat(M):
    """(x, y, z, w) of a rotation matrix, from the largest of the four squared components (Shepperd)"""
    tr = M[0][0] + M[1][1] + M[2][2]
    four = [1 + 2 * M[0][0] - tr, 1 + 2 * M[1][1] - tr, 1 + 2 * M[2][2] - tr, 1 + tr]       # 4 x^2, 4 y^2, 4 z^2, 4 w^2
    c = max(range(4), key=lambda i: four[i])
    s = mp.sqrt(four[c])                                                                  # 2 |component c|
    asym = [M[2][1] - M[1][2], M[0][2] - M[2][0], M[1][0] - M[0][1]]                      # 4 w (x, y, z)
    q = [None] * 4
    if c == 3:
        q[3] = s / 2
        for i in range(3):
            q[i] = asym[i] / (2 * s)
    else:
        q[c] = s / 2
        q[3] = asym[c] / (2 * s)
        for i in range(3):
            if i != c:
                q[i] = (M[i][c] + M[c][i]) / (2 * s)                                      # 4 q_i q_c
    return q


def _out12(R, p):
    return [float(R[i][j]) for i in range(3) for j in range(3)] + [float(v) for v in p]


def role_frame_ids(data):
    ids = []
    for name, kind in ROLE_FRAMES:
        ids.append(next(i for i, f in enumerate(data["frames"]) if f["name"] == name and f["type"] == kind))
    return ids


def _tree(data, q, base_R=None):
    """world rotation R[j], origin p[j] of every joint, and per joint the list of (velocity column, kind, world axis): kind "rev" turns about the
    axis through p[j], "lin" slides along it. base_R: the free-flyer's rotation as a 3 x 3 of mpmath values, in place of the quaternion's"""
    js = data["joints"]
    R, p, cols = [_eye()], [[mp.mpf(0)] * 3], [[]]
    for j in js[1:]:
        P, t = _mat(j["placement_R"]), [_f(v) for v in j["placement_p"]]
        kind = j["type"]
        Rl, pl = _eye(), [mp.mpf(0)] * 3
        if kind == "FF":
            i = j["idx_q"]
            Rl = _quat_matrix(*[_f(v) for v in q[i + 3:i + 7]]) if base_R is None else base_R
            pl = [_f(v) for v in q[i:i + 3]]
        else:
            e = [mp.mpf(int(k == "XYZ".index(kind[1]))) for k in range(3)]
            if kind[0] == "R":
                Rl = _rodrigues(e, _f(q[j["idx_q"]]))
            else:
                pl = [_f(q[j["idx_q"]]) * v for v in e]
        Rp, pp = R[j["parent"]], p[j["parent"]]
        Rj = _mm(Rp, _mm(P, Rl))
        pj = _add(pp, _mv(Rp, _add(t, _mv(P, pl))))
        R.append(Rj)
        p.append(pj)
        v = j["idx_v"]
        axes = [[Rj[r][k] for r in range(3)] for k in range(3)]
        if kind == "FF":
            cols.append([(v + k, "lin", axes[k]) for k in range(3)] + [(v + 3 + k, "rev", axes[k]) for k in range(3)])
        else:
            cols.append([(v, "rev" if kind[0] == "R" else "lin", axes["XYZ".index(kind[1])])])
    return R, p, cols


def _chain(data, j):
    out = []
    while j > 0:
        out.append(j)
        j = data["joints"][j]["parent"]
    return out


def _point_jacobian(data, p, cols, joint, point):
    """6 x NV: the velocity of `point` (carried by `joint`) on world axes, stacked on the angular velocity of that body"""
    J = np.zeros((6, NV))
    for a in _chain(data, joint):
        for col, kind, axis in cols[a]:
            lin = _cross(axis, _sub(point, p[a])) if kind == "rev" else axis
            for r in range(3):
                J[r, col] = float(lin[r])
                if kind == "rev":
                    J[3 + r, col] = float(axis[r])
    return J


def fk(data, q, frames=None):
    """One configuration q [27] -> dict of float arrays in WbcFkOut's layouts: oMi [nj, 12], oMf [nf, 12], J [6, 26] (WORLD: the reference point
    of every column is the world origin), Jf [nf, 6, 26] (LOCAL_WORLD_ALIGNED Jacobian of every frame), com [3], Jcom [3, 26],
    euler [3] (xyz angles of the trunk frame). frames: indices into data["frames"] (default: the controller's role frames)."""
    with mp.workdps(DPS):
        q = np.asarray(q, dtype=np.float64).reshape(-1)
        js = data["joints"]
        nj = len(js)
        R, p, cols = _tree(data, q)
        out = dict(oMi=np.array([_out12(R[j], p[j]) for j in range(nj)]))
        # data.J: every column taken at the world origin
        J = np.zeros((6, NV))
        origin = [mp.mpf(0)] * 3
        for j in range(1, nj):
            for col, kind, axis in cols[j]:
                lin = _cross(axis, _sub(origin, p[j])) if kind == "rev" else axis
                for r in range(3):
                    J[r, col] = float(lin[r])
                    if kind == "rev":
                        J[3 + r, col] = float(axis[r])
        out["J"] = J
        ids = role_frame_ids(data) if frames is None else list(frames)
        oMf, Jf = [], []
        for fid in ids:
            f = data["frames"][fid]
            pj = f["parent_joint"]
            Rf = _mm(R[pj], _mat(f["R"]))
            pf = _add(p[pj], _mv(R[pj], [_f(v) for v in f["p"]]))
            oMf.append(_out12(Rf, pf))
            Jf.append(_point_jacobian(data, p, cols, pj, pf))
            if frames is None and len(oMf) == TRUNK + 1:
                out["euler"] = np.array([float(v) for v in _euler_xyz(Rf)])
        out["oMf"], out["Jf"] = np.array(oMf), np.array(Jf)
        # centre of mass: sum of m_j c_j over the bodies; subtree sums for the Jacobian
        m = [_f(j["mass"]) for j in js]
        c = [_add(p[j], _mv(R[j], [_f(v) for v in js[j]["com"]])) for j in range(nj)]
        M = sum(m)
        out["com"] = np.array([float(sum(m[j] * c[j][r] for j in range(nj)) / M) for r in range(3)])
        sub = [[j] for j in range(nj)]
        for j in range(nj - 1, 0, -1):
            sub[js[j]["parent"]] += sub[j]
        Jc = np.zeros((3, NV))
        for j in range(1, nj):
            ms = sum(m[k] for k in sub[j])
            if ms == 0:
                continue
            cs = [sum(m[k] * c[k][r] for k in sub[j]) / ms for r in range(3)]
            for col, kind, axis in cols[j]:
                lin = _cross(axis, _sub(cs, p[j])) if kind == "rev" else axis
                for r in range(3):
                    Jc[r, col] = float(ms / M * lin[r])
        out["Jcom"] = Jc
        return out


def quat_euler(quat, frame_R=None):
    """xyz angles of the attitude of quaternion (x, y, z, w) (times a fixed frame rotation): the trunk angles of a free-flyer pose without the tree"""
    with mp.workdps(DPS):
        M = _quat_matrix(*[_f(v) for v in quat])
        if frame_R is not None:
            M = _mm(M, _mat(frame_R))
        return np.array([float(v) for v in _euler_xyz(M)])


def trunk_euler(data, q):
    """xyz angles of the trunk frame when it hangs on the free-flyer joint itself (every baked model); else through the whole tree"""
    f = data["frames"][role_frame_ids(data)[TRUNK]]
    j = data["joints"][f["parent_joint"]]
    if j["type"] == "FF" and j["parent"] == 0 and np.array_equal(np.asarray(j["placement_R"]), np.eye(3)):
        return quat_euler(q[j["idx_q"] + 3:j["idx_q"] + 7], f["R"])
    return fk(data, q)["euler"]


def integrate(data, q, v):
    """q [27], v [26] (the tangent step, = rate x dt) -> q_next [27]: the free-flyer goes to M exp6(v) with v a body-frame twist, its quaternion
    read off the matrix, given the sign that keeps it continuous with the input and renormalised to first order (x (3 - |q|^2) / 2);
    a 1-DoF joint goes to q + v"""
    with mp.workdps(DPS):
        q = np.asarray(q, dtype=np.float64).reshape(-1)
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        out = np.zeros(NQS)
        for j in data["joints"][1:]:
            iq, iv = j["idx_q"], j["idx_v"]
            if j["type"] != "FF":
                out[iq] = float(_f(q[iq]) + _f(v[iv]))
                continue
            lin, w = [_f(x) for x in v[iv:iv + 3]], [_f(x) for x in v[iv + 3:iv + 6]]
            q0 = [_f(x) for x in q[iq + 3:iq + 7]]
            R0 = _quat_matrix(*q0)
            t = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
            if t == 0:
                Re, pe = _eye(), lin
            else:
                u = [x / t for x in w]
                Re = _rodrigues(u, t)
                # the translation of exp6: V lin, V = I + (1 - cos t) / t K + (t - sin t) / t K^2 with K = [u]x
                K = _hat(u)
                K2 = _mm(K, K)
                a, b = (1 - mp.cos(t)) / t, (t - mp.sin(t)) / t
                pe = _add(lin, _add([a * x for x in _mv(K, lin)], [b * x for x in _mv(K2, lin)]))
            R1 = _mm(R0, Re)
            p1 = _add([_f(x) for x in q[iq:iq + 3]], _mv(R0, pe))
            qq = _matrix_quat(R1)
            if sum(x * y for x, y in zip(qq, q0)) < 0:
                qq = [-x for x in qq]
            f = (3 - sum(x * x for x in qq)) / 2
            out[iq:iq + 3] = [float(x) for x in p1]
            out[iq + 3:iq + 7] = [float(x * f) for x in qq]
        return out
