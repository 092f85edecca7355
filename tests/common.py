"""Shared helpers for the tests: models, configurations of BASELINE.json, oracle-backed FK for input generation."""
import ctypes

import numpy as np

import oracle
import wbc_capi as capi
import wbc_model
import wbc_workload


class OracleFK:
    """fk callable for wbc_workload.make_tick_inputs backed by the CPU oracle."""

    def __init__(self, models, model_id=None):
        self.models, self.model_id = models, model_id

    def __call__(self, q):
        return oracle.fk(self.models, q, self.model_id, want_com=False)["oMf"]

    def com(self, q):
        return oracle.fk(self.models, q, self.model_id)["com"]


def models():
    return wbc_model.load_model("a1_wx200"), wbc_model.load_model("a1_px100_pin_ver")


def config(name, model):
    """BASELINE.json configs: c1/c3 = sim3 switch set, c2 = equality-only, full = every task on."""
    if name in ("c1", "c3"):
        return wbc_model.sim3_config(model)
    if name == "c2":
        return wbc_model.equality_only_config(model)
    if name == "full":   # the warm-up problem of setInitialState: all 6 Cartesian tasks + Tikhonov, bounds only
        return wbc_model.make_config(model, Trunk=True, FR=True, FL=True, RR=True, RL=True, Grip=True, Joint=True)
    if name == "everything":  # every task and every constraint type at once (coverage, not a reference preset)
        return wbc_model.make_config(model, Trunk=True, FR=True, FL=True, RR=True, RL=True, Grip=True, Joint="PREV",
                                     task_com=True, cCoM=True, cTrunk=True, cFR=True, cFL=True, cRR=True, cRL=True,
                                     mode="static_reach")
    if name in ("c3_hybrid", "c3_hybrid_clean", "c3_mani"):   # sim3.py:145 sets Joint="HYBRID"; literal = to the letter (C.4)
        return wbc_model.sim3_config(model, Joint="MANI" if name == "c3_mani" else "HYBRID",
                                     posture_literal=not name.endswith("clean"))
    if name == "hybrid_grip_com":  # HYBRID + constraints that DO depend on the arm: the leaked perturbed state shows in C
        return wbc_model.make_config(model, Grip=True, Joint="HYBRID", cCoM=True, cTrunk=True, cFR=True, cFL=True, cRR=True,
                                     cRL=True, cGrip=True, mode="static_reach")
    if name == "c3_nobounds":   # sim3 switch set without the velocity-damper box: the presolve adds no leg-bound rows
        return wbc_model.make_config(model, Grip=True, Joint="PREV", cTrunk=True, cFR=True, cFL=True, cRR=True, cRL=True,
                                     mode="static_reach", use_bounds=False)
    if name == "c3_two_feet":   # only two stance feet: 26 - 6 = 20 unknowns > 16 -> general path, no presolve
        return wbc_model.make_config(model, Grip=True, Joint="PREV", cTrunk=True, cFR=True, cRL=True, mode="static_reach")
    if name == "c3_trunk_task":  # trunk task on top (base-only support: the plan stays enabled, two task blocks)
        return wbc_model.make_config(model, Grip=True, Trunk=True, Joint="PREV", cTrunk=True, cFR=True, cFL=True, cRR=True,
                                     cRL=True, mode="static_reach")
    if name == "c3_custom":
        return wbc_model.sim3_config(model, Joint="CUSTOM")
    raise KeyError(name)


def tick_inputs(model, cfg, B, seed, stress=True, with_rot=False):
    d = wbc_workload.make_tick_inputs(model, cfg, B, seed, OracleFK([model]), stress=stress)
    if with_rot:
        add_rot_references(d, B, seed)
    return d


def add_rot_references(d, B, seed):
    """exercise the orientation feed-forward terms with a moving reference (tick_inputs(with_rot=True))"""
    rng = np.random.default_rng(seed + 1000)
    from scipy.spatial.transform import Rotation as R
    e = rng.uniform(-0.3, 0.3, (B, 5, 3))
    de = rng.normal(0, 1e-3, (B, 5, 3))
    d["ee_ref_rot"] = R.from_euler("xyz", e.reshape(-1, 3)).as_matrix().reshape(B, 5, 9)
    d["ee_prev_rot"] = R.from_euler("xyz", (e - de).reshape(-1, 3)).as_matrix().reshape(B, 5, 9)
    d["trunk_ref_euler"] = d["trunk_ref_euler"] + rng.normal(0, 0.02, (B, 3))
    d["trunk_prev_rot"] = R.from_euler("xyz", d["trunk_ref_euler"] - rng.normal(0, 1e-3, (B, 3))).as_matrix().reshape(B, 9)
    return d


# ---- poses far from the nominal stance: sample_q keeps the base within 5 cm and 0.1 rad of the origin, where no tick test can see
# the Euler angles a kernel computes and no kernel leaves the first quadrant of anything
def _attitude_ok(model, q):
    """not at the gimbal pole and not on a cut of atan2, judged by the 50-digit reference: there one ulp in R legitimately flips an angle by 2 pi"""
    import kin_reference
    e = kin_reference.trunk_euler(model.data, q)
    return abs(e[1]) <= 1.3 and abs(abs(e[0]) - np.pi) >= 0.02 and abs(abs(e[2]) - np.pi) >= 0.02


# roll, pitch, yaw ranges of the narrowed attitudes: inside +-0.3, +-0.3, +-0.5 rad, and on the side where the CoM box (RR and FL foot positions on
# WORLD axes) keeps the CoM's y between its bounds — at yaw < -0.2 or roll > 0.15 the oracle finds a quarter of the instances infeasible
NARROW = np.array([[-0.3, 0.15], [-0.3, 0.3], [-0.2, 0.5]])


def _far_base(model, q, rng, narrow=False):
    """base x, y uniform in +-3 m; attitude cycling over four kinds: 0, 1, 2 a rotation by +-(pi - 0.2) about unit(e_k + 0.15 N(0, I)) (tr R < 0
    with R_kk the largest diagonal entry: the three non-trace quaternion branches), 3 a rotation by +-U(0.5, 2.6) about a random axis; every
    second quaternion negated (w < 0). narrow: roll, pitch, yaw uniform in NARROW instead (the CoM box stays feasible)."""
    B = q.shape[0]
    q[:, 0:2] = rng.uniform(-3.0, 3.0, (B, 2))
    for b in range(B):
        while True:
            if narrow:
                quat = wbc_workload.euler_xyz_to_quat(rng.uniform(NARROW[:, 0], NARROW[:, 1], (1, 3)))[0]
            else:
                kind = b % 4
                if kind < 3:
                    axis = np.eye(3)[kind] + 0.15 * rng.normal(size=3)
                    ang = np.pi - 0.2
                else:
                    axis = rng.normal(size=3)
                    ang = rng.uniform(0.5, 2.6)
                ang *= 1.0 if rng.random() < 0.5 else -1.0
                axis /= np.linalg.norm(axis)
                quat = np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]])
            q[b, 3:7] = -quat if b % 2 else quat
            if _attitude_ok(model, q[b]):
                break
    return q


def far_q(model, B, rng, narrow=False):
    """legs and arm of wbc_workload.sample_q, the base far from the origin at a large attitude (_far_base)"""
    return _far_base(model, wbc_workload.sample_q(model, B, rng), rng, narrow)


def far_fk_q(model, B, rng):
    """FK only: every 1-DoF joint uniform over its full [q_lo, q_hi], four instances exactly on all lower limits and four on all upper limits;
    the base as far_q"""
    q = wbc_workload.sample_q(model, B, rng)
    lo, hi = model.q_lo[7:model.nq], model.q_hi[7:model.nq]
    q[:, 7:model.nq] = rng.uniform(lo, hi, (B, model.nq - 7))
    q[:4, 7:model.nq], q[4:8, 7:model.nq] = lo, hi
    return _far_base(model, q, rng)


def edge_trunk_box(d, cfg, rng, f_lo=0.97):
    """every instance, each of the three angles: the box centre moved by trunk_box_ang * f * s, f ~ U(f_lo, 1.005), s = +-1 — the current angle
    at the edge of its box, a few just outside (what make_tick_inputs' stress recipe does to the z row alone)"""
    B = d["q"].shape[0]
    f = rng.uniform(f_lo, 1.005, (B, 3))
    s = np.where(rng.random((B, 3)) < 0.5, 1.0, -1.0)
    d["trunk_box_center"] = d["trunk_box_center"].copy()
    d["trunk_box_center"][:, 1:] += cfg.trunk_box_ang * f * s
    return d


def far_tick_inputs(model, cfg, B, seed, narrow=False, edge=True, with_rot=False, f_lo=0.97):
    """wbc_workload.make_tick_inputs(stress=True) restated on far_q poses (that function draws its own sample_q and stays as it is): the same
    damper and z-box stress, targets on the robot, then edge_trunk_box where the configuration has a trunk box."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fk = OracleFK([model])
    q = far_q(model, B, rng, narrow)
    if cfg.use_bounds:
        arm_dofs = np.arange(19, model.nv - 3)
        for b in np.nonzero(rng.random(B) < 0.25)[0]:
            i = int(rng.choice(arm_dofs))
            qi = cfg.damper_qidx[i]
            v = (cfg.damper_lo[i] + rng.uniform(0.0, 0.01)) if rng.random() < 0.5 else (cfg.damper_hi[i] - rng.uniform(0.0, 0.01))
            if model.q_lo[qi] <= v <= model.q_hi[qi]:
                q[b, qi] = v
    oMf = fk(q)
    pos = oMf[:, :, 9:12]
    trunk = pos[:, capi.FR_TRUNK, :].copy()
    ee_target = pos[:, capi.FR_EE0:capi.FR_EE0 + 5, :].copy()
    ee_target[:, 4, :] += rng.normal(0, 0.01, (B, 3))
    d = dict(q=q, ee_target=ee_target, prev_ee_target=ee_target - rng.normal(0, 0.0005, (B, 5, 3)),
             trunk_target=trunk.copy(), prev_trunk_target=trunk - rng.normal(0, 0.0005, (B, 3)))
    eul = wbc_workload.R_to_euler_xyz(oMf[:, capi.FR_TRUNK, 0:9])
    box = np.concatenate([trunk[:, 2:3], eul], axis=1)
    if cfg.con_trunk:
        pick = rng.random(B) < 0.25
        frac = rng.uniform(0.245, 0.2505, B) * np.where(rng.random(B) < 0.5, 1.0, -1.0)
        box[pick, 0] = trunk[pick, 2] / (1.0 + frac[pick])
    d["trunk_box_center"] = box
    d["trunk_ref_euler"] = eul.copy()
    d["trunk_prev_rot"] = oMf[:, capi.FR_TRUNK, 0:9].copy()
    if cfg.task_com:
        d["com_target"] = fk.com(q) + rng.normal(0, 0.002, (B, 3))
        d["com_target_vel"] = rng.normal(0, 0.05, (B, 3))
    if cfg.con_trunk and edge:
        edge_trunk_box(d, cfg, rng, f_lo)
    if with_rot:
        add_rot_references(d, B, seed)
    return d


# ---- the velocity damper's zones: sample_q and the stress recipe reach the band 0 <= d < qs of one arm DoF and nothing else
DAMPER_CLASSES = ("base", "leg", "arm")
DAMPER_KINDS = ("regular", "flipped", "beyond", "edge", "qs")         # shares 3/8, 2/8, 1/8, 1/8, 1/8
DAMPER_COUNTS = (1, 2, 3, 5)
DAMPER_WIDEN = 0.06                                                   # rad: a written coordinate may leave its joint's own range by this much
DAMPER_FAR_X = 11.0                                                   # m: the last instance's base x; 6 m beyond the upper limit, the clamp at -v_max


def damper_class(i):
    """class of DoF i, the variable the bound is on: the packed kernels eliminate base and stance-leg DoF and keep the arm's"""
    return 0 if i < 6 else (1 if i < 18 else 2)


def damper_candidates(model, cfg):
    """DoF i < lock_from whose watched coordinate damper_qidx[i] is base x, y, z or a 1-DoF joint coordinate (never the quaternion)"""
    return [i for i in range(min(model.nv, int(cfg.lock_from))) if cfg.damper_qidx[i] < 3 or cfg.damper_qidx[i] >= 7]


def _damper_depth(cfg, rng, edges):
    """-> (kind, d or None): the distance to the limit of one draw; None where the coordinate is formed from the limit as the code forms it"""
    qi, qs = cfg.damper_qi, cfg.damper_qs
    k = int(rng.integers(0, 8)) if edges else int(rng.integers(0, 6))
    if k < 3:
        return 0, rng.uniform(qs + 1e-3, qi - 1e-3)
    if k < 5:
        return 1, rng.uniform(0.0, qs - 1e-3)
    if k == 5:
        return 2, -rng.uniform(0.0, 0.05)
    return (3, None) if k == 6 else (4, None)


def damper_q(model, cfg, B, rng, edges=True, classes=DAMPER_CLASSES, far=True):
    """wbc_workload.sample_q with n = (1, 2, 3, 5)[b % 4] DoF of instance b inside a damper zone: the first from the class
    (base, leg, arm)[(b // 4) % 3] (the next class on where `classes` leaves it out), the others from every candidate of `classes`; each at a
    random side, at a depth of _damper_depth. The watched coordinate becomes lo[i] + d or hi[i] - d (`edge`: lo + qi / hi - qi, `qs`: lo + qs /
    hi - qs, each one double operation as the kernels form them); base z on the upper side only; a value outside the watched joint's own model
    range widened by DAMPER_WIDEN is drawn again (DoF, side and depth; an instance of a narrowed pool that runs out of admissible DoF keeps
    what it has). far: the last instance's base x is DAMPER_FAR_X (needs the base class)."""
    q = wbc_workload.sample_q(model, B, rng)
    cand = [i for i in damper_candidates(model, cfg) if DAMPER_CLASSES[damper_class(i)] in classes]
    by_class = [[i for i in cand if damper_class(i) == c] for c in range(3)]
    for b in range(B):
        first = (b // 4) % 3
        while not by_class[first]:
            first = (first + 1) % 3
        taken = []
        for slot in range(DAMPER_COUNTS[b % 4]):
            pool = [i for i in (by_class[first] if slot == 0 else cand) if i not in taken]
            if not pool:                                              # (fewer candidates than n: a narrowed recipe)
                break
            for _ in range(64):
                i = int(rng.choice(pool))
                c = int(cfg.damper_qidx[i])
                upper = True if c == 2 else bool(rng.random() < 0.5)
                kind, d = _damper_depth(cfg, rng, edges)
                lo, hi = cfg.damper_lo[i], cfg.damper_hi[i]
                if kind == 3:
                    v = hi - cfg.damper_qi if upper else lo + cfg.damper_qi
                elif kind == 4:
                    v = hi - cfg.damper_qs if upper else lo + cfg.damper_qs
                else:
                    v = hi - d if upper else lo + d
                if model.q_lo[c] - DAMPER_WIDEN <= v <= model.q_hi[c] + DAMPER_WIDEN:
                    q[b, c] = v
                    taken.append(i)
                    break
            else:                                                     # (what is left of a narrowed recipe's pool admits no value)
                break
    if far and "base" in classes:
        q[B - 1, 0] = DAMPER_FAR_X
    return q


def damper_zones(cfg, nv, q):
    """-> zone [B, 26, 2] (lower side, upper side) of every DoF < lock_from: -1 outside every zone, else the index into DAMPER_KINDS, read off
    q with the comparisons of the code: edge where the coordinate IS lo + qi / hi - qi, qs where it IS lo + qs / hi - qs"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, capi.Q_STRIDE)
    z = np.full((q.shape[0], capi.V_STRIDE, 2), -1, dtype=np.int8)
    for i in range(min(nv, int(cfg.lock_from))):
        c, lo, hi = q[:, cfg.damper_qidx[i]], cfg.damper_lo[i], cfg.damper_hi[i]
        for side, inside, d, edge, at_qs in ((0, c <= lo + cfg.damper_qi, c - lo, lo + cfg.damper_qi, lo + cfg.damper_qs),
                                             (1, c >= hi - cfg.damper_qi, hi - c, hi - cfg.damper_qi, hi - cfg.damper_qs)):
            kind = np.where(d < 0, 2, np.where(d < cfg.damper_qs, 1, 0))
            kind = np.where(c == edge, 3, np.where(c == at_qs, 4, kind))
            z[:, i, side] = np.where(inside, kind, -1)
    return z


def damper_active(cfg, nv, q, lb, ub, qdot, tol=1e-9):
    """-> active [B, 26, 2]: q̇ on the bound (within tol) and the bound not -+v_max, lower and upper side"""
    vm = np.array([cfg.damper_vmax[i] for i in range(capi.V_STRIDE)])[None, :]
    act = np.zeros(qdot.shape + (2,), dtype=bool)
    act[:, :, 0] = (np.abs(qdot - lb) <= tol) & (lb != -vm)
    act[:, :, 1] = (np.abs(qdot - ub) <= tol) & (ub != vm)
    act[:, min(nv, int(cfg.lock_from)):] = False
    return act


def damper_tick_inputs(model, cfg, B, seed, edges=True, classes=DAMPER_CLASSES, far=True, with_rot=False):
    """tick inputs on damper_q poses; targets, trunk box, CoM target and rotation references as far_tick_inputs(edge=False) makes them (that
    function draws its own poses and stays as it is): on the robot, the box centred on the robot's own angles"""
    rng = np.random.Generator(np.random.PCG64(seed))
    fk = OracleFK([model])
    q = damper_q(model, cfg, B, rng, edges, classes, far)
    oMf = fk(q)
    pos = oMf[:, :, 9:12]
    trunk = pos[:, capi.FR_TRUNK, :].copy()
    ee_target = pos[:, capi.FR_EE0:capi.FR_EE0 + 5, :].copy()
    ee_target[:, 4, :] += rng.normal(0, 0.01, (B, 3))
    d = dict(q=q, ee_target=ee_target, prev_ee_target=ee_target - rng.normal(0, 0.0005, (B, 5, 3)),
             trunk_target=trunk.copy(), prev_trunk_target=trunk - rng.normal(0, 0.0005, (B, 3)))
    eul = wbc_workload.R_to_euler_xyz(oMf[:, capi.FR_TRUNK, 0:9])
    box = np.concatenate([trunk[:, 2:3], eul], axis=1)
    if cfg.con_trunk:
        pick = rng.random(B) < 0.25
        frac = rng.uniform(0.245, 0.2505, B) * np.where(rng.random(B) < 0.5, 1.0, -1.0)
        box[pick, 0] = trunk[pick, 2] / (1.0 + frac[pick])
    d["trunk_box_center"] = box
    d["trunk_ref_euler"] = eul.copy()
    d["trunk_prev_rot"] = oMf[:, capi.FR_TRUNK, 0:9].copy()
    if cfg.task_com:
        d["com_target"] = fk.com(q) + rng.normal(0, 0.002, (B, 3))
        d["com_target_vel"] = rng.normal(0, 0.05, (B, 3))
    if with_rot:
        add_rot_references(d, B, seed)
    return d


def kkt_residuals(H, g, C, lb, ub, cl, cu, x, act_tol=1e-7):
    """Solver-independent optimality certificate: (primal violation, stationarity residual with sign-correct multipliers)."""
    from scipy.optimize import lsq_linear
    n = len(g)
    viol = 0.0
    if lb is not None:
        viol = max(viol, (lb - x).max(), (x - ub).max())
    if C is not None and len(cl):
        v = C @ x
        viol = max(viol, (cl - v).max(), (v - cu).max())
    r = H @ x + g
    rows, free_sign = [], []
    if lb is not None:
        for k in range(n):
            e = np.zeros(n)
            e[k] = 1
            if lb[k] == ub[k]:
                rows.append(e), free_sign.append(True)
            else:
                if abs(x[k] - lb[k]) < act_tol * max(1, abs(lb[k])):
                    rows.append(e), free_sign.append(False)
                if abs(x[k] - ub[k]) < act_tol * max(1, abs(ub[k])):
                    rows.append(-e), free_sign.append(False)
    if C is not None and len(cl):
        v = C @ x
        for i in range(len(cl)):
            if cl[i] == cu[i]:
                rows.append(C[i]), free_sign.append(True)
            else:
                if abs(v[i] - cl[i]) < act_tol * max(1, abs(cl[i])):
                    rows.append(C[i]), free_sign.append(False)
                if abs(v[i] - cu[i]) < act_tol * max(1, abs(cu[i])):
                    rows.append(-C[i]), free_sign.append(False)
    if rows:
        N = np.array(rows).T
        lo = [-np.inf if f else 0.0 for f in free_sign]
        res = lsq_linear(N, r, bounds=(lo, np.inf), tol=1e-14)
        stat = np.abs(N @ res.x - r).max()
    else:
        stat = np.abs(r).max()
    return viol, stat


def exact_normal_equations(A, b):
    """H = A'A and g = -A'b of double-precision A, b in EXACT rational arithmetic (lists of Fractions): the least-squares problem itself,
    free of the rounding that forming H in doubles adds (1e-5 relative on the posture block of the benchmark tick)."""
    from fractions import Fraction
    m, n = A.shape
    Af = [[Fraction(float(A[i, j])) for j in range(n)] for i in range(m)]
    bf = [Fraction(float(v)) for v in b]
    nz = [[k for k in range(m) if Af[k][i] != 0] for i in range(n)]
    H = [[sum(Af[k][i] * Af[k][j] for k in nz[i]) for j in range(n)] for i in range(n)]
    g = [-sum(Af[k][i] * bf[k] for k in nz[i]) for i in range(n)]
    return H, g


def exact_kkt(H, g, rows, rhs):
    """Exact (rational) solution of  H x + N'lam = -g,  N x = rhs  for double-precision data (or H, g already given as Fractions:
    exact_normal_equations); returns (x, lam) as floats."""
    from fractions import Fraction
    n, p = len(g), len(rhs)
    N = n + p
    M = [[Fraction(0)] * (N + 1) for _ in range(N)]
    for i in range(n):
        for j in range(n):
            M[i][j] = Fraction(H[i][j])
        for j in range(p):
            M[i][n + j] = M[n + j][i] = Fraction(float(rows[j][i]))
        M[i][N] = -Fraction(g[i])
    for j in range(p):
        M[n + j][N] = Fraction(float(rhs[j]))
    for c in range(N):
        piv = max(range(c, N), key=lambda r: abs(M[r][c]))
        assert M[piv][c] != 0, "active rows are dependent"
        M[c], M[piv] = M[piv], M[c]
        inv = 1 / M[c][c]
        for r in range(N):
            if r != c and M[r][c] != 0:
                f = M[r][c] * inv
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    sol = [float(M[i][N] / M[i][i]) for i in range(N)]
    return np.array(sol[:n]), np.array(sol[n:])



def exact_ls_optimum(A, b, C, lb, ub, Clb, Cub, x_float):
    """exact_optimum for the least-squares form  min 1/2 |A x - b|^2  (QP_Wrapper.py:17-18: H = A'A, g = -A'b) with H and g formed in
    rational arithmetic from the double-precision A, b — the optimum every correct rounding of H approximates."""
    H, g = exact_normal_equations(np.asarray(A), np.asarray(b))
    return exact_optimum(H, g, C, lb, ub, Clb, Cub, x_float)


def exact_optimum(H, g, C, lb, ub, Clb, Cub, x_float):
    """The exact optimum of the double-precision QP data on the active set read off `x_float`, with the optimality checks
    (primal feasibility, multiplier signs) asserted. Returns x_exact."""
    n = len(g)
    lo, hi = np.concatenate([lb, Clb]), np.concatenate([ub, Cub])
    Nall = np.vstack([np.eye(n), C])
    v = Nall @ x_float
    rows, rhs, kind = [], [], []
    for i in range(len(lo)):
        if lo[i] == hi[i]:
            rows.append(Nall[i]); rhs.append(lo[i]); kind.append(0)
        elif abs(v[i] - lo[i]) < 1e-7 * max(1, abs(lo[i])):
            rows.append(Nall[i]); rhs.append(lo[i]); kind.append(-1)
        elif abs(v[i] - hi[i]) < 1e-7 * max(1, abs(hi[i])):
            rows.append(Nall[i]); rhs.append(hi[i]); kind.append(+1)
    x, lam = exact_kkt(H, g, rows, rhs)
    vx = Nall @ x
    assert (vx >= lo - 1e-9 * np.maximum(1, np.abs(lo))).all() and (vx <= hi + 1e-9 * np.maximum(1, np.abs(hi))).all()
    for k, l in zip(kind, lam):              # H x + g + N'lam = 0: at a lower bound lam <= 0, at an upper bound lam >= 0
        assert not (k == -1 and l > 1e-9 * (1 + abs(l))) and not (k == +1 and l < -1e-9 * (1 + abs(l)))
    return x


# ---- tracks (wbc_rollout_tracks): the recipe, the oracle's loop and the scores, shared by test_gpu_rollout_tracks.py and test_gpu_device_inplace.py
DT_TRACKS = 0.002
GRIP, TRUNK = 4, capi.TARGET_TRUNK


def track_frames(models, q, mid):
    """positions [B, 6, 3] of the five EE frames and the trunk frame"""
    oMf = oracle.fk(models, q, mid, want_com=False)["oMf"]
    return np.concatenate([oMf[:, capi.FR_EE0:capi.FR_EE0 + 5, 9:], oMf[:, capi.FR_TRUNK:capi.FR_TRUNK + 1, 9:]], axis=1)


def base_tracks(d, grip_pos, seed):
    """the base recipe: a trunk track (HERMITE, 2..5 milestones) and a gripper track (LINEAR, 2..4), drawn in this order"""
    rng = np.random.default_rng(seed)
    B = len(grip_pos)
    tp = d["trunk_target"][:, None, :] + rng.normal(0, 0.01, (B, 5, 3))
    tp[:, 0] = d["trunk_target"]
    tn = rng.choice([2, 3, 4, 5], B).astype(np.int32)
    tdu = rng.choice([1 / 8, 1 / 5, 0.3], B)
    gp = grip_pos[:, None, :] + rng.normal(0, 0.01, (B, 4, 3))
    gp[:, 0] = grip_pos
    gn = rng.choice([2, 3, 4], B).astype(np.int32)
    gdu = rng.choice([1 / 8, 1 / 5, 0.3], B)
    return [dict(target="trunk", points=tp, kind="hermite", n_points=tn, du=tdu), dict(target=GRIP, points=gp, kind="linear", n_points=gn, du=gdu)]


def track_index(t):
    return TRUNK if t == "trunk" else int(t)


def track_at(track, k):
    return wbc_workload.track_targets(track["points"], track.get("n_points"), track.get("du", 0.002), k, track.get("kind", "linear"), track.get("tangents"))


def start_previous_targets(d, tracks):
    """prev_* of the followed targets = the first milestones (the followed rows of ee_target / trunk_target keep what the generator put there:
    the call must not read them)"""
    for t in tracks:
        if track_index(t["target"]) == TRUNK:
            d["prev_trunk_target"] = t["points"][:, 0].copy()
        else:
            d["prev_ee_target"][:, track_index(t["target"])] = t["points"][:, 0]


def per_instance_configs(models, cfgs, mid, rows):
    """the oracle's form of per-instance task rows: B (model, configuration) pairs, model_id = arange(B)"""
    off = capi.WbcConfig.ee_W.offset
    ms, cs = [], []
    for b in range(len(rows)):
        i = 0 if mid is None else int(mid[b])
        c = capi.WbcConfig.from_buffer_copy(cfgs[i])
        ctypes.memmove(ctypes.addressof(c) + off, rows[b].ctypes.data, 85 * 8)
        ms.append(models[i])
        cs.append(c)
    return ms, cs, np.arange(len(rows), dtype=np.int32)


def tracks_reference(p, dt=DT_TRACKS):
    """oracle.rollout's loop with a target hook per track: -> dict(q, qdot, status (max), iters (sum), ee_target, trunk_target (the targets the
    next tick would get), tick_status [K, B], frames [K, B, 6, 3] reached, targets [K, B, 6, 3] of the tick). The arrays are read-only."""
    from scipy.spatial.transform import Rotation as R
    models, cfgs, mid, B, K = p["models"], p["cfgs"], p["mid"], p["B"], p["K"]
    ms, cs, d = models, cfgs, {k: np.array(v, copy=True) for k, v in p["d"].items()}
    if p["rows"] is not None:
        ms, cs, pid = per_instance_configs(models, cfgs, mid, p["rows"])
        d["model_id"] = pid
    assert "ee_ref_rot" not in d                                    # (no EE orientation reference state to carry in this restatement)

    def set_targets(k):
        for t in p["tracks"]:
            if track_index(t["target"]) == TRUNK:
                d["trunk_target"] = track_at(t, k)
            else:
                d["ee_target"][:, track_index(t["target"])] = track_at(t, k)
    status, iters = np.zeros(B, np.int32), np.zeros(B, np.int32)
    tick_status = np.zeros((K, B), np.int32)
    frames, targets = np.zeros((K, B, 6, 3)), np.zeros((K, B, 6, 3))
    out = None
    for k in range(K):
        set_targets(k)
        targets[k, :, :5], targets[k, :, 5] = d["ee_target"], d["trunk_target"]
        out = oracle.tick(ms, cs, d, dt, B, nthreads=8, want_q_next=True)
        tick_status[k] = out["status"]
        status = np.maximum(status, out["status"])
        iters += out["iters"]
        d["q"] = oracle.update_state(models, d["q"], out["q_next"], d["ee_target"], p["imu"], mid) if p["running"] else out["q_next"]
        frames[k] = track_frames(models, d["q"], mid)
        for i, c in enumerate(cfgs):                                # the reference-state side effects of qpb()
            sel = slice(None) if mid is None else (mid == i)
            for e in range(capi.NEE):
                if c.task_ee[e]:
                    d["prev_ee_target"][sel, e] = d["ee_target"][sel, e]
            if c.task_trunk:
                d["prev_trunk_target"][sel] = d["trunk_target"][sel]
                d["trunk_prev_rot"][sel] = R.from_euler("xyz", d["trunk_ref_euler"][sel]).as_matrix().reshape(-1, 9)
    set_targets(K)
    ref = dict(q=d["q"], qdot=out["qdot"], status=status, iters=iters, ee_target=d["ee_target"], trunk_target=d["trunk_target"],
               tick_status=tick_status, frames=frames, targets=targets)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def numpy_scores(trace, targets, status):
    """the scores of [K, F, B, 3] positions against [K, F, B, 3] targets and [K, B] statuses, summed in tick order"""
    K, B = status.shape
    d = trace - targets
    e2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    err = np.sqrt(e2)
    ssum = np.zeros(e2.shape[1:])
    for k in range(K):
        ssum = ssum + e2[k]
    bad = status != 0
    return dict(err_sq_sum=ssum, err_max=err.max(axis=0), err_max_tick=err.argmax(axis=0).astype(np.int32), err_final=err[-1],
                first_bad_tick=np.where(bad.any(axis=0), bad.argmax(axis=0), -1).astype(np.int32), bad_ticks=bad.sum(axis=0).astype(np.int32))
