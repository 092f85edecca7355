"""Synthetic tick inputs for the benchmark configurations of BASELINE.json.

The reference has no input generator (its inputs come from a PyBullet GUI simulation); this module draws
robot states from the distribution SURVEY.md §8(d) fixes so that tests, bench.py and the oracle all see the
same seeded inputs. It needs a forward-kinematics callable to place the targets on the robot
(``fk(q[B,27]) -> oMf[B, nframes, 12]``): tests pass the oracle's, bench.py passes the GPU's.
"""
import os

import numpy as np

import wbc_capi as capi

_MOCAP = os.path.join(capi.HERE, "data", "mocap_wx200_legs.csv")   # ships with the package: the product never reads tests/
_mocap_cache = None


def mocap_legs():
    """Rows of 12 leg angles in the log's FR, FL, RR, RL order (fixture sampled from the reference's
    tests_NOT_FOR_USE/mocap_wx200.txt)."""
    global _mocap_cache
    if _mocap_cache is None:
        _mocap_cache = np.loadtxt(_MOCAP, delimiter=",", comments="#")
    return _mocap_cache


def euler_xyz_to_quat(e):
    """(x, y, z, w) of Rz(c) Ry(b) Rx(a), vectorised over rows."""
    a, b, c = e[:, 0] / 2, e[:, 1] / 2, e[:, 2] / 2
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return np.stack([sa * cb * cc - ca * sb * sc, ca * sb * cc + sa * cb * sc,
                     ca * cb * sc - sa * sb * cc, ca * cb * cc + sa * sb * sc], axis=1)


def R_to_euler_xyz(R):
    """extrinsic xyz angles of [B, 9] row-major rotations (scipy as_euler('xyz'))."""
    return np.stack([np.arctan2(R[:, 7], R[:, 8]), -np.arcsin(np.clip(R[:, 6], -1, 1)), np.arctan2(R[:, 3], R[:, 0])], axis=1)


def sample_q(model, B, rng):
    """Robot configurations: mocap gait legs + noise, arm in the middle 80 % of its range, small base tilt."""
    nq = model.nq
    q = np.zeros((B, capi.Q_STRIDE))
    q[:, 0:2] = rng.uniform(-0.05, 0.05, (B, 2))
    q[:, 2] = 0.30 + rng.uniform(-0.03, 0.03, B)
    q[:, 3:7] = euler_xyz_to_quat(rng.uniform(-0.1, 0.1, (B, 3)))
    legs = mocap_legs()[rng.integers(0, len(mocap_legs()), B)]
    legs = legs.reshape(B, 4, 3)[:, [1, 0, 3, 2], :].reshape(B, 12)      # FR,FL,RR,RL -> FL,FR,RL,RR
    legs = legs + rng.normal(0, 0.02, (B, 12))
    lo, hi = model.q_lo[7:19], model.q_hi[7:19]
    q[:, 7:19] = np.clip(legs, lo + 0.03, hi - 0.03)
    grip = "gripper" in model.joint_names                                 # a1 arms: a revolute gripper at nq - 3; Laikago's is fixed
    n_arm = nq - 19 - (3 if grip else 2)                                  # waist .. last wrist joint
    lo, hi = model.q_lo[19:19 + n_arm], model.q_hi[19:19 + n_arm]
    mid, half = 0.5 * (lo + hi), 0.4 * (hi - lo)
    q[:, 19:19 + n_arm] = mid + half * rng.uniform(-1, 1, (B, n_arm))
    if grip:
        q[:, nq - 3] = 0.0                                                # gripper
    q[:, nq - 2], q[:, nq - 1] = 0.02, -0.02                              # fingers, as in the mocap log
    return q


def make_tick_inputs(model, cfg, B, seed, fk, stress=True):
    """dict of numpy arrays keyed like WbcTickIn for `B` instances of `model` under `cfg`.

    stress=True applies the C3 recipe: 25 % of the instances get one arm DoF's damper inside its limit zone
    and 25 % get the trunk at the edge of (a few just outside) its z box, so bounds and box rows activate.
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    q = sample_q(model, B, rng)
    if stress and cfg.use_bounds:
        pick = rng.random(B) < 0.25
        arm_dofs = np.arange(19, model.nv - 3)
        for b in np.nonzero(pick)[0]:
            i = int(rng.choice(arm_dofs))
            qi = cfg.damper_qidx[i]
            side = rng.random() < 0.5
            v = (cfg.damper_lo[i] + rng.uniform(0.0, 0.01)) if side else (cfg.damper_hi[i] - rng.uniform(0.0, 0.01))
            if model.q_lo[qi] <= v <= model.q_hi[qi]:
                q[b, qi] = v
    oMf = fk(q)
    pos = oMf[:, :, 9:12]
    ee = pos[:, capi.FR_EE0:capi.FR_EE0 + 5, :].copy()
    trunk = pos[:, capi.FR_TRUNK, :].copy()
    ee_target = ee.copy()
    ee_target[:, 4, :] += rng.normal(0, 0.01, (B, 3))
    d = dict(q=q, ee_target=ee_target,
             prev_ee_target=ee_target - rng.normal(0, 0.0005, (B, 5, 3)),
             trunk_target=trunk.copy(), prev_trunk_target=trunk - rng.normal(0, 0.0005, (B, 3)))
    eul = R_to_euler_xyz(oMf[:, capi.FR_TRUNK, 0:9])
    box = np.concatenate([trunk[:, 2:3], eul], axis=1)
    if stress and cfg.con_trunk:
        pick = rng.random(B) < 0.25
        frac = rng.uniform(0.245, 0.2505, B) * np.where(rng.random(B) < 0.5, 1.0, -1.0)
        # centre z0 such that the current z sits frac*z0 away from it: z = z0 (1 + frac)
        box[pick, 0] = trunk[pick, 2] / (1.0 + frac[pick])
    d["trunk_box_center"] = box
    d["trunk_ref_euler"] = eul.copy()
    Rt = oMf[:, capi.FR_TRUNK, 0:9]
    d["trunk_prev_rot"] = Rt.copy()           # steady state: R*_prev == R* 
    com = None
    if cfg.task_com:
        com = fk.com(q) if hasattr(fk, "com") else None
        if com is None:
            raise ValueError("CoM task needs fk.com(q)")
        d["com_target"] = com + rng.normal(0, 0.002, (B, 3))
        d["com_target_vel"] = rng.normal(0, 0.05, (B, 3))
    return d


def traj_targets(points, n_points, du, k):
    """Targets [B, 3] of tick k along per-instance milestone trajectories: wbc_rollout_traj's evaluation restated for a whole batch, bit for
    bit (include/wbc.h). points [B, S, 3]; n_points [B] milestones of each instance (None: S); du [B] or a scalar: parameter advance per
    tick. Instance b gets klampt's Trajectory(milestones=points[b, :n_points[b]]).eval(k * du[b]) (Robot_Wrapper4._LinearTrajectory):
    clamped ends, otherwise i = floor(t), u = t - i, (1 - u) * m[i] + u * m[i + 1]."""
    points = np.asarray(points, dtype=np.float64)
    B, S = points.shape[0], points.shape[1]
    n = np.full(B, S, dtype=np.int64) if n_points is None else np.asarray(n_points, dtype=np.int64).reshape(B)
    t = float(k) * np.broadcast_to(np.asarray(du, dtype=np.float64), (B,))
    inner = (t > 0) & (t < n - 1)
    i = np.where(inner, np.floor(np.where(inner, t, 0.0)), 0.0).astype(np.int64)
    u = (t - i)[:, None]
    rows = np.arange(B)
    out = (1 - u) * points[rows, i] + u * points[rows, np.minimum(i + 1, S - 1)]
    out[t <= 0] = points[t <= 0, 0]
    last = t >= n - 1
    out[last] = points[last, n[last] - 1]
    return out


def spline_tangents(points, n_points=None):
    """Default tangents [B, S, 3] of Hermite tracks (wbc_rollout_tracks with tangents == NULL, include/wbc.h), bit for bit: the rule of
    klampt's HermiteTrajectory.makeSpline(preventOvershoot=True). Two milestones: the chord. Three or more: zero at both ends; interior
    milestone i per component with a = m[i - 1], x = m[i], b = m[i + 1], w = (b - a) * 0.5: 0 at an extremum or a flat, else 3 (x - a) /
    3 (b - x) where the centred difference w would overshoot a / b, else w. Rows beyond n_points[b] are never read and come back zero."""
    points = np.asarray(points, dtype=np.float64)
    B, S = points.shape[0], points.shape[1]
    n = np.full(B, S, dtype=np.int64) if n_points is None else np.asarray(n_points, dtype=np.int64).reshape(B)
    v = np.zeros((B, S, 3))
    third = 1.0 / 3.0
    with np.errstate(invalid="ignore"):
        for i in range(1, S - 1):
            rows = n > i + 1                                            # milestone i is interior
            if not rows.any():
                continue
            a, x, b = points[rows, i - 1], points[rows, i], points[rows, i + 1]
            w = (b - a) * 0.5
            flat = (x <= np.minimum(a, b)) | (x >= np.maximum(a, b))
            lo = ((w < 0) & (x - w * third >= a)) | ((w > 0) & (x - w * third <= a))
            hi = ((w < 0) & (x + w * third < b)) | ((w > 0) & (x + w * third > b))
            v[rows, i] = np.where(flat, 0.0, np.where(lo, 3.0 * (x - a), np.where(hi, 3.0 * (b - x), w)))
    two = n == 2
    if two.any():
        chord = points[two, 1] - points[two, 0]
        v[two, 0] = chord
        v[two, 1] = chord
    return v


def track_targets(points, n_points, du, k, kind="linear", tangents=None):
    """Targets [B, 3] of tick k along per-instance tracks: wbc_rollout_tracks' evaluation restated for a whole batch, bit for bit
    (include/wbc.h). kind "linear": traj_targets. kind "hermite": the cubic Hermite spline through the milestones with unit knot spacing
    (Robot_Wrapper4._HermiteTrajectory); tangents [B, S, 3], None: spline_tangents(points, n_points)."""
    if kind == "linear":
        if tangents is not None:
            raise ValueError("a linear track has no tangents")
        return traj_targets(points, n_points, du, k)
    if kind != "hermite":
        raise ValueError("kind %r is neither 'linear' nor 'hermite'" % (kind,))
    points = np.asarray(points, dtype=np.float64)
    B, S = points.shape[0], points.shape[1]
    n = np.full(B, S, dtype=np.int64) if n_points is None else np.asarray(n_points, dtype=np.int64).reshape(B)
    vel = spline_tangents(points, n) if tangents is None else np.asarray(tangents, dtype=np.float64).reshape(B, S, 3)
    t = float(k) * np.broadcast_to(np.asarray(du, dtype=np.float64), (B,))
    inner = (t > 0) & (t < n - 1)
    i = np.where(inner, np.floor(np.where(inner, t, 0.0)), 0.0).astype(np.int64)
    i1 = np.minimum(i + 1, S - 1)
    u = np.where(inner, t - i, 0.0)[:, None]
    rows = np.arange(B)
    u2 = u * u
    u3 = u * u2
    cx1 = (2.0 * u3 - 3.0 * u2) + 1.0
    cx2 = (-2.0 * u3) + 3.0 * u2
    cv1 = (u3 - 2.0 * u2) + u
    cv2 = u3 - u2
    with np.errstate(invalid="ignore"):                                 # (rows at a clamped end may touch entries beyond n_points: overwritten below)
        out = ((cx1 * points[rows, i] + cx2 * points[rows, i1]) + cv1 * vel[rows, i]) + cv2 * vel[rows, i1]
    out[t <= 0] = points[t <= 0, 0]
    last = t >= n - 1
    out[last] = points[last, n[last] - 1]
    return out


def _tangent_case(a, x, b):
    """the case (1..4, include/wbc.h) the default-tangent rule takes for one component at an interior milestone"""
    w, third = (b - a) * 0.5, 1.0 / 3.0
    if x <= min(a, b) or x >= max(a, b):
        return 1
    if (w < 0 and x - w * third >= a) or (w > 0 and x - w * third <= a):
        return 2
    if (w < 0 and x + w * third < b) or (w > 0 and x + w * third > b):
        return 3
    return 4


def _tangent_adjoint(m, d, n, i, vb):
    """vb, the cotangent of the default tangent at milestone i, into d (both one instance's [S, 3]); per component, the plus term first"""
    if n == 2:
        d[1] = d[1] + vb
        d[0] = d[0] - vb
        return
    if i == 0 or i == n - 1:
        return
    for c in range(3):
        case = _tangent_case(m[i - 1, c], m[i, c], m[i + 1, c])
        if case == 2:
            d[i, c] = d[i, c] + 3.0 * vb[c]
            d[i - 1, c] = d[i - 1, c] - 3.0 * vb[c]
        elif case == 3:
            d[i + 1, c] = d[i + 1, c] + 3.0 * vb[c]
            d[i, c] = d[i, c] - 3.0 * vb[c]
        elif case == 4:
            d[i + 1, c] = d[i + 1, c] + 0.5 * vb[c]
            d[i - 1, c] = d[i - 1, c] - 0.5 * vb[c]


def track_target_gradients(points, n_points, du, ticks, kind="linear", tangents=None, e=None):
    """The adjoint of track_targets over ticks k = 0 .. ticks - 1: wbc_rollout_vjp_tracks' track kernel restated, the same operations in the
    same order (include/wbc.h), so the sums round alike. e [ticks, B, 3]: the cotangent of the target of each tick. Returns (d_points
    [B, S, 3], d_tangents [B, S, 3] — None unless kind is "hermite" with caller tangents —, d_du [B]). Per instance, from the last tick to
    the first, with t = float(k) * du and the forward's comparisons: t <= 0 -> d_points[0] += e; t >= n - 1 -> d_points[n - 1] += e;
    otherwise i = floor(t), u = t - i (an exact knot: segment i with u = 0), the segment's coefficients times e into milestones i and i + 1,
    the tangent cotangents cv1 e, cv2 e into d_tangents or, default tangents, through the rule's branch into the neighbouring milestones,
    and d_du += k ((x + y) + z) with x, y, z the components of d(target)/dt times e. A bad row (a non-finite point or tangent among the
    first n_points, du not finite and positive, n_points outside 2..S) gets zeros."""
    if kind not in ("linear", "hermite"):
        raise ValueError("kind %r is neither 'linear' nor 'hermite'" % (kind,))
    if kind == "linear" and tangents is not None:
        raise ValueError("a linear track has no tangents")
    points = np.asarray(points, dtype=np.float64)
    B, S = points.shape[0], points.shape[1]
    K = int(ticks)
    e = np.asarray(e, dtype=np.float64).reshape(K, B, 3)
    n_all = np.full(B, S, dtype=np.int64) if n_points is None else np.asarray(n_points, dtype=np.int64).reshape(B)
    du_all = np.broadcast_to(np.asarray(du, dtype=np.float64), (B,))
    vel = None if tangents is None else np.asarray(tangents, dtype=np.float64).reshape(B, S, 3)
    dflt = spline_tangents(points, np.clip(n_all, 2, S)) if (kind == "hermite" and vel is None) else None
    d_points, d_du = np.zeros((B, S, 3)), np.zeros(B)
    d_tangents = np.zeros((B, S, 3)) if vel is not None else None
    for b in range(B):
        n, dub, m = int(n_all[b]), float(du_all[b]), points[b]
        if n < 2 or n > S or not np.isfinite(dub) or not dub > 0.0 or not np.isfinite(m[:n]).all() or (vel is not None and not np.isfinite(vel[b, :n]).all()):
            continue
        v = vel[b] if vel is not None else (dflt[b] if dflt is not None else None)
        dp = d_points[b]
        for k in range(K - 1, -1, -1):
            eb = e[k, b]
            t = float(k) * dub
            if t <= 0.0:
                dp[0] = dp[0] + eb
                continue
            if t >= float(n - 1):
                dp[n - 1] = dp[n - 1] + eb
                continue
            fi = np.floor(t)
            i = int(fi)
            u = t - fi
            if kind == "linear":
                dp[i] = dp[i] + (1.0 - u) * eb
                dp[i + 1] = dp[i + 1] + u * eb
                x = (m[i + 1] - m[i]) * eb
            else:
                u2 = u * u
                u3 = u * u2
                cx1, cx2, cv1, cv2 = (2.0 * u3 - 3.0 * u2) + 1.0, (-2.0 * u3) + 3.0 * u2, (u3 - 2.0 * u2) + u, u3 - u2
                dx1, dx2, dv1, dv2 = 6.0 * u2 - 6.0 * u, (-6.0 * u2) + 6.0 * u, (3.0 * u2 - 4.0 * u) + 1.0, 3.0 * u2 - 2.0 * u
                x = (((dx1 * m[i] + dx2 * m[i + 1]) + dv1 * v[i]) + dv2 * v[i + 1]) * eb
                dp[i] = dp[i] + cx1 * eb
                dp[i + 1] = dp[i + 1] + cx2 * eb
                vb0, vb1 = cv1 * eb, cv2 * eb
                if vel is not None:
                    d_tangents[b, i] = d_tangents[b, i] + vb0
                    d_tangents[b, i + 1] = d_tangents[b, i + 1] + vb1
                else:
                    _tangent_adjoint(m, dp, n, i, vb0)
                    _tangent_adjoint(m, dp, n, i + 1, vb1)
            d_du[b] = d_du[b] + float(k) * ((x[0] + x[1]) + x[2])
    return d_points, d_tangents, d_du


# ---- constraint slack (wbc_state_slack / wbc_rollout_watch, include/wbc.h): the four families restated in numpy
def slack_joint_dofs(model, cfg):
    """(d, i) of every velocity DoF 6 <= d < cfg.lock_from of the model with the q index i of its own joint"""
    q_of = {j["idx_v"]: j["idx_q"] for j in model.data["joints"][2:model.njoints]}
    return [(d, q_of[d]) for d in range(6, min(int(cfg.lock_from), model.nv)) if d in q_of]


def state_slack(model, cfg, q, trunk_box_center, fk):
    """wbc_state_slack restated for B instances of ONE model: q [B, 27], trunk_box_center [B, 4] or None, fk a callable with
    fk(q) -> oMf [B, nframes, 12] and fk.com(q) -> [B, 3] (as wbc_workload.make_tick_inputs takes one). Returns dict(slack [B, 4],
    which [B, 4] int32, components [B, 12], joint_components [B, 2 n], joint_codes [2 n]): slack >= 0 inside, < 0 outside; families CoM box
    (RR / FL foot positions against data.com[0], x and y), trunk z box, trunk angle box (angles by the tick kernels' atan2 formula), joint range
    (the model's own q_lo / q_hi of each DoF's own joint, 6 <= d < cfg.lock_from). `which`: the code of the smallest component, the lowest
    code on a tie. A row with a non-finite q (or, families 1 and 2, box centre) gives NaN and -1."""
    q = np.array(q, dtype=np.float64).reshape(-1, capi.Q_STRIDE)
    B = q.shape[0]
    rowbad = ~np.isfinite(q[:, :model.nq]).all(axis=1)
    if rowbad.any():
        neutral = np.zeros(capi.Q_STRIDE)
        neutral[6] = 1.0
        q[rowbad] = neutral                                               # (the kinematics see a valid pose; the row is NaN below)
    oMf, com = fk(q), fk.com(q)
    pos = oMf[:, :, 9:12]
    pFL, pRR = pos[:, capi.FR_EE0 + 1], pos[:, capi.FR_EE0 + 2]
    comp = np.full((B, capi.N_SLACK_COMPONENTS), np.nan)
    for r in range(2):
        comp[:, 2 * r] = -(pRR[:, r] - com[:, r])
        comp[:, 2 * r + 1] = pFL[:, r] - com[:, r]
    bad1 = bad2 = np.ones(B, dtype=bool)
    if trunk_box_center is not None:
        c = np.asarray(trunk_box_center, dtype=np.float64).reshape(B, 4)
        bad1, bad2 = ~np.isfinite(c[:, 0]), ~np.isfinite(c[:, 1:]).all(axis=1)
        R = oMf[:, capi.FR_TRUNK, 0:9]
        e = np.stack([np.arctan2(R[:, 7], R[:, 8]), np.arctan2(-R[:, 6], np.sqrt(R[:, 7] * R[:, 7] + R[:, 8] * R[:, 8])),
                      np.arctan2(R[:, 3], R[:, 0])], axis=1)
        with np.errstate(invalid="ignore"):
            z, v = pos[:, capi.FR_TRUNK, 2], c[:, 0] * cfg.trunk_box_z_frac
            comp[:, 4] = -((c[:, 0] - v) - z)
            comp[:, 5] = (c[:, 0] + v) - z
            for a in range(3):
                comp[:, 6 + 2 * a] = -((c[:, 1 + a] - cfg.trunk_box_ang) - e[:, a])
                comp[:, 7 + 2 * a] = (c[:, 1 + a] + cfg.trunk_box_ang) - e[:, a]
    bad1, bad2 = bad1 | rowbad, bad2 | rowbad
    dofs = slack_joint_dofs(model, cfg)
    jcomp = np.zeros((B, 2 * len(dofs)))
    jcodes = np.zeros(2 * len(dofs), dtype=np.int32)
    for n, (d, i) in enumerate(dofs):
        jcomp[:, 2 * n], jcomp[:, 2 * n + 1] = q[:, i] - model.q_lo[i], model.q_hi[i] - q[:, i]
        jcodes[2 * n], jcodes[2 * n + 1] = 2 * d, 2 * d + 1
    slack, which = np.full((B, capi.N_SLACK), np.nan), np.full((B, capi.N_SLACK), -1, dtype=np.int32)
    for f, (lo, hi, bad) in enumerate(((0, 4, rowbad), (4, 6, bad1), (6, 12, bad2))):
        comp[bad, lo:hi] = np.nan
        part = np.where(bad[:, None], 0.0, comp[:, lo:hi])
        k = part.argmin(axis=1)                                           # the first of equal minima: the lowest code
        slack[:, f] = np.where(bad, np.nan, part[np.arange(B), k])
        which[:, f] = np.where(bad, -1, k)
    if dofs:
        k = jcomp.argmin(axis=1)
        slack[:, 3], which[:, 3] = jcomp[np.arange(B), k], jcodes[k]
    else:
        slack[:, 3] = np.inf
    slack[rowbad, 3], which[rowbad, 3] = np.nan, -1
    jcomp[rowbad] = np.nan
    return dict(slack=slack, which=which, components=comp, joint_components=jcomp, joint_codes=jcodes)


def watch_summary(trace, which=None):
    """wbc_rollout_watch's reduction over ticks restated: trace [K, ...] per-tick slacks (any trailing shape) -> dict(slack_min,
    slack_min_tick (the FIRST tick of the minimum), slack_final, neg_ticks (ticks with slack < 0), first_neg_tick (-1: none)[,
    slack_min_which: with `which` [K, ...], the per-tick codes]). A NaN tick makes the minimum NaN for good: slack_min_tick is the first such
    tick, the code -1, and neg_ticks does not count it."""
    t = np.asarray(trace, dtype=np.float64)
    nan = np.isnan(t)
    anynan = nan.any(axis=0)
    filled = np.where(nan, np.inf, t)
    tick = np.where(anynan, nan.argmax(axis=0), filled.argmin(axis=0)).astype(np.int32)
    mn = np.where(anynan, np.nan, np.take_along_axis(filled, tick[None].astype(np.int64), axis=0)[0])
    neg = t < 0
    out = dict(slack_min=mn, slack_min_tick=tick, slack_final=t[-1].copy(), neg_ticks=neg.sum(axis=0).astype(np.int32),
               first_neg_tick=np.where(neg.any(axis=0), neg.argmax(axis=0), -1).astype(np.int32))
    if which is not None:
        w = np.take_along_axis(np.asarray(which), tick[None].astype(np.int64), axis=0)[0]
        out["slack_min_which"] = np.where(anynan, -1, w).astype(np.int32)
    return out


# ---- dual solution, KKT certificate and sensitivities of a solved QP: the host restatement of wbc_qp_certificate (include/wbc.h), one problem
# (qp_certificate needs scipy, for solve_triangular — the only function of the package that does; it is imported inside the function)
QP_INF = 1e20
CERT_DEP_TOL = 1e-12


def _ws_bits(word):
    w = int(word) & 0xFFFFFFFFFFFFFFFF
    return [((w >> i) & 1) | (((w >> (32 + i)) & 1) << 1) for i in range(32)]


def qp_active_sides(x, C_=None, lb=None, ub=None, Clb=None, Cub=None, working_set=None):
    """-> (side, lo, hi, val), each [n + p], variables then rows: side 0 inactive, 1 at the lower side, 2 at the upper side, 3 equality; the rule of
    include/wbc.h (with a working set [2]: its marked sides; without: read off x as tests/common.py exact_optimum does)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    p = 0 if C_ is None else len(C_)
    lo = np.concatenate([np.full(n, -1e30) if lb is None else np.asarray(lb, float), np.asarray(Clb, float) if p else np.zeros(0)])
    hi = np.concatenate([np.full(n, 1e30) if ub is None else np.asarray(ub, float), np.asarray(Cub, float) if p else np.zeros(0)])
    val = np.concatenate([x, np.asarray(C_, float) @ x if p else np.zeros(0)])
    bits = None if working_set is None else _ws_bits(working_set[0])[:n] + _ws_bits(working_set[1])[:p]
    side = np.zeros(n + p, dtype=np.int32)
    for i in range(n + p):
        flo, fhi = abs(lo[i]) < QP_INF, abs(hi[i]) < QP_INF
        if lo[i] == hi[i] and flo:
            side[i] = 3
        elif bits is not None:
            side[i] = 1 if (bits[i] == 1 and flo) else (2 if (bits[i] == 2 and fhi) else 0)
        elif flo and abs(val[i] - lo[i]) < 1e-7 * max(1.0, abs(lo[i])):
            side[i] = 1
        elif fhi and abs(val[i] - hi[i]) < 1e-7 * max(1.0, abs(hi[i])):
            side[i] = 2
    return side, lo, hi, val


def qp_certificate(x, H=None, g=None, A=None, b=None, C_=None, lb=None, ub=None, Clb=None, Cub=None, status=None, working_set=None, v=None):
    """wbc_qp_certificate for ONE problem in numpy, the same algebra: Cholesky H = L L', Y = L^-1 N', QR Y = Q1 R, y = R^-1 Q1' L^-1 grad f, and
    with z = L^-1 v: w = R^-1 Q1' z, u = L^-T (z - Q1 Q1' z). Give H, g or A, b. Returns dict(y_bounds [n], y_rows [p], kkt [4], objective,
    n_active, sens_x, sens_bounds, sens_rows, cert_status); side [n + p] (qp_active_sides) comes along for qp_gradients."""
    from scipy.linalg import solve_triangular
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    p = 0 if C_ is None else len(C_)
    out = dict(y_bounds=np.zeros(n), y_rows=np.zeros(p), kkt=np.zeros(4), objective=0.0, n_active=0, sens_x=np.zeros(n), sens_bounds=np.zeros(n),
               sens_rows=np.zeros(p), cert_status=capi.CERT_OK, side=np.zeros(n + p, dtype=np.int32))
    if status is not None and int(status) != 0:
        out["cert_status"] = capi.CERT_UNSOLVED
        return out
    ls = A is not None
    data = [x] + ([np.asarray(A, float), np.asarray(b, float)] if ls else [np.asarray(H, float), np.asarray(g, float)])
    data += [np.asarray(C_, float)] if p else []
    data += [np.asarray(v, float)] if v is not None else []
    bounds = [np.asarray(a, float) for a in (lb, ub, Clb if p else None, Cub if p else None) if a is not None]
    if not all(np.isfinite(a).all() for a in data) or any(np.isnan(a).any() for a in bounds):
        out["cert_status"] = capi.CERT_NUMERICAL
        return out
    side, lo, hi, val = qp_active_sides(x, C_, lb, ub, Clb, Cub, working_set)
    flo, fhi = np.abs(lo) < QP_INF, np.abs(hi) < QP_INF
    viol = max(0.0, float(np.where(flo, lo - val, 0.0).max()), float(np.where(fhi, val - hi, 0.0).max()))
    if ls:
        A, b = np.asarray(A, float), np.asarray(b, float)
        Hm = A.T @ A
        ax = A @ x
        grad = A.T @ (ax - b)
        obj = 0.5 * ax @ ax - b @ ax
    else:
        Hm, g = np.asarray(H, float), np.asarray(g, float)
        hx = Hm @ x
        grad = hx + g
        obj = x @ (0.5 * hx + g)
    act = np.nonzero(side)[0]
    k = len(act)
    out.update(n_active=k, objective=float(obj), side=side)
    out["kkt"][1] = viol
    if k > n:
        out["cert_status"] = capi.CERT_DEPENDENT
        return out
    try:
        L = np.linalg.cholesky(Hm)
    except np.linalg.LinAlgError:
        out.update(cert_status=capi.CERT_NUMERICAL, n_active=0, objective=0.0, kkt=np.zeros(4), side=np.zeros(n + p, dtype=np.int32))
        return out
    Nall = np.vstack([np.eye(n)] + ([np.asarray(C_, float)] if p else []))
    N = Nall[act]
    Y = solve_triangular(L, N.T, lower=True) if k else np.zeros((n, 0))
    Q1, R = np.linalg.qr(Y)
    if k and (np.abs(np.diag(R)) <= CERT_DEP_TOL * np.linalg.norm(Y, axis=0)).any():
        out["cert_status"] = capi.CERT_DEPENDENT
        return out
    y = solve_triangular(R, Q1.T @ solve_triangular(L, grad, lower=True)) if k else np.zeros(0)
    yall = np.zeros(n + p)
    yall[act] = y
    e = np.where(side == 2, hi, lo)
    out["y_bounds"], out["y_rows"] = yall[:n], yall[n:]
    out["kkt"][0] = np.abs(grad - Nall.T @ yall).max()
    out["kkt"][2] = max(0.0, float(np.where(side == 1, -yall, 0.0).max()), float(np.where(side == 2, yall, 0.0).max()))
    out["kkt"][3] = float(np.abs(yall * (val - e))[side != 0].max()) if k else 0.0
    if v is not None:
        z = solve_triangular(L, np.asarray(v, float), lower=True)
        qz = Q1.T @ z
        wall = np.zeros(n + p)
        wall[act] = solve_triangular(R, qz) if k else np.zeros(0)
        out["sens_x"] = solve_triangular(L.T, z - Q1 @ qz, lower=False)
        out["sens_bounds"], out["sens_rows"] = wall[:n], wall[n:]
    return out


def qp_gradients(x, y, u, w, side, C_=None):
    """The gradients of L(x*) for dL/dx = v, from a certificate with sensitivities (include/wbc.h): y, w, side are [n + p], variables then rows
    (qp_certificate's y_bounds | y_rows, sens_bounds | sens_rows, side), u = sens_x.  dL/dg = -u, dL/dH = -1/2 (u x' + x u'),
    dL/dC_j = -w_j x' + y_j u', and dL/de_i = w_i goes to the side constraint i sits at: lb / Clb at a lower side, ub / Cub at an upper side,
    half and half on an equality. Returns dict(g, H, C, lb, ub, Clb, Cub)."""
    x, y, u, w, side = (np.asarray(a) for a in (x, y, u, w, side))
    n = len(x)
    glo = np.where(side == 1, w, 0.0) + np.where(side == 3, 0.5 * w, 0.0)
    ghi = np.where(side == 2, w, 0.0) + np.where(side == 3, 0.5 * w, 0.0)
    return dict(g=-u, H=-0.5 * (np.outer(u, x) + np.outer(x, u)), C=-np.outer(w[n:], x) + np.outer(y[n:], u),
                lb=glo[:n], ub=ghi[:n], Clb=glo[n:], Cub=ghi[n:])


# ---- the tick as a layer (wbc_tick_vjp, include/wbc.h): dL/d(task weights, gains, targets) restated in numpy from UNWEIGHTED Jacobian rows
def _support_columns(model, joint):
    """bool [26]: the velocity columns that move a body of `joint` (the joint and its ancestors)"""
    sup = np.zeros(capi.V_STRIDE, dtype=bool)
    j = int(joint)
    while j > 0:
        jd = model.data["joints"][j]
        sup[jd["idx_v"]:jd["idx_v"] + (6 if jd["type_id"] == capi.JT["FF"] else 1)] = True
        j = jd["parent"]
    return sup


def frame_rows(model, J, oMf, role, world):
    """The six unweighted Jacobian rows [B, 6, 26] of the controller frame `role` (capi.FR_*) from the WORLD joint Jacobians J [B, 6, 26]
    (pin.computeJointJacobians) and the frame placements oMf: getFrameJacobian in WORLD (world=True) or LOCAL_WORLD_ALIGNED."""
    Jf = np.where(_support_columns(model, model.blob.frame_joint[role])[None, None, :], J, 0.0)
    if not world:                                                         # reference point at the frame origin: lin - p x ang
        p = oMf[:, role, 9:12]
        Jf = Jf.copy()
        Jf[:, 0:3, :] -= np.cross(p[:, None, :], Jf[:, 3:6, :].transpose(0, 2, 1)).transpose(0, 2, 1)
    return Jf


def _R_to_quat(R):
    """scipy Rotation.from_matrix(R).as_quat() branch logic on [B, 9] row-major rotations, (x, y, z, w), no sign canonicalisation
    (Robot_Wrapper4.py:964-965)"""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 9)
    out = np.zeros((len(R), 4))
    for n, M in enumerate(R):
        tr = M[0] + M[4] + M[8]
        dec = [M[0], M[4], M[8], tr]
        c = 0
        for i in range(1, 4):
            if dec[i] > dec[c]:
                c = i
        q = np.zeros(4)
        if c != 3:
            i, j = c, (c + 1) % 3
            k = (j + 1) % 3
            q[i] = 1 - tr + 2 * M[3 * i + i]
            q[j] = M[3 * j + i] + M[3 * i + j]
            q[k] = M[3 * k + i] + M[3 * i + k]
            q[3] = M[3 * k + j] - M[3 * j + k]
        else:
            q[:] = M[7] - M[5], M[2] - M[6], M[3] - M[1], 1 + tr
        out[n] = q / np.sqrt(q @ q)
    return out


def _euler_xyz_to_R(e):
    """[B, 9] row-major Rz(c) Ry(b) Rx(a)"""
    sa, ca, sb, cb, sc, cc = np.sin(e[:, 0]), np.cos(e[:, 0]), np.sin(e[:, 1]), np.cos(e[:, 1]), np.sin(e[:, 2]), np.cos(e[:, 2])
    return np.stack([cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa,
                     -sb, cb * sa, cb * ca], axis=1)


def tick_gradients(model, cfg, inputs, x, u, dt, fk, task_params=None):
    """wbc_tick_vjp restated for B instances of ONE model: x = qdot [B, 26], u = the certificate's sens_x [B, 26] for the caller's
    v = dL/dqdot, inputs keyed like WbcTickIn, task_params [B, 85] or None (the configuration's block). fk follows state_slack's convention
    (fk(q) -> oMf [B, nframes, 12], fk.com(q) -> [B, 3]) and also gives the unweighted rows' source, fk.jacobians(q) -> (J [B, 6, 26] the WORLD
    joint Jacobians of pin.computeJointJacobians, Jcom [B, 3, 26]). Task rows see q (never q_con). MANI / HYBRID need inputs["posture_u"].
    With r = b - A x and s = A u: dL/dA = r u' - s x', dL/db = s; every row is (weights) x (an unweighted row), and the rules of
    include/wbc.h follow block by block. Returns dict(d_task_params [B, 85], d_ee_target, d_prev_ee_target [B, 5, 3], d_trunk_target,
    d_prev_trunk_target, d_com_target, d_com_target_vel [B, 3], d_posture_u [B, 26] — zeros where the configuration does not read the input —
    and dA [B, m, 26], db [B, m], A [B, m, 26], b [B, m]: the task stack rebuilt from the unweighted rows, and dL/dA, dL/db)."""
    import wbc_model
    q = np.asarray(inputs["q"], dtype=np.float64).reshape(-1, capi.Q_STRIDE)
    B, NVs, nv = q.shape[0], capi.V_STRIDE, model.nv
    x, u = np.asarray(x, dtype=np.float64).reshape(B, NVs), np.asarray(u, dtype=np.float64).reshape(B, NVs)
    tp = wbc_model.task_params(cfg, B) if task_params is None else np.asarray(task_params, dtype=np.float64).reshape(B, capi.TASK_PARAMS_DOUBLES)
    L = wbc_model.TASK_PARAMS_LAYOUT
    P = {k: tp[:, sl].reshape((B,) + shape) for k, (sl, shape) in L.items()}
    oMf = fk(q)
    J, Jcom = fk.jacobians(q)
    g = {k: np.zeros((B,) + shape) for k, (sl, shape) in L.items()}
    out = dict(d_ee_target=np.zeros((B, 5, 3)), d_prev_ee_target=np.zeros((B, 5, 3)), d_trunk_target=np.zeros((B, 3)),
               d_prev_trunk_target=np.zeros((B, 3)), d_com_target=np.zeros((B, 3)), d_com_target_vel=np.zeros((B, 3)),
               d_posture_u=np.zeros((B, NVs)))
    A_, b_, dA_, db_ = [], [], [], []

    def block(Jr, c, bv):
        """rows A = c J_r, b = bv (c, bv [B, R]): -> jx, ju, s, rho [B, R], and the rows are recorded"""
        jx, ju = np.einsum("brk,bk->br", Jr, x), np.einsum("brk,bk->br", Jr, u)
        s, rho = c * ju, bv - c * jx
        A_.append(c[:, :, None] * Jr)
        b_.append(bv)
        dA_.append(rho[:, :, None] * u[:, None, :] - s[:, :, None] * x[:, None, :])
        db_.append(s)
        return jx, ju, s, rho

    for e in range(capi.NEE):
        if not cfg.task_ee[e]:
            continue
        Jr = frame_rows(model, J, oMf, capi.FR_EE0 + e, world=False)
        xt = np.asarray(inputs["ee_target"], dtype=np.float64).reshape(B, 5, 3)[:, e]
        xp = np.asarray(inputs["prev_ee_target"], dtype=np.float64).reshape(B, 5, 3)[:, e]
        W, w, gain = P["ee_W"][:, e], P["ee_w"][:, e][:, None], P["ee_gain"][:, e]
        err = (xt - oMf[:, capi.FR_EE0 + e, 9:12]) / dt
        vel = np.zeros((B, 6))
        vel[:, :3] = (xt - xp) / dt + gain[:, :3] * err
        if inputs.get("ee_ref_rot") is not None:
            Rs = np.asarray(inputs["ee_ref_rot"], dtype=np.float64).reshape(B, 5, 3, 3)[:, e]
            Rp = np.asarray(inputs["ee_prev_rot"], dtype=np.float64).reshape(B, 5, 3, 3)[:, e]
            S = np.einsum("bij,bkj->bik", (Rs - Rp) / dt, Rs)               # ((R* - R*_prev) / dt) R*^T
            vel[:, 3:] = np.stack([S[:, 2, 1], S[:, 0, 2], S[:, 1, 0]], axis=1)
        jx, ju, s, rho = block(Jr, W * w, w * vel)
        t = rho * ju - s * jx
        dvel = w * s
        g["ee_W"][:, e] = w * t
        g["ee_w"][:, e] = (W * t + s * vel).sum(axis=1)
        g["ee_gain"][:, e, :3] = dvel[:, :3] * err
        out["d_ee_target"][:, e] = dvel[:, :3] * (1.0 + gain[:, :3]) / dt
        out["d_prev_ee_target"][:, e] = -dvel[:, :3] / dt
    if cfg.task_trunk:
        Jr = frame_rows(model, J, oMf, capi.FR_TRUNK, world=True)
        xt = np.asarray(inputs["trunk_target"], dtype=np.float64).reshape(B, 3)
        xp = np.asarray(inputs["prev_trunk_target"], dtype=np.float64).reshape(B, 3)
        W, w, gain = P["trunk_W"], P["trunk_w"].reshape(B, 1), P["trunk_gain"]
        err = (xt - oMf[:, capi.FR_TRUNK, 9:12]) / dt
        fq = _R_to_quat(oMf[:, capi.FR_TRUNK, 0:9])
        er = np.asarray(inputs["trunk_ref_euler"], dtype=np.float64).reshape(B, 3)
        rq, Rs = euler_xyz_to_quat(er), _euler_xyz_to_R(er).reshape(B, 3, 3)
        qe = np.stack([fq[:, 3] * rq[:, 0] - fq[:, 0] * rq[:, 3] + fq[:, 1] * rq[:, 2] - fq[:, 2] * rq[:, 1],
                       fq[:, 3] * rq[:, 1] - fq[:, 1] * rq[:, 3] - fq[:, 0] * rq[:, 2] + fq[:, 2] * rq[:, 0],
                       fq[:, 3] * rq[:, 2] - fq[:, 3] * rq[:, 2] + fq[:, 0] * rq[:, 1] - fq[:, 1] * rq[:, 0]], axis=1)   # :974-976 (sic)
        Ro = np.asarray(inputs["trunk_prev_rot"], dtype=np.float64).reshape(B, 3, 3)
        S = np.einsum("bij,bjk->bik", (Rs - Ro) / dt, Rs)                   # D R* (not R*^T: :984)
        vel = np.zeros((B, 6))
        vel[:, :3] = (xt - xp) / dt + gain[:, :3] * err
        vel[:, 3:] = np.stack([S[:, 2, 1], S[:, 0, 2], S[:, 1, 0]], axis=1) + gain[:, 3:] * qe
        jx, ju, s, rho = block(Jr, W * w, w * vel)
        t = rho * ju - s * jx
        dvel = w * s
        g["trunk_W"][:] = w * t
        g["trunk_w"][:] = (W * t + s * vel).sum(axis=1)
        g["trunk_gain"][:, :3] = dvel[:, :3] * err
        g["trunk_gain"][:, 3:] = dvel[:, 3:] * qe
        out["d_trunk_target"][:] = dvel[:, :3] * (1.0 + gain[:, :3]) / dt
        out["d_prev_trunk_target"][:] = -dvel[:, :3] / dt
    if cfg.task_com:
        ct = np.asarray(inputs["com_target"], dtype=np.float64).reshape(B, 3)
        cv = np.asarray(inputs["com_target_vel"], dtype=np.float64).reshape(B, 3)
        W, gain = P["com_W"], P["com_gain"]
        err = ct - fk.com(q)
        jx, ju, s, rho = block(Jcom, W, cv + gain * err)
        g["com_W"][:] = rho * ju - s * jx
        g["com_gain"][:] = s * err
        out["d_com_target"][:] = s * gain
        out["d_com_target_vel"][:] = s
    if cfg.task_joint:
        d = ((1.0 / nv) * P["joint_w"]).reshape(B, 1)
        up = np.zeros((B, NVs))
        if cfg.task_joint == capi.JOINT_PREV:
            up[:, :nv] = np.delete(q, 6, axis=1)[:, :nv]
        elif cfg.task_joint >= capi.JOINT_MANI:
            up[:, :nv] = np.asarray(inputs["posture_u"], dtype=np.float64).reshape(B, NVs)[:, :nv]
        own = (np.arange(NVs) < nv)[None, :]
        Jr = np.broadcast_to(np.where(own[0][:, None], np.eye(NVs), 0.0), (B, NVs, NVs))
        block(Jr, np.broadcast_to(d, (B, NVs)), d * up)
        g["joint_w"][:] = (2.0 / nv) * np.where(own, d * (up - x) * u, 0.0).sum(axis=1)
        if cfg.task_joint >= capi.JOINT_MANI:
            out["d_posture_u"][:] = np.where(own, d * d * u, 0.0)
    dtp = np.zeros((B, capi.TASK_PARAMS_DOUBLES))
    for k, (sl, shape) in L.items():
        dtp[:, sl] = g[k].reshape(B, -1)
    cat = (lambda a, w: np.concatenate(a, axis=1) if a else np.zeros((B, 0) + w))
    out.update(d_task_params=dtp, A=cat(A_, (NVs,)), b=cat(b_, ()), dA=cat(dA_, (NVs,)), db=cat(db_, ()))
    return out


# ---- the tick as a layer, state side (wbc_tick_vjp_state, include/wbc.h): dL/dq in tangent coordinates, restated in numpy
def _dof_tree(model):
    """(joint [26] of every velocity column (-1: none), after [26, 26] bool): after[k, d] — column d's WORLD Jacobian column moves with the
    tangent coordinate k: k's joint is a strict ancestor of d's joint, or k and d are two free-flyer columns (M <- M exp(delta))."""
    NVs = capi.V_STRIDE
    joints = model.data["joints"]
    jof = np.full(NVs, -1, dtype=np.int64)
    ff = np.zeros(NVs, dtype=bool)
    for j in range(1, model.njoints):
        jd = joints[j]
        n = 6 if jd["type_id"] == capi.JT["FF"] else 1
        jof[jd["idx_v"]:jd["idx_v"] + n] = j
        ff[jd["idx_v"]:jd["idx_v"] + n] = n == 6
    after = np.zeros((NVs, NVs), dtype=bool)
    for d in range(NVs):
        if jof[d] < 0:
            continue
        a = joints[int(jof[d])]["parent"]
        while a > 0:
            after[jof == a, d] = True
            a = joints[a]["parent"]
        if ff[d]:
            after[ff, d] = True
    return jof, after


def _point_rows_dq(J, sup, after, p, world, z):
    """d(J_r z)/d delta [B, 6, 26] of the six rows of a frame with support `sup` [26] at the point p [B, 3] (LOCAL_WORLD_ALIGNED) or at the
    world origin (world=True), from the WORLD joint Jacobians J [B, 6, 26]:  S_k x_m T_k(z),  T_k(z) = sum of S_d z_d over the support columns
    d after k; LOCAL_WORLD_ALIGNED adds (d ang) x p + ang x (l_k + a_k x p) to the linear rows."""
    Jz = np.where(sup[None, None, :], J, 0.0) * z[:, None, :]
    T = np.einsum("bcd,kd->bkc", Jz, after.astype(np.float64))           # [B, k, 6]
    S = J.transpose(0, 2, 1)                                             # [B, k, 6]
    lk, ak = S[:, :, 0:3], S[:, :, 3:6]
    D = np.concatenate([np.cross(ak, T[:, :, 0:3]) + np.cross(lk, T[:, :, 3:6]), np.cross(ak, T[:, :, 3:6])], axis=2)
    if not world:
        ang = Jz[:, 3:6, :].sum(axis=2)[:, None, :]
        dp = lk + np.cross(ak, p[:, None, :])
        D[:, :, 0:3] += np.cross(D[:, :, 3:6], p[:, None, :]) + np.cross(ang, dp)
    return np.where(sup[None, :, None], D, 0.0).transpose(0, 2, 1)


def frame_rows_dq(model, J, oMf, role, world, z):
    """d(J_r z)/d delta_k [B, 6, 26] (row, k) of frame_rows(model, J, oMf, role, world) contracted with a fixed z [B, 26]; delta: the tangent
    coordinates of q (+) delta = pin.integrate(q, delta), base columns in the base-local frame. No 26 x 26 x 6 tensor is formed."""
    sup = _support_columns(model, model.blob.frame_joint[role])
    return _point_rows_dq(J, sup, _dof_tree(model)[1], oMf[:, role, 9:12], world, np.asarray(z, dtype=np.float64))


def com_rows_dq(model, J, oMi, z):
    """d(Jcom z)/d delta_k [B, 3, 26]: the mass-weighted mean over the bodies of the LOCAL_WORLD_ALIGNED linear rows at the bodies' centres of
    mass. oMi [B, >= njoints, 12]: the joint placements (rotation row-major, then the translation)."""
    z = np.asarray(z, dtype=np.float64)
    after = _dof_tree(model)[1]
    out, mtot = np.zeros((J.shape[0], 3, capi.V_STRIDE)), 0.0
    for j in range(1, model.njoints):
        m = float(model.blob.mass[j])
        if m == 0.0:
            continue
        c = np.einsum("bij,j->bi", oMi[:, j, 0:9].reshape(-1, 3, 3), np.array(model.blob.com[j][:])) + oMi[:, j, 9:12]
        out += m * _point_rows_dq(J, _support_columns(model, j), after, c, False, z)[:, 0:3]
        mtot += m
    return out / mtot


def _quat_right(q4, e):
    """q (x) (e, 0), Hamilton, (x, y, z, w): [B, 4]"""
    v, w = q4[:, 0:3], q4[:, 3:4]
    e = np.broadcast_to(e, v.shape)
    return np.concatenate([w * e + np.cross(v, e), -(v * e).sum(axis=1, keepdims=True)], axis=1)


def _quat_to_R(q4):
    x, y, z, w = q4[:, 0], q4[:, 1], q4[:, 2], q4[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def raw_tangent_map(model, q):
    """G = d q_raw / d delta [B, 27, 26] at delta = 0 of q (+) delta: xyz rows R (the base rotation), quaternion rows 1/2 q (x) (e_k, 0), joint
    rows the identity (q index of the joint's own angle)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, capi.Q_STRIDE)
    G = np.zeros((q.shape[0], capi.Q_STRIDE, capi.V_STRIDE))
    G[:, 0:3, 0:3] = _quat_to_R(q[:, 3:7])
    for k in range(3):
        G[:, 3:7, 3 + k] = 0.5 * _quat_right(q[:, 3:7], np.eye(3)[k])
    for jd in model.data["joints"][2:model.njoints]:
        G[:, jd["idx_q"], jd["idx_v"]] = 1.0
    return G


def tangent_to_raw(q, d):
    """The gradient [B, 27] in raw coordinates of L(tick(q_raw with its quaternion normalised)) from d = dL/d delta [B, 26] (wbc_tick_vjp_state's
    d_q). With the unit quaternion qn = quat / |quat| = (x, y, z, w), R = R(qn) the base rotation, d_lin = d[0:3], d_ang = d[3:6]:
      xyz        <- R d_lin
      quaternion <- 2 qn (x) (d_ang, 0) / |quat|  =  2 (w d_ang + (x, y, z) x d_ang ; -(x, y, z) . d_ang) / |quat|
      joints     <- d[6:]  (raw index one higher; entries beyond a model's nq get what d holds beyond its nv: 0)
    The quaternion rows are the pull-back of the tangent through the normalisation: delta_ang = 2 Im(conj(qn) (x) dq) / |quat| for a raw
    perturbation dq, so the gradient has no component along the quaternion itself. numpy arrays or torch tensors; written in elementwise
    operations in one fixed order, so that both give the same bits."""
    if hasattr(q, "detach"):
        import torch as xp
        cat = lambda parts: xp.stack(parts, dim=1)      # noqa: E731
    else:
        xp = np
        q, d = np.asarray(q, dtype=np.float64).reshape(-1, capi.Q_STRIDE), np.asarray(d, dtype=np.float64).reshape(-1, capi.V_STRIDE)
        cat = lambda parts: np.stack(parts, axis=1)     # noqa: E731
    nrm = xp.sqrt(q[:, 3] * q[:, 3] + q[:, 4] * q[:, 4] + q[:, 5] * q[:, 5] + q[:, 6] * q[:, 6])
    x, y, z, w = q[:, 3] / nrm, q[:, 4] / nrm, q[:, 5] / nrm, q[:, 6] / nrm
    l0, l1, l2, a0, a1, a2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4], d[:, 5]
    cols = [(1 - 2 * (y * y + z * z)) * l0 + (2 * (x * y - z * w)) * l1 + (2 * (x * z + y * w)) * l2,
            (2 * (x * y + z * w)) * l0 + (1 - 2 * (x * x + z * z)) * l1 + (2 * (y * z - x * w)) * l2,
            (2 * (x * z - y * w)) * l0 + (2 * (y * z + x * w)) * l1 + (1 - 2 * (x * x + y * y)) * l2,
            2 * (w * a0 + (y * a2 - z * a1)) / nrm,
            2 * (w * a1 + (z * a0 - x * a2)) / nrm,
            2 * (w * a2 + (x * a1 - y * a0)) / nrm,
            2 * (-(x * a0 + y * a1 + z * a2)) / nrm]
    return cat(cols + [d[:, k] for k in range(6, capi.V_STRIDE)])


def damper_bounds(cfg, nv, q):
    """velDamperJointConstraints as the oracle states it (oracle/wbc_oracle.c): -> lb, ub, dlb, dub [B, 26]; dlb, dub the derivative with
    respect to q[damper_qidx[i]], branch by branch: 0 on a constant branch, at a kink the branch the oracle's comparisons select."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, capi.Q_STRIDE)
    B, NVs = q.shape[0], capi.V_STRIDE
    lb, ub, dlb, dub = np.zeros((B, NVs)), np.zeros((B, NVs)), np.zeros((B, NVs)), np.zeros((B, NVs))
    if not cfg.use_bounds:
        lb[:, :nv], ub[:, :nv] = -1e30, 1e30
        return lb, ub, dlb, dub
    slope = cfg.damper_coef / (cfg.damper_qi - cfg.damper_qs)
    for i in range(min(nv, int(cfg.lock_from))):
        qi, lo, hi, vm = q[:, cfg.damper_qidx[i]], cfg.damper_lo[i], cfg.damper_hi[i], cfg.damper_vmax[i]
        zone = qi <= lo + cfg.damper_qi
        lraw = -cfg.damper_coef * (qi - lo - cfg.damper_qs) / (cfg.damper_qi - cfg.damper_qs)
        lin = zone & ~(lraw > vm) & ~(lraw < -vm)
        l = np.where(zone, np.clip(lraw, -vm, vm), -vm)
        dl = np.where(lin, -slope, 0.0)
        zone = qi >= hi - cfg.damper_qi
        uraw = cfg.damper_coef * (hi - qi - cfg.damper_qs) / (cfg.damper_qi - cfg.damper_qs)
        lin = zone & ~(uraw < -vm) & ~(uraw > vm)
        uu = np.where(zone, np.clip(uraw, -vm, vm), vm)
        du = np.where(lin, -slope, 0.0)
        lb[:, i], dlb[:, i] = np.where(l > 0, -l, l), np.where(l > 0, -dl, dl)
        ub[:, i], dub[:, i] = np.where(uu < 0, -uu, uu), np.where(uu < 0, -du, du)
    return lb, ub, dlb, dub


def _side_split(w, val, lo, hi, bits):
    """(dL/d lower, dL/d upper) of the constraints with values val between lo and hi and sensitivities w: wbc_qp_certificate's rule — with a
    working set its marked side (bits: 1 lower, 2 upper), without one the lower side if |val - lo| < 1e-7 max(1, |lo|), else the upper; half and
    half where lo == hi."""
    if bits is None:
        low = np.abs(val - lo) < 1e-7 * np.maximum(1.0, np.abs(lo))
        up = ~low
    else:
        low, up = bits == 1, bits == 2
    eq = lo == hi
    return np.where(eq, 0.5 * w, np.where(low, w, 0.0)), np.where(eq, 0.5 * w, np.where(up, w, 0.0))


def tick_state_gradients(model, cfg, inputs, x, u, dt, fk, sens_bounds=None, sens_rows=None, y_rows=None, task_params=None, working_set=None):
    """wbc_tick_vjp_state restated for B instances of ONE model, from unweighted rows: x = qdot, u = sens_x, w = sens_bounds [B, 26] /
    sens_rows [B, p], y = y_rows [B, p] of the certificate for the caller's v = dL/dqdot; working_set [B, 2] uint64 or None. Conventions of
    tick_gradients; fk also gives fk.joints(q) -> oMi [B, njoints, 12]. q_con is not supported; posture_u and the orientation references are
    held constant. With r = b - A x and s = A u:
      dL/d delta_k = sum_rows (r_i u - s_i x) . dA_i/d delta_k + s_i db_i/d delta_k + sum_j (y_j u - w_j x) . dC_j/d delta_k + sum_active w_i de_i/d delta_k
    Returns dict(d_q [B, 26] (tangent coordinates: q (+) delta = pin.integrate(q, delta)), d_trunk_box_center [B, 4], and what the algebra
    contracts: dA, db (tick_gradients'), dC [B, p, 26], dClb, dCub [B, p], dlb, dub [B, 26])."""
    q = np.asarray(inputs["q"], dtype=np.float64).reshape(-1, capi.Q_STRIDE)
    B, NVs, nv = q.shape[0], capi.V_STRIDE, model.nv
    x, u = np.asarray(x, dtype=np.float64).reshape(B, NVs), np.asarray(u, dtype=np.float64).reshape(B, NVs)
    tg = tick_gradients(model, cfg, inputs, x, u, dt, fk, task_params)
    import wbc_model
    tp = wbc_model.task_params(cfg, B) if task_params is None else np.asarray(task_params, dtype=np.float64).reshape(B, capi.TASK_PARAMS_DOUBLES)
    P = {k: tp[:, sl].reshape((B,) + shape) for k, (sl, shape) in wbc_model.TASK_PARAMS_LAYOUT.items()}
    oMf, oMi = fk(q), fk.joints(q)
    J, Jcom = fk.jacobians(q)
    G = raw_tangent_map(model, q)
    dq = np.zeros((B, NVs))
    A, b = tg["A"], tg["b"]
    rr, ss = b - np.einsum("bmk,bk->bm", A, x), np.einsum("bmk,bk->bm", A, u)
    row = 0

    def rows_term(alpha, beta, Dx, Du):
        return np.einsum("br,brk->bk", alpha, Du) - np.einsum("br,brk->bk", beta, Dx)

    def lwa_lin(role):
        return frame_rows(model, J, oMf, role, world=False)[:, 0:3]
    # ---- task rows
    for e in range(capi.NEE):
        if not cfg.task_ee[e]:
            continue
        c = P["ee_W"][:, e] * P["ee_w"][:, e][:, None]
        r6, s6 = rr[:, row:row + 6], ss[:, row:row + 6]
        dq += rows_term(c * r6, c * s6, frame_rows_dq(model, J, oMf, capi.FR_EE0 + e, False, x), frame_rows_dq(model, J, oMf, capi.FR_EE0 + e, False, u))
        db = -(P["ee_w"][:, e][:, None] * P["ee_gain"][:, e, :3] / dt)          # b_i = w (.. + gain_i (xt_i - p_i) / dt)
        dq += np.einsum("br,brk->bk", s6[:, :3] * db, lwa_lin(capi.FR_EE0 + e))
        row += 6
    if cfg.task_trunk:
        c = P["trunk_W"] * P["trunk_w"].reshape(B, 1)
        r6, s6 = rr[:, row:row + 6], ss[:, row:row + 6]
        dq += rows_term(c * r6, c * s6, frame_rows_dq(model, J, oMf, capi.FR_TRUNK, True, x), frame_rows_dq(model, J, oMf, capi.FR_TRUNK, True, u))
        w = P["trunk_w"].reshape(B, 1)
        dq += np.einsum("br,brk->bk", s6[:, :3] * (-(w * P["trunk_gain"][:, :3] / dt)), lwa_lin(capi.FR_TRUNK))
        # quaternion feedback: qe is linear in fq, d fq / d delta_k = 1/2 fq (x) (R_f' a_k, 0) for the columns that move the frame
        Rf = oMf[:, capi.FR_TRUNK, 0:9].reshape(B, 3, 3)
        fq = _R_to_quat(oMf[:, capi.FR_TRUNK, 0:9])
        rq = euler_xyz_to_quat(np.asarray(inputs["trunk_ref_euler"], dtype=np.float64).reshape(B, 3))

        def qe_of(f):
            return np.stack([f[:, 3] * rq[:, 0] - f[:, 0] * rq[:, 3] + f[:, 1] * rq[:, 2] - f[:, 2] * rq[:, 1],
                             f[:, 3] * rq[:, 1] - f[:, 1] * rq[:, 3] - f[:, 0] * rq[:, 2] + f[:, 2] * rq[:, 0],
                             f[:, 3] * rq[:, 2] - f[:, 3] * rq[:, 2] + f[:, 0] * rq[:, 1] - f[:, 1] * rq[:, 0]], axis=1)
        Jang = frame_rows(model, J, oMf, capi.FR_TRUNK, world=True)[:, 3:6]     # a_k of the support columns
        loc = np.einsum("bji,bjk->bik", Rf, Jang)                             # R_f' a_k
        coef = s6[:, 3:] * w * P["trunk_gain"][:, 3:]
        for m in range(3):
            dq += (coef * qe_of(0.5 * _quat_right(fq, np.eye(3)[m]))).sum(axis=1)[:, None] * loc[:, m, :]
        row += 6
    if cfg.task_com:
        c = P["com_W"]
        r3, s3 = rr[:, row:row + 3], ss[:, row:row + 3]
        dq += rows_term(c * r3, c * s3, com_rows_dq(model, J, oMi, x), com_rows_dq(model, J, oMi, u))
        dq += np.einsum("br,brk->bk", s3 * (-P["com_gain"]), Jcom)
        row += 3
    if cfg.task_joint:
        if cfg.task_joint == capi.JOINT_PREV:                                 # b_k = d up_k, up = np.delete(q, 6)[:nv]
            d = ((1.0 / nv) * P["joint_w"]).reshape(B, 1)
            Gd = np.delete(G, 6, axis=1)[:, :NVs]
            dq += np.einsum("bi,bik->bk", np.where(np.arange(NVs)[None, :] < nv, ss[:, row:row + NVs] * d, 0.0), Gd)
        row += NVs
    # ---- constraint rows, in findConstraints' order
    rows_, cl_, cu_, dcur_ = [], [], [], []                                    # unweighted rows, bounds, and d(bounds)/d delta [B, 26] per row (lower, upper)
    com = fk.com(q) if (cfg.con_com or cfg.task_com) else None
    bc = None
    if cfg.con_com:
        pFL, pRR = oMf[:, capi.FR_EE0 + 1, 9:12], oMf[:, capi.FR_EE0 + 2, 9:12]
        JFL, JRR = lwa_lin(capi.FR_EE0 + 1), lwa_lin(capi.FR_EE0 + 2)
        k = cfg.com_box_scale / dt
        for r in range(2):
            rows_.append(("com", r))
            cl_.append((pRR[:, r] - com[:, r]) / dt * cfg.com_box_scale)
            cu_.append((pFL[:, r] - com[:, r]) / dt * cfg.com_box_scale)
            dcur_.append((k * (JRR[:, r] - Jcom[:, r]), k * (JFL[:, r] - Jcom[:, r])))
    if cfg.con_trunk:
        bc = np.asarray(inputs["trunk_box_center"], dtype=np.float64).reshape(B, 4)
        R = oMf[:, capi.FR_TRUNK, 0:9]
        Jt = frame_rows(model, J, oMf, capi.FR_TRUNK, world=False)
        om = Jt[:, 3:6]                                                       # world angular velocity per column: dR = [om] R
        dR = lambda i, j: np.cross(om.transpose(0, 2, 1), R.reshape(B, 3, 3)[:, None, :, j])[:, :, i]   # noqa: E731  d R_ij / d delta_k [B, 26]
        R00, R10, R20, R21, R22 = (R[:, i][:, None] for i in (0, 3, 6, 7, 8))
        cxy = np.sqrt(R21 * R21 + R22 * R22)
        de = [(R22 * dR(2, 1) - R21 * dR(2, 2)) / (R21 * R21 + R22 * R22),
              (-cxy * dR(2, 0) + R20 * ((R21 * dR(2, 1) + R22 * dR(2, 2)) / cxy)) / (R20 * R20 + cxy * cxy),
              (R00 * dR(1, 0) - R10 * dR(0, 0)) / (R00 * R00 + R10 * R10)]
        cur = np.stack([oMf[:, capi.FR_TRUNK, 11], np.arctan2(R[:, 7], R[:, 8]), np.arctan2(-R[:, 6], cxy[:, 0]), np.arctan2(R[:, 3], R[:, 0])], axis=1)
        dcur = [Jt[:, 2]] + de
        var = np.stack([bc[:, 0] * cfg.trunk_box_z_frac] + [np.full(B, cfg.trunk_box_ang)] * 3, axis=1)
        k = cfg.trunk_box_scale / dt
        for r in range(4):
            rows_.append(("trunk", r))
            cl_.append(((bc[:, r] - var[:, r]) - cur[:, r]) / dt * cfg.trunk_box_scale)
            cu_.append(((bc[:, r] + var[:, r]) - cur[:, r]) / dt * cfg.trunk_box_scale)
            dcur_.append((-k * dcur[r], -k * dcur[r]))
    for e in range(capi.NEE):
        if cfg.con_ee[e]:
            for r in range(3):
                rows_.append(("ee", e, r))
                cl_.append(np.zeros(B))
                cu_.append(np.zeros(B))
                dcur_.append((np.zeros((B, NVs)), np.zeros((B, NVs))))
    p = len(rows_)
    out = dict(dA=tg["dA"], db=tg["db"], dC=np.zeros((B, p, NVs)), dClb=np.zeros((B, p)), dCub=np.zeros((B, p)), d_trunk_box_center=np.zeros((B, 4)))
    ws = None if working_set is None else np.asarray(working_set, dtype=np.uint64).reshape(B, 2)

    def bits_of(word, n):
        i = np.arange(n, dtype=np.uint64)[None, :]
        return (((word[:, None] >> i) & np.uint64(1)) | (((word[:, None] >> (i + np.uint64(32))) & np.uint64(1)) << np.uint64(1))).astype(np.int64)
    if p:
        w = np.asarray(sens_rows, dtype=np.float64).reshape(B, p)
        y = np.asarray(y_rows, dtype=np.float64).reshape(B, p)
        out["dC"] = y[:, :, None] * u[:, None, :] - w[:, :, None] * x[:, None, :]
        Dcx = Dcu = None
        Dfx, Dfu = {}, {}
        Cx = np.zeros((B, p))
        for i, rdesc in enumerate(rows_):
            if rdesc[0] == "com":
                if Dcx is None:
                    Dcx, Dcu = com_rows_dq(model, J, oMi, x), com_rows_dq(model, J, oMi, u)
                Dx, Du, Crow = Dcx[:, rdesc[1]], Dcu[:, rdesc[1]], Jcom[:, rdesc[1]]
            else:
                role, world, r = (capi.FR_TRUNK, False, 2 + rdesc[1]) if rdesc[0] == "trunk" else (capi.FR_EE0 + rdesc[1], True, rdesc[2])
                if (role, world) not in Dfx:
                    Dfx[role, world] = frame_rows_dq(model, J, oMf, role, world, x)
                    Dfu[role, world] = frame_rows_dq(model, J, oMf, role, world, u)
                Dx, Du, Crow = Dfx[role, world][:, r], Dfu[role, world][:, r], frame_rows(model, J, oMf, role, world)[:, r]
            dq += y[:, i:i + 1] * Du - w[:, i:i + 1] * Dx
            Cx[:, i] = np.einsum("bk,bk->b", Crow, x)
        cl, cu = np.stack(cl_, axis=1), np.stack(cu_, axis=1)
        out["dClb"], out["dCub"] = _side_split(w, Cx, cl, cu, None if ws is None else bits_of(ws[:, 1], p))
        for i in range(p):
            dq += out["dClb"][:, i:i + 1] * dcur_[i][0] + out["dCub"][:, i:i + 1] * dcur_[i][1]
        if cfg.con_trunk:
            i0 = 2 if cfg.con_com else 0
            k = cfg.trunk_box_scale / dt
            out["d_trunk_box_center"][:, 0] = k * (out["dClb"][:, i0] * (1.0 - cfg.trunk_box_z_frac) + out["dCub"][:, i0] * (1.0 + cfg.trunk_box_z_frac))
            out["d_trunk_box_center"][:, 1:] = k * (out["dClb"][:, i0 + 1:i0 + 4] + out["dCub"][:, i0 + 1:i0 + 4])
    # ---- the velocity bounds
    lb, ub, dlb, dub = damper_bounds(cfg, nv, q)
    wb = np.zeros((B, NVs)) if sens_bounds is None else np.asarray(sens_bounds, dtype=np.float64).reshape(B, NVs)
    out["dlb"], out["dub"] = _side_split(wb, x, lb, ub, None if ws is None else bits_of(ws[:, 0], NVs))
    if cfg.use_bounds:
        qidx = np.array([cfg.damper_qidx[i] for i in range(NVs)])
        dq += np.einsum("bi,bik->bk", out["dlb"] * dlb + out["dub"] * dub, G[:, qidx, :])
    dq[:, nv:] = 0.0
    out["d_q"] = dq
    return out


# ---- the state step as a layer (wbc_step_vjp, include/wbc.h): integrate, then the estimator, in tangent coordinates
def raw_to_tangent(q, c_raw):
    """raw_tangent_map(q)' c_raw: the gradient [B, 26] in tangent coordinates at q of a loss whose gradient in raw coordinates is c_raw [B, 27].
    With (x, y, z, w) = q[3:7] as it stands, R = R(x, y, z, w), c_p = c_raw[0:3], (c_v, c_w) = c_raw[3:7]:
      linear  <- R' c_p
      angular <- (w c_v + c_v x (x, y, z) - c_w (x, y, z)) / 2
      joints  <- c_raw[7:]  (tangent index one lower)
    numpy arrays or torch tensors; elementwise operations in one fixed order, so that both give the same bits (as tangent_to_raw)."""
    if hasattr(q, "detach"):
        import torch as xp
        cat = lambda parts: xp.stack(parts, dim=1)      # noqa: E731
    else:
        xp = np
        q, c_raw = np.asarray(q, dtype=np.float64).reshape(-1, capi.Q_STRIDE), np.asarray(c_raw, dtype=np.float64).reshape(-1, capi.Q_STRIDE)
        cat = lambda parts: np.stack(parts, axis=1)     # noqa: E731
    x, y, z, w = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
    p0, p1, p2, v0, v1, v2, cw = c_raw[:, 0], c_raw[:, 1], c_raw[:, 2], c_raw[:, 3], c_raw[:, 4], c_raw[:, 5], c_raw[:, 6]
    cols = [(1 - 2 * (y * y + z * z)) * p0 + (2 * (x * y + z * w)) * p1 + (2 * (x * z - y * w)) * p2,
            (2 * (x * y - z * w)) * p0 + (1 - 2 * (x * x + z * z)) * p1 + (2 * (y * z + x * w)) * p2,
            (2 * (x * z + y * w)) * p0 + (2 * (y * z - x * w)) * p1 + (1 - 2 * (x * x + y * y)) * p2,
            0.5 * (w * v0 + (v1 * z - v2 * y) - cw * x),
            0.5 * (w * v1 + (v2 * x - v0 * z) - cw * y),
            0.5 * (w * v2 + (v0 * y - v1 * x) - cw * z)]
    return cat(cols + [c_raw[:, k] for k in range(7, capi.Q_STRIDE)])


def _hat(v):
    """[B, 3] -> the cross-product matrices [B, 3, 3]"""
    o = np.zeros(len(v))
    return np.stack([o, -v[:, 2], v[:, 1], v[:, 2], o, -v[:, 0], -v[:, 1], v[:, 0], o], axis=1).reshape(-1, 3, 3)


def _series(X, first_div, sign):
    """I + (sign X) / first_div + (sign X)^2 / (first_div (first_div + 1)) + ...: first_div = 1 the exponential, first_div = 2
    sum_k (sign X)^k / (k + 1)!. The plain power series of [B, n, n] matrices, run until a term no longer changes the sum."""
    n = X.shape[1]
    term = np.broadcast_to(np.eye(n), X.shape).copy()
    total = term.copy()
    for k in range(1, 400):
        term = sign * np.einsum("bij,bjk->bik", term, X) / (k + first_div - 1)
        new = total + term
        if (new == total).all():
            break
        total = new
    return total


def _exp_and_phi(X, want_phi):
    """exp(X) and (want_phi) phi(X) = sum_k X^k / (k + 1)! of [B, n, n] matrices by scaling and doubling: X is halved s times, per instance,
    until its largest absolute row sum is 1 or below; there the plain power series (_series) converge in some twenty terms, none larger than
    the sum itself; then s times exp(2 x) = exp(x)^2 and phi(2 x) = (I + exp(x)) phi(x) / 2. (Summed as
    they stand, the series of a twist of |omega| dt = 30 pass through terms of 1e11 on their way to a sum of order 1.) s = 0 leaves the plain
    series as it was."""
    B, n = X.shape[0], X.shape[1]
    norm = np.abs(X).sum(axis=2).max(axis=1)
    s = np.where(norm > 1.0, np.ceil(np.log2(np.maximum(norm, 1.0))), 0.0).astype(np.int64)
    x = X / (2.0 ** s)[:, None, None]
    E = _series(x, 1, 1.0)
    P = _series(x, 2, 1.0) if want_phi else None
    I = np.eye(n)
    for j in range(int(s.max()) if B else 0):
        on = s > j
        if want_phi:
            P[on] = 0.5 * np.einsum("bij,bjk->bik", I + E[on], P[on])
        E[on] = np.einsum("bij,bjk->bik", E[on], E[on])
    return E, P


def step_gradients(model, q_cur, qdot, foot_targets, dt, g, fk, imu=None, mode=capi.ROLLOUT_RUNNING):
    """wbc_step_vjp restated for B instances of ONE model: the gradient of a loss on q_new = update_state(q_cur, integrate(q_cur, qdot dt),
    foot_targets, imu) (mode ROLLOUT_WARMUP: q_new = integrate(q_cur, qdot dt)) from g = dL/d delta_new [B, 26], the tangent coordinates at
    q_new, with respect to q_cur (tangent coordinates at q_cur), qdot and foot_targets. fk follows tick_state_gradients' convention (fk(q) ->
    oMf, fk.joints(q) -> oMi, fk.jacobians(q) -> (J, Jcom)). The exponential and the right Jacobian of SE(3) are the plain power series of
    the 4 x 4 twist matrix and of -ad_xi, run to convergence on the argument halved until its norm is 1 or below, then doubled back
    (_exp_and_phi): held to a 50-digit reference up to |omega| dt = 30 (tests/test_step_se3_host.py). The IMU quaternion is held constant.
    Returns dict(d_q [B, 26], d_qdot [B, 26], d_foot_targets [B, 5, 3])."""
    q = np.asarray(q_cur, dtype=np.float64).reshape(-1, capi.Q_STRIDE)
    B, NVs, nv = q.shape[0], capi.V_STRIDE, model.nv
    x = np.asarray(qdot, dtype=np.float64).reshape(B, NVs)
    g = np.asarray(g, dtype=np.float64).reshape(B, NVs).copy()
    g[:, nv:] = 0.0
    xi = dt * x[:, 0:6]
    W, V = _hat(xi[:, 3:6]), _hat(xi[:, 0:3])
    X4 = np.zeros((B, 4, 4))
    X4[:, 0:3, 0:3], X4[:, 0:3, 3] = W, xi[:, 0:3]
    E4, _ = _exp_and_phi(X4, False)                                       # exp6(xi)
    Re, pe = E4[:, 0:3, 0:3], E4[:, 0:3, 3]
    c = g.copy()
    dft = np.zeros((B, 5, 3))
    if mode == capi.ROLLOUT_RUNNING:
        # the configuration the estimator's kinematics run at: [q_cur xyz, the quaternion q_new carries, the joints of q_next]
        cq = q.copy()
        for jd in model.data["joints"][2:model.njoints]:
            cq[:, jd["idx_q"]] = q[:, jd["idx_q"]] + dt * x[:, jd["idx_v"]]
        if imu is not None:
            cq[:, 3:7] = np.asarray(imu, dtype=np.float64).reshape(B, 4)
        else:
            Rn = np.einsum("bij,bjk->bik", _quat_to_R(q[:, 3:7]), Re)
            cq[:, 3:7] = _R_to_quat(Rn.reshape(B, 9))
        oMf, oMi = fk(cq), fk.joints(cq)
        J, _ = fk.jacobians(cq)
        Rb = oMi[:, 1, 0:9].reshape(B, 3, 3)
        pt = oMf[:, capi.FR_TRUNK, 9:12]
        BPA = sum(oMf[:, capi.FR_EE0 + e, 9:12] - pt for e in range(4)) / 4
        rbar = np.einsum("bji,bj->bi", Rb, BPA)
        Jbar = sum(frame_rows(model, J, oMf, capi.FR_EE0 + e, world=False)[:, 0:3] for e in range(4)) / 4
        gp = g[:, 0:3]
        dft[:, 0:4] = (np.einsum("bij,bj->bi", Rb, gp) / 4)[:, None, :]
        c[:, 6:] = g[:, 6:] - np.einsum("bik,bi->bk", Jbar[:, :, 6:], gp)
        if imu is None:
            c[:, 3:6] = g[:, 3:6] - np.cross(BPA, gp) - np.cross(rbar, np.einsum("bji,bj->bi", Rb, gp))
        else:
            c[:, 3:6] = 0.0
        c[:, 0:3] = 0.0
    c[:, nv:] = 0.0
    # ---- integrate: q_next = q (+) dt qdot
    Ad = np.zeros((B, 6, 6))                                             # Ad of exp(-xi)
    Ret = Re.transpose(0, 2, 1)
    Ad[:, 0:3, 0:3] = Ad[:, 3:6, 3:6] = Ret
    Ad[:, 0:3, 3:6] = -np.einsum("bij,bjk->bik", Ret, _hat(pe))
    ad = np.zeros((B, 6, 6))
    ad[:, 0:3, 0:3] = ad[:, 3:6, 3:6] = W
    ad[:, 0:3, 3:6] = V
    _, Jr = _exp_and_phi(-ad, True)                                       # sum_k (-ad)^k / (k + 1)!
    dq, dx = np.zeros((B, NVs)), np.zeros((B, NVs))
    dq[:, 0:6] = np.einsum("bji,bj->bi", Ad, c[:, 0:6])
    dx[:, 0:6] = dt * np.einsum("bji,bj->bi", Jr, c[:, 0:6])
    dq[:, 6:], dx[:, 6:] = c[:, 6:], dt * c[:, 6:]
    if mode == capi.ROLLOUT_RUNNING:
        dq[:, 0:3] = dx[:, 0:3] = 0.0                                     # (c_p = 0: exactly)
    return dict(d_q=dq, d_qdot=dx, d_foot_targets=dft)


# ---- the track scores as a loss (wbc_rollout_vjp_scored, include/wbc.h)
def score_seed_gradients(model, q_after, ee_target, trunk_target, fk, mask, g_err_sq_sum=None, g_err_final=None, g_err_max=None,
                         err_max_tick=None):
    """The cotangent of the track scores restated for B instances of ONE model. q_after [K, B, 27]: the state after every tick (q_(k+1));
    ee_target [K, B, 5, 3] / trunk_target [K, B, 3] (None without score bit 5): the targets tick k saw; fk as tick_state_gradients takes it
    (fk(q) -> oMf, fk.jacobians(q) -> (J, Jcom)); mask: the score mask (bit f: 0..4 the end effectors, 5 the trunk); g_err_* [n_scored, B]
    the cotangents of err_sq_sum, err_final and err_max, each optional; err_max_tick [n_scored, B] as the record call returned it.
    With d = FK_f(q_(k+1)) - target_f(k), e = |d|:  c = ((2 g_sq + [k == K - 1] g_fin / e) + [k == err_max_tick] g_max / e) d, the 1 / e
    terms taken as 0 where e == 0. Returns dict(g_q_trace [K, B, 26]: sum_f J_f' c_f, tangent at q_(k+1) — J_f the [:, :3] block of
    frame_rows(..., world=False); c [K, B, 6, 3]: the cotangent of d, 0 for an unscored frame (the target of tick k gets -c); e [K, B, 6])."""
    q_after = np.asarray(q_after, dtype=np.float64)
    K, B = q_after.shape[:2]
    frames = [f for f in range(capi.TARGET_TRUNK + 1) if (int(mask) >> f) & 1]
    take = lambda a: None if a is None else np.asarray(a, dtype=np.float64).reshape(len(frames), B)      # noqa: E731
    g_sq, g_fin, g_max = take(g_err_sq_sum), take(g_err_final), take(g_err_max)
    tick = None if err_max_tick is None else np.asarray(err_max_tick).reshape(len(frames), B)
    if g_max is not None and tick is None:
        raise ValueError("g_err_max needs err_max_tick")
    g = np.zeros((K, B, capi.V_STRIDE))
    c_all, e_all = np.zeros((K, B, capi.TARGET_TRUNK + 1, 3)), np.zeros((K, B, capi.TARGET_TRUNK + 1))
    for k in range(K):
        oMf = fk(q_after[k])
        J, _ = fk.jacobians(q_after[k])
        for i, f in enumerate(frames):
            role = capi.FR_TRUNK if f == capi.TARGET_TRUNK else capi.FR_EE0 + f
            tg = (np.asarray(trunk_target[k], dtype=np.float64).reshape(B, 3) if f == capi.TARGET_TRUNK
                  else np.asarray(ee_target[k], dtype=np.float64).reshape(B, capi.NEE, 3)[:, f])
            d = oMf[:, role, 9:12] - tg
            e = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            inv = np.divide(1.0, e, out=np.zeros(B), where=e > 0.0)
            coef = np.zeros(B) if g_sq is None else 2.0 * g_sq[i]
            if g_fin is not None and k == K - 1:
                coef = coef + np.where(e > 0.0, g_fin[i] * inv, 0.0)
            if g_max is not None:
                coef = coef + np.where((tick[i] == k) & (e > 0.0), g_max[i] * inv, 0.0)
            c = coef[:, None] * d
            Jf = frame_rows(model, J, oMf, role, world=False)[:, :3]
            g[k] += np.einsum("brk,br->bk", Jf, c)
            c_all[k, :, f], e_all[k, :, f] = c, e
    return dict(g_q_trace=g, c=c_all, e=e_all)


# ---- the constraint slack as a loss (wbc_state_slack_vjp / wbc_rollout_vjp_watched, include/wbc.h)
_SLACK_BLOCKS = ((0, 4), (4, 6), (6, 12))      # the components of families 0..2


def slack_gradients(model, cfg, q, trunk_box_center, fk, g_slack=None, g_components=None):
    """wbc_state_slack_vjp restated for B instances of ONE model: the cotangent of state_slack's outputs. q [B, 27], trunk_box_center [B, 4] or
    None, fk as tick_state_gradients takes it (fk(q) -> oMf, fk.com(q), fk.jacobians(q) -> (J, Jcom)); g_slack [B, 4] = dL/d slack and / or
    g_components [B, 12] = dL/d components. Component i of families 0..2 gets gamma_i = g_components[i] + g_slack[f] where i is the component
    state_slack selects for family f (the lowest code on a tie: a subgradient there); g_slack[3] goes to the DoF and side of the joint
    family's code. The first-order pieces are frame_rows' LOCAL_WORLD_ALIGNED rows of the FL / RR feet and the trunk frame and Jcom; the
    angles go through d angle_a = N_a . omega. Returns dict(d_q [B, 26] tangent at q, d_trunk_box_center [B, 4], which [B, 4] int32 —
    state_slack's —, grad_status [B] int32, gamma [B, 12]). A bad row (non-finite q or cotangent, non-finite box entry of a family with a
    non-zero cotangent) gives zero rows and GRAD_NONFINITE."""
    q = np.array(q, dtype=np.float64).reshape(-1, capi.Q_STRIDE)
    B = q.shape[0]
    if g_slack is None and g_components is None:
        raise ValueError("a cotangent is required (g_slack or g_components)")
    gs = np.zeros((B, capi.N_SLACK)) if g_slack is None else np.array(g_slack, dtype=np.float64).reshape(B, capi.N_SLACK)
    gc = np.zeros((B, capi.N_SLACK_COMPONENTS)) if g_components is None else np.array(g_components, dtype=np.float64).reshape(B, capi.N_SLACK_COMPONENTS)
    on1 = (gs[:, 1] != 0.0) | (gc[:, 4:6] != 0.0).any(axis=1)
    on2 = (gs[:, 2] != 0.0) | (gc[:, 6:12] != 0.0).any(axis=1)
    if trunk_box_center is None:
        if (on1 | on2).any():
            raise ValueError("trunk_box_center is required with a non-zero cotangent on a trunk family")
        c = np.full((B, 4), np.nan)
    else:
        c = np.asarray(trunk_box_center, dtype=np.float64).reshape(B, 4)
    st = state_slack(model, cfg, q, trunk_box_center, fk)
    which = st["which"]
    bad = ~np.isfinite(q[:, :model.nq]).all(axis=1) | ~np.isfinite(gs).all(axis=1) | ~np.isfinite(gc).all(axis=1)
    bad |= (on1 & ~np.isfinite(c[:, 0])) | (on2 & ~np.isfinite(c[:, 1:]).all(axis=1))
    neutral = np.zeros(capi.Q_STRIDE)
    neutral[6] = 1.0
    q[bad] = neutral
    gs, gc = np.where(bad[:, None], 0.0, gs), np.where(bad[:, None], 0.0, gc)
    gamma = gc.copy()
    rows = np.arange(B)
    for f, (lo, hi) in enumerate(_SLACK_BLOCKS):
        sel = which[:, f] >= 0
        gamma[rows[sel], lo + which[sel, f]] += gs[sel, f]
    oMf = fk(q)
    J, Jcom = fk.jacobians(q)
    JFL = frame_rows(model, J, oMf, capi.FR_EE0 + 1, world=False)
    JRR = frame_rows(model, J, oMf, capi.FR_EE0 + 2, world=False)
    JT = frame_rows(model, J, oMf, capi.FR_TRUNK, world=False)
    col = lambda v: v[:, None]      # noqa: E731
    dq = col(gamma[:, 1]) * JFL[:, 0] + col(gamma[:, 3]) * JFL[:, 1] - col(gamma[:, 0]) * JRR[:, 0] - col(gamma[:, 2]) * JRR[:, 1]
    dq = dq + col(gamma[:, 0] - gamma[:, 1]) * Jcom[:, 0] + col(gamma[:, 2] - gamma[:, 3]) * Jcom[:, 1]
    dq = dq + col(gamma[:, 4] - gamma[:, 5]) * JT[:, 2]
    # the three atan2 angles through dR = [omega] R: d angle_a = N_a . omega (R row-major: R[:, 3 i + j] = R_ij)
    R = oMf[:, capi.FR_TRUNK, 0:9]
    R00, R01, R02, R10, R11, R12, R20, R21, R22 = (R[:, i] for i in range(9))
    n0 = R21 * R21 + R22 * R22
    cxy = np.sqrt(n0)
    n1, n2 = R20 * R20 + n0, R00 * R00 + R10 * R10
    z = np.zeros(B)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = R20 / cxy
        N = [np.stack([R22 * R11 - R21 * R12, R21 * R02 - R22 * R01, z], axis=1) / col(n0),
             np.stack([-cxy * R10 + t1 * (R21 * R11 + R22 * R12), cxy * R00 - t1 * (R21 * R01 + R22 * R02), z], axis=1) / col(n1),
             np.stack([-R00 * R20, -R10 * R20, R00 * R00 + R10 * R10], axis=1) / col(n2)]
    ce = np.stack([gamma[:, 6 + 2 * a] - gamma[:, 7 + 2 * a] for a in range(3)], axis=1)
    for a in range(3):
        Na = np.where(col(ce[:, a]) != 0.0, N[a], 0.0)                    # (a zero cotangent takes no part, whatever the rotation)
        dq = dq + col(ce[:, a]) * np.einsum("bi,bik->bk", Na, JT[:, 3:6])
    code = which[:, 3]
    sel = (code >= 0) & (gs[:, 3] != 0.0)
    dq[rows[sel], code[sel] >> 1] += np.where(code[sel] & 1, -gs[sel, 3], gs[sel, 3])
    dq[:, model.nv:] = 0.0
    zf = float(cfg.trunk_box_z_frac)
    dbox = np.concatenate([col(-(1.0 - zf) * gamma[:, 4] + (1.0 + zf) * gamma[:, 5]), -ce], axis=1)
    dq[bad], dbox[bad] = 0.0, 0.0
    return dict(d_q=dq, d_trunk_box_center=dbox, which=which, grad_status=np.where(bad, capi.GRAD_NONFINITE, capi.GRAD_OK).astype(np.int32),
                gamma=gamma)


def watch_seed_gradients(model, cfg, q_after, trunk_box_center, fk, mask, g_slack_min=None, g_slack_final=None, g_trace=None,
                         slack_min_tick=None):
    """The cotangent of wbc_rollout_watch's results restated for B instances of ONE model. q_after [K, B, 27]: the state after every tick
    (q_(k+1)); mask: the watched families (rows of the arrays below in increasing family order); g_slack_min, g_slack_final [n_w, B], g_trace
    [K, n_w, B], each optional; slack_min_tick [n_w, B] as the record call returned it. On tick k family f carries
    g_trace[k] + [k == K - 1] g_slack_final + [k == slack_min_tick] g_slack_min, applied through slack_gradients at q_(k+1). Returns
    dict(g_q_trace [K, B, 26] tangent at q_(k+1), d_trunk_box_center [B, 4]: the sum over the ticks from the last, g_slack [K, B, 4])."""
    q_after = np.asarray(q_after, dtype=np.float64)
    K, B = q_after.shape[:2]
    fams = [f for f in range(capi.N_SLACK) if (int(mask) >> f) & 1]
    take = lambda a, lead: None if a is None else np.asarray(a, dtype=np.float64).reshape(lead + (len(fams), B))      # noqa: E731
    g_min, g_fin, g_tr = take(g_slack_min, ()), take(g_slack_final, ()), take(g_trace, (K,))
    tick = None if slack_min_tick is None else np.asarray(slack_min_tick).reshape(len(fams), B)
    if g_min is not None and tick is None:
        raise ValueError("g_slack_min needs slack_min_tick")
    g, dbox, gs_all = np.zeros((K, B, capi.V_STRIDE)), np.zeros((B, 4)), np.zeros((K, B, capi.N_SLACK))
    for k in range(K - 1, -1, -1):
        gs = np.zeros((B, capi.N_SLACK))
        for i, f in enumerate(fams):
            x = np.zeros(B) if g_tr is None else g_tr[k, i]
            if g_fin is not None and k == K - 1:
                x = x + g_fin[i]
            if g_min is not None:
                x = x + np.where(tick[i] == k, g_min[i], 0.0)
            gs[:, f] = x
        r = slack_gradients(model, cfg, q_after[k], trunk_box_center, fk, g_slack=gs)
        g[k], gs_all[k] = r["d_q"], gs
        dbox = dbox + r["d_trunk_box_center"]
    return dict(g_q_trace=g, d_trunk_box_center=dbox, g_slack=gs_all)


# ---- K ticks as one reverse sweep (wbc_rollout_vjp, include/wbc.h)
_ROLLOUT_SUMS = ("d_task_params", "d_com_target", "d_com_target_vel", "d_posture_u")


def rollout_gradients(model, cfg, ticks_in, x, dt, fk, assemble, g_q_final=None, g_qdot_last=None, g_q_trace=None, task_params=None, imu=None,
                      mode=capi.ROLLOUT_RUNNING, status=None, working_set=None, tracks=None, score_seed=None, watch_seed=None):
    """wbc_rollout_vjp restated for B instances of ONE model over step_gradients, qp_certificate, tick_gradients and tick_state_gradients,
    tick by tick from the last. ticks_in: K dicts, the inputs tick k SAW (q, the targets as running sums, the previous rotations); x [K, B, 26]:
    the ticks' qdot; assemble(inputs) -> dict(A, b, C, Clb, Cub, lb, ub) of a tick's problem (a model with nv < 26 gets unit rows on its padded
    columns here). Seeds in tangent coordinates: g_q_final [B, 26] at q_K, g_qdot_last [B, 26], g_q_trace [K, B, 26] at the state after each
    tick. status [K, B] / working_set [K, B, 2]: the ticks' own, or None (every tick solved; the active sets read off x).
    Target bookkeeping (E ee_target, P prev_ee_target, s the step; forward E' = E + s, P' = E where the task is on, else P), with Ebar, Pbar
    the cotangents of E', P', a = tick.d_ee_target + step.d_foot_targets, p = tick.d_prev_ee_target:
        d_step += Ebar;  Ebar <- Ebar + a + on Pbar;  Pbar <- p + (1 - on) Pbar          (the trunk pair: the same under task_trunk)
    A tick that is unsolved, uncertified or non-finite for an instance gives that instance zero from the tick's layer (ticks_dropped += 1);
    the step's part flows on. Returns dict(d_q0 (tangent at q_0), d_task_params, d_ee_target, d_prev_ee_target, d_trunk_target,
    d_prev_trunk_target, d_com_target, d_com_target_vel, d_posture_u, d_trunk_box_center, d_ee_target_step, d_trunk_target_step,
    ticks_dropped [B], sens_max [B]: the largest |sens_x| entry over the ticks).
    tracks (wbc_rollout_vjp_tracks): a list of dicts(target: 0..4 or 5 / "trunk", points, n_points, du, kind, tangents) as track_targets takes
    them. A followed target is eval(k * du) on every tick, so its whole cotangent e_k = a + on Pbar goes into the track and nothing is
    carried (Ebar of a followed row is 0 in front of every tick; Pbar updates as above). The dict then also holds tracks = [dict(d_points,
    d_tangents, d_du), ...] from track_target_gradients; the followed rows of d_ee_target / d_trunk_target are 0 and the steps mean nothing.
    score_seed (wbc_rollout_vjp_scored): dict(mask, q_final [B, 27], g_err_sq_sum, g_err_final, g_err_max, err_max_tick) — the cotangents of
    the track scores through score_seed_gradients: its g_q_trace rows join the state seed where g_q_trace enters, and -c_k joins the
    cotangent of tick k's targets BEHIND that tick's bookkeeping (so the step sums see the later ticks' alone) and in front of the tracks.
    watch_seed (wbc_rollout_vjp_watched): dict(mask, q_final [B, 27], g_slack_min, g_slack_final, g_trace, slack_min_tick) — the cotangents of
    the watch's results through watch_seed_gradients at the states after the ticks, with ticks_in[0]["trunk_box_center"] as the box: its
    g_q_trace rows join the state seed where g_q_trace enters, its box term joins d_trunk_box_center."""
    K = len(ticks_in)
    w_box = None
    if watch_seed is not None:
        q_after = np.stack([np.asarray(ticks_in[k + 1]["q"], dtype=np.float64) for k in range(K - 1)] + [np.asarray(watch_seed["q_final"], dtype=np.float64)])
        wg = watch_seed_gradients(model, cfg, q_after, ticks_in[0].get("trunk_box_center"), fk, watch_seed["mask"], watch_seed.get("g_slack_min"),
                                  watch_seed.get("g_slack_final"), watch_seed.get("g_trace"), watch_seed.get("slack_min_tick"))
        g_q_trace = wg["g_q_trace"] if g_q_trace is None else np.asarray(g_q_trace, dtype=np.float64).reshape(wg["g_q_trace"].shape) + wg["g_q_trace"]
        w_box = wg["d_trunk_box_center"]
    sc_c = None
    if score_seed is not None:
        q_after = np.stack([np.asarray(ticks_in[k + 1]["q"], dtype=np.float64) for k in range(K - 1)] + [np.asarray(score_seed["q_final"], dtype=np.float64)])
        want_t = (int(score_seed["mask"]) >> capi.TARGET_TRUNK) & 1
        ss = score_seed_gradients(model, q_after, [t["ee_target"] for t in ticks_in], [t["trunk_target"] for t in ticks_in] if want_t else None, fk,
                                  score_seed["mask"], score_seed.get("g_err_sq_sum"), score_seed.get("g_err_final"), score_seed.get("g_err_max"),
                                  score_seed.get("err_max_tick"))
        g_q_trace = ss["g_q_trace"] if g_q_trace is None else np.asarray(g_q_trace, dtype=np.float64).reshape(ss["g_q_trace"].shape) + ss["g_q_trace"]
        sc_c = ss["c"]
    followed = [capi.TARGET_TRUNK if t["target"] == "trunk" else int(t["target"]) for t in (tracks or [])]
    e_tracks = [np.zeros((K, np.asarray(x).reshape(K, -1, capi.V_STRIDE).shape[1], 3)) for _ in followed]
    x = np.asarray(x, dtype=np.float64).reshape(K, -1, capi.V_STRIDE)
    B, NVs, nv = x.shape[1], capi.V_STRIDE, model.nv
    on = np.array([bool(cfg.task_ee[e]) for e in range(capi.NEE)])[None, :, None]
    on_t = bool(cfg.task_trunk)
    g = np.zeros((B, NVs)) if g_q_final is None else np.array(g_q_final, dtype=np.float64).reshape(B, NVs)
    if g_q_trace is not None:
        g_q_trace = np.asarray(g_q_trace, dtype=np.float64).reshape(K, B, NVs)
        g = g + g_q_trace[K - 1]
    Eb, Pb, TEb, TPb = np.zeros((B, 5, 3)), np.zeros((B, 5, 3)), np.zeros((B, 3)), np.zeros((B, 3))
    d_es, d_ts = np.zeros((B, 5, 3)), np.zeros((B, 3))
    acc = dict(d_task_params=np.zeros((B, capi.TASK_PARAMS_DOUBLES)), d_com_target=np.zeros((B, 3)), d_com_target_vel=np.zeros((B, 3)),
               d_posture_u=np.zeros((B, NVs)), d_trunk_box_center=np.zeros((B, 4)))
    dropped, sens_max = np.zeros(B, dtype=np.int32), np.zeros(B)
    for k in range(K - 1, -1, -1):
        d = ticks_in[k]
        sg = step_gradients(model, d["q"], x[k], d["ee_target"], dt, g, fk, imu=imu, mode=mode)
        v = sg["d_qdot"]
        if k == K - 1 and g_qdot_last is not None:
            v = v + np.asarray(g_qdot_last, dtype=np.float64).reshape(B, NVs)
        a = assemble(d)
        A, b = np.asarray(a["A"], dtype=np.float64), np.asarray(a["b"], dtype=np.float64)
        if nv < NVs:
            A = np.concatenate([A, np.broadcast_to(np.eye(NVs)[nv:], (B, NVs - nv, NVs))], axis=1)
            b = np.concatenate([b, np.zeros((B, NVs - nv))], axis=1)
        rows = a["C"].shape[1] > 0
        cert = [qp_certificate(x[k][i], A=A[i], b=b[i], C_=a["C"][i] if rows else None, lb=a["lb"][i], ub=a["ub"][i],
                               Clb=a["Clb"][i] if rows else None, Cub=a["Cub"][i] if rows else None,
                               status=None if status is None else status[k][i], working_set=None if working_set is None else working_set[k][i],
                               v=v[i]) for i in range(B)]
        st = lambda name: np.stack([c[name] for c in cert])      # noqa: E731
        ok = np.array([c["cert_status"] == capi.CERT_OK for c in cert]) & np.isfinite(d["q"]).all(axis=1) & np.isfinite(x[k]).all(axis=1)
        u = st("sens_x")
        sens_max = np.maximum(sens_max, np.abs(u).max(axis=1))
        res = tick_state_gradients(model, cfg, d, x[k], u, dt, fk, st("sens_bounds"), st("sens_rows"), st("y_rows"), task_params=task_params,
                                   working_set=None if working_set is None else working_set[k])
        tg = tick_gradients(model, cfg, d, x[k], u, dt, fk, task_params)
        take = lambda t: np.where(ok.reshape((B,) + (1,) * (t.ndim - 1)), t, 0.0)      # noqa: E731
        dropped += ~ok
        g = sg["d_q"] + take(res["d_q"])
        if k > 0 and g_q_trace is not None:
            g = g + g_q_trace[k - 1]
        for name in _ROLLOUT_SUMS:
            acc[name] = acc[name] + take(tg[name])
        acc["d_trunk_box_center"] = acc["d_trunk_box_center"] + take(res["d_trunk_box_center"])
        a_k, p_k = take(tg["d_ee_target"]) + sg["d_foot_targets"], take(tg["d_prev_ee_target"])
        d_es = d_es + Eb
        Eb, Pb = Eb + a_k + np.where(on, Pb, 0.0), p_k + np.where(on, 0.0, Pb)
        d_ts = d_ts + TEb
        TEb, TPb = TEb + take(tg["d_trunk_target"]) + (TPb if on_t else 0.0), take(tg["d_prev_trunk_target"]) + (0.0 if on_t else TPb)
        if sc_c is not None:                   # the scores' own dependence on the targets of tick k
            Eb = Eb - sc_c[k][:, :capi.NEE]
            TEb = TEb - sc_c[k][:, capi.TARGET_TRUNK]
        for j, f in enumerate(followed):       # the followed rows: into the track, nothing carried
            if f == capi.TARGET_TRUNK:
                e_tracks[j][k] = TEb
                TEb = np.zeros((B, 3))
            else:
                e_tracks[j][k] = Eb[:, f]
                Eb[:, f] = 0.0
    if w_box is not None:
        acc["d_trunk_box_center"] = acc["d_trunk_box_center"] + w_box
    if tracks:
        names = ("d_points", "d_tangents", "d_du")
        acc["tracks"] = [dict(zip(names, track_target_gradients(t["points"], t.get("n_points"), t.get("du", 0.002), K, t.get("kind", "linear"),
                                                                 t.get("tangents"), e_tracks[j]))) for j, t in enumerate(tracks)]
    return dict(acc, d_q0=g, d_ee_target=Eb, d_prev_ee_target=Pb, d_trunk_target=TEb, d_prev_trunk_target=TPb, d_ee_target_step=d_es,
                d_trunk_target_step=d_ts, ticks_dropped=dropped, sens_max=sens_max)
