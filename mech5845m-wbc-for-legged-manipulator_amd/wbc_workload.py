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
