"""Inputs that reach the SE(3) terms of the state step's VJP, and their 50-digit references (se3_reference.py), built once per process.
Shared by test_step_se3_host.py and test_gpu_step_se3.py.

step_common.step_problem draws the rates from N(0, 0.5): the base translation of a step is |v| = dt |qdot_lin| = 1e-3, and the coefficients c2,
c3 of the coupling block enter the outputs only through Q' c_p, which scales with |v|. Here |v| is 1e-3, 1 and 30, along omega, across it and
in a random direction, |omega| dt climbs a ladder from 0 to 30 that brackets integrate_ff's 1e-4 switch and the kernel's own at 1, and at
dt = 1 (xi = qdot exactly) rows sit one ulp either side of t^2 = 1.

WARMUP rows: 13 |omega| dt x 3 |v| (the direction of v cycles so that every |omega| dt and every |v| meets all three), the zero twist and a pure
rotation: 41; at dt = 1 also 6 seam rows x 3 |v|: 59. RUNNING rows (translation does not enter): the ladder x 3 models at |v| = 1e-3, three
poses per model: 39; at dt = 1 also the seam rows once per model: 57. The single-model handle runs every WARMUP row (no kinematics there)
and the a1_wx200 rows of the RUNNING sets (13 and 19). No count is a multiple of 4, the kernel's instances per wavefront."""
import functools
import math
from fractions import Fraction

import numpy as np

import se3_reference as s3
import wbc_model
import wbc_workload

MODELS = ("a1_wx200", "a1_px100_pin_ver", "laikago_vx300")           # step_common.MODELS: the three-model handle runs the ROT variant
LADDER = (0.0, 1e-9, 1e-5, 0.99e-4, 1.01e-4, 1e-3, 3e-2, 0.3, 2.0, math.pi, 2 * math.pi, 10.0, 30.0)
VS = (1e-3, 1.0, 30.0)
DTS = (0.002, 1.0)
DIRS = ("parallel", "perpendicular", "random")
POSES = 3
BLOCKS = {"d_q lin": ("d_q", slice(0, 3)), "d_q ang": ("d_q", slice(3, 6)), "d_q joints": ("d_q", slice(6, 26)),
          "d_qdot lin": ("d_qdot", slice(0, 3)), "d_qdot ang": ("d_qdot", slice(3, 6)), "d_qdot joints": ("d_qdot", slice(6, 26)),
          "d_foot_targets": ("d_foot_targets", slice(None))}


@functools.lru_cache(maxsize=None)
def model(name):
    return wbc_model.load_model(name)


def _fma(a, b, c):
    """a b + c rounded once (float(Fraction) rounds to nearest even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def norm2_all_ways(w):
    """w[0] w[0] + w[1] w[1] + w[2] w[2] as the kernel writes it, in that order, every way a compiler may contract it into fused
    multiply-adds: the plain sum of rounded squares and the five contractions of its two additions"""
    a, b, c = (float(x) for x in w)
    inner = (a * a + b * b, _fma(b, b, a * a), _fma(a, a, b * b))
    return tuple(x + c * c for x in inner) + tuple(_fma(c, c, x) for x in inner)


@functools.lru_cache(maxsize=None)
def seam_rows():
    """omega at dt = 1 around t^2 = 1: one ulp either side on an axis, the point itself on two axes, and an off-axis pair, neighbours in their
    last component, whose w . w falls on opposite sides of 1.0 however it is contracted -> [6, 3]; rows (0, 2) and (3, 4) are the pairs"""
    lo = np.array([0.48, 0.6, 0.64])
    while not all(x < 1.0 for x in norm2_all_ways(lo)):
        lo[2] = np.nextafter(lo[2], 0.0)
    hi = lo.copy()
    for _ in range(8):
        hi[2] = np.nextafter(hi[2], 2.0)
        if all(x >= 1.0 for x in norm2_all_ways(hi)):
            break
    rows = np.array([[np.nextafter(1.0, 0.0), 0, 0], [1.0, 0, 0], [np.nextafter(1.0, 2.0), 0, 0], lo, hi, [0, 0, -1.0]])
    rows.setflags(write=False)
    return rows


SEAM_PAIRS = ((0, 2), (3, 4))


def _unit(rng):
    u = rng.normal(0, 1.0, 3)
    return u / np.linalg.norm(u)


def _v_dir(kind, u, rng):
    """a unit vector along u, across u, or anywhere"""
    r = _unit(rng)
    if kind == "parallel":
        return u.copy()
    if kind == "perpendicular":
        r = r - (r @ u) * u
        return r / np.linalg.norm(r)
    return r


def _twists(dt, running):
    """-> (xi [n, 6] = dt qdot[0:6] as intended (v, omega dt), labels [n], seam groups: lists of the six row indices of seam_rows(), one
    group per model; the rows of a group differ in omega alone)"""
    rng = np.random.default_rng(20 + int(running))
    xi, labels = [], []
    for it, t in enumerate(LADDER):
        for iv, vm in enumerate((VS[0],) * 3 if running else VS):
            if dt == 1.0 and t == math.pi:
                u = np.array([0.0, 1.0, 0.0])                              # (the nearest double to pi itself)
            else:
                u = _unit(rng)
            kind = DIRS[(it + iv) % 3]
            xi.append(np.concatenate([vm * _v_dir(kind, u, rng), t * u]))
            labels.append("t %g, |v| %g %s" % (t, vm, kind))
    groups = []
    if not running:
        xi += [np.zeros(6), np.concatenate([np.zeros(3), 2.0 * _unit(rng)])]
        labels += ["zero twist", "t 2, v = 0"]
    if dt == 1.0:
        for iv, vm in enumerate((VS[0],) * 3 if running else VS):
            v = vm * _v_dir(DIRS[iv], np.array([1.0, 0.0, 0.0]), rng)
            groups.append(list(range(len(xi), len(xi) + len(seam_rows()))))
            for i, w in enumerate(seam_rows()):
                xi.append(np.concatenate([v, w]))
                labels.append("seam %d, |v| %g %s to x" % (i, vm, DIRS[iv]))
    return np.array(xi), labels, groups


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _mid(B, groups):
    """models interleaved row by row; a seam group is of one model, group k of model k"""
    mid = (np.arange(B) % 3).astype(np.int32)
    for k, grp in enumerate(groups):
        mid[grp] = k
    return mid


def _inputs(names, mid, xi, dt, seed, running, imu, groups):
    B = len(xi)
    rng = np.random.default_rng(seed)
    q, x = np.zeros((B, 27)), np.zeros((B, 26))
    g = rng.normal(0, 1.0, (B, 26))                                             # dense; columns >= nv carry values the kernel must not read
    ft = rng.normal(0, 0.3, (B, 5, 3))
    for i, n in enumerate(names):
        m = model(n)
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        k = int(sel.sum())
        poses = wbc_workload.sample_q(m, POSES, rng)
        q[sel] = poses[np.arange(k) % POSES]
        x[sel, 6:m.nv] = rng.normal(0, 0.5, (k, m.nv - 6)) * (0.002 / dt)       # the joints step as they do at 2 ms
    x[:, 0:6] = xi / dt
    if dt == 1.0:
        assert np.array_equal(dt * x[:, 0:6], xi)
    iq = None
    if imu:
        iq = q[:, 3:7] + rng.normal(0, 0.05, (B, 4))
        iq /= np.linalg.norm(iq, axis=1, keepdims=True)
    for grp in groups:                                                          # the rows of a seam group differ in omega alone
        for a in (q, x[:, 6:], g, ft) + (() if iq is None else (iq,)):
            a[grp] = a[grp[0]]
    return dict(q=q, qdot=x, foot_targets=ft, imu=iq, g=g)


@functools.lru_cache(maxsize=None)
def warmup_base(dt):
    """the base block of the WARMUP reference, which no model enters: (Ad_{exp(-xi)}' g6, dt Jr(xi)' g6) per row of the set -> ([n, 6], [n, 6]).
    Rates and g are those of warmup_case (same seed, same draws for the base block)."""
    p = warmup_case("mixed", dt, _with_ref=False)
    a, j = zip(*[s3.base_vjp(p["qdot"][b, 0:6], dt, p["g"][b, 0:6]) for b in range(len(p["q"]))])
    return np.array(a), np.array(j)


@functools.lru_cache(maxsize=None)
def warmup_case(handle, dt, _with_ref=True):
    """handle "wx200" (one model, ROT off) or "mixed" (three models interleaved, ROT on) -> dict(names, mid, q, qdot, foot_targets, imu, g,
    labels, groups (_twists), nv [B], ref (d_q, d_qdot, d_foot_targets))"""
    xi, labels, groups = _twists(dt, False)
    B = len(xi)
    names = MODELS if handle == "mixed" else MODELS[:1]
    mid = _mid(B, groups) if handle == "mixed" else None
    p = _inputs(names, mid, xi, dt, 31, False, False, groups)                   # (the base block's draws do not depend on the handle)
    p.update(names=names, mid=mid, labels=labels, groups=groups, nv=np.array([model(names[k]).nv for k in (np.zeros(B, int) if mid is None else mid)]))
    if _with_ref:
        a, j = warmup_base(dt)
        assert np.array_equal(p["qdot"][:, 0:6], warmup_case("mixed", dt, _with_ref=False)["qdot"][:, 0:6])
        assert np.array_equal(p["g"][:, 0:6], warmup_case("mixed", dt, _with_ref=False)["g"][:, 0:6])
        own = np.arange(26)[None, :] < p["nv"][:, None]
        dq, dx = np.where(own, p["g"], 0.0), np.where(own, dt * p["g"], 0.0)     # the joints pass through (dt g: one rounding of an exact product)
        dq[:, 0:6], dx[:, 0:6] = a, j
        p["ref"] = _freeze(dict(d_q=dq, d_qdot=dx, d_foot_targets=np.zeros((B, 5, 3))))
    return _freeze(p)


@functools.lru_cache(maxsize=None)
def running_case(handle, dt, imu):
    """as warmup_case, mode RUNNING with or without an IMU quaternion. The single-model handle runs the a1_wx200 rows of the mixed set."""
    xi, labels, groups = _twists(dt, True)
    B = len(xi)
    mid = _mid(B, groups)
    if handle == "wx200":
        full = running_case("mixed", dt, imu)
        sel = np.flatnonzero(mid == 0)
        p = {k: (None if full[k] is None else full[k][sel]) for k in ("q", "qdot", "foot_targets", "imu", "g", "nv")}
        p.update(names=MODELS[:1], mid=None, labels=[labels[i] for i in sel], ref={k: v[sel] for k, v in full["ref"].items()},
                 groups=[[int(np.searchsorted(sel, i)) for i in grp] for grp in groups[:1]])
        return _freeze(p)
    p = _inputs(MODELS, mid, xi, dt, 37 + int(imu), True, imu, groups)
    p.update(names=MODELS, mid=mid, labels=labels, groups=groups, nv=np.array([model(MODELS[k]).nv for k in mid]))
    rows = [s3.step_vjp(model(MODELS[mid[b]]).data, p["q"][b], p["qdot"][b], p["foot_targets"][b], dt, p["g"][b],
                        None if p["imu"] is None else p["imu"][b], s3.RUNNING) for b in range(B)]
    p["ref"] = _freeze({k: np.stack([r[k] for r in rows]) for k in rows[0]})
    return _freeze(p)


def block_errors(got, ref):
    """per block of BLOCKS and per row: max|got - ref| / max(1, max|ref|) over the block's entries of that row -> {block: [B]}"""
    out = {}
    for name, (key, sl) in BLOCKS.items():
        a, r = np.asarray(got[key])[:, sl].reshape(len(ref[key]), -1), ref[key][:, sl].reshape(len(ref[key]), -1)
        out[name] = np.abs(a - r).max(axis=1) / np.maximum(1.0, np.abs(r).max(axis=1))
    return out
