"""The far-pose cases shared by test_pose_envelope_host.py (the oracle alone, no GPU) and test_gpu_pose_envelope.py.

Every problem is built once (inputs, the oracle's answer, the 50-digit reference's kinematics) and handed out read-only."""
import functools

import numpy as np

import common
import kin_reference
import oracle
import wbc_capi as capi
import wbc_model

DT = 0.002
QDOT_TOL = 1e-5          # test_gpu_parity.py: the bound of BASELINE.json for q̇
REFINED_TOL = 1e-7       # test_gpu_parity.py: a path with the refinement on, against the oracle (which refines too)
B0 = 67                  # test_gpu_device_inplace.py: 16 full groups of four + 3, 22 of three + 1, past one 64-lane block
SEED = 7
T = 0                    # MODE_TICK
GEN = {"packed_kernel": 0, "sim3_kernel": 0}
PO = {"packed_orth": 2}

# name -> models, configuration, handle options, the row that must run (family + template flags as "last_tick_variant" reports them, or the
# path alone for the compact kernel, which has no variant table), the tolerance of the path's existing parity test
# (test_gpu_device_inplace.run_case), recipe switches. One case per code path that restates the Euler extraction or the integrate tail.
# f_lo: the lower end of edge_trunk_box's f where the default 0.97 leaves fewer than 40 % of the instances with an active angle row (the
# observability condition of test_pose_envelope_host.py: a condition on the inputs, met by the recipe, never by the threshold).
TICK_CASES = {
    "c3": dict(models=("wx200",), cfg="c3", opts={}, row=("sim3p", (0, 0, 0, 0, 0)), tol=REFINED_TOL),
    "c3_trunk_task": dict(models=("wx200",), cfg="c3_trunk_task", opts={}, row=("sim3p", (0, 1, 0, 0, 0)), tol=QDOT_TOL, f_lo=0.99),
    "c3_custom": dict(models=("wx200",), cfg="c3_custom", opts={}, row=("sim3p", (0, 0, 1, 0, 0)), tol=QDOT_TOL, qcon=True),
    "rot_c3": dict(models=("rot",), cfg="c3", opts={}, row=("sim3p", (0, 0, 0, 1, 0)), tol=QDOT_TOL, f_lo=0.99),
    "c3_tp": dict(models=("wx200",), cfg="c3", opts={}, row=("sim3p", (0, 0, 0, 0, 1)), tol=QDOT_TOL, tp=True),
    # the compact kernel does not refine: with the refinement on, packed_kernel = 0 alone selects the general kernel (select_tick_path)
    "c3_compact": dict(models=("wx200",), cfg="c3", opts={"packed_kernel": 0, "refine": 0}, row=None, path=1, tol=QDOT_TOL),
    "c3_general": dict(models=("wx200",), cfg="c3", opts=GEN, row=("general", (T, 0, 0, 0, 0)), tol=QDOT_TOL),
    "c2_orthp": dict(models=("wx200",), cfg="c2", opts=PO, row=("orthp", (0, 0, 0, 0)), tol=QDOT_TOL),
    # the CoM box's bounds are the RR and FL foot positions on WORLD axes (the reference's formula): under yaw or tilt lower > upper, so the case that
    # must solve draws its attitudes from common.NARROW (translation, quaternion flips and edge angles as everywhere)
    "everything_orthp": dict(models=("wx200",), cfg="everything", opts=PO, row=("orthp", (1, 0, 0, 0)), tol=QDOT_TOL, narrow=True, with_rot=True),
    "full": dict(models=("wx200",), cfg="full", opts={}, row=("boxp", (0, 0, 0)), tol=QDOT_TOL, with_rot=True),
    "laikago_c3": dict(models=("laikago",), cfg="c3", opts={}, row=("general", (T, 0, 0, 1, 0)), tol=QDOT_TOL, f_lo=0.99),
    "mixed_c3": dict(models=("wx200", "px100"), cfg="c3", opts={}, row=("sim3p", (0, 0, 0, 0, 0)), tol=QDOT_TOL),
}
# ... and `everything` on the full far_q attitudes, where the CoM box is infeasible almost everywhere: statuses, q̇ = 0, empty working sets
INFEASIBLE_CASE = dict(models=("wx200",), cfg="everything", opts=PO, row=("orthp", (1, 0, 0, 0)), tol=QDOT_TOL, with_rot=True)
LAST_PATH = {"general": 0, "sim3p": 2, "orthp": 3, "boxp": 4}
FK_MODELS = ("wx200", "px100", "laikago", "rot")


def key_of(flags):
    k = 0
    for a in tuple(flags) + (0,) * (5 - len(flags)):
        k = k * 256 + int(a)
    return k


@functools.lru_cache(maxsize=None)
def model(name):
    if name == "rot":
        from test_gpu_wave_order import _rotated_wx200
        return _rotated_wx200()
    return wbc_model.load_model({"wx200": "a1_wx200", "px100": "a1_px100_pin_ver", "laikago": "laikago_vx300"}[name])


def _freeze(*dicts):
    for d in dicts:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)


def gain_rows(cfg, B, seed):
    """per-instance task rows that differ from the configuration's in the GAINS only (x log-uniform [0.5, 2]): H and cond(H) stay the
    configuration's, so the parity tolerances hold as they are (test_gpu_device_inplace._gain_rows)"""
    rng = np.random.default_rng(seed)
    rows = wbc_model.task_params(cfg, B)
    sl = wbc_model.TASK_PARAMS_SLICES
    for f in ("ee_gain", "trunk_gain", "com_gain"):
        rows[:, sl[f]] *= np.exp(rng.uniform(np.log(0.5), np.log(2.0), (B, sl[f].stop - sl[f].start)))
    return rows


def merge(parts, mid):
    d = {}
    for k in parts[0]:
        v = parts[0][k].copy()
        for i in range(1, len(parts)):
            v[mid == i] = parts[i][k][mid == i]
        d[k] = v
    d["model_id"] = mid
    return d


def build_problem(case, B=B0, seed=SEED):
    """-> dict(models, cfgs, d, mid, rows, ref (oracle.tick, cold), oracle_args, q_int (the configuration the tick integrates from))"""
    models = [model(n) for n in case["models"]]
    cfgs = [common.config(case["cfg"], m) for m in models]
    kw = dict(narrow=case.get("narrow", False), with_rot=case.get("with_rot", False), f_lo=case.get("f_lo", 0.97))
    seed = case.get("seed", seed)
    mid = None
    if len(models) == 1:
        d = common.far_tick_inputs(models[0], cfgs[0], B, seed, **kw)
    else:
        mid = (np.arange(B) % len(models)).astype(np.int32)
        d = merge([common.far_tick_inputs(m, c, B, seed + i, **kw) for i, (m, c) in enumerate(zip(models, cfgs))], mid)
    if case.get("qcon"):     # test_tick_custom_posture_and_q_con
        rng = np.random.default_rng(seed + 4)
        d["posture_u"] = rng.normal(size=(B, 26))
        d["q_con"] = d["q"].copy()
        d["q_con"][:, 7:] += rng.normal(0, 1e-3, (B, 20))
    rows = None
    ms, cs, dd = models, cfgs, d
    if case.get("tp"):
        rows = gain_rows(cfgs[0], B, seed + 7)
        ms, cs, pid = common.per_instance_configs(models, cfgs, mid, rows)
        dd = dict(d, model_id=pid)
    ref = oracle.tick(ms, cs, dd, DT, B, nthreads=8)
    _freeze(d, ref)
    return dict(models=models, cfgs=cfgs, d=d, mid=mid, rows=rows, ref=ref, oracle_args=(ms, cs, dd), q_int=d.get("q_con", d["q"]), B=B, case=case)


@functools.lru_cache(maxsize=None)
def tick_problem(name):
    return build_problem(INFEASIBLE_CASE if name == "everything_far" else TICK_CASES[name])


def shifted_reference(p, shift):
    """the oracle's answer with the three angle centres of the trunk box moved by `shift` rad"""
    ms, cs, dd = p["oracle_args"]
    box = dd["trunk_box_center"].copy()
    box[:, 1:] += shift
    return oracle.tick(ms, cs, dict(dd, trunk_box_center=box), DT, p["B"], nthreads=8)


def observability(p, shift=1e-6, moved=1e-5):
    """(share of the instances the oracle solves, share of those whose q̇ moves by more than `moved` when the angle centres move by `shift`)"""
    ref = p["ref"]
    ok = ref["status"] == 0
    if not p["cfgs"][0].con_trunk:
        return ok.mean(), None
    sh = shifted_reference(p, shift)
    both = ok & (sh["status"] == 0)
    dq = np.abs(sh["qdot"] - ref["qdot"]).max(axis=1)
    return ok.mean(), float(((dq > moved) & both).sum()) / max(1, int(ok.sum()))


def leg_block_ratio(a):
    """min over the four stance feet of |det K| / (sum |K_ij|)^3 (test_gpu_sim3p_cold_paths.py)"""
    r = np.full(a["C"].shape[0], np.inf)
    for f, d0 in enumerate((9, 6, 15, 12)):
        K = a["C"][:, 4 + 3 * f:7 + 3 * f, d0:d0 + 3]
        r = np.minimum(r, np.abs(np.linalg.det(K)) / np.abs(K).sum(axis=(1, 2)) ** 3)
    return r


# ---- kinematics against the 50-digit reference
FK_POSES = 24
KIN_KEYS = ("oMi", "oMf", "J", "com", "Jcom")


@functools.lru_cache(maxsize=None)
def fk_problem(name):
    """-> (model, q [24, 27] of far_fk_q, reference: dict of stacked arrays incl. Jf [24, nf, 6, 26] and euler [24, 3])"""
    m = model(name)
    q = common.far_fk_q(m, FK_POSES, np.random.default_rng(40 + FK_MODELS.index(name)))
    per = [kin_reference.fk(m.data, q[b]) for b in range(FK_POSES)]
    ref = {k: np.stack([r[k] for r in per]) for k in per[0]}
    q.setflags(write=False)
    _freeze(ref)
    return m, q, ref


def kin_tol(ref):
    """the suite's kinematic tolerance: 1e-12 x max(1, |ref|max)"""
    return 1e-12 * max(1.0, float(np.abs(ref).max()))


def pad(a, n, axis=1):
    """rows beyond an instance's own model are zero (WbcFkOut in a mixed batch)"""
    if a.shape[axis] == n:
        return a
    w = [(0, 0)] * a.ndim
    w[axis] = (0, n - a.shape[axis])
    return np.pad(a, w)
