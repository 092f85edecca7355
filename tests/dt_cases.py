"""Time steps other than 2 ms: the steps, the bounds' scaling rule, the problems and the oracle's answers, shared by
test_dt_host.py (the oracle and the host restatements alone, no GPU) and test_gpu_dt.py.

Every kernel family re-derives 1 / dt for itself and uses dt three ways: it scales the feed-forward and feedback rows of b, the CoM-box and
trunk-box rows of Clb / Cub, and multiplies qdot back into q_next. At dt = 0.002 alone 1 / dt rounds to exactly 500.0, so a constant where dt
belongs passes every test recorded at 2 ms.

Bounds. H, A and C do not depend on dt; the right-hand sides, and with them qdot, grow like 1 / dt, and the project's tolerances on qdot are
absolute. So a qdot bound at step dt is the named constant of the path times max(1, 0.002 / dt) (never wider for dt > 0.002), a roll-out's
state bound is ROLLOUT_Q_TOL max(1, dt / 0.002) (the state integrates qdot dt), and the relative bounds (ASSEMBLE_TOL through relerr, the
gradients' PARITY_BOUND max(1, max|ref|)) and INTEGRATE_TOL stay as they are."""
import functools

import numpy as np

import oracle
import test_gpu_task_params as tgp
from test_gpu_parity import QDOT_TOL, REFINED_TOL, ROLLOUT_Q_TOL

DT0 = 0.002
# a quarter of the nominal step (velocities up to four times larger, many more damper bounds active); a step whose 1 / dt is no round number;
# the reference's own regime, a measured step just above 2 ms; ten times the nominal step (the box rows shrink, the feed-forward nearly vanishes)
DTS = (0.0005, 1 / 240, 0.0020173, 0.02)
LAW_DTS = (1 / 240, 0.0020173)          # the power-of-two law: (dt, 2 dt)
GRAD_DTS = (0.0005, 1 / 240)
B0 = 67                                 # test_gpu_device_inplace.py: 16 full groups of four + 3, 22 of three + 1, past one 64-lane block
SEED = 5
ONE = ("a1_wx200",)                     # no model_id: c3 takes the packed sim3 kernel's FIXD form
TWO = ("a1_wx200", "a1_px100_pin_ver")
THREE = ("a1_wx200", "a1_px100_pin_ver", "laikago_vx300")
WITH_ROT = ("everything", "c3_trunk_task", "full")
TICK_CONFIGS = ("c3", "c2", "everything", "full", "c3_trunk_task", "c3_hybrid")


def qdot_scale(dt):
    return max(1.0, DT0 / dt)


def qdot_bound(tol, dt):
    """a qdot tolerance of the 2 ms tests at step dt"""
    return tol * qdot_scale(dt)


def state_bound(dt):
    """state and gripper trace after K ticks at step dt"""
    return ROLLOUT_Q_TOL * max(1.0, dt / DT0)


def path_refines(cfg, path, orth, refine):
    """Whether the kernel a tick ran on (last_path, last_orth, option refine) takes the refinement step at the final working set, read off the
    kernels: the packed sim3 kernel (path 2) and the general kernel (path 0) do, the general kernel not behind the orthonormal presolve and not
    with the CoM task on (n_refine = cfg.task_com ? 0 : refine); the compact kernel (1), the packed orth kernel (3) and the packed box kernel (4)
    have no refinement. A refining path is held to REFINED_TOL, every other to QDOT_TOL."""
    return bool(refine) and orth == 0 and (path == 2 or (path == 0 and not cfg.task_com))


def path_tol(cfg, path, orth, refine, dt):
    return qdot_bound(REFINED_TOL if path_refines(cfg, path, orth, refine) else QDOT_TOL, dt)


# ---- the power-of-two law. assemble at dt and at 2 dt: A, C, H, lb, ub bitwise equal; every row of b, Clb, Cub either bitwise equal ("E": no
# dt in it) or bitwise doubled at dt ("D": one factor 1 / dt, and halving 1 / dt is exact under any evaluation order as long as nothing
# underflows — for the device's x * (1 / dt) as for the oracle's x / dt), except the three angular trunk-task rows ("M"), which mix a 1 / dt
# term with a dt-free quaternion term. Rows in the assembly's order: EE tasks (6 each), trunk task (3 linear, 3 angular), CoM task, posture;
# constraints: CoM box (2), trunk box (4), stance feet (3 each).
ROW_CLASSES = {
    "everything": dict(b="D" * 33 + "M" * 3 + "E" * 29, box="D" * 6 + "E" * 12),
    "c3": dict(b="D" * 6 + "E" * 26, box="D" * 4 + "E" * 12),
    "c3_trunk_task": dict(b="D" * 9 + "M" * 3 + "E" * 26, box="D" * 4 + "E" * 12),
    "full": dict(b="D" * 33 + "M" * 3 + "E" * 26, box=""),
    "c2": dict(b="D" * 30 + "E" * 29, box="E" * 12),
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_doubling_law(at_dt, at_2dt, cfg_name, what):
    """the law above between two assemblies of the same inputs; -> the number of doubled rows that are not all zero (the law says nothing
    about a zero row)"""
    for k in ("A", "C", "H", "lb", "ub"):
        assert np.array_equal(_bits(at_dt[k]), _bits(at_2dt[k])), "%s: %s depends on dt" % (what, k)
    live = 0
    for k, classes in (("b", ROW_CLASSES[cfg_name]["b"]), ("Clb", ROW_CLASSES[cfg_name]["box"]), ("Cub", ROW_CLASSES[cfg_name]["box"])):
        assert at_dt[k].shape[1] == len(classes), (what, k, at_dt[k].shape)
        for r, c in enumerate(classes):
            x, y = at_dt[k][:, r], at_2dt[k][:, r]
            if c == "E":
                assert np.array_equal(_bits(x), _bits(y)), "%s: %s row %d must not depend on dt" % (what, k, r)
            elif c == "D":
                assert np.array_equal(_bits(x), _bits(2.0 * y)), "%s: %s row %d at dt is not twice the row at 2 dt" % (what, k, r)
                assert np.isfinite(x).all()
                live += bool(np.any(x != 0))
    return live


# ---- problems and the oracle's answers: built once, handed out read-only
def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def problem(names, cfg_name, B=B0, seed=SEED):
    """test_gpu_task_params._problem (the stress recipe; several models interleaved by model_id = arange(B) % n) with the orientation
    references where the configuration has a trunk task, and posture_u from the oracle under HYBRID -> (models, cfgs, d, mid)"""
    models, cfgs, d, mid = tgp._problem(list(names), cfg_name, B, seed=seed, with_rot=cfg_name in WITH_ROT)
    if cfg_name == "c3_hybrid":
        d["posture_u"] = oracle.posture_target(models, cfgs, d["q"], mid, nthreads=8)[0]
    return models, cfgs, _freeze(d), mid


@functools.lru_cache(maxsize=None)
def reference(names, cfg_name, dt, B=B0, seed=SEED):
    """oracle.tick of problem(...) at step dt"""
    models, cfgs, d, _ = problem(names, cfg_name, B, seed)
    return _freeze(oracle.tick(models, cfgs, d, dt, B, nthreads=8, want_q_next=True))


@functools.lru_cache(maxsize=None)
def assembled(names, cfg_name, dt, B=B0, seed=SEED):
    models, cfgs, d, _ = problem(names, cfg_name, B, seed)
    return _freeze(oracle.assemble(models, cfgs, d, dt, B))


_WORST = {}


def report(test, cfg_name, dt, value, bound=None):
    """print the worst measured deviation per (test, config, dt) — the table of DESIGN.md §3.39 is these lines"""
    key = (test, cfg_name, dt)
    _WORST[key] = max(_WORST.get(key, 0.0), float(value))
    print("DT-TABLE | %s | %s | %.7g | %.3e | %s" % (test, cfg_name, dt, _WORST[key], "" if bound is None else "%.3e" % bound))
