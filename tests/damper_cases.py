"""The velocity-damper cases shared by test_damper_envelope_host.py (the oracle alone, no GPU) and test_gpu_damper_envelope.py.

Every problem is built once (inputs of common.damper_tick_inputs, the oracle's assembly and answer, the zone and the active side of every bound)
and handed out read-only. One case per code path that states the damper, each under the reference's index map and under the corrected one."""
import functools

import numpy as np

import common
import oracle
import pose_cases as pc
import wbc_capi as capi
import wbc_model

DT, QDOT_TOL, REFINED_TOL, B0 = pc.DT, pc.QDOT_TOL, pc.REFINED_TOL, pc.B0
SEED = 15                # of the seeds 7 .. 18 tried the one at which EVERY case under both maps meets each condition of the host file
T, GEN, PO = pc.T, pc.GEN, pc.PO
QS_SHIFT = 1e-4          # the observability probe: damper_qs moved by this much
NO_LEG = ("base", "arm")

# name -> as pose_cases.TICK_CASES (models, configuration, handle options, the row that must run, the tolerance of the path's existing parity
# test) plus the recipe's switches: classes (the DoF classes the recipe draws from), fates ("mixed": no solved share is asked for)
TICK_CASES = {
    "c3": dict(models=("wx200",), cfg="c3", opts={}, row=("sim3p", (0, 0, 0, 0, 0)), tol=REFINED_TOL),
    "c3_trunk_task": dict(models=("wx200",), cfg="c3_trunk_task", opts={}, row=("sim3p", (0, 1, 0, 0, 0)), tol=QDOT_TOL),
    "c3_custom": dict(models=("wx200",), cfg="c3_custom", opts={}, row=("sim3p", (0, 0, 1, 0, 0)), tol=QDOT_TOL, qcon=True),
    "rot_c3": dict(models=("rot",), cfg="c3", opts={}, row=("sim3p", (0, 0, 0, 1, 0)), tol=QDOT_TOL),
    "c3_tp": dict(models=("wx200",), cfg="c3", opts={}, row=("sim3p", (0, 0, 0, 0, 1)), tol=QDOT_TOL, tp=True),
    "c3_compact": dict(models=("wx200",), cfg="c3", opts={"packed_kernel": 0, "refine": 0}, row=None, path=1, tol=QDOT_TOL),
    "c3_general": dict(models=("wx200",), cfg="c3", opts=GEN, row=("general", (T, 0, 0, 0, 0)), tol=QDOT_TOL),
    # a stance leg at a limit moves its foot, and with it the CoM box (RR and FL foot positions), off the CoM: with the leg class in the recipe the
    # oracle finds 12 - 40 % of the instances infeasible (seeds 7, 8, 15; with base and arm alone at most 1 of 67). So the case that must solve
    # draws from base and arm; the leg class of this path is in everything_fates below.
    "everything_orthp": dict(models=("wx200",), cfg="everything", opts=PO, row=("orthp", (1, 0, 0, 0)), tol=QDOT_TOL, with_rot=True, classes=NO_LEG),
    "full": dict(models=("wx200",), cfg="full", opts={}, row=("boxp", (0, 0, 0)), tol=QDOT_TOL, with_rot=True),
    "laikago_c3": dict(models=("laikago",), cfg="c3", opts={}, row=("general", (T, 0, 0, 1, 0)), tol=QDOT_TOL),
    "mixed_c3": dict(models=("wx200", "px100"), cfg="c3", opts={}, row=("sim3p", (0, 0, 0, 0, 0)), tol=QDOT_TOL),
    # presolve_tol_exp = 3 with dbg_force_defer (test_gpu_sim3p_cold_paths.py): flagged instances leave the packed path for their wave's tail
    "c3_tail": dict(models=("wx200",), cfg="c3", opts={"presolve_tol_exp": 3, "dbg_force_defer": 1}, row=("sim3p", (0, 0, 0, 0, 0)), tol=QDOT_TOL),
    # the full recipe on `everything`: a batch of mixed fates (status on every instance, values on the solved ones)
    "everything_fates": dict(models=("wx200",), cfg="everything", opts=PO, row=("orthp", (1, 0, 0, 0)), tol=QDOT_TOL, with_rot=True, fates="mixed"),
}
MAPS = (True, False)     # damper_compat: the reference's off-by-one index map, the corrected one


def config(name, m, compat=True, qs_shift=0.0):
    """common.config with the damper's tables of the index map asked for (wbc_model.damper_tables) and damper_qs moved by qs_shift"""
    c = capi.WbcConfig.from_buffer_copy(common.config(name, m))
    if not compat:
        qidx, lo, hi, vm, lock_from = wbc_model.damper_tables(m, False)
        assert lock_from == c.lock_from
        for i in range(m.nv):
            c.damper_qidx[i], c.damper_lo[i], c.damper_hi[i], c.damper_vmax[i] = int(qidx[i]), lo[i], hi[i], vm[i]
    c.damper_qs += qs_shift
    return c


def _per_model(models, mid, B, f):
    """f(i, model, rows of the batch that are this model's) -> an array per model, merged by model_id"""
    out = None
    for i, m in enumerate(models):
        sel = np.ones(B, dtype=bool) if mid is None else (mid == i)
        r = f(i, m, sel)
        if out is None:
            out = np.zeros((B,) + r.shape[1:], dtype=r.dtype)
        out[sel] = r
    return out


def zones_and_active(models, cfgs, mid, q, asm, ref):
    """-> (zone, active) [B, 26, 2] (lower, upper side): common.damper_zones of q, common.damper_active of a solved tick (nothing is active
    where the status is not 0); both read-only"""
    B = len(q)
    zone = _per_model(models, mid, B, lambda i, m, sel: common.damper_zones(cfgs[i], m.nv, q[sel]))
    active = _per_model(models, mid, B, lambda i, m, sel: common.damper_active(cfgs[i], m.nv, q[sel], asm["lb"][sel], asm["ub"][sel], ref["qdot"][sel]))
    active[ref["status"] != 0] = False
    zone.setflags(write=False)
    active.setflags(write=False)
    return zone, active


def build_problem(case, compat, B=B0, seed=SEED, edges=True):
    """-> dict(models, cfgs, d, mid, rows, ref (oracle.tick, cold), asm (oracle.assemble), oracle_args, q_int (the state the damper and the
    integration see), zone, active [B, 26, 2], B, case, compat)"""
    models = [pc.model(n) for n in case["models"]]
    cfgs = [config(case["cfg"], m, compat) for m in models]
    kw = dict(edges=edges, classes=case.get("classes", common.DAMPER_CLASSES), with_rot=case.get("with_rot", False))
    mid = None
    if len(models) == 1:
        d = common.damper_tick_inputs(models[0], cfgs[0], B, seed, **kw)
    else:
        mid = (np.arange(B) % len(models)).astype(np.int32)
        d = pc.merge([common.damper_tick_inputs(m, c, B, seed + i, **kw) for i, (m, c) in enumerate(zip(models, cfgs))], mid)
    if case.get("qcon"):     # test_tick_custom_posture_and_q_con, the other way round: q_con IS the damper pose, the tasks see a state 1 mrad off
        rng = np.random.default_rng(seed + 4)
        d["posture_u"] = rng.normal(size=(B, 26))
        d["q_con"] = d["q"].copy()
        d["q"] = d["q"].copy()
        d["q"][:, 7:] += rng.normal(0, 1e-3, (B, 20))
    rows = None
    ms, cs, dd = models, cfgs, d
    if case.get("tp"):
        rows = pc.gain_rows(cfgs[0], B, seed + 7)
        ms, cs, pid = common.per_instance_configs(models, cfgs, mid, rows)
        dd = dict(d, model_id=pid)
    ref = oracle.tick(ms, cs, dd, DT, B, nthreads=8)
    asm = oracle.assemble(ms, cs, dd, DT, B)
    q_int = d.get("q_con", d["q"])
    zone, active = zones_and_active(models, cfgs, mid, q_int, asm, ref)
    pc._freeze(d, ref, asm)
    return dict(models=models, cfgs=cfgs, d=d, mid=mid, rows=rows, ref=ref, asm=asm, oracle_args=(ms, cs, dd), q_int=q_int, zone=zone, active=active,
                B=B, case=case, compat=compat)


@functools.lru_cache(maxsize=None)
def tick_problem(name, compat):
    return build_problem(TICK_CASES[name], compat)


def classes_of(p):
    return p["case"].get("classes", common.DAMPER_CLASSES)


def coverage(p):
    """-> {(class, kind): instances the oracle solves with an ACTIVE bound of that DoF class in that zone}, kind over common.DAMPER_KINDS"""
    cls = np.array([common.damper_class(i) for i in range(capi.V_STRIDE)])
    out = {}
    for c, cname in enumerate(common.DAMPER_CLASSES):
        for k, kname in enumerate(common.DAMPER_KINDS):
            hit = p["active"] & (p["zone"] == k) & (cls == c)[None, :, None]
            out[cname, kname] = int(hit.any(axis=(1, 2)).sum())
    return out


def q_dependent(p):
    """active bounds that move with q: in the regular, flipped, edge or qs kinds and not clamped -> count per instance"""
    return (p["active"] & (p["zone"] >= 0) & (p["zone"] != 2)).sum(axis=(1, 2))


def shifted_reference(p, shift=QS_SHIFT):
    """the oracle's answer with damper_qs moved by `shift`"""
    ms, cs, dd = p["oracle_args"]
    cs2 = []
    for c in cs:
        c2 = capi.WbcConfig.from_buffer_copy(c)
        c2.damper_qs += shift
        cs2.append(c2)
    return oracle.tick(ms, cs2, dd, DT, p["B"], nthreads=8)


def observability(p, moved=QDOT_TOL):
    """(share of the instances the oracle solves, share of those whose q̇ moves by more than `moved` when damper_qs moves by QS_SHIFT)"""
    ref = p["ref"]
    ok = ref["status"] == 0
    sh = shifted_reference(p)
    both = ok & (sh["status"] == 0)
    dq = np.abs(sh["qdot"] - ref["qdot"]).max(axis=1)
    return ok.mean(), float(((dq > moved) & both).sum()) / max(1, int(ok.sum()))


def literal_bounds(p):
    """test_oracle_assembly._damper_literal on every instance -> lb, ub [B, 26] (columns >= the model's nv zero)"""
    from test_oracle_assembly import _damper_literal
    B = p["B"]
    lb, ub = np.zeros((B, capi.V_STRIDE)), np.zeros((B, capi.V_STRIDE))
    for b in range(B):
        m = p["models"][0 if p["mid"] is None else int(p["mid"][b])]
        lb[b, :m.nv], ub[b, :m.nv] = _damper_literal(m, p["q_int"][b], p["compat"])
    return lb, ub
