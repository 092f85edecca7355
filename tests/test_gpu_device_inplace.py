"""Every kernel variant, in place on device memory (WBC_MEM_DEVICE), against the CPU oracle under guard rows ("The device-path suite").

The host path stages every array into a padded private workspace and copies exactly B rows back, so it cannot show a store outside [0, B),
an input that was written, an aliasing hazard, or WHICH instantiation of a kernel family ran. Here every array is the live part of a
guarded device allocation (tests/devguard.py), every call runs on a side stream, the statistic "last_tick_variant" / "last_qp_variant"
must report the row the case is meant for, and the closing census holds the case table to the variant tables' own row counts
(wbc_variant_count). Tolerances are the existing parity tests' (test_gpu_parity.py) — none is new."""
import functools

import numpy as np
import pytest

import common
import devguard
import oracle
import wbc_capi as capi
import wbc_model
import wbc_workload
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
QDOT_TOL = 1e-5          # test_gpu_parity.py: the bound of BASELINE.json for q̇
REFINED_TOL = 1e-7       # test_gpu_parity.py: a path with the refinement on, against the oracle (which refines too)
QP_TOL, QP_WARM_TOL = 1e-8, 1e-7   # test_qp_hot_start_on_the_packed_kernel: cold / own set, and a perturbed problem's set
B0 = 67                  # 16 full groups of four + 3, 22 of three + 1, past one 64-lane block
BAR_EXP = 3              # test_gpu_sim3p_cold_paths.py: option presolve_tol_exp of the tail recipe
G = devguard.G

# ------------------------------------------------------------------------------------------------ the case table
# (family, template flags in the table's order (include/wbc.h, "last_tick_variant"), recipe). One entry per row of the six variant tables:
# a row added to a table needs its entry here (tests/test_capi_and_host.py holds the two to the same count without a GPU).
# Recipes: cfg = a common.config name, opts = handle options, entry = tick / assemble / fk / qp / qp_ls; ROT, TP and WARM follow from the flags
# (the rotated wx200, per-instance task rows, working sets in and out).
GEN = {"packed_kernel": 0, "sim3_kernel": 0}     # the sim3 switch set on the general kernel
NOPK = {"packed_orth": 0}                        # the equality-only set on the general kernel's ORTH variant
PO = {"packed_orth": 2}                          # the packed orth kernel at every batch size
T, A_, F = 0, 1, 2                               # MODE_TICK, MODE_ASSEMBLE, MODE_FK
CASES = [
    # general: MODE, WARM, ORTH, ROT, TP
    ("general", (T, 0, 0, 0, 0), dict(entry="tick", cfg="c3", opts=GEN)),
    ("general", (T, 1, 0, 0, 0), dict(entry="tick", cfg="c3", opts=GEN)),
    ("general", (T, 0, 1, 0, 0), dict(entry="tick", cfg="c2", opts=NOPK)),
    ("general", (A_, 0, 0, 0, 0), dict(entry="assemble", cfg="c3", opts={})),
    ("general", (F, 0, 0, 0, 0), dict(entry="fk", cfg="c3", opts={})),
    ("general", (T, 0, 0, 1, 0), dict(entry="tick", cfg="c3", opts=GEN)),
    ("general", (T, 1, 0, 1, 0), dict(entry="tick", cfg="c3", opts=GEN)),
    ("general", (T, 0, 1, 1, 0), dict(entry="tick", cfg="c2", opts=NOPK)),
    ("general", (A_, 0, 0, 1, 0), dict(entry="assemble", cfg="everything", opts={})),
    ("general", (F, 0, 0, 1, 0), dict(entry="fk", cfg="c3", opts={})),
    ("general", (T, 0, 0, 0, 1), dict(entry="tick", cfg="c3", opts=GEN)),
    ("general", (T, 1, 0, 0, 1), dict(entry="tick", cfg="c3", opts=GEN)),
    ("general", (A_, 0, 0, 0, 1), dict(entry="assemble", cfg="everything", opts={})),
    ("general", (T, 0, 1, 0, 1), dict(entry="tick", cfg="c2", opts=NOPK)),
    ("general", (T, 0, 1, 1, 1), dict(entry="tick", cfg="c2", opts=NOPK)),
    ("general", (T, 0, 0, 1, 1), dict(entry="tick", cfg="c3", opts=GEN)),
    ("general", (T, 1, 0, 1, 1), dict(entry="tick", cfg="c3", opts=GEN)),
    ("general", (A_, 0, 0, 1, 1), dict(entry="assemble", cfg="c3", opts={})),
    # sim3p: WARM, TRUNK, QCON, ROT, TP   (QCON: posture mode CUSTOM with the caller's posture_u and q_con)
    ("sim3p", (0, 0, 0, 0, 0), dict(entry="tick", cfg="c3", opts={})),
    ("sim3p", (1, 0, 0, 0, 0), dict(entry="tick", cfg="c3", opts={})),
    ("sim3p", (0, 1, 0, 0, 0), dict(entry="tick", cfg="c3_trunk_task", opts={})),
    ("sim3p", (1, 1, 0, 0, 0), dict(entry="tick", cfg="c3_trunk_task", opts={})),
    ("sim3p", (0, 0, 1, 0, 0), dict(entry="tick", cfg="c3_custom", opts={})),
    ("sim3p", (1, 0, 1, 0, 0), dict(entry="tick", cfg="c3_custom", opts={})),
    ("sim3p", (0, 0, 0, 1, 0), dict(entry="tick", cfg="c3", opts={})),
    ("sim3p", (1, 0, 0, 1, 0), dict(entry="tick", cfg="c3", opts={})),
    ("sim3p", (0, 1, 0, 1, 0), dict(entry="tick", cfg="c3_trunk_task", opts={})),
    ("sim3p", (1, 1, 0, 1, 0), dict(entry="tick", cfg="c3_trunk_task", opts={})),
    ("sim3p", (0, 0, 1, 1, 0), dict(entry="tick", cfg="c3_custom", opts={})),
    ("sim3p", (1, 0, 1, 1, 0), dict(entry="tick", cfg="c3_custom", opts={})),
    ("sim3p", (0, 0, 0, 0, 1), dict(entry="tick", cfg="c3", opts={})),
    ("sim3p", (1, 0, 0, 0, 1), dict(entry="tick", cfg="c3", opts={})),
    ("sim3p", (0, 1, 0, 0, 1), dict(entry="tick", cfg="c3_trunk_task", opts={})),
    ("sim3p", (1, 1, 0, 0, 1), dict(entry="tick", cfg="c3_trunk_task", opts={})),
    ("sim3p", (0, 0, 1, 0, 1), dict(entry="tick", cfg="c3_custom", opts={})),
    ("sim3p", (1, 0, 1, 0, 1), dict(entry="tick", cfg="c3_custom", opts={})),
    ("sim3p", (0, 0, 0, 1, 1), dict(entry="tick", cfg="c3", opts={})),
    ("sim3p", (1, 0, 0, 1, 1), dict(entry="tick", cfg="c3", opts={})),
    ("sim3p", (0, 1, 0, 1, 1), dict(entry="tick", cfg="c3_trunk_task", opts={})),
    ("sim3p", (1, 1, 0, 1, 1), dict(entry="tick", cfg="c3_trunk_task", opts={})),
    ("sim3p", (0, 0, 1, 1, 1), dict(entry="tick", cfg="c3_custom", opts={})),
    ("sim3p", (1, 0, 1, 1, 1), dict(entry="tick", cfg="c3_custom", opts={})),
    # orthp: INEQ, WARM, ROT, TP   (option packed_orth = 2: the packed kernel below its batch-size policy)
    ("orthp", (0, 0, 0, 0), dict(entry="tick", cfg="c2", opts=PO)),
    ("orthp", (1, 0, 0, 0), dict(entry="tick", cfg="everything", opts=PO)),
    ("orthp", (1, 1, 0, 0), dict(entry="tick", cfg="everything", opts=PO)),
    ("orthp", (0, 0, 1, 0), dict(entry="tick", cfg="c2", opts=PO)),
    ("orthp", (1, 0, 1, 0), dict(entry="tick", cfg="everything", opts=PO)),
    ("orthp", (1, 1, 1, 0), dict(entry="tick", cfg="everything", opts=PO)),
    ("orthp", (0, 0, 0, 1), dict(entry="tick", cfg="c2", opts=PO)),
    ("orthp", (1, 0, 0, 1), dict(entry="tick", cfg="everything", opts=PO)),
    ("orthp", (1, 1, 0, 1), dict(entry="tick", cfg="everything", opts=PO)),
    ("orthp", (0, 0, 1, 1), dict(entry="tick", cfg="c2", opts=PO)),
    ("orthp", (1, 0, 1, 1), dict(entry="tick", cfg="everything", opts=PO)),
    ("orthp", (1, 1, 1, 1), dict(entry="tick", cfg="everything", opts=PO)),
    # boxp: WARM, ROT, TP   (the warm-up problem: every Cartesian task, no constraint row)
    ("boxp", (0, 0, 0), dict(entry="tick", cfg="full", opts={})),
    ("boxp", (1, 0, 0), dict(entry="tick", cfg="full", opts={})),
    ("boxp", (0, 1, 0), dict(entry="tick", cfg="full", opts={})),
    ("boxp", (1, 1, 0), dict(entry="tick", cfg="full", opts={})),
    ("boxp", (0, 0, 1), dict(entry="tick", cfg="full", opts={})),
    ("boxp", (1, 0, 1), dict(entry="tick", cfg="full", opts={})),
    ("boxp", (0, 1, 1), dict(entry="tick", cfg="full", opts={})),
    ("boxp", (1, 1, 1), dict(entry="tick", cfg="full", opts={})),
    # qpp: G, PV, WARM, HALF   ((m, n, p) of test_qp_packed_edge_cases... / test_qp_hot_start_on_the_packed_kernel)
    ("qpp", (16, 16, 0, 0), dict(entry="qp_ls", mnp=(20, 14, 9), packed=1)),
    ("qpp", (32, 26, 0, 0), dict(entry="qp_ls", mnp=(96, 26, 24), packed=1)),
    ("qpp", (16, 16, 1, 0), dict(entry="qp_ls", mnp=(20, 14, 9), packed=1)),
    ("qpp", (32, 26, 1, 0), dict(entry="qp_ls", mnp=(36, 26, 20), packed=1)),
    ("qpp", (32, 26, 0, 1), dict(entry="qp_ls", mnp=(32, 26, 16), packed=1)),
    ("qpp", (32, 26, 1, 1), dict(entry="qp_ls", mnp=(32, 26, 16), packed=1)),
    # qp: NM, WARM   (option packed_kernel = 0)
    ("qp", (12, 0), dict(entry="qp", mnp=(7, 5, 8), packed=0)),
    ("qp", (16, 0), dict(entry="qp_ls", mnp=(20, 14, 9), packed=0)),
    ("qp", (24, 0), dict(entry="qp_ls", mnp=(40, 20, 20), packed=0)),
    ("qp", (26, 0), dict(entry="qp_ls", mnp=(96, 26, 24), packed=0)),
    ("qp", (16, 1), dict(entry="qp", mnp=(20, 14, 9), packed=0)),
    ("qp", (26, 1), dict(entry="qp_ls", mnp=(32, 26, 16), packed=0)),
]
LAST_PATH = {"general": 0, "sim3p": 2, "orthp": 3, "boxp": 4}
FLAG_NAMES = {"general": ("MODE", "WARM", "ORTH", "ROT", "TP"), "sim3p": ("WARM", "TRUNK", "QCON", "ROT", "TP"),
              "orthp": ("INEQ", "WARM", "ROT", "TP"), "boxp": ("WARM", "ROT", "TP"), "qpp": ("G", "PV", "WARM", "HALF"), "qp": ("NM", "WARM")}


def case_rows(family):
    """the distinct rows the table holds for a family (the CPU census of tests/test_capi_and_host.py)"""
    return {flags for fam, flags, _ in CASES if fam == family}


def key_of(flags):
    k = 0
    for a in tuple(flags) + (0,) * (5 - len(flags)):
        k = k * 256 + int(a)
    return k


def _traits(family, flags):
    f = dict(zip(FLAG_NAMES[family], flags))
    return dict(rot=bool(f.get("ROT")), tp=bool(f.get("TP")), warm=bool(f.get("WARM")), qcon=bool(f.get("QCON")))


def _case_id(i):
    fam, flags, r = CASES[i]
    on = "+".join(n for n, v in zip(FLAG_NAMES[fam], flags) if v and n != "MODE") or "plain"
    mode = {T: "", A_: "assemble-", F: "fk-"}[flags[0]] if fam == "general" else ""
    return "%s-%s%s" % (fam, mode, on if fam not in ("qpp", "qp") else "x".join(map(str, flags)))


# ------------------------------------------------------------------------------------------------ problems (CPU: inputs + the oracle's answer)
@functools.lru_cache(maxsize=None)
def _model(rot):
    if rot:
        from test_gpu_wave_order import _rotated_wx200
        return _rotated_wx200()
    return wbc_model.load_model("a1_wx200")


def _gain_rows(cfg, B, seed):
    """per-instance task rows that differ from the configuration's in the GAINS only (x log-uniform [0.5, 2]): gains enter the right-hand side
    b alone, H = A'WA and with it cond(H) stay the configuration's, so the parity tests' tolerances hold as they are"""
    rng = np.random.default_rng(seed)
    rows = wbc_model.task_params(cfg, B)
    sl = wbc_model.TASK_PARAMS_SLICES
    for f in ("ee_gain", "trunk_gain", "com_gain"):
        rows[:, sl[f]] *= np.exp(rng.uniform(np.log(0.5), np.log(2.0), (B, sl[f].stop - sl[f].start)))
    return rows


def _per_instance(model, cfg, rows):
    """the oracle's form of per-instance rows (test_gpu_task_params.py): B (model, configuration) pairs, model_id = arange(B)"""
    import ctypes as C
    off = capi.WbcConfig.ee_W.offset
    cs = []
    for r in rows:
        c = capi.WbcConfig.from_buffer_copy(cfg)
        C.memmove(C.addressof(c) + off, np.ascontiguousarray(r).ctypes.data, 85 * 8)
        cs.append(c)
    return [model] * len(rows), cs, np.arange(len(rows), dtype=np.int32)


def _inputs(model, cfg, cfg_name, B, seed, qcon):
    d = common.tick_inputs(model, cfg, B, seed=seed, with_rot=cfg_name in ("everything", "full"))
    if cfg.con_trunk and B > 8:     # two instances of another fate, one of them in the last, partial group: the trunk box three times the trunk
        d["trunk_box_center"] = d["trunk_box_center"].copy()      # height away contradicts the velocity bounds (test_infeasible_and_degenerate_instances...)
        d["trunk_box_center"][[3, B - 2], 0] *= 3.0
    if qcon:     # test_tick_custom_posture_and_q_con
        rng = np.random.default_rng(seed + 4)
        d["posture_u"] = rng.normal(size=(B, 26))
        d["q_con"] = d["q"].copy()
        d["q_con"][:, 7:] += rng.normal(0, 1e-3, (B, 20))
    return d


@functools.lru_cache(maxsize=None)
def tick_problem(cfg_name, rot, tp, qcon, B):
    """-> dict(model, cfg, d, other (2 G rows of another valid batch), rows, rows_other, ref (oracle.tick), asm (oracle.assemble on demand))"""
    model = _model(rot)
    cfg = common.config(cfg_name, model)
    seed = 211 + B     # (checked on the CPU: with it every case meets condition_on_inputs on the oracle alone)
    d = _inputs(model, cfg, cfg_name, B, seed, qcon)
    other = _inputs(model, cfg, cfg_name, 2 * G, seed + 500, qcon)
    rows = rows_other = None
    ms, cs, dd = [model], [cfg], d
    if tp:
        rows, rows_other = _gain_rows(cfg, B, seed + 7), _gain_rows(cfg, 2 * G, seed + 8)
        ms, cs, pid = _per_instance(model, cfg, rows)
        dd = dict(d, model_id=pid)
    ref = oracle.tick(ms, cs, dd, DT, B, nthreads=8)
    for v in list(d.values()) + list(ref.values()):
        v.setflags(write=False)
    return dict(model=model, cfg=cfg, d=d, other=other, rows=rows, rows_other=rows_other, ref=ref, oracle_args=(ms, cs, dd), B=B)


def _qp_data(m, n, p, B, seed):
    """test_qp_hot_start_on_the_packed_kernel's problems (a fixed variable, an equality row) with two instances of another fate: rows that
    contradict the box (infeasible), one of them in the last, partial group"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(B, m, n))
    if m < n:
        A = np.concatenate([A, np.broadcast_to(0.1 * np.eye(n), (B, n, n))], axis=1)
    b = rng.normal(size=(B, A.shape[1])) * 3
    C = rng.normal(size=(B, p, n))
    lb, ub = -rng.uniform(0.05, 0.6, (B, n)), rng.uniform(0.05, 0.6, (B, n))
    lb[:, 2] = ub[:, 2] = 0.01
    cl, cu = -rng.uniform(0.05, 0.6, (B, p)), rng.uniform(0.05, 0.6, (B, p))
    cl[:, 1] = cu[:, 1] = 0.02
    for bad in ({3, B - 2} if B > 8 else ()):
        cl[bad, 0], cu[bad, 0] = 50.0, 60.0
    return dict(A=A, b=b, C=C, lb=lb, ub=ub, Clb=cl, Cub=cu)


@functools.lru_cache(maxsize=None)
def qp_problem(entry, m, n, p, B):
    d = _qp_data(m, n, p, B, 70 + n + p)
    other = _qp_data(m, n, p, 2 * G, 170 + n + p)
    pert = d["b"] + np.random.default_rng(5).normal(size=d["b"].shape) * 0.1      # the "previous tick" the WARM seeds come from
    if entry == "qp":
        for x in (d, other):
            x["H"] = np.einsum("bmi,bmj->bij", x["A"], x["A"]) + 1e-3 * np.eye(n)
            x["g"] = -np.einsum("bmi,bm->bi", x["A"], x["b"])
        d["g_pert"] = -np.einsum("bmi,bm->bi", d["A"], pert)
        xr, sr, ir = oracle.qp_solve(d["H"], d["g"], d["C"], d["lb"], d["ub"], d["Clb"], d["Cub"])
    else:
        d["b_pert"] = pert
        xr, sr, ir = oracle.qp_solve_ls(d["A"], d["b"], d["C"], d["lb"], d["ub"], d["Clb"], d["Cub"])
    return dict(d=d, other=other, ref=(xr, sr, ir), B=B)


def condition_on_inputs(ref_status, mixed):
    """the oracle alone: at least 90 % optimal, and a non-optimal instance where the case mixes fates"""
    ok = np.asarray(ref_status) == 0
    assert ok.mean() >= 0.9, "only %d of %d instances optimal on the oracle" % (int(ok.sum()), len(ok))
    if mixed:
        assert (~ok).any(), "no non-optimal instance in a case that mixes fates"
    return ok


# ------------------------------------------------------------------------------------------------ running under guards
@functools.lru_cache(maxsize=None)
def _side():
    import torch
    return torch.cuda.Stream()


def _handle(models, cfg, max_batch, opts):
    bt = WbcBatch(models, max_batch)
    if cfg is not None:
        bt.configure(cfg)
    for k, v in (opts or {}).items():
        bt.set_option(k, v)
    return bt


def run_modes(bt, modes, call, what, aliased=(), after=None):
    """call(session) under every mode of devguard.Session, each on the side stream with the handle's outputs allocated under guards; guard and
    input checks after each; the live results of all modes byte-identical. -> the first mode's results (numpy). after(bt): asserted after each call."""
    import torch
    outs = []
    for mode in modes:
        s = devguard.Session(mode, _side())
        bt.allocator = s.alloc
        torch.cuda.synchronize()
        try:
            res = devguard.to_host(s.run(lambda: call(s)))
        except RuntimeError as e:                           # a failed HIP call is a device fault: nothing more is started on that device
            hip = getattr(e, "code", None) == capi.E_HIP if isinstance(e, capi.WbcError) else ("HIP error" in str(e) or "illegal memory access" in str(e))
            if hip:
                pytest.exit("device fault in %s [%s]: %s" % (what, mode, e), returncode=3)
            raise
        finally:
            bt.allocator = None
        s.check("%s [%s]" % (what, mode), aliased)
        if after:
            after(bt)
        outs.append(res)
    for mode, res in zip(modes[1:], outs[1:]):
        assert devguard.same_bytes(res, outs[0]), "%s: live results with guards [%s] differ from %s" % (what, mode, modes[0])
    return outs[0]


TICK_MODES = ("exact", "other", "nan")       # NaN guard rows: the ticks' in-batch NaN containment is asserted by test_non_finite_inputs_are_contained
PLAIN_MODES = ("exact", "other")             # every other entry point (assemble and fk included): rows of another valid batch only


def _ws_other(seeds):
    return np.resize(seeds[::-1], (2 * G, 2))


def _tick_call(bt, p, seeds=None, want_ws=False, alias_ws=False):
    def call(s):
        dev = s.put_all(p["d"], p["other"])
        tp = s.put("task_params", p["rows"], p["rows_other"])
        if seeds is not None:
            dev["working_set"] = s.put("working_set", seeds, _ws_other(seeds))
        if alias_ws:      # the header: "WbcTickOut.working_set may alias the input"
            B = p["B"]
            out = dict(qdot=s.out((B, 26)), status=s.out((B,), np.int32), iters=s.out((B,), np.int32), q_next=s.out((B, 27)),
                       working_set=dev["working_set"])
            res = dict(bt.tick(dev, DT, out=out, task_params=tp))
            res["working_set"] = res["working_set"].clone()
            return res
        return bt.tick(dev, DT, want_q_next=True, want_working_set=want_ws, task_params=tp)
    return call


def _seeds(bt, p):
    """working sets of a perturbed solve (test_warm_started_tick_reaches_the_cold_optimum: the same robots a moment earlier, targets 0.3 mm back)"""
    prev = dict(p["d"], ee_target=p["d"]["ee_target"] - 3e-4)
    got = run_modes(bt, ("exact",), _tick_call(bt, dict(p, d=prev), want_ws=True), "seed solve")
    return got["working_set"]


# equal working-set changes on a COLD tick, as the existing parity test of the path asserts them (the share of the optimal instances that must
# agree exactly): test_packed_orth_kernel_with_inequality_rows, test_packed_box_kernel_variants_and_non_finite_inputs,
# test_packed_box_kernel_redoes_what_its_reduction_does_not_cover. (Warm ticks count other changes than the cold oracle; the other paths'
# parity tests assert no per-instance equality.)
ITERS_SHARE = {"orthp-ineq": 0.98, "boxp": 0.99, "boxp-tail": 0.98}


def check_tick(got, p, tol, what, mixed=False, iters=None):
    ref = p["ref"]
    ok = condition_on_inputs(ref["status"], mixed)
    if iters is not None:
        share = (got["iters"] == ref["iters"])[ok].mean()
        print("%s: iters equal to the oracle's on %.4f of the optimal instances (gpu mean %.2f, oracle %.2f)" % (
            what, share, got["iters"][ok].mean(), ref["iters"][ok].mean()))
        assert share > ITERS_SHARE[iters], (what, share)
    assert (got["status"] == ref["status"]).all(), (what, np.flatnonzero(got["status"] != ref["status"]))
    err = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    print("%s: qdot max-abs err vs oracle %.3e, optimal %d/%d" % (what, err, int(ok.sum()), len(ok)))
    assert err < tol, (what, err)
    assert np.abs(got["q_next"] - ref["q_next"])[ok].max() < 1e-7, what
    return ok


def _expect_variant(bt, stat, family, flags):
    def after(bt_):
        if family in LAST_PATH:
            assert bt_.stat("last_path") == LAST_PATH[family], (family, bt_.stat("last_path"))
        got = bt_.stat(stat)
        assert got == key_of(flags), "%s: %s = %s, want %s %s" % (family, stat, capi.variant_args(got), flags, FLAG_NAMES[family])
    return after


REACHED = {}     # case index -> key reported (the census)


def run_case(i, B=B0):
    fam, flags, r = CASES[i]
    what = "%s B=%d" % (_case_id(i), B)
    if r["entry"] in ("qp", "qp_ls"):
        return _run_qp_case(i, B, what)
    t = _traits(fam, flags)
    p = tick_problem(r["cfg"], t["rot"], t["tp"], t["qcon"], B)
    bt = _handle(p["model"], p["cfg"], B, r["opts"])
    after = _expect_variant(bt, "last_tick_variant", fam, flags)
    try:
        if r["entry"] == "tick":
            seeds = _seeds(bt, p) if t["warm"] else None
            got = run_modes(bt, TICK_MODES, _tick_call(bt, p, seeds, want_ws=t["warm"]), what, after=after)
            tol = REFINED_TOL if (fam == "sim3p" and flags == (0, 0, 0, 0, 0)) else QDOT_TOL    # (test_stress_instances_drop_slots)
            cold_iters = None if t["warm"] else ("boxp" if fam == "boxp" else "orthp-ineq" if fam == "orthp" and flags[0] else None)
            ok = check_tick(got, p, tol, what, mixed=bool(p["cfg"].con_trunk) and B > 8, iters=cold_iters)
            if t["warm"]:
                assert (got["working_set"][~ok] == 0).all(), what               # an unsolved QP carries nothing
        elif r["entry"] == "assemble":
            def call(s):
                return bt.assemble(s.put_all(p["d"], p["other"]), DT, task_params=s.put("task_params", p["rows"], p["rows_other"]))
            got = run_modes(bt, PLAIN_MODES, call, what, after=after)
            ms, cs, dd = p["oracle_args"]
            ref = oracle.assemble(ms, cs, dd, DT, B)
            for k in ("A", "b", "H", "g", "C", "Clb", "Cub", "lb", "ub"):       # test_assemble_parity
                assert got[k].shape == ref[k].shape, (what, k)
                e = 0.0 if got[k].size == 0 else np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
                assert e < 1e-11, (what, k, e)
        else:
            def call(s):
                return bt.fk(s.put("q", p["d"]["q"], p["other"]["q"]))
            got = run_modes(bt, PLAIN_MODES, call, what, after=after)
            ref = oracle.fk([p["model"]], p["d"]["q"])
            for k in ("oMi", "oMf", "J", "com", "Jcom"):                        # test_fk_jacobians_parity
                assert np.abs(got[k] - ref[k]).max() < 1e-12, (what, k)
        REACHED[i] = bt.stat("last_tick_variant")
    finally:
        bt.close()


def _qp_call(bt, r, p, seeds, want_ws, alias_ws=False):
    d, o = p["d"], p["other"]

    def call(s):
        a = {k: s.put(k, d[k], o[k]) for k in ("A", "b", "H", "g", "C", "lb", "ub", "Clb", "Cub") if k in d}
        ws = None if seeds is None else s.put("working_set", seeds, _ws_other(seeds))
        if alias_ws:      # the header: working_set_in == working_set_out is allowed — straight through the C entry point
            return _qp_raw(bt, r["entry"], a, ws, s)
        if r["entry"] == "qp":
            return bt.qp_solve(a["H"], a["g"], a["C"], a["lb"], a["ub"], a["Clb"], a["Cub"], working_set=ws, want_working_set=want_ws)
        return bt.qp_solve_ls(a["A"], a["b"], a["C"], a["lb"], a["ub"], a["Clb"], a["Cub"], working_set=ws, want_working_set=want_ws)
    return call


def _qp_raw(bt, entry, a, ws, s):
    """wbc_qp_solve / wbc_qp_solve_ls with ONE working-set buffer (in == out); -> (x, status, iters, the buffer's contents after the call)"""
    import torch
    B, n = a["lb"].shape
    p = a["C"].shape[1]
    x, st, it = s.out((B, n)), s.out((B,), np.int32), s.out((B,), np.int32)
    stream = torch.cuda.current_stream(bt.device_id).cuda_stream
    P = lambda t: None if t is None else t.data_ptr()
    if entry == "qp":
        rc = bt.lib.wbc_qp_solve(bt._h, B, n, p, P(a["H"]), P(a["g"]), P(a["C"]), P(a["lb"]), P(a["ub"]), P(a["Clb"]), P(a["Cub"]), capi.MEM_DEVICE,
                                 P(x), P(st), P(it), P(ws), P(ws), stream)
    else:
        m = a["A"].shape[1]
        rc = bt.lib.wbc_qp_solve_ls(bt._h, B, m, n, p, P(a["A"]), P(a["b"]), P(a["C"]), P(a["lb"]), P(a["ub"]), P(a["Clb"]), P(a["Cub"]),
                                    capi.MEM_DEVICE, -1, P(x), P(st), P(it), None, None, P(ws), P(ws), stream)
    capi.check(rc, bt.lib)
    return x, st, it, ws.clone()


def _qp_seeds(bt, r, p):
    d = p["d"]
    pert = dict(d, g=d["g_pert"]) if r["entry"] == "qp" else dict(d, b=d["b_pert"])
    return run_modes(bt, ("exact",), _qp_call(bt, r, dict(p, d=pert), None, True), "seed solve")[-1]


def _run_qp_case(i, B, what):
    fam, flags, r = CASES[i]
    m, n, p_ = r["mnp"]
    warm = bool(flags[-2] if fam == "qpp" else flags[-1])
    p = qp_problem(r["entry"], m, n, p_, B)
    xr, sr, ir = p["ref"]
    ok = condition_on_inputs(sr, mixed=B > 8)
    bt = _handle([], None, B, {"packed_kernel": r["packed"]})
    after = _expect_variant(bt, "last_qp_variant", fam, flags)
    try:
        seeds = _qp_seeds(bt, r, p) if warm else None
        got = run_modes(bt, PLAIN_MODES, _qp_call(bt, r, p, seeds, warm), what, after=after)
        x, st, it = got[:3]
        assert (st == sr).all(), (what, np.flatnonzero(st != sr))
        assert (x[~ok] == 0).all(), what                                          # x = 0 where unsolved (test_qp_packed_edge_cases...)
        err = np.abs(x - xr)[ok].max()
        print("%s: x max-abs err vs oracle %.3e, optimal %d/%d" % (what, err, int(ok.sum()), B))
        assert err < (QP_WARM_TOL if warm else QP_TOL), (what, err)
        if not warm:
            assert (it[ok] == ir[ok]).all(), what                                 # cold: the textbook method's working-set changes
        else:
            assert (got[3][~ok] == 0).all(), what
        REACHED[i] = bt.stat("last_qp_variant")
        assert bt.stat("last_qp_path") == ({16: 4, 32: 2}[flags[0]] if fam == "qpp" else 1)
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 0. the guards themselves
def test_the_guards_notice_a_stray_write_and_a_written_input():
    """tests/devguard.py on its own: the live view starts 1080 bytes into a [B][27] allocation; one element written next to the live rows,
    before or behind them, or inside an input, fails the check; NaN guard rows are NaN and the output pattern is a NaN with a payload."""
    import torch
    s = devguard.Session("nan", _side())
    out = s.out((B0, 27))
    q = s.put("q", np.zeros((B0, 27)), np.ones((2 * G, 27)))
    ws = s.put("working_set", np.zeros((B0, 2), np.int64), np.ones((2 * G, 2), np.int64))
    go, gq, gw = s.outputs[0], s.inputs["q"], s.inputs["working_set"]
    assert out.data_ptr() - go.flat.data_ptr() == 1080 and q.data_ptr() - gq.flat.data_ptr() == 1080 and ws.data_ptr() - gw.flat.data_ptr() == 80
    assert torch.isnan(gq.flat[:G * 27]).all() and torch.isnan(gq.flat[-G * 27:]).all() and not torch.isnan(q).any()
    assert (gw.flat[:2 * G] == 1).all() and (ws == 0).all()                   # (no NaN for integers: the other batch's rows)
    assert torch.isnan(go.flat).all() and go.flat.view(torch.int64)[0].item() == 0x7FF8DEADBEEF5A5A
    s.check("untouched")
    out.fill_(1.0)                                                            # the live rows are the call's to write
    s.check("live rows written")
    for where, at in (("BEFORE", G * 27 - 1), ("BEHIND", (G + B0) * 27)):
        bits = go.flat.view(torch.int64)                                      # (as integers: the pattern's payload comes back bit for bit)
        keep = bits[at].item()
        go.flat[at] = 0.0
        with pytest.raises(AssertionError, match=where):
            s.check("stray write")
        bits[at] = keep
        s.check("restored")
    q[B0 - 1, 26] = 1.0
    with pytest.raises(AssertionError, match="input q was written"):
        s.check("written input")
    s.check("an input aliased to an output may change", aliased=("q",))
    gq.flat[0] = 0.0
    with pytest.raises(AssertionError, match="guards of aliased q"):
        s.check("aliased, but written outside", aliased=("q",))


# ------------------------------------------------------------------------------------------------ 1. every row of every table, B = 67
@pytest.mark.parametrize("i", range(len(CASES)), ids=_case_id)
def test_every_variant_in_place_under_guards(i):
    """B = 67: the statistic reports the row, live rows held to the oracle, guards intact, inputs unchanged, both guard fills and exact-size
    tensors byte-identical, all on a side stream from the handle's first call on."""
    run_case(i)


def _index(family, flags):
    return next(i for i, c in enumerate(CASES) if c[0] == family and c[1] == tuple(flags))


# one cold and one WARM row of each packed family
SMALL_ROWS = [("sim3p", (0, 0, 0, 0, 0)), ("sim3p", (1, 0, 0, 0, 0)), ("orthp", (0, 0, 0, 0)), ("orthp", (1, 1, 0, 0)), ("boxp", (0, 0, 0)),
              ("boxp", (1, 0, 0)), ("qpp", (16, 16, 0, 0)), ("qpp", (16, 16, 1, 0))]
SMALL = [(_index(f, fl), B) for f, fl in SMALL_ROWS for B in (1, 5)]


@pytest.mark.parametrize("i,B", SMALL, ids=["%s-B%d" % (_case_id(i), B) for i, B in SMALL])
def test_packed_kernels_with_one_wave_mostly_shadow(i, B):
    """B = 1 and 5 for a cold and a WARM row of each packed family: one live instance beside three (one) shadow groups"""
    run_case(i, B)


# ------------------------------------------------------------------------------------------------ 2. the census
@pytest.mark.parametrize("family", capi.VARIANT_FAMILIES)
def test_census_every_row_of_the_table_was_reached(family):
    for i, (fam, _, _) in enumerate(CASES):
        if fam == family and i not in REACHED:
            run_case(i)                                      # (run alone, e.g. with -k: the cases are run here)
    keys = {REACHED[i] for i, (fam, _, _) in enumerate(CASES) if fam == family}
    n = capi.variant_count(family)
    print("%s: %d of %d rows reached" % (family, len(keys), n))
    assert len(keys) == n, (family, sorted(capi.variant_args(k) for k in keys))


# ------------------------------------------------------------------------------------------------ 3. tails in the last, partial group
def _leg_block_ratio(a):
    """min over the four stance feet of |det K| / (sum |K_ij|)^3 (test_gpu_sim3p_cold_paths.py)"""
    r = np.full(a["C"].shape[0], np.inf)
    for f, d0 in enumerate((9, 6, 15, 12)):
        K = a["C"][:, 4 + 3 * f:7 + 3 * f, d0:d0 + 3]
        r = np.minimum(r, np.abs(np.linalg.det(K)) / np.abs(K).sum(axis=(1, 2)) ** 3)
    return r


def _subset(p, idx, other_idx):
    d = {k: np.ascontiguousarray(v[idx]) for k, v in p["d"].items()}
    other = {k: np.ascontiguousarray(v[other_idx]) for k, v in p["d"].items()}
    ref = {k: v[idx] for k, v in p["ref"].items()}
    return dict(p, d=d, other=other, ref=ref, B=len(idx))


@functools.lru_cache(maxsize=None)
def tail_problem(family):
    """-> (problem of B0 instances, options, mask of the instances the tail must redo): tail instances in row 2 and in the last, partial group"""
    if family == "sim3p":        # a flagged stance-leg block + dbg_force_defer (test_forced_defer_takes_the_tail_and_counts)
        big = tick_problem("c3", False, False, False, 512)
        ratio = _leg_block_ratio(oracle.assemble([big["model"]], [big["cfg"]], big["d"], DT, 512))
        bar = 10.0 ** -BAR_EXP
        optimal = big["ref"]["status"] == 0
        flagged, plain = np.flatnonzero((ratio < 0.5 * bar) & optimal), np.flatnonzero(ratio > 2.0 * bar)
        idx = plain[:B0].copy()
        idx[2], idx[B0 - 2] = flagged[0], flagged[1]
        return _subset(big, idx, plain[B0:B0 + 2 * G]), {"presolve_tol_exp": BAR_EXP, "dbg_force_defer": 1}, ratio[idx] < bar
    if family == "orthp":        # option orth_qr: EVERY instance (test_packed_orth_ineq_tail_hot_started_matches_cold)
        p = tick_problem("everything", False, False, False, B0)
        return p, {"packed_orth": 2, "orth_qr": 1}, np.ones(B0, bool)
    # boxp: the base box shrunk — an eliminated DoF at its bound (test_packed_box_kernel_redoes_what_its_reduction_does_not_cover, "base_bound";
    # at 0.5 instead of 0.05 some instances of this batch stay on the packed path: tail and packed rows share wavefronts)
    model = _model(False)
    cfg = common.config("full", model)
    for i in range(6):
        cfg.damper_vmax[i] = 0.5
    d = common.tick_inputs(model, cfg, B0, seed=93, with_rot=True)
    ref = oracle.tick([model], [cfg], d, DT, B0, nthreads=8)
    at_bound = ((np.abs(np.abs(ref["qdot"][:, :6]) - 0.5) < 1e-12).sum(axis=1) > 0) & (ref["status"] == 0)
    assert at_bound[B0 - 3:].any() and not at_bound.all()
    other = common.tick_inputs(model, cfg, 2 * G, seed=94, with_rot=True)
    return dict(model=model, cfg=cfg, d=d, other=other, ref=ref, rows=None, rows_other=None, B=B0), {}, at_bound


TAIL_FAMILIES = ("sim3p", "orthp", "boxp")
TAIL_FLAGS = {"sim3p": lambda warm: (warm, 0, 0, 0, 0), "orthp": lambda warm: (1, warm, 0, 0), "boxp": lambda warm: (warm, 0, 0)}    # the rows the tail recipes run on


@pytest.mark.parametrize("warm", [0, 1], ids=["cold", "warm"])
@pytest.mark.parametrize("family", TAIL_FAMILIES)
def test_in_kernel_tail_meets_shadow_lanes_and_guards(family, warm):
    """An instance that takes the in-kernel tail (redone on the general path by its own wave) in the last, partial group of B = 67: tail,
    shadow groups and guard rows meet. Cold and with working sets in and out."""
    p, opts, expect = tail_problem(family)
    bt = _handle(p["model"], p["cfg"], B0, opts)
    what = "%s tail, %s" % (family, "warm" if warm else "cold")

    variant = _expect_variant(bt, "last_tick_variant", family, TAIL_FLAGS[family](warm))

    def after(bt_):
        variant(bt_)
        assert bt_.stat("deferred_last", _side().cuda_stream) == int(expect.sum()), (what, bt_.stat("deferred_last"), int(expect.sum()))
    try:
        seeds = None
        if warm:
            for k, v in opts.items():                         # the seeds: a perturbed solve on the packed path itself
                if k in ("dbg_force_defer", "orth_qr"):
                    bt.set_option(k, 0)
            seeds = _seeds(bt, p)
            for k, v in opts.items():
                bt.set_option(k, v)
        got = run_modes(bt, TICK_MODES, _tick_call(bt, p, seeds, want_ws=bool(warm)), what, after=after)
        assert expect[B0 - 3:].any()                          # (a tail instance in the last, partial group)
        check_tick(got, p, QDOT_TOL, what, iters="boxp-tail" if family == "boxp" and not warm else None)
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 4. the wave order across its 127-wave slice
def test_wave_order_across_a_slice_boundary_with_one_live_instance_in_the_last_wave():
    """B = 513 with wave_order = 2: 129 waves cross the 127-wave slice, the last wave has one live instance. Run twice: the second call runs
    in the order the first recorded. Guards and the oracle on both."""
    B = 513
    p = tick_problem("c3", False, False, False, B)
    bt = _handle(p["model"], p["cfg"], B, {"wave_order": 2})
    after = _expect_variant(bt, "last_tick_variant", "sim3p", (0, 0, 0, 0, 0))
    try:
        first = run_modes(bt, ("other",), _tick_call(bt, p), "wave order, first call", after=after)
        assert bt.stat("wave_order_slices", _side().cuda_stream) == 2
        second = run_modes(bt, ("other", "nan"), _tick_call(bt, p), "wave order, recorded order", after=after)
        for name, got in (("first", first), ("second", second)):
            check_tick(got, p, REFINED_TOL, "wave order, %s call" % name, mixed=True)
        assert devguard.same_bytes(first, second)             # (test_gpu_wave_order.py: the order never changes a result)
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 5. aliasing
ALIAS_TICKS = [("sim3p", (1, 0, 0, 0, 0), 0), ("orthp", (1, 1, 0, 0), 0), ("boxp", (1, 0, 0), 0), ("general", (T, 1, 0, 0, 0), 0),
               ("sim3p", (1, 0, 0, 0, 0), 1), ("orthp", (1, 1, 0, 0), 1), ("boxp", (1, 0, 0), 1)]      # (the general kernel has no tail)


@pytest.mark.parametrize("family,flags,tail", ALIAS_TICKS, ids=["%s-%s" % (f, "tail" if t else "packed") for f, _, t in ALIAS_TICKS])
def test_tick_working_set_out_may_be_the_input(family, flags, tail):
    """include/wbc.h: "WbcTickOut.working_set may alias the input". One buffer for both, byte for byte what separate buffers give — on a WARM
    row of each tick family, and with an instance in the in-kernel tail for the packed ones."""
    expect = None
    if tail:
        p, opts, expect = tail_problem(family)
    else:
        i = _index(family, flags)
        t = _traits(family, flags)
        p, opts = tick_problem(CASES[i][2]["cfg"], t["rot"], t["tp"], t["qcon"], B0), CASES[i][2]["opts"]
    bt = _handle(p["model"], p["cfg"], B0, opts)
    variant = _expect_variant(bt, "last_tick_variant", family, flags)

    def after(bt_):
        variant(bt_)
        if tail:                                              # instances took the tail in THIS call, with the buffer aliased or not
            nd = bt_.stat("deferred_last", _side().cuda_stream)
            assert nd > 0 and nd == int(expect.sum()), (family, nd, int(expect.sum()))
    try:
        if tail:                                              # (the seeds: a perturbed solve on the packed path itself, as in the tail test)
            for k in opts:
                if k in ("dbg_force_defer", "orth_qr"):
                    bt.set_option(k, 0)
        seeds = _seeds(bt, p)
        for k, v in opts.items():
            bt.set_option(k, v)
        apart = run_modes(bt, ("other",), _tick_call(bt, p, seeds, want_ws=True), "separate buffers", after=after)
        alias = run_modes(bt, ("other", "nan"), _tick_call(bt, p, seeds, alias_ws=True), "working_set in == out", aliased=("working_set",), after=after)
        assert devguard.same_bytes(alias, apart), "%s: aliasing the working set changes the result" % family
    finally:
        bt.close()


# every WARM row of both QP tables as the case table runs it, and each WARM row with the OTHER entry point as well: wbc_qp_solve (H and g given,
# m = 0: another input path of the kernels) and wbc_qp_solve_ls, each with packed_kernel on and off
QP_ALIAS = [(c[0], c[1], dict(c[2], entry=e)) for c in CASES if c[0] in ("qpp", "qp") and (c[1][-2] if c[0] == "qpp" else c[1][-1])
            for e in ("qp", "qp_ls")]


@pytest.mark.parametrize("fam,flags,r", QP_ALIAS, ids=["%s-%s-%s" % (f, "x".join(map(str, fl)), r["entry"]) for f, fl, r in QP_ALIAS])
def test_qp_working_set_in_may_be_working_set_out(fam, flags, r):
    """include/wbc.h: working_set_in == working_set_out is allowed in wbc_qp_solve AND wbc_qp_solve_ls — on the packed kernel and (option
    packed_kernel 0) the one-per-wavefront kernel, every WARM row of both tables: byte for byte what separate buffers give, which is held to
    the oracle."""
    m, n, p_ = r["mnp"]
    p = qp_problem(r["entry"], m, n, p_, B0)
    xr, sr, _ = p["ref"]
    ok = condition_on_inputs(sr, mixed=True)
    bt = _handle([], None, B0, {"packed_kernel": r["packed"]})
    after = _expect_variant(bt, "last_qp_variant", fam, flags)
    try:
        seeds = _qp_seeds(bt, r, p)
        apart = run_modes(bt, ("other",), _qp_call(bt, r, p, seeds, True), "separate buffers", after=after)
        assert (apart[1] == sr).all() and np.abs(apart[0] - xr)[ok].max() < QP_WARM_TOL and (apart[0][~ok] == 0).all()
        alias = run_modes(bt, ("other",), _qp_call(bt, r, p, seeds, True, alias_ws=True), "one buffer", aliased=("working_set",), after=after)
        assert devguard.same_bytes(alias, apart)
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 6. integrate, update_state, posture_target
def _update_problem(B):
    rng = np.random.default_rng(13 + B)
    m = _model(False)
    n = B + 2 * G
    d = dict(q_cur=wbc_workload.sample_q(m, n, rng), q_next=wbc_workload.sample_q(m, n, rng), targets=rng.normal(size=(n, 5, 3)), imu=rng.normal(size=(n, 4)))
    d["imu"] /= np.linalg.norm(d["imu"], axis=1, keepdims=True)
    return m, {k: v[:B] for k, v in d.items()}, {k: v[B:] for k, v in d.items()}


@pytest.mark.parametrize("B", [4, B0])
def test_integrate_in_place(B):
    rng = np.random.default_rng(9)
    m = _model(False)
    q, v = wbc_workload.sample_q(m, B + 2 * G, rng), rng.normal(size=(B + 2 * G, 26)) * 2
    bt = _handle(m, None, B, {})
    try:
        got = run_modes(bt, PLAIN_MODES, lambda s: bt.integrate(s.put("q", q[:B], q[B:]), s.put("v", v[:B], v[B:]), DT), "integrate")
        assert np.abs(got - oracle.integrate([m], q[:B], v[:B], DT)).max() < 1e-13      # test_integrate_parity
    finally:
        bt.close()


@pytest.mark.parametrize("imu", [1, 0], ids=["imu", "noimu"])
@pytest.mark.parametrize("packed", [1, 0], ids=["packed", "one_per_wave"])
@pytest.mark.parametrize("B", [4, B0])
def test_update_state_in_place_and_with_q_new_being_q_cur(B, packed, imu):
    """wbc_update_state on both kernels, with and without the IMU, against the oracle; then with q_new == q_cur (include/wbc.h allows it): byte for
    byte what separate buffers give"""
    import torch
    m, d, o = _update_problem(B)
    bt = _handle(m, common.config("c3", m), B, {"packed_update": packed})
    ref = oracle.update_state([m], d["q_cur"], d["q_next"], d["targets"], d["imu"] if imu else None)

    def call(s, alias):
        a = {k: s.put(k, d[k], o[k]) for k in ("q_cur", "q_next", "targets")}
        im = s.put("imu", d["imu"], o["imu"]) if imu else None
        if not alias:
            return bt.update_state(a["q_cur"], a["q_next"], a["targets"], im)
        P = lambda t: None if t is None else t.data_ptr()
        capi.check(bt.lib.wbc_update_state(bt._h, B, P(a["q_cur"]), P(a["q_next"]), P(im), P(a["targets"]), None, capi.MEM_DEVICE, P(a["q_cur"]),
                                           torch.cuda.current_stream(bt.device_id).cuda_stream), bt.lib)
        return a["q_cur"].clone()
    try:
        got = run_modes(bt, PLAIN_MODES, lambda s: call(s, False), "update_state")
        assert bt.stat("last_update_packed") == packed
        assert np.abs(got - ref).max() < 1e-13 and (got[:, 3:] == ref[:, 3:]).all()       # test_update_state_parity
        alias = run_modes(bt, ("other",), lambda s: call(s, True), "update_state, q_new == q_cur", aliased=("q_cur",))
        assert bt.stat("last_update_packed") == packed
        assert devguard.same_bytes(alias, got), "q_new == q_cur changes the result"
    finally:
        bt.close()


@pytest.mark.parametrize("form,par", [("three_per_wave", 1), ("one_per_wave", 3), ("sequential", 0)])
@pytest.mark.parametrize("B", [4, B0])
def test_posture_target_in_place(B, form, par):
    """wbc_posture_target on its three kernels; B = 4: the three-instances-per-wave kernel with one live instance in its second wave"""
    rng = np.random.default_rng(17)
    m = _model(False)
    cfg = wbc_model.sim3_config(m, Joint="MANI", posture_literal=True)
    q = wbc_workload.sample_q(m, B + 2 * G, rng)
    ur, qar = oracle.posture_target([m], [cfg], q[:B])
    bt = _handle(m, cfg, B, {"posture_par": par})
    try:
        u, qa = run_modes(bt, PLAIN_MODES, lambda s: bt.posture_target(s.put("q", q[:B], q[B:])), "posture_target " + form)
        assert bt.stat("last_posture_par") == {1: 2, 3: 1, 0: 0}[par]
        assert np.abs(u - ur).max() < 1e-9 and (qa == qar).all()                          # test_posture_target_parity
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ 7. roll-outs, and max_batch independence
K, HOLD = 4, 1


@functools.lru_cache(maxsize=None)
def rollout_problem(mode):
    B = B0
    cfg_name = "c3" if mode == "running" else "full"
    p = tick_problem(cfg_name, False, False, False, B)
    rng = np.random.default_rng(2)
    n = B + 2 * G
    step = np.zeros((n, 5, 3))
    step[:, 4] = rng.normal(0, 1e-4, (n, 3))
    imu = np.concatenate([p["d"]["q"][:, 3:7], p["other"]["q"][:, 3:7]]) if mode == "running" else None
    targets = [p["d"]["ee_target"].copy()]
    for k in range(K + HOLD - 1):                              # the device adds the step K times, then holds
        targets.append(targets[-1] + step[:B] if k < K else targets[-1])
    ref = oracle.rollout([p["model"]], [p["cfg"]], {k: v for k, v in p["d"].items()}, DT, B, K + HOLD, imu=None if imu is None else imu[:B],
                         nthreads=8, running=mode == "running", ee_target_at=lambda k: targets[k])
    return dict(p=p, step=step, imu=imu, ref=ref, final_target=targets[-1] if HOLD else targets[-1] + step[:B])


def _rollout_call(bt, rp, mode):
    p, B = rp["p"], B0

    def call(s):
        dev = s.put_all(p["d"], p["other"])
        imu = None if rp["imu"] is None else s.put("imu", rp["imu"][:B], rp["imu"][B:], nan_ok=False)
        return bt.rollout(dev, DT, K, ee_target_step=s.put("ee_target_step", rp["step"][:B], rp["step"][B:], nan_ok=False), imu=imu, want_trace=True,
                          mode=capi.ROLLOUT_RUNNING if mode == "running" else capi.ROLLOUT_WARMUP, hold_ticks=HOLD)
    return call


@pytest.mark.parametrize("warm", [0, 1], ids=["cold", "warm_start"])
@pytest.mark.parametrize("mode", ["running", "warmup"])
def test_rollout_in_place_and_independent_of_max_batch(mode, warm):
    """wbc_rollout (ticks 4, hold 1, the gripper trace on) under guards against the oracle's loop at test_rollout_parity's tolerances — and on a
    handle with max_batch = B + 61 byte for byte what max_batch = B gives: the workspaces are laid out [block][max_batch], an overrun of one
    block lands in the next block's instance 0 exactly when max_batch == B."""
    rp = rollout_problem(mode)
    ref, res = rp["ref"], []
    ok = condition_on_inputs(ref["status"], mixed=False)
    for mb in (B0, B0 + 61):
        bt = _handle(rp["p"]["model"], rp["p"]["cfg"], mb, {"warm_start": warm})
        try:
            res.append(run_modes(bt, TICK_MODES, _rollout_call(bt, rp, mode), "rollout %s max_batch %d" % (mode, mb)))
            assert bt.stat("last_path") == (2 if mode == "running" else 4) and bt.stat("last_update_packed") == 1
        finally:
            bt.close()
    got = res[0]
    assert devguard.same_bytes(res[0], res[1]), "the roll-out depends on max_batch"
    assert (got["status"] == ref["status"]).all()
    assert np.abs(got["q"] - ref["q"])[ok].max() < 1e-6 and np.abs(got["qdot"] - ref["qdot"])[ok].max() < 10 * QDOT_TOL
    assert np.abs(got["ee_target"] - rp["final_target"]).max() < 1e-15
    assert got["grip_trace"].shape == (K + HOLD, B0, 3) and np.abs(got["grip_trace"] - ref["grip_trace"])[:, ok].max() < 1e-6
    if not warm:                                              # cold: the oracle's working-set changes (test_rollout_parity: 2 per tick)
        gap = np.abs(got["iters"][ok] - ref["iters"][ok]).max()
        print("rollout %s: iters sums differ from the oracle's by at most %d over %d ticks" % (mode, gap, K + HOLD))
        assert gap <= 2 * (K + HOLD)


MB_TICKS = [_index("general", (T, 0, 0, 0, 0)), _index("sim3p", (0, 0, 0, 0, 0)), _index("orthp", (1, 0, 0, 0)), _index("boxp", (0, 0, 0))]


@pytest.mark.parametrize("i", MB_TICKS, ids=_case_id)
def test_tick_is_independent_of_max_batch(i):
    """one tick case per family on a handle with max_batch = B and one with B + 61 (off any power-of-two stride): byte-identical"""
    fam, flags, r = CASES[i]
    t = _traits(fam, flags)
    p = tick_problem(r["cfg"], t["rot"], t["tp"], t["qcon"], B0)
    res = []
    for mb in (B0, B0 + 61):
        bt = _handle(p["model"], p["cfg"], mb, dict(r["opts"], wave_order=2))
        try:
            res.append([run_modes(bt, ("other",), _tick_call(bt, p), "max_batch %d" % mb, after=_expect_variant(bt, "last_tick_variant", fam, flags)) for _ in range(2)])
        finally:
            bt.close()
    assert devguard.same_bytes(res[0][0], res[1][0]) and devguard.same_bytes(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------ 8. trajectories and tracks (B = 66: groups exist)
BT = 66


TAU = 1e-6           # trace tolerance of test_rollout_parity (test_gpu_rollout_tracks.py)
GRIP = common.GRIP
ROLLOUT_KEYS = ("q", "qdot", "status", "iters", "ee_target")
FRAME_SCORES = ("err_sq_sum", "err_max", "err_final", "err_max_tick")


def _tracks_batch(B, seed, track_seed):
    """test_gpu_rollout_tracks.py's base recipe (common.base_tracks: a HERMITE trunk track and a LINEAR gripper track) on c3_trunk_task"""
    model = _model(False)
    cfg = common.config("c3_trunk_task", model)
    d = {k: v.copy() for k, v in common.tick_inputs(model, cfg, B, seed=seed, stress=False).items()}
    tracks = common.base_tracks(d, common.track_frames([model], d["q"], None)[:, GRIP], track_seed)
    common.start_previous_targets(d, tracks)
    return dict(models=[model], cfgs=[cfg], d=d, mid=None, tracks=tracks, B=B, K=K, imu=d["q"][:, 3:7].copy(), running=True, rows=None)


@functools.lru_cache(maxsize=None)
def tracks_problem():
    """-> (the problem at B = 66 and four ticks, 2 G instances of another seed for the guard rows, the oracle's loop: common.tracks_reference)"""
    p = _tracks_batch(BT, 41, 5)
    return p, _tracks_batch(2 * G, 57, 8), common.tracks_reference(p)


def _put_tracks(s, tracks, others):
    """(NaN guard rows around the trajectory points only: their in-batch NaN containment is asserted by the trajectory tests)"""
    out = []
    for j, (t, o) in enumerate(zip(tracks, others)):
        out.append({k: (s.put("track%d.%s" % (j, k), v, o[k], nan_ok=(k == "points")) if isinstance(v, np.ndarray) else v) for k, v in t.items()})
    return out


@pytest.mark.parametrize("group_size", [1, 11])
def test_rollout_tracks_in_place_and_independent_of_max_batch(group_size):
    """wbc_rollout_tracks: two tracks (trunk HERMITE, gripper LINEAR), the gripper and one frame that is NOT followed (foot 0) scored, groups of 1
    and 11 at B = 66. The [n_scored][B] and [ticks][n_scored][B][3] arrays are guarded around the whole array."""
    p, o, ref = tracks_problem()
    ok = condition_on_inputs(ref["status"], mixed=False)
    scored = (0, GRIP)
    res = []
    for mb in (BT, BT + 61):
        bt = _handle(p["models"], p["cfgs"][0], mb, {})

        def call(s):
            dev = s.put_all(p["d"], o["d"])
            return bt.rollout_tracks(dev, DT, K, _put_tracks(s, p["tracks"], o["tracks"]), score=scored, group_size=group_size,
                                     want_trace=True, imu=s.put("imu", p["imu"], o["imu"], nan_ok=False))
        try:
            res.append(run_modes(bt, TICK_MODES, call, "rollout_tracks max_batch %d" % mb))
            assert bt.stat("last_traj_bad_rows", _side().cuda_stream) == 0
        finally:
            bt.close()
    got = res[0]
    assert devguard.same_bytes(res[0], res[1]), "wbc_rollout_tracks depends on max_batch"
    assert (got["status"] == ref["status"]).all()
    assert np.abs(got["q"] - ref["q"])[ok].max() < 1e-6 and np.abs(got["qdot"] - ref["qdot"])[ok].max() < 1e-4      # test_gpu_rollout_tracks.test_parity_with_the_oracle
    assert np.abs(got["grip_trace"] - ref["frames"][:, :, GRIP])[:, ok].max() < TAU
    assert got["trace"].shape == (K, 2, BT, 3)
    for j, f in enumerate(scored):
        assert np.abs(got["trace"][:, j] - ref["frames"][:, :, f])[:, ok].max() < TAU
    assert max(np.abs(got["ee_target"] - ref["ee_target"]).max(), np.abs(got["trunk_target"] - ref["trunk_target"]).max()) < 1e-15
    # the scores are the reduction of the call's own trace against the oracle's targets (test_scores_are_the_reduction_of_the_calls_own_trace)
    tg = np.stack([ref["targets"][:, :, f] for f in scored], axis=1)
    want = common.numpy_scores(got["trace"], tg, ref["tick_status"])
    assert got["err_sq_sum"].shape == (2, BT)
    for k in ("err_max_tick", "first_bad_tick", "bad_ticks"):
        assert (got[k] == want[k]).all(), k
    for k in ("err_sq_sum", "err_max", "err_final"):
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
    ng = BT // group_size
    assert got["group_rms"].shape == (2, ng) and got["group_worst_status"].shape == (ng,)
    assert (got["group_worst_status"] == ref["status"].reshape(ng, group_size).max(axis=1)).all()
    rms = np.sqrt(got["err_sq_sum"].reshape(2, ng, group_size).sum(axis=2) / (K * group_size))
    assert np.abs(got["group_rms"] - rms).max() <= 1e-12 * max(1.0, rms.max())


def test_rollout_traj_in_place_and_independent_of_max_batch():
    """wbc_rollout_traj (one LINEAR gripper trajectory) under guards; it is the one-track call of wbc_rollout_tracks bit for bit
    (test_one_linear_gripper_track_is_rollout_traj_bit_for_bit), which is held to the oracle above."""
    p, o, _ = tracks_problem()
    g, go = p["tracks"][1], o["tracks"][1]
    res = []
    for mb in (BT, BT + 61):
        bt = _handle(p["models"], p["cfgs"][0], mb, {})

        def traj(s):
            dev = s.put_all(p["d"], o["d"])
            return bt.rollout_traj(dev, DT, K, points=s.put("points", g["points"], go["points"]), n_points=s.put("n_points", g["n_points"], go["n_points"], nan_ok=False),
                                   du=s.put("du", g["du"], go["du"], nan_ok=False), ee_index=GRIP, group_size=11, want_trace=True, imu=s.put("imu", p["imu"], o["imu"], nan_ok=False))

        def tracks(s):
            dev = s.put_all(p["d"], o["d"])
            return bt.rollout_tracks(dev, DT, K, _put_tracks(s, [g], [go]), score=(GRIP,), group_size=11, want_trace=True,
                                     imu=s.put("imu", p["imu"], o["imu"], nan_ok=False))
        try:
            old = run_modes(bt, TICK_MODES, traj, "rollout_traj max_batch %d" % mb)
            new = run_modes(bt, ("other",), tracks, "one-track rollout_tracks")
        finally:
            bt.close()
        for k in ROLLOUT_KEYS + ("grip_trace", "first_bad_tick", "bad_ticks", "group_worst_status", "group_bad_instances"):
            assert new[k].tobytes() == old[k].tobytes(), k
        for k in FRAME_SCORES + ("group_rms", "group_err_max"):
            assert new[k].tobytes() == old[k].tobytes(), k
        res.append(old)
    assert devguard.same_bytes(res[0], res[1]), "wbc_rollout_traj depends on max_batch"
