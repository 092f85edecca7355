"""The batches of tests/test_gpu_sim3p_entry.py and tools/make_entry_golden.py: what the packed sim3 kernel's entry can get wrong
when the issue order of its loads changes — a lone row, rows without an instance, a short second wave, the wave order's identity tick and its list
ticks, optional inputs left out, tables that depend on the instance, and each variant's own inputs. One definition, so that the recording and the
test run the same calls. The B = 67 inputs are those of tests/golden/sim3p_guards.npz; the B <= 5 batches are its b5 rows with orientation
references added (stored in tests/golden/sim3p_entry.npz)."""
import numpy as np

import common
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch

DT = 0.002
OUT = ("qdot", "status", "iters", "q_next")
ROLL_OUT = ("q", "qdot", "ee_target", "status", "iters")
OPTIONAL = ("ee_target", "prev_ee_target", "trunk_box_center", "ee_ref_rot")     # ee_ref_rot: ee_prev_rot goes with it
ROLL_TICKS = 3


def _inputs(zg, src):
    pre = src + "_in_"
    return {k[len(pre):]: np.ascontiguousarray(zg[k]) for k in zg.files if k.startswith(pre)}


def _without(d, names):
    drop = set(names) | ({"ee_prev_rot"} if "ee_ref_rot" in names else set())
    return {k: v for k, v in d.items() if k not in drop}


def cases(zg, small_rot):
    """zg: the loaded sim3p_guards.npz; small_rot: dict(ee_ref_rot, ee_prev_rot) [5, 5, 9] for the small batch.
    -> {name: dict(models, cfg, d, opts, ticks, kw, kind, fixd)}; fixd: what "last_tick_fixd" must say (None: not asked)"""
    small = dict(_inputs(zg, "b5"), **small_rot)
    single, mixed = _inputs(zg, "single"), _inputs(zg, "mixed")
    tp = _inputs(zg, "tp")
    rows = tp.pop("task_params")
    c = {}

    def add(name, d, models=("a1_wx200",), cfg="c3", opts=None, ticks=1, kw=None, kind="tick", fixd=1):
        c[name] = dict(models=models, cfg=cfg, d=d, opts=dict(opts or {}), ticks=ticks, kw=dict(kw or {}), kind=kind, fixd=fixd)

    for B in (1, 3, 4, 5):
        add("small_B%d" % B, {k: np.ascontiguousarray(v[:B]) for k, v in small.items()}, opts={"wave_order": 0})
    add("wo_B5", small, opts={"wave_order": 2}, ticks=3)
    add("wo_B67", single, opts={"wave_order": 2}, ticks=3)
    for name in OPTIONAL:
        add("absent_" + name, _without(small, (name,)), opts={"wave_order": 0})
    add("absent_all", _without(small, OPTIONAL), opts={"wave_order": 0})
    add("mixed", mixed, models=("a1_wx200", "a1_px100_pin_ver"), fixd=0)
    add("single_fixd1", single, opts={"sim3p_fixd": 1})
    add("single_fixd0", single, opts={"sim3p_fixd": 0}, fixd=0)
    add("warm", dict(single, working_set=np.ascontiguousarray(zg["warm_in_working_set"])), kw={"want_working_set": True})
    add("trunk", _inputs(zg, "trunk"), cfg="c3_trunk_task")
    add("tp", tp, kw={"task_params": np.ascontiguousarray(rows)})
    add("qcon", _inputs(zg, "qcon"), cfg="c3_mani", fixd=0)
    add("rollout", single, kind="rollout", fixd=None)
    return c


def other_rows(zg):
    """rows of other valid batches for devguard's input guards, by input name (at least 2 G = 10 rows each)"""
    o = dict(_inputs(zg, "trunk"))
    o["model_id"] = np.zeros(16, np.int32)
    o["working_set"] = np.ascontiguousarray(zg["warm_in_working_set"][::-1])
    o["task_params"] = np.ascontiguousarray(zg["tp_in_task_params"][::-1])
    return o


def keys_of(case):
    if case["kind"] == "rollout":
        return ROLL_OUT
    return OUT + (("working_set",) if case["kw"].get("want_working_set") else ())


def run(case, put=None, before=None, after=None):
    """Runs the case on a fresh handle. put(name, array) -> what the library is handed (None: the host array); before(bt) / after(bt, tick) around
    every call. -> ("ok", [per tick: {output: array as returned}], [per tick: stats]) or ("refused", message): the library's own argument check
    turned the call down (an input the configuration needs was left out)."""
    put = put or (lambda name, a: a)
    models = [wbc_model.load_model(m) for m in case["models"]]
    bt = WbcBatch(models, len(case["d"]["q"]))
    try:
        for i, m in enumerate(models):
            bt.configure(common.config(case["cfg"], m), i)
        for k, v in case["opts"].items():
            bt.set_option(k, v)
        res, stats = [], []
        for tick in range(1, case["ticks"] + 1):
            if before:
                before(bt)
            d = {k: put(k, v) for k, v in case["d"].items()}
            kw = {k: (put(k, v) if isinstance(v, np.ndarray) else v) for k, v in case["kw"].items()}
            try:
                if case["kind"] == "rollout":
                    got = bt.rollout(d, DT, ROLL_TICKS, want_trace=False, **kw)
                else:
                    got = bt.tick(d, DT, want_q_next=True, **kw)
            except capi.WbcError as e:
                if getattr(e, "code", None) == capi.E_ARG:
                    return "refused", str(e)
                raise
            if after:
                after(bt, tick)
            st = {"last_path": bt.stat("last_path"), "wave_order_slices": bt.stat("wave_order_slices")}
            if case["kind"] == "tick":
                st["last_tick_fixd"] = bt.stat("last_tick_fixd")
            res.append(got)
            stats.append(st)
        return "ok", res, stats
    finally:
        bt.close()
