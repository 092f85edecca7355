"""The packed sim3 kernel's wave order (option "wave_order") changes which wave and row run an instance, never its result.

Every check compares a handle with the order on (option value 2: at every batch size) against a handle with it off: qdot, status, iters and the working set must be
bit-identical on the first call (identity order), on later calls (the recorded order), after the inputs are permuted (a wrong prediction), after
the batch size changes, and on the variants the packed kernel has (mixed models, task rows, rotated joint placements, WARM, the tail)."""
import copy
import json
import os

import numpy as np
import pytest

import common
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
KEYS = ("qdot", "status", "iters", "working_set", "q_next")


def _rotated_wx200():
    """a1_wx200 with rotated joint placements (as test_gpu_rotated_placement.py): the packed kernel's ROT instantiations"""
    with open(os.path.join(wbc_model.MODELS_DIR, "a1_wx200.json")) as f:
        data = copy.deepcopy(json.load(f))
    for name, rpy in (("elbow", (3.14, 0, 0)), ("wrist_rotate", (-3.14, 0, 0))):
        r, p_, y = rpy
        cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p_), np.sin(p_), np.cos(y), np.sin(y)
        R = [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
             [-sp, cp * sr, cp * cr]]
        next(j for j in data["joints"] if j["name"] == name)["placement_R"] = R
    data["name"] = "a1_wx200_rotated"
    return wbc_model.Model(data, dict(wbc_model.A1_ROLES))


def _problem(names, cfg_name, B, seed):
    models = [_rotated_wx200() if n == "rot" else wbc_model.load_model(n) for n in names]
    cfgs = [common.config(cfg_name, m) for m in models]
    if len(models) == 1:
        return models, cfgs, common.tick_inputs(models[0], cfgs[0], B, seed=seed)
    mid = (np.arange(B) % len(models)).astype(np.int32)
    parts = [common.tick_inputs(m, c, B, seed=seed + i) for i, (m, c) in enumerate(zip(models, cfgs))]
    d = {}
    for k in parts[0]:
        v = parts[0][k].copy()
        for i in range(1, len(parts)):
            v[mid == i] = parts[i][k][mid == i]
        d[k] = v
    d["model_id"] = mid
    return models, cfgs, d


def _pair(models, cfgs, max_batch, options=None):
    """(order on, order off) handles with the same configuration and options"""
    out = []
    for wo in (2, 0):                                 # (2: at every batch size; the default 1 takes batches from 16384 instances on)
        bt = WbcBatch(models, max_batch)
        for i, c in enumerate(cfgs):
            bt.configure(c, i)
        for k, v in (options or {}).items():
            bt.set_option(k, v)
        bt.set_option("wave_order", wo)
        out.append(bt)
    return out


def _same(a, b, what):
    for k in KEYS:
        if k in a or k in b:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape, (what, k)
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs in %d instances" % (
                what, k, int((x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1).sum()))


def _slices(B):
    """slices of waves whose order the next launch reads once the order is in effect (wbc_device.h WO_SW = 127 waves per slice)"""
    return -(-(-(-B // 4)) // 127)


def _sub(d, idx):
    return {k: v[idx] for k, v in d.items()}


def _tick(bt, d, **kw):
    return bt.tick(d, DT, want_q_next=True, **kw)


@pytest.mark.parametrize("case", ["c3", "mixed", "tp", "rot", "rot_tp", "trunk"])
def test_identical_on_repeated_and_permuted_calls(case):
    """Calls 1, 2 and 10 on the same inputs, then a permutation of them (the recorded order predicts nothing): identical to the order off."""
    B = 4096
    names = {"mixed": ["a1_wx200", "a1_px100_pin_ver"], "rot": ["rot"], "rot_tp": ["rot"]}.get(case, ["a1_wx200"])
    models, cfgs, d = _problem(names, "c3_trunk_task" if case == "trunk" else "c3", B, seed=31)
    kw = {}
    if case.endswith("tp"):
        rows = wbc_model.task_params(cfgs[0], B)
        rng = np.random.default_rng(5)
        rows *= rng.uniform(0.5, 2.0, rows.shape)
        kw["task_params"] = rows
    on, off = _pair(models, cfgs, B)
    ref = _tick(off, d, **kw)
    st = np.asarray(ref["status"])
    it = np.asarray(ref["iters"])
    print("%s: %d of %d optimal, iters %d..%d" % (case, int((st == 0).sum()), B, it.min(), it.max()))
    for call in range(1, 11):
        got = _tick(on, d, **kw)
        if call in (1, 2, 10):
            _same(got, ref, "%s call %d" % (case, call))
    assert on.stat("last_path") == 2
    assert on.stat("wave_order_slices") == _slices(B) and off.stat("wave_order_slices") == 0   # (a recorded order is in effect)
    perm = np.random.default_rng(7).permutation(B)
    dp = _sub(d, perm)
    kwp = {k: v[perm] for k, v in kw.items()}
    refp = _tick(off, dp, **kwp)
    for call in range(2):
        _same(_tick(on, dp, **kwp), refp, "%s permuted, call %d" % (case, call))
        assert on.stat("wave_order_slices") == _slices(B)
    on.close(); off.close()


def test_batch_size_changes():
    """B changes between calls (multiples of four and not, B = 1): every call identical to the order off."""
    Bmax = 4097
    models, cfgs, d = _problem(["a1_wx200"], "c3", Bmax, seed=41)
    on, off = _pair(models, cfgs, Bmax)
    for B in (4097, 4097, 5, 1, 5, 4096, 4097, 4097, 1000, 1000, 3):
        s = _sub(d, np.arange(B))
        _same(_tick(on, s), _tick(off, s), "B = %d" % B)
        assert on.stat("wave_order_slices") == _slices(B)
    on.close(); off.close()


def test_default_takes_large_batches_only():
    """The default (option 1) records and reads the order from 16384 instances on, and leaves smaller batches in the identity order."""
    B = 16384
    models, cfgs, d = _problem(["a1_wx200"], "c3", B, seed=17)
    dflt = WbcBatch(models, B)
    dflt.configure(cfgs[0], 0)
    _, off = _pair(models, cfgs, B)
    ref = _tick(off, d)
    for call in range(3):
        _same(_tick(dflt, d), ref, "default, call %d" % call)
        assert dflt.stat("wave_order_slices") == _slices(B)
    s = _sub(d, np.arange(4096))
    _same(_tick(dflt, s), _tick(off, s), "default, B = 4096")
    assert dflt.stat("wave_order_slices") == 0
    dflt.close(); off.close()


def test_warm_variant_and_working_sets():
    """The WARM variant reads ws_in and writes ws_out at the permuted instance."""
    B = 2048
    models, cfgs, d = _problem(["a1_wx200"], "c3", B, seed=51)
    on, off = _pair(models, cfgs, B)
    ws = _tick(off, d, want_working_set=True)["working_set"]
    dw = dict(d, working_set=np.asarray(ws))
    ref = _tick(off, dw, want_working_set=True)
    for call in range(3):
        _same(_tick(on, dw, want_working_set=True), ref, "warm call %d" % call)
    perm = np.random.default_rng(3).permutation(B)
    dp = _sub(dw, perm)
    _same(_tick(on, dp, want_working_set=True), _tick(off, dp, want_working_set=True), "warm permuted")
    on.close(); off.close()


def test_tail_instances_are_recorded():
    """Instances redone by the kernel's tail (dbg_force_defer with a raised singularity bar) are written and counted once."""
    B = 3001
    models, cfgs, d = _problem(["a1_wx200", "a1_px100_pin_ver"], "c3", B, seed=83)
    on, off = _pair(models, cfgs, B, {"presolve_tol_exp": 3, "dbg_force_defer": 1})
    ref = _tick(off, d)
    assert off.stat("deferred_last") > 0
    for call in range(3):
        _same(_tick(on, d), ref, "tail call %d" % call)
        assert on.stat("deferred_last") == off.stat("deferred_last")
    on.close(); off.close()


def test_every_output_slot_is_written_on_device():
    """Outputs prefilled with NaN / -1 on the device: after each call no slot keeps its fill."""
    import torch
    B = 1029
    models, cfgs, d = _problem(["a1_wx200"], "c3", B, seed=61)
    on, off = _pair(models, cfgs, B)
    ref = _tick(off, d)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    for call in range(4):
        out = dict(qdot=torch.full((B, 26), float("nan"), dtype=torch.float64, device="cuda"),
                   status=torch.full((B,), -1, dtype=torch.int32, device="cuda"), iters=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
                   q_next=torch.full((B, 27), float("nan"), dtype=torch.float64, device="cuda"))
        on.tick(dev, DT, out=out)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert not np.isnan(got["qdot"]).any() and (got["status"] >= 0).all() and (got["iters"] >= 0).all()
        _same(got, ref, "device call %d" % call)
    on.close(); off.close()


def test_graph_capture_replays():
    """A captured tick replayed several times (the order moves on inside the graph) gives the uncaptured results."""
    import torch
    B = 2048
    models, cfgs, d = _problem(["a1_wx200"], "c3", B, seed=71)
    on, off = _pair(models, cfgs, B)
    ref = _tick(off, d)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    out = dict(qdot=torch.empty((B, 26), dtype=torch.float64, device="cuda"), status=torch.empty(B, dtype=torch.int32, device="cuda"),
               iters=torch.empty(B, dtype=torch.int32, device="cuda"))
    call = on.make_tick_call(dev, out, DT)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                        # (warm-up outside the capture: lazy workspaces)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for rep in range(4):
        out["qdot"].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        ref_ = {k: np.asarray(ref[k]) for k in ("qdot", "status", "iters")}
        _same(got, ref_, "replay %d" % rep)
    on.close(); off.close()


def test_rollout_identical():
    """A 10-tick closed loop (the order carried from tick to tick inside wbc_rollout) is identical with the order on and off."""
    B, K = 2048, 10
    m = wbc_model.load_model("a1_wx200")
    cfg = common.config("c3", m)
    d = common.tick_inputs(m, cfg, B, seed=91)
    rng = np.random.default_rng(3)
    step = np.zeros((B, 5, 3))
    step[:, 4] = rng.normal(0, 1e-4, (B, 3))
    imu = d["q"][:, 3:7].copy()
    on, off = _pair([m], [cfg], B)
    a = on.rollout(d, DT, K, ee_target_step=step, imu=imu, mode=capi.ROLLOUT_RUNNING)
    b = off.rollout(d, DT, K, ee_target_step=step, imu=imu, mode=capi.ROLLOUT_RUNNING)
    assert on.stat("last_path") == 2
    for k in b:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k
    on.close(); off.close()


def test_configure_resets_to_identity():
    """A reconfigured handle starts from the identity order again and stays identical."""
    B = 1024
    models, cfgs, d = _problem(["a1_wx200"], "c3", B, seed=13)
    on, off = _pair(models, cfgs, B)
    ref = _tick(off, d)
    _same(_tick(on, d), ref, "before configure")
    assert on.stat("wave_order_slices") == _slices(B)
    on.configure(cfgs[0], 0)
    _same(_tick(on, d), ref, "after configure")
    _same(_tick(on, d), ref, "after configure, call 2")
    on.close(); off.close()
