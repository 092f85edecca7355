"""One long-lived WbcBatch handle through every switch set and entry point.

A handle keeps, between calls, its host-staging workspace, a dozen lazily allocated device workspaces (status, deferred list and its tail words,
the deferred statistic and its launch sequence, the wave order, the posture targets, the roll-out / score / watch state), the per-model
configurations and plans, and the last_* statistics. Here one handle per model mix walks through the warm-up switch set, c3, c3_trunk_task,
"everything", c2, the MANI / HYBRID sets, the general-kernel sets and the one-instance compact kernel, with batch sizes 67 -> 5 -> 66 -> 1 -> 67
under max_batch 70, alternating host arrays and torch device tensors on a side stream, with refused calls in between. The rule of every step:
every output (key set, dtype, shape, bytes) and every statistic the call sets equal what the same call returns on a FRESH handle — created,
configured, given the same options, called once, closed. No tolerance: include/wbc.h promises that no knob and no order changes a result.
Every fresh reference is itself held to the CPU oracle (tick_grad, state_slack: to the numpy restatement) at the bound of the test that
already makes that call (handle_walk.hold), and the conditions under which a step means something are asserted there and here.

Mixes: (A) a1_wx200 + a1_px100_pin_ver + laikago_vx300 interleaved by model_id (nv 26 / 25 / 25, the ROT variants); (B) a1_wx200 alone
without model_id (the FIXD form); (C) a1_wx200 + a1_px100_pin_ver. The packed sim3 / INEQ-orth / box plans decline the Laikago model
(test_gpu_laikago.PATHS), so (A) walks the general kernel's ROT instantiations (and the packed orth kernel under c2) through the same
route; (B) and (C) reach every path, and the deferred lists and the wave order exist there.

The second test settles wbc_batch_configure against work in flight (include/wbc.h): a device-mode roll-out enqueued before a configure
runs to its end under the old configuration."""
import itertools

import numpy as np
import pytest
import torch

import handle_walk as hw
import wbc_capi as capi
import wbc_model

pytestmark = pytest.mark.gpu

FULL = ("tick", "tick_qdot_only", "tick_tp", "assemble", "tick_grad", "rollout", "qp32", "rollout_shift", "update_state", "state_slack", "fk", "integrate",
        "qp12", "rollout_warmup_rot")
C3_EXTRA = ("rollout_traj", "rollout_tracks", "rollout_watch", "tick")
LIGHT = ("tick", "tick_tp", "assemble", "rollout", "qp12", "tick_qdot_only")
POSTURE = ("tick", "posture_target", "assemble", "tick_grad", "rollout", "tick_tp")


class Walk:
    """the long-lived handle of one mix: its current switch set and options, the batch-size and memory-kind cycles, what differed so far"""

    def __init__(self, mix, base_options=None):
        self.mix, self.bt = mix, hw.new_handle(mix)
        self.options = dict(hw.DEFAULTS)
        self.cfg_name = None
        self.batches = itertools.cycle(hw.BATCHES)
        self.host, self.device = hw.Host(), hw.Device()
        self.mems = itertools.cycle((self.host, self.device))
        self.wrong, self.steps, self.paths, self.fixd = [], [], set(), set()
        self.opt(**(base_options or {}))

    def opt(self, **kw):
        for k, v in kw.items():
            self.bt.set_option(k, v)
            self.options[k] = v

    def defaults(self, keep=()):
        self.opt(**{k: v for k, v in hw.DEFAULTS.items() if k not in keep})

    def configure(self, cfg_name, only=None):
        """the switch set on every model of the handle, one wbc_batch_configure per model (only: that model index alone)"""
        p = hw.problem(self.mix, cfg_name)
        for i, c in enumerate(p["cfgs"]):
            if only is None or i == only:
                self.bt.configure(c, i)
        if only is None:
            self.cfg_name = cfg_name

    def _record(self, call, B, mem, got, want):
        bad = hw.differences(got, want)
        name = "%s %s %s B=%d %s %s" % (self.mix, self.cfg_name, call, B, type(mem).__name__, dict(hw.option_key(self.options)))
        self.steps.append(name)
        if bad:
            self.wrong.append((name, bad))
        if "last_path" in got[1]:
            self.paths.add(got[1]["last_path"])
            self.fixd.add(got[1]["last_tick_fixd"])
        return got

    def call(self, call, B=None, mem=None, cfg_name=None):
        B = next(self.batches) if B is None else B
        mem = next(self.mems) if mem is None else mem
        cfg_name = cfg_name or self.cfg_name
        got = mem.run(self.bt, cfg_name, call, B)
        return self._record(call, B, mem, got, hw.fresh(self.mix, cfg_name, hw.option_key(self.options), call, B, mem))

    def calls(self, names):
        for c in names:
            self.call(c)

    # ---- refused calls: each leaves the handle as it was; the caller makes the next good call
    def refuse_batch_71(self):
        d = {k: np.concatenate([v, v[:1]]) for k, v in hw.problem(self.mix, self.cfg_name)["d"].items()}
        with pytest.raises(capi.WbcError, match="max_batch"):
            self.bt.tick(d, hw.DT)                                   # the wrapper's own check
        self.bt.max_batch = hw.MAX_BATCH + 1                         # ... and, past it, the library's
        try:
            with pytest.raises(capi.WbcError, match="max_batch = %d" % hw.MAX_BATCH):
                self.bt.tick(d, hw.DT)
        finally:
            self.bt.max_batch = hw.MAX_BATCH

    def refuse_missing_box(self):
        d = {k: v[:66] for k, v in hw.problem(self.mix, self.cfg_name)["d"].items() if k != "trunk_box_center"}
        with pytest.raises(capi.WbcError, match="trunk_box_center"):
            self.bt.tick(d, hw.DT)

    def refuse_watch_mask_0(self):
        p = hw.problem(self.mix, self.cfg_name)
        self.bt._watch_struct = lambda *a, **k: capi.WbcSlackWatch()     # a watch that names no family
        try:
            with pytest.raises(capi.WbcError, match="mask"):
                self.bt.rollout_watch({k: v[:67] for k, v in p["d"].items()}, hw.DT, hw.K, watch=("com",))
        finally:
            del self.bt._watch_struct

    def move_to(self, cfg_name):
        """to the next switch set one model at a time; with several models a tick in between is refused (the models disagree)"""
        if len(hw.MIXES[self.mix]) > 1:
            self.configure(cfg_name, only=0)
            d = {k: v[:67] for k, v in hw.problem(self.mix, self.cfg_name)["d"].items()}
            with pytest.raises(capi.WbcError, match="share the task/constraint switches"):
                self.bt.tick(d, hw.DT)
        self.configure(cfg_name)

    def close(self):
        self.bt.close()


def _route(w):
    """the walk of the module docstring on Walk w (any mix, any base options)"""
    base = dict(w.options)
    keep = tuple(k for k, v in base.items() if hw.DEFAULTS[k] != v)       # the run's own options stay through every "back to the defaults"
    packed = hw.PACKED[w.mix]
    # 1. the warm-up switch set (packed box kernel, path 4), left on the handle; then straight to c3 (packed sim3, path 2)
    w.cfg_name = "full"
    w.call("warm_up", B=67, mem=w.host)
    w.calls(("tick", "rollout", "tick_tp"))
    w.configure("c3")
    w.calls(FULL + C3_EXTRA)
    w.configure("c3+w")                                         # the same switch set with other weights and gains (what a gain sweep through
    w.calls(("tick", "tick_tp", "assemble", "tick_grad", "rollout"))   # RobotModel does): every model index's configuration is replaced
    w.configure("c3")
    w.refuse_batch_71()
    w.call("tick")
    w.refuse_watch_mask_0()
    w.calls(("rollout_watch", "rollout"))
    # 2. the trunk task on top (the packed kernel's TRUNK variant: a.packed_trunk from cfg_host[0]; FIXD no longer)
    w.move_to("c3_trunk_task")
    w.calls(FULL)
    w.refuse_missing_box()
    w.call("tick")
    # 3. every task and constraint (packed orth kernel's INEQ variant, path 3)
    w.opt(packed_orth=2)
    w.move_to("everything")
    w.calls(FULL)
    # 4. equality-only: the general kernel under the default batch policy, then the packed orth kernel
    w.opt(packed_orth=1)
    w.move_to("c2")
    w.calls(LIGHT)
    w.opt(packed_orth=2)
    w.calls(LIGHT)
    w.opt(packed_orth=1)
    # 5. MANI (posture kernel into d_pu / d_pq + the QCON variant), HYBRID, a PREV set in between, MANI again at another batch size
    w.move_to("c3_mani")
    w.calls(POSTURE)
    w.configure("c3_hybrid")                                    # (the same switches as MANI and c3: no tick in between would be refused)
    w.calls(POSTURE)
    w.configure("c3")
    w.calls(("tick", "rollout"))
    w.configure("c3_mani")
    w.calls(("tick", "rollout", "tick"))
    # 6. the general kernel, with and without the structural presolve
    w.move_to("hybrid_grip_com")
    w.calls(LIGHT[:4])
    w.move_to("c3_two_feet")
    w.calls(LIGHT)
    w.opt(presolve=0)
    w.calls(LIGHT[:4])
    w.opt(presolve=1)
    # 7. the one-instance compact kernel and its second pass (path 1), then a non-empty deferred list on it and on the packed path
    w.move_to("c3")
    w.opt(packed_kernel=0, refine=0)
    w.calls(("tick", "tick_qdot_only", "rollout", "tick"))
    w.opt(presolve_tol_exp=3, dbg_force_defer=1)
    for B in (67, 66):
        got = w.call("tick", B=B, mem=w.host)
        assert not packed or (got[1]["last_path"] == 1 and hw.fresh(w.mix, "c3", hw.option_key(w.options), "tick", B, w.host)[1]["deferred_last"] > 0)
    w.opt(packed_kernel=1, refine=1)
    for B in (67, 5):
        got = w.call("tick", B=B, mem=w.device)
        assert not packed or (got[1]["last_path"] == 2 and hw.fresh(w.mix, "c3", hw.option_key(w.options), "tick", 67, w.device)[1]["deferred_last"] > 0)
    # 8. the options back to the defaults: the next plain ticks equal fresh, nothing deferred
    w.defaults(keep)
    for mem in (w.host, w.device):
        got = w.call("tick", B=67, mem=mem)
        assert got[1]["deferred_last"] == 0 and got[1]["last_path"] == (2 if packed else 0)
    w.calls(FULL[:8] + C3_EXTRA)


def _report(walks):
    wrong = [x for w in walks for x in w.wrong]
    n = sum(len(w.steps) for w in walks)
    print("%d steps compared with fresh handles (%d fresh references held to the oracle); differing: %s" % (n, len(hw._FRESH), wrong or "nothing"))
    assert not wrong, wrong


@pytest.mark.parametrize("mix", ["A", "B", "C"])
def test_every_call_of_the_walk_equals_a_fresh_handle(mix):
    w = Walk(mix)
    try:
        _route(w)
    finally:
        w.close()
    _report([w])
    if hw.PACKED[mix]:
        assert w.paths == {0, 1, 2, 3, 4}, w.paths
        assert w.fixd == ({0, 1} if mix == "B" else {0}), w.fixd   # one model: c3 runs the FIXD form, c3_trunk_task and the rest do not
    else:
        assert 0 in w.paths and not w.paths & {2, 4} and w.fixd == {0}, (w.paths, w.fixd)   # (what test_gpu_laikago.PATHS says of the packed sim3 and box kernels)


@pytest.mark.parametrize("mix", ["A", "B", "C"])
def test_the_walk_with_the_wave_order_and_warm_starts(mix):
    """the whole walk once more with wave_order = 2 and warm_start = 1: the order exists at these batch sizes ((B), (C)) and survives a
    configure of one model index, a change of B and a change of path; the roll-outs carry working sets in d_roll from tick to tick"""
    w = Walk(mix, dict(wave_order=2, warm_start=1))
    try:
        _route(w)
        slices = w.bt.stat("wave_order_slices")
    finally:
        w.close()
    _report([w])
    assert slices == (1 if hw.PACKED[mix] else 0)                   # (the last packed sim3 launch published its order)


def test_two_handles_alive_at_once():
    """(A) under c3_trunk_task and (B) under c3 alternate device-mode calls on two side streams without a synchronisation in between: each
    call equals fresh"""
    wa, wb = Walk("A"), Walk("B")
    try:
        wa.configure("c3_trunk_task")
        wb.configure("c3")
        torch.cuda.synchronize()
        pending = []
        for call, B in (("tick", 67), ("rollout", 66), ("tick_tp", 5), ("rollout_tracks", 67), ("tick", 1), ("tick_grad", 67), ("rollout_watch", 66), ("tick", 67)):
            for w in (wa, wb):
                pending.append((w, call, B) + w.device.launch(w.bt, w.cfg_name, call, B))
        for w, call, B, out, stats in pending:
            got = w.device.finish(w.bt, w.cfg_name, call, out, stats, waiting=False)
            want = hw.fresh(w.mix, w.cfg_name, (), call, B, w.device)
            w._record(call, B, w.device, got, (want[0], {k: v for k, v in want[1].items() if k not in hw.WAITING_STATS}))
    finally:
        wa.close()
        wb.close()
    _report([wa, wb])


# ------------------------------------------------------------------------------------------------ wbc_batch_configure against work in flight
# profiles/r19_ab_rollout_host.txt: a stressed c3 roll-out at B = 64 takes 60 us per tick on the device: IN_FLIGHT_K = 200 ticks last 12 ms.
# The host needs 48.5 us per tick to enqueue them, so on its own the device would be only ~2 ms behind when the call returns (less once the
# closed loop has settled): sweeps over a 1 GiB tensor enqueued ahead of the roll-out on the same stream keep it queued whatever the host's speed.
IN_FLIGHT_K = 200


def test_configure_waits_for_a_rollout_in_flight():
    """Benign by construction: the configure raced is one of the SAME switch set (same sizes, same plan, other weights and gains only)."""
    B = 67
    p = hw.problem("B", "c3")
    cfg = p["cfgs"][0]
    new = hw.other_weights(cfg, fill_zeros=True)                 # the same switch set, every weight and gain of the 85 changed and non-zero
    assert (wbc_model.task_params(new, 1) != 0).all() and (wbc_model.task_params(new, 1) != wbc_model.task_params(cfg, 1)).all()
    dev = hw.Device()
    args = dict(ee_target_step=p["ee_step"][:B] * 0.01, imu=p["imu"][:B], want_trace=False)
    d = {k: v[:B] for k, v in p["d"].items()}

    def fresh(c):
        bt = hw.new_handle("B")
        bt.configure(c)
        out = bt.rollout(d, hw.DT, IN_FLIGHT_K, **args)
        bt.close()
        return out
    old_ref, new_ref = fresh(cfg), fresh(new)
    assert any(old_ref[k].tobytes() != new_ref[k].tobytes() for k in ("q", "qdot"))          # (the weights do reach the answer)
    bt = hw.new_handle("B")
    bt.configure(cfg)
    rows = (bt.task_rows, bt.constraint_rows)
    dd = {k: dev.cv(v) for k, v in d.items()}
    da = dict(args, ee_target_step=dev.cv(args["ee_target_step"]), imu=dev.cv(args["imu"]))
    ballast = torch.zeros(1 << 28, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(dev.stream):
        bt.rollout(dd, hw.DT, 2, **da)                           # (first use: the lazy workspaces are allocated outside the measured call)
        dev.stream.synchronize()
        for _ in range(16):
            ballast.mul_(0.5).add_(1.0)                          # (2 GiB of traffic per kernel: a fraction of a millisecond each)
        got = bt.rollout(dd, hw.DT, IN_FLIGHT_K, **da)
        done = torch.cuda.Event()
        done.record(dev.stream)
    assert not done.query(), "not in flight: raise K"
    bt.configure(new)
    assert (bt.task_rows, bt.constraint_rows) == rows            # the same plan
    torch.cuda.synchronize()
    wrong = [k for k, v in got.items() if v.cpu().numpy().tobytes() != old_ref[k].tobytes()]
    assert not wrong, "the roll-out in flight saw the new configuration: %s" % wrong
    with torch.cuda.stream(dev.stream):
        nxt = bt.rollout(dd, hw.DT, IN_FLIGHT_K, **da)
    dev.stream.synchronize()
    wrong = [k for k, v in nxt.items() if v.cpu().numpy().tobytes() != new_ref[k].tobytes()]
    assert not wrong, "the call after the configure did not see it: %s" % wrong
    bt.close()
