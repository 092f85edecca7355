"""CPU: time steps other than 2 ms, the oracle and the host restatements alone (dt_cases.py).

  the oracle off 2 ms   oracle.tick against the exact rational optimum of oracle.assemble's data at every step of DTS
  the doubling law      assemble at dt and at 2 dt: which rows double, which stay, bit for bit (the law the device is held to as well)
  working sets          the quarter step moves the oracle's iteration counts: the other steps are other QPs, not the 2 ms one rescaled
  gradients             the central-difference checks of tick_gradients and tick_state_gradients at two more steps
  the mirror's dt       RobotModel's pace_realtime branch measures dt on a scripted clock and hands that number to the tick"""
import types

import numpy as np
import pytest

import common
import dt_cases as dc
import test_tick_grad_host as tgh
import test_tick_grad_q_host as tgqh

DT0, DTS, B0 = dc.DT0, dc.DTS, dc.B0
ORACLE_EXACT_TOL = 1e-11     # measured: 3.6e-14 (c3), 1.1e-14 (full) at worst over the steps


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cfg_name", ["c3", "full"])
def test_oracle_against_the_exact_optimum(cfg_name, dt):
    B = 8
    models, cfgs, d, mid = dc.problem(dc.ONE, cfg_name, B, 71)
    nv = models[0].nv
    a, t = dc.assembled(dc.ONE, cfg_name, dt, B, 71), dc.reference(dc.ONE, cfg_name, dt, B, 71)
    assert (t["status"] == 0).sum() >= B - 4
    worst = 0.0
    for b in np.flatnonzero(t["status"] == 0):
        x = common.exact_ls_optimum(a["A"][b][:, :nv], a["b"][b], a["C"][b][:, :nv], a["lb"][b][:nv], a["ub"][b][:nv], a["Clb"][b], a["Cub"][b],
                                    t["qdot"][b][:nv])
        worst = max(worst, np.abs(t["qdot"][b][:nv] - x).max())
    dc.report("oracle against the exact optimum", cfg_name, dt, worst, ORACLE_EXACT_TOL)
    assert worst < ORACLE_EXACT_TOL


@pytest.mark.parametrize("dt", dc.LAW_DTS)
@pytest.mark.parametrize("names", [dc.ONE, dc.THREE], ids=["one", "three"])
@pytest.mark.parametrize("cfg_name", list(dc.ROW_CLASSES))
def test_doubling_law_on_the_oracle(cfg_name, names, dt):
    live = dc.check_doubling_law(dc.assembled(names, cfg_name, dt), dc.assembled(names, cfg_name, 2 * dt), cfg_name,
                                 "oracle, %s, dt %.7g" % (cfg_name, dt))
    doubled = 2 * dc.ROW_CLASSES[cfg_name]["box"].count("D") + 3      # every doubled box row of Clb and Cub, the gripper's linear rows of b
    assert live >= doubled, (live, doubled)
    # the mixed rows are mixed: neither equal nor doubled
    a1, a2 = dc.assembled(names, cfg_name, dt), dc.assembled(names, cfg_name, 2 * dt)
    for r, c in enumerate(dc.ROW_CLASSES[cfg_name]["b"]):
        if c == "M":
            assert (a1["b"][:, r] != a2["b"][:, r]).any() and (a1["b"][:, r] != 2.0 * a2["b"][:, r]).any(), r


@pytest.mark.parametrize("names", [dc.ONE, dc.TWO, dc.THREE], ids=["one", "two", "three"])
@pytest.mark.parametrize("cfg_name", dc.TICK_CONFIGS)
def test_the_oracle_solves_every_step(cfg_name, names):
    """what keeps test_gpu_dt.py from passing on nothing: at least B - 4 instances solved at every (configuration, dt)"""
    for dt in DTS:
        n = int((dc.reference(names, cfg_name, dt)["status"] == 0).sum())
        assert n >= B0 - 4, (cfg_name, dt, n)


@pytest.mark.parametrize("cfg_name", ["c3", "everything"])
def test_the_quarter_step_moves_the_working_sets(cfg_name):
    r0, r1 = dc.reference(dc.THREE, cfg_name, DT0), dc.reference(dc.THREE, cfg_name, 0.0005)
    moved = int((r0["iters"] != r1["iters"]).sum())
    print("%s: the oracle's iteration count at 0.0005 differs from the one at 0.002 on %d of %d instances" % (cfg_name, moved, B0))
    assert moved >= B0 / 4


@pytest.mark.parametrize("dt", dc.GRAD_DTS)
@pytest.mark.parametrize("cfg_name,model_name", [("everything", "a1_wx200"), ("c3_trunk_task", "laikago_vx300")])
def test_gradient_algebra_at_other_steps(cfg_name, model_name, dt):
    """the central-difference checks of test_tick_grad_host.py and test_tick_grad_q_host.py, their step-size rule and bounds, at step dt"""
    tgh.algebra_check(cfg_name, model_name, dt)
    tgqh.algebra_check(cfg_name, model_name, dt)


# ---- the mirror's measured dt (Robot_Wrapper4.py _pace: the reference's busy-wait, :1337-1342)
class _Clock:
    """time.time() scripted: call n returns t0 + n tick"""

    def __init__(self, t0, tick):
        self.t0, self.tick, self.calls = t0, tick, 0

    def __call__(self):
        self.calls += 1
        return self.t0 + self.calls * self.tick


class _RecordingBatch:
    """stands in for WbcBatch: records the dt every call was given"""

    def __init__(self):
        self.dts = []

    def configure(self, cfg):
        pass

    def tick(self, inputs, dt, **kw):
        self.dts.append(("tick", dt))
        return dict(qdot=np.zeros((1, 26)), q_next=np.zeros((1, 27)), status=np.zeros(1, np.int32), iters=np.zeros(1, np.int32),
                    working_set=np.zeros((1, 2), np.int64))


def _mirror(step_time):
    import Robot_Wrapper4
    rm = object.__new__(Robot_Wrapper4.RobotModel)          # (no handle, no GPU: only what _pace and _solve_tick read)
    rm.step_time, rm.dt, rm.pace_realtime, rm.previous_time = step_time, step_time, True, 0
    rm._bt = _RecordingBatch()
    rm._model = types.SimpleNamespace(nv=26, nq=27)
    rm._tick_inputs = lambda target_EE, target_trunk: {}
    rm.hotstart, rm.firstQP, rm._working_set, rm.q_vel = True, True, None, None
    return rm, Robot_Wrapper4


def test_the_mirror_measures_dt_inside_its_busy_wait(monkeypatch):
    """With time.time() advancing 0.71 ms per call from T0 and previous_time = T0: the loop's condition reads 0.71 ms (< 2 ms), its body sets
    dt = 1.42 ms, the condition reads 2.13 ms and ends the wait — dt is the LAST value measured inside the wait, 1.42 ms, not step_time, and
    that number is what the tick gets. A tick that comes late (the condition false at once) keeps the dt of the tick before, as the
    reference does."""
    T0, TICK = 1000.0, 0.00071
    rm, module = _mirror(0.002)
    clock = _Clock(T0, TICK)
    monkeypatch.setattr(module.time, "time", clock)
    rm.previous_time = T0
    rm._pace()
    want = (T0 + 2 * TICK) - T0
    assert clock.calls == 4 and rm.dt == want and rm.dt != rm.step_time and 0.0014 < rm.dt < 0.0015
    assert rm.previous_time == T0 + 4 * TICK
    rm._solve_tick(None, None, None)
    assert rm._bt.dts == [("tick", want)]
    # a late tick: 3 ms since the last one
    clock.t0, clock.calls = rm.previous_time + 0.003, 0
    rm._pace()
    assert clock.calls == 2 and rm.dt == want
    rm._solve_tick(None, None, None)
    assert rm._bt.dts[-1] == ("tick", want)
    # pace_realtime off: the fixed step
    rm.pace_realtime = False
    rm._pace()
    rm._solve_tick(None, None, None)
    assert rm.dt == 0.002 and rm._bt.dts[-1] == ("tick", 0.002)
