"""The velocity damper's zones, on the CPU: the conditions on the INPUTS that keep test_gpu_damper_envelope.py honest, held with
the oracle alone — it solves them, every DoF class has active bounds in the regular and in the flipped zone, both "exactly" kinds are in the
batch, its q̇ answers to a 1e-4 change of damper_qs, and its lb / ub are the literal transcription's; the finding that made the new inputs
necessary, pinned on the old ones; and the state gradient's host restatement on the new ones (algebra and end to end), where its un-flipped
derivative branch is weighed for the first time. A case that misses a condition gets another recipe, never another threshold."""
import numpy as np
import pytest

import common
import damper_cases as dc
import oracle
import pose_cases as pc
import test_tick_grad_q_host as tq

REG, FLIP, BEYOND, EDGE, AT_QS = range(5)      # common.DAMPER_KINDS
MIN_ACTIVE = 3                                  # solved instances with an active bound, per DoF class and zone
CASES = [(n, c) for n in dc.TICK_CASES for c in dc.MAPS]


# ------------------------------------------------------------------------------------------------ 1. the gap itself, on the old inputs
@pytest.mark.parametrize("compat", dc.MAPS)
def test_the_stress_inputs_never_hold_an_active_regular_zone_bound(compat):
    """A property of tick_inputs(stress=True) (`c3`, seed 21, B = 256), not of the product: the stress recipe puts one arm DoF 0 - 10 mrad from
    a limit, below damper_qs = 15 mrad, so what is active there is the sign-flipped band 0 <= d < qs. No bound of the regular zone qs < d <= qi
    (the damper as designed) is active in any solution, and no base DoF is in any zone — which is why those inputs cannot stand in for
    common.damper_tick_inputs."""
    m = pc.model("wx200")
    cfg = dc.config("c3", m, compat)
    B = 256
    d = common.tick_inputs(m, cfg, B, seed=21)
    ref = oracle.tick([m], [cfg], d, pc.DT, B, nthreads=8)
    asm = oracle.assemble([m], [cfg], d, pc.DT, B)
    zone, active = dc.zones_and_active([m], [cfg], None, d["q"], asm, ref)
    in_reg = int((zone == REG).any(axis=(1, 2)).sum())
    act_reg, act_flip = int((active & (zone == REG)).sum()), int((active & (zone == FLIP)).any(axis=(1, 2)).sum())
    print("stress inputs, %s map: %d of %d instances have a DoF in the regular zone, %d active regular-zone bounds, %d instances with an active "
          "flipped-zone bound, base DoF in a zone: %d" % ("reference" if compat else "corrected", in_reg, B, act_reg, act_flip, (zone[:, :6] >= 0).sum()))
    assert (ref["status"] == 0).all()
    assert act_reg == 0 and in_reg <= 1
    assert act_flip >= 10
    assert (zone[:, :6] < 0).all()
    if not compat:
        assert (zone[:, 6:18] < 0).all()        # under the corrected map no leg DoF leaves -+v_max either


# ------------------------------------------------------------------------------------------------ 2. the conditions, case by case
@pytest.mark.parametrize("name,compat", CASES)
def test_the_oracle_solves_the_damper_cases_and_every_class_and_zone_is_active(name, compat):
    p = dc.tick_problem(name, compat)
    case, zone, active, ref = p["case"], p["zone"], p["active"], p["ref"]
    mixed = case.get("fates") == "mixed"
    solved, moved = dc.observability(p)
    cov = dc.coverage(p)
    classes = dc.classes_of(p)
    lb, ub = dc.literal_bounds(p)
    e_lit = max(np.abs(p["asm"]["lb"] - lb).max(), np.abs(p["asm"]["ub"] - ub).max())
    in_batch = {k: int((zone == i).any(axis=(1, 2)).sum()) for i, k in enumerate(common.DAMPER_KINDS)}
    qdep = dc.q_dependent(p)
    print("%s, %s map: solved %d/%d (%.3f); active bounds by class: %s; instances holding each kind: %s; up to %d active q-dependent bounds in one "
          "instance; damper_qs + 1e-4 moves qdot by > %.0e on %.3f of the solved; |oracle lb, ub - literal| %.1e" % (
              name, "reference" if compat else "corrected", (ref["status"] == 0).sum(), p["B"], solved,
              ", ".join("%s %d regular / %d flipped" % (c, cov[c, "regular"], cov[c, "flipped"]) for c in common.DAMPER_CLASSES),
              in_batch, qdep.max(), dc.QDOT_TOL, moved, e_lit))
    if mixed:                                                            # mixed fates: both fates are there, and the leg class the must-solve case leaves out
        assert 0.5 < solved < 1.0
        classes = ("leg",)
    else:
        assert solved >= 0.9, (name, solved)
    for c in classes:
        for k in ("regular", "flipped"):
            assert cov[c, k] >= MIN_ACTIVE, (name, compat, c, k, cov[c, k])
    assert in_batch["edge"] >= 1 and in_batch["qs"] >= 1 and in_batch["beyond"] >= 1
    assert moved >= 0.4, (name, moved)
    assert e_lit < 1e-13, (name, e_lit)
    assert qdep.max() <= 8                                               # (working sets at the packed kernels' capacity are not this file's)
    if "base" in classes or mixed:                                       # the far instance: base x 6 m beyond its limit, clamped at -v_max, then flipped
        b = p["B"] - 1
        assert p["q_int"][b, 0] == common.DAMPER_FAR_X and zone[b, 0, 1] == BEYOND
        assert p["asm"]["ub"][b, 0] == p["cfgs"][0].damper_vmax[0] and p["asm"]["lb"][b, 0] == -p["cfgs"][0].damper_vmax[0]


@pytest.mark.parametrize("compat", dc.MAPS)
def test_bounds_at_d_equal_qs_are_zero_to_an_ulp_of_the_limit(compat):
    """d = qs formed as lo + qs / hi - qs. The code computes (c - lo) - qs: c - lo is exact, but lo + qs was rounded at the LIMIT's magnitude
    (2e-16 at 1 rad, 9e-16 at 5 m), so the bound is not 0 but coef / (qi - qs) times that rounding error, of either sign before the flip: with
    these models' limits no coordinate gives a bound of exactly 0 (lo + qs would have to be a double). What the kind reaches is the flip deciding
    on a number of ulp size — a device that formed the difference in another order would land on the other side of it, at the same |value|."""
    p = dc.tick_problem("c3", compat)
    at = p["zone"] == AT_QS
    vals = np.concatenate([p["asm"]["lb"][at[:, :, 0]], p["asm"]["ub"][at[:, :, 1]]])
    print("bounds at d = qs, %s map: %d, of which %d exactly zero; largest |bound| %.1e" % (
        "reference" if compat else "corrected", len(vals), (vals == 0).sum(), np.abs(vals).max()))
    assert len(vals) >= 10 and np.abs(vals).max() < 0.01 / 0.011 * 2.0 ** -50


# ------------------------------------------------------------------------------------------------ 3. the state gradient's host restatement
def _inputs(compat, **kw):
    def make(m, cfg_name, B, seed):
        cfg = dc.config(cfg_name, m, compat)
        return cfg, common.damper_tick_inputs(m, cfg, B, seed, edges=False, with_rot=True, **kw)
    return make


@pytest.mark.parametrize("compat", dc.MAPS)
@pytest.mark.parametrize("model_name", tq.MODELS)
@pytest.mark.parametrize("cfg_name", ["c3", "everything", "full"])
def test_algebra_on_damper_inputs(cfg_name, model_name, compat):
    """test_tick_grad_q_host.algebra_check as it stands (its step, its tolerance) on damper_tick_inputs(edges=False), B = 8: the sensitivities
    are random on all 26 bounds and both sides, so every DoF in a zone weighs its branch of the derivative — the un-flipped one included"""
    m, cfg, d = tq.algebra_check(cfg_name, model_name, inputs=_inputs(compat), B=8)
    zone = common.damper_zones(cfg, m.nv, d["q"])
    n = {k: int((zone == i).sum()) for i, k in enumerate(common.DAMPER_KINDS[:3])}
    print("  DoF sides in a zone: %s" % n)
    assert n["regular"] >= 3 and n["flipped"] >= 2


@pytest.mark.parametrize("cfg_name,seed", [("c3", 3), ("full", 3)])
def test_end_to_end_on_damper_inputs_with_active_regular_zone_bounds(cfg_name, seed):
    """the end-to-end directional check as it stands (its tolerance rule, at most B // 4 instances left out) on damper_tick_inputs(edges=False)
    under the corrected index map; and at least 4 of the kept instances hold an active regular-zone bound"""
    m, cfg, d, keep, t0, a0, side0 = tq.end_to_end_check(cfg_name, "damper", seed, inputs=_inputs(False))
    zone, active = dc.zones_and_active([m], [cfg], None, d["q"], a0, t0)
    n = int(((active & (zone == REG)).any(axis=(1, 2)) & keep).sum())
    nf = int(((active & (zone == FLIP)).any(axis=(1, 2)) & keep).sum())
    print("  kept instances with an active regular-zone bound: %d, with an active flipped-zone bound: %d" % (n, nf))
    assert n >= 4
