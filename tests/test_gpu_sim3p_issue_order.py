"""The packed sim3 kernel issues some of its work earlier than the statement order suggests: the wave order's atomic goes out
at the end of the dual loop and is waited for at the end of the kernel (wo_post / wo_finish), and the FK seed's sines and cosines share one
block. No operation changed its operands, so every result is bit for bit what it was: the wave order on against off, every kind of variant
(all of them run the seed; the ones whose bounds a hoist ahead of the FK sweep would have treated differently — tried, measured slower, not
shipped) against the oracle at the tolerance tests/test_gpu_parity.py holds its configuration to, and two batches against outputs recorded
from the build before the change (tests/golden/sim3p_issue_order.npz, made by tools/make_issue_order_golden.py)."""
import copy
import json
import os

import numpy as np
import pytest

import common
import oracle
import wbc_capi as capi
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
QDOT_TOL = 1e-5          # test_gpu_parity.py: the bound of BASELINE.json for q̇ (c3, WARM, the trunk task, custom posture + q_con, rotated placements, Laikago)
REFINED_TOL = 1e-7       # test_gpu_parity.py test_tick_parity_posture_modes: c3_hybrid and c3_mani against the oracle (both refine)
BAR_EXP = 3              # option presolve_tol_exp (test_gpu_sim3p_cold_paths.py): |det K| <= 1e-3 (sum |K|)^3 counts as rank deficient
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3p_issue_order.npz")
OUT = ("qdot", "status", "iters")


@pytest.fixture(scope="module")
def wx200():
    return wbc_model.load_model("a1_wx200")


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


def _handle(model, cfg, B, wave_order=None, options=None):
    bt = WbcBatch(model, B)
    bt.configure(cfg)
    for k, v in (options or {}).items():
        bt.set_option(k, v)
    if wave_order is not None:
        bt.set_option("wave_order", wave_order)
    return bt


def _bits_equal(a, b, what, keys=OUT):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs in %d instances" % (
            what, k, int((x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1).sum()))


def _slices(B):
    """slices of waves (wbc_device.h WO_SW = 127 waves per slice)"""
    return -(-(-(-B // 4)) // 127)


def _classes(dual_iters):
    """wbc_packed.h wo_class of instances the tail does not redo: 0 the heaviest (>= 10 dual iterations) .. 5 (none)"""
    it = np.asarray(dual_iters)
    return np.where(it >= 10, 0, np.where(it >= 6, 1, np.where(it >= 3, 2, 5 - it)))


def _recorded_order_moves_someone(iters, n_eq, B):
    """Does the order a launch with these iteration counts records differ from the identity? A slice's order is its instances by class, heaviest
    first (inside a class: as the waves arrive); wave grp is wave grp // ns of slice grp % ns and takes positions 4 k .. 4 k + 3 of it. If the
    classes of a slice's instances, in position order, are not already ascending, some wave of the slice gets other instances than its own."""
    ns = _slices(B)
    cls = _classes(np.asarray(iters) - n_eq)
    for g in range(ns):
        members = np.concatenate([np.arange(4 * w, min(4 * w + 4, B)) for w in range(g, -(-B // 4), ns)])
        if (np.diff(cls[members]) < 0).any():
            return True
    return False


# seeds of the C3 stress recipe at which the first tick's classes are out of order (checked below on the device's own iteration counts)
@pytest.mark.parametrize("B,seed", [(5, 3), (515, 3)])
def test_wave_order_with_the_early_atomic(wx200, B, seed):
    """wave_order 2 (the order at every batch size), C3 stress recipe, three consecutive ticks on one handle — the first on the inputs as drawn,
    the second and third on a permutation of them (the order recorded by the tick before predicts nothing, then is right again). B = 5: two
    waves, the last with one valid row; B = 515: 129 waves in two slices. After each tick every slice has published, and qdot, status and iters
    are those of the same ticks with the order off, bit for bit. That the order in effect from tick 2 on is not the identity is read off tick 1's
    iteration counts; tick 2's outputs landing where the order-off handle puts them is then the check that the recorded order is followed."""
    cfg = common.config("c3", wx200)
    d = common.tick_inputs(wx200, cfg, B, seed=seed, stress=True)
    perm = np.random.default_rng(7).permutation(B)
    dp = {k: v[perm] for k, v in d.items()}
    a = oracle.assemble([wx200], [cfg], d, DT, B)
    n_eq = int(((a["lb"] == a["ub"]).sum(axis=1) + (a["Clb"] == a["Cub"]).sum(axis=1))[0])   # contact rows + locked DoF: counted in iters, not dual iterations
    on, off = _handle(wx200, cfg, B, 2), _handle(wx200, cfg, B, 0)
    for tick, inp in enumerate((d, dp, dp), start=1):
        ref = off.tick(inp, DT)
        got = on.tick(inp, DT)
        assert on.stat("last_path") == 2 and off.stat("last_path") == 2
        assert on.stat("wave_order_slices") == _slices(B) and off.stat("wave_order_slices") == 0
        _bits_equal(got, ref, "B = %d, tick %d" % (B, tick))
        if tick == 1:
            print("B = %d: dual iterations %d..%d" % (B, ref["iters"].min() - n_eq, ref["iters"].max() - n_eq))
            assert _recorded_order_moves_someone(ref["iters"], n_eq, B), "tick 1 records the identity order: choose another seed"
    on.close(); off.close()


def _leg_block_ratio(a):
    """min over the four stance feet of |det K| / (sum |K_ij|)^3 (test_gpu_sim3p_cold_paths.py)"""
    r = np.full(a["C"].shape[0], np.inf)
    for f, d0 in enumerate((9, 6, 15, 12)):
        K = a["C"][:, 4 + 3 * f:7 + 3 * f, d0:d0 + 3]
        r = np.minimum(r, np.abs(np.linalg.det(K)) / np.abs(K).sum(axis=(1, 2)) ** 3)
    return r


def test_tail_and_class_zero(wx200):
    """B = 8 with one rank-deficient stance leg (under the raised bar) plus dbg_force_defer: that instance is redone by its wave's tail and
    recorded in class 0. Two ticks with the order on: bit-identical to the order off, status as the oracle's."""
    B = 8
    cfg = common.config("c3", wx200)
    pool = common.tick_inputs(wx200, cfg, 512, seed=123)
    ratio = _leg_block_ratio(oracle.assemble([wx200], [cfg], pool, DT, 512))
    bar = 10.0 ** -BAR_EXP
    flagged, plain = np.flatnonzero(ratio < 0.5 * bar), np.flatnonzero(ratio > 2.0 * bar)
    idx = plain[:B].copy()
    idx[5] = flagged[0]
    d = {k: v[idx] for k, v in pool.items()}
    ref = oracle.tick([wx200], [cfg], d, DT, B, nthreads=8)
    opts = {"presolve_tol_exp": BAR_EXP, "dbg_force_defer": 1}
    on, off = _handle(wx200, cfg, B, 2, opts), _handle(wx200, cfg, B, 0, opts)
    for tick in (1, 2):
        want = off.tick(d, DT)
        got = on.tick(d, DT)
        assert off.stat("deferred_last") == 1 and on.stat("deferred_last") == 1
        assert on.stat("wave_order_slices") == 1
        _bits_equal(got, want, "tail, tick %d" % tick)
        assert (got["status"] == ref["status"]).all()
    on.close(); off.close()


def _against_oracle(got, ref, tol, what, min_ok=0.9):
    assert (got["status"] == ref["status"]).all(), what
    ok = ref["status"] == 0
    assert ok.mean() > min_ok, what
    err = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    print("%s: qdot max-abs err vs oracle %.3e" % (what, err))
    assert err < tol, what
    assert np.abs(got["q_next"] - ref["q_next"])[ok].max() < 1e-7, what
    return ok


@pytest.mark.parametrize("case", ["cold", "warm", "trunk", "qcon_mani", "static_hybrid", "laikago", "rotated", "tp_refused_row"])
def test_every_kind_of_variant_against_the_oracle(wx200, case):
    """B = 64 on every kind of variant: cold and WARM, TRUNK (its own front block ahead of the seed), QCON (MANI posture: a second seed and
    sweep at q_con, whose bounds belong to that state), static HYBRID (the post_static block perturbs the state the dampers see), the Laikago
    model (rotated placements; its sim3 tick runs on the general kernel's ROT instantiation) and the rotated a1_wx200 (the packed kernel's
    ROT instantiation), per-instance rows with one refused."""
    B = 64
    model = {"laikago": lambda: wbc_model.load_model("laikago_vx300"), "rotated": _rotated_wx200}.get(case, lambda: wx200)()
    cfg_name = {"trunk": "c3_trunk_task", "qcon_mani": "c3_mani", "static_hybrid": "c3_hybrid"}.get(case, "c3")
    tol = REFINED_TOL if case in ("qcon_mani", "static_hybrid") else QDOT_TOL
    cfg = common.config(cfg_name, model)
    d = common.tick_inputs(model, cfg, B, seed=23, with_rot=(case == "trunk"))
    ref = oracle.tick([model], [cfg], d, DT, B, nthreads=8)
    bt = _handle(model, cfg, B)
    kw = {}
    if case == "warm":        # seeded with the cold run's own working sets
        ws = np.asarray(bt.tick(d, DT, want_working_set=True)["working_set"])
        d = dict(d, working_set=ws)
        kw["want_working_set"] = True
    if case == "tp_refused_row":
        rows = wbc_model.task_params(cfg, B)
        rows[9, :] = np.nan
        kw["task_params"] = rows
    got = bt.tick(d, DT, want_q_next=True, **kw)
    assert bt.stat("last_path") == (0 if case == "laikago" else 2)
    if case == "tp_refused_row":
        assert got["status"][9] == capi.QP_NUMERICAL and (got["qdot"][9] == 0.0).all()
        keep = np.arange(B) != 9
        got, ref = {k: np.asarray(v)[keep] for k, v in got.items()}, {k: np.asarray(v)[keep] for k, v in ref.items()}
    _against_oracle(got, ref, tol, case)
    bt.close()


@pytest.mark.parametrize("case", ["cold", "static_hybrid"])
def test_bit_identical_to_the_recorded_outputs(wx200, case):
    """The fixture holds the inputs of a B = 64 batch and what the build before the issue-order change returned for it (default options, with
    q_next): the same bits come back."""
    z = np.load(GOLDEN)
    cfg = common.config("c3" if case == "cold" else "c3_hybrid", wx200)
    d = {k[len(case) + 4:]: z[k] for k in z.files if k.startswith(case + "_in_")}
    want = {k[len(case) + 5:]: z[k] for k in z.files if k.startswith(case + "_out_")}
    B = len(d["q"])
    assert B == 64 and set(want) == {"qdot", "status", "iters", "q_next"}
    bt = _handle(wx200, cfg, B)
    got = bt.tick(d, DT, want_q_next=True)
    assert bt.stat("last_path") == 2
    _bits_equal(got, want, case, keys=("qdot", "status", "iters", "q_next"))
    bt.close()
