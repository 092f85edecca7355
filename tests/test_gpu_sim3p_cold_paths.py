"""The rarely taken blocks of the packed sim3 kernel (wbc_k_sim3p.hip), which the compiler lays out behind the packed path:
the pivoted elimination of a rank-deficient stance-leg block and its SWAP, the tail with its statistic, drop_slot in the dual iterations and in
the WARM variant's restoration, and the post_static state. Small batches (B = 64: 16 wavefronts) that are sure to enter each block, against the
oracle at the tolerances of test_gpu_parity.py, with the wave order off and on (option wave_order 0 / 2: bit-identical, as
test_gpu_wave_order.py asserts)."""
import numpy as np
import pytest

import common
import oracle
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
B = 64
QDOT_TOL = 1e-5          # test_gpu_parity.py: the bound of BASELINE.json for q̇
REFINED_TOL = 1e-7       # test_gpu_parity.py: a path with the refinement on, against the oracle (which refines too)
BAR_EXP = 3              # option presolve_tol_exp: a leg block with |det K| <= 1e-3 (sum |K|)^3 counts as rank deficient (tools/singular_sweep.py)


@pytest.fixture(scope="module")
def wx200():
    return wbc_model.load_model("a1_wx200")


def _leg_block_ratio(a):
    """min over the four stance feet of |det K| / (sum |K_ij|)^3 (test_gpu_parity.py, tools/singular_sweep.py)"""
    r = np.full(a["C"].shape[0], np.inf)
    for f, d0 in enumerate((9, 6, 15, 12)):
        K = a["C"][:, 4 + 3 * f:7 + 3 * f, d0:d0 + 3]
        r = np.minimum(r, np.abs(np.linalg.det(K)) / np.abs(K).sum(axis=(1, 2)) ** 3)
    return r


@pytest.fixture(scope="module")
def singular(wx200):
    """Two batches drawn from one sample by its leg-block ratios (well clear of the bar on either side): `one` has a flagged instance in row 0 of
    every wavefront and plain ones in the other rows, `all` has flagged instances only. With each: the oracle's answer and the flagged mask."""
    cfg = common.config("c3", wx200)
    d = common.tick_inputs(wx200, cfg, 512, seed=123)
    ratio = _leg_block_ratio(oracle.assemble([wx200], [cfg], d, DT, 512))
    bar = 10.0 ** -BAR_EXP
    flagged, plain = np.flatnonzero(ratio < 0.5 * bar), np.flatnonzero(ratio > 2.0 * bar)
    assert len(flagged) >= B and len(plain) >= B
    idx_one = plain[:B].copy()
    idx_one[::4] = flagged[:B // 4]
    out = {}
    for name, idx in (("one", idx_one), ("all", flagged[:B])):
        sub = {k: v[idx] for k, v in d.items()}
        out[name] = (sub, oracle.tick([wx200], [cfg], sub, DT, B, nthreads=8), ratio[idx] < bar)
    return cfg, out


def _handle(model, cfg, wave_order, options=None):
    bt = WbcBatch(model, B)
    bt.configure(cfg)
    for k, v in (options or {}).items():
        bt.set_option(k, v)
    bt.set_option("wave_order", wave_order)
    return bt


def _both_orders(model, cfg, d, options=None, calls=2, **kw):
    """the tick with the wave order off, then `calls` times with it on (the first in the identity order, the next in the recorded one): every
    call bit-identical; -> (result, {statistic: value} of the last call with the order off)"""
    off = _handle(model, cfg, 0, options)
    ref = off.tick(d, DT, want_q_next=True, **kw)
    stats = {k: off.stat(k) for k in ("last_path", "deferred_last")}
    off.close()
    on = _handle(model, cfg, 2, options)
    for call in range(calls):
        got = on.tick(d, DT, want_q_next=True, **kw)
        assert on.stat("last_path") == stats["last_path"] and on.stat("deferred_last") == stats["deferred_last"]
        for k in ref:
            x, y = np.asarray(got[k]), np.asarray(ref[k])
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "wave order on, call %d: %s differs" % (call, k)
    on.close()
    return ref, stats


def _against_oracle(got, ref, tol, what):
    assert (got["status"] == ref["status"]).all(), what
    ok = ref["status"] == 0
    assert ok.mean() > 0.9, what
    err = np.abs(got["qdot"] - ref["qdot"])[ok].max()
    print("%s: qdot max-abs err vs oracle %.3e, iters %d..%d" % (what, err, got["iters"].min(), got["iters"].max()))
    assert err < tol, what
    assert np.abs(got["q_next"] - ref["q_next"])[ok].max() < 1e-7, what
    return ok


@pytest.mark.parametrize("rows", ["one", "all"])
def test_rank_deficient_leg_block_pivot_and_swap(wx200, singular, rows):
    """(a) A flagged stance-leg block in one row of every wavefront, then in all four: pivoted elimination and SWAP inside the packed kernel,
    nothing deferred."""
    cfg, batches = singular
    d, ref, flagged = batches[rows]
    assert flagged.sum() == (B // 4 if rows == "one" else B) and (rows == "all" or flagged.reshape(-1, 4)[:, 0].all())
    got, stats = _both_orders(wx200, cfg, d, {"presolve_tol_exp": BAR_EXP})
    assert stats["last_path"] == 2 and stats["deferred_last"] == 0
    _against_oracle(got, ref, QDOT_TOL, "pivot + swap, %s" % rows)


@pytest.mark.parametrize("rows", ["one", "all"])
def test_forced_defer_takes_the_tail_and_counts(wx200, singular, rows):
    """(b) The same batches with dbg_force_defer: every flagged instance is redone by its wave's tail on the general path and counted in
    deferred_last; the plain rows of the same wavefronts stay on the packed path."""
    cfg, batches = singular
    d, ref, flagged = batches[rows]
    got, stats = _both_orders(wx200, cfg, d, {"presolve_tol_exp": BAR_EXP, "dbg_force_defer": 1})
    assert stats["last_path"] == 2 and stats["deferred_last"] == int(flagged.sum())
    _against_oracle(got, ref, QDOT_TOL, "forced defer, %s" % rows)


@pytest.fixture(scope="module")
def stress(wx200):
    cfg = common.config("c3", wx200)
    d = common.tick_inputs(wx200, cfg, B, seed=6, stress=True)
    return cfg, d, oracle.tick([wx200], [cfg], d, DT, B, nthreads=8)


def test_stress_instances_drop_slots(wx200, stress):
    """(c) The stress recipe's instances leave constraints again that they took (drop + add pairs): drop_slot in the step loop. That the batch
    holds such instances is checked on the oracle's answer: working-set changes beyond the equalities that exceed the inequalities active at the
    optimum are drops (one drop and its add each)."""
    cfg, d, ref = stress
    a = oracle.assemble([wx200], [cfg], d, DT, B)
    lo, hi = np.concatenate([a["lb"], a["Clb"]], axis=1), np.concatenate([a["ub"], a["Cub"]], axis=1)
    v = np.concatenate([ref["qdot"], np.einsum("bij,bj->bi", a["C"], ref["qdot"])], axis=1)
    ineq = lo != hi
    active = ineq & ((np.abs(v - lo) < 1e-7 * np.maximum(1, np.abs(lo))) | (np.abs(v - hi) < 1e-7 * np.maximum(1, np.abs(hi))))
    drops = (ref["iters"] - (~ineq).sum(axis=1) - active.sum(axis=1)) // 2
    assert (drops[ref["status"] == 0] >= 1).sum() >= 1, "no instance of this seed drops a constraint"
    got, stats = _both_orders(wx200, cfg, d)
    assert stats["last_path"] == 2 and stats["deferred_last"] == 0
    ok = _against_oracle(got, ref, REFINED_TOL, "stress recipe (%d instances with drops)" % int((drops >= 1).sum()))
    assert abs(got["iters"][ok].mean() - ref["iters"][ok].mean()) < 1.01      # (test_gpu_parity.py's bound on the working-set changes)


def test_warm_seeds_that_are_dropped_again(wx200, stress):
    """(d) The WARM variant seeded with the optimum's constraints on their OPPOSITE sides, and with garbage: seeds with a negative multiplier are
    dropped again (restoration) and the cold answer comes back."""
    cfg, d, ref = stress
    bt = _handle(wx200, cfg, 0)
    cold = bt.tick(d, DT, want_working_set=True)
    bt.close()
    ws = np.asarray(cold["working_set"])
    opposite = np.stack([((w & 0xFFFFFFFF) << 32) | ((w >> 32) & 0xFFFFFFFF) for w in ws.T], axis=1)
    junk = np.random.default_rng(3).integers(-2 ** 62, 2 ** 62, (B, 2), dtype=np.int64)
    for name, seed in (("opposite sides", opposite), ("garbage", junk)):
        got, stats = _both_orders(wx200, cfg, dict(d, working_set=seed), want_working_set=True)
        assert stats["last_path"] == 2 and stats["deferred_last"] == 0
        ok = _against_oracle(got, ref, QDOT_TOL, "warm, %s" % name)
        assert np.abs(got["qdot"] - cold["qdot"])[ok].max() < QDOT_TOL
        more = got["iters"][ok] > cold["iters"][ok]
        kept = (np.asarray(got["working_set"])[ok] == seed[ok]).all(axis=1) & (seed[ok] != 0).any(axis=1)
        print("warm, %s: %d of %d instances with more working-set changes than cold, %d return their seed" % (name, int(more.sum()), int(ok.sum()), int(kept.sum())))
        # a seed on the wrong side of its constraint, or a garbage one, cannot be in the final set: no instance hands its seed back ...
        assert not kept.any(), name
        # ... and the seeds were TAKEN and dropped again, not merely ignored: a seed that is taken and has to leave costs two working-set changes the
        # cold run does not have (its add and its drop). A garbage word names a quarter of all bounds and rows on either side, those near x0 are
        # taken, and the optimum holds six at most: some instance of the batch must show the surplus.
        if name == "garbage":
            assert more.any(), name


def test_post_static_configuration(wx200):
    """(e) sim3.py's own posture mode to the letter ("HYBRID", literal): the packed kernel forms the static target itself and the rest of the
    tick sees the perturbed state (the post_static / post_pert block)."""
    cfg = common.config("c3_hybrid", wx200)
    d = common.tick_inputs(wx200, cfg, B, seed=23)
    ref = oracle.tick([wx200], [cfg], d, DT, B, nthreads=8)
    got, stats = _both_orders(wx200, cfg, d)
    assert stats["last_path"] == 2
    ok = _against_oracle(got, ref, REFINED_TOL, "post_static")
    bt = _handle(wx200, cfg, 0)
    plain = bt.integrate(d["q"], got["qdot"], DT)
    bt.close()
    assert np.abs(plain - got["q_next"])[ok].max() > 1e-4            # (the leak is visible: integration started from the perturbed state)
