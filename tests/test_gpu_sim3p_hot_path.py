"""The packed sim3 kernel's hot path lost instructions that are not arithmetic: DPP moves without the operand copy where all
lanes are active, and the wave order's index arithmetic on launch constants (a reciprocal from the host instead of three divisions). No
floating-point operation changed its operands or its place in its dependency tree, so every result is bit for bit what it was:
  * four B = 67 batches (16 full waves and one wave with a single invalid row: cold C3 on a stress-recipe seed with drops, WARM seeded with the
    cold run's working sets, TRUNK, QCON) against outputs recorded from the build before the change (tests/golden/sim3p_hot_path.npz, made by
    tools/make_hot_path_golden.py), with the wave order off and over three ticks with it on (ticks 2 and 3 in a recorded order);
  * the slice geometry: batches of 1, 1, 2 and 3 slices with the order on against off, and the number of slices that published."""
import os

import numpy as np
import pytest

import common
import oracle
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3p_hot_path.npz")
OUT = ("qdot", "status", "iters", "q_next")
CONFIG = {"cold": "c3", "warm": "c3", "trunk": "c3_trunk_task", "qcon": "c3_mani"}


@pytest.fixture(scope="module")
def wx200():
    return wbc_model.load_model("a1_wx200")


def _handle(model, cfg, B, wave_order):
    bt = WbcBatch(model, B)
    bt.configure(cfg)
    bt.set_option("wave_order", wave_order)
    return bt


def _bits_equal(a, b, what):
    for k in OUT:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s differs in %d instances" % (
            what, k, int((x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1).sum()))


def _recorded_order_moves_someone(dual_iters, B):
    """Does the order a launch with these dual iteration counts records differ from the identity (tests/test_gpu_sim3p_issue_order.py)? A slice's
    order is its instances by work class, heaviest first (wbc_packed.h wo_class: 0 for >= 10 dual iterations .. 5 for none); if the classes of a
    slice's instances, in position order, are not already ascending, some wave gets other instances than its own. B = 67: one slice."""
    it = np.asarray(dual_iters)
    cls = np.where(it >= 10, 0, np.where(it >= 6, 1, np.where(it >= 3, 2, 5 - it)))
    assert -(-B // 4) <= 127
    return bool((np.diff(cls) < 0).any())


@pytest.mark.parametrize("case", ["cold", "warm", "trunk", "qcon"])
def test_bit_identical_to_the_build_before(wx200, case):
    """The recorded bits come back: one tick with the wave order off, three ticks on one handle with wave_order 2. That ticks 2 and 3 of the cold
    case run in another order than the identity is read off the recorded iteration counts."""
    z = np.load(GOLDEN)
    src = "cold" if case == "warm" else case          # (the WARM case: the cold case's inputs plus its working sets)
    d = {k[len(src) + 4:]: z[k] for k in z.files if k.startswith(src + "_in_")}
    kw = {}
    if case == "warm":
        d["working_set"] = z["warm_in_working_set"]
        kw["want_working_set"] = True
    want = {k: z["%s_out_%s" % (case, k)] for k in OUT}
    B = len(d["q"])
    assert B == 67
    cfg = common.config(CONFIG[case], wx200)
    if case == "cold":
        a = oracle.assemble([wx200], [cfg], d, DT, B)
        n_eq = int(((a["lb"] == a["ub"]).sum(axis=1) + (a["Clb"] == a["Cub"]).sum(axis=1))[0])   # contact rows + locked DoF: counted in iters, not dual iterations
        assert _recorded_order_moves_someone(want["iters"] - n_eq, B), "the recorded order is the identity: choose another seed"
    off = _handle(wx200, cfg, B, 0)
    got = off.tick(d, DT, want_q_next=True, **kw)
    assert off.stat("last_path") == 2 and off.stat("wave_order_slices") == 0
    _bits_equal(got, want, "%s, order off" % case)
    off.close()
    on = _handle(wx200, cfg, B, 2)
    for tick in (1, 2, 3):
        got = on.tick(d, DT, want_q_next=True, **kw)
        assert on.stat("last_path") == 2 and on.stat("wave_order_slices") == 1
        _bits_equal(got, want, "%s, order on, tick %d" % (case, tick))
    on.close()


@pytest.fixture(scope="module")
def pool(wx200):
    cfg = common.config("c3", wx200)
    return cfg, common.tick_inputs(wx200, cfg, 1021, seed=6, stress=True)


@pytest.mark.parametrize("B,ns", [(4, 1), (508, 1), (512, 2), (1021, 3)])
def test_slice_geometry(wx200, pool, B, ns):
    """1, 127, 128 and 256 waves: one full slice and less, two slices, three with a short last wave. Two ticks with the order on (the second in the
    recorded order) are bit for bit the ticks with it off, and every slice published after the first."""
    cfg, d = pool
    d = {k: v[:B] for k, v in d.items()}
    assert ns == -(-(-(-B // 4)) // 127)
    on, off = _handle(wx200, cfg, B, 2), _handle(wx200, cfg, B, 0)
    for tick in (1, 2):
        ref = off.tick(d, DT, want_q_next=True)
        got = on.tick(d, DT, want_q_next=True)
        assert on.stat("last_path") == 2 and off.stat("last_path") == 2
        assert on.stat("wave_order_slices") == ns and off.stat("wave_order_slices") == 0
        _bits_equal(got, ref, "B = %d, tick %d" % (B, tick))
    on.close(); off.close()
