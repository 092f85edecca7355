"""The packed kernels' dual active-set runs on one text of its factor updates (wbc_packed.h pk_qp_products / pk_qp_add_step / pk_qp_drop_slot and
their scalar cores). The refactor changed no floating-point operation's operands or place, so the packed orth tick's INEQ
variant, the packed box tick and the packed QP kernel give, bit for bit, what the build before it gave (tests/golden/packed_qp_shared.npz,
made by tools/make_packed_qp_golden.py; the packed sim3 tick's records are those of tests/test_gpu_sim3p_*.py):
  * ticks, B = 67 (sixteen full waves and one short one): cold, WARM seeded with the cold run's working sets, and WARM seeded with another
    seed's working sets — wrong seeds, which the restoration loop drops again (its own call of the drop step: the record holds instances
    that run more iterations on the other seed's working sets than on their own); the variant that ran (WARM or not) is read back;
  * one batch of 67 QPs for each group of the packed QP kernel's variants — four problems per wavefront, two, two with HALF — each plain,
    asking for the working sets (WARM) and hot-started, with the variant that ran read back."""
import os

import numpy as np
import pytest

import common
import wbc_capi
import wbc_model
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu

DT = 0.002
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_qp_shared.npz")
OUT = ("qdot", "status", "iters", "q_next")
TICKS = {"orth": ("everything", "packed_orth", (3, 1)), "box": ("full", "packed_box", (4, 0))}
QPS = {"qp16": (16, 16, 0), "qp32": (32, 26, 0), "qp32h": (32, 26, 1)}     # (G, PV, HALF) of the variant rows: include/wbc.h "last_qp_variant"


@pytest.fixture(scope="module")
def wx200():
    return wbc_model.load_model("a1_wx200")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _same_bits(got, want, what):
    x, y = np.asarray(got), np.asarray(want)
    assert x.shape == y.shape and x.dtype == y.dtype, what
    assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s differs in %d instances" % (
        what, int((x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1).sum()))


@pytest.mark.parametrize("case", ["cold", "warm", "wrong"])
@pytest.mark.parametrize("kernel", ["orth", "box"])
def test_tick_bit_identical_to_the_build_before(wx200, golden, kernel, case):
    z = golden
    name, option, path = TICKS[kernel]
    d = {k[len(kernel) + 4:]: z[k] for k in z.files if k.startswith(kernel + "_in_")}
    B = len(d["q"])
    assert B == 67
    kw, outs = {}, OUT
    if case != "cold":
        d["working_set"] = z["%s_%s_in_working_set" % (kernel, case)]
        kw, outs = {"want_working_set": True}, OUT + ("working_set",)
    if case == "wrong":      # wrong seeds are in the record: other working sets, and instances that need more iterations to get rid of them
        assert (z[kernel + "_wrong_in_working_set"] != z[kernel + "_warm_in_working_set"]).any()
        assert (z[kernel + "_wrong_out_iters"] > z[kernel + "_warm_out_iters"]).any()
    bt = WbcBatch(wx200, B)
    bt.configure(common.config(name, wx200))
    bt.set_option(option, 2)
    got = bt.tick(d, DT, want_q_next=True, **kw)
    assert (bt.stat("last_path"), bt.stat("last_orth")) == path
    flags = wbc_capi.variant_args(bt.stat("last_tick_variant"))      # orthp: (INEQ, WARM, ROT, TP), boxp: (WARM, ROT, TP)
    assert (flags[:2] == (1, int(case != "cold"))) if kernel == "orth" else (flags[0] == int(case != "cold")), flags
    bt.close()
    assert 2 * int((np.asarray(got["status"]) == 0).sum()) >= B
    for k in outs:
        _same_bits(got[k], z["%s_%s_out_%s" % (kernel, case, k)], "%s %s: %s" % (kernel, case, k))


@pytest.mark.parametrize("tag", ["plain", "cold", "hot"])
@pytest.mark.parametrize("case", ["qp16", "qp32", "qp32h"])
def test_qp_bit_identical_to_the_build_before(golden, case, tag):
    z = golden
    g, pv, half = QPS[case]
    stored = {k[len(case) + 4:]: z[k] for k in z.files if k.startswith(case + "_in_")}
    q = {k: v.astype(np.float64) / 16.0 for k, v in stored.items()}      # (stored as int8 sixteenths, a NaN as -128)
    q["lb"][stored["lb"] == -128] = np.nan
    B = len(q["A"])
    assert B == 67
    kw = {} if tag == "plain" else {"want_working_set": True}
    if tag == "hot":
        kw["working_set"] = z[case + "_cold_out_working_set"].copy()
    bt = WbcBatch([], B)
    got = bt.qp_solve_ls(q["A"], q["b"], q["C"], q["lb"], q["ub"], q["Clb"], q["Cub"], **kw)
    assert bt.stat("last_qp_path") == 64 // g
    assert wbc_capi.variant_args(bt.stat("last_qp_variant"))[:4] == (g, pv, int(tag != "plain"), half)
    bt.close()
    for k, v in zip(("x", "status", "iters", "working_set"), got):
        _same_bits(v, z["%s_%s_out_%s" % (case, tag, k)], "%s %s: %s" % (case, tag, k))
