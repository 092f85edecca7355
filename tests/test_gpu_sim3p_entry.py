"""The packed sim3 kernel's entry issues its loads level by level: the wave order's slice block (one scalar load group), then
the list entry, then every input of the instance at once — one address per lane and one predicated load where nested arms had a load each —,
then the per-lane tables. Operands, operations and their order are what they were, so every result is bit for bit what it was: the outputs recorded
from the build before the change (tests/golden/sim3p_entry.npz, made by tools/make_entry_golden.py) must come back. The batches
(tests/sim3p_entry_cases.py) are those where the entry can go wrong:
  * small_B1 / B3 / B4 / B5: a lone row, rows without an instance (they take instance B - 1's inputs and store nothing), a short second wave;
    wave order off; the FIXD form must have run;
  * wo_B5 / wo_B67: three ticks on one handle with wave_order 2 — tick 1 finds the slice block's batch size mismatching and takes the identity
    order, ticks 2 and 3 read the block and the list; the statistic wave_order_slices equals the recording too;
  * absent_*: the B = 5 batch with each optional input left out, and all of them — the null tests the single load folds into a select. Where the
    library's argument check refuses the call (the configuration needs the input), it must still refuse it;
  * mixed: two models in one wave through model_id — the tables depend on the instance; the form that reads the plan must have run;
  * single_fixd1 / single_fixd0: both forms on one batch, equal to each other and to the recording;
  * warm, trunk, tp, qcon: each variant's own inputs; rollout: three closed-loop ticks (the q_next stores and their table entries).
Every call runs on guarded device buffers (tests/devguard.py): rows of another batch in front of and behind every input, a bit pattern around
every output — a stray store shows; a stray READ cannot be seen here without risking a fault, tests/test_sim3p_entry_host.py checks the addresses."""
import os

import numpy as np
import pytest

import devguard
import sim3p_entry_cases as ec

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["small_B1", "small_B3", "small_B4", "small_B5", "wo_B5", "wo_B67"] + ["absent_" + n for n in ec.OPTIONAL] + [
    "absent_all", "mixed", "single_fixd1", "single_fixd0", "warm", "trunk", "tp", "qcon", "rollout"]


@pytest.fixture(scope="module")
def data():
    zg = np.load(os.path.join(HERE, "golden", "sim3p_guards.npz"))
    z = np.load(os.path.join(HERE, "golden", "sim3p_entry.npz"))
    cases = ec.cases(zg, {k: z["small_in_" + k] for k in ("ee_ref_rot", "ee_prev_rot")})
    assert list(cases) == NAMES
    return z, cases, ec.other_rows(zg)


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream()


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), "%s differs in %d instances" % (
        what, int((got.reshape(len(got), -1) != want.reshape(len(want), -1)).any(axis=1).sum()))


def _run_guarded(case, other, side):
    """-> ec.run's result with every tick's outputs as numpy copies; guards checked after every call"""
    sess = []

    def before(bt):
        sess.append(devguard.Session("other", side))
        bt.allocator = sess[-1].alloc

    def put(name, a):
        return sess[-1].put(name, a, other[name])

    def after(bt, tick):
        import torch
        torch.cuda.synchronize()
        bt.allocator = None
        sess[-1].check("tick %d" % tick)

    import torch
    with torch.cuda.stream(side):
        r = ec.run(case, put=put, before=before, after=after)
    if r[0] == "ok":
        r = ("ok", [devguard.to_host(dict(g)) for g in r[1]], r[2])
    return r


@pytest.mark.parametrize("name", NAMES)
def test_bit_identical_to_the_build_before(data, side, name):
    z, cases, other = data
    case = cases[name]
    r = _run_guarded(case, other, side)
    if name + "_refused" in z.files:
        assert r[0] == "refused", "%s: the recording build's argument check refused this call, this build ran it" % name
        return
    assert r[0] == "ok", "%s: refused (%s); the recording build ran it" % (name, r[1])
    _, res, stats = r
    assert len(res) == case["ticks"]
    for t, (got, st) in enumerate(zip(res, stats), 1):
        what = "%s, tick %d" % (name, t)
        if case["kind"] == "tick":
            assert st["last_path"] == 2, what                                  # the packed sim3 kernel
            assert st["last_tick_fixd"] == case["fixd"], what
        assert st["wave_order_slices"] == int(z[name + "_slices"][t - 1]), what
        for k in ec.keys_of(case):
            _same_bits(got[k], z["%s_t%d_%s" % (name, t, k)], "%s: %s" % (what, k))


def test_both_forms_agree(data):
    """the recording itself: the FIXD form and the form that reads the plan gave the same bits on the single batch, and the wave order's ticks the
    bits of the identity order"""
    z = data[0]
    for k in ec.OUT:
        _same_bits(z["single_fixd1_t1_" + k], z["single_fixd0_t1_" + k], "single: " + k)
        for t in (1, 2, 3):
            _same_bits(z["wo_B67_t%d_%s" % (t, k)], z["single_fixd1_t1_" + k], "wave order tick %d: %s" % (t, k))
            _same_bits(z["wo_B5_t%d_%s" % (t, k)], z["small_B5_t1_" + k], "wave order tick %d (B = 5): %s" % (t, k))
