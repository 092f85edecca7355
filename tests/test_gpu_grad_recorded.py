"""The gradient entry points give, bit for bit, what they gave before their host code was reorganised into one path per layer, shared by the
single calls and the roll-out's sweep: tests/golden/grad_recorded.npz, recorded by tools/make_grad_golden.py from the library
and the wrappers of the commit before. The calls and their order are grad_recorded_cases.py's — three configurations (`everything` and `full`
over three interleaved models, one with nv < 26 and one with rotated placements: constraint rows and none; c3 with instances that go unsolved),
max_batch = 12 and B = 9, twenty calls on one handle each: the tick's certificate, tick_vjp (all outputs, a subset, with a q_con it must not
see), tick_vjp_state, tick_grad, tick_grad_q, step_vjp in both modes, rollout_record + rollout_vjp (d_q0 alone first: the sweep
that skips the tick kernel; cold, warm, each seed alone, WARMUP)
and the backward of the four torch layers; one row of q holds a NaN throughout. Every output's key set, dtype, shape and bits are held (the
array itself or its SHA-256), and the statistics last_grad_variant, last_gradq_variant, last_stepvjp_variant and last_rollvjp_variant after
every call; once from numpy arrays (the library stages them) and once from torch device tensors (the pointers pass through). Every refusal of
the six entry points and of their wrappers is held to its error code and its full text, with the caller's outputs and tape untouched."""
import os

import numpy as np
import pytest
import torch

import grad_recorded_cases as gr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_recorded.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def test_the_record_holds_what_the_cases_claim(golden):
    z = golden
    bad = np.arange(gr.B) == gr.BAD
    for name in ("rows", "norows"):
        assert z["in__%s__d_q" % name].shape == (gr.B, 27) and gr.B < gr.MAX_BATCH and np.isnan(z["in__%s__d_q" % name][gr.BAD]).any()
        assert (z["in__%s__nvs" % name] < 26).any() and len(set(z["in__%s__d_model_id" % name].tolist())) == 3
        assert (z["out__%s__certificate__n_active" % name][~bad] > 0).any()
        for call in gr.CALLS:
            key = "out__%s__%s__grad_status" % (name, call)
            if key in z:
                assert np.array_equal(z[key] != 0, bad), key
    assert np.abs(z["out__rows__certificate__sens_rows"][~bad]).max() > 0 and z["out__rows__certificate__sens_rows"].shape[1] > 0
    assert z["out__rows__tick_vjp_state__d_q"].shape == (gr.B, 26) and not z["out__rows__tick_vjp_state__d_q"][gr.BAD].any()
    assert str(z["out__norows__certificate__sens_rows"]).startswith("<f8|(%d, 0)|" % gr.B)                 # the p == 0 branch
    assert not [k for k in z if k.startswith("out__rows__rollout_q0_only__d_") and not k.endswith("__d_q0")]
    assert z["stats__rows__rollout_q0_only"].tolist()[0] == -1 and z["stats__rows__rollout_q0_only"].tolist()[1] >= 0      # no tick kernel ran
    assert sum(k.startswith("refusal__") for k in z) >= 75
    assert sorted(k for k in z if "/schedule" in k) == ["refusal__%s/schedule" % c for c in ("record", "rollout_vjp", "step_vjp", "tick_vjp", "tick_vjp_state")]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", list(gr.CONFIGS))
def test_every_gradient_call_gives_the_recorded_bits(golden, name, mem):
    z = golden
    inputs = {k[4:]: v for k, v in z.items() if k.startswith("in__")}
    conv = (lambda a: a) if mem == "host" else (lambda a: torch.from_numpy(a).cuda())
    bt = gr.handle(name)
    wrong = []
    for call, got, stats, _ in gr.run_cases(bt, name, inputs, conv):
        pre = "out__%s__%s__" % (name, call)
        want = {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}
        if set(got) != set(want):
            wrong.append((call, "keys", sorted(set(got) ^ set(want))))
            continue
        for k, v in got.items():
            if not gr.same(gr.pack(name, call, v), want[k]):
                wrong.append((call, k, str(v.dtype), v.shape))
        if stats.tolist() != z["stats__%s__%s" % (name, call)].tolist():
            wrong.append((call, "stats", stats.tolist(), z["stats__%s__%s" % (name, call)].tolist()))
    bt.close()
    print("%s / %s: differing from the record: %s" % (name, mem, wrong or "nothing"))
    assert not wrong, wrong


def test_every_refusal_keeps_its_code_and_its_text(golden):
    z = golden
    inputs = {k[4:]: v for k, v in z.items() if k.startswith("in__")}
    hs = gr.refusal_handles()
    wrong, seen = [], set()
    for name, code, msg, ok in gr.run_refusals(hs, inputs):
        seen.add("refusal__" + name)
        want = str(z.get("refusal__" + name))
        if "%s|%s" % (code, msg) != want:
            wrong.append((name, "%s|%s" % (code, msg), want))
        if not ok:
            wrong.append((name, "a refused call touched its outputs or its tape"))
    for bt in hs.values():
        bt.close()
    print("refusals differing from the record: %s" % (wrong or "nothing"))
    assert seen == {k for k in z if k.startswith("refusal__")}
    assert not wrong, wrong
