"""The recorded roll-outs along tracks and their reverse sweeps give, bit for bit, what they gave before the sweep's host code was reorganised
into two extensions beside the forward loop's and the track evaluation of the forward and the adjoint kernel into one header (DESIGN.md
§3.47): tests/golden/sweep_recorded.npz, recorded by tools/make_sweep_golden.py from the library and the wrappers of the commit before. The
calls and their order are sweep_recorded_cases.py's — `everything` and `full` over three interleaved models, max_batch = 12, B = 9, K = 4, a
NaN in row 4 (a tangent along six tracks, a milestone along two), twenty-three calls on one handle each: rollout_record along six tracks (all kinds, n_points of {2, 3, 5}, every clamp
branch and default-tangent case) cold and under warm_start with the scores and a hash of the tape; rollout_vjp on those tapes from each state
seed, all of them, a subset of the outputs, the caller's arrays, each score cotangent alone, scores with state seeds and an all-zero score
seed; two tracks with one du_all; the plain record and sweep afterwards; the backward of wbc_rollout_tracks_fused and of
wbc_rollout_tracks_scored under a score-only, a state-only and a mixed loss. Every output's key set, dtype, shape and bits are held (the array
itself or its SHA-256) and the statistics last_rollvjp_variant, last_trackvjp_variant and last_scorevjp_variant after every call; once from
numpy arrays (the library stages them) and once from torch device tensors (the pointers pass through). Every refusal of the sweep's own checks
is held to its error code and its full text, with the caller's outputs and the tape untouched."""
import os

import numpy as np
import pytest
import torch

import sweep_recorded_cases as sr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_recorded.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def test_the_record_holds_what_the_cases_claim(golden):
    z = golden
    bad = np.arange(sr.B) == sr.BAD
    for name in sr.CONFIGS:
        raw = sr.inputs_of({k[4:]: v for k, v in z.items() if k.startswith("in__")}, name)
        assert raw["d_q"].shape == (sr.B, 27) and sr.B < sr.MAX_BATCH and not np.isnan(raw["d_q"]).any()
        assert (raw["nvs"] < 26).any() and len(set(raw["d_model_id"].tolist())) == 3
        six, two = sr.tracks_of(raw, "six"), sr.tracks_of(raw, "two")
        assert len(six) == 6 and {t["kind"] for t in six} == {"linear", "hermite"} and sum("tangents" in t for t in six) == 2
        assert all(set(t["n_points"].tolist()) == {2, 3, 5} and t["points"].shape == (sr.B, 5, 3) for t in six)
        assert not any(np.isnan(t["points"]).any() for t in six) and [j for j, t in enumerate(six) if "tangents" in t and np.isnan(t["tangents"]).any()] == [2]
        assert np.isnan(six[2]["tangents"]).any(axis=(1, 2)).tolist() == bad.tolist()      # the bad row of `six`: a tangent alone
        assert sr.coverage(six) == ({"first", "inside", "last"}, {1, 2, 3, 4})
        assert all("n_points" not in t and t["du"] == sr.DU_ALL for t in two) and np.isnan(two[1]["points"][sr.BAD]).any()
        for call in sr.CALLS:
            key = "out__%s__%s__grad_status" % (name, call)
            if key in z:
                assert np.array_equal(z[key] != 0, bad if call != "plain" else bad & False), key
        assert "out__%s__six_all__t5_d_points" % name in z and "out__%s__six_all__t5_d_tangents" % name in z
        held = lambda v: v if v.dtype.kind in "iU" else sr.pack("", "", v)      # noqa: E731
        for k in (k for k in z if k.startswith("out__%s__six_all__" % name)):      # the caller's arrays and an all-zero score seed: the same sweep
            for other in ("six_out", "six_score_zero"):
                assert sr.same(held(z[k.replace("six_all", other)]), held(z[k])), k
        stats = {call: z["stats__%s__%s" % (name, call)].tolist() for call in sr.CALLS}
        assert stats["six_final"][1] >= 0 and stats["six_final"][2] == -1 and stats["six_score_sq"][2] >= 0      # no score stage before the first score seed
    assert not z["out__rows__six_score_state__t2_d_points"][sr.BAD].any() and z["out__rows__six_score_state__t2_d_points"][~bad].any()
    assert sum(k.startswith("refusal__") for k in z) >= 30


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", list(sr.CONFIGS))
def test_every_sweep_call_gives_the_recorded_bits(golden, name, mem):
    z = golden
    inputs = {k[4:]: v for k, v in z.items() if k.startswith("in__")}
    conv = (lambda a: a) if mem == "host" else (lambda a: torch.from_numpy(a).cuda())
    bt = sr.handle(name)
    wrong = []
    for call, got, stats in sr.run_cases(bt, name, inputs, conv):
        pre = "out__%s__%s__" % (name, call)
        want = {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}
        if set(got) != set(want):
            wrong.append((call, "keys", sorted(set(got) ^ set(want))))
            continue
        for k, v in got.items():
            if not sr.same(sr.pack(name, call, v), want[k]):
                wrong.append((call, k, str(v.dtype), v.shape))
        if stats.tolist() != z["stats__%s__%s" % (name, call)].tolist():
            wrong.append((call, "stats", stats.tolist(), z["stats__%s__%s" % (name, call)].tolist()))
    bt.close()
    print("%s / %s: differing from the record: %s" % (name, mem, wrong or "nothing"))
    assert not wrong, wrong


def test_every_refusal_keeps_its_code_and_its_text(golden):
    z = golden
    inputs = {k[4:]: v for k, v in z.items() if k.startswith("in__")}
    bt = sr.handle("rows")
    wrong, seen = [], set()
    for name, code, msg, ok in sr.run_refusals(bt, inputs):
        seen.add("refusal__" + name)
        want = str(z.get("refusal__" + name))
        if "%s|%s" % (code, msg) != want:
            wrong.append((name, "%s|%s" % (code, msg), want))
        if not ok:
            wrong.append((name, "a refused call touched its outputs or the tape"))
    bt.close()
    print("refusals differing from the record: %s" % (wrong or "nothing"))
    assert seen == {k for k in z if k.startswith("refusal__")}
    assert not wrong, wrong


@pytest.mark.parametrize("mem", ["host", "device"])
def test_the_score_seed_without_rotated_placements_gives_the_recorded_bits(golden, mem):
    """wbc_scorevjp_kernel<SEED, no ROT>, which no call of CALLS launches: a1_wx200 alone at B = 5 (a full wave and one with three padding
    rows), held to the bits recorded from the library before the whole-tree kernels shared a header"""
    z = golden
    inputs = {k[4:]: v for k, v in z.items() if k.startswith("in__")}
    want = {k[len("b5__out__"):]: v for k, v in z.items() if k.startswith("b5__out__")}
    assert want["d_q0"].shape == (sr.B5, 26) and want["d_q0"].any() and not want["grad_status"].any()
    rot = [int(z["stats__rows__six_score_state"][2]), int(z["b5__variant"])]
    assert rot[0] >= 0 and rot[1] >= 0 and rot[0] != rot[1], rot      # another variant than the configurations' calls
    conv = (lambda a: a) if mem == "host" else (lambda a: torch.from_numpy(a).cuda())
    got, variant = sr.run_b5(inputs, conv)
    wrong = [k for k in want if k not in got or got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes()]
    assert set(got) == set(want) and variant == int(z["b5__variant"]) and not wrong, (wrong, variant)
