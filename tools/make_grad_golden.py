#!/usr/bin/env python3
"""Writes tests/golden/grad_recorded.npz: what the gradient entry points (qp_certificate, tick_vjp, tick_vjp_state, tick_grad, tick_grad_q,
step_vjp, rollout_record + rollout_vjp) and the torch layers over them gave BEFORE their host code was reorganised into one path per layer
(DESIGN.md §3.43), with the inputs of the calls, the statistics last_*_variant after each, and the error code and full message of every
refused call. The calls, their order and the refusals are tests/grad_recorded_cases.py's; tests/test_gpu_grad_recorded.py expects all of it
back from every later build, from host arrays and from device tensors. The committed file was made on an MI355X in a checkout of the commit
before the change (library AND Python wrappers of that commit), with this tool and tests/grad_recorded_cases.py copied in:

    python __graft_entry__.py build && python tools/make_grad_golden.py [output.npz]

Asserted while recording, so that the cases exercise what they claim to: an instance has nv < 26; a bound or a constraint row is active;
grad_status != 0 exactly on the bad row, whose gradient rows are zero; sens_rows is not trivial where there are constraint rows; q_con does not
reach the tick layer; every call run a second time, on a second handle, gives the same bits; every refused call is refused and leaves its
outputs and its tape alone; the file stays below tests/golden/packed_qp_shared.npz (the outputs of most
calls are held as dtype, shape and SHA-256: grad_recorded_cases.pack). The tick inputs are drawn from the first seed of SEEDS
under which all of this holds (the seed is stored)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mech5845m-wbc-for-legged-manipulator_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

import grad_recorded_cases as gr  # noqa: E402

SEEDS = (7, 8, 9, 10, 11, 12)


def record(seed):
    """-> (z, None) or (None, the claim that does not hold under this seed)"""
    inputs = gr.make_inputs(seed)
    z = {"in__" + k: v for k, v in inputs.items()}
    z["seed"] = np.int64(seed)
    for name in gr.CONFIGS:
        runs = []
        for rep in range(2):
            bt = gr.handle(name)
            runs.append(list(gr.run_cases(bt, name, inputs)))
            bt.close()
        nvs = inputs[name + "__nvs"]
        bad = np.arange(gr.B) == gr.BAD
        for (call, o, stats, p), (_, o2, stats2, _) in zip(*runs):
            assert set(o) == set(o2) and stats.tolist() == stats2.tolist(), (name, call)
            for k in o:
                assert o[k].tobytes() == o2[k].tobytes(), "%s / %s: %s differs between two runs" % (name, call, k)
            print("%-7s %-18s stats %s keys %s" % (name, call, [hex(int(s)) for s in stats], " ".join(sorted(o))))
            z["stats__%s__%s" % (name, call)] = stats
            for k, v in o.items():
                z["out__%s__%s__%s" % (name, call, k)] = gr.pack(name, call, v)
            gs = o.get("grad_status")
            if gs is not None and name != "c3s3" and not np.array_equal(gs != 0, bad):
                return None, "%s / %s: grad_status %s" % (name, call, gs.tolist())
            if gs is not None:
                for k, v in o.items():
                    if k.startswith("d_"):
                        assert not v[gr.BAD].view(np.uint64).any(), (name, call, k)
            if call == "certificate":
                print("        status %s cert_status %s n_active %s" % (o["status"].tolist(), o["cert_status"].tolist(), o["n_active"].tolist()))
                if not (o["n_active"][~bad] > 0).any():
                    return None, "%s: no bound or row is active" % name
                if p > 0 and not (np.abs(o["sens_rows"][~bad]).max() > 0 and np.abs(o["y_rows"][~bad]).max() > 0):
                    return None, "%s: sens_rows / y_rows are trivial" % name
                assert o["sens_rows"].shape == (gr.B, p)
            if call.startswith("rollout"):
                print("        ticks_dropped %s rec_status %s" % (o["ticks_dropped"].tolist(), o["rec_status"].tolist()))
        got = {call: o for call, o, _, _ in runs[0]}
        for k in got["tick_vjp_q_con"]:
            assert got["tick_vjp_q_con"][k].tobytes() == got["tick_vjp_subset"][k].tobytes(), "%s: q_con reaches the tick layer (%s)" % (name, k)
        assert set(got["rollout_q0_only"]) - {k for k in got["rollout_cold"] if k.startswith("rec_")} == {"d_q0", "grad_status", "ticks_dropped"}
        assert got["rollout_q0_only"]["d_q0"].tobytes() == got["rollout_cold"]["d_q0"].tobytes(), name
        if name != "c3s3":
            assert (nvs < 26).any() and (runs[0][0][3] > 0) == (name == "rows")
        else:
            print("c3s3: ticks_dropped of the cold roll-out %s" % got["rollout_cold"]["ticks_dropped"].tolist())
    hs = gr.refusal_handles()
    for name, code, msg, ok in gr.run_refusals(hs, inputs):
        print("refused %-48s %s %s" % (name, code, msg))
        assert code != 0, "%s was not refused" % name
        assert ok, "%s: a refused call touched its outputs or its tape" % name
        z["refusal__" + name] = np.array("%s|%s" % (code, msg))
    for bt in hs.values():
        bt.close()
    return z, None


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "grad_recorded.npz")
    for seed in SEEDS:
        z, why = record(seed)
        if z is not None:
            break
        print("seed %d: %s" % (seed, why))
    assert z is not None, "no seed of %s gives cases that exercise what they claim" % (SEEDS,)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **z)
    size = os.path.getsize(out)
    assert size < os.path.getsize(os.path.join(ROOT, "tests", "golden", "packed_qp_shared.npz")), size
    print("wrote %s (%d bytes, seed %d)" % (out, size, int(z["seed"])))


if __name__ == "__main__":
    main()
