"""The conditions under which the steps of test_gpu_handle_lifetime.py mean something, checked with the oracle alone: for every
(switch set, model mix, B >= 5) of the walk the oracle solves at least B // 2 instances, and on the tick_grad steps at least B // 2 are solved
and certified by wbc_workload.qp_certificate. The GPU test asserts the same where it makes its fresh references; this one needs no GPU."""
import pytest

import handle_walk as hw

BATCHES = sorted({B for B in hw.BATCHES if B >= 5})


@pytest.mark.parametrize("mix", list(hw.MIXES))
def test_the_oracle_alone_solves_the_walks_ticks(mix):
    for cfg_name in hw.ROUTE_CONFIGS:
        for B in BATCHES:
            n = hw.solved_by_the_oracle(mix, cfg_name, B)
            assert n >= B // 2, (mix, cfg_name, B, n)


@pytest.mark.parametrize("mix", list(hw.MIXES))
def test_the_tick_grad_steps_are_solved_and_certified(mix):
    for cfg_name in hw.GRAD_CONFIGS:
        for B in BATCHES:
            n = hw.certified_on_the_host(mix, cfg_name, B)
            assert n >= B // 2, (mix, cfg_name, B, n)


def test_the_configurations_with_other_weights_keep_their_switches_and_sizes():
    """"c3+w" and the in-flight test's configuration: same rows, every non-zero weight and gain moved (fill_zeros: all 85 non-zero)"""
    import oracle
    import wbc_model
    for mix in hw.MIXES:
        for c, w in zip(hw.problem(mix, "c3")["cfgs"], hw.problem(mix, "c3+w")["cfgs"]):
            assert oracle.task_rows(c) == oracle.task_rows(w) and oracle.constraint_rows(c) == oracle.constraint_rows(w)
            a, b = wbc_model.task_params(c, 1), wbc_model.task_params(w, 1)
            assert ((a == 0) == (b == 0)).all() and (b[a != 0] != a[a != 0]).all()
            f = wbc_model.task_params(hw.other_weights(c, fill_zeros=True), 1)
            assert (f != 0).all() and (f != a).all()
