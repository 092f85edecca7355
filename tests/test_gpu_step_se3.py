"""wbc_step_vjp on the device against the 50-digit reference of se3_reference.py, block by block, on the inputs of step_se3_cases.py: base
translations of 1e-3, 1 and 30 along, across and askew of omega, |omega| dt from 0 to 30, dt 0.002 and 1, and rows one ulp either side of
the kernel's switch at t^2 = 1. test_gpu_step_grad.py holds the kernel to the numpy restatement at this workload's velocities, where the
coefficients c2 and c3 of the coupling block cannot be seen; here they can.

Bounds (test_step_se3_host.py states the reasoning): the base blocks of WARMUP within 1e-13 x max(1, max|ref block|), per row and block;
RUNNING within the suite's kinematic 1e-12 x max(1, max|ref block|); everything that is a copy, one rounding or a literal zero bit for bit.
One handle per model set for the module, one launch per (mode, IMU, dt), the references built once per process (step_se3_cases).

Measured on an MI355X (DESIGN.md §3.41 has the table): WARMUP's base blocks 4.3e-15 at worst (d_q lin at |omega| dt = 30; d_qdot ang 4.2e-15
at |omega| dt = |v| = 30), RUNNING 3.7e-15 (d_q ang); across the seam the outputs differ by the reference's difference plus 3.0e-16."""
import functools

import numpy as np
import pytest

import common
import se3_reference as s3
import step_se3_cases as cases
import test_gpu_task_params as tgp
import test_step_se3_host as th
import wbc_capi as capi

pytestmark = pytest.mark.gpu

HANDLES = ("wx200", "mixed")
CAPACITY = 64
_OPEN = {}


def _bt(handle):
    if handle not in _OPEN:
        models = [tgp._model(n) for n in (cases.MODELS if handle == "mixed" else cases.MODELS[:1])]
        _OPEN[handle] = tgp._handle(models, [common.config("c3", m) for m in models], CAPACITY, {})
    return _OPEN[handle]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for bt in _OPEN.values():
        bt.close()
    _OPEN.clear()


def _case(handle, mode, dt, imu):
    return cases.warmup_case(handle, dt) if mode == s3.WARMUP else cases.running_case(handle, dt, imu)


def _launch(handle, p, dt, mode, qdot=None):
    bt = _bt(handle)
    got = bt.step_vjp(p["q"], p["qdot"] if qdot is None else qdot, p["foot_targets"], p["g"], dt, imu=p["imu"], model_id=p["mid"], mode=mode)
    assert bt.stat("last_stepvjp_variant") == (0 if handle == "wx200" else 1 << 32)                  # variant_key(ROT)
    return got


@functools.lru_cache(maxsize=None)
def _run(handle, mode, dt, imu):
    """the one launch of a (handle, mode, IMU, dt): the device's outputs, shared by the tests that read them"""
    p = _case(handle, mode, dt, imu)
    assert len(p["q"]) % 4 != 0 and len(p["q"]) > 4
    return _launch(handle, p, dt, mode)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _common_laws(got, p):
    assert (got["grad_status"] == capi.GRAD_OK).all()
    beyond = np.arange(26)[None, :] >= p["nv"][:, None]
    assert not _bits(got["d_q"])[beyond].any() and not _bits(got["d_qdot"])[beyond].any()
    assert not _bits(got["d_foot_targets"][:, 4]).any()


@pytest.mark.parametrize("dt", cases.DTS)
@pytest.mark.parametrize("handle", HANDLES)
def test_warmup_against_the_reference(handle, dt):
    p = _case(handle, s3.WARMUP, dt, False)
    got = _run(handle, s3.WARMUP, dt, False)
    th.hold(got, p, th.WARMUP_BOUNDS, "device / %s / warmup / dt %g" % (handle, dt))
    _common_laws(got, p)
    own = (np.arange(26)[None, :] >= 6) & (np.arange(26)[None, :] < p["nv"][:, None])
    assert np.array_equal(_bits(got["d_q"])[own], _bits(p["g"])[own])                                  # a copy
    assert np.array_equal(_bits(got["d_qdot"])[own], _bits(dt * p["g"])[own])                          # one rounding
    assert not _bits(got["d_foot_targets"]).any()
    assert np.abs(got["d_q"][:, 0:6]).max() > 0 and np.abs(got["d_qdot"][:, 0:6]).max() > 0


@pytest.mark.parametrize("imu", [False, True])
@pytest.mark.parametrize("dt", cases.DTS)
@pytest.mark.parametrize("handle", HANDLES)
def test_running_against_the_reference(handle, dt, imu):
    p = _case(handle, s3.RUNNING, dt, imu)
    got = _run(handle, s3.RUNNING, dt, imu)
    th.hold(got, p, th.RUNNING_BOUNDS, "device / %s / running%s / dt %g" % (handle, " with IMU" if imu else "", dt))
    _common_laws(got, p)
    assert not _bits(got["d_q"][:, 0:3]).any() and not _bits(got["d_qdot"][:, 0:3]).any()              # c_p = 0: the literal
    if imu:
        assert (got["d_q"][:, 3:6] == 0).all() and (got["d_qdot"][:, 3:6] == 0).all()     # Re 0 and Jr' 0: zeros of either sign
    assert np.abs(got["d_q"][:, 6:]).max() > 0 and np.abs(got["d_foot_targets"][:, 0:4]).max() > 0
    # translation does not enter: c_p = 0 and q's xyz cancels in the differences of frame origins
    x = p["qdot"].copy()
    x[:, 0:3] *= 1e4
    again = _launch(handle, p, dt, s3.RUNNING, qdot=x)
    for k in capi.STEP_GRAD_FIELDS:
        assert np.array_equal(_bits(again[k]), _bits(got[k])), k
    assert np.array_equal(again["grad_status"], got["grad_status"])


@pytest.mark.parametrize("variant", ["warmup", "running", "running_imu"])
@pytest.mark.parametrize("handle", HANDLES)
def test_across_the_seam(handle, variant):
    """rows that differ in omega alone, one ulp either side of t^2 = 1 (series below, closed forms above): each holds its bound (asserted with
    the whole set above, and here), and the two outputs differ by no more than the reference's own difference plus twice the bound"""
    mode, imu, dt = (s3.WARMUP if variant == "warmup" else s3.RUNNING), variant == "running_imu", 1.0
    p = _case(handle, mode, dt, imu)
    got = _run(handle, mode, dt, imu)
    bounds = th.WARMUP_BOUNDS if mode == s3.WARMUP else th.RUNNING_BOUNDS
    errs = cases.block_errors(got, p["ref"])
    assert len(p["groups"]) == (1 if (handle == "wx200" and mode == s3.RUNNING) else 3)
    worst = 0.0
    for grp in p["groups"]:
        assert np.array_equal(p["qdot"][grp, 3:6], cases.seam_rows())
        for i, j in cases.SEAM_PAIRS:
            a, b = grp[i], grp[j]
            for name, (key, sl) in cases.BLOCKS.items():
                assert errs[name][a] <= bounds[name] and errs[name][b] <= bounds[name], (name, p["labels"][a])
                ga, gb = np.asarray(got[key])[a][sl].ravel(), np.asarray(got[key])[b][sl].ravel()
                ra, rb = p["ref"][key][a][sl].ravel(), p["ref"][key][b][sl].ravel()
                scale = max(1.0, np.abs(ra).max(), np.abs(rb).max())
                jump, own = np.abs(ga - gb).max(), np.abs(ra - rb).max()
                worst = max(worst, (jump - own) / scale)
                assert jump <= own + 2 * bounds[name] * scale, "%s across %s: |dev a - dev b| %.3e, |ref a - ref b| %.3e" % (
                    name, p["labels"][a], jump, own)
    print("%s / %s: worst (|dev a - dev b| - |ref a - ref b|) / max(1, max|ref block|) across the seam: %.2e" % (handle, variant, worst))
