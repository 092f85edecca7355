"""Per-instance task weights and gains (WbcTaskParams) on the host: the ctypes layout against the header's WbcConfig block, and
wbc_model.task_params (rows from a configuration, overrides, shape / dtype checks)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wbc_batch
import wbc_capi as capi
import wbc_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("ee_W", "ee_w", "ee_gain", "trunk_W", "trunk_w", "trunk_gain", "com_W", "com_gain", "joint_w")


def test_struct_is_85_doubles_with_the_config_offsets():
    assert C.sizeof(capi.WbcTaskParams) == 85 * 8 == capi.TASK_PARAMS_DOUBLES * 8
    base = capi.WbcConfig.ee_W.offset
    assert [f for f, _ in capi.WbcTaskParams._fields_] == list(FIELDS)
    for f in FIELDS:
        assert getattr(capi.WbcTaskParams, f).offset == getattr(capi.WbcConfig, f).offset - base, f
        assert getattr(capi.WbcTaskParams, f).size == getattr(capi.WbcConfig, f).size, f


def test_header_declares_the_struct_and_the_entry_points():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    body = re.search(r"typedef struct WbcTaskParams \{(.*?)\} WbcTaskParams;", header, re.S).group(1)
    names = re.findall(r"double ([a-zA-Z_]+)", body) + re.findall(r", ([a-z_]+)(?=[\[;,])", body)
    assert set(FIELDS) <= set(names)
    for name in ("wbc_tick_tp", "wbc_assemble_tp", "wbc_rollout_tp"):
        assert name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)
    lib = capi.load_library()
    for name in ("wbc_tick_tp", "wbc_assemble_tp", "wbc_rollout_tp"):
        assert hasattr(lib, name)


def test_layout_map_covers_the_row():
    seen = np.zeros(85, dtype=int)
    for f in FIELDS:
        sl, shape = wbc_model.TASK_PARAMS_LAYOUT[f]
        assert sl.stop - sl.start == int(np.prod(shape)) if shape else sl.stop - sl.start == 1
        assert sl.start * 8 == getattr(capi.WbcTaskParams, f).offset
        assert wbc_model.TASK_PARAMS_SLICES[f] == sl
        seen[sl] += 1
    assert (seen == 1).all()


def _row_of(cfg):
    """the 85 doubles of cfg from ee_W on, read straight from the struct's memory"""
    raw = (C.c_double * 85).from_buffer_copy(bytes(cfg)[capi.WbcConfig.ee_W.offset:capi.WbcConfig.ee_W.offset + 85 * 8])
    return np.array(raw)


@pytest.mark.parametrize("preset", ["sim3", "full", "equality_only"])
def test_rows_reproduce_the_configuration(preset):
    m = wbc_model.load_model("a1_wx200")
    cfg = {"sim3": lambda: wbc_model.sim3_config(m), "equality_only": lambda: wbc_model.equality_only_config(m),
           "full": lambda: wbc_model.make_config(m, Trunk=True, FR=True, FL=True, RR=True, RL=True, Grip=True, Joint=True)}[preset]()
    tp = wbc_model.task_params(cfg, 7)
    assert tp.shape == (7, 85) and tp.dtype == np.float64 and tp.flags.c_contiguous
    assert (tp == _row_of(cfg)).all()
    assert tp[0, wbc_model.TASK_PARAMS_SLICES["joint_w"]][0] == cfg.joint_w
    assert (tp[3, wbc_model.TASK_PARAMS_SLICES["ee_gain"]].reshape(5, 6) == np.ctypeslib.as_array(cfg.ee_gain)).all()


def test_overrides_land_in_their_slices():
    m = wbc_model.load_model("a1_wx200")
    cfg = wbc_model.sim3_config(m)
    B = 6
    rng = np.random.default_rng(0)
    gains = rng.uniform(0.1, 2, (B, 5, 6))
    jw = rng.uniform(1e-4, 1e-2, B)
    tw = rng.uniform(0.5, 5, B)
    tp = wbc_model.task_params(cfg, B, ee_gain=gains, joint_w=jw, trunk_w=tw, com_W=[1.0, 2.0, 3.0])
    S = wbc_model.TASK_PARAMS_SLICES
    assert (tp[:, S["ee_gain"]] == gains.reshape(B, 30)).all()
    assert (tp[:, S["joint_w"]][:, 0] == jw).all() and (tp[:, S["trunk_w"]][:, 0] == tw).all()
    assert (tp[:, S["com_W"]] == [1.0, 2.0, 3.0]).all()                   # (no batch dimension: every instance)
    base = _row_of(cfg)
    untouched = np.ones(85, bool)
    for f in ("ee_gain", "joint_w", "trunk_w", "com_W"):
        untouched[S[f]] = False
    assert (tp[:, untouched] == base[untouched]).all()
    # what the device reads: row b as a WbcTaskParams
    row = capi.WbcTaskParams.from_buffer_copy(tp[2].tobytes())
    assert row.joint_w == jw[2] and row.ee_gain[4][1] == gains[2, 4, 1] and row.trunk_w == tw[2]


def test_wrong_shapes_and_dtypes_raise():
    m = wbc_model.load_model("a1_wx200")
    cfg = wbc_model.sim3_config(m)
    with pytest.raises(ValueError):
        wbc_model.task_params(cfg, 4, ee_gain=np.ones((4, 6, 5)))
    with pytest.raises(ValueError):
        wbc_model.task_params(cfg, 4, joint_w=np.ones(3))
    with pytest.raises(ValueError):
        wbc_model.task_params(cfg, 4, ee_W=np.ones((4, 30)))
    with pytest.raises(KeyError):
        wbc_model.task_params(cfg, 4, damper_coef=np.ones(4))             # per model, not per instance
    with pytest.raises(TypeError):
        wbc_model.task_params(cfg, 4, joint_w=np.array(["a"] * 4))
    with pytest.raises(ValueError):
        wbc_model.task_params(cfg, 0)
    # the batch front end refuses what the kernels would misread
    keep = []
    with pytest.raises(capi.WbcError):
        wbc_batch._task_params(np.zeros((4, 85), np.float32), 4, keep, 0)
    with pytest.raises(capi.WbcError):
        wbc_batch._task_params(np.zeros((4, 84)), 4, keep, 0)
    with pytest.raises(capi.WbcError):
        wbc_batch._task_params(np.zeros((5, 85)), 4, keep, 0)
    with pytest.raises(capi.WbcError):
        wbc_batch._task_params(np.zeros((4, 5, 17)), 4, keep, 0)
    assert wbc_batch._task_params(None, 4, keep, 0) is None
    assert wbc_batch._task_params(np.zeros((4, 85)), 4, keep, 0) is not None
