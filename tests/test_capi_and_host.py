"""CPU: the C-ABI library loads and exports every symbol include/wbc.h declares (no compute calls without a GPU),
struct layouts agree, the host-side logic (model blobs, configs, sharding, trajectory) behaves, and the product path
fails loudly when it cannot reach a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wbc_capi as capi
import wbc_model
import wbc_shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    declared = set(re.findall(r"\b(wbc_[a-z_]+)\s*\(", header))
    assert declared == set(capi.SIGNATURES), declared ^ set(capi.SIGNATURES)
    lib = capi.load_library()
    for name in declared:
        assert hasattr(lib, name)
    assert b"gfx950" in lib.wbc_version()


def test_struct_layouts_match_the_library():
    lib = capi.load_library()
    sb, sc = C.c_int32(), C.c_int32()
    assert lib.wbc_abi_sizes(C.byref(sb), C.byref(sc)) == 0
    assert (sb.value, sc.value) == (C.sizeof(capi.WbcModelBlob), C.sizeof(capi.WbcConfig))


def test_model_validation_runs_on_the_host():
    lib = capi.load_library()
    m = wbc_model.load_model("a1_wx200")
    h = C.c_void_p()
    assert lib.wbc_model_create(C.byref(m.blob), C.byref(h)) == 0
    lib.wbc_model_destroy(h)
    bad = capi.WbcModelBlob.from_buffer_copy(m.blob)
    bad.place_R[3][1] = 0.5                                   # rotated placement: refused, not silently mis-computed
    assert lib.wbc_model_create(C.byref(bad), C.byref(h)) == -3
    assert b"rotated joint placement" in lib.wbc_last_error()
    bad = capi.WbcModelBlob.from_buffer_copy(m.blob)
    bad.jtype[1] = capi.JT["RX"]
    assert lib.wbc_model_create(C.byref(bad), C.byref(h)) == -3


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_product_fails_loudly_without_gpu():
    from wbc_batch import WbcBatch
    with pytest.raises(capi.WbcError, match="no HIP device|no CPU fallback"):
        WbcBatch(wbc_model.load_model("a1_wx200"), 4)
    import QP_Wrapper
    with pytest.raises(capi.WbcError):
        QP_Wrapper.QP(np.eye(3), np.zeros(3), -np.ones(3), np.ones(3)).solveQP()


def test_missing_library_is_an_error(tmp_path):
    with pytest.raises(capi.WbcError, match="not built"):
        capi.load_library(str(tmp_path / "nope.so"))


def test_product_never_imports_the_oracle():
    """only tests/, smoke() and bench.py's cpu_baseline leg may touch oracle/ (comments may mention it)."""
    pkg = os.path.join(ROOT, "mech5845m-wbc-for-legged-manipulator_amd")
    bad = re.compile(r"^\s*(import\s+oracle|from\s+oracle\b)|#\s*include\s*[\"<][^\n]*oracle|\borc_[a-z_]+\s*\(|libwbc_oracle", re.M)
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")) or f == "Makefile":
                m = bad.search(open(os.path.join(dirpath, f)).read())
                assert m is None, (f, m.group(0))


def test_configs_follow_the_reference_presets():
    m = wbc_model.load_model("a1_wx200")
    c = wbc_model.sim3_config(m)                               # sim3.py:145-148 + staticReachMode (:1415-1464)
    assert list(c.task_ee) == [0, 0, 0, 0, 1] and c.task_trunk == 0 and c.task_joint == capi.JOINT_PREV
    assert c.con_trunk == 1 and list(c.con_ee) == [1, 1, 1, 1, 0] and c.con_com == 0
    assert list(c.ee_w) == [100, 100, 100, 100, 1] and c.joint_w == 0.001 and c.ee_gain[4][0] == 0.05 and c.ee_gain[0][0] == 0.8
    assert c.lock_from == 23                                   # gripper jid 19 - 2 + 6 (:627-630)
    d = wbc_model.make_config(m, Grip=True, Joint=True)
    assert d.joint_w == 0.05 and d.ee_gain[4][0] == 0.5 and d.task_joint == capi.JOINT_TIKHONOV
    px = wbc_model.load_model("a1_px100_pin_ver")
    assert wbc_model.sim3_config(px).lock_from == 22
    h = wbc_model.make_config(m, Grip=True, Joint="HYBRID")   # sim3.py:145's own posture mode
    assert h.task_joint == capi.JOINT_HYBRID and h.arm_base_id == 14 and h.posture_literal == 1   # getJointId("waist"), :37
    assert wbc_model.make_config(m, Joint="MANI", posture_literal=False).posture_literal == 0
    with pytest.raises(ValueError):
        wbc_model.make_config(m, Grip=True, Joint="SOMETHING")
    qidx, lo, hi, vm, _ = wbc_model.damper_tables(m, compat=True)
    assert list(qidx[:8]) == list(range(8)) and vm[6] == 5.0 and lo[6] == m.q_lo[7]     # quirk C.3
    qidx, lo, hi, vm, _ = wbc_model.damper_tables(m, compat=False)
    assert qidx[6] == 7 and vm[6] == 52.4


def test_shard_ranges_partition_the_batch():
    for n, w in ((524288, 8), (65536, 1), (10, 4), (7, 8)):
        got = [wbc_shard.shard_range(n, r, w) for r in range(w)]
        assert got[0][0] == 0 and got[-1][1] == n
        assert all(got[i][1] == got[i + 1][0] for i in range(w - 1))
        sizes = [hi - lo for lo, hi in got]
        assert max(sizes) - min(sizes) <= 1
    assert wbc_shard.shard_range(524288, 3, 8) == (196608, 262144)     # BASELINE config 4: 8 x 65536


def test_linear_trajectory_is_klampt_piecewise_linear():
    from Robot_Wrapper4 import _LinearTrajectory
    tr = _LinearTrajectory([[0, 0, 0], [1, 2, 3], [1, 0, 3]])
    assert tr.eval(0) == [0, 0, 0] and tr.eval(-1) == [0, 0, 0] and tr.eval(5) == [1, 0, 3]
    assert np.allclose(tr.eval(0.25), [0.25, 0.5, 0.75]) and np.allclose(tr.eval(1.5), [1, 1, 3])


def test_array_shapes_are_checked_on_the_host():
    """wbc_batch._prep is the gate in front of every raw pointer: B x width values with B leading, or an error."""
    import wbc_batch
    keep = []
    assert wbc_batch._prep(np.zeros((4, 27)), np.float64, keep, 4, 27, "q")
    assert wbc_batch._prep(np.zeros((4, 5, 3)), np.float64, keep, 4, 15, "ee_target")
    assert wbc_batch._prep(None, np.float64, keep, 4, 15, "ee_target") is None
    for bad in (np.zeros((4, 26)), np.zeros((3, 27)), np.zeros(4 * 27), np.zeros((27, 4))):
        with pytest.raises(capi.WbcError, match="q: shape"):
            wbc_batch._prep(bad, np.float64, keep, 4, 27, "q")
    assert set(wbc_batch.TICK_IN_WIDTH) == {n for n, _ in capi.WbcTickIn._fields_}


def test_every_option_and_statistic_is_documented_in_the_header():
    """include/wbc.h is the boundary's only documentation: every name wbc_batch_set_option / wbc_batch_get_stat accept (read off csrc/wbc_api.hip)
    must be described there — a knob a maintainer cannot find does not exist."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    api = open(os.path.join(root, "mech5845m-wbc-for-legged-manipulator_amd", "csrc", "wbc_api.hip")).read()
    hdr = open(os.path.join(root, "include", "wbc.h")).read()
    for fn in ("wbc_batch_set_option", "wbc_batch_get_stat"):
        a = api.index("int " + fn)
        names = re.findall(r'!strcmp\(name, "(\w+)"\)', api[a:api.index("\n}\n", a)])
        assert len(names) >= 9, (fn, names)
        missing = [n for n in names if '"%s"' % n not in hdr]
        assert not missing, (fn, missing)
    assert '"refine"' in hdr and "numRefinementSteps" in hdr and '"packed_min_batch"' in hdr


def test_device_case_table_covers_every_row_of_the_variant_tables():
    """The case table of tests/test_gpu_device_inplace.py holds exactly as many distinct rows per kernel family as the family's variant table
    (wbc_variant_count: generated from the table, needs no device) — a variant added to a table without its case fails here, without a GPU;
    on the GPU the census of that module shows that each case reaches the row it names. An unknown family is refused."""
    import test_gpu_device_inplace as dev
    lib = capi.load_library()
    assert {fam for fam, _, _ in dev.CASES} == set(capi.VARIANT_FAMILIES)
    for fam in capi.VARIANT_FAMILIES:
        n = lib.wbc_variant_count(fam.encode())
        assert n == capi.variant_count(fam) and n > 0
        rows = dev.case_rows(fam)
        assert len(rows) == n, (fam, len(rows), n)
        assert len([c for c in dev.CASES if c[0] == fam]) == n, fam                      # ... and no row twice
        assert all(len(r) == len(dev.FLAG_NAMES[fam]) and all(0 <= a < 256 for a in r) for r in rows), fam
        assert len({dev.key_of(r) for r in rows}) == n
    assert all(capi.variant_args(dev.key_of(flags), len(flags)) == flags for _, flags, _ in dev.CASES)
    assert lib.wbc_variant_count(b"sim3") < 0 and b"unknown kernel family" in lib.wbc_last_error()
    assert lib.wbc_variant_count(None) < 0
    with pytest.raises(capi.WbcError, match="unknown kernel family"):
        capi.variant_count("nope")
