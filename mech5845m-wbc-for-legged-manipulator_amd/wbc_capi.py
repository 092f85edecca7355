"""ctypes mirror of include/wbc.h and loader of the HIP shared library.

This directory is a flat module directory, like the reference's ``wrappers/`` (its modules import each
other as ``from QP_Wrapper import QP``, reference wrappers/Robot_Wrapper4.py:6): put it on ``sys.path``
in place of ``wrappers/`` and ``QP_Wrapper`` / ``Robot_Wrapper4`` resolve to the MI355X versions.

There is no CPU fallback: if ``csrc/build/libwbc_hip.so`` is missing or does not load, importing the
product classes fails loudly.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WBC_HIP_LIB") or os.path.join(HERE, "csrc", "build", "libwbc_hip.so")   # WBC_HIP_LIB: e.g. the profile build

# ---- limits (include/wbc.h)
MAX_JOINTS, MAX_NQ, MAX_NV, NEE, MAX_FRAMES, MAX_P, MAX_M, MAX_MODELS = 24, 28, 26, 5, 16, 24, 96, 4
Q_STRIDE, V_STRIDE = 27, 26
JT = dict(UNIVERSE=0, FF=1, RX=2, RY=3, RZ=4, PX=5, PY=6, PZ=7)
FR_EE0, FR_TRUNK, FR_HIP0, FR_ARM_BASE, FR_NROLES = 0, 5, 6, 11, 12
MEM_HOST, MEM_DEVICE = 0, 1
QP_OPTIMAL, QP_MAX_ITER, QP_INFEASIBLE, QP_NUMERICAL = 0, 1, 2, 3
JOINT_OFF, JOINT_TIKHONOV, JOINT_PREV, JOINT_MANI, JOINT_HYBRID, JOINT_CUSTOM = 0, 1, 2, 3, 4, 5

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)


class WbcModelBlob(C.Structure):
    _fields_ = [
        ("nq", C.c_int32), ("nv", C.c_int32), ("njoints", C.c_int32),
        ("jtype", C.c_int32 * MAX_JOINTS), ("parent", C.c_int32 * MAX_JOINTS),
        ("idx_q", C.c_int32 * MAX_JOINTS), ("idx_v", C.c_int32 * MAX_JOINTS),
        ("place_R", (C.c_double * 9) * MAX_JOINTS), ("place_p", (C.c_double * 3) * MAX_JOINTS),
        ("mass", C.c_double * MAX_JOINTS), ("com", (C.c_double * 3) * MAX_JOINTS),
        ("q_lo", C.c_double * MAX_NQ), ("q_hi", C.c_double * MAX_NQ), ("v_max", C.c_double * MAX_NV),
        ("nframes", C.c_int32), ("frame_joint", C.c_int32 * MAX_FRAMES),
        ("frame_R", (C.c_double * 9) * MAX_FRAMES), ("frame_p", (C.c_double * 3) * MAX_FRAMES),
        ("ee_joint", C.c_int32 * NEE),
    ]


class WbcConfig(C.Structure):
    _fields_ = [
        ("task_ee", C.c_int32 * NEE), ("task_trunk", C.c_int32), ("task_com", C.c_int32), ("task_joint", C.c_int32),
        ("con_com", C.c_int32), ("con_trunk", C.c_int32), ("con_ee", C.c_int32 * NEE),
        ("use_bounds", C.c_int32), ("lock_from", C.c_int32),
        ("arm_base_id", C.c_int32), ("posture_literal", C.c_int32),
        ("damper_qidx", C.c_int32 * MAX_NV),
        ("damper_lo", C.c_double * MAX_NV), ("damper_hi", C.c_double * MAX_NV), ("damper_vmax", C.c_double * MAX_NV),
        ("damper_coef", C.c_double), ("damper_qi", C.c_double), ("damper_qs", C.c_double),
        ("ee_W", (C.c_double * 6) * NEE), ("ee_w", C.c_double * NEE), ("ee_gain", (C.c_double * 6) * NEE),
        ("trunk_W", C.c_double * 6), ("trunk_w", C.c_double), ("trunk_gain", C.c_double * 6),
        ("com_W", C.c_double * 3), ("com_gain", C.c_double * 3),
        ("joint_w", C.c_double),
        ("trunk_box_z_frac", C.c_double), ("trunk_box_ang", C.c_double), ("trunk_box_scale", C.c_double),
        ("com_box_scale", C.c_double),
    ]


class WbcTickIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "q", "ee_target", "prev_ee_target", "trunk_target", "prev_trunk_target", "trunk_box_center",
        "ee_ref_rot", "ee_prev_rot", "trunk_ref_euler", "trunk_prev_rot", "com_target", "com_target_vel", "model_id",
        "posture_u", "q_con", "working_set")]


class WbcQpData(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("A", "b", "H", "g", "C", "Clb", "Cub", "lb", "ub")]


class WbcTickOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("qdot", "status", "iters", "q_next", "working_set")]


ROLLOUT_RUNNING, ROLLOUT_WARMUP = 0, 1


class WbcRollout(C.Structure):
    _fields_ = [("ticks", C.c_int32), ("mode", C.c_int32)] + [(n, C.c_void_p) for n in (
        "ee_target_step", "trunk_target_step", "imu", "q_final", "qdot_last", "ee_target_final", "grip_trace",
        "status_max", "iters_sum")] + [("hold_ticks", C.c_int32), ("pad_", C.c_int32)]


# wbc_rollout_traj: per-instance milestone trajectory of one end effector's target, and the roll-out summary (include/wbc.h)
MAX_TRAJ_POINTS = 32


class WbcTrajectory(C.Structure):
    _fields_ = [("max_points", C.c_int32), ("ee_index", C.c_int32), ("points", C.c_void_p), ("n_points", C.c_void_p), ("du", C.c_void_p),
                ("du_all", C.c_double)]


class WbcRolloutSummary(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("err_sq_sum", "err_max", "err_max_tick", "err_final", "first_bad_tick", "bad_ticks")] + [
        ("group_size", C.c_int32), ("pad_", C.c_int32)] + [(n, C.c_void_p) for n in (
            "group_rms", "group_err_max", "group_worst_status", "group_bad_instances")]


# wbc_rollout_tracks: several followed targets (end effectors 0..4 and the trunk, 5), linear or Hermite, any frame scored (include/wbc.h)
MAX_TRACKS, TARGET_TRUNK = 6, 5
TRACK_LINEAR, TRACK_HERMITE = 0, 1


class WbcTrack(C.Structure):
    _fields_ = [("target", C.c_int32), ("kind", C.c_int32), ("max_points", C.c_int32), ("pad_", C.c_int32), ("points", C.c_void_p),
                ("tangents", C.c_void_p), ("n_points", C.c_void_p), ("du", C.c_void_p), ("du_all", C.c_double)]


class WbcTracks(C.Structure):
    _fields_ = [("n_tracks", C.c_int32), ("pad_", C.c_int32), ("track", WbcTrack * MAX_TRACKS), ("trunk_target_final", C.c_void_p)]


class WbcTrackScores(C.Structure):
    _fields_ = [("score_mask", C.c_int32), ("group_size", C.c_int32)] + [(n, C.c_void_p) for n in (
        "err_sq_sum", "err_max", "err_final", "err_max_tick", "first_bad_tick", "bad_ticks", "trace", "group_rms", "group_err_max",
        "group_worst_status", "group_bad_instances")]


# wbc_state_slack / wbc_rollout_watch: slack of the CoM box, the trunk box (z, angles) and the joint range (include/wbc.h)
N_SLACK, N_SLACK_COMPONENTS = 4, 12
SLACK_COM, SLACK_TRUNK_Z, SLACK_TRUNK_ANG, SLACK_JOINT = 0, 1, 2, 3


class WbcSlackOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("slack", "which", "components")]


class WbcSlackWatch(C.Structure):
    _fields_ = [("mask", C.c_int32), ("group_size", C.c_int32)] + [(n, C.c_void_p) for n in (
        "slack_min", "slack_final", "slack_min_tick", "slack_min_which", "neg_ticks", "first_neg_tick", "trace", "group_min",
        "group_neg_instances")]


# wbc_qp_certificate: dual solution, KKT certificate and sensitivities of a solved QP (include/wbc.h)
CERT_OK, CERT_UNSOLVED, CERT_DEPENDENT, CERT_NUMERICAL = 0, 1, 2, 3


class WbcQpProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("p", C.c_int32), ("m", C.c_int32), ("pad_", C.c_int32)] + [(n, C.c_void_p) for n in (
        "H", "g", "A", "b", "C", "lb", "ub", "Clb", "Cub", "x", "status", "working_set", "v")]


class WbcQpCert(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("y_bounds", "y_rows", "kkt", "objective", "n_active", "sens_x", "sens_bounds", "sens_rows",
                                          "cert_status")]


# wbc_tick_vjp: dL/d(task weights, gains, targets) of a solved tick (include/wbc.h)
GRAD_OK, GRAD_UNSOLVED, GRAD_CERT, GRAD_NONFINITE = 0, 1, 2, 3
TICK_GRAD_FIELDS = dict(d_task_params=(85,), d_ee_target=(NEE, 3), d_prev_ee_target=(NEE, 3), d_trunk_target=(3,), d_prev_trunk_target=(3,),
                        d_com_target=(3,), d_com_target_vel=(3,), d_posture_u=(V_STRIDE,))     # output name -> per-instance shape


class WbcTickGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in tuple(TICK_GRAD_FIELDS) + ("grad_status",)]


# wbc_tick_vjp_state: dL/dq (tangent coordinates) and dL/d trunk_box_center of a solved tick (include/wbc.h)
TICK_SENS_FIELDS = ("qdot", "sens_x", "sens_bounds", "sens_rows", "y_rows", "status", "cert_status", "working_set")
TICK_STATE_GRAD_FIELDS = dict(d_q=(V_STRIDE,), d_trunk_box_center=(4,))     # output name -> per-instance shape


class WbcTickSens(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TICK_SENS_FIELDS]


class WbcTickStateGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in tuple(TICK_STATE_GRAD_FIELDS) + ("grad_status",)]


# wbc_step_vjp: dL/d(q, qdot, foot targets) of the state step between two ticks (include/wbc.h)
STEP_GRAD_FIELDS = dict(d_q=(V_STRIDE,), d_qdot=(V_STRIDE,), d_foot_targets=(5, 3))     # output name -> per-instance shape


class WbcStepGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in tuple(STEP_GRAD_FIELDS) + ("grad_status",)]


# wbc_rollout_record / wbc_rollout_vjp: the reverse sweep over a recorded roll-out (include/wbc.h)
ROLLOUT_SEED_FIELDS = ("g_q_final", "g_qdot_last", "g_q_trace")
ROLLOUT_GRAD_FIELDS = dict(d_q0=(V_STRIDE,), d_task_params=(85,), d_ee_target=(NEE, 3), d_prev_ee_target=(NEE, 3), d_trunk_target=(3,),
                           d_prev_trunk_target=(3,), d_com_target=(3,), d_com_target_vel=(3,), d_posture_u=(V_STRIDE,), d_trunk_box_center=(4,),
                           d_ee_target_step=(NEE, 3), d_trunk_target_step=(3,))     # output name -> per-instance shape
TAPE_HEAD_BYTES, TAPE_TICK_BYTES = 432, 736     # per instance; per instance and tick (wbc_rollout_tape_bytes)


class WbcRolloutSeed(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ROLLOUT_SEED_FIELDS]


class WbcRolloutGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in tuple(ROLLOUT_GRAD_FIELDS) + ("grad_status", "ticks_dropped")]


# wbc_rollout_record_tracks / wbc_rollout_vjp_tracks: the sweep's outputs per track (include/wbc.h); the shapes are per instance, S = max_points
TRACK_GRAD_FIELDS = dict(d_points=("S", 3), d_tangents=("S", 3), d_du=())


class WbcTrackGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TRACK_GRAD_FIELDS]


class WbcTracksGrad(C.Structure):
    _fields_ = [("track", WbcTrackGrad * MAX_TRACKS)]


# wbc_rollout_vjp_scored: the cotangents of the track scores as a seed of the sweep (include/wbc.h)
SCORE_SEED_FIELDS = ("g_err_sq_sum", "g_err_final", "g_err_max", "err_max_tick", "q_final")


class WbcScoreSeed(C.Structure):
    _fields_ = [("score_mask", C.c_int32), ("pad_", C.c_int32)] + [(n, C.c_void_p) for n in SCORE_SEED_FIELDS]


# wbc_state_slack_vjp: dL/dq (tangent coordinates) and dL/d trunk_box_center of the slack families at a state (include/wbc.h)
SLACK_GRAD_FIELDS = dict(d_q=(V_STRIDE,), d_trunk_box_center=(4,))     # output name -> per-instance shape


class WbcSlackGrad(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in tuple(SLACK_GRAD_FIELDS) + ("which", "grad_status")]


# wbc_rollout_vjp_watched: the cotangents of the watch's results as a seed of the sweep (include/wbc.h)
WATCH_SEED_FIELDS = ("g_slack_min", "g_slack_final", "g_trace", "slack_min_tick", "q_final")


class WbcWatchSeed(C.Structure):
    _fields_ = [("mask", C.c_int32), ("pad_", C.c_int32)] + [(n, C.c_void_p) for n in WATCH_SEED_FIELDS]


class WbcFkOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("oMi", "oMf", "J", "com", "Jcom")]


# the weight / gain block of WbcConfig (ee_W .. joint_w), one row per instance: wbc_tick_tp / wbc_assemble_tp / wbc_rollout_tp
class WbcTaskParams(C.Structure):
    _fields_ = [
        ("ee_W", (C.c_double * 6) * NEE), ("ee_w", C.c_double * NEE), ("ee_gain", (C.c_double * 6) * NEE),
        ("trunk_W", C.c_double * 6), ("trunk_w", C.c_double), ("trunk_gain", C.c_double * 6),
        ("com_W", C.c_double * 3), ("com_gain", C.c_double * 3),
        ("joint_w", C.c_double),
    ]


TASK_PARAMS_DOUBLES = 85


# every symbol include/wbc.h declares, with its ctypes signature
_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
SIGNATURES = {
    "wbc_model_create": (_i, [C.POINTER(WbcModelBlob), C.POINTER(_vp)]),
    "wbc_model_destroy": (None, [_vp]),
    "wbc_batch_create": (_i, [C.POINTER(_vp), _i, _i, _i, C.POINTER(_vp)]),
    "wbc_batch_destroy": (None, [_vp]),
    "wbc_batch_configure": (_i, [_vp, _i, C.POINTER(WbcConfig)]),
    "wbc_task_rows": (_i, [_vp]),
    "wbc_constraint_rows": (_i, [_vp]),
    "wbc_fk_jacobians": (_i, [_vp, _i, _vp, _vp, _i, C.POINTER(WbcFkOut), _vp]),
    "wbc_assemble": (_i, [_vp, _i, C.POINTER(WbcTickIn), _d, _i, C.POINTER(WbcQpData), _vp]),
    "wbc_qp_solve": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wbc_qp_solve_ls": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wbc_qp_certificate": (_i, [_vp, _i, C.POINTER(WbcQpProblem), C.POINTER(WbcQpCert), _i, _vp]),
    "wbc_qp_certificate_sizes": (_i, [c_int32_p, c_int32_p]),
    "wbc_tick_vjp": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, _vp, _vp, _vp, _vp, _i, C.POINTER(WbcTickGrad), _vp]),
    "wbc_tick_grad_sizes": (_i, [c_int32_p]),
    "wbc_tick_vjp_state": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcTickSens), _i, C.POINTER(WbcTickStateGrad), _vp]),
    "wbc_tick_state_grad_sizes": (_i, [c_int32_p, c_int32_p]),
    "wbc_step_vjp": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _d, _i, _vp, _i, C.POINTER(WbcStepGrad), _vp]),
    "wbc_step_grad_sizes": (_i, [c_int32_p]),
    "wbc_posture_target": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "wbc_tick": (_i, [_vp, _i, C.POINTER(WbcTickIn), _d, _i, C.POINTER(WbcTickOut), _vp]),
    "wbc_update_state": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "wbc_rollout": (_i, [_vp, _i, C.POINTER(WbcTickIn), _d, C.POINTER(WbcRollout), _i, _vp]),
    "wbc_tick_tp": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, _i, C.POINTER(WbcTickOut), _vp]),
    "wbc_assemble_tp": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, _i, C.POINTER(WbcQpData), _vp]),
    "wbc_rollout_tp": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), _i, _vp]),
    "wbc_rollout_tape_bytes": (C.c_size_t, [_i, _i]),
    "wbc_rollout_record": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), _vp, C.c_size_t, _vp, _i, _vp]),
    "wbc_rollout_vjp": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), _vp, C.c_size_t, C.POINTER(WbcRolloutSeed), _i,
                             C.POINTER(WbcRolloutGrad), _vp]),
    "wbc_rollout_grad_sizes": (_i, [c_int32_p, c_int32_p]),
    "wbc_rollout_record_tracks": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), C.POINTER(WbcTracks),
                                       C.POINTER(WbcTrackScores), _vp, C.c_size_t, _vp, _i, _vp]),
    "wbc_rollout_vjp_tracks": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), C.POINTER(WbcTracks), _vp, C.c_size_t,
                                    C.POINTER(WbcRolloutSeed), _i, C.POINTER(WbcRolloutGrad), C.POINTER(WbcTracksGrad), _vp]),
    "wbc_rollout_tracks_grad_sizes": (_i, [c_int32_p, c_int32_p]),
    "wbc_rollout_vjp_scored": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), C.POINTER(WbcTracks), _vp, C.c_size_t,
                                    C.POINTER(WbcRolloutSeed), C.POINTER(WbcScoreSeed), _i, C.POINTER(WbcRolloutGrad),
                                    C.POINTER(WbcTracksGrad), _vp]),
    "wbc_rollout_scored_sizes": (_i, [c_int32_p]),
    "wbc_rollout_traj": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), C.POINTER(WbcTrajectory),
                              C.POINTER(WbcRolloutSummary), _i, _vp]),
    "wbc_rollout_tracks": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), C.POINTER(WbcTracks),
                                C.POINTER(WbcTrackScores), _i, _vp]),
    "wbc_state_slack": (_i, [_vp, _i, _vp, _vp, _vp, _i, C.POINTER(WbcSlackOut), _vp]),
    "wbc_rollout_watch": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), C.POINTER(WbcTracks),
                               C.POINTER(WbcTrackScores), C.POINTER(WbcSlackWatch), _i, _vp]),
    "wbc_state_slack_vjp": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(WbcSlackGrad), _vp]),
    "wbc_slack_grad_sizes": (_i, [c_int32_p]),
    "wbc_rollout_record_watch": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), C.POINTER(WbcTracks),
                                      C.POINTER(WbcTrackScores), C.POINTER(WbcSlackWatch), _vp, C.c_size_t, _vp, _i, _vp]),
    "wbc_rollout_vjp_watched": (_i, [_vp, _i, C.POINTER(WbcTickIn), _vp, _d, C.POINTER(WbcRollout), C.POINTER(WbcTracks), _vp, C.c_size_t,
                                     C.POINTER(WbcRolloutSeed), C.POINTER(WbcScoreSeed), C.POINTER(WbcWatchSeed), _i,
                                     C.POINTER(WbcRolloutGrad), C.POINTER(WbcTracksGrad), _vp]),
    "wbc_rollout_watched_sizes": (_i, [c_int32_p]),
    "wbc_integrate": (_i, [_vp, _i, _vp, _vp, _vp, _d, _i, _vp, _vp]),
    "wbc_batch_set_option": (_i, [_vp, C.c_char_p, _i]),
    "wbc_batch_get_stat": (_i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64)]),
    "wbc_batch_synchronize": (_i, [_vp, _vp]),
    "wbc_debug_cycles": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "wbc_last_error": (C.c_char_p, []),
    "wbc_version": (C.c_char_p, []),
    "wbc_abi_sizes": (_i, [c_int32_p, c_int32_p]),
    "wbc_variant_count": (_i, [C.c_char_p]),
}

_lib = None


E_ARG, E_HIP, E_UNSUPPORTED, E_STATE = -1, -2, -3, -4      # include/wbc.h


class WbcError(RuntimeError):
    code = None      # the library's return code where the error comes from a library call (check), else None


def load_library(path=None):
    """dlopen the HIP library and bind every entry point; raises if it is missing (no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise WbcError("HIP extension not built: %s is missing (run `python __graft_entry__.py build`)" % p)
    # PyTorch ships its own copy of the HIP runtime. If this library (linked against /opt/rocm's) is loaded first and torch
    # afterwards, the process ends up with two runtimes and the second one to initialise sees no device. Loading torch
    # first makes both share one runtime; without torch installed there is only ours.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    sb, sc = C.c_int32(), C.c_int32()
    lib.wbc_abi_sizes(C.byref(sb), C.byref(sc))
    if sb.value != C.sizeof(WbcModelBlob) or sc.value != C.sizeof(WbcConfig):
        raise WbcError("ABI mismatch: library (%d, %d) vs ctypes (%d, %d)" % (
            sb.value, sc.value, C.sizeof(WbcModelBlob), C.sizeof(WbcConfig)))
    lib.wbc_qp_certificate_sizes(C.byref(sb), C.byref(sc))
    if sb.value != C.sizeof(WbcQpProblem) or sc.value != C.sizeof(WbcQpCert):
        raise WbcError("ABI mismatch (certificate structs): library (%d, %d) vs ctypes (%d, %d)" % (
            sb.value, sc.value, C.sizeof(WbcQpProblem), C.sizeof(WbcQpCert)))
    lib.wbc_tick_grad_sizes(C.byref(sb))
    if sb.value != C.sizeof(WbcTickGrad):
        raise WbcError("ABI mismatch (WbcTickGrad): library %d vs ctypes %d" % (sb.value, C.sizeof(WbcTickGrad)))
    lib.wbc_tick_state_grad_sizes(C.byref(sb), C.byref(sc))
    if sb.value != C.sizeof(WbcTickSens) or sc.value != C.sizeof(WbcTickStateGrad):
        raise WbcError("ABI mismatch (WbcTickSens / WbcTickStateGrad): library (%d, %d) vs ctypes (%d, %d)" % (
            sb.value, sc.value, C.sizeof(WbcTickSens), C.sizeof(WbcTickStateGrad)))
    lib.wbc_step_grad_sizes(C.byref(sb))
    if sb.value != C.sizeof(WbcStepGrad):
        raise WbcError("ABI mismatch (WbcStepGrad): library %d vs ctypes %d" % (sb.value, C.sizeof(WbcStepGrad)))
    lib.wbc_rollout_grad_sizes(C.byref(sb), C.byref(sc))
    if sb.value != C.sizeof(WbcRolloutSeed) or sc.value != C.sizeof(WbcRolloutGrad):
        raise WbcError("ABI mismatch (WbcRolloutSeed / WbcRolloutGrad): library (%d, %d) vs ctypes (%d, %d)" % (
            sb.value, sc.value, C.sizeof(WbcRolloutSeed), C.sizeof(WbcRolloutGrad)))
    lib.wbc_rollout_tracks_grad_sizes(C.byref(sb), C.byref(sc))
    if sb.value != C.sizeof(WbcTrackGrad) or sc.value != C.sizeof(WbcTracksGrad):
        raise WbcError("ABI mismatch (WbcTrackGrad / WbcTracksGrad): library (%d, %d) vs ctypes (%d, %d)" % (
            sb.value, sc.value, C.sizeof(WbcTrackGrad), C.sizeof(WbcTracksGrad)))
    lib.wbc_rollout_scored_sizes(C.byref(sb))
    if sb.value != C.sizeof(WbcScoreSeed):
        raise WbcError("ABI mismatch (WbcScoreSeed): library %d vs ctypes %d" % (sb.value, C.sizeof(WbcScoreSeed)))
    lib.wbc_slack_grad_sizes(C.byref(sb))
    if sb.value != C.sizeof(WbcSlackGrad):
        raise WbcError("ABI mismatch (WbcSlackGrad): library %d vs ctypes %d" % (sb.value, C.sizeof(WbcSlackGrad)))
    lib.wbc_rollout_watched_sizes(C.byref(sb))
    if sb.value != C.sizeof(WbcWatchSeed):
        raise WbcError("ABI mismatch (WbcWatchSeed): library %d vs ctypes %d" % (sb.value, C.sizeof(WbcWatchSeed)))
    if path is None:
        _lib = lib
    return lib


VARIANT_FAMILIES = ("general", "sim3p", "orthp", "boxp", "qpp", "qp")


def variant_count(family):
    """rows of a kernel family's variant table (wbc_variant_count, include/wbc.h); needs no device. Unknown family: WbcError."""
    lib = load_library()
    n = lib.wbc_variant_count(family.encode())
    if n < 0:
        check(n, lib)
    return n


def variant_args(key, nargs=5):
    """the template arguments behind a "last_tick_variant" / "last_qp_variant" key (include/wbc.h): first argument in the top byte"""
    return tuple((int(key) >> (8 * (4 - i))) & 255 for i in range(nargs))


def check(rc, lib=None):
    if rc != 0:
        lib = lib or load_library()
        e = WbcError("wbc call failed (%d): %s" % (rc, (lib.wbc_last_error() or b"").decode()))
        e.code = rc
        raise e
