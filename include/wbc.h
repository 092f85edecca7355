/*
 * wbc.h — C-ABI of the MI355X batched whole-body-control hot path.
 *
 * This is the drop-in boundary for the per-tick hot loop of the reference
 * (joey156/MECH5845M-WBC-for-Legged-Manipulator):
 *
 *   RobotModel.runWBC            wrappers/Robot_Wrapper4.py:1330-1412
 *     -> updateState             wrappers/Robot_Wrapper4.py:387-428     (FK, joint Jacobians, frames)
 *     -> qpA / qpb               wrappers/Robot_Wrapper4.py:1271-1294   (task stack A, b)
 *     -> findConstraints         wrappers/Robot_Wrapper4.py:764-836     (C, Clb, Cub)
 *     -> velDamperJointConstraints  wrappers/Robot_Wrapper4.py:572-637  (lb, ub)
 *     -> QP.solveQP / solveQPHotstart  wrappers/QP_Wrapper.py:23-73     (H = A'A, g = -A'b, QP)
 *     -> jointVelocitiestoConfig wrappers/Robot_Wrapper4.py:440-449     (pin.integrate)
 *
 * The reference has no FFI layer (it is pure Python calling pinocchio + qpOASES); the boundary is
 * its two Python classes `QP` and `RobotModel`.  The Python mirrors in
 * mech5845m-wbc-for-legged-manipulator_amd/{QP_Wrapper,Robot_Wrapper4}.py keep those signatures and
 * bind the entry points below through ctypes.
 *
 * Conventions: plain C types only; all matrices row-major fp64; every per-instance array is
 * [B][k] with an instance's k values contiguous; quaternions are (x, y, z, w) as in pinocchio,
 * PyBullet and scipy; Jacobian rows are linear 0-2, angular 3-5 (pinocchio Motion order).
 * Buffers are caller-allocated; `mem` says whether the pointers are host (the library stages them
 * through its own device workspace) or device pointers (used in place, zero copies).
 * With device pointers every call only enqueues kernels (and, on first use of a feature, allocates its workspace):
 * after one warm-up call the same call sequence can be captured into a hipGraph on the caller's stream.
 * Return value: 0 = ok, negative = API-level failure (message via wbc_last_error()).  Per-instance
 * solver outcome goes to the `status` array.  No global state except the thread-local error string;
 * handles are not thread-safe, independent handles may be used concurrently.
 */
#ifndef WBC_H_
#define WBC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ limits */
#define WBC_MAX_JOINTS 24  /* model joints incl. universe (a1_wx200: 22)                           */
#define WBC_MAX_NQ 28      /* a1_wx200: 27                                                          */
#define WBC_MAX_NV 26      /* a1_wx200: 26 = QP size n; one wavefront lane per DoF   */
#define WBC_NEE 5          /* end effectors in reference order FR, FL, RR, RL, GRIP (sim3.py:56)    */
#define WBC_MAX_FRAMES 16
#define WBC_MAX_P 24       /* constraint rows: CoM 2 + trunk 4 + 5 EE x 3 = 21 max                  */
#define WBC_MAX_M 96       /* task rows accepted by wbc_qp_solve_ls (A is m x n)                    */
#define WBC_MAX_MODELS 4   /* morphologies interleaved in one batch (BASELINE config 5)             */
#define WBC_MFMA_AUTO_ROWS 30 /* "auto" puts H = A'A on the fp64 matrix cores from this many rows of A on    */

/* joint types (pinocchio JointModel*) */
enum { WBC_JT_UNIVERSE = 0, WBC_JT_FF = 1, WBC_JT_RX = 2, WBC_JT_RY = 3, WBC_JT_RZ = 4,
       WBC_JT_PX = 5, WBC_JT_PY = 6, WBC_JT_PZ = 7 };

/* controller frame roles: index into WbcModelBlob.frame_* */
enum { WBC_FR_EE0 = 0 /* ..4: FR, FL, RR, RL foot_fixed, gripper_bar */, WBC_FR_TRUNK = 5,
       WBC_FR_HIP0 = 6 /* ..10: FR/FL/RR/RL hip joint frames, waist */, WBC_FR_ARM_BASE = 11,
       WBC_FR_NROLES = 12 };

enum { WBC_MEM_HOST = 0, WBC_MEM_DEVICE = 1 };

/* per-instance solver status */
enum { WBC_QP_OPTIMAL = 0, WBC_QP_MAX_ITER = 1, WBC_QP_INFEASIBLE = 2, WBC_QP_NUMERICAL = 3 };

/* posture-task mode = RobotModel.task_active_Joint (Robot_Wrapper4.py:1209-1268) */
enum { WBC_JOINT_OFF = 0, WBC_JOINT_TIKHONOV = 1 /* True */, WBC_JOINT_PREV = 2 /* "PREV" */,
       WBC_JOINT_MANI = 3 /* "MANI": manipulability gradient, :1220-1242 */,
       WBC_JOINT_HYBRID = 4 /* "HYBRID": PREV for the quadruped + manipulability gradient for the arm, :1245-1260 */,
       WBC_JOINT_CUSTOM = 5 /* u supplied per instance in WbcTickIn.posture_u */ };

/* API return codes */
enum { WBC_OK = 0, WBC_E_ARG = -1, WBC_E_HIP = -2, WBC_E_UNSUPPORTED = -3, WBC_E_STATE = -4 };

/* ------------------------------------------------------------------ model
 * What pin.buildModelFromUrdf(urdf, JointModelFreeFlyer()) holds that the path reads
 * (Robot_Wrapper4.py:21); produced by tools/bake_model.py, SURVEY.md Appendix A. */
typedef struct WbcModelBlob {
  int32_t nq, nv, njoints;               /* njoints includes universe (index 0)                   */
  int32_t jtype[WBC_MAX_JOINTS];
  int32_t parent[WBC_MAX_JOINTS];
  int32_t idx_q[WBC_MAX_JOINTS];
  int32_t idx_v[WBC_MAX_JOINTS];
  double place_R[WBC_MAX_JOINTS][9];     /* joint placement in parent joint frame (row-major); the
                                          * identity or a proper rotation (orthonormal, det +1, both
                                          * within 1e-12: the ViperX-300's rpy="3.14 0 0"); the root
                                          * joint's is the identity                                */
  double place_p[WBC_MAX_JOINTS][3];
  double mass[WBC_MAX_JOINTS];           /* lumped body (fixed children merged), joint frame      */
  double com[WBC_MAX_JOINTS][3];
  double q_lo[WBC_MAX_NQ], q_hi[WBC_MAX_NQ]; /* model.lower/upperPositionLimit (nq-sized)         */
  double v_max[WBC_MAX_NV];                  /* model.velocityLimit (nv-sized)                     */
  int32_t nframes;                       /* >= WBC_FR_NROLES                                      */
  int32_t frame_joint[WBC_MAX_FRAMES];   /* supporting joint                                      */
  double frame_R[WBC_MAX_FRAMES][9];     /* placement in the supporting joint's frame: must be the
                                          * identity (no robot of the reference needs a rotated
                                          * frame offset; any other is refused)                   */
  double frame_p[WBC_MAX_FRAMES][3];
  int32_t ee_joint[WBC_NEE];             /* end_effector_index_list_joint (Robot_Wrapper4.py:49)  */
} WbcModelBlob;

/* ------------------------------------------------------------------ batch-uniform settings
 * = the RobotModel attributes set by __init__/setTasks/setConstraints/staticReachMode
 * (Robot_Wrapper4.py:72-125, 176-193, 1415-1464). 6x6 weights/gains are diagonal in every preset
 * of the reference, so only the diagonals cross the ABI (the Python mirror refuses non-diagonal). */
typedef struct WbcConfig {
  int32_t task_ee[WBC_NEE];    /* task_active_{FR,FL,RR,RL}_foot, task_active_GRIP                */
  int32_t task_trunk;          /* task_active_Trunk                                               */
  int32_t task_com;            /* Robot_Wrapper2 taskActiveCoM (Robot_Wrapper2.py:600-603)        */
  int32_t task_joint;          /* WBC_JOINT_*                                                     */
  int32_t con_com, con_trunk;  /* const_active_CoM / _Trunk                                       */
  int32_t con_ee[WBC_NEE];     /* const_active_{FR,FL,RR,RL}_foot, const_active_GRIP              */
  int32_t use_bounds;          /* 1: velDamperJointConstraints box; 0: no box (equality-only QP)  */
  int32_t lock_from;           /* DoF >= lock_from get lb = ub = 0 (Robot_Wrapper4.py:627-630)    */
  int32_t arm_base_id;         /* model.getJointId(G_base) (Robot_Wrapper4.py:37): HYBRID differentiates joints >= it */
  int32_t posture_literal;     /* MANI/HYBRID: 1 = the reference's arithmetic to the letter (q is perturbed at
                                  the velocity index, perturbations accumulate, and the perturbed configuration is what
                                  findConstraints / velDamperJointConstraints / integrate then see); 0 = the intended
                                  central difference (own q index, configuration restored)                           */
  int32_t damper_qidx[WBC_MAX_NV]; /* which q entry DoF i's damper looks at (quirk C.3)           */
  double damper_lo[WBC_MAX_NV], damper_hi[WBC_MAX_NV], damper_vmax[WBC_MAX_NV];
  double damper_coef, damper_qi, damper_qs;      /* 0.01, 0.026, 0.015 (Robot_Wrapper4.py:574-576) */
  double ee_W[WBC_NEE][6];     /* diag(EE_weight[i])                                              */
  double ee_w[WBC_NEE];        /* cart_task_weight_EE_list[i]                                     */
  double ee_gain[WBC_NEE][6];  /* diag(EE_gains[i]), indexed by EE index as at Robot_Wrapper4.py:908 */
  double trunk_W[6], trunk_w, trunk_gain[6];
  double com_W[3], com_gain[3];
  double joint_w;              /* joint_task_weight                                               */
  double trunk_box_z_frac;     /* 0.25  (Robot_Wrapper4.py:719)                                   */
  double trunk_box_ang;        /* 0.15  (Robot_Wrapper4.py:720-722)                               */
  double trunk_box_scale;      /* 0.5   (Robot_Wrapper4.py:735-736)                               */
  double com_box_scale;        /* 0.8   (Robot_Wrapper4.py:675-677)                               */
} WbcConfig;

/* ------------------------------------------------------------------ per-instance task weights and gains
 * The weight / gain block of WbcConfig (ee_W .. joint_w: 85 contiguous doubles, same names, order and meaning, the ee_gain
 * indexing of Robot_Wrapper4.py:908 included), one row per instance: what a weight / gain sweep or domain randomisation varies.
 * Passed as `tp` [B] to wbc_tick_tp / wbc_assemble_tp / wbc_rollout_tp, in the same memory kind as the call's other arrays; row b
 * replaces the block of cfgs[model_id[b]] for instance b only (switches, posture mode, damper tables, box constants and lock_from
 * stay per model). Rows are read on the device by every call. A row with a non-finite entry or joint_w == 0 (H = A'A singular)
 * gives its instance WBC_QP_NUMERICAL and zero qdot; the other instances are unaffected. */
typedef struct WbcTaskParams {
  double ee_W[WBC_NEE][6];     /* diag(EE_weight[i])                                              */
  double ee_w[WBC_NEE];        /* cart_task_weight_EE_list[i]                                     */
  double ee_gain[WBC_NEE][6];  /* diag(EE_gains[i]), indexed by EE index as at Robot_Wrapper4.py:908 */
  double trunk_W[6], trunk_w, trunk_gain[6];
  double com_W[3], com_gain[3];
  double joint_w;              /* joint_task_weight                                               */
} WbcTaskParams;
#define WBC_TASK_PARAMS_DOUBLES 85

/* ------------------------------------------------------------------ per-instance tick inputs
 * (the arguments of runWBC plus the controller state it reads). NULL is allowed where noted. */
typedef struct WbcTickIn {
  const double* q;                 /* [B][WBC_MAX_NQ-1=27] current_joint_config (xyz, quat xyzw, joints) */
  const double* ee_target;         /* [B][5][3] target_cartesian_pos_EE                               */
  const double* prev_ee_target;    /* [B][5][3] prev_EE_pos                                           */
  const double* trunk_target;      /* [B][3]    target_cartesian_pos_trunk     (NULL if no trunk task) */
  const double* prev_trunk_target; /* [B][3]    prev_trunk_ref                 (NULL if no trunk task) */
  const double* trunk_box_center;  /* [B][4]    initial_trunk_pos[2], initial_trunk_ori_euler (NULL if no trunk constraint) */
  const double* ee_ref_rot;        /* [B][5][9] R* = from_euler('xyz', default_EE_ori_list[i]); NULL => R* == R*_prev (omega_ref = 0) */
  const double* ee_prev_rot;       /* [B][5][9] prev_EE_CoM_rot                                       */
  const double* trunk_ref_euler;   /* [B][3]    default_trunk_ori              (NULL if no trunk task) */
  const double* trunk_prev_rot;    /* [B][9]    old_ref_trunk_rot_matrix       (NULL if no trunk task) */
  const double* com_target;        /* [B][3]    Robot_Wrapper2 target_cartesian_pos_CoM (NULL if no CoM task) */
  const double* com_target_vel;    /* [B][3]    Robot_Wrapper2 target_cartesian_vel_CoM               */
  const int32_t* model_id;         /* [B] index into the batch's models; NULL => all model 0          */
  const double* posture_u;         /* [B][26]   posture target u of qpJointb before the (1/nv) w scaling: required for
                                                WBC_JOINT_CUSTOM; for MANI/HYBRID NULL => computed by the library (wbc_posture_target) */
  const double* q_con;             /* [B][27]   configuration seen by findConstraints, velDamperJointConstraints and integrate when it
                                                differs from q (the state qpJointb MANI/HYBRID leaves behind); NULL => q          */
  const uint64_t* working_set;     /* [B][2]    warm start = what solveQPHotstart keeps between ticks (QP_Wrapper.py:55-73, the qpOASES
                                                object's working set): WbcTickOut.working_set of the previous tick. Word 0: velocity
                                                bounds (bit d: DoF d at its lower bound, bit 32 + d: at its upper bound); word 1:
                                                constraint rows in findConstraints' order (bit i: row i at Clb, bit 32 + i: at Cub).
                                                Any bit pattern is accepted: a seed is used only if the equalities-only minimiser
                                                violates it or comes close to it, and wrong seeds are dropped again (restoration
                                                + refresh, csrc/wbc_common.h qp_core); NULL or zeros => cold start */
} WbcTickIn;

#define WBC_Q_STRIDE 27   /* doubles per instance in q / q_next (nq of the largest model)           */
#define WBC_V_STRIDE 26   /* doubles per instance in qdot, g, lb, ub; row length of H, C, A         */

/* the QP data of one tick, as the reference hands it to QP(...) (all optional outputs, [B][...]) */
typedef struct WbcQpData {
  double* A;    /* [B][m][26]  qpA()  (m = wbc_task_rows())          */
  double* b;    /* [B][m]      qpb()                                  */
  double* H;    /* [B][26][26] A'A   (QP_Wrapper.py:17)               */
  double* g;    /* [B][26]     -A'b  (QP_Wrapper.py:18)               */
  double* C;    /* [B][p][26]  findConstraints() before its final .T  */
  double* Clb;  /* [B][p]                                             */
  double* Cub;  /* [B][p]                                             */
  double* lb;   /* [B][26]     velDamperJointConstraints()            */
  double* ub;   /* [B][26]                                            */
} WbcQpData;

typedef struct WbcTickOut {
  double* qdot;     /* [B][26] xOpt; all zeros for an instance whose status is not WBC_QP_OPTIMAL (the reference's xOpt on
                       its first QP: qpOASES does not write the vector of an unsolved problem, QP_Wrapper.py:50-51) */
  int32_t* status;  /* [B] WBC_QP_*                                                       */
  int32_t* iters;   /* [B] working-set changes (may be NULL)                              */
  double* q_next;   /* [B][27] pin.integrate(q, qdot*dt) (may be NULL)                    */
  uint64_t* working_set; /* [B][2] the inequality constraints active at the solution, format of WbcTickIn.working_set (may be
                            NULL; may alias the input); zeros for an instance whose QP was not solved */
} WbcTickOut;

/* forward-kinematics outputs of updateState (all optional). In a handle with several models the per-instance strides of
 * oMi / oMf are the LARGEST model's njoints / nframes; an instance of a smaller model fills its own rows and zeroes the rest. */
typedef struct WbcFkOut {
  double* oMi;     /* [B][max njoints][12]  R (9, row-major) then p (3); joint 0 = identity   */
  double* oMf;     /* [B][max nframes][12]  controller frames (WbcModelBlob.frame_*)          */
  double* J;       /* [B][6][26] data.J of computeJointJacobians (WORLD)                      */
  double* com;     /* [B][3]     data.com[0]                                                  */
  double* Jcom;    /* [B][3][26] jacobianCenterOfMass                                         */
} WbcFkOut;

typedef struct WbcModel WbcModel;
typedef struct WbcBatch WbcBatch;

/* ------------------------------------------------------------------ entry points */

/* replaces pin.buildModelFromUrdf + createData (Robot_Wrapper4.py:21-23); validates the blob: sizes, a free-flyer root,
 * axis-aligned 1-DoF joints, joint placements that are the identity or a proper rotation, unrotated frame offsets
 * (WBC_E_UNSUPPORTED otherwise, with "rotated joint placement" / "rotated frame offset" in wbc_last_error()). */
int wbc_model_create(const WbcModelBlob* blob, WbcModel** out);
void wbc_model_destroy(WbcModel* m);

/* one handle per device/stream: device workspace for up to max_batch instances.
 * n_models == 0 gives a QP-only handle (wbc_qp_solve / wbc_qp_solve_ls), as QP_Wrapper.QP needs no robot model. */
int wbc_batch_create(const WbcModel* const* models, int n_models, int max_batch, int device_id, WbcBatch** out);
void wbc_batch_destroy(WbcBatch* b);

/* replaces setTasks / setConstraints / staticReachMode and the weight attributes
 * (Robot_Wrapper4.py:176-193, 1415-1464); cfg applies to model `model_index` of the batch.
 * Ordering: the call waits for the device (every stream, the caller's non-blocking ones included) before it overwrites the model's
 * configuration and plan, and returns when they are in place. A device-mode call enqueued BEFORE it therefore runs to its end under the old
 * configuration, every call made AFTER it sees the new one; no call ever sees a mixture. It is not for the hot loop and cannot be captured.
 * State of a handle ("one handle per device/stream"): a handle keeps, between calls, its options, the per-model configurations and plans,
 * and device workspaces that it allocates on first use and that every later call of the handle writes (the host-staging workspace, the
 * status / deferred-list / statistic words of the tick kernels, the wave order, the posture targets, the roll-out, score and watch state).
 * None of it carries a result from one call into the next: a call returns what it returns on a handle created, configured, given the same
 * options and called once (the wave order and a warm start change which wave runs an instance and how many working-set changes it takes,
 * never the answer's definition). Because the workspaces are shared by the handle's calls, calls on ONE handle must be enqueued on one
 * stream, or be ordered by the caller; independent handles may run on different streams concurrently. */
int wbc_batch_configure(WbcBatch* b, int model_index, const WbcConfig* cfg);
int wbc_task_rows(const WbcBatch* b);       /* m of qpA() under the current switches        */
int wbc_constraint_rows(const WbcBatch* b); /* p of findConstraints()                        */

/* replaces the pinocchio calls of updateState (Robot_Wrapper4.py:400-405) and
 * pin.jacobianCenterOfMass (Robot_Wrapper4.py:670). */
int wbc_fk_jacobians(WbcBatch* b, int B, const double* q, const int32_t* model_id, int mem,
                     const WbcFkOut* out, void* stream);

/* The time step. Every entry point below that takes `dt` (wbc_assemble, wbc_tick, wbc_rollout and their _tp / _traj / _tracks / _watch forms,
 * wbc_tick_vjp, wbc_tick_vjp_state) requires dt > 0 with dt and 1 / dt both finite: the kernels form x * (1 / dt) and qdot * dt, so NaN, 0,
 * a negative step, +inf (1 / dt = 0, qdot * dt = 0 * inf) and a subnormal step (1 / dt = inf) are refused with WBC_E_ARG before any launch.
 * wbc_integrate requires dt and 1 / dt finite only: dt < 0 there is a step back. Nothing else about dt is assumed (no nominal 2 ms). */

/* replaces qpA/qpb/findConstraints/velDamperJointConstraints + QP.__init__'s H, g
 * (Robot_Wrapper4.py:1348-1361, QP_Wrapper.py:17-18). */
int wbc_assemble(WbcBatch* b, int B, const WbcTickIn* in, double dt, int mem, const WbcQpData* out, void* stream);

/* replaces QP.solveQP / solveQPHotstart given H, g (QP_Wrapper.py:23-73):
 * argmin 1/2 x'Hx + g'x  s.t. lb <= x <= ub, Clb <= C x <= Cub.
 * n <= 26, p <= WBC_MAX_P; H is [B][n][n], C is [B][p][n] (row-major, NOT the reference's C.T view —
 * SURVEY.md C.1); lb/ub/C may be NULL (no box / no rows).
 * Hot start (solveQPHotstart, QP_Wrapper.py:55-73: qpOASES keeps its working set between calls): working_set_in / working_set_out,
 * [B][2] words in the QP's own indexing — word 0: bit i = variable i at its lower bound, bit 32 + i = at its upper bound; word 1: the
 * same for constraint row i. Either may be NULL (cold start / nothing returned); they may be the same buffer. A seed is only a hint:
 * the answer is the cold solve's (H > 0), wrong seeds are dropped again. An unsolved QP returns an empty set.
 * Kernel: several problems per wavefront (csrc/wbc_k_qpp.hip: four when n <= 16 and p <= 16, else two; statistic "last_qp_path" = 4 / 2),
 * cold and hot start alike; option "packed_kernel" 0 keeps one problem per wavefront (csrc/wbc_k_misc.hip, "last_qp_path" = 1). Same status,
 * iteration count and working set from both; answers equal to rounding. */
int wbc_qp_solve(WbcBatch* b, int B, int n, int p, const double* H, const double* g, const double* C,
                 const double* lb, const double* ub, const double* Clb, const double* Cub, int mem,
                 double* x, int32_t* status, int32_t* iters, const uint64_t* working_set_in, uint64_t* working_set_out,
                 void* stream);

/* replaces QP(A, b, ...) + solveQP(): forms H = A'A, g = -A'b on the device (QP_Wrapper.py:17-18)
 * and solves. A is [B][m][n], m <= WBC_MAX_M. H_out/g_out optional. The packed kernel (see wbc_qp_solve) forms A'A on the fp64 matrix cores
 * always; use_mfma chooses inside the one-per-wavefront kernel only: 1 = fp64 MFMA contraction, 0 = VALU, -1 = MFMA from WBC_MFMA_AUTO_ROWS rows on.
 * With option "refine" (default 1) the answer gets one step of iterative refinement from A, b themselves where the problem's pivot ratio asks
 * for it (csrc/wbc_common.h WBC_REFINE_COND; QP_Wrapper.py:37 numRefinementSteps); wbc_qp_solve (H, g alone) is never refined.
 * working_set_in / working_set_out: as in wbc_qp_solve (QP.solveQPHotstart passes the previous call's set). */
int wbc_qp_solve_ls(WbcBatch* b, int B, int m, int n, int p, const double* A, const double* bvec, const double* C,
                    const double* lb, const double* ub, const double* Clb, const double* Cub, int mem, int use_mfma,
                    double* x, int32_t* status, int32_t* iters, double* H_out, double* g_out,
                    const uint64_t* working_set_in, uint64_t* working_set_out, void* stream);

/* ------------------------------------------------------------------ dual solution, KKT certificate and sensitivities of a solved QP
 * What qpOASES users read with getDualSolution() / getObjVal(), a certificate of optimality computed from the caller's own data, and the
 * vector-Jacobian product of the solution — one kernel of its own behind the solve (csrc/wbc_k_cert.hip; no solve kernel takes part).
 * The problem is wbc_qp_solve's:  min 1/2 x'Hx + g'x  s.t. lb <= x <= ub, Clb <= C x <= Cub,  n <= 26, p <= WBC_MAX_P, C row-major [p][n];
 * or it is given as (A, b) with m <= WBC_MAX_M rows, H = A'A and g = -A'b. A bound with |value| >= 1e20 is infinite.
 * Active normals N (k rows), in this order: variables by index, then rows of C by index.
 *   - a variable with lb == ub, or a row with Clb == Cub, is always active, as an equality;
 *   - with a working set (format of wbc_qp_solve: word 0 bit i / 32 + i = variable i at its lower / upper bound, word 1 the same for
 *     the rows): the marked sides; a bit on an equality, on an infinite side, or on both sides at once, is ignored;
 *   - without one the set is read off x, with v = (x; C x) entry by entry: at the lower side if |v - lo| < 1e-7 max(1, |lo|), else at
 *     the upper side by the same test.
 * Duals, in qpOASES' sign convention: grad f(x) = N'y, that is H x + g = y_bounds + C'y_rows; y >= 0 at an active lower side, y <= 0 at
 *   an active upper side, either sign on an equality, exactly 0 on an inactive entry.
 * grad f: from (H, g) it is H x + g; from (A, b) it is A'(A x - b) as two products from the unfactored data, never through fl(A'A)
 *   (the reason option "refine" gives). The objective is 1/2 x'Hx + g'x, in the (A, b) form 1/2 |A x|^2 - b'(A x) (the constant
 *   1/2 |b|^2 is left out, as in H, g).
 * Sensitivity, for a caller-given v = dL/dx: with K = [H N'; N 0] solve K (u; w) = (v; 0). Then, e_i being the bound value active
 *   constraint i sits at:  dL/dg = -u,  dL/de_i = w_i,  dL/dH = -1/2 (u x' + x u'),  dL/dC_j = -w_j x' + y_j u'
 *   (the host side builds these from the outputs; the gradient of an equality's value belongs to both of its sides).
 * Method: Cholesky H = L L', Y = L^-1 N' (n x k), Householder QR Y = Q1 R, y = R^-1 Q1' L^-1 grad f, and with z = L^-1 v:
 *   w = R^-1 Q1' z, u = L^-T (z - Q1 Q1' z). The Schur complement Y'Y is never formed.
 * cert_status per instance: */
enum { WBC_CERT_OK = 0         /* the numbers were computed; judging them is the caller's job (no thresholds live in the library)    */,
       WBC_CERT_UNSOLVED = 1   /* the input status[b] != 0: everything is zero                                                       */,
       WBC_CERT_DEPENDENT = 2  /* the active normals are dependent: k > n, or a diagonal entry of R with |R_jj| <= 1e-12 x the
                                  Euclidean norm of column j of Y. kkt[1], objective and n_active are still given; duals, sensitivities
                                  and kkt[0], [2], [3] are zero                                                                      */,
       WBC_CERT_NUMERICAL = 3  /* a non-finite input (NaN or +-inf in H, g, A, b, C, x, v; NaN in a bound) or a Cholesky pivot that
                                  is not positive: everything is zero. Nothing non-finite reaches another instance's outputs         */ };
typedef struct WbcQpProblem {
  int32_t n, p, m, pad_;           /* m = 0 with H, g; 1..WBC_MAX_M with A, b                                          */
  const double* H;                 /* [B][n][n]   \  exactly one pair                                                   */
  const double* g;                 /* [B][n]      /                                                                     */
  const double* A;                 /* [B][m][n]   \                                                                     */
  const double* b;                 /* [B][m]      /                                                                     */
  const double* C;                 /* [B][p][n]; C, Clb, Cub required when p > 0                                        */
  const double* lb;                /* [B][n]; lb and ub go together, NULL => no box                                     */
  const double* ub;
  const double* Clb;               /* [B][p]                                                                            */
  const double* Cub;
  const double* x;                 /* [B][n] the answer to certify (required)                                           */
  const int32_t* status;           /* [B] the solve's status; NULL => every instance counts as solved                   */
  const uint64_t* working_set;     /* [B][2] the solve's working_set_out; NULL => the active set is read off x          */
  const double* v;                 /* [B][n] dL/dx; NULL => no sensitivities                                            */
} WbcQpProblem;
typedef struct WbcQpCert {         /* all optional; an output left NULL is not written                                  */
  double* y_bounds;                /* [B][n]                                                                            */
  double* y_rows;                  /* [B][p]                                                                            */
  double* kkt;                     /* [B][4]: [0] |grad f - N'y|_inf; [1] the largest violation of any bound or row, >= 0; [2] the largest
                                      wrong-signed multiplier magnitude over the inequality actives; [3] max |y_i (v_i - e_i)| over actives */
  double* objective;               /* [B] getObjVal                                                                     */
  int32_t* n_active;               /* [B] k                                                                             */
  double* sens_x;                  /* [B][n] u                                                                          */
  double* sens_bounds;             /* [B][n] w scattered to the variables' own indices, 0 where inactive                */
  double* sens_rows;               /* [B][p] w of the rows likewise                                                     */
  int32_t* cert_status;            /* [B] WBC_CERT_*                                                                    */
} WbcQpCert;
/* Works on a QP-only handle. With device pointers the call enqueues exactly one kernel: no allocation, no memset, so it can be captured.
 * WBC_E_ARG, naming the field: both pairs (H, g and A, b) given, or neither, or half of one; x NULL; n, p or m out of range; C, Clb or
 * Cub missing with p > 0; lb without ub; sens_x, sens_bounds or sens_rows requested without v. */
int wbc_qp_certificate(WbcBatch* b, int B, const WbcQpProblem* problem, const WbcQpCert* out, int mem, void* stream);
int wbc_qp_certificate_sizes(int32_t* sizeof_problem, int32_t* sizeof_cert); /* ctypes layout self-check */

/* ------------------------------------------------------------------ the tick as a layer: dL/d(task weights, gains, targets)
 * For a solved tick x = qdot and the certificate's u = sens_x of a caller's v = dL/dqdot (wbc_qp_certificate on the tick's own A, b, C, bounds):
 * the gradient of L with respect to what the tick's CALLER owns — the 85 weights and gains (WbcTaskParams) and the task targets. With
 * r = b - A x and s = A u:  dL/dA = r u' - s x',  dL/db = s;  every task row is (weights) x (an unweighted Jacobian row), so each entry is a
 * few 26-term products of unweighted rows with x and u. The kernel (csrc/wbc_k_grad.hip, four instances per wavefront) recomputes the
 * kinematics from q — task rows see q, never q_con — and reads neither A nor H. Per block, with jx = J_r x, ju = J_r u:
 *   EE e, row r (A = W_r w J_r, b = w vel_r):  s = W_r w ju, rho = w vel_r - W_r w jx;  dW_r = w (rho ju - s jx);
 *     dw += W_r (rho ju - s jx) + s vel_r;  dvel_r = w s;  r < 3: dgain_r = dvel_r (xt - x_fk) / dt, d ee_target = dvel_r (1 + gain_r) / dt,
 *     d prev_ee_target = -dvel_r / dt;  ee_gain[e][3..5] never reach b: exactly 0.
 *   trunk: the same on the WORLD Jacobian; trunk_gain[3..5] multiply the reference's literal quaternion-error components (Robot_Wrapper4.py:974-976).
 *   CoM (A = com_W_r Jcom_r, b = cv_r + com_gain_r (ct_r - com_r)): com_W, com_gain, com_target, com_target_vel.
 *   posture (d = joint_w / nv, b_k = d up_k): d joint_w = (2 / nv) sum_k d (up_k - x_k) u_k,  d posture_u_k = d^2 u_k.
 * Entries of a switched-off task are exactly 0. An instance with status != 0, cert_status != WBC_CERT_OK or a non-finite input gets all-zero
 * rows; nothing non-finite reaches another instance's rows. grad_status per instance: */
enum { WBC_GRAD_OK = 0, WBC_GRAD_UNSOLVED = 1 /* status[b] != 0 */, WBC_GRAD_CERT = 2 /* cert_status[b] != WBC_CERT_OK */,
       WBC_GRAD_NONFINITE = 3 /* NaN or +-inf in q, qdot, sens_x, the weights and gains or a target the configuration reads */ };
typedef struct WbcTickGrad {         /* all optional; an output left NULL is not written                                  */
  double* d_task_params;             /* [B][85], WbcTaskParams layout                                                     */
  double* d_ee_target;               /* [B][5][3]; rows of end effectors without a task are 0                             */
  double* d_prev_ee_target;          /* [B][5][3]                                                                         */
  double* d_trunk_target;            /* [B][3]                                                                            */
  double* d_prev_trunk_target;       /* [B][3]                                                                            */
  double* d_com_target;              /* [B][3]                                                                            */
  double* d_com_target_vel;          /* [B][3]                                                                            */
  double* d_posture_u;               /* [B][26]; posture modes MANI / HYBRID / CUSTOM (the others never read posture_u)   */
  int32_t* grad_status;              /* [B] WBC_GRAD_*                                                                    */
} WbcTickGrad;
/* in: the fields the task rows read (q, ee_target, prev_ee_target, trunk_target, prev_trunk_target, trunk_ref_euler, trunk_prev_rot,
 * ee_ref_rot, ee_prev_rot, com_target, com_target_vel, posture_u, model_id); tp: per-instance rows or NULL (the configuration's block);
 * qdot, sens_x [B][26]; status, cert_status [B] (NULL: every instance counts as solved / certified). Host or device buffers. With device
 * pointers, and posture_u given or the posture mode not MANI / HYBRID, the call enqueues exactly one kernel: no allocation, no memset.
 * MANI / HYBRID with posture_u NULL: the posture target is computed first, as wbc_assemble does. Needs every model of the handle to fit the
 * packed whole-tree schedule (as wbc_state_slack: WBC_E_UNSUPPORTED otherwise). WBC_E_ARG, naming the field: qdot or sens_x NULL; an output
 * requested whose inputs the configuration does not read (d_ee_target without an EE task, d_trunk_target without the trunk task,
 * d_com_target without the CoM task, d_posture_u outside MANI / HYBRID / CUSTOM).
 * Gradients with respect to q and trunk_box_center come from wbc_tick_vjp_state below (it contracts what kinematic Hessians would hold with
 * x and u and never forms them). Not offered: ee_ref_rot / ee_prev_rot, trunk_ref_euler / trunk_prev_rot. Gradients through roll-outs are offered as
 * chained layers (this call, wbc_tick_vjp_state and wbc_step_vjp below, composed per tick: wbc_torch.wbc_rollout) and as a fused reverse sweep
 * over a recorded roll-out (wbc_rollout_record / wbc_rollout_vjp below).
 * Statistic "last_grad_variant": the row of csrc/wbc_k_grad.hip's table the last call launched (key of ROT), -1 before the first. */
int wbc_tick_vjp(WbcBatch* b, int B, const WbcTickIn* in, const WbcTaskParams* tp, double dt, const double* qdot, const double* sens_x,
                 const int32_t* status, const int32_t* cert_status, int mem, const WbcTickGrad* out, void* stream);
int wbc_tick_grad_sizes(int32_t* sizeof_grad); /* ctypes layout self-check */

/* ------------------------------------------------------------------ the tick as a layer, state side: dL/dq and dL/d trunk_box_center
 * For a solved tick x = qdot and its certificate for the caller's v = dL/dqdot — u = sens_x, w = sens_bounds / sens_rows, y = y_rows
 * (wbc_qp_certificate on the tick's own A, b, C, bounds) — the gradient of L with respect to the STATE the tick was solved at. With r = b - A x
 * and s = A u:
 *   dL/d delta_k = sum_rows (r_i u - s_i x) . dA_i/d delta_k + s_i db_i/d delta_k + sum_j (y_j u - w_j x) . dC_j/d delta_k + sum_active w_i de_i/d delta_k
 * Tangent convention: d_q[b][k] = dL/d delta_k at delta = 0 for q(delta) = pin.integrate(q, delta) = wbc_integrate(q, delta, dt = 1); the base
 * DoF are in the base-local frame; columns >= the model's nv are 0. (wbc_workload.tangent_to_raw turns it into a gradient in raw coordinates.)
 * Every Jacobian row appears only contracted with x or u, and d(J_W z)/d delta_k = S_k x_m T_k(z) with S_k the WORLD column of DoF k and T_k(z)
 * the frame body's spatial velocity under z minus that of k's own body: the kernel (csrc/wbc_k_gradq.hip, four instances per wavefront)
 * recomputes the kinematics from q, keeps one table of body velocities under x and u, and forms no second-order tensor.
 * Differentiated: every task and constraint row, the position, quaternion and CoM feedback in b, the PREV posture target, the CoM and trunk
 * boxes (the Euler angles are the three atan2 forms stated under wbc_state_slack), the velocity-damper bounds branch by branch (0 on a
 * clipped or constant branch; at a kink the branch the tick's own comparisons select).
 * HELD CONSTANT: posture_u in MANI / HYBRID / CUSTOM (its own dependence on q is not differentiated; wbc_tick_vjp gives d_posture_u), and
 * the orientation references (ee_ref_rot, ee_prev_rot, trunk_ref_euler, trunk_prev_rot).
 * Which side a w belongs to: wbc_qp_certificate's rule. With working_set the marked side; without, the lower side if
 * |value - lo| < 1e-7 max(1, |lo|), else the upper side; half and half where lo == hi. The kernel recomputes the bounds from q.
 * d_trunk_box_center: z row scale (1 -+ z_frac) / dt, angle rows scale / dt, each times the active side's w. */
typedef struct WbcTickSens {          /* a solved tick and its certificate for the caller's v = dL/dqdot */
  const double* qdot;                 /* [B][26] required */
  const double* sens_x;               /* [B][26] required: u */
  const double* sens_bounds;          /* [B][26] w of the velocity bounds; NULL => zeros (required with use_bounds) */
  const double* sens_rows;            /* [B][p]  w of the rows;  required when p > 0 */
  const double* y_rows;               /* [B][p]  duals of the rows; required when p > 0 */
  const int32_t* status;              /* [B] NULL => all solved */
  const int32_t* cert_status;         /* [B] NULL => all certified */
  const uint64_t* working_set;        /* [B][2] the tick's working_set out; NULL => sides read off qdot */
} WbcTickSens;
typedef struct WbcTickStateGrad {     /* all optional */
  double* d_q;                        /* [B][26] tangent coordinates, see above */
  double* d_trunk_box_center;         /* [B][4]  needs the trunk constraint */
  int32_t* grad_status;               /* [B] WBC_GRAD_* (the codes of wbc_tick_vjp) */
} WbcTickStateGrad;
/* in: every field the tick reads; tp: per-instance rows or NULL. Host or device buffers. With device pointers the call enqueues exactly one
 * kernel: no allocation, no memset, so it can be captured. An instance with status != 0, cert_status != WBC_CERT_OK or a non-finite value in
 * q, qdot, the four sensitivity arrays, the weights and gains, trunk_box_center or a target the configuration reads gets all-zero rows and its
 * grad_status; nothing non-finite reaches another instance's rows; rows >= B are never written. WBC_E_UNSUPPORTED when a model does not fit
 * the packed whole-tree schedule (as wbc_state_slack). WBC_E_ARG, naming the field: q_con not NULL (the constraints would see another
 * configuration); posture mode MANI / HYBRID with posture_u NULL; qdot or sens_x NULL; sens_bounds NULL with use_bounds; sens_rows or y_rows
 * NULL with p > 0; d_trunk_box_center without the trunk constraint; trunk_box_center NULL with the trunk constraint.
 * Statistic "last_gradq_variant": the row of csrc/wbc_k_gradq.hip's table the last call launched (key of ROT), -1 before the first;
 * wbc_variant_count("gradq") == 2. */
int wbc_tick_vjp_state(WbcBatch* b, int B, const WbcTickIn* in, const WbcTaskParams* tp, double dt, const WbcTickSens* sens, int mem,
                       const WbcTickStateGrad* out, void* stream);
int wbc_tick_state_grad_sizes(int32_t* sizeof_sens, int32_t* sizeof_grad); /* ctypes layout self-check */

/* replaces qpJointb's "MANI" / "HYBRID" branches (Robot_Wrapper4.py:1220-1260) under the configured task_joint,
 * arm_base_id and posture_literal: u [B][26] = the posture target before scaling (PREV / zeros for the other modes),
 * q_after [B][27] = the configuration the reference's state holds afterwards (optional). wbc_tick / wbc_assemble call
 * this themselves when task_joint is MANI or HYBRID and WbcTickIn.posture_u is NULL. */
int wbc_posture_target(WbcBatch* b, int B, const double* q, const int32_t* model_id, int mem, double* u, double* q_after,
                       void* stream);

/* the fused hot path = one runWBC tick up to and including the QP (+ optional integrate):
 * FK -> Jacobians -> task stack -> H, g, C, bounds -> QP -> qdot [-> q_next]. */
int wbc_tick(WbcBatch* b, int B, const WbcTickIn* in, double dt, int mem, const WbcTickOut* out, void* stream);

/* replaces jointVelocitiestoConfig / pin.integrate (Robot_Wrapper4.py:440-441): q_next = q (+) v*dt */
int wbc_integrate(WbcBatch* b, int B, const double* q, const double* v, const int32_t* model_id, double dt, int mem,
                  double* q_next, void* stream);

/* replaces the tail of runWBC, updateState(joint_config, base_config, running=True) (Robot_Wrapper4.py:1397-1399, 387-428)
 * with the foot-anchored base estimator trunkWorldPos (:1297-1327):
 *   q_new = [base xyz re-estimated from the stance-foot targets, imu quaternion, joints of q_next].
 * q_cur: current_joint_config (its base xyz is read); q_next: wbc_tick's q_next; imu [B][4] (x, y, z, w) = base_config,
 * NULL => the quaternion of q_next; foot_targets [B][5][3] = the tick's ee_target (FR, FL, RR, RL are read).
 * q_new may alias q_cur. */
int wbc_update_state(WbcBatch* b, int B, const double* q_cur, const double* q_next, const double* imu,
                     const double* foot_targets, const int32_t* model_id, int mem, double* q_new, void* stream);

/* ------------------------------------------------------------------ the state step as a layer: dL/d(q, qdot, foot targets)
 * The link between tick k and tick k + 1:  q_next = wbc_integrate(q, qdot, dt),  q_new = wbc_update_state(q, q_next, imu, foot_targets)
 * (mode WBC_ROLLOUT_WARMUP: q_new = q_next). For g = dL/d delta_new [B][26], the gradient of a loss in the tangent coordinates at q_new, one
 * kernel launch (csrc/wbc_k_stepvjp.hip, four instances per wavefront) gives the gradient with respect to q (d_q, tangent
 * coordinates at q), qdot and foot_targets. Tangent convention of wbc_tick_vjp_state: q (+) delta = wbc_integrate with dt = 1, base DoF in the
 * base-local frame, linear before angular; columns >= the model's nv are 0.
 * Update part (RUNNING). R_b: the rotation of the quaternion q_new carries (the IMU's if given, else q_next's); p_e (e = 0..3), p_t: the world
 * positions of the foot frames and the trunk frame at [q xyz, that quaternion, the joints of q_next]; BPA = mean_e (p_e - p_t); rbar = R_b' BPA;
 * Jbar = mean_e of the LOCAL_WORLD_ALIGNED linear rows of foot frame e. With g_p = g[0:3], g_phi = g[3:6], g_theta = g[6:]:
 *   d_foot_targets[e] = R_b g_p / 4  (e = 0..3; row 4 = 0)
 *   c_theta = g_theta - Jbar[:, 6:]' g_p
 *   c_phi   = g_phi - BPA x g_p - rbar x (R_b' g_p)
 *   c_p     = 0   (q's xyz cancels in the estimator; q_next's is not read)
 * In WARMUP c = g and d_foot_targets = 0.
 * Integrate part. xi = dt qdot[0:6], (Re, pe) = exp6(xi), c6 = (c_p, c_phi):
 *   d_q[0:6]    = Ad' c6,  Ad = [[Re', -Re' [pe]x], [0, Re']]  (the adjoint of the inverse of exp6(xi))
 *   d_qdot[0:6] = dt Jr(xi)' c6,  Jr the right Jacobian of SE(3) = sum_k (-ad_xi)^k / (k + 1)!
 *   d_q[6:]     = c_theta,   d_qdot[6:] = dt c_theta
 * HELD CONSTANT: the IMU quaternion (no d_imu is offered; with an IMU c_phi = 0).
 * EXACT ZEROS: d_q[0:3] and d_qdot[0:3] in RUNNING; d_q[3:6] and d_qdot[3:6] with an IMU; row 4 of d_foot_targets; columns >= nv.
 * The quaternion's sign continuity and first-order renormalisation do not appear in tangent coordinates. */
typedef struct WbcStepGrad {          /* all optional */
  double* d_q;                        /* [B][26] tangent coordinates at q_cur */
  double* d_qdot;                     /* [B][26] */
  double* d_foot_targets;             /* [B][5][3] */
  int32_t* grad_status;               /* [B] WBC_GRAD_OK or WBC_GRAD_NONFINITE */
} WbcStepGrad;
/* q_cur [B][27], qdot [B][26], foot_targets [B][5][3], g_q_new [B][26] required; imu [B][4] or NULL; mode WBC_ROLLOUT_*. Host or device
 * buffers. With device pointers the call enqueues exactly one kernel: no allocation, no memset, so it can be captured. An instance with a
 * non-finite value among its model's own entries of q_cur, qdot or g_q_new, in the foot targets read (rows 0..3, RUNNING) or in its IMU row
 * gets all-zero rows and WBC_GRAD_NONFINITE; nothing non-finite reaches another instance's rows; rows >= B are never written. dt: the rule of
 * a forward step (dt > 0, dt and 1 / dt finite). WBC_E_ARG, naming the field: q_cur, qdot, foot_targets, g_q_new or out NULL; a mode other
 * than WBC_ROLLOUT_RUNNING / WBC_ROLLOUT_WARMUP; model_id NULL with several models. WBC_E_UNSUPPORTED when a model does not fit the packed
 * whole-tree schedule (as wbc_state_slack).
 * Statistic "last_stepvjp_variant": the row of csrc/wbc_k_stepvjp.hip's table the last call launched (key of ROT), -1 before the first;
 * wbc_variant_count("stepvjp") == 2. */
int wbc_step_vjp(WbcBatch* b, int B, const double* q_cur, const double* qdot, const double* foot_targets, const double* imu,
                 const int32_t* model_id, double dt, int mode, const double* g_q_new, int mem, const WbcStepGrad* out, void* stream);
int wbc_step_grad_sizes(int32_t* sizeof_grad); /* ctypes layout self-check */

/* K closed-loop ticks without leaving the device (the 2000 QPs of setInitialState for B robots in one
 * call with mode = WBC_ROLLOUT_WARMUP, ticks = hold_ticks = 1000): per tick wbc_tick -> wbc_update_state -> the
 * reference-state side effects of qpb() (prev_EE_pos / prev_EE_CoM_rot, calcTargetVelEE3 :1151-1152; prev_trunk_ref /
 * old_ref_trunk_rot_matrix, calcTargetVelTrunk2 :995-996) -> the targets advance by a per-tick step (one linear segment
 * of sim3.py's milestone trajectory, sim3.py:207-228). `in0` is the state and the targets of the first tick (never
 * written); all outputs optional. */
enum { WBC_ROLLOUT_RUNNING = 0  /* updateState(joint_config, base_config, running=True): IMU quaternion fed back, base xyz
                                   re-estimated from the stance-foot targets (trunkWorldPos)                            */,
       WBC_ROLLOUT_WARMUP = 1   /* updateState(new_config, feedback=False, running=False) as inside setInitialState's loop
                                   (Robot_Wrapper4.py:287-326, 440-447 with initialised == False): the integrated
                                   configuration becomes the state as it is — free-floating base, no IMU, no estimator   */ };
typedef struct WbcRollout {
  int32_t ticks;                    /* K >= 1 ticks during which the targets advance by their steps        */
  int32_t mode;                     /* WBC_ROLLOUT_*                                                        */
  const double* ee_target_step;     /* [B][5][3] added to ee_target after every tick; NULL => constant     */
  const double* trunk_target_step;  /* [B][3]; NULL => constant                                            */
  const double* imu;                /* [B][4] base quaternion fed back every tick; NULL => the integrated one */
  double* q_final;                  /* [B][27] current_joint_config after K ticks                          */
  double* qdot_last;                /* [B][26] xOpt of the last tick                                       */
  double* ee_target_final;          /* [B][5][3] targets the NEXT tick would get                           */
  double* grip_trace;               /* [K][B][3] gripper_bar position reached after every tick (sim3.py:340-348's log) */
  int32_t* status_max;              /* [B] worst WBC_QP_* status over the K ticks                          */
  int32_t* iters_sum;               /* [B] working-set changes over the K ticks                            */
  int32_t hold_ticks;               /* further ticks with the targets held where the K ticks left them (the second, clamped
                                       segment of setInitialState's trajectories, Robot_Wrapper4.py:275); grip_trace then holds
                                       ticks + hold_ticks entries                                           */
  int32_t pad_;
} WbcRollout;
int wbc_rollout(WbcBatch* b, int B, const WbcTickIn* in0, double dt, const WbcRollout* r, int mem, void* stream);

/* per-instance task weights and gains (WbcTaskParams, tp [B]); tp == NULL is exactly the call without the suffix.
 * wbc_tick_tp: every kernel of wbc_tick takes the rows (the one-instance compact sim3 kernel of option refine = 0 excepted: such a call
 * runs on the general kernel, statistic "last_path" 0). wbc_rollout_tp: the same rows on every tick, RUNNING and WARMUP alike. */
int wbc_tick_tp(WbcBatch* b, int B, const WbcTickIn* in, const WbcTaskParams* tp, double dt, int mem, const WbcTickOut* out, void* stream);
int wbc_assemble_tp(WbcBatch* b, int B, const WbcTickIn* in, const WbcTaskParams* tp, double dt, int mem, const WbcQpData* out, void* stream);
int wbc_rollout_tp(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r, int mem, void* stream);

/* ------------------------------------------------------------------ roll-out gradients in two calls: recorded forward, device reverse sweep
 * wbc_rollout_record is wbc_rollout_tp that also writes a TAPE; wbc_rollout_vjp sweeps the tape from the last tick to the first and gives
 * dL/d(q_0, weights and gains, targets, target steps) of a loss seeded at q_K, at the last tick's qdot and / or at the state after every tick
 * (DESIGN.md §3.42). The sweep composes, per tick and unchanged, the kernels of wbc_step_vjp, wbc_assemble_tp, wbc_qp_certificate (the
 * (A, b) form), wbc_tick_vjp and wbc_tick_vjp_state above, plus one link kernel of its own (csrc/wbc_k_rollvjp.hip, four instances per
 * wavefront) for the algebra between them. It is the reverse of the forward users run, not of a restatement of it.
 * THE TAPE is device memory the caller owns (several may coexist; the handle keeps no pointer to one): wbc_rollout_tape_bytes(B, ticks) =
 * 432 B + 736 B ticks bytes. Per instance and tick, 736 bytes: q_k [27], qdot_k [26], ee_target, prev_ee_target [5][3] each, trunk_target,
 * prev_trunk_target [3] each as the tick SAW them (the running sums: never k * step), all doubles (89); the tick's status (int32, + one int32
 * of padding); the tick's working set (2 x uint64: written under option "warm_start" alone — a cold tick returns none). Per instance, once, 432
 * bytes: ee_prev_rot [5][9] and trunk_prev_rot [9] as every tick after the first saw them (tick 0 saw in0's). Blocks are strided by B.
 * wbc_rollout_record: the arguments of wbc_rollout_tp, the tape, and q_trace [ticks][B][27] (optional, host or device as `mem` says): the
 * state after every tick; q_trace[ticks - 1] is q_final. Every output is bit-identical to wbc_rollout_tp's on the same inputs and handle
 * state: the ticks are launched exactly as wbc_rollout_tp launches them. WBC_E_ARG, naming the field, before any launch: hold_ticks > 0; q_con;
 * posture mode MANI / HYBRID with posture_u NULL (wbc_tick_vjp_state's rule: the posture target would change per tick); tape NULL or
 * tape_bytes too small. WBC_E_UNSUPPORTED: a model that does not fit the packed whole-tree schedule (as the layers). */
size_t wbc_rollout_tape_bytes(int B, int ticks);
int wbc_rollout_record(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r, void* tape,
                       size_t tape_bytes, double* q_trace, int mem, void* stream);
/* Seeds: cotangents in the tangent coordinates of wbc_tick_vjp_state (q (+) delta = wbc_integrate with dt = 1); at least one is required. */
typedef struct WbcRolloutSeed {
  const double* g_q_final;            /* [B][26] tangent at q_K                                                            */
  const double* g_qdot_last;          /* [B][26] dL/d(qdot of the last tick)                                               */
  const double* g_q_trace;            /* [ticks][B][26] tangent at the state after each tick (row ticks - 1 adds to g_q_final) */
} WbcRolloutSeed;
typedef struct WbcRolloutGrad {       /* all optional; an output left NULL is not written                                  */
  double* d_q0;                       /* [B][26] tangent at q_0                                                            */
  double* d_task_params;              /* [B][85] summed over the ticks, as the five below                                  */
  double* d_ee_target;                /* [B][5][3] with respect to in0's ee_target                                         */
  double* d_prev_ee_target;           /* [B][5][3] with respect to in0's prev_ee_target                                    */
  double* d_trunk_target;             /* [B][3]                                                                            */
  double* d_prev_trunk_target;        /* [B][3]                                                                            */
  double* d_com_target;               /* [B][3]                                                                            */
  double* d_com_target_vel;           /* [B][3]                                                                            */
  double* d_posture_u;                /* [B][26]                                                                           */
  double* d_trunk_box_center;         /* [B][4]                                                                            */
  double* d_ee_target_step;           /* [B][5][3] with respect to WbcRollout.ee_target_step                               */
  double* d_trunk_target_step;        /* [B][3]                                                                            */
  int32_t* grad_status;               /* [B] the worst WBC_GRAD_* of any layer over the ticks                              */
  int32_t* ticks_dropped;             /* [B] ticks whose tick layer gave zero for the instance                             */
} WbcRolloutGrad;
/* in0, tp, dt, r: what wbc_rollout_record was called with (r's outputs and steps are not read: the tape holds the targets; mode and imu are).
 * Per tick k = K - 1 .. 0, everything on `stream`, no host round trip and no synchronisation (device buffers):
 *   1. wbc_step_vjp's kernel at the taped (q_k, qdot_k, ee_target_k) with g = the carried cotangent of q_(k+1) (+ g_q_trace[k]; k = K - 1: g_q_final)
 *   2. v = the step's d_qdot (k = K - 1: + g_qdot_last)
 *   3. wbc_assemble_tp's kernel at the taped inputs (A, b, C, bounds; a model with nv < 26 gets unit rows on its padded columns behind A's task
 *      rows, written on the device), then wbc_qp_certificate's kernel with v, the taped status and, under option "warm_start", the taped
 *      working set (without: the active sides are read off qdot, wbc_qp_certificate's rule; the option must be what it was at the record)
 *   4. wbc_tick_vjp's and wbc_tick_vjp_state's kernels from the certificate's outputs
 *   5. the link kernel: g <- step.d_q + tickstate.d_q (both tangent at q_k: no raw coordinates anywhere in the sweep); the summed outputs +=
 *      this tick's; the adjoint of the target bookkeeping.
 * TARGET BOOKKEEPING. Forward, with s = ee_target_step: E_(k+1) = E_k + s, and P_(k+1) = E_k where the end effector's task is on, else P_k
 * (E: ee_target, P: prev_ee_target). With Ebar, Pbar the cotangents of E_(k+1), P_(k+1) (both 0 behind the last tick), a_k = tick.d_ee_target
 * + step.d_foot_targets and p_k = tick.d_prev_ee_target:
 *     d_ee_target_step += Ebar;   Ebar <- Ebar + a_k + on o Pbar;   Pbar <- p_k + (1 - on) o Pbar
 * and after tick 0 d_ee_target = Ebar, d_prev_ee_target = Pbar. The trunk pair follows the same rule under task_trunk (a_k = tick.d_trunk_target).
 * HELD CONSTANT, as in the layers: the orientation references, the IMU quaternion, posture_u's own dependence on q.
 * UNSOLVED TICKS: an instance whose tick k is unsolved, uncertified or non-finite gets zero from that tick's layer (wbc_tick_vjp's rule) and
 * ticks_dropped += 1; what flows through the step alone continues. An instance with WBC_GRAD_NONFINITE from any layer gets all-zero rows.
 * Nothing non-finite reaches another instance; rows >= B are never written. The workspaces live in the handle and grow on demand: once they
 * have their size a call allocates nothing, and with device buffers both calls can be captured into a HIP graph.
 * WBC_E_ARG, naming the field, before any launch: no seed; what wbc_rollout_record refuses; an output whose inputs the configuration does
 * not read (the rules of wbc_tick_vjp and wbc_tick_vjp_state; d_*_target_step as d_*_target). WBC_E_UNSUPPORTED as wbc_rollout_record.
 * Not offered: hold_ticks, the one-track trajectory call (roll-outs along tracks: wbc_rollout_record_tracks / wbc_rollout_vjp_tracks
 * below; the watch roll-outs: wbc_rollout_record_watch / wbc_rollout_vjp_watched further below), checkpoint-and-recompute (the tape holds
 * every tick).
 * Statistic "last_rollvjp_variant": the row of csrc/wbc_k_rollvjp.hip's table the last call launched last (key of the stage: 0 BEGIN, 1 ADDV,
 * 2 LINK), -1 before the first; wbc_variant_count("rollvjp") == 3. */
int wbc_rollout_vjp(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r, const void* tape,
                    size_t tape_bytes, const WbcRolloutSeed* seed, int mem, const WbcRolloutGrad* out, void* stream);
int wbc_rollout_grad_sizes(int32_t* sizeof_seed, int32_t* sizeof_grad); /* ctypes layout self-check */

/* ------------------------------------------------------------------ roll-outs along per-instance milestone trajectories, scored on device
 * The experiment of sim3.py as one call: the target of one end effector follows a piecewise-linear trajectory through the instance's own
 * milestones (sim3.py:207-228: klampt Trajectory(milestones=...), evaluated at a parameter that advances by 0.002 per tick, :225), and what
 * the reference logs of it — the gripper's target against the position reached, sim3.py:287-296, :340-348 — comes back reduced per
 * instance and per group of instances instead of as a [K][B][3] trace. Instances may differ in milestones, their number and their speed. */
#define WBC_MAX_TRAJ_POINTS 32
typedef struct WbcTrajectory {
  int32_t max_points;       /* S: row length of `points`, 2 <= S <= WBC_MAX_TRAJ_POINTS                          */
  int32_t ee_index;         /* 0..4: which end effector's target follows the trajectory (sim3.py: 4, the gripper) */
  const double* points;     /* [B][S][3] milestones; milestone i sits at parameter i (klampt Trajectory(milestones=...)) */
  const int32_t* n_points;  /* [B] milestones of instance b, 2..S; NULL => S for all                              */
  const double* du;         /* [B] parameter advance per tick (sim3.py:225: 0.002); NULL => du_all for all        */
  double du_all;
} WbcTrajectory;

typedef struct WbcRolloutSummary {   /* all optional; per instance [B], per group [B / group_size] */
  double*  err_sq_sum;      /* sum over ticks of |gripper reached after tick k - gripper target of tick k|^2 */
  double*  err_max;  int32_t* err_max_tick;   /* largest such error and the FIRST tick it occurred at */
  double*  err_final;       /* the last tick's error */
  int32_t* first_bad_tick;  /* first tick whose status != WBC_QP_OPTIMAL, -1 if none */
  int32_t* bad_ticks;       /* number of such ticks */
  int32_t  group_size;      /* M > 0: instances [g*M, (g+1)*M) form group g (B % M == 0 required); 0: no groups */
  int32_t  pad_;
  double*  group_rms;       /* sqrt(sum of err_sq_sum over the group / (M * ticks)) */
  double*  group_err_max;
  int32_t* group_worst_status;   /* max of status_max over the group */
  int32_t* group_bad_instances;  /* instances of the group with bad_ticks > 0 */
} WbcRolloutSummary;

/* wbc_rollout_tp with the target of end effector traj->ee_index following the instance's trajectory: on tick k = 0 .. r->ticks - 1 it is
 * eval_b(k * du_b) — the parameter is the PRODUCT, not a running sum, and eval is klampt's: t <= 0 gives the first milestone, t >= n_points - 1
 * the last (the hold phase), otherwise i = floor(t), u = t - i, (1 - u) * m[i] + u * m[i + 1], each product and sum rounded on its own, so a host
 * restatement (wbc_workload.traj_targets) is bit-exact. in0->ee_target's row of that end effector is not read (tick 0 gets eval(0)); every other
 * target and every WbcRollout field is wbc_rollout's (trunk_target_step included; ee_target_final holds eval(ticks * du) in the followed row).
 * Refused with WBC_E_ARG: r->ee_target_step not NULL, r->hold_ticks not 0, max_points / ee_index out of range, points NULL, du NULL with a
 * du_all that is not finite and positive, a group_size that does not divide B. mode RUNNING and WARMUP alike; tp NULL = no per-instance rows.
 * Bad rows — a non-finite point among the instance's first n_points, du non-finite or <= 0, n_points outside 2..S — are found on the device:
 * that instance's followed target stays at in0's value for the whole roll-out (nothing non-finite reaches a solve), its status_max is
 * WBC_QP_NUMERICAL, first_bad_tick 0 and bad_ticks = ticks; the other instances are unaffected (statistic "last_traj_bad_rows").
 * The errors are those of the gripper (end effector 4) whichever end effector follows the trajectory. sum may be NULL (no summary). Group
 * results come from one wavefront per group and a reduction of fixed shape, no floating-point atomics: two identical calls give identical bits.
 * Per tick: the tick kernel and the update kernel of wbc_rollout plus one small kernel (csrc/wbc_k_traj.hip), one lane per instance. */
int wbc_rollout_traj(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                     const WbcTrajectory* traj, const WbcRolloutSummary* sum /* may be NULL */, int mem, void* stream);

/* ------------------------------------------------------------------ roll-outs with several followed targets (tracks), trunk included
 * What the reference's drivers do beyond one gripper trajectory: the trunk target follows its own milestones while the gripper target stands
 * still (sim3.py:207, :216-217, :297-298 with sim_id == 1; sim2.py:202, :291-292), the trajectory is a Hermite spline (sim2.py:216-218:
 * HermiteTrajectory().makeSpline(traj)), and several targets move at once (setInitialState, Robot_Wrapper4.py:264-283). A track is one target
 * (an end effector's or the trunk's) on one per-instance trajectory; every frame may be scored against its target of the tick, followed or not. */
#define WBC_MAX_TRACKS 6
#define WBC_TARGET_TRUNK 5                 /* targets / frames: 0..4 = end effectors FR, FL, RR, RL, GRIP; 5 = trunk */
enum { WBC_TRACK_LINEAR = 0, WBC_TRACK_HERMITE = 1 };

typedef struct WbcTrack {
  int32_t target;            /* 0..5, each target at most once per call */
  int32_t kind;              /* WBC_TRACK_* */
  int32_t max_points;        /* S: 2 <= S <= WBC_MAX_TRAJ_POINTS */
  int32_t pad_;
  const double*  points;     /* [B][S][3] milestones, milestone i at parameter i */
  const double*  tangents;   /* [B][S][3] HERMITE only: d(target)/d(parameter) at the milestones (what klampt keeps as the second half of
                                a HermiteTrajectory milestone); NULL => the rule below. Must be NULL for LINEAR */
  const int32_t* n_points;   /* [B] 2..S; NULL => S */
  const double*  du;         /* [B]; NULL => du_all */
  double du_all;
} WbcTrack;

typedef struct WbcTracks {
  int32_t n_tracks, pad_;    /* 1..WBC_MAX_TRACKS */
  WbcTrack track[WBC_MAX_TRACKS];
  double* trunk_target_final;   /* [B][3] optional: the trunk target the NEXT tick would get */
} WbcTracks;

typedef struct WbcTrackScores {  /* all arrays optional */
  int32_t score_mask;        /* bit f: frame f is scored against its target of the tick, followed or constant; n_scored = popcount */
  int32_t group_size;        /* as WbcRolloutSummary */
  double  *err_sq_sum, *err_max, *err_final;  int32_t* err_max_tick;      /* [n_scored][B], frames in increasing index order */
  int32_t *first_bad_tick, *bad_ticks;                                    /* [B] */
  double  *trace;            /* [ticks][n_scored][B][3] positions reached (optional) */
  double  *group_rms, *group_err_max;                                     /* [n_scored][B / M] */
  int32_t *group_worst_status, *group_bad_instances;                      /* [B / M] */
} WbcTrackScores;

/* wbc_rollout_tp with every followed target on its track: on tick k = 0 .. r->ticks - 1 the target of track j is eval_b(k * du_b) (the PRODUCT,
 * as in wbc_rollout_traj), clamped at both ends (t <= 0: the first milestone, t >= n_points - 1: the last). The followed rows of in0->ee_target
 * and in0->trunk_target are not read; ee_target_final and trunk_target_final hold eval(ticks * du) in the followed rows. Everything else is
 * wbc_rollout_tp's: both modes, tp, imu, grip_trace, status_max, iters_sum, the warm start carried between ticks.
 *   LINEAR   i = floor(t), u = t - i: (1 - u) * m[i] + u * m[i + 1] — wbc_rollout_traj's arithmetic.
 *   HERMITE  unit knot spacing, per component: u2 = u * u, u3 = u * u2, cx1 = (2.0 * u3 - 3.0 * u2) + 1.0, cx2 = (-2.0 * u3) + 3.0 * u2,
 *            cv1 = (u3 - 2.0 * u2) + u, cv2 = u3 - u2, x = ((cx1 * m[i] + cx2 * m[i + 1]) + cv1 * v[i]) + cv2 * v[i + 1]; every operation
 *            rounded on its own, so the host restatement (wbc_workload.track_targets) is bit-exact.
 *   Default tangents (tangents == NULL; the rule of klampt's makeSpline(preventOvershoot=True)): n = 2: v[0] = v[1] = m[1] - m[0]. n >= 3:
 *            v[0] = v[n - 1] = 0; interior i, per component with a = m[i - 1], x = m[i], b = m[i + 1], w = (b - a) * 0.5, third = 1.0 / 3.0,
 *            the first case that matches: (1) x <= min(a, b) or x >= max(a, b): 0; (2) (w < 0 and x - w * third >= a) or (w > 0 and
 *            x - w * third <= a): 3.0 * (x - a); (3) (w < 0 and x + w * third < b) or (w > 0 and x + w * third > b): 3.0 * (b - x); (4) w.
 *            No segment of such a spline leaves the interval of its two milestones. Computed on the fly from the neighbouring milestones.
 * The error of frame f on tick k is |frame f reached after tick k - target of frame f on tick k|, formed as (dx * dx + dy * dy) + dz * dz, summed
 * in tick order, the maximum kept with a strictly-greater comparison (the first tick of the maximum). scores may be NULL.
 * Refused with WBC_E_ARG, naming the field: r->ee_target_step not NULL; r->hold_ticks not 0; r->trunk_target_step together with a trunk track
 * (without one it stays allowed); n_tracks outside 1..6; a repeated target; target, kind or max_points out of range; points NULL; tangents
 * with a LINEAR track; du NULL with a du_all that is not finite and positive; a trunk track or score bit 5 without in0->trunk_target /
 * prev_trunk_target; score_mask bits >= 6; a group_size that does not divide B.
 * Bad rows, found on the device: an instance is bad if any of its tracks has a non-finite point or caller tangent among its first n_points, a
 * du that is not finite and positive, or n_points outside 2..S. ALL of that instance's followed targets stay at in0's values (nothing
 * non-finite reaches a solve), its status is WBC_QP_NUMERICAL, first_bad_tick 0 and bad_ticks = ticks; it is counted in the statistic
 * "last_traj_bad_rows"; the other instances keep identical bits. Group results: one wavefront per group, fixed-shape reduction, no
 * floating-point atomics. Per tick: the tick and update kernels of wbc_rollout plus ONE launch of the trajectory kernel however many tracks. */
int wbc_rollout_tracks(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                       const WbcTracks* tracks, const WbcTrackScores* scores /* may be NULL */, int mem, void* stream);

/* ------------------------------------------------------------------ roll-out gradients along tracks: dL/d(milestones, tangents, speed)
 * wbc_rollout_record_tracks is wbc_rollout_tracks that also writes wbc_rollout_record's tape (same layout, same wbc_rollout_tape_bytes: the
 * tape holds every target as the tick saw it, followed or not); wbc_rollout_vjp_tracks is wbc_rollout_vjp's sweep with the target
 * bookkeeping of a followed target replaced by the adjoint of the track evaluation. Every output of the record call, the
 * scores included, is bit-identical to wbc_rollout_tracks' on the same inputs and handle state. It refuses what wbc_rollout_tracks refuses,
 * what wbc_rollout_record refuses, and tracks == NULL (the plain call exists for that).
 * THE SWEEP. Forward, a followed target is E_k = eval_b(k * du_b) on every tick (the PRODUCT; tick 0 gets eval(0), in0's followed row is not
 * read), and P_(k+1) = E_k where the task is on, as before. So for a followed end effector at tick k the whole cotangent of E_k is
 *     e_k = a_k + on o Pbar        (a_k = tick.d_ee_target + step.d_foot_targets; the trunk track: the same under task_trunk)
 * it goes into the track and nothing is carried: Ebar of a followed row is 0 in front of every tick; Pbar updates as in wbc_rollout_vjp.
 * Adjoint of the evaluation, with t = (double)k * du, n = n_points and the forward's own comparisons:
 *   t <= 0: d_points[0] += e.   t >= n - 1: d_points[n - 1] += e (neither gives anything to d_du).   Otherwise i = floor(t), u = t - i (at an
 *   exact knot the forward selects segment i with u = 0, and d_du uses that segment's derivative) and
 *   LINEAR   d_points[i] += (1 - u) e; d_points[i + 1] += u e; d_du += k ((x + y) + z), x, y, z = (m[i + 1][c] - m[i][c]) e[c].
 *   HERMITE  d_points[i] += cx1 e; d_points[i + 1] += cx2 e; vbar_i = cv1 e, vbar_(i+1) = cv2 e; d_du += k ((x + y) + z) with, per component,
 *            ((((6 u2 - 6 u) m[i] + (-6 u2 + 6 u) m[i + 1]) + ((3 u2 - 4 u) + 1) v[i]) + (3 u2 - 2 u) v[i + 1]) e. Caller tangents:
 *            d_tangents[i] += vbar_i, d_tangents[i + 1] += vbar_(i+1). Default tangents: vbar goes through the branch the rule took for that
 *            milestone and component (first milestone i, then i + 1; the plus term first): n = 2: +vbar to m[1], -vbar to m[0]; end
 *            milestones and case (1): nothing; (2) +3 vbar to m[i], -3 vbar to m[i - 1]; (3) +3 vbar to m[i + 1], -3 vbar to m[i];
 *            (4) +vbar / 2 to m[i + 1], -vbar / 2 to m[i - 1].
 * Every entry is summed in reverse tick order by one lane, without atomics or contraction: two identical calls give identical bits and the
 * host restatement (wbc_workload.track_target_gradients) runs the same operations in the same order.
 * EXACT ZEROS AND BAD ROWS. The followed rows of d_ee_target / d_trunk_target are exactly 0; rows of d_points / d_tangents at or beyond
 * n_points[b] are exactly 0. A bad row (wbc_rollout_tracks' definition) gets all-zero rows in every output of the call and grad_status
 * WBC_GRAD_NONFINITE, as an instance with WBC_GRAD_NONFINITE from any layer; the other instances keep their bits; rows >= B are never
 * written. Unsolved ticks are dropped by wbc_rollout_vjp's rule; what reaches a dropped tick's targets through the step still flows into the track.
 * WBC_E_ARG, naming the field, before any launch: d_ee_target_step (no step exists under tracks); d_trunk_target_step together with a trunk
 * track (without one trunk_target_step stays allowed and d_trunk_target_step is wbc_rollout_vjp's); d_tangents on a LINEAR track or a
 * HERMITE track with tangents == NULL; tracks_out NULL; a tracks_out->track[j] member set for j >= n_tracks; what wbc_rollout_tracks and
 * what wbc_rollout_vjp refuse.
 * Not offered: hold ticks, gradients with respect to n_points, checkpoint-and-recompute (the scores as a loss: wbc_rollout_vjp_scored
 * below; the watch as a loss: wbc_rollout_vjp_watched further below).
 * Neither call allocates once the workspaces have their size; with device buffers both can be captured into a HIP graph.
 * Statistic "last_trackvjp_variant": the row of csrc/wbc_k_trackvjp.hip's table the last call launched last (key of the stage: 0 BEGIN,
 * 1 TICK), -1 before the first; wbc_variant_count("trackvjp") == 2. */
typedef struct WbcTrackGrad {          /* all optional; an output left NULL is not written */
  double* d_points;                    /* [B][S][3], S = the track's max_points; rows >= n_points[b] exactly 0 */
  double* d_tangents;                  /* [B][S][3]; HERMITE with caller tangents only */
  double* d_du;                        /* [B] (also when the track uses du_all: the caller sums) */
} WbcTrackGrad;
typedef struct WbcTracksGrad { WbcTrackGrad track[WBC_MAX_TRACKS]; } WbcTracksGrad;   /* track[j] belongs to tracks->track[j] */
int wbc_rollout_record_tracks(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                              const WbcTracks* tracks, const WbcTrackScores* scores /* may be NULL */, void* tape, size_t tape_bytes,
                              double* q_trace, int mem, void* stream);
int wbc_rollout_vjp_tracks(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                           const WbcTracks* tracks, const void* tape, size_t tape_bytes, const WbcRolloutSeed* seed, int mem,
                           const WbcRolloutGrad* out, const WbcTracksGrad* tracks_out, void* stream);
int wbc_rollout_tracks_grad_sizes(int32_t* sizeof_track_grad, int32_t* sizeof_tracks_grad); /* ctypes layout self-check */

/* ------------------------------------------------------------------ roll-out scores as a loss: dL/d(err_sq_sum, err_final, err_max)
 * wbc_rollout_vjp_scored is wbc_rollout_vjp_tracks' sweep seeded (also, or alone) with the cotangents of the scores the record call returned
 * (WbcTrackScores.err_sq_sum, err_final, err_max), formed on the device: one launch in front of every reverse tick's step layer and one
 * behind its link stage. wbc_rollout_vjp and wbc_rollout_vjp_tracks launch what they launched and return the same bits.
 * FORWARD (wbc_rollout_tracks): for a scored frame f (0..4 the end effectors, 5 the trunk) on tick k, d = reached_f(after tick k) -
 * target_f(of tick k), e2 = (dx dx + dy dy) + dz dz, e = sqrt(e2); err_sq_sum += e2, err_final = e, err_max with its FIRST tick. reached_f
 * is the frame's position at the integrated configuration shifted rigidly by (estimated base - integrated base); without an IMU quaternion
 * the state after the tick keeps the integrated orientation and joints and takes the estimated base, so reached_f = FK_f(q_(k+1)) up to
 * rounding in both modes. The sweep recomputes d from the FK at q_(k+1) (the tape's q of tick k + 1; q_final for k = K - 1: the tape ends
 * at q_(K-1)) and the taped target of tick k. The recomputed e differs from the forward's by the rounding of the FK, which moves the
 * gradient's value at rounding level and no branch: the one branch, err_max's tick, is the caller's err_max_tick.
 * THE COTANGENT of d on tick k, with the caller's g_sq, g_fin, g_max [n_scored][B]:
 *     c = ((2 g_sq + [k == K - 1] g_fin / e) + [k == err_max_tick] g_max / e) d          (both 1 / e terms are 0 where e == 0)
 * To the state: g(q_(k+1)) += J_f(q_(k+1))' c, J_f the frame's translational Jacobian in the sweep's tangent coordinates (base DoF in the
 * base-local frame; a column is lin + ang x p_f of the WORLD joint Jacobian), summed over the scored frames in increasing order, added
 * BEFORE the step layer of tick k runs: where g_q_trace[k] enters. To the target: -c joins the cotangent of E_k (the trunk target for f = 5)
 * AFTER the link stage of tick k and before the track stage: LINK's d_*_target_step += Ebar must see the cotangent of E_(k+1) alone. A
 * followed row then reaches the track adjoint with e_k containing -c; a row no track follows ends in d_ee_target / d_trunk_target
 * (- sum_k c_k); a trunk target under trunk_target_step without a trunk track gives d_trunk_target_step - sum_k k c_k; at k = 0 LINK has
 * written the caller's d_*_target rows, which take -c_0 as well. The score's cotangent flows whatever the tick's QP status was (the forward
 * sums e2 on every tick); ticks_dropped keeps its meaning. An exact zero is never added (all-zero cotangents with a state seed give
 * wbc_rollout_vjp_tracks' bits). Nothing is contracted into fused multiply-adds and there are no atomics: identical calls, identical bits.
 * PER-INSTANCE FAULTS: a g_err_* value of a scored frame or a q_final entry (among the model's nq) that is not finite, or an err_max_tick
 * outside [0, K) while g_err_max != 0, gives the instance all-zero rows in every output and WBC_GRAD_NONFINITE, as a bad track row does; the
 * other instances keep their bits; rows >= B are never written.
 * WBC_E_ARG, naming the field, before any launch: score NULL (the other entry points exist for that); no g_err_* at all; g_err_max without
 * err_max_tick; q_final NULL; score_mask 0 or with bits >= 6; bit 5 without in0->trunk_target; r->imu not NULL (the state then discards the
 * orientation the scored position was formed with); whatever wbc_rollout_vjp_tracks refuses — except that `seed` may be NULL or empty here:
 * with both seeds the gradients are those of the summed loss. WBC_E_UNSUPPORTED as wbc_rollout_record (the packed whole-tree schedule).
 * Not offered: an IMU quaternion fed back under a score seed, hold ticks, wbc_rollout_traj's one-track summary, the
 * group scores (group RMS is an expression of err_sq_sum), gradients with respect to n_points, checkpoint-and-recompute.
 * The workspace lives in the handle with wbc_rollout_vjp's: no allocation after the first call of a size; with device buffers the call
 * can be captured into a HIP graph.
 * Statistic "last_scorevjp_variant": the SEED row of csrc/wbc_k_scorevjp.hip's table the last call launched (key of (STAGE, ROT) = (0, 0) or
 * (0, 1): the stage with the kinematics; the TARGET stage has the one row (1, 0)), -1 before the first; wbc_variant_count("scorevjp") == 3. */
typedef struct WbcScoreSeed {
  int32_t score_mask, pad_;        /* as the record call's WbcTrackScores.score_mask; n_scored = popcount */
  const double*  g_err_sq_sum;     /* [n_scored][B] dL/d err_sq_sum; optional */
  const double*  g_err_final;      /* [n_scored][B] dL/d err_final;  optional */
  const double*  g_err_max;        /* [n_scored][B] dL/d err_max;    optional, needs err_max_tick */
  const int32_t* err_max_tick;     /* [n_scored][B] as the record call returned it */
  const double*  q_final;          /* [B][27] the state after the last tick (record's q_final): the tape ends at q_(K-1) */
} WbcScoreSeed;
int wbc_rollout_vjp_scored(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                           const WbcTracks* tracks, const void* tape, size_t tape_bytes, const WbcRolloutSeed* seed /* may be NULL */,
                           const WbcScoreSeed* score, int mem, const WbcRolloutGrad* out, const WbcTracksGrad* tracks_out, void* stream);
int wbc_rollout_scored_sizes(int32_t* sizeof_score_seed); /* ctypes layout self-check */

/* ------------------------------------------------------------------ constraint slack: CoM box, trunk box, joint range
 * How far a configuration is from the reference's constraint limits, whether or not the configuration enforces them: what sim3.py prints
 * by hand (robot_data.com[0] and the frame positions, sim3.py:237-261, :353-355). Slack >= 0 inside, < 0 outside. All families are evaluated
 * at a configuration q [27] under instance b's model and configuration; four families in a fixed order, each the minimum of its components,
 * each component with a code:
 *   0 WBC_SLACK_COM        r = x, y: lower -(p_RR[r] - com[r]) (code 2 r), upper p_FL[r] - com[r] (2 r + 1); p_FL, p_RR: world positions of EE
 *                          frames 1 and 2, com: data.com[0] — the operands of CoMConstraint (Robot_Wrapper4.py:669-677) before 1 / dt and
 *                          com_box_scale.
 *   1 WBC_SLACK_TRUNK_Z    lower -((c0 - v) - z) (0), upper (c0 + v) - z (1); c0 = trunk_box_center[0], v = c0 * cfg.trunk_box_z_frac, z the
 *                          trunk frame's world z (trunkConstraint, :719, :735-736).
 *   2 WBC_SLACK_TRUNK_ANG  a = roll, pitch, yaw: lower -((c[1 + a] - cfg.trunk_box_ang) - e[a]) (2 a), upper (c[1 + a] + cfg.trunk_box_ang) - e[a]
 *                          (2 a + 1); e from the trunk rotation R as the tick kernels form it: atan2(R21, R22), atan2(-R20, sqrt(R21^2 + R22^2)),
 *                          atan2(R10, R00).
 *   3 WBC_SLACK_JOINT      every velocity DoF d with 6 <= d < cfg.lock_from, its joint's q index i: lower q[i] - q_lo[i] (2 d), upper
 *                          q_hi[i] - q[i] (2 d + 1) — the model's own range of the DoF's own joint (WbcModelBlob.q_lo / q_hi), not the damper's
 *                          index map (damper_qidx) and not the base. No such DoF: +inf, code -1.
 * `which` is the code of the component at the minimum: components are scanned in increasing code order with a strict <, so the lowest code wins
 * a tie. A row whose q holds a non-finite entry (among the model's nq) gives NaN and code -1 in all four families and NaN components; so do
 * family 1 when trunk_box_center[0] is not finite and family 2 when one of trunk_box_center[1..3] is not. The other instances are unaffected.
 * One kernel (csrc/wbc_k_slack.hip), four instances per wavefront, FK over the whole tree. WBC_E_UNSUPPORTED (the message names the limit) when
 * a model of the handle does not fit that kernel's schedule: more than 22 joints, a tree deeper than 7, more than 16 joints at one depth. */
#define WBC_N_SLACK 4
enum { WBC_SLACK_COM = 0, WBC_SLACK_TRUNK_Z = 1, WBC_SLACK_TRUNK_ANG = 2, WBC_SLACK_JOINT = 3 };
typedef struct WbcSlackOut {      /* all optional */
  double*  slack;       /* [B][4] */
  int32_t* which;       /* [B][4] */
  double*  components;  /* [B][12]: family 0's four, family 1's two, family 2's six, in code order */
} WbcSlackOut;
/* q [B][27]; trunk_box_center [B][4] or NULL (families 1, 2 and their components come back NaN / -1); model_id [B], required with several
 * models. Refused with WBC_E_ARG, naming the field: q NULL, out NULL. Needs a configured handle (lock_from, the box constants). */
int wbc_state_slack(WbcBatch* b, int B, const double* q, const double* trunk_box_center, const int32_t* model_id, int mem,
                    const WbcSlackOut* out, void* stream);

typedef struct WbcSlackWatch {
  int32_t mask;          /* bit f: family f is watched; n_w = popcount; rows below in increasing family order */
  int32_t group_size;    /* as WbcTrackScores */
  double  *slack_min, *slack_final;                  /* [n_w][B] */
  int32_t *slack_min_tick, *slack_min_which;         /* [n_w][B]: FIRST tick of the minimum (strictly-smaller rule), its code */
  int32_t *neg_ticks, *first_neg_tick;               /* [n_w][B]: ticks with slack < 0; the first of them, -1 if none */
  double  *trace;                                    /* [ticks + hold_ticks][n_w][B], optional */
  double  *group_min;  int32_t *group_neg_instances; /* [n_w][B / M]: min of slack_min; instances with neg_ticks > 0 */
} WbcSlackWatch;
/* The roll-outs above with the slacks watched: after every tick the roll-out runs (hold ticks included) ONE launch of the slack kernel
 * evaluates the watched families at the state the update kernel just wrote (current_joint_config after tick k: what q_final would hold),
 * with in0->trunk_box_center as the box centres, and folds them into the per-instance results — no second accumulation launch. All arrays
 * optional. A tick whose family slack is NaN makes that family's slack_min NaN for good: slack_min_tick is the first such tick, the code -1,
 * and neg_ticks does not count it. Group results come from one wavefront per group after the last tick (a fixed-shape reduction, no atomics:
 * two identical calls give identical bits); a NaN slack_min in a group gives a NaN group_min.
 * watch == NULL: exactly the tracks call when tracks are given, the plain per-instance-rows roll-out otherwise — the same launches, memsets
 * and outputs bit for bit. With a watch the roll-out's own outputs and scores are unchanged: the watch only reads. tracks may be NULL (then
 * r->ee_target_step and r->hold_ticks are allowed as in the plain roll-out); scores may be NULL and needs tracks.
 * Refused with WBC_E_ARG, naming the field: mask 0 or with bits >= 4; scores without tracks; a group_size that does not divide B; family 1
 * or 2 watched without in0->trunk_box_center; with tracks, the tracks call's own refusals. WBC_E_UNSUPPORTED as in the state call above. */
int wbc_rollout_watch(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                      const WbcTracks* tracks /* may be NULL */, const WbcTrackScores* scores /* may be NULL; needs tracks */,
                      const WbcSlackWatch* watch /* may be NULL */, int mem, void* stream);

/* ------------------------------------------------------------------ constraint slack as a loss: dL/d(q, trunk_box_center) at a state
 * wbc_state_slack_vjp is the cotangent of wbc_state_slack's outputs: with g_slack = dL/d slack [B][4] and g_components = dL/d components
 * [B][12] (either may be NULL, not both) it returns dL/dq in tangent coordinates at q (wbc_tick_vjp_state's convention: base DoF in the
 * base-local frame, joint DoF the identity) and dL/d trunk_box_center. One kernel launch (csrc/wbc_k_slackvjp.hip, the STATE stage), no
 * allocation and no memset: with device buffers the call can be captured into a HIP graph.
 * WHERE A FAMILY'S COTANGENT GOES. Component i of families 0..2 gets gamma_i = g_components[i] + g_slack[f], the second term only where i is
 * family f's `which`: the component the forward's scan selects (increasing code order, strict <: the lowest code wins a tie). The kernel runs
 * the forward's own evaluation (one set of inline functions, csrc/wbc_slack.h), so the selection is wbc_state_slack's bit for bit. At a tie
 * the slack is not differentiable and what is returned is a SUBGRADIENT: the gradient of the selected component. The joint family has no
 * exposed components: g_slack[3] goes to the DoF and side of its code (code -1: nowhere).
 * THE COTANGENTS, with the components as stated under wbc_state_slack:
 *     on p_FL (gamma1, gamma3, 0)     on p_RR (-gamma0, -gamma2, 0)     on com (gamma0 - gamma1, gamma2 - gamma3, 0)
 *     on the trunk frame's z  gamma4 - gamma5           on trunk_box_center[0]  -(1 - z_frac) gamma4 + (1 + z_frac) gamma5
 *     on angle a  c_e[a] = gamma(6 + 2a) - gamma(7 + 2a)  on trunk_box_center[1 + a]  -c_e[a]
 *     joint range: d_q[d] += +gamma for the lower side (even code), -gamma for the upper side
 * To the state, per DoF d with l, a its WORLD joint Jacobian column (linear part at the world origin, angular part), the frames' supports as
 * the model states them, mc and ms the sums of m_j c_j and m_j over the bodies of d's sub-tree and M the total mass:
 *     d_q[d] = [FL has d] (l + a x p_FL) . c_FL + [RR has d] (l + a x p_RR) . c_RR + ((ms l + a x mc) / M) . c_com
 *            + [trunk has d] ((l + a x p_T)_z (gamma4 - gamma5) + a . sum_a c_e[a] N_a(R)) + the joint term
 * N_a: d angle_a = N_a . omega under dR = [omega]x R, the three atan2 forms of wbc_tick_vjp_state's trunk box.
 * EXACT ZEROS AND BAD ROWS. Columns >= nv of d_q are 0; rows >= B are never written. A row is bad if q holds a non-finite entry among the
 * model's nq, if a cotangent of the row is not finite, or if a trunk_box_center entry is not finite while its family (1: entry 0; 2: entries
 * 1..3) carries a non-zero cotangent (g_slack[f] or one of the family's g_components). A bad row gets all-zero d_q and d_trunk_box_center
 * rows and WBC_GRAD_NONFINITE; the other rows keep their bits. `which` is no gradient: on every row it is wbc_state_slack's, bad or not.
 * WBC_E_UNSUPPORTED as wbc_state_slack (the packed whole-tree schedule). WBC_E_ARG, naming the field: q NULL, out NULL, both g arrays NULL,
 * model_id NULL with several models; trunk_box_center NULL together with a non-zero cotangent on family 1 or 2 — with host arrays; with
 * device arrays the cotangents are not read on the host, a NULL box counts as non-finite entries and the row is a bad row.
 * Statistic "last_slackvjp_variant": the row of csrc/wbc_k_slackvjp.hip's table the last call (this one or wbc_rollout_vjp_watched) launched
 * (key of (STAGE, ROT): STAGE 0 STATE, 1 SEED), -1 before the first; wbc_variant_count("slackvjp") == 4. */
typedef struct WbcSlackGrad {        /* all optional */
  double*  d_q;                 /* [B][26] tangent coordinates at q; columns >= nv are 0 */
  double*  d_trunk_box_center;  /* [B][4] */
  int32_t* which;               /* [B][4] the component each family's cotangent went to: wbc_state_slack's `which`, bit for bit */
  int32_t* grad_status;         /* [B] WBC_GRAD_OK / WBC_GRAD_NONFINITE */
} WbcSlackGrad;
int wbc_state_slack_vjp(WbcBatch* b, int B, const double* q, const double* trunk_box_center, const int32_t* model_id,
                        const double* g_slack /* [B][4], may be NULL */, const double* g_components /* [B][12], may be NULL */, int mem,
                        const WbcSlackGrad* out, void* stream);
int wbc_slack_grad_sizes(int32_t* sizeof_grad); /* ctypes layout self-check */

/* ------------------------------------------------------------------ the watch as a loss: dL/d(slack_min, slack_final, trace) through a roll-out
 * wbc_rollout_record_watch is wbc_rollout_watch with the record extension behind the watch (tracks optional; scores needs tracks; watch
 * required): every output is wbc_rollout_watch's bit for bit on the same inputs, the tape wbc_rollout_record's / _record_tracks'. It refuses
 * what those calls refuse; hold_ticks is refused (a recorded roll-out has none).
 * wbc_rollout_vjp_watched is the reverse sweep seeded (also, or alone) with the cotangents of what the watch returned. On tick k the
 * cotangent of watched family f is
 *     gamma_f = g_trace[k] + [k == K - 1] g_slack_final + [k == slack_min_tick] g_slack_min
 * (g_trace: dL/d(WbcSlackWatch.trace), the hook for any per-tick penalty, hinge or barrier), applied through wbc_state_slack_vjp's algebra
 * at q_(k+1) — the tape's q of tick k + 1, q_final behind the last tick — with in0->trunk_box_center as the box: ONE launch of the SEED
 * stage in front of tick k's step layer, behind the score seed's SEED stage where both are given (the order is fixed: the bits depend on
 * it). g(q_(k+1)) += the state term, the sweep's trunk_box_center accumulator += the box term; an exact zero is never added (all-zero
 * cotangents beside a state seed give wbc_rollout_vjp's / _tracks' bits). The selected component is recomputed at the taped state by the
 * forward's own evaluation; at a tie it is a subgradient as under wbc_state_slack_vjp.
 * The slack is evaluated at the state the update kernel wrote, which is exactly the taped state: an IMU quaternion fed back is allowed here
 * (the step layer zeroes the orientation part as it already does); a call with both a score seed and an IMU keeps the score's refusal.
 * d_trunk_box_center keeps the sweep's rule (it needs the trunk constraint) and then also holds the watch's box term. wbc_rollout_vjp,
 * _tracks and _scored launch what they launched and return the same bits.
 * PER-INSTANCE FAULTS: a seeded cotangent of the tick that is not finite (found at that tick), a non-finite q_final entry (among the
 * model's nq), a slack_min_tick outside [0, K) while g_slack_min != 0, a non-finite trunk_box_center entry of a family with a non-zero
 * cotangent: the instance gets all-zero rows in every output and WBC_GRAD_NONFINITE, like a layer that reports it mid-sweep.
 * WBC_E_ARG, naming the field, before any launch: watch NULL; no g array; g_slack_min without slack_min_tick; q_final NULL; mask 0 or with
 * bits >= 4; family 1 or 2 without in0->trunk_box_center; tracks_out not NULL exactly when tracks is; score without tracks; whatever the
 * sweep refuses — except that `seed` may be NULL or empty. The workspace is wbc_rollout_vjp's: no allocation after the first call of a
 * size; with device buffers the call can be captured into a HIP graph.
 * Not offered: hold ticks, wbc_rollout_traj's one-track call, the group minima (expressions of slack_min), neg_ticks / first_neg_tick
 * (integers), gradients with respect to the box constants of WbcConfig, checkpoint-and-recompute. */
typedef struct WbcWatchSeed {
  int32_t mask, pad_;             /* families of the rows below, increasing order; n_w = popcount; bits < 4 */
  const double*  g_slack_min;     /* [n_w][B]; optional, needs slack_min_tick */
  const double*  g_slack_final;   /* [n_w][B]; optional */
  const double*  g_trace;         /* [ticks][n_w][B]; optional */
  const int32_t* slack_min_tick;  /* [n_w][B] as the record call returned it */
  const double*  q_final;         /* [B][27] the state after the last tick */
} WbcWatchSeed;
int wbc_rollout_record_watch(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                             const WbcTracks* tracks /* may be NULL */, const WbcTrackScores* scores /* may be NULL; needs tracks */,
                             const WbcSlackWatch* watch, void* tape, size_t tape_bytes, double* q_trace, int mem, void* stream);
int wbc_rollout_vjp_watched(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                            const WbcTracks* tracks /* may be NULL */, const void* tape, size_t tape_bytes,
                            const WbcRolloutSeed* seed /* may be NULL */, const WbcScoreSeed* score /* may be NULL; needs tracks */,
                            const WbcWatchSeed* watch, int mem, const WbcRolloutGrad* out,
                            const WbcTracksGrad* tracks_out /* NULL exactly when tracks is NULL */, void* stream);
int wbc_rollout_watched_sizes(int32_t* sizeof_watch_seed); /* ctypes layout self-check */

/* Knobs of a handle (none of them changes a result beyond rounding; defaults in brackets):
 *   "jtj_mfma"        [-1] H = A'A of wbc_tick / wbc_assemble (QP_Wrapper.py:17) on the fp64 matrix cores (v_mfma_f64_16x16x4_f64)
 *                          or as the sparse vector-unit contraction. -1: matrix cores when the Cartesian task stack has
 *                          >= WBC_MFMA_AUTO_ROWS rows (measured: +9 % ticks/s at 33 and 45 rows, a wash at 6); 0: never;
 *                          1: always — that also selects the general tick kernel (the compact sim3 kernel has no matrix-core
 *                          path), so on the sim3 switch set it costs the structural speed-up.
 *   "presolve"         [1] structural elimination of the stance-foot contact equalities (Robot_Wrapper4.py:757-761) where no
 *                          task touches the stance legs; 0: every QP runs at its full size n = nv.
 *   "presolve_orth"    [1] the same elimination where tasks DO touch the stance legs (foot / trunk / CoM tasks, e.g. BASELINE
 *                          configs[1]), through an orthonormal basis of the contact rows' null space (Householder QR per instance):
 *                          the reduced QP is as well conditioned as the full one; the base and stance-leg velocity bounds become
 *                          6 + 3 x (stance feet) two-sided rows. 0: those configurations run at full size. Needs "presolve".
 *   "orth_qr"          [0] diagnostic: that basis always by the Householder QR of the contact rows; by default only instances with a
 *                          nearly rank-deficient stance-leg block take it, the others orthonormalise [I; -K^-1 B] through a 6 x 6
 *                          Cholesky factor (same null space, a quarter of the instructions).
 *   "sim3_kernel"      [1] batches whose every model has such an elimination plan, <= 16 constraint rows and no orientation
 *                          references run on the compact wbc_tick_sim3_kernel (+ a second pass of the general kernel over the
 *                          instances whose leg blocks it could not eliminate); 0: the general kernel does the elimination.
 *   "packed_kernel"    [1] batches of the sim3 switch-set family itself (Grip task or none, optionally the trunk task, trunk box + foot
 *                          contacts, velocity bounds, posture PREV / Tikhonov / static HYBRID — or any mode with posture_u / q_con
 *                          supplied by the posture kernel or the caller: the QCON variant; the gripper's orientation reference is
 *                          honoured; working sets in and out are taken: the WARM variant) run FOUR instances per wavefront
 *                          (wbc_tick_sim3p_kernel: ONE kernel per tick — an instance it cannot reduce, a stance-leg block of rank < 2, is
 *                          redone by its own wave on the general path at the end of the same kernel); 0: one instance per wavefront
 *                          (wbc_tick_sim3_kernel + second pass). Also gates "packed_orth", "packed_box" and the packed QP kernel of
 *                          wbc_qp_solve / wbc_qp_solve_ls (0: one problem per wavefront there too).
 *   "wave_order"       [1] the packed sim3 kernel records how many dual iterations each instance needed, and the next launch on the
 *                          handle groups instances of like work into the same wavefronts, heaviest first (wbc_rollout carries it from
 *                          tick to tick; a changed batch size or wbc_batch_configure gives one launch in the identity order), from
 *                          16384 instances on (below, one round of waves has nothing to regroup and the bookkeeping costs 2-5 us);
 *                          2: at every batch size up to 130048; 0: the identity order (A/B timing). Results are bit-identical either way.
 *   "packed_orth"      [1] the equality-only task problems (BASELINE configs[1]: EE tasks + CoM task + posture Tikhonov / PREV, foot
 *                          contacts the only constraints, no velocity box) run FOUR instances per wavefront on wbc_tick_orthp_kernel
 *                          (orthonormal contact presolve, unconstrained reduced problem) from 4608 instances on — below that one round
 *                          of waves covers the batch and the one-instance kernel's shorter dependent chain wins (25 vs 55 us at
 *                          B = 1024, equal at 4096, 0.29 vs 0.78 ms at 65536); 2: at every batch size; 0: never. Its INEQ variant covers
 *                          the same task problems WITH inequality rows (trunk box, CoM box, the velocity box — rows of Z in the reduced
 *                          coordinates, two per lane — and the trunk task: tests' "everything", 0.58 vs 1.24 ms at 65536), cold or hot-started.
 *   "packed_box"       [1] the task problems WITHOUT constraint rows (the warm-up problem of setInitialState, Robot_Wrapper4.py:196-351:
 *                          trunk / EE tasks + posture Tikhonov / PREV, velocity box only) run FOUR instances per wavefront on
 *                          wbc_tick_boxp_kernel: the base and, where 16 lanes do not hold the rest, the limb DoF with the widest box are
 *                          eliminated by a Schur complement, the dual method works on <= 16 bounded unknowns, and an instance whose
 *                          optimum holds an eliminated DoF at its own velocity bound (or more than 12 active bounds) is redone by
 *                          its wave on the general path. Working sets in / out: its WARM variant. At every batch size (28 vs 29 us at
 *                          B = 1, 40 vs 46 us at 1024, 0.37 vs 1.23 ms at 65536); 0: never (general kernel).
 *   "posture_par"      [1] qpJointb "MANI" / "HYBRID" targets on the parallel posture kernels: every sweep on a lane of its own (both sides of
 *                          the central difference one after the other), three instances per wavefront, where no model has more than 21
 *                          sweeps (statistic "last_posture_par" = 2), else every finite-difference point on a lane of its own, one instance
 *                          per wavefront (= 1; value 3 forces this form); 0: the sequential whole-tree kernel (52 sweeps per instance).
 *   "packed_update"    [1] wbc_update_state / the roll-out's state update run four instances per wavefront where every model's
 *                          configuration is of the packed kernel's family (statistic "last_update_packed"); 0: one per wavefront.
 *   "presolve_tol_exp" [7] a stance-leg 3 x 3 block K with |det K| <= 10^-value (sum |K_ij|)^3 is treated as rank deficient: the
 *                          compact kernel eliminates it with column pivoting and keeps one leg velocity + one contact equality
 *                          in the reduced QP (the general kernel's in-kernel presolve falls back to the full problem).
 *                          0: every block of every instance takes that path.
 *   "count_pivoted"    [0] diagnostic: count the instances that took the pivoted elimination (statistic "pivoted_last"; one
 *                          atomic per such instance — leave it off when timing).
 *   "dbg_force_defer"  [0] diagnostic: an instance with a flagged block takes the path of a block of rank < 2 instead of the pivoted
 *                          elimination — the packed kernel's tail (general path, same kernel), the one-instance kernel's second pass.
 *   "warm_start"       [0] 1: wbc_rollout carries every instance's final working set into its next tick (the hot start the
 *                          reference gets from QP.solveQPHotstart, Robot_Wrapper4.py:1389-1394); 0: every tick starts cold.
 *                          Same minimiser either way (H > 0). Warm ticks stay on the packed kernel (its WARM variant: seeds through
 *                          the add step, x / u rebuilt from the factors, restoration). Measured on MI355X at B = 65536
 *                          (profiles/r03_rollout_warm_vs_cold.txt): closed loop 277.5 vs 280.6 M ticks/s un-stressed (-1 %), 190.0
 *                          vs 197.7 M on the stress recipe (-4 %); open-loop ticks seeded with their own set +2 % / 0 %, with the
 *                          previous tick's -1.5 %: a dual method that starts at the unconstrained minimiser needs one iteration
 *                          per active inequality (0.9-1.05 here), a seed replaces it by an add step + a share of the rebuild, and
 *                          both pay the final feasibility scan. Off by default; never the 2.2x of round 2's fallback kernel.
 *                          (wbc_tick is warm exactly when WbcTickIn.working_set is passed.)
 *   "refine"           [1] one step of iterative refinement at the final working set (0 = off) — the analogue of the reference's
 *                          qpOASES option numRefinementSteps = 100 (QP_Wrapper.py:37). With the active normals N, their multipliers u
 *                          and the dual method's factors (J J' = H^-1, J'N' = [R; 0]):  r1 = -(grad f - N'u),  x += J2 J2' r1 (+ the
 *                          active rows' own residual through R). grad f is formed from the UNFACTORED least-squares data — A'(A x - b)
 *                          as two products, task block by task block, never through H = A'A: fl(A'A) carries the benchmark tick's
 *                          1.5e-9 posture block with 1e-5 relative error, which is the whole 1e-6 the plain method is off by at
 *                          cond(H) ~ 3e9. One step lands within 1e-8 of the exact least-squares optimum (oracle: qp_refine; both sides
 *                          refine, so the parity margin on BASELINE configs[2] went from 5.7e-6 to 6.6e-8 against the 1e-5 tolerance,
 *                          profiles/r04_soak_long.txt). A correction larger than 0.25 max(1, |x|) or non-finite is not applied; on wbc_qp_solve_ls (arbitrary
 *                          problems) a QP whose smallest Cholesky pivot is above 1e-5 x its largest diagonal entry skips the step — the ticks refine always. Cost on the benchmark: 5.5 % (profiles/r04_ab_refine.txt). Refined: the packed
 *                          sim3 kernel and its variants, the general kernel (full size and structural presolve), wbc_qp_solve_ls
 *                          (wbc_qp_solve, given H and g alone, could only use -(H x + g): no gain where H itself is the rounding — measured — so it does not refine). Not refined, because their
 *                          stacks are well conditioned (1e-8 .. 1e-10 without): the packed orth / box kernels and the orthonormal
 *                          presolve; and the one-instance compact kernel (path 1: no room at 168 VGPRs / 13 KB LDS) — with refine > 0
 *                          what it would take runs on the general kernel instead (refine = 0 brings it back).
 *   "sim3p_fixd"       [1] a handle with ONE model whose sim3 plan has the a1_wx200 dimensions (26 DoF, 27 coordinates, 11 reduced unknowns,
 *                          4 stance feet eliminated, 4 kept rows) runs a call without a model_id array on the packed sim3 kernel's FIXD form:
 *                          those dimensions are compile-time constants there (statistic "last_tick_fixd"). Every other handle and call
 *                          runs the form that reads them from the plan; 0: always that form (A/B timing, tests). Results are
 *                          bit-identical either way.
 *   "packed_min_batch" [1] the packed sim3 kernel takes batches from this many instances on. 1: it is the fastest path of the sim3
 *                          family at EVERY batch size (13.6 us at B = 1 against 19 us on either one-instance kernel, 41 vs 53-55 us at
 *                          1024: profiles/r04_small_batch_c3.txt).
 *   "grid"                 workgroups of the grid-stride kernels (wbc_qp_solve*, wbc_integrate); default = what fills the chip.
 *   "dbg_alias_inputs" [0] diagnostic: every instance reads instance 0's inputs (isolates input latency in timings).
 *   "dbg_stop"         [0] diagnostic (ablation build of the library only): the sim3 kernel stops after stage k (1..7, see csrc/wbc_k_sim3.hip;
 *                          101.. the packed sim3 kernel, 201.. the packed orth kernel, 301.. the packed box kernel) — outputs are garbage,
 *                          only the run time means something (tools/ablate_sim3.py, ablate_orthp.py, ablate_boxp.py). */
int wbc_batch_set_option(WbcBatch* b, const char* name, int value);

/* Read-only statistics of a handle: "last_path" (kernel the last tick ran on: 0 general, 1 compact sim3 + second pass, 2 packed
 * compact sim3 — four instances per wavefront, one kernel —, 3 packed orth kernel, 4 packed box kernel), "last_orth" (1: that tick ran with the
 * orthonormal contact presolve, option "presolve_orth": the general kernel's ORTH variant or the packed orth kernel),
 * "last_qp_path" (problems per wavefront of the last wbc_qp_solve / wbc_qp_solve_ls call: 4, 2 or 1),
 * "last_tick_fixd" (1: the last tick ran the packed sim3 kernel's FIXD form, option "sim3p_fixd" — the same row of the variant table, same
 * "last_tick_variant"; 0: the form with the plan's dimensions read at run time, or another kernel),
 * "last_update_packed" (1: the last state update ran on the packed kernel), "last_posture_par" (1 / 2: the last MANI / HYBRID posture target
 * ran on the parallel posture kernel, one / three instances per wavefront), "deferred_last" (instances the last tick's kernel could not reduce itself: redone in the packed kernels'
 * tail or left to the one-instance kernel's second pass; waits for `stream`), "pivoted_last" (instances that took the pivoted
 * elimination, with option "count_pivoted"), "wave_order_slices" (slices of waves whose recorded order the next packed sim3 launch at
 * the last such launch's batch size will read: ceil(ceil(B / 4) / 127) once the order is in effect, 0 without it; waits for `stream`),
 * "last_traj_bad_rows" (bad rows the last wbc_rollout_traj / wbc_rollout_tracks on the handle found; waits for `stream`),
 * "sim3_lds_bytes" / "tick_lds_bytes" / "orthp_lds_bytes" (LDS per workgroup of the tick kernels).
 *
 * "last_tick_variant" / "last_qp_variant": WHICH instantiation of a kernel family the last launch resolved — the row of the family's variant
 * table (csrc/wbc_k_<family>.hip, <FAMILY>_VARIANTS), as a five-byte key; -1 before the first such launch. "last_tick_variant" covers wbc_tick*,
 * every tick of the roll-outs, wbc_assemble* and wbc_fk_jacobians; "last_qp_variant" covers wbc_qp_solve and wbc_qp_solve_ls. The key holds the
 * row's template arguments in the table's order, first argument in the most significant byte, unused trailing bytes 0:
 *     key = (((a0 * 256 + a1) * 256 + a2) * 256 + a3) * 256 + a4          a_i = (key >> 8 * (4 - i)) & 255
 * The family comes from "last_path" (ticks) or "last_qp_path" (QPs: 1 -> qp, 2 / 4 -> qpp); wbc_assemble* and wbc_fk_jacobians always run on the
 * general family. Arguments per family (flags are 0 / 1):
 *     general (last_path 0)  MODE, WARM, ORTH, ROT, TP       MODE: 0 = MODE_TICK, 1 = MODE_ASSEMBLE, 2 = MODE_FK
 *     sim3p   (last_path 2)  WARM, TRUNK, QCON, ROT, TP
 *     orthp   (last_path 3)  INEQ, WARM, ROT, TP
 *     boxp    (last_path 4)  WARM, ROT, TP
 *     qpp     (last_qp_path 2, 4)  G, PV, WARM, HALF         G: lanes per problem (16 / 32), PV: the layout's row capacity (16 / 26)
 *     qp      (last_qp_path 1)     NM, WARM                  NM: the solver core's size (12, 16, 24, 26)
 *     compact sim3 (last_path 1; no table, four forms)  WARM, ROT
 * WARM: working sets are read / written; ORTH: the orthonormal contact presolve; ROT: a model of the handle has a rotated joint placement;
 * TP: per-instance task rows (wbc_tick_tp); TRUNK: the trunk task; QCON: posture_u / q_con given or computed by the posture kernel;
 * INEQ: the packed orth kernel's form with inequality rows; HALF: rows of C split over the two halves of a problem. */
int wbc_batch_get_stat(WbcBatch* b, const char* name, void* stream, int64_t* out);

/* wait for everything queued by this handle on `stream`. */
int wbc_batch_synchronize(WbcBatch* b, void* stream);

/* diagnostics: per-phase shader-cycle sums of wbc_tick since the last call, filled only by the -DWBC_PROFILE build of
 * the library (zeros otherwise): [0] ticks, [1] FK+Jacobians, [2] task stack, [3] Cholesky, [4] L^-1 and x0,
 * [5] equality phase, [6] inequality phase, [7] output/integrate, [8] working-set changes, [9..12] task-stack sub-phases, [13..19] contact-presolve sub-phases (24 values). */
int wbc_debug_cycles(WbcBatch* b, uint64_t* out24);

const char* wbc_last_error(void);
const char* wbc_version(void);
int wbc_abi_sizes(int32_t* sizeof_blob, int32_t* sizeof_config); /* ctypes layout self-check */
/* rows of a kernel family's variant table ("general", "sim3p", "orthp", "boxp", "qpp", "qp"; "grad": statistic "last_grad_variant"), generated from the table itself: what a census of
 * the statistics "last_tick_variant" / "last_qp_variant" has to reach. Needs no handle and no device. Unknown family: WBC_E_ARG. */
int wbc_variant_count(const char* family);

#ifdef __cplusplus
}
#endif
#endif /* WBC_H_ */
