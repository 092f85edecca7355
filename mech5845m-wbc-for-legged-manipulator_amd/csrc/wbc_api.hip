// wbc_api.hip — the C-ABI of include/wbc.h on top of the gfx950 kernels (handles, validation, host staging).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <cmath>
#include <new>
#include <vector>
#include "wbc_device.h"
#include "wbc_traj.h"        // (brings in wbc_track.h, whose file-scope `#pragma clang fp contract(off)` holds for the rest of this unit: host code
                             //  only, no device code, and the x86 build contracts nothing either way)
#include "wbc_slack.h"
#include "wbc_cert.h"
#include "wbc_grad.h"
#include "wbc_gradq.h"
#include "wbc_stepvjp.h"
#include "wbc_rollvjp.h"
#include "wbc_trackvjp.h"
#include "wbc_scorevjp.h"
#include "wbc_slackvjp.h"

// (the layouts of the handle's roll-out workspaces d_roll, d_traj and d_slack: RollWs, TrajWs and SlackWs below)

using namespace wbc;

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
// The time step of every entry point that takes one (include/wbc.h): dt and 1 / dt both finite and positive. +inf (1 / dt = 0, qdot * dt =
// 0 * inf) and a subnormal dt (1 / dt = inf) pass a bare "dt > 0". backward: wbc_integrate alone, where dt < 0 is a step back.
static int check_dt(double dt, const char* who, bool backward = false) {
  const double inv = 1.0 / dt;
  if (std::isfinite(dt) && std::isfinite(inv) && (backward || dt > 0)) return WBC_OK;
  if (backward) return fail(WBC_E_ARG, "%s: dt = %g: dt and 1 / dt finite required", who, dt);
  return fail(WBC_E_ARG, "%s: dt = %g: dt > 0 with dt and 1 / dt finite required", who, dt);
}
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(WBC_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
  } while (0)

// the kernels a tick runs on (select_tick_path); the values are those of the statistic "last_path"
enum TickPath : int { TICK_GENERAL = 0, TICK_SIM3 = 1, TICK_SIM3P = 2, TICK_ORTHP = 3, TICK_BOXP = 4 };

struct WbcModel {
  WbcModelBlob blob;
  DevModel dev;
};

// The packed sim3 kernel's batch-size policy (tools/small_batch.py, profiles/r04_small_batch_c3.txt): below this many instances a launch is a
// single partial round of waves and one tick's latency is what counts.
constexpr int WBC_SIM3P_MIN_BATCH = 1;
// The packed sim3 kernel's wave order (option "wave_order" 1) from this many instances on: it costs a launch a dependent load at entry and a
// returning atomic at exit, 2-5 us at B = 1 .. 4096 (one partial round of waves, nothing to regroup), neutral at 8192, -21 % at 16384
// (tools/small_batch.py, profiles/r07_small_batch_c3_wave_order.txt).
constexpr int WBC_WAVE_ORDER_MIN_BATCH = 16384;

struct WbcBatch {
  int device_id, n_models, max_batch, grid;
  const WbcModel* models[WBC_MAX_MODELS];
  WbcConfig cfg_host[WBC_MAX_MODELS];
  DevPlan plan_host[WBC_MAX_MODELS];
  bool configured[WBC_MAX_MODELS];
  DevModel* d_models;
  WbcConfig* d_cfgs;
  DevPlan* d_plans;
  void* ws;
  size_t ws_bytes;
  int mrows, prows, mcart;
  int jtj_mfma;
  int presolve, presolve_orth, orth_qr;
  double sing_tol;
  int sim3_kernel;       // 1 (default): batches that qualify run on wbc_tick_sim3_kernel (compact LDS) + a deferred pass
  int32_t* d_status;     // status buffer of our own when the caller passes none (the deferred pass needs one)
  int dbg_alias, dbg_stop;
  int count_pivoted, force_defer;   // diagnostics of the sim3 kernel's pivoted elimination / second pass
  int packed_min_batch;  // the packed sim3 kernel takes batches from this many instances on (default WBC_SIM3P_MIN_BATCH; option "packed_min_batch")
  int packed_kernel;     // 1 (default): eligible batches run four instances per wavefront (wbc_tick_sim3p_kernel)
  int posture_par, last_posture_par;   // option [1]: MANI / HYBRID posture targets on wbc_posture_par_kernel (every finite-difference point on its own lane); what the last one ran on
  int packed_box;        // 1 (default): task problems without constraint rows (the warm-up problem) run four instances per wavefront (wbc_tick_boxp_kernel)
  int packed_orth;       // 1 (default): equality-only task problems run four instances per wavefront (wbc_tick_orthp_kernel)
  int refine;            // iterative-refinement steps at the final working set (default 1; 0 = the plain dual method: tests / A-B timing)
  int warm_start;        // 1: wbc_rollout carries each instance's working set from tick to tick (default 0: measured slower)
  int32_t* d_defer;      // [1 + max_batch]: count + compact list of the instances the sim3 kernel deferred (lazy)
  unsigned long long* d_dstat;   // packed kernel: (launch sequence, instances its tail redid on the general path) (lazy)
  int wave_order;        // 1 (default): the packed sim3 kernel deals instances out by last launch's work (KernelArgs.worder) from WBC_WAVE_ORDER_MIN_BATCH
                         // instances on; 2: at every batch size; 0: identity order
  WaveOrder* d_worder;   // that order: slice blocks and two lists per slice (lazy)
  int worder_reset;      // wbc_batch_configure was called: the next launch that uses the order clears it first, on its own stream
  int worder_B;          // batch size of the last packed sim3 launch that used the order (0: none; statistic "wave_order_slices")
  uint32_t tick_seq;
  int packed_update, last_update_packed;   // option: wbc_update_packed_kernel where every plan allows it [1]; what the last update ran on
  int last_orth;         // the last general-kernel tick ran the variant with the orthonormal contact presolve
  int last_qp_path;      // problems per wavefront of the last wbc_qp_solve / wbc_qp_solve_ls: 1 (wbc_qp_kernel), 2 or 4 (wbc_qp_packed_kernel)
  long long last_grad_variant;   // ... and of the last wbc_tick_vjp launch
  long long last_gradq_variant;  // ... and of the last wbc_tick_vjp_state launch
  long long last_stepvjp_variant;   // ... and of the last wbc_step_vjp launch
  long long last_rollvjp_variant;   // ... and of the last link-kernel launch of wbc_rollout_vjp
  long long last_trackvjp_variant;  // ... and of the last track-adjoint launch of wbc_rollout_vjp_tracks
  long long last_scorevjp_variant;  // ... and of the last score-cotangent launch of wbc_rollout_vjp_scored
  long long last_slackvjp_variant;  // ... and of the last slack-cotangent launch (wbc_state_slack_vjp, wbc_rollout_vjp_watched)
  long long last_tick_variant, last_qp_variant;   // variant_key(...) of the row the last tick / assemble / fk launch and the last stand-alone QP launch resolved (-1: none yet)
  int sim3p_fixd;        // option [1]: the packed sim3 kernel's FIXD form where the handle qualifies (fixd_dims)
  bool fixd_dims[WBC_MAX_MODELS];   // wbc_batch_configure: the model's plan has exactly the SIM3P_FIXD_* dimensions
  int last_tick_fixd;    // the last tick ran a FIXD instantiation of the packed sim3 kernel
  int last_path;         // TickPath of the last wbc_tick / wbc_rollout tick: 0 general, 1 sim3 (+ deferred pass), 2 packed sim3, 3 packed orth, 4 packed box
  int max_nj, max_nf;    // FK output strides: the largest model's joint / frame counts
  int rot;               // a model of the handle has a rotated joint placement: the packed kernels run their ROT instantiations
  unsigned long long* d_prof;
  double *d_pu, *d_pq;   // qpJointb MANI/HYBRID results: u [max_batch][26], q_after [max_batch][27] (lazy)
  void* d_roll;          // wbc_rollout's mutable controller state for max_batch instances (lazy)
  void* d_traj;          // wbc_rollout_traj / wbc_rollout_tracks: per-instance scores of six frames, their positions of the tick, bad-row flags and their count (lazy)
  SlackLimits* d_slack_lim;   // wbc_state_slack / wbc_rollout_watch: the models' own joint ranges by DoF (lazy)
  void* d_slack;         // wbc_rollout_watch: per-instance accumulators of the four families for max_batch instances (lazy)
  void* d_rvjp;          // wbc_rollout_vjp: one tick's QP image, certificate, layer outputs and the sweep's accumulators for max_batch instances (lazy, grown)
  size_t rvjp_bytes;
};

// ---------------------------------------------------------------------------------------------- workspaces
// A workspace the handle allocates on first use (wbc_batch_destroy frees what is non-null).
template <class T> static int ensure(T*& p, size_t bytes) {
  if (!p) HIP_TRY(hipMalloc((void**)&p, bytes));
  return WBC_OK;
}
// d_defer: the count, the list of up to max_batch instances the compact sim3 kernel leaves to the deferred pass, and four words behind the
// list (KernelArgs.defer_aux): [0] the pivot counter (statistic "pivoted_last"), [1] the deferred pass's own, [2] the statistic "deferred_last".
enum { DEFER_TAIL_WORDS = 4, DEFER_TAIL_LAST = 2 };
static size_t defer_bytes(const WbcBatch* b) { return sizeof(int32_t) * ((size_t)b->max_batch + DEFER_TAIL_WORDS); }
static int32_t* defer_tail(const WbcBatch* b) { return b->d_defer + 1 + b->max_batch; }

// The roll-out workspaces, each stated once as tables of blocks: a block holds `width` values per instance of max_batch (NB), the blocks follow
// one another without padding, doubles first. Every block is strided by NB — never by a call's B, which strides the caller's outputs.
template <class W, class T> struct Block { T* W::*ptr; size_t width; };
template <class W, class T, size_t N> constexpr size_t block_bytes(const Block<W, T> (&t)[N]) {   // per instance
  size_t s = 0;
  for (size_t i = 0; i < N; ++i) s += t[i].width * sizeof(T);
  return s;
}
template <class W, class T, size_t N> static char* carve_blocks(W& w, char* p, size_t NB, const Block<W, T> (&t)[N]) {
  for (size_t i = 0; i < N; ++i) { w.*t[i].ptr = (T*)p; p += NB * t[i].width * sizeof(T); }
  return p;
}

struct RollWs {   // d_roll: wbc_rollout's mutable controller state, the tick's outputs, the working sets carried from tick to tick [NB][2]
  double *q, *q_next, *qdot, *ee_target, *prev_ee_target, *trunk_target, *prev_trunk_target, *ee_prev_rot, *trunk_prev_rot;
  int32_t *status, *iters;
  unsigned long long* working_set;
  static size_t bytes(size_t NB);
  static RollWs carve(void* base, size_t NB);
};
constexpr Block<RollWs, double> ROLL_D[] = {{&RollWs::q, WBC_Q_STRIDE}, {&RollWs::q_next, WBC_Q_STRIDE}, {&RollWs::qdot, WBC_V_STRIDE},
    {&RollWs::ee_target, 3 * WBC_NEE}, {&RollWs::prev_ee_target, 3 * WBC_NEE}, {&RollWs::trunk_target, 3}, {&RollWs::prev_trunk_target, 3},
    {&RollWs::ee_prev_rot, 9 * WBC_NEE}, {&RollWs::trunk_prev_rot, 9}};
constexpr Block<RollWs, int32_t> ROLL_I[] = {{&RollWs::status, 1}, {&RollWs::iters, 1}};
constexpr Block<RollWs, unsigned long long> ROLL_U[] = {{&RollWs::working_set, 2}};
static_assert(block_bytes(ROLL_D) == 170 * sizeof(double) && block_bytes(ROLL_I) == 2 * sizeof(int32_t) && block_bytes(ROLL_U) == 2 * sizeof(unsigned long long),
              "d_roll: 170 doubles, 2 int32 and 2 64-bit words per instance");
static_assert(block_bytes(ROLL_I) % 8 == 0, "d_roll: the working sets begin at a multiple of 8 bytes for any max_batch");
size_t RollWs::bytes(size_t NB) { return NB * (block_bytes(ROLL_D) + block_bytes(ROLL_I) + block_bytes(ROLL_U)); }
RollWs RollWs::carve(void* base, size_t NB) {
  RollWs w;
  carve_blocks(w, carve_blocks(w, carve_blocks(w, (char*)base, NB, ROLL_D), NB, ROLL_I), NB, ROLL_U);
  return w;
}

struct TrajWs {   // d_traj: per-instance scores of six frames, the frames' positions of the tick [6][3], bad-row flags; one int32 follows: their count
  double *err_sq_sum, *err_max, *err_final, *frames;
  int32_t *bad, *first_bad_tick, *bad_ticks, *status_max, *err_max_tick, *bad_count;
  static size_t bytes(size_t NB);
  static TrajWs carve(void* base, size_t NB);
};
constexpr Block<TrajWs, double> TRAJ_D[] = {{&TrajWs::err_sq_sum, WBC_MAX_TRACKS}, {&TrajWs::err_max, WBC_MAX_TRACKS}, {&TrajWs::err_final, WBC_MAX_TRACKS},
    {&TrajWs::frames, 3 * WBC_MAX_TRACKS}};
constexpr Block<TrajWs, int32_t> TRAJ_I[] = {{&TrajWs::bad, 1}, {&TrajWs::first_bad_tick, 1}, {&TrajWs::bad_ticks, 1}, {&TrajWs::status_max, 1},
    {&TrajWs::err_max_tick, WBC_MAX_TRACKS}};
static_assert(block_bytes(TRAJ_D) == 36 * sizeof(double) && block_bytes(TRAJ_I) == 10 * sizeof(int32_t), "d_traj: 36 doubles and 10 int32 per instance (+ one int32)");
size_t TrajWs::bytes(size_t NB) { return NB * (block_bytes(TRAJ_D) + block_bytes(TRAJ_I)) + sizeof(int32_t); }
TrajWs TrajWs::carve(void* base, size_t NB) {
  TrajWs w;
  w.bad_count = (int32_t*)carve_blocks(w, carve_blocks(w, (char*)base, NB, TRAJ_D), NB, TRAJ_I);
  return w;
}

struct SlackWs {   // d_slack: wbc_rollout_watch's per-instance accumulators of the four families
  double *slack_min, *slack_final;
  int32_t *min_tick, *min_which, *neg_ticks, *first_neg;
  static size_t bytes(size_t NB);
  static SlackWs carve(void* base, size_t NB);
};
constexpr Block<SlackWs, double> SLACK_D[] = {{&SlackWs::slack_min, SLACK_NF}, {&SlackWs::slack_final, SLACK_NF}};
constexpr Block<SlackWs, int32_t> SLACK_I[] = {{&SlackWs::min_tick, SLACK_NF}, {&SlackWs::min_which, SLACK_NF}, {&SlackWs::neg_ticks, SLACK_NF},
    {&SlackWs::first_neg, SLACK_NF}};
static_assert(block_bytes(SLACK_D) + block_bytes(SLACK_I) == SLACK_NF * (2 * sizeof(double) + 4 * sizeof(int32_t)), "d_slack: 2 doubles and 4 int32 per family and instance");
size_t SlackWs::bytes(size_t NB) { return NB * (block_bytes(SLACK_D) + block_bytes(SLACK_I)); }
SlackWs SlackWs::carve(void* base, size_t NB) {
  SlackWs w;
  carve_blocks(w, carve_blocks(w, (char*)base, NB, SLACK_D), NB, SLACK_I);
  return w;
}

// The tape of wbc_rollout_record (the CALLER's device memory; include/wbc.h states the layout): a head of the previous rotations every tick
// after the first saw, then one TapeWs per tick. Unlike the handle's workspaces the blocks are strided by the call's B: the tape is sized by it.
struct TapeHead {
  double *ee_prev_rot, *trunk_prev_rot;
  static TapeHead carve(void* tape, size_t B);
};
constexpr Block<TapeHead, double> TAPE_HEAD_D[] = {{&TapeHead::ee_prev_rot, 9 * WBC_NEE}, {&TapeHead::trunk_prev_rot, 9}};
struct TapeWs {   // tick k: the state and the targets the tick saw, its answer, status and working set
  double *q, *qdot, *ee_target, *prev_ee_target, *trunk_target, *prev_trunk_target;
  int32_t *status, *pad;
  unsigned long long* working_set;
  static TapeWs carve(void* tape, size_t B, int k);
};
constexpr Block<TapeWs, double> TAPE_D[] = {{&TapeWs::q, WBC_Q_STRIDE}, {&TapeWs::qdot, WBC_V_STRIDE}, {&TapeWs::ee_target, 3 * WBC_NEE},
    {&TapeWs::prev_ee_target, 3 * WBC_NEE}, {&TapeWs::trunk_target, 3}, {&TapeWs::prev_trunk_target, 3}};
constexpr Block<TapeWs, int32_t> TAPE_I[] = {{&TapeWs::status, 1}, {&TapeWs::pad, 1}};
constexpr Block<TapeWs, unsigned long long> TAPE_U[] = {{&TapeWs::working_set, 2}};
constexpr size_t TAPE_HEAD_BYTES = block_bytes(TAPE_HEAD_D), TAPE_TICK_BYTES = block_bytes(TAPE_D) + block_bytes(TAPE_I) + block_bytes(TAPE_U);
static_assert(TAPE_HEAD_BYTES == 432 && TAPE_TICK_BYTES == 736, "the tape: 432 bytes per instance, 736 bytes per instance and tick (include/wbc.h)");
static_assert(block_bytes(TAPE_D) % 8 == 0 && block_bytes(TAPE_I) % 8 == 0, "the tape: the working sets begin at a multiple of 8 bytes for any B");
TapeHead TapeHead::carve(void* tape, size_t B) {
  TapeHead h;
  carve_blocks(h, (char*)tape, B, TAPE_HEAD_D);
  return h;
}
TapeWs TapeWs::carve(void* tape, size_t B, int k) {
  TapeWs w;
  carve_blocks(w, carve_blocks(w, carve_blocks(w, (char*)tape + B * (TAPE_HEAD_BYTES + (size_t)k * TAPE_TICK_BYTES), B, TAPE_D), B, TAPE_I), B, TAPE_U);
  return w;
}

// The gradient layers' outputs, each struct stated once as a table: the member, its doubles per instance, its name, which
// input of the configuration it is the gradient of (Read: the "requested, but ..." refusals, the wiring of the sweep's tick outputs) and that
// input's name in the refusal. The rows stand in the struct's order, which is the order the entry points stage them in.
enum Read { R_ALWAYS, R_EE, R_EE_EST, R_TRUNK, R_COM, R_PU, R_BOX };
template <class G> struct OutRow { double* G::*ptr; size_t width; const char* name; Read need; const char* src; };
constexpr OutRow<WbcTickGrad> TICK_OUT[] = {{&WbcTickGrad::d_task_params, WBC_TASK_PARAMS_DOUBLES, "d_task_params", R_ALWAYS, nullptr},
    {&WbcTickGrad::d_ee_target, 3 * WBC_NEE, "d_ee_target", R_EE, "ee_target"}, {&WbcTickGrad::d_prev_ee_target, 3 * WBC_NEE, "d_prev_ee_target", R_EE, "prev_ee_target"},
    {&WbcTickGrad::d_trunk_target, 3, "d_trunk_target", R_TRUNK, nullptr}, {&WbcTickGrad::d_prev_trunk_target, 3, "d_prev_trunk_target", R_TRUNK, nullptr},
    {&WbcTickGrad::d_com_target, 3, "d_com_target", R_COM, nullptr}, {&WbcTickGrad::d_com_target_vel, 3, "d_com_target_vel", R_COM, nullptr},
    {&WbcTickGrad::d_posture_u, WBC_V_STRIDE, "d_posture_u", R_PU, nullptr}};
constexpr OutRow<WbcTickStateGrad> TICKQ_OUT[] = {{&WbcTickStateGrad::d_q, WBC_V_STRIDE, "d_q", R_ALWAYS, nullptr},
    {&WbcTickStateGrad::d_trunk_box_center, 4, "d_trunk_box_center", R_BOX, nullptr}};
constexpr OutRow<WbcStepGrad> STEP_OUT[] = {{&WbcStepGrad::d_q, WBC_V_STRIDE, "d_q", R_ALWAYS, nullptr}, {&WbcStepGrad::d_qdot, WBC_V_STRIDE, "d_qdot", R_ALWAYS, nullptr},
    {&WbcStepGrad::d_foot_targets, 3 * WBC_NEE, "d_foot_targets", R_ALWAYS, nullptr}};
template <class G, size_t N> constexpr size_t out_width(const OutRow<G> (&t)[N], double* G::*ptr) {
  for (size_t i = 0; i < N; ++i) if (t[i].ptr == ptr) return t[i].width;
  return 0;
}
// (the roll-out's outputs: the tick's and the tick-state's at their widths there, the steps as the targets they advance)
constexpr size_t tw(double* WbcTickGrad::*p) { return out_width(TICK_OUT, p); }
constexpr size_t qw(double* WbcTickStateGrad::*p) { return out_width(TICKQ_OUT, p); }
constexpr OutRow<WbcRolloutGrad> ROLL_OUT[] = {{&WbcRolloutGrad::d_q0, qw(&WbcTickStateGrad::d_q), "d_q0", R_ALWAYS, nullptr},
    {&WbcRolloutGrad::d_task_params, tw(&WbcTickGrad::d_task_params), "d_task_params", R_ALWAYS, nullptr}, {&WbcRolloutGrad::d_ee_target, tw(&WbcTickGrad::d_ee_target), "d_ee_target", R_EE_EST, "ee_target"},
    {&WbcRolloutGrad::d_prev_ee_target, tw(&WbcTickGrad::d_prev_ee_target), "d_prev_ee_target", R_EE, "prev_ee_target"}, {&WbcRolloutGrad::d_trunk_target, tw(&WbcTickGrad::d_trunk_target), "d_trunk_target", R_TRUNK, nullptr},
    {&WbcRolloutGrad::d_prev_trunk_target, tw(&WbcTickGrad::d_prev_trunk_target), "d_prev_trunk_target", R_TRUNK, nullptr}, {&WbcRolloutGrad::d_com_target, tw(&WbcTickGrad::d_com_target), "d_com_target", R_COM, nullptr},
    {&WbcRolloutGrad::d_com_target_vel, tw(&WbcTickGrad::d_com_target_vel), "d_com_target_vel", R_COM, nullptr}, {&WbcRolloutGrad::d_posture_u, tw(&WbcTickGrad::d_posture_u), "d_posture_u", R_PU, nullptr},
    {&WbcRolloutGrad::d_trunk_box_center, qw(&WbcTickStateGrad::d_trunk_box_center), "d_trunk_box_center", R_BOX, nullptr},
    {&WbcRolloutGrad::d_ee_target_step, tw(&WbcTickGrad::d_ee_target), "d_ee_target_step", R_EE_EST, "ee_target"}, {&WbcRolloutGrad::d_trunk_target_step, tw(&WbcTickGrad::d_trunk_target), "d_trunk_target_step", R_TRUNK, nullptr}};

struct RollVjpWs {   // d_rvjp: wbc_rollout_vjp's workspace — one tick's QP image and certificate, the layers' outputs of the tick, the sweep's accumulators
  double *lb, *ub, *v, *g, *s_dq, *s_dft, *sens_x, *sens_bounds, *t_dq, *t_box, *t_tp, *t_ee, *t_pee, *t_tt, *t_ptt, *t_com, *t_comv, *t_pu;
  double *Ebar, *Pbar, *TEbar, *TPbar, *d_estep, *d_tstep, *acc_tp, *acc_com, *acc_comv, *acc_pu, *acc_box;
  double* stash;   // wbc_rollout_vjp_scored: -c of the tick's six scored frames [NB][6][3]
  int32_t *cert_status, *gs_step, *gs_tick, *gs_tickq, *worst, *dropped;
  double *A, *b, *C, *Clb, *Cub, *y_rows, *sens_rows;   // [NB][M][26], [NB][M], [NB][p][26], [NB][p] x 4: M = task rows + padding rows, p = constraint rows
  static size_t bytes(size_t NB, size_t M, size_t p);
  static RollVjpWs carve(void* base, size_t NB, size_t M, size_t p);
};
// where the sweep keeps one tick's outputs of the tick layer: the block's width is the output's
constexpr struct TickWire { double* WbcTickGrad::*out; double* RollVjpWs::*ws; } TICK_WS[] = {{&WbcTickGrad::d_task_params, &RollVjpWs::t_tp},
    {&WbcTickGrad::d_ee_target, &RollVjpWs::t_ee}, {&WbcTickGrad::d_prev_ee_target, &RollVjpWs::t_pee}, {&WbcTickGrad::d_trunk_target, &RollVjpWs::t_tt},
    {&WbcTickGrad::d_prev_trunk_target, &RollVjpWs::t_ptt}, {&WbcTickGrad::d_com_target, &RollVjpWs::t_com}, {&WbcTickGrad::d_com_target_vel, &RollVjpWs::t_comv},
    {&WbcTickGrad::d_posture_u, &RollVjpWs::t_pu}};
constexpr Block<RollVjpWs, double> tick_block(int i) { return {TICK_WS[i].ws, tw(TICK_WS[i].out)}; }
constexpr Block<RollVjpWs, double> RVJP_D[] = {{&RollVjpWs::lb, WBC_V_STRIDE}, {&RollVjpWs::ub, WBC_V_STRIDE}, {&RollVjpWs::v, WBC_V_STRIDE},
    {&RollVjpWs::g, WBC_V_STRIDE}, {&RollVjpWs::s_dq, out_width(STEP_OUT, &WbcStepGrad::d_q)}, {&RollVjpWs::s_dft, out_width(STEP_OUT, &WbcStepGrad::d_foot_targets)},
    {&RollVjpWs::sens_x, WBC_V_STRIDE}, {&RollVjpWs::sens_bounds, WBC_V_STRIDE}, {&RollVjpWs::t_dq, qw(&WbcTickStateGrad::d_q)},
    {&RollVjpWs::t_box, qw(&WbcTickStateGrad::d_trunk_box_center)}, tick_block(0), tick_block(1), tick_block(2), tick_block(3),
    tick_block(4), tick_block(5), tick_block(6), tick_block(7), {&RollVjpWs::Ebar, 3 * WBC_NEE}, {&RollVjpWs::Pbar, 3 * WBC_NEE}, {&RollVjpWs::TEbar, 3},
    {&RollVjpWs::TPbar, 3}, {&RollVjpWs::d_estep, 3 * WBC_NEE}, {&RollVjpWs::d_tstep, 3}, {&RollVjpWs::acc_tp, WBC_TASK_PARAMS_DOUBLES},
    {&RollVjpWs::acc_com, 3}, {&RollVjpWs::acc_comv, 3}, {&RollVjpWs::acc_pu, WBC_V_STRIDE}, {&RollVjpWs::acc_box, 4}, {&RollVjpWs::stash, 3 * WBC_MAX_TRACKS}};
static_assert(sizeof(TICK_WS) / sizeof(TICK_WS[0]) == sizeof(TICK_OUT) / sizeof(TICK_OUT[0]) && sizeof(TICK_WS) / sizeof(TICK_WS[0]) == 8, "one block of d_rvjp per output of the tick layer");
constexpr Block<RollVjpWs, int32_t> RVJP_I[] = {{&RollVjpWs::cert_status, 1}, {&RollVjpWs::gs_step, 1}, {&RollVjpWs::gs_tick, 1}, {&RollVjpWs::gs_tickq, 1},
    {&RollVjpWs::worst, 1}, {&RollVjpWs::dropped, 1}};
static_assert(block_bytes(RVJP_D) == 573 * sizeof(double) && block_bytes(RVJP_I) == 6 * sizeof(int32_t), "d_rvjp: 573 doubles and 6 int32 per instance (+ the QP image)");
static_assert(block_bytes(RVJP_I) % 8 == 0, "d_rvjp: the QP image begins at a multiple of 8 bytes for any max_batch");
size_t RollVjpWs::bytes(size_t NB, size_t M, size_t p) {
  return NB * (block_bytes(RVJP_D) + block_bytes(RVJP_I) + sizeof(double) * (M * (WBC_V_STRIDE + 1) + p * (WBC_V_STRIDE + 4)));
}
RollVjpWs RollVjpWs::carve(void* base, size_t NB, size_t M, size_t p) {
  RollVjpWs w;
  double* d = (double*)carve_blocks(w, carve_blocks(w, (char*)base, NB, RVJP_D), NB, RVJP_I);
  w.A = d; d += NB * M * WBC_V_STRIDE;
  w.b = d; d += NB * M;
  w.C = d; d += NB * p * WBC_V_STRIDE;
  w.Clb = d; d += NB * p;
  w.Cub = d; d += NB * p;
  w.y_rows = d; d += NB * p;
  w.sens_rows = d;
  return w;
}

// ---------------------------------------------------------------------------------------------- model
static bool is_identity(const double* R) {
  static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 9; ++i)
    if (R[i] != I[i]) return false;
  return true;
}
// A proper rotation: R R' = I and det R = +1, each within 1e-12 (the URDF's rpy="3.14 0 0" of the ViperX-300 elbow / wrist_rotate is one;
// a reflection or a sheared matrix is not).
static bool is_rotation(const double* R) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2];
      if (!(fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-12)) return false;
    }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  return fabs(det - 1.0) <= 1e-12;
}

extern "C" int wbc_model_create(const WbcModelBlob* b, WbcModel** out) {
  if (!b || !out) return fail(WBC_E_ARG, "wbc_model_create: null argument");
  if (b->njoints < 2 || b->njoints > WBC_MAX_JOINTS || b->nv < 6 || b->nv > WBC_MAX_NV || b->nq != b->nv + 1 || b->nq > WBC_Q_STRIDE)
    return fail(WBC_E_ARG, "wbc_model_create: sizes out of range (njoints %d, nq %d, nv %d)", b->njoints, b->nq, b->nv);
  if (b->jtype[1] != WBC_JT_FF || b->parent[1] != 0 || b->idx_q[1] != 0 || b->idx_v[1] != 0)
    return fail(WBC_E_UNSUPPORTED, "wbc_model_create: joint 1 must be the free-flyer root (Robot_Wrapper4.py:21)");
  if (b->nframes < WBC_FR_NROLES || b->nframes > WBC_MAX_FRAMES) return fail(WBC_E_ARG, "wbc_model_create: nframes %d", b->nframes);
  WbcModel* m = new (std::nothrow) WbcModel;
  if (!m) return fail(WBC_E_ARG, "out of memory");
  m->blob = *b;
  DevModel& d = m->dev;
  memset(&d, 0, sizeof d);
  d.nq = b->nq; d.nv = b->nv; d.njoints = b->njoints; d.nframes = b->nframes;
  int depth[WBC_MAX_JOINTS] = {0};
  double total = 0;
  for (int j = 1; j < b->njoints; ++j) {
    const int t = b->jtype[j];
    if (b->parent[j] < 0 || b->parent[j] >= j) { delete m; return fail(WBC_E_ARG, "joint %d: parent %d not before it", j, b->parent[j]); }
    if (j > 1 && !(t >= WBC_JT_RX && t <= WBC_JT_PZ)) { delete m; return fail(WBC_E_UNSUPPORTED, "joint %d: type %d unsupported on device", j, t); }
    if (j == 1 && !is_identity(b->place_R[1])) { delete m; return fail(WBC_E_UNSUPPORTED, "root joint placement must be identity"); }
    if (!is_identity(b->place_R[j]) && !is_rotation(b->place_R[j])) {
      delete m; return fail(WBC_E_UNSUPPORTED, "joint %d: rotated joint placement is not a proper rotation (orthonormal, det +1)", j);
    }
    if (j > 1 && b->parent[j] < 1) { delete m; return fail(WBC_E_UNSUPPORTED, "joint %d: only one root joint supported", j); }
    if (j == 1 && (b->place_p[1][0] != 0 || b->place_p[1][1] != 0 || b->place_p[1][2] != 0)) { delete m; return fail(WBC_E_UNSUPPORTED, "root joint placement must be identity"); }
    depth[j] = depth[b->parent[j]] + 1;
    if (depth[j] > d.maxdepth) d.maxdepth = depth[j];
    d.parent[j] = b->parent[j]; d.depth[j] = depth[j]; d.jtype[j] = t; d.idx_q[j] = b->idx_q[j]; d.idx_v_of[j] = b->idx_v[j];
    const int a = (t >= WBC_JT_RX && t <= WBC_JT_RZ) ? t - WBC_JT_RX : (t >= WBC_JT_PX ? t - WBC_JT_PX : 0);
    d.ax0[j] = a; d.ax1[j] = (a + 1) % 3; d.ax2[j] = (a + 2) % 3;
    d.tp[j][0] = b->place_p[j][d.ax0[j]]; d.tp[j][1] = b->place_p[j][d.ax1[j]]; d.tp[j][2] = b->place_p[j][d.ax2[j]];
    if (!is_identity(b->place_R[j])) {   // columns P e_a, P e_a1, P e_a2 of the row-major placement rotation, then t (fk_place_rot)
      d.rot_mask |= 1u << j;
      const int ax[3] = {d.ax0[j], d.ax1[j], d.ax2[j]};
      for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) d.rp[j][3 * c + r] = b->place_R[j][3 * r + ax[c]];
      for (int r = 0; r < 3; ++r) d.rp[j][9 + r] = b->place_p[j][r];
    }
    d.mass[j] = b->mass[j];
    for (int i = 0; i < 3; ++i) d.com[j][i] = b->com[j][i];
    total += b->mass[j];
    // velocity columns of this joint
    const int nvj = (t == WBC_JT_FF) ? 6 : 1;
    if (b->idx_v[j] < 0 || b->idx_v[j] + nvj > b->nv) { delete m; return fail(WBC_E_ARG, "joint %d: idx_v out of range", j); }
    // idx_q becomes a global write index (q_next) and a shift count in the kernels: 1-DoF joints live in [7, nq)
    if (t != WBC_JT_FF && (b->idx_q[j] < 7 || b->idx_q[j] >= b->nq)) { delete m; return fail(WBC_E_ARG, "joint %d: idx_q %d outside [7, nq = %d)", j, b->idx_q[j], b->nq); }
    for (int c = 0; c < nvj; ++c) {
      const int k = b->idx_v[j] + c;
      d.col_joint[k] = j; d.col_lin[k] = -1; d.col_ang[k] = -1; d.col_q[k] = b->idx_q[j] + c;
      if (t == WBC_JT_FF) { if (c < 3) d.col_lin[k] = c; else d.col_ang[k] = c - 3; }
      else if (t <= WBC_JT_RZ) d.col_ang[k] = a;
      else d.col_lin[k] = a;
    }
  }
  d.total_mass = total;
  auto on_path = [&](int anc, int j) { while (j > 0) { if (j == anc) return true; j = b->parent[j]; } return false; };
  for (int k = 0; k < b->nv; ++k) {
    uint32_t mask = 0;
    for (int j = 1; j < b->njoints; ++j) if (on_path(d.col_joint[k], j)) mask |= 1u << j;
    d.col_subtree[k] = mask;
  }
  for (int f = 0; f < b->nframes; ++f) {
    const int jf = b->frame_joint[f];
    if (jf < 1 || jf >= b->njoints) { delete m; return fail(WBC_E_ARG, "frame %d: supporting joint %d out of range", f, jf); }
    if (!is_identity(b->frame_R[f])) { delete m; return fail(WBC_E_UNSUPPORTED, "frame %d: rotated frame offset unsupported on device (no robot of the reference needs one)", f); }
    d.frame_joint[f] = jf;
    for (int i = 0; i < 3; ++i) d.frame_p[f][i] = b->frame_p[f][i];
    uint32_t mask = 0;
    for (int k = 0; k < b->nv; ++k) if (on_path(d.col_joint[k], jf)) mask |= 1u << k;
    d.frame_support[f] = mask;
  }
  *out = m;
  return WBC_OK;
}

extern "C" void wbc_model_destroy(WbcModel* m) { delete m; }

// ---------------------------------------------------------------------------------------------- batch
extern "C" void wbc_batch_destroy(WbcBatch* b);
extern "C" int wbc_batch_create(const WbcModel* const* models, int n_models, int max_batch, int device_id, WbcBatch** out) {
  if (!out || n_models < 0 || n_models > WBC_MAX_MODELS || (n_models > 0 && !models) || max_batch < 1)
    return fail(WBC_E_ARG, "wbc_batch_create: bad arguments (n_models %d, max_batch %d)", n_models, max_batch);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(WBC_E_HIP, "wbc_batch_create: no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(WBC_E_ARG, "wbc_batch_create: device %d of %d", device_id, ndev);
  HIP_TRY(hipSetDevice(device_id));
  WbcBatch* b = new (std::nothrow) WbcBatch;
  if (!b) return fail(WBC_E_ARG, "out of memory");
  memset(b, 0, sizeof *b);
  b->device_id = device_id; b->n_models = n_models; b->max_batch = max_batch; b->presolve = 1; b->presolve_orth = 1; b->packed_update = 1; b->sim3_kernel = 1; b->sing_tol = 1e-7; b->wave_order = 1; b->sim3p_fixd = 1;
  b->last_tick_variant = b->last_qp_variant = b->last_grad_variant = b->last_gradq_variant = b->last_stepvjp_variant = b->last_rollvjp_variant = b->last_trackvjp_variant = b->last_scorevjp_variant = b->last_slackvjp_variant = -1;
  b->jtj_mfma = -1; b->refine = 1; b->packed_min_batch = WBC_SIM3P_MIN_BATCH; b->warm_start = 0; b->packed_kernel = 1; b->packed_orth = 1; b->packed_box = 1; b->posture_par = 1;
  std::vector<DevModel> dm(n_models);
  for (int i = 0; i < n_models; ++i) {
    if (!models[i]) { delete b; return fail(WBC_E_ARG, "wbc_batch_create: model %d is null", i); }
    b->models[i] = models[i];
    dm[i] = models[i]->dev;
    if (models[i]->blob.njoints > b->max_nj) b->max_nj = models[i]->blob.njoints;
    if (models[i]->blob.nframes > b->max_nf) b->max_nf = models[i]->blob.nframes;
    if (models[i]->dev.rot_mask) b->rot = 1;
  }
  // everything allocated so far is released on any failure below (wbc_batch_destroy frees what is non-null)
#define HIP_TRY_B(expr)                                                                                              \
  do {                                                                                                               \
    hipError_t e_ = (expr);                                                                                          \
    if (e_ != hipSuccess) { wbc_batch_destroy(b); return fail(WBC_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); }  \
  } while (0)
  hipDeviceProp_t prop;
  HIP_TRY_B(hipGetDeviceProperties(&prop, device_id));
  const int per_cu = (int)(prop.maxSharedMemoryPerMultiProcessor / (size_t)tick_lds_bytes());
  b->grid = prop.multiProcessorCount * (per_cu < 1 ? 1 : (per_cu > 16 ? 16 : per_cu));
  if (n_models > 0) {   // n_models == 0: a QP-only handle (wbc_qp_solve / wbc_qp_solve_ls)
    HIP_TRY_B(hipMalloc((void**)&b->d_models, sizeof(DevModel) * n_models));
    HIP_TRY_B(hipMalloc((void**)&b->d_cfgs, sizeof(WbcConfig) * n_models));
    HIP_TRY_B(hipMalloc((void**)&b->d_plans, sizeof(DevPlan) * n_models));
    HIP_TRY_B(hipMemset(b->d_plans, 0, sizeof(DevPlan) * n_models));
    HIP_TRY_B(hipMemcpy(b->d_models, dm.data(), sizeof(DevModel) * n_models, hipMemcpyHostToDevice));
  }
#undef HIP_TRY_B
  *out = b;
  return WBC_OK;
}

extern "C" void wbc_batch_destroy(WbcBatch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device_id);
  if (b->d_models) (void)hipFree(b->d_models);
  if (b->d_cfgs) (void)hipFree(b->d_cfgs);
  if (b->d_plans) (void)hipFree(b->d_plans);
  if (b->ws) (void)hipFree(b->ws);
  if (b->d_prof) (void)hipFree(b->d_prof);
  if (b->d_pu) (void)hipFree(b->d_pu);
  if (b->d_pq) (void)hipFree(b->d_pq);
  if (b->d_roll) (void)hipFree(b->d_roll);
  if (b->d_traj) (void)hipFree(b->d_traj);
  if (b->d_slack_lim) (void)hipFree(b->d_slack_lim);
  if (b->d_slack) (void)hipFree(b->d_slack);
  if (b->d_rvjp) (void)hipFree(b->d_rvjp);
  if (b->d_status) (void)hipFree(b->d_status);
  if (b->d_defer) (void)hipFree(b->d_defer);
  if (b->d_dstat) (void)hipFree(b->d_dstat);
  if (b->d_worder) (void)hipFree(b->d_worder);
  delete b;
}

static int rows_task(const WbcConfig& c, int* mcart) {
  int m = 0;
  for (int i = 0; i < WBC_NEE; ++i) m += c.task_ee[i] ? 6 : 0;
  m += c.task_trunk ? 6 : 0;
  m += c.task_com ? 3 : 0;
  *mcart = m;
  return m + (c.task_joint ? WBC_V_STRIDE : 0);
}
static int rows_con(const WbcConfig& c) {
  int p = (c.con_com ? 2 : 0) + (c.con_trunk ? 4 : 0);
  for (int i = 0; i < WBC_NEE; ++i) p += c.con_ee[i] ? 3 : 0;
  return p;
}

static int any_orth_plan(const WbcBatch* b) {
  for (int i = 0; i < b->n_models; ++i) if (b->plan_host[i].orth) return 1;
  return 0;
}

// Which stance feet's contact equalities the tick kernel eliminates structurally (contact_presolve in wbc_common.h).
// Enabled only when (1) every contact foot's rows are supported by the 6 base DoF + 3 own leg DoF, the leg sets disjoint,
// (2) NO active task touches an eliminated leg DoF (then H_ll = d^2 I, H_lf = 0 and the reduction costs no accuracy),
// (3) the reduced problem fits qp_core<16>.
// qpJointb "MANI"/"HYBRID" (Robot_Wrapper4.py:1220-1260) analysed on the tree: DoF i differentiates joint_id with respect to
// q[qi]; that finite difference is exactly zero unless q[qi] belongs to the free-flyer or to a PROPER ancestor of joint_id
// (wbc_posture_kernel makes the same test per sweep). If no sweep matters the tick kernels need no posture kernel at all.
// The sweeps of qpJointb "MANI" / "HYBRID" that matter, for wbc_posture_par_kernel (same loop, same skips, same `matters` test as
// wbc_posture_kernel): one record per sweep, with the configuration entries the reference's loop has left perturbed before it.
static void build_posture_par_plan(const DevModel& M, const WbcConfig& c, DevPlan* P) {
  P->mp_ok = 0; P->mp_n = 0; P->mp_all = 0; P->mp_prevmode = 0;
  const int mode = c.task_joint, literal = c.posture_literal;
  if (mode != WBC_JOINT_MANI && mode != WBC_JOINT_HYBRID) return;
  if (M.njoints > 22 || M.maxdepth > 8) return;
  uint32_t prev = 0, swept = 0;
  int n = 0;
  for (int i = 0; i < M.nv; ++i) {
    int joint_id;
    if (mode == WBC_JOINT_MANI) joint_id = (i < 6) ? 1 : (literal ? i + 1 - 5 : i - 4);
    else { joint_id = i - 6; if (joint_id < c.arm_base_id) continue; }
    if (joint_id >= M.njoints) continue;
    const int qi = literal ? i : ((i < 6) ? i : i + 1);
    swept |= 1u << i;                                            // (a sweep that does not matter still sets u_i = 0.5 (0 - 0) / d = 0)
    int jp = 1;
    for (int j = 2; j < M.njoints; ++j) if (M.idx_q[j] == qi) jp = j;
    const bool matters = (jp == 1) || (jp != joint_id && ((M.col_subtree[M.idx_v_of[jp]] >> joint_id) & 1u));
    if (matters) {
      if (n >= 32) return;
      P->mp_i[n] = i; P->mp_qi[n] = qi; P->mp_joint[n] = joint_id; P->mp_prev[n] = literal ? prev : 0u;
      int chain[8], len = 0;
      for (int j = joint_id; j > 1; j = M.parent[j]) { if (len >= 8) return; chain[len++] = j; }
      for (int k = 0; k < 8; ++k) P->mp_chain[n][k] = (k < len) ? chain[len - 1 - k] : -1;
      ++n;
    }
    if (literal) prev |= 1u << qi;
  }
  P->mp_n = n; P->mp_all = literal ? prev : 0u;
  if (mode == WBC_JOINT_HYBRID) P->mp_prevmode = ((M.nv >= 32) ? 0xFFFFFFFFu : ((1u << M.nv) - 1u)) & ~swept;   // DoF whose u stays the PREV value
  P->mp_ok = 1;
}

static void build_posture_plan(const DevModel& M, const WbcConfig& c, DevPlan* P) {
  const int mode = c.task_joint;
  if (mode != WBC_JOINT_MANI && mode != WBC_JOINT_HYBRID) return;
  build_posture_par_plan(M, c, P);
  const int literal = c.posture_literal;
  uint32_t zero = 0, pert = 0;
  for (int i = 0; i < M.nv; ++i) {
    int joint_id;
    if (mode == WBC_JOINT_MANI) joint_id = (i < 6) ? 1 : i - 4;
    else { joint_id = i - 6; if (joint_id < c.arm_base_id) continue; }
    if (joint_id >= M.njoints) continue;
    const int qi = literal ? i : ((i < 6) ? i : i + 1);
    if (qi < 7) return;                                    // the free-flyer moves everything: the sweeps are needed
    int jp = -1;
    for (int j = 2; j < M.njoints; ++j) if (M.idx_q[j] == qi) jp = j;
    if (jp < 0) return;
    if (jp != joint_id && ((M.col_subtree[M.idx_v_of[jp]] >> joint_id) & 1u)) return;   // a proper ancestor: matters
    zero |= 1u << i;
    if (literal) pert |= 1u << qi;
  }
  if (mode == WBC_JOINT_MANI) return;                      // (MANI starts from u = 0, not PREV; it never gets here anyway: i < 6)
  P->post_static = 1; P->post_zero = zero; P->post_pert = pert;
  // does an active constraint depend on a perturbed joint? (then the second FK pass is needed)
  uint32_t dofs = 0;
  for (int k = 0; k < M.nv; ++k) if ((pert >> M.col_q[k]) & 1u) dofs |= 1u << k;
  bool dep = c.con_com != 0 && dofs != 0;
  if (c.con_trunk && (M.frame_support[WBC_FR_TRUNK] & dofs)) dep = true;
  for (int e = 0; e < WBC_NEE; ++e) if (c.con_ee[e] && (M.frame_support[WBC_FR_EE0 + e] & dofs)) dep = true;
  P->post_fk2 = dep ? 1 : 0;
}

// The packed FK schedule shared by wbc_tick_sim3p_kernel and wbc_update_packed_kernel: the joints of tree depth 2 + L (L < 5) up to need_depth,
// one per lane-in-instance, and the q index of every revolute joint it reaches. Returns false if a level holds more than 16 joints.
static bool build_pk_fk(const DevModel& M, int need_depth, DevPlan* P) {
  for (int i = 0; i < 32; ++i) P->pk_scq[i] = -1;
  for (int L = 0; L < 5; ++L) {
    int cnt = 0;
    for (int i = 0; i < 16; ++i) { memset(&P->pk_fk[L][i], 0, sizeof P->pk_fk[L][i]); P->pk_fk[L][i].joint = -1; }
    for (int j = 2; j < M.njoints; ++j)
      if (M.depth[j] == L + 2 && M.depth[j] <= need_depth) {
        if (cnt < 16) {
          DevPlan::PkJoint& r = P->pk_fk[L][cnt];
          const bool rev = M.jtype[j] >= WBC_JT_RX && M.jtype[j] <= WBC_JT_RZ;
          r.joint = j; r.parent = M.parent[j]; r.a0 = 3 * M.ax0[j]; r.a1 = 3 * M.ax1[j]; r.a2 = 3 * M.ax2[j];
          r.rev = rev ? 1 : 0; r.q_idx = M.idx_q[j]; r.t0 = M.tp[j][0]; r.t1 = M.tp[j][1]; r.t2 = M.tp[j][2]; r.rot = (M.rot_mask >> j) & 1u;
          if (rev && j < 32) P->pk_scq[j] = M.idx_q[j];
        }
        ++cnt;
      }
    if (cnt > 16) return false;
  }
  return true;
}

// Tables the packed orth and the packed box kernels share: the FK schedule over EVERY joint (tree depth 2 + L, L < 6, one joint per
// lane-in-instance), the revolute joints' q indices, body masses / centres, and per DoF its Jacobian column, the EE frames it moves and
// (need_subtree: the CoM Jacobian) the contiguous joint range of its subtree. Returns false if the model does not fit the layout.
static bool build_q_tables(const DevModel& M, DevPlan* P, bool need_subtree) {
  if (M.njoints > 22 || M.maxdepth > 7) return false;
  for (int i = 0; i < 32; ++i) { P->q_scq[i] = -1; memset(&P->q_dof[i], 0, sizeof P->q_dof[i]); P->q_dof[i].bl = P->q_dof[i].red = -1; memset(&P->q_jm[i], 0, sizeof P->q_jm[i]); }
  for (int L = 0; L < 6; ++L) {
    int cnt = 0;
    for (int i = 0; i < 16; ++i) { memset(&P->q_fk[L][i], 0, sizeof P->q_fk[L][i]); P->q_fk[L][i].joint = -1; }
    for (int j = 2; j < M.njoints; ++j)
      if (M.depth[j] == L + 2) {
        if (cnt >= 16) return false;
        DevPlan::PkJoint& r = P->q_fk[L][cnt++];
        const bool rev = M.jtype[j] >= WBC_JT_RX && M.jtype[j] <= WBC_JT_RZ;
        r.joint = j; r.parent = M.parent[j]; r.a0 = 3 * M.ax0[j]; r.a1 = 3 * M.ax1[j]; r.a2 = 3 * M.ax2[j];
        r.rev = rev ? 1 : 0; r.q_idx = M.idx_q[j]; r.t0 = M.tp[j][0]; r.t1 = M.tp[j][1]; r.t2 = M.tp[j][2]; r.rot = (M.rot_mask >> j) & 1u;
        if (rev) P->q_scq[j] = M.idx_q[j];
      }
  }
  for (int j = 1; j < M.njoints; ++j) { P->q_jm[j].m = M.mass[j]; P->q_jm[j].c0 = M.com[j][0]; P->q_jm[j].c1 = M.com[j][1]; P->q_jm[j].c2 = M.com[j][2]; }
  for (int d = 0; d < M.nv; ++d) {
    DevPlan::QDof& r = P->q_dof[d];
    const int j = M.col_joint[d];
    r.joint = j; r.lin = M.col_lin[d]; r.ang = M.col_ang[d];
    const uint32_t sub = M.col_subtree[d];
    int lo = -1, hi = -1, cntj = 0;
    for (int k = 1; k < M.njoints; ++k) if ((sub >> k) & 1u) { if (lo < 0) lo = k; hi = k; ++cntj; }
    if (need_subtree) {
      if (lo < 0 || hi - lo + 1 != cntj) return false;                    // not contiguous
      if (j != 1 && cntj > 8) return false;                               // the kernel's sub-tree loop
    }
    r.sub_lo = lo; r.sub_hi = hi;
    for (int e = 0; e < WBC_NEE; ++e) if ((M.frame_support[WBC_FR_EE0 + e] >> d) & 1u) r.supmask |= 1u << e;
  }
  return true;
}

// The packed orth kernel's plan (wbc_tick_orthp_kernel): equality-only task problems — the only constraints are the eliminated stance
// feet's contact rows (no trunk / CoM box, no velocity box), tasks = any EE tasks + optionally the CoM task + posture Tikhonov / PREV.
static void build_orthp_plan(const DevModel& M, const WbcConfig& c, DevPlan* P) {
  P->q_ok = 0;
  const int nelim = P->nelim, nl = 3 * nelim;
  if (!P->orth || nelim < 1 || nelim > 4) return;
  // INEQ: the kernel's variant with inequality rows (trunk box, CoM box, the velocity box of every DoF — in the reduced coordinates rows of Z) and a
  // trunk task: everything beyond the equality-only family of BASELINE configs[1]
  const bool ineq = c.use_bounds || c.con_trunk || c.con_com || c.task_trunk;
  const bool trunk_is_root = M.frame_joint[WBC_FR_TRUNK] == 1 && M.frame_p[WBC_FR_TRUNK][0] == 0 && M.frame_p[WBC_FR_TRUNK][1] == 0 && M.frame_p[WBC_FR_TRUNK][2] == 0;
  if (ineq && (!c.use_bounds || c.con_ee[4] || ((c.con_trunk || c.task_trunk) && !trunk_is_root) || P->n_red > 12)) return;
  if (P->p_keep != (ineq ? (c.con_com ? 2 : 0) + (c.con_trunk ? 4 : 0) : 0)) return;
  if (c.task_joint != WBC_JOINT_TIKHONOV && c.task_joint != WBC_JOINT_PREV) return;
  if (P->n_red > 15) return;
  uint32_t lockmask = 0;
  if (c.use_bounds) for (int d = c.lock_from; d < M.nv; ++d) if (d >= 6 && P->lidx[d] < 0) lockmask |= 1u << d;
  if (!build_q_tables(M, P, true)) return;
  for (int i = 0; i < 18; ++i) P->q_bl2dof[i] = 0;
  for (int i = 0; i < 16; ++i) P->q_red2dof[i] = 0;
  for (int e = 0; e < 8; ++e) P->q_efoot[e] = -1;
  // DoF records: [base; eliminated legs] positions, reduced (free) variables 6.., subtree = a contiguous joint range (depth-first numbering)
  int nred = 6;
  uint32_t freemask = 0;
  for (int d = 0; d < M.nv; ++d) {
    DevPlan::QDof& r = P->q_dof[d];
    if (d < 6) r.bl = d;
    else if (P->lidx[d] >= 0) r.bl = 6 + P->lidx[d];
    else if ((lockmask >> d) & 1u) { }                              // locked at 0 by the velocity box: its column leaves the problem
    else { if (nred >= 15) return; r.red = nred; P->q_red2dof[nred++] = d; freemask |= 1u << d; }
    if (r.bl >= 0) P->q_bl2dof[r.bl] = d;
    DevPlan::XVar& v = P->q_dmp[d];
    memset(&v, 0, sizeof v);
    v.dof = d; v.dq_idx = c.damper_qidx[d]; v.d_lo = c.damper_lo[d]; v.d_hi = c.damper_hi[d]; v.d_vm = c.damper_vmax[d];
  }
  if (nred != P->n_red) return;
  P->q_nred = nred;
  // EE tasks: support = base + (one eliminated foot's own leg | free variables)
  P->q_armsup = 0;
  uint32_t legall = 0;
  for (int l = 0; l < nl; ++l) legall |= 1u << P->legd[l];
  for (int e = 0; e < WBC_NEE; ++e) {
    if (!c.task_ee[e]) continue;
    const uint32_t sup = M.frame_support[WBC_FR_EE0 + e];
    if (M.depth[M.frame_joint[WBC_FR_EE0 + e]] > 7) return;
    if (sup & freemask) P->q_armsup |= 1u << e;
    const uint32_t legs = sup & legall;
    if (sup & ~(0x3Fu | legall | freemask | lockmask)) return;
    if (legs) {
      int f = -1;
      for (int t = 0; t < nelim; ++t) {
        const uint32_t own = (1u << P->legd[3 * t]) | (1u << P->legd[3 * t + 1]) | (1u << P->legd[3 * t + 2]);
        if (legs == own) f = t;
      }
      if (f < 0) return;
      P->q_efoot[e] = f;
    }
  }
  P->q_ok = ineq ? 2 : 1;
  P->q_nlock = __builtin_popcount(lockmask);
  // roll-outs of these configurations update their state on wbc_update_packed_kernel too: its FK schedule down to the deepest frame the estimator reads
  int need = M.depth[M.frame_joint[WBC_FR_TRUNK]];
  for (int e = 0; e < 5; ++e) if (M.depth[M.frame_joint[WBC_FR_EE0 + e]] > need) need = M.depth[M.frame_joint[WBC_FR_EE0 + e]];
  P->pk_update_ok = (need <= 6 && build_pk_fk(M, need, P)) ? 1 : 0;
}

// The packed box kernel's plan (wbc_tick_boxp_kernel): task problems without a single constraint row (the warm-up problem of setInitialState,
// Robot_Wrapper4.py:196-351): trunk task (trunk frame = the free-flyer's placement) and / or EE tasks + posture Tikhonov / PREV, velocity box on.
// Eliminated: the six base DoF and, if more than 16 bounded DoF remain, those with the widest box (position range x velocity limit of the damper
// entry the DoF looks at): their bounds are checked after the solve, a violation sends the instance to the general path. Every limb DoF must
// move at most ONE active task's frame (the block-arrow structure of H).
static void build_boxp_plan(const DevModel& M, const WbcConfig& c, int prows, DevPlan* P) {
  P->x_ok = 0;
  if (prows != 0 || !c.use_bounds || c.task_com) return;
  if (c.task_joint != WBC_JOINT_TIKHONOV && c.task_joint != WBC_JOINT_PREV) return;
  const bool trunk_is_root = M.frame_joint[WBC_FR_TRUNK] == 1 && M.frame_p[WBC_FR_TRUNK][0] == 0 && M.frame_p[WBC_FR_TRUNK][1] == 0 && M.frame_p[WBC_FR_TRUNK][2] == 0;
  if (c.task_trunk && !trunk_is_root) return;
  if (M.nv > 26 || !build_q_tables(M, P, false)) return;
  for (int d = 0; d < M.nv; ++d) if (M.col_joint[d] == 1 ? d >= 6 : (M.col_q[d] < 0 || M.col_q[d] >= M.nq)) return;   // one free-flyer + 1-DoF joints
  for (int e = 0; e < WBC_NEE; ++e) if (c.task_ee[e] && M.depth[M.frame_joint[WBC_FR_EE0 + e]] > 7) return;
  uint32_t lockmask = 0, tmask = 0;
  for (int d = c.lock_from; d < M.nv; ++d) if (d >= 6) lockmask |= 1u << d;
  for (int e = 0; e < WBC_NEE; ++e) if (c.task_ee[e]) tmask |= 1u << e;
  int freed[32], nfree = 0;
  for (int d = 6; d < M.nv; ++d) {
    if ((lockmask >> d) & 1u) continue;
    if (__builtin_popcount(P->q_dof[d].supmask & tmask) > 1) return;
    freed[nfree++] = d;
  }
  int extra = nfree - 16;
  if (extra > 2) return;
  for (int i = 0; i < 32; ++i) P->x_role[i] = -1;
  for (int i = 0; i < 16; ++i) { memset(&P->x_kept[i], 0, sizeof P->x_kept[i]); P->x_kept[i].task = -1; P->x_limb[i] = 1u << i; }
  for (int i = 0; i < 8; ++i) { memset(&P->x_elim[i], 0, sizeof P->x_elim[i]); P->x_elim[i].task = -1; }
  auto fill = [&](DevPlan::XVar& v, int d) {
    v.dof = d; v.dq_idx = c.damper_qidx[d]; v.d_lo = c.damper_lo[d]; v.d_hi = c.damper_hi[d]; v.d_vm = c.damper_vmax[d];
    const uint32_t tk = P->q_dof[d].supmask & tmask;
    v.task = (d >= 6 && tk) ? __builtin_ctz(tk) : -1;
  };
  int ne = 6;
  for (int d = 0; d < 6; ++d) { P->x_role[d] = d; fill(P->x_elim[d], d); }
  uint32_t elim_extra = 0;
  for (; extra > 0; --extra) {
    int best = -1; double bs = -1.0;
    for (int i = 0; i < nfree; ++i) {
      const int d = freed[i];
      if ((elim_extra >> d) & 1u) continue;
      const double sc = (c.damper_hi[d] - c.damper_lo[d]) * c.damper_vmax[d];
      if (sc > bs) { bs = sc; best = d; }
    }
    if (best < 0) return;
    elim_extra |= 1u << best;
    P->x_role[best] = ne; fill(P->x_elim[ne], best); ++ne;
  }
  int nk = 0;
  for (int i = 0; i < nfree; ++i) {
    const int d = freed[i];
    if ((elim_extra >> d) & 1u) continue;
    P->x_role[d] = 16 + nk; fill(P->x_kept[nk], d); ++nk;
  }
  for (int k = 0; k < nk; ++k)
    for (int k2 = 0; k2 < nk; ++k2)
      if (P->x_kept[k].task >= 0 && P->x_kept[k].task == P->x_kept[k2].task) P->x_limb[k] |= 1u << k2;
  P->x_ne = ne; P->x_nk = nk; P->x_nlock = __builtin_popcount(lockmask);
  P->x_ok = 1;
  // the warm-up roll-out (mode WBC_ROLLOUT_WARMUP) updates its state on wbc_update_packed_kernel too: its FK schedule down to the deepest frame it reads
  int need = M.depth[M.frame_joint[WBC_FR_TRUNK]];
  for (int e = 0; e < 5; ++e) if (M.depth[M.frame_joint[WBC_FR_EE0 + e]] > need) need = M.depth[M.frame_joint[WBC_FR_EE0 + e]];
  P->pk_update_ok = (need <= 6 && build_pk_fk(M, need, P)) ? 1 : 0;
}

static void build_plan(const DevModel& M, const WbcConfig& c, int prows, DevPlan* P) {
  memset(P, 0, sizeof *P);
  // the whole-tree tables for every configured model (wbc_slack_kernel); the orth / box plan builders below refill them with the same entries
  P->slack_ok = build_q_tables(M, P, false) ? 1 : 0;
  build_posture_plan(M, c, P);
  for (int e = 0; e < WBC_NEE; ++e) { if (c.task_ee[e]) P->task_ee_mask |= 1u << e; if (c.con_ee[e]) P->con_ee_mask |= 1u << e; }
  P->flags = (c.con_com ? 1u : 0u) | (c.con_trunk ? 2u : 0u) | (c.task_trunk ? 4u : 0u) | (c.use_bounds ? 8u : 0u) | ((uint32_t)(c.task_joint & 7) << 4);
  for (int i = 0; i < 32; ++i) { P->pos[i] = -1; P->lidx[i] = -1; }
  uint32_t legmask = 0;
  int prow = (c.con_com ? 2 : 0) + (c.con_trunk ? 4 : 0), nelim = 0, l = 0;
  for (int e = 0; e < 4; ++e) {
    if (!c.con_ee[e]) continue;
    const uint32_t sup = M.frame_support[WBC_FR_EE0 + e], legs = sup & ~0x3Fu;
    if ((sup & 0x3Fu) != 0x3Fu || __builtin_popcount(legs) != 3 || (legs & legmask)) return;
    legmask |= legs;
    P->elimrows |= 7u << prow;
    P->rowstart[nelim++] = prow;
    for (int d = 0; d < M.nv; ++d) if ((legs >> d) & 1u) { P->lidx[d] = l; P->legd[l++] = d; }
    prow += 3;
  }
  if (!nelim && c.task_joint) build_boxp_plan(M, c, prows, P);
  if (!nelim || !c.task_joint) return;
  // `clean`: no task touches the stance legs (H_ll = d^2 I, H_lf = 0): the explicit G = -K^-1 B costs no accuracy (contact_presolve,
  // the sim3 kernels). Otherwise the elimination goes through an orthonormal null-space basis (contact_presolve_orth).
  bool clean = !c.task_com;
  for (int e = 0; e < WBC_NEE; ++e) if (c.task_ee[e] && (M.frame_support[WBC_FR_EE0 + e] & legmask)) clean = false;
  if (c.task_trunk && (M.frame_support[WBC_FR_TRUNK] & legmask)) clean = false;
  // DoF the velocity box locks at 0 (lb = ub = 0 from lock_from on, Robot_Wrapper4.py:627-630) are known: they leave the reduced
  // problem altogether (their q̇ is 0, they contribute to nothing else) — which also leaves room in qp_core<16> for the
  // extra unknown a rank-deficient stance-leg block keeps (pivoted elimination in wbc_tick_sim3_kernel)
  uint32_t lockmask = 0;
  if (c.use_bounds) for (int d = c.lock_from; d < M.nv; ++d) if (d >= 6 && !((legmask >> d) & 1u)) lockmask |= 1u << d;
  // (exact whatever rows touch them: a column that multiplies a velocity fixed at 0 contributes to nothing)
  const int nlock = __builtin_popcount(lockmask);
  const int n_red = M.nv - 3 * nelim - nlock, p_keep = prows - 3 * nelim;
  if (n_red > WBC_PLAN_NR || n_red < 6 || p_keep + (c.use_bounds ? 3 * nelim + (clean ? 0 : 6) : 0) > WBC_MAX_P) return;
  int cnt = 0;
  for (int d = 0; d < M.nv; ++d) if (!(((legmask | lockmask) >> d) & 1u)) { P->pos[d] = cnt; P->Fd[cnt++] = d; }
  P->nlock = nlock;
  for (int f = 0; f < M.nframes; ++f)
    for (int d = 0; d < M.nv; ++d)
      if (((M.frame_support[f] >> d) & 1u) && P->pos[d] >= 0) P->redsup[f] |= 1u << P->pos[d];
  // kept rows in findConstraints order: CoM (whole-body support), trunk box (trunk frame), Grip contact
  {
    int r = 0;
    if (c.con_com) { P->legrows |= 3u << r; r += 2; }
    if (c.con_trunk) { if (M.frame_support[WBC_FR_TRUNK] & legmask) P->legrows |= 15u << r; r += 4; }
    for (int e = 0; e < WBC_NEE; ++e) {
      if (!c.con_ee[e]) continue;
      if (!((P->elimrows >> r) & 1u) && (M.frame_support[WBC_FR_EE0 + e] & legmask)) P->legrows |= 7u << r;
      r += 3;
    }
  }
  P->nelim = nelim; P->n_red = n_red; P->p_keep = p_keep;
  if (!clean) { P->orth = 1; build_orthp_plan(M, c, P); return; }
  P->enabled = 1;
  // ---- the packed kernel (wbc_tick_sim3p_kernel) covers the sim3 switch-set family only: Grip task or none, no trunk / CoM
  // task, the kept rows = the trunk box (base support only), velocity bounds on, a posture mode it can form itself, every
  // joint it needs within tree depth 6 and at most 16 joints per level
  // (a trunk task — base support only — runs on the kernel's TRUNK variant)
  const bool trunk_is_root = M.frame_joint[WBC_FR_TRUNK] == 1 && M.frame_p[WBC_FR_TRUNK][0] == 0 && M.frame_p[WBC_FR_TRUNK][1] == 0 && M.frame_p[WBC_FR_TRUNK][2] == 0;
  bool ok = c.use_bounds && !(c.task_trunk && !trunk_is_root) && !c.task_com && !c.con_com && !c.con_ee[4] && p_keep == (c.con_trunk ? 4 : 0) &&
            n_red <= 12 && (P->task_ee_mask & ~16u) == 0 && P->legrows == 0 &&
            true;
  // the posture modes the packed kernel forms itself; any other (MANI / HYBRID with sweeps that matter, CUSTOM) runs on its QCON variant with
  // the posture kernel's (or the caller's) posture_u / q_con — without the trunk task
  const bool own_mode = c.task_joint == WBC_JOINT_TIKHONOV || c.task_joint == WBC_JOINT_PREV ||
                        (c.task_joint >= WBC_JOINT_MANI && c.task_joint <= WBC_JOINT_HYBRID && P->post_static && !P->post_fk2);
  int need_depth = 0;
  for (int k = 0; k < n_red; ++k) if (M.depth[M.col_joint[P->Fd[k]]] > need_depth) need_depth = M.depth[M.col_joint[P->Fd[k]]];
  for (int l = 0; l < 3 * nelim; ++l) if (M.depth[M.col_joint[P->legd[l]]] > need_depth) need_depth = M.depth[M.col_joint[P->legd[l]]];
  if (M.depth[M.frame_joint[WBC_FR_EE0 + 4]] > need_depth) need_depth = M.depth[M.frame_joint[WBC_FR_EE0 + 4]];
  if (need_depth > 6) ok = false;
  for (int i = 0; i < 32; ++i) P->pk_scq[i] = -1;
  if (ok && !build_pk_fk(M, need_depth, P)) ok = false;
  for (int i = 0; i < 16; ++i) {
    memset(&P->pk_var[i], 0, sizeof P->pk_var[i]);
    memset(&P->pk_leg[i], 0, sizeof P->pk_leg[i]);
    for (int pass = 0; pass < 2; ++pass) {
      DevPlan::PkCol& r = pass ? P->pk_leg[i] : P->pk_var[i];
      const bool on = pass ? (i < 3 * nelim) : (i < n_red);
      const int d = on ? (pass ? P->legd[i] : P->Fd[i]) : 0;
      r.dof = d; r.joint = M.col_joint[d]; r.lin = M.col_lin[d]; r.ang = M.col_ang[d];
      r.dq_idx = c.damper_qidx[d]; r.d_lo = c.damper_lo[d]; r.d_hi = c.damper_hi[d]; r.d_vm = c.damper_vmax[d];
    }
  }
  P->packed_ok = (ok && own_mode) ? 1 : 0;
  P->packed_ok_pu = (ok && !c.task_trunk) ? 1 : 0;
  bool upd = ok;   // (any posture mode: the state update does not depend on it; the trunk reference state is advanced too since round 3)
  for (int e = 0; e < 5; ++e) if (M.depth[M.frame_joint[WBC_FR_EE0 + e]] > need_depth) upd = false;
  if (M.depth[M.frame_joint[WBC_FR_TRUNK]] > need_depth) upd = false;
  P->pk_update_ok = upd ? 1 : 0;
}

extern "C" int wbc_batch_configure(WbcBatch* b, int mi, const WbcConfig* cfg) {
  if (!b || !cfg || mi < 0 || mi >= b->n_models) return fail(WBC_E_ARG, "wbc_batch_configure: bad arguments");
  const int nv = b->models[mi]->blob.nv, nq = b->models[mi]->blob.nq;
  if (cfg->task_joint < 0 || cfg->task_joint > WBC_JOINT_CUSTOM) return fail(WBC_E_ARG, "unknown posture mode %d", cfg->task_joint);
  if (cfg->task_joint == WBC_JOINT_HYBRID && (cfg->arm_base_id < 1 || cfg->arm_base_id >= b->models[mi]->blob.njoints))
    return fail(WBC_E_ARG, "HYBRID posture: arm_base_id %d is not a joint of the model", cfg->arm_base_id);
  if (!cfg->task_joint) return fail(WBC_E_UNSUPPORTED, "the posture task must be on: without it H = J'J is singular (Robot_Wrapper4.py:1199-1206)");
  for (int i = 0; i < nv; ++i)
    if (cfg->use_bounds && (cfg->damper_qidx[i] < 0 || cfg->damper_qidx[i] >= nq)) return fail(WBC_E_ARG, "damper_qidx[%d] = %d out of range", i, cfg->damper_qidx[i]);
  int mcart = 0;
  const int m = rows_task(*cfg, &mcart), p = rows_con(*cfg);
  if (p > WBC_MAX_P) return fail(WBC_E_ARG, "too many constraint rows (%d)", p);
  // (all models of a batch must share the task / constraint switches; that is checked when the batch is USED, so that a
  //  configured multi-model batch can be moved to another switch set one model at a time — same_switches below)
  HIP_TRY(hipSetDevice(b->device_id));
  // The copies below go through the null stream, which is not ordered against a non-blocking caller stream (torch's side streams are): a
  // device-mode call still in flight there would read the new configuration from some tick on. The call is rare and blocks the host anyway:
  // wait for the device first (include/wbc.h states this as the contract).
  HIP_TRY(hipDeviceSynchronize());
  b->cfg_host[mi] = *cfg;
  b->configured[mi] = true;
  b->plan_host[mi] = DevPlan();
  b->mrows = m; b->prows = p; b->mcart = mcart;
  HIP_TRY(hipMemcpy(b->d_cfgs + mi, cfg, sizeof *cfg, hipMemcpyHostToDevice));
  DevPlan plan;
  build_plan(b->models[mi]->dev, *cfg, p, &plan);
  b->plan_host[mi] = plan;
  b->fixd_dims[mi] = b->models[mi]->dev.nv == SIM3P_FIXD_NV && b->models[mi]->dev.nq == SIM3P_FIXD_NQ && plan.n_red == SIM3P_FIXD_N && plan.nelim == SIM3P_FIXD_NELIM && plan.p_keep == SIM3P_FIXD_PKEEP;
  HIP_TRY(hipMemcpy(b->d_plans + mi, &plan, sizeof plan, hipMemcpyHostToDevice));
  b->worder_reset = 1;                     // the next packed tick runs in the identity order (cleared on that tick's stream)
  return WBC_OK;
}

extern "C" int wbc_task_rows(const WbcBatch* b) { return b ? b->mrows : WBC_E_ARG; }
extern "C" int wbc_constraint_rows(const WbcBatch* b) { return b ? b->prows : WBC_E_ARG; }

extern "C" int wbc_batch_set_option(WbcBatch* b, const char* name, int value) {
  if (!b || !name) return fail(WBC_E_ARG, "wbc_batch_set_option: null");
  if (!strcmp(name, "jtj_mfma")) { b->jtj_mfma = value < 0 ? -1 : (value ? 1 : 0); return WBC_OK; }
  if (!strcmp(name, "presolve")) { b->presolve = value; return WBC_OK; }
  if (!strcmp(name, "presolve_orth")) { b->presolve_orth = value; return WBC_OK; }
  if (!strcmp(name, "orth_qr")) { b->orth_qr = value; return WBC_OK; }
  if (!strcmp(name, "packed_update")) { b->packed_update = value; return WBC_OK; }
  if (!strcmp(name, "presolve_tol_exp")) { double t = 1.0; for (int i = 0; i < value; ++i) t *= 0.1; b->sing_tol = t; return WBC_OK; }
  if (!strcmp(name, "sim3_kernel")) { b->sim3_kernel = value; return WBC_OK; }
  if (!strcmp(name, "packed_kernel")) { b->packed_kernel = value; return WBC_OK; }
  if (!strcmp(name, "wave_order")) { b->wave_order = value < 0 ? 0 : (value > 2 ? 2 : value); return WBC_OK; }
  if (!strcmp(name, "sim3p_fixd")) { b->sim3p_fixd = value != 0; return WBC_OK; }
  if (!strcmp(name, "packed_min_batch")) { b->packed_min_batch = value < 1 ? 1 : value; return WBC_OK; }
  if (!strcmp(name, "packed_orth")) { b->packed_orth = value; return WBC_OK; }
  if (!strcmp(name, "packed_box")) { b->packed_box = value; return WBC_OK; }
  if (!strcmp(name, "posture_par")) { b->posture_par = value; return WBC_OK; }
  if (!strcmp(name, "dbg_alias_inputs")) { b->dbg_alias = value; return WBC_OK; }
  if (!strcmp(name, "warm_start")) { b->warm_start = value != 0; return WBC_OK; }
  if (!strcmp(name, "refine")) { b->refine = value > 0; return WBC_OK; }
  if (!strcmp(name, "count_pivoted")) { b->count_pivoted = value != 0; return WBC_OK; }
  if (!strcmp(name, "dbg_force_defer")) { b->force_defer = value != 0; return WBC_OK; }
  if (!strcmp(name, "dbg_stop")) {
#ifdef WBC_ABLATE
    b->dbg_stop = value; return WBC_OK;
#else
    return value == 0 ? WBC_OK : fail(WBC_E_UNSUPPORTED, "dbg_stop needs the ablation build of the library (make -C csrc ablate; WBC_HIP_LIB=.../libwbc_hip_ablate.so)");
#endif
  }
  if (!strcmp(name, "grid")) { if (value < 1) return fail(WBC_E_ARG, "grid must be >= 1"); b->grid = value; return WBC_OK; }
  return fail(WBC_E_ARG, "unknown option %s", name);
}

extern "C" int wbc_batch_get_stat(WbcBatch* b, const char* name, void* stream, int64_t* out) {
  if (!b || !name || !out) return fail(WBC_E_ARG, "wbc_batch_get_stat: null");
  HIP_TRY(hipSetDevice(b->device_id));
  if (!strcmp(name, "last_path")) { *out = b->last_path; return WBC_OK; }
  if (!strcmp(name, "last_qp_path")) { *out = b->last_qp_path; return WBC_OK; }
  if (!strcmp(name, "last_tick_variant")) { *out = b->last_tick_variant; return WBC_OK; }
  if (!strcmp(name, "last_tick_fixd")) { *out = b->last_path == TICK_SIM3P ? b->last_tick_fixd : 0; return WBC_OK; }
  if (!strcmp(name, "last_qp_variant")) { *out = b->last_qp_variant; return WBC_OK; }
  if (!strcmp(name, "last_grad_variant")) { *out = b->last_grad_variant; return WBC_OK; }
  if (!strcmp(name, "last_gradq_variant")) { *out = b->last_gradq_variant; return WBC_OK; }
  if (!strcmp(name, "last_stepvjp_variant")) { *out = b->last_stepvjp_variant; return WBC_OK; }
  if (!strcmp(name, "last_rollvjp_variant")) { *out = b->last_rollvjp_variant; return WBC_OK; }
  if (!strcmp(name, "last_trackvjp_variant")) { *out = b->last_trackvjp_variant; return WBC_OK; }
  if (!strcmp(name, "last_scorevjp_variant")) { *out = b->last_scorevjp_variant; return WBC_OK; }
  if (!strcmp(name, "last_slackvjp_variant")) { *out = b->last_slackvjp_variant; return WBC_OK; }
  if (!strcmp(name, "last_update_packed")) { *out = b->last_update_packed; return WBC_OK; }
  if (!strcmp(name, "last_posture_par")) { *out = b->last_posture_par; return WBC_OK; }
  if (!strcmp(name, "last_orth")) { *out = (b->last_path == TICK_GENERAL || b->last_path == TICK_ORTHP) ? b->last_orth : 0; return WBC_OK; }
  if (!strcmp(name, "deferred_last")) {      // waits for `stream`
    *out = 0;
    if (b->last_path >= TICK_SIM3P) {       // packed kernels: instances the tail redid on the general path in the last launch
      if (!b->d_dstat) return WBC_OK;
      unsigned long long v = 0;
      HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      HIP_TRY(hipMemcpy(&v, b->d_dstat, sizeof v, hipMemcpyDeviceToHost));
      *out = ((uint32_t)(v >> 32) == b->tick_seq) ? (int64_t)(v & 0xFFFFFFFFull) : 0;
      return WBC_OK;
    }
    if (!b->d_defer || b->last_path == TICK_GENERAL) return WBC_OK;
    int32_t c = 0;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(&c, defer_tail(b) + DEFER_TAIL_LAST, sizeof c, hipMemcpyDeviceToHost));
    *out = c;
    return WBC_OK;
  }
  if (!strcmp(name, "pivoted_last")) {       // needs option "count_pivoted"; waits for `stream`
    *out = 0;
    if (!b->d_defer || b->last_path == TICK_GENERAL || !b->count_pivoted) return WBC_OK;
    int32_t c = 0;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(&c, defer_tail(b), sizeof c, hipMemcpyDeviceToHost));
    *out = c;
    return WBC_OK;
  }
  if (!strcmp(name, "wave_order_slices")) {  // slices whose published order the next launch of the last packed sim3 batch size reads; waits for `stream`
    *out = 0;
    if (!b->d_worder || !b->worder_B || b->last_path != TICK_SIM3P) return WBC_OK;
    std::vector<WaveOrder> sl(WO_NS);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(sl.data(), b->d_worder, WO_NS * sizeof(WaveOrder), hipMemcpyDeviceToHost));
    for (const WaveOrder& w : sl) *out += w.B == (uint32_t)b->worder_B;
    return WBC_OK;
  }
  if (!strcmp(name, "last_traj_bad_rows")) {  // bad rows of the last wbc_rollout_traj / wbc_rollout_tracks; waits for `stream`
    *out = 0;
    if (!b->d_traj) return WBC_OK;
    int32_t c = 0;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(&c, TrajWs::carve(b->d_traj, (size_t)b->max_batch).bad_count, sizeof c, hipMemcpyDeviceToHost));
    *out = c;
    return WBC_OK;
  }
  if (!strcmp(name, "sim3_lds_bytes")) { *out = sim3_lds_bytes(); return WBC_OK; }
  if (!strcmp(name, "orthp_lds_bytes")) { *out = orthp_lds_bytes(); return WBC_OK; }
  if (!strcmp(name, "tick_lds_bytes")) { *out = tick_lds_bytes(); return WBC_OK; }
  return fail(WBC_E_ARG, "unknown statistic %s", name);
}

extern "C" int wbc_batch_synchronize(WbcBatch* b, void* stream) {
  if (!b) return fail(WBC_E_ARG, "null batch");
  HIP_TRY(hipSetDevice(b->device_id));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return WBC_OK;
}

// ---------------------------------------------------------------------------------------------- staging
// mem == WBC_MEM_HOST: inputs are copied into the batch workspace, outputs copied back after the launch.
// mem == WBC_MEM_DEVICE: pointers pass through untouched (no copies, no synchronisation).
struct Stager {
  WbcBatch* b; int mem; hipStream_t s;
  struct Item { void** slot; const void* host; size_t bytes; bool out; };
  std::vector<Item> items;
  template <class T> void in(const T** slot, size_t count) { add((void**)slot, count * sizeof(T), false); }
  template <class T> void out(T** slot, size_t count) { add((void**)slot, count * sizeof(T), true); }
  void add(void** slot, size_t bytes, bool is_out) {
    if (mem == WBC_MEM_DEVICE || !*slot || !bytes) return;
    items.push_back({slot, *slot, bytes, is_out});
  }
  int stage() {
    if (mem == WBC_MEM_DEVICE) return WBC_OK;
    size_t total = 0;
    for (auto& it : items) total += (it.bytes + 255) & ~(size_t)255;
    if (total > b->ws_bytes) {
      if (b->ws) HIP_TRY(hipFree(b->ws));
      b->ws = nullptr; b->ws_bytes = 0;
      HIP_TRY(hipMalloc(&b->ws, total));
      b->ws_bytes = total;
    }
    size_t off = 0;
    for (auto& it : items) {
      void* d = (char*)b->ws + off;
      off += (it.bytes + 255) & ~(size_t)255;
      if (!it.out) HIP_TRY(hipMemcpyAsync(d, it.host, it.bytes, hipMemcpyHostToDevice, s));
      *it.slot = d;
    }
    return WBC_OK;
  }
  int finish() {
    if (mem == WBC_MEM_DEVICE) return WBC_OK;
    for (auto& it : items)
      if (it.out) HIP_TRY(hipMemcpyAsync((void*)it.host, *it.slot, it.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return WBC_OK;
  }
};

// the switches that fix the row layout of A, C and which inputs a tick reads: identical for every model of a batch
static bool same_switches(const WbcConfig& a, const WbcConfig& c) {
  for (int i = 0; i < WBC_NEE; ++i)
    if ((a.task_ee[i] != 0) != (c.task_ee[i] != 0) || (a.con_ee[i] != 0) != (c.con_ee[i] != 0)) return false;
  return (a.task_trunk != 0) == (c.task_trunk != 0) && (a.task_com != 0) == (c.task_com != 0) &&
         (a.con_com != 0) == (c.con_com != 0) && (a.con_trunk != 0) == (c.con_trunk != 0) &&
         (a.use_bounds != 0) == (c.use_bounds != 0) && (a.task_joint != 0) == (c.task_joint != 0);
}
static int check_batch(WbcBatch* b, int B, const char* who, bool need_cfg, bool need_model = true) {
  if (!b) return fail(WBC_E_ARG, "%s: null batch", who);
  if (need_model && b->n_models < 1) return fail(WBC_E_STATE, "%s: this handle was created without a model", who);
  if (B < 1 || B > b->max_batch) return fail(WBC_E_ARG, "%s: B = %d outside [1, max_batch = %d]", who, B, b->max_batch);
  if (need_cfg) {
    for (int i = 0; i < b->n_models; ++i)
      if (!b->configured[i]) return fail(WBC_E_STATE, "%s: model %d has no configuration (wbc_batch_configure)", who, i);
    for (int i = 1; i < b->n_models; ++i)
      if (!same_switches(b->cfg_host[0], b->cfg_host[i]))
        return fail(WBC_E_STATE, "%s: all models of a batch must share the task/constraint switches (model %d differs from model 0)", who, i);
  }
  return WBC_OK;
}
static int grid_for(const WbcBatch* b, int B) { return B < b->grid ? B : b->grid; }   // persistent kernels (QP, integrate)
static int grid_tick(const WbcBatch*, int B) { return B; }                           // tick kernels: one instance per workgroup

static void stage_tick_in(Stager& st, WbcTickIn& in, int B, const WbcBatch* b) {
  const size_t n = (size_t)B;
  st.in(&in.q, n * WBC_Q_STRIDE);
  st.in(&in.ee_target, n * 15); st.in(&in.prev_ee_target, n * 15);
  st.in(&in.trunk_target, n * 3); st.in(&in.prev_trunk_target, n * 3);
  st.in(&in.trunk_box_center, n * 4);
  st.in(&in.ee_ref_rot, n * 45); st.in(&in.ee_prev_rot, n * 45);
  st.in(&in.trunk_ref_euler, n * 3); st.in(&in.trunk_prev_rot, n * 9);
  st.in(&in.com_target, n * 3); st.in(&in.com_target_vel, n * 3);
  st.in(&in.model_id, n);
  st.in(&in.posture_u, n * WBC_V_STRIDE); st.in(&in.q_con, n * WBC_Q_STRIDE);
  st.in(&in.working_set, n * 2);
  (void)b;
}

static int validate_tick_in(const WbcBatch* b, const WbcTickIn* in, const char* who) {
  const WbcConfig& c = b->cfg_host[0];
  if (!in || !in->q) return fail(WBC_E_ARG, "%s: q is required", who);
  bool any_ee = false;
  for (int i = 0; i < WBC_NEE; ++i) any_ee |= c.task_ee[i] != 0;
  if (any_ee && (!in->ee_target || !in->prev_ee_target)) return fail(WBC_E_ARG, "%s: EE tasks need ee_target and prev_ee_target", who);
  if ((in->ee_ref_rot != nullptr) != (in->ee_prev_rot != nullptr)) return fail(WBC_E_ARG, "%s: ee_ref_rot and ee_prev_rot go together", who);
  if (c.task_trunk && (!in->trunk_target || !in->prev_trunk_target || !in->trunk_ref_euler || !in->trunk_prev_rot))
    return fail(WBC_E_ARG, "%s: the trunk task needs trunk_target, prev_trunk_target, trunk_ref_euler, trunk_prev_rot", who);
  if (c.con_trunk && !in->trunk_box_center) return fail(WBC_E_ARG, "%s: the trunk constraint needs trunk_box_center", who);
  if (c.task_com && (!in->com_target || !in->com_target_vel)) return fail(WBC_E_ARG, "%s: the CoM task needs com_target and com_target_vel", who);
  if (b->n_models > 1 && !in->model_id) return fail(WBC_E_ARG, "%s: model_id is required with %d models", who, b->n_models);
  for (int i = 0; i < b->n_models; ++i)
    if (b->cfg_host[i].task_joint == WBC_JOINT_CUSTOM && !in->posture_u) return fail(WBC_E_ARG, "%s: posture mode CUSTOM needs posture_u", who);
  return WBC_OK;
}

// qpJointb "MANI" / "HYBRID" (Robot_Wrapper4.py:1220-1260) ahead of the tick kernel: fills a.in.posture_u (and a.in.q_con
// in literal mode) from the device-resident q unless the caller supplied them. Pointers in `a` are device pointers here.
static int run_posture(WbcBatch* b, int B, const double* q, const int32_t* model_id, double* u, double* q_after, void* stream) {
  PostureArgs pa;
  memset(&pa, 0, sizeof pa);
  pa.models = b->d_models; pa.cfgs = b->d_cfgs; pa.plans = b->d_plans; pa.B = B; pa.n_models = b->n_models; pa.q = q; pa.model_id = model_id; pa.u = u; pa.q_after = q_after; pa.rot = b->rot;
  bool par = b->posture_par != 0;
  for (int i = 0; i < b->n_models && par; ++i) par = b->configured[i] && b->plan_host[i].mp_ok != 0;
  bool three = par && b->posture_par != 3;                 // three instances per wavefront where every model has at most 21 sweeps (option value 3: one per wavefront)
  for (int i = 0; i < b->n_models && three; ++i) three = b->plan_host[i].mp_n <= 21;
  b->last_posture_par = par ? (three ? 2 : 1) : 0;
  if (int e = par ? launch_posture_par(pa, B, stream, three) : launch_posture(pa, B, stream)) return fail(WBC_E_HIP, "posture kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  return WBC_OK;
}
static int auto_posture(WbcBatch* b, KernelArgs& a, int B, void* stream) {
  bool need = false, literal = false;
  for (int i = 0; i < b->n_models; ++i) {
    const int tj = b->cfg_host[i].task_joint;
    if (tj == WBC_JOINT_MANI || tj == WBC_JOINT_HYBRID) { need = true; literal |= b->cfg_host[i].posture_literal != 0; }
  }
  if (!need || a.in.posture_u) return WBC_OK;
  if (b->presolve) {   // every sweep structurally zero on every model: the tick derives u and the leaked state itself
    bool all_static = true;
    for (int i = 0; i < b->n_models; ++i) {
      const int tj = b->cfg_host[i].task_joint;
      if ((tj == WBC_JOINT_MANI || tj == WBC_JOINT_HYBRID) && !b->plan_host[i].post_static) all_static = false;
      if (tj != WBC_JOINT_MANI && tj != WBC_JOINT_HYBRID && tj >= WBC_JOINT_MANI) all_static = false;
    }
    if (all_static && !a.in.q_con) { a.post_static = 1; return WBC_OK; }
  }
  int rc;
  if ((rc = ensure(b->d_pu, sizeof(double) * WBC_V_STRIDE * (size_t)b->max_batch)) || (rc = ensure(b->d_pq, sizeof(double) * WBC_Q_STRIDE * (size_t)b->max_batch))) return rc;
  if ((rc = run_posture(b, B, a.in.q, a.in.model_id, b->d_pu, b->d_pq, stream))) return rc;
  a.in.posture_u = b->d_pu;
  if (literal && !a.in.q_con) a.in.q_con = b->d_pq;
  return WBC_OK;
}

static void fill_args(KernelArgs& a, const WbcBatch* b, int B, double dt) {
  memset(&a, 0, sizeof a);
  a.models = b->d_models; a.cfgs = b->d_cfgs; a.plans = b->d_plans; a.n_models = b->n_models; a.rot = b->rot;
  // J'J on the matrix cores: forced (1), off (0) or, by default (-1), for wide Cartesian stacks only — measured on MI355X
  // (profiles/r02_mfma_evidence.txt): +9 % ticks/s at 33 and 45 Cartesian rows (config 2, "everything"), a wash at 6 (config 3)
  a.B = B; a.mrows = b->mrows; a.prows = b->prows; a.mcart = b->mcart; a.jtj_mfma = b->jtj_mfma < 0 ? (b->mcart >= WBC_MFMA_AUTO_ROWS) : b->jtj_mfma; a.presolve = b->presolve; a.presolve_orth = b->presolve_orth ? 1 + any_orth_plan(b) : 0; a.orth_qr = b->orth_qr; a.refine = b->refine; a.sing_tol = b->sing_tol; a.dbg_alias = b->dbg_alias; a.dt = dt;
  a.prof = b->d_prof; a.dbg_stop = b->dbg_stop;
  a.fk_nj = b->max_nj; a.fk_nf = b->max_nf;
}

// What a launcher (wbc_k_*.hip) returned (0, a hipError_t, or WBC_E_UNSUPPORTED: its variant table holds no kernel for the call's flags) -> ours
static int launch_rc(int e, const char* what) {
  if (e == WBC_E_UNSUPPORTED) return fail(e, "%s kernel: no variant of it is built for this combination of inputs", what);
  return e ? fail(WBC_E_HIP, "%s kernel launch failed: %s", what, hipGetErrorString((hipError_t)e)) : WBC_OK;
}
static int launch_update_auto(WbcBatch* b, UpdateArgs& u, int B, void* stream) {   // the state update of wbc_update / wbc_rollout: four instances per wavefront where every plan allows it
  bool packed = b->packed_update != 0;
  for (int i = 0; i < b->n_models && packed; ++i) packed = b->configured[i] && b->plan_host[i].pk_update_ok != 0;
  u.plans = b->d_plans;
  b->last_update_packed = packed;
  return packed ? launch_update_packed(u, stream) : launch_update(u, B, stream);
}
// ---- The fused tick (wbc_tick, every tick of wbc_rollout): launch_tick_auto selects one of the five paths (select_tick_path: no side effects),
// records it for the statistics, prepares what that path's kernels read and nothing else (prepare_tick), and launches. `a` holds device pointers.
static bool packed_eligible(const WbcBatch* b, const KernelArgs& a) {
  const bool qcon = a.in.q_con || a.in.posture_u;     // the QCON variant (second kinematics pass at q_con, posture target from posture_u)
  bool packed = b->packed_kernel && a.B >= b->packed_min_batch &&
                !b->count_pivoted && !(b->dbg_stop > 0 && b->dbg_stop < 100) && !b->dbg_alias;   // (dbg_stop 101.. cuts the packed kernel)
  for (int i = 0; i < b->n_models && packed; ++i) packed = qcon ? (b->plan_host[i].packed_ok_pu != 0) : (b->plan_host[i].packed_ok != 0);
  return packed;
}
static bool sim3_eligible(const WbcBatch* b, const KernelArgs& a) {   // the sim3 switch-set family (compact LDS, reduced QP only): every plan enabled, the problem fits the layout
  if (!b->sim3_kernel || !b->presolve || b->n_models < 1) return false;
  if (b->jtj_mfma > 0) return false;   // forced: the compact kernel has no matrix-core contraction, the option selects the general kernel
  if (a.in.com_target || a.in.com_target_vel) return false;
  if (b->prows > WBC_SIM3_MAXP || b->mcart > 12) return false;
  for (int i = 0; i < b->n_models; ++i) {
    const DevPlan& P = b->plan_host[i];
    if (!P.enabled || P.p_keep + (b->cfg_host[i].use_bounds ? 3 * P.nelim : 0) > WBC_SIM3_MAXP) return false;
  }
  return true;
}
// the packed orth kernel: every plan q_ok, nothing passed that it does not read (caller's posture target / constraint state; working sets are accepted: no inequality to seed, an empty set out),
// the orthonormal presolve on, no forced matrix-core contraction (the EE tasks' orientation references are honoured)
// packed_orth: 1 (default) from WBC_ORTHP_MIN_BATCH instances on — below that a launch is a single round of waves and the one-instance
// kernel's shorter dependent chain wins (measured on MI355X, tools/debug_orthp.py: 25 us vs 55 us at B = 1024, equal at 4096, 0.075 vs
// 0.108 ms at 8192, 0.318 vs 0.782 ms at 65536); 2: always (tests)
constexpr int WBC_ORTHP_MIN_BATCH = 4608;
static bool orthp_eligible(const WbcBatch* b, const KernelArgs& a) {
  if (b->packed_orth == 1 && a.B < WBC_ORTHP_MIN_BATCH) return false;
  if (!b->packed_orth || !b->packed_kernel || !b->presolve || !b->presolve_orth || b->n_models < 1 || b->jtj_mfma > 0) return false;
  if (a.in.q_con || a.in.posture_u || b->dbg_alias || (b->dbg_stop > 0 && b->dbg_stop < 200)) return false;   // (dbg_stop 201.. cuts this kernel; working sets: nothing to seed, an empty set out)
  for (int i = 0; i < b->n_models; ++i) if (!b->plan_host[i].q_ok || b->plan_host[i].q_ok != b->plan_host[0].q_ok) return false;
  return true;
}
// the packed box kernel: every plan x_ok, nothing passed that it does not read; packed_box: 1 (default) from WBC_BOXP_MIN_BATCH instances on, 2: always.
// Unlike the packed orth kernel it wins at every batch size (measured on MI355X, tools/small_batch_boxp.py: 28.1 vs 29.3 us at B = 1, 39.9 vs 46.4 us
// at 1024, 46 vs 104 us at 4096): the one-instance kernel's chain through a 23-wide Cholesky and ~5 working-set changes is the longer one.
constexpr int WBC_BOXP_MIN_BATCH = 1;
static bool boxp_eligible(const WbcBatch* b, const KernelArgs& a) {
  if (b->packed_box == 1 && a.B < WBC_BOXP_MIN_BATCH) return false;
  if (!b->packed_box || !b->packed_kernel || !b->presolve || b->n_models < 1 || b->jtj_mfma > 0 || b->prows != 0) return false;
  if (a.in.q_con || a.in.posture_u || b->dbg_alias || (b->dbg_stop > 0 && b->dbg_stop < 300)) return false;   // (dbg_stop 301.. cuts this kernel; working sets: its WARM variant)
  for (int i = 0; i < b->n_models; ++i) if (!b->plan_host[i].x_ok) return false;
  return true;
}
static TickPath select_tick_path(const WbcBatch* b, const KernelArgs& a, const WbcTaskParams* tp) {
  if (boxp_eligible(b, a)) return TICK_BOXP;
  if (orthp_eligible(b, a)) return TICK_ORTHP;
  if (!sim3_eligible(b, a)) return TICK_GENERAL;
  if (packed_eligible(b, a)) return TICK_SIM3P;
  // What the packed kernel does not take runs on the one-instance compact kernel, unless the call asks for what that kernel does not have. Orientation
  // references: the packed kernel honours the gripper's, the compact kernel none. The refinement (default on): the compact kernel lives on 168 VGPRs /
  // 13.2 KB LDS (3 waves per SIMD) and has room neither for the task image nor for the Jacobian columns the residual is formed from; the general kernel's
  // structural presolve solves the same reduced problem and refines it (refine = 0 brings the compact kernel back). Per-instance weights: it has no TP variant.
  if (a.in.ee_ref_rot || b->refine > 0 || tp) return TICK_GENERAL;
  return TICK_SIM3;
}

// What the kernels of `path` read, and nothing else. Paths 1-4: a status buffer when the caller passed none. The packed kernels (2-4): the word of
// the "deferred_last" statistic (the instances a packed kernel's tail redid) and this launch's sequence number (0 is the cleared word's).
static int prepare_tick(WbcBatch* b, KernelArgs& a, void* stream, TickPath path) {
  if (path != TICK_GENERAL && !a.out.status) {
    if (int rc = ensure(b->d_status, sizeof(int32_t) * (size_t)b->max_batch)) return rc;
    a.out.status = b->d_status;
  }
  if (path >= TICK_SIM3P) {
    if (!b->d_dstat) {
      HIP_TRY(hipMalloc((void**)&b->d_dstat, sizeof(unsigned long long)));
      HIP_TRY(hipMemsetAsync(b->d_dstat, 0, sizeof(unsigned long long), (hipStream_t)stream));
    }
    a.defer_stat = b->d_dstat;
    a.tick_seq = ++b->tick_seq;
    if (!b->tick_seq) a.tick_seq = ++b->tick_seq;
  }
  if (path == TICK_SIM3 || path == TICK_SIM3P) a.dbg_force_defer = b->force_defer;
  if (path == TICK_SIM3) {    // the list of the instances the compact kernel leaves to the deferred pass, the pivot counter
    if (!b->d_defer) {
      HIP_TRY(hipMalloc((void**)&b->d_defer, defer_bytes(b)));
      HIP_TRY(hipMemsetAsync(b->d_defer, 0, defer_bytes(b), (hipStream_t)stream));   // (on the CALL's stream: a null-stream memset is not ordered against a non-blocking caller stream)
    }
    a.defer = b->d_defer;                                  // (count = 0 here: wbc_tick_deferred_kernel leaves the list empty behind it)
    a.defer_aux = defer_tail(b);
    if (b->count_pivoted) {
      a.pivot_count = defer_tail(b);
      HIP_TRY(hipMemsetAsync(a.pivot_count, 0, sizeof(int32_t), (hipStream_t)stream));
    }
  }
  if (path == TICK_SIM3P) {   // the trunk task's variant, the wave order
    a.packed_trunk = b->cfg_host[0].task_trunk != 0;
    if ((b->wave_order == 2 || (b->wave_order == 1 && a.B >= WBC_WAVE_ORDER_MIN_BATCH)) && !b->dbg_stop) {   // (an ablation cut returns before the kernel records its instances; batches above 130048: identity)
      if (!b->d_worder) {
        const size_t bytes = wave_order_bytes(b->max_batch);
        if (bytes) {
          HIP_TRY(hipMalloc((void**)&b->d_worder, bytes));
          b->worder_reset = 1;
        }
      }
      if (b->d_worder && b->worder_reset) {   // (on the CALL's stream: ordered after any tick still running on it)
        HIP_TRY(hipMemsetAsync(b->d_worder, 0, WO_NS * sizeof(WaveOrder), (hipStream_t)stream));
        b->worder_reset = 0;
      }
      a.worder = b->d_worder;
    }
    b->worder_B = a.worder ? a.B : 0;
  }
  return WBC_OK;
}
static int launch_tick_auto(WbcBatch* b, KernelArgs& a, int B, void* stream, const WbcTaskParams* tp = nullptr) {
  const TickPath path = select_tick_path(b, a, tp);
  b->last_path = path;
  if (path == TICK_GENERAL) b->last_orth = a.presolve && a.presolve_orth == 2 && !(a.ws_in || a.ws_out);
  else if (path >= TICK_ORTHP) b->last_orth = path == TICK_ORTHP;
  int rc = prepare_tick(b, a, stream, path);
  if (rc) return rc;
  switch (path) {   // (the packed kernels: ONE kernel per tick, what a packed kernel cannot reduce its own wave redoes on the general path)
    case TICK_GENERAL: return launch_rc(launch_tick(a, MODE_TICK, grid_tick(b, B), stream, tp, &b->last_tick_variant), "tick");
    case TICK_SIM3P:   // (FIXD: one model, its plan of the fixed dimensions; the launcher adds: no model_id array, a row that has the form)
      return launch_rc(launch_tick_sim3p(a, stream, tp, &b->last_tick_variant, b->sim3p_fixd && b->n_models == 1 && b->fixd_dims[0], &b->last_tick_fixd), "packed sim3 tick");
    case TICK_ORTHP: return launch_rc(launch_tick_orthp(a, stream, b->plan_host[0].q_ok == 2, tp, &b->last_tick_variant), "packed orth tick");
    case TICK_BOXP: return launch_rc(launch_tick_boxp(a, stream, tp, &b->last_tick_variant), "packed box tick");
    case TICK_SIM3: break;   // two kernels, below: the compact one, then the general path over the instances it deferred (singular leg block)
  }
  if ((rc = launch_rc(launch_tick_sim3(a, B, stream, &b->last_tick_variant), "sim3 tick"))) return rc;
  if ((rc = launch_rc(launch_tick_deferred(a, stream), "deferred tick")))
    (void)hipMemsetAsync(b->d_defer, 0, sizeof(int32_t), (hipStream_t)stream);   // the list the sim3 kernel may have filled stays behind: empty it, or the next tick appends after a stale count
  return rc;
}

// ---------------------------------------------------------------------------------------------- entry points
extern "C" int wbc_fk_jacobians(WbcBatch* b, int B, const double* q, const int32_t* model_id, int mem,
                                const WbcFkOut* out, void* stream) {
  int rc = check_batch(b, B, "wbc_fk_jacobians", false);
  if (rc) return rc;
  if (!q || !out) return fail(WBC_E_ARG, "wbc_fk_jacobians: null argument");
  if (b->n_models > 1 && !model_id) return fail(WBC_E_ARG, "wbc_fk_jacobians: model_id is required with %d models", b->n_models);
  HIP_TRY(hipSetDevice(b->device_id));
  KernelArgs a;
  fill_args(a, b, B, 0.0);
  if (!b->configured[0]) {   // FK needs no settings; give the kernel a zeroed config to read its (unused) switches from
    WbcConfig z;
    memset(&z, 0, sizeof z);
    for (int i = 0; i < b->n_models; ++i)
      if (!b->configured[i]) HIP_TRY(hipMemcpy(b->d_cfgs + i, &z, sizeof z, hipMemcpyHostToDevice));
  }
  a.in.q = q; a.in.model_id = model_id; a.fk = *out;
  const int nj = b->max_nj, nf = b->max_nf;   // output strides: the largest model of the handle
  Stager st{b, mem, (hipStream_t)stream, {}};
  st.in(&a.in.q, (size_t)B * WBC_Q_STRIDE); st.in(&a.in.model_id, (size_t)B);
  st.out(&a.fk.oMi, (size_t)B * nj * 12); st.out(&a.fk.oMf, (size_t)B * nf * 12);
  st.out(&a.fk.J, (size_t)B * 6 * WBC_V_STRIDE); st.out(&a.fk.com, (size_t)B * 3); st.out(&a.fk.Jcom, (size_t)B * 3 * WBC_V_STRIDE);
  if ((rc = st.stage())) return rc;
  if ((rc = launch_rc(launch_tick(a, MODE_FK, grid_tick(b, B), stream, nullptr, &b->last_tick_variant), "fk"))) return rc;
  return st.finish();
}

extern "C" int wbc_assemble(WbcBatch* b, int B, const WbcTickIn* in, double dt, int mem, const WbcQpData* out, void* stream) {
  return wbc_assemble_tp(b, B, in, nullptr, dt, mem, out, stream);
}
extern "C" int wbc_assemble_tp(WbcBatch* b, int B, const WbcTickIn* in, const WbcTaskParams* tp, double dt, int mem, const WbcQpData* out,
                               void* stream) {
  int rc = check_batch(b, B, "wbc_assemble", true);
  if (rc) return rc;
  if (!out) return fail(WBC_E_ARG, "wbc_assemble: null output");
  if ((rc = check_dt(dt, "wbc_assemble"))) return rc;
  if ((rc = validate_tick_in(b, in, "wbc_assemble"))) return rc;
  HIP_TRY(hipSetDevice(b->device_id));
  KernelArgs a;
  fill_args(a, b, B, dt);
  a.in = *in; a.qp = *out;
  Stager st{b, mem, (hipStream_t)stream, {}};
  stage_tick_in(st, a.in, B, b);
  st.in(&tp, (size_t)B);
  const size_t n = (size_t)B, m = b->mrows, p = b->prows, V = WBC_V_STRIDE;
  st.out(&a.qp.A, n * m * V); st.out(&a.qp.b, n * m); st.out(&a.qp.H, n * V * V); st.out(&a.qp.g, n * V);
  st.out(&a.qp.C, n * p * V); st.out(&a.qp.Clb, n * p); st.out(&a.qp.Cub, n * p); st.out(&a.qp.lb, n * V); st.out(&a.qp.ub, n * V);
  if ((rc = st.stage())) return rc;
  if ((rc = auto_posture(b, a, B, stream))) return rc;
  if ((rc = launch_rc(launch_tick(a, MODE_ASSEMBLE, grid_tick(b, B), stream, tp, &b->last_tick_variant), "assemble"))) return rc;
  return st.finish();
}

extern "C" int wbc_tick(WbcBatch* b, int B, const WbcTickIn* in, double dt, int mem, const WbcTickOut* out, void* stream) {
  return wbc_tick_tp(b, B, in, nullptr, dt, mem, out, stream);
}
extern "C" int wbc_tick_tp(WbcBatch* b, int B, const WbcTickIn* in, const WbcTaskParams* tp, double dt, int mem, const WbcTickOut* out,
                           void* stream) {
  int rc = check_batch(b, B, "wbc_tick", true);
  if (rc) return rc;
  if (!out || !out->qdot) return fail(WBC_E_ARG, "wbc_tick: qdot output required");
  if ((rc = check_dt(dt, "wbc_tick"))) return rc;
  if ((rc = validate_tick_in(b, in, "wbc_tick"))) return rc;
  HIP_TRY(hipSetDevice(b->device_id));
  KernelArgs a;
  fill_args(a, b, B, dt);
  a.in = *in; a.out = *out;
  Stager st{b, mem, (hipStream_t)stream, {}};
  stage_tick_in(st, a.in, B, b);
  st.in(&tp, (size_t)B);
  const size_t n = (size_t)B;
  st.out(&a.out.qdot, n * WBC_V_STRIDE); st.out(&a.out.status, n); st.out(&a.out.iters, n); st.out(&a.out.q_next, n * WBC_Q_STRIDE);
  st.out(&a.out.working_set, n * 2);
  if ((rc = st.stage())) return rc;
  a.ws_in = (const unsigned long long*)a.in.working_set; a.ws_out = (unsigned long long*)a.out.working_set;
  if ((rc = auto_posture(b, a, B, stream))) return rc;
  if ((rc = launch_tick_auto(b, a, B, stream, tp))) return rc;
  return st.finish();
}

extern "C" int wbc_posture_target(WbcBatch* b, int B, const double* q, const int32_t* model_id, int mem, double* u, double* q_after,
                                  void* stream) {
  int rc = check_batch(b, B, "wbc_posture_target", true);
  if (rc) return rc;
  if (!q || !u) return fail(WBC_E_ARG, "wbc_posture_target: q and u required");
  if (b->n_models > 1 && !model_id) return fail(WBC_E_ARG, "wbc_posture_target: model_id is required with %d models", b->n_models);
  HIP_TRY(hipSetDevice(b->device_id));
  Stager st{b, mem, (hipStream_t)stream, {}};
  st.in(&q, (size_t)B * WBC_Q_STRIDE); st.in(&model_id, (size_t)B);
  st.out(&u, (size_t)B * WBC_V_STRIDE); st.out(&q_after, (size_t)B * WBC_Q_STRIDE);
  if ((rc = st.stage())) return rc;
  if ((rc = run_posture(b, B, q, model_id, u, q_after, stream))) return rc;
  return st.finish();
}

extern "C" int wbc_update_state(WbcBatch* b, int B, const double* q_cur, const double* q_next, const double* imu,
                                const double* foot_targets, const int32_t* model_id, int mem, double* q_new, void* stream) {
  int rc = check_batch(b, B, "wbc_update_state", true);
  if (rc) return rc;
  if (!q_cur || !q_next || !foot_targets || !q_new) return fail(WBC_E_ARG, "wbc_update_state: q_cur, q_next, foot_targets and q_new are required");
  if (b->n_models > 1 && !model_id) return fail(WBC_E_ARG, "wbc_update_state: model_id is required with %d models", b->n_models);
  HIP_TRY(hipSetDevice(b->device_id));
  UpdateArgs a;
  memset(&a, 0, sizeof a);
  a.models = b->d_models; a.cfgs = b->d_cfgs; a.B = B; a.n_models = b->n_models; a.rot = b->rot;
  a.q_cur = q_cur; a.q_next = q_next; a.imu = imu; a.foot_targets = foot_targets; a.model_id = model_id; a.q_new = q_new;
  Stager st{b, mem, (hipStream_t)stream, {}};
  const size_t n = (size_t)B;
  const bool alias = (const double*)q_new == q_cur;
  st.in(&a.q_cur, n * WBC_Q_STRIDE); st.in(&a.q_next, n * WBC_Q_STRIDE); st.in(&a.imu, n * 4); st.in(&a.foot_targets, n * 15);
  st.in(&a.model_id, n);
  st.out(&a.q_new, n * WBC_Q_STRIDE);
  if ((rc = st.stage())) return rc;
  (void)alias;
  if (int e = launch_update_auto(b, a, B, stream)) return fail(WBC_E_HIP, "update kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  return st.finish();
}

// wbc_state_slack / wbc_rollout_watch: every model of the handle fits wbc_slack_kernel's whole-tree schedule (DevPlan.slack_ok, else
// WBC_E_UNSUPPORTED naming the limit build_q_tables found), and the models' own joint ranges by DoF are on the device (first use).
static int slack_ready(WbcBatch* b, const char* who) {
  for (int i = 0; i < b->n_models; ++i) {
    if (b->plan_host[i].slack_ok) continue;
    const DevModel& M = b->models[i]->dev;
    if (M.njoints > 22) return fail(WBC_E_UNSUPPORTED, "%s: model %d does not fit the packed whole-tree schedule: %d joints (at most 22)", who, i, M.njoints);
    if (M.maxdepth > 7) return fail(WBC_E_UNSUPPORTED, "%s: model %d does not fit the packed whole-tree schedule: tree depth %d (at most 7)", who, i, M.maxdepth);
    return fail(WBC_E_UNSUPPORTED, "%s: model %d does not fit the packed whole-tree schedule: more than 16 joints at one tree depth", who, i);
  }
  if (!b->d_slack_lim) {
    std::vector<SlackLimits> lim(b->n_models);
    for (int i = 0; i < b->n_models; ++i) {
      const DevModel& M = b->models[i]->dev;
      const WbcModelBlob& blob = b->models[i]->blob;
      memset(&lim[i], 0, sizeof lim[i]);
      for (int d = 0; d < NL; ++d) {
        const int qi = (d >= 6 && d < M.nv) ? M.col_q[d] : 7;       // 1-DoF joints live in [7, nq) (wbc_model_create)
        lim[i].qi[d] = qi; lim[i].lo[d] = blob.q_lo[qi]; lim[i].hi[d] = blob.q_hi[qi];
      }
    }
    SlackLimits* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, sizeof(SlackLimits) * b->n_models));
    if (hipError_t e = hipMemcpy(d, lim.data(), sizeof(SlackLimits) * b->n_models, hipMemcpyHostToDevice)) {
      (void)hipFree(d);
      return fail(WBC_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    b->d_slack_lim = d;
  }
  return WBC_OK;
}

// The four slack families at q for every instance (include/wbc.h): one launch of wbc_slack_kernel.
extern "C" int wbc_state_slack(WbcBatch* b, int B, const double* q, const double* trunk_box_center, const int32_t* model_id, int mem,
                               const WbcSlackOut* out, void* stream) {
  int rc = check_batch(b, B, "wbc_state_slack", true);
  if (rc) return rc;
  if (!q) return fail(WBC_E_ARG, "wbc_state_slack: q is required");
  if (!out) return fail(WBC_E_ARG, "wbc_state_slack: out is required");
  if (b->n_models > 1 && !model_id) return fail(WBC_E_ARG, "wbc_state_slack: model_id is required with %d models", b->n_models);
  HIP_TRY(hipSetDevice(b->device_id));
  if ((rc = slack_ready(b, "wbc_state_slack"))) return rc;
  SlackArgs a;
  memset(&a, 0, sizeof a);
  a.models = b->d_models; a.cfgs = b->d_cfgs; a.plans = b->d_plans; a.lim = b->d_slack_lim;
  a.B = B; a.n_models = b->n_models; a.rot = b->rot;
  a.q = q; a.box = trunk_box_center; a.model_id = model_id;
  a.slack = out->slack; a.which = out->which; a.components = out->components;
  Stager st{b, mem, (hipStream_t)stream, {}};
  const size_t n = (size_t)B;
  st.in(&a.q, n * WBC_Q_STRIDE); st.in(&a.box, n * 4); st.in(&a.model_id, n);
  st.out(&a.slack, n * SLACK_NF); st.out(&a.which, n * SLACK_NF); st.out(&a.components, n * SLACK_NC);
  if ((rc = st.stage())) return rc;
  if (int e = launch_slack(a, stream)) return fail(WBC_E_HIP, "slack kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  return st.finish();
}

// The cotangent of the four slack families at q (include/wbc.h): argument checks, staging of host arrays, ONE launch of wbc_slackvjp_kernel's
// STATE stage (csrc/wbc_k_slackvjp.hip). No memset; the kernel writes every row of every output it is given.
static_assert(sizeof(WbcSlackGrad) == 4 * sizeof(void*), "wbc_capi.WbcSlackGrad");
static void slackvjp_args(SlackVjpArgs& a, WbcBatch* b, int B, const double* q, const double* box, const int32_t* model_id) {
  memset(&a, 0, sizeof a);
  a.models = b->d_models; a.cfgs = b->d_cfgs; a.plans = b->d_plans; a.lim = b->d_slack_lim;
  a.B = B; a.n_models = b->n_models; a.rot = b->rot;
  a.q = q; a.box = box; a.model_id = model_id;
}
extern "C" int wbc_state_slack_vjp(WbcBatch* b, int B, const double* q, const double* trunk_box_center, const int32_t* model_id,
                                   const double* g_slack, const double* g_components, int mem, const WbcSlackGrad* out, void* stream) {
  const char* who = "wbc_state_slack_vjp";
  int rc = check_batch(b, B, who, true);
  if (rc) return rc;
  if (!q) return fail(WBC_E_ARG, "%s: q is required", who);
  if (!out) return fail(WBC_E_ARG, "%s: out is required", who);
  if (!g_slack && !g_components) return fail(WBC_E_ARG, "%s: a cotangent is required (g_slack or g_components)", who);
  if (b->n_models > 1 && !model_id) return fail(WBC_E_ARG, "%s: model_id is required with %d models", who, b->n_models);
  if (!trunk_box_center && mem == WBC_MEM_HOST) {   // (device cotangents are not read here: the kernel then reports the row, see include/wbc.h)
    for (int i = 0; i < B; ++i) {
      bool on = g_slack && (g_slack[4 * i + WBC_SLACK_TRUNK_Z] != 0.0 || g_slack[4 * i + WBC_SLACK_TRUNK_ANG] != 0.0);
      for (int c = 4; g_components && c < SLACK_NC; ++c) on = on || g_components[(size_t)SLACK_NC * i + c] != 0.0;
      if (on) return fail(WBC_E_ARG, "%s: trunk_box_center is required: instance %d carries a non-zero cotangent on a trunk family", who, i);
    }
  }
  HIP_TRY(hipSetDevice(b->device_id));
  if ((rc = slack_ready(b, who))) return rc;
  SlackVjpArgs a;
  slackvjp_args(a, b, B, q, trunk_box_center, model_id);
  a.g_slack = g_slack; a.g_comp = g_components;
  a.d_q = out->d_q; a.d_box = out->d_trunk_box_center; a.which = out->which; a.grad_status = out->grad_status;
  Stager st{b, mem, (hipStream_t)stream, {}};
  const size_t n = (size_t)B;
  st.in(&a.q, n * WBC_Q_STRIDE); st.in(&a.box, n * 4); st.in(&a.model_id, n); st.in(&a.g_slack, n * SLACK_NF); st.in(&a.g_comp, n * SLACK_NC);
  st.out(&a.d_q, n * WBC_V_STRIDE); st.out(&a.d_box, n * 4); st.out(&a.which, n * SLACK_NF); st.out(&a.grad_status, n);
  if ((rc = st.stage())) return rc;
  if ((rc = launch_rc(launch_slackvjp(a, SLACKVJP_STATE, stream, &b->last_slackvjp_variant), "slack cotangent"))) return rc;
  return st.finish();
}
extern "C" int wbc_slack_grad_sizes(int32_t* sizeof_grad) {
  if (sizeof_grad) *sizeof_grad = (int32_t)sizeof(WbcSlackGrad);
  return WBC_OK;
}

// ---- The roll-out pipeline (wbc_rollout / _tp / _traj / _tracks / _watch): rollout_run is the one loop — check, stage,
// seed, begin extensions, per tick {posture, tick, update, extensions}, gather extensions, gather state, finish. An extension (TracksExt,
// WatchExt) holds the caller's structs, its kernels' argument struct and its counts, and provides stage (its Stager registrations), begin,
// after_tick(k) and gather; one the entry point does not pass adds nothing to the stream.
struct Roll {                // what the stages of one call share
  WbcBatch* b; int B, ticks, total; size_t n; hipStream_t s;   // total: ticks + hold_ticks
  WbcRollout ro; RollWs w;   // the caller's struct, its pointers staged; the workspace
  WbcTickIn first;           // the call's inputs as staged, before the loop points the mutable ones at the workspace
  UpdateArgs u;
};
static int give(hipStream_t s, void* dst, const void* src, size_t bytes) {   // a block to where it is wanted: a result the caller asked for, a state the caller gave
  if (dst && src) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  return WBC_OK;
}

// every track's inputs and, in the sweep (tg), behind each track's inputs its outputs
static void stage_tracks(Stager& st, WbcTracks& tj, size_t n, WbcTracksGrad* tg = nullptr) {
  for (int j = 0; j < tj.n_tracks; ++j) {
    WbcTrack& t = tj.track[j];
    const size_t np = n * (size_t)t.max_points * 3;
    st.in(&t.points, np); st.in(&t.tangents, np); st.in(&t.n_points, n); st.in(&t.du, n);
    if (tg) { st.out(&tg->track[j].d_points, np); st.out(&tg->track[j].d_tangents, np); st.out(&tg->track[j].d_du, n); }
  }
}

// Tracks (wbc_rollout_traj / wbc_rollout_tracks, arguments checked by the entry point): the update kernel leaves the followed targets alone
// and one wbc_traj_tick_kernel per tick scores the tick and writes every followed target of the next. one_track: wbc_rollout_traj's call —
// the gripper's position comes from the update kernel's grip_trace row, and a constant trunk step stays with the update kernel; otherwise
// the update kernel writes the six frames' positions of the tick into the workspace, beside the scores ([scored frame][B] within regions
// sized for six frames of max_batch), the bad-row flags and their count.
struct TracksExt {
  bool scored, one_track; size_t nsc;   // nsc: scored frames
  WbcTracks tj; WbcTrackScores so; TrajArgs ta; TrajWs ws;
  TracksExt(const WbcTracks& tracks, const WbcTrackScores* scores, bool one)
      : scored(scores != nullptr), one_track(one), nsc(scores ? (size_t)__builtin_popcount((unsigned)scores->score_mask) : 0), tj(tracks), so(scores ? *scores : WbcTrackScores{}), ta{}, ws{} {}
  void stage(Stager& st, size_t n, int ticks) {
    const size_t ng = so.group_size > 0 ? n / (size_t)so.group_size : 0;
    stage_tracks(st, tj, n);
    st.out(&tj.trunk_target_final, n * 3);
    st.out(&so.err_sq_sum, nsc * n); st.out(&so.err_max, nsc * n); st.out(&so.err_max_tick, nsc * n); st.out(&so.err_final, nsc * n);
    st.out(&so.first_bad_tick, n); st.out(&so.bad_ticks, n); st.out(&so.trace, (size_t)ticks * nsc * n * 3);
    st.out(&so.group_rms, nsc * ng); st.out(&so.group_err_max, nsc * ng); st.out(&so.group_worst_status, ng); st.out(&so.group_bad_instances, ng);
  }
  int begin(Roll& R) {
    if (int rc = ensure(R.b->d_traj, TrajWs::bytes((size_t)R.b->max_batch))) return rc;
    ws = TrajWs::carve(R.b->d_traj, (size_t)R.b->max_batch);
    ta.err_sq_sum = ws.err_sq_sum; ta.err_max = ws.err_max; ta.err_final = ws.err_final; ta.err_max_tick = ws.err_max_tick;
    ta.bad = ws.bad; ta.first_bad_tick = ws.first_bad_tick; ta.bad_ticks = ws.bad_ticks; ta.status_max = ws.status_max; ta.bad_count = ws.bad_count;
    ta.B = R.B; ta.ticks = R.ticks; ta.n_tracks = tj.n_tracks; ta.do_sum = scored; ta.score_mask = so.score_mask;
    for (int j = 0; j < tj.n_tracks; ++j) fill_track(ta.tr[j], tj.track[j]);
    ta.ee_target = R.w.ee_target; ta.trunk_target = R.w.trunk_target;
    if (!one_track) R.u.trunk_step = nullptr;   // wbc_rollout_tracks' constant trunk step is added by the trajectory kernel, after the tick was scored
    if (!one_track && ta.trunk_target) ta.trunk_step = R.ro.trunk_target_step;
    ta.one_track = one_track ? 1 : 0;
    if (one_track) ta.reached_stride = 3;                 // reached_off all 0: the gripper row
    else {
      ta.reached_stride = 3 * WBC_MAX_TRACKS;
      for (int f = 0; f < WBC_MAX_TRACKS; ++f) ta.reached_off[f] = 3 * f;
      if (ta.do_sum && nsc > 0) R.u.frames_out = ws.frames;
    }
    ta.status = R.w.status; ta.ro_status_max = R.ro.status_max;
    HIP_TRY(hipMemsetAsync(ta.bad_count, 0, sizeof(int32_t), R.s));
    return launch_rc(launch_traj_begin(ta, R.s), "trajectory");
  }
  // no trace asked for in a one-track call: the summary reads the tick's gripper row from the workspace
  double* grip_row() const { return one_track && ta.do_sum ? ws.frames : nullptr; }
  int after_tick(Roll& R, int k) {
    ta.reached = one_track ? R.u.grip_trace : ws.frames;
    ta.trace = so.trace ? so.trace + (size_t)k * nsc * R.n * 3 : nullptr;
    return launch_rc(launch_traj_tick(ta, k, R.s), "trajectory");
  }
  int gather(Roll& R) {
    if (!scored) return WBC_OK;
    const size_t fd = nsc * R.n * sizeof(double), fi = nsc * R.n * sizeof(int32_t), ii = R.n * sizeof(int32_t);
    int rc;
    if ((rc = give(R.s, so.err_sq_sum, ta.err_sq_sum, fd)) || (rc = give(R.s, so.err_max, ta.err_max, fd)) || (rc = give(R.s, so.err_final, ta.err_final, fd)) ||
        (rc = give(R.s, so.err_max_tick, ta.err_max_tick, fi)) || (rc = give(R.s, so.first_bad_tick, ta.first_bad_tick, ii)) ||
        (rc = give(R.s, so.bad_ticks, ta.bad_ticks, ii))) return rc;
    if (so.group_size <= 0 || !(so.group_rms || so.group_err_max || so.group_worst_status || so.group_bad_instances)) return WBC_OK;
    TrajGroupArgs ga{};
    ga.G = R.B / so.group_size; ga.M = so.group_size; ga.ticks = R.ticks; ga.n_scored = (int32_t)nsc;
    ga.err_sq_sum = ta.err_sq_sum; ga.err_max = ta.err_max; ga.status_max = ta.status_max; ga.bad_ticks = ta.bad_ticks;
    ga.group_rms = so.group_rms; ga.group_err_max = so.group_err_max; ga.group_worst_status = so.group_worst_status;
    ga.group_bad_instances = so.group_bad_instances;
    return launch_rc(launch_traj_groups(ga, R.s), "trajectory");
  }
};

// The watch (wbc_rollout_watch, arguments checked by the entry point; slack_ready has run): one wbc_slack_kernel per tick behind the update
// kernel, on the state it just wrote; the kernel keeps the per-instance results in the handle's workspace ([watched family][B] within regions
// sized for four families of max_batch), copied out (and reduced per group) after the last tick.
struct WatchExt {
  WbcSlackWatch wo; size_t nw; SlackArgs sa;   // nw: watched families
  explicit WatchExt(const WbcSlackWatch& watch) : wo(watch), nw((size_t)__builtin_popcount((unsigned)wo.mask)), sa{} {}
  void stage(Stager& st, size_t n, int total) {
    const size_t ng = wo.group_size > 0 ? n / (size_t)wo.group_size : 0;
    st.out(&wo.slack_min, nw * n); st.out(&wo.slack_final, nw * n); st.out(&wo.slack_min_tick, nw * n); st.out(&wo.slack_min_which, nw * n);
    st.out(&wo.neg_ticks, nw * n); st.out(&wo.first_neg_tick, nw * n); st.out(&wo.trace, (size_t)total * nw * n);
    st.out(&wo.group_min, nw * ng); st.out(&wo.group_neg_instances, nw * ng);
  }
  int begin(Roll& R) {
    WbcBatch* b = R.b;
    if (int rc = ensure(b->d_slack, SlackWs::bytes((size_t)b->max_batch))) return rc;
    const SlackWs ws = SlackWs::carve(b->d_slack, (size_t)b->max_batch);
    sa.slack_min = ws.slack_min; sa.slack_final = ws.slack_final;
    sa.min_tick = ws.min_tick; sa.min_which = ws.min_which; sa.neg_ticks = ws.neg_ticks; sa.first_neg = ws.first_neg;
    sa.models = b->d_models; sa.cfgs = b->d_cfgs; sa.plans = b->d_plans; sa.lim = b->d_slack_lim;
    sa.B = R.B; sa.n_models = b->n_models; sa.rot = b->rot; sa.mask = wo.mask;
    sa.q = R.w.q; sa.box = R.first.trunk_box_center; sa.model_id = R.first.model_id;
    return WBC_OK;
  }
  int after_tick(Roll& R, int k) {
    sa.k = k;
    sa.trace = wo.trace ? wo.trace + (size_t)k * nw * R.n : nullptr;
    return launch_rc(launch_slack(sa, R.s), "slack");
  }
  int gather(Roll& R) {
    const size_t fd = nw * R.n * sizeof(double), fi = nw * R.n * sizeof(int32_t);
    int rc;
    if ((rc = give(R.s, wo.slack_min, sa.slack_min, fd)) || (rc = give(R.s, wo.slack_final, sa.slack_final, fd)) ||
        (rc = give(R.s, wo.slack_min_tick, sa.min_tick, fi)) || (rc = give(R.s, wo.slack_min_which, sa.min_which, fi)) ||
        (rc = give(R.s, wo.neg_ticks, sa.neg_ticks, fi)) || (rc = give(R.s, wo.first_neg_tick, sa.first_neg, fi))) return rc;
    if (wo.group_size <= 0 || !(wo.group_min || wo.group_neg_instances)) return WBC_OK;
    SlackGroupArgs ga{};
    ga.G = R.B / wo.group_size; ga.M = wo.group_size; ga.n_w = (int32_t)nw;
    ga.slack_min = sa.slack_min; ga.neg_ticks = sa.neg_ticks; ga.group_min = wo.group_min; ga.group_neg_instances = wo.group_neg_instances;
    return launch_rc(launch_slack_groups(ga, R.s), "slack");
  }
};

// The record (wbc_rollout_record, arguments checked by the entry point): one wbc_tape_copy_kernel per tick behind the update kernel. Tick k's
// part of the tape holds what the tick saw — written by begin (k = 0) or behind tick k - 1's update — and what it answered. The loop is
// wbc_rollout_tp's, launch for launch: the ticks return working sets under option "warm_start" and then the tape holds them; a cold
// roll-out's ticks return none (asking for one selects other kernel variants, whose answers differ in the last bits: DESIGN.md §3.42), and
// the sweep reads the active sides off qdot, as wbc_qp_certificate and wbc_tick_vjp_state do without a working set.
struct RecordExt {
  void* tape; double* q_trace;
  RecordExt(void* t, double* qt) : tape(t), q_trace(qt) {}
  void stage(Stager& st, size_t n, int ticks) { st.out(&q_trace, (size_t)ticks * n * WBC_Q_STRIDE); }
  static void seg(TapeCopyArgs& c, const void* src, void* dst, size_t bytes_per_row) {
    if (src && dst) c.seg[c.n_seg++] = TapeSeg{src, dst, (int32_t)(bytes_per_row / 4), 0};
  }
  static void seen(TapeCopyArgs& c, const RollWs& w, const TapeWs& t) {   // the state and the targets the next tick sees
    const size_t d = sizeof(double);
    seg(c, w.q, t.q, d * WBC_Q_STRIDE); seg(c, w.ee_target, t.ee_target, d * 3 * WBC_NEE); seg(c, w.prev_ee_target, t.prev_ee_target, d * 3 * WBC_NEE);
    seg(c, w.trunk_target, t.trunk_target, d * 3); seg(c, w.prev_trunk_target, t.prev_trunk_target, d * 3);
  }
  int begin(Roll& R) {
    TapeCopyArgs c{};
    c.B = R.B;
    seen(c, R.w, TapeWs::carve(tape, R.n, 0));
    return launch_rc(launch_tape_copy(c, R.s), "tape");
  }
  int after_tick(Roll& R, int k) {
    TapeCopyArgs c{};
    c.B = R.B;
    const TapeWs t = TapeWs::carve(tape, R.n, k);
    seg(c, R.w.qdot, t.qdot, sizeof(double) * WBC_V_STRIDE); seg(c, R.w.status, t.status, sizeof(int32_t));
    if (R.b->warm_start) seg(c, R.w.working_set, t.working_set, 2 * sizeof(unsigned long long));   // (a cold tick returns none)
    if (q_trace) seg(c, R.w.q, q_trace + (size_t)k * R.n * WBC_Q_STRIDE, sizeof(double) * WBC_Q_STRIDE);
    if (k + 1 < R.ticks) seen(c, R.w, TapeWs::carve(tape, R.n, k + 1));
    return launch_rc(launch_tape_copy(c, R.s), "tape");
  }
  int gather(Roll& R) {   // the previous rotations every tick after the first saw: constant from the first update on
    if (R.ticks < 2 || !(R.w.ee_prev_rot || R.w.trunk_prev_rot)) return WBC_OK;
    TapeCopyArgs c{};
    c.B = R.B;
    const TapeHead h = TapeHead::carve(tape, R.n);
    seg(c, R.w.ee_prev_rot, h.ee_prev_rot, sizeof(double) * 9 * WBC_NEE); seg(c, R.w.trunk_prev_rot, h.trunk_prev_rot, sizeof(double) * 9);
    return launch_rc(launch_tape_copy(c, R.s), "tape");
  }
};

// K closed-loop ticks: the mutable controller state lives in the handle's rollout workspace; in0 is only read. Without extensions (tk, wx, rx
// NULL): one linear segment (WbcRollout.ee_target_step), the launches, memsets and copies of wbc_rollout_tp and nothing else.
static int rollout_run(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r, int mem, void* stream,
                       TracksExt* tk = nullptr, WatchExt* wx = nullptr, RecordExt* rx = nullptr) {
  // check
  int rc = check_batch(b, B, "wbc_rollout", true);
  if (rc) return rc;
  if (!r || r->ticks < 1) return fail(WBC_E_ARG, "wbc_rollout: ticks >= 1 required");
  if ((rc = check_dt(dt, "wbc_rollout"))) return rc;
  if (r->hold_ticks < 0 || (r->mode != WBC_ROLLOUT_RUNNING && r->mode != WBC_ROLLOUT_WARMUP))
    return fail(WBC_E_ARG, "wbc_rollout: hold_ticks >= 0 and mode WBC_ROLLOUT_RUNNING / WBC_ROLLOUT_WARMUP required");
  if ((rc = validate_tick_in(b, in0, "wbc_rollout"))) return rc;
  if (!in0->ee_target || !in0->prev_ee_target) return fail(WBC_E_ARG, "wbc_rollout: ee_target / prev_ee_target are required (the base estimator reads the foot targets)");
  HIP_TRY(hipSetDevice(b->device_id));
  if (wx && (rc = slack_ready(b, "wbc_rollout_watch"))) return rc;
  Roll R{};
  R.b = b; R.B = B; R.ticks = r->ticks; R.total = r->ticks + r->hold_ticks; R.n = (size_t)B; R.s = (hipStream_t)stream; R.ro = *r;
  const size_t n = R.n;
  hipStream_t s = R.s;
  if ((rc = ensure(b->d_roll, RollWs::bytes((size_t)b->max_batch)))) return rc;
  RollWs& w = R.w = RollWs::carve(b->d_roll, (size_t)b->max_batch);
  // the blocks of the optional inputs the caller did not give: NULL from here on, like the inputs
  if (!in0->trunk_target) w.trunk_target = nullptr;
  if (!in0->prev_trunk_target) w.prev_trunk_target = nullptr;
  if (!in0->ee_prev_rot) w.ee_prev_rot = nullptr;
  if (!in0->trunk_prev_rot) w.trunk_prev_rot = nullptr;
  // stage
  KernelArgs a;
  fill_args(a, b, B, dt);
  a.in = *in0;
  WbcRollout& ro = R.ro;
  Stager st{b, mem, s, {}};
  stage_tick_in(st, a.in, B, b);
  st.in(&tp, n);                         // (every tick reads the same rows)
  st.in(&ro.ee_target_step, n * 3 * WBC_NEE); st.in(&ro.trunk_target_step, n * 3); st.in(&ro.imu, n * 4);
  st.out(&ro.q_final, n * WBC_Q_STRIDE); st.out(&ro.qdot_last, n * WBC_V_STRIDE); st.out(&ro.ee_target_final, n * 3 * WBC_NEE);
  st.out(&ro.grip_trace, (size_t)R.total * n * 3); st.out(&ro.status_max, n); st.out(&ro.iters_sum, n);
  if (tk) tk->stage(st, n, R.ticks);
  if (wx) wx->stage(st, n, R.total);
  if (rx) rx->stage(st, n, R.ticks);
  if ((rc = st.stage())) return rc;
  const size_t d = n * sizeof(double);   // seed the mutable state from in0
  if ((rc = give(s, w.q, a.in.q, d * WBC_Q_STRIDE)) || (rc = give(s, w.ee_target, a.in.ee_target, d * 3 * WBC_NEE)) ||
      (rc = give(s, w.prev_ee_target, a.in.prev_ee_target, d * 3 * WBC_NEE)) || (rc = give(s, w.trunk_target, a.in.trunk_target, d * 3)) ||
      (rc = give(s, w.prev_trunk_target, a.in.prev_trunk_target, d * 3)) || (rc = give(s, w.ee_prev_rot, a.in.ee_prev_rot, d * 9 * WBC_NEE)) ||
      (rc = give(s, w.trunk_prev_rot, a.in.trunk_prev_rot, d * 9))) return rc;
  if (b->warm_start) {   // first tick: the caller's working set if there is one, else cold
    if (a.in.working_set) HIP_TRY(hipMemcpyAsync(w.working_set, a.in.working_set, n * 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    else HIP_TRY(hipMemsetAsync(w.working_set, 0, n * 2 * sizeof(unsigned long long), s));
    a.ws_in = w.working_set; a.ws_out = w.working_set;
  }
  if (ro.status_max) HIP_TRY(hipMemsetAsync(ro.status_max, 0, n * sizeof(int32_t), s));
  if (ro.iters_sum) HIP_TRY(hipMemsetAsync(ro.iters_sum, 0, n * sizeof(int32_t), s));
  R.first = a.in;
  a.in.q = w.q; a.in.ee_target = w.ee_target; a.in.prev_ee_target = w.prev_ee_target; a.in.trunk_target = w.trunk_target;
  a.in.prev_trunk_target = w.prev_trunk_target; a.in.ee_prev_rot = w.ee_prev_rot; a.in.trunk_prev_rot = w.trunk_prev_rot;
  a.out.qdot = w.qdot; a.out.q_next = w.q_next; a.out.status = w.status; a.out.iters = w.iters;
  UpdateArgs& u = R.u;
  u.models = b->d_models; u.cfgs = b->d_cfgs; u.B = B; u.n_models = b->n_models; u.mode = r->mode; u.rot = b->rot;
  u.q_cur = w.q; u.q_next = w.q_next; u.imu = ro.imu; u.foot_targets = w.ee_target; u.model_id = a.in.model_id; u.q_new = w.q;
  u.ee_target = w.ee_target; u.prev_ee_target = w.prev_ee_target; u.trunk_target = w.trunk_target; u.prev_trunk_target = w.prev_trunk_target;
  u.ee_prev_rot = w.ee_prev_rot; u.trunk_prev_rot = w.trunk_prev_rot; u.ee_ref_rot = a.in.ee_ref_rot; u.trunk_ref_euler = a.in.trunk_ref_euler;
  u.ee_step = ro.ee_target_step; u.trunk_step = ro.trunk_target_step;   // (a trajectory call has no ee_target_step: wbc_traj_tick_kernel moves those targets)
  u.status = w.status; u.iters = w.iters; u.status_max = ro.status_max; u.iters_sum = ro.iters_sum;
  // begin extensions
  if ((tk && (rc = tk->begin(R))) || (wx && (rc = wx->begin(R))) || (rx && (rc = rx->begin(R)))) return rc;
  const WbcTickIn loop_in = a.in;
  for (int k = 0; k < R.total; ++k) {
    if (k == R.ticks) { u.ee_step = nullptr; u.trunk_step = nullptr; }   // hold phase: the targets stay where they are
    a.in = loop_in;                       // auto_posture fills posture_u / q_con afresh every tick
    if ((rc = auto_posture(b, a, B, stream))) return rc;
    if ((rc = launch_tick_auto(b, a, B, stream, tp))) return rc;
    u.grip_trace = ro.grip_trace ? ro.grip_trace + (size_t)k * n * 3 : (tk ? tk->grip_row() : nullptr);
    if (int e = launch_update_auto(b, u, B, stream)) return fail(WBC_E_HIP, "update kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if ((tk && (rc = tk->after_tick(R, k))) || (wx && (rc = wx->after_tick(R, k))) || (rx && (rc = rx->after_tick(R, k)))) return rc;
  }
  // gather extensions, then the state
  if ((wx && (rc = wx->gather(R))) || (tk && (rc = tk->gather(R))) || (rx && (rc = rx->gather(R)))) return rc;
  if ((rc = give(s, ro.q_final, w.q, d * WBC_Q_STRIDE)) || (rc = give(s, ro.qdot_last, w.qdot, d * WBC_V_STRIDE)) ||
      (rc = give(s, ro.ee_target_final, w.ee_target, d * 3 * WBC_NEE)) ||
      (rc = give(s, tk ? tk->tj.trunk_target_final : nullptr, w.trunk_target, d * 3))) return rc;
  return st.finish();
}

extern "C" int wbc_rollout_tp(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r, int mem, void* stream) {
  return rollout_run(b, B, in0, tp, dt, r, mem, stream);
}
extern "C" int wbc_rollout(WbcBatch* b, int B, const WbcTickIn* in0, double dt, const WbcRollout* r, int mem, void* stream) {
  return wbc_rollout_tp(b, B, in0, nullptr, dt, r, mem, stream);
}

// ---- The gradient layers: what every entry point and the roll-out's sweep share. One refusal of a model the packed whole-tree
// schedule cannot hold, one answer to "what does the configuration read", the refusals and the staging driven by the output tables (OutRow),
// and ONE function per layer that fills the layer's kernel arguments from what the layer consumes and launches: an entry point is check,
// stage, that function, finish; the sweep calls the same functions with pointers into the tape and RollVjpWs.
static int layers_fit(const WbcBatch* b, const char* who) {
  for (int i = 0; i < b->n_models; ++i) {
    if (b->plan_host[i].slack_ok) continue;
    const DevModel& M = b->models[i]->dev;
    return fail(WBC_E_UNSUPPORTED, "%s: model %d does not fit the packed whole-tree schedule (%d joints, at most 22; tree depth %d, at most 7; at most 16 joints at one depth)",
                who, i, M.njoints, M.maxdepth);
  }
  return WBC_OK;
}
struct Reads {   // of a handle check_batch passed (the switches are every model's); est: the base estimator runs (roll-outs in RUNNING mode) and reads ee_target
  bool any_ee, est, trunk, com, reads_pu, con_trunk;
  uint32_t ee_on;
  int p, no_pu;   // constraint rows (b->prows: rows_con of switches every model shares); the first model whose posture mode does not read posture_u
  Reads(const WbcBatch* b, bool est_) : est(est_), ee_on(0), p(b->prows), no_pu(-1) {
    const WbcConfig& c = b->cfg_host[0];
    for (int i = 0; i < WBC_NEE; ++i) if (c.task_ee[i]) ee_on |= 1u << i;
    any_ee = ee_on != 0; trunk = c.task_trunk != 0; com = c.task_com != 0; con_trunk = c.con_trunk != 0;
    for (int i = b->n_models - 1; i >= 0; --i) if (b->cfg_host[i].task_joint < WBC_JOINT_MANI) no_pu = i;
    reads_pu = no_pu < 0;
  }
  bool operator()(Read what) const {
    switch (what) {
      case R_EE: return any_ee;
      case R_EE_EST: return any_ee || est;
      case R_TRUNK: return trunk;
      case R_COM: return com;
      case R_PU: return reads_pu;
      case R_BOX: return con_trunk;
      default: return true;
    }
  }
};
// "<name> requested, but ...": the first output of the table that is asked for and is the gradient of nothing the configuration reads.
// name_model: wbc_tick_vjp names the model whose posture mode does not read posture_u, wbc_rollout_vjp does not (each caller's wording is kept).
template <class G, size_t N> static int check_outs(const G& out, const OutRow<G> (&t)[N], const Reads& rd, const char* who, bool name_model) {
  for (const OutRow<G>& r : t) {
    if (!(out.*r.ptr) || rd(r.need)) continue;
    switch (r.need) {
      case R_EE: return fail(WBC_E_ARG, "%s: %s requested, but no EE task reads %s", who, r.name, r.src);
      case R_EE_EST: return fail(WBC_E_ARG, "%s: %s requested, but no EE task and no estimator reads %s", who, r.name, r.src);
      case R_TRUNK: return fail(WBC_E_ARG, "%s: %s requested, but the trunk task is off", who, r.name);
      case R_COM: return fail(WBC_E_ARG, "%s: %s requested, but the CoM task is off", who, r.name);
      case R_BOX: return fail(WBC_E_ARG, "%s: %s requested, but the trunk constraint is off", who, r.name);
      default:
        if (name_model) return fail(WBC_E_ARG, "%s: %s requested, but the posture mode of model %d does not read posture_u", who, r.name, rd.no_pu);
        return fail(WBC_E_ARG, "%s: %s requested, but the posture mode of a model does not read posture_u", who, r.name);
    }
  }
  return WBC_OK;
}
template <class G, size_t N> static void stage_outs(Stager& st, G& out, const OutRow<G> (&t)[N], size_t n) {
  for (const OutRow<G>& r : t) st.out(&(out.*r.ptr), n * r.width);
}

// the state step: g -> d_q, d_qdot, d_foot_targets (wbc_stepvjp_kernel)
static int step_layer(WbcBatch* b, int B, double dt, int mode, const double* q_cur, const double* qdot, const double* foot_targets, const double* imu,
                      const int32_t* model_id, const double* g, const WbcStepGrad& out, void* stream) {
  StepVjpArgs a;
  memset(&a, 0, sizeof a);
  a.models = b->d_models; a.plans = b->d_plans; a.B = B; a.n_models = b->n_models; a.rot = b->rot; a.mode = mode; a.dt = dt;
  a.q_cur = q_cur; a.qdot = qdot; a.foot_targets = foot_targets; a.imu = imu; a.model_id = model_id; a.g = g; a.out = out;
  return launch_rc(launch_stepvjp(a, stream, &b->last_stepvjp_variant), "state step gradient");
}
// the certificate of solved QPs (wbc_qp_cert_kernel). Without constraint rows the row blocks are not read or written, whatever the pointers are.
static int cert_layer(WbcBatch* b, int B, const WbcQpProblem& q, const WbcQpCert& out, void* stream) {
  const bool rows = q.p > 0;
  CertArgs a;
  memset(&a, 0, sizeof a);
  a.B = B; a.n = q.n; a.p = q.p; a.m = q.m;
  a.H = q.H; a.g = q.g; a.A = q.A; a.bvec = q.b; a.C = rows ? q.C : nullptr; a.lb = q.lb; a.ub = q.ub;
  a.Clb = rows ? q.Clb : nullptr; a.Cub = rows ? q.Cub : nullptr;
  a.x = q.x; a.v = q.v; a.status = q.status; a.ws = (const unsigned long long*)q.working_set;
  a.y_bounds = out.y_bounds; a.y_rows = rows ? out.y_rows : nullptr; a.kkt = out.kkt; a.objective = out.objective;
  a.sens_x = out.sens_x; a.sens_bounds = out.sens_bounds; a.sens_rows = rows ? out.sens_rows : nullptr;
  a.n_active = out.n_active; a.cert_status = out.cert_status;
  return launch_rc(launch_cert(a, grid_for(b, B), stream), "qp certificate");
}
// the tick over its weights, gains and targets (wbc_grad_kernel), after the posture kernel where the tick itself would run it
static int tick_layer(WbcBatch* b, int B, double dt, const WbcTickIn& in, const WbcTaskParams* tp, const double* qdot, const double* sens_x,
                      const int32_t* status, const int32_t* cert_status, const WbcTickGrad& out, void* stream) {
  KernelArgs ka;                       // (auto_posture's view of the call: in, and whether the tick would derive u itself)
  fill_args(ka, b, B, dt);
  ka.in = in;
  ka.in.q_con = nullptr;               // cleared after staging: the task rows see q, no leaked configuration is asked for
  if (int rc = auto_posture(b, ka, B, stream)) return rc;
  GradArgs a;
  memset(&a, 0, sizeof a);
  a.models = b->d_models; a.cfgs = b->d_cfgs; a.plans = b->d_plans; a.B = B; a.n_models = b->n_models; a.rot = b->rot; a.dt = dt;
  a.in = ka.in;                        // posture_u AFTER auto_posture (still null: every sweep is structurally zero, the kernel reads DevPlan.post_zero)
  a.tp = tp; a.qdot = qdot; a.sens_x = sens_x; a.status = status; a.cert_status = cert_status; a.out = out;
  return launch_rc(launch_grad(a, stream, &b->last_grad_variant), "tick gradient");
}
// the tick over its state (wbc_gradq_kernel). No posture kernel: the layer sees the CALLER's posture_u, which is held constant.
static int tickq_layer(WbcBatch* b, int B, double dt, const WbcTickIn& in, const WbcTaskParams* tp, const WbcTickSens& sens, const WbcTickStateGrad& out,
                       void* stream) {
  GradQArgs a;
  memset(&a, 0, sizeof a);
  a.models = b->d_models; a.cfgs = b->d_cfgs; a.plans = b->d_plans; a.B = B; a.n_models = b->n_models; a.rot = b->rot; a.dt = dt;
  a.in = in; a.tp = tp; a.sens = sens; a.out = out;
  if (b->prows == 0) a.sens.sens_rows = a.sens.y_rows = nullptr;
  return launch_rc(launch_gradq(a, stream, &b->last_gradq_variant), "tick state gradient");
}

// ---- Roll-out gradients in two calls (include/wbc.h): wbc_rollout_record is rollout_run with the RecordExt extension;
// wbc_rollout_vjp walks the tape from the last tick to the first and launches, per tick, the layers' own kernels on the taped inputs
// (wbc_stepvjp_kernel, the general kernel's assemble mode, wbc_qp_cert_kernel, wbc_grad_kernel, wbc_gradq_kernel) and the link kernel.
static_assert(sizeof(WbcRolloutSeed) == 3 * sizeof(void*) && sizeof(WbcRolloutGrad) == 14 * sizeof(void*), "wbc_capi.WbcRolloutSeed / WbcRolloutGrad");
extern "C" size_t wbc_rollout_tape_bytes(int B, int ticks) {
  return (B < 1 || ticks < 1) ? 0 : (size_t)B * (TAPE_HEAD_BYTES + (size_t)ticks * TAPE_TICK_BYTES);
}
// what both calls refuse, before any launch
static int check_record_call(WbcBatch* b, int B, const WbcTickIn* in0, const WbcRollout* r, const void* tape, size_t tape_bytes, const char* who) {
  int rc = check_batch(b, B, who, true);
  if (rc) return rc;
  if (!r || r->ticks < 1) return fail(WBC_E_ARG, "%s: ticks >= 1 required", who);
  if (r->hold_ticks != 0) return fail(WBC_E_ARG, "%s: hold_ticks = %d: a recorded roll-out has no hold phase", who, r->hold_ticks);
  if (!in0) return fail(WBC_E_ARG, "%s: q is required", who);
  if (in0->q_con) return fail(WBC_E_ARG, "%s: q_con is not supported (the constraints would see another configuration than the task rows)", who);
  for (int i = 0; i < b->n_models; ++i) {
    const int tj = b->cfg_host[i].task_joint;
    if ((tj == WBC_JOINT_MANI || tj == WBC_JOINT_HYBRID) && !in0->posture_u)
      return fail(WBC_E_ARG, "%s: posture mode MANI / HYBRID of model %d needs posture_u (it is held constant over the ticks)", who, i);
  }
  if (!tape) return fail(WBC_E_ARG, "%s: tape is required (device memory of wbc_rollout_tape_bytes(B, ticks) bytes)", who);
  const size_t want = wbc_rollout_tape_bytes(B, r->ticks);
  if (tape_bytes < want) return fail(WBC_E_ARG, "%s: tape_bytes = %zu, wbc_rollout_tape_bytes(%d, %d) = %zu", who, tape_bytes, B, r->ticks, want);
  return layers_fit(b, who);
}
extern "C" int wbc_rollout_record(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r, void* tape,
                                  size_t tape_bytes, double* q_trace, int mem, void* stream) {
  if (int rc = check_record_call(b, B, in0, r, tape, tape_bytes, "wbc_rollout_record")) return rc;
  RecordExt rx(tape, q_trace);
  return rollout_run(b, B, in0, tp, dt, r, mem, stream, nullptr, nullptr, &rx);
}

template <class T> static int ensure_size(T*& p, size_t& have, size_t want) {   // a workspace that grows with the configuration's row counts
  if (want <= have) return WBC_OK;
  if (p) HIP_TRY(hipFree(p));
  p = nullptr; have = 0;
  HIP_TRY(hipMalloc((void**)&p, want));
  have = want;
  return WBC_OK;
}
// ---- argument checks of the track calls. `who`: the entry point's name; `pre`: "" or "track J: " (the text of every message is the callers')
static int check_group_size(const char* who, int group_size, int B) {
  if (group_size < 0 || (group_size > 0 && (B < 1 || B % group_size != 0))) return fail(WBC_E_ARG, "%s: group_size = %d does not divide B = %d", who, group_size, B);
  return WBC_OK;
}
static int check_track(const WbcTrack& t, const char* who, const char* pre) {
  if (t.max_points < 2 || t.max_points > WBC_MAX_TRAJ_POINTS)
    return fail(WBC_E_ARG, "%s: %smax_points = %d outside [2, %d]", who, pre, t.max_points, WBC_MAX_TRAJ_POINTS);
  if (!t.points) return fail(WBC_E_ARG, "%s: %spoints is required", who, pre);
  if (t.tangents && t.kind == WBC_TRACK_LINEAR) return fail(WBC_E_ARG, "%s: %stangents must be NULL for a LINEAR track", who, pre);
  if (!t.du && !(std::isfinite(t.du_all) && t.du_all > 0)) return fail(WBC_E_ARG, "%s: %sdu_all must be finite and positive when du is NULL", who, pre);
  return WBC_OK;
}

// The argument checks of wbc_rollout_tracks (several followed targets — WbcTracks: end effectors and trunk, LINEAR or HERMITE — any frame
// scored: WbcTrackScores), also wbc_rollout_watch's with tracks.
static int check_tracks_call(int B, const WbcTickIn* in0, const WbcRollout* r, const WbcTracks* tracks, const WbcTrackScores* scores) {
  const char* who = "wbc_rollout_tracks";
  if (!r || !tracks) return fail(WBC_E_ARG, "wbc_rollout_tracks: r and tracks are required");
  if (r->ee_target_step) return fail(WBC_E_ARG, "wbc_rollout_tracks: ee_target_step must be NULL (tracks move the followed targets; the other EE targets are constant)");
  if (r->hold_ticks != 0) return fail(WBC_E_ARG, "wbc_rollout_tracks: hold_ticks must be 0 (a track holds its last milestone by itself)");
  if (tracks->n_tracks < 1 || tracks->n_tracks > WBC_MAX_TRACKS)
    return fail(WBC_E_ARG, "wbc_rollout_tracks: n_tracks = %d outside [1, %d]", tracks->n_tracks, WBC_MAX_TRACKS);
  unsigned seen = 0;
  for (int j = 0; j < tracks->n_tracks; ++j) {
    const WbcTrack& t = tracks->track[j];
    if (t.target < 0 || t.target > WBC_TARGET_TRUNK) return fail(WBC_E_ARG, "wbc_rollout_tracks: track %d: target = %d outside [0, %d]", j, t.target, WBC_TARGET_TRUNK);
    if (seen & (1u << t.target)) return fail(WBC_E_ARG, "wbc_rollout_tracks: track %d: target = %d is repeated (each target at most once)", j, t.target);
    seen |= 1u << t.target;
    if (t.kind != WBC_TRACK_LINEAR && t.kind != WBC_TRACK_HERMITE) return fail(WBC_E_ARG, "wbc_rollout_tracks: track %d: kind = %d is no WBC_TRACK_*", j, t.kind);
    char pre[24];
    snprintf(pre, sizeof pre, "track %d: ", j);
    if (int rc = check_track(t, who, pre)) return rc;
  }
  const bool trunk_track = (seen >> WBC_TARGET_TRUNK) & 1;
  if (trunk_track && r->trunk_target_step)
    return fail(WBC_E_ARG, "wbc_rollout_tracks: trunk_target_step must be NULL with a trunk track (the track moves that target)");
  if (scores) {
    if (scores->score_mask < 0 || scores->score_mask >= (1 << WBC_MAX_TRACKS))
      return fail(WBC_E_ARG, "wbc_rollout_tracks: score_mask = 0x%x has bits beyond frame %d", (unsigned)scores->score_mask, WBC_TARGET_TRUNK);
    if (int rc = check_group_size(who, scores->group_size, B)) return rc;
  }
  const bool trunk_scored = scores && ((scores->score_mask >> WBC_TARGET_TRUNK) & 1);
  if ((trunk_track || trunk_scored) && in0 && (!in0->trunk_target || !in0->prev_trunk_target))
    return fail(WBC_E_ARG, "wbc_rollout_tracks: a trunk track or score bit %d needs in0->trunk_target and prev_trunk_target", WBC_TARGET_TRUNK);
  return WBC_OK;
}

// ---- The reverse sweep (wbc_rollout_vjp / _tracks / _scored): rollout_vjp_run is the one sweep, as rollout_run is the one
// loop — check, stage, link BEGIN, begin extensions, per tick from K - 1 down to 0 {before_step, step, [ADDV], posture, assemble, certificate,
// [tick layer], tick-state layer, LINK, after_link}, finish. An extension (TrackAdjExt, ScoreSeedExt) holds the caller's structs and its
// kernel's argument struct and provides check (what its call refuses beyond the sweep's own refusals, before any launch), stage (its Stager
// registrations), begin, before_step(k) and after_link(k); one the entry point does not pass adds nothing to the stream.
struct Sweep {               // what the stages of one sweep share
  WbcBatch* b; int B, K; size_t n; void* stream; void* tape;
  RollVjpWs w; WbcRolloutGrad og; WbcTickIn first;   // the workspace; the caller's outputs and inputs, their pointers staged
};

// The track adjoint (wbc_rollout_vjp_tracks): one stage of wbc_trackvjp_kernel behind the link kernel's BEGIN and behind every LINK.
struct TrackAdjExt {
  const WbcTracks* in; const WbcTracksGrad* out;   // as the caller gave them: either may be NULL until the sweep's checks are through
  WbcTracks tj; WbcTracksGrad tg; TrackVjpArgs va;
  TrackAdjExt(const WbcTracks* tracks, const WbcTracksGrad* tracks_out) : in(tracks), out(tracks_out), tj{}, tg{} { memset(&va, 0, sizeof va); }
  // what wbc_rollout_vjp_tracks refuses beyond both calls' own refusals, before any launch (og: the sweep's outputs as the caller gave them)
  int check(const WbcRolloutGrad* og, const char* who) const {
    if (!out) return fail(WBC_E_ARG, "%s: tracks_out is required", who);
    if (og && og->d_ee_target_step) return fail(WBC_E_ARG, "%s: d_ee_target_step requested, but a roll-out along tracks has no ee_target_step", who);
    for (int j = 0; j < WBC_MAX_TRACKS; ++j) {
      const WbcTrackGrad& g = out->track[j];
      if (j >= in->n_tracks) {
        if (g.d_points || g.d_tangents || g.d_du)
          return fail(WBC_E_ARG, "%s: tracks_out->track[%d] has an output set, but n_tracks = %d", who, j, in->n_tracks);
        continue;
      }
      const WbcTrack& t = in->track[j];
      if (t.target == WBC_TARGET_TRUNK && og && og->d_trunk_target_step)
        return fail(WBC_E_ARG, "%s: d_trunk_target_step requested, but track %d moves the trunk target (there is no trunk_target_step)", who, j);
      if (g.d_tangents && (t.kind != WBC_TRACK_HERMITE || !t.tangents))
        return fail(WBC_E_ARG, "%s: tracks_out->track[%d].d_tangents requested, but the track is %s", who, j,
                    t.kind != WBC_TRACK_HERMITE ? "LINEAR" : "HERMITE with tangents == NULL (the default rule: its gradient is part of d_points)");
    }
    return WBC_OK;
  }
  void stage(Stager& st, size_t n) { tj = *in; tg = *out; stage_tracks(st, tj, n, &tg); }
  bool wanted() const {   // an output is asked for (a track's cotangent is the tick layer's d_*_target)
    for (int j = 0; j < tj.n_tracks; ++j) if (tg.track[j].d_points || tg.track[j].d_tangents || tg.track[j].d_du) return true;
    return false;
  }
  int launch(const Sweep& W, int stage, int k) {
    va.k = k;
    return launch_rc(launch_trackvjp(va, stage, W.stream, &W.b->last_trackvjp_variant), "roll-out gradient track adjoint");
  }
  int begin(const Sweep& W) {
    va.B = W.B; va.n_tracks = tj.n_tracks; va.Ebar = W.w.Ebar; va.TEbar = W.w.TEbar; va.worst = W.w.worst;
    va.d_ee_target = W.og.d_ee_target; va.d_trunk_target = W.og.d_trunk_target;
    for (int j = 0; j < tj.n_tracks; ++j) {
      TrackVjpTrack& d = va.tr[j];
      fill_track(d, tj.track[j]);
      d.d_points = tg.track[j].d_points; d.d_tangents = tg.track[j].d_tangents; d.d_du = tg.track[j].d_du;
    }
    return launch(W, TRACKVJP_BEGIN, W.K - 1);
  }
  int after_link(const Sweep& W, int k) { return launch(W, TRACKVJP_TICK, k); }
};

// The score seed (wbc_rollout_vjp_scored): one stage of wbc_scorevjp_kernel in front of every tick's step layer (SEED: g += J' c at q_(k+1),
// -c into the stash) and one between LINK and the track stage (TARGET).
struct ScoreSeedExt {
  const WbcScoreSeed* in;   // as the caller gave it: NULL is the sweep's first refusal
  WbcScoreSeed ss; ScoreVjpArgs sa;
  explicit ScoreSeedExt(const WbcScoreSeed* score) : in(score), ss{} { memset(&sa, 0, sizeof sa); }
  // what wbc_rollout_vjp_scored refuses beyond wbc_rollout_vjp_tracks' refusals, before any launch
  int check(const WbcTickIn* in0, const WbcRollout* r, const char* who) const {
    const WbcScoreSeed& sc = *in;
    if (!sc.g_err_sq_sum && !sc.g_err_final && !sc.g_err_max)
      return fail(WBC_E_ARG, "%s: a score cotangent is required (g_err_sq_sum, g_err_final or g_err_max)", who);
    if (sc.g_err_max && !sc.err_max_tick) return fail(WBC_E_ARG, "%s: g_err_max needs err_max_tick (as the record call returned it)", who);
    if (!sc.q_final) return fail(WBC_E_ARG, "%s: q_final is required (the state after the last tick: the tape ends one state earlier)", who);
    if (sc.score_mask <= 0 || sc.score_mask >= (1 << WBC_MAX_TRACKS))
      return fail(WBC_E_ARG, "%s: score_mask = 0x%x, want a bit of the frames 0..%d and none beyond", who, (unsigned)sc.score_mask, WBC_TARGET_TRUNK);
    if (((sc.score_mask >> WBC_TARGET_TRUNK) & 1) && !in0->trunk_target)
      return fail(WBC_E_ARG, "%s: score_mask bit %d needs in0->trunk_target", who, WBC_TARGET_TRUNK);
    if (r->imu) return fail(WBC_E_ARG, "%s: imu must be NULL (with an IMU quaternion fed back the state discards the orientation the scored position was formed with)", who);
    return WBC_OK;
  }
  void stage(Stager& st, size_t n) {
    ss = *in;
    const size_t ns = (size_t)__builtin_popcount((unsigned)ss.score_mask) * n;
    st.in(&ss.g_err_sq_sum, ns); st.in(&ss.g_err_final, ns); st.in(&ss.g_err_max, ns); st.in(&ss.err_max_tick, ns); st.in(&ss.q_final, n * WBC_Q_STRIDE);
  }
  int launch(const Sweep& W, int stage, int k) {
    sa.k = k;
    // (the statistic names the SEED row, the stage with kinematics and a ROT form; TARGET has one row)
    return launch_rc(launch_scorevjp(sa, stage, W.stream, stage == SCOREVJP_SEED ? &W.b->last_scorevjp_variant : nullptr), "roll-out gradient score cotangent");
  }
  int begin(const Sweep& W) {
    WbcBatch* b = W.b;
    sa.models = b->d_models; sa.plans = b->d_plans; sa.model_id = W.first.model_id; sa.B = W.B; sa.n_models = b->n_models; sa.K = W.K; sa.rot = b->rot;
    sa.score_mask = ss.score_mask; sa.g_sq = ss.g_err_sq_sum; sa.g_fin = ss.g_err_final; sa.g_max = ss.g_err_max; sa.err_max_tick = ss.err_max_tick;
    sa.g = W.w.g; sa.stash = W.w.stash; sa.worst = W.w.worst; sa.Ebar = W.w.Ebar; sa.TEbar = W.w.TEbar;
    sa.d_ee_target = W.og.d_ee_target; sa.d_trunk_target = W.og.d_trunk_target;
    return WBC_OK;
  }
  int before_step(const Sweep& W, int k, const TapeWs& T) {   // q_(k+1): the tape's q of tick k + 1, the caller's q_final behind the last tick
    sa.q = k == W.K - 1 ? ss.q_final : TapeWs::carve(W.tape, W.n, k + 1).q;
    sa.ee_target = T.ee_target; sa.trunk_target = W.first.trunk_target ? T.trunk_target : nullptr;
    return launch(W, SCOREVJP_SEED, k);
  }
  int after_link(const Sweep& W, int k) { return launch(W, SCOREVJP_TARGET, k); }
};

// The watch seed (wbc_rollout_vjp_watched): the SEED stage of wbc_slackvjp_kernel in front of every tick's step layer (g += the slack
// families' cotangent at q_(k+1), the box term into acc_box). No after_link: a slack reads no target.
struct WatchSeedExt {
  const WbcWatchSeed* in;   // as the caller gave it: NULL is the sweep's first refusal
  WbcWatchSeed ws; SlackVjpArgs sa; size_t nw;
  explicit WatchSeedExt(const WbcWatchSeed* watch) : in(watch), ws{}, nw(0) { memset(&sa, 0, sizeof sa); }
  // what wbc_rollout_vjp_watched refuses beyond the sweep's own refusals, before any launch
  int check(const WbcTickIn* in0, const char* who) const {
    const WbcWatchSeed& w = *in;
    if (!w.g_slack_min && !w.g_slack_final && !w.g_trace)
      return fail(WBC_E_ARG, "%s: a slack cotangent is required (g_slack_min, g_slack_final or g_trace)", who);
    if (w.g_slack_min && !w.slack_min_tick) return fail(WBC_E_ARG, "%s: g_slack_min needs slack_min_tick (as the record call returned it)", who);
    if (!w.q_final) return fail(WBC_E_ARG, "%s: q_final is required (the state after the last tick: the tape ends one state earlier)", who);
    if (w.mask <= 0 || w.mask >= (1 << WBC_N_SLACK))
      return fail(WBC_E_ARG, "%s: mask = 0x%x must have at least one of the bits 0..%d and none beyond", who, (unsigned)w.mask, WBC_N_SLACK - 1);
    if ((w.mask & ((1 << WBC_SLACK_TRUNK_Z) | (1 << WBC_SLACK_TRUNK_ANG))) && !in0->trunk_box_center)
      return fail(WBC_E_ARG, "%s: the trunk families (mask bits %d, %d) need in0->trunk_box_center", who, WBC_SLACK_TRUNK_Z, WBC_SLACK_TRUNK_ANG);
    return WBC_OK;
  }
  void stage(Stager& st, size_t n, int K) {
    ws = *in;
    nw = (size_t)__builtin_popcount((unsigned)ws.mask);
    st.in(&ws.g_slack_min, nw * n); st.in(&ws.g_slack_final, nw * n); st.in(&ws.g_trace, (size_t)K * nw * n); st.in(&ws.slack_min_tick, nw * n);
    st.in(&ws.q_final, n * WBC_Q_STRIDE);
  }
  int begin(const Sweep& W) {
    slackvjp_args(sa, W.b, W.B, nullptr, W.first.trunk_box_center, W.first.model_id);
    sa.K = W.K; sa.mask = ws.mask; sa.g_min = ws.g_slack_min; sa.g_fin = ws.g_slack_final; sa.min_tick = ws.slack_min_tick;
    sa.g = W.w.g; sa.acc_box = W.w.acc_box; sa.worst = W.w.worst;
    return WBC_OK;
  }
  int before_step(const Sweep& W, int k) {   // q_(k+1): the tape's q of tick k + 1, the caller's q_final behind the last tick
    sa.k = k;
    sa.q = k == W.K - 1 ? ws.q_final : TapeWs::carve(W.tape, W.n, k + 1).q;
    sa.g_trace = ws.g_trace ? ws.g_trace + (size_t)k * nw * W.n : nullptr;
    return launch_rc(launch_slackvjp(sa, SLACKVJP_SEED, W.stream, &W.b->last_slackvjp_variant), "roll-out gradient slack cotangent");
  }
};

static int rollout_vjp_run(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r, const void* tape,
                           size_t tape_bytes, const WbcRolloutSeed* seed, int mem, const WbcRolloutGrad* out, void* stream, const char* who,
                           TrackAdjExt* tx = nullptr, ScoreSeedExt* sx = nullptr, WatchSeedExt* wx = nullptr) {
  int rc;
  if (wx && !wx->in) return fail(WBC_E_ARG, "%s: watch is required (wbc_rollout_vjp / _tracks / _scored are the calls without one)", who);
  if (sx && !sx->in) return fail(WBC_E_ARG, "%s: score is required (wbc_rollout_vjp_tracks is the call without one)", who);
  if (tx && (rc = check_tracks_call(B, in0, r, tx->in, nullptr))) return rc;   // (first: tracks == NULL is refused before a field of it is read)
  if ((rc = check_record_call(b, B, in0, r, tape, tape_bytes, who))) return rc;
  if (!out) return fail(WBC_E_ARG, "%s: out is required", who);
  if (tx && (rc = tx->check(out, who))) return rc;
  if (!sx && !wx && (!seed || !(seed->g_q_final || seed->g_qdot_last || seed->g_q_trace)))
    return fail(WBC_E_ARG, "%s: a seed is required (g_q_final, g_qdot_last or g_q_trace)", who);
  if (sx && (rc = sx->check(in0, r, who))) return rc;
  if (wx && (rc = wx->check(in0, who))) return rc;
  if ((rc = check_dt(dt, who))) return rc;
  if (r->mode != WBC_ROLLOUT_RUNNING && r->mode != WBC_ROLLOUT_WARMUP)
    return fail(WBC_E_ARG, "%s: mode = %d, want WBC_ROLLOUT_RUNNING (%d) or WBC_ROLLOUT_WARMUP (%d)", who, r->mode, WBC_ROLLOUT_RUNNING, WBC_ROLLOUT_WARMUP);
  if ((rc = validate_tick_in(b, in0, who))) return rc;
  if (!in0->ee_target || !in0->prev_ee_target) return fail(WBC_E_ARG, "%s: ee_target / prev_ee_target are required (the base estimator reads the foot targets)", who);
  const Reads rd(b, r->mode == WBC_ROLLOUT_RUNNING);   // the estimator reads ee_target: the step's d_foot_targets reaches it without an EE task
  if ((rc = check_outs(*out, ROLL_OUT, rd, who, false))) return rc;
  HIP_TRY(hipSetDevice(b->device_id));
  if (wx && (rc = slack_ready(b, who))) return rc;
  // size the workspace: the task rows of wbc_assemble, the unit rows on the padded columns of the handle's smallest model, the constraint rows
  int min_nv = WBC_V_STRIDE;
  for (int i = 0; i < b->n_models; ++i) if (b->models[i]->dev.nv < min_nv) min_nv = b->models[i]->dev.nv;
  const int m = b->mrows, pad_rows = WBC_V_STRIDE - min_nv, M = m + pad_rows, p = rd.p, K = r->ticks;
  if (M > WBC_MAX_M) return fail(WBC_E_UNSUPPORTED, "%s: %d task rows + %d padding rows exceed the certificate's %d", who, m, pad_rows, WBC_MAX_M);
  const size_t NB = (size_t)b->max_batch, n = (size_t)B;
  if ((rc = ensure_size(b->d_rvjp, b->rvjp_bytes, RollVjpWs::bytes(NB, (size_t)M, (size_t)p)))) return rc;   // (after one call of these row counts: no allocation)
  Sweep W{};
  W.b = b; W.B = B; W.K = K; W.n = n; W.stream = stream; W.tape = const_cast<void*>(tape);   // (read only: TapeWs carves non-const pointers)
  const RollVjpWs& w = W.w = RollVjpWs::carve(b->d_rvjp, NB, (size_t)M, (size_t)p);
  // stage
  KernelArgs a;
  fill_args(a, b, B, dt);
  a.in = *in0;
  a.in.working_set = nullptr;
  WbcRolloutSeed sd = seed ? *seed : WbcRolloutSeed{};
  WbcRolloutGrad& og = W.og = *out;
  const double* imu = r->imu;
  Stager st{b, mem, (hipStream_t)stream, {}};
  stage_tick_in(st, a.in, B, b);
  st.in(&tp, n); st.in(&imu, n * 4);
  st.in(&sd.g_q_final, n * WBC_V_STRIDE); st.in(&sd.g_qdot_last, n * WBC_V_STRIDE); st.in(&sd.g_q_trace, (size_t)K * n * WBC_V_STRIDE);
  if (sx) sx->stage(st, n);
  if (wx) wx->stage(st, n, K);
  stage_outs(st, og, ROLL_OUT, n);
  st.out(&og.grad_status, n); st.out(&og.ticks_dropped, n);
  if (tx) tx->stage(st, n);
  if ((rc = st.stage())) return rc;
  const WbcTickIn& first = W.first = a.in;
  const bool have_ws = b->warm_start != 0;   // the tape holds working sets (the option as it was when the tape was recorded: include/wbc.h)
  const TapeHead head = TapeHead::carve(W.tape, n);
  // the outputs of the layers, in the workspace. The tick layer runs where an output of the sweep needs one of its (the state side runs on
  // every tick: g needs it); each of its outputs is wired where the configuration reads what it is the gradient of
  bool want_tick = false;
  for (const OutRow<WbcRolloutGrad>& row : ROLL_OUT) want_tick |= og.*row.ptr && row.ptr != &WbcRolloutGrad::d_q0 && row.ptr != &WbcRolloutGrad::d_trunk_box_center;
  if (tx) want_tick |= tx->wanted();
  const WbcStepGrad s_out{w.s_dq, w.v, w.s_dft, w.gs_step};
  const WbcTickStateGrad q_out{w.t_dq, rd.con_trunk ? w.t_box : nullptr, w.gs_tickq};
  WbcQpCert c_out{};
  c_out.y_rows = w.y_rows; c_out.sens_x = w.sens_x; c_out.sens_bounds = w.sens_bounds; c_out.sens_rows = w.sens_rows; c_out.cert_status = w.cert_status;
  RollVjpArgs L;
  memset(&L, 0, sizeof L);
  if (want_tick) {
    L.t.grad_status = w.gs_tick;
    for (size_t i = 0; i < sizeof(TICK_WS) / sizeof(TICK_WS[0]); ++i)
      if (rd(TICK_OUT[i].need)) L.t.*TICK_WS[i].out = w.*TICK_WS[i].ws;
  }
  L.models = b->d_models; L.model_id = first.model_id; L.B = B; L.n_models = b->n_models; L.K = K; L.m = m; L.pad_rows = pad_rows;
  L.ee_on = rd.ee_on; L.trunk_on = rd.trunk;
  L.g_q_final = sd.g_q_final; L.g_qdot_last = sd.g_qdot_last; L.g_q_trace = sd.g_q_trace;
  L.A = w.A; L.b = w.b; L.g = w.g; L.v = w.v;
  L.s_dq = s_out.d_q; L.s_dft = rd.est ? s_out.d_foot_targets : nullptr; L.t_dq = q_out.d_q; L.t_box = q_out.d_trunk_box_center;
  L.gs_step = w.gs_step; L.gs_tickq = w.gs_tickq;
  L.Ebar = w.Ebar; L.Pbar = w.Pbar; L.TEbar = w.TEbar; L.TPbar = w.TPbar; L.d_estep = w.d_estep; L.d_tstep = w.d_tstep; L.acc_tp = w.acc_tp;
  L.acc_com = w.acc_com; L.acc_comv = w.acc_comv; L.acc_pu = w.acc_pu; L.acc_box = w.acc_box; L.worst = w.worst; L.dropped = w.dropped;
  L.out = og;
  auto link = [&](int stage, int k) {   // (the launch chain is linear: every stage waits for the one before it on the stream)
    L.k = k;
    return launch_rc(launch_rollvjp(L, stage, stream, &b->last_rollvjp_variant), "roll-out gradient link");
  };
  if ((rc = link(ROLLVJP_BEGIN, K - 1))) return rc;
  if ((tx && (rc = tx->begin(W))) || (sx && (rc = sx->begin(W))) || (wx && (rc = wx->begin(W)))) return rc;
  for (int k = K - 1; k >= 0; --k) {
    const TapeWs T = TapeWs::carve(W.tape, n, k);
    WbcTickIn in = first;   // the inputs tick k saw
    in.q = T.q; in.ee_target = T.ee_target; in.prev_ee_target = T.prev_ee_target;
    if (first.trunk_target) in.trunk_target = T.trunk_target;
    if (first.prev_trunk_target) in.prev_trunk_target = T.prev_trunk_target;
    if (k > 0 && first.ee_prev_rot) in.ee_prev_rot = head.ee_prev_rot;
    if (k > 0 && first.trunk_prev_rot) in.trunk_prev_rot = head.trunk_prev_rot;
    if (sx && (rc = sx->before_step(W, k, T))) return rc;
    if (wx && (rc = wx->before_step(W, k))) return rc;
    // the step: g -> d_q, v = d_qdot, d_foot_targets; on the last tick v += g_qdot_last
    if ((rc = step_layer(b, B, dt, r->mode, T.q, T.qdot, T.ee_target, imu, first.model_id, w.g, s_out, stream))) return rc;
    if (k == K - 1 && sd.g_qdot_last && (rc = link(ROLLVJP_ADDV, K - 1))) return rc;
    // the tick's problem at the taped inputs. mrows = M is the stride of A: the padding rows stay where BEGIN wrote them
    a.in = in;
    a.mrows = M;
    a.qp = WbcQpData{};
    a.qp.A = w.A; a.qp.b = w.b; a.qp.lb = w.lb; a.qp.ub = w.ub;
    if (p > 0) { a.qp.C = w.C; a.qp.Clb = w.Clb; a.qp.Cub = w.Cub; }
    if ((rc = auto_posture(b, a, B, stream))) return rc;
    if ((rc = launch_rc(launch_tick(a, MODE_ASSEMBLE, grid_tick(b, B), stream, tp, &b->last_tick_variant), "assemble"))) return rc;
    // its certificate with v. The working set reaches the certificate and the tick-state layer under warm_start alone: only then the tape holds it
    WbcQpProblem qp{};
    qp.n = WBC_V_STRIDE; qp.p = p; qp.m = M;
    qp.A = w.A; qp.b = w.b; qp.C = w.C; qp.lb = w.lb; qp.ub = w.ub; qp.Clb = w.Clb; qp.Cub = w.Cub;
    qp.x = T.qdot; qp.v = w.v; qp.status = T.status; qp.working_set = have_ws ? (const uint64_t*)T.working_set : nullptr;
    if ((rc = cert_layer(b, B, qp, c_out, stream))) return rc;
    // the tick's two layers: the first is skipped when none of its outputs is asked for
    if (want_tick && (rc = tick_layer(b, B, dt, a.in, tp, T.qdot, w.sens_x, T.status, w.cert_status, L.t, stream))) return rc;
    WbcTickSens sn{};
    sn.qdot = T.qdot; sn.sens_x = w.sens_x; sn.sens_bounds = w.sens_bounds; sn.sens_rows = w.sens_rows; sn.y_rows = w.y_rows;
    sn.status = T.status; sn.cert_status = w.cert_status; sn.working_set = qp.working_set;
    if ((rc = tickq_layer(b, B, dt, in, tp, sn, q_out, stream))) return rc;
    if ((rc = link(ROLLVJP_LINK, k))) return rc;
    if ((sx && (rc = sx->after_link(W, k))) || (tx && (rc = tx->after_link(W, k)))) return rc;
  }
  return st.finish();
}
extern "C" int wbc_rollout_vjp(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r, const void* tape,
                               size_t tape_bytes, const WbcRolloutSeed* seed, int mem, const WbcRolloutGrad* out, void* stream) {
  return rollout_vjp_run(b, B, in0, tp, dt, r, tape, tape_bytes, seed, mem, out, stream, "wbc_rollout_vjp");
}
extern "C" int wbc_rollout_grad_sizes(int32_t* sizeof_seed, int32_t* sizeof_grad) {
  if (sizeof_seed) *sizeof_seed = (int32_t)sizeof(WbcRolloutSeed);
  if (sizeof_grad) *sizeof_grad = (int32_t)sizeof(WbcRolloutGrad);
  return WBC_OK;
}

// The roll-out along per-instance milestone trajectories (WbcTrajectory), scored on the device (WbcRolloutSummary): argument checks, then
// the shared loop on the one-track call: a LINEAR track of end effector ee_index, the gripper scored.
extern "C" int wbc_rollout_traj(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                                const WbcTrajectory* traj, const WbcRolloutSummary* sum, int mem, void* stream) {
  if (!r || !traj) return fail(WBC_E_ARG, "wbc_rollout_traj: r and traj are required");
  if (r->ee_target_step) return fail(WBC_E_ARG, "wbc_rollout_traj: ee_target_step must be NULL (the trajectory moves the followed target; the other EE targets are constant)");
  if (r->hold_ticks != 0) return fail(WBC_E_ARG, "wbc_rollout_traj: hold_ticks must be 0 (a trajectory holds its last milestone by itself)");
  if (traj->ee_index < 0 || traj->ee_index >= WBC_NEE) return fail(WBC_E_ARG, "wbc_rollout_traj: ee_index = %d outside [0, %d]", traj->ee_index, WBC_NEE - 1);
  WbcTracks tk{};
  WbcTrackScores sc{};
  WbcTrack& t = tk.track[0];
  tk.n_tracks = 1; sc.score_mask = 1 << 4;
  t.target = traj->ee_index; t.kind = WBC_TRACK_LINEAR; t.max_points = traj->max_points;
  t.points = traj->points; t.n_points = traj->n_points; t.du = traj->du; t.du_all = traj->du_all;
  int rc;
  if ((rc = check_track(t, "wbc_rollout_traj", "")) || (sum && (rc = check_group_size("wbc_rollout_traj", sum->group_size, B)))) return rc;
  if (sum) {
    sc.group_size = sum->group_size;
    sc.err_sq_sum = sum->err_sq_sum; sc.err_max = sum->err_max; sc.err_final = sum->err_final; sc.err_max_tick = sum->err_max_tick;
    sc.first_bad_tick = sum->first_bad_tick; sc.bad_ticks = sum->bad_ticks;
    sc.group_rms = sum->group_rms; sc.group_err_max = sum->group_err_max;
    sc.group_worst_status = sum->group_worst_status; sc.group_bad_instances = sum->group_bad_instances;
  }
  TracksExt ext(tk, sum ? &sc : nullptr, true);
  return rollout_run(b, B, in0, tp, dt, r, mem, stream, &ext);
}

extern "C" int wbc_rollout_tracks(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                                  const WbcTracks* tracks, const WbcTrackScores* scores, int mem, void* stream) {
  if (int rc = check_tracks_call(B, in0, r, tracks, scores)) return rc;
  TracksExt tk(*tracks, scores, false);
  return rollout_run(b, B, in0, tp, dt, r, mem, stream, &tk);
}

// The recorded roll-out along tracks and its sweep (include/wbc.h): wbc_rollout_tracks' loop with the record extension behind
// the tracks extension (tick k's part of the tape holds the followed targets the tick saw), then wbc_rollout_vjp's sweep with the adjoint of
// the track evaluation behind every link stage.
static_assert(sizeof(WbcTrackGrad) == 3 * sizeof(void*) && sizeof(WbcTracksGrad) == WBC_MAX_TRACKS * sizeof(WbcTrackGrad), "wbc_capi.WbcTrackGrad / WbcTracksGrad");
extern "C" int wbc_rollout_record_tracks(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                                         const WbcTracks* tracks, const WbcTrackScores* scores, void* tape, size_t tape_bytes, double* q_trace,
                                         int mem, void* stream) {
  int rc;
  if ((rc = check_tracks_call(B, in0, r, tracks, scores)) || (rc = check_record_call(b, B, in0, r, tape, tape_bytes, "wbc_rollout_record_tracks"))) return rc;
  TracksExt tk(*tracks, scores, false);
  RecordExt rx(tape, q_trace);
  return rollout_run(b, B, in0, tp, dt, r, mem, stream, &tk, nullptr, &rx);
}
extern "C" int wbc_rollout_vjp_tracks(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                                      const WbcTracks* tracks, const void* tape, size_t tape_bytes, const WbcRolloutSeed* seed, int mem,
                                      const WbcRolloutGrad* out, const WbcTracksGrad* tracks_out, void* stream) {
  TrackAdjExt tx(tracks, tracks_out);
  return rollout_vjp_run(b, B, in0, tp, dt, r, tape, tape_bytes, seed, mem, out, stream, "wbc_rollout_vjp_tracks", &tx);
}
extern "C" int wbc_rollout_vjp_scored(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                                      const WbcTracks* tracks, const void* tape, size_t tape_bytes, const WbcRolloutSeed* seed,
                                      const WbcScoreSeed* score, int mem, const WbcRolloutGrad* out, const WbcTracksGrad* tracks_out, void* stream) {
  TrackAdjExt tx(tracks, tracks_out);
  ScoreSeedExt sx(score);
  return rollout_vjp_run(b, B, in0, tp, dt, r, tape, tape_bytes, seed, mem, out, stream, "wbc_rollout_vjp_scored", &tx, &sx);
}
static_assert(sizeof(WbcScoreSeed) == 8 + 5 * sizeof(void*), "wbc_capi.WbcScoreSeed");
extern "C" int wbc_rollout_scored_sizes(int32_t* sizeof_score_seed) {
  if (sizeof_score_seed) *sizeof_score_seed = (int32_t)sizeof(WbcScoreSeed);
  return WBC_OK;
}
extern "C" int wbc_rollout_tracks_grad_sizes(int32_t* sizeof_track_grad, int32_t* sizeof_tracks_grad) {
  if (sizeof_track_grad) *sizeof_track_grad = (int32_t)sizeof(WbcTrackGrad);
  if (sizeof_tracks_grad) *sizeof_tracks_grad = (int32_t)sizeof(WbcTracksGrad);
  return WBC_OK;
}

// what every call with a WbcSlackWatch refuses of it
static int check_watch(const char* who, const WbcTickIn* in0, const WbcSlackWatch* watch, int B) {
  if (watch->mask <= 0 || watch->mask >= (1 << WBC_N_SLACK))
    return fail(WBC_E_ARG, "%s: mask = 0x%x must have at least one of the bits 0..%d and none beyond", who, (unsigned)watch->mask, WBC_N_SLACK - 1);
  if (int rc = check_group_size(who, watch->group_size, B)) return rc;
  if ((watch->mask & ((1 << WBC_SLACK_TRUNK_Z) | (1 << WBC_SLACK_TRUNK_ANG))) && in0 && !in0->trunk_box_center)
    return fail(WBC_E_ARG, "%s: the trunk families (mask bits %d, %d) need in0->trunk_box_center", who, WBC_SLACK_TRUNK_Z, WBC_SLACK_TRUNK_ANG);
  return WBC_OK;
}

// The roll-outs with the slack families watched (WbcSlackWatch): the watch's own argument checks, then the tracks call's (with tracks) and
// the shared loop. watch == NULL: the call without a watch, launch for launch.
extern "C" int wbc_rollout_watch(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                                 const WbcTracks* tracks, const WbcTrackScores* scores, const WbcSlackWatch* watch, int mem, void* stream) {
  int rc;
  if (scores && !tracks) return fail(WBC_E_ARG, "wbc_rollout_watch: scores needs tracks");
  if (watch) {
    if ((rc = check_watch("wbc_rollout_watch", in0, watch, B))) return rc;
  }
  if (tracks && (rc = check_tracks_call(B, in0, r, tracks, scores))) return rc;
  TracksExt tk(tracks ? *tracks : WbcTracks{}, scores, false);
  WatchExt wx(watch ? *watch : WbcSlackWatch{});
  return rollout_run(b, B, in0, tp, dt, r, mem, stream, tracks ? &tk : nullptr, watch ? &wx : nullptr);
}

// The recorded roll-out with the slack families watched, and its sweep seeded with the cotangents of what the watch returned (include/wbc.h;
// DESIGN.md §3.50): wbc_rollout_watch's loop with the record extension behind the watch, then the one sweep with the watch seed's stage in
// front of every step layer.
extern "C" int wbc_rollout_record_watch(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                                        const WbcTracks* tracks, const WbcTrackScores* scores, const WbcSlackWatch* watch, void* tape,
                                        size_t tape_bytes, double* q_trace, int mem, void* stream) {
  const char* who = "wbc_rollout_record_watch";
  int rc;
  if (!watch) return fail(WBC_E_ARG, "%s: watch is required (wbc_rollout_record / _record_tracks are the calls without one)", who);
  if (scores && !tracks) return fail(WBC_E_ARG, "%s: scores needs tracks", who);
  if ((rc = check_watch(who, in0, watch, B))) return rc;
  if (tracks && (rc = check_tracks_call(B, in0, r, tracks, scores))) return rc;
  if ((rc = check_record_call(b, B, in0, r, tape, tape_bytes, who))) return rc;
  TracksExt tk(tracks ? *tracks : WbcTracks{}, scores, false);
  WatchExt wx(*watch);
  RecordExt rx(tape, q_trace);
  return rollout_run(b, B, in0, tp, dt, r, mem, stream, tracks ? &tk : nullptr, &wx, &rx);
}
static_assert(sizeof(WbcWatchSeed) == 8 + 5 * sizeof(void*), "wbc_capi.WbcWatchSeed");
extern "C" int wbc_rollout_vjp_watched(WbcBatch* b, int B, const WbcTickIn* in0, const WbcTaskParams* tp, double dt, const WbcRollout* r,
                                       const WbcTracks* tracks, const void* tape, size_t tape_bytes, const WbcRolloutSeed* seed,
                                       const WbcScoreSeed* score, const WbcWatchSeed* watch, int mem, const WbcRolloutGrad* out,
                                       const WbcTracksGrad* tracks_out, void* stream) {
  const char* who = "wbc_rollout_vjp_watched";
  if (!watch) return fail(WBC_E_ARG, "%s: watch is required (wbc_rollout_vjp / _tracks / _scored are the calls without one)", who);
  if (score && !tracks) return fail(WBC_E_ARG, "%s: score needs tracks", who);
  if (!tracks && tracks_out) return fail(WBC_E_ARG, "%s: tracks_out must be NULL without tracks", who);
  TrackAdjExt tx(tracks, tracks_out);
  ScoreSeedExt sx(score);
  WatchSeedExt wx(watch);
  return rollout_vjp_run(b, B, in0, tp, dt, r, tape, tape_bytes, seed, mem, out, stream, who, tracks ? &tx : nullptr, score ? &sx : nullptr, &wx);
}
extern "C" int wbc_rollout_watched_sizes(int32_t* sizeof_watch_seed) {
  if (sizeof_watch_seed) *sizeof_watch_seed = (int32_t)sizeof(WbcWatchSeed);
  return WBC_OK;
}

static int qp_common(WbcBatch* b, int B, QpArgs& a, int mem, void* stream, const char* who) {
  int rc = check_batch(b, B, who, false, false);
  if (rc) return rc;
  const int n = a.n, p = a.p, m = a.m;
  if (n < 1 || n > WBC_MAX_NV || p < 0 || p > WBC_MAX_P || m < 0 || m > WBC_MAX_M) return fail(WBC_E_ARG, "%s: n = %d, p = %d, m = %d out of range", who, n, p, m);
  if (!a.x) return fail(WBC_E_ARG, "%s: x output required", who);
  if (p > 0 && (!a.C || !a.Clb || !a.Cub)) return fail(WBC_E_ARG, "%s: C, Clb, Cub required when p > 0", who);
  if ((a.lb != nullptr) != (a.ub != nullptr)) return fail(WBC_E_ARG, "%s: lb and ub go together", who);
  HIP_TRY(hipSetDevice(b->device_id));
  Stager st{b, mem, (hipStream_t)stream, {}};
  const size_t N = (size_t)B;
  st.in(&a.H, N * n * n); st.in(&a.g, N * n); st.in(&a.A, N * m * n); st.in(&a.bvec, N * m);
  st.in(&a.C, N * p * n); st.in(&a.lb, N * n); st.in(&a.ub, N * n); st.in(&a.Clb, N * p); st.in(&a.Cub, N * p);
  st.out(&a.x, N * n); st.out(&a.status, N); st.out(&a.iters, N); st.out(&a.H_out, N * n * n); st.out(&a.g_out, N * n);
  st.in(&a.ws_in, N * 2); st.out(&a.ws_out, N * 2);   // (host buffers are staged separately, so in and out may be the same host array)
  if ((rc = st.stage())) return rc;
  a.refine = b->refine; a.dbg_stop = b->dbg_stop;
  // several problems per wavefront (wbc_k_qpp.hip) unless the call carries working sets (hot start) or option packed_kernel is 0
  const int lanes = b->packed_kernel ? qp_packed_lanes(a) : 0;
  b->last_qp_path = lanes ? lanes : 1;
  if ((rc = launch_rc(lanes ? launch_qp_packed(a, stream, &b->last_qp_variant) : launch_qp(a, grid_for(b, B), stream, &b->last_qp_variant), "qp"))) return rc;
  return st.finish();
}

extern "C" int wbc_qp_solve(WbcBatch* b, int B, int n, int p, const double* H, const double* g, const double* C,
                            const double* lb, const double* ub, const double* Clb, const double* Cub, int mem,
                            double* x, int32_t* status, int32_t* iters, const uint64_t* working_set_in, uint64_t* working_set_out,
                            void* stream) {
  if (!H || !g) return fail(WBC_E_ARG, "wbc_qp_solve: H and g required");
  QpArgs a;
  memset(&a, 0, sizeof a);
  a.B = B; a.n = n; a.p = p; a.m = 0;
  a.H = H; a.g = g; a.C = C; a.lb = lb; a.ub = ub; a.Clb = Clb; a.Cub = Cub; a.x = x; a.status = status; a.iters = iters;
  a.ws_in = (const unsigned long long*)working_set_in; a.ws_out = (unsigned long long*)working_set_out;
  return qp_common(b, B, a, mem, stream, "wbc_qp_solve");
}

extern "C" int wbc_qp_solve_ls(WbcBatch* b, int B, int m, int n, int p, const double* A, const double* bvec, const double* C,
                               const double* lb, const double* ub, const double* Clb, const double* Cub, int mem, int use_mfma,
                               double* x, int32_t* status, int32_t* iters, double* H_out, double* g_out,
                               const uint64_t* working_set_in, uint64_t* working_set_out, void* stream) {
  if (!A || !bvec || m < 1) return fail(WBC_E_ARG, "wbc_qp_solve_ls: A, b and m >= 1 required");
  QpArgs a;
  memset(&a, 0, sizeof a);
  a.B = B; a.n = n; a.p = p; a.m = m; a.use_mfma = use_mfma < 0 ? (m >= WBC_MFMA_AUTO_ROWS) : (use_mfma != 0);
  a.A = A; a.bvec = bvec; a.C = C; a.lb = lb; a.ub = ub; a.Clb = Clb; a.Cub = Cub;
  a.x = x; a.status = status; a.iters = iters; a.H_out = H_out; a.g_out = g_out;
  a.ws_in = (const unsigned long long*)working_set_in; a.ws_out = (unsigned long long*)working_set_out;
  return qp_common(b, B, a, mem, stream, "wbc_qp_solve_ls");
}

// Dual solution, KKT certificate and sensitivities of solved QPs (include/wbc.h): argument checks, staging of host arrays, ONE launch of
// wbc_qp_cert_kernel (csrc/wbc_k_cert.hip). No workspace of its own, no memset: with device pointers the call can be captured.
static_assert(sizeof(WbcQpProblem) == 16 + 13 * sizeof(void*), "WbcQpProblem: four int32 and thirteen pointers (wbc_capi.WbcQpProblem)");
static_assert(sizeof(WbcQpCert) == 9 * sizeof(void*), "WbcQpCert: nine pointers (wbc_capi.WbcQpCert)");
extern "C" int wbc_qp_certificate(WbcBatch* b, int B, const WbcQpProblem* q, const WbcQpCert* out, int mem, void* stream) {
  const char* who = "wbc_qp_certificate";
  int rc = check_batch(b, B, who, false, false);
  if (rc) return rc;
  if (!q || !out) return fail(WBC_E_ARG, "%s: problem and out are required", who);
  const int n = q->n, p = q->p, m = q->m;
  const bool hg = q->H || q->g, ab = q->A || q->b;
  if (hg && ab) return fail(WBC_E_ARG, "%s: both H, g and A, b are given (exactly one pair)", who);
  if (!hg && !ab) return fail(WBC_E_ARG, "%s: neither H, g nor A, b is given (exactly one pair)", who);
  if (hg && (!q->H || !q->g)) return fail(WBC_E_ARG, "%s: H and g go together", who);
  if (ab && (!q->A || !q->b)) return fail(WBC_E_ARG, "%s: A and b go together", who);
  if (n < 1 || n > WBC_MAX_NV) return fail(WBC_E_ARG, "%s: n = %d outside [1, %d]", who, n, WBC_MAX_NV);
  if (p < 0 || p > WBC_MAX_P) return fail(WBC_E_ARG, "%s: p = %d outside [0, %d]", who, p, WBC_MAX_P);
  if (ab ? (m < 1 || m > WBC_MAX_M) : (m != 0)) return fail(WBC_E_ARG, "%s: m = %d (with A, b: 1..%d; with H, g: 0)", who, m, WBC_MAX_M);
  if (!q->x) return fail(WBC_E_ARG, "%s: x is required", who);
  if (p > 0 && (!q->C || !q->Clb || !q->Cub)) return fail(WBC_E_ARG, "%s: C, Clb, Cub required when p > 0", who);
  if ((q->lb != nullptr) != (q->ub != nullptr)) return fail(WBC_E_ARG, "%s: lb and ub go together", who);
  if (!q->v && out->sens_x) return fail(WBC_E_ARG, "%s: sens_x requested without v", who);
  if (!q->v && out->sens_bounds) return fail(WBC_E_ARG, "%s: sens_bounds requested without v", who);
  if (!q->v && out->sens_rows) return fail(WBC_E_ARG, "%s: sens_rows requested without v", who);
  HIP_TRY(hipSetDevice(b->device_id));
  WbcQpProblem a = *q;
  WbcQpCert o = *out;
  Stager st{b, mem, (hipStream_t)stream, {}};
  const size_t N = (size_t)B;
  st.in(&a.H, N * n * n); st.in(&a.g, N * n); st.in(&a.A, N * m * n); st.in(&a.b, N * m);
  st.in(&a.C, N * p * n); st.in(&a.lb, N * n); st.in(&a.ub, N * n); st.in(&a.Clb, N * p); st.in(&a.Cub, N * p);
  st.in(&a.x, N * n); st.in(&a.v, N * n); st.in(&a.status, N); st.in(&a.working_set, N * 2);
  st.out(&o.y_bounds, N * n); st.out(&o.y_rows, N * p); st.out(&o.kkt, N * 4); st.out(&o.objective, N);
  st.out(&o.sens_x, N * n); st.out(&o.sens_bounds, N * n); st.out(&o.sens_rows, N * p);
  st.out(&o.n_active, N); st.out(&o.cert_status, N);
  if ((rc = st.stage())) return rc;
  if ((rc = cert_layer(b, B, a, o, stream))) return rc;
  return st.finish();
}
extern "C" int wbc_qp_certificate_sizes(int32_t* sizeof_problem, int32_t* sizeof_cert) {
  if (sizeof_problem) *sizeof_problem = (int32_t)sizeof(WbcQpProblem);
  if (sizeof_cert) *sizeof_cert = (int32_t)sizeof(WbcQpCert);
  return WBC_OK;
}

// dL/d(task weights, gains, targets) of solved ticks (include/wbc.h): argument checks, staging of host arrays, ONE launch of wbc_grad_kernel
// (csrc/wbc_k_grad.hip) — after the posture kernel where the mode is MANI / HYBRID, posture_u is not given and a sweep matters, as wbc_assemble.
// No memset; the kernel writes every row of every output it is given.
static_assert(sizeof(WbcTickGrad) == 9 * sizeof(void*), "WbcTickGrad: nine pointers (wbc_capi.WbcTickGrad)");
extern "C" int wbc_tick_vjp(WbcBatch* b, int B, const WbcTickIn* in, const WbcTaskParams* tp, double dt, const double* qdot, const double* sens_x,
                            const int32_t* status, const int32_t* cert_status, int mem, const WbcTickGrad* out, void* stream) {
  const char* who = "wbc_tick_vjp";
  int rc = check_batch(b, B, who, true);
  if (rc) return rc;
  if (!out) return fail(WBC_E_ARG, "%s: out is required", who);
  if ((rc = check_dt(dt, who))) return rc;
  if (!qdot) return fail(WBC_E_ARG, "%s: qdot is required", who);
  if (!sens_x) return fail(WBC_E_ARG, "%s: sens_x is required", who);
  if ((rc = validate_tick_in(b, in, who))) return rc;
  if ((rc = check_outs(*out, TICK_OUT, Reads(b, false), who, true))) return rc;
  if ((rc = layers_fit(b, who))) return rc;
  HIP_TRY(hipSetDevice(b->device_id));
  WbcTickIn ti = *in;
  WbcTickGrad og = *out;
  Stager st{b, mem, (hipStream_t)stream, {}};
  stage_tick_in(st, ti, B, b);
  const size_t n = (size_t)B;
  st.in(&tp, n); st.in(&qdot, n * WBC_V_STRIDE); st.in(&sens_x, n * WBC_V_STRIDE); st.in(&status, n); st.in(&cert_status, n);
  stage_outs(st, og, TICK_OUT, n);
  st.out(&og.grad_status, n);
  if ((rc = st.stage())) return rc;
  if ((rc = tick_layer(b, B, dt, ti, tp, qdot, sens_x, status, cert_status, og, stream))) return rc;
  return st.finish();
}
extern "C" int wbc_tick_grad_sizes(int32_t* sizeof_grad) {
  if (sizeof_grad) *sizeof_grad = (int32_t)sizeof(WbcTickGrad);
  return WBC_OK;
}

// dL/dq (tangent coordinates) and dL/d trunk_box_center of solved ticks (include/wbc.h): argument checks, staging of host arrays, ONE launch of
// wbc_gradq_kernel (csrc/wbc_k_gradq.hip). No posture kernel: MANI / HYBRID need the caller's posture_u, which is held constant. No memset;
// the kernel writes every row of every output it is given.
static_assert(sizeof(WbcTickSens) == 8 * sizeof(void*) && sizeof(WbcTickStateGrad) == 3 * sizeof(void*), "wbc_capi.WbcTickSens / WbcTickStateGrad");
extern "C" int wbc_tick_vjp_state(WbcBatch* b, int B, const WbcTickIn* in, const WbcTaskParams* tp, double dt, const WbcTickSens* sens, int mem,
                                  const WbcTickStateGrad* out, void* stream) {
  const char* who = "wbc_tick_vjp_state";
  int rc = check_batch(b, B, who, true);
  if (rc) return rc;
  if (!out) return fail(WBC_E_ARG, "%s: out is required", who);
  if (!sens) return fail(WBC_E_ARG, "%s: sens is required", who);
  if ((rc = check_dt(dt, who))) return rc;
  if (!sens->qdot) return fail(WBC_E_ARG, "%s: qdot is required", who);
  if (!sens->sens_x) return fail(WBC_E_ARG, "%s: sens_x is required", who);
  if ((rc = validate_tick_in(b, in, who))) return rc;
  if (in->q_con) return fail(WBC_E_ARG, "%s: q_con is not supported (the constraints would see another configuration than the task rows)", who);
  for (int i = 0; i < b->n_models; ++i) {
    const int tj = b->cfg_host[i].task_joint;
    if ((tj == WBC_JOINT_MANI || tj == WBC_JOINT_HYBRID) && !in->posture_u)
      return fail(WBC_E_ARG, "%s: posture mode MANI / HYBRID of model %d needs posture_u (it is held constant)", who, i);
  }
  const Reads rd(b, false);
  const int p = rd.p;
  if (b->cfg_host[0].use_bounds && !sens->sens_bounds) return fail(WBC_E_ARG, "%s: sens_bounds is required with use_bounds", who);
  if (p > 0 && !sens->sens_rows) return fail(WBC_E_ARG, "%s: sens_rows is required with %d constraint rows", who, p);
  if (p > 0 && !sens->y_rows) return fail(WBC_E_ARG, "%s: y_rows is required with %d constraint rows", who, p);
  if ((rc = check_outs(*out, TICKQ_OUT, rd, who, true))) return rc;
  if ((rc = layers_fit(b, who))) return rc;
  HIP_TRY(hipSetDevice(b->device_id));
  WbcTickIn ti = *in;
  WbcTickSens sn = *sens;
  WbcTickStateGrad og = *out;
  Stager st{b, mem, (hipStream_t)stream, {}};
  stage_tick_in(st, ti, B, b);
  const size_t n = (size_t)B;
  st.in(&tp, n); st.in(&sn.qdot, n * WBC_V_STRIDE); st.in(&sn.sens_x, n * WBC_V_STRIDE); st.in(&sn.sens_bounds, n * WBC_V_STRIDE);
  st.in(&sn.sens_rows, n * p); st.in(&sn.y_rows, n * p); st.in(&sn.status, n); st.in(&sn.cert_status, n);
  st.in(&sn.working_set, n * 2);
  stage_outs(st, og, TICKQ_OUT, n);
  st.out(&og.grad_status, n);
  if ((rc = st.stage())) return rc;
  if ((rc = tickq_layer(b, B, dt, ti, tp, sn, og, stream))) return rc;
  return st.finish();
}
extern "C" int wbc_tick_state_grad_sizes(int32_t* sizeof_sens, int32_t* sizeof_grad) {
  if (sizeof_sens) *sizeof_sens = (int32_t)sizeof(WbcTickSens);
  if (sizeof_grad) *sizeof_grad = (int32_t)sizeof(WbcTickStateGrad);
  return WBC_OK;
}

// dL/d(q, qdot, foot_targets) of the state step between two ticks (include/wbc.h): argument checks, staging of host arrays, ONE launch of
// wbc_stepvjp_kernel (csrc/wbc_k_stepvjp.hip). No memset; the kernel writes every row of every output it is given.
static_assert(sizeof(WbcStepGrad) == 4 * sizeof(void*), "wbc_capi.WbcStepGrad");
extern "C" int wbc_step_vjp(WbcBatch* b, int B, const double* q_cur, const double* qdot, const double* foot_targets, const double* imu,
                            const int32_t* model_id, double dt, int mode, const double* g_q_new, int mem, const WbcStepGrad* out, void* stream) {
  const char* who = "wbc_step_vjp";
  int rc = check_batch(b, B, who, true);
  if (rc) return rc;
  if (!out) return fail(WBC_E_ARG, "%s: out is required", who);
  if (!q_cur) return fail(WBC_E_ARG, "%s: q_cur is required", who);
  if (!qdot) return fail(WBC_E_ARG, "%s: qdot is required", who);
  if (!foot_targets) return fail(WBC_E_ARG, "%s: foot_targets is required", who);
  if (!g_q_new) return fail(WBC_E_ARG, "%s: g_q_new is required", who);
  if (mode != WBC_ROLLOUT_RUNNING && mode != WBC_ROLLOUT_WARMUP)
    return fail(WBC_E_ARG, "%s: mode = %d, want WBC_ROLLOUT_RUNNING (%d) or WBC_ROLLOUT_WARMUP (%d)", who, mode, WBC_ROLLOUT_RUNNING, WBC_ROLLOUT_WARMUP);
  if ((rc = check_dt(dt, who))) return rc;
  if (b->n_models > 1 && !model_id) return fail(WBC_E_ARG, "%s: model_id is required with %d models", who, b->n_models);
  if ((rc = layers_fit(b, who))) return rc;
  HIP_TRY(hipSetDevice(b->device_id));
  WbcStepGrad og = *out;
  Stager st{b, mem, (hipStream_t)stream, {}};
  const size_t n = (size_t)B;
  st.in(&q_cur, n * WBC_Q_STRIDE); st.in(&qdot, n * WBC_V_STRIDE); st.in(&foot_targets, n * 15); st.in(&imu, n * 4);
  st.in(&model_id, n); st.in(&g_q_new, n * WBC_V_STRIDE);
  stage_outs(st, og, STEP_OUT, n);
  st.out(&og.grad_status, n);
  if ((rc = st.stage())) return rc;
  if ((rc = step_layer(b, B, dt, mode, q_cur, qdot, foot_targets, imu, model_id, g_q_new, og, stream))) return rc;
  return st.finish();
}
extern "C" int wbc_step_grad_sizes(int32_t* sizeof_grad) {
  if (sizeof_grad) *sizeof_grad = (int32_t)sizeof(WbcStepGrad);
  return WBC_OK;
}

extern "C" int wbc_integrate(WbcBatch* b, int B, const double* q, const double* v, const int32_t* model_id, double dt, int mem,
                             double* q_next, void* stream) {
  int rc = check_batch(b, B, "wbc_integrate", false);
  if (rc) return rc;
  if (!q || !v || !q_next) return fail(WBC_E_ARG, "wbc_integrate: null argument");
  if ((rc = check_dt(dt, "wbc_integrate", true))) return rc;      // (dt < 0: a step back)
  if (b->n_models > 1 && !model_id) return fail(WBC_E_ARG, "wbc_integrate: model_id is required with %d models", b->n_models);
  HIP_TRY(hipSetDevice(b->device_id));
  IntegrateArgs a;
  memset(&a, 0, sizeof a);
  a.models = b->d_models; a.B = B; a.n_models = b->n_models; a.dt = dt; a.q = q; a.v = v; a.model_id = model_id; a.q_next = q_next;
  Stager st{b, mem, (hipStream_t)stream, {}};
  st.in(&a.q, (size_t)B * WBC_Q_STRIDE); st.in(&a.v, (size_t)B * WBC_V_STRIDE); st.in(&a.model_id, (size_t)B);
  st.out(&a.q_next, (size_t)B * WBC_Q_STRIDE);
  if ((rc = st.stage())) return rc;
  if (int e = launch_integrate(a, grid_for(b, B), stream)) return fail(WBC_E_HIP, "integrate kernel launch failed: %s", hipGetErrorString((hipError_t)e));
  return st.finish();
}

extern "C" int wbc_debug_cycles(WbcBatch* b, uint64_t* out24) {
  if (!b || !out24) return fail(WBC_E_ARG, "wbc_debug_cycles: null argument");
  HIP_TRY(hipSetDevice(b->device_id));
  if (!b->d_prof) {   // first call arms the counters (they stay zero in non-profile builds)
    HIP_TRY(hipMalloc((void**)&b->d_prof, 24 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(b->d_prof, 0, 24 * sizeof(unsigned long long)));
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out24, b->d_prof, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(b->d_prof, 0, 24 * sizeof(unsigned long long)));
  return WBC_OK;
}

extern "C" const char* wbc_last_error(void) { return g_err; }
#ifdef WBC_PROFILE
extern "C" const char* wbc_version(void) { return "wbc-hip 0.1 (gfx950, PROFILE build)"; }
#else
extern "C" const char* wbc_version(void) { return "wbc-hip 0.1 (gfx950)"; }
#endif
extern "C" int wbc_variant_count(const char* family) {
  if (!family) return fail(WBC_E_ARG, "wbc_variant_count: null family");
  if (!strcmp(family, "general")) return general_variant_count();
  if (!strcmp(family, "sim3p")) return sim3p_variant_count();
  if (!strcmp(family, "orthp")) return orthp_variant_count();
  if (!strcmp(family, "boxp")) return boxp_variant_count();
  if (!strcmp(family, "qpp")) return qpp_variant_count();
  if (!strcmp(family, "qp")) return qp_variant_count();
  if (!strcmp(family, "grad")) return grad_variant_count();
  if (!strcmp(family, "gradq")) return gradq_variant_count();
  if (!strcmp(family, "stepvjp")) return stepvjp_variant_count();
  if (!strcmp(family, "rollvjp")) return rollvjp_variant_count();
  if (!strcmp(family, "trackvjp")) return trackvjp_variant_count();
  if (!strcmp(family, "scorevjp")) return scorevjp_variant_count();
  if (!strcmp(family, "slackvjp")) return slackvjp_variant_count();
  return fail(WBC_E_ARG, "wbc_variant_count: unknown kernel family %s", family);
}
extern "C" int wbc_abi_sizes(int32_t* sb, int32_t* sc) {
  if (sb) *sb = (int32_t)sizeof(WbcModelBlob);
  if (sc) *sc = (int32_t)sizeof(WbcConfig);
  return WBC_OK;
}
