// wbc_k_rollvjp.hip — wbc_rollout_record / wbc_rollout_vjp: the kernels between the layers (include/wbc.h). The layers
// themselves are the existing kernels, unchanged: wbc_stepvjp_kernel, the general kernel's assemble mode, wbc_qp_cert_kernel, wbc_grad_kernel,
// wbc_gradq_kernel. Here:
//   wbc_tape_copy_kernel   the forward's tape: up to TAPE_MAX_SEG row blocks copied in one launch per tick
//   wbc_rollvjp_kernel     the reverse sweep's per-instance algebra, four instances per wavefront (lane = 16 r + s), a stage per row of the table:
//     BEGIN  accumulators <- 0; the unit rows on a model's padded columns behind the task rows of A; g <- g_q_final + g_q_trace[K - 1]
//     ADDV   v += g_qdot_last (tick K - 1)
//     LINK   g <- step.d_q + tickstate.d_q (+ g_q_trace[k - 1]): both tangent at q_k, no raw coordinates anywhere; the accumulators += this
//            tick's; the adjoint of the target bookkeeping
//                d_step += Ebar;  Ebar <- Ebar + a_k + on o Pbar;  Pbar <- p_k + (1 - on) o Pbar
//            with a_k = tick.d_ee_target + step.d_foot_targets, p_k = tick.d_prev_ee_target (the trunk pair: the same under task_trunk); at
//            k == 0 the caller's outputs.
// A tick whose layer reported a grad_status counts as dropped: its tick-layer terms are taken as zero (the layers wrote zero rows), what the
// step gave flows on. An instance with WBC_GRAD_NONFINITE anywhere gets all-zero outputs. Everything is elementwise within the instance's 16
// lanes: no cross-lane traffic at all. Rows >= B are never written.
#include <hip/hip_runtime.h>
#include "wbc_packed.h"
#include "wbc_grad.h"
#include "wbc_rollvjp.h"

namespace wbc {

__global__ void __launch_bounds__(256) wbc_tape_copy_kernel(const TapeCopyArgs A) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int i = 0; i < A.n_seg; ++i) {
    const TapeSeg sg = A.seg[i];
    if (!sg.src || !sg.dst) continue;
    const uint32_t* src = (const uint32_t*)sg.src;
    uint32_t* dst = (uint32_t*)sg.dst;
    const size_t total = (size_t)A.B * (size_t)sg.words;
    for (size_t j = first; j < total; j += stride) dst[j] = src[j];
  }
}

int launch_tape_copy(const TapeCopyArgs& a, void* stream) {
  int widest = 1;
  for (int i = 0; i < a.n_seg; ++i) if (a.seg[i].words > widest) widest = a.seg[i].words;
  const size_t total = (size_t)a.B * (size_t)widest;
  size_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(wbc_tape_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("tape copy");
}

__device__ __forceinline__ double rv_get(const double* p, size_t i) { return p ? p[i] : 0.0; }

template <int STAGE>
__global__ void __launch_bounds__(64) wbc_rollvjp_kernel(const RollVjpArgs A) {
  const int lane = threadIdx.x, r = lane >> 4, s = lane & 15;
  const int b_raw = 4 * blockIdx.x + r;
  if (b_raw >= A.B) return;                                         // (no cross-lane traffic below: a lane may leave)
  const size_t b = (size_t)b_raw, nB = (size_t)A.B;
  if (STAGE == ROLLVJP_ADDV) {
    for (int i = s; i < NV; i += 16) A.v[b * NV + i] += A.g_qdot_last[b * NV + i];
    return;
  }
  if (STAGE == ROLLVJP_BEGIN) {
    int mid = 0;
    if (A.model_id) { mid = A.model_id[b]; mid = mid < 0 ? 0 : (mid >= A.n_models ? A.n_models - 1 : mid); }
    const int nv = A.models[mid].nv;
    const int rows = A.m + A.pad_rows;
    for (int j = 0; j < A.pad_rows; ++j) {                          // e_c on column c = nv + j (WbcBatch._padding_rows): none when c >= 26
      for (int c = s; c < NV; c += 16) A.A[(b * rows + A.m + j) * NV + c] = (c == nv + j) ? 1.0 : 0.0;
      if (s == 0) A.b[b * rows + A.m + j] = 0.0;
    }
    const double* tr = A.g_q_trace ? A.g_q_trace + (size_t)(A.K - 1) * nB * NV : nullptr;
    for (int i = s; i < NV; i += 16) A.g[b * NV + i] = rv_get(A.g_q_final, b * NV + i) + rv_get(tr, b * NV + i);
    if (s < 15) { A.Ebar[b * 15 + s] = 0.0; A.Pbar[b * 15 + s] = 0.0; A.d_estep[b * 15 + s] = 0.0; }
    if (s < 3) { A.TEbar[b * 3 + s] = 0.0; A.TPbar[b * 3 + s] = 0.0; A.d_tstep[b * 3 + s] = 0.0; A.acc_com[b * 3 + s] = 0.0; A.acc_comv[b * 3 + s] = 0.0; }
    if (s < 4) A.acc_box[b * 4 + s] = 0.0;
    for (int i = s; i < NV; i += 16) A.acc_pu[b * NV + i] = 0.0;
    for (int i = s; i < WBC_TASK_PARAMS_DOUBLES; i += 16) A.acc_tp[b * WBC_TASK_PARAMS_DOUBLES + i] = 0.0;
    if (s == 0) { A.worst[b] = 0; A.dropped[b] = 0; }
    return;
  }
  // ---- LINK
  const int gs_s = A.gs_step ? A.gs_step[b] : 0, gs_q = A.gs_tickq ? A.gs_tickq[b] : 0, gs_t = A.t.grad_status ? A.t.grad_status[b] : 0;
  const bool tick_bad = gs_q != 0 || gs_t != 0;
  const double tm = tick_bad ? 0.0 : 1.0;                           // (the layers' rows of a dropped tick are zero already: the product keeps them so)
  int worst = A.worst[b];
  worst = gs_s > worst ? gs_s : worst; worst = gs_q > worst ? gs_q : worst; worst = gs_t > worst ? gs_t : worst;
  const int dropped = A.dropped[b] + (tick_bad ? 1 : 0);
  const bool last = A.k == 0;
  const bool zero = last && worst == GRAD_NONFINITE;
  const double* tr = (A.g_q_trace && A.k > 0) ? A.g_q_trace + (size_t)(A.k - 1) * nB * NV : nullptr;
  for (int i = s; i < NV; i += 16) {
    double gn = A.s_dq[b * NV + i] + (tick_bad ? 0.0 : rv_get(A.t_dq, b * NV + i));
    if (tr) gn += tr[b * NV + i];
    A.g[b * NV + i] = gn;
    if (last && A.out.d_q0) A.out.d_q0[b * NV + i] = zero ? 0.0 : gn;
    const double pu = A.acc_pu[b * NV + i] + tm * rv_get(A.t.d_posture_u, b * NV + i);
    A.acc_pu[b * NV + i] = pu;
    if (last && A.out.d_posture_u) A.out.d_posture_u[b * NV + i] = zero ? 0.0 : pu;
  }
  for (int i = s; i < WBC_TASK_PARAMS_DOUBLES; i += 16) {
    const size_t o = b * WBC_TASK_PARAMS_DOUBLES + i;
    const double x = A.acc_tp[o] + tm * rv_get(A.t.d_task_params, o);
    A.acc_tp[o] = x;
    if (last && A.out.d_task_params) A.out.d_task_params[o] = zero ? 0.0 : x;
  }
  if (s < 15) {
    const size_t o = b * 15 + s;
    const bool on = (A.ee_on >> (s / 3)) & 1u;
    const double a = tm * rv_get(A.t.d_ee_target, o) + rv_get(A.s_dft, o), p = tm * rv_get(A.t.d_prev_ee_target, o);
    const double E = A.Ebar[o], P = A.Pbar[o];
    const double st = A.d_estep[o] + E, En = E + a + (on ? P : 0.0), Pn = p + (on ? 0.0 : P);
    A.d_estep[o] = st; A.Ebar[o] = En; A.Pbar[o] = Pn;
    if (last) {
      if (A.out.d_ee_target) A.out.d_ee_target[o] = zero ? 0.0 : En;
      if (A.out.d_prev_ee_target) A.out.d_prev_ee_target[o] = zero ? 0.0 : Pn;
      if (A.out.d_ee_target_step) A.out.d_ee_target_step[o] = zero ? 0.0 : st;
    }
  }
  if (s < 3) {
    const size_t o = b * 3 + s;
    const bool on = A.trunk_on != 0;
    const double a = tm * rv_get(A.t.d_trunk_target, o), p = tm * rv_get(A.t.d_prev_trunk_target, o);
    const double E = A.TEbar[o], P = A.TPbar[o];
    const double st = A.d_tstep[o] + E, En = E + a + (on ? P : 0.0), Pn = p + (on ? 0.0 : P);
    A.d_tstep[o] = st; A.TEbar[o] = En; A.TPbar[o] = Pn;
    const double c = A.acc_com[o] + tm * rv_get(A.t.d_com_target, o), cv = A.acc_comv[o] + tm * rv_get(A.t.d_com_target_vel, o);
    A.acc_com[o] = c; A.acc_comv[o] = cv;
    if (last) {
      if (A.out.d_trunk_target) A.out.d_trunk_target[o] = zero ? 0.0 : En;
      if (A.out.d_prev_trunk_target) A.out.d_prev_trunk_target[o] = zero ? 0.0 : Pn;
      if (A.out.d_trunk_target_step) A.out.d_trunk_target_step[o] = zero ? 0.0 : st;
      if (A.out.d_com_target) A.out.d_com_target[o] = zero ? 0.0 : c;
      if (A.out.d_com_target_vel) A.out.d_com_target_vel[o] = zero ? 0.0 : cv;
    }
  }
  if (s < 4) {
    const size_t o = b * 4 + s;
    const double x = A.acc_box[o] + tm * rv_get(A.t_box, o);
    A.acc_box[o] = x;
    if (last && A.out.d_trunk_box_center) A.out.d_trunk_box_center[o] = zero ? 0.0 : x;
  }
  if (s == 0) {
    A.worst[b] = worst; A.dropped[b] = dropped;
    if (last && A.out.grad_status) A.out.grad_status[b] = worst;
    if (last && A.out.ticks_dropped) A.out.ticks_dropped[b] = dropped;
  }
}

// The variants (wbc_common.h, "Kernel variant tables"): the part that instantiates the row, then the template arguments.
#ifndef ROLLVJP_PART
#define ROLLVJP_PART -1      // -1: everything in one unit
#endif
#define WBC_PART ROLLVJP_PART
#define WBC_KERNEL wbc_rollvjp_kernel
#define WBC_KPARAMS (const RollVjpArgs)
typedef void (*RollVjpKernel) WBC_KPARAMS;
#define ROLLVJP_VARIANTS(V) /* STAGE */ \
  V(0, ROLLVJP_BEGIN) \
  V(0, ROLLVJP_ADDV) \
  V(0, ROLLVJP_LINK)
#if ROLLVJP_PART == -1
ROLLVJP_VARIANTS(WBC_VARIANT_INST)
#else
ROLLVJP_VARIANTS(WBC_VARIANT_UNIT)
#endif
#if ROLLVJP_PART <= 0
static RollVjpKernel rollvjp_variant(long long key) {
  ROLLVJP_VARIANTS(WBC_VARIANT_FIND)
  return nullptr;
}
int rollvjp_variant_count() { return 0 ROLLVJP_VARIANTS(WBC_VARIANT_COUNT); }
int launch_rollvjp(const RollVjpArgs& a, int stage, void* stream, long long* key_out) {
  const long long key = variant_key(stage);
  if (key_out) *key_out = key;
  const RollVjpKernel k = rollvjp_variant(key);
  if (!k) return WBC_E_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3((a.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, a);
  return check_launch("rollout_vjp");
}
#endif

}  // namespace wbc
