// wbc_rollvjp.h — what the kernels of wbc_rollout_record / wbc_rollout_vjp's own translation unit (wbc_k_rollvjp.hip) consume, and their
// launchers (internal, C++). A header of its own, as wbc_stepvjp.h: no other kernel's translation unit sees it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "wbc_device.h"

namespace wbc {

// The tape's copies of one moment of a roll-out (wbc_rollout_record): up to TAPE_MAX_SEG blocks, each `words` 32-bit words per instance,
// row b of src to row b of dst, in one launch. A block with a null end is skipped.
enum { TAPE_MAX_SEG = 10 };
struct TapeSeg { const void* src; void* dst; int32_t words, pad_; };
struct TapeCopyArgs {
  int32_t B, n_seg;
  TapeSeg seg[TAPE_MAX_SEG];
};
int launch_tape_copy(const TapeCopyArgs& a, void* stream);   // grid-stride over B x (the widest block's words)

// The link between two layers of the reverse sweep (wbc_rollout_vjp; include/wbc.h states the algebra), four instances per wavefront.
// Stage BEGIN (once, before tick K - 1): accumulators <- 0, the unit rows on the padded columns of A (rows m .. m + pad_rows - 1, with b = 0),
//   g <- g_q_final + g_q_trace[K - 1].
// Stage ADDV (once, tick K - 1, g_qdot_last given): v += g_qdot_last.
// Stage LINK (every tick k, after the layers): g <- s_dq + t_dq (+ g_q_trace[k - 1]), accumulators += this tick's, the target bookkeeping's
//   adjoint; at k == 0 the caller's outputs. Every workspace pointer is strided by the call's rows alone: row b of each.
enum { ROLLVJP_BEGIN = 0, ROLLVJP_ADDV = 1, ROLLVJP_LINK = 2 };
struct RollVjpArgs {
  const DevModel* models;
  const int32_t* model_id;              // [B] or null
  int32_t B, n_models, k, K;
  int32_t m, pad_rows;                  // task rows of wbc_assemble; unit rows behind them
  uint32_t ee_on;                       // bit e: end effector e's task is on
  int32_t trunk_on;
  // seeds (null: zero)
  const double *g_q_final, *g_qdot_last, *g_q_trace;   // [B][26], [B][26], [K][B][26]
  // the QP image the padding rows go into
  double *A, *b;                                       // [B][m + pad_rows][26], [B][m + pad_rows]
  // the carried cotangent and the certificate's v
  double *g, *v;                                       // [B][26]
  // this tick's layer outputs (LINK; null: zero)
  const double *s_dq, *s_dft, *t_dq, *t_box;           // step d_q [B][26], step d_foot_targets [B][15], tick-state d_q [B][26], d_trunk_box_center [B][4]
  WbcTickGrad t;                                       // wbc_grad_kernel's outputs of this tick (read)
  const int32_t *gs_step, *gs_tickq;                   // the layers' grad_status (t.grad_status: the tick gradient's)
  // accumulators (workspace)
  double *Ebar, *Pbar, *TEbar, *TPbar, *d_estep, *d_tstep, *acc_tp, *acc_com, *acc_comv, *acc_pu, *acc_box;
  int32_t *worst, *dropped;
  WbcRolloutGrad out;                                  // the caller's, written by LINK at k == 0
};
int launch_rollvjp(const RollVjpArgs& a, int stage, void* stream, long long* key_out = nullptr);   // grid = ceil(B / 4)
int rollvjp_variant_count();

}  // namespace wbc
