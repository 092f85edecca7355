// wbc_scorevjp.h — what the kernels of wbc_rollout_vjp_scored's own translation unit (wbc_k_scorevjp.hip) consume, and their launcher
// (internal, C++). A header of its own, as wbc_trackvjp.h: no other kernel's translation unit sees it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/wbc.h"
#include "wbc_device.h"

namespace wbc {

// The cotangent of the track scores (include/wbc.h states the algebra), four instances per wavefront.
// Stage SEED (every tick k, in front of the step layer): whole-tree FK at q_(k+1) (the tape's q of tick k + 1, q_final for k == K - 1), the
//   scored frames' d = reached - target of tick k, c = (2 g_sq + [k == K - 1] g_fin / e + [k == err_max_tick] g_max / e) d, then
//   g += sum_f J_f' c_f on the lanes of the DoF (two per lane, the frames in increasing order) and stash[b][f][:] <- -c_f (0 for an unscored
//   frame). At k == K - 1 also the per-instance test: a non-finite g_err_* / q_final entry, or err_max_tick outside [0, K) with g_err_max
//   != 0, gives worst[b] <- WBC_GRAD_NONFINITE (the link kernel then zeroes the instance's outputs at k == 0). Such an instance adds nothing.
// Stage TARGET (every tick k, between LINK and the track stage): Ebar / TEbar += stash, one lane per (instance, frame, component); at k == 0
//   the caller's d_ee_target / d_trunk_target += stash as well (LINK has just written them).
enum { SCOREVJP_SEED = 0, SCOREVJP_TARGET = 1 };
struct ScoreVjpArgs {
  const DevModel* models;
  const DevPlan* plans;
  const int32_t* model_id;
  int32_t B, n_models, K, k, score_mask, rot;
  const double* q;                       // [B][27] q_(k+1)
  const double *ee_target, *trunk_target; // [B][15], [B][3]: the targets tick k saw (trunk_target: null without score bit 5)
  const double *g_sq, *g_fin, *g_max;     // [n_scored][B], each optional
  const int32_t* err_max_tick;            // [n_scored][B] (with g_max)
  double* g;                             // [B][26] the carried cotangent
  double* stash;                         // [B][6][3]
  int32_t* worst;                        // the link kernel's worst grad_status [B]
  double *Ebar, *TEbar;                  // the link kernel's carried target cotangents [B][15], [B][3]
  double *d_ee_target, *d_trunk_target;  // the caller's outputs (TARGET at k == 0), each optional
};
int launch_scorevjp(const ScoreVjpArgs& a, int stage, void* stream, long long* key_out = nullptr);   // grid = ceil(B / 4)
int scorevjp_variant_count();

}  // namespace wbc
