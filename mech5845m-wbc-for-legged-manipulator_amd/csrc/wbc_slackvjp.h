// wbc_slackvjp.h — what the kernel of wbc_state_slack_vjp / wbc_rollout_vjp_watched (wbc_k_slackvjp.hip) consumes, and its launcher (internal,
// C++). A header of its own, as wbc_scorevjp.h: no other kernel's translation unit sees it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/wbc.h"
#include "wbc_device.h"
#include "wbc_slack.h"

namespace wbc {

// The cotangent of the slack families (include/wbc.h states the algebra), four instances per wavefront. The slack is evaluated by the forward's
// own inline functions (wbc_slack.h), so the component a family's cotangent goes to is the forward's `which`.
// Stage STATE (wbc_state_slack_vjp): gamma_i = g_comp[i] + [i == which[f]] g_slack[f]; d_q, d_box, which and grad_status are WRITTEN, every
//   row [0, B): a bad row (non-finite q / cotangent, non-finite box entry of a family with a non-zero cotangent) gets zeros and
//   WBC_GRAD_NONFINITE.
// Stage SEED (every tick k of wbc_rollout_vjp_watched, in front of the step layer): q is q_(k+1); the cotangent of watched family f is
//   g_trace[w][b] (this tick's block) + [k == K - 1] g_fin[w][b] + [k == min_tick[w][b]] g_min[w][b], w = popcount(mask below bit f);
//   g[b][d] += term and acc_box[b][i] += box term, an exact zero not added. The per-instance test of the tick (non-finite cotangent of the
//   tick, non-finite q, min_tick outside [0, K) under g_min != 0 — that one at k == K - 1 —, non-finite box entry of a seeded family):
//   worst[b] <- WBC_GRAD_NONFINITE (the link kernel then zeroes the instance's outputs at k == 0). Such an instance adds nothing.
enum { SLACKVJP_STATE = 0, SLACKVJP_SEED = 1 };
struct SlackVjpArgs {
  const DevModel* models;
  const WbcConfig* cfgs;
  const DevPlan* plans;
  const SlackLimits* lim;
  const int32_t* model_id;
  int32_t B, n_models, K, k, mask, rot;
  const double* q;                       // [B][27]
  const double* box;                     // [B][4] trunk_box_center, or null (families 1 and 2 then have no component to give a cotangent to)
  // STATE
  const double* g_slack;                 // [B][4], optional
  const double* g_comp;                  // [B][12], optional
  double* d_q;                           // [B][26]
  double* d_box;                         // [B][4]
  int32_t* which;                        // [B][4]
  int32_t* grad_status;                  // [B]
  // SEED
  const double *g_min, *g_fin, *g_trace; // [n_w][B] each (g_trace: tick k's block), each optional
  const int32_t* min_tick;               // [n_w][B] (with g_min)
  double* g;                             // [B][26] the carried cotangent
  double* acc_box;                       // [B][4] the sweep's d_trunk_box_center accumulator, or null (then the box term is dropped)
  int32_t* worst;                        // the link kernel's worst grad_status [B]
};
int launch_slackvjp(const SlackVjpArgs& a, int stage, void* stream, long long* key_out = nullptr);   // grid = ceil(B / 4)
int slackvjp_variant_count();

}  // namespace wbc
