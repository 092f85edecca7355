// wbc_slack.h — what the kernels of wbc_state_slack / wbc_rollout_watch (wbc_k_slack.hip) consume, and their launchers (internal, C++). A
// header of its own, as wbc_traj.h: the tick / update / trajectory kernels' translation units do not see it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "wbc_device.h"

namespace wbc {

constexpr int SLACK_NF = WBC_N_SLACK;          // families: CoM box, trunk z, trunk angles, joint range
constexpr int SLACK_NC = 12;                   // components of families 0..2 in code order: 4 + 2 + 6

// The model's own position range by velocity DoF (WbcModelBlob.q_lo / q_hi of the DoF's own joint): DoF d looks at q[qi[d]]. One per model
// of the handle, built on first use (the range is the model's, not the configuration's; cfg.lock_from bounds the DoF that count).
struct SlackLimits {
  double lo[NL], hi[NL];
  int32_t qi[NL];
};

// One launch evaluates the four families at q for every instance. `slack` / `which` / `components`: the row outputs of wbc_state_slack
// (each may be null). `mask` != 0: the roll-out's watch — lane s < 4 of an instance's row folds family s (if watched) of tick k into row
// w = popcount(mask below bit s) of the accumulators, [n_w][B] each; tick 0 initialises them, so no reset launch precedes it.
struct SlackArgs {
  const DevModel* models;
  const WbcConfig* cfgs;
  const DevPlan* plans;
  const SlackLimits* lim;
  int32_t B, n_models, rot, k;
  const double* q;                      // [B][27]
  const double* box;                    // [B][4] trunk_box_center, or null: families 1 and 2 are NaN / -1
  const int32_t* model_id;
  double* slack;                        // [B][4]
  int32_t* which;                       // [B][4]
  double* components;                   // [B][12]
  int32_t mask, pad_;
  double *slack_min, *slack_final;      // [n_w][B]
  int32_t *min_tick, *min_which, *neg_ticks, *first_neg;
  double* trace;                        // [n_w][B] of this tick, or null
};

struct SlackGroupArgs {
  int32_t G, M, n_w, pad_;              // G groups of M consecutive instances; [n_w][G * M] in, [n_w][G] out
  const double* slack_min;
  const int32_t* neg_ticks;
  double* group_min;                    // each optional
  int32_t* group_neg_instances;
};

int launch_slack(const SlackArgs& a, void* stream);               // four instances per wavefront, grid = ceil(B / 4)
int launch_slack_groups(const SlackGroupArgs& a, void* stream);   // one wavefront per group

}  // namespace wbc
