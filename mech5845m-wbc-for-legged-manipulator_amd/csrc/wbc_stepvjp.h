// wbc_stepvjp.h — what the kernel of wbc_step_vjp (wbc_k_stepvjp.hip) consumes, and its launcher (internal, C++). A header of its own, as
// wbc_gradq.h: no other kernel's translation unit sees it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "wbc_device.h"

namespace wbc {

// One launch gives dL/d(q_cur, qdot, foot_targets) of every instance's state step (include/wbc.h, wbc_step_vjp). imu and model_id may be
// null; every output may be null. The kernel reads no configuration: the step has no switches.
struct StepVjpArgs {
  const DevModel* models;
  const DevPlan* plans;
  int32_t B, n_models, rot, mode;       // mode: WBC_ROLLOUT_RUNNING / WBC_ROLLOUT_WARMUP
  double dt;
  const double* q_cur;                  // [B][27]
  const double* qdot;                   // [B][26]
  const double* foot_targets;           // [B][5][3] (RUNNING: rows 0..3 are checked for non-finite values; their values do not enter)
  const double* imu;                    // [B][4] or null
  const int32_t* model_id;              // [B] or null
  const double* g;                      // [B][26] dL/d delta_new
  WbcStepGrad out;
};

int launch_stepvjp(const StepVjpArgs& a, void* stream, long long* key_out = nullptr);   // four instances per wavefront, grid = ceil(B / 4)
int stepvjp_variant_count();

}  // namespace wbc
