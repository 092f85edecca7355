// wbc_grad.h — what the kernel of wbc_tick_vjp (wbc_k_grad.hip) consumes, and its launcher (internal, C++). A header of its own, as
// wbc_traj.h, wbc_slack.h and wbc_cert.h: no other kernel's translation unit sees it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "wbc_device.h"

namespace wbc {

enum { GRAD_OK = 0, GRAD_UNSOLVED = 1, GRAD_CERT = 2, GRAD_NONFINITE = 3 };   // WBC_GRAD_* of include/wbc.h

// One launch gives dL/d(task weights, gains, targets) of every instance (include/wbc.h, wbc_tick_vjp). `in`: the fields the task rows
// read; a field the configuration does not read may be null. tp / status / cert_status may be null. Every output may be null.
// in.posture_u null under MANI / HYBRID: every sweep is structurally zero and u comes from DevPlan.post_zero, as in the tick kernels.
struct GradArgs {
  const DevModel* models;
  const WbcConfig* cfgs;
  const DevPlan* plans;
  int32_t B, n_models, rot, pad_;
  double dt;
  WbcTickIn in;
  const WbcTaskParams* tp;              // [B] rows, or null: the configuration's block
  const double *qdot, *sens_x;          // [B][26]
  const int32_t *status, *cert_status;  // [B]
  WbcTickGrad out;
};

int launch_grad(const GradArgs& a, void* stream, long long* key_out = nullptr);   // four instances per wavefront, grid = ceil(B / 4)
int grad_variant_count();

}  // namespace wbc
