// wbc_gradq.h — what the kernel of wbc_tick_vjp_state (wbc_k_gradq.hip) consumes, and its launcher (internal, C++). A header of its own, as
// wbc_grad.h: no other kernel's translation unit sees it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "wbc_device.h"

namespace wbc {

// One launch gives dL/dq (tangent coordinates) and dL/d trunk_box_center of every instance (include/wbc.h, wbc_tick_vjp_state). `in`: the
// fields the tick reads (q_con refused by the caller); tp may be null; sens.* as WbcTickSens says; every output may be null.
struct GradQArgs {
  const DevModel* models;
  const WbcConfig* cfgs;
  const DevPlan* plans;
  int32_t B, n_models, rot, pad_;
  double dt;
  WbcTickIn in;
  const WbcTaskParams* tp;              // [B] rows, or null: the configuration's block
  WbcTickSens sens;
  WbcTickStateGrad out;
};

int launch_gradq(const GradQArgs& a, void* stream, long long* key_out = nullptr);   // four instances per wavefront, grid = ceil(B / 4)
int gradq_variant_count();

}  // namespace wbc
