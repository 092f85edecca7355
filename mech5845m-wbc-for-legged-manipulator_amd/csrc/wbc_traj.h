// wbc_traj.h — what wbc_rollout_traj's kernels (wbc_k_traj.hip) consume, and their launchers (internal, C++). A header of its own: the
// tick / update kernels' translation units do not see it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/wbc.h"

namespace wbc {

// Per-instance milestone trajectory of one end effector + the roll-out summary it is scored by. Every array is [B] (points: [B][S][3]).
struct TrajArgs {
  int32_t B, S, ee, ticks;
  int32_t do_sum, pad_;                 // 1: the per-tick kernel accumulates the summary
  const double* points;                 // [B][S][3]
  const int32_t* n_points;              // null => S
  const double* du;                     // null => du_all
  double du_all;
  double* ee_target;                    // the roll-out's [B][5][3] target block: rows `ee` are written, row 4 (gripper) is read
  const double* grip;                   // [B][3] gripper position the update kernel of this tick wrote
  const int32_t* status;                // [B] this tick's solver status
  int32_t* ro_status_max;               // the roll-out's status_max (bad rows get WBC_QP_NUMERICAL), or null
  // state in the handle's workspace
  int32_t* bad;                         // 1: bad row (the followed target stays where in0 put it)
  int32_t* bad_count;                   // [1] bad rows of the call
  double *err_sq_sum, *err_max, *err_final;
  int32_t *err_max_tick, *first_bad_tick, *bad_ticks, *status_max;
};

struct TrajGroupArgs {
  int32_t G, M, ticks, pad_;            // G groups of M consecutive instances
  const double *err_sq_sum, *err_max;
  const int32_t *status_max, *bad_ticks;
  double *group_rms, *group_err_max;    // outputs [G], each optional
  int32_t *group_worst_status, *group_bad_instances;
};

int launch_traj_begin(const TrajArgs& a, void* stream);            // bad-row check, summary reset, the target of tick 0
int launch_traj_tick(const TrajArgs& a, int k, void* stream);      // after the update kernel of tick k: score it, write the target of tick k + 1
int launch_traj_groups(const TrajGroupArgs& a, void* stream);      // one wavefront per group

}  // namespace wbc
