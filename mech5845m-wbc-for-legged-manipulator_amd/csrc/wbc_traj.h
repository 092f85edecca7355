// wbc_traj.h — what the kernels of wbc_rollout_traj / wbc_rollout_tracks (wbc_k_traj.hip) consume, and their launchers (internal, C++). A
// header of its own: the tick / update kernels' translation units do not see it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/wbc.h"
#include "wbc_track.h"

namespace wbc {

constexpr int TRAJ_FRAMES = WBC_MAX_TRACKS;   // targets / frames 0..4: the end effectors, 5: the trunk

// The tracks of a call + the scores of the frames in `score_mask`. wbc_rollout_traj is the one-track call: a LINEAR track of end effector
// `ee`, the gripper scored, its position read from the update kernel's grip_trace row (reached_stride 3, reached_off[4] 0).
struct TrajArgs {
  int32_t B, ticks;
  int32_t n_tracks, do_sum;             // do_sum 1: the per-tick kernel accumulates the scores
  int32_t score_mask;                   // bit f: frame f is scored (n_scored = popcount, frames in increasing order)
  int32_t one_track;                    // 1: wbc_rollout_traj's call (wbc_traj_tick_kernel<true>)
  DevTrack tr[WBC_MAX_TRACKS];          // (wbc_track.h)
  double* ee_target;                    // the roll-out's [B][5][3] target block
  double* trunk_target;                 // the roll-out's [B][3] trunk target (null without one)
  const double* trunk_step;             // [B][3] added to trunk_target after the tick was scored (wbc_rollout_tracks without a trunk track), or null
  const double* reached;                // positions the update kernel of this tick wrote: frame f of instance b at [b * reached_stride + reached_off[f]]
  int32_t reached_stride, pad_;
  int32_t reached_off[TRAJ_FRAMES];
  double* trace;                        // [n_scored][B][3] of this tick (positions reached, scored frames in increasing order), or null
  const int32_t* status;                // [B] this tick's solver status
  int32_t* ro_status_max;               // the roll-out's status_max (bad rows get WBC_QP_NUMERICAL), or null
  // state in the handle's workspace; per-frame arrays are [n_scored][B]
  int32_t* bad;                         // 1: bad row (its followed targets stay where in0 put them)
  int32_t* bad_count;                   // [1] bad rows of the call
  double *err_sq_sum, *err_max, *err_final;
  int32_t *err_max_tick, *first_bad_tick, *bad_ticks, *status_max;
};

struct TrajGroupArgs {
  int32_t G, M, ticks, n_scored;        // G groups of M consecutive instances; per-frame arrays [n_scored][G * M] in, [n_scored][G] out
  const double *err_sq_sum, *err_max;
  const int32_t *status_max, *bad_ticks;
  double *group_rms, *group_err_max;    // each optional
  int32_t *group_worst_status, *group_bad_instances;
};

int launch_traj_begin(const TrajArgs& a, void* stream);            // bad-row check, summary reset, the targets of tick 0
int launch_traj_tick(const TrajArgs& a, int k, void* stream);      // after the update kernel of tick k: score it, write the targets of tick k + 1
int launch_traj_groups(const TrajGroupArgs& a, void* stream);      // one wavefront per group

}  // namespace wbc
