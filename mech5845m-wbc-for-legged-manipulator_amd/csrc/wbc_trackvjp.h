// wbc_trackvjp.h — what the kernels of wbc_rollout_vjp_tracks' own translation unit (wbc_k_trackvjp.hip) consume, and their launcher
// (internal, C++). A header of its own, as wbc_rollvjp.h: no other kernel's translation unit sees it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/wbc.h"
#include "wbc_track.h"

namespace wbc {

// The adjoint of the track evaluation (include/wbc.h states the algebra), four instances per wavefront, one lane per (instance, track,
// component): tracks 0..4 in a first pass, track 5 in a second.
// Stage BEGIN (once, behind the link kernel's BEGIN): the bad-row test of wbc_traj_begin_kernel; a bad row's worst[b] <- WBC_GRAD_NONFINITE
//   (the link kernel then zeroes the instance's outputs at k == 0); the track outputs <- 0.
// Stage TICK (every tick k, directly behind LINK): e = the followed rows of Ebar / TEbar (LINK has just made them e_k), the adjoint of
//   eval_b(k * du_b) into the track outputs, the followed rows <- 0; at k == 0 the followed rows of the caller's d_ee_target / d_trunk_target
//   <- 0 and the all-zero rule on the track outputs.
enum { TRACKVJP_BEGIN = 0, TRACKVJP_TICK = 1 };
struct TrackVjpTrack : DevTrack {       // the followed track (wbc_track.h), then its outputs
  double *d_points, *d_tangents, *d_du; // the caller's (or the staged) outputs, each optional: the accumulators live in them
};
static_assert(sizeof(TrackVjpTrack) == sizeof(DevTrack) + 3 * sizeof(double*) && sizeof(DevTrack) == 56, "the outputs directly behind the nine shared fields");
struct TrackVjpArgs {
  int32_t B, k, n_tracks, pad_;
  TrackVjpTrack tr[WBC_MAX_TRACKS];
  double *Ebar, *TEbar;                 // the link kernel's carried target cotangents [B][15], [B][3]
  int32_t* worst;                       // the link kernel's worst grad_status [B]
  double *d_ee_target, *d_trunk_target; // the caller's outputs (TICK at k == 0: followed rows <- 0), each optional
};
int launch_trackvjp(const TrackVjpArgs& a, int stage, void* stream, long long* key_out = nullptr);   // grid = ceil(B / 4)
int trackvjp_variant_count();

}  // namespace wbc
