// wbc_k_trackvjp.hip — wbc_rollout_vjp_tracks: the adjoint of the track evaluation of wbc_k_traj.hip (include/wbc.h states
// the algebra). The sweep is wbc_rollout_vjp's, kernel for kernel; behind the link kernel's BEGIN and behind every LINK it launches one stage of
//   wbc_trackvjp_kernel    four instances per wavefront (lane = 16 r + s), one lane per (instance, track, component): s = 3 j + c for the
//                          tracks j = 0..4 in a first pass, s = c for track 5 in a second
//     BEGIN  the bad-row test wbc_traj_begin_kernel runs (wbc_track.h's; lane s == 0): a bad row's worst[b] <- WBC_GRAD_NONFINITE, so the
//            unchanged LINK zeroes that instance's outputs at k == 0; the track outputs <- 0
//     TICK   e <- the followed row of Ebar / TEbar (LINK has just made it e_k = a_k + on o Pbar), that row <- 0 (nothing is carried: the
//            target of every tick comes from the track); the adjoint of eval_b(k * du_b) applied to e; at k == 0 the followed rows of the
//            caller's d_ee_target / d_trunk_target <- 0 and all-zero track outputs for an instance with WBC_GRAD_NONFINITE
// The accumulators are the outputs themselves. Every d_points / d_tangents entry belongs to one lane, which adds to it in reverse tick order;
// d_du's three components meet in the lane of component 0 as (x + y) + z. No atomics, no LDS; the forward's comparisons select the branch
// (wbc_track.h: one bad-row test, one default-tangent rule, one segment lookup and one Hermite basis for both kernels) and nothing is
// contracted into fused multiply-adds, so the host restatement (wbc_workload.track_target_gradients) runs the same operations.
// Rows >= B are never written.
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_grad.h"
#include "wbc_trackvjp.h"

#pragma clang fp contract(off)

namespace wbc {

// the adjoint of wbc_track.h's default tangent at milestone i: vb, the cotangent of that tangent, into d (the instance's d_points at this
// component, stride 3) through the branch tangent_case takes: the plus term first
__device__ __forceinline__ void tv_tangent_adj(const double* __restrict__ m, double* __restrict__ d, int n, int i, double vb) {
  if (n == 2) { d[3] = d[3] + vb; d[0] = d[0] - vb; return; }
  if (i == 0 || i == n - 1) return;
  const double a = m[3 * (i - 1)], x = m[3 * i], b = m[3 * (i + 1)];
  double w;
  switch (tangent_case(a, x, b, w)) {
    case 1: return;
    case 2: d[3 * i] = d[3 * i] + 3.0 * vb; d[3 * (i - 1)] = d[3 * (i - 1)] - 3.0 * vb; return;
    case 3: d[3 * (i + 1)] = d[3 * (i + 1)] + 3.0 * vb; d[3 * i] = d[3 * i] - 3.0 * vb; return;
    default: d[3 * (i + 1)] = d[3 * (i + 1)] + 0.5 * vb; d[3 * (i - 1)] = d[3 * (i - 1)] - 0.5 * vb; return;
  }
}

template <int STAGE>
__global__ void __launch_bounds__(64) wbc_trackvjp_kernel(const TrackVjpArgs A) {
  const int lane = threadIdx.x, r = lane >> 4, s = lane & 15;
  const int b_raw = 4 * blockIdx.x + r;
  if (b_raw >= A.B) return;                                         // (the shuffle below stays within an instance's 16 lanes: a whole instance leaves)
  const size_t b = (size_t)b_raw;
  if (STAGE == TRACKVJP_BEGIN && s == 0) {                          // wbc_traj_begin_kernel's test, one lane per instance
    bool bad = false;
#pragma unroll 1
    for (int j = 0; j < A.n_tracks; ++j) bad |= track_bad(A.tr[j], b);
    if (bad) A.worst[b] = GRAD_NONFINITE;
  }
  const int dead = STAGE == TRACKVJP_TICK ? (A.worst[b] == GRAD_NONFINITE) : 0;   // a bad row, or a layer's non-finite: nothing is accumulated
  const bool last = A.k == 0;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1 && A.n_tracks <= 5) break;
    const int j = pass == 0 ? s / 3 : 5, c = pass == 0 ? s % 3 : s;
    const bool mine = (pass == 0 ? s < 15 : s < 3) && j < A.n_tracks;
    const TrackVjpTrack& T = A.tr[mine ? j : 0];
    const size_t row = b * (size_t)T.S * 3 + c;                     // component c of milestone 0
    double* dp = T.d_points ? T.d_points + row : nullptr;
    double* dt = T.d_tangents ? T.d_tangents + row : nullptr;
    if (STAGE == TRACKVJP_BEGIN) {
      if (!mine) continue;
      for (int i = 0; i < T.S; ++i) {
        if (dp) dp[3 * i] = 0.0;
        if (dt) dt[3 * i] = 0.0;
      }
      if (c == 0 && T.d_du) T.d_du[b] = 0.0;
      continue;
    }
    // ---- TICK
    double x = 0.0;                                                 // this component's term of d(loss)/d(t)
    if (mine) {
      double* eb = T.target == WBC_TARGET_TRUNK ? A.TEbar + b * 3 + c : A.Ebar + b * 15 + 3 * T.target + c;
      const double e = *eb;
      *eb = 0.0;
      if (last) {
        if (T.target == WBC_TARGET_TRUNK) { if (A.d_trunk_target) A.d_trunk_target[b * 3 + c] = 0.0; }
        else if (A.d_ee_target) A.d_ee_target[b * 15 + 3 * T.target + c] = 0.0;
      }
      if (!dead) {                                                  // (n, du and the milestones passed BEGIN's test)
        const int n = T.n_points ? T.n_points[b] : T.S;             // (track_n / track_du spelled out: through the calls this stage takes 76
        const double du = T.du ? T.du[b] : T.du_all;                //  VGPRs instead of 72, one wave per SIMD less; tools/kernel_resources.py)
        const double* m = T.points + row;
        const TrackSeg sg = track_segment((double)A.k * du, n);
        if (sg.where == SEG_FIRST) {
          if (dp) dp[0] = dp[0] + e;
        } else if (sg.where == SEG_LAST) {
          if (dp) dp[3 * (n - 1)] = dp[3 * (n - 1)] + e;
        } else {
          const int i = sg.i;                                       // 0 <= i <= n - 2 here
          const double u = sg.u;
          const double m0 = m[3 * i], m1 = m[3 * i + 3];
          if (T.kind != WBC_TRACK_HERMITE) {
            if (dp) { dp[3 * i] = dp[3 * i] + (1.0 - u) * e; dp[3 * i + 3] = dp[3 * i + 3] + u * e; }
            x = (m1 - m0) * e;
          } else {
            const double u2 = u * u;
            const HermiteBasis h = hermite_basis(u);
            const double* v = T.tangents ? T.tangents + row : nullptr;
            const double v0 = v ? v[3 * i] : track_tangent(m, n, i), v1 = v ? v[3 * i + 3] : track_tangent(m, n, i + 1);
            const double dx1 = 6.0 * u2 - 6.0 * u, dx2 = (-6.0 * u2) + 6.0 * u, dv1 = (3.0 * u2 - 4.0 * u) + 1.0, dv2 = 3.0 * u2 - 2.0 * u;
            x = (((dx1 * m0 + dx2 * m1) + dv1 * v0) + dv2 * v1) * e;
            if (dp) { dp[3 * i] = dp[3 * i] + h.cx1 * e; dp[3 * i + 3] = dp[3 * i + 3] + h.cx2 * e; }
            const double vb0 = h.cv1 * e, vb1 = h.cv2 * e;
            if (v) {
              if (dt) { dt[3 * i] = dt[3 * i] + vb0; dt[3 * i + 3] = dt[3 * i + 3] + vb1; }
            } else if (dp) {
              tv_tangent_adj(m, dp, n, i, vb0);
              tv_tangent_adj(m, dp, n, i + 1, vb1);
            }
          }
        }
      }
    }
    const double y = __shfl_down(x, 1), z = __shfl_down(x, 2);     // components 1 and 2 of the same track: lanes s + 1, s + 2 of the instance
    if (mine && c == 0 && T.d_du) {
      if (!dead) T.d_du[b] = T.d_du[b] + (double)A.k * ((x + y) + z);
      if (last && dead) T.d_du[b] = 0.0;
    }
    if (mine && last && dead) {
      for (int i = 0; i < T.S; ++i) {
        if (dp) dp[3 * i] = 0.0;
        if (dt) dt[3 * i] = 0.0;
      }
    }
  }
}

// The variants (wbc_common.h, "Kernel variant tables"): the part that instantiates the row, then the template arguments.
#ifndef TRACKVJP_PART
#define TRACKVJP_PART -1      // -1: everything in one unit
#endif
#define WBC_PART TRACKVJP_PART
#define WBC_KERNEL wbc_trackvjp_kernel
#define WBC_KPARAMS (const TrackVjpArgs)
typedef void (*TrackVjpKernel) WBC_KPARAMS;
#define TRACKVJP_VARIANTS(V) /* STAGE */ \
  V(0, TRACKVJP_BEGIN) \
  V(0, TRACKVJP_TICK)
#if TRACKVJP_PART == -1
TRACKVJP_VARIANTS(WBC_VARIANT_INST)
#else
TRACKVJP_VARIANTS(WBC_VARIANT_UNIT)
#endif
#if TRACKVJP_PART <= 0
static TrackVjpKernel trackvjp_variant(long long key) {
  TRACKVJP_VARIANTS(WBC_VARIANT_FIND)
  return nullptr;
}
int trackvjp_variant_count() { return 0 TRACKVJP_VARIANTS(WBC_VARIANT_COUNT); }
int launch_trackvjp(const TrackVjpArgs& a, int stage, void* stream, long long* key_out) {
  const long long key = variant_key(stage);
  if (key_out) *key_out = key;
  const TrackVjpKernel k = trackvjp_variant(key);
  if (!k) return WBC_E_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3((a.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, a);
  return check_launch("rollout_vjp_tracks");
}
#endif

}  // namespace wbc
