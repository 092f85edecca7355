// wbc_track.h — one followed track as a kernel sees it, and what the forward (wbc_k_traj.hip) and its adjoint (wbc_k_trackvjp.hip) share of
// its evaluation (internal, C++): which rows are bad, which branch the default-tangent rule takes, which segment a parameter falls into, the
// Hermite basis. The arithmetic is klampt's Trajectory.eval / HermiteTrajectory.eval as Robot_Wrapper4._LinearTrajectory / _HermiteTrajectory
// restate them, operation for operation and without contraction into fused multiply-adds (the pragma below holds to the end of the including
// unit: both kernel units state it themselves, the API unit has no device code), so that the host restatements are bit-exact.
#pragma once
#include <math.h>
#include "wbc_device.h"

#pragma clang fp contract(off)

namespace wbc {

// One followed target: per-instance milestones (and, HERMITE, tangents) as WbcTrack.
struct DevTrack {
  int32_t target, kind, S, pad_;
  const double* points;                 // [B][S][3]
  const double* tangents;               // [B][S][3], HERMITE only; null => the default rule, computed on the fly
  const int32_t* n_points;              // null => S
  const double* du;                     // null => du_all
  double du_all;
};
inline void fill_track(DevTrack& d, const WbcTrack& t) {   // (host) the caller's track, its pointers staged
  d.target = t.target; d.kind = t.kind; d.S = t.max_points;
  d.points = t.points; d.tangents = t.tangents; d.n_points = t.n_points; d.du = t.du; d.du_all = t.du_all;
}

__device__ __forceinline__ int track_n(const DevTrack& T, size_t b) { return T.n_points ? T.n_points[b] : T.S; }
__device__ __forceinline__ double track_du(const DevTrack& T, size_t b) { return T.du ? T.du[b] : T.du_all; }

// instance b's row of track T is bad: n outside [2, S], du not finite and positive, or a non-finite milestone or tangent among the first n
__device__ __forceinline__ bool track_bad(const DevTrack& T, size_t b) {
  const int n = track_n(T, b);
  const double du = track_du(T, b);
  const bool bad_n = n < 2 || n > T.S;
  bool bad = bad_n || !is_finite(du) || !(du > 0.0);
  if (!bad_n) {
    const double* m = T.points + b * T.S * 3;
#pragma unroll 1
    for (int i = 0; i < 3 * n; ++i) bad |= !is_finite(m[i]);
    if (T.tangents) {
      const double* v = T.tangents + b * T.S * 3;
#pragma unroll 1
      for (int i = 0; i < 3 * n; ++i) bad |= !is_finite(v[i]);
    }
  }
  return bad;
}

// The default tangent of one component at an interior milestone x between a and b: the rule of klampt's makeSpline(preventOvershoot=True) as
// include/wbc.h states and numbers it (no segment of the spline leaves the interval of its two milestones). -> the case 1..4; w: the centred
// difference, the tangent of case 4
__device__ __forceinline__ int tangent_case(double a, double x, double b, double& w) {
  w = (b - a) * 0.5;
  const double third = 1.0 / 3.0;
  if (x <= fmin(a, b) || x >= fmax(a, b)) return 1;
  if ((w < 0.0 && x - w * third >= a) || (w > 0.0 && x - w * third <= a)) return 2;
  if ((w < 0.0 && x + w * third < b) || (w > 0.0 && x + w * third > b)) return 3;
  return 4;
}
// the default tangent at milestone i of n; m: the instance's milestones at this component, stride 3
__device__ __forceinline__ double track_tangent(const double* __restrict__ m, int n, int i) {
  if (n == 2) return m[3] - m[0];
  if (i == 0 || i == n - 1) return 0.0;
  const double a = m[3 * (i - 1)], x = m[3 * i], b = m[3 * (i + 1)];
  double w;
  switch (tangent_case(a, x, b, w)) {
    case 1: return 0.0;
    case 2: return 3.0 * (x - a);
    case 3: return 3.0 * (b - x);
    default: return w;
  }
}

// where the parameter t falls among n milestones: clamped ends, unit parameter per segment
enum { SEG_FIRST = 0, SEG_LAST = 1, SEG_INSIDE = 2 };
struct TrackSeg { int where, i; double u; };   // INSIDE: segment i (0 <= i <= n - 2) at u in [0, 1); FIRST / LAST: milestone i
__device__ __forceinline__ TrackSeg track_segment(double t, int n) {
  if (t <= 0.0) return TrackSeg{SEG_FIRST, 0, 0.0};
  if (t >= (double)(n - 1)) return TrackSeg{SEG_LAST, n - 1, 0.0};
  const double fi = floor(t);
  return TrackSeg{SEG_INSIDE, (int)fi, t - fi};
}

// the cubic Hermite basis at u: the coefficients of milestones i, i + 1 and of their tangents
struct HermiteBasis { double cx1, cx2, cv1, cv2; };
__device__ __forceinline__ HermiteBasis hermite_basis(double u) {
  const double u2 = u * u, u3 = u * u2;
  return HermiteBasis{(2.0 * u3 - 3.0 * u2) + 1.0, (-2.0 * u3) + 3.0 * u2, (u3 - 2.0 * u2) + u, u3 - u2};
}

}  // namespace wbc
