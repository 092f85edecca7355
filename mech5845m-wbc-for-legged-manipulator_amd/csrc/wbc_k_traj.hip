// wbc_k_traj.hip — wbc_rollout_traj / wbc_rollout_tracks: per-instance milestone trajectories (tracks) of the end effectors' and the trunk's
// targets, piecewise linear or a Hermite spline, and the roll-out's scores (the target-versus-reached log of sim3.py:340-348 reduced on the
// device, for any of the six frames). Three small kernels beside the roll-out's tick and update kernels, one lane per instance:
//   wbc_traj_begin_kernel   once: bad-row check, score reset, the targets of tick 0
//   wbc_traj_tick_kernel    after the update kernel of tick k: the tick's errors and status into the scores, then every followed target of
//                           tick k + 1 (one launch however many tracks)
//   wbc_traj_groups_kernel  once at the end: one wavefront per group of M consecutive instances, fixed-shape reduction (no atomics)
// The target arithmetic is klampt's Trajectory.eval / HermiteTrajectory.eval as Robot_Wrapper4._LinearTrajectory / _HermiteTrajectory restate
// them, operation for operation and without contraction into fused multiply-adds, so that the host restatements
// (wbc_workload.traj_targets / track_targets) are bit-exact. wbc_rollout_traj is the one-track call (LINEAR, the gripper scored).
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_traj.h"

#pragma clang fp contract(off)

namespace wbc {

constexpr int TRAJ_BLOCK = 256;

// _LinearTrajectory.eval(t) (HERMITE: _HermiteTrajectory.eval(t)) over the n milestones m[n][3] (Robot_Wrapper4.py): wbc_track.h's segment,
// basis and default-tangent rule. v: the caller's tangents [n][3] or null (HERMITE only)
template <bool HERMITE>
__device__ __forceinline__ void traj_eval(const double* __restrict__ m, const double* __restrict__ v, int n, double t, double out[3]) {
  const TrackSeg sg = track_segment(t, n);
  const double* a = m + 3 * sg.i;
  if (sg.where != SEG_INSIDE) {
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2];
  } else if (!HERMITE) {
    const double u = sg.u;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (1.0 - u) * a[c] + u * a[3 + c];
  } else {
    const int i = sg.i;
    const HermiteBasis h = hermite_basis(sg.u);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v0 = v ? v[3 * i + c] : track_tangent(m + c, n, i);
      const double v1 = v ? v[3 * i + 3 + c] : track_tangent(m + c, n, i + 1);
      out[c] = ((h.cx1 * a[c] + h.cx2 * a[3 + c]) + h.cv1 * v0) + h.cv2 * v1;
    }
  }
}

// the target of track T for instance b at tick k (the parameter is the product k * du, not a running sum) into its row of the target blocks
__device__ __forceinline__ void traj_write_target(const TrajArgs& A, const DevTrack& T, int b, int k) {
  const int n = track_n(T, b);
  const double du = track_du(T, b);
  const double* m = T.points + (size_t)b * T.S * 3;
  const double t = (double)k * du;
  double nx[3];
  if (T.kind == WBC_TRACK_HERMITE) traj_eval<true>(m, T.tangents ? T.tangents + (size_t)b * T.S * 3 : nullptr, n, t, nx);
  else traj_eval<false>(m, nullptr, n, t, nx);
  double* out = T.target == WBC_TARGET_TRUNK ? A.trunk_target + (size_t)b * 3 : A.ee_target + (size_t)b * 15 + 3 * T.target;
  out[0] = nx[0]; out[1] = nx[1]; out[2] = nx[2];
}

__global__ void __launch_bounds__(TRAJ_BLOCK) wbc_traj_begin_kernel(const TrajArgs A) {
  const int b = blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (b >= A.B) return;
  bool bad = false;
#pragma unroll 1
  for (int j = 0; j < A.n_tracks; ++j) bad |= track_bad(A.tr[j], b);
  A.bad[b] = bad ? 1 : 0;
  int nsc = 0;
#pragma unroll 1
  for (int f = 0; f < TRAJ_FRAMES; ++f) {
    if (!((A.score_mask >> f) & 1)) continue;
    const size_t i = (size_t)nsc * A.B + b;
    A.err_sq_sum[i] = 0.0; A.err_max[i] = -1.0; A.err_final[i] = 0.0; A.err_max_tick[i] = -1;
    ++nsc;
  }
  A.first_bad_tick[b] = -1; A.bad_ticks[b] = 0;
  A.status_max[b] = bad ? WBC_QP_NUMERICAL : WBC_QP_OPTIMAL;
  if (bad) {
    atomicAdd(A.bad_count, 1);
    if (A.ro_status_max) A.ro_status_max[b] = WBC_QP_NUMERICAL;   // (the update kernels keep the maximum)
    return;                                                        // every followed target stays at in0's value
  }
#pragma unroll 1
  for (int j = 0; j < A.n_tracks; ++j) traj_write_target(A, A.tr[j], b, 0);
}

// ONE: the one-track call (wbc_rollout_traj) — track 0 is LINEAR and follows an end effector, the gripper alone is scored from its own
// [B][3] row, no trace, no trunk step. The same arithmetic with every loop and lookup of the general form resolved at compile time: the
// general form costs that call 1.1 us per tick at B = 65536 (profiles/r08_rollout_tracks.txt).
template <bool ONE>
__global__ void __launch_bounds__(TRAJ_BLOCK) wbc_traj_tick_kernel(const TrajArgs A, const int k) {
  const int b = blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (b >= A.B) return;
  const bool bad = A.bad[b] != 0;
  if (ONE) {
    if (A.do_sum) {
      const double* g = A.reached + (size_t)b * 3;
      const double* tg = A.ee_target + (size_t)b * 15 + 12;           // the gripper's target of THIS tick (the update kernel left it in place)
      const double dx = g[0] - tg[0], dy = g[1] - tg[1], dz = g[2] - tg[2];
      const double e2 = (dx * dx + dy * dy) + dz * dz;
      const double e = sqrt(e2);
      const int st = A.status[b];
      A.err_sq_sum[b] = A.err_sq_sum[b] + e2;                         // summed in tick order
      if (e > A.err_max[b]) { A.err_max[b] = e; A.err_max_tick[b] = k; }   // strictly larger: the FIRST tick of the maximum
      A.err_final[b] = e;
      if (!bad && st > A.status_max[b]) A.status_max[b] = st;
      if (bad || st != WBC_QP_OPTIMAL) {
        if (A.first_bad_tick[b] < 0) A.first_bad_tick[b] = k;
        A.bad_ticks[b] = A.bad_ticks[b] + 1;
      }
    }
    if (bad) return;
    const DevTrack& T = A.tr[0];
    double nx[3];
    traj_eval<false>(T.points + (size_t)b * T.S * 3, nullptr, track_n(T, b), (double)(k + 1) * track_du(T, b), nx);   // the parameter is the product, not a running sum
    double* out = A.ee_target + (size_t)b * 15 + 3 * T.target;
    out[0] = nx[0]; out[1] = nx[1]; out[2] = nx[2];
    return;
  }
  if (A.do_sum) {
    int nsc = 0;
#pragma unroll 1
    for (int f = 0; f < TRAJ_FRAMES; ++f) {
      if (!((A.score_mask >> f) & 1)) continue;
      const double* g = A.reached + (size_t)b * A.reached_stride + A.reached_off[f];
      // the frame's target of THIS tick (the update kernel left it in place)
      const double* tg = f == WBC_TARGET_TRUNK ? A.trunk_target + (size_t)b * 3 : A.ee_target + (size_t)b * 15 + 3 * f;
      const double gx = g[0], gy = g[1], gz = g[2];
      const double dx = gx - tg[0], dy = gy - tg[1], dz = gz - tg[2];
      const double e2 = (dx * dx + dy * dy) + dz * dz;
      const double e = sqrt(e2);
      const size_t i = (size_t)nsc * A.B + b;
      A.err_sq_sum[i] = A.err_sq_sum[i] + e2;                         // summed in tick order
      if (e > A.err_max[i]) { A.err_max[i] = e; A.err_max_tick[i] = k; }   // strictly larger: the FIRST tick of the maximum
      A.err_final[i] = e;
      if (A.trace) { double* tr = A.trace + i * 3; tr[0] = gx; tr[1] = gy; tr[2] = gz; }
      ++nsc;
    }
    const int st = A.status[b];
    if (!bad && st > A.status_max[b]) A.status_max[b] = st;
    if (bad || st != WBC_QP_OPTIMAL) {
      if (A.first_bad_tick[b] < 0) A.first_bad_tick[b] = k;
      A.bad_ticks[b] = A.bad_ticks[b] + 1;
    }
  }
  if (A.trunk_step) {                                                 // a constant step of a trunk target no track follows (as the update kernel's)
    double* tt = A.trunk_target + (size_t)b * 3;
    const double* ts = A.trunk_step + (size_t)b * 3;
    tt[0] = tt[0] + ts[0]; tt[1] = tt[1] + ts[1]; tt[2] = tt[2] + ts[2];
  }
  if (bad) return;
#pragma unroll 1
  for (int j = 0; j < A.n_tracks; ++j) traj_write_target(A, A.tr[j], b, k + 1);
}

// One wavefront per group: lane l takes instances l, l + 64, ... of the group in that order, then a butterfly over the 64 lanes. The
// shape of the reduction depends on M alone, so two runs give the same bits.
__global__ void __launch_bounds__(64) wbc_traj_groups_kernel(const TrajGroupArgs A) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= A.G) return;
  const size_t base = (size_t)g * A.M, nb = (size_t)A.G * A.M;
  int worst = 0, nbad = 0;
#pragma unroll 1
  for (int i = lane; i < A.M; i += 64) {
    const int s = A.status_max[base + i];
    worst = s > worst ? s : worst;
    nbad += A.bad_ticks[base + i] > 0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int w = __shfl_xor(worst, off, 64);
    worst = w > worst ? w : worst;
    nbad += __shfl_xor(nbad, off, 64);
  }
  if (lane == 0) {
    if (A.group_worst_status) A.group_worst_status[g] = worst;
    if (A.group_bad_instances) A.group_bad_instances[g] = nbad;
  }
#pragma unroll 1
  for (int j = 0; j < A.n_scored; ++j) {
    const double* sq = A.err_sq_sum + j * nb + base;
    const double* em = A.err_max + j * nb + base;
    double sum = 0.0, emax = -1.0;
#pragma unroll 1
    for (int i = lane; i < A.M; i += 64) {
      sum = sum + sq[i];
      emax = fmax(emax, em[i]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sum = sum + __shfl_xor(sum, off, 64);
      emax = fmax(emax, __shfl_xor(emax, off, 64));
    }
    if (lane == 0) {
      if (A.group_rms) A.group_rms[(size_t)j * A.G + g] = sqrt(sum / ((double)A.M * (double)A.ticks));
      if (A.group_err_max) A.group_err_max[(size_t)j * A.G + g] = emax;
    }
  }
}

static int traj_launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int launch_traj_begin(const TrajArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_traj_begin_kernel, dim3((a.B + TRAJ_BLOCK - 1) / TRAJ_BLOCK), dim3(TRAJ_BLOCK), 0, (hipStream_t)stream, a);
  return traj_launched();
}

int launch_traj_tick(const TrajArgs& a, int k, void* stream) {
  const dim3 grid((a.B + TRAJ_BLOCK - 1) / TRAJ_BLOCK), block(TRAJ_BLOCK);
  if (a.one_track) hipLaunchKernelGGL(wbc_traj_tick_kernel<true>, grid, block, 0, (hipStream_t)stream, a, k);
  else hipLaunchKernelGGL(wbc_traj_tick_kernel<false>, grid, block, 0, (hipStream_t)stream, a, k);
  return traj_launched();
}

int launch_traj_groups(const TrajGroupArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_traj_groups_kernel, dim3(a.G), dim3(64), 0, (hipStream_t)stream, a);
  return traj_launched();
}

}  // namespace wbc
