// wbc_k_traj.hip — wbc_rollout_traj: per-instance milestone trajectories of one end effector's target, and the roll-out summary
// (the gripper's target-versus-reached log of sim3.py:340-348 reduced on the device). Three small kernels beside the roll-out's tick and
// update kernels, one lane per instance:
//   wbc_traj_begin_kernel   once: bad-row check, summary reset, the target of tick 0
//   wbc_traj_tick_kernel    after the update kernel of tick k: the tick's error and status into the summary, then the target of tick k + 1
//   wbc_traj_groups_kernel  once at the end: one wavefront per group of M consecutive instances, fixed-shape reduction (no atomics)
// The target arithmetic is klampt's Trajectory.eval as Robot_Wrapper4._LinearTrajectory restates it, operation for operation and without
// contraction into fused multiply-adds, so that the host restatement (wbc_workload.traj_targets) is bit-exact.
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_traj.h"

#pragma clang fp contract(off)

namespace wbc {

constexpr int TRAJ_BLOCK = 256;

__device__ __forceinline__ bool traj_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// _LinearTrajectory.eval(t) over the n milestones m[n][3] (Robot_Wrapper4.py): clamped ends, unit parameter per segment
__device__ __forceinline__ void traj_eval(const double* __restrict__ m, int n, double t, double out[3]) {
  if (t <= 0.0) {
    out[0] = m[0]; out[1] = m[1]; out[2] = m[2];
  } else if (t >= (double)(n - 1)) {
    const double* e = m + 3 * (n - 1);
    out[0] = e[0]; out[1] = e[1]; out[2] = e[2];
  } else {
    const double fi = floor(t);
    const int i = (int)fi;                 // 0 <= i <= n - 2 here
    const double u = t - fi;
    const double* a = m + 3 * i;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (1.0 - u) * a[c] + u * a[3 + c];
  }
}

__global__ void __launch_bounds__(TRAJ_BLOCK) wbc_traj_begin_kernel(const TrajArgs A) {
  const int b = blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (b >= A.B) return;
  const int n = A.n_points ? A.n_points[b] : A.S;
  const double du = A.du ? A.du[b] : A.du_all;
  const double* m = A.points + (size_t)b * A.S * 3;
  bool bad = n < 2 || n > A.S || !traj_finite(du) || !(du > 0.0);
  if (!bad) {
#pragma unroll 1
    for (int i = 0; i < 3 * n; ++i) bad |= !traj_finite(m[i]);
  }
  A.bad[b] = bad ? 1 : 0;
  A.err_sq_sum[b] = 0.0; A.err_max[b] = -1.0; A.err_final[b] = 0.0;
  A.err_max_tick[b] = -1; A.first_bad_tick[b] = -1; A.bad_ticks[b] = 0;
  A.status_max[b] = bad ? WBC_QP_NUMERICAL : WBC_QP_OPTIMAL;
  if (bad) {
    atomicAdd(A.bad_count, 1);
    if (A.ro_status_max) A.ro_status_max[b] = WBC_QP_NUMERICAL;   // (the update kernels keep the maximum)
    return;                                                        // the followed target stays at in0's value
  }
  double t0[3];
  traj_eval(m, n, 0.0, t0);
  double* tg = A.ee_target + (size_t)b * 15 + 3 * A.ee;
  tg[0] = t0[0]; tg[1] = t0[1]; tg[2] = t0[2];
}

__global__ void __launch_bounds__(TRAJ_BLOCK) wbc_traj_tick_kernel(const TrajArgs A, const int k) {
  const int b = blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (b >= A.B) return;
  const bool bad = A.bad[b] != 0;
  if (A.do_sum) {
    const double* g = A.grip + (size_t)b * 3;
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
  const int n = A.n_points ? A.n_points[b] : A.S;
  const double du = A.du ? A.du[b] : A.du_all;
  double nx[3];
  traj_eval(A.points + (size_t)b * A.S * 3, n, (double)(k + 1) * du, nx);   // the parameter is the product, not a running sum
  double* out = A.ee_target + (size_t)b * 15 + 3 * A.ee;
  out[0] = nx[0]; out[1] = nx[1]; out[2] = nx[2];
}

// One wavefront per group: lane l takes instances l, l + 64, ... of the group in that order, then a butterfly over the 64 lanes. The
// shape of the reduction depends on M alone, so two runs give the same bits.
__global__ void __launch_bounds__(64) wbc_traj_groups_kernel(const TrajGroupArgs A) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= A.G) return;
  const size_t base = (size_t)g * A.M;
  double sum = 0.0, emax = -1.0;
  int worst = 0, nbad = 0;
#pragma unroll 1
  for (int i = lane; i < A.M; i += 64) {
    sum = sum + A.err_sq_sum[base + i];
    emax = fmax(emax, A.err_max[base + i]);
    const int s = A.status_max[base + i];
    worst = s > worst ? s : worst;
    nbad += A.bad_ticks[base + i] > 0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sum = sum + __shfl_xor(sum, off, 64);
    emax = fmax(emax, __shfl_xor(emax, off, 64));
    const int w = __shfl_xor(worst, off, 64);
    worst = w > worst ? w : worst;
    nbad += __shfl_xor(nbad, off, 64);
  }
  if (lane == 0) {
    if (A.group_rms) A.group_rms[g] = sqrt(sum / ((double)A.M * (double)A.ticks));
    if (A.group_err_max) A.group_err_max[g] = emax;
    if (A.group_worst_status) A.group_worst_status[g] = worst;
    if (A.group_bad_instances) A.group_bad_instances[g] = nbad;
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
  hipLaunchKernelGGL(wbc_traj_tick_kernel, dim3((a.B + TRAJ_BLOCK - 1) / TRAJ_BLOCK), dim3(TRAJ_BLOCK), 0, (hipStream_t)stream, a, k);
  return traj_launched();
}

int launch_traj_groups(const TrajGroupArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_traj_groups_kernel, dim3(a.G), dim3(64), 0, (hipStream_t)stream, a);
  return traj_launched();
}

}  // namespace wbc
