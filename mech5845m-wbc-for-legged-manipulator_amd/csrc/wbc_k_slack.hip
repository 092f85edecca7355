// wbc_k_slack.hip — wbc_state_slack / wbc_rollout_watch: the slack of the reference's constraint quantities at a configuration q, whether or
// not the configuration enforces them (include/wbc.h). Four families, slack >= 0 inside and < 0 outside:
//   0 CoM box      the operands of CoMConstraint (Robot_Wrapper4.py:669-677; wbc_common.h, P6) before inv_dt and com_box_scale
//   1 trunk z box  trunkConstraint's z row (:719, :735-736) before inv_dt and trunk_box_scale
//   2 trunk angles its three angle rows, the angles by the tick kernels' atan2 formula
//   3 joint range  the model's own range of each free DoF's OWN joint (not the damper's index map)
// Two kernels:
//   wbc_slack_kernel         the whole-tree shape (wbc_qtree.h): four instances per wavefront (lane = 16 r + s), FK over the whole-tree
//                            schedule DevPlan.q_fk (the CoM needs every body). Writes the row (wbc_state_slack) and / or folds the tick into
//                            the watch's accumulators (lanes s < 4 of a row, one family each): no second accumulation launch.
//   wbc_slack_groups_kernel  once at the end: one wavefront per group of M consecutive instances, fixed-shape reduction (no atomics)
// The evaluation itself (frames, CoM, joint scan, components, family scans) stands in wbc_slack.h as inline functions: wbc_k_slackvjp.hip, the
// cotangent of these families, runs the same ones and so selects the same components.
// Reads q, the box centres and the tables; writes nothing but its outputs, rows [0, B) only.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_qtree.h"
#include "wbc_slack.h"      // behind wbc_qtree.h: the evaluation is declared

namespace wbc {

struct __attribute__((aligned(16))) SInst {
  QtKin K;
  double pf[12];                            // FL foot, RR foot, trunk frame: world positions (stride 4)
  double eul[4];                            // roll, pitch, yaw of the trunk rotation
};
struct __attribute__((aligned(16))) SSmemP { SInst I[4]; };
static_assert(sizeof(SInst) == 3200 && offsetof(SInst, pf) == 3072 && offsetof(SInst, eul) == 3168, "the instance's LDS record");

template <bool ROT>   // ROT: rotated joint placements in the batch (wbc_k_sim3p.hip)
__global__ void __launch_bounds__(64) wbc_slack_kernel(const SlackArgs A, const DevModel* __restrict__ models, const WbcConfig* __restrict__ cfgs,
                                                       const DevPlan* __restrict__ plans) {
  __shared__ SSmemP SP;
  const QtLane T(A.B);
  const int s = T.s; const size_t b = T.b;
  SInst& U = SP.I[T.r];
  const int mid = qt_model_index(A.model_id, b, A.n_models);
  const DevModel& M = models[mid];
  const WbcConfig& cfg = cfgs[mid];
  const DevPlan& P = plans[mid];
  const SlackLimits& Lm = A.lim[mid];
  const int nq = M.nq;
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  // ---- every global read first
  const double* qg = A.q + b * NQ;
  const double q0 = qg[s], q1 = (16 + s < nq) ? qg[16 + s] : 0.0;
  double bc[4] = {qnan, qnan, qnan, qnan};
  if (A.box) {
#pragma unroll
    for (int i = 0; i < 4; ++i) bc[i] = A.box[b * 4 + i];
  }
  DevPlan::PkJoint fkn = P.q_fk[0][s];
  const int scq0 = P.q_scq[(2 + s) & 31], scq1 = P.q_scq[(18 + s) & 31];
  const SlackLane L(M, cfg, P, Lm, s);
  const bool qbad = (s < nq && !is_finite(q0)) || (16 + s < nq && !is_finite(q1));
  const bool rowbad = ((__ballot(qbad) >> T.rbase) & 0xFFFFull) != 0ull;
  qt_fk<ROT>(U.K, q0, q1, scq0, scq1, M, P, fkn, s);
  const double* const qv = U.K.q;
  const double* const oMi = U.K.oMi;
  // ---- the evaluation (wbc_slack.h)
  slack_frames(U.pf, U.eul, oMi, L, s);
  double com0, com1, cm;
  slack_com_xy(oMi, L, s, com0, com1, cm);
  double jv;
  int jc;
  slack_joint_scan(qv, L, s, jv, jc);
  WSYNC();                                                          // pf, eul are visible
  double comp[SLACK_NC], sl[SLACK_NF];
  int wh[SLACK_NF];
  slack_components(U.pf, U.eul, com0, com1, bc, L, comp);
  slack_families(comp, jv, jc, sl, wh);
  const bool bad1 = rowbad || !is_finite(bc[0]);
  const bool bad2 = rowbad || !is_finite(bc[1]) || !is_finite(bc[2]) || !is_finite(bc[3]);
  if (rowbad) { sl[0] = qnan; wh[0] = -1; sl[3] = qnan; wh[3] = -1; }
  if (bad1) { sl[1] = qnan; wh[1] = -1; }
  if (bad2) { sl[2] = qnan; wh[2] = -1; }
#pragma unroll
  for (int i = 0; i < SLACK_NC; ++i) if (i < 4 ? rowbad : (i < 6 ? bad1 : bad2)) comp[i] = qnan;
  if (!T.valid) return;
  // ---- the row (wbc_state_slack): component s on lane s < 12, family s on lane s < 4
  double cs = comp[0];
#pragma unroll
  for (int i = 1; i < SLACK_NC; ++i) cs = (s == i) ? comp[i] : cs;
  if (A.components && s < SLACK_NC) A.components[b * SLACK_NC + s] = cs;
  const double fs = (s == 0) ? sl[0] : (s == 1) ? sl[1] : (s == 2) ? sl[2] : sl[3];
  const int fw = (s == 0) ? wh[0] : (s == 1) ? wh[1] : (s == 2) ? wh[2] : wh[3];
  if (s < SLACK_NF) {
    if (A.slack) A.slack[b * SLACK_NF + s] = fs;
    if (A.which) A.which[b * SLACK_NF + s] = fw;
  }
  // ---- the watch: lane s < 4 folds family s of tick k into row w of the accumulators (tick 0 initialises them)
  if (s < SLACK_NF && ((A.mask >> s) & 1)) {
    const size_t i = (size_t)__popc((unsigned)A.mask & ((1u << s) - 1u)) * (size_t)A.B + b;
    const int k = A.k;
    double mn = fs;
    int mt = 0, mw = fw, neg = 0, fneg = -1;
    if (k > 0) {
      mn = A.slack_min[i]; mt = A.min_tick[i]; mw = A.min_which[i]; neg = A.neg_ticks[i]; fneg = A.first_neg[i];
      if (mn == mn) {                                               // a NaN minimum stays: the first NaN tick, no code
        if (fs != fs) { mn = fs; mt = k; mw = -1; }
        else if (fs < mn) { mn = fs; mt = k; mw = fw; }              // strictly smaller: the FIRST tick of the minimum
      }
    }
    if (fs < 0.0) { neg += 1; if (fneg < 0) fneg = k; }             // (a NaN tick is not counted)
    A.slack_min[i] = mn; A.min_tick[i] = mt; A.min_which[i] = mw; A.neg_ticks[i] = neg; A.first_neg[i] = fneg;
    A.slack_final[i] = fs;
    if (A.trace) A.trace[i] = fs;
  }
}

// One wavefront per group: lane l takes instances l, l + 64, ... of the group in that order, then a butterfly over the 64 lanes. The
// shape of the reduction depends on M alone, so two runs give the same bits. A NaN slack_min in the group gives a NaN group_min.
__global__ void __launch_bounds__(64) wbc_slack_groups_kernel(const SlackGroupArgs A) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= A.G) return;
  const size_t base = (size_t)g * A.M, nb = (size_t)A.G * A.M;
#pragma unroll 1
  for (int j = 0; j < A.n_w; ++j) {
    const double* sm = A.slack_min + j * nb + base;
    const int32_t* ng = A.neg_ticks + j * nb + base;
    double mn = __longlong_as_double(0x7FF0000000000000ll);
    int nan = 0, nneg = 0;
#pragma unroll 1
    for (int i = lane; i < A.M; i += 64) {
      const double v = sm[i];
      nan |= (v != v) ? 1 : 0;
      mn = fmin(mn, v);
      nneg += ng[i] > 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      mn = fmin(mn, __shfl_xor(mn, off, 64));
      nan |= __shfl_xor(nan, off, 64);
      nneg += __shfl_xor(nneg, off, 64);
    }
    if (lane == 0) {
      if (A.group_min) A.group_min[(size_t)j * A.G + g] = nan ? __longlong_as_double(0x7FF8000000000000ll) : mn;
      if (A.group_neg_instances) A.group_neg_instances[(size_t)j * A.G + g] = nneg;
    }
  }
}

static int slack_launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int launch_slack(const SlackArgs& a, void* stream) {
  const dim3 grid((a.B + 3) / 4), block(64);
  if (a.rot) hipLaunchKernelGGL(wbc_slack_kernel<true>, grid, block, 0, (hipStream_t)stream, a, a.models, a.cfgs, a.plans);
  else hipLaunchKernelGGL(wbc_slack_kernel<false>, grid, block, 0, (hipStream_t)stream, a, a.models, a.cfgs, a.plans);
  return slack_launched();
}

int launch_slack_groups(const SlackGroupArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_slack_groups_kernel, dim3(a.G), dim3(64), 0, (hipStream_t)stream, a);
  return slack_launched();
}

}  // namespace wbc
