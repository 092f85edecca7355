// wbc_k_stepvjp.hip — wbc_step_vjp: the state step between two ticks as a layer (include/wbc.h). For
//   q_next = pin.integrate(q, qdot dt),  q_new = updateState(running=True) + trunkWorldPos   (mode WARMUP: q_new = q_next)
// and g = dL/d delta_new in the tangent coordinates at q_new, one launch gives dL/d(q, qdot, foot_targets), q's in the tangent coordinates at q.
// Update part (RUNNING), with R_b the base rotation q_new carries, p_e / p_t the foot / trunk frame origins at [q xyz, that rotation, the joints
// of q_next], BPA = mean(p_e - p_t), rbar = R_b' BPA, g_p = g[0:3], g_phi = g[3:6]:
//   d_foot_targets[e] = R_b g_p / 4;  c_theta[d] = g[d] - (1/4) sum_e (LOCAL_WORLD_ALIGNED linear column of DoF d at foot e) . g_p;
//   c_phi = g_phi - BPA x g_p - rbar x (R_b' g_p)  (0 with an IMU quaternion: it is held constant);  c_p = 0.
// Integrate part, xi = dt qdot[0:6], (Re, pe) = exp6(xi), c6 = (c_p, c_phi):
//   d_q[0:6] = Ad_{exp(-xi)}' c6 = (Re c_p, pe x (Re c_p) + Re c_phi);  d_qdot[0:6] = dt Jr(xi)' c6;  d_q[6:] = c_theta;  d_qdot[6:] = dt c_theta.
// Jr' in closed form: the SO(3) block I + b W + c1 W^2 and the coupling block
//   Q = V / 2 + c1 (W V + V W + W V W) + c2 (W W V + V W W - 3 W V W) + c3 (W V W W + W W V W),   W = omega x, V = v x,
// with a = sin t / t, b = (1 - cos t) / t^2, c1 = (1 - a) / t^2, c2 = (1 / 2 - b) / t^2, c3 = (3 c1 - b) / (2 t^2), t = |omega| dt. Below t = 1 all
// five come from their power series in t^2 (sv_coef): the closed forms cancel like eps / t^2 (c1) and eps / t^4 (c2, c3).
// The whole-tree shape (wbc_qtree.h): four instances per wavefront (lane = 16 r + s), FK over the whole-tree schedule DevPlan.q_fk (its own
// sequence: q is assembled in LDS and the seed's rotation replaced, so not qt_fk). No Jacobian is
// stored: lane s forms the transposed foot point-Jacobian product of its DoF s and 16 + s from the joint axes and origins in LDS. Reads its
// inputs and the tables; writes nothing but its outputs, rows [0, B) only.
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_grad.h"
#include "wbc_stepvjp.h"
#include "wbc_qtree.h"

namespace wbc {

struct __attribute__((aligned(16))) VInst {
  double oMi[24 * 12];
  double q[32];                             // the configuration the estimator's kinematics run at
  double sc[64];
  double qc[32];                            // q_cur
  double xi[8];                             // dt qdot[0:6]
  double g6[8];                             // g[0:6]
  double pf[5 * 4];                         // feet 0..3, trunk frame: world positions (stride 4)
};
struct __attribute__((aligned(16))) VSmemP { VInst I[4]; };

// sum_k (-t2)^k c_k with c_0 = 1 and c_k / c_(k-1) = NUM(k) / ((2 k + OFF - 1) (2 k + OFF)), nested from k = N down: every partial sum is
// within [1 - t2 / 6, 1], so nothing cancels
template <int OFF, bool C3, int N>
__device__ __forceinline__ double sv_series(const double t2) {
  const double z = -t2;
  double sum = 1.0;
#pragma unroll
  for (int k = N; k >= 1; --k) {
    const double ratio = (C3 ? (double)(k + 1) / (double)k : 1.0) / (double)((2 * k + OFF - 1) * (2 * k + OFF));
    sum = fma(z * sum, ratio, 1.0);
  }
  return sum;
}

struct SE3Coef { double a, b, c1, c2, c3; };
// a = sin t / t, b = (1 - cos t) / t^2, c1 = (t - sin t) / t^3, c2 = (t^2 + 2 cos t - 2) / (2 t^4), c3 = (2 t - 3 sin t + t cos t) / (2 t^5).
// t < 1: ten terms of each series (the eleventh is below 1 / 23! of the first). t >= 1: closed forms; the worst cancellation is c3's at t = 1,
// 3 c1 - b = 0.016 from terms of 0.46: 30 eps.
constexpr int SV_TERMS = 10;
__device__ __forceinline__ SE3Coef sv_coef(const double t2) {
  SE3Coef o;
  if (t2 < 1.0) {
    o.a = sv_series<1, false, SV_TERMS>(t2);
    o.b = sv_series<2, false, SV_TERMS>(t2) * 0.5;
    o.c1 = sv_series<3, false, SV_TERMS>(t2) * (1.0 / 6);
    o.c2 = sv_series<4, false, SV_TERMS>(t2) * (1.0 / 24);
    o.c3 = sv_series<5, true, SV_TERMS>(t2) * (1.0 / 120);
  } else {
    const double t = sqrt(t2);
    const SinCos sc = sincos_cw(t);
    o.a = sc.s / t;
    o.b = (1 - sc.c) / t2;
    o.c1 = (1 - o.a) / t2;
    o.c2 = (0.5 - o.b) / t2;
    o.c3 = (3 * o.c1 - o.b) / (2 * t2);
  }
  return o;
}

// (1/4) sum over the feet DoF d moves (bit e of sup) of the LOCAL_WORLD_ALIGNED linear column of d at foot e, dotted with gp: a revolute
// column is axis x (p_e - o), a prismatic one the axis
__device__ __forceinline__ double sv_jt(const double* const oMi, const int joint, const int lin_axis, const int ang_axis, const unsigned sup,
                                        const double* const pf, const double (&gp)[3]) {
  const double* Pj = oMi + 12 * joint;
  const int ax = ang_axis >= 0 ? ang_axis : (lin_axis >= 0 ? lin_axis : 0);
  const double axis[3] = {Pj[3 * ax], Pj[3 * ax + 1], Pj[3 * ax + 2]};
  double acc = 0.0;
  if (ang_axis >= 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d[3] = {pf[4 * e] - Pj[9], pf[4 * e + 1] - Pj[10], pf[4 * e + 2] - Pj[11]};
      double c[3];
      cross3(axis, d, c);
      const double t = c[0] * gp[0] + c[1] * gp[1] + c[2] * gp[2];
      acc += ((sup >> e) & 1u) ? t : 0.0;
    }
  } else if (lin_axis >= 0) {
    acc = (double)__popc(sup & 15u) * (axis[0] * gp[0] + axis[1] * gp[1] + axis[2] * gp[2]);
  }
  return acc / 4;
}

template <bool ROT>   // ROT: rotated joint placements in the batch (wbc_k_sim3p.hip)
__global__ void __launch_bounds__(64) wbc_stepvjp_kernel(const StepVjpArgs A, const DevModel* __restrict__ models, const DevPlan* __restrict__ plans) {
  __shared__ VSmemP SP;
  const QtLane T(A.B);
  const int s = T.s; const size_t b = T.b;
  VInst& U = SP.I[T.r];
  const int mid = qt_model_index(A.model_id, b, A.n_models);
  const DevModel& M = models[mid];
  const DevPlan& P = plans[mid];
  const int nq = M.nq, nv = M.nv;
  const bool running = A.mode != WBC_ROLLOUT_WARMUP;                // (the same for the whole launch)
  const bool have_imu = running && A.imu != nullptr;
  const double dt = A.dt;
  // ---- every global read first
  const double* qg = A.q_cur + b * NQ;
  const double q0 = qg[s], q1 = (16 + s < nq) ? qg[16 + s] : 0.0;
  const int d0 = s, d1 = 16 + s;                                    // DoF of this lane
  const bool h0 = d0 < nv, h1 = d1 < nv;
  const double xd0 = h0 ? A.qdot[b * NV + d0] : 0.0, xd1 = h1 ? A.qdot[b * NV + d1] : 0.0;
  const double gd0 = h0 ? A.g[b * NV + d0] : 0.0, gd1 = h1 ? A.g[b * NV + d1] : 0.0;
  const double ft = (running && s < 12) ? A.foot_targets[b * 15 + s] : 0.0;
  const double im = (have_imu && s >= 3 && s < 7) ? A.imu[b * 4 + (s - 3)] : 0.0;
  DevPlan::PkJoint fkn = P.q_fk[0][s];
  const int scq0 = P.q_scq[(2 + s) & 31], scq1 = P.q_scq[(18 + s) & 31];
  const QtDof Dc(M, s, nv);                                         // ... and where their columns come from
  const int cq0 = M.col_q[h0 ? d0 : 6], cq1 = M.col_q[h1 ? d1 : 6];
  unsigned sup0 = 0u, sup1 = 0u;                                    // bit e: the DoF moves foot frame e
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned fs = M.frame_support[WBC_FR_EE0 + e];
    sup0 |= (h0 && ((fs >> d0) & 1u)) ? 1u << e : 0u;
    sup1 |= (h1 && ((fs >> d1) & 1u)) ? 1u << e : 0u;
  }
  const int fr = (s < 4) ? WBC_FR_EE0 + s : WBC_FR_TRUNK;           // frame of this lane: feet 0..3, trunk
  const int fjoint = M.frame_joint[fr];
  const double f0 = M.frame_p[fr][0], f1 = M.frame_p[fr][1], f2 = M.frame_p[fr][2];
  const bool bad = (s < nq && !is_finite(q0)) || (16 + s < nq && !is_finite(q1)) || !is_finite(xd0) || !is_finite(xd1) || !is_finite(gd0) ||
                   !is_finite(gd1) || !is_finite(ft) || !is_finite(im);
  U.qc[s] = q0; U.qc[16 + s] = q1;
  U.q[s] = 0.0; U.q[16 + s] = 0.0;
  if (s < 6) { U.xi[s] = dt * xd0; U.g6[s] = gd0; }
  WSYNC();
  // ---- exp6(xi) and the coefficients, every lane of the instance alike
  const double vl[3] = {U.xi[0], U.xi[1], U.xi[2]}, w[3] = {U.xi[3], U.xi[4], U.xi[5]};
  const double gp[3] = {U.g6[0], U.g6[1], U.g6[2]}, gphi[3] = {U.g6[3], U.g6[4], U.g6[5]};
  const SE3Coef k = sv_coef(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double Re[9], pe[3];                                              // Re row-major
  {
    const double wx = w[0], wy = w[1], wz = w[2], a = k.a, bq = k.b;
    Re[0] = 1 - bq * (wy * wy + wz * wz); Re[1] = -a * wz + bq * wx * wy;       Re[2] = a * wy + bq * wx * wz;
    Re[3] = a * wz + bq * wx * wy;        Re[4] = 1 - bq * (wx * wx + wz * wz); Re[5] = -a * wx + bq * wy * wz;
    Re[6] = -a * wy + bq * wx * wz;       Re[7] = a * wx + bq * wy * wz;        Re[8] = 1 - bq * (wx * wx + wy * wy);
    double wxv[3];
    cross3(w, vl, wxv);
    const double wv = w[0] * vl[0] + w[1] * vl[1] + w[2] * vl[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) pe[i] = a * vl[i] + bq * wxv[i] + k.c1 * wv * w[i];
  }
  // ---- the update part: c = (c_p, c_phi, c_theta) and d_foot_targets
  double cp[3] = {gp[0], gp[1], gp[2]}, cf[3] = {gphi[0], gphi[1], gphi[2]}, ct0 = gd0, ct1 = gd1, Rg[3] = {0.0, 0.0, 0.0};
  if (running) {
    // config = [current base xyz, the quaternion q_new carries, new joint angles]  (wbc_update_packed_kernel)
    if (s < 7) U.q[s] = (s < 3 || !have_imu) ? q0 : im;
    if (h0 && d0 >= 6) U.q[cq0] = U.qc[cq0] + dt * xd0;
    if (h1) U.q[cq1] = U.qc[cq1] + dt * xd1;
    WSYNC();
    const double* const qv = U.q;
    double* const oMi = U.oMi;
    pk_fk_seed(oMi, U.sc, qv, scq0, scq1, s);
    if (s == 0 && !have_imu) {                                      // the rotation of q_next: R(q) Re, in place of the seed's R(q) (same lane, in order)
      double R0[9];
      quat_to_R(qv + 3, R0);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) oMi[12 + 3 * j + i] = R0[3 * i] * Re[j] + R0[3 * i + 1] * Re[3 + j] + R0[3 * i + 2] * Re[6 + j];
    }
    WSYNC();
    pk_fk_sweep<ROT>(oMi, U.sc, qv, M, P.q_fk, fkn, s);             // pin.forwardKinematics over every joint, level by level
    if (s < 5) {
      const double* Pj = oMi + 12 * fjoint;
#pragma unroll
      for (int rr = 0; rr < 3; ++rr) U.pf[4 * s + rr] = qt_point(Pj, f0, f1, f2, rr);
    }
    WSYNC();
    const double* P1 = oMi + 12;                                    // the base rotation R_b, column-major: R_b(i, j) = P1[3 j + i]
    const double* pf = U.pf;
    double BPA[3], rbar[3], Rtg[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double t = pf[4 * 4 + i];
      BPA[i] = ((pf[i] - t) + (pf[4 + i] - t) + (pf[8 + i] - t) + (pf[12 + i] - t)) / 4;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      rbar[j] = P1[3 * j] * BPA[0] + P1[3 * j + 1] * BPA[1] + P1[3 * j + 2] * BPA[2];
      Rtg[j] = P1[3 * j] * gp[0] + P1[3 * j + 1] * gp[1] + P1[3 * j + 2] * gp[2];
      Rg[j] = P1[j] * gp[0] + P1[3 + j] * gp[1] + P1[6 + j] * gp[2];
    }
    double c1[3], c2[3];
    cross3(BPA, gp, c1); cross3(rbar, Rtg, c2);
#pragma unroll
    for (int i = 0; i < 3; ++i) { cp[i] = 0.0; cf[i] = have_imu ? 0.0 : gphi[i] - c1[i] - c2[i]; }
    if (h0 && d0 >= 6) ct0 = gd0 - sv_jt(oMi, Dc.cj0, Dc.cl0, Dc.ca0, sup0, pf, gp);
    if (h1) ct1 = gd1 - sv_jt(oMi, Dc.cj1, Dc.cl1, Dc.ca1, sup1, pf, gp);
  }
  // ---- the integrate part on the base block
  double ql[3], qa[3], xl[3], xa[3];
  {
    double Rc[3], Rf[3], pxr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Rc[i] = Re[3 * i] * cp[0] + Re[3 * i + 1] * cp[1] + Re[3 * i + 2] * cp[2];
      Rf[i] = Re[3 * i] * cf[0] + Re[3 * i + 1] * cf[1] + Re[3 * i + 2] * cf[2];
    }
    cross3(pe, Rc, pxr);
#pragma unroll
    for (int i = 0; i < 3; ++i) { ql[i] = Rc[i]; qa[i] = pxr[i] + Rf[i]; }
    // Jr' c6 = (Js' c_p, Q' c_p + Js' c_phi),  Js' y = y + b w x y + c1 w x (w x y)
    double wy[3], wwy[3], wf[3], wwf[3];
    cross3(w, cp, wy); cross3(w, wy, wwy); cross3(w, cf, wf); cross3(w, wf, wwf);
    // Q' y = Q_left(W, V) y, eleven cross products
    double vy[3], vwy[3], vwwy[3], WVy[3], WWVy[3], WVWy[3], WWVWy[3], WVWWy[3];
    cross3(vl, cp, vy); cross3(vl, wy, vwy); cross3(vl, wwy, vwwy);
    cross3(w, vy, WVy); cross3(w, WVy, WWVy); cross3(w, vwy, WVWy); cross3(w, WVWy, WWVWy); cross3(w, vwwy, WVWWy);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      xl[i] = dt * (cp[i] + k.b * wy[i] + k.c1 * wwy[i]);
      const double Qy = 0.5 * vy[i] + k.c1 * (WVy[i] + vwy[i] + WVWy[i]) + k.c2 * (WWVy[i] + vwwy[i] - 3 * WVWy[i]) + k.c3 * (WVWWy[i] + WWVWy[i]);
      xa[i] = dt * (Qy + (cf[i] + k.b * wf[i] + k.c1 * wwf[i]));
    }
    if (running) { ql[0] = ql[1] = ql[2] = 0.0; xl[0] = xl[1] = xl[2] = 0.0; }   // c_p = 0: exactly
  }
  const double rq0 = (s == 0) ? ql[0] : (s == 1) ? ql[1] : (s == 2) ? ql[2] : (s == 3) ? qa[0] : (s == 4) ? qa[1] : (s == 5) ? qa[2] : ct0;
  const double rx0 = (s == 0) ? xl[0] : (s == 1) ? xl[1] : (s == 2) ? xl[2] : (s == 3) ? xa[0] : (s == 4) ? xa[1] : (s == 5) ? xa[2] : dt * ct0;
  const double rq1 = ct1, rx1 = dt * ct1;
  const int fe = s / 3, fi = s - 3 * fe;
  const double rf = (running && fe < 4) ? ((fi == 0) ? Rg[0] : (fi == 1) ? Rg[1] : Rg[2]) / 4 : 0.0;
  // ---- out: zero rows for a non-finite instance; nothing non-finite leaves the instance
  const bool obad = (h0 && (!is_finite(rq0) || !is_finite(rx0))) || (h1 && (!is_finite(rq1) || !is_finite(rx1))) || !is_finite(rf);
  const bool zero = ((__ballot(bad || obad) >> T.rbase) & 0xFFFFull) != 0ull;
  if (!T.valid) return;
  if (A.out.d_q) {
    A.out.d_q[b * NV + d0] = (zero || !h0) ? 0.0 : rq0;
    if (d1 < NV) A.out.d_q[b * NV + d1] = (zero || !h1) ? 0.0 : rq1;
  }
  if (A.out.d_qdot) {
    A.out.d_qdot[b * NV + d0] = (zero || !h0) ? 0.0 : rx0;
    if (d1 < NV) A.out.d_qdot[b * NV + d1] = (zero || !h1) ? 0.0 : rx1;
  }
  if (A.out.d_foot_targets && s < 15) A.out.d_foot_targets[b * 15 + s] = zero ? 0.0 : rf;
  if (s == 0 && A.out.grad_status) A.out.grad_status[b] = zero ? GRAD_NONFINITE : GRAD_OK;
}

// The variants (wbc_common.h, "Kernel variant tables"): the part that instantiates the row, then the template arguments.
#ifndef STEPVJP_PART
#define STEPVJP_PART -1      // -1: everything in one unit
#endif
#define WBC_PART STEPVJP_PART
#define WBC_KERNEL wbc_stepvjp_kernel
#define WBC_KPARAMS (const StepVjpArgs, const DevModel* __restrict__, const DevPlan* __restrict__)
typedef void (*StepVjpKernel) WBC_KPARAMS;
#define STEPVJP_VARIANTS(V) /* ROT */ \
  V(0, false) \
  V(0, true)
#if STEPVJP_PART == -1
STEPVJP_VARIANTS(WBC_VARIANT_INST)
#else
STEPVJP_VARIANTS(WBC_VARIANT_UNIT)
#endif
#if STEPVJP_PART <= 0
static StepVjpKernel stepvjp_variant(long long key) {
  STEPVJP_VARIANTS(WBC_VARIANT_FIND)
  return nullptr;
}
int stepvjp_variant_count() { return 0 STEPVJP_VARIANTS(WBC_VARIANT_COUNT); }
int launch_stepvjp(const StepVjpArgs& a, void* stream, long long* key_out) {
  const long long key = variant_key(a.rot != 0);
  if (key_out) *key_out = key;
  const StepVjpKernel k = stepvjp_variant(key);
  if (!k) return WBC_E_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3((a.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, a, a.models, a.plans);
  return check_launch("step_vjp");
}
#endif

}  // namespace wbc
