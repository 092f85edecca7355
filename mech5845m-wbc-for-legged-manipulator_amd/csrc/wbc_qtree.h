// wbc_qtree.h — what the whole-tree kernels share (internal, C++): wbc_k_grad.hip, wbc_k_gradq.hip, wbc_k_slack.hip,
// wbc_k_stepvjp.hip, wbc_k_scorevjp.hip and wbc_k_slackvjp.hip, and no other unit. Their common shape: four instances per wavefront (lane = 16 r + s), FK over
// the whole-tree schedule DevPlan.q_fk, lane s owning DoF s and 16 + s (and bodies s and 16 + s), sums over DoF by DPP row butterflies.
// Everything is inlined into its caller and works on the caller's LDS block; a function keeps the operation order its callers had (their bits).
// Floating-point contraction is the including unit's: wbc_k_scorevjp.hip includes this header behind its `fp contract(off)`.
#pragma once
#define WBC_QTREE_H 1      // (wbc_k_scorevjp.hip checks that no earlier include brought this header in)
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_grad.h"

namespace wbc {

// ---- 1. lane and instance. Rows past the batch compute on the last instance and store nothing (valid).
struct QtLane {
  int lane, r, s, rbase, b_raw; bool valid; size_t b;
  __device__ __forceinline__ explicit QtLane(const int B) : lane(threadIdx.x), r(lane >> 4), s(lane & 15), rbase(lane & 48),
                                                            b_raw(4 * blockIdx.x + r), valid(b_raw < B), b(valid ? b_raw : B - 1) {}
};
// model index of instance b, clamped to the handle's models. Not wbc_common.h's model_index: that one makes the index wave-uniform by
// readfirstlane, and a wave here holds four instances, each with a model of its own — the select is per lane.
__device__ __forceinline__ int qt_model_index(const int32_t* const model_id, const size_t b, const int n_models) {
  int mid = 0;
  if (model_id) { mid = model_id[b]; mid = mid < 0 ? 0 : (mid >= n_models ? n_models - 1 : mid); }
  return mid;
}

// ---- 2. the kinematics block: the leading member of an instance's LDS record
struct QtKin {
  double oMi[24 * 12];                      // joint j: R column-major, then p
  double q[32];                             // the configuration the kinematics run at
  double sc[64];                            // sin / cos of joint j at 2 j
};
// stage q, seed, sweep (pin.forwardKinematics, level by level). scq0 / scq1, fkn: DevPlan.q_scq of joints 2 + s, 18 + s and q_fk[0][s], loaded by the
// caller with its other global reads. Ends fenced: oMi is complete on return.
template <bool ROT>
__device__ __forceinline__ void qt_fk(QtKin& K, const double q0, const double q1, const int scq0, const int scq1, const DevModel& M,
                                      const DevPlan& P, DevPlan::PkJoint& fkn, const int s) {
  K.q[s] = q0; K.q[16 + s] = q1;
  WSYNC();
  pk_fk_seed(K.oMi, K.sc, K.q, scq0, scq1, s);
  WSYNC();
  pk_fk_sweep<ROT>(K.oMi, K.sc, K.q, M, P.q_fk, fkn, s);
}

// ---- 3. the lane's two DoF and where their WORLD Jacobian columns come from
struct QtDof {
  int d0, d1; bool h0, h1;                  // DoF of this lane, and whether the model has them
  int cj0, cl0, ca0, cj1, cl1, ca1;         // col_joint / col_lin / col_ang of each
  __device__ __forceinline__ QtDof(const DevModel& M, const int s, const int nv)
      : d0(s), d1(16 + s), h0(d0 < nv), h1(d1 < nv), cj0(M.col_joint[h0 ? d0 : 0]), cl0(M.col_lin[h0 ? d0 : 0]), ca0(M.col_ang[h0 ? d0 : 0]),
        cj1(M.col_joint[h1 ? d1 : 0]), cl1(M.col_lin[h1 ? d1 : 0]), ca1(M.col_ang[h1 ? d1 : 0]) {}
};
// computeJointJacobians: linear part at the world origin, angular part; zero for a DoF the model lacks
__device__ __forceinline__ void qt_jac_cols(const double* const oMi, const QtDof& D, double (&l0)[3], double (&a0)[3], double (&l1)[3],
                                            double (&a1)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) { l0[i] = 0.0; a0[i] = 0.0; l1[i] = 0.0; a1[i] = 0.0; }
  if (D.h0) pk_jac_col(oMi, D.cj0, D.cl0, D.ca0, l0, a0);
  if (D.h1) pk_jac_col(oMi, D.cj1, D.cl1, D.ca1, l1, a1);
}

// ---- 4. component i of p + R c for a placement Pj (a frame's origin, a body's centre of mass), and a frame's origin from the model's tables
__device__ __forceinline__ double qt_point(const double* const Pj, const double c0, const double c1, const double c2, const int i) {
  return Pj[9 + i] + Pj[i] * c0 + Pj[3 + i] * c1 + Pj[6 + i] * c2;
}
__device__ __forceinline__ void qt_frame_origin(const double* const oMi, const DevModel& M, const int fr, double (&pf)[3]) {
  const double* Pj = oMi + 12 * M.frame_joint[fr];
  const double f0 = M.frame_p[fr][0], f1 = M.frame_p[fr][1], f2 = M.frame_p[fr][2];
#pragma unroll
  for (int i = 0; i < 3; ++i) pf[i] = qt_point(Pj, f0, f1, f2, i);
}

// ---- 5. the task image of the tick gradients: wt [96], the 85 weights and gains (wbc_packed.h WT_*), rest zero; tin [TI_N], the task inputs
constexpr int TI_EE = 0, TI_EEP = 15, TI_TR = 30, TI_CT = 48, TI_CV = 51, TI_PU = 54, TI_OM = 80, TI_N = 96;
// Entry k of the staged inputs; an input the configuration does not read is 0 and is never loaded
__device__ __forceinline__ double qt_task_input(const WbcTickIn& in, const size_t b, const int k, const unsigned eemask, const bool trunk,
                                                const bool com, const bool pu) {
  if (k < TI_TR) {
    const int kk = (k < TI_EEP) ? k : k - TI_EEP, e = kk / 3;
    if (!((eemask >> e) & 1u)) return 0.0;
    return (k < TI_EEP) ? in.ee_target[b * 15 + kk] : in.prev_ee_target[b * 15 + kk];
  }
  if (k < TI_CT) return trunk ? pk_trunk_input(in, (int)b, k - TI_TR) : 0.0;
  if (k < TI_CV) return com ? in.com_target[b * 3 + (k - TI_CT)] : 0.0;
  if (k < TI_PU) return com ? in.com_target_vel[b * 3 + (k - TI_CV)] : 0.0;
  if (k < TI_PU + NV) return pu ? in.posture_u[b * NV + (k - TI_PU)] : 0.0;
  return 0.0;
}
// wt from the instance's row of tp (null: the configuration's block), tin in five passes, calcTargetVelEE3's feed-forward at TI_OM (one
// component per lane). Returns whether this lane staged something non-finite. The caller fences.
__device__ __forceinline__ bool qt_stage_task_image(double* const wt, double* const tin, const WbcTickIn& in, const WbcTaskParams* const tp,
                                                    const WbcConfig& cfg, const size_t b, const int s, const unsigned eemask, const bool trunk,
                                                    const bool com, const bool pu, const double inv_dt) {
  const double* cw = &cfg.ee_W[0][0];
  const double* rw = tp ? reinterpret_cast<const double*>(tp + b) : cw;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int k = s + 16 * i;
    const double v = (k < WBC_TASK_PARAMS_DOUBLES) ? rw[k] : 0.0;
    bad = bad || !is_finite(v);
    wt[k] = v;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int k = s + 16 * i;
    const double v = qt_task_input(in, b, k, eemask, trunk, com, pu);
    bad = bad || !is_finite(v);
    tin[k] = v;
  }
  const double om = (eemask >> ((s < 15 ? s : 0) / 3) & 1u) ? pk_ee_omega(in, (int)b, s, inv_dt) : 0.0;
  bad = bad || !is_finite(om);
  tin[TI_OM + s] = om;
  return bad;
}

// ---- 6. the trunk frame and calcTargetVelTrunk2 (Robot_Wrapper4.py:948-1015) on the recomputed kinematics: ptr, the frame's origin; with `task`
// also fq, the frame's quaternion, rq, the reference's, tqe, the literal qe, and tvel [6] (without it only ptr is touched: a trunk box alone).
// sh [12]: LDS scratch of the instance (sines / cosines of the reference angles and their halves, one per lane); fences once inside.
// Bug-compatible with the reference on purpose, as pk_trunk_target_vel: qe2's first two terms cancel (:976), and the skew matrix is D R*, not
// D R*^T (:984). The gradient kernels' one statement of it: a change here reaches both.
__device__ __forceinline__ void qt_trunk_target(const double* const oMi, const DevModel& M, const double* const tin, const double* const wt,
                                                double* const sh, const double inv_dt, const int s, const bool task, double (&ptr)[3],
                                                double (&fq)[4], double (&rq)[4], double (&tqe)[3], double (&tvel)[6]) {
  qt_frame_origin(oMi, M, WBC_FR_TRUNK, ptr);
  if (!task) return;
  const double* Pt = oMi + 12 * M.frame_joint[WBC_FR_TRUNK];       // R column-major: R(i, j) = Pt[3 j + i]
  double Rtr[9], Rs[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rtr[3 * i + j] = Pt[3 * j + i];
  R_to_quat(Rtr, fq);
  const double *xt = tin + TI_TR, *xp = tin + TI_TR + 3, *er = tin + TI_TR + 6;
  const SinCos t = sincos_cw(s < 3 ? er[s < 3 ? s : 0] : 0.5 * er[(s < 6 ? s : 3) - 3]);   // reference angles and their halves, one per lane
  if (s < 6) { sh[2 * s] = t.s; sh[2 * s + 1] = t.c; }
  WSYNC();
  euler_to_R(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], Rs);
  const double qx[4] = {sh[6], 0, 0, sh[7]}, qy[4] = {0, sh[8], 0, sh[9]}, qz[4] = {0, 0, sh[10], sh[11]};
  double tq[4];
  quat_mul(qy, qx, tq);
  quat_mul(qz, tq, rq);
  tqe[0] = fq[3] * rq[0] - fq[0] * rq[3] + fq[1] * rq[2] - fq[2] * rq[1];   // :974
  tqe[1] = fq[3] * rq[1] - fq[1] * rq[3] - fq[0] * rq[2] + fq[2] * rq[0];   // :975
  tqe[2] = fq[3] * rq[2] - fq[3] * rq[2] + fq[0] * rq[1] - fq[1] * rq[0];   // :976 (sic)
  double D[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) D[i] = (Rs[i] - tin[TI_TR + 9 + i]) * inv_dt;
#pragma unroll
  for (int i = 0; i < 3; ++i) tvel[i] = (xt[i] - xp[i]) * inv_dt + wt[WT_TG + i] * ((xt[i] - ptr[i]) * inv_dt);
  // skew = D Rs (R*, not R*^T: :984); omega = (S[2][1], S[0][2], S[1][0]) + K qe
  tvel[3] = (D[6] * Rs[1] + D[7] * Rs[4] + D[8] * Rs[7]) + wt[WT_TG + 3] * tqe[0];
  tvel[4] = (D[0] * Rs[2] + D[1] * Rs[5] + D[2] * Rs[8]) + wt[WT_TG + 4] * tqe[1];
  tvel[5] = (D[3] * Rs[0] + D[4] * Rs[3] + D[5] * Rs[6]) + wt[WT_TG + 5] * tqe[2];
}

// ---- 7. the CoM pieces. mcw [24][4], body j: m_j (R_j c_j + p_j), then m_j; lane s writes bodies s (>= 1) and 16 + s (m0, m1: their q_jm records). The caller fences.
__device__ __forceinline__ void qt_body_mass_table(double* const mcw, const double* const oMi, const DevPlan::QJnt& m0, const DevPlan::QJnt& m1,
                                                   const bool hb0, const bool hb1, const int s) {
  const int j1 = 16 + s;
  const double* Pa = oMi + 12 * (hb0 ? s : 1);
  const double* Pb = oMi + 12 * (hb1 ? j1 : 1);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double ca = qt_point(Pa, m0.c0, m0.c1, m0.c2, i);
    const double cb = qt_point(Pb, m1.c0, m1.c1, m1.c2, i);
    mcw[4 * s + i] = hb0 ? m0.m * ca : 0.0;
    if (j1 < 24) mcw[4 * j1 + i] = hb1 ? m1.m * cb : 0.0;
  }
  mcw[4 * s + 3] = hb0 ? m0.m : 0.0;
  if (j1 < 24) mcw[4 * j1 + 3] = hb1 ? m1.m : 0.0;
}
// mc, ms <- the sums of m_j c_j and m_j over the bodies of mask, in increasing order
__device__ __forceinline__ void qt_subtree_mass(const double* const mcw, unsigned mask, double (&mc)[3], double& ms) {
  mc[0] = mc[1] = mc[2] = 0.0; ms = 0.0;
  while (mask) {
    const int j = __ffs((int)mask) - 1; mask &= mask - 1;
    mc[0] += mcw[4 * j]; mc[1] += mcw[4 * j + 1]; mc[2] += mcw[4 * j + 2]; ms += mcw[4 * j + 3];
  }
}

// ---- 8. row k of a Cartesian task block (frame f: an end effector's LOCAL_WORLD_ALIGNED rows, endEffectorA2 :474-484, else the trunk's WORLD rows,
// trunkA :487-490): vel (calcTargetVelEE3 :1063, :1070 at the frame origin pf, TI_OM's feed-forward; the trunk's is tvel), c = W_k w, sv = c (J u)_k, rho = w vel - c (J x)_k.
struct QtRow { double vel, c, sv, rho; };
__device__ __forceinline__ QtRow qt_task_row(const double* const wt, const double* const tin, const double (&tvel)[6], const double (&pf)[3],
                                             const bool ee, const int f, const int k, const double w, const double jxk, const double juk,
                                             const double inv_dt) {
  const int oW = ee ? WT_W + 6 * f : WT_TW, oG = ee ? WT_G + 6 * f : WT_TG, fe = ee ? f : 0;
  const double *xt = tin + TI_EE + 3 * fe, *xp = tin + TI_EEP + 3 * fe;
  QtRow o;
  if (k < 3) o.vel = ee ? (xt[k] - xp[k]) * inv_dt + wt[oG + k] * ((xt[k] - pf[k]) * inv_dt) : tvel[k];
  else o.vel = ee ? tin[TI_OM + 3 * fe + (k - 3)] : tvel[k];
  o.c = wt[oW + k] * w;
  o.sv = o.c * juk;
  o.rho = fma(w, o.vel, -(o.c * jxk));
  return o;
}

// ---- 9. the exit rule of the tick gradients: unsolved, then uncertified, then anything non-finite on a lane of the instance's row
__device__ __forceinline__ int qt_grad_status(const int st, const int cst, const bool bad, const int rbase) {
  const bool nonfin = ((__ballot(bad) >> rbase) & 0xFFFFull) != 0ull;
  return st != 0 ? GRAD_UNSOLVED : (cst != 0 ? GRAD_CERT : (nonfin ? GRAD_NONFINITE : GRAD_OK));
}

}  // namespace wbc
