// wbc_k_grad.hip — wbc_tick_vjp: dL/d(task weights, gains, targets) of a solved tick from x = qdot and the certificate's u = sens_x
// (include/wbc.h). With r = b - A x and s = A u the chain is dL/dA = r u' - s x', dL/db = s, and every task row is
// (weights) x (an unweighted Jacobian row): the kernel never forms A, H or a Jacobian. It recomputes the kinematics from q (the task rows
// see q, not q_con), sums the WORLD twists  sum_d col_d x_d  and  sum_d col_d u_d  of each task frame over the frame's support — J_r x and
// J_r u of all six rows of the frame at once — and applies the block rules of include/wbc.h.
// One kernel, wbc_slack_kernel's shape: four instances per wavefront (lane = 16 r + s), FK over the whole-tree schedule DevPlan.q_fk.
// Lane s owns the DoF s and 16 + s (their WORLD Jacobian columns, pk_jac_col) and the bodies s and 16 + s (the CoM); sums over DoF are DPP row
// butterflies. The 85 + 42 results of an instance are collected in LDS (zero-initialised: a switched-off task's entries are never touched)
// and leave in coalesced stores. Reads its inputs and the tables; writes nothing but its outputs, rows [0, B) only.
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_grad.h"

namespace wbc {

// tin: the staged task inputs of an instance
constexpr int GI_EE = 0, GI_EEP = 15, GI_TR = 30, GI_CT = 48, GI_CV = 51, GI_PU = 54, GI_OM = 80, GI_N = 96;
// tout: the target gradients of an instance
constexpr int GO_EE = 0, GO_EEP = 15, GO_TT = 30, GO_TP = 33, GO_CT = 36, GO_CV = 39, GO_N = 42;
constexpr int WT_TW = 65, WT_Tw = 71, WT_TG = 72, WT_JW = 84;   // trunk_W, trunk_w, trunk_gain, joint_w inside the weights image (wbc_packed.h WT_*)
static_assert(offsetof(WbcTaskParams, trunk_W) == WT_TW * sizeof(double) && offsetof(WbcTaskParams, trunk_w) == WT_Tw * sizeof(double) &&
              offsetof(WbcTaskParams, trunk_gain) == WT_TG * sizeof(double) && offsetof(WbcTaskParams, joint_w) == WT_JW * sizeof(double) &&
              offsetof(WbcTaskParams, ee_w) == WT_w * sizeof(double) && offsetof(WbcTaskParams, ee_gain) == WT_G * sizeof(double) &&
              offsetof(WbcTaskParams, com_W) == WT_CW * sizeof(double) && offsetof(WbcTaskParams, com_gain) == WT_CG * sizeof(double),
              "the weights image is WbcTaskParams, double for double");

struct __attribute__((aligned(16))) GInst {
  double oMi[24 * 12];
  double q[32];
  double sc[64];
  double wt[96];                            // the 85 weights and gains (WbcTaskParams layout), rest zero
  double tin[GI_N];
  double mcw[24 * 4];                       // body j: m_j (R_j c_j + p_j), then m_j
  double sh[16];
  double gout[96];                          // d_task_params of the instance
  double tout[48];                          // d_ee_target [15], d_prev_ee_target [15], d_trunk_target, d_prev_trunk_target, d_com_target, d_com_target_vel
};
struct __attribute__((aligned(16))) GSmemP { GInst I[4]; };

// Entry k of the staged inputs; an input the configuration does not read is 0 and is never loaded
__device__ __forceinline__ double grad_input(const WbcTickIn& in, const size_t b, const int k, const unsigned eemask, const bool trunk, const bool com,
                                             const bool pu) {
  if (k < GI_TR) {
    const int kk = (k < GI_EEP) ? k : k - GI_EEP, e = kk / 3;
    if (!((eemask >> e) & 1u)) return 0.0;
    return (k < GI_EEP) ? in.ee_target[b * 15 + kk] : in.prev_ee_target[b * 15 + kk];
  }
  if (k < GI_CT) return trunk ? pk_trunk_input(in, (int)b, k - GI_TR) : 0.0;
  if (k < GI_CV) return com ? in.com_target[b * 3 + (k - GI_CT)] : 0.0;
  if (k < GI_PU) return com ? in.com_target_vel[b * 3 + (k - GI_CV)] : 0.0;
  if (k < GI_PU + NV) return pu ? in.posture_u[b * NV + (k - GI_PU)] : 0.0;
  return 0.0;
}

template <bool ROT>   // ROT: rotated joint placements in the batch (wbc_k_sim3p.hip)
__global__ void __launch_bounds__(64) wbc_grad_kernel(const GradArgs A, const DevModel* __restrict__ models, const WbcConfig* __restrict__ cfgs,
                                                      const DevPlan* __restrict__ plans) {
  __shared__ GSmemP SP;
  const int lane = threadIdx.x, r = lane >> 4, s = lane & 15, rbase = lane & 48;
  GInst& U = SP.I[r];
  const int b_raw = 4 * blockIdx.x + r;
  const bool valid = b_raw < A.B;
  const size_t b = valid ? b_raw : A.B - 1;
  int mid = 0;
  if (A.in.model_id) { mid = A.in.model_id[b]; mid = mid < 0 ? 0 : (mid >= A.n_models ? A.n_models - 1 : mid); }
  const DevModel& M = models[mid];
  const WbcConfig& cfg = cfgs[mid];
  const DevPlan& P = plans[mid];
  const int nq = M.nq, nv = M.nv, nj = M.njoints;
  const double inv_dt = 1.0 / A.dt;
  // ---- the switches (the same for every model of the batch: check_batch)
  unsigned eemask = 0u;
#pragma unroll
  for (int e = 0; e < WBC_NEE; ++e) eemask |= cfg.task_ee[e] ? 1u << e : 0u;
  const bool t_trunk = cfg.task_trunk != 0, t_com = cfg.task_com != 0;
  const int t_joint = cfg.task_joint;
  const bool pu_static = t_joint >= WBC_JOINT_MANI && !A.in.posture_u;      // (the host hands posture_u on unless every sweep is structurally zero)
  const bool pu_read = t_joint >= WBC_JOINT_MANI && A.in.posture_u;
  // ---- every global read first
  const double* qg = A.in.q + b * NQ;
  const double q0 = qg[s], q1 = (16 + s < nq) ? qg[16 + s] : 0.0;
  const int d0 = s, d1 = 16 + s;                                    // DoF of this lane
  const bool h0 = d0 < nv, h1 = d1 < nv;
  const double xd0 = h0 ? A.qdot[b * NV + d0] : 0.0, xd1 = h1 ? A.qdot[b * NV + d1] : 0.0;
  const double ud0 = h0 ? A.sens_x[b * NV + d0] : 0.0, ud1 = h1 ? A.sens_x[b * NV + d1] : 0.0;
  const int st = A.status ? A.status[b] : 0, cst = A.cert_status ? A.cert_status[b] : 0;
  DevPlan::PkJoint fkn = P.q_fk[0][s];
  const int scq0 = P.q_scq[(2 + s) & 31], scq1 = P.q_scq[(18 + s) & 31];
  const int cj0 = M.col_joint[h0 ? d0 : 0], cl0 = M.col_lin[h0 ? d0 : 0], ca0 = M.col_ang[h0 ? d0 : 0];
  const int cj1 = M.col_joint[h1 ? d1 : 0], cl1 = M.col_lin[h1 ? d1 : 0], ca1 = M.col_ang[h1 ? d1 : 0];
  const unsigned sub0 = h0 ? M.col_subtree[d0] : 0u, sub1 = h1 ? M.col_subtree[d1] : 0u;
  const int j1 = 16 + s;                                            // bodies of this lane: joints s (>= 1) and 16 + s
  const bool hb0 = s >= 1 && s < nj, hb1 = j1 < nj;
  const DevPlan::QJnt m0 = P.q_jm[hb0 ? s : 1], m1 = P.q_jm[hb1 ? j1 : 1];
  bool bad = (s < nq && !is_finite(q0)) || (16 + s < nq && !is_finite(q1)) || !is_finite(xd0) || !is_finite(xd1) || !is_finite(ud0) ||
             !is_finite(ud1);
  {
    const double* cw = &cfg.ee_W[0][0];
    const double* rw = A.tp ? reinterpret_cast<const double*>(A.tp + b) : cw;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int k = s + 16 * i;
      const double v = (k < WBC_TASK_PARAMS_DOUBLES) ? rw[k] : 0.0;
      bad = bad || !is_finite(v);
      U.wt[k] = v;
      U.gout[k] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = s + 16 * i;
      const double v = grad_input(A.in, b, k, eemask, t_trunk, t_com, pu_read);
      bad = bad || !is_finite(v);
      U.tin[k] = v;
    }
    const double om = (eemask >> ((s < 15 ? s : 0) / 3) & 1u) ? pk_ee_omega(A.in, (int)b, s, inv_dt) : 0.0;   // calcTargetVelEE3's feed-forward, one component per lane
    bad = bad || !is_finite(om);
    U.tin[GI_OM + s] = om;
#pragma unroll
    for (int i = 0; i < 3; ++i) U.tout[s + 16 * i] = 0.0;
  }
  U.q[s] = q0; U.q[16 + s] = q1;
  WSYNC();
  const double* const qv = U.q;
  double* const oMi = U.oMi;
  const double* const wt = U.wt;
  const double* const tin = U.tin;
  pk_fk_seed(oMi, U.sc, qv, scq0, scq1, s);
  WSYNC();
  pk_fk_sweep<ROT>(oMi, U.sc, qv, M, P.q_fk, fkn, s);               // pin.forwardKinematics over every joint, level by level
  // ---- WORLD Jacobian columns of the lane's two DoF (computeJointJacobians: linear part at the world origin, angular part)
  double l0[3] = {0.0, 0.0, 0.0}, a0[3] = {0.0, 0.0, 0.0}, l1[3] = {0.0, 0.0, 0.0}, a1[3] = {0.0, 0.0, 0.0};
  if (h0) pk_jac_col(oMi, cj0, cl0, ca0, l0, a0);
  if (h1) pk_jac_col(oMi, cj1, cl1, ca1, l1, a1);
  // ---- the trunk frame and calcTargetVelTrunk2 (Robot_Wrapper4.py:948-1015), bug-compatible as pk_trunk_target_vel: vel [6], the literal qe [3]
  double tvel[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tqe[3] = {0.0, 0.0, 0.0}, ptr[3] = {0.0, 0.0, 0.0};
  if (t_trunk) {
    const double* Pt = oMi + 12 * M.frame_joint[WBC_FR_TRUNK];
    const double f0 = M.frame_p[WBC_FR_TRUNK][0], f1 = M.frame_p[WBC_FR_TRUNK][1], f2 = M.frame_p[WBC_FR_TRUNK][2];
    double Rtr[9], fq[4], rq[4], Rs[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ptr[i] = Pt[9 + i] + Pt[i] * f0 + Pt[3 + i] * f1 + Pt[6 + i] * f2;
#pragma unroll
      for (int j = 0; j < 3; ++j) Rtr[3 * i + j] = Pt[3 * j + i];
    }
    R_to_quat(Rtr, fq);
    const double* xt = tin + GI_TR;
    const double* xp = tin + GI_TR + 3;
    const double* er = tin + GI_TR + 6;
    const SinCos t = sincos_cw(s < 3 ? er[s < 3 ? s : 0] : 0.5 * er[(s < 6 ? s : 3) - 3]);   // reference angles and their halves, one per lane
    if (s < 6) { U.sh[2 * s] = t.s; U.sh[2 * s + 1] = t.c; }
    WSYNC();
    const double* sh = U.sh;
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
    for (int i = 0; i < 9; ++i) D[i] = (Rs[i] - tin[GI_TR + 9 + i]) * inv_dt;
#pragma unroll
    for (int i = 0; i < 3; ++i) tvel[i] = (xt[i] - xp[i]) * inv_dt + wt[WT_TG + i] * ((xt[i] - ptr[i]) * inv_dt);
    // skew = D Rs (R*, not R*^T: :984); omega = (S[2][1], S[0][2], S[1][0]) + K qe
    tvel[3] = (D[6] * Rs[1] + D[7] * Rs[4] + D[8] * Rs[7]) + wt[WT_TG + 3] * tqe[0];
    tvel[4] = (D[0] * Rs[2] + D[1] * Rs[5] + D[2] * Rs[8]) + wt[WT_TG + 4] * tqe[1];
    tvel[5] = (D[3] * Rs[0] + D[4] * Rs[3] + D[5] * Rs[6]) + wt[WT_TG + 5] * tqe[2];
  }
  // ---- Cartesian blocks: EE 0..4 (LOCAL_WORLD_ALIGNED rows, endEffectorA2 :474-484) and the trunk (WORLD rows, trunkA :487-490)
#pragma unroll 1
  for (int f = 0; f < WBC_NEE + 1; ++f) {
    const bool ee = f < WBC_NEE;
    if (ee ? !((eemask >> f) & 1u) : !t_trunk) continue;             // (wave-uniform: the switches are the batch's)
    const int fr = ee ? WBC_FR_EE0 + f : WBC_FR_TRUNK;
    const unsigned sup = M.frame_support[fr];
    const bool on0 = h0 && ((sup >> d0) & 1u), on1 = h1 && ((sup >> (d1 & 31)) & 1u);
    const double x0 = on0 ? xd0 : 0.0, x1 = on1 ? xd1 : 0.0, u0 = on0 ? ud0 : 0.0, u1 = on1 ? ud1 : 0.0;
    double jx[6], ju[6];                                             // the frame's WORLD twist under x and under u
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      jx[c] = rsum16(fma(l0[c], x0, l1[c] * x1)); jx[3 + c] = rsum16(fma(a0[c], x0, a1[c] * x1));
      ju[c] = rsum16(fma(l0[c], u0, l1[c] * u1)); ju[3 + c] = rsum16(fma(a0[c], u0, a1[c] * u1));
    }
    const double* Pj = oMi + 12 * M.frame_joint[fr];
    const double f0 = M.frame_p[fr][0], f1 = M.frame_p[fr][1], f2 = M.frame_p[fr][2];
    double pf[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pf[i] = Pj[9 + i] + Pj[i] * f0 + Pj[3 + i] * f1 + Pj[6 + i] * f2;
    if (ee) {                                                        // reference point at the frame origin: lin + ang x p
      double cx[3], cu[3];
      cross3(jx + 3, pf, cx); cross3(ju + 3, pf, cu);
#pragma unroll
      for (int i = 0; i < 3; ++i) { jx[i] += cx[i]; ju[i] += cu[i]; }
    }
    const int oW = ee ? WT_W + 6 * f : WT_TW, ow = ee ? WT_w + f : WT_Tw, oG = ee ? WT_G + 6 * f : WT_TG;
    const double* xt = ee ? tin + GI_EE + 3 * f : tin + GI_TR;
    const double* xp = ee ? tin + GI_EEP + 3 * f : tin + GI_TR + 3;
    const double w = wt[ow];
    double vel[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      vel[i] = ee ? (xt[i] - xp[i]) * inv_dt + wt[oG + i] * ((xt[i] - pf[i]) * inv_dt) : tvel[i];   // calcTargetVelEE3 :1063, :1070
      vel[3 + i] = ee ? tin[GI_OM + 3 * f + i] : tvel[3 + i];
    }
    double dw = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double W = wt[oW + k], c = W * w;
      const double sv = c * ju[k], rho = fma(w, vel[k], -(c * jx[k]));
      const double t = fma(rho, ju[k], -(sv * jx[k]));
      const double dvel = w * sv;
      dw += fma(W, t, sv * vel[k]);
      if (s == 0) {
        U.gout[oW + k] = w * t;
        if (k < 3) {
          U.gout[oG + k] = dvel * ((xt[k] - pf[k]) * inv_dt);
          U.tout[(ee ? GO_EE + 3 * f : GO_TT) + k] = dvel * (1.0 + wt[oG + k]) * inv_dt;
          U.tout[(ee ? GO_EEP + 3 * f : GO_TP) + k] = -dvel * inv_dt;
        } else if (!ee) {
          U.gout[oG + k] = dvel * tqe[k - 3];
        }
      }
    }
    if (s == 0) U.gout[ow] = dw;
  }
  // ---- CoM block (Robot_Wrapper2 comJacobian :600-603, cartesianTargetCoM :661-668): column d of Jcom is (m_sub lin_d + ang_d x mc_sub) / M over
  // the sub-tree of the DoF's joint
  if (t_com) {
    {
      const double* Pa = oMi + 12 * (hb0 ? s : 1);
      const double* Pb = oMi + 12 * (hb1 ? j1 : 1);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double ca = Pa[9 + i] + Pa[i] * m0.c0 + Pa[3 + i] * m0.c1 + Pa[6 + i] * m0.c2;
        const double cb = Pb[9 + i] + Pb[i] * m1.c0 + Pb[3 + i] * m1.c1 + Pb[6 + i] * m1.c2;
        U.mcw[4 * s + i] = hb0 ? m0.m * ca : 0.0;
        if (j1 < 24) U.mcw[4 * j1 + i] = hb1 ? m1.m * cb : 0.0;
      }
      U.mcw[4 * s + 3] = hb0 ? m0.m : 0.0;
      if (j1 < 24) U.mcw[4 * j1 + 3] = hb1 ? m1.m : 0.0;
    }
    WSYNC();
    double com[3], cm;
    {
      const double* a = U.mcw + 4 * s;
      const double* c = U.mcw + 4 * (j1 < 24 ? j1 : 0);
      const bool two = j1 < 24;
      cm = rsum16(a[3] + (two ? c[3] : 0.0));
#pragma unroll
      for (int i = 0; i < 3; ++i) com[i] = rsum16(a[i] + (two ? c[i] : 0.0)) / cm;
    }
    double c0[3], c1[3];                                             // M x column d of Jcom
    {
      double mc[3] = {0.0, 0.0, 0.0}, ms = 0.0, cr[3];
      unsigned mask = sub0 & 0x00FFFFFEu;
      while (mask) { const int j = __ffs((int)mask) - 1; mask &= mask - 1; mc[0] += U.mcw[4 * j]; mc[1] += U.mcw[4 * j + 1]; mc[2] += U.mcw[4 * j + 2]; ms += U.mcw[4 * j + 3]; }
      cross3(a0, mc, cr);
#pragma unroll
      for (int i = 0; i < 3; ++i) c0[i] = fma(ms, l0[i], cr[i]);
      mc[0] = mc[1] = mc[2] = 0.0; ms = 0.0;
      mask = sub1 & 0x00FFFFFEu;
      while (mask) { const int j = __ffs((int)mask) - 1; mask &= mask - 1; mc[0] += U.mcw[4 * j]; mc[1] += U.mcw[4 * j + 1]; mc[2] += U.mcw[4 * j + 2]; ms += U.mcw[4 * j + 3]; }
      cross3(a1, mc, cr);
#pragma unroll
      for (int i = 0; i < 3; ++i) c1[i] = fma(ms, l1[i], cr[i]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double jx = rsum16(fma(c0[k], xd0, c1[k] * xd1)) / cm, ju = rsum16(fma(c0[k], ud0, c1[k] * ud1)) / cm;
      const double W = wt[WT_CW + k], g = wt[WT_CG + k];
      const double e = tin[GI_CT + k] - com[k], bv = tin[GI_CV + k] + g * e;
      const double sv = W * ju, rho = fma(-W, jx, bv);
      if (s == 0) {
        U.gout[WT_CW + k] = fma(rho, ju, -(sv * jx));
        U.gout[WT_CG + k] = sv * e;
        U.tout[GO_CT + k] = sv * g;
        U.tout[GO_CV + k] = sv;
      }
    }
  }
  // ---- posture block (qpJointA :1199-1206, qpJointb :1209-1268): d = joint_w / nv on the diagonal, b_k = d up_k
  double pu0 = 0.0, pu1 = 0.0;
  if (t_joint) {
    const double d = (1.0 / nv) * wt[WT_JW];
    double up0 = 0.0, up1 = 0.0;
    if (t_joint >= WBC_JOINT_PREV) {
      const double p0 = qv[d0 < 6 ? d0 : d0 + 1], p1 = qv[(d1 + 1) & 31];   // np.delete(q, 6) :1216-1217
      up0 = p0; up1 = p1;
      if (t_joint >= WBC_JOINT_MANI) {
        if (pu_static) { up0 = ((P.post_zero >> d0) & 1u) ? 0.0 : p0; up1 = ((P.post_zero >> (d1 & 31)) & 1u) ? 0.0 : p1; }
        else { up0 = tin[GI_PU + d0]; up1 = tin[GI_PU + (h1 ? d1 : 0)]; }
      }
    }
    const double t0 = h0 ? d * (up0 - xd0) * ud0 : 0.0, t1 = h1 ? d * (up1 - xd1) * ud1 : 0.0;
    const double sum = rsum16(t0 + t1);
    if (s == 0) U.gout[WT_JW] = (2.0 / nv) * sum;
    if (t_joint >= WBC_JOINT_MANI) { pu0 = (d * d) * ud0; pu1 = (d * d) * ud1; }
  }
  WSYNC();
  // ---- out: zero rows for an unsolved / uncertified / non-finite instance; nothing non-finite leaves the instance
  double go[6], to[3];
  bool obad = !is_finite(pu0) || !is_finite(pu1);
#pragma unroll
  for (int i = 0; i < 6; ++i) { go[i] = U.gout[s + 16 * i]; obad = obad || !is_finite(go[i]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { to[i] = U.tout[s + 16 * i]; obad = obad || !is_finite(to[i]); }
  const bool nonfin = ((__ballot(bad || obad) >> rbase) & 0xFFFFull) != 0ull;
  const int gs = st != 0 ? GRAD_UNSOLVED : (cst != 0 ? GRAD_CERT : (nonfin ? GRAD_NONFINITE : GRAD_OK));
  if (!valid) return;
  const bool zero = gs != GRAD_OK;
  if (A.out.d_task_params) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int k = s + 16 * i;
      if (k < WBC_TASK_PARAMS_DOUBLES) A.out.d_task_params[b * WBC_TASK_PARAMS_DOUBLES + k] = zero ? 0.0 : go[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int k = s + 16 * i;
    const double v = zero ? 0.0 : to[i];
    if (k < GO_EEP) { if (A.out.d_ee_target) A.out.d_ee_target[b * 15 + k] = v; }
    else if (k < GO_TT) { if (A.out.d_prev_ee_target) A.out.d_prev_ee_target[b * 15 + (k - GO_EEP)] = v; }
    else if (k < GO_TP) { if (A.out.d_trunk_target) A.out.d_trunk_target[b * 3 + (k - GO_TT)] = v; }
    else if (k < GO_CT) { if (A.out.d_prev_trunk_target) A.out.d_prev_trunk_target[b * 3 + (k - GO_TP)] = v; }
    else if (k < GO_CV) { if (A.out.d_com_target) A.out.d_com_target[b * 3 + (k - GO_CT)] = v; }
    else if (k < GO_N) { if (A.out.d_com_target_vel) A.out.d_com_target_vel[b * 3 + (k - GO_CV)] = v; }
  }
  if (A.out.d_posture_u) {
    A.out.d_posture_u[b * NV + d0] = zero ? 0.0 : pu0;
    if (d1 < NV) A.out.d_posture_u[b * NV + d1] = zero ? 0.0 : pu1;
  }
  if (s == 0 && A.out.grad_status) A.out.grad_status[b] = gs;
}

// The variants (wbc_common.h, "Kernel variant tables"): the part that instantiates the row, then the template arguments.
#ifndef GRAD_PART
#define GRAD_PART -1      // -1: everything in one unit
#endif
#define WBC_PART GRAD_PART
#define WBC_KERNEL wbc_grad_kernel
#define WBC_KPARAMS (const GradArgs, const DevModel* __restrict__, const WbcConfig* __restrict__, const DevPlan* __restrict__)
typedef void (*GradKernel) WBC_KPARAMS;
#define GRAD_VARIANTS(V) /* ROT */ \
  V(0, false) \
  V(0, true)
#if GRAD_PART == -1
GRAD_VARIANTS(WBC_VARIANT_INST)
#else
GRAD_VARIANTS(WBC_VARIANT_UNIT)
#endif
#if GRAD_PART <= 0
static GradKernel grad_variant(long long key) {
  GRAD_VARIANTS(WBC_VARIANT_FIND)
  return nullptr;
}
int grad_variant_count() { return 0 GRAD_VARIANTS(WBC_VARIANT_COUNT); }
int launch_grad(const GradArgs& a, void* stream, long long* key_out) {
  const long long key = variant_key(a.rot != 0);
  if (key_out) *key_out = key;
  const GradKernel k = grad_variant(key);
  if (!k) return WBC_E_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3((a.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, a, a.models, a.cfgs, a.plans);
  return check_launch("tick_vjp");
}
#endif

}  // namespace wbc
