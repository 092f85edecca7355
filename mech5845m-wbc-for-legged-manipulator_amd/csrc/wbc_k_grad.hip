// wbc_k_grad.hip — wbc_tick_vjp: dL/d(task weights, gains, targets) of a solved tick from x = qdot and the certificate's u = sens_x
// (include/wbc.h). With r = b - A x and s = A u the chain is dL/dA = r u' - s x', dL/db = s, and every task row is
// (weights) x (an unweighted Jacobian row): the kernel never forms A, H or a Jacobian. It recomputes the kinematics from q (the task rows
// see q, not q_con), sums the WORLD twists  sum_d col_d x_d  and  sum_d col_d u_d  of each task frame over the frame's support — J_r x and
// J_r u of all six rows of the frame at once — and applies the block rules of include/wbc.h.
// One kernel of the whole-tree shape (wbc_qtree.h): four instances per wavefront (lane = 16 r + s), FK over the whole-tree schedule DevPlan.q_fk.
// Lane s owns the DoF s and 16 + s (their WORLD Jacobian columns, qt_jac_cols) and the bodies s and 16 + s (the CoM); sums over DoF are DPP row
// butterflies. The staged task image, the trunk target, the row terms and the exit rule are wbc_qtree.h's, shared with wbc_k_gradq.hip. The 85 + 42 results of an instance are collected in LDS (zero-initialised: a switched-off task's entries are never touched)
// and leave in coalesced stores. Reads its inputs and the tables; writes nothing but its outputs, rows [0, B) only.
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_grad.h"
#include "wbc_qtree.h"

namespace wbc {

// tout: the target gradients of an instance
constexpr int GO_EE = 0, GO_EEP = 15, GO_TT = 30, GO_TP = 33, GO_CT = 36, GO_CV = 39, GO_N = 42;
struct __attribute__((aligned(16))) GInst {
  QtKin K;
  double wt[96];                            // the 85 weights and gains (WbcTaskParams layout), rest zero
  double tin[TI_N];
  double mcw[24 * 4];                       // body j: m_j (R_j c_j + p_j), then m_j
  double sh[16];
  double gout[96];                          // d_task_params of the instance
  double tout[48];                          // d_ee_target [15], d_prev_ee_target [15], d_trunk_target, d_prev_trunk_target, d_com_target, d_com_target_vel
};
struct __attribute__((aligned(16))) GSmemP { GInst I[4]; };
static_assert(sizeof(GInst) == 6656 && offsetof(GInst, wt) == 3072 && offsetof(GInst, tin) == 3840 && offsetof(GInst, mcw) == 4608 &&
              offsetof(GInst, sh) == 5376 && offsetof(GInst, gout) == 5504 && offsetof(GInst, tout) == 6272, "the instance's LDS record");

template <bool ROT>   // ROT: rotated joint placements in the batch (wbc_k_sim3p.hip)
__global__ void __launch_bounds__(64) wbc_grad_kernel(const GradArgs A, const DevModel* __restrict__ models, const WbcConfig* __restrict__ cfgs,
                                                      const DevPlan* __restrict__ plans) {
  __shared__ GSmemP SP;
  const QtLane T(A.B);
  const int s = T.s; const size_t b = T.b;
  GInst& U = SP.I[T.r];
  const int mid = qt_model_index(A.in.model_id, b, A.n_models);
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
  const QtDof Dc(M, s, nv);                                         // ... and where their columns come from
  const unsigned sub0 = h0 ? M.col_subtree[d0] : 0u, sub1 = h1 ? M.col_subtree[d1] : 0u;
  const int j1 = 16 + s;                                            // bodies of this lane: joints s (>= 1) and 16 + s
  const bool hb0 = s >= 1 && s < nj, hb1 = j1 < nj;
  const DevPlan::QJnt m0 = P.q_jm[hb0 ? s : 1], m1 = P.q_jm[hb1 ? j1 : 1];
  bool bad = (s < nq && !is_finite(q0)) || (16 + s < nq && !is_finite(q1)) || !is_finite(xd0) || !is_finite(xd1) || !is_finite(ud0) ||
             !is_finite(ud1);
  bad = qt_stage_task_image(U.wt, U.tin, A.in, A.tp, cfg, b, s, eemask, t_trunk, t_com, pu_read, inv_dt) || bad;
#pragma unroll
  for (int i = 0; i < 6; ++i) U.gout[s + 16 * i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) U.tout[s + 16 * i] = 0.0;
  qt_fk<ROT>(U.K, q0, q1, scq0, scq1, M, P, fkn, s);
  const double* const qv = U.K.q;
  const double* const oMi = U.K.oMi;
  const double* const wt = U.wt;
  const double* const tin = U.tin;
  // ---- WORLD Jacobian columns of the lane's two DoF (computeJointJacobians: linear part at the world origin, angular part)
  double l0[3], a0[3], l1[3], a1[3];
  qt_jac_cols(oMi, Dc, l0, a0, l1, a1);
  // ---- the trunk frame and calcTargetVelTrunk2 (qt_trunk_target): vel [6], the literal qe [3]
  double tvel[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tqe[3] = {0.0, 0.0, 0.0}, ptr[3] = {0.0, 0.0, 0.0}, fq[4], rq[4];
  if (t_trunk) qt_trunk_target(oMi, M, tin, wt, U.sh, inv_dt, s, true, ptr, fq, rq, tqe, tvel);
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
    double pf[3];
    qt_frame_origin(oMi, M, fr, pf);
    if (ee) {                                                        // reference point at the frame origin: lin + ang x p
      double cx[3], cu[3];
      cross3(jx + 3, pf, cx); cross3(ju + 3, pf, cu);
#pragma unroll
      for (int i = 0; i < 3; ++i) { jx[i] += cx[i]; ju[i] += cu[i]; }
    }
    const int oW = ee ? WT_W + 6 * f : WT_TW, ow = ee ? WT_w + f : WT_Tw, oG = ee ? WT_G + 6 * f : WT_TG;
    const double* xt = ee ? tin + TI_EE + 3 * f : tin + TI_TR;
    const double w = wt[ow];
    double dw = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const QtRow R = qt_task_row(wt, tin, tvel, pf, ee, f, k, w, jx[k], ju[k], inv_dt);
      const double W = wt[oW + k], sv = R.sv;
      const double t = fma(R.rho, ju[k], -(sv * jx[k]));
      const double dvel = w * sv;
      dw += fma(W, t, sv * R.vel);
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
    {                                                                // (qt_body_mass_table's text: through the helper this kernel takes four SGPRs more)
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
      double mc[3], ms, cr[3];
      qt_subtree_mass(U.mcw, sub0 & 0x00FFFFFEu, mc, ms);
      cross3(a0, mc, cr);
#pragma unroll
      for (int i = 0; i < 3; ++i) c0[i] = fma(ms, l0[i], cr[i]);
      qt_subtree_mass(U.mcw, sub1 & 0x00FFFFFEu, mc, ms);
      cross3(a1, mc, cr);
#pragma unroll
      for (int i = 0; i < 3; ++i) c1[i] = fma(ms, l1[i], cr[i]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double jx = rsum16(fma(c0[k], xd0, c1[k] * xd1)) / cm, ju = rsum16(fma(c0[k], ud0, c1[k] * ud1)) / cm;
      const double W = wt[WT_CW + k], g = wt[WT_CG + k];
      const double e = tin[TI_CT + k] - com[k], bv = tin[TI_CV + k] + g * e;
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
        else { up0 = tin[TI_PU + d0]; up1 = tin[TI_PU + (h1 ? d1 : 0)]; }
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
  const int gs = qt_grad_status(st, cst, bad || obad, T.rbase);
  if (!T.valid) return;
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
