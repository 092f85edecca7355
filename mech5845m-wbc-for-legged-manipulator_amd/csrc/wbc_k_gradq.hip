// wbc_k_gradq.hip — wbc_tick_vjp_state: dL/dq of a solved tick, in tangent coordinates, and dL/d trunk_box_center, from x = qdot and the
// certificate's u = sens_x, w = sens_bounds / sens_rows, y = y_rows (include/wbc.h). With r = b - A x and s = A u:
//   dL/d delta_k = sum_rows (r_i u - s_i x) . dA_i/d delta_k + s_i db_i/d delta_k + sum_j (y_j u - w_j x) . dC_j/d delta_k + sum_active w_i de_i/d delta_k
// Every Jacobian row appears contracted with a fixed z in {x, u}, and d(J_W z)/d delta_k = S_k x_m T_k(z): S_k the WORLD column of DoF k,
// T_k(z) the frame body's spatial velocity under z minus that of k's own body (nothing is subtracted for a free-flyer column). So the kernel
// keeps ONE table per instance — the spatial velocity of every body under x and under u — and no second-order tensor. Per frame the rows'
// coefficients fold into four uniform vectors: aW, bW [6] on the WORLD derivative under u and under x (LOCAL_WORLD_ALIGNED rows fold in
// through p_f), E [3] on d p_f / d delta_k = l_k + a_k x p_f, Ea [3] on a_k; lane s then adds the terms of its DoF s and 16 + s.
// The whole-tree shape (wbc_qtree.h): four instances per wavefront (lane = 16 r + s), FK over the whole-tree schedule DevPlan.q_fk, sums over
// DoF by DPP row butterflies. The staged task image, the trunk target, the row terms and the exit rule are wbc_qtree.h's, as wbc_k_grad.hip's. Reads its inputs and the tables; writes nothing but its outputs, rows [0, B) only.
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_grad.h"
#include "wbc_gradq.h"
#include "wbc_qtree.h"

namespace wbc {

struct __attribute__((aligned(16))) QInst {
  QtKin K;
  double wt[96];                            // the 85 weights and gains (WbcTaskParams layout), rest zero
  double tin[TI_N];
  double mcw[24 * 4];                       // body j: m_j (R_j c_j + p_j), then m_j
  double VT[24 * 12];                       // body j: its WORLD spatial velocity under x (lin, ang), then under u
  double sh[16];
  double wy[48];                            // sens_rows [24], then y_rows [24]
  double dmp[32];                           // DoF i: w_i d(bound_i)/d q[damper_qidx[i]] of its active side
  double pst[32];                           // DoF i: d^2 u_i (PREV posture rows)
  double craw[32];                          // raw coordinate c: the coefficient of d q_raw[c] / d delta
};
struct __attribute__((aligned(16))) QSmemP { QInst I[4]; };
static_assert(sizeof(QInst) == 8960 && offsetof(QInst, wt) == 3072 && offsetof(QInst, tin) == 3840 && offsetof(QInst, mcw) == 4608 &&
              offsetof(QInst, VT) == 5376 && offsetof(QInst, sh) == 7680 && offsetof(QInst, wy) == 7808 && offsetof(QInst, dmp) == 8192 &&
              offsetof(QInst, pst) == 8448 && offsetof(QInst, craw) == 8704, "the instance's LDS record");

// (dL/d lower, dL/d upper) of a constraint with value val, sides lo / hi and sensitivity w: wbc_qp_certificate's rule
__device__ __forceinline__ void gq_share(const double w, const double val, const double lo, const double hi, const int bits, const bool have_ws,
                                         double& wl, double& wu) {
  const bool low = have_ws ? bits == 1 : fabs(val - lo) < 1e-7 * fmax(1.0, fabs(lo));
  const bool up = have_ws ? bits == 2 : !low;
  const bool eq = lo == hi;
  wl = eq ? 0.5 * w : (low ? w : 0.0);
  wu = eq ? 0.5 * w : (up ? w : 0.0);
}

// velDamperJointConstraints (wbc_common.h damper_bounds) with the derivative of each side with respect to qi, branch by branch
__device__ __forceinline__ void gq_damper(const double qi, const double lo, const double hi, const double vm, const double dcoef, const double dqi,
                                          const double dqs, double& l, double& u, double& dl, double& du) {
  const double slope = dcoef / (dqi - dqs);
  if (qi <= lo + dqi) { l = -dcoef * (qi - lo - dqs) / (dqi - dqs); dl = -slope; if (l > vm) { l = vm; dl = 0.0; } if (l < -vm) { l = -vm; dl = 0.0; } }
  else { l = -vm; dl = 0.0; }
  if (qi >= hi - dqi) { u = dcoef * (hi - qi - dqs) / (dqi - dqs); du = -slope; if (u < -vm) { u = -vm; du = 0.0; } if (u > vm) { u = vm; du = 0.0; } }
  else { u = vm; du = 0.0; }
  if (l > 0) { l = -l; dl = -dl; }
  if (u < 0) { u = -u; du = -du; }
}

// LOCAL_WORLD_ALIGNED rows at p with coefficients al (on the derivative under u) and be (under x) fold into the WORLD coefficients, and the
// ang x d p / d delta_k term into E
__device__ __forceinline__ void gq_lwa_fold(const double (&al)[6], const double (&be)[6], const double (&p)[3], const double* jx, const double* ju,
                                            double (&aW)[6], double (&bW)[6], double (&E)[3]) {
  double ca[3], cb[3], ea[3], eb[3];
  cross3(p, al, ca); cross3(p, be, cb);
  cross3(al, ju + 3, ea); cross3(be, jx + 3, eb);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    aW[i] += al[i]; aW[3 + i] += al[3 + i] + ca[i];
    bW[i] += be[i]; bW[3 + i] += be[3 + i] + cb[i];
    E[i] += ea[i] - eb[i];
  }
}

// DoF k's share of a frame: aW . (S_k x_m T_k(u)) - bW . (S_k x_m T_k(x)) + E . (l_k + a_k x p) + Ea . a_k;  T_k(z) = Vf(z) - Vk(z) (own: k is
// not a free-flyer column)
__device__ __forceinline__ double gq_frame_term(const double (&l)[3], const double (&a)[3], const double* Vf, const double* Vk, const bool own,
                                                const double (&aW)[6], const double (&bW)[6], const double (&E)[3], const double (&Ea)[3],
                                                const double (&p)[3]) {
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = Vf[i] - (own ? Vk[i] : 0.0);
  double c1[3], c2[3], c3[3], dp[3];
  double acc = 0.0;
  cross3(a, T + 6, c1); cross3(l, T + 9, c2); cross3(a, T + 9, c3);        // under u
#pragma unroll
  for (int i = 0; i < 3; ++i) acc += aW[i] * (c1[i] + c2[i]) + aW[3 + i] * c3[i];
  cross3(a, T, c1); cross3(l, T + 3, c2); cross3(a, T + 3, c3);            // under x
#pragma unroll
  for (int i = 0; i < 3; ++i) acc -= bW[i] * (c1[i] + c2[i]) + bW[3 + i] * c3[i];
  cross3(a, p, dp);
#pragma unroll
  for (int i = 0; i < 3; ++i) acc += E[i] * (l[i] + dp[i]) + Ea[i] * a[i];
  return acc;
}

// DoF k's share of the CoM rows: (ac . D(u) - bc . D(x) + Ec . M Jcom_k) / M over the bodies of k's sub-tree, D(z) = sum_j m_j x (the
// LOCAL_WORLD_ALIGNED linear rule at body j's centre of mass)
__device__ __forceinline__ double gq_com_term(const double (&l)[3], const double (&a)[3], unsigned mask, const double* VT, const double* mcw,
                                              const double* Vk, const bool own, const double (&ac)[3], const double (&bc)[3], const double (&Ec)[3],
                                              const double cm) {
  double Dx[3] = {0.0, 0.0, 0.0}, Du[3] = {0.0, 0.0, 0.0}, mc[3] = {0.0, 0.0, 0.0}, ms = 0.0;
  while (mask) {
    const int j = __ffs((int)mask) - 1;
    mask &= mask - 1;
    const double* Vj = VT + 12 * j;
    const double mj = mcw[4 * j + 3];
    const double cj[3] = {mcw[4 * j], mcw[4 * j + 1], mcw[4 * j + 2]};
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = Vj[i] - (own ? Vk[i] : 0.0);
    double ac_[3], w[3];
    cross3(a, cj, ac_);
#pragma unroll
    for (int i = 0; i < 3; ++i) { w[i] = fma(mj, l[i], ac_[i]); mc[i] += cj[i]; }
    ms += mj;
    double c1[3], c2[3], c3[3], c4[3], c5[3];
    cross3(a, T, c1); cross3(l, T + 3, c2); cross3(a, T + 3, c3); cross3(c3, cj, c4); cross3(Vj + 3, w, c5);
#pragma unroll
    for (int i = 0; i < 3; ++i) Dx[i] += mj * (c1[i] + c2[i]) + c4[i] + c5[i];
    cross3(a, T + 6, c1); cross3(l, T + 9, c2); cross3(a, T + 9, c3); cross3(c3, cj, c4); cross3(Vj + 9, w, c5);
#pragma unroll
    for (int i = 0; i < 3; ++i) Du[i] += mj * (c1[i] + c2[i]) + c4[i] + c5[i];
  }
  double cr[3], acc = 0.0;
  cross3(a, mc, cr);
#pragma unroll
  for (int i = 0; i < 3; ++i) acc += ac[i] * Du[i] - bc[i] * Dx[i] + Ec[i] * fma(ms, l[i], cr[i]);
  return acc / cm;
}

template <bool ROT>   // ROT: rotated joint placements in the batch (wbc_k_sim3p.hip)
__global__ void __launch_bounds__(64) wbc_gradq_kernel(const GradQArgs A, const DevModel* __restrict__ models, const WbcConfig* __restrict__ cfgs,
                                                       const DevPlan* __restrict__ plans) {
  __shared__ QSmemP SP;
  const QtLane T(A.B);
  const int s = T.s; const size_t b = T.b;
  QInst& U = SP.I[T.r];
  const int mid = qt_model_index(A.in.model_id, b, A.n_models);
  const DevModel& M = models[mid];
  const WbcConfig& cfg = cfgs[mid];
  const DevPlan& P = plans[mid];
  const int nq = M.nq, nv = M.nv, nj = M.njoints;
  const double inv_dt = 1.0 / A.dt;
  // ---- the switches (the same for every model of the batch: check_batch)
  unsigned eemask = 0u, cemask = 0u;
#pragma unroll
  for (int e = 0; e < WBC_NEE; ++e) { eemask |= cfg.task_ee[e] ? 1u << e : 0u; cemask |= cfg.con_ee[e] ? 1u << e : 0u; }
  const bool t_trunk = cfg.task_trunk != 0, t_com = cfg.task_com != 0, c_com = cfg.con_com != 0, c_trunk = cfg.con_trunk != 0;
  const bool use_b = cfg.use_bounds != 0, any_com = t_com || c_com;
  const int t_joint = cfg.task_joint;
  const int prow_tr = c_com ? 2 : 0, prow_ee0 = prow_tr + (c_trunk ? 4 : 0), p = prow_ee0 + 3 * __popc(cemask);
  // ---- every global read first
  const double* qg = A.in.q + b * NQ;
  const double q0 = qg[s], q1 = (16 + s < nq) ? qg[16 + s] : 0.0;
  const int d0 = s, d1 = 16 + s;                                    // DoF of this lane
  const bool h0 = d0 < nv, h1 = d1 < nv;
  const double xd0 = h0 ? A.sens.qdot[b * NV + d0] : 0.0, xd1 = h1 ? A.sens.qdot[b * NV + d1] : 0.0;
  const double ud0 = h0 ? A.sens.sens_x[b * NV + d0] : 0.0, ud1 = h1 ? A.sens.sens_x[b * NV + d1] : 0.0;
  const bool rb = use_b && A.sens.sens_bounds;
  const double wb0 = (rb && h0) ? A.sens.sens_bounds[b * NV + d0] : 0.0, wb1 = (rb && h1) ? A.sens.sens_bounds[b * NV + d1] : 0.0;
  const int st = A.sens.status ? A.sens.status[b] : 0, cst = A.sens.cert_status ? A.sens.cert_status[b] : 0;
  const bool have_ws = A.sens.working_set != nullptr;
  const unsigned long long ws0 = have_ws ? A.sens.working_set[2 * b] : 0ull, ws1 = have_ws ? A.sens.working_set[2 * b + 1] : 0ull;
  DevPlan::PkJoint fkn = P.q_fk[0][s];
  const int scq0 = P.q_scq[(2 + s) & 31], scq1 = P.q_scq[(18 + s) & 31];
  const int cj0 = M.col_joint[h0 ? d0 : 0], cl0 = M.col_lin[h0 ? d0 : 0], ca0 = M.col_ang[h0 ? d0 : 0];
  const int cj1 = M.col_joint[h1 ? d1 : 0], cl1 = M.col_lin[h1 ? d1 : 0], ca1 = M.col_ang[h1 ? d1 : 0];
  const int cq0 = M.col_q[h0 ? d0 : 6], cq1 = M.col_q[h1 ? d1 : 6];
  const unsigned sub0 = h0 ? M.col_subtree[d0] : 0u, sub1 = h1 ? M.col_subtree[d1] : 0u;
  const int j1 = 16 + s;                                            // bodies of this lane: joints s (>= 1) and 16 + s
  const bool hb0 = s >= 1 && s < nj, hb1 = j1 < nj;
  const DevPlan::QJnt m0 = P.q_jm[hb0 ? s : 1], m1 = P.q_jm[hb1 ? j1 : 1];
  const int dqi0 = cfg.damper_qidx[h0 ? d0 : 0], dqi1 = cfg.damper_qidx[h1 ? d1 : 0];
  const double dlo0 = cfg.damper_lo[h0 ? d0 : 0], dhi0 = cfg.damper_hi[h0 ? d0 : 0], dvm0 = cfg.damper_vmax[h0 ? d0 : 0];
  const double dlo1 = cfg.damper_lo[h1 ? d1 : 0], dhi1 = cfg.damper_hi[h1 ? d1 : 0], dvm1 = cfg.damper_vmax[h1 ? d1 : 0];
  double bc[4] = {0.0, 0.0, 0.0, 0.0};
  if (c_trunk) {
#pragma unroll
    for (int i = 0; i < 4; ++i) bc[i] = A.in.trunk_box_center[b * 4 + i];
  }
  bool bad = (s < nq && !is_finite(q0)) || (16 + s < nq && !is_finite(q1)) || !is_finite(xd0) || !is_finite(xd1) || !is_finite(ud0) ||
             !is_finite(ud1) || !is_finite(wb0) || !is_finite(wb1) || !is_finite(bc[0]) || !is_finite(bc[1]) || !is_finite(bc[2]) || !is_finite(bc[3]);
  {
    const bool ibad = qt_stage_task_image(U.wt, U.tin, A.in, A.tp, cfg, b, s, eemask, t_trunk, t_com, false, inv_dt);
    bad = bad || ibad;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int k = s + 16 * i, kk = (k < 24) ? k : k - 24;
      const double v = (kk < p) ? ((k < 24) ? A.sens.sens_rows[b * p + kk] : A.sens.y_rows[b * p + kk]) : 0.0;
      bad = bad || !is_finite(v);
      U.wy[k] = v;
    }
#pragma unroll
    for (int i = 0; i < 18; ++i) U.VT[s + 16 * i] = 0.0;
  }
  qt_fk<ROT>(U.K, q0, q1, scq0, scq1, M, P, fkn, s);
  const double* const qv = U.K.q;
  double* const oMi = U.K.oMi;
  const double* const wt = U.wt;
  const double* const tin = U.tin;
  const double* const wr = U.wy;
  const double* const yr = U.wy + 24;
  // ---- WORLD Jacobian columns of the lane's two DoF; not QtDof / qt_jac_cols: with the record this kernel takes four VGPRs more
  double l0[3] = {0.0, 0.0, 0.0}, a0[3] = {0.0, 0.0, 0.0}, l1[3] = {0.0, 0.0, 0.0}, a1[3] = {0.0, 0.0, 0.0};
  if (h0) pk_jac_col(oMi, cj0, cl0, ca0, l0, a0);
  if (h1) pk_jac_col(oMi, cj1, cl1, ca1, l1, a1);
  // ---- the body velocity table. First each joint's own columns: the free-flyer's six (joint 1, lanes 0..5) by a row sum, a 1-DoF joint's from its lane
  {
    const bool ff = h0 && d0 < 6;
    double fv[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      fv[c] = rsum16(ff ? l0[c] * xd0 : 0.0); fv[3 + c] = rsum16(ff ? a0[c] * xd0 : 0.0);
      fv[6 + c] = rsum16(ff ? l0[c] * ud0 : 0.0); fv[9 + c] = rsum16(ff ? a0[c] * ud0 : 0.0);
    }
    if (s == 0) {
#pragma unroll
      for (int c = 0; c < 12; ++c) U.VT[12 + c] = fv[c];
    }
    if (h0 && d0 >= 6) {
      double* o = U.VT + 12 * cj0;
#pragma unroll
      for (int c = 0; c < 3; ++c) { o[c] = l0[c] * xd0; o[3 + c] = a0[c] * xd0; o[6 + c] = l0[c] * ud0; o[9 + c] = a0[c] * ud0; }
    }
    if (h1) {
      double* o = U.VT + 12 * cj1;
#pragma unroll
      for (int c = 0; c < 3; ++c) { o[c] = l1[c] * xd1; o[3 + c] = a1[c] * xd1; o[6 + c] = l1[c] * ud1; o[9 + c] = a1[c] * ud1; }
    }
  }
  WSYNC();
  // ... then body j's velocity: the sum over the joints whose sub-tree holds j (lane s: bodies s and 16 + s), in place behind a fence
  {
    double v0[12], v1[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) { v0[c] = 0.0; v1[c] = 0.0; }
#pragma unroll 1
    for (int a = 1; a < nj; ++a) {
      const unsigned sub = M.col_subtree[M.idx_v_of[a]];
      const bool in0 = (sub >> s) & 1u, in1 = (sub >> (16 + s)) & 1u;
      const double* o = U.VT + 12 * a;
#pragma unroll
      for (int c = 0; c < 12; ++c) { const double t = o[c]; v0[c] += in0 ? t : 0.0; v1[c] += in1 ? t : 0.0; }
    }
    WSYNC();
    if (hb0) {
#pragma unroll
      for (int c = 0; c < 12; ++c) U.VT[12 * s + c] = v0[c];
    }
    if (hb1 && j1 < 24) {
#pragma unroll
      for (int c = 0; c < 12; ++c) U.VT[12 * j1 + c] = v1[c];
    }
  }
  // ---- the bodies' mass-weighted centres (CoM rows)
  if (any_com) qt_body_mass_table(U.mcw, oMi, m0, m1, hb0, hb1, s);
  WSYNC();
  const double* const VT = U.VT;
  const double* const Vk0 = VT + 12 * cj0;
  const double* const Vk1 = VT + 12 * cj1;
  const bool own0 = d0 >= 6;
  // ---- the CoM, and Jcom x, Jcom u
  double com[3] = {0.0, 0.0, 0.0}, cm = 1.0, jxc[3] = {0.0, 0.0, 0.0}, juc[3] = {0.0, 0.0, 0.0};
  if (any_com) {
    const double* ma = U.mcw + 4 * s;
    const double* mb = U.mcw + 4 * (j1 < 24 ? j1 : 0);
    const bool two = j1 < 24;
    const double* Va = VT + 12 * s;
    const double* Vb = VT + 12 * (two ? j1 : 0);
    cm = rsum16(ma[3] + (two ? mb[3] : 0.0));
    double cxa[3], cxb[3], cua[3], cub[3];
    cross3(Va + 3, ma, cxa); cross3(Vb + 3, mb, cxb); cross3(Va + 9, ma, cua); cross3(Vb + 9, mb, cub);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      com[i] = rsum16(ma[i] + (two ? mb[i] : 0.0)) / cm;
      jxc[i] = rsum16((hb0 ? fma(ma[3], Va[i], cxa[i]) : 0.0) + ((two && hb1) ? fma(mb[3], Vb[i], cxb[i]) : 0.0)) / cm;
      juc[i] = rsum16((hb0 ? fma(ma[3], Va[6 + i], cua[i]) : 0.0) + ((two && hb1) ? fma(mb[3], Vb[6 + i], cub[i]) : 0.0)) / cm;
    }
  }
  // ---- the trunk frame; calcTargetVelTrunk2 (qt_trunk_target): vel [6], and fq, rq for the literal qe. A trunk box alone needs the origin.
  double tvel[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ptr[3] = {0.0, 0.0, 0.0}, fq[4] = {0.0, 0.0, 0.0, 1.0}, rq[4] = {0.0, 0.0, 0.0, 1.0}, tqe[3];
  const double* const Pt = oMi + 12 * M.frame_joint[WBC_FR_TRUNK];   // R column-major: R(i, j) = Pt[3 j + i]
  if (t_trunk || c_trunk) qt_trunk_target(oMi, M, tin, wt, U.sh, inv_dt, s, t_trunk, ptr, fq, rq, tqe, tvel);
  // ---- which side each inequality row's w belongs to (the bounds recomputed from q), and d_trunk_box_center
  double cwl[2] = {0.0, 0.0}, cwu[2] = {0.0, 0.0}, twl[4] = {0.0, 0.0, 0.0, 0.0}, twu[4] = {0.0, 0.0, 0.0, 0.0};
  const double kc = cfg.com_box_scale * inv_dt, kt = cfg.trunk_box_scale * inv_dt;
  if (c_com) {
    double pfl[3], prr[3];                                          // the FL and RR feet: x and y are read
    qt_frame_origin(oMi, M, WBC_FR_EE0 + 1, pfl);
    qt_frame_origin(oMi, M, WBC_FR_EE0 + 2, prr);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      gq_share(wr[i], jxc[i], ((prr[i] - com[i]) * inv_dt) * cfg.com_box_scale, ((pfl[i] - com[i]) * inv_dt) * cfg.com_box_scale, pk_ws_bits(ws1, i),
               have_ws, cwl[i], cwu[i]);
    }
  }
  double tbc = 0.0;                                                 // d_trunk_box_center entry s < 4
  if (c_trunk) {
    const double* Vf = VT + 12 * M.frame_joint[WBC_FR_TRUNK];
    const double R00 = Pt[0], R10 = Pt[1], R20 = Pt[2], R21 = Pt[5], R22 = Pt[8];
    const double cur[4] = {ptr[2], atan2(R21, R22), atan2(-R20, sqrt(fma(R21, R21, R22 * R22))), atan2(R10, R00)};
    const double var[4] = {bc[0] * cfg.trunk_box_z_frac, cfg.trunk_box_ang, cfg.trunk_box_ang, cfg.trunk_box_ang};
    const double val[4] = {Vf[2] + (Vf[3] * ptr[1] - Vf[4] * ptr[0]), Vf[3], Vf[4], Vf[5]};   // LOCAL_WORLD_ALIGNED rows 2..5 times x
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gq_share(wr[prow_tr + i], val[i], (((bc[i] - var[i]) - cur[i]) * inv_dt) * cfg.trunk_box_scale,
               (((bc[i] + var[i]) - cur[i]) * inv_dt) * cfg.trunk_box_scale, pk_ws_bits(ws1, prow_tr + i), have_ws, twl[i], twu[i]);
    }
    const double z = kt * fma(twl[0], 1.0 - cfg.trunk_box_z_frac, twu[0] * (1.0 + cfg.trunk_box_z_frac));
    tbc = (s == 0) ? z : ((s == 1) ? kt * (twl[1] + twu[1]) : ((s == 2) ? kt * (twl[2] + twu[2]) : kt * (twl[3] + twu[3])));
  }
  // ---- the six frames: EE 0..4 (task rows LOCAL_WORLD_ALIGNED, contact rows WORLD, FL / RR the CoM box's corners) and the trunk (task rows
  // WORLD, box rows LOCAL_WORLD_ALIGNED 2..5)
  double res0 = 0.0, res1 = 0.0;
  int prow = prow_ee0;
#pragma unroll 1
  for (int f = 0; f < WBC_NEE + 1; ++f) {
    const bool ee = f < WBC_NEE;
    const bool task = ee ? ((eemask >> f) & 1u) != 0u : t_trunk;
    const bool con = ee ? ((cemask >> f) & 1u) != 0u : c_trunk;
    const bool corner = c_com && (f == 1 || f == 2);
    if (!task && !con && !corner) continue;                          // (wave-uniform: the switches are the batch's)
    const int fr = ee ? WBC_FR_EE0 + f : WBC_FR_TRUNK;
    const unsigned sup = M.frame_support[fr];
    const bool on0 = h0 && ((sup >> d0) & 1u), on1 = h1 && ((sup >> (d1 & 31)) & 1u);
    const int fj = M.frame_joint[fr];
    const double* Vf = VT + 12 * fj;
    double pf[3];
    qt_frame_origin(oMi, M, fr, pf);
    double aW[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bW[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, E[3] = {0.0, 0.0, 0.0}, Ea[3] = {0.0, 0.0, 0.0};
    if (task) {
      const int ow = ee ? WT_w + f : WT_Tw, oG = ee ? WT_G + 6 * f : WT_TG;
      const double w = wt[ow];
      double jx[6], ju[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) { jx[i] = Vf[i]; ju[i] = Vf[6 + i]; }
      if (ee) {                                                      // reference point at the frame origin: lin + ang x p
        double cx[3], cu[3];
        cross3(jx + 3, pf, cx); cross3(ju + 3, pf, cu);
#pragma unroll
        for (int i = 0; i < 3; ++i) { jx[i] += cx[i]; ju[i] += cu[i]; }
      }
      double al[6], be[6], svv[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const QtRow R = qt_task_row(wt, tin, tvel, pf, ee, f, k, w, jx[k], ju[k], inv_dt);
        const double c = R.c, sv = R.sv;
        al[k] = c * R.rho; be[k] = c * sv; svv[k] = sv;
        if (k < 3) E[k] -= sv * (w * wt[oG + k] * inv_dt);            // d b_k / d p_f
      }
      if (ee) {
        gq_lwa_fold(al, be, pf, Vf, Vf + 6, aW, bW, E);
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) { aW[k] += al[k]; bW[k] += be[k]; }
        // quaternion feedback: qe is linear in fq and d fq / d delta = 1/2 fq (x) (R_f' a_k, 0):  Ea += R_f h,  h_m = sum_i coef_i d qe_i / d local axis m
        const double c3 = svv[3] * (w * wt[oG + 3]), c4 = svv[4] * (w * wt[oG + 4]), c5 = svv[5] * (w * wt[oG + 5]);
        double h[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const double em[4] = {m == 0 ? 0.5 : 0.0, m == 1 ? 0.5 : 0.0, m == 2 ? 0.5 : 0.0, 0.0};
          double g[4];
          quat_mul(fq, em, g);
          const double e0 = g[3] * rq[0] - g[0] * rq[3] + g[1] * rq[2] - g[2] * rq[1];
          const double e1 = g[3] * rq[1] - g[1] * rq[3] - g[0] * rq[2] + g[2] * rq[0];
          const double e2 = g[0] * rq[1] - g[1] * rq[0];
          h[m] = c3 * e0 + c4 * e1 + c5 * e2;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) Ea[i] += Pt[i] * h[0] + Pt[3 + i] * h[1] + Pt[6 + i] * h[2];
      }
    }
    if (con) {
      if (ee) {                                                      // EEConstraint: WORLD rows 0..2, 0 <= . <= 0
#pragma unroll
        for (int i = 0; i < 3; ++i) { aW[i] += yr[prow + i]; bW[i] += wr[prow + i]; }
        prow += 3;
      } else {                                                       // trunkConstraint: LOCAL_WORLD_ALIGNED rows 2..5; e = ((c -+ var) - [z, euler]) scale / dt
        const double al[6] = {0.0, 0.0, yr[prow_tr], yr[prow_tr + 1], yr[prow_tr + 2], yr[prow_tr + 3]};
        const double be[6] = {0.0, 0.0, wr[prow_tr], wr[prow_tr + 1], wr[prow_tr + 2], wr[prow_tr + 3]};
        gq_lwa_fold(al, be, pf, Vf, Vf + 6, aW, bW, E);
        E[2] -= kt * (twl[0] + twu[0]);
        // the three atan2 angles through dR = [omega] R: d angle_a = N_a . omega
        const double R00 = Pt[0], R10 = Pt[1], R20 = Pt[2], R01 = Pt[3], R11 = Pt[4], R21 = Pt[5], R02 = Pt[6], R12 = Pt[7], R22 = Pt[8];
        const double d0_ = fma(R21, R21, R22 * R22), cxy = sqrt(d0_), d1_ = fma(R20, R20, d0_), d2_ = fma(R00, R00, R10 * R10);
        const double g0 = -kt * (twl[1] + twu[1]) / d0_, g1 = -kt * (twl[2] + twu[2]) / d1_, g2 = -kt * (twl[3] + twu[3]) / d2_;
        const double t1 = R20 / cxy;
        Ea[0] += g0 * (R22 * R11 - R21 * R12) + g1 * (-cxy * R10 + t1 * (R21 * R11 + R22 * R12)) + g2 * (-R00 * R20);
        Ea[1] += g0 * (R21 * R02 - R22 * R01) + g1 * (cxy * R00 - t1 * (R21 * R01 + R22 * R02)) + g2 * (-R10 * R20);
        Ea[2] += g2 * (R00 * R00 + R10 * R10);
      }
    }
    if (corner) {                                                    // CoMConstraint: lower side at the RR foot, upper side at the FL foot
      E[0] += kc * (f == 1 ? cwu[0] : cwl[0]);
      E[1] += kc * (f == 1 ? cwu[1] : cwl[1]);
    }
    if (on0) res0 += gq_frame_term(l0, a0, Vf, Vk0, own0, aW, bW, E, Ea, pf);
    if (on1) res1 += gq_frame_term(l1, a1, Vf, Vk1, true, aW, bW, E, Ea, pf);
  }
  // ---- CoM rows (task: A = com_W Jcom, b = cv + com_gain (ct - com); box: C = Jcom rows 0, 1, e = (p_foot - com) scale / dt)
  if (any_com) {
    double ac[3] = {0.0, 0.0, 0.0}, bcf[3] = {0.0, 0.0, 0.0}, Ec[3] = {0.0, 0.0, 0.0};
    if (t_com) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double W = wt[WT_CW + k], g = wt[WT_CG + k];
        const double bv = tin[TI_CV + k] + g * (tin[TI_CT + k] - com[k]);
        const double sv = W * juc[k], rho = fma(-W, jxc[k], bv);
        ac[k] = W * rho; bcf[k] = W * sv; Ec[k] = -(sv * g);
      }
    }
    if (c_com) {
#pragma unroll
      for (int k = 0; k < 2; ++k) { ac[k] += yr[k]; bcf[k] += wr[k]; Ec[k] -= kc * (cwl[k] + cwu[k]); }
    }
    if (h0) res0 += gq_com_term(l0, a0, sub0 & 0x00FFFFFEu, VT, U.mcw, Vk0, own0, ac, bcf, Ec, cm);
    if (h1) res1 += gq_com_term(l1, a1, sub1 & 0x00FFFFFEu, VT, U.mcw, Vk1, true, ac, bcf, Ec, cm);
  }
  // ---- what reads q itself: the PREV posture target (up = np.delete(q, 6)[:nv], b_k = d up_k) and the velocity-damper bounds, through
  // G = d q_raw / d delta (xyz rows R, quaternion rows 1/2 q (x) (e, 0), joint rows the identity)
  {
    double t0 = 0.0, t1 = 0.0;
    if (use_b) {
      double lo, hi, dl, du, wl, wu;
      gq_damper(qv[dqi0], dlo0, dhi0, dvm0, cfg.damper_coef, cfg.damper_qi, cfg.damper_qs, lo, hi, dl, du);
      if (d0 >= cfg.lock_from) { lo = hi = 0.0; dl = du = 0.0; }
      gq_share(wb0, xd0, lo, hi, pk_ws_bits(ws0, d0), have_ws, wl, wu);
      t0 = h0 ? wl * dl + wu * du : 0.0;
      gq_damper(qv[dqi1], dlo1, dhi1, dvm1, cfg.damper_coef, cfg.damper_qi, cfg.damper_qs, lo, hi, dl, du);
      if (d1 >= cfg.lock_from) { lo = hi = 0.0; dl = du = 0.0; }
      gq_share(wb1, xd1, lo, hi, pk_ws_bits(ws0, d1), have_ws, wl, wu);
      t1 = h1 ? wl * dl + wu * du : 0.0;
    }
    const double dj = (t_joint == WBC_JOINT_PREV) ? (1.0 / nv) * wt[WT_JW] : 0.0;
    U.dmp[d0] = t0; U.dmp[d1] = t1;
    U.pst[d0] = h0 ? (dj * dj) * ud0 : 0.0; U.pst[d1] = h1 ? (dj * dj) * ud1 : 0.0;
    WSYNC();
    const int c0 = s, c1 = 16 + s;                                  // raw coordinates of this lane
    double r0 = (c0 < 6) ? U.pst[c0] : ((c0 > 6) ? U.pst[c0 - 1] : 0.0), r1 = (c1 < NQ) ? U.pst[c1 - 1] : 0.0;
    if (use_b) {
#pragma unroll 1
      for (int i = 0; i < nv; ++i) {
        const int qi = cfg.damper_qidx[i];
        const double t = U.dmp[i];
        r0 += (qi == c0) ? t : 0.0; r1 += (qi == c1) ? t : 0.0;
      }
    }
    U.craw[c0] = r0; U.craw[c1] = r1;
    WSYNC();
    const double* cr = U.craw;
    const double* P1 = oMi + 12;                                    // the base rotation, column-major
    if (d0 < 3) {
      res0 += cr[0] * P1[3 * d0] + cr[1] * P1[3 * d0 + 1] + cr[2] * P1[3 * d0 + 2];
    } else if (d0 < 6) {
      const double e[3] = {d0 == 3 ? 1.0 : 0.0, d0 == 4 ? 1.0 : 0.0, d0 == 5 ? 1.0 : 0.0};
      const double v[3] = {qv[3], qv[4], qv[5]}, qw = qv[6];
      double ve[3];
      cross3(v, e, ve);
      res0 += 0.5 * (cr[3] * fma(qw, e[0], ve[0]) + cr[4] * fma(qw, e[1], ve[1]) + cr[5] * fma(qw, e[2], ve[2]) -
                     cr[6] * (v[0] * e[0] + v[1] * e[1] + v[2] * e[2]));
    } else if (h0) {
      res0 += cr[cq0];
    }
    if (h1) res1 += cr[cq1];
  }
  // ---- out: zero rows for an unsolved / uncertified / non-finite instance; nothing non-finite leaves the instance
  const bool obad = !is_finite(res0) || !is_finite(res1) || !is_finite(tbc);
  const int gs = qt_grad_status(st, cst, bad || obad, T.rbase);
  if (!T.valid) return;
  const bool zero = gs != GRAD_OK;
  if (A.out.d_q) {
    A.out.d_q[b * NV + d0] = (zero || !h0) ? 0.0 : res0;
    if (d1 < NV) A.out.d_q[b * NV + d1] = (zero || !h1) ? 0.0 : res1;
  }
  if (A.out.d_trunk_box_center && s < 4) A.out.d_trunk_box_center[b * 4 + s] = zero ? 0.0 : tbc;
  if (s == 0 && A.out.grad_status) A.out.grad_status[b] = gs;
}

// The variants (wbc_common.h, "Kernel variant tables"): the part that instantiates the row, then the template arguments.
#ifndef GRADQ_PART
#define GRADQ_PART -1      // -1: everything in one unit
#endif
#define WBC_PART GRADQ_PART
#define WBC_KERNEL wbc_gradq_kernel
#define WBC_KPARAMS (const GradQArgs, const DevModel* __restrict__, const WbcConfig* __restrict__, const DevPlan* __restrict__)
typedef void (*GradQKernel) WBC_KPARAMS;
#define GRADQ_VARIANTS(V) /* ROT */ \
  V(0, false) \
  V(0, true)
#if GRADQ_PART == -1
GRADQ_VARIANTS(WBC_VARIANT_INST)
#else
GRADQ_VARIANTS(WBC_VARIANT_UNIT)
#endif
#if GRADQ_PART <= 0
static GradQKernel gradq_variant(long long key) {
  GRADQ_VARIANTS(WBC_VARIANT_FIND)
  return nullptr;
}
int gradq_variant_count() { return 0 GRADQ_VARIANTS(WBC_VARIANT_COUNT); }
int launch_gradq(const GradQArgs& a, void* stream, long long* key_out) {
  const long long key = variant_key(a.rot != 0);
  if (key_out) *key_out = key;
  const GradQKernel k = gradq_variant(key);
  if (!k) return WBC_E_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3((a.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, a, a.models, a.cfgs, a.plans);
  return check_launch("tick_vjp_state");
}
#endif

}  // namespace wbc
