// wbc_k_slackvjp.hip — wbc_state_slack_vjp / wbc_rollout_vjp_watched: the cotangent of the four slack families of wbc_k_slack.hip at a
// configuration q (include/wbc.h states the algebra). One kernel,
//   wbc_slackvjp_kernel    four instances per wavefront (lane = 16 r + s), the whole-tree shape (wbc_qtree.h)
//     every global read, then FK over the whole-tree schedule DevPlan.q_fk at q, then the forward's own evaluation (wbc_slack.h: frames, CoM,
//     joint scan, components, family scans — the selected components are wbc_state_slack's `which` bit for bit). From the components'
//     cotangents gamma_0..11 and the joint family's gamma_J:
//         c_FL = (gamma1, gamma3, 0)   c_RR = (-gamma0, -gamma2, 0)   c_com = (gamma0 - gamma1, gamma2 - gamma3, 0)
//         c_z = gamma4 - gamma5        c_e[a] = gamma(6 + 2a) - gamma(7 + 2a)        Ea = sum_a c_e[a] N_a(R)   (d angle_a = N_a . omega)
//     Lane s owns DoF s and 16 + s: with l, a the DoF's WORLD Jacobian column,
//         t = [FL has d] (l + a x p_FL) . c_FL + [RR has d] (l + a x p_RR) . c_RR + ((ms l + a x mc) / M) . c_com
//           + [trunk has d] ((l + a x p_T)_z c_z + a . Ea) + [d is the joint family's DoF] (+gamma_J lower side, -gamma_J upper side)
//     (mc, ms: the sums of m_j c_j and m_j over the DoF's sub-tree), and to the box centre -(1 - z_frac) gamma4 + (1 + z_frac) gamma5 and -c_e[a].
//     STATE  gamma_i = g_comp[i] + [i == which[f]] g_slack[f]; writes d_q, d_box, which, grad_status (a bad row: zeros, WBC_GRAD_NONFINITE)
//     SEED   gamma of watched family f on its selected component alone, g_trace + [k == K - 1] g_fin + [k == min_tick] g_min; g[d] += t and
//            acc_box += the box term, an exact zero not added (the carried cotangent keeps its bits, the sign of a zero included, under
//            all-zero cotangents); a bad instance: worst[b] <- WBC_GRAD_NONFINITE and nothing added.
// No atomics, no scratch; the cross-lane traffic is the evaluation's own (row butterflies). Identical calls give identical bits. Rows >= B
// are never written.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_grad.h"
#include "wbc_qtree.h"      // NOT behind an `fp contract` pragma: the evaluation below must contract as it does in wbc_k_slack.hip
#include "wbc_slackvjp.h"

namespace wbc {

struct __attribute__((aligned(16))) WInst {
  QtKin K;
  double pf[12];                            // FL foot, RR foot, trunk frame: world positions (stride 4)
  double eul[4];                            // roll, pitch, yaw of the trunk rotation
  double mcw[24 * 4];                       // body j: m_j c_j (world), m_j
};
struct __attribute__((aligned(16))) WSmemP { WInst I[4]; };
static_assert(sizeof(WInst) == 3968 && offsetof(WInst, pf) == 3072 && offsetof(WInst, eul) == 3168 && offsetof(WInst, mcw) == 3200, "the instance's LDS record");

struct SvCot {                              // the cotangents every lane of the row holds
  double cfl[2], crr[2], ccom[2], cz, Ea[3];
};

// this DoF's term without the joint family's
__device__ __forceinline__ double sw_dof_term(const double* const pf, const double* const mcw, const DevModel& M, const int d, const unsigned sub,
                                              const double (&l)[3], const double (&a)[3], const SvCot& C, const double cm) {
  const double* pFL = pf;
  const double* pRR = pf + 4;
  const double* pT = pf + 8;
  double acc = 0.0;
  if ((M.frame_support[WBC_FR_EE0 + 1] >> d) & 1u) {
    const double v0 = l[0] + (a[1] * pFL[2] - a[2] * pFL[1]), v1 = l[1] + (a[2] * pFL[0] - a[0] * pFL[2]);
    acc += v0 * C.cfl[0] + v1 * C.cfl[1];
  }
  if ((M.frame_support[WBC_FR_EE0 + 2] >> d) & 1u) {
    const double v0 = l[0] + (a[1] * pRR[2] - a[2] * pRR[1]), v1 = l[1] + (a[2] * pRR[0] - a[0] * pRR[2]);
    acc += v0 * C.crr[0] + v1 * C.crr[1];
  }
  {
    double mc[3], ms;
    qt_subtree_mass(mcw, sub & 0x00FFFFFEu, mc, ms);
    const double v0 = ms * l[0] + (a[1] * mc[2] - a[2] * mc[1]), v1 = ms * l[1] + (a[2] * mc[0] - a[0] * mc[2]);
    acc += (v0 * C.ccom[0] + v1 * C.ccom[1]) / cm;
  }
  if ((M.frame_support[WBC_FR_TRUNK] >> d) & 1u) {
    const double v2 = l[2] + (a[0] * pT[1] - a[1] * pT[0]);
    acc += v2 * C.cz + ((a[0] * C.Ea[0] + a[1] * C.Ea[1]) + a[2] * C.Ea[2]);
  }
  return acc;
}

template <int STAGE, bool ROT>   // ROT: rotated joint placements in the batch (wbc_k_sim3p.hip)
__global__ void __launch_bounds__(64) wbc_slackvjp_kernel(const SlackVjpArgs A) {
  __shared__ WSmemP SP;
  const QtLane T(A.B);
  const int s = T.s; const size_t b = T.b, nB = (size_t)A.B;
  WInst& U = SP.I[T.r];
  const int mid = qt_model_index(A.model_id, b, A.n_models);
  const DevModel& M = A.models[mid];
  const WbcConfig& cfg = A.cfgs[mid];
  const DevPlan& P = A.plans[mid];
  const SlackLimits& Lm = A.lim[mid];
  const int nq = M.nq, nv = M.nv;
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  // ---- every global read first
  const double* qg = A.q + b * NQ;
  const double q0 = qg[s], q1 = (16 + s < nq) ? qg[16 + s] : 0.0;
  double bc[4] = {qnan, qnan, qnan, qnan};
  if (A.box) {
#pragma unroll
    for (int i = 0; i < 4; ++i) bc[i] = A.box[b * 4 + i];
  }
  double gs[SLACK_NF] = {0.0, 0.0, 0.0, 0.0}, gc[SLACK_NC];
#pragma unroll
  for (int i = 0; i < SLACK_NC; ++i) gc[i] = 0.0;
  bool tickbad = false;                     // SEED: slack_min_tick outside [0, K) under a non-zero g_slack_min
  if (STAGE == SLACKVJP_STATE) {
    if (A.g_slack) {
#pragma unroll
      for (int f = 0; f < SLACK_NF; ++f) gs[f] = A.g_slack[b * SLACK_NF + f];
    }
    if (A.g_comp) {
#pragma unroll
      for (int i = 0; i < SLACK_NC; ++i) gc[i] = A.g_comp[b * SLACK_NC + i];
    }
  } else {
    const bool lastk = A.k == A.K - 1;
#pragma unroll
    for (int f = 0; f < SLACK_NF; ++f) {
      if (!((A.mask >> f) & 1)) continue;
      const size_t gi = (size_t)__popc((unsigned)A.mask & ((1u << f) - 1u)) * nB + b;
      double x = A.g_trace ? A.g_trace[gi] : 0.0;
      if (lastk && A.g_fin) x = x + A.g_fin[gi];
      if (A.g_min) {
        const double gm = A.g_min[gi];
        const int tk = A.min_tick[gi];
        if (A.k == tk) x = x + gm;
        tickbad = tickbad || (lastk && (!is_finite(gm) || (gm != 0.0 && (tk < 0 || tk >= A.K))));
      }
      gs[f] = x;
    }
  }
  DevPlan::PkJoint fkn = P.q_fk[0][s];
  const int scq0 = P.q_scq[(2 + s) & 31], scq1 = P.q_scq[(18 + s) & 31];
  const SlackLane L(M, cfg, P, Lm, s);
  const QtDof Dc(M, s, nv);                                         // DoF of this lane
  const int d0 = Dc.d0, d1 = Dc.d1; const bool h0 = Dc.h0, h1 = Dc.h1;
  const unsigned sub0 = h0 ? M.col_subtree[d0] : 0u, sub1 = h1 ? M.col_subtree[d1] : 0u;
  // ---- the row's test: q among the model's nq, the cotangents, the box entries of a family that carries a non-zero cotangent
  bool bad = (s < nq && !is_finite(q0)) || (16 + s < nq && !is_finite(q1)) || tickbad;
  const bool qbad = ((__ballot((s < nq && !is_finite(q0)) || (16 + s < nq && !is_finite(q1))) >> T.rbase) & 0xFFFFull) != 0ull;
#pragma unroll
  for (int f = 0; f < SLACK_NF; ++f) bad = bad || !is_finite(gs[f]);
#pragma unroll
  for (int i = 0; i < SLACK_NC; ++i) bad = bad || !is_finite(gc[i]);
  const bool on1 = gs[1] != 0.0 || gc[4] != 0.0 || gc[5] != 0.0;
  bool on2 = gs[2] != 0.0;
#pragma unroll
  for (int i = 6; i < SLACK_NC; ++i) on2 = on2 || gc[i] != 0.0;
  bad = bad || (on1 && !is_finite(bc[0])) || (on2 && (!is_finite(bc[1]) || !is_finite(bc[2]) || !is_finite(bc[3])));
  const bool rowbad = ((__ballot(bad) >> T.rbase) & 0xFFFFull) != 0ull;
  const bool dead = rowbad || (STAGE == SLACKVJP_SEED && A.worst[b] == GRAD_NONFINITE);
  qt_fk<ROT>(U.K, q0, q1, scq0, scq1, M, P, fkn, s);
  const double* const qv = U.K.q;
  const double* const oMi = U.K.oMi;
  // ---- the forward's evaluation (wbc_slack.h), and the body mass table for the CoM columns
  slack_frames(U.pf, U.eul, oMi, L, s);
  double com0, com1, cm;
  slack_com_xy(oMi, L, s, com0, com1, cm);
  double jv;
  int jc;
  slack_joint_scan(qv, L, s, jv, jc);
  qt_body_mass_table(U.mcw, oMi, L.m0, L.m1, L.hb0, L.hb1, s);
  WSYNC();                                                          // pf, eul, mcw are visible
  double comp[SLACK_NC], sl[SLACK_NF];
  int wh[SLACK_NF];
  slack_components(U.pf, U.eul, com0, com1, bc, L, comp);
  slack_families(comp, jv, jc, sl, wh);
  // ---- the components' cotangents: a family's own goes to the component its scan selected
  double gm[SLACK_NC];
#pragma unroll
  for (int i = 0; i < SLACK_NC; ++i) {
    const int f = i < 4 ? 0 : (i < 6 ? 1 : 2), i0 = i < 4 ? 0 : (i < 6 ? 4 : 6);
    gm[i] = (wh[f] == i - i0) ? gc[i] + gs[f] : gc[i];
  }
  SvCot C;
  C.cfl[0] = gm[1]; C.cfl[1] = gm[3];
  C.crr[0] = -gm[0]; C.crr[1] = -gm[2];
  C.ccom[0] = gm[0] - gm[1]; C.ccom[1] = gm[2] - gm[3];
  C.cz = gm[4] - gm[5];
  const double ce0 = gm[6] - gm[7], ce1 = gm[8] - gm[9], ce2 = gm[10] - gm[11];
  {
    // the three atan2 angles through dR = [omega] R: d angle_a = N_a . omega (wbc_k_gradq.hip's three forms)
    const double* Pt = oMi + 12 * L.tjoint;                         // R column-major: R(i, j) = Pt[3 j + i]
    const double R00 = Pt[0], R10 = Pt[1], R20 = Pt[2], R01 = Pt[3], R11 = Pt[4], R21 = Pt[5], R02 = Pt[6], R12 = Pt[7], R22 = Pt[8];
    const double n0 = fma(R21, R21, R22 * R22), cxy = sqrt(n0), n1 = fma(R20, R20, n0), n2 = fma(R00, R00, R10 * R10);
    const double t1 = R20 / cxy;
    // (a zero cotangent takes no part: a degenerate rotation's 0 / 0 stays out of the rows of a family nobody seeded)
    const double g0 = ce0 != 0.0 ? ce0 / n0 : 0.0, g1 = ce1 != 0.0 ? ce1 / n1 : 0.0, g2 = ce2 != 0.0 ? ce2 / n2 : 0.0;
    const double a10 = g1 != 0.0 ? g1 * (-cxy * R10 + t1 * (R21 * R11 + R22 * R12)) : 0.0;
    const double a11 = g1 != 0.0 ? g1 * (cxy * R00 - t1 * (R21 * R01 + R22 * R02)) : 0.0;
    C.Ea[0] = g0 * (R22 * R11 - R21 * R12) + a10 + g2 * (-R00 * R20);
    C.Ea[1] = g0 * (R21 * R02 - R22 * R01) + a11 + g2 * (-R10 * R20);
    C.Ea[2] = g2 * (R00 * R00 + R10 * R10);
  }
  // ---- the lane's two DoF
  double l0[3], a0[3], l1[3], a1[3];
  qt_jac_cols(oMi, Dc, l0, a0, l1, a1);
  double t0 = h0 ? sw_dof_term(U.pf, U.mcw, M, d0, sub0, l0, a0, C, cm) : 0.0;
  double t1 = h1 ? sw_dof_term(U.pf, U.mcw, M, d1, sub1, l1, a1, C, cm) : 0.0;
  if (wh[3] >= 0 && gs[3] != 0.0) {                                 // the joint family: DoF code / 2, +gamma on the lower side, -gamma on the upper
    const int dj = wh[3] >> 1;
    const double gj = (wh[3] & 1) ? -gs[3] : gs[3];
    if (h0 && dj == d0) t0 += gj;
    if (h1 && dj == d1) t1 += gj;
  }
  const double bz = -(1.0 - L.z_frac) * gm[4] + (1.0 + L.z_frac) * gm[5];
  const double tb = (s == 0) ? bz : ((s == 1) ? -ce0 : ((s == 2) ? -ce1 : -ce2));
  if (!T.valid) return;
  if (STAGE == SLACKVJP_STATE) {
    if (A.d_q) {
      A.d_q[b * NV + d0] = (h0 && !rowbad) ? t0 : 0.0;
      if (d1 < NV) A.d_q[b * NV + d1] = (h1 && !rowbad) ? t1 : 0.0;
    }
    if (s < 4) {
      if (A.d_box) A.d_box[b * 4 + s] = rowbad ? 0.0 : tb;
      // which: the forward's row as wbc_state_slack gives it (-1 where it gives NaN), whatever the cotangents are
      if (A.which) {
        const bool wbad = qbad || (s == 1 && !is_finite(bc[0])) || (s == 2 && (!is_finite(bc[1]) || !is_finite(bc[2]) || !is_finite(bc[3])));
        const int w = (s == 0) ? wh[0] : (s == 1) ? wh[1] : (s == 2) ? wh[2] : wh[3];
        A.which[b * SLACK_NF + s] = wbad ? -1 : w;
      }
    }
    if (s == 0 && A.grad_status) A.grad_status[b] = rowbad ? GRAD_NONFINITE : GRAD_OK;
    return;
  }
  // ---- SEED
  if (s == 0 && rowbad) A.worst[b] = GRAD_NONFINITE;
  if (dead) return;
  if (h0 && t0 != 0.0) A.g[b * NV + d0] = A.g[b * NV + d0] + t0;
  if (h1 && t1 != 0.0) A.g[b * NV + d1] = A.g[b * NV + d1] + t1;
  if (s < 4 && A.acc_box && tb != 0.0) A.acc_box[b * 4 + s] = A.acc_box[b * 4 + s] + tb;
}

// The variants (wbc_common.h, "Kernel variant tables"): the part that instantiates the row, then the template arguments.
#ifndef SLACKVJP_PART
#define SLACKVJP_PART -1      // -1: everything in one unit
#endif
#define WBC_PART SLACKVJP_PART
#define WBC_KERNEL wbc_slackvjp_kernel
#define WBC_KPARAMS (const SlackVjpArgs)
typedef void (*SlackVjpKernel) WBC_KPARAMS;
#define SLACKVJP_VARIANTS(V) /* STAGE, ROT */ \
  V(0, SLACKVJP_STATE, false) \
  V(0, SLACKVJP_STATE, true) \
  V(0, SLACKVJP_SEED, false) \
  V(0, SLACKVJP_SEED, true)
#if SLACKVJP_PART == -1
SLACKVJP_VARIANTS(WBC_VARIANT_INST)
#else
SLACKVJP_VARIANTS(WBC_VARIANT_UNIT)
#endif
#if SLACKVJP_PART <= 0
static SlackVjpKernel slackvjp_variant(long long key) {
  SLACKVJP_VARIANTS(WBC_VARIANT_FIND)
  return nullptr;
}
int slackvjp_variant_count() { return 0 SLACKVJP_VARIANTS(WBC_VARIANT_COUNT); }
int launch_slackvjp(const SlackVjpArgs& a, int stage, void* stream, long long* key_out) {
  const long long key = variant_key(stage, a.rot != 0);
  if (key_out) *key_out = key;
  const SlackVjpKernel k = slackvjp_variant(key);
  if (!k) return WBC_E_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3((a.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, a);
  return check_launch("slack_vjp");
}
#endif

}  // namespace wbc
