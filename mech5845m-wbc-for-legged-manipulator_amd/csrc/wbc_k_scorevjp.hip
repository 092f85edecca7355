// wbc_k_scorevjp.hip — wbc_rollout_vjp_scored: the cotangent of the track scores err_sq_sum / err_final / err_max of wbc_k_traj.hip, formed
// where the sweep runs (include/wbc.h states the algebra). The sweep is wbc_rollout_vjp_tracks', kernel for kernel; in front
// of every tick's step layer and between LINK and the track stage it launches one stage of
//   wbc_scorevjp_kernel    four instances per wavefront (lane = 16 r + s)
//     SEED    FK over the whole-tree schedule DevPlan.q_fk at q_(k+1) (the whole-tree shape, wbc_qtree.h). Lane s < 6 owns frame s (0..4 the end
//             effectors, 5 the trunk): position, d = position - target of tick k, e = sqrt((dx dx + dy dy) + dz dz),
//                 c = ((2 g_sq + [k == K - 1] g_fin / e) + [k == err_max_tick] g_max / e) d          (the 1 / e terms: 0 where e == 0)
//             and stash[b][s][:] <- -c (0 for an unscored frame). Lane s then owns DoF s and 16 + s: the WORLD Jacobian column (pk_jac_col)
//             moved to each scored frame's origin, v = lin + ang x p, contracted with c as (v0 c0 + v1 c1) + v2 c2 and summed over the
//             frames in increasing order; g[d] += that sum. At k == K - 1 the per-instance test (non-finite g_err_* or q_final, err_max_tick
//             outside [0, K) under g_err_max != 0): worst[b] <- WBC_GRAD_NONFINITE. An instance with that status adds nothing.
//     TARGET  one lane per (instance, frame, component) in two passes: Ebar / TEbar += stash; at k == 0 the caller's d_ee_target /
//             d_trunk_target += stash too.
// An exact zero is not added (g and the target cotangents keep their bits, the sign of a zero included, under all-zero score cotangents).
// No atomics, no cross-lane arithmetic, nothing contracted into fused multiply-adds: identical calls give identical bits. Rows >= B are
// never written.
#include <hip/hip_runtime.h>
#include <math.h>
#include "wbc_packed.h"
#include "wbc_grad.h"
#include "wbc_scorevjp.h"

#ifdef WBC_QTREE_H
#error "wbc_qtree.h came in through an earlier include: qt_point would be contracted here; it must first be included behind the pragma below"
#endif
#pragma clang fp contract(off)
#include "wbc_qtree.h"      // behind the pragma: its arithmetic (qt_point) is this unit's, uncontracted

namespace wbc {

struct __attribute__((aligned(16))) VInst {
  QtKin K;
  double pf[24];                            // the six frames' world positions (stride 4)
  double c[24];                             // their cotangents (stride 4; 0 for an unscored frame)
};
struct __attribute__((aligned(16))) VSmemP { VInst I[4]; };
static_assert(sizeof(VInst) == 3456 && offsetof(VInst, pf) == 3072 && offsetof(VInst, c) == 3264, "the instance's LDS record");

// this DoF's term: sum over the scored frames the column moves of (lin + ang x p_f) . c_f, the frames in increasing order
__device__ __forceinline__ double sv_contract(const double* const pf, const double* const c, const DevModel& M, const int mask, const int d,
                                              const double (&lin)[3], const double (&ang)[3]) {
  double acc = 0.0;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const int fr = f < 5 ? WBC_FR_EE0 + f : WBC_FR_TRUNK;
    if (!((mask >> f) & 1) || !((M.frame_support[fr] >> d) & 1u)) continue;
    const double* p = pf + 4 * f;
    const double* cf = c + 4 * f;
    const double v0 = lin[0] + (ang[1] * p[2] - ang[2] * p[1]);
    const double v1 = lin[1] + (ang[2] * p[0] - ang[0] * p[2]);
    const double v2 = lin[2] + (ang[0] * p[1] - ang[1] * p[0]);
    acc = acc + ((v0 * cf[0] + v1 * cf[1]) + v2 * cf[2]);
  }
  return acc;
}

template <int STAGE, bool ROT>   // ROT: rotated joint placements in the batch (wbc_k_sim3p.hip); the TARGET stage has no kinematics
__global__ void __launch_bounds__(64) wbc_scorevjp_kernel(const ScoreVjpArgs A) {
  const QtLane T(A.B); const int s = T.s;
  if (STAGE == SCOREVJP_TARGET) {
    if (!T.valid) return;                                           // (no cross-lane traffic in this stage: a lane may leave)
    const size_t b = (size_t)T.b_raw;
    if (A.worst[b] == GRAD_NONFINITE) return;                       // all-zero rows: LINK wrote them at k == 0, nothing is added
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int i = 16 * pass + s;                                  // 3 f + component
      if (i >= 18) continue;
      const double x = A.stash[b * 18 + i];
      if (x == 0.0) continue;
      double* e = i < 15 ? A.Ebar + b * 15 + i : A.TEbar + b * 3 + (i - 15);
      *e = *e + x;
      if (A.k == 0) {
        double* o = i < 15 ? (A.d_ee_target ? A.d_ee_target + b * 15 + i : nullptr) : (A.d_trunk_target ? A.d_trunk_target + b * 3 + (i - 15) : nullptr);
        if (o) *o = *o + x;
      }
    }
    return;
  }
  // ---- SEED
  __shared__ VSmemP SP;
  VInst& U = SP.I[T.r];
  const size_t b = T.b, nB = (size_t)A.B;
  const int mid = qt_model_index(A.model_id, b, A.n_models);
  const DevModel& M = A.models[mid];
  const DevPlan& P = A.plans[mid];
  const int nq = M.nq, nv = M.nv, mask = A.score_mask;
  const bool lastk = A.k == A.K - 1;
  // ---- every global read first
  const double* qg = A.q + b * NQ;
  const double q0 = qg[s], q1 = (16 + s < nq) ? qg[16 + s] : 0.0;
  DevPlan::PkJoint fkn = P.q_fk[0][s];
  const int scq0 = P.q_scq[(2 + s) & 31], scq1 = P.q_scq[(18 + s) & 31];
  const int f = s < 6 ? s : 0;                                      // frame of this lane
  const bool scored = s < 6 && ((mask >> f) & 1);
  const int fr = f < 5 ? WBC_FR_EE0 + f : WBC_FR_TRUNK;
  const int fjoint = M.frame_joint[fr];
  const double f0 = M.frame_p[fr][0], f1 = M.frame_p[fr][1], f2 = M.frame_p[fr][2];
  const size_t gi = (size_t)__popc((unsigned)mask & ((1u << f) - 1u)) * nB + b;
  const double gsq = (scored && A.g_sq) ? A.g_sq[gi] : 0.0;
  const double gfin = (scored && lastk && A.g_fin) ? A.g_fin[gi] : 0.0;
  const double gmax = (scored && A.g_max) ? A.g_max[gi] : 0.0;
  const int tk = (scored && A.g_max) ? A.err_max_tick[gi] : -1;
  const double* tg = (scored && f == WBC_TARGET_TRUNK) ? A.trunk_target + b * 3 : A.ee_target + b * 15 + 3 * f;   // the target tick k saw
  const double t0 = scored ? tg[0] : 0.0, t1 = scored ? tg[1] : 0.0, t2 = scored ? tg[2] : 0.0;
  const QtDof Dc(M, s, nv);                                         // DoF of this lane
  const int d0 = Dc.d0, d1 = Dc.d1; const bool h0 = Dc.h0, h1 = Dc.h1;
  const bool bad = lastk && ((s < nq && !is_finite(q0)) || (16 + s < nq && !is_finite(q1)) || !is_finite(gsq) || !is_finite(gfin) ||
                             !is_finite(gmax) || (gmax != 0.0 && (tk < 0 || tk >= A.K)));
  const bool rowbad = ((__ballot(bad) >> T.rbase) & 0xFFFFull) != 0ull;
  const bool dead = rowbad || A.worst[b] == GRAD_NONFINITE;
  qt_fk<ROT>(U.K, q0, q1, scq0, scq1, M, P, fkn, s);
  const double* const oMi = U.K.oMi;
  // ---- the frame's position, d, e and c (wbc_traj_tick_kernel's expressions on the recomputed position)
  double cx = 0.0, cy = 0.0, cz = 0.0;
  {
    const double* Pj = oMi + 12 * fjoint;
    const double px = qt_point(Pj, f0, f1, f2, 0), py = qt_point(Pj, f0, f1, f2, 1), pz = qt_point(Pj, f0, f1, f2, 2);
    if (scored && !dead) {
      const double dx = px - t0, dy = py - t1, dz = pz - t2;
      const double e2 = (dx * dx + dy * dy) + dz * dz;
      const double e = sqrt(e2);
      double coef = 2.0 * gsq;
      if (e > 0.0) {
        coef = coef + (lastk ? gfin / e : 0.0);
        coef = coef + (A.k == tk ? gmax / e : 0.0);
      }
      cx = coef * dx; cy = coef * dy; cz = coef * dz;
    }
    if (s < 6) {
      U.pf[4 * s] = px; U.pf[4 * s + 1] = py; U.pf[4 * s + 2] = pz;
      U.c[4 * s] = cx; U.c[4 * s + 1] = cy; U.c[4 * s + 2] = cz;
    }
  }
  WSYNC();
  // ---- WORLD Jacobian columns of the lane's two DoF, moved to each scored frame and contracted with its c
  double l0[3], a0[3], l1[3], a1[3];
  qt_jac_cols(oMi, Dc, l0, a0, l1, a1);
  const double acc0 = h0 ? sv_contract(U.pf, U.c, M, mask, d0, l0, a0) : 0.0;
  const double acc1 = h1 ? sv_contract(U.pf, U.c, M, mask, d1, l1, a1) : 0.0;
  if (!T.valid) return;
  if (s < 6) {
    double* st = A.stash + b * 18 + 3 * s;
    const bool z = !scored || dead;
    st[0] = z ? 0.0 : -cx; st[1] = z ? 0.0 : -cy; st[2] = z ? 0.0 : -cz;
  }
  if (s == 0 && rowbad) A.worst[b] = GRAD_NONFINITE;
  if (dead) return;
  if (h0 && acc0 != 0.0) A.g[b * NV + d0] = A.g[b * NV + d0] + acc0;
  if (h1 && acc1 != 0.0) A.g[b * NV + d1] = A.g[b * NV + d1] + acc1;
}

// The variants (wbc_common.h, "Kernel variant tables"): the part that instantiates the row, then the template arguments.
#ifndef SCOREVJP_PART
#define SCOREVJP_PART -1      // -1: everything in one unit
#endif
#define WBC_PART SCOREVJP_PART
#define WBC_KERNEL wbc_scorevjp_kernel
#define WBC_KPARAMS (const ScoreVjpArgs)
typedef void (*ScoreVjpKernel) WBC_KPARAMS;
#define SCOREVJP_VARIANTS(V) /* STAGE, ROT */ \
  V(0, SCOREVJP_SEED, false) \
  V(0, SCOREVJP_SEED, true) \
  V(0, SCOREVJP_TARGET, false)
#if SCOREVJP_PART == -1
SCOREVJP_VARIANTS(WBC_VARIANT_INST)
#else
SCOREVJP_VARIANTS(WBC_VARIANT_UNIT)
#endif
#if SCOREVJP_PART <= 0
static ScoreVjpKernel scorevjp_variant(long long key) {
  SCOREVJP_VARIANTS(WBC_VARIANT_FIND)
  return nullptr;
}
int scorevjp_variant_count() { return 0 SCOREVJP_VARIANTS(WBC_VARIANT_COUNT); }
int launch_scorevjp(const ScoreVjpArgs& a, int stage, void* stream, long long* key_out) {
  const long long key = variant_key(stage, stage == SCOREVJP_SEED && a.rot != 0);
  if (key_out) *key_out = key;
  const ScoreVjpKernel k = scorevjp_variant(key);
  if (!k) return WBC_E_UNSUPPORTED;
  hipLaunchKernelGGL(k, dim3((a.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, a);
  return check_launch("rollout_vjp_scored");
}
#endif

}  // namespace wbc
