// wbc_slack.h — what the kernels of wbc_state_slack / wbc_rollout_watch (wbc_k_slack.hip) consume, and their launchers (internal, C++). A
// header of its own, as wbc_traj.h: the tick / update / trajectory kernels' translation units do not see it. Behind wbc_qtree.h (the two
// kernel units, wbc_k_slack.hip and wbc_k_slackvjp.hip) it also holds the ONE evaluation of the slack: the frames, the CoM, the joint scan,
// the components and the family scans as inline functions, so that the forward and its cotangent select the same component bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "wbc_device.h"

namespace wbc {

constexpr int SLACK_NF = WBC_N_SLACK;          // families: CoM box, trunk z, trunk angles, joint range
constexpr int SLACK_NC = 12;                   // components of families 0..2 in code order: 4 + 2 + 6

// The model's own position range by velocity DoF (WbcModelBlob.q_lo / q_hi of the DoF's own joint): DoF d looks at q[qi[d]]. One per model
// of the handle, built on first use (the range is the model's, not the configuration's; cfg.lock_from bounds the DoF that count).
struct SlackLimits {
  double lo[NL], hi[NL];
  int32_t qi[NL];
};

// One launch evaluates the four families at q for every instance. `slack` / `which` / `components`: the row outputs of wbc_state_slack
// (each may be null). `mask` != 0: the roll-out's watch — lane s < 4 of an instance's row folds family s (if watched) of tick k into row
// w = popcount(mask below bit s) of the accumulators, [n_w][B] each; tick 0 initialises them, so no reset launch precedes it.
struct SlackArgs {
  const DevModel* models;
  const WbcConfig* cfgs;
  const DevPlan* plans;
  const SlackLimits* lim;
  int32_t B, n_models, rot, k;
  const double* q;                      // [B][27]
  const double* box;                    // [B][4] trunk_box_center, or null: families 1 and 2 are NaN / -1
  const int32_t* model_id;
  double* slack;                        // [B][4]
  int32_t* which;                       // [B][4]
  double* components;                   // [B][12]
  int32_t mask, pad_;
  double *slack_min, *slack_final;      // [n_w][B]
  int32_t *min_tick, *min_which, *neg_ticks, *first_neg;
  double* trace;                        // [n_w][B] of this tick, or null
};

struct SlackGroupArgs {
  int32_t G, M, n_w, pad_;              // G groups of M consecutive instances; [n_w][G * M] in, [n_w][G] out
  const double* slack_min;
  const int32_t* neg_ticks;
  double* group_min;                    // each optional
  int32_t* group_neg_instances;
};

int launch_slack(const SlackArgs& a, void* stream);               // four instances per wavefront, grid = ceil(B / 4)
int launch_slack_groups(const SlackGroupArgs& a, void* stream);   // one wavefront per group

#ifdef WBC_QTREE_H
// ---- The evaluation (device; the whole-tree shape of wbc_qtree.h: lane = 16 r + s, every lane of an instance's row alike unless said). Both
// units compile it under the default floating-point contraction: wbc_k_slackvjp.hip may not put it behind a pragma of its own.

// (v, c) <- the smaller of (v, c) and (ov, oc): by value, a tie by the lower code — what a scan in increasing code order with a strict < gives
__device__ __forceinline__ void slack_take(double& v, int& c, const double ov, const int oc) {
  if (ov < v || (ov == v && oc < c)) { v = ov; c = oc; }
}
template <int CTRL>
__device__ __forceinline__ void slack_take_dpp(double& v, int& c) {
  const double ov = dpp<CTRL>(v);
  const int oc = __builtin_amdgcn_update_dpp(c, c, CTRL, 0xF, 0xF, false);
  slack_take(v, c, ov, oc);
}
// minimum of N components scanned in increasing code order with a strict <
template <int N>
__device__ __forceinline__ void slack_scan(const double* c, double& v, int& w) {
  v = c[0]; w = 0;
#pragma unroll
  for (int i = 1; i < N; ++i) if (c[i] < v) { v = c[i]; w = i; }
}

// What a lane loads for the evaluation with its other global reads (before qt_fk): its frame (FL foot, RR foot — EE_frame_pos[1], [2], the CoM
// box's corners — on lanes 0 and 1, else the trunk), its two bodies' mass records and its two free DoF's range.
struct SlackLane {
  int fjoint, tjoint, j1; double f0, f1, f2;
  bool hb0, hb1; DevPlan::QJnt m0, m1;                 // bodies of this lane: joints s (>= 1) and 16 + s
  bool hd0, hd1; int qi0, qi1; double lo0, hi0, lo1, hi1;   // free DoF of this lane: d = s and 16 + s
  double z_frac, box_ang;
  __device__ __forceinline__ SlackLane(const DevModel& M, const WbcConfig& cfg, const DevPlan& P, const SlackLimits& Lm, const int s) {
    const int nv = M.nv, nj = M.njoints;
    const int fr = (s == 0) ? WBC_FR_EE0 + 1 : ((s == 1) ? WBC_FR_EE0 + 2 : WBC_FR_TRUNK);
    fjoint = M.frame_joint[fr];
    f0 = M.frame_p[fr][0]; f1 = M.frame_p[fr][1]; f2 = M.frame_p[fr][2];
    tjoint = M.frame_joint[WBC_FR_TRUNK];
    j1 = 16 + s;
    hb0 = s >= 1 && s < nj; hb1 = j1 < nj;
    m0 = P.q_jm[hb0 ? s : 1]; m1 = P.q_jm[hb1 ? j1 : 1];
    const int lock = cfg.lock_from;
    hd0 = s >= 6 && s < lock && s < nv; hd1 = j1 < lock && j1 < nv;
    qi0 = Lm.qi[hd0 ? s : 6]; qi1 = Lm.qi[hd1 ? j1 : 6];
    lo0 = Lm.lo[hd0 ? s : 6]; hi0 = Lm.hi[hd0 ? s : 6]; lo1 = Lm.lo[hd1 ? j1 : 6]; hi1 = Lm.hi[hd1 ? j1 : 6];
    z_frac = cfg.trunk_box_z_frac; box_ang = cfg.trunk_box_ang;
  }
};

// frame origins into pf (FL foot, RR foot, trunk frame: stride 4) and the trunk's Euler angles into eul (one atan2 per row on lanes 0..2, the
// tick kernels' formula: wbc_common.h, P6). The caller fences before it reads them.
__device__ __forceinline__ void slack_frames(double* const pf, double* const eul, const double* const oMi, const SlackLane& L, const int s) {
  const double* Pj = oMi + 12 * L.fjoint;
  const double* Pt = oMi + 12 * L.tjoint;                           // R column-major: R(i, j) = Pt[3 j + i]
  const double R21 = Pt[5], R22 = Pt[8], R20 = Pt[2], R10 = Pt[1], R00 = Pt[0];
  const double ay = (s == 0) ? R21 : ((s == 1) ? -R20 : R10);
  const double ax = (s == 0) ? R22 : ((s == 1) ? sqrt(fma(R21, R21, R22 * R22)) : R00);
  const double e = atan2(ay, ax);
  if (s < 3) {
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) pf[4 * s + rr] = qt_point(Pj, L.f0, L.f1, L.f2, rr);
    eul[s] = e;
  }
}

// data.com[0], x and y: lane s sums m_j (R_j c_j + p_j) over joints s and 16 + s in that order, then the row butterfly and one division each
// (qt_body_mass_table's centres, but two components summed per lane in this order: spelled out, and not through qt_point). cm: the total mass.
__device__ __forceinline__ void slack_com_xy(const double* const oMi, const SlackLane& L, const int s, double& com0, double& com1, double& cm) {
  double cx = 0.0, cy = 0.0;
  cm = 0.0;
  const DevPlan::QJnt &m0 = L.m0, &m1 = L.m1;
  const double* Pa = oMi + 12 * (L.hb0 ? s : 1);
  const double* Pb = oMi + 12 * (L.hb1 ? L.j1 : 1);
  const double xa = Pa[9] + Pa[0] * m0.c0 + Pa[3] * m0.c1 + Pa[6] * m0.c2, ya = Pa[10] + Pa[1] * m0.c0 + Pa[4] * m0.c1 + Pa[7] * m0.c2;
  const double xb = Pb[9] + Pb[0] * m1.c0 + Pb[3] * m1.c1 + Pb[6] * m1.c2, yb = Pb[10] + Pb[1] * m1.c0 + Pb[4] * m1.c1 + Pb[7] * m1.c2;
  if (L.hb0) { cx = m0.m * xa; cy = m0.m * ya; cm = m0.m; }
  if (L.hb1) { cx += m1.m * xb; cy += m1.m * yb; cm += m1.m; }
  cx = rsum16(cx); cy = rsum16(cy); cm = rsum16(cm);
  com0 = cx / cm; com1 = cy / cm;
}

// joint range: one DoF pair per lane, then a 16-lane minimum that carries the code (2 d lower side, 2 d + 1 upper side; no free DoF: +inf, -1)
__device__ __forceinline__ void slack_joint_scan(const double* const qv, const SlackLane& L, const int s, double& jv, int& jc) {
  jv = __longlong_as_double(0x7FF0000000000000ll);
  jc = INT_MAX;
  const double x0 = qv[L.qi0], x1 = qv[L.qi1];
  if (L.hd0) { slack_take(jv, jc, x0 - L.lo0, 2 * s); slack_take(jv, jc, L.hi0 - x0, 2 * s + 1); }
  if (L.hd1) { slack_take(jv, jc, x1 - L.lo1, 2 * L.j1); slack_take(jv, jc, L.hi1 - x1, 2 * L.j1 + 1); }
  slack_take_dpp<DPP_XOR1>(jv, jc); slack_take_dpp<DPP_XOR2>(jv, jc); slack_take_dpp<DPP_HALF_MIRROR>(jv, jc); slack_take_dpp<DPP_MIRROR>(jv, jc);
  if (jc == INT_MAX) jc = -1;
}

// the components of families 0..2 in code order (bc: the instance's trunk_box_center)
__device__ __forceinline__ void slack_components(const double* const pf, const double* const eul, const double com0, const double com1,
                                                 const double (&bc)[4], const SlackLane& L, double (&comp)[SLACK_NC]) {
  const double* pFL = pf;
  const double* pRR = pf + 4;
  comp[0] = -(pRR[0] - com0); comp[1] = pFL[0] - com0;
  comp[2] = -(pRR[1] - com1); comp[3] = pFL[1] - com1;
  const double z = pf[8 + 2], v = bc[0] * L.z_frac;
  comp[4] = -((bc[0] - v) - z); comp[5] = (bc[0] + v) - z;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double e = eul[a];
    comp[6 + 2 * a] = -((bc[1 + a] - L.box_ang) - e); comp[7 + 2 * a] = (bc[1 + a] + L.box_ang) - e;
  }
}

// the four families: the scans of families 0..2, the joint scan's result as family 3
__device__ __forceinline__ void slack_families(const double (&comp)[SLACK_NC], const double jv, const int jc, double (&sl)[SLACK_NF],
                                               int (&wh)[SLACK_NF]) {
  slack_scan<4>(comp, sl[0], wh[0]);
  slack_scan<2>(comp + 4, sl[1], wh[1]);
  slack_scan<6>(comp + 6, sl[2], wh[2]);
  sl[3] = jv; wh[3] = jc;
}
#endif   // WBC_QTREE_H

}  // namespace wbc
