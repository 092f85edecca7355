// wbc_packed.h — what the packed kernels share (four instances per wavefront, lane = 16 r + s): the packed sim3 tick's LDS layout, the DPP
// row reductions and broadcast, chol_sweep2, the dual active-set's factor updates (pk_qp_products, pk_qp_add_step, pk_qp_drop_slot, with their scalar
// cores pk_givens / pk_householder and the working-set decoder pk_ws_bits), the wave order, and the kinematics and input staging every packed
// tick / update kernel runs — the FK seed and level sweep (pk_fk_seed, pk_fk_sweep), the WORLD Jacobian column of a DoF (pk_jac_col), calcTargetVelTrunk2 (pk_trunk_target_vel) with its
// inputs (pk_trunk_input), the EE orientation feed-forward (pk_ee_omega) and the staged weights image (pk_stage_weights). The per-DoF
// velocity damper and the Euler matrix, which the one-instance kernels use too, are in wbc_common.h (damper_bounds, euler_to_R).
#pragma once
#include "wbc_common.h"
#include "wbc_wave_geom.h"

namespace wbc {

// ================================================================================================
// The PACKED sim3-tick kernel: FOUR robot instances per wavefront, one per 16-lane DPP row.
//
// The compact kernel above keeps one instance per wave, and its reduced QP (n' = 11 unknowns, <= 16 rows) lights 11-16 of the 64
// lanes: 3.3 k VALU wave-instructions per tick for ~1.4e4 useful flops. Here lane = 16 r + s: instance r of the wave, s = reduced
// variable / constraint row / FK slot. Every stage is written for 16 lanes:
//   FK          level-synchronous over a per-plan schedule (DevPlan.pk_fk: at most five joints per tree level — four legs + the
//               arm chain), sin/cos of the joint angles computed beforehand two per lane;
//   columns     lane s owns the WORLD Jacobian column of reduced variable s (task rows, trunk-box rows) and of eliminated leg DoF
//               s < 12 (contact rows -> K_e, velocity bounds);
//   assembly    row s of H' accumulated straight into registers from the task image At (LDS), G = -K^-1 B on lanes s < 12;
//   QP          the dual active-set of qp_core with per-row state: reductions are DPP row butterflies (no v_readlane), a value
//               at a row-dependent lane comes through ds_bpermute, the Cholesky column is broadcast through a per-instance LDS
//               vector, control flow is per-row predication with the loops running to the slowest of the four instances.
// Applies to the sim3 switch-set family only (launch_tick_auto): Grip task or none, optionally the trunk task (TRUNK variant), posture PREV /
// Tikhonov / static HYBRID, trunk box + foot contacts, velocity bounds on, no CoM rows; working sets in and out on the WARM variant; the gripper's
// orientation reference is honoured. A rank-deficient leg block is pivoted in place (the swap); instances with a
// leg block of rank < 2 are redone on the general path by their own wave at the end of this kernel (the tail: tail_instance). Same arithmetic per
// instance as process_sim3.
// ================================================================================================
constexpr int PLD = 14;                     // row stride of the matrices (even: rows are 16-byte aligned for ds_read_b128; 7 s mod 16 is a
                                            // permutation, so "lane = row" b128 reads of two instances interleave conflict-free)
constexpr int PN = 16;                      // lanes = constraint rows per instance
constexpr int PV = 12;                      // reduced variables per instance the packed kernel is compiled for (n' = 11 / 10 here)
struct __attribute__((aligned(16))) PInst {
  double M1[PV * PLD];                      // oMi scratch (runs on into M2: 22 joints x 12 doubles) -> T = R^-1
  double M2[PV * PLD];                      // ... sin / cos table in its tail during FK; then At [16][6], K / B scratch -> J
  double Cq[PN * 6];                        // reduced constraint rows x base columns (all the reduced rows touch the base only);
                                            // rows p_keep + l are the rows of G (eliminated leg DoF l x base DoF)
  double pad_[8];
};
struct __attribute__((aligned(16))) PVec {
  double in[40];                            // q [27], gripper target [3] @28, previous [3] @31, trunk box centre [4] @34
  double xv[PN], dv[PN], yv[PN], tv[PN];
  double cl[32];                            // row-bound staging -> Cholesky column broadcast (entries 12..31 zero) -> qdot by DoF
  double pad_[8];
};
// Bank placement (ds_read_b64 / b128 bank = dword address mod 64; the four instances of a wave issue every access together): the vectors are read
// as broadcasts or "lane = element" b64, which collide when the instances sit a multiple of the 256-byte bank row apart and are conflict-free
// 128 B (mod 256) apart. The matrix blocks sat a multiple of 256 B apart in round 2 (measured best for the "lane = row" b128 reads then);
// with the broadcast row reads the kernel has since (At / Cq rows in the H' accumulation, the violation scan and normal_d: all lanes of an
// instance on one address, four instances on four) that distance made all four meet in one bank group — 192 B (mod 256) apart measures
// +1.3 % on the benchmark (same-box A/B, four rounds: 330.1 vs 325.9 M ticks/s; 160 B apart +0.6 %).
static_assert(sizeof(PInst) % 256 == 192, "matrix blocks: 192 B (mod the 256-byte bank row) apart");
static_assert(sizeof(PVec) % 256 == 128, "vector blocks: half a bank row apart (mod 256 B)");
struct __attribute__((aligned(16))) SmemP { PInst I[4]; PVec V[4]; };

__device__ __forceinline__ double rsum16(double v) {     // sum over the lane's 16-lane row, result in every lane of the row
  v += dpp<DPP_XOR1>(v); v += dpp<DPP_XOR2>(v); v += dpp<DPP_HALF_MIRROR>(v); v += dpp<DPP_MIRROR>(v);
  return v;
}
__device__ __forceinline__ double rmin16(double v) {
  v = fmin(v, dpp<DPP_XOR1>(v)); v = fmin(v, dpp<DPP_XOR2>(v)); v = fmin(v, dpp<DPP_HALF_MIRROR>(v)); v = fmin(v, dpp<DPP_MIRROR>(v));
  return v;
}
__device__ __forceinline__ double bperm(double v, int src_lane) {     // v of lane src_lane (any lane index 0..63, per lane)
  const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int bpermi(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_or(unsigned long long v) {
  int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  lo |= __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  hi |= __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ unsigned long long ror16(unsigned long long v) {   // bitwise OR over the lane's 16-lane row
  v = dpp_or<DPP_XOR1>(v); v = dpp_or<DPP_XOR2>(v); v = dpp_or<DPP_HALF_MIRROR>(v); v = dpp_or<DPP_MIRROR>(v);
  return v;
}

// ---- the same reductions for call sites at which ALL 64 LANES ARE ACTIVE. dpp<> passes the moved value as the instruction's
// `old` operand too, which ties the destination to it: the compiler copies each half first (v_mov_b32 tmp, src; v_mov_b32_dpp tmp, src). dpp_all<>
// has no `old` (bound_ctrl: a lane whose source lane is switched off in exec reads 0 instead of keeping its own value) and needs no copy. The two
// are the same function wherever every source lane is active — the row controls used here never leave the row, so that is the only difference.
// Rows of a short last wave (valid == false) are active lanes. A site inside a divergent region keeps dpp<>. The packed sim3 tick alone uses
// these (every rsum16 / rmin16 / ror16 site of wbc_k_sim3p.hip sits in wave-uniform control flow); the other packed kernels keep theirs.
// A/B switch (make variant VFLAGS=-D...): SIM3P_DPP_COPY gives the sim3 tick the copying helpers back.
template <int CTRL>
__device__ __forceinline__ double dpp_all(double v) {
#ifdef SIM3P_DPP_COPY
  return dpp<CTRL>(v);
#else
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
#endif
}
__device__ __forceinline__ double rsum16a(double v) {
  v += dpp_all<DPP_XOR1>(v); v += dpp_all<DPP_XOR2>(v); v += dpp_all<DPP_HALF_MIRROR>(v); v += dpp_all<DPP_MIRROR>(v);
  return v;
}
__device__ __forceinline__ double rmin16a(double v) {
  v = fmin(v, dpp_all<DPP_XOR1>(v)); v = fmin(v, dpp_all<DPP_XOR2>(v)); v = fmin(v, dpp_all<DPP_HALF_MIRROR>(v)); v = fmin(v, dpp_all<DPP_MIRROR>(v));
  return v;
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_or_all(unsigned long long v) {
#ifdef SIM3P_DPP_COPY
  return dpp_or<CTRL>(v);
#else
  int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  lo |= __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
  hi |= __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
#endif
}
__device__ __forceinline__ unsigned long long ror16a(unsigned long long v) {
  v = dpp_or_all<DPP_XOR1>(v); v = dpp_or_all<DPP_XOR2>(v); v = dpp_or_all<DPP_HALF_MIRROR>(v); v = dpp_or_all<DPP_MIRROR>(v);
  return v;
}

// The value of lane K of the caller's 16-lane row, in every lane of the row: ONE v_mov_b64_dpp row_newbcast:K — no LDS, no wait.
// The contract of rsum16a & co. above: only where ALL 64 LANES ARE ACTIVE, in wave-uniform control flow. There is no `old` operand (bound_ctrl): a
// lane whose source lane is switched off in exec reads 0, not its own value. Rows of a short last wave (valid == false) are active lanes. The
// 64-bit builtin form is the one that lowers to a single move; the two-halves form of dpp_all<> gives two v_mov_b32_dpp.
template <int K>
__device__ __forceinline__ double row_bc(double v) {
  static_assert(K >= 0 && K < 16, "a lane of the 16-lane row");
  return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + K, 0xF, 0xF, true);
}
template <int N, int K0, int K = K0>
__device__ __forceinline__ void row_bc_from(double (&c)[N], const double v) {     // c[k] = row_bc<k>(v), k = K0 .. N - 1
  if constexpr (K < N) { c[K] = row_bc<K>(v); row_bc_from<N, K0, K + 1>(c, v); }
}

// The packed kernels' Cholesky sweep H' = L L' fused with the forward substitution L y = rhs (y comes in holding the lane's right-hand side: e_s, or g'
// on a padding lane), two columns per trip: the raw columns j and j + 1 of every row go through the LDS vectors c0v / c1v together and each lane redoes,
// for the rows below, the one update that column j + 1 receives from step j — the same operations in the same order as two single steps, one LDS round
// trip instead of two. Fully unrolled on fixed registers (round 4): trip j reads and updates the entries k >= j only — for N = 12: 42 b128 reads and
// 156 multiply-adds over the sweep instead of the 72 and 306 of the rotating-register loop this replaces (which did the rest on zeros: same results
// bit for bit); N = 16: 72 / 288 instead of 128 / 568. `wr`: this lane carries a row (s < N). Returns the smallest pivot (-1: not positive / NaN).
template <int N>
__device__ __forceinline__ double chol_sweep2(double (&h)[N], double (&y)[N], double* const c0v, double* const c1v, const int s, const bool wr) {
  double pmin = 1.0;
#pragma unroll
  for (int j = 0; j < N; j += 2) {
    WSYNC();
    if (wr) { c0v[s] = h[j]; c1v[s] = h[j + 1]; }
    WSYNC();
    double cm0[N], cm1[N];
#pragma unroll
    for (int k = j; k < N; k += 2) {
      const double2a v0 = lds2(c0v + k), v1 = lds2(c1v + k);
      cm0[k] = v0.x; cm0[k + 1] = v0.y; cm1[k] = v1.x; cm1[k + 1] = v1.y;
    }
    const double pj = cm0[j];
    pmin = (pj > 0.0) ? fmin(pmin, pj) : -1.0;
    const double rinv = rsqrt(pj), ipj = rinv * rinv;
    // step j on this row
    const double th = h[j] * ipj, ty = y[j] * ipj, yk = y[j] * rinv;
    const double h1 = fma(-th, cm0[j + 1], h[j + 1]), y1 = fma(-ty, cm0[j + 1], y[j + 1]);
    // step j as it acts on column j + 1 of the rows below (what their own lanes compute for themselves)
    const double a = cm0[j + 1];
#pragma unroll
    for (int k = j + 1; k < N; ++k) cm1[k] = fma(-(cm0[k] * ipj), a, cm1[k]);
    const double pj2 = cm1[j + 1];
    pmin = (pj2 > 0.0) ? fmin(pmin, pj2) : -1.0;
    const double rinv2 = rsqrt(pj2), ipj2 = rinv2 * rinv2;
    const double th2 = h1 * ipj2, ty2 = y1 * ipj2, yk2 = y1 * rinv2;
#pragma unroll
    for (int k = j + 2; k < N; ++k) h[k] = fma(-th2, cm1[k], fma(-th, cm0[k], h[k]));
#pragma unroll
    for (int k = j + 2; k < N; ++k) y[k] = fma(-ty2, cm1[k], fma(-ty, cm0[k], y[k]));
    y[j] = fma(-ty2, 0.0, yk); y[j + 1] = yk2;
  }
  return pmin;
}
// The same sweep with its columns taken by DPP row broadcast instead of through LDS: entry k of column j is h[j] of lane k of the
// same 16-lane row, so trip j takes cm0[k] = row_bc<k>(h[j]), cm1[k] = row_bc<k>(h[j + 1]) for the k >= j the LDS form reads and goes on with the
// same expressions in the same order — the same bits, without the six store / ds_read_b128 round trips that each stood in front of a pivot's
// rsqrt chain. row_bc's contract: call it at top level, all 64 lanes active. Lanes s >= N are a source for no k < N and run the same arithmetic
// on their own h as in the LDS form. The packed sim3 tick alone uses it; the orth and box ticks keep the LDS form.
template <int N, int J = 0>
__device__ __forceinline__ void chol_sweep2_bc_trip(double (&h)[N], double (&y)[N], double& pmin) {
  if constexpr (J < N) {
    constexpr int j = J;
    double cm0[N], cm1[N];
    row_bc_from<N, j>(cm0, h[j]);
    row_bc_from<N, j>(cm1, h[j + 1]);
    const double pj = cm0[j];
    pmin = (pj > 0.0) ? fmin(pmin, pj) : -1.0;
    const double rinv = rsqrt(pj), ipj = rinv * rinv;
    // step j on this row
    const double th = h[j] * ipj, ty = y[j] * ipj, yk = y[j] * rinv;
    const double h1 = fma(-th, cm0[j + 1], h[j + 1]), y1 = fma(-ty, cm0[j + 1], y[j + 1]);
    // step j as it acts on column j + 1 of the rows below (what their own lanes compute for themselves)
    const double a = cm0[j + 1];
#pragma unroll
    for (int k = j + 1; k < N; ++k) cm1[k] = fma(-(cm0[k] * ipj), a, cm1[k]);
    const double pj2 = cm1[j + 1];
    pmin = (pj2 > 0.0) ? fmin(pmin, pj2) : -1.0;
    const double rinv2 = rsqrt(pj2), ipj2 = rinv2 * rinv2;
    const double th2 = h1 * ipj2, ty2 = y1 * ipj2, yk2 = y1 * rinv2;
#pragma unroll
    for (int k = j + 2; k < N; ++k) h[k] = fma(-th2, cm1[k], fma(-th, cm0[k], h[k]));
#pragma unroll
    for (int k = j + 2; k < N; ++k) y[k] = fma(-ty2, cm1[k], fma(-ty, cm0[k], y[k]));
    y[j] = fma(-ty2, 0.0, yk); y[j + 1] = yk2;
    // the trips stay six separate steps: without a fence between them nothing else keeps the scheduler from spreading the unrolled trips over
    // each other (the pin of qp_core's sweep, wbc_common.h)
#pragma unroll
    for (int k = j + 2; k < N; ++k) asm volatile("" : "+v"(h[k]), "+v"(y[k]));
    chol_sweep2_bc_trip<N, J + 2>(h, y, pmin);
  }
}
template <int N>
__device__ __forceinline__ double chol_sweep2_bc(double (&h)[N], double (&y)[N]) {
  static_assert(N % 2 == 0 && N <= 16, "two columns per trip; a row's lanes");
  double pmin = 1.0;
  chol_sweep2_bc_trip<N>(h, y, pmin);
  return pmin;
}

// ---- the dual active-set's factor updates: ONE text for the packed ticks. The orth and box ticks call all of it; the sim3 tick
// calls the Givens core and the seed decoder (its three steps are written out on PV / PLD: §3.33); the packed QP kernel, which keeps T as a packed
// triangle and J's row in registers (§3.16), takes the scalar cores pk_givens / pk_householder and the seed decoder. The method is
// qp_core's (Goldfarb-Idnani): with H = L L', J = L^-T Q and the working set's normals N = Q1 R, the kernels carry J [NJ][LDJ] (row s = variable
// s, column k = slot k; J1 = the first q columns, J2 the rest) and T = R^-1 [NT][LDT] (upper triangular in the first q slots, zero elsewhere).
// Lane s is row s of both, slot s of u / a_code (the slot's multiplier and its constraint code | side << 8); q is uniform over the 16-lane row.
// Every function is called by all 64 lanes in wave-uniform control flow; per-instance work is predicated (`dr`, `add`). sJ / sT: lane s, or the last
// row of J / T on the lanes beyond it (they read that row's shadow and never write). has_b: the lane carries a variable (stores to J).
// Working-set word w, entry i -> 0 none, 1 lower side, 2 upper side, 3 both (the caller drops those)
__device__ __forceinline__ int pk_ws_bits(const unsigned long long w, const int i) {
  return (int)(((w >> (i & 31)) & 1ull) | (((w >> (32 + (i & 31))) & 1ull) << 1));
}
// Givens rotation of a drop: the removed row of T leaves the pair (hrun, tb) in columns k, k + 1; (c, s) turns it into (0, rho)
struct PkGivens { double c, s, rho; };
__device__ __forceinline__ PkGivens pk_givens(const double hrun, const double tb) {
  const double nrm2 = fma(hrun, hrun, tb * tb);
  PkGivens g = {1.0, 0.0, 0.0};
  if (nrm2 > 0.0) { const double ri = rsqrt(nrm2); g.c = tb * ri; g.s = -hrun * ri; g.rho = nrm2 * ri; }
  return g;
}
// Householder reflection of an add: P = I - v v' / hv with P d2 = delta e_q, v = d2 - delta e_q, zn = |d2|^2, dq = d_q (delta takes the sign that
// avoids cancellation in v_q), hv = v'v / 2. Row s of J2 P is J2 - w v' with w = (J2 v)_s / hv = (z - delta jq) / hv; idel = 1 / delta. ok: v != 0
struct PkHouse { double delta, w, idel; bool ok; };
__device__ __forceinline__ PkHouse pk_householder(const double zn, const double dq, const double z, const double jq) {
  PkHouse o;
  const double rsz = frsq(zn), sz = zn * rsz;
  o.delta = (dq >= 0.0) ? -sz : sz;
  const double hv = zn - o.delta * dq;
  const double vv = 2.0 * hv;
  o.w = (z - o.delta * jq) * ((vv > 0.0) ? frcp(hv) : 0.0);
  o.idel = (dq >= 0.0) ? -rsz : rsz;
  o.ok = vv > 0.0;
  return o;
}
// With d = J'n staged (dv = d, yv = d restricted to the slots >= q): z = J2 d2 (the primal step direction, row s), r = T d1 (the dual one, slot s;
// want_r: some instance of the wave has an active constraint — nothing to do otherwise), and what the add step needs of slot q, read in the same
// round: dq = d_q, jq = J[s][q]
struct PkZr { double z, rv, dq, jq; };
template <int NJ, int LDJ, int NT, int LDT>
__device__ __forceinline__ PkZr pk_qp_products(const double* const J, const double* const T, const double* const dv, const double* const yv,
                                               const int sJ, const int sT, const int s, const int q, const bool has_b, const bool want_r) {
  constexpr int NTE = (NT + 1) & ~1;        // T's slots, two per read
  static_assert(NJ % 2 == 0 && NJ <= LDJ && NTE <= LDT && NTE <= 16, "rows are read in pairs inside their stride");
  PkZr o;
  double z = 0.0, zb = 0.0, rv = 0.0, rvb = 0.0;
  o.dq = dv[q & 15];
  o.jq = J[sJ * LDJ + (q & 15)];
#pragma unroll
  for (int k = 0; k < NJ; k += 2) {
    const double2a j2 = lds2(J + sJ * LDJ + k); const double2a y2 = lds2(yv + k);
    z = fma(j2.x, y2.x, z); zb = fma(j2.y, y2.y, zb);
  }
  z += zb;
  if (want_r) {
#pragma unroll
    for (int k = 0; k < NTE; k += 2) {
      const double2a t2 = lds2(T + sT * LDT + k); const double2a d2 = lds2(dv + k);
      rv = fma(t2.x, d2.x, rv); rvb = fma(t2.y, d2.y, rvb);
    }
    rv += rvb;
  }
  if (s >= q) rv = 0.0;
  if (!has_b) z = 0.0;
  o.z = z; o.rv = rv;
  return o;
}
// Add the constraint with code wc as slot q of the instances `add`: J2 <- J2 P (pk_householder), T gets the column (-r / delta, 1 / delta), the
// new slot's multiplier is u_new. The sweep over row s of J runs on d2 alone (yv = d for k >= q, else 0) and entry q is then stored with its own
// term — the same arithmetic as selecting v_k inside the loop, without two compares and four selects per pair. mark(): the caller's activity
// flag of the constraint's own lane.
template <int NJ, int LDJ, int NT, int LDT, class Mark>
__device__ __forceinline__ void pk_qp_add_step(double* const J, double* const T, const double* const yv, const int s, const bool has_b, const bool add,
                                               const double zn, const PkZr& zr, const int wc, const double u_new, double& u, int& a_code, int& q,
                                               Mark&& mark) {
  const PkHouse hh = pk_householder(zn, zr.dq, zr.z, zr.jq);
  if (add && has_b && hh.ok) {
#pragma unroll
    for (int k = 0; k < NJ; k += 2) {
      const double2a j2 = lds2(J + s * LDJ + k); const double2a y2 = lds2(yv + k);
      sts2(J + s * LDJ + k, fma(-hh.w, y2.x, j2.x), fma(-hh.w, y2.y, j2.y));
    }
    J[s * LDJ + q] = fma(-hh.w, zr.dq - hh.delta, zr.jq);
  }
  if (add) {
    if (s < q) T[s * LDT + q] = -zr.rv * hh.idel;
    if (s == q) { T[s * LDT + q] = hh.idel; u = u_new; a_code = wc; }
    mark();
    ++q;
  }
}
// Drop slot l_ of the instances `dr` (rare path): u / a_code of the slots behind it move up one (through yv / tv), and the Givens sequence read off
// the removed row l of T — rotation k = l .. q - 2 on the column pair (k, k + 1), pk_givens — makes T upper triangular again one slot shorter;
// J's columns take the same rotations (lane s: row s of J, and the row of T that becomes its new row s). The loop runs to the longest sequence
// of the wave. unmark(code): the caller's activity flag of the dropped constraint.
template <int NJ, int LDJ, int NT, int LDT, class Unmark>
__device__ __forceinline__ void pk_qp_drop_slot(double* const J, double* const T, double* const yv, double* const tv, const int sJ, const int sT,
                                                const int s, const int rbase, const bool has_b, const bool dr, const int l_, double& u, int& a_code,
                                                int& q, Unmark&& unmark) {
  const int l = dr ? l_ : 0;
  const int lc = bpermi(a_code, rbase + l) & 255;
  if (dr) unmark(lc);
  WSYNC();
  yv[s] = u; tv[s] = (double)a_code;
  WSYNC();
  if (dr && s >= l && s < q - 1) { u = yv[s + 1]; a_code = (int)tv[s + 1]; }
  if (dr && s == q - 1) { u = 0.0; a_code = 0; }
  const int srow = (sT >= l) ? ((sT + 1 < NT) ? sT + 1 : sT) : sT;
  double tx = T[srow * LDT + l];
  double jx = J[sJ * LDJ + l];
  double hrun = T[l * LDT + l];
  const int kend = dr ? q - 1 : 0;          // this instance's rotations run k = l .. q - 2
#pragma unroll 1
  for (int k0 = 0; k0 < NT - 1; ++k0) {
    const bool on = dr && (l + k0 < kend);
    if (!__ballot(on)) break;
    const int k = on ? l + k0 : 0;
    const PkGivens g = pk_givens(hrun, T[l * LDT + k + 1]);
    const double ty_ = T[srow * LDT + k + 1];
    const double jy = J[sJ * LDJ + k + 1];
    WSYNC();
    if (on) {
      hrun = g.rho;
      if (s < q - 1) T[s * LDT + k] = fma(g.c, tx, g.s * ty_);
      if (has_b) J[s * LDJ + k] = fma(g.c, jx, g.s * jy);
      tx = fma(-g.s, tx, g.c * ty_);
      jx = fma(-g.s, jx, g.c * jy);
    }
    WSYNC();
  }
  WSYNC();
  if (dr) {
    if (s < q) T[s * LDT + q - 1] = 0.0;
  }
  WSYNC();
  if (dr) {
    if (s < q) T[(q - 1) * LDT + s] = 0.0;
    if (has_b) J[s * LDJ + q - 1] = jx;
    --q;
  }
  WSYNC();
}

// ---- the wave order (KernelArgs.worder, wbc_device.h WaveOrder). A wave runs as many dual passes as the slowest of its four rows:
// each launch records how many iterations every instance needed, and the next launch on the same handle deals the instances out heaviest class first,
// so that heavy rows share waves and those waves start first. Results do not depend on it: an instance's arithmetic does not depend on its wave or row.
// Wave grp is wave k = grp / ns of slice grp mod ns (ns = ceil(waves / WO_SW)); its row r holds position j = 4 k + r of the slice's order.
// Work class of an instance from the dual iterations it ran, 0 the heaviest (>= 10, or redone by the kernel's tail) .. 5 (none).
__device__ __forceinline__ int wo_class(const int iters, const bool tail) {
  return (tail || iters >= 10) ? 0 : iters >= 6 ? 1 : iters >= 3 ? 2 : 5 - iters;
}
__device__ __forceinline__ uint32_t* wo_list(WaveOrder* wo, const uint32_t l, const int g, const int c) {
  return reinterpret_cast<uint32_t*>(wo + WO_NS) + ((size_t)(l * WO_NS + g) * WO_NCLS + c) * WO_CAP;
}
// The index arithmetic runs on launch constants (wbc_wave_geom.h WoGeom, the kernel's own extra parameter): ns and a reciprocal
// for grp / ns — one scalar multiply-high where the kernel used to run three signed 32-bit divisions by ns (the compiler's expansion: a float
// reciprocal and two correction rounds each) — and the slices' wave counts as quotient and remainder. Unsigned throughout. Each of wo_instance and
// wo_post forms g and k = grp / ns from the block index (three scalar instructions): carried from the kernel's entry to the end of the dual loop
// they would live in spill lanes (§3.23). wo_post hands g on to wo_finish. A/B switch: SIM3P_WO_DIVIDE divides.
static_assert(WO_GEOM_SW == (uint32_t)WO_SW && WO_GEOM_XMAX > (uint32_t)(WO_SW * WO_NS), "wbc_wave_geom.h: the slice width; the reciprocal's range covers every grid the order takes");
__device__ __forceinline__ uint32_t wo_divk(const WoGeom& wg, const uint32_t x) {
#ifdef SIM3P_WO_DIVIDE
  return (uint32_t)((int)x / (int)wg.ns);
#else
  return wo_div(wg, x);
#endif
}
// The instance row r of wave grp takes: the identity (pos = 4 grp + r < B) unless the slice's order was built for this batch size. The slice's
// block is wave-uniform (scalar loads at kernel entry); the index is read from the list of the position's class: the LAST class c with off[c] <= j
// (the offsets ascend), entry j - off[c] of list c — j + (c WO_CAP - off[c]) in the slice's lists, clamped to them (off[c] <= j < 4 WO_SW: the
// clamp changes nothing the launches write themselves; it keeps a stray block from turning into a read outside the allocation).
__device__ __forceinline__ int wo_instance(WaveOrder* __restrict__ wo, const WoGeom& wg, const int B, const int grp, const int r, const int pos) {
  if (!wo || wg.ns > (uint32_t)WO_NS) return pos;
  const uint32_t k = wo_divk(wg, (uint32_t)grp), g = wo_mod(wg, (uint32_t)grp, k);
  const WaveOrder& sl = wo[g];
#ifdef SIM3P_ENTRY_OLD_SLICE   // (A/B: B in a scalar round of its own, cur and the offsets in a second one behind the early return)
  if (sl.B != (uint32_t)B) return pos;
  const uint32_t cur = sl.cur & 1u, j = 4u * k + (uint32_t)r;
  uint32_t d = 0;
#pragma unroll
  for (int c = 1; c < WO_NCLS; ++c) {
    const uint32_t o = sl.off[c];
    if (j >= o) d = (uint32_t)(c * WO_CAP) - o;
  }
#else
  // cur, B and off[0..5] are bytes 16..47 of the block: ONE scalar load group, read before B is looked at — the same line either
  // way, and nothing is read through them unless B matches
  static_assert(offsetof(WaveOrder, cur) == 16 && offsetof(WaveOrder, B) == 20 && offsetof(WaveOrder, off) == 24, "cur, B, off[0..5]: eight words from byte 16");
  uint32_t w[8];
  const uint32_t* const wp = reinterpret_cast<const uint32_t*>(&sl) + 4;
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = wp[i];
  // (opaque: left alone the compiler sinks all but B behind the early return again, a second round to the same line)
  asm volatile("" : "+s"(w[0]), "+s"(w[1]), "+s"(w[2]), "+s"(w[3]), "+s"(w[4]), "+s"(w[5]), "+s"(w[6]), "+s"(w[7]));
  if (w[1] != (uint32_t)B) return pos;
  const uint32_t cur = w[0] & 1u, j = 4u * k + (uint32_t)r;
  uint32_t d = 0;
#pragma unroll
  for (int c = 1; c < WO_NCLS; ++c) {
    const uint32_t o = w[2 + c];
    if (j >= o) d = (uint32_t)(c * WO_CAP) - o;
  }
#endif
  const uint32_t i = wo_list(wo, cur, g, 0)[min(j + d, (uint32_t)(WO_NCLS * WO_CAP) - 1u)];
  return i < (uint32_t)B ? (int)i : B - 1;
}
// Append the wave's instances to its slice's class lists that the next launch reads and count the wave done: ONE returning 64-bit atomicAdd per
// wave carries both (the old word gives each row its place in its class list). The slice's last wave publishes the slice's order — prefix
// offsets from the final word, the list, the batch size it was built for, or 0 if the slice did not count each of its instances once — and zeroes
// the word the next launch will append to. No host sequence number: a captured graph replays this as it is. The lists are read by the next launch
// only. `valid`: the row holds an instance (b, class cls: uniform over the row).
// In two halves, so that the atomic's round trip runs behind the work between them: wo_post forms the wave's word and ISSUES the
// atomic — as soon as the classes are final, which is at the end of the dual loop — and wo_finish, at the end of the kernel, is the first to wait
// for the word that comes back: the list stores and the slice's publish step. A wave is counted at its post, so the publishing wave may find others
// of its slice still before their list stores; like the lists themselves, what it publishes is read by the next launch only. The slice's `cur` is
// read by wo_post, BEFORE the wave is counted, and handed on: once posted, the slice's block may be republished under this wave (a slice is
// published when every one of its waves has posted), so wo_finish must not read it again.
struct WoPost { unsigned long long old, add; unsigned same; uint32_t cur, ns, g; };   // old: in lane 0 alone, still in flight
__device__ __forceinline__ WoPost wo_post(WaveOrder* wo, const WoGeom& wg, const int grp, const bool valid, const int cls, const int r, const int s) {
  WoPost t; t.old = 0ull; t.add = 1ull << 54; t.same = 0u; t.cur = 0u;
  t.ns = wg.ns; t.g = 0u;
  if (t.ns > (uint32_t)WO_NS) return t;
  t.g = wo_mod(wg, (uint32_t)grp, wo_divk(wg, (uint32_t)grp));
  t.cur = wo[t.g].cur & 1u;
  const unsigned long long vm = __ballot(valid && s == 0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ck = __builtin_amdgcn_readlane(cls, 16 * k);
    const bool vk = (vm >> (16 * k)) & 1ull;
    t.same |= (vk && ck == cls) ? 1u << k : 0u;
    t.add += vk ? 1ull << (9 * ck) : 0ull;
  }
  if (r == 0 && s == 0) {
#ifdef SIM3P_LATE_ATOMIC
    t.old = atomicAdd(&wo[t.g].word[t.cur ^ 1u], t.add);
#else
    // (the word's index goes through an opaque VGPR: with an address it can prove uniform the compiler's atomic optimizer rewrites the operation
    //  as "first active lane adds, then broadcast" and waits for the result on the spot)
    uint32_t wi = t.cur ^ 1u;
    asm volatile("" : "+v"(wi));
    t.old = atomicAdd(&wo[t.g].word[wi & 1u], t.add);
#endif
  }
  return t;
}
__device__ __forceinline__ void wo_finish(WaveOrder* wo, const WoGeom& wg, const int B, const bool valid, const int b, const int cls, const int r,
                                          const int s, const WoPost& t) {
  const uint32_t ns = t.ns, g = t.g;
  if (ns > (uint32_t)WO_NS) return;
  WaveOrder& sl = wo[g];
  const uint32_t cur = t.cur, nxt = cur ^ 1u;
  const unsigned long long old =
      ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(t.old >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)t.old);
  const uint32_t at = (uint32_t)((old >> (9 * cls)) & 511ull) + (uint32_t)__popc(t.same & ((1u << r) - 1u));
  if (valid && s == 0 && at < WO_CAP) wo_list(wo, nxt, g, cls)[at] = (uint32_t)b;
#ifdef SIM3P_WO_DIVIDE
  const int G_ = (int)gridDim.x;
  const uint32_t nwaves = (uint32_t)((G_ - (int)g + (int)ns - 1) / (int)ns);
#else
  const uint32_t nwaves = wg.wq + (g < wg.wr ? 1u : 0u);                          // waves of slice g
#endif
  if (r == 0 && s == 0 && (uint32_t)(old >> 54) == nwaves - 1u) {
    const unsigned long long fin = old + t.add;
    uint32_t n = 0u;
#pragma unroll
    for (int c = 0; c < WO_NCLS; ++c) { sl.off[c] = n; n += (uint32_t)((fin >> (9 * c)) & 511ull); }
    const uint32_t G = gridDim.x, glast = (wg.wr ? wg.wr : ns) - 1u;             // (the batch's last wave may be short: it sits in slice (G - 1) % ns)
    const uint32_t expect = 4u * nwaves - ((g == glast) ? 4u * G - (uint32_t)B : 0u);
    sl.B = (n == expect) ? (uint32_t)B : 0u;
    sl.cur = nxt;
    sl.word[cur] = 0ull;
  }
}

// shared by the packed orth and box kernels: FK levels of their whole-tree schedule (DevPlan.q_fk) and the staged weights image wt [96]
constexpr int QLEV = 6;
static_assert(offsetof(WbcConfig, joint_w) - offsetof(WbcConfig, ee_W) == 84 * sizeof(double), "ee_W [30] ee_w [5] ee_gain [30] trunk [13] com_W [3] com_gain [3] joint_w");
// offsets inside wt: ee_W, ee_w, ee_gain, trunk_W, trunk_w, trunk_gain, com_W, com_gain, joint_w
constexpr int WT_W = 0, WT_w = 30, WT_G = 35, WT_TW = 65, WT_Tw = 71, WT_TG = 72, WT_CW = 78, WT_CG = 81, WT_JW = 84;
#define WT_AT(field, k) (offsetof(WbcTaskParams, field) == (k) * sizeof(double))
static_assert(WT_AT(ee_W, WT_W) && WT_AT(ee_w, WT_w) && WT_AT(ee_gain, WT_G) && WT_AT(trunk_W, WT_TW) && WT_AT(trunk_w, WT_Tw) && WT_AT(trunk_gain, WT_TG) &&
              WT_AT(com_W, WT_CW) && WT_AT(com_gain, WT_CG) && WT_AT(joint_w, WT_JW), "the weights image is WbcTaskParams, double for double");
#undef WT_AT

// ---- the packed kinematics (tick kernels: sim3p over DevPlan.pk_fk, orthp / boxp over DevPlan.q_fk; wbc_update_packed_kernel over pk_fk).
// oMi [joint][12]: R column-major then p; sc: sin / cos of joint j at 2 j; qv: the staged configuration.
// Seed: sin / cos of the joint angles, two joints per lane (joint j >= 2 reads q[idx_q[j]]: scq0 / scq1 = DevPlan.pk_scq / q_scq of joints 2 + s,
// 18 + s), and the root free-flyer (joint 1) on lane 0: R from the quaternion exactly as Eigen's toRotationMatrix, p = xyz. The caller fences.
__device__ __forceinline__ void pk_fk_seed(double* const oMi, double* const sc, const double* const qv, const int scq0, const int scq1, const int s) {
#ifdef PK_SEED_SERIAL      // (A/B variant builds only: each joint's sine and cosine inside its own branch, as before DESIGN.md §3.23)
  if (scq0 >= 0) { const SinCos t = sincos_cw(qv[scq0]); sc[2 * (2 + s)] = t.s; sc[2 * (2 + s) + 1] = t.c; }
  if (scq1 >= 0) { const SinCos t = sincos_cw(qv[scq1]); sc[2 * (18 + s)] = t.s; sc[2 * (18 + s) + 1] = t.c; }
#else
  // both joints' angles in one straight-line block, so that their four polynomial chains interleave; a lane without a joint computes on 0 and
  // stores nothing (the same operations on the same values for the joints that exist: bit for bit the same table)
  const double a0 = qv[scq0 >= 0 ? scq0 : 0], a1 = qv[scq1 >= 0 ? scq1 : 0];
  const SinCos t0 = sincos_cw(scq0 >= 0 ? a0 : 0.0), t1 = sincos_cw(scq1 >= 0 ? a1 : 0.0);
  if (scq0 >= 0) { sc[2 * (2 + s)] = t0.s; sc[2 * (2 + s) + 1] = t0.c; }
  if (scq1 >= 0) { sc[2 * (18 + s)] = t1.s; sc[2 * (18 + s) + 1] = t1.c; }
#endif
  if (s == 0) {
    double Rt[9];
    quat_to_R(qv + 3, Rt);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int rr = 0; rr < 3; ++rr) oMi[12 + 3 * c + rr] = Rt[3 * rr + c];
    oMi[12 + 9] = qv[0]; oMi[12 + 10] = qv[1]; oMi[12 + 11] = qv[2];
  }
}
// pin.forwardKinematics, level by level (Robot_Wrapper4.py:400): lane s places the joint of sched[L][s] (joint -1: none) on its parent's placement.
// fkn: the caller's register record holding sched[0][s], loaded well before (its latency is hidden behind the caller's own work); the next
// level's record is on its way while a level is computed (L1-resident tables: kept live for all levels the records cost 60 VGPRs).
// ROT: the batch holds a model with a rotated joint placement; the instantiations without it compile to exactly the code they had before the
// flag existed. Ends fenced: oMi is complete on return.
template <bool ROT, int NLEV>
__device__ __forceinline__ void pk_fk_sweep(double* const oMi, const double* const sc, const double* const qv, const DevModel& M,
                                            const DevPlan::PkJoint (&sched)[NLEV][16], DevPlan::PkJoint& fkn, const int s) {
#pragma unroll 1
  for (int L = 0; L < NLEV; ++L) {
    const DevPlan::PkJoint fk = fkn;
    if (L + 1 < NLEV) fkn = sched[L + 1][s];
    const int j = fk.joint;
    if (j >= 0) {
      const bool rev = fk.rev != 0;
      const int a0 = fk.a0, a1 = fk.a1, a2 = fk.a2;
      const double* Pp = oMi + 12 * fk.parent;
      const double sn = rev ? sc[2 * j] : 0.0, cs = rev ? sc[2 * j + 1] : 1.0;
      const double pris = rev ? 0.0 : qv[fk.q_idx];
      if (ROT && fk.rot) {
        fk_place_rot_lds(oMi + 12 * j, Pp, M.rp[j], a0, a1, a2, sn, cs, pris);
      } else {
        double Av[3], Bv[3], Cv[3], Pv[3];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) { Av[rr] = Pp[a0 + rr]; Bv[rr] = Pp[a1 + rr]; Cv[rr] = Pp[a2 + rr]; Pv[rr] = Pp[9 + rr]; }
        double* Po = oMi + 12 * j;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
          Po[a0 + rr] = Av[rr];
          Po[a1 + rr] = cs * Bv[rr] + sn * Cv[rr];
          Po[a2 + rr] = cs * Cv[rr] - sn * Bv[rr];
          Po[9 + rr] = Pv[rr] + Av[rr] * (fk.t0 + pris) + Bv[rr] * fk.t1 + Cv[rr] * fk.t2;
        }
      }
    }
    WSYNC();
  }
}
// WORLD Jacobian column of a DoF from oMi: the DoF's joint, and which column of its R is the linear / angular axis (-1: none). lin and ang come in
// zero; a column whose angular part the caller has no use for passes a scratch ang.
__device__ __forceinline__ void pk_jac_col(const double* const oMi, const int joint, const int lin_axis, const int ang_axis, double (&lin)[3],
                                           double (&ang)[3]) {
  const double* Pj = oMi + 12 * joint;
  const double pj[3] = {Pj[9], Pj[10], Pj[11]};
  if (ang_axis >= 0) { ang[0] = Pj[3 * ang_axis]; ang[1] = Pj[3 * ang_axis + 1]; ang[2] = Pj[3 * ang_axis + 2]; cross3(pj, ang, lin); }
  if (lin_axis >= 0) { lin[0] = Pj[3 * lin_axis]; lin[1] = Pj[3 * lin_axis + 1]; lin[2] = Pj[3 * lin_axis + 2]; }
}

// ---- input staging of the tick kernels
// Entry k of the trunk task's 18 inputs: trunk_target [3], prev_trunk_target [3], trunk_ref_euler [3], trunk_prev_rot [9]
__device__ __forceinline__ double pk_trunk_input(const WbcTickIn& in, const int b, const int k) {
  return (k < 3) ? in.trunk_target[(size_t)b * 3 + k] : (k < 6) ? in.prev_trunk_target[(size_t)b * 3 + (k - 3)]
       : (k < 9) ? in.trunk_ref_euler[(size_t)b * 3 + (k - 6)] : in.trunk_prev_rot[(size_t)b * 9 + (k - 9)];
}
// the same entry's address: one load per lane whatever the array (the packed sim3 kernel's single input level)
__device__ __forceinline__ const double* pk_trunk_input_at(const WbcTickIn& in, const int b, const int k) {
  const double* const base = (k < 3) ? in.trunk_target : (k < 6) ? in.prev_trunk_target : (k < 9) ? in.trunk_ref_euler : in.trunk_prev_rot;
  const size_t off = (k < 3) ? (size_t)b * 3 + k : (k < 6) ? (size_t)b * 3 + (k - 3) : (k < 9) ? (size_t)b * 3 + (k - 6) : (size_t)b * 9 + (k - 9);
  return base + off;
}
// calcTargetVelEE3's orientation feed-forward (Robot_Wrapper4.py:1125-1133): omega = vee(((R* - R*_prev) / dt) R*^T), one component per lane
// (EE s / 3, component s % 3), straight from the caller's [B][5][9] references; zero when none are passed
__device__ __forceinline__ double pk_ee_omega(const WbcTickIn& in, const int b, const int s, const double inv_dt) {
  double om = 0.0;
  if (in.ee_ref_rot && s < 15) {
    const int e = s / 3, i = s - 3 * e;
    const double* Rs = in.ee_ref_rot + (size_t)b * 45 + 9 * e;
    const double* Rp = in.ee_prev_rot + (size_t)b * 45 + 9 * e;
    const int ra = (i == 0) ? 6 : ((i == 1) ? 0 : 3), rb = (i == 0) ? 3 : ((i == 1) ? 6 : 0);   // S[2][1] = D row 2 . R row 1; S[0][2]; S[1][0]
    om = ((Rs[ra] - Rp[ra]) * inv_dt) * Rs[rb] + ((Rs[ra + 1] - Rp[ra + 1]) * inv_dt) * Rs[rb + 1] + ((Rs[ra + 2] - Rp[ra + 2]) * inv_dt) * Rs[rb + 2];
  }
  return om;
}
// The weights and gains image wt: the 85 contiguous doubles of the configuration's block (WT_* offsets), or with TP of the instance's row, six per
// lane; entries 85 .. ncfg - 1 (ncfg = 85, or 89: + trunk_box_z_frac, _ang, _scale, com_box_scale) stay the configuration's, the rest of wt [96]
// is zero. Returns whether the row is refused (tp_row_bad16's rule): the image is then the configuration's block and the instance reports
// WBC_QP_NUMERICAL. Without TP, tps is never read.
template <bool TP>
__device__ __forceinline__ bool pk_stage_weights(double* const wt, const WbcConfig& cfg, const WbcTaskParams* const tps, const int b, const int s,
                                                 const int rbase, const int ncfg) {
  const double* cw = &cfg.ee_W[0][0];
  bool tpbad = false;
  if (TP) {
    const double* rw = reinterpret_cast<const double*>(tps + b);
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int k = s + 16 * i;
      const double v = (k < WBC_TASK_PARAMS_DOUBLES) ? rw[k] : ((k < ncfg) ? cw[k] : 0.0);
      bad = bad || (k < WBC_TASK_PARAMS_DOUBLES && tp_entry_bad(k, v));
      wt[s + 16 * i] = v;
    }
    tpbad = ((__ballot(bad) >> rbase) & 0xFFFFull) != 0ull;
  }
  if (!TP || tpbad) {
#pragma unroll
    for (int i = 0; i < 6; ++i) wt[s + 16 * i] = (s + 16 * i < ncfg) ? cw[s + 16 * i] : 0.0;
  }
  return tpbad;
}
// calcTargetVelTrunk2 (Robot_Wrapper4.py:948-1015): the trunk task's target velocity vel [6] from the staged inputs alone — the trunk frame is
// the free-flyer's own placement (the plan checks it). tin: pk_trunk_input's 18 entries; tw: trunk_W [0..5], trunk_w [6], trunk_gain [7..12];
// sh [12]: LDS scratch of the instance (the six sines / cosines of the reference angles and their halves, one per lane); Rt: the trunk's
// rotation, row-major, for the caller that goes on with it. Fences once inside (sh); the staged inputs are visible on entry.
// Bug-compatible with the reference on purpose: qe2's first two terms cancel (:976), and the skew matrix is D R*, not D R*^T (:984).
__device__ __forceinline__ void pk_trunk_target_vel(const double* const qv, const double* const tin, const double* const tw, double* const sh,
                                                    const double inv_dt, const int s, double (&Rt_)[9], double (&vel)[6]) {
  const double* xt = tin;
  const double* xp = tin + 3;
  const double* er = tin + 6;
  double fq[4], rq[4], Rs[9];
  quat_to_R(qv + 3, Rt_);
  R_to_quat(Rt_, fq);
  {
    const SinCos t = sincos_cw(s < 3 ? er[s < 3 ? s : 0] : 0.5 * er[(s < 6 ? s : 3) - 3]);   // reference angles and their halves, one per lane
    if (s < 6) { sh[2 * s] = t.s; sh[2 * s + 1] = t.c; }
    WSYNC();
    const double sa = sh[0], ca = sh[1], sb = sh[2], cb = sh[3], sc_ = sh[4], cc = sh[5];
    euler_to_R(sa, ca, sb, cb, sc_, cc, Rs);
    const double qx[4] = {sh[6], 0, 0, sh[7]}, qy[4] = {0, sh[8], 0, sh[9]}, qz[4] = {0, 0, sh[10], sh[11]};
    double tq[4];
    quat_mul(qy, qx, tq);
    quat_mul(qz, tq, rq);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) vel[i] = (xt[i] - xp[i]) * inv_dt + tw[7 + i] * ((xt[i] - qv[i]) * inv_dt);
  const double qe0 = fq[3] * rq[0] - fq[0] * rq[3] + fq[1] * rq[2] - fq[2] * rq[1];   // :974
  const double qe1 = fq[3] * rq[1] - fq[1] * rq[3] - fq[0] * rq[2] + fq[2] * rq[0];   // :975
  const double qe2 = fq[3] * rq[2] - fq[3] * rq[2] + fq[0] * rq[1] - fq[1] * rq[0];   // :976 (sic)
  double D[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) D[i] = (Rs[i] - tin[9 + i]) * inv_dt;
  // skew = D Rs (R*, not R*^T: :984); omega = (S[2][1], S[0][2], S[1][0]) + K qe
  vel[3] = (D[6] * Rs[1] + D[7] * Rs[4] + D[8] * Rs[7]) + tw[10] * qe0;
  vel[4] = (D[0] * Rs[2] + D[1] * Rs[5] + D[2] * Rs[8]) + tw[11] * qe1;
  vel[5] = (D[3] * Rs[0] + D[4] * Rs[3] + D[5] * Rs[6]) + tw[12] * qe2;
}

}  // namespace wbc
