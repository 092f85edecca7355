// wbc_k_cert.hip — wbc_qp_certificate: dual solution, KKT certificate and sensitivities of a solved QP, in a kernel of its own behind the
// solve (include/wbc.h). No solve kernel is touched and this kernel has no variant table.
//   min 1/2 x'Hx + g'x  s.t. lb <= x <= ub, Clb <= C x <= Cub      (or H = A'A, g = -A'b from the unfactored A, b)
// One problem per wavefront, grid-stride, everything in LDS, fp64; lane = variable (or constraint row, or column of Y, as noted at each loop).
//   1. data -> LDS by flat coalesced copies (H = A'A on the vector unit when A is given; A x - b and A'(A x - b) from the same staged image: A
//      is read once), C x, the active list N by ballot: variables by index, then rows by index
//   2. grad f (from A, b: A'(A x - b) as two products, never through fl(A'A)), objective, primal violation
//   3. Cholesky H = L L' in place
//   4. Y = L^-1 N' (n x k), with L^-1 grad f and L^-1 v as two more columns behind it: lane = column
//   5. Householder QR of Y, Y = Q1 R: the reflectors stay below R's diagonal, the two extra columns become Q'z
//   6. y = R^-1 Q1' L^-1 grad f,  w = R^-1 Q1' L^-1 v  (one back substitution, lane = row),  u = L^-T Q2 Q2' L^-1 v
// The Schur complement Y'Y is never formed: it squares cond(Y) (the table). Reads its inputs, writes rows [0, B) of the
// outputs that are not null; an instance's non-finite data ends in its own cert_status and zeros.
#include <stddef.h>
#include "wbc_packed.h"
#include "wbc_cert.h"

namespace wbc {

constexpr int CERT_COLS = NV + 2;             // columns of Y (k <= n <= 26) + L^-1 grad f + L^-1 v
constexpr int CERT_MT = 50, CERT_CH = 48;     // staging of A by DoF while H = A'A is formed: row stride, rows per chunk (wbc_qp_kernel's)
constexpr double CERT_DEP_TOL = 1e-12;        // DEPENDENT: |R_jj| <= CERT_DEP_TOL x |column j of Y| (include/wbc.h)

struct __attribute__((aligned(16))) CertSmem {
  double Hm[NV * LDJ];                        // H, then L in its lower triangle
  double Yt[CERT_COLS * LDJ];                 // column c of [Y, L^-1 grad f, L^-1 v] at Yt[c * LDJ + row]; before that (with Cm): A by DoF
  double Cm[PMAX * LDJ];                      // constraint rows (p x n)
  double e[WBC_MAX_M];                        // A x - b
  double xv[32], ys[32], ws[32], yr[32];      // x; y and w by position in the active list; y of the rows by row
};
static_assert(sizeof(CertSmem) <= sizeof(Smem), "the certificate kernel's LDS footprint is no larger than the solve's");
static_assert(offsetof(CertSmem, Cm) == offsetof(CertSmem, Yt) + sizeof(double) * CERT_COLS * LDJ, "Yt and Cm are one staging area");
static_assert((CERT_COLS + PMAX) * LDJ >= NV * CERT_MT, "A by DoF fits Yt + Cm");

__device__ __forceinline__ bool cert_bounded(double x) { return fabs(x) < QP_INF; }                    // a bound the problem really has
// sum / max over all 64 lanes, wave-uniform result: butterfly inside each 16-lane row, the four rows joined by readlane
__device__ __forceinline__ double cert_sum(double v) {
  v += dpp<DPP_XOR1>(v); v += dpp<DPP_XOR2>(v); v += dpp<DPP_HALF_MIRROR>(v); v += dpp<DPP_MIRROR>(v);
  return (rdl(v, 0) + rdl(v, 16)) + (rdl(v, 32) + rdl(v, 48));
}
__device__ __forceinline__ double cert_max(double v) {
  v = fmax(v, dpp<DPP_XOR1>(v)); v = fmax(v, dpp<DPP_XOR2>(v)); v = fmax(v, dpp<DPP_HALF_MIRROR>(v)); v = fmax(v, dpp<DPP_MIRROR>(v));
  return fmax(fmax(rdl(v, 0), rdl(v, 16)), fmax(rdl(v, 32), rdl(v, 48)));
}
// side of one constraint: 0 inactive, 1 at its lower side, 2 at its upper side, 3 equality (always active). `bits`: the working set's
// (lower | upper << 1) when there is one — a bit on an infinite side, or both at once, is ignored; else the rule of tests/common.py exact_optimum
__device__ __forceinline__ int cert_side(const double v, const double lo, const double hi, const bool have_ws, const int bits) {
  const bool flo = cert_bounded(lo), fhi = cert_bounded(hi);
  if (lo == hi && flo) return 3;
  if (have_ws) return (bits == 1 && flo) ? 1 : ((bits == 2 && fhi) ? 2 : 0);
  if (flo && fabs(v - lo) < 1e-7 * fmax(1.0, fabs(lo))) return 1;
  if (fhi && fabs(v - hi) < 1e-7 * fmax(1.0, fabs(hi))) return 2;
  return 0;
}

__global__ void __launch_bounds__(64, 2) wbc_qp_cert_kernel(const CertArgs A) {
  __shared__ CertSmem S;
#pragma unroll 1
  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
    int lane = threadIdx.x, n = A.n, p = A.p, m = A.m;
    asm volatile("" : "+v"(lane), "+s"(n), "+s"(p), "+s"(m));   // no LICM of lane/n-derived masks
    const size_t bn = (size_t)b * n, bp = (size_t)b * p;
    const bool isv = lane < n, isr = lane < p;
    // what the instance writes at the end: zeros unless a stage below fills them
    double o_yb = 0.0, o_yr = 0.0, o_u = 0.0, o_wb = 0.0, o_wr = 0.0, k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0, obj = 0.0;
    int nact = 0, cst = CERT_OK;
    WSYNC();                                                      // the previous instance's LDS reads are done
    do {
      if (A.status && A.status[b] != 0) { cst = CERT_UNSOLVED; break; }
      // ---- 1. data. Every value is checked while it is staged: a non-finite one ends the instance at the end of this stage, and what the (A, b)
      // form has formed from the staged image by then (A x - b, grad f, the objective) is dropped
      const double xk = isv ? A.x[bn + lane] : 0.0;
      const double vk = (A.v && isv) ? A.v[bn + lane] : 0.0;
      double lo = -1e30, hi = 1e30, clo = 0.0, chi = 0.0;
      if (A.lb && isv) { lo = A.lb[bn + lane]; hi = A.ub[bn + lane]; }
      if (isr) { clo = A.Clb[bp + lane]; chi = A.Cub[bp + lane]; }
      bool bad = !is_finite(xk) || !is_finite(vk) || lo != lo || hi != hi || clo != clo || chi != chi;   // (an infinite bound is no bound)
      double gk = 0.0, grad = 0.0;
      if (lane < 32) S.xv[lane] = isv ? xk : 0.0;
      if (m > 0) {
        // H = A'A on the vector unit: A staged by DoF (At[dof][row]) in chunks of <= 48 rows by a flat, coalesced copy, H accumulates in Hm
        // (wbc_qp_kernel's vector path). The same image gives A x - b (lane = row) and A'(A x - b) (lane = DoF): A is read from HBM once.
        const double* Ab = A.A + (size_t)b * m * n;
        const double* bb = A.bvec + (size_t)b * m;
        double* const At = S.Yt;
        double part = 0.0;                                          // 1/2 |A x|^2 - b'(A x), rows on lanes
        if (isv) for (int k = 0; k < n; ++k) S.Hm[lane * LDJ + k] = 0.0;
#pragma unroll 1
        for (int r0 = 0; r0 < m; r0 += CERT_CH) {
          const int mc = (m - r0 < CERT_CH) ? m - r0 : CERT_CH, mc2 = (mc + 1) & ~1;
          const double* Ac = Ab + (size_t)r0 * n;
          for (int idx = lane; idx < mc * n; idx += 64) {
            const int r = idx / n, c = idx - r * n;
            const double a = Ac[idx];
            bad |= !is_finite(a);
            At[c * CERT_MT + r] = a;
          }
          if (isv && mc2 > mc) At[lane * CERT_MT + mc] = 0.0;       // (the products below go two rows at a time)
          const double br = (lane < mc) ? bb[r0 + lane] : 0.0;
          bad |= !is_finite(br);
          WSYNC();
          if (lane < mc) {
            double ax = 0.0;
            for (int k = 0; k < n; ++k) ax = fma(At[k * CERT_MT + lane], S.xv[k], ax);
            S.e[r0 + lane] = ax - br;
            part += fma(0.5 * ax, ax, -br * ax);
          }
          if (lane == mc && mc2 > mc) S.e[r0 + mc] = 0.0;           // (mc odd and < 48: r0 + mc < WBC_MAX_M)
          WSYNC();
          if (isv) {
#pragma unroll 1
            for (int i = 0; i < n; ++i) {
              double s = S.Hm[lane * LDJ + i];
#pragma unroll 2
              for (int r = 0; r < mc2; r += 2) {
                const double2a x2 = lds2(At + i * CERT_MT + r); const double2a y2 = lds2(At + lane * CERT_MT + r);
                s = fma(x2.x, y2.x, fma(x2.y, y2.y, s));
              }
              S.Hm[lane * LDJ + i] = s;
            }
            for (int r = 0; r < mc2; r += 2) {
              const double2a a2 = lds2(At + lane * CERT_MT + r); const double2a e2 = lds2(S.e + r0 + r);
              grad = fma(a2.x, e2.x, fma(a2.y, e2.y, grad));
            }
          }
          WSYNC();
        }
        obj = cert_sum(part);
      } else {
        const double* Hb = A.H + bn * n;
        for (int idx = lane; idx < n * n; idx += 64) {
          const int r = idx / n, c = idx - r * n;
          const double h = Hb[idx];
          bad |= !is_finite(h);
          S.Hm[r * LDJ + c] = h;
        }
        gk = isv ? A.g[bn + lane] : 0.0;
        bad |= !is_finite(gk);
      }
      {
        const double* Cb = A.C + bp * n;
        for (int idx = lane; idx < p * n; idx += 64) {
          const int r = idx / n, c = idx - r * n;
          const double cv = Cb[idx];
          bad |= !is_finite(cv);
          S.Cm[r * LDJ + c] = cv;
        }
      }
      WSYNC();
      if (__ballot(bad) != 0ull) { cst = CERT_NUMERICAL; obj = 0.0; break; }   // (obj: the (A, b) form has summed it from the staged image already)
      // ---- C x (lane = row), the active list: variables by index, then rows by index
      double cx = 0.0;
      if (isr) for (int k = 0; k < n; ++k) cx = fma(S.Cm[lane * LDJ + k], S.xv[k], cx);
      int bits_b = 0, bits_r = 0;
      if (A.ws) {
        const unsigned long long w0 = A.ws[2 * (size_t)b], w1 = A.ws[2 * (size_t)b + 1];
        bits_b = (lane < 32) ? (int)(((w0 >> lane) & 1ull) | (((w0 >> (32 + lane)) & 1ull) << 1)) : 0;
        bits_r = (lane < 32) ? (int)(((w1 >> lane) & 1ull) | (((w1 >> (32 + lane)) & 1ull) << 1)) : 0;
      }
      const int ab = isv ? cert_side(xk, lo, hi, A.ws != nullptr, bits_b) : 0;
      const int ar = isr ? cert_side(cx, clo, chi, A.ws != nullptr, bits_r) : 0;
      const unsigned long long mb = __ballot(ab != 0), mr = __ballot(ar != 0), below = (1ull << lane) - 1ull;
      const int kb = __popcll(mb), k = kb + __popcll(mr);
      const int posb = __popcll(mb & below), posr = kb + __popcll(mr & below);   // place in the list (valid where the constraint is active)
      // ---- 2. primal violation; grad f and the objective from the caller's own data
      {
        double vb = 0.0;
        if (isv) vb = fmax(cert_bounded(lo) ? lo - xk : 0.0, cert_bounded(hi) ? xk - hi : 0.0);
        if (isr) vb = fmax(vb, fmax(cert_bounded(clo) ? clo - cx : 0.0, cert_bounded(chi) ? cx - chi : 0.0));
        k1 = cert_max(fmax(vb, 0.0));
      }
      if (m == 0) {
        double hx = 0.0;
        if (isv) for (int k = 0; k < n; ++k) hx = fma(S.Hm[lane * LDJ + k], S.xv[k], hx);
        grad = isv ? hx + gk : 0.0;
        obj = cert_sum(isv ? xk * fma(0.5, hx, gk) : 0.0);
      }
      nact = k;
      if (k > n) { cst = CERT_DEPENDENT; break; }                   // more normals than variables (and more than Yt holds)
      WSYNC();
      // ---- 3. Cholesky H = L L' in place, lane = row: column j from the columns before it
      bool chol_bad = false;
#pragma unroll 1
      for (int j = 0; j < n; ++j) {
        double s = 0.0;
        if (isv && lane >= j) {
          s = S.Hm[lane * LDJ + j];
          for (int t = 0; t < j; ++t) s = fma(-S.Hm[lane * LDJ + t], S.Hm[j * LDJ + t], s);
        }
        const double d = rdl(s, j);
        if (!(d > 0.0) || !is_finite(d)) { chol_bad = true; break; }
        const double sq = sqrt(d);
        if (isv && lane >= j) S.Hm[lane * LDJ + j] = (lane == j) ? sq : s / sq;
        WSYNC();
      }
      if (chol_bad) { cst = CERT_NUMERICAL; nact = 0; k1 = 0.0; obj = 0.0; break; }
      // ---- 4. the columns of N' (unit vectors, rows of C), then grad f and v; lane = column: L y = column, forward substitution in place
      if (ab != 0) for (int t = 0; t < n; ++t) S.Yt[posb * LDJ + t] = (t == lane) ? 1.0 : 0.0;
      if (ar != 0) for (int t = 0; t < n; ++t) S.Yt[posr * LDJ + t] = S.Cm[lane * LDJ + t];
      if (isv) { S.Yt[k * LDJ + lane] = grad; S.Yt[(k + 1) * LDJ + lane] = vk; }
      WSYNC();
      const int ncol = k + 2;
      double cn2 = 0.0;
      if (lane < ncol) {
        double* const yc = S.Yt + lane * LDJ;
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
          double s = yc[i];
          for (int t = 0; t < i; ++t) s = fma(-S.Hm[i * LDJ + t], yc[t], s);
          s /= S.Hm[i * LDJ + i];
          yc[i] = s;
          cn2 = fma(s, s, cn2);
        }
      }
      const double cn = sqrt(cn2);                                  // |column| of Y, lane = column
      WSYNC();
      // ---- 5. Householder QR of Y. Step j: the reflector of column j (lane = row for its norm), applied to the columns behind it (lane = column).
      // R's diagonal stays in registers (lane j: R_jj), the reflector's entries below row j stay in column j, its entry j and 2 / v'v go to ys / ws
      bool dep = false;
      double rdiag = 1.0;
#pragma unroll 1
      for (int j = 0; j < k; ++j) {
        const double a = (isv && lane >= j) ? S.Yt[j * LDJ + lane] : 0.0;
        const double nrm2 = cert_sum(a * a), ajj = rdl(a, j), nrm = sqrt(nrm2);
        if (!(nrm > CERT_DEP_TOL * rdl(cn, j))) { dep = true; break; }
        const double alpha = ajj > 0.0 ? -nrm : nrm;                // R_jj
        const double vj = ajj - alpha, beta = 1.0 / fma(-alpha, ajj, nrm2);   // 2 / v'v, v'v = 2 (|a|^2 - alpha a_j) > 0
        rdiag = (lane == j) ? alpha : rdiag;
        if (lane == 0) { S.ys[j] = vj; S.ws[j] = beta; }
        if (lane > j && lane < ncol) {
          double* const yc = S.Yt + lane * LDJ;
          const double* const vc = S.Yt + j * LDJ;
          double s = vj * yc[j];
          for (int i = j + 1; i < n; ++i) s = fma(vc[i], yc[i], s);
          s *= beta;
          yc[j] = fma(-s, vj, yc[j]);
          for (int i = j + 1; i < n; ++i) yc[i] = fma(-s, vc[i], yc[i]);
        }
        WSYNC();
      }
      if (dep) { cst = CERT_DEPENDENT; break; }
      // ---- 6. R y = Q1'(L^-1 grad f) and R w = Q1'(L^-1 v): one back substitution, lane = row, column c of R at Yt[c][row < c]
      double qa = (lane < k) ? S.Yt[k * LDJ + lane] : 0.0, qb = (lane < k) ? S.Yt[(k + 1) * LDJ + lane] : 0.0;
#pragma unroll 1
      for (int c = k - 1; c >= 0; --c) {
        const double rc = rdl(rdiag, c);
        const double ya = rdl(qa, c) / rc, yb = rdl(qb, c) / rc;
        const double ric = (lane < c) ? S.Yt[c * LDJ + lane] : 0.0;
        qa = (lane == c) ? ya : fma(-ric, ya, qa);
        qb = (lane == c) ? yb : fma(-ric, yb, qb);
      }
      // u = L^-T Q [0; Q2'z]: the reflectors in reverse order (lane = row), then L'u = t column by column
      double t = 0.0;
      if (A.v) {
        t = (isv && lane >= k) ? S.Yt[(k + 1) * LDJ + lane] : 0.0;
#pragma unroll 1
        for (int j = k - 1; j >= 0; --j) {
          const double vj = S.ys[j], beta = S.ws[j];
          const double vi = (lane == j) ? vj : ((isv && lane > j) ? S.Yt[j * LDJ + lane] : 0.0);
          const double s = cert_sum(vi * t) * beta;
          t = fma(-s, vi, t);
        }
#pragma unroll 1
        for (int c = n - 1; c >= 0; --c) {
          const double uc = rdl(t, c) / S.Hm[c * LDJ + c];
          const double lci = (lane < c) ? S.Hm[c * LDJ + lane] : 0.0;
          t = (lane == c) ? uc : fma(-lci, uc, t);
        }
        o_u = isv ? t : 0.0;
      }
      WSYNC();                                                      // ys / ws: the reflectors are done with them
      if (lane < 32) { S.ys[lane] = (lane < k) ? qa : 0.0; S.ws[lane] = (lane < k) ? qb : 0.0; }
      WSYNC();
      o_yb = (ab != 0) ? S.ys[posb] : 0.0;
      o_yr = (ar != 0) ? S.ys[posr] : 0.0;
      if (A.v) { o_wb = (ab != 0) ? S.ws[posb] : 0.0; o_wr = (ar != 0) ? S.ws[posr] : 0.0; }
      if (lane < 32) S.yr[lane] = o_yr;
      WSYNC();
      // ---- the certificate: stationarity, multiplier signs, complementarity
      double nty = o_yb;
      if (isv) for (int r = 0; r < p; ++r) nty = fma(S.Cm[r * LDJ + lane], S.yr[r], nty);
      k0 = cert_max(isv ? fabs(grad - nty) : 0.0);
      const double sgb = (ab == 1) ? fmax(-o_yb, 0.0) : ((ab == 2) ? fmax(o_yb, 0.0) : 0.0);
      const double sgr = (ar == 1) ? fmax(-o_yr, 0.0) : ((ar == 2) ? fmax(o_yr, 0.0) : 0.0);
      k2 = cert_max(fmax(sgb, sgr));
      const double cpb = (ab != 0) ? fabs(o_yb * (xk - ((ab == 2) ? hi : lo))) : 0.0;
      const double cpr = (ar != 0) ? fabs(o_yr * (cx - ((ar == 2) ? chi : clo))) : 0.0;
      k3 = cert_max(fmax(cpb, cpr));
    } while (0);
    // ---- outputs (vector stores; rows [0, B) only)
    if (isv) {
      if (A.y_bounds) A.y_bounds[bn + lane] = o_yb;
      if (A.sens_x) A.sens_x[bn + lane] = o_u;
      if (A.sens_bounds) A.sens_bounds[bn + lane] = o_wb;
    }
    if (isr) {
      if (A.y_rows) A.y_rows[bp + lane] = o_yr;
      if (A.sens_rows) A.sens_rows[bp + lane] = o_wr;
    }
    if (A.kkt && lane < 4) A.kkt[4 * (size_t)b + lane] = (lane == 0) ? k0 : ((lane == 1) ? k1 : ((lane == 2) ? k2 : k3));
    if (lane == 0) {
      if (A.objective) A.objective[b] = obj;
      if (A.n_active) A.n_active[b] = nact;
      if (A.cert_status) A.cert_status[b] = cst;
    }
  }
}

int cert_lds_bytes() { return (int)sizeof(CertSmem); }

int launch_cert(const CertArgs& a, int grid, void* stream) {
  hipLaunchKernelGGL(wbc_qp_cert_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace wbc
