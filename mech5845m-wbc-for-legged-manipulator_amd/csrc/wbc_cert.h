// wbc_cert.h — what the kernel of wbc_qp_certificate (wbc_k_cert.hip) consumes, and its launcher (internal, C++). A header of its own, as
// wbc_traj.h and wbc_slack.h: no other kernel's translation unit sees it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "wbc_device.h"

namespace wbc {

enum { CERT_OK = 0, CERT_UNSOLVED = 1, CERT_DEPENDENT = 2, CERT_NUMERICAL = 3 };   // WBC_CERT_* of include/wbc.h

// One launch certifies x of every problem: m > 0 is the least-squares form (A, bvec), m == 0 the (H, g) form. Every pointer below `x` may
// be null; a null output is not written.
struct CertArgs {
  int32_t B, n, p, m;
  const double *H, *g, *A, *bvec, *C, *lb, *ub, *Clb, *Cub;
  const double* x;                      // [B][n]
  const double* v;                      // [B][n] dL/dx for the sensitivities, or null
  const int32_t* status;                // [B] the solve's status, or null: every instance counts as solved
  const unsigned long long* ws;         // [B][2] working set of the solve, or null: the active set is read off x
  double *y_bounds, *y_rows;            // [B][n], [B][p]
  double *kkt, *objective;              // [B][4], [B]
  double *sens_x, *sens_bounds, *sens_rows;
  int32_t *n_active, *cert_status;      // [B]
};

int launch_cert(const CertArgs& a, int grid, void* stream);   // one problem per wavefront, grid-stride
int cert_lds_bytes();

}  // namespace wbc
